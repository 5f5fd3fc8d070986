"""Shared by tests/test_reference_volume.py and tests/test_reference_volume_gpu.py: the numpy float64 restatement of
svr_resample_to_reconstruction (csrc/svr_seed.inc, include/svr_hip.h) -- vectorised over the target voxels, a loop over the eight
neighbours only -- and the moving tiny phantom of the command-line tests."""
import math

import numpy as np

from fetalreconstruction_amd import geometry as geo


def compose(src_attr, recon_attr):
    """M = source world-to-image x reconstruction image-to-world, in double, with the helpers that build these matrices everywhere else
    (plain sums from 0, as csrc/svr_prep.h's mul)"""
    return geo.mat_mul(geo.world_to_image(src_attr), geo.image_to_world(recon_attr))


def coordinates(m, shape):
    """source position (px, py, pz) of every target voxel, [vz][vy][vx] each, evaluated left to right in double"""
    m = np.asarray(m, np.float64).reshape(-1, 4)
    vz, vy, vx = shape
    k, j, i = np.meshgrid(np.arange(vz, dtype=np.float64), np.arange(vy, dtype=np.float64), np.arange(vx, dtype=np.float64), indexing="ij")
    return tuple(m[r, 0] * i + m[r, 1] * j + m[r, 2] * k + m[r, 3] for r in range(3))


def weights(src, m, shape, padding=-1.0):
    """-> (W, A): the sum of the weights that take part and of weight x value, float64 [vz][vy][vx], added in the kernel's order
    (z outermost, x fastest; a neighbour that does not take part adds 0.0, which changes nothing)"""
    s = np.asarray(src, np.float32).astype(np.float64)
    nz, ny, nx = s.shape
    pad = float(np.float32(padding))
    px, py, pz = coordinates(m, shape)
    fx, fy, fz = np.floor(px), np.floor(py), np.floor(pz)
    tx, ty, tz = px - fx, py - fy, pz - fz
    ix, iy, iz = (np.clip(f, -2, n + 1).astype(np.int64) for f, n in ((fx, nx), (fy, ny), (fz, nz)))
    W, A = np.zeros(shape), np.zeros(shape)
    for dz in (0, 1):
        zi, wz = iz + dz, (tz if dz else 1.0 - tz)
        for dy in (0, 1):
            yi, wy = iy + dy, (ty if dy else 1.0 - ty)
            for dx in (0, 1):
                xi = ix + dx
                w = ((tx if dx else 1.0 - tx) * wy) * wz
                inside = (xi >= 0) & (xi < nx) & (yi >= 0) & (yi < ny) & (zi >= 0) & (zi < nz)
                v = s[np.clip(zi, 0, nz - 1), np.clip(yi, 0, ny - 1), np.clip(xi, 0, nx - 1)]
                take = inside & (v > pad)
                W = W + np.where(take, w, 0.0)
                A = A + np.where(take, w * v, 0.0)
    return W, A


def stats_of(values):
    """{n, sum v, sum v^2, min, max} of float32 values held in double, the sums exactly rounded (math.fsum)"""
    v = np.asarray(values, np.float32).astype(np.float64).ravel()
    if v.size == 0:
        return np.array([0.0, 0.0, 0.0, np.inf, -np.inf])
    return np.array([float(v.size), math.fsum(v), math.fsum(v * v), v.min(), v.max()])


def resample(src, m, shape, padding=-1.0, mask=None, scale=None):
    """-> (volume float32 [vz][vy][vx], valid bool, stats float64 [5] of the valid voxels before scaling)"""
    W, A = weights(src, m, shape, padding)
    inside = np.ones(shape, bool) if mask is None else (np.asarray(mask).reshape(shape) != 0)
    valid = inside & (W >= 0.5)
    with np.errstate(invalid="ignore", divide="ignore"):
        val = (A / W).astype(np.float32)                   # accumulated in double, rounded once
    out = np.where(valid, val, np.float32(padding)).astype(np.float32)
    out[~inside] = -1.0
    stats = stats_of(out[valid])
    if scale is not None:
        out[valid] = out[valid] * np.float32(scale)        # float32 x float32, as the second pass
    assert out.dtype == np.float32
    return out, valid, stats


# ---- inputs shared by the CPU and the GPU tests ----------------------------------------------------------------------------------------

def ints(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape).astype(np.float32)


def ball(n=16, lo=100, hi=200, seed=5):
    """integers lo..hi inside a ball, -1 (a previous output's background) outside"""
    c = (np.arange(n) - (n - 1) / 2.0) ** 2
    r2 = c[:, None, None] + c[None, :, None] + c[None, None, :]
    v = np.random.default_rng(seed).integers(lo, hi + 1, (n, n, n)).astype(np.float32)
    v[r2 >= (0.35 * n) ** 2] = -1.0
    return v


def oblique_pair(scale=0.8):
    """the bundled mask's oblique grid as the source's axes and a world-aligned grid of `scale` x its voxel size as the target's"""
    from tests import real_mask
    _, a, _ = real_mask.load()
    src = geo.ImageAttributes(30, 34, 26, a.dx, a.dy, a.dz, a.xaxis.copy(), a.yaxis.copy(), a.zaxis.copy(), origin=np.asarray(a.origin, np.float64).copy())
    rec = geo.ImageAttributes(40, 36, 28, scale * a.dx, scale * a.dy, scale * a.dz, origin=np.asarray(a.origin, np.float64) + np.array([0.37, -0.21, 0.13]))
    return src, rec


# ---- the command line's phantom: the tiny phantom's three stacks (32 x 32 x 8, phantom.make_stacks) with every slice moved on its own ----

def moving_stacks(motion_mm, motion_deg, seed=1, noise_sigma=5.0):
    """-> (stacks, recon_attr, recon_mask): phantom.make_stacks' geometry and intensities; slice j of a stack is the phantom seen
    through its own small rigid transformation, so only slice-to-volume registration can put it back"""
    from fetalreconstruction_amd import phantom
    stacks, _, _, rattr, rmask = phantom.make_stacks(3, (32, 32, 8), 1.1, 2.2, None, 1.0, 14.0, seed=seed, orientations=("ax", "cor", "sag"),
                                                     stack_motion_mm=0.0, stack_motion_deg=0.0)
    rng = np.random.default_rng(seed + 100)
    for st in stacks:
        a = st.attr
        jj, ii = np.meshgrid(np.arange(a.ny), np.arange(a.nx), indexing="ij")
        for j in range(a.nz):
            p = np.concatenate([rng.uniform(-motion_mm, motion_mm, 3), rng.uniform(-motion_deg, motion_deg, 3)])
            pix = np.stack([ii, jj, np.full_like(ii, j), np.ones_like(ii)], -1).astype(np.float64)
            w = (pix @ geo.image_to_world(a).T) @ geo.rigid_matrix(*p).T
            val = phantom.phantom_intensity(w[..., :3], 14.0) * 700.0 / 0.55 + rng.normal(0.0, noise_sigma, w.shape[:-1])
            st.data[j] = np.maximum(val, 0.0).astype(np.float32)
    return stacks, rattr, rmask


def write_cli_case(d, motion_mm, motion_deg):
    """the stacks and the mask as files -> the common arguments of the command line (registration on)"""
    from fetalreconstruction_amd import nifti
    stacks, rattr, rmask = moving_stacks(motion_mm, motion_deg)
    paths = []
    for k, st in enumerate(stacks):
        nifti.write(d / f"stack{k}.nii.gz", st.data, st.attr)
        paths.append(str(d / f"stack{k}.nii.gz"))
    nifti.write(d / "mask.nii.gz", rmask, rattr)
    return ["-i", *paths, "-m", str(d / "mask.nii.gz"), "--thickness", "2.2", "2.2", "2.2", "--resolution", "1.0", "--rec_iterations_first", "2",
            "--rec_iterations_last", "4", "--smooth_mask", "0"], rattr, rmask


def ncc(a, b, sel):
    x, y = np.asarray(a, np.float64)[sel], np.asarray(b, np.float64)[sel]
    x, y = x - x.mean(), y - y.mean()
    return float((x * y).sum() / math.sqrt((x * x).sum() * (y * y).sum()))
