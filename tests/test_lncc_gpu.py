"""The engine's windowed cross correlation (csrc/svr_lncc.inc) against the numpy restatement (tests/lncc_ref.py): {N, S} and the per-pixel
k maps bit for bit on planes smaller than the window, at odd sizes and at the widths and heights where the kernel retiles; the same
optimiser trajectory from the engine and from the restatement, slices and packages; the command line end to end."""
import subprocess

import numpy as np
import pytest

from fetalreconstruction_amd import build, host
from tests import lncc_ref
from tests.test_lncc_registration import _lncc_backend, ramp
from tests.test_nmi_gpu import _plane_matrices
from tests.test_nmi_registration import _analytic_slice_case, _package_case, _slice_case, cli_case  # noqa: F401  (cli_case: a fixture)


def _padded(planes, tx, ty):
    out = np.full((len(planes), ty, tx), -1, np.int16)
    for k, p in enumerate(planes):
        out[k, :p.shape[0], :p.shape[1]] = p
    return out


def _check(rec, targets, idx, mats, src, R, what):
    """one call against the restatement, then the same call again: the same bits"""
    sums, kmap = rec.lncc_evaluate(idx, mats, R, maps=True)
    for e, (i, M) in enumerate(zip(idx, mats)):
        N, S, k = lncc_ref.lncc_plane(targets[i], M, src, R)
        assert (int(sums[e, 0]), int(sums[e, 1])) == (N, S), (what, R, e, sums[e], N, S)
        assert np.array_equal(kmap[e], k), (what, R, e, np.argwhere(kmap[e] != k)[:5])
    sums2, kmap2 = rec.lncc_evaluate(idx, mats, R, maps=True)
    assert np.array_equal(sums, sums2) and np.array_equal(kmap, kmap2)
    sums3, none = rec.lncc_evaluate(idx, mats, R)                       # without the maps
    assert none is None and np.array_equal(sums, sums3)
    return sums


@pytest.mark.gpu
@pytest.mark.parametrize("R", [1, 3, 7])
def test_device_lncc_is_the_restatement_bit_for_bit(R):
    from fetalreconstruction_amd import engine as E
    rec = E.Reconstruction(0)
    rng = np.random.default_rng(10 + R)
    ssize = (30, 34, 28)                                                # (x, y, z)
    src = rng.integers(-1, 2500, ssize[::-1]).astype(np.int16)
    src = np.maximum(src, (np.indices(src.shape).sum(0) * 40 % 3000).astype(np.int16) // 2)   # structure, and -1 only where both say so
    src[:, :, :2] = -1
    shapes = [(7, 5), (16, 16), (33, 17), (29, 37)]                     # (rows, columns): 5 x 7 is smaller than the window at R = 3 and 7
    planes = []
    for ty, tx in shapes:
        p = rng.integers(0, 1800, (ty, tx)).astype(np.int16)
        p[rng.random((ty, tx)) < 0.08] = -1                             # padding scattered inside the plane
        planes.append(p)
    planes.append(np.full((33, 37), 77, np.int16))                      # a flat target
    tx, ty = 37, 33
    targets = _padded(planes, tx, ty)
    rec.ncc_set_targets(targets)
    rec.ncc_set_source(src)
    # oblique matrices, several planes per call with repeated target indices, parts of planes outside the source, one fully outside
    idx = np.array([0, 1, 2, 3, 3, 1, 0, 2, 4, 3], np.int32)
    mats = np.concatenate([_plane_matrices(rng, (*planes[i].shape[::-1], 1), ssize, 1) for i in idx])   # centred on the plane itself
    mats[4, :3, 3] += (9.0, -7.0, 4.0)                                  # partly outside
    mats[9, :3, 3] += 500.0                                             # fully outside
    sums = _check(rec, targets, idx, mats, src, R, "mixed planes")
    print("R", R, "N", sums[:, 0], "S / N", np.round(sums[:, 1] / np.maximum(sums[:, 0], 1) / 2.0 ** 24, 4))
    assert sums[9, 0] == 0 and sums[9, 1] == 0                          # nothing sampled
    assert sums[8, 0] == 0                                              # a flat target has no window with structure
    assert (sums[:8, 0] > 0).sum() >= (6 if R < 7 else 3) and (sums[:, 1] != 0).any()
    if R == 1:
        assert sums[0, 0] > 0 and sums[6, 0] > 0                        # the 5 x 7 plane (at R = 3 and 7 every window of it is clipped)
    # a flat source: every window with target structure is counted and scores nothing
    flat = np.full(ssize[::-1], 123, np.int16)
    rec.ncc_set_source(flat)
    s_flat = _check(rec, targets, idx[:4], mats[:4], flat, R, "flat source")
    assert (s_flat[:, 1] == 0).all() and s_flat[1:, 0].min() > 0


@pytest.mark.gpu
def test_device_lncc_has_integer_headroom_at_the_largest_window():
    from fetalreconstruction_amd import engine as E
    rec = E.Reconstruction(0)
    rng = np.random.default_rng(5)
    ssize = (24, 26, 22)
    top = lambda shape: np.where(rng.random(shape) < 0.5, 32767, rng.integers(32000, 32768, shape)).astype(np.int16)   # noqa: E731
    src, plane = top(ssize[::-1]), top((40, 45))
    plane[3, 4] = 0
    src[5, 6, 7] = 0
    targets = plane[None]
    rec.ncc_set_targets(targets)
    rec.ncc_set_source(src)
    mats = np.stack([np.array([[0.4, 0.02, 0, 2.5], [-0.02, 0.45, 0, 3.5], [0.01, 0.03, 1, 9.25], [0, 0, 0, 1.0]]),
                     np.array([[0.45, 0, 0, 1.0], [0, 0.5, 0, 1.0], [0, 0, 1, 5.0], [0, 0, 0, 1.0]])])   # the second lands on voxels: s = 32767
    sums = _check(rec, targets, np.zeros(2, np.int32), mats, src, 7, "headroom")
    assert sums[:, 0].min() > 1000


@pytest.mark.gpu
@pytest.mark.parametrize("tx,ty,R", [(20, 9, 3), (32, 33, 1), (64, 32, 3), (65, 70, 7), (100, 93, 3), (129, 40, 7), (256, 34, 3), (300, 70, 7)])
def test_device_lncc_at_the_sizes_where_the_kernel_retiles(tx, ty, R):
    """the column groups of a workgroup change at 32, 64 and 128 columns, planes beyond 256 columns go in strips, and the rows in bands of
    32 whose halo stays in the ring"""
    from fetalreconstruction_amd import engine as E
    rec = E.Reconstruction(0)
    rng = np.random.default_rng(tx * 1000 + ty)
    ssize = (40, 44, 36)
    src = (rng.integers(0, 400, ssize[::-1]) + np.indices(ssize[::-1]).sum(0) * 25).astype(np.int16)
    targets = rng.integers(-1, 3000, (2, ty, tx)).astype(np.int16)
    targets[1][rng.random((ty, tx)) < 0.3] = -1
    rec.ncc_set_targets(targets)
    rec.ncc_set_source(src)
    idx = np.array([0, 1, 1], np.int32)
    mats = np.concatenate([_plane_matrices(rng, (tx, ty, 1), ssize, 1) for _ in idx])
    mats[:, :3, :2] *= min(1.0, 36.0 / max(tx, ty))                     # keep most of a large plane inside the source
    mats[:, :3, 3] = (np.array(ssize) - 1) / 2 - mats[:, :3, :2] @ ((np.array([tx, ty]) - 1) / 2)
    sums = _check(rec, targets, idx, mats, src, R, (tx, ty))
    assert sums[0, 0] > 0.2 * tx * ty


@pytest.mark.gpu
def test_lncc_evaluate_checks_its_arguments():
    from fetalreconstruction_amd import engine as E
    rec = E.Reconstruction(0)
    with pytest.raises(E.SvrError):                                     # no targets, no source
        rec.lncc_evaluate([0], np.eye(4)[None])
    rec.ncc_set_targets(np.zeros((2, 8, 8), np.int16))
    rec.ncc_set_source(np.zeros((4, 4, 4), np.int16))
    for bad in (0, 8, -3):
        with pytest.raises(E.SvrError):
            rec.lncc_evaluate([0], np.eye(4)[None], bad)
    with pytest.raises(E.SvrError):
        rec.lncc_evaluate([2], np.eye(4)[None])
    rec.lncc_evaluate([1], np.eye(4)[None])


@pytest.mark.gpu
def test_engine_and_restatement_give_the_same_lncc_trajectory(tiny, oracle_mod):
    """the decisions of the optimiser coincide between the device (on the device pyramids) and the numpy restatement behind the C++
    schedule (on the host pyramids): identical transformations and evaluation counts"""
    from fetalreconstruction_amd import engine as E
    rec = E.Reconstruction(0)
    vol, rattr, sel, T, P = _slice_case(tiny, oracle_mod)
    sattr = [tiny.slice_attr[k] for k in sel]
    slices, aattr, AP, ara, avol = _analytic_slice_case()
    for args, R in (((tiny.slices[sel], sattr, P, rattr, vol), 3), ((ramp(slices, 10.0)[:3], aattr[:3], AP[:3], ara, avol), 2)):
        dev, nev_d = host.SliceToVolumeRegistration(rec, *args, similarity="lncc", radius=R)
        cpu, nev_c = host.SliceToVolumeRegistration(None, *args, backend=_lncc_backend(R), similarity="lncc", radius=R)
        assert nev_d == nev_c and nev_d > 100 and np.array_equal(dev, cpu)
        assert not np.array_equal(dev, args[2])
    a, data, t_pack, ra, pvol = _package_case()
    start = np.tile(np.eye(4), (a.nz, 1, 1))
    dev, nev_d = host.PackageToVolume(rec, [data], [a], [2], start, ra, pvol, similarity="lncc")
    cpu, nev_c = host.PackageToVolume(None, [data], [a], [2], start, ra, pvol, backend=_lncc_backend(), similarity="lncc")
    assert nev_d == nev_c and nev_d > 50 and np.array_equal(dev, cpu)


@pytest.mark.gpu
def test_command_line_use_lncc(cli_case):   # noqa: F811
    from fetalreconstruction_amd import nifti
    d, common = cli_case
    out = d / "lncc.nii.gz"
    # (--smooth_mask 0: the default 4 mm smoothing thresholds this phantom's 10 mm mask away, whatever the metric)
    r = subprocess.run([build.CLI, "-o", str(out), *common, "--useLNCC", "--lnccRadius", "2", "--iterations", "2", "--smooth_mask", "0"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    vol, _ = nifti.read(out)
    assert np.isfinite(vol).all() and vol.max() > 0
    assert "slice-to-volume registration (LNCC, radius 2):" in r.stderr
