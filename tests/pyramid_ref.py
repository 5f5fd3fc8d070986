"""An independent numpy reference of one level of the registration pyramid, written from the IRTK text, not from the kernels:

  irtkConvolutionWithPadding_1D<short>::Run            IRTKSimple2/image++/src/irtkConvolutionWithPadding_1D.cc:38-90
  irtkGaussianBlurringWithPadding<short>::Run          .../irtkGaussianBlurringWithPadding.cc:35-121  (x, y, then z unless nz == 1)
  irtkResamplingWithPadding<short>::Initialize / Run   .../irtkResamplingWithPadding.cc:202-443
  irtkImageRegistrationWithPadding::Initialize         IRTKSimple2/packages/registration/src/irtkImageRegistrationWithPadding.cc:120-160
  irtkImageRigidRegistrationWithPadding::GuessParameterThickSlices / GuessParameterSliceToVolume   ...RigidRegistrationWithPadding.cc:110-205, 304-400

Images are int16 [nz][ny][nx].  Everything is vectorised over the voxels but every voxel's arithmetic is the reference's, IEEE
double, in the reference's order, so the result equals the C++ (host and device) exactly: the tests compare with array_equal.

Every quotient can also be evaluated with another accumulator type (`acc=np.longdouble`): the order-independent second
opinion of tests/test_pyramid_ref.py -- a float64 result may differ from it only where the exact quotient is an integer to
1e-9, i.e. where the truncation to short is decided by the last bits.
"""
from __future__ import annotations

import copy

import numpy as np

from fetalreconstruction_amd import geometry as geo

MIN_GREY, MAX_GREY = -32768, 32767


def put_as_double(q):
    """irtkGenericImage<short>::PutAsDouble (irtkGenericImage.h:303-333): clamp to the range of short, then static_cast
    (truncation towards zero)"""
    return np.trunc(np.clip(q, float(MIN_GREY), float(MAX_GREY))).astype(np.int16)


# ---- blur ------------------------------------------------------------------------------------------------------------------
def blur_quotient(img, axis, ker, pad, acc=np.float64):
    """One 1-D pass along axis 0 = x, 1 = y, 2 = z: (val / sum or 0 where sum is not > 0, the voxels > pad).
    The taps are added in ascending order; a tap counts only if it lies inside the axis and its voxel is > pad."""
    img = np.asarray(img, np.int16)
    ker = np.asarray(ker, np.float64)
    assert ker.size % 2 == 1
    half = ker.size // 2
    ax = 2 - axis                                            # [z][y][x]
    n = img.shape[ax]
    pos = np.arange(n)
    val = np.zeros(img.shape, acc)
    tot = np.zeros(img.shape, acc)
    shape = [1, 1, 1]
    shape[ax] = n
    for t in range(-half, half + 1):
        q = pos + t
        inside = ((q >= 0) & (q < n)).reshape(shape)
        g = np.take(img, np.clip(q, 0, n - 1), axis=ax)
        ok = inside & (g > pad)
        k = acc(ker[t + half])
        val = val + np.where(ok, k * g.astype(acc), acc(0))
        tot = tot + np.where(ok, k, acc(0))
    good = tot > 0
    return np.where(good, val / np.where(good, tot, acc(1)), acc(0)), img > pad


def blur_pass(img, axis, ker, pad):
    q, centre = blur_quotient(img, axis, ker, pad)
    return np.where(centre, put_as_double(q), np.int16(pad)).astype(np.int16)       # a centre <= pad stays pad (CWP_1D.cc:45)


def blur(img, kernels, pad):
    """the passes of irtkGaussianBlurringWithPadding in its order x, y, z, each truncated back to short; kernels[a] None or
    empty: no pass on that axis (the reference skips z when nz == 1)"""
    out = np.asarray(img, np.int16)
    for axis in range(3):
        if kernels[axis] is not None and len(kernels[axis]):
            out = blur_pass(out, axis, kernels[axis], pad)
    return out


def gaussian_kernel(sigma, voxel):
    """the taps irtkGaussianBlurringWithPadding samples from irtkScalarGaussian (GBWP.cc:60-120): 2 round(4 sigma / voxel) + 1 taps
    of exp(-x^2 / 2 s^2) / (sqrt(2 pi) s (sqrt(2 pi))^2), s = sigma / voxel.  (numpy's exp need not have libm's last bit: the tests
    feed both sides the host's own kernel and compare that kernel with this one to a few ulp.)"""
    s = sigma / voxel
    r = geo.irtk_round(4 * sigma / voxel)
    x = np.arange(-r, r + 1, dtype=np.float64)
    return np.exp(-(x * x) / (2.0 * s * s)) / (np.sqrt(2.0 * np.pi) * s * np.sqrt(2.0 * np.pi) * np.sqrt(2.0 * np.pi))


# ---- resampling ------------------------------------------------------------------------------------------------------------
def resampled_attr(attr, res):
    """irtkResamplingWithPadding::Initialize (RWP.cc:202-252): n' = round(n d / d'), and an axis that would get no voxel keeps
    one voxel of its old size"""
    out = copy.copy(attr)
    n_new, d_new = [], []
    for n, old, new in zip((attr.nx, attr.ny, attr.nz), (attr.dx, attr.dy, attr.dz), res):
        m = geo.irtk_round(n * old / new)
        if m < 1:
            m, new = 1, old
        n_new.append(int(m))
        d_new.append(float(new))
    out.nx, out.ny, out.nz = n_new
    out.dx, out.dy, out.dz = d_new
    return out


def resample_quotient(img, attr, out_attr, pad, acc=np.float64):
    """Run (RWP.cc:254-443) -> (val / sum, written): every output voxel goes ImageToWorld of the output grid, then WorldToImage of
    the input grid (two matrix applications, each a11 x + a12 y + a13 z + a14 from left to right), u = floor, d = x - u.

    The eight corners are visited as (u,v,w) (u,v,w+1) (u,v+1,w) (u,v+1,w+1) (u+1,v,w) (u+1,v,w+1) (u+1,v+1,w) (u+1,v+1,w+1) with
    the weights (1-dx)(1-dy)(1-dz), (1-dx)(1-dy)dz, (1-dx)dy(1-dz), ... multiplied from left to right.  A corner inside the image
    whose voxel is not `pad` (!=, not >) adds voxel * weight to val and weight to sum.  The count of padded corners starts at 8
    and goes down by one for every corner that contributed AND for every corner outside the image -- an out-of-bounds corner
    counts as not padded.  The voxel is written when fewer than 4 corners are padded (npad < 4) and sum > 0, else it is `pad`.
    The positions are always float64 (they decide which corners are read); `acc` is the type of the weights' sums."""
    img = np.asarray(img, np.int16)
    nz, ny, nx = img.shape
    kk, jj, ii = np.meshgrid(np.arange(out_attr.nz, dtype=np.float64), np.arange(out_attr.ny, dtype=np.float64),
                             np.arange(out_attr.nx, dtype=np.float64), indexing="ij")
    world = geo.apply_points(geo.image_to_world(out_attr), np.stack([ii, jj, kk], -1))
    p = geo.apply_points(geo.world_to_image(attr), world)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    u, v, w = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64), np.floor(z).astype(np.int64)
    dx, dy, dz = (x - u).astype(acc), (y - v).astype(acc), (z - w).astype(acc)
    one = acc(1)
    val = np.zeros(x.shape, acc)
    tot = np.zeros(x.shape, acc)
    npad = np.full(x.shape, 8, np.int64)
    for du, fx in ((0, one - dx), (1, dx)):
        for dv, fy in ((0, one - dy), (1, dy)):
            for dw, fz in ((0, one - dz), (1, dz)):
                wt = fx * fy * fz
                a, b, c = u + du, v + dv, w + dw
                inb = (a >= 0) & (a < nx) & (b >= 0) & (b < ny) & (c >= 0) & (c < nz)
                g = img[np.clip(c, 0, nz - 1), np.clip(b, 0, ny - 1), np.clip(a, 0, nx - 1)]
                ok = inb & (g != pad)
                val = val + np.where(ok, g.astype(acc) * wt, acc(0))
                tot = tot + np.where(ok, wt, acc(0))
                npad = npad - (ok | ~inb)
    written = (npad < 4) & (tot > 0)
    return np.where(written, val / np.where(written, tot, one), acc(0)), written


def resample(img, attr, res, pad):
    """-> (int16 [nz'][ny'][nx'], the new attributes)"""
    out_attr = resampled_attr(attr, res)
    q, written = resample_quotient(img, attr, out_attr, pad)
    return np.where(written, put_as_double(q), np.int16(pad)).astype(np.int16), out_attr


# ---- the range above the padding, the shift ----------------------------------------------------------------------------------
def range_and_shift(img, pad):
    """Initialize (IRWP.cc:120-160): min and max of the voxels > pad (MAX_GREY, MIN_GREY when there is none), every such voxel
    becomes v - min and every other voxel -1.  A range above MAX_GREY stops the reference."""
    img = np.asarray(img, np.int16)
    above = img > pad
    mn = int(img[above].min()) if above.any() else MAX_GREY
    mx = int(img[above].max()) if above.any() else MIN_GREY
    if mx - mn > MAX_GREY:
        raise ValueError("dynamic range of an image is too large")
    return np.where(above, img.astype(np.int32) - mn, -1).astype(np.int16), mn, mx


def needs_resampling(attr, res0, level):
    """Initialize resamples at every level but the finest, and there when the level's resolution is not the image's (IRWP.cc:62-80)"""
    return level > 0 or abs(res0[0] - attr.dx) + abs(res0[1] - attr.dy) + abs(res0[2] - attr.dz) > 0.000001


def prepare_level(img, attr, kernels, do_resample, res, pad):
    """blur, resample, range, shift -> (int16 image, its attributes, min, max)"""
    out, out_attr = blur(img, kernels, pad), attr
    if do_resample:
        out, out_attr = resample(out, attr, res, pad)
    out, mn, mx = range_and_shift(out, pad)
    return out, out_attr, mn, mx


def schedule(attr, slice_to_volume):
    """GuessParameterThickSlices (an image of a stack registration: the z resolution stays) / GuessParameterSliceToVolume (the
    source volume: isotropic at the smallest voxel size) -> [(blur sigma in mm, (rx, ry, rz))] for levels 0, 1, 2: the blur and
    the in-plane resolution double from level to level, z doubles for the volume only."""
    size = min(attr.dx, attr.dy)
    if slice_to_volume:
        size = min(size, attr.dz)
    blur_, res = size / 2.0, [size, size, size if slice_to_volume else attr.dz]
    out = []
    for _ in range(3):
        out.append((blur_, tuple(res)))
        blur_ = blur_ * 2
        res = [res[0] * 2, res[1] * 2, res[2] * 2 if slice_to_volume else res[2]]
    return out
