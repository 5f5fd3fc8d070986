"""An independent numpy restatement, in float64, of one evaluateCostsMultipleSlices call of the float slice-to-volume
registration (csrc/svr_reg.inc, oracle/reg_oracle.c) and of the patch cost computeCCpatch -- written from what the operations
mean, not from either implementation, and returning every intermediate so that a test can say which stage went wrong.

What is kept in float32 on purpose: the coordinate chain (offset matrix, slice matrix, world-to-image, the texture unit's
normalised coordinate and its 8-bit filter fraction), because it decides WHICH voxels are read and with which weights; that is
part of the definition, not of the arithmetic.  Everything that adds or multiplies intensities is float64."""
import numpy as np

F = np.float32


def gauss_half(sigma):
    """the registration's Gaussian: int(5 sigma) taps, at least 7, at most 63, made odd downwards; normalised over the whole
    kernel.  -> (taps, half kernel [centre, +1, ...] in float64)"""
    sigma = F(sigma)
    k = int(sigma * F(5))
    k = max(min(k, 63), 7)
    if k % 2 == 0:
        k -= 1
    d = np.arange(k) - k // 2
    w = np.exp(-(d.astype(np.float64) ** 2) / (2.0 * float(sigma) ** 2))
    w /= w.sum()
    return k, w[k // 2:]


def level_sigma(vdim, level):
    s = F(vdim) / F(2)
    for _ in range(level):
        s = s * F(2)
    return s


def matvec32(M, x, y, z):
    """rows 0..2 of a row-major 4x4 (or of n of them, [n][16], one per leading index of the coordinates) applied to
    (x, y, z, 1): float32, products added left to right"""
    M = np.asarray(M, F)
    x, y, z = (np.asarray(v, F) for v in (x, y, z))
    M = M.reshape(-1) if M.size == 16 else M.reshape(-1, 16).T.reshape((16, -1) + (1,) * (x.ndim - 1))
    return (M[0] * x + M[1] * y + M[2] * z + M[3], M[4] * x + M[5] * y + M[6] * z + M[7], M[8] * x + M[9] * y + M[10] * z + M[11])


def _tex_axis(p, n):
    """normalised texture coordinate of a linear filter: u = p / n, xB = n u - 0.5, cell = floor, 8-bit fraction"""
    n = F(n)
    xb = (p / n) * n - F(0.5)
    fl = np.floor(xb)
    fr = xb - fl
    return fl.astype(np.int64), (np.floor(fr * F(256) + F(0.5)) / F(256)).astype(np.float64)


def _fetch0(vol, i, j, k):
    """vol [vz][vy][vx]; 0 outside (border colour)"""
    vz, vy, vx = vol.shape
    ok = (i >= 0) & (j >= 0) & (k >= 0) & (i < vx) & (j < vy) & (k < vz)
    return np.where(ok, vol[np.clip(k, 0, vz - 1), np.clip(j, 0, vy - 1), np.clip(i, 0, vx - 1)], 0.0)


def sample_slices(vol, w2i, ofs, mats, W, H, active):
    """the sampled slices [3][len(active)][H][W] at through-plane offsets -2, 0, +2 of the slice grid: trilinear, border 0,
    a negative sample is padding (-1)"""
    vol = np.asarray(vol, np.float64)
    vz, vy, vx = vol.shape
    yy, xx = np.meshgrid(np.arange(H, dtype=F), np.arange(W, dtype=F), indexing="ij")
    n = len(active)
    out = np.zeros((3, n, H, W))
    xx, yy = np.broadcast_to(xx, (n, H, W)), np.broadcast_to(yy, (n, H, W))
    ofs, mats = np.asarray(ofs, F).reshape(-1, 16)[active], np.asarray(mats, F).reshape(-1, 16)[active]
    for o in range(3):
        p = matvec32(ofs, xx, yy, np.full((n, H, W), (o - 1) * 2, F))
        p = matvec32(mats, *p)
        p = matvec32(w2i, *p)
        (i, a), (j, b), (k, c) = _tex_axis(p[0], vx), _tex_axis(p[1], vy), _tex_axis(p[2], vz)
        t = 0.0
        for dk, wk in ((0, 1 - c), (1, c)):
            for dj, wj in ((0, 1 - b), (1, b)):
                for di, wi in ((0, 1 - a), (1, a)):
                    t = t + wi * wj * wk * _fetch0(vol, i + di, j + dj, k + dk)
        out[o] = np.where(t < 0, -1.0, t)
    return out


def blur(layers, half, half_y=None, outside_zero=False):
    """separable blur of [n][H][W]: a pixel equal to -1 stays; any other becomes the un-normalised sum of the taps over its
    neighbours with negative neighbours read as 0; a neighbour beyond the edge is the clamped edge pixel (outside_zero: 0, the
    patch-based filter).  half_y: another half kernel for the second pass (the patch path's 13-tap quirk)."""
    a = np.asarray(layers, np.float64)
    for axis, h in ((2, half), (1, half if half_y is None else half_y)):
        n = a.shape[axis]
        idx = np.arange(n)
        pos = np.maximum(a, 0.0)
        acc = a * h[0]
        for i in range(1, len(h)):
            for d in (i, -i):
                j = idx + d
                v = np.take(pos, np.clip(j, 0, n - 1), axis=axis)
                if outside_zero:
                    shape = [1, 1, 1]
                    shape[axis] = n
                    v = v * ((j >= 0) & (j < n)).reshape(shape)
                acc = acc + h[i] * v
        a = np.where(a == -1, -1.0, acc)
    return a


def sums(layers):
    """per layer: sum and count of the values > -1"""
    a = np.asarray(layers, np.float64)
    m = a > -1
    ax = tuple(range(a.ndim - 2, a.ndim))
    return np.where(m, a, 0.0).sum(ax), m.sum(ax)


def combine(mom, a, s):
    """the three per-offset moments of each slot -> its similarity, through the reference's scratch layout: one float array of
    6 s entries, the accumulated value of slot i at 2a + i and its moments at 3a + 3i + k, of which the entries [2s, 5s) are
    cleared before every offset's moments are added"""
    buf = np.zeros(6 * s)
    slots = np.arange(a)
    for o in range(3):
        buf[2 * s:5 * s] = 0
        for k in range(3):
            buf[3 * a + 3 * slots + k] += mom[o, :, k]
        r = buf[3 * a:6 * a].reshape(a, 3)
        norm = r[:, 1] * r[:, 2]
        res = np.where(norm > 0, r[:, 0] / np.sqrt(np.where(norm > 0, norm, 1.0)), 0.0)
        buf[2 * a + slots] += res
    return buf[2 * a:3 * a].copy()


def evaluate(vol, vdim, w2i, ofs, targets, mats, level, active=None):
    """one cost evaluation on the blurred targets of `level` -> dict of every stage"""
    targets = np.asarray(targets, np.float64)
    ns, H, W = targets.shape
    active = list(range(ns)) if active is None else [int(v) for v in active]
    a = len(active)
    klen, half = gauss_half(level_sigma(vdim, level))
    r = {"klen": klen}
    r["targets"] = blur(targets, half)
    r["sumA"], r["cntA"] = sums(r["targets"])
    r["sampled"] = sample_slices(vol, w2i, ofs, mats, W, H, active)
    r["blurred"] = blur(r["sampled"].reshape(3 * a, H, W), half).reshape(3, a, H, W)
    r["sumB"], r["cntB"] = sums(r["blurred"])
    def mean(s, c):
        return np.where(s != 0, s / np.maximum(c, 1), 0.0)[:, None, None]
    A = r["targets"][active]
    mean_a = mean(r["sumA"][active], r["cntA"][active])
    mom = np.zeros((3, a, 3))
    keep = (np.arange(H * W) % (level + 1) == 0).reshape(H, W)
    run_s, run_c = np.cumsum(r["sumB"], 0), np.cumsum(r["cntB"], 0)          # the sampled-slice mean runs over the offsets so far
    for o in range(3):
        B = r["blurred"][o]
        m = (A >= 0) & (B >= 0) & keep
        sa, sb = np.where(m, A - mean_a, 0.0), np.where(m, B - mean(run_s[o], run_c[o]), 0.0)
        mom[o] = np.stack([(sa * sb).sum((1, 2)), (sa * sa).sum((1, 2)), (sb * sb).sum((1, 2))], -1)
    r["pairs"] = np.stack([((A >= 0) & (r["blurred"][o] >= 0) & keep).sum((1, 2)) for o in range(3)])
    r["mom"] = mom
    sim = np.zeros(ns)
    sim[active] = combine(mom, a, ns)
    r["sim"] = sim
    return r


# ---- the patch cost -----------------------------------------------------------------------------------------------------------
def matmul32(A, B):
    A, B = np.asarray(A, F).reshape(4, 4), np.asarray(B, F).reshape(4, 4)
    out = np.zeros((4, 4), F)
    for i in range(4):
        for j in range(4):
            out[i, j] = A[i, 0] * B[0, j] + A[i, 1] * B[1, j] + A[i, 2] * B[2, j] + A[i, 3] * B[3, j]
    return out


def patch_samples(vol, w2i, M, xs, ys, zs):
    """the volume [vz][vy][vx] at the patch-grid points (xs, ys, zs) through M (patch grid -> world) and w2i: software trilinear
    with lower = max(base, 0), upper = min(base + 1, n - 1) and 0 for an index out of range (so below 0 the lower corner is voxel 0
    and the upper one reads 0); coordinates in float32, the interpolation in float64"""
    vol = np.asarray(vol, np.float64)
    vz, vy, vx = vol.shape
    p = matvec32(M, np.asarray(xs, F), np.asarray(ys, F), np.asarray(zs, F))
    p = matvec32(w2i, *p)
    lo, up, fr = [], [], []
    for c, n in zip(p, (vx, vy, vz)):
        fl = np.floor(c)
        base = fl.astype(np.int64)
        fr.append((c - fl).astype(np.float64))
        lo.append(np.maximum(base, 0))
        up.append(np.minimum(base + 1, n - 1))
    b = 0.0
    for kz, wz in ((lo[2], 1 - fr[2]), (up[2], fr[2])):
        for jy, wy in ((lo[1], 1 - fr[1]), (up[1], fr[1])):
            for ix, wx in ((lo[0], 1 - fr[0]), (up[0], fr[0])):
                b = b + _fetch0(vol, ix, jy, kz) * wx * wy * wz
    return b


def cc_patch(buf, ri2w, tmat, w2i, vol, level):
    """raw-moment NCC of one patch [py][px] against the volume [vz][vy][vx]: every (level+1)-th pixel, patch-grid offsets
    z = -1, 0, 1, software trilinear with lower = max(base, 0), upper = min(base + 1, n - 1) and 0 for an index out of range;
    pairs with a >= 0 and b >= 0 count.  -> (ncc, [n, sum a, sum b, sum a^2, sum b^2, sum ab])"""
    buf, vol = np.asarray(buf, np.float64), np.asarray(vol, np.float64)
    py, px = buf.shape
    vz, vy, vx = vol.shape
    st = level + 1
    ys, xs, zs = np.meshgrid(np.arange(0, py, st), np.arange(0, px, st), np.arange(-1, 2), indexing="ij")
    a = buf[ys, xs]
    b = patch_samples(vol, w2i, matmul32(tmat, ri2w), xs, ys, zs)
    m = (a >= 0) & (b >= 0)
    a, b = a[m], b[m]
    s = np.array([m.sum(), a.sum(), b.sum(), (a * a).sum(), (b * b).sum(), (a * b).sum()], np.float64)
    if s[0] == 0:
        return 0.0, s
    den = np.sqrt(s[3] - s[1] * s[1] / s[0]) * np.sqrt(s[4] - s[2] * s[2] / s[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        return float((s[5] - s[1] * s[2] / s[0]) / den), s
