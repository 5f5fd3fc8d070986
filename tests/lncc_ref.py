"""The windowed cross correlation of csrc/svr_lncc.inc (--useLNCC) restated in numpy: the sampling of k_ncc (double trilinear in
EvaluateInside's order, strict inside test, value >= 0, IRTK round()), the (2R+1)^2 box sums over the sampled pixels by cumulative sums
in int64, the signed squared local correlation in double (two divisions, one multiplication) and its 2^-24 fixed point.  Everything
summed is an integer, so the device must give these numbers bit for bit."""
import numpy as np

NOT_COUNTED = np.iinfo(np.int32).min
SCALE = float(1 << 24)


def sample_plane(target, M, source):
    """-> (valid bool [ty][tx], t int64, s int64): V, and the two integer operands on it (0 elsewhere)"""
    tg = np.asarray(target)
    src = np.asarray(source).astype(np.float64)
    vz, vy, vx = src.shape
    ty, tx = tg.shape
    valid = np.zeros((ty, tx), bool)
    t, s = np.zeros((ty, tx), np.int64), np.zeros((ty, tx), np.int64)
    jj, ii = np.nonzero(tg >= 0)
    i, j = ii.astype(np.float64), jj.astype(np.float64)
    X = M[0, 0] * i + M[0, 1] * j + M[0, 3]
    Y = M[1, 0] * i + M[1, 1] * j + M[1, 3]
    Z = M[2, 0] * i + M[2, 1] * j + M[2, 3]
    ok = (X > 0) & (X < vx - 1) & (Y > 0) & (Y < vy - 1) & (Z > 0) & (Z < vz - 1)
    X, Y, Z, ii, jj = X[ok], Y[ok], Z[ok], ii[ok], jj[ok]
    a, b, c = X.astype(np.int64), Y.astype(np.int64), Z.astype(np.int64)
    t1, u1, v1 = X - a, Y - b, Z - c
    t2, u2, v2 = 1 - t1, 1 - u1, 1 - v1

    def q(dz, dy, dx):
        return src[c + dz, b + dy, a + dx]
    value = (t1 * (u2 * (v2 * q(0, 0, 1) + v1 * q(1, 0, 1)) + u1 * (v2 * q(0, 1, 1) + v1 * q(1, 1, 1))) +
             t2 * (u2 * (v2 * q(0, 0, 0) + v1 * q(1, 0, 0)) + u1 * (v2 * q(0, 1, 0) + v1 * q(1, 1, 0))))
    keep = value >= 0
    ii, jj = ii[keep], jj[keep]
    valid[jj, ii] = True
    t[jj, ii] = tg[jj, ii]
    s[jj, ii] = (value[keep] + 0.5).astype(np.int64)          # IRTK round() of a value >= 0
    return valid, t, s


def box_sum(a, R):
    """the sum of int64 a over the (2R+1)^2 box around every pixel, clipped to the plane: differences of a 2-D cumulative sum"""
    ty, tx = a.shape
    c = np.zeros((ty + 1, tx + 1), np.int64)
    c[1:, 1:] = np.cumsum(np.cumsum(a, 0, dtype=np.int64), 1, dtype=np.int64)
    y0, y1 = np.clip(np.arange(ty) - R, 0, ty), np.clip(np.arange(ty) + R + 1, 0, ty)
    x0, x1 = np.clip(np.arange(tx) - R, 0, tx), np.clip(np.arange(tx) + R + 1, 0, tx)
    return c[y1][:, x1] - c[y0][:, x1] - c[y1][:, x0] + c[y0][:, x0]


def lncc_from_samples(valid, t, s, R):
    """-> (N, S, k int32 [ty][tx] with NOT_COUNTED where a pixel is not counted)"""
    m = box_sum(valid.astype(np.int64), R)
    St, Ss, Stt, Sss, Sts = (box_sum(v, R) for v in (t, s, t * t, s * s, t * s))
    A, B, C = m * Sts - St * Ss, m * Stt - St * St, m * Sss - Ss * Ss
    assert max(np.abs(A).max(initial=0), np.abs(B).max(initial=0), np.abs(C).max(initial=0)) < 2 ** 53
    counted = valid & (m >= ((2 * R + 1) ** 2 + 1) // 2) & (B > 0)
    scored = counted & (C != 0)
    q = np.zeros(valid.shape, np.float64)
    Ad = A[scored].astype(np.float64)
    q[scored] = (Ad / B[scored].astype(np.float64)) * (Ad / C[scored].astype(np.float64))
    q[scored & (A < 0)] *= -1.0
    k = np.floor(q * SCALE + 0.5).astype(np.int64)
    kmap = np.where(counted, k, NOT_COUNTED).astype(np.int32)
    return int(counted.sum()), int(k[counted].sum()), kmap


def lncc_plane(target, M, source, R=3):
    """one plane of one evaluation -> (N, S, k map)"""
    return lncc_from_samples(*sample_plane(target, M, source), R)


def evaluator(R=3):
    """the `fn` of host.NccBackend for similarity="lncc": {N, S} of a plane"""
    return lambda target, M, source: lncc_plane(target, M, source, R)[:2]


def similarity(pairs):
    """(sum S / sum N) / 2^24 over the planes' (N, S) of one evaluation, 0 when nothing is counted"""
    n, s = sum(p[0] for p in pairs), sum(p[1] for p in pairs)
    return (float(s) / float(n)) / SCALE if n > 0 else 0.0
