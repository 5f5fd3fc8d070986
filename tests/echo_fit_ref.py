"""The mono-exponential fit S(x) = A exp(-R x) of DESIGN 9e (svr_monoexp_fit, csrc/svr_fit.inc) restated in numpy float64, voxel by voxel, with
the same sample order and the same decisions.  Written from the formulas, not from the kernel: it is the yardstick of tests/test_echo_fit.py
and tests/test_echo_fit_gpu.py.

Per voxel, over the samples k = 0 .. K-1 in that order:
    usable_k = C_k finite and C_k > floor;   count = the number of usable samples;   count < 2 -> every other output 0
    y = ln C_k, w = C_k^2;   Sw, Swx, Swxx, Swy, Swxy;   D = Sw Swxx - Swx^2;   D not positive -> 0
    R = -(Sw Swxy - Swx Swy) / D,   A = exp((Swxx Swy - Swx Swxy) / D);   not finite -> 0
    iterations > 0: that many Gauss-Newton steps on the residuals C_k - a exp(-r x_k), kept if their sum of squares is not above (A, R)'s
    rmse = sqrt(sum (C_k - A exp(-R x_k))^2 / count) for the pair returned
    an output that is not finite once rounded to float32 -> rate, amplitude and rmse 0
"""
import math

import numpy as np


def _exp(v):
    """exp in IEEE terms: inf where the result overflows (math.exp raises there)"""
    try:
        return math.exp(v)
    except OverflowError:
        return math.inf


def _sum_squares(c, x, a, r):
    ss = 0.0
    for ck, xk in zip(c, x):
        d = ck - a * _exp(-r * xk)
        ss += d * d
    return ss


def fit_voxel(c, x, iterations=0, floor=0.0):
    """c: the K samples of one voxel (any floats), x: the K abscissae -> (rate, amplitude, rmse, count) as Python floats (float64)"""
    use = [(float(ck), float(xk)) for ck, xk in zip(c, x) if math.isfinite(ck) and ck > floor]
    count = float(len(use))
    zero = (0.0, 0.0, 0.0, count)
    if len(use) < 2:
        return zero
    cs = [u[0] for u in use]
    xs = [u[1] for u in use]
    sw = swx = swxx = swy = swxy = 0.0
    for ck, xk in use:                                       # (Python floats: a product that overflows is inf, and inf - inf below is nan)
        y = math.log(ck)
        w = ck * ck
        wx = w * xk
        sw = sw + w
        swx = swx + wx
        swxx = swxx + wx * xk
        swy = swy + w * y
        swxy = swxy + wx * y
    d = sw * swxx - swx * swx
    if not d > 0.0:
        return zero
    rate = -(sw * swxy - swx * swy) / d
    ln_a = (swxx * swy - swx * swxy) / d
    amp = _exp(ln_a)
    if not (math.isfinite(rate) and math.isfinite(amp)):
        return zero
    if iterations > 0:
        a, r = amp, rate
        for _ in range(int(iterations)):
            a11 = a12 = a22 = g1 = g2 = 0.0
            for ck, xk in use:
                e = _exp(-r * xk)
                j1 = e
                j2 = -a * xk * e
                res = ck - a * e
                a11 += j1 * j1
                a12 += j1 * j2
                a22 += j2 * j2
                g1 += j1 * res
                g2 += j2 * res
            det = a11 * a22 - a12 * a12
            if not det > 1e-30 * a11 * a22:
                break
            a = a + (a22 * g1 - a12 * g2) / det
            r = r + (a11 * g2 - a12 * g1) / det
            if not (math.isfinite(a) and math.isfinite(r)):
                a, r = amp, rate
                break
        if _sum_squares(cs, xs, a, r) <= _sum_squares(cs, xs, amp, rate):
            amp, rate = a, r
    ss = _sum_squares(cs, xs, amp, rate)
    rmse = math.sqrt(ss / count) if ss == ss else math.nan
    with np.errstate(all="ignore"):
        if not all(np.isfinite(np.float32(v)) for v in (rate, amp, rmse)):
            return zero
    return rate, amp, rmse, count


def fit(vols, x, iterations=0, floor=0.0):
    """vols [K][n] (or [K][...]), x [K] -> rate, amplitude, rmse, count as float64 arrays of vols[0]'s shape, not yet rounded to float32"""
    v = np.asarray(vols)
    k = v.shape[0]
    flat = v.reshape(k, -1)
    xs = [float(t) for t in x]
    assert len(xs) == k
    out = np.zeros((4, flat.shape[1]), np.float64)
    for i in range(flat.shape[1]):
        out[:, i] = fit_voxel([float(t) for t in flat[:, i]], xs, iterations, floor)
    return tuple(o.reshape(v.shape[1:]) for o in out)


def t_map(rate, amplitude, t_max):
    """--fitT from the float32 maps the command line holds: 1 / R where R > 1 / Tmax, Tmax where a fitted voxel has R <= 1 / Tmax, 0 where nothing
    was fitted.  A voxel is fitted where its amplitude is positive: an amplitude is the exponential of something, and 0 only as the refusal."""
    r = np.asarray(rate, np.float32).astype(np.float64)
    fitted = np.asarray(amplitude, np.float32) > 0
    with np.errstate(all="ignore"):
        t = np.where(r > 1.0 / t_max, 1.0 / r, t_max)
    return np.where(fitted, t, 0.0).astype(np.float32)
