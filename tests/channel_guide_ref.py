"""Shared by tests/test_channel_guide.py and tests/test_channel_guide_gpu.py: the guided volume update of a channel's SR iterations
(svr_channel_sr_guide, csrc/svr_channel.inc; the GUIDED kernels of csrc/svr_regul.inc; --channelGuide of csrc/svr_cli.cpp) restated in numpy, and
the noisy recovery case both legs run.

  update    orc_regularization_prep with an unbounded range and the clamp [lo, hi] on the float32 values, as channel_sr_ref.update has them; then
            the 13 directions in double, restated here because the weight of a pair is no longer the oracle's:
                b = f / sqrt(1 + omega f ((C_q - C_p) / delta)^2 + f ((G_q - G_p) / delta_g)^2),   f = 1 / |d|_1,
            b = 0 where either post-Prep confidence is <= 0 or q lies outside the volume; val, valW, k = alpha lambda / delta^2 and val / valW as
            orc_regularization (oracle/svr_oracle.c) has them.  Without a guide (guide = None) it is that function in double.
  the loop  channel_sr_ref's forward / factors / scatter around it.
"""
import ctypes as C

import numpy as np

from tests import channel_sr_ref as sr

DIRS = ((1, 0, -1), (0, 1, -1), (1, 1, -1), (1, -1, -1), (1, 0, 0), (0, 1, 0), (1, 1, 0), (1, -1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1), (1, -1, 1),
        (0, 0, 1))


def _shift(a, d, fill):
    """a[z + dz, y + dy, x + dx], `fill` where that lies outside"""
    dx, dy, dz = d
    p = np.pad(a, 1, constant_values=fill)
    vz, vy, vx = a.shape
    return p[1 + dz:1 + dz + vz, 1 + dy:1 + dy + vy, 1 + dx:1 + dx + vx]


def regularize(vsize, s, original, cmap, delta, alpha, lam, guide=None, delta_g=1.0, guide_only=False):
    """s, cmap: post-Prep value and confidence; original: the pre-update volume -> the updated volume (float64, flat)"""
    vx, vy, vz = vsize
    shp = (vz, vy, vx)
    s, o, c = (np.asarray(a, np.float64).reshape(shp) for a in (s, original, cmap))
    g = None if guide is None else np.asarray(guide, np.float64).reshape(shp)
    omega = 0.0 if (guide_only and g is not None) else 1.0
    inside = np.ones(shp, bool)
    sc = s * c
    val, valw, tot = np.zeros(shp), np.zeros(shp), np.zeros(shp)

    def weight(f, oa, ob, ca, cb, ga, gb, ok):
        w = 1.0 + omega * f * ((ob - oa) / delta) ** 2
        if g is not None:
            w = w + f * ((gb - ga) / delta_g) ** 2
        return np.where(ok & (ca > 0) & (cb > 0), f / np.sqrt(w), 0.0)

    for d in DIRS:
        f = 1.0 / float(sum(abs(v) for v in d))
        m = tuple(-v for v in d)
        in2, in3 = _shift(inside, d, False), _shift(inside, m, False)
        o2, c2, sc2 = _shift(o, d, 0.0), _shift(c, d, 0.0), _shift(sc, d, 0.0)
        o3, c3, sc3 = _shift(o, m, 0.0), _shift(c, m, 0.0), _shift(sc, m, 0.0)
        g2 = g3 = None
        if g is not None:
            g2, g3 = _shift(g, d, 0.0), _shift(g, m, 0.0)
        b = weight(f, o, o2, c, c2, g, g2, in2)                       # (pos, pos2)
        val += b * sc2; valw += b * c2; tot += b
        b = weight(f, o3, o2, c3, c2, g3, g2, in2 & in3)              # (pos3, pos2)
        val += b * sc3; valw += b * c3; tot += b
    val -= tot * sc
    valw -= tot * c
    k = float(alpha) * float(lam) / (float(delta) * float(delta))
    val = sc + k * val
    valw = c + k * valw
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(valw > 0, val / valw, 0.0).reshape(-1)


def update(po, prob, vol, addon, cmap, p, guide=None, delta_g=1.0, guide_only=False):
    """channel_sr_ref.update with the 13 directions restated in double; p as there (lam: the engine's lambda delta^2) -> float32"""
    vx, vy, vz = prob.vsize
    rec, ad, cm = po._f32(vol).reshape(-1).copy(), po._f32(addon).copy(), po._f32(cmap).copy()
    original = rec.copy()
    po.lib().orc_regularization_prep(vx, vy, vz, int(bool(p["adaptive"])), C.c_float(p["alpha"]), C.c_float(-np.inf), C.c_float(np.inf), po._p(rec), po._p(ad),
                                     po._p(cm))
    lo, hi = np.float32(p["lo"]), np.float32(p["hi"])
    rec[rec < lo] = lo
    rec[rec > hi] = hi
    return regularize(prob.vsize, rec, original, cm, p["delta"], p["alpha"], p["lam"], guide, delta_g, guide_only).astype(np.float32)


def superresolve(po, orc, prob, c, n, p, sw, guide=None, delta_g=1.0, guide_only=False, unit_on=None):
    """channel_sr_ref.superresolve with this module's update -> (volume, cover)"""
    vol, cover = sr.seed(po, orc, prob, c, sw, unit_on)
    for _ in range(n):
        sim, simw = sr.forward(po, orc, prob, vol)
        gate, e = sr.factors(prob, orc, c, sim, simw, unit_on)
        addon, cmap = sr.scatter(po, orc, prob, e, gate, sw)
        vol = update(po, prob, vol, addon, cmap, p, guide, delta_g, guide_only)
    return np.where(cover, vol, np.float32(0)).astype(np.float32), cover


# ---- a guide for the one-iteration tests -----------------------------------------------------------------------------------------------------
def smooth_guide_with_a_step(prob, seed=3):
    """a random smooth field (a few low-frequency waves, amplitude ~ 100) plus a step of 400 across an oblique plane"""
    vx, vy, vz = prob.vsize
    rng = np.random.default_rng(seed)
    kk, jj, ii = np.meshgrid(np.arange(vz), np.arange(vy), np.arange(vx), indexing="ij")
    g = np.zeros((vz, vy, vx))
    for _ in range(4):
        w = rng.uniform(-0.35, 0.35, 3)
        g += rng.uniform(20, 50) * np.sin(w[0] * ii + w[1] * jj + w[2] * kk + rng.uniform(0, 6.28))
    d = (ii - (vx - 1) / 2.0) * 0.4 + (jj - (vy - 1) / 2.0) * 1.0 - (kk - (vz - 1) / 2.0) * 0.6
    return (300.0 + g + np.where(d < 0, 0.0, 400.0)).astype(np.float32).reshape(-1)


# ---- the noisy recovery case -----------------------------------------------------------------------------------------------------------------
# channel_sr_ref's recovery case (the 100 | 300 step seen through the tiny problem's slices, eight iterations, RMSE to the truth over cover eroded
# by two voxels, after the iterations over the average's) with Gaussian noise of sigma 40 from default_rng(11) on every channel pixel that has a
# value (sim-weight > 0), lambda_c = 0.05 (alpha = 1) and a guide of 200 | 800 across the same plane.  delta's "default" is the command line's rule
# on the noise-free channel's range (20.5: the range the noise adds says nothing about the edges); the clamp is the noisy channel's range widened
# by a tenth, as the command line would set it.
NOISE_SIGMA, NOISE_SEED, LAMBDA_C = 40.0, 11, 0.05
DELTA_WIDE, DELTA_G = 120.0, 20.0
# what the restatement reaches (tests/test_channel_guide.py::test_guided_recovery_on_the_oracle_leg recomputes them to 1e-3)
ORACLE_UNGUIDED_DEFAULT = 0.7222021669307954
ORACLE_UNGUIDED_WIDE = 0.7827430436155296
ORACLE_GUIDED = 0.5222018641163204
_CASE, _LEG = {}, {}


def step_guide(prob):
    return np.where(sr.step_truth(prob) < 200, np.float32(200), np.float32(800)).astype(np.float32)


def noisy_case(po, orc, prob, key="tiny"):
    """-> dict(c, truth, sw, guide, p_default, p_wide, vol0, cover): shared, computed once"""
    if key not in _CASE:
        c, truth, sw = sr.recovery_case(po, orc, prob)
        clean = sr.parameters(prob, orc, c, lam=LAMBDA_C)
        noise = np.random.default_rng(NOISE_SEED).normal(0.0, NOISE_SIGMA, c.shape).astype(np.float32)
        _, simw = sr.forward(po, orc, prob, truth)
        cn = np.where(simw > 0, c + noise, np.float32(0)).astype(np.float32)
        noisy = sr.parameters(prob, orc, cn, lam=LAMBDA_C)
        at = lambda delta: dict(adaptive=False, alpha=noisy["alpha"], lo=noisy["lo"], hi=noisy["hi"], delta=delta, lam=LAMBDA_C * delta * delta)
        vol0, cover = sr.seed(po, orc, prob, cn, sw)
        _CASE[key] = dict(c=cn, truth=truth, sw=sw, guide=step_guide(prob), p_default=at(clean["delta"]), p_wide=at(DELTA_WIDE), vol0=vol0, cover=cover)
    return _CASE[key]


def rmse_ratio(prob, case, vol):
    vx, vy, vz = prob.vsize
    inner = sr.erode(case["cover"].reshape(vz, vy, vx), 2).reshape(-1)
    assert inner.sum() > 500
    rm = lambda v: float(np.sqrt(np.mean((np.asarray(v)[inner].astype(np.float64) - case["truth"][inner]) ** 2)))
    return rm(vol) / rm(case["vol0"])


def oracle_leg(po, orc, prob, which, key="tiny"):
    """which: "default" | "wide" | "guided" -> the RMSE ratio of that run on the restatement, once per session"""
    if (key, which) not in _LEG:
        case = noisy_case(po, orc, prob, key)
        p = case["p_default"] if which == "default" else case["p_wide"]
        kw = dict(guide=case["guide"], delta_g=DELTA_G) if which == "guided" else {}
        vol, _ = superresolve(po, orc, prob, case["c"], sr.RECOVERY_ITERATIONS, p, case["sw"], **kw)
        _LEG[(key, which)] = rmse_ratio(prob, case, vol)
    return _LEG[(key, which)]
