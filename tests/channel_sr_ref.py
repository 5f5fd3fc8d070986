"""Shared by tests/test_channel_sr.py and tests/test_channel_sr_gpu.py: the SR iterations on a channel (svr_channel_sr_*, csrc/svr_channel.inc;
--channelIterations of csrc/svr_cli.cpp) restated on the oracle library, stage by stage, and the recovery case both legs run.

The oracle's functions are called, not changed:
  forward   orc_simulate_slices on the channel volume (the primary's pixel set: slice != -1, v_PSF_sums != 0)
  factors   numpy: gate = P and sim-weight > 0, e = c - sim, f1 = weights * slice_weights / v_PSF_sums
  scatter   orc_superresolution_backproject fed with e: slices' = e / k with scales = k (k a power of two: the product is e exactly), a
            simulated slice of the smallest positive float (the oracle's gate `ss > 0` is open, e - ss is e to within 1.4e-45), and -1 --
            no pixel -- where the gate is shut.  k is the first of 2, 4, .. 2^15 for which no open pixel's e / k is -1.
  update    orc_regularization_prep with an unbounded range (its clamp, 0.9 min / 1.1 max, presumes positive intensities), the clamp
            [lo, hi] in numpy on the float32 values, orc_regularization
"""
import ctypes as C

import numpy as np

TINY = np.float32(1e-45)          # the smallest positive float32


def pixel_set(prob, orc, unit_on=None):
    """P of svr_channel_scatter: primary slice pixel != -1, v_PSF_sums != 0, the slice switched on"""
    on = np.ones(prob.ns, bool) if unit_on is None else np.asarray(unit_on) != 0
    return (prob.slices != -1) & (orc.psf_sums != 0) & on[:, None, None]


def f1_of(orc, sw):
    with np.errstate(divide="ignore", invalid="ignore"):
        f = (orc.weights * np.asarray(sw, np.float32)[:, None, None]) / orc.psf_sums
    return np.where(orc.psf_sums != 0, f, 0).astype(np.float32)


def forward(po, orc, prob, vol):
    """-> (sim, sim-weight) of the volume on the slice grid, 0 where the pass writes nothing"""
    shp = prob.slices.shape
    sim, simw = np.zeros(shp, np.float32), np.zeros(shp, np.float32)
    inside, sl_inside = np.zeros(shp, np.uint8), np.zeros(prob.ns, np.uint8)
    v = po._f32(vol).reshape(-1)
    po.lib().orc_simulate_slices(C.byref(orc.g), po._p(orc.slices), po._p(orc.psf_sums), po._p(v), po._p(orc.mask), po._p(sim), po._p(simw),
                                 po._p(inside), po._p(sl_inside))
    return sim, simw


def scatter(po, orc, prob, e, gate, sw):
    """sum coeff f1 e | sum coeff f1 over the gated pixels -> (addon, cmap)"""
    e = np.asarray(e, np.float32)
    for k in 2.0 ** np.arange(1, 16):
        s2 = (e / np.float32(k)).astype(np.float32)
        if not (gate & (s2 == -1)).any():
            break
    else:
        raise AssertionError("no power of two keeps e / k off -1")
    s2 = np.where(gate, s2, np.float32(-1)).astype(np.float32)
    sim = np.full(prob.slices.shape, TINY, np.float32)
    assert sim.min() > 0
    scales = np.full(prob.ns, k, np.float32)
    nv = prob.nvox
    pair = np.zeros(2 * nv, np.float32)
    addon, cmap = pair[:nv], pair[nv:]
    po.lib().orc_superresolution_backproject(C.byref(orc.g), po._p(s2), po._p(orc.weights), po._p(sim), po._p(po._f32(sw)), po._p(scales), po._p(orc.mask),
                                             po._p(orc.psf_sums), po._p(addon), po._p(cmap))
    return addon, cmap


def seed(po, orc, prob, c, sw, unit_on=None):
    """C0 = num / den where den > 0, else 0; cover = den > 0 (svr_channel_scatter + svr_channel_finish with background 0)"""
    P = pixel_set(prob, orc, unit_on)
    num, den = scatter(po, orc, prob, c, P, sw)
    with np.errstate(divide="ignore", invalid="ignore"):
        c0 = np.where(den > 0, num / den, np.float32(0)).astype(np.float32)
    return c0, den > 0


def factors(prob, orc, c, sim, simw, unit_on=None):
    """-> (gate, e): mode 4 of k_cell_factors"""
    gate = pixel_set(prob, orc, unit_on) & (simw > 0)
    e = np.where(gate, np.asarray(c, np.float32) - sim, np.float32(0)).astype(np.float32)
    return gate, e


def update(po, prob, vol, addon, cmap, p):
    """the SR volume update on (vol, addon, cmap); p = dict(adaptive, alpha, lo, hi, delta, lam): lam is the engine's (lambda delta^2)"""
    vx, vy, vz = prob.vsize
    rec, ad, cm = po._f32(vol).reshape(-1).copy(), po._f32(addon).copy(), po._f32(cmap).copy()
    original = rec.copy()
    po.lib().orc_regularization_prep(vx, vy, vz, int(bool(p["adaptive"])), C.c_float(p["alpha"]), C.c_float(-np.inf), C.c_float(np.inf), po._p(rec), po._p(ad),
                                     po._p(cm))
    lo, hi = np.float32(p["lo"]), np.float32(p["hi"])
    rec[rec < lo] = lo
    rec[rec > hi] = hi
    po.lib().orc_regularization(vx, vy, vz, C.c_float(p["delta"]), C.c_float(p["alpha"]), C.c_float(p["lam"]), po._p(rec), po._p(original), po._p(cm))
    return rec


def parameters(prob, orc, c, unit_on=None, delta=150.0, lam=0.01, adaptive=False):
    """The command line's defaults: delta_c = delta R_c / R_s, lambda_c = lam (--lastIterLambda's default), alpha = min(1, 0.05 / lambda_c), the
    clamp [c_min - 0.1 R_c, c_max + 0.1 R_c]; R_c over P, R_s the problem's intensity range"""
    P = pixel_set(prob, orc, unit_on)
    c_min, c_max = float(np.asarray(c)[P].min()), float(np.asarray(c)[P].max())
    R_c, R_s = c_max - c_min, float(prob.max_intensity) - float(prob.min_intensity)
    delta_c = delta * R_c / R_s
    return dict(adaptive=adaptive, alpha=min(1.0, 0.05 / lam), lo=c_min - 0.1 * R_c, hi=c_max + 0.1 * R_c, delta=delta_c, lam=lam * delta_c * delta_c)


def residual(orc, sw, gate, e):
    """sum f1 e^2 over the gated pixels, in double"""
    f1 = f1_of(orc, sw).astype(np.float64)
    return float((f1[gate] * e[gate].astype(np.float64) ** 2).sum())


def superresolve(po, orc, prob, c, n, p, sw, unit_on=None, seed_volume=None):
    """The whole call: seed, n iterations, 0 outside cover -> (volume, cover, [weighted residual before every iteration])"""
    vol, cover = seed(po, orc, prob, c, sw, unit_on)
    if seed_volume is not None:
        vol = po._f32(seed_volume).reshape(-1).copy()
    res = []
    for _ in range(n):
        sim, simw = forward(po, orc, prob, vol)
        gate, e = factors(prob, orc, c, sim, simw, unit_on)
        res.append(residual(orc, sw, gate, e))
        addon, cmap = scatter(po, orc, prob, e, gate, sw)
        vol = update(po, prob, vol, addon, cmap, p)
    vol = np.where(cover, vol, np.float32(0)).astype(np.float32)
    return vol, cover, res


# ---- the recovery case -----------------------------------------------------------------------------------------------------------------------
def erode(mask3, n):
    """n erosions with the 6-neighbourhood; the volume's border counts as outside"""
    m = np.asarray(mask3, bool)
    for _ in range(n):
        p = np.pad(m, 1, constant_values=False)
        m = (p[1:-1, 1:-1, 1:-1] & p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1] & p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:])
    return m


def step_truth(prob):
    """100 | 300 across an oblique plane through the volume's centre"""
    vx, vy, vz = prob.vsize
    kk, jj, ii = np.meshgrid(np.arange(vz), np.arange(vy), np.arange(vx), indexing="ij")
    n = np.array([1.0, 0.5, 0.3])
    d = (ii - (vx - 1) / 2.0) * n[0] + (jj - (vy - 1) / 2.0) * n[1] + (kk - (vz - 1) / 2.0) * n[2]
    return np.where(d < 0, np.float32(100), np.float32(300)).astype(np.float32).reshape(-1)


def recovery_case(po, orc, prob):
    """-> (channel = the forward projection of the truth with the problem's transformations, truth, slice weights)"""
    truth = step_truth(prob)
    sim, simw = forward(po, orc, prob, truth)
    return np.where(simw > 0, sim, np.float32(0)).astype(np.float32), truth, orc.slice_weights.copy()


def recovery_figures(prob, c, truth, vol0, vol, cover, res0, res):
    """-> (RMSE ratio, residual ratio): after the iterations over before, RMSE to the truth over cover eroded by two voxels"""
    vx, vy, vz = prob.vsize
    inner = erode(cover.reshape(vz, vy, vx), 2).reshape(-1)
    assert inner.sum() > 500
    rm = lambda v: float(np.sqrt(np.mean((v[inner].astype(np.float64) - truth[inner]) ** 2)))
    return rm(vol) / rm(vol0), res / res0


RECOVERY_ITERATIONS = 8
# what the oracle reaches on the tiny problem (tests/test_channel_sr.py::test_recovery_on_the_oracle recomputes them): the RMSE to
# the truth and the weighted residual after eight iterations over those of the average.  The yardstick of the device's leg
ORACLE_RMSE_RATIO = 0.5912259995298687
ORACLE_RESIDUAL_RATIO = 0.027905957703330243
_ORACLE_RECOVERY = {}


def oracle_recovery(po, orc, prob, key):
    """the recovery case on the oracle, once per session and problem -> dict(c, truth, sw, p, vol0, vol, cover, res0, res, rmse_ratio, res_ratio)"""
    if key not in _ORACLE_RECOVERY:
        c, truth, sw = recovery_case(po, orc, prob)
        p = parameters(prob, orc, c)
        vol0, cover, _ = superresolve(po, orc, prob, c, 0, p, sw)
        vol, _, res = superresolve(po, orc, prob, c, RECOVERY_ITERATIONS, p, sw)
        res_end = final_residual(po, orc, prob, c, vol, sw)
        rr, qq = recovery_figures(prob, c, truth, vol0, vol, cover, res[0], res_end)
        _ORACLE_RECOVERY[key] = dict(c=c, truth=truth, sw=sw, p=p, vol0=vol0, vol=vol, cover=cover, res0=res[0], res=res_end, rmse_ratio=rr, res_ratio=qq)
    return _ORACLE_RECOVERY[key]


def final_residual(po, orc, prob, c, vol, sw, unit_on=None):
    """the weighted residual of a finished volume (its forward projection against the channel)"""
    sim, simw = forward(po, orc, prob, vol)
    gate, e = factors(prob, orc, c, sim, simw, unit_on)
    return residual(orc, sw, gate, e)
