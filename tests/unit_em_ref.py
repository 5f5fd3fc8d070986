"""The unit-level EM of csrc/svr_em.inc restated in numpy, operation by operation: no engine, no GPU.

The library is built with -ffp-contract=off -fno-fast-math, so k_slice_em's sums are plain IEEE double additions in a fixed order
(thread t adds the units t, t + 256, .. of the visit order, then the halving tree o = 128 .. 1) and can be written down bit for bit.
Every array is in the HOST numbering, as the device holds them; by_ref[k] is the host index of the unit with reference index k: the
order the sums visit the units in.  The expression types are the kernel's (and the oracle's, oracle/svr_oracle.c orc_host_estep):
`pot * w` is a float product widened to double, `pot * (1.0 - w)` a double product, the variance terms are float throughout.

  unit_em        one pass: (pot_out, w_out, state5_out), sums `serial` (the reference's) or `tree256` (k_slice_em's)
  class_scalars, unit_weights, unit_mix   its three parts, for a caller that evaluates the weights with scalars of its own
  unpack         the ranks' [world][3][maxn] floats -> the global raw potentials, scales, inside flags
  mstep_scalars  mstep_scalars of csrc/svr_hip.hip in float32;  combine_ranks  k_mstep_scalars_ranks' sums over the ranks
"""
import math

import numpy as np

F32 = np.float32
F64 = np.float64
FLT_MAX = F32(3.402823466e+38)
FLT_MIN = F32(1.175494351e-38)


# ---- sums in a fixed order ---------------------------------------------------------------------------------------------------
def sum_serial(terms, take):
    """0.0 + the terms that take part, one after the other"""
    t = np.asarray(terms, F64)[np.asarray(take, bool)]
    return F64(np.add.accumulate(t)[-1]) if t.size else F64(0.0)


def sum_tree256(terms, take):
    """k_slice_em's: thread t adds the terms t, t + 256, .. that take part, in order, from 0.0; then block_reduce256's tree"""
    terms, take = np.asarray(terms, F64), np.asarray(take, bool)
    n = terms.size
    rows = -(-n // 256) if n else 0
    v = np.zeros(rows * 256, F64)
    m = np.zeros(rows * 256, bool)
    v[:n], m[:n] = terms, take
    v, m = v.reshape(rows, 256), m.reshape(rows, 256)
    acc = np.zeros(256, F64)
    for r in range(rows):
        acc = np.where(m[r], acc + v[r], acc)
    o = 128
    while o > 0:
        acc[:o] = acc[:o] + acc[o:2 * o]
        o >>= 1
    return F64(acc[0])


SUMS = {"serial": sum_serial, "tree256": sum_tree256}


# ---- the two forms' Gaussians ------------------------------------------------------------------------------------------------
def gauss_slice(x, s, step):
    """SliceGauss: double, from the float difference x and the float variance s"""
    x, s = float(F32(x)), float(F32(s))
    if s == 0.0 or s != s:
        with np.errstate(all="ignore"):
            return float(F64(step) * np.exp(F64(-x * x) / F64(2 * s)) / np.sqrt(F64(6.28 * s)))
    a = -x * x / (2 * s)
    return step * (math.exp(a) if a > -800.0 else 0.0) / math.sqrt(6.28 * s)


def gauss_patch32(x, s):
    """PatchGauss: float32 throughout, the literal 0.00001f"""
    x, s = F32(x), F32(s)
    with np.errstate(all="ignore"):
        return float(F32(0.00001) * np.exp(-x * x / (F32(2.0) * s)) / np.sqrt(F32(6.28) * s))


def gauss_patch64(x, s):
    """PatchGauss evaluated in float64 from the same float32 x, s and the same float32 constants"""
    x, s = float(F32(x)), float(F32(s))
    a = -x * x / (2.0 * s)
    return float(F32(0.00001)) * (math.exp(a) if a > -800.0 else 0.0) / math.sqrt(float(F32(6.28)) * s)


def var_floor(form, step):
    if form == "patch":
        return F64(F32(step) * F32(step)) / F64(6.28)
    return F64(step) * F64(step) / F64(6.28)


# ---- the EM's parts ----------------------------------------------------------------------------------------------------------
def apply_exclusions(raw, scale, excluded, src=None):
    """raw potentials [through src, -1 -> 0] -> -1 where excluded or the scale is outside [0.2, 5] (float against double constants)"""
    raw = np.asarray(raw, F32)
    pot = raw.copy()
    if src is not None:
        src = np.asarray(src)
        pot = np.where(src >= 0, raw[np.maximum(src, 0)], F32(0)).astype(F32)
    sc = np.asarray(scale, F32).astype(F64)
    pot[np.asarray(excluded) != 0] = -1
    pot[(sc < 0.2) | (sc > 5)] = -1
    return pot


def class_scalars(pot, w, by_ref, form, step, order, by_ref2=None):
    """the two passes over the units in the visit order -> (mean_s, mean_s2, sigma_s, sigma_s2 as float32, den, sums) where sums
    holds the eight double sums (for comparing the two orders).  by_ref2: another visit order for the second pass (what a kernel
    that forgot by_ref there would add; for the cases that must tell)"""
    add = SUMS[order]
    pot, w = np.asarray(pot, F32), np.asarray(w, F32)
    pot2, w2 = (pot, w) if by_ref2 is None else (pot[by_ref2], w[by_ref2])
    p, w = pot[by_ref], w[by_ref]
    take = p >= 0
    pd, wd = p.astype(F64), w.astype(F64)
    t_sum, t_den = (p * w).astype(F64), wd                    # float product, widened
    t_sum2, t_den2 = pd * (1.0 - wd), 1.0 - wd                # double
    s_sum, den, sum2, den2 = add(t_sum, take), add(t_den, take), add(t_sum2, take), add(t_den2, take)
    maxs = max(0.0, float(pd[take].max())) if take.any() else 0.0
    mins = min(1.0, float(pd[take].min())) if take.any() else 1.0
    with np.errstate(all="ignore"):
        mean_s = F32(s_sum / den) if den > 0 else F32(mins)
        mean_s2 = F32(sum2 / den2) if den2 > 0 else F32((maxs + F64(mean_s)) / 2.0)
        if by_ref2 is not None:
            p, w = pot2, w2
            take, wd = p >= 0, w.astype(F64)
        v1 = ((p - mean_s) * (p - mean_s) * w).astype(F64)    # float throughout
        v2 = ((p - mean_s2) * (p - mean_s2) * (F32(1) - w)).astype(F64)
        d2 = (F32(1) - w).astype(F64)
    vsum, vden, vsum2, vden2 = add(v1, take), add(wd, take), add(v2, take), add(d2, take)
    floor_ = var_floor(form, step)
    if vsum > 0 and vden > 0:
        sigma_s = F32(vsum / vden)
        if F64(sigma_s) < floor_:
            sigma_s = F32(floor_)
    else:
        sigma_s = F32(0.025)
    if vsum2 > 0 and vden2 > 0:
        sigma_s2 = F32(vsum2 / vden2)
    else:
        with np.errstate(all="ignore"):
            sigma_s2 = F32((mean_s2 - mean_s) * (mean_s2 - mean_s) / F32(4))
    if F64(sigma_s2) < floor_:
        sigma_s2 = F32(floor_)
    sums = dict(sum=s_sum, den=den, sum2=sum2, den2=den2, vsum=vsum, vden=vden, vsum2=vsum2, vden2=vden2,
                terms=dict(sum=(t_sum, take), den=(t_den, take), sum2=(t_sum2, take), den2=(t_den2, take), vsum=(v1, take),
                           vden=(wd, take), vsum2=(v2, take), vden2=(d2, take)))
    return mean_s, mean_s2, sigma_s, sigma_s2, vden, sums


def unit_weights(pot, w, mean_s, mean_s2, sigma_s, sigma_s2, mix_s, den, form, step, gauss="f32"):
    """the weight loop with the given scalars (float32).  Patch form: gauss = "f32" (the restatement proper) or "f64" (the
    high-precision reference).  -> (weights float32, exponent arguments [n][2] with nan where a Gaussian is not evaluated, and
    `exact` [n]: the weight is a branch's 0 or 1, not a quotient)"""
    pot, out = np.asarray(pot, F32), np.asarray(w, F32).copy()
    mean_s, mean_s2, sigma_s, sigma_s2, mix_s = F32(mean_s), F32(mean_s2), F32(sigma_s), F32(sigma_s2), F32(mix_s)
    args = np.full((len(pot), 2), np.nan)
    exact = np.ones(len(pot), bool)
    one_class = den <= 0 or mean_s2 <= mean_s
    if form == "slice":
        g = lambda x, s: gauss_slice(x, s, step)   # noqa: E731
    else:
        g = gauss_patch32 if gauss == "f32" else gauss_patch64
    mix, mix1 = float(mix_s), float(F32(1) - mix_s)
    for i, p in enumerate(pot):
        if p == -1:
            out[i] = 0
            continue
        if one_class:
            out[i] = 1
            continue
        gs1 = gs2 = 0.0
        with np.errstate(all="ignore"):
            if p < mean_s2:
                x = F32(p - mean_s)
                gs1 = g(x, sigma_s)
                args[i, 0] = float(x) * float(x) / (2.0 * float(sigma_s))
            if p > mean_s:
                x = F32(p - mean_s2)
                gs2 = g(x, sigma_s2)
                args[i, 1] = float(x) * float(x) / (2.0 * float(sigma_s2))
        likelihood = gs1 * mix + gs2 * mix1
        if likelihood > 0:
            out[i] = F32(gs1 * mix / likelihood)
            exact[i] = gs1 == 0 or gs2 * mix1 == 0                   # 0 / x and x / x
        else:
            if p <= mean_s:
                out[i] = 1
            if p >= mean_s2:
                out[i] = 0
            if p < mean_s2 and p > mean_s:
                out[i] = 1
    return out, args, exact


def unit_mix(pot, w, by_ref, order):
    """the mixing proportion: the sum in the visit order, the count in any; 0.9f when nothing takes part"""
    p, wv = np.asarray(pot, F32)[by_ref], np.asarray(w, F32)[by_ref]
    take = p >= 0
    num = int(take.sum())
    return F32(SUMS[order](wv.astype(F64), take) / F64(num)) if num > 0 else F32(0.9)


def unit_em(pot, w, scale, excluded, step, state5, form, order, by_ref=None, src=None, gauss="f32"):
    """One pass of k_slice_em after its unpack: pot = the raw potentials as the ranks sent them, w = the weights before, state5 =
    {mean_s, mean_s2, sigma_s, sigma_s2, mix_s} before (only mix_s is read).  src (patch form, host numbering): the unit whose raw
    potential unit g reads, -1 = none.  -> (pot_out, w_out, state5_out as float32)"""
    n = len(pot)
    by_ref = np.arange(n) if by_ref is None else np.asarray(by_ref)
    p = apply_exclusions(pot, scale, excluded, src if form == "patch" else None)
    mean_s, mean_s2, sigma_s, sigma_s2, den, _ = class_scalars(p, w, by_ref, form, step, order)
    wn, _, _ = unit_weights(p, w, mean_s, mean_s2, sigma_s, sigma_s2, F32(state5[4]), den, form, step, gauss)
    return p, wn, np.array([mean_s, mean_s2, sigma_s, sigma_s2, unit_mix(p, wn, by_ref, order)], F32)


# ---- numberings --------------------------------------------------------------------------------------------------------------
def order_of(by_ref):
    """svr_slice_em_setup's `order` (order[k] = the reference index of host unit k) for a given by_ref"""
    by_ref = np.asarray(by_ref)
    order = np.empty(len(by_ref), np.int32)
    order[by_ref] = np.arange(len(by_ref), dtype=np.int32)
    return order


def stack_potential_sources(counts):
    """csrc/svr_unit_em.h: stack k's potentials land on the indices 0 .. counts[k]-1 (no stack offset), the later stacks win; in the
    REFERENCE's numbering, -1 = none"""
    src = np.full(int(sum(counts)), -1, np.int32)
    ofs = 0
    for c in counts:
        src[:c] = ofs + np.arange(c)
        ofs += c
    return src


def src_host(src_ref, by_ref):
    """svr_slice_em_set_patch_form: the reference-numbered map in the host numbering, src[by_ref[t]] = by_ref[src_ref[t]]"""
    src_ref, by_ref = np.asarray(src_ref), np.asarray(by_ref)
    out = np.full(len(src_ref), -1, np.int32)
    for t, u in enumerate(src_ref):
        out[by_ref[t]] = -1 if u < 0 else by_ref[u]
    return out


# ---- the exchange's layout ---------------------------------------------------------------------------------------------------
def pack(raw, scale, inside, world, rlo, maxn):
    """global vectors -> the [world][3][maxn] floats the ranks' all-gather leaves, zeros behind each rank's count"""
    recv = np.zeros((world, 3, maxn), F32)
    for r in range(world):
        lo, hi = rlo[r], rlo[r + 1]
        for k, v in enumerate((raw, scale, inside)):
            recv[r, k, :hi - lo] = np.asarray(v, F32)[lo:hi]
    return recv.reshape(-1)


def unpack(recv, world, rlo, maxn, ns):
    """k_slice_em's first loop, with its walk over the ranks (an empty range is walked over) -> raw, scale, inside"""
    recv = np.asarray(recv, F32).reshape(-1)
    out = np.zeros((3, ns), F32)
    for g in range(ns):
        r = 0
        while r + 1 < world and g >= rlo[r + 1]:
            r += 1
        base = r * 3 * maxn + (g - rlo[r])
        out[:, g] = recv[base], recv[base + maxn], recv[base + 2 * maxn]
    return out[0], out[1], out[2]


def max_count(rlo):
    return max(1, max(int(rlo[r + 1]) - int(rlo[r]) for r in range(len(rlo) - 1)))


# ---- the M-step's scalars ----------------------------------------------------------------------------------------------------
def mstep_scalars(s5, iter, step, pvr, sigma, mix):
    """mstep_scalars of csrc/svr_hip.hip in float32 -> (sigma, mix, m)"""
    with np.errstate(all="ignore"):
        s_sigma, s_mix, s_num = F32(s5[0]), F32(s5[1]), F32(s5[2])
        mn, mx = F32(s5[3]), F32(s5[4])
        sigma, mix, step = F32(sigma), F32(mix), F32(step)
        if not pvr:                                                # slices only: std::min(FLT_MAX, .), std::max(FLT_MIN, .)
            mn = mn if mn < FLT_MAX else FLT_MAX
            mx = mx if FLT_MIN < mx else FLT_MIN
        if s_mix > 0:
            sigma = F32(s_sigma / s_mix)
        floor_ = F32(F32(step * step) / F32(6.28))
        if sigma < floor_:
            sigma = floor_
        if iter > 1:
            mix = F32(s_mix / s_num)
        m = F32(F32(1.0) / F32(mx - mn))
    return sigma, mix, m


def combine_ranks(all8, world):
    """k_mstep_scalars_ranks / k_mstep_scalars_dev: three sums from 0.0 in rank order, fmin / fmax of the extremes"""
    a = np.asarray(all8, F64).reshape(world, 8)
    s5 = np.zeros(5, F64)
    for r in range(world):
        for k in range(3):
            s5[k] = s5[k] + a[r, k]
        s5[3] = np.fmin(s5[3], a[r, 3]) if r else a[0, 3]
        s5[4] = np.fmax(s5[4], a[r, 4]) if r else a[0, 4]
    return s5


def ulp_diff(a, b):
    """distance in float32 ulps (the integer distance of the bit patterns, sign-magnitude unfolded)"""
    a, b = np.atleast_1d(np.asarray(a, F32)), np.atleast_1d(np.asarray(b, F32))
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)
