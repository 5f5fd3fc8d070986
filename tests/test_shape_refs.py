"""CPU legs of the shape sweeps (tests/test_shape_sweep_gpu.py): the selection formulas of tests/shape_select.py reproduce the
boundaries worked out by hand from the host code, and its numpy references of the NormaliseBias tail and the per-slice EM
reductions agree with the C oracle, so that a sweep failure points at a kernel and not at the test's reference."""
import ctypes as C

import numpy as np
import pytest

from tests import shape_select as S


def test_selection_boundaries_at_half_48():
    half = S.gauss_half(12.0, 1.0)
    assert half == 48
    assert [S.bias_field_max_sy(b, half) for b in (64, 32, 16, 8)] == [116, 220, 392, 592]
    for b, m in zip((64, 32, 16, 8), (116, 220, 392, 592)):
        assert S.bias_field_bx(m, half) == b and S.bias_field_bx(m + 1, half) == (b // 2 if b > 8 else 0)
    assert S.bias_field_bx(10, 256) == 0 and S.bias_field_bx(10, 255) == 64       # BIAS_HMAX
    assert S.gauss_half(12.0, 0.75) == 64 and S.gauss_half(12.0, 0.04) > S.BIAS_HMAX


def test_tail_boundaries():
    assert S.tail_rows_max(16) == 1008 and S.tail_rows(1008) == 16 and S.tail_rows(1009) == 8
    assert S.tail_rows(16128) == 1 and S.tail_rows(16129) == 0
    assert [S.tail_strip_max(b) for b in (64, 32, 16, 8, 4)] == [252, 504, 1008, 2016, 4032]
    for b, m in zip((64, 32, 16, 8, 4), (252, 504, 1008, 2016, 4032)):
        assert S.tail_strip(m) == b and S.tail_strip(m + 1) == (b // 2 if b > 4 else 0)
    one = (1.0, 1.0, 1.0)
    assert S.tail_choice((256, 128, 127), one, 12.0, 1) == (0, 0, 0, 0)                # under BIAS_LDS_TAIL_MIN: the stencils
    assert S.tail_choice((256, 128, 128), one, 12.0, 1) == (1, 16, 64, 64)
    assert S.tail_choice((37, 4033, 2), one, 12.0, 2) == (0, 0, 0, 0)
    assert S.tail_choice((37, 2, 2), (1.0, 1.0, 0.04), 12.0, 2) == (0, 0, 0, 0)        # half > BIAS_HMAX on one axis


def test_regulariser_chunking():
    assert S.reg_chunking(250, 250, 71, -1) == (5, 15)                                  # 256 tiles of 32 x 8
    assert S.reg_chunking(250, 250, 71, 0) == (5, 15) and S.reg_chunking(250, 250, 71, 1) == (5, 15)
    for t in (-1, 0, 1, 2):
        assert S.reg_chunking(33, 9, 5, t) == (4, 2)                                   # small volumes: zc = 4, a one-plane last chunk
        assert S.reg_chunking(1, 1, 1, t) == (4, 1)
    assert S.reg_chunking(32 * 64, 8 * 64, 33, 2) == (32, 2)


def test_em_chunks():
    assert [S.em_chunks(sx, sy) for sx, sy in ((23, 89), (64, 32), (683, 3), (63, 65), (17, 241), (5, 1229))] == [1, 1, 2, 2, 3, 4]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("vsize,vdim", [((19, 7, 5), (1.0, 1.0, 1.0)), ((40, 33, 9), (1.0, 0.8, 2.5)), ((3, 60, 2), (0.9, 1.0, 1.0))])
def test_smoothing_reference_is_the_oracle(oracle_mod, vsize, vdim):
    """shape_select.smooth3d (float64, the kernels' float32 weights, clamped borders) against the oracle's X -> Y -> Z passes
    (orc_smooth_mask: the same passes NormaliseBias runs after its division by the weights), axes shorter than the half-width
    included"""
    vx, vy, vz = vsize
    a = np.random.default_rng(vx).normal(0.0, 1.0, (vz, vy, vx)).astype(np.float32)
    out = np.zeros_like(a)
    dim = np.array(vdim, np.float32)
    oracle_mod.lib().orc_smooth_mask(vx, vy, vz, _p(dim), _p(a), C.c_float(12.0), _p(out))
    ref = S.smooth3d(a, 12.0, vdim)
    assert np.max(np.abs(out - ref)) <= 2e-6 * np.max(np.abs(ref))


def _em_data(sx, sy, ns, seed):
    rng = np.random.default_rng(seed)
    sh = (ns, sy, sx)
    slices = rng.uniform(0.0, 150.0, sh).astype(np.float32)
    slices[rng.random(sh) < 0.1] = -1
    slices[0] = -1
    sims = (slices * rng.uniform(0.8, 1.2, sh)).astype(np.float32)
    simw = rng.choice(np.array([0.0, 0.3, 0.99, 1.0], np.float32), sh, p=[0.1, 0.1, 0.2, 0.6])
    simw[1] = np.minimum(simw[1], np.float32(0.5))
    weights = rng.uniform(0.0, 1.0, sh).astype(np.float32)
    inside = (rng.random(sh) < 0.8).astype(np.uint8)
    scales = rng.uniform(0.8, 1.2, ns).astype(np.float32)
    slicew = rng.uniform(0.5, 1.0, ns).astype(np.float32)
    bias = rng.normal(0.0, 0.1, sh).astype(np.float32)
    return slices, sims, simw, weights, inside, scales, slicew, bias


def _ulp(a, b):
    ia, ib = np.asarray(a, np.float32).view(np.int32).astype(np.int64), np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(np.where(ia < 0, -(ia & 0x7FFFFFFF), ia) - np.where(ib < 0, -(ib & 0x7FFFFFFF), ib))


def test_em_references_are_the_oracle(oracle_mod):
    L = oracle_mod.lib()
    sx, sy, ns = 45, 50, 5
    slices, sims, simw, weights, inside, scales, slicew, bias = _em_data(sx, sy, ns, 3)
    for b in (None, bias):
        o5 = np.zeros(5)
        L.orc_mstep_sums(sx, sy, ns, _p(slices), _p(weights), _p(sims), _p(simw), _p(scales), _p(o5), None if b is None else _p(b))
        ref = S.mstep_sums(slices, weights, sims, simw, scales, b)
        assert o5[2] == ref[2]
        if b is None:
            assert o5[3] == ref[3] and o5[4] == ref[4] and np.allclose(o5[:2], ref[:2], rtol=1e-12, atol=0)
        else:
            assert np.allclose(o5, ref, rtol=1e-6, atol=0)
        sc = np.zeros(ns, np.float32)
        L.orc_calculate_scale_vector(sx, sy, ns, _p(slices), _p(weights), _p(sims), _p(simw), _p(sc), None if b is None else _p(b))
        sref = S.scale_vector(slices, weights, sims, simw, b)
        assert sc[0] == 1.0 and (_ulp(sc, sref) <= (1 if b is None else 4)).all()
        w = np.zeros_like(slices)
        pot = np.zeros(ns, np.float32)
        L.orc_estep(sx, sy, ns, _p(slices), _p(sims), _p(simw), _p(scales), C.c_float(1 / 160.0), C.c_float(150.0), C.c_float(0.85),
                    _p(w), _p(pot), None if b is None else _p(b))
        w_ref, p_ref = S.estep(slices, sims, simw, scales, 1 / 160.0, 150.0, 0.85, b)
        if b is None:
            assert (_ulp(w, w_ref) <= 4).all()
        else:                                            # one ulp of expf(-bias) moves e by ~1e-5: weights in [0, 1]
            assert np.allclose(w, w_ref, rtol=0, atol=1e-5)
        assert pot[1] == -1 and pot[0] == 1
        assert np.allclose(pot, p_ref, rtol=1e-6, atol=0)
    sa, sb = C.c_double(0), C.c_double(0)
    L.orc_initialize_robust_statistics.restype = C.c_float
    L.orc_initialize_robust_statistics(C.c_size_t(slices.size), _p(slices), _p(inside), _p(sims), _p(simw), C.byref(sa), C.byref(sb))
    rs = S.robust_sums(slices, inside, sims, simw)
    assert sb.value == rs[1] and np.isclose(sa.value, rs[0], rtol=1e-12, atol=0)
    recon = np.ones(8, np.float32)
    L.orc_scale_volume.restype = C.c_float
    scale = L.orc_scale_volume(sx, sy, ns, _p(slices), _p(weights), _p(sims), _p(simw), _p(slicew), C.c_size_t(8), _p(recon))
    num, den = S.scalevol_sums(slices, weights, sims, simw, slicew)
    assert scale == np.float32(num / den)
