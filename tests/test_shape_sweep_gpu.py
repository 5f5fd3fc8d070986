"""Shape sweeps of the kernels that choose their launch geometry from the data: k_regul_fused (tile, z-chunk, partial last
chunk, the mask-box shortcut), k_bias_field_lds (strip width, stencil fallback, per-slice half-widths), the NormaliseBias
LDS tail (x rows, y / z strip widths, fallback, the bias_mode 1 switch) and the per-slice EM reductions (chunks of
CHUNK_PIX pixels, more than 256 slices).  Each case derives its shape from tests/shape_select.py's restatement of the
host's selection and asserts, through the read-only options the library records, that it reached that branch."""
import numpy as np
import pytest

from tests import shape_select as S
from tests.util import rel_err

pytestmark = pytest.mark.gpu

SIGMA = 12.0


def _eye(n):
    return np.broadcast_to(np.eye(4, dtype=np.float32), (n, 4, 4)).copy()


def _ctx(vsize, vdim=(1.0, 1.0, 1.0), mask=None, sgrid=None, slice_dims=None, slices=None, bias=False, scales=None):
    """a context of any shape through the ABI: volume + mask, optionally a slice grid (sx, sy, ns) with identity matrices"""
    from fetalreconstruction_amd import engine as E
    rec = E.Reconstruction(0)
    vx, vy, vz = vsize
    rec.InitReconstructionVolume(vsize, vdim)
    rec.setMask(vsize, vdim, np.ones((vz, vy, vx), np.float32) if mask is None else mask, SIGMA)
    if sgrid is not None:
        sx, sy, ns = sgrid
        rec.initStorageVolumes((sx, sy, ns), (1.0, 1.0, 1.0))
        rec.FillSlices(slices, np.full(ns, sx, np.int32), np.full(ns, sy, np.int32))
        rec.setSliceDims(np.ones((ns, 3), np.float32) if slice_dims is None else slice_dims, 2.0)
        m = _eye(ns)
        rec.SetSliceMatrices(m, m, m, m, m, m, np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32))
        rec.UpdateScaleVector(np.ones(ns, np.float32) if scales is None else scales, np.ones(ns, np.float32))
    if bias:
        rec.set_flags(disable_bias_correction=False)
    return rec


# ================================ 1. the fused volume update ================================
def _reg_inputs(vsize, seed, adaptive):
    vx, vy, vz = vsize
    rng = np.random.default_rng(seed)
    orig = rng.uniform(20.0, 120.0, (vz, vy, vx)).astype(np.float32)
    addon = rng.normal(0.0, 30.0, (vz, vy, vx)).astype(np.float32)
    blob = rng.random((vz // 2 + 1, vy // 2 + 1, vx // 2 + 1)) < 0.25                 # zeros in 2 x 2 x 2 blobs ...
    zero = blob.repeat(2, 0).repeat(2, 1).repeat(2, 2)[:vz, :vy, :vx]
    zero = zero | (rng.random((vz, vy, vx)) < 0.08)                                   # ... and isolated voxels
    cmap = (rng.uniform(0.2, 3.0, (vz, vy, vx)) if adaptive else np.ones((vz, vy, vx))).astype(np.float32)
    cmap[zero] = 0
    return orig, addon, cmap


def _reg_args(orig, adaptive):
    # both clamps fire: min / max at the 25th / 60th percentile of orig + addon
    delta, alpha = 30.0, 1.0
    lam = 0.05 * delta * delta / alpha
    lo, hi = np.percentile(orig, 25), np.percentile(orig, 60)
    return (adaptive, alpha, float(lo), float(hi), delta, lam)


def _reg_update(rec, orig, addon, cmap, args, reg_mode=1, reg_tile=-1):
    from fetalreconstruction_amd import engine as E
    rec.set_option("reg_mode", reg_mode)
    rec.set_option("reg_tile", reg_tile)
    rec.debug_set(E.BUF_RECONSTRUCTED, orig.ravel())
    rec.debug_set(E.BUF_ADDON, addon.ravel())
    rec.debug_set(E.BUF_CONFIDENCE_MAP, cmap.ravel())
    rec.SuperresolutionUpdate(*args)
    return rec.syncCPU()


def _reg_oracle(vsize, orig, addon, cmap, args):
    import ctypes as C
    from oracle import pyoracle as po
    adaptive, alpha, lo, hi, delta, lam = args
    vx, vy, vz = vsize
    r, a, c = orig.ravel().copy(), addon.ravel().copy(), cmap.ravel().copy()
    o = r.copy()
    po.lib().orc_regularization_prep(vx, vy, vz, int(adaptive), C.c_float(alpha), C.c_float(lo), C.c_float(hi), po._p(r), po._p(a), po._p(c))
    po.lib().orc_regularization(vx, vy, vz, C.c_float(delta), C.c_float(alpha), C.c_float(lam), po._p(r), po._p(o), po._p(c))
    return r


def _reg_shapes():
    out = set()
    for t in (0, 1, 2):
        tw, th = S.REG_TILES[t]
        for vx in (1, tw - 1, tw, tw + 1, 2 * tw + 1):
            for vy, vz in zip((1, th - 1, th, th + 1), (5, 3, 9, 2)):
                out.add((vx, vy, vz))
    for vz in (1, 4):
        out.add((33, 9, vz))
    return sorted(out)


@pytest.mark.parametrize("adaptive", [False, True])
def test_regulariser_small_shapes_against_oracle_and_across_tiles(adaptive):
    """every reg_tile at volumes around each tile's width and height, z = 1 .. 9 (zc = 4; vz = 5 and 9 end on a one-plane
    chunk): the oracle to 1e-6 of its maximum, reg_mode 0 likewise, and the same bits from every tile"""
    shapes = _reg_shapes()
    rec = None
    for k, vs in enumerate(shapes):
        if rec is not None:
            rec.close()
        rec = _ctx(vs)
        orig, addon, cmap = _reg_inputs(vs, k, adaptive)
        args = _reg_args(orig + addon, adaptive)
        ref = _reg_oracle(vs, orig, addon, cmap, args)
        outs = {}
        for t in (-1, 0, 1, 2):
            outs[t] = _reg_update(rec, orig, addon, cmap, args, 1, t)
            zc, chunks = S.reg_chunking(vs[0], vs[1], vs[2], t)
            assert (rec.get_option("reg_zc"), rec.get_option("reg_chunks")) == (zc, chunks), (vs, t)
        mode0 = _reg_update(rec, orig, addon, cmap, args, 0)
        assert rel_err(outs[-1], ref) < 1e-6, (vs, rel_err(outs[-1], ref))
        assert rel_err(mode0, ref) < 1e-6, vs
        for t in (0, 1, 2):
            assert np.array_equal(outs[t], outs[-1]), (vs, t)
    rec.close()


@pytest.mark.parametrize("adaptive", [False, True])
def test_regulariser_medium_volume_with_partial_last_chunk(adaptive):
    """a volume whose z-chunk lies strictly between 4 and 32 and whose last chunk holds one plane (250 x 250 x 71: 256 tiles
    of 32 x 8, 128 of 64 x 8 or 32 x 16, zc 5, 15 chunks): every tile the same bits, against reg_mode 0"""
    vs = (250, 250, 71)
    rec = _ctx(vs)
    orig, addon, cmap = _reg_inputs(vs, 100, adaptive)
    args = _reg_args(orig + addon, adaptive)
    mode0 = _reg_update(rec, orig, addon, cmap, args, 0)
    first = None
    for t in (-1, 0, 1, 2):
        out = _reg_update(rec, orig, addon, cmap, args, 1, t)
        zc, chunks = S.reg_chunking(*vs, t)
        assert (rec.get_option("reg_zc"), rec.get_option("reg_chunks")) == (zc, chunks)
        assert 4 < zc < 32 and vs[2] % zc == 1                      # the last chunk holds one plane
        first = out if first is None else first
        assert np.array_equal(out, first), t
    assert rel_err(first, mode0) < 1e-6
    rec.close()


def _box_problem():
    from fetalreconstruction_amd import phantom
    return phantom.make_problem(2, (72, 40, 10), 1.0, 2.0, None, 1.0, 30.0, seed=5, orientations=("ax", "cor"), name="box")


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_mask_box_shortcut_changes_no_bits(d):
    """the mask replaced by a box whose faces sit at a tile / chunk boundary - 1, at it and + 1; the update with cmap straight
    from the scatter (tiles outside the box grown by one write zeros unread) against the same update with the shortcut off"""
    from fetalreconstruction_amd import engine as E
    P = _box_problem()
    vx, vy, vz = P.vsize
    for t in (0, 1, 2):
        tw, th = S.REG_TILES[t]
        zc, _ = S.reg_chunking(vx, vy, vz, t)
        # faces at a multiple of the tile / chunk - 1, at it, + 1, around the phantom's centre
        lo = [min(v - 1, s * max(1, 24 // s) + d) for v, s in ((vx, tw), (vy, th), (vz, zc))]
        hi = [min(v - 1, s * max(2, 40 // s) + d) for v, s in ((vx, tw), (vy, th), (vz, zc))]
        mask = np.zeros((vz, vy, vx), np.float32)
        mask[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = 1
        P.mask = mask
        rec = E.Reconstruction(0)
        E.sync_gpu(rec, P)
        rec.set_option("reg_tile", t)
        rec.UpdateScaleVector(np.ones(P.ns, np.float32), np.ones(P.ns, np.float32))
        rec.GaussianReconstruction()
        rec.SimulateSlices()
        rec.InitializeEMValues()
        for adaptive in (False, True):
            rec.SuperresolutionBackproject(np.ones(P.ns, np.float32))
            orig = rec.syncCPU()
            addon, cmap = rec.debug_get(E.BUF_ADDON), rec.debug_get(E.BUF_CONFIDENCE_MAP)
            assert np.all(cmap.reshape(vz, vy, vx)[mask == 0] == 0) and (cmap != 0).any()
            args = _reg_args(orig[orig > 0] + 0, adaptive)
            rec.SuperresolutionUpdate(*args)                       # shortcut on: cmap is the scatter's
            on = rec.syncCPU()
            assert rec.get_option("reg_zc") == zc
            rec.debug_set(E.BUF_RECONSTRUCTED, orig)
            rec.debug_set(E.BUF_ADDON, addon)
            rec.debug_set(E.BUF_CONFIDENCE_MAP, cmap)
            rec.SuperresolutionUpdate(*args)                       # shortcut off
            off = rec.syncCPU()
            assert (on != 0).any() and np.array_equal(on, off), (t, d, adaptive)
            rec.debug_set(E.BUF_RECONSTRUCTED, orig)
        rec.close()


# ================================ 2. CorrectBias ================================
def _bias_inputs(sgrid, seed, pad=0):
    sx, sy, ns = sgrid
    rng = np.random.default_rng(seed)
    slices = rng.uniform(5.0, 200.0, (ns, sy, sx)).astype(np.float32)
    if pad:
        slices[:, :, sx - pad:] = -1                     # padded slices: -1 beyond sizes_x / sizes_y
        slices[:, sy - pad:, :] = -1
    slices[rng.random(slices.shape) < 0.05] = -1
    scales = rng.uniform(0.8, 1.2, ns).astype(np.float32)
    weights = rng.uniform(0.0, 1.0, slices.shape).astype(np.float32)
    sims = (slices * scales[:, None, None] * rng.uniform(0.7, 1.3, slices.shape)).astype(np.float32)
    simw = rng.choice(np.array([0.0, 0.5, 0.99, 1.0], np.float32), slices.shape, p=[0.1, 0.1, 0.1, 0.7])
    bias = rng.normal(0.0, 0.05, slices.shape).astype(np.float32)
    if ns > 1:
        sims[0] = 0.5                                   # residual wr = 0 on a whole slice: the wr pass gives 0 (the quirk)
    bias[-1].flat[rng.integers(sx * sy)] = np.nan       # a NaN in the field (the last slice's mean follows it)
    return slices, scales, weights, sims, simw, bias


def _bias_run(rec, ins, mode):
    from fetalreconstruction_amd import engine as E
    slices, scales, weights, sims, simw, bias = ins
    rec.set_option("bias_mode", mode)
    for b, a in ((E.BUF_WEIGHTS, weights), (E.BUF_SIMSLICES, sims), (E.BUF_SIMWEIGHTS, simw), (E.BUF_BIAS, bias)):
        rec.debug_set(b, a)
    rec.CorrectBias(SIGMA, True)                         # global: no per-slice mean
    first = rec.debug_get(E.BUF_BIAS)
    bx = rec.get_option("bias_field_bx")
    rec.CorrectBias(SIGMA, False)                        # a second pass from a non-zero field, per-slice mean
    return first, rec.debug_get(E.BUF_BIAS), bx


def _bias_case(sgrid, dims=None, pad=0, seed=0, sigma_dim=1.0):
    sx, sy, ns = sgrid
    ins = _bias_inputs(sgrid, seed, pad)
    sd = np.tile(np.array([[sigma_dim, sigma_dim, 2.0]], np.float32), (ns, 1)) if dims is None else dims
    rec = _ctx((4, 4, 4), sgrid=sgrid, slices=ins[0], slice_dims=sd, scales=ins[1], bias=True)
    half = max(S.gauss_half(SIGMA, float(x)) for x in sd[:, 0])
    lds = _bias_run(rec, ins, 1)
    sten = _bias_run(rec, ins, 0)
    rec.close()
    assert lds[2] == S.bias_field_bx(sy, half), (sgrid, half, lds[2])
    assert sten[2] == 0
    assert np.array_equal(lds[0], sten[0], equal_nan=True), sgrid
    assert np.array_equal(lds[1], sten[1], equal_nan=True), sgrid
    assert np.isfinite(lds[0]).sum() == lds[0].size - 1 and np.isfinite(lds[1][:-1]).all()
    return ins, sd, lds


def test_correct_bias_strip_widths_and_fallback_are_the_stencils():
    """one sy on each side of every strip boundary at half 48 (64 | 32 | 16 | 8 | stencils), sx not a multiple of the strip"""
    half = S.gauss_half(SIGMA, 1.0)
    seen = set()
    for bx in (64, 32, 16, 8):
        m = S.bias_field_max_sy(bx, half)
        for sy in (m, m + 1):
            ins, sd, lds = _bias_case((bx + 5 if bx > 8 else 21, sy, 2), seed=sy)
            seen.add(lds[2])
    assert seen == {64, 32, 16, 8, 0}


def test_correct_bias_edge_shapes_are_the_stencils():
    """slices narrower than the half-width in x and in y, padded slices, half-widths that differ from slice to slice inside
    one launch, and a half-width beyond BIAS_HMAX (the stencils)"""
    _bias_case((5, 7, 3), seed=1)                                        # both axes shorter than half 48
    _bias_case((150, 9, 2), seed=2)
    _bias_case((9, 130, 2), seed=3)                                      # > 116 rows: strips of 32
    _bias_case((70, 60, 3), pad=13, seed=4)
    dims = np.array([[1.0, 1.0, 2.0], [0.75, 0.75, 2.0], [1.3, 1.3, 2.0], [2.6, 2.6, 2.0]], np.float32)
    ins, sd, lds = _bias_case((45, 100, 4), dims=dims, seed=5)          # halves 48, 64, 37, 18: the LDS sized for 64
    assert lds[2] == 64
    _, _, lds = _bias_case((40, 30, 2), seed=6, sigma_dim=0.04)         # half 1200 > BIAS_HMAX
    assert lds[2] == 0


def test_correct_bias_against_the_oracle_across_strips():
    import ctypes as C
    from oracle import pyoracle as po
    half = S.gauss_half(SIGMA, 1.0)
    dims = np.array([[1.0, 1.0, 2.0], [0.75, 0.75, 2.0], [1.3, 1.3, 2.0]], np.float32)
    for sgrid, d in (((37, 40, 3), dims), ((9, S.bias_field_max_sy(64, half) + 1, 3), None), ((11, 6, 3), dims)):
        ins, sd, lds = _bias_case(sgrid, dims=d, seed=sgrid[1])
        slices, scales, weights, sims, simw, bias = ins
        ob = bias.copy()
        wb, wr, buf = (np.zeros_like(bias) for _ in range(3))
        sx, sy, ns = sgrid
        po.lib().orc_correct_bias(sx, sy, ns, po._p(slices), po._p(ob), po._p(weights), po._p(simw), po._p(sims), po._p(scales),
                                  po._p(np.ascontiguousarray(sd, np.float32)), C.c_float(SIGMA), 1, po._p(wb), po._p(wr), po._p(buf))
        ok = np.isfinite(ob)
        assert np.array_equal(ok, np.isfinite(lds[0]))
        assert rel_err(lds[0][ok], ob[ok], floor=1.0) < 2e-5, sgrid


# ================================ 3. the NormaliseBias tail ================================
def _tail_inputs(vsize, seed, nan=False):
    vx, vy, vz = vsize
    rng = np.random.default_rng(seed)
    sh = (vz, vy, vx)
    field = rng.normal(0.0, 0.3, sh).astype(np.float32)
    volw = rng.uniform(0.5, 2.0, sh).astype(np.float32)
    volw[rng.random(sh) < 0.05] = 0                      # voxels of zero weight
    maskC = rng.uniform(0.2, 1.0, sh).astype(np.float32)
    maskC[rng.random(sh) < 0.05] = 0
    recon = rng.uniform(0.0, 100.0, sh).astype(np.float32)
    recon[rng.random(sh) < 0.05] = -1
    if nan:
        field.flat[rng.integers(field.size)] = np.nan
    return field, volw, maskC, recon


def _tail_run(rec, ins, mode):
    import ctypes as C
    from fetalreconstruction_amd import engine as E
    field, volw, maskC, recon = ins
    rec.set_option("bias_mode", mode)
    for b, a in ((E.BUF_BIAS_VOLUME, field), (E.BUF_VOL_WEIGHTS, volw), (E.BUF_SMOOTH_MASK, maskC), (E.BUF_RECONSTRUCTED, recon)):
        rec.debug_set(b, a.ravel())
    assert rec._lib.svr_normalise_bias_finish(rec._h, C.c_float(SIGMA)) == 0
    got = tuple(rec.get_option(k) for k in ("bias_tail_lds", "bias_tail_rows", "bias_tail_bxy", "bias_tail_bxz"))
    return rec.debug_get(E.BUF_BIAS_VOLUME), rec.syncCPU(), got


def _tail_case(vsize, vdim=(1.0, 1.0, 1.0), mode=2, seed=0, nan=False, ref=False):
    ins = _tail_inputs(vsize, seed, nan)
    rec = _ctx(vsize, vdim, bias=True)
    a = _tail_run(rec, ins, mode)
    b = _tail_run(rec, ins, 0)
    rec.close()
    assert a[2] == S.tail_choice(vsize, vdim, SIGMA, mode), (vsize, a[2])
    assert b[2] == (0, 0, 0, 0)
    assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True), vsize
    if ref:
        vx, vy, vz = vsize
        rb, rr = S.normalise_tail(*ins, SIGMA, vdim)
        assert rel_err(a[0].reshape(vz, vy, vx), rb) < 1e-5, vsize
        assert rel_err(a[1].reshape(vz, vy, vx), rr) < 1e-5, vsize
    return a[2]


def test_normalise_tail_launch_choices_are_the_stencils():
    """x rows 16 / 8 / 1 / none, y and z strips of 64 .. 4 on each side of every boundary and beyond the last (the stencils),
    x not a multiple of the strip, axes shorter than the half-width, anisotropic voxels; NaN-free cases also against float64"""
    seen_rows, seen_bxy, seen_bxz, fallback = set(), set(), set(), 0
    cases = []
    for r in (16, 1):
        m = S.tail_rows_max(r)
        cases += [(m, 3, 2), (m + 1, 2, 2)]
    for b in (64, 32, 16, 8, 4):
        m = S.tail_strip_max(b)
        cases += [(37, m, 2), (37, m + 1, 2), (21, 2, m), (21, 2, m + 1)]
    for k, vs in enumerate(sorted(set(cases))):
        vdim = (1.0, 0.8, 2.5) if k % 3 == 0 else (1.0, 1.0, 1.0)
        got = _tail_case(vs, vdim, seed=k, nan=k % 4 == 1, ref=k % 4 != 1 and np.prod(vs) < 400_000)
        if got[0]:
            seen_rows.add(got[1]); seen_bxy.add(got[2]); seen_bxz.add(got[3])
        else:
            fallback += 1
    assert {16, 8, 1} <= seen_rows and {64, 32, 16, 8, 4} <= seen_bxy and {64, 32, 16, 8, 4} <= seen_bxz and fallback >= 3


def test_normalise_tail_switch_at_bias_lds_tail_min():
    """bias_mode 1: one volume just under BIAS_LDS_TAIL_MIN voxels (the stencils), one at it (the LDS tail), both the stencils' bits"""
    under = (256, 128, 127)
    at = (256, 128, 128)
    assert np.prod(under) < S.BIAS_LDS_TAIL_MIN == np.prod(at)
    assert _tail_case(under, mode=1, seed=1, nan=True)[0] == 0
    assert _tail_case(at, mode=1, seed=2, nan=True)[0] == 1


# ================================ 4. the per-slice EM reductions ================================
def _em_inputs(sgrid, seed, pad=0):
    sx, sy, ns = sgrid
    rng = np.random.default_rng(seed)
    sh = (ns, sy, sx)
    slices = rng.uniform(0.0, 150.0, sh).astype(np.float32)
    slices[rng.random(sh) < 0.1] = -1
    if pad:
        slices[:, :, sx - pad:] = -1
    if ns >= 3:
        slices[0] = -1                                    # a slice with no valid pixel: scale 1
    sims = (slices * rng.uniform(0.8, 1.2, sh)).astype(np.float32)
    simw = rng.choice(np.array([0.0, 0.3, 0.99, 1.0], np.float32), sh, p=[0.1, 0.1, 0.2, 0.6])   # 0.99f: > 0.99 in double only
    if ns >= 3:
        simw[1] = np.minimum(simw[1], np.float32(0.5))    # a slice with no simweights > 0.99 pixel: potential -1
    weights = rng.uniform(0.0, 1.0, sh).astype(np.float32)
    inside = (rng.random(sh) < 0.8).astype(np.uint8)
    scales = rng.uniform(0.8, 1.2, ns).astype(np.float32)
    slicew = rng.uniform(0.5, 1.0, ns).astype(np.float32)
    return slices, sims, simw, weights, inside, scales, slicew


def _em_ctx(ins, sgrid, bias=None):
    from fetalreconstruction_amd import engine as E
    slices, sims, simw, weights, inside, scales, slicew = ins
    rec = _ctx((4, 4, 4), sgrid=sgrid, slices=slices, scales=scales, bias=bias is not None)
    rec.UpdateScaleVector(scales, slicew)
    for b, a in ((E.BUF_SIMSLICES, sims), (E.BUF_SIMWEIGHTS, simw), (E.BUF_WEIGHTS, weights), (E.BUF_SIMINSIDE, inside)):
        rec.debug_set(b, a)
    if bias is not None:
        rec.debug_set(E.BUF_BIAS, bias)
    return rec


def _ulp_diff(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


EM_GRIDS = [((23, 89), 1), ((64, 32), 255), ((683, 3), 256), ((63, 65), 257), ((17, 241), 513), ((5, 1229), 3),
            ((64, 32), 2), ((2049, 1), 257)]


@pytest.mark.parametrize("grid,ns", EM_GRIDS)
def test_em_reductions_against_float64(grid, ns):
    """sx sy in {2047, 2048, 2049, 4095, 4097, 6145} pixels (one to four CHUNK_PIX blocks, a last block of one pixel), ns across
    k_reduce_slices' 256-thread stride; a slice with no valid pixel and one with no simweights > 0.99"""
    from fetalreconstruction_amd import engine as E
    sx, sy = grid
    sgrid = (sx, sy, ns)
    ins = _em_inputs(sgrid, sx * 7 + ns, pad=3 if ns == 2 else 0)
    slices, sims, simw, weights, inside, scales, slicew = ins
    rec = _em_ctx(ins, sgrid)
    assert S.em_chunks(sx, sy) == -(-(sx * sy) // 2048)
    ms = rec.MStepSums()
    ref = S.mstep_sums(slices, weights, sims, simw, scales)
    assert ms[2] == ref[2] and ms[3] == ref[3] and ms[4] == ref[4], (ms, ref)
    assert np.allclose(ms[:2], ref[:2], rtol=1e-10, atol=0), (ms, ref)
    rs = rec.RobustStatisticsSums()
    rref = S.robust_sums(slices, inside, sims, simw)
    assert rs[1] == rref[1] and np.allclose(rs[0], rref[0], rtol=1e-10, atol=0)
    vs = rec.ScaleVolumeSums()
    assert np.allclose(vs, S.scalevol_sums(slices, weights, sims, simw, slicew), rtol=1e-10, atol=0)
    sc = rec.CalculateScaleVector()
    sref = S.scale_vector(slices, weights, sims, simw)
    assert (ns < 3 or sc[0] == 1.0) and (_ulp_diff(sc, sref) <= 1).all(), np.max(_ulp_diff(sc, sref))
    rec.UpdateScaleVector(scales, slicew)                 # (CalculateScaleVector moved the device's scales along)
    m, sigma, mix = 1.0 / 160.0, 150.0, 0.85
    pot = rec.EStep(m, sigma, mix)
    w_ref, p_ref = S.estep(slices, sims, simw, scales, m, sigma, mix)
    w = rec.debug_get(E.BUF_WEIGHTS)
    assert (_ulp_diff(w, w_ref) <= 4).all(), np.max(_ulp_diff(w, w_ref))
    assert ns < 3 or (pot[0] == 1 and pot[1] == -1)
    assert np.allclose(pot, p_ref, rtol=1e-6, atol=0)
    rec.close()


def test_em_reductions_with_bias_against_float64():
    """bias on: the device's expf(-bias) in every term, rtol 1e-6"""
    from fetalreconstruction_amd import engine as E
    sgrid = (63, 65, 257)
    ins = _em_inputs(sgrid, 5)
    slices, sims, simw, weights, inside, scales, slicew = ins
    bias = np.random.default_rng(6).normal(0.0, 0.1, slices.shape).astype(np.float32)
    rec = _em_ctx(ins, sgrid, bias)
    ms = rec.MStepSums()
    ref = S.mstep_sums(slices, weights, sims, simw, scales, bias)
    assert ms[2] == ref[2] and np.allclose(ms, ref, rtol=1e-6, atol=0), (ms, ref)
    sc = rec.CalculateScaleVector()
    assert np.allclose(sc, S.scale_vector(slices, weights, sims, simw, bias), rtol=1e-6, atol=0)
    rec.UpdateScaleVector(scales, slicew)
    pot = rec.EStep(1.0 / 160.0, 150.0, 0.85)
    w_ref, p_ref = S.estep(slices, sims, simw, scales, 1.0 / 160.0, 150.0, 0.85, bias)
    assert np.allclose(rec.debug_get(E.BUF_WEIGHTS), w_ref, rtol=0, atol=1e-5)   # one ulp of expf(-bias) moves e by ~1e-5: weights in [0, 1]
    assert np.allclose(pot, p_ref, rtol=1e-6, atol=0)
    rec.close()
