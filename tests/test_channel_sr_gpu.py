"""SR iterations on a channel on the device (csrc/svr_channel.inc: svr_channel_sr_begin / _seed / _backproject / _update / _end, factor
mode 4 of k_cell_factors) and from the command line (--channelIterations).

Tolerances, stated once (none is new):
  * addon | cmap of an iteration against the oracle's scatter: the project's TOL_SUM (2e-5 of the buffer's maximum, tests/test_parity_gpu.py);
    the sets where they are non-zero exactly.
  * the updated volume against the oracle's update of the SAME inputs (the device's seed and the device's addon | cmap): row a7's 1e-6 of the
    volume's maximum (tests/test_parity_gpu.py::test_regulariser_parity).  The stages are compared one by one, each fed what the device fed
    its own, as the suite compares the primary's.
  * against the primary SR iteration, between two calls, with the table on and off, and everything the call must leave alone: bit patterns.
  * recovery: no worse than the oracle's two ratios (tests/channel_sr_ref.py) by more than 5 % -- the two legs differ by float
    effects of order 1e-5, so 5 % only guards against a wrong sign, gate or step.
  * two ranks against one: what tests/test_channel_gpu.py::test_cli_two_ranks_on_one_device demands of the average, 2e-5 of the maximum.
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

from fetalreconstruction_amd import build
from tests import channel_ref as ref
from tests import channel_sr_ref as sr
from tests.test_channel_gpu import _channel, _engine_at_scale, _num_den, _problem, _state
from tests.util import _snap, rel_err

pytestmark = pytest.mark.gpu

TOL_SUM = 2e-5          # tests/test_parity_gpu.py
TOL_A7 = 1e-6           # row a7: the fused volume update against the oracle's, of the volume's maximum


def _switches(prob, orc, switch):
    """switch: unit_on switches one whole slice off and another slice's weight is 0 (tests/test_channel_gpu.py's pair)"""
    sw = orc.slice_weights.copy()
    if not switch:
        return sw, None
    live = [s for s in range(prob.ns) if (orc.psf_sums[s] != 0).any() and sw[s] > 0]
    sw[live[len(live) // 3]] = 0
    unit_on = np.ones(prob.ns, np.uint8)
    unit_on[live[len(live) // 2]] = 0
    return sw, unit_on


def _quot(num, den):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, num / den, np.float32(0)).astype(np.float32)


def _one_iteration(rec, c, unit_on, sw, p, seed=None):
    """begin .. end with one iteration -> (num, den of the seed scatter, addon, cmap of the iteration, the volume)"""
    rec.channel_sr_begin(c, unit_on=unit_on, slice_weights=sw)
    num, den = _num_den(rec)
    rec.channel_sr_seed(seed)
    rec.channel_sr_backproject()
    addon, cmap = _num_den(rec)
    rec.channel_sr_update(p["adaptive"], p["alpha"], p["lo"], p["hi"], p["delta"], p["lam"])
    return num, den, addon, cmap, rec.channel_sr_end()


@pytest.mark.parametrize("name,switch", [("tiny", False), ("tiny", True), ("awkward", False), ("awkward", True)])
def test_one_iteration_against_the_restatement(tiny, oracle_mod, name, switch):
    prob, rec, orc = _state(name, tiny, oracle_mod)
    c = _channel(prob, 1) + np.float32(1)                    # positive integers
    sw, unit_on = _switches(prob, orc, switch)
    p = sr.parameters(prob, orc, c, unit_on)
    rec.channel_scatter(c, unit_on=unit_on, slice_weights=sw)
    plain = _num_den(rec)
    num, den, addon, cmap, vol = _one_iteration(rec, c, unit_on, sw, p)
    rec.UpdateSliceWeights(orc.slice_weights)
    assert np.array_equal(num.view(np.uint32), plain[0].view(np.uint32)) and np.array_equal(den.view(np.uint32), plain[1].view(np.uint32))   # begin is svr_channel_scatter
    cover = den > 0
    c0 = _quot(num, den)
    sim, simw = sr.forward(oracle_mod, orc, prob, c0)
    gate, e = sr.factors(prob, orc, c, sim, simw, unit_on)
    oaddon, ocmap = sr.scatter(oracle_mod, orc, prob, e, gate, sw)
    ovol = np.where(cover, sr.update(oracle_mod, prob, c0, addon, cmap, p), np.float32(0))
    ea, ec, ev = rel_err(addon, oaddon), rel_err(cmap, ocmap), rel_err(vol, ovol)
    print(name, switch, "covered", int(cover.sum()), "rel_err addon", ea, "cmap", ec, "volume", ev, "moved by", rel_err(vol, c0))
    assert cover.sum() > 1000 and (ocmap > 0).sum() > 1000
    assert np.array_equal(addon != 0, oaddon != 0) and np.array_equal(cmap != 0, ocmap != 0)
    assert ea < TOL_SUM and ec < TOL_SUM
    assert ev <= TOL_A7
    assert not vol[~cover].any() and rel_err(vol, c0) > 1e-3                 # outside cover 0; the iteration did something
    if switch:
        assert not np.array_equal(ocmap, sr.scatter(oracle_mod, orc, prob, e, gate, orc.slice_weights)[1])


@pytest.mark.parametrize("name", ["tiny", "awkward"])
def test_same_bits_as_the_primary_sr_iteration(tiny, name):
    """State "scale", no bias field, a positive volume V0, the channel = the float product slices * scale: the channel's iteration from the
    seed V0 is the primary's SR iteration, bit for bit on cover (0.9 min / 1.1 max handed over as the clamp)."""
    from fetalreconstruction_amd import engine as E
    prob = _problem(name, tiny)
    rec, d = _engine_at_scale(prob)
    v0 = (np.abs(rec.syncCPU()) + np.float32(1)).astype(np.float32)
    scales = np.linspace(0.9, 1.1, prob.ns).astype(np.float32)
    sw = np.asarray(d._slice_weight_gpu, np.float32).copy()
    rec.UpdateScaleVector(scales, sw)
    rec.UpdateReconstructed(prob.vsize, v0)
    rec.SimulateSlices()
    ss, simw, psf = rec.debug_get(E.BUF_SIMSLICES), rec.debug_get(E.BUF_SIMWEIGHTS), rec.debug_get(E.BUF_PSF_SUMS)
    P = ((prob.slices != -1) & (psf.reshape(prob.slices.shape) != 0)).reshape(-1)
    assert P.sum() > 1000 and np.array_equal((ss.reshape(-1) > 0)[P], (simw.reshape(-1) > 0)[P])       # the two gates coincide on the one pixel set
    c = (prob.slices * scales[:, None, None]).astype(np.float32)
    alpha, delta, lam = d._alpha, d._delta, d._lambda
    mn, mx = np.float32(d._min_intensity), np.float32(d._max_intensity)
    rec.Superresolution(1, sw, False, alpha, float(mn), float(mx), delta, lam)
    v1 = rec.syncCPU()
    p = dict(adaptive=False, alpha=alpha, lo=float(np.float32(np.float64(mn) * 0.9)), hi=float(np.float32(np.float64(mx) * 1.1)), delta=delta, lam=lam)
    num, den, addon, cmap, vol = _one_iteration(rec, c, None, sw, p, seed=v0)
    cover = den > 0
    print(name, "cover", int(cover.sum()), "differing voxels on cover", int((vol[cover].view(np.uint32) != v1[cover].view(np.uint32)).sum()))
    assert cover.sum() > 1000 and rel_err(v1, v0) > 1e-3
    assert np.array_equal(vol[cover].view(np.uint32), v1[cover].view(np.uint32))
    assert np.array_equal(rec.syncCPU().view(np.uint32), v1.view(np.uint32))                          # the reconstruction was not touched
    rec.close()


@pytest.mark.parametrize("name", ["tiny", "awkward"])
def test_a_channel_with_zeros_and_negative_values(tiny, oracle_mod, name):
    """The integers minus 100.  addon | cmap of one back-projection against the oracle's SR scatter fed with e directly, through
    tests/test_channel_gpu.py's device: slices' = e + 256 (-1 where the gate is shut), scales 1, simulated slices 256."""
    po = oracle_mod
    prob, rec, orc = _state(name, tiny, oracle_mod)
    c = _channel(prob, 1) - np.float32(100)
    sw = orc.slice_weights.copy()
    rec.channel_sr_begin(c, slice_weights=sw)
    num, den = _num_den(rec)
    rec.channel_sr_seed()
    rec.channel_sr_backproject()
    addon, cmap = _num_den(rec)
    rec.channel_sr_end(want_volume=False)
    c0 = _quot(num, den)
    sim, simw = sr.forward(po, orc, prob, c0)
    gate, e = sr.factors(prob, orc, c, sim, simw)
    neg = gate & (sim <= 0)
    assert neg.any() and (e[neg] != 0).any() and (orc.weights[neg] > 0).any()        # a pixel with sim <= 0 and sim-weight > 0 contributes
    s2 = np.where(gate, e + np.float32(256), np.float32(-1)).astype(np.float32)
    s256, one = np.full(prob.slices.shape, 256, np.float32), np.ones(prob.ns, np.float32)
    pair = np.zeros(2 * prob.nvox, np.float32)
    oaddon, ocmap = pair[:prob.nvox], pair[prob.nvox:]
    po.lib().orc_superresolution_backproject(C.byref(orc.g), po._p(s2), po._p(orc.weights), po._p(s256), po._p(po._f32(sw)), po._p(one), po._p(orc.mask),
                                             po._p(orc.psf_sums), po._p(oaddon), po._p(ocmap))
    print(name, "pixels with sim <= 0 behind an open gate", int(neg.sum()), "rel_err addon", rel_err(addon, oaddon), "cmap", rel_err(cmap, ocmap))
    assert np.array_equal(cmap != 0, ocmap != 0)
    assert rel_err(addon, oaddon) < TOL_SUM and rel_err(cmap, ocmap) < TOL_SUM
    # the sign of the simulated value did not shut the gate: with `sim > 0` as the gate those pixels' weights would be missing from cmap
    g_sign = gate & (sim > 0)
    assert rel_err(cmap, sr.scatter(po, orc, prob, e, g_sign, sw)[1]) > TOL_SUM


def _iterate(rec, c, p, n=2):
    rec.channel_sr_begin(c)
    rec.channel_sr_seed()
    for _ in range(n):
        rec.channel_sr_backproject()
        rec.channel_sr_update(p["adaptive"], p["alpha"], p["lo"], p["hi"], p["delta"], p["lam"])
    return rec.channel_sr_end()


def test_repeats_bit_for_bit_and_leaves_the_run_alone():
    from fetalreconstruction_amd import engine as E
    prob = ref.awkward_problem()
    c = _channel(prob, 4) - np.float32(50)
    R_c = 255.0
    p = dict(adaptive=False, alpha=1.0, lo=-50 - 0.1 * R_c, hi=205 + 0.1 * R_c, delta=30.0, lam=0.01 * 30.0 * 30.0)
    engines = []
    for _ in range(2):                                       # the second one never sees the call
        rec, d = _engine_at_scale(prob)
        d.SuperresolutionGPU(1); d.SimulateSlicesGPU(); d.MStepGPU(1); d.EStepGPU(); d.ScaleGPU()
        engines.append((rec, d))
    (rec, d), (rec2, d2) = engines
    bufs = (E.BUF_RECONSTRUCTED, E.BUF_SIMSLICES, E.BUF_SIMWEIGHTS, E.BUF_SIMINSIDE, E.BUF_WEIGHTS, E.BUF_PSF_SUMS)

    def snapshot(r, dd):
        s = {b: r.debug_get(b).copy() for b in bufs}
        s["scale"] = np.asarray(r.GetScaleVector()).copy()
        s["driver"] = {k: v for k, (kind, v) in _snap(dd).items()}     # the slice weights, the scale vector's host copy and the EM scalars
        return s
    before = snapshot(rec, d)
    assert rec.get_option("coeff_table") == 1 and rec.get_option("coeff_valid") == 1
    v1 = _iterate(rec, c, p)
    assert rec.get_option("coeff_table") == 1 and rec.get_option("coeff_valid") == 1      # the table is still there and valid
    v2 = _iterate(rec, c, p)
    rec.set_option("coeff_table", 0)
    fly = _iterate(rec, c, p)
    rec.set_option("coeff_table", 1)
    assert np.abs(v1).max() > 0 and np.array_equal(v1.view(np.uint32), v2.view(np.uint32)) and np.array_equal(v1.view(np.uint32), fly.view(np.uint32))
    fb = rec.fallbacks()
    assert fb["scatter_to_atomics"] == 0 and fb["gather_to_tiles"] == 0
    after = snapshot(rec, d)
    for b in bufs:
        assert np.array_equal(before[b].view(np.uint8), after[b].view(np.uint8)), b
    assert np.array_equal(before["scale"], after["scale"])
    for k, v in before["driver"].items():
        assert np.array_equal(np.asarray(v), np.asarray(after["driver"][k])), k
    rec2.set_option("coeff_table", 0); rec2.set_option("coeff_table", 1)     # (the twin's table goes through the same off / on)
    for dd in (d, d2):
        dd.SuperresolutionGPU(2)
    assert np.array_equal(rec.syncCPU().view(np.uint32), rec2.syncCPU().view(np.uint32))
    for dd in (d, d2):
        dd.SimulateSlicesGPU()
    assert np.array_equal(rec.debug_get(E.BUF_SIMSLICES), rec2.debug_get(E.BUF_SIMSLICES))
    rec.close(); rec2.close()


def test_recovery_on_the_device(tiny, oracle_mod):
    """tests/test_channel_sr.py's recovery case: both ratios no worse than the oracle's recorded ones by more than 5 %."""
    po = oracle_mod
    prob, rec, orc = _state("tiny", tiny, oracle_mod)
    c, truth, sw = sr.recovery_case(po, orc, prob)
    p = sr.parameters(prob, orc, c)
    rec.channel_scatter(c, slice_weights=sw)
    den = _num_den(rec)[1]
    vol0 = rec.channel_finish(background=0.0)
    cover = den > 0
    rec.channel_sr_begin(c, slice_weights=sw)
    rec.channel_sr_seed()
    for _ in range(sr.RECOVERY_ITERATIONS):
        rec.channel_sr_backproject()
        rec.channel_sr_update(p["adaptive"], p["alpha"], p["lo"], p["hi"], p["delta"], p["lam"])
    vol = rec.channel_sr_end()
    res0, res = sr.final_residual(po, orc, prob, c, vol0, sw), sr.final_residual(po, orc, prob, c, vol, sw)
    rr, qq = sr.recovery_figures(prob, c, truth, vol0, vol, cover, res0, res)
    print("device recovery: RMSE ratio %.9g (oracle %.9g), weighted residual ratio %.9g (oracle %.9g)" % (rr, sr.ORACLE_RMSE_RATIO, qq, sr.ORACLE_RESIDUAL_RATIO))
    assert rr < 1.0 and qq < 1.0
    assert rr <= 1.05 * sr.ORACLE_RMSE_RATIO and qq <= 1.05 * sr.ORACLE_RESIDUAL_RATIO


def test_refusals_are_errors_and_the_context_goes_on(tiny):
    from fetalreconstruction_amd import engine as E
    c = _channel(tiny, 9)
    fresh = E.Reconstruction(0)
    E.sync_gpu(fresh, tiny)
    with pytest.raises(E.SvrError, match="EM weights"):      # missing state
        fresh.channel_sr_begin(c)
    fresh.close()
    rec, _ = _engine_at_scale(tiny)
    rec.channel_scatter(c)
    usual = _num_den(rec)
    ok = dict(adaptive=False, alpha=1.0, lo=0.0, hi=300.0, delta=20.0, lam=4.0)

    def upd(**kw):
        q = {**ok, **kw}
        rec.channel_sr_update(q["adaptive"], q["alpha"], q["lo"], q["hi"], q["delta"], q["lam"])
    for call, word in ((lambda: rec.channel_sr_end(), "svr_channel_sr_begin first"), (lambda: rec.channel_sr_seed(), "svr_channel_sr_begin first"),
                       (lambda: rec.channel_sr_backproject(), "svr_channel_sr_seed first"), (upd, "svr_channel_sr_backproject first")):
        with pytest.raises(E.SvrError, match=word):          # out of order, nothing in flight
            call()
    with pytest.raises(E.SvrError, match="no channel"):
        rec.channel_sr_begin(None)
    with pytest.raises(E.SvrError, match="label indicators"):
        rec.channel_sr_begin(c, flags=E.CHANNEL_INDICATOR)
    with pytest.raises(E.SvrError, match="unknown flag"):
        rec.channel_sr_begin(c, flags=4)
    rec.set_option("back_mode", 4)                           # the atomic scatters: no channel path
    with pytest.raises(E.SvrError, match="no fallback"):
        rec.channel_sr_begin(c)
    rec.set_option("back_mode", 5)
    rec.channel_sr_begin(c)
    with pytest.raises(E.SvrError, match="in flight"):       # begin twice
        rec.channel_sr_begin(c)
    with pytest.raises(E.SvrError, match="svr_channel_sr_seed first"):
        rec.channel_sr_backproject()
    rec.channel_sr_seed()
    with pytest.raises(E.SvrError, match="one seed per call"):
        rec.channel_sr_seed()
    with pytest.raises(E.SvrError, match="svr_channel_sr_backproject first"):   # update before backproject
        upd()
    rec.channel_sr_backproject()
    with pytest.raises(E.SvrError, match="svr_channel_sr_update after"):
        rec.channel_sr_backproject()
    for kw in (dict(delta=0.0), dict(delta=-1.0), dict(delta=float("nan")), dict(delta=float("inf")), dict(lam=0.0), dict(lam=float("nan")), dict(lam=float("inf"))):
        with pytest.raises(E.SvrError, match="finite and positive"):
            upd(**kw)
    with pytest.raises(E.SvrError, match="lo <= hi"):
        upd(lo=5.0, hi=4.0)
    with pytest.raises(E.SvrError, match="lo <= hi"):
        upd(lo=float("nan"))
    upd()                                                    # a refused update left the call where it was
    vol = rec.channel_sr_end()
    assert np.isfinite(vol).all() and np.abs(vol).max() > 0
    with pytest.raises(E.SvrError, match="svr_channel_sr_begin first"):
        rec.channel_sr_end()
    rec.channel_scatter(c)                                   # ... and a plain scatter gives its usual bits
    again = _num_den(rec)
    assert np.array_equal(usual[0].view(np.uint32), again[0].view(np.uint32)) and np.array_equal(usual[1].view(np.uint32), again[1].view(np.uint32))
    rec.close()
    pv = E.Reconstruction(0)
    pv.set_option("pvr", 1)
    pv.sgrid = tiny.slices.shape
    with pytest.raises(E.SvrError, match="pvr"):
        pv.channel_sr_begin(c)
    pv.close()


def test_refused_beyond_the_cell_lists_limit():
    """a geometry the cell lists cannot hold (tests/cell_limit_cases.py): refused with a message, nothing in flight afterwards"""
    from fetalreconstruction_amd import engine as E
    from tests import cell_limit_cases as L
    from tests.test_cell_limits_gpu import _engine, _sequence
    case = L.build("centres-x-beyond")
    rec = _engine(case)
    _sequence(rec, case)
    with pytest.raises(E.SvrError, match="cannot hold this geometry"):
        rec.channel_sr_begin(np.ones(case.problem.slices.shape, np.float32))
    with pytest.raises(E.SvrError, match="svr_channel_sr_begin first"):
        rec.channel_sr_end()
    rec.close()


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def _cli(args):
    return subprocess.run(["timeout", "-k", "10", "240", build.CLI, *args], capture_output=True, text=True)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """plain | the channel's average (no option) | --channelIterations 0 | 4 iterations on a ramp | 4 on a constant | the ramp on two ranks"""
    from fetalreconstruction_amd import nifti
    build.build()
    d = tmp_path_factory.mktemp("channel_sr")
    args, paths, stacks = ref.write_cli_case(d)
    err = {}

    def go(name, extra):
        r = _cli(["-o", str(d / f"{name}.nii.gz"), *args, *extra])
        assert r.returncode == 0, r.stderr[-3000:]
        err[name] = r.stderr
    ramp = ref.write_like(d, "ramp", stacks, lambda k, st: 50.0 + 2.0 * ref.pixel_world(st.attr)[..., 0] - 1.0 * ref.pixel_world(st.attr)[..., 2])
    eight = ref.write_like(d, "eight", stacks, lambda k, st: np.full(st.data.shape, 8.0))
    ch = lambda files, out: ["--channelStacks", *files, "--channelOutput", str(d / out)]
    go("plain", [])
    go("avg", ch(ramp, "c_avg.nii.gz"))
    go("zero", [*ch(ramp, "c_zero.nii.gz"), "--channelIterations", "0"])
    go("four", [*ch(ramp, "c_four.nii.gz"), "--channelIterations", "4"])
    go("const", [*ch(eight, "c_const.nii.gz"), "--channelIterations", "4"])
    go("two", [*ch(ramp, "c_two.nii.gz"), "--channelIterations", "4", "-d", "0", "0"])
    return d, err


def _vol(d, name):
    from fetalreconstruction_amd import nifti
    return nifti.read(d / name)[0]


def test_cli_without_iterations_nothing_changes(runs):
    """no option and --channelIterations 0: the same bytes (the parent commit's file is the no-option one: that path is not touched)"""
    d, err = runs
    assert (d / "c_avg.nii.gz").read_bytes() == (d / "c_zero.nii.gz").read_bytes()
    assert "--channelIterations" not in err["avg"] and "--channelIterations" not in err["zero"]


def test_cli_primary_volume_is_unchanged(runs):
    d, err = runs
    plain = (d / "plain.nii.gz").read_bytes()
    for name in ("avg", "zero", "four", "const", "two"):
        if name != "two":                                    # (two ranks sum in another order: not a statement about the channel)
            assert (d / f"{name}.nii.gz").read_bytes() == plain, name
    assert "--channelIterations 4: delta" in err["four"] and "alpha" in err["four"] and "channel range [" in err["four"]


def test_cli_iterations_change_the_channel_and_keep_its_cover(runs):
    d, err = runs
    a, f = _vol(d, "c_avg.nii.gz"), _vol(d, "c_four.nii.gz")
    assert np.array_equal(a != 0, f != 0) and rel_err(f, a) > 1e-4
    assert np.isfinite(f).all()


def test_cli_constant_channel_stays_constant(runs):
    """a constant channel: within 1e-5 of its value on the cover eroded by two voxels (in fact nothing runs: R_c = 0 returns the average)"""
    d, err = runs
    v = _vol(d, "c_const.nii.gz")
    inner = sr.erode(v != 0, 2)
    assert inner.sum() > 500 and np.abs(v[inner] - 8.0).max() <= 1e-5
    assert "constant channel" in err["const"]


def test_cli_two_ranks_on_one_device(runs):
    d, err = runs
    assert "2 ranks" in err["two"]
    c1, c2 = _vol(d, "c_four.nii.gz"), _vol(d, "c_two.nii.gz")
    assert np.array_equal(c1 != 0, c2 != 0)
    print("two ranks against one: channel after 4 iterations", rel_err(c2, c1))
    assert rel_err(c2, c1) < 2e-5
