"""The cell lists (csrc/svr_cell.inc) at their layout limits, and the tile kernels they fall back onto beyond them (cells_or_fallback,
csrc/svr_hip.hip), on the geometries of tests/cell_limit_cases.py: a `beyond` case has to leave the cell path audibly (svr_fallbacks) and
still agree with the oracle on back_mode 4's atomics, fwd_unit_kernel and the tile form of pass 1; its `inside` twin has to stay on the
cell path, agree with the oracle and repeat bit for bit.  Tolerances are those of tests/test_parity_gpu.py / tests/test_fuzz_gpu.py."""
import os

import numpy as np
import pytest

from tests import cell_limit_cases as C
from tests.util import rel_err

pytestmark = pytest.mark.gpu
TOL = 2e-5
# SVR_CELL_LIMIT_ORACLE=1: case 4 (16 k pixels of one slice in one cell) against the oracle too -- several seconds of CPU per case
RUN_ORACLE = os.environ.get("SVR_CELL_LIMIT_ORACLE", "0") not in ("", "0")

ORACLE_CASES = tuple(n for n in C.NAMES if not n.startswith("run-"))       # (case 4: below)


def _flat(a):
    return np.asarray(a).reshape(-1)


def _engine(case, pvr=False, **options):
    from fetalreconstruction_amd import engine as E
    rec = E.Reconstruction(0)
    if pvr:
        rec.set_option("pvr", 1)
        E.sync_gpu(rec, case.problem, quality_factor=1.0)
    else:
        E.sync_gpu(rec, case.problem)
    assert rec.get_option("back_mode") == 5 and rec.get_option("fwd_mode") == 2 and rec.get_option("gauss_mode") == 1     # the defaults: the cell kernels
    for k, v in {**case.options, **options}.items():
        rec.set_option(k, v)
    return rec


def _sequence(rec, case, ref=None, volume=None, scatter_repeats=False, check=True):
    """The sequence of test_random_geometry_against_the_oracle; compared with the oracle's buffers where ref is given.  The gather runs twice
    and has to give the same bits (the cell gather, and fwd_unit_kernel it falls back onto); the scatter too where it is the cell scatter."""
    from fetalreconstruction_amd import engine as E
    P = case.problem
    ones = np.ones(P.ns, np.float32)
    rec.UpdateScaleVector(ones, ones)
    rec.InitializeEMValues()
    rec.GaussianReconstruction()
    out = dict(psf_sums=_flat(rec.debug_get(E.BUF_PSF_SUMS)).copy(), volw=_flat(rec.getVolWeights()).copy(), recon=_flat(rec.syncCPU()).copy())
    rec.debug_set(E.BUF_RECONSTRUCTED, ref["recon"] if ref is not None else volume if volume is not None else out["recon"])

    def gather():
        rec.debug_set(E.BUF_SIMSLICES, np.zeros(P.slices.shape, np.float32))
        rec.SimulateSlices()
        return [_flat(rec.debug_get(b)).copy() for b in (E.BUF_SIMSLICES, E.BUF_SIMWEIGHTS, E.BUF_SIMINSIDE)]
    g1, g2 = gather(), gather()
    for a, b in zip(g1, g2):
        assert np.array_equal(a, b, equal_nan=True)
    out.update(simslices=g1[0], simweights=g1[1], siminside=g1[2])
    w, ss, sw = C.em_inputs(P)
    rec.debug_set(E.BUF_WEIGHTS, w)

    def scatter():
        rec.debug_set(E.BUF_SIMSLICES, ss)
        rec.SuperresolutionBackproject(sw)
        return _flat(rec.debug_get(E.BUF_CONFIDENCE_MAP)).copy(), _flat(rec.debug_get(E.BUF_ADDON)).copy()
    out["cmap"], out["addon"] = scatter()
    if scatter_repeats:
        cm, ad = scatter()
        assert np.array_equal(cm, out["cmap"]) and np.array_equal(ad, out["addon"])
    if ref is not None and check:
        _is_the_oracles(case, out, ref)
    return out


def _figures(what, out, ref):
    e = {k: rel_err(out[k], _flat(ref[k])) for k in ("volw", "simslices", "simweights", "cmap", "addon")}
    print(f"{what}: against the oracle: rel_err " + ", ".join(f"{k} {v:.3g}" for k, v in e.items()))
    return e


def _is_the_oracles(case, out, ref, only_scatter=False, e=None):
    """every figure first, then the assertions: hit sets bit for bit, v_PSF_sums to rtol 1e-6, the scatters' and the gather's buffers to TOL"""
    e = e or _figures(case.name, out, ref)
    if not only_scatter:
        assert np.array_equal(out["psf_sums"] != 0, _flat(ref["psf_sums"]) != 0)
        assert np.allclose(out["psf_sums"], _flat(ref["psf_sums"]), rtol=1e-6, atol=0, equal_nan=True)
        assert np.array_equal(out["volw"] > 0, ref["volw"] > 0) and e["volw"] < TOL
        assert np.array_equal(out["siminside"], _flat(ref["siminside"]))
        assert e["simslices"] < TOL and e["simweights"] < TOL
    assert (ref["cmap"] > 0).sum() > 100
    assert np.array_equal(out["cmap"] > 0, ref["cmap"] > 0)
    assert e["cmap"] < TOL and e["addon"] < TOL


def _counts_say(rec, case, gather_on_cells=True):
    fb = rec.fallbacks()
    print(f"{case.name}: fallbacks {fb}, cells {rec.cell_stats()}")
    if case.side == "inside":
        assert not any(fb.values()), fb
        assert rec.cell_stats()["sorted_pixels"] > 0
    else:
        assert fb["scatter_to_atomics"] >= 2, fb                       # pass 2 of the Gaussian reconstruction and the SR scatter
        if case.split_gather or not gather_on_cells:                   # the gather's own lists hold the geometry / the gather never asked for them
            assert fb["gather_to_tiles"] == 0 and fb["gauss1_to_tiles"] == 0, fb
        else:
            assert fb["gather_to_tiles"] >= 1 and fb["gauss1_to_tiles"] >= 1, fb


def _both_tables(case, ref, pvr=False):
    """the sequence with the coefficient table on and with every tap evaluated: each against the oracle, the gathers bit for bit against
    each other (cell path and fallback alike), the scatters too where they are the cell scatter (an atomic scatter's last bits depend on the run)"""
    inside = case.side == "inside"
    res = []
    for table in (1, 0):
        rec = _engine(case, pvr=pvr, coeff_table=table)
        res.append(_sequence(rec, case, ref, scatter_repeats=inside))
        # (a patch-based gather that streams the table runs on slice tiles by choice where the cells are small -- pass_path: table_on_cells -- and
        # so does pass 1; that is no fallback and is not counted)
        _counts_say(rec, case, gather_on_cells=not (pvr and table))
        rec.close()
    a, b = res
    for k in ("psf_sums", "simslices", "simweights", "siminside") + (("volw", "cmap", "addon") if inside else ()):
        assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_limit_case_against_the_oracle(name):
    case = C.build(name)
    _both_tables(case, C.oracle_run(name))


@pytest.mark.parametrize("name", ["centres-x-beyond", "centres-x-inside"])
def test_patch_based_limit_case_against_the_oracle(name):
    """support 12 (NC = 5, NH = 6), five slots: the same centre limit"""
    case = C.build(name)
    _both_tables(case, C.oracle_run(name, pvr=True), pvr=True)


@pytest.mark.parametrize("name", ["run-beyond", "run-inside"])
def test_pixels_of_one_slice_in_one_cell(name):
    """Case 4: 16 512 / 16 384 pixels of one slice in one cell (CELL_RUN_MAX).  The oracle needs several seconds for them, so the reference
    here is a second context with the tile kernels asked for by name; SVR_CELL_LIMIT_ORACLE=1 adds the oracle for both contexts.
    The limit stood at 65 535 (what CellRun::n can say) when this test was written, with 256 x 257 and 255 x 257 pixels: the cell path then
    left volw 3.99e-05 from the oracle and 4.07e-05 from the tile kernels (cmap 2.48e-06, addon 5.53e-06; the tile kernels 6.92e-06 from the
    oracle) -- a slot adds its quarter of a run to a voxel in one chain of float adds.  The limit moved to 16 384 and the case with it.
    Recorded on an MI355X with the oracle on (rel_err of volw, simslices, simweights, cmap, addon against the oracle):
      run-beyond  the automatic fallback 1.3e-06, 2.99e-07, 2.98e-07, 1.4e-06, 9.56e-07; the tile kernels by name 1.3e-06, 2.99e-07, 2.98e-07, 1.08e-06, 1.53e-06
      run-inside  the cell path 1.57e-05, 3.59e-07, 2.98e-07, 1.26e-06, 3.77e-06; the tile kernels by name 1.24e-06, 3.59e-07, 2.98e-07, 1.11e-06, 1.79e-06
    and the two contexts against each other: run-beyond volw 1.92e-06, cmap 2.15e-06, addon 1.72e-06; run-inside 1.55e-05, 1.9e-06, 4.52e-06."""
    case = C.build(name)
    ref = C.oracle_run(name) if RUN_ORACLE else None
    rec = _engine(case)
    a = _sequence(rec, case, ref, scatter_repeats=case.side == "inside", check=False)
    _counts_say(rec, case)
    rec.close()
    tiles = _engine(case, back_mode=4, fwd_mode=1, gauss_mode=1)
    b = _sequence(tiles, case, ref, volume=a["recon"], check=False)
    fb = tiles.fallbacks()
    assert not (fb["scatter_to_atomics"] or fb["gather_to_tiles"] or fb["gauss1_to_tiles"]), fb      # asked for by name: nothing fell back
    tiles.close()
    for k in ("psf_sums", "simslices", "simweights", "siminside"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert (a["cmap"] > 0).sum() > 100 and np.array_equal(a["cmap"] > 0, b["cmap"] > 0)
    ev, ec, ea = rel_err(a["volw"], b["volw"]), rel_err(a["cmap"], b["cmap"]), rel_err(a["addon"], b["addon"])
    print(f"{name}: against the tile kernels: volw rel_err {ev:.3g}, cmap {ec:.3g}, addon {ea:.3g}")
    figs = None if ref is None else (_figures(name, a, ref), _figures(name + " on the tile kernels", b, ref))
    assert ev < TOL and ec < TOL and ea < TOL
    if ref is not None:
        _is_the_oracles(case, a, ref, e=figs[0])
        _is_the_oracles(case, b, ref, e=figs[1])


def test_channel_scatter_refuses_beyond_the_limit_and_the_context_goes_on():
    from fetalreconstruction_amd import engine as E
    name = "centres-x-beyond"
    case, ref = C.build(name), C.oracle_run(name)
    rec = _engine(case)
    out = _sequence(rec, case, ref)
    with pytest.raises(E.SvrError, match="cannot hold this geometry"):
        rec.channel_scatter(np.ones(case.problem.slices.shape, np.float32))
    w, ss, sw = C.em_inputs(case.problem)
    rec.debug_set(E.BUF_SIMSLICES, ss)
    rec.SuperresolutionBackproject(sw)
    out["cmap"], out["addon"] = _flat(rec.debug_get(E.BUF_CONFIDENCE_MAP)).copy(), _flat(rec.debug_get(E.BUF_ADDON)).copy()
    _is_the_oracles(case, out, ref, only_scatter=True)
    rec.close()


def test_the_first_psf_pass_where_the_lazy_store_is_impossible():
    """The table wanted, not there and left to the first evaluating cell pass (table_plan, csrc/svr_plan.h), on a geometry whose cell lists
    cannot be built: the scatter evaluates on the tiles and leaves the table unwritten; the gather builds it with k_coeff_build and
    streams it, and gives the bits of a context that evaluates every tap.  (The expectations were read from the code before the table's
    decisions moved into table_plan, and agree with a transcription of that code over every input combination.)"""
    from fetalreconstruction_amd import engine as E
    case = C.build("centres-x-beyond")
    assert not case.split_gather                                       # (neither the scatter's lists nor the gather's hold the geometry)
    P = case.problem
    ones = np.ones(P.ns, np.float32)

    def after_the_gaussian(**options):
        rec = _engine(case, **options)
        rec.timer_enable(True)
        rec.UpdateScaleVector(ones, ones)
        rec.InitializeEMValues()
        rec.GaussianReconstruction()
        return rec

    rec = after_the_gaussian()
    assert rec.get_option("coeff_table") == 1 and rec.get_option("coeff_state") == 0
    volume = _flat(rec.syncCPU()).copy()                               # (pass 2 ran on the atomics: one volume for the gathers below)
    w, ss, sw = C.em_inputs(P)
    rec.debug_set(E.BUF_WEIGHTS, w)
    rec.debug_set(E.BUF_SIMSLICES, ss)
    rec.SuperresolutionBackproject(sw)
    t = rec.timers()
    print(f"scatter first: coeff_state {rec.get_option('coeff_state')}, coeff_build {t['coeff_build']}, backproject_store {t['backproject_store']}, backproject_table {t['backproject_table']}")
    assert rec.get_option("coeff_state") == 0 and t["coeff_build"][1] == 0
    assert t["backproject"][1] == 1 and t["backproject_store"] == (0.0, 0) and t["backproject_table"][1] == 0
    rec.close()

    res = []
    for table in (1, 0):
        rec = after_the_gaussian(coeff_table=table)
        assert rec.get_option("coeff_state") == 0
        rec.debug_set(E.BUF_RECONSTRUCTED, volume)
        rec.debug_set(E.BUF_SIMSLICES, np.zeros(P.slices.shape, np.float32))
        rec.SimulateSlices()
        t = rec.timers()
        print(f"gather first, coeff_table {table}: coeff_state {rec.get_option('coeff_state')}, coeff_build {t['coeff_build']}, forward_store {t['forward_store']}, forward_table {t['forward_table']}")
        assert rec.get_option("coeff_state") == (2 if table else 0) and t["coeff_build"][1] == table
        assert t["forward"][1] == 1 and t["forward_store"][1] == 0 and t["forward_table"][1] == table
        res.append([_flat(rec.debug_get(b)).copy() for b in (E.BUF_SIMSLICES, E.BUF_SIMWEIGHTS, E.BUF_SIMINSIDE)])
        rec.close()
    assert np.abs(res[0][0]).max() > 0
    for a, b in zip(*res):
        assert np.array_equal(a, b, equal_nan=True)


def test_normalise_bias_scatter_falls_back_onto_the_atomics():
    """NormaliseBias where the scatter's lists cannot be built (case 7 beyond): the sequence of test_bias_steps_against_the_oracle"""
    from fetalreconstruction_amd import engine as E
    from oracle import pyoracle as po
    from tests.test_bias_gpu import _biased
    from tests.twins.reconstruction import irtkReconstruction
    from tests.util import run_to_state
    case = C.build("lds-beyond")
    P = _biased(case.problem)
    rec = E.Reconstruction(0)
    rec.set_flags(disable_bias_correction=False)
    E.sync_gpu(rec, P)
    for k, v in case.options.items():
        rec.set_option(k, v)
    orc = po.OracleReconstruction(P, po.CANON, bias_correction=True)
    drivers = []
    for eng in (rec, orc):
        d = irtkReconstruction(eng, P.ns, max_intensity=P.max_intensity, min_intensity=P.min_intensity)
        d.SetSmoothingParameters(150, 0.02)
        d._disableBiasC = False
        run_to_state(d, "estep0")
        drivers.append(d)
    do = drivers[1]
    for b, a in ((E.BUF_WEIGHTS, orc.weights), (E.BUF_SIMSLICES, orc.simslices), (E.BUF_SIMWEIGHTS, orc.simweights)):
        rec.debug_set(b, a)
    rec.CorrectBias(12.0, False)
    orc.CorrectBias(12.0, False)
    assert rel_err(rec.debug_get(E.BUF_BIAS), orc.bias, floor=1.0) < 2e-5
    rec.debug_set(E.BUF_BIAS, orc.bias)
    rec.debug_set(E.BUF_WEIGHTS, orc.weights)
    rec.SuperresolutionBackproject(orc.slice_weights)
    orc.SuperresolutionBackproject(orc.slice_weights)
    orc.SuperresolutionUpdate(do._adaptive, do._alpha, do._min_intensity, do._max_intensity, do._delta, do._lambda)
    rec.debug_set(E.BUF_RECONSTRUCTED, orc.recon)
    before = rec.fallbacks()["scatter_to_atomics"]
    rec.NormaliseBias(0, 12.0)
    orc.NormaliseBias(0, 12.0)
    assert rec.fallbacks()["scatter_to_atomics"] == before + 1 and rec.get_option("bias_scatters_on_cells") == 0
    eb, er = rel_err(rec.debug_get(E.BUF_BIAS_VOLUME), orc.bias_vol, floor=1.0), rel_err(rec.syncCPU(), orc.recon)
    print(f"lds-beyond: bias_vol rel_err {eb:.3g}, volume {er:.3g}")
    assert np.abs(orc.bias_vol).max() > 0
    assert eb < 2e-5 and er < 2e-5
    rec.close()
