"""Every rung of the tile kernels' box fallbacks against the oracle (tests/tile_rungs.py has the rules and the cases, tests/operator_entries.py the
impulse design and the reasoning behind its bounds).

launch_scatter's ladder (back_wave_kernel, its large-box second pass with the table, back_slot_kernel<8>, back_tiled_kernel with the box in the LDS and
without, pvr_tiles_kernel) and the memory-read arm of fwd_unit_kernel run for the inputs that are hard -- fine volumes, coarse or oblique slices -- and
nobody chooses them.  Here options alone (wave_cap, tile_w / tile_h, fwd_unit_cap) push the two problems of operator_entries off rung 1, and a third
problem, "coarse" (96^3 voxels, 14 x 14-pixel slices of 6.3 voxels a pixel), reaches the last resort; the census of tile_rungs says on the CPU which tile
ends where, and the device's counters are held to it:
  a. the SR scatter of impulses: addon and the confidence map are the oracle's BITS at every voxel whatever rung a pixel's tile ends on;
     fallbacks()["tiles_rerun"] rises by the census's count per pass, counters()["rerun8_tiles"] / ["fallback_tiles"] equal it (an interval where the
     slot rule is undecided), the options stand as set (tile_cap read from the device), the other fallback counters stay 0;
  b. the same set scattered on different rungs gives array_equal buffers;
  c. passes 1 and 2 of the Gaussian reconstruction down the same ladder: the bounds of test_operator_entries_gpu.py, part c (3 u, u = 2^-24);
  d. the gather and pass 1 through the memory-read arm: 4 u (support 16) and 12 u (support 12) an entry; for the coarse problem a pixel below the low
     face sums m folded taps into one entry, m - 1 more roundings: (4 + m - 1) u, m from operator_entries.fold_terms;
  e. one dense Gaussian pass, scatter and gather per case: 2e-5 and (n + 6) u sum|terms| an element, n from terms_folded for the coarse problem;
  f. a re-run list sent out in more than one piece (SVR_LIST_PIECE, the hook of in_pieces).
What stayed out of reach: the wave kernel's reject Dz > 64 (the widest tile of the coarse problem spans 60 planes; with the table rung 1 takes all 60,
case coarse-16-8x8-table), and at tile_cap 18 304 a support-16 tile whose vox lies between its two bounds and FITS (the device rejected every undecided
tile: these thick slices have no dead units).  in_pieces' piece can be lowered (SVR_LIST_PIECE): part f.

Recorded on an MI355X (tile_cap 18 304; u = 2^-24; the census per case is in DESIGN.md 5.1, "The rungs under test", and printed with -s):
  scatters    bit for bit on every rung and between rungs: 36 794 / 30 406 / 283 342 entries a pass on tiny / ones24 / coarse for the support of 16,
              44 598 / 29 782 / 195 970 for 12; tiles_rerun, rerun8_tiles and fallback_tiles as the census has them; undecided tiles: coarse 4 x 4
              27 of 27 rejected, with the table 18 of 18, 8 x 8 2 of 2
  Gaussian    pass 2 within 3 u: worst 2.63 (coarse, 16; 152 702 entries), 2.44 (tiny, 16), 2.28 (tiny, 12), 2.26 (coarse, 12), 2.23 (ones24)
  gathers     memory-read arm: worst 0.58 of the bound for 16 (2.3 u of 4), 0.35 for 12 (4.2 u of 12); LDS arm 0.29; pass 1: psf_sums the oracle's bits
  dense       at most 0.69 of (n + 6) u sum|terms| (coarse, 12, addon); 0.58 for 16
Scratch libraries with one mistake each (nothing of them committed), this file against test_operator_entries_gpu.py, test_cell_limits_gpu.py and
test_coeff_layout_gpu.py (97 tests):
  (a) no d_tiles_fb2 -> d_tiles_fb move after the large-box pass: part a and e failed for coarse-16-4x4-table and coarse-16-8x8-table, part b for
      coarse / 16; the 97 older tests passed
  (b) `- lox` dropped from rbase in back_tiled_kernel's LDS arm: parts a, c, e and f failed for coarse-16-8x8, part b for coarse / 16; of the older tests
      the two back_mode 1 paths of test_operator_entries_gpu.py (lds-atomics-1) failed as well: that mode runs the LDS arm for every tile, so this arm
      was covered before; its hand-off from a slot reject and the direct-atomic arm were not
  (c) the memory-read arm of fwd_unit_kernel ignores the mask: part d failed for tiny-16-evaluated, tiny-16-table and tiny-12-evaluated; the 97 passed"""
import numpy as np
import pytest

from tests import operator_entries as O
from tests import tile_rungs as T
from tests.test_operator_entries_gpu import TOL_SUM, _engine, _f32, _gather, _scatter_set, _scatter_values
from tests.util import rel_err

pytestmark = pytest.mark.gpu

TILES = (("fwd_mode", 1),)                              # the gathers of these contexts stay on the tile kernel: no cell list is built
QUIET = ("scatter_to_atomics", "gather_to_tiles", "gauss1_to_tiles")


def _caps(rec, options):
    """the options stand as set; -> tile_cap as the device has it"""
    for k, v in options:
        assert rec.get_option(k) == v, (k, v, rec.get_option(k))
    cap = rec.get_option("tile_cap")
    assert cap in T.TILE_CAPS, cap
    return cap


def _counted(rec, cen, passes, what):
    """the path ran: the re-run counters are the census's"""
    fb, cnt = rec.fallbacks(), rec.counters()
    assert fb["tiles_rerun"] == passes * cen["rerun"], (what, fb, cen["rerun"], passes)
    assert not any(fb[k] for k in QUIET), fb
    assert cnt["rerun8_tiles"] == cen["rerun"], (what, cnt, cen["rerun"])
    lo, hi = cen["fallback"]
    assert lo <= cnt["fallback_tiles"] <= hi, (what, cnt, cen["fallback"])
    return cnt["fallback_tiles"]


def _census_line(cen):
    return ", ".join(f"{r} {n}" for r, n in cen["tiles"].items() if n)


# ---- a. the scatter down the ladder -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(T.SCATTER_CASES))
def test_scatter_gives_the_oracles_bits_on_every_rung(case):
    name, pvr, tile, wave_cap, table, reach = T.SCATTER_CASES[case]
    options = T.scatter_options(case)
    sets, _ = T.pixel_sets(name, pvr)
    E, rec = _engine(name, pvr, options + TILES)
    cap = _caps(rec, options)
    cen = T.scatter_census(case, cap)
    assert all(cen["tiles"][r] > 0 and cen["pixels"][r] & {p for s in sets for p in s} for r in reach[cap])
    act = _scatter_values(E, rec, name, 3.0)
    entries = 0
    for k, s in enumerate(sets[:1] + sets):                        # (the first set twice: a context that has run the ladder once)
        n, _ = _scatter_set(E, rec, name, pvr, act, s, 3.0, (case, k - 1))
        slot_rejects = _counted(rec, cen, k + 1, (case, k - 1))
        entries += 2 * n * (k > 0)
    tm = rec.timers()
    assert tm["backproject"][1] == len(sets) + 1 and tm["backproject_store"][1] == 0
    assert tm["backproject_table"][1] == (len(sets) + 1 if table else 0) and (tm["coeff_build"][1] > 0) == table
    assert rec.counters()["tiles"] == sum(cen["tiles"].values())
    _scatter_values(E, rec, name, 1.5)
    _scatter_set(E, rec, name, pvr, act, sets[0], 1.5, (case, "e = 0.5"))
    if cen["tiles"]["slot?"]:
        print(f"scatter {case}: the undecided tiles, if rejected: {T.if_rejected(name, pvr, tile, cap, cen['pixels']['slot?'])}")
    print(f"scatter {case}: tile_cap {cap}, tiles: {_census_line(cen)}; re-run {cen['rerun']}, slot rejects {slot_rejects} of {cen['fallback']}; "
          f"{len(sets)} sets, {sum(len(s) for s in sets)} impulse pixels, {entries} entries bit for bit")
    rec.close()


# ---- b. the same bits between rungs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pvr", [(n, v) for n in O.PROBLEMS + O.RUNG_PROBLEMS for v in (False, True)], ids=lambda v: str(v))
def test_the_same_bits_between_rungs(name, pvr):
    """every output element is one tap or the sum of two, so the order of the atomics is no order: the buffers of a set scattered with the default caps
    (6 x 4 tiles, rung 1 wherever a tile fits) and with every case of this problem are array_equal"""
    cases = [c for c, v in T.SCATTER_CASES.items() if v[:2] == (name, pvr)]
    sets, _ = T.pixel_sets(name, pvr)
    ones = np.ones(O.problem(name).ns, np.float32)
    ref = None
    for case in [None] + cases:
        options = (("coeff_table", 0), ("back_mode", 4), ("tile_w", 6), ("tile_h", 4)) if case is None else T.scatter_options(case)
        E, rec = _engine(name, pvr, options + TILES)
        act = _scatter_values(E, rec, name, 3.0)
        got = []
        for s in sets:
            rec.debug_set(E.BUF_SIMSLICES, _f32(act))
            rec.debug_set(E.BUF_WEIGHTS, _f32(O.indicator(name, s)))
            rec.SuperresolutionBackproject(ones)
            got.append((rec.debug_get(E.BUF_ADDON), rec.debug_get(E.BUF_CONFIDENCE_MAP)))
        rerun = rec.fallbacks()["tiles_rerun"]
        rec.close()
        if ref is None:
            ref, ref_rerun = got, rerun
            assert all(np.count_nonzero(c) for _, c in ref)
            continue
        for k, ((a, c), (ra, rc)) in enumerate(zip(got, ref)):
            assert np.array_equal(a, ra) and np.array_equal(c, rc), (case, k)
    print(f"same bits {name} support {O.support(pvr)}: {len(cases)} cases against the default caps ({ref_rerun} tiles re-run there), {len(sets)} sets")


# ---- c. the Gaussian reconstruction down the ladder ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(T.GAUSS_CASES))
def test_gaussian_passes_down_the_ladder(case):
    """part c of test_operator_entries_gpu.py with the case's options: only the set's pixels are live, a tile's box is that of its one or two pixels (or
    of a pair of tile_rungs.gauss_pairs), pass 2 takes the ladder with ta.gauss set -- and pvr_tiles_kernel<MODE_GAUSS2> where the patch-based slot
    kernel rejects"""
    name, pvr, tile, wave_cap, table, _ = T.SCATTER_CASES[case]
    from fetalreconstruction_amd import engine as E
    options = T.scatter_options(case) + TILES
    P = O.problem(name)
    reached, entries, worst_all = set(), 0, 0.0
    for i, s in enumerate(T.gauss_sets(name, pvr)):
        Q = O.padded(name, O.indicator(name, s), 512.0)
        rec = E.Reconstruction(0)
        if pvr:
            rec.set_option("pvr", 1)
            E.sync_gpu(rec, Q, quality_factor=1.0)
        else:
            E.sync_gpu(rec, Q)
        rec.timer_enable(True)
        for k, v in options:
            rec.set_option(k, v)
        cap = _caps(rec, options)
        ones = np.ones(P.ns, np.float32)
        rec.UpdateScaleVector(ones, ones)
        rec.GaussianReconstructionLocal()
        psf_sums, volw, recon, voxcount = O.expected_gauss(name, pvr, s)
        ps = rec.debug_get(E.BUF_PSF_SUMS)
        assert np.array_equal(ps != 0, psf_sums != 0) and np.count_nonzero(ps) > 0
        assert np.allclose(ps, psf_sums, rtol=1e-6, atol=0)
        assert np.array_equal(rec.debug_get(E.BUF_VOXEL_COUNT), voxcount) and voxcount.sum() > 0
        cen = T.scatter_census(case, cap, psf_sums != 0)               # pass 2's tiles: the pixels that passed the gate
        _counted(rec, cen, 1, (case, i))
        reached |= {r for r, n in cen["tiles"].items() if n}
        got_w = rec.getVolWeights()
        want = O.gauss_from_taps(name, pvr, s, ps)
        worst = np.max(np.abs(got_w - want)[want != 0] / want[want != 0]) / O.U
        worst_all = max(worst_all, worst)
        assert np.array_equal(got_w != 0, volw != 0)
        bad = O.within_relative(got_w, want, 3)
        assert not len(bad), (case, i, O.describe(bad, got_w, want))
        got_r = rec.debug_get(E.BUF_RECONSTRUCTED)
        bad = O.within_relative(got_r, 512.0 * want, 3)
        assert not len(bad), (case, i, "volume", O.describe(bad, got_r, 512.0 * want))
        assert rec.get_option("gauss_mode") == 1 and rec.timers()["gauss"][1] == 1
        entries += np.count_nonzero(want)
        print(f"gauss {case} set {i}: tiles: {_census_line(cen)}; {np.count_nonzero(want)} entries, worst {worst:.2f} u of 3")
        rec.close()
    assert set(T.GAUSS_CASES[case][cap]) <= reached, (case, cap, reached)
    print(f"gauss {case}: tile_cap {cap}, rungs reached {sorted(reached)}, {entries} entries within 3 u (worst {worst_all:.2f})")


# ---- d. the gather and pass 1 through the memory-read arm -----------------------------------------------------------------------------
def _gather_options(case):
    name, pvr, cap, kind, _ = T.GATHER_CASES[case]
    opt = [("coeff_table", 1 if kind == "table" else 0)]
    if kind == "table":
        opt.append(("coeff_lazy", 0))
    opt += [("fwd_mode", 1), ("back_mode", 4), ("fwd_tile_w", T.GATHER_TILE[0]), ("fwd_tile_h", T.GATHER_TILE[1])]      # (back_mode 4: no cell list is built)
    if cap is not None:
        opt.append(("fwd_unit_cap", cap))
    return tuple(opt)


@pytest.mark.parametrize("case", list(T.GATHER_CASES))
def test_gather_through_the_memory_read_arm(case):
    """One rounding chain per entry as in part b of test_operator_entries_gpu.py: k = 4 for the support of 16, 8 + 4 for the patch-based 12.  A pixel
    of the coarse problem whose footprint hangs below a low face sends m taps to ONE voxel (operator_entries.fold_terms): its entry is a sum of m
    positive terms, recursive summation in any order loses at most (m - 1) u of it: k + m - 1.  m is 1 everywhere on the other two problems."""
    name, pvr, unit_cap, kind, arms = T.GATHER_CASES[case]
    O.warm(name, pvr)
    options = _gather_options(case)
    k = (12 if pvr else 4) + O.fold_terms(name, pvr).astype(np.float64) - 1
    sets, _ = O.impulse_voxel_sets(name, pvr)
    P = O.problem(name)
    act = P.slices != -1
    w_all, inside_all = O.gather_weights(name, pvr)
    E, rec = _engine(name, pvr, options)
    cap = _caps(rec, options)
    cen = T.gather_case_census(case, cap)
    assert all(cen["tiles"][a] > 0 for a in arms)
    rec.debug_set(E.BUF_PSF_SUMS, _f32(act))
    entries, worst_arm = 0, dict(lds=0.0, mem=0.0)
    arm_of = np.full(P.slices.shape, "", dtype="U3")
    for a in ("lds", "mem"):
        for sl, px, py in cen["pixels"][a]:
            arm_of[sl, py, px] = a
    for i, v in enumerate(sets[:1] + sets):
        sim, w, inside = _gather(E, rec, name, O.impulse_volume(name, v))
        want_sim, _, _, reach = O.expected_gather(name, pvr, v)
        got, want = sim.astype(np.float64) * w.astype(np.float64), want_sim.astype(np.float64) * w_all.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            dev = np.where(want != 0, np.abs(got - want) / (O.U * np.abs(want)), np.where(got != 0, np.inf, 0.0))
        for a in worst_arm:
            if np.any((arm_of == a) & (want != 0)):
                worst_arm[a] = max(worst_arm[a], float((dev / k)[(arm_of == a) & (want != 0)].max()))
        bad = np.flatnonzero(~(dev <= k).reshape(-1))
        assert not len(bad), (case, i - 1, O.describe(bad, got, want))
        assert np.count_nonzero(want) > 0 and not np.any(want[~reach])
        assert np.array_equal(inside, inside_all)
        assert rel_err(w, w_all) < TOL_SUM
        entries += np.count_nonzero(want) * (i > 0)
    tm = rec.timers()
    assert tm["forward"][1] == len(sets) + 1 and tm["forward_table"][1] == (len(sets) + 1 if kind == "table" else 0)
    assert not any(rec.fallbacks().values()), rec.fallbacks()
    reach_any = np.any([O.expected_gather(name, pvr, v)[3] for v in sets], 0)
    assert all(np.any((arm_of == a) & reach_any) for a in arms)
    print(f"gather {case}: box {min(cap, T.FWD_UNIT_CAP if unit_cap is None else unit_cap)}, tiles {cen['tiles']}; {len(sets)} sets, {entries} entries, "
          f"worst of its bound: LDS arm {worst_arm['lds']:.3f}, memory arm {worst_arm['mem']:.3f} (bound {12 if pvr else 4} u, + m - 1 below a face)")
    # pass 1 of the Gaussian reconstruction (fwd_unit_kernel<GAUSS1>; with the table its COEFF instantiation) on the full problem, and the dense gather
    want = O.expected_dense(name, pvr)
    cen1 = T.gather_case_census(case, cap, gauss1=True)
    assert all(cen1["tiles"][a] > 0 for a in arms)
    rec.InitializeEMValues()
    rec.GaussianReconstructionLocal()
    ps = rec.debug_get(E.BUF_PSF_SUMS)
    assert np.array_equal(ps != 0, want["psf_sums"] != 0)             # the gate
    bad = O.within_relative(ps, want["psf_sums"], 3)                  # both sides add the same products in double and round once
    assert not len(bad), (case, "psf_sums", O.describe(bad, ps, want["psf_sums"]))
    assert np.array_equal(rec.debug_get(E.BUF_VOXEL_COUNT), want["voxcount"])
    nz = want["psf_sums"] != 0
    worst1 = float(np.max(np.abs(ps.astype(np.float64) - want["psf_sums"])[nz] / want["psf_sums"][nz]) / O.U)
    rec.debug_set(E.BUF_PSF_SUMS, want["psf_sums"])
    sim, w, inside = _gather(E, rec, name, want["volume"])
    assert np.array_equal(inside, want["siminside"])
    n_p = O.support(pvr) ** 3 * (8 if pvr else 1)
    for what, g, r in (("simweights", w, want["simweights"]),
                       ("simslices * simweights", sim.astype(np.float64) * w.astype(np.float64), want["simslices"].astype(np.float64) * want["simweights"].astype(np.float64))):
        bad = O.within_terms(g, r, n_p)
        assert not len(bad), (case, what, O.describe(bad, g, r))
        assert rel_err(g, r) < TOL_SUM
    assert rel_err(sim, want["simslices"]) < TOL_SUM
    assert not any(rec.fallbacks()[q] for q in QUIET), rec.fallbacks()
    print(f"gather {case}: pass 1 tiles {cen1['tiles']}, {int(nz.sum())} psf_sums worst {worst1:.2f} u of 3, {len(O.same_bits(ps, want['psf_sums']))} differ in bits; "
          f"dense gather of {int(np.count_nonzero(want['simweights']))} pixels within its bounds")
    rec.close()


# ---- e. dense passes down the ladder ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(T.SCATTER_CASES))
def test_dense_passes_down_the_ladder(case):
    """part d of test_operator_entries_gpu.py with the case's options: every pixel live, pass 2 of the Gaussian reconstruction and the SR scatter take
    the ladder with full tiles.  n: the pixels whose footprint box holds the voxel; for the coarse problem every tap counted where the index rule
    sends it (terms_folded: its last slice folds whole rows of taps onto the low face)."""
    name, pvr, tile, wave_cap, table, reach = T.SCATTER_CASES[case]
    O.warm(name, pvr)
    want = O.expected_dense(name, pvr)
    n_v = O.terms_folded(name, pvr) if name in O.RUNG_PROBLEMS else O.terms_bound(name, pvr)
    options = T.scatter_options(case)
    E, rec = _engine(name, pvr, options + TILES)
    cap = _caps(rec, options)
    cen = T.scatter_census(case, cap, want["psf_sums"] != 0)
    assert all(cen["tiles"][r] > 0 for r in reach[cap])
    rec.InitializeEMValues()
    rec.GaussianReconstructionLocal()
    ps = rec.debug_get(E.BUF_PSF_SUMS)
    assert np.array_equal(ps != 0, want["psf_sums"] != 0) and np.allclose(ps, want["psf_sums"], rtol=1e-6, atol=0)
    assert np.array_equal(rec.debug_get(E.BUF_VOXEL_COUNT), want["voxcount"])
    _counted(rec, cen, 1, (case, "pass 2"))
    report = []

    def check(what, got, ref, n, magnitude=None):
        bad = O.within_terms(got, ref, n, magnitude)
        s = np.abs(np.asarray(ref, np.float64).reshape(-1)) if magnitude is None else np.asarray(magnitude, np.float64).reshape(-1)
        d = np.abs(np.asarray(got, np.float64).reshape(-1) - np.asarray(ref, np.float64).reshape(-1))
        nn = np.broadcast_to(np.asarray(n, np.float64).reshape(-1), d.shape) + 6
        report.append(f"{what} {float(np.max(d[s > 0] / (nn[s > 0] * O.U * s[s > 0]))):.3f}")
        assert not len(bad), (case, what, O.describe(bad, got, ref))
        assert rel_err(got, ref) < TOL_SUM, (case, what, rel_err(got, ref))

    volw = rec.getVolWeights()
    assert np.array_equal(volw > 0, want["volw"] > 0)
    check("volw", volw, want["volw"], n_v)
    check("recon", rec.syncCPU(), want["recon"], n_v)
    rec.debug_set(E.BUF_PSF_SUMS, want["psf_sums"])
    wts, ss, sw = O.dense_inputs(name)
    rec.debug_set(E.BUF_WEIGHTS, wts)
    rec.debug_set(E.BUF_SIMSLICES, ss)
    rec.SuperresolutionBackproject(sw)
    cm, ad = rec.debug_get(E.BUF_CONFIDENCE_MAP), rec.debug_get(E.BUF_ADDON)
    _counted(rec, cen, 2, (case, "scatter"))
    assert np.array_equal(cm > 0, want["cmap"] > 0)
    check("cmap", cm, want["cmap"], n_v)
    check("addon", ad, want["addon"], n_v, magnitude=want["addon_abs"])
    print(f"dense {case}: tiles: {_census_line(cen)}; worst of its bound: {', '.join(report)}")
    rec.close()


# ---- f. a re-run list longer than one launch piece --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,piece", [("tiny-16-wave1024", 64), ("coarse-16-8x8", 4), ("coarse-12-8x8", 4)])
def test_rerun_lists_in_pieces(case, piece, monkeypatch):
    """in_pieces' piece lowered by its hook: the slot kernel's list (and the last resort's) goes out in several launches, offsets and counts per piece"""
    monkeypatch.setenv("SVR_LIST_PIECE", str(piece))
    name, pvr = T.SCATTER_CASES[case][:2]
    options = T.scatter_options(case)
    sets, _ = T.pixel_sets(name, pvr)
    E, rec = _engine(name, pvr, options + TILES)
    cen = T.scatter_census(case, _caps(rec, options))
    assert cen["rerun"] > 2 * piece and (case.startswith("tiny") or cen["fallback"][0] > 2 * piece)
    act = _scatter_values(E, rec, name, 3.0)
    for k, s in enumerate(sets):
        _scatter_set(E, rec, name, pvr, act, s, 3.0, (case, "pieces", k))
        _counted(rec, cen, k + 1, (case, "pieces", k))
    print(f"pieces {case}: {cen['rerun']} tiles re-run and {cen['fallback']} slot rejects in pieces of {piece}")
    rec.close()
