"""The production PSF kernels, entry by entry against the oracle's taps (tests/operator_entries.py has the inputs and the reasoning).

DESIGN.md: "the device implements the oracle's canonical sequence bit for bit".  The parity tests hold the scatters and the gather to
|x - ref| <= 2e-5 max|ref|, under which four in ten of a pixel's taps can be dropped, doubled or moved by a voxel unseen.  Here the
operator is fed impulses, so that every output element is one kept tap or the sum of two, on the tiny problem and on the 24^3 problem under
a mask of ones, for the support of 16 and the patch-based 12:
  a. the SR scatter of unit weights at a set of pixels, among live neighbours of weight 0: addon and the confidence map are the oracle's
     BITS at every voxel, on every kernel path, each asserted to have run (options read back, timers, fallbacks, cell statistics);
  b. the gather of a volume that holds 4.0 on a lattice of voxels: simslices * simweights within 4 * 2^-24 of the oracle's, element by
     element (patch-based: 8 + 4, an entry is the sum of up to 8 terms of the eight-voxel average);
  c. passes 1 and 2 of the Gaussian reconstruction of a set of pixels that hold 512.0: the volume weights against the taps over the
     device's own psf_sums within 3 * 2^-24, the volume 512 times that, footprint and voxel counts exact;
  d. one dense scatter, gather and Gaussian pass per support with a bound per element, (n + 6) 2^-24 sum|terms|, beside the 2e-5.

Recorded on an MI355X (u = 2^-24; "worst" = the largest deviation met, in u):
  problem, support   scatter, per path                              gather, per path                          Gaussian passes, per mode
  tiny, 16           3 sets, 17 pixels, 36 794 entries bit for bit  5 sets, 40 voxels, 10 598 within 4 u      3 sets, 17 pixels, 18 397 weights and as many
                     (addon and confidence map; 7 350 sums of two)  (worst 2.43)                              volume entries within 3 u (worst 2.44)
  tiny, 12           3 sets, 25 pixels, 44 598 (15 100)             4 sets, 93 voxels, 29 110 within 12 u     3 sets, 25 pixels, 22 299 (worst 2.28)
                                                                    (worst 4.23)
  ones24, 16         4 sets, 11 pixels, 30 406 (4 604)              3 sets, 18 voxels, 1 176 (worst 2.23)     4 sets, 11 pixels, 15 203 (worst 2.23)
  ones24, 12         3 sets, 13 pixels, 29 782 (9 928)              3 sets, 20 voxels, 2 901 (worst 3.23)     3 sets, 13 pixels, 14 891 (worst 2.39)
Scatter paths: 11 for the support of 16, 7 for 12; gather paths: 7 and 6; Gaussian modes: 2.  The device's psf_sums of the impulse pixels were the
oracle's bits throughout.  Dense passes: 11 536 to 12 712 voxels and 997 to 8 951 pixels per buffer, none beyond 0.45 of its bound.
With a library whose table-reading support-16 scatter skips the first quad of every row (a scratch build, nothing committed), a. failed on the first
set that streams the table in all the paths that do (1 303 voxels of addon, from 1e-15 to 1e-4, read 0) and passed in those that evaluate; with only
the first tap of every row skipped, the same (456 voxels).  Both changes are still coarse enough for test_coefficient_table_against_the_oracle to
fail too (the first tap of a central row reaches 1.7e-3): a change that stays under its 2e-5 was not tried."""
import numpy as np
import pytest

from tests import operator_entries as O
from tests.util import rel_err

pytestmark = pytest.mark.gpu

CASES = [(name, pvr) for name in O.PROBLEMS for pvr in (False, True)]
TOL_SUM = 2e-5                                                    # tests/test_parity_gpu.py


def _ids(case):
    return f"{case[0]}-{'12' if case[1] else '16'}"


@pytest.fixture
def case(request):
    name, pvr = request.param
    O.warm(name, pvr)                                             # the oracle's full passes, once per session and side by side
    return name, pvr


def _with_paths(paths):
    """every (problem, support) with every path that support has"""
    args = [pytest.param(c, path, id=f"{_ids(c)}-{path}") for c in CASES for path in paths[c[1]]]
    return pytest.mark.parametrize("case,path", args, indirect=["case"])


each_case = pytest.mark.parametrize("case", CASES, ids=_ids, indirect=True)


def _engine(name, pvr, options):
    """the full problem on a fresh context, the options in the order given, scales and slice weights 1"""
    from fetalreconstruction_amd import engine as E
    P = O.problem(name)
    rec = E.Reconstruction(0)
    if pvr:
        rec.set_option("pvr", 1)
        E.sync_gpu(rec, P, quality_factor=1.0)
    else:
        E.sync_gpu(rec, P)
    rec.timer_enable(True)
    for k, v in options:
        rec.set_option(k, v)
    ones = np.ones(P.ns, np.float32)
    rec.UpdateScaleVector(ones, ones)
    return E, rec


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


READABLE = ("back_mode", "fwd_mode", "gauss_mode", "pvr_mode", "coeff_table", "coeff_lazy", "cell_w", "cell_h")


def _ran(rec, options, timer, passes, store, table, build=None, cells=None):
    """the intended path ran: the options stand as set, nothing fell back, the timers count the passes by kind"""
    for k, v in options:
        if k in READABLE:
            assert rec.get_option(k) == v, (k, v, rec.get_option(k))
    assert not any(rec.fallbacks().values()), rec.fallbacks()
    tm = rec.timers()
    n, ns, nt = tm[timer][1], tm[timer + "_store"][1], tm[timer + "_table"][1]
    assert n == passes, (timer, n, passes)
    if table:
        assert ns == store and nt == passes - store, (timer, n, ns, nt)
    else:
        assert ns == 0 and nt == 0, (timer, n, ns, nt)
    if build is not None:
        assert (tm["coeff_build"][1] > 0) == build, tm["coeff_build"]
    if cells:
        assert rec.cell_stats()["sorted_pixels"] > 0, rec.cell_stats()


# ---- a. the SR scatter ----------------------------------------------------------------------------------------------------------
CELL = tuple(O.CELL.items())
LEGACY = ("legacy_kernels", 1)
# name -> (options, the first pass writes the table, later passes stream it, k_coeff_build ran, on the cell lists)
SCATTER_PATHS = {
    False: {
        "cells-evaluated": ((("coeff_table", 0), ("back_mode", 5)), 0, False, False, True),
        "cells-table": ((("coeff_table", 1), ("back_mode", 5)), 1, True, False, True),            # the pass that writes the table, then the one that streams it
        "cells-table-built": ((("coeff_table", 1), ("coeff_lazy", 0), ("back_mode", 5)), 0, True, True, True),      # k_coeff_build's table
        "ring-cells-table": ((("coeff_table", 1), ("back_mode", 5)) + CELL, 1, True, False, True),
        "ring-cells-evaluated": ((("coeff_table", 0), ("back_mode", 5)) + CELL, 0, False, False, True),
        "defaults": ((), 1, True, False, True),
        "tiles-4": ((("coeff_table", 0), LEGACY, ("back_mode", 4)), 0, False, False, None),
        "tiles-4-table-built": ((("coeff_table", 1), ("coeff_lazy", 0), LEGACY, ("back_mode", 4)), 0, True, True, None),
        "workgroup-3": ((("coeff_table", 0), LEGACY, ("back_mode", 3)), 0, False, False, None),
        "lds-atomics-1": ((("coeff_table", 0), LEGACY, ("back_mode", 1)), 0, False, False, None),
        "atomics-0": ((("coeff_table", 0), LEGACY, ("back_mode", 0)), 0, False, False, None),
    },
    True: {
        "cells-evaluated": ((("coeff_table", 0), ("back_mode", 5)), 0, False, False, True),
        "cells-table-built": ((("coeff_table", 1), ("back_mode", 5)), 0, True, True, True),
        "ring-cells-evaluated": ((("coeff_table", 0), ("back_mode", 5)) + CELL, 0, False, False, True),
        "defaults": ((), 0, False, False, True),
        "tiles-4": ((("coeff_table", 0), ("back_mode", 4)), 0, False, False, None),
        "tiles-4-table-built": ((("coeff_table", 1), ("back_mode", 4)), 0, True, True, None),
        "pixels": ((("coeff_table", 0), ("pvr_mode", 0)), 0, False, False, None),
    },
}


def _scatter_values(E, rec, name, value):
    """slices = value and psf_sums = 1 on the active pixels (e = value - 1 with simslices 1)"""
    act = O.problem(name).slices != -1
    rec.debug_set(E.BUF_SLICES, np.where(act, np.float32(value), np.float32(-1.0)).astype(np.float32))
    rec.debug_set(E.BUF_PSF_SUMS, _f32(act))
    return act


def _scatter_set(E, rec, name, pvr, act, pixels, value, what):
    """one scatter of unit weights at `pixels`: the oracle's bits everywhere, no voxel left out -> (entries, sums of two)"""
    P = O.problem(name)
    rec.debug_set(E.BUF_SIMSLICES, _f32(act))
    rec.debug_set(E.BUF_WEIGHTS, _f32(O.indicator(name, pixels)))
    rec.SuperresolutionBackproject(np.ones(P.ns, np.float32))
    want = O.expected_scatter(name, pvr, pixels, value)
    for buf, w, nm in ((E.BUF_ADDON, want[0], "addon"), (E.BUF_CONFIDENCE_MAP, want[1], "confidence map")):
        g = rec.debug_get(buf)
        bad = O.same_bits(g, w)
        assert not len(bad), (what, nm, O.describe(bad, g, w))
        assert np.count_nonzero(g) == np.count_nonzero(w) > 0
    return np.count_nonzero(want[1]), int((O.terms_per_voxel(name, pvr, pixels) == 2).sum())


@_with_paths(SCATTER_PATHS)
def test_scatter_gives_the_oracles_bits(case, path):
    """a: every set, then the first set once more with slices 1.5 (e = 0.5, in case a path treats e specially)"""
    name, pvr = case
    options, store, table, build, cells = SCATTER_PATHS[pvr][path]
    sets, _ = O.impulse_pixel_sets(name, pvr)
    E, rec = _engine(name, pvr, options)
    if not options:                                                # the defaults are the cell scatter (support 16: with the table, written lazily)
        assert rec.get_option("back_mode") == 5 and rec.get_option("coeff_table") == (0 if pvr else 1) and rec.get_option("coeff_lazy") == 1
    act = _scatter_values(E, rec, name, 3.0)
    entries = twos = 0
    for k, s in enumerate(sets[:1] + sets):                        # (the first set twice: the pass that writes the table, and one that reads it)
        n, t = _scatter_set(E, rec, name, pvr, act, s, 3.0, (path, k - 1))
        entries, twos = entries + 2 * n * (k > 0), twos + 2 * t * (k > 0)
    _ran(rec, options, "backproject", len(sets) + 1, store, table, build, cells)
    if "cell_w" in dict(options):
        assert rec.cell_stats()["cell"] == (O.CELL["cell_w"], O.CELL["cell_h"])
    _scatter_values(E, rec, name, 1.5)
    _scatter_set(E, rec, name, pvr, act, sets[0], 1.5, (path, "e = 0.5"))
    assert not any(rec.fallbacks().values()), rec.fallbacks()
    print(f"scatter {name} support {O.support(pvr)} {path}: {len(sets)} sets, {sum(len(s) for s in sets)} impulse pixels, {entries} entries bit for bit "
          f"({twos} of them sums of two)")
    rec.close()


# ---- b. the gather ----------------------------------------------------------------------------------------------------------------
GATHER_PATHS = {
    False: {
        "cells-evaluated": ((("coeff_table", 0), ("fwd_mode", 2)), 0, False, False, None),
        "cells-table": ((("coeff_table", 1), ("fwd_mode", 2)), 1, True, False, None),         # writing, then reading
        "tiles-evaluated": ((("coeff_table", 0), LEGACY, ("fwd_mode", 1)), 0, False, False, None),
        "tiles-table": ((("coeff_table", 1), LEGACY, ("fwd_mode", 1)), 0, True, True, None),
        "pixels": ((("coeff_table", 0), LEGACY, ("fwd_mode", 0)), 0, False, False, None),
        "tiles-in-pieces": ((("coeff_table", 0), ("fwd_mode", 1)), 0, False, False, "48"),
        "defaults": ((), 1, True, False, None),
    },
    True: {
        "cells-evaluated": ((("coeff_table", 0), ("fwd_mode", 2)), 0, False, False, None),
        "cells-table": ((("coeff_table", 1), ("fwd_mode", 2)), 0, True, True, None),
        "tiles-evaluated": ((("coeff_table", 0), ("fwd_mode", 1)), 0, False, False, None),
        "pixels": ((("coeff_table", 0), ("pvr_mode", 0)), 0, False, False, None),
        "tiles-in-pieces": ((("coeff_table", 0), ("fwd_mode", 1)), 0, False, False, "48"),
        "defaults": ((), 0, False, False, None),
    },
}


def _gather(E, rec, name, volume):
    shape = O.problem(name).slices.shape
    rec.debug_set(E.BUF_RECONSTRUCTED, _f32(volume))
    rec.debug_set(E.BUF_SIMSLICES, np.zeros(shape, np.float32))
    rec.debug_set(E.BUF_SIMWEIGHTS, np.zeros(shape, np.float32))
    rec.debug_set(E.BUF_SIMINSIDE, np.zeros(shape, np.uint8))
    rec.SimulateSlices()
    return rec.debug_get(E.BUF_SIMSLICES), rec.debug_get(E.BUF_SIMWEIGHTS), rec.debug_get(E.BUF_SIMINSIDE)


@_with_paths(GATHER_PATHS)
def test_gather_entry_by_entry(case, path, monkeypatch):
    """b: one rounding chain per entry.  Each side rounds at most one division, one reciprocal and one product (2^-24 each), one term is
    exact, and the oracle's own product carries the same chain: k = 4.  The patch-based gather reads the volume through the eight-voxel
    average (visit_sim), an entry is then a sum of up to 8 non-negative terms: k = 8 + 4."""
    name, pvr = case
    options, store, table, build, piece = GATHER_PATHS[pvr][path]
    if piece:
        monkeypatch.setenv("SVR_FWD_PIECE", piece)
    k = 12 if pvr else 4
    sets, _ = O.impulse_voxel_sets(name, pvr)
    P = O.problem(name)
    act = P.slices != -1
    w_all, inside_all = O.gather_weights(name, pvr)
    E, rec = _engine(name, pvr, options)
    if not options:
        assert rec.get_option("fwd_mode") == 2
    rec.debug_set(E.BUF_PSF_SUMS, _f32(act))
    entries = 0
    for i, v in enumerate(sets[:1] + sets):
        sim, w, inside = _gather(E, rec, name, O.impulse_volume(name, v))
        want_sim, _, _, reach = O.expected_gather(name, pvr, v)
        got, want = sim.astype(np.float64) * w.astype(np.float64), want_sim.astype(np.float64) * w_all.astype(np.float64)
        worst = np.max(np.abs(got - want)[want != 0] / want[want != 0]) / O.U
        print(f"gather {name} support {O.support(pvr)} {path} set {i - 1}: {np.count_nonzero(want)} entries, worst {worst:.2f} u of {k}")
        bad = O.within_relative(got, want, k)
        assert not len(bad), (path, i - 1, O.describe(bad, got, want))
        assert np.count_nonzero(want) > 0 and not np.any(want[~reach])
        assert np.array_equal(inside, inside_all)
        assert rel_err(w, w_all) < TOL_SUM
        entries += np.count_nonzero(want) * (i > 0)
    _ran(rec, options, "forward", len(sets) + 1, store, table, build)
    if piece and name == "tiny":
        assert rec.counters()["Va"] // 32 > int(piece)              # more tiles than one piece holds, whatever their shape
    print(f"gather {name} support {O.support(pvr)} {path}: {len(sets)} sets, {sum(len(s) for s in sets)} impulse voxels, {entries} entries within {k} u")
    rec.close()


# ---- c. the Gaussian reconstruction's passes 1 and 2 ------------------------------------------------------------------------------
@each_case
@pytest.mark.parametrize("gauss_mode", [1, 0])
def test_gaussian_passes_entry_by_entry(case, gauss_mode):
    """c: the set's pixels hold 512.0 and every other pixel is padding.  Pass 2 adds tap / psf_sums (one rounded division) to the volume
    weights and 512 times that (exact) to the volume, at most two terms a voxel (one rounded sum): against the taps over the DEVICE's own
    psf_sums in float64, 3 * 2^-24 holds both.  Pass 1 apart: the same pixels pass its gate, psf_sums to 1e-6 as in the parity tests."""
    name, pvr = case
    from fetalreconstruction_amd import engine as E
    sets, _ = O.impulse_pixel_sets(name, pvr)
    P = O.problem(name)
    entries = 0
    for i, s in enumerate(sets):
        Q = O.padded(name, O.indicator(name, s), 512.0)
        rec = E.Reconstruction(0)
        if pvr:
            rec.set_option("pvr", 1)
            E.sync_gpu(rec, Q, quality_factor=1.0)
        else:
            E.sync_gpu(rec, Q)
        rec.timer_enable(True)
        rec.set_option("gauss_mode", gauss_mode)
        ones = np.ones(P.ns, np.float32)
        rec.UpdateScaleVector(ones, ones)
        rec.GaussianReconstructionLocal()
        psf_sums, volw, recon, voxcount = O.expected_gauss(name, pvr, s)
        ps = rec.debug_get(E.BUF_PSF_SUMS)
        assert np.array_equal(ps != 0, psf_sums != 0) and np.count_nonzero(ps) > 0
        assert np.allclose(ps, psf_sums, rtol=1e-6, atol=0)
        assert np.array_equal(rec.debug_get(E.BUF_VOXEL_COUNT), voxcount) and voxcount.sum() > 0
        got_w = rec.getVolWeights()
        want = O.gauss_from_taps(name, pvr, s, ps)
        worst = np.max(np.abs(got_w - want)[want != 0] / want[want != 0]) / O.U
        print(f"gauss {name} support {O.support(pvr)} mode {gauss_mode} set {i}: {np.count_nonzero(want)} entries, worst {worst:.2f} u of 3, "
              f"{len(O.same_bits(ps, psf_sums))} psf_sums differ from the oracle's in bits")
        assert np.array_equal(got_w != 0, volw != 0)                       # the footprint
        bad = O.within_relative(got_w, want, 3)
        assert not len(bad), (gauss_mode, i, O.describe(bad, got_w, want))
        got_r = rec.debug_get(E.BUF_RECONSTRUCTED)                           # (not equalised: GaussianReconstructionLocal stops before)
        bad = O.within_relative(got_r, 512.0 * want, 3)
        assert not len(bad), (gauss_mode, i, "volume", O.describe(bad, got_r, 512.0 * want))
        assert rec.get_option("gauss_mode") == gauss_mode and not any(rec.fallbacks().values()) and rec.timers()["gauss"][1] == 1
        entries += np.count_nonzero(want)
        rec.close()
    print(f"gauss {name} support {O.support(pvr)} mode {gauss_mode}: {len(sets)} sets, {sum(len(s) for s in sets)} impulse pixels, {entries} entries within 3 u")


# ---- d. dense passes, a bound per element -----------------------------------------------------------------------------------------
@each_case
def test_dense_passes_with_a_bound_per_element(case):
    """d: impulses cannot show cross-talk between live neighbours.  Every element of a dense pass within (n + 6) 2^-24 S of the oracle: n =
    an upper bound on its terms (a voxel: the pixels whose footprint box holds it; a pixel: the taps of a footprint), S = the sum of the
    terms' magnitudes (want itself where no term is negative; for addon the oracle's scatter of |e|).  Recursive summation in any order,
    atomics included, loses at most (n - 1) u sum|terms|; the product orders of the two sides differ by at most 6 roundings per term.
    The 2e-5 of the parity tests is asserted beside it."""
    name, pvr = case
    want = O.expected_dense(name, pvr)
    n_v = O.terms_bound(name, pvr)
    n_p = O.support(pvr) ** 3 * (8 if pvr else 1)
    P = O.problem(name)
    E, rec = _engine(name, pvr, ())
    rec.InitializeEMValues()
    rec.GaussianReconstructionLocal()
    ps = rec.debug_get(E.BUF_PSF_SUMS)
    assert np.array_equal(ps != 0, want["psf_sums"] != 0) and np.allclose(ps, want["psf_sums"], rtol=1e-6, atol=0)
    assert np.array_equal(rec.debug_get(E.BUF_VOXEL_COUNT), want["voxcount"])
    report = []

    def check(what, got, ref, n, magnitude=None, tol=TOL_SUM):
        bad = O.within_terms(got, ref, n, magnitude)
        s = np.abs(np.asarray(ref, np.float64).reshape(-1)) if magnitude is None else np.asarray(magnitude, np.float64).reshape(-1)
        d = np.abs(np.asarray(got, np.float64).reshape(-1) - np.asarray(ref, np.float64).reshape(-1))
        nn = np.broadcast_to(np.asarray(n, np.float64).reshape(-1), d.shape) + 6
        worst = float(np.max(d[s > 0] / (nn[s > 0] * O.U * s[s > 0])))
        report.append(f"{what} {np.count_nonzero(s)} elements, worst {worst:.3f} of its bound, rel_err {rel_err(got, ref):.2g}")
        print(f"dense {name} support {O.support(pvr)}: {report[-1]}")
        assert not len(bad), (what, O.describe(bad, got, ref))
        assert rel_err(got, ref) < tol

    volw = rec.getVolWeights()
    assert np.array_equal(volw > 0, want["volw"] > 0)
    check("volw", volw, want["volw"], n_v)
    check("recon", rec.syncCPU(), want["recon"], n_v)
    rec.debug_set(E.BUF_PSF_SUMS, want["psf_sums"])
    sim, w, inside = _gather(E, rec, name, want["volume"])
    assert np.array_equal(inside, want["siminside"])
    check("simweights", w, want["simweights"], n_p)
    check("simslices * simweights", sim.astype(np.float64) * w.astype(np.float64),
          want["simslices"].astype(np.float64) * want["simweights"].astype(np.float64), n_p)
    assert rel_err(sim, want["simslices"]) < TOL_SUM
    wts, ss, sw = O.dense_inputs(name)
    rec.debug_set(E.BUF_WEIGHTS, wts)
    rec.debug_set(E.BUF_SIMSLICES, ss)
    rec.SuperresolutionBackproject(sw)
    cm, ad = rec.debug_get(E.BUF_CONFIDENCE_MAP), rec.debug_get(E.BUF_ADDON)
    assert np.array_equal(cm > 0, want["cmap"] > 0)
    check("cmap", cm, want["cmap"], n_v)
    check("addon", ad, want["addon"], n_v, magnitude=want["addon_abs"])
    assert not any(rec.fallbacks().values()), rec.fallbacks()
    rec.close()
