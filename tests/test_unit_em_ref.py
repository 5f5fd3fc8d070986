"""The numpy restatement of the device's unit-level EM (tests/unit_em_ref.py) against the CPU oracle and the host form, and the
conditions the shared cases (tests/unit_em_cases.py) must meet so that tests/test_unit_em_gpu.py can ask the device for bits.
No engine, no GPU.  Run with -s for the measured figures ("The unit-level EM, checked directly")."""
import math

import numpy as np
import pytest

from tests import unit_em_cases as K
from tests import unit_em_ref as R
from tests.test_unit_em_cpu import driver, run_unit_em   # noqa: F401  (the g++ driver of tests/unit_em_check.cpp, a fixture)

STEP = K.STEP
SLICE = [k for k, c in K.CASES.items() if c["form"] == "slice"]
PATCH = [k for k, c in K.CASES.items() if c["form"] == "patch"]
SCALARS = ("mean_s", "mean_s2", "sigma_s", "sigma_s2", "mix_s")


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _cut(name):
    """the old cases as they are, the 200 204-unit one cut to 2 204 (the restatement's weight loop is a Python loop)"""
    pot, w, scale, fe, small, st = K.SLICE_CASES[name]
    if len(pot) > 100000:
        keep = np.r_[0:200, 200:2200, len(pot) - 4:len(pot)]
        pot, w, scale = pot[keep], w[keep], scale[keep]
    return pot, w, scale, fe, small, st


@pytest.mark.parametrize("name", list(K.SLICE_CASES))
def test_serial_slice_form_is_the_oracle_on_the_host_forms_cases(oracle_mod, name):
    pot, w, scale, fe, small, st = _cut(name)
    excl = np.zeros(len(pot), np.uint8)
    excl[fe] = 1
    excl[small] = 1
    p, wt, c = R.unit_em(pot, w, scale, excl, STEP, np.float32(st), "slice", "serial")
    op, ow, ost = oracle_mod.host_estep(pot, w, scale, fe, small, STEP, np.float32(st))
    assert np.array_equal(_bits(p), _bits(op)) and np.array_equal(_bits(wt), _bits(ow)) and np.array_equal(_bits(c), _bits(ost)), (name, c, ost)


@pytest.mark.parametrize("name", SLICE)
def test_serial_slice_form_is_the_oracle_bit_for_bit(oracle_mod, name):
    """the oracle in the reference's numbering, the restatement in the host's with by_ref: the same bits, unit by unit"""
    c = K.CASES[name]
    p, wt, st = K.restate(c, "serial")
    pot, w, scale, excl, _ = K.reference_view(c)
    op, ow, ost = oracle_mod.host_estep(pot, w, scale, np.flatnonzero(excl), [], STEP, c["state5"])
    br = c["by_ref"]
    assert np.array_equal(_bits(p[br]), _bits(op)) and np.array_equal(_bits(wt[br]), _bits(ow)), name
    assert np.array_equal(_bits(st), _bits(ost)), (name, st, ost)


@pytest.mark.parametrize("name", PATCH)
def test_serial_patch_form_against_the_host_form(driver, tmp_path, name):   # noqa: F811
    """unit_em of csrc/svr_unit_em.h with the float Gaussian, at tests/test_unit_em_cpu.py's tolerances (glibc's expf against numpy's)"""
    c = K.CASES[name]
    p, wt, st = K.restate(c, "serial", "f32")
    pot, w, scale, excl, _ = K.reference_view(c)
    counts = [int(x) for x in name.split("[")[1].split("]")[0].split(",")]
    hp, hw, hc = run_unit_em(driver, tmp_path, 1, pot, w, scale, excl, np.float32(0.0001) * np.float32(0.0001) / 6.28, c["state5"], counts)
    br = c["by_ref"]
    assert np.array_equal(p[br], hp), name
    assert np.allclose(wt[br], hw, atol=1e-4), np.abs(wt[br] - hw).max()
    assert np.allclose(st, hc, rtol=1e-5), (st, hc)
    src = R.src_host(c["src_ref"], br)
    assert (src == -1).any() and (src[src >= 0] != np.flatnonzero(src >= 0)).any()        # -1 and cross-references both occur


def test_tree_order_is_within_one_ulp_of_the_serial_order():
    """the five scalars of k_slice_em's order against the reference's: at most 1 float32 ulp (double sums of <= 7503 terms differ by
    ~1e-13 relative before one rounding to float); where the case puts potentials on a mean on purpose, the same bits"""
    worst = dict.fromkeys(SCALARS, 0)
    w_worst = 0
    for name, c in K.CASES.items():
        _, ws, ss = K.restate(c, "serial")
        _, wt, st = K.restate(c, "tree256")
        d = R.ulp_diff(ss, st)
        for k, s in enumerate(SCALARS):
            worst[s] = max(worst[s], int(d[k]))
        w_worst = max(w_worst, int(R.ulp_diff(ws, wt).max()))
        assert d.max() <= 1, (name, ss, st)
        for k in c["at_mean"]:                                       # a mean the case puts potentials on: the same bits
            assert d[int(k) - 1] == 0, (name, ss, st)
    print("\ntree256 vs serial, largest float32 ulp distance over", len(K.CASES), "cases:", worst, "weights:", w_worst)


def test_tree_sums_against_fsum():
    worst = 0.0
    for name, c in K.CASES.items():
        src = None if c["src_ref"] is None else R.src_host(c["src_ref"], c["by_ref"])
        p = R.apply_exclusions(c["pot"], c["scale"], c["excl"], src)
        sums = R.class_scalars(p, c["w"], c["by_ref"], c["form"], STEP, "tree256")[5]
        for k, (terms, take) in sums["terms"].items():
            exact = math.fsum(terms[take].tolist())
            err = abs(float(sums[k]) - exact) / exact if exact else abs(float(sums[k]))
            worst = max(worst, err)
            assert err <= 1e-12, (name, k, float(sums[k]), exact)
    print("\ntree256 sums vs math.fsum, largest relative difference:", worst)


@pytest.mark.parametrize("name", list(K.CASES))
def test_case_conditions(name):
    """No decision may hinge on an exp in the subnormal range or on the last bit of a mean: every exponent argument is below 600
    or above 900 (patch form, float Gaussian: below 60 or above 900), and no potential lies within 16 float ulps of a class mean
    unless the case puts it there on purpose (at_mean names that mean; the other one is still checked).  For the first run and for
    the second, which starts from the first's weights and mix_s (tests/test_unit_em_gpu.py runs both)."""
    c = K.CASES[name]
    src = None if c["src_ref"] is None else R.src_host(c["src_ref"], c["by_ref"])
    p = R.apply_exclusions(c["pot"], c["scale"], c["excl"], src)
    w, mix = c["w"], c["state5"][4]
    for run in (1, 2):
        m1, m2, s1, s2, den, _ = R.class_scalars(p, w, c["by_ref"], c["form"], STEP, "serial")
        _, args, _ = R.unit_weights(p, w, m1, m2, s1, s2, mix, den, c["form"], STEP, "f64")
        a = args[np.isfinite(args)]
        low = 600.0 if c["form"] == "slice" else 60.0
        assert ((a < low) | (a > 900.0)).all(), (name, run, a[(a >= low) & (a <= 900.0)])
        if run == 1 and name.startswith(("mixed", "patch", "scales", "potentials", "likelihood", "order")) and c["n"] > 1:
            assert a.size > 0, name                                  # these must reach the Gaussians
        take = p >= 0
        # (one class, mean_s2 <= mean_s or no inlier weight: every weight is 1 and no potential is compared with a mean)
        if take.any() and not (den <= 0 or m2 <= m1):
            for k, m in (("1", m1), ("2", m2)):
                if k not in c["at_mean"]:
                    d = R.ulp_diff(p[take], np.full(int(take.sum()), m, np.float32))
                    assert d.min() > 16, (name, run, k, m, d.min())
        _, w, st = K.restate(c, "tree256", "f32", runs=run)
        mix = st[4]
    assert c["rlo"][c["rank"] + 1] > c["rlo"][c["rank"]]             # svr_slice_em_setup needs a unit on the rank under test
    assert sorted(c["by_ref"].tolist()) == list(range(c["n"]))


def test_the_branches_are_reached():
    """each named branch case does what its name says, in the restatement (so the device test that passes on it checked that branch)"""
    for n in (257, 513):
        g = lambda s: K.restate(K.CASES[f"{s} @ {n}"], "tree256")   # noqa: E731
        p, w, st = g("all excluded")
        assert (p == -1).all() and (w == 0).all() and st[4] == np.float32(0.9)
        p, w, st = g("every weight 0 (den == 0)")
        assert (w[p >= 0] == 1).all() and st[0] == p[p >= 0].min()
        p, w, st = g("every weight 1 (den2 == 0)")
        assert st[1] == np.float32((float(p.max()) + float(st[0])) / 2.0)
        p, w, st = g("mean_s2 <= mean_s")
        assert st[1] <= st[0] and (w == 1).all()
        p, w, st = g("sum == 0: sigma_s = 0.025f")
        assert st[2] == np.float32(0.025) and st[3] == np.float32((st[1] - st[0]) * (st[1] - st[0]) / np.float32(4))
        p, w, st = g("both variances at the floor")
        assert st[2] == st[3] == np.float32(STEP * STEP / 6.28)
        p, w, st = g("likelihood == 0 by mix_s == 1")
        assert (p >= st[1]).sum() > 10 and (w[p >= st[1]] == 0).all() and (w[(p >= 0) & (p < st[1])] == 1).all()
        p, w, st = g("likelihood == 0 by mix_s == 0")
        assert ((p >= 0) & (p <= st[0])).sum() > 10 and (w[(p >= 0) & (p <= st[0])] == 1).all() and (w[p > st[0]] == 0).all()
        for mix in (1, 0):                                           # all three positions take the likelihood == 0 branch
            c = K.CASES[f"likelihood == 0: below, between, above (mix_s == {mix}) @ {n}"]
            p, w, st = K.restate(c, "tree256")
            far = c["by_ref"][-3:]                                   # the reference's last three units: 0.0, 0.5, 1.3
            assert p[far].tolist() == [0.0, 0.5, np.float32(1.3)] and p[far[0]] < st[0] < p[far[1]] < st[1] < p[far[2]]
            wr, _, exact = R.unit_weights(p, c["w"], st[0], st[1], st[2], st[3], c["state5"][4], 1.0, "slice", STEP)
            decides = (st[0], st[2]) if mix else (st[1], st[3])      # the Gaussian that mix_s leaves in the likelihood: 0 at all three
            assert all(R.gauss_slice(np.float32(x - decides[0]), decides[1], STEP) == 0 for x in p[far])
            assert w[far].tolist() == [1.0, 1.0, 0.0] and exact[far].all()
        c = K.CASES[f"scales at 0.2f, 5.0f, 0.19999f, 5.0001f @ {n}"]
        p, w, st = K.restate(c, "tree256")
        first8 = p[R.order_of(c["by_ref"]) < 8][np.argsort(R.order_of(c["by_ref"])[R.order_of(c["by_ref"]) < 8])]
        assert ((first8 == -1) == np.array([0, 0, 1, 1, 0, 0, 1, 1], bool)).all(), first8
    c = K.CASES["likelihood == 0: below, between, above @ 7503"]
    p, w, st = K.restate(c, "tree256")
    far = c["by_ref"][-3:]                                           # the reference's last three units: 0.0, 0.5, 1.3
    assert p[far].tolist() == [0.0, 0.5, np.float32(1.3)] and st[0] < 0.5 < st[1] < 1.3
    g = lambda x, m, s: R.gauss_slice(np.float32(x - m), s, STEP)   # noqa: E731
    assert all(g(x, st[0], st[2]) == 0 and g(x, st[1], st[3]) == 0 for x in p[far])
    assert w[far].tolist() == [1.0, 1.0, 0.0]


def test_patch_gauss_gap_is_measured():
    """float32 Gaussian against the same Gaussian in float64, in weights: the yardstick of the device's patch form"""
    gap = K.patch_gauss_gap()
    print("\npatch form, float32-flavour weights vs float64-flavour weights, largest gap over the patch cases: %.3e" % gap)
    assert 0 < gap < 1e-4                                            # (tests/test_unit_em_cpu.py's tolerance for the same difference)


def test_unpack_walks_over_empty_ranks_and_combine_ranks():
    for c in (K.CASES["mixed 255"], K.CASES["mixed 257"], K.CASES["mixed 513"]):
        maxn = R.max_count(c["rlo"])
        recv = R.pack(c["pot"], c["scale"], c["inside"], c["world"], c["rlo"], maxn)
        raw, sc, ins = R.unpack(recv, c["world"], c["rlo"], maxn, c["n"])
        assert np.array_equal(_bits(raw), _bits(c["pot"])) and np.array_equal(sc, c["scale"]) and np.array_equal(ins, c["inside"])
    a = np.arange(24, dtype=np.float64).reshape(3, 8)
    a[1, 3], a[1, 4] = np.inf, -np.inf
    s5 = R.combine_ranks(a, 3)
    assert s5.tolist() == [0 + 8 + 16, 1 + 9 + 17, 2 + 10 + 18, 3.0, 20.0]
    # mstep_scalars: the clamps (slices only), mix > 0, the floor, iter > 1
    f = np.float32
    sg, mx, m = R.mstep_scalars([8.0, 2.0, 4.0, -3.0, 5.0], 2, 0.0001, 0, 9.0, 0.5)
    assert (sg, mx, m) == (f(4), f(0.5), f(0.125))
    sg, mx, m = R.mstep_scalars([8.0, 0.0, 4.0, np.inf, 1e-40], 1, 0.0001, 0, 1e-12, 0.25)
    assert sg == f(f(0.0001) * f(0.0001) / f(6.28)) and mx == f(0.25) and m == f(1) / (R.FLT_MIN - R.FLT_MAX)
    sg, mx, m = R.mstep_scalars([8.0, 0.0, 4.0, np.inf, 1e-40], 1, 0.0001, 1, 9.0, 0.25)
    assert sg == f(9) and m == 0 and mx == f(0.25)                   # patches: no clamps, 1 / (1e-40f - inf) = -0


def test_the_order_sensitive_case_tells_the_visit_orders_apart():
    """mean_s in the 256-thread order over by_ref (and in the serial order) is the tie rounded to even; over the host order 0, 1, 2, ..
    -- what a first pass that forgot by_ref would add -- it is one ulp higher"""
    c = K.CASES["order-sensitive mean @ 768"]
    p = R.apply_exclusions(c["pot"], c["scale"], c["excl"])
    right = R.class_scalars(p, c["w"], c["by_ref"], "slice", STEP, "tree256")
    wrong = R.class_scalars(p, c["w"], np.arange(c["n"]), "slice", STEP, "tree256")
    assert right[5]["den"] == 4.0 and right[5]["sum"] == 1.0 + 2.0 ** -24 and wrong[5]["sum"] == 1.0 + 2.0 ** -24 + 2.0 ** -52
    assert int(_bits(right[0])) + 1 == int(_bits(wrong[0])) and right[0] == np.float32(0.25)


def test_the_order_sensitive_variance_case_tells_the_visit_orders_apart():
    """the same for the second pass: sigma_s over by_ref is the tie 2^-6 (1 + 2^-24) rounded to even, over the host order one ulp higher"""
    c = K.CASES["order-sensitive variance @ 768"]
    p = R.apply_exclusions(c["pot"], c["scale"], c["excl"])
    right = R.class_scalars(p, c["w"], c["by_ref"], "slice", STEP, "tree256")
    wrong = R.class_scalars(p, c["w"], c["by_ref"], "slice", STEP, "tree256", by_ref2=np.arange(c["n"]))
    assert right[5]["vden"] == 8.0 and right[5]["vsum"] == 2.0 ** -3 * (1 + 2.0 ** -24) and wrong[5]["vsum"] == 2.0 ** -3 * (1 + 2.0 ** -24) + 2.0 ** -55
    assert right[0] == wrong[0] == np.float32(0.5) and right[2] == np.float32(2.0 ** -6)
    assert int(_bits(right[2])) + 1 == int(_bits(wrong[2]))
