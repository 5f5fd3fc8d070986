"""Named inputs of the unit-level EM, shared by the CPU tests (tests/test_unit_em_cpu.py: the host form; tests/test_unit_em_ref.py: the
numpy restatement) and the device tests (tests/test_unit_em_gpu.py: k_slice_em).  Each case is a plain dict of arrays in the HOST
numbering:

  form "slice" | "patch", n, pot (raw potentials, as the ranks send them), w, scale, inside, excl (uint8), state5 (float32),
  by_ref (host index of the unit with reference index k), world, rank, rlo (the ranks' ranges), src_ref (patch form: the
  reference-numbered source map, or None), at_mean (the case puts potentials exactly on a class mean on purpose)

at_mean names the class means ("1": mean_s, "2": mean_s2, "12": both) that the case puts potentials on, or next to, on purpose.

likelihood == 0.  With 0 < mix_s < 1 a unit between the classes has likelihood 0 only if BOTH Gaussians underflow at it; it takes
part in both variances itself (weights w and 1 - w), so var_c >= w_c d^2 / N_c and that needs more than ~1490 units: that form runs
once, at 7503 units.  With mix_s exactly 1 the likelihood is gs1 * 1 + gs2 * 0: far units of weight 0 take no part in the inliers'
variance, two tight classes make gs1 underflow at them, and all three positions (below -> 1, between -> 1, above -> 0) are reached
at any size; with mix_s exactly 0 and far units of weight 1 the mirror image.  Those run at 257 and 513.

The order of the sums.  Sums of positive terms of one magnitude round to the same float in any order, so the other cases cannot tell
by_ref from another permutation; "order-sensitive mean @ 768" (first pass) and "order-sensitive variance @ 768" (second pass) can:
their sums sit on a float tie that two sub-ulp terms break only when they meet each other in one thread before they meet the large
terms (see _order_sensitive, _order_sensitive_variance).  The mixing sum cannot be put on a tie: its terms are computed weights.
"""
import numpy as np

from tests import unit_em_ref as R

STEP = 0.0001
F32 = np.float32


# ---- the builders of tests/test_unit_em_cpu.py (moved here unchanged) -------------------------------------------------------
def _case(rng, n, p_scale_out=0.1):
    pot = rng.uniform(0.0, 1.0, n).astype(np.float32)
    w = rng.uniform(0.0, 1.0, n).astype(np.float32)
    scale = rng.uniform(0.5, 2.0, n).astype(np.float32)
    out = rng.random(n) < p_scale_out
    scale[out] = rng.choice(np.float32([0.0, 0.1, 0.19999, 5.0001, 7.0]), int(out.sum()))
    return pot, w, scale


def _slice_cases():
    rng = np.random.default_rng(20261015)
    cases = {}
    pot, w, scale = _case(rng, 64)
    scale[:4] = np.float32([0.2, 5.0, 0.19999, 5.0001])             # the bounds themselves take part
    cases["mixed, scales outside [0.2, 5], force-excluded and small slices"] = (pot, w, scale, [3, 17, 40], [8, 9], [0.3, 0.6, 0.02, 0.03, 0.8])
    pot, w, scale = _case(rng, 20, 0.0)
    cases["all units excluded"] = (pot, w, scale, list(range(10)), list(range(10, 20)), [0, 0, 0.02, 0.03, 0.8])
    pot, w, scale = _case(rng, 30, 0.0)
    cases["den2 == 0 (every weight 1)"] = (pot, np.ones(30, np.float32), scale, [2], [], [0, 0, 0.02, 0.03, 0.9])
    pot, w, scale = _case(rng, 30, 0.0)
    cases["weights 0: den == 0"] = (pot, np.zeros(30, np.float32), scale, [], [], [0, 0, 0.02, 0.03, 0.9])
    pot = np.linspace(0.1, 0.9, 40).astype(np.float32)
    w = (pot > 0.5).astype(np.float32)                               # the high potentials weigh as inliers: mean_s2 <= mean_s
    cases["mean_s2 <= mean_s"] = (pot, w, np.ones(40, np.float32), [], [], [0, 0, 0.02, 0.03, 0.7])
    # two tight classes and units far from both: the Gaussians underflow, likelihood == 0
    pot = np.concatenate([np.full(200, 0.1), np.full(200000, 0.9), [0.5, 0.7, 3.0, 0.0]]).astype(np.float32)
    w = np.concatenate([np.ones(200), np.zeros(200000), [1e-7, 0.0, 0.0, 1.0]]).astype(np.float32)
    cases["likelihood == 0"] = (pot, w, np.ones(len(pot), np.float32), [], [], [0, 0, 0.02, 0.03, 0.5])
    for k in range(3):
        pot, w, scale = _case(rng, 300)
        pot[rng.random(300) < 0.05] = -1                             # potentials the engine marked
        fe = sorted(rng.choice(300, 6, replace=False).tolist())
        cases[f"seeded {k}"] = (pot, w, scale, fe, [], rng.uniform(0, 1, 5).tolist())
    return cases


SLICE_CASES = _slice_cases()


# ---- numberings and shardings ------------------------------------------------------------------------------------------------
def numbering(kind, n, seed=0):
    if kind == "identity":
        return np.arange(n, dtype=np.int32)
    if kind == "reversed":
        return np.arange(n, dtype=np.int32)[::-1].copy()
    return np.random.default_rng(1000 + seed).permutation(n).astype(np.int32)


def sharding(world, n):
    """(world, the rank under test, rlo): the rank under test always holds at least one unit"""
    if world == 1:
        return 1, 0, [0, n]
    if world == 3:                                   # an empty rank in the middle
        a = min(100, n - 1)
        return 3, 2, [0, a, a, n]
    if world == 4:                                   # very uneven: maxn much larger than this rank's count
        assert n >= 48
        return 4, 0, [0, 5, n - 40, n - 1, n]
    assert world == 8 and n >= 7                     # the first rank empty
    return 8, 7, [0, 0] + [int(round(n * k / 7.0)) for k in range(1, 7)] + [n]


def _finish(name, form, pot, w, scale, excl, state5, by_ref="identity", world=1, src_ref=None, at_mean="", seed=0, inside=None):
    """the arrays are given in the REFERENCE's numbering (the builders' own); the case holds them in the host numbering"""
    n = len(pot)
    br = numbering(by_ref, n, seed) if isinstance(by_ref, str) else np.asarray(by_ref, np.int32)
    host = lambda v, dt: np.ascontiguousarray(np.asarray(v, dt)[R.order_of(br)])   # noqa: E731  host unit k = reference unit order[k]
    e = np.zeros(n, np.uint8)
    e[np.asarray(excl, np.int64)] = 1
    if inside is None:
        inside = (np.arange(n) % 3 != 1).astype(np.float32)
    wd, rank, rlo = sharding(world, n)
    return dict(name=name, form=form, n=n, pot=host(pot, F32), w=host(w, F32), scale=host(scale, F32), inside=host(inside, F32),
                excl=host(e, np.uint8), state5=np.asarray(state5, F32), by_ref=br, world=wd, rank=rank, rlo=[int(x) for x in rlo],
                src_ref=None if src_ref is None else np.asarray(src_ref, np.int32), at_mean=at_mean)


def _two(rng, n, p_scale_out=0.1):
    """_case with weights that fall with the potential, so that mean_s < mean_s2 and the Gaussians are reached"""
    pot, w, scale = _case(rng, n, p_scale_out)
    w = ((1 - pot) * rng.uniform(0.5, 1.0, n)).astype(np.float32)
    return pot, w, scale


def _mixed(rng, n):
    pot, w, scale = _two(rng, n)
    if n >= 16:
        pot[rng.random(n) < 0.05] = -1
        fe = sorted(rng.choice(n, max(1, n // 50), replace=False).tolist())
    else:
        fe = []
        scale[:] = 1
    st = [0, 0, 0.02, 0.03, float(F32(rng.uniform(0.2, 0.9)))]
    return pot, w, scale, fe, st


def _grid(n, centre):
    """n potentials in two even runs, centre - 5e-4 .. - 2e-4 and centre + 2e-4 .. + 5e-4: the class mean falls into the gap, in the
    first run and in the second (when a far unit or two have changed class)"""
    k = 3e-4 * np.arange(n // 2) / (n // 2)
    return np.concatenate([centre - 5e-4 + k, centre + 2e-4 + k]).astype(np.float32)


def _branch_cases(n, rng):
    """every branch of the EM at n units -> {name: (pot, w, scale, excluded, state5, at_mean)}"""
    out = {}
    ones = np.ones(n, np.float32)
    pot, w, scale = _case(rng, n, 0.0)
    scale[1::2] = np.float32(0.1)                                    # the other half by their scales
    out["all excluded"] = (pot, w, scale, list(range(0, n, 2)), [0, 0, 0.02, 0.03, 0.8], "")
    pot, w, scale = _case(rng, n, 0.0)
    out["every weight 1 (den2 == 0)"] = (pot, ones.copy(), scale, [2], [0, 0, 0.02, 0.03, 0.9], "")
    pot, w, scale = _case(rng, n, 0.0)
    out["every weight 0 (den == 0)"] = (pot, np.zeros(n, np.float32), scale, [], [0, 0, 0.02, 0.03, 0.9], "1")   # mean_s = the least potential
    pot = np.linspace(0.1, 0.9, n).astype(np.float32)
    w = (pot > 0.5).astype(np.float32)                               # the high potentials weigh as inliers
    w[-1], w[0] = 0.5, 0.25                                          # (and the means fall between the grid's potentials,
    pot[0] = np.float32(0.13)                                        # in the second run too, where every weight is 1)
    out["mean_s2 <= mean_s"] = (pot, w, ones.copy(), [], [0, 0, 0.02, 0.03, 0.7], "")
    # likelihood == 0 from outside the classes (see the module's text): mix_s exactly 1 and exactly 0
    for mix in (1.0, 0.0):
        pot, w, scale = _two(rng, n, 0.0)
        out[f"likelihood == 0 by mix_s == {mix:g}"] = (pot, w, scale, [5], [0, 0, 0.02, 0.03, mix], "")
    # ... and all three positions at once: two tight classes, far units below, between and above them whose weight keeps them out
    # of the variance of the class whose Gaussian decides (mix_s 1: gs1, far weights 0; mix_s 0: gs2, far weights 1)
    h = 2 * ((n - 3) // 6)
    for mix in (1.0, 0.0):
        pot = np.concatenate([_grid(h, 0.1), _grid(n - 3 - h, 0.9), [0.0, 0.5, 1.3]]).astype(np.float32)
        w = np.concatenate([np.ones(h), np.zeros(n - 3 - h), np.full(3, 1.0 - mix)]).astype(np.float32)
        out[f"likelihood == 0: below, between, above (mix_s == {mix:g})"] = (pot, w, ones.copy(), [], [0, 0, 0.02, 0.03, mix], "")
    # identical potentials within each class, weights 1 and 0: both variances are 0 -> 0.025f for the inliers (sum == 0), and
    # (mean_s2 - mean_s)^2 / 4 for the outliers
    h = n // 3
    pot = np.concatenate([np.full(h, 0.25), np.full(n - h, 0.75)]).astype(np.float32)
    w = np.concatenate([np.ones(h), np.zeros(n - h)]).astype(np.float32)
    out["sum == 0: sigma_s = 0.025f"] = (pot, w, ones.copy(), [], [0, 0, 0.02, 0.03, 0.6], "12")
    # both class variances at the floor: identical potentials within a class but for one unit an ulp off, so that both sums
    # are positive and tiny
    pot = np.concatenate([np.full(h, 0.25), np.full(n - h, 0.75)]).astype(np.float32)
    pot[0] = np.nextafter(np.float32(0.25), np.float32(1))
    pot[-1] = np.nextafter(np.float32(0.75), np.float32(1))
    out["both variances at the floor"] = (pot, w.copy(), ones.copy(), [], [0, 0, 0.02, 0.03, 0.6], "12")
    pot, w, scale = _two(rng, n, 0.0)
    scale[:8] = np.float32([0.2, 5.0, 0.19999, 5.0001, 0.2, 5.0, 0.19999, 5.0001])
    out["scales at 0.2f, 5.0f, 0.19999f, 5.0001f"] = (pot, w, scale, [], [0, 0, 0.02, 0.03, 0.8], "")
    pot, w, scale = _two(rng, n, 0.0)
    pot[rng.random(n) < 0.3] = -1
    pot[[0, n - 1, 255 % n, 256 % n]] = -1
    out["potentials of exactly -1 from the engine"] = (pot, w, scale, [], [0, 0, 0.02, 0.03, 0.8], "")
    return out


def _likelihood_zero_big():
    """2500 inliers around 0.1, 5000 outliers around 0.9 and three units far from both: 0.0 (below, weight 1), 0.5 (between, weight
    0) and 1.3 (above, weight 0).  var ~ 0.01 / 2501, var2 ~ 0.32 / 5002: every far unit's exponent argument is above 1200."""
    pot = np.concatenate([_grid(2500, 0.1), _grid(5000, 0.9), [0.0, 0.5, 1.3]]).astype(np.float32)
    w = np.concatenate([np.ones(2500), np.zeros(5000), [1.0, 0.0, 0.0]]).astype(np.float32)
    return pot, w, np.ones(len(pot), np.float32), [], [0, 0, 0.02, 0.03, 0.5]


def _order_sensitive(n=768):
    """A case whose mean_s depends on the ORDER of the first pass's sum.  Reference units 0, 256, 512 (one thread of the 256 in the
    visit order) hold 1.0, 3 x 2^-55, 3 x 2^-55 with weight 1: each tiny term alone is under half an ulp of 1.0 and is absorbed.
    Reference unit 1 holds 2^-24, weight 1; every other unit 0.9 with weight 0, so den = 4 and sum = 1 + 2^-24 exactly: a float tie,
    to even.  by_ref puts the two tiny units on host indices 5 and 261: visited in HOST order they meet each other first (thread 5),
    make 0.75 ulp and carry through the tree: sum = 1 + 2^-24 + 2^-52, above the tie.  Asserted here, not assumed."""
    pot = np.full(n, 0.9)
    w = np.zeros(n, np.float32)
    pot[[0, 256, 512, 1]] = [1.0, 3 * 2.0 ** -55, 3 * 2.0 ** -55, 2.0 ** -24]
    w[[0, 256, 512, 1]] = 1
    rest = np.random.default_rng(768).permutation([k for k in range(n) if k not in (0, 5, 261)])
    br = np.empty(n, np.int32)
    br[0], br[256], br[512] = 0, 5, 261
    br[[k for k in range(n) if k not in (0, 256, 512)]] = rest
    c = _finish(f"order-sensitive mean @ {n}", "slice", pot, w, np.ones(n, np.float32), [], [0, 0, 0.02, 0.03, 0.7], br, 3, at_mean="2")
    p = R.apply_exclusions(c["pot"], c["scale"], c["excl"])
    right = R.class_scalars(p, c["w"], c["by_ref"], "slice", STEP, "tree256")[0]
    wrong = R.class_scalars(p, c["w"], np.arange(n), "slice", STEP, "tree256")[0]
    serial = R.class_scalars(p, c["w"], c["by_ref"], "slice", STEP, "serial")[0]
    assert right == serial and R.ulp_diff(right, wrong)[0] == 1, (right, wrong, serial)
    return c


def _order_sensitive_variance(n=768):
    """The same for the SECOND pass: sigma_s depends on the order of sum((pot - mean_s)^2 w).  Around mean_s = 0.5 (exactly: the
    inliers are symmetric), in the reference's numbering: units 0 and 256 at 0.5 +- 2^-2 (terms 2^-4), units 1 and 2 at 0.5 +- 2^-14
    (terms 2^-28), units 3 .. 5 on the mean with weight 1 and unit 6 with weight 1 - 2^-24, so that with the two tiny units' weights of
    2^-25 the weights add up to 8 exactly; the tiny units 512 and 257 at 0.5 +- 5 x 2^-18, terms 25 x 2^-61: under half an ulp of the
    sum 2^-3 each, over it together.  Units 0, 256, 512 share a thread of the visit order, so each tiny term meets the large sum
    alone: sum / 8 = 2^-6 (1 + 2^-24), a float tie, to even.  by_ref puts the tiny units on host indices 5 and 261 (one thread, with
    nothing else in it): in host order they add up first and carry: one float ulp higher.  Asserted here."""
    w = np.zeros(n, np.float32)
    s = 5 * 2.0 ** -18
    idx = [0, 256, 1, 2, 3, 4, 5, 6, 512, 257]
    pot = np.zeros(n)
    pot[[k for k in range(n) if k not in idx]] = _grid(n - len(idx), 0.9).astype(np.float64)   # weight 0: terms 0 in the inliers' sums
    pot[idx] = [0.75, 0.25, 0.5 + 2.0 ** -14, 0.5 - 2.0 ** -14, 0.5, 0.5, 0.5, 0.5, 0.5 + s, 0.5 - s]
    w[idx] = [1, 1, 1, 1, 1, 1, 1, 1 - 2.0 ** -24, 2.0 ** -25, 2.0 ** -25]
    fixed = {0: 0, 512: 5, 257: 261}                                            # reference index -> host index
    free_host = np.random.default_rng(769).permutation([k for k in range(n) if k not in fixed.values()])
    free_ref = [k for k in range(n) if k not in fixed and k not in idx]         # the units of weight 0 first: host 517 (thread 5) among them
    other_ref = [k for k in idx if k not in fixed]
    free_host = [517] + [k for k in free_host if k != 517]
    br = np.empty(n, np.int32)
    for r_, h_ in fixed.items():
        br[r_] = h_
    br[free_ref + other_ref] = free_host
    c = _finish(f"order-sensitive variance @ {n}", "slice", pot, w, np.ones(n, np.float32), [], [0, 0, 0.02, 0.03, 0.7], br, 4, at_mean="1")
    assert np.array_equal(c["pot"].astype(np.float64)[c["by_ref"]], pot) and np.array_equal(c["w"].astype(np.float64)[c["by_ref"]], w.astype(np.float64))
    p = R.apply_exclusions(c["pot"], c["scale"], c["excl"])
    right = R.class_scalars(p, c["w"], c["by_ref"], "slice", STEP, "tree256")
    wrong = R.class_scalars(p, c["w"], c["by_ref"], "slice", STEP, "tree256", by_ref2=np.arange(n))
    serial = R.class_scalars(p, c["w"], c["by_ref"], "slice", STEP, "serial")
    assert right[0] == wrong[0] == F32(0.5) and right[2] == serial[2] == F32(2.0 ** -6) and R.ulp_diff(right[2], wrong[2])[0] == 1, (right[:4], wrong[:4], serial[:4])
    return c


def _all_cases():
    rng = np.random.default_rng(20261019)
    cases = []
    plan = [(1, "identity", 1), (2, "reversed", 1), (255, "permuted", 3), (256, "identity", 4), (257, "permuted", 8), (511, "reversed", 3),
            (513, "permuted", 4), (1120, "permuted", 8)]
    for n, num, world in plan:
        pot, w, scale, fe, st = _mixed(rng, n)
        cases.append(_finish(f"mixed {n}", "slice", pot, w, scale, fe, st, num, world, seed=n, at_mean="12" if n <= 2 else ""))   # (two units: the second run has one in each class)
    cross = [("identity", 1), ("permuted", 3), ("reversed", 4), ("permuted", 8), ("identity", 3), ("reversed", 1), ("permuted", 4), ("identity", 8),
             ("reversed", 3), ("permuted", 1), ("identity", 4)]
    for n in (257, 513):
        for k, (name, (pot, w, scale, fe, st, at_mean)) in enumerate(_branch_cases(n, rng).items()):
            num, world = cross[(k + (n == 513) * 3) % len(cross)]
            cases.append(_finish(f"{name} @ {n}", "slice", pot, w, scale, fe, st, num, world, at_mean=at_mean, seed=n + k))
    pot, w, scale, fe, st = _likelihood_zero_big()
    cases.append(_finish("likelihood == 0: below, between, above @ 7503", "slice", pot, w, scale, fe, st, "permuted", 3, seed=7))
    cases.append(_order_sensitive())
    cases.append(_order_sensitive_variance())
    # the patch form: the stacks' offset-less copy, a permuted numbering
    for counts, num, world in (([9, 4, 13, 6], "permuted", 1), ([9, 4, 13, 6], "reversed", 3), ([130, 127, 256], "permuted", 4),
                               ([130, 127, 256], "identity", 8)):
        n = sum(counts)
        pot, w, scale = _two(rng, n, 0.15)
        src = R.stack_potential_sources(counts)                      # the weights fall with the potential a unit READS
        w = ((1 - np.where(src >= 0, pot[np.maximum(src, 0)], 0)) * rng.uniform(0.5, 1.0, n)).astype(np.float32)
        scale[[0, 12, 13]] = 1
        st = [0, 0, 0.02, 0.03, 0.8]
        cases.append(_finish(f"patch {counts} {num} world {world}", "patch", pot, w, scale, [1, n - 2], st, num, world,
                             src_ref=R.stack_potential_sources(counts), seed=n + world))
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    return {c["name"]: c for c in cases}


CASES = _all_cases()


def reference_view(c):
    """the case in the REFERENCE's numbering (what the host form and the oracle take): pot, w, scale, excl, inside"""
    br = c["by_ref"]
    return tuple(c[k][br] for k in ("pot", "w", "scale", "excl", "inside"))


def restate(c, order, gauss="f32", runs=1):
    """the restatement applied `runs` times in a row (each run starts from the previous weights and mix_s) -> the last (pot, w, st)"""
    src = None if c["src_ref"] is None else R.src_host(c["src_ref"], c["by_ref"])
    w, st = c["w"], c["state5"]
    for _ in range(runs):
        pot, w, st = R.unit_em(c["pot"], w, c["scale"], c["excl"], STEP, st, c["form"], order, c["by_ref"], src, gauss)
    return pot, w, st


def patch_gauss_gap():
    """the largest difference between the patch form's weights with its float32 Gaussian and with the same Gaussian in float64, both
    with the same (tree256) scalars, over the patch cases: what a float Gaussian costs, whoever's expf it is"""
    gap = 0.0
    for c in CASES.values():
        if c["form"] == "patch":
            _, w32, _ = restate(c, "tree256", "f32")
            _, w64, _ = restate(c, "tree256", "f64")
            gap = max(gap, float(np.abs(w32.astype(np.float64) - w64.astype(np.float64)).max()))
    return gap
