"""The numpy float64 reference of the float slice-to-volume registration (tests/reg_ref.py) against the C oracle
(oracle/reg_oracle.c) on every case of tests/reg_cases.py, so that each vouches for the other before the device is compared
with both (tests/test_reg_shapes_gpu.py): padding, counts and hit sets exactly, values within the float-to-float64 distance
that is measured here and recorded in reg_cases.MEASURED, and the conditioning of whole runs recorded in reg_cases.TRAJECTORY."""
import numpy as np
import pytest

import reg_cases as cases
import reg_ref as ref


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_mod):
    return oracle_mod


def test_gauss_kernel_is_the_oracle_s(oracle_mod):
    for sigma, taps in ((0.5, 7), (1.35, 7), (2.7, 13), (6.4, 31), (12.8, 63), (100.0, 63), (2.0, 9)):
        k, half = oracle_mod.reg_gauss_kernel(sigma)
        kr, hr = ref.gauss_half(sigma)
        assert k == kr == taps and len(half) == len(hr) == (taps + 1) // 2
        assert np.allclose(half, hr, rtol=0, atol=2e-7)                 # float exp, float sum of <= 63 terms


def test_the_cases_reach_their_edges():
    """what each shape was chosen for, so that a change of a case cannot silently lose it"""
    taps = {n: [ref.gauss_half(ref.level_sigma(cases.SPECS[n][1], lv))[0] for lv in (0, 1)] for n in cases.NAMES}
    assert taps["wide_37x5"] == taps["tall_5x37"] == [7, 13] and taps["cap_63"] == [31, 63] and taps["one_slice"] == [7, 7]
    c = cases.get("wide_37x5")
    assert c.W != c.H and c.H < 7 < c.W and cases.get("tall_5x37").W < 7
    c = cases.get("cap_63")
    assert c.W < 32 and c.H < 16                                           # narrower than the 32 (16) half taps on both axes
    assert cases.get("wave_3x3").W * cases.get("wave_3x3").H < 64 and cases.get("line_257").W * cases.get("line_257").H == 257
    assert cases.get("red_4096").W * cases.get("red_4096").H == 4096
    n = cases.get("red_4270").W * cases.get("red_4270").H
    assert n > 4096 and n % 1024
    assert cases.get("one_slice").ns == 1 and [cases.get(k).ns for k in ("ns_1024", "ns_1025", "ns_1100")] == [1024, 1025, 1100]
    c = cases.get("skew_9x14x11")                                          # samples leave the volume through every face
    r = cases.reference(c.name, 0, 0)
    assert all(v & (v - 1) for v in (c.vx, c.vy, c.vz)) and len({c.vx, c.vy, c.vz}) == 3
    s = r["sampled"]
    for edge in (s[:, :, 0, :], s[:, :, -1, :], s[:, :, :, 0], s[:, :, :, -1]):
        assert (edge == 0).any()                                           # border colour 0 ...
    assert (s == -1).any() and (s > 0).any() and (c.vol == np.rint(c.vol)).all()   # ... the mask's -1 inside, integer voxels
    c = cases.get("dead_slices")
    for level in (0, 1):
        r = cases.reference(c.name, level, 0)
        assert r["cntA"][1] == 0 and r["sumA"][1] == 0 and r["sim"][1] == 0        # no target data
        assert (r["cntB"][:, 3] == c.W * c.H).all() and (r["sumB"][:, 3] == 0).all() and r["sim"][3] == 0   # all zeros: norm 0
        assert (r["sim"][[0, 2, 4]] != 0).all()
    for name in cases.NAMES:                                               # NCC is informative everywhere else
        c = cases.get(name)
        frac = (c.targets >= 0).mean()
        assert 0.5 < frac < 1.0, (name, frac)


@pytest.mark.parametrize("name", cases.NAMES)
def test_reference_is_the_oracle(name, oracle_mod):
    c = cases.get(name)
    o = cases.oracle_for(c)
    scale = float(c.vol.max())
    d_slices = d_sim = 0.0
    for level in (1, 0):
        for k, act in enumerate(cases.active_lists(c)):
            so, do_ = o.evaluate_costs(c.start, level, act)
            r = cases.reference(name, level, k)
            what = (name, level, k)
            a = c.ns if act is None else len(act)
            idx = np.arange(c.ns) if act is None else np.asarray(act)
            tb = o._resampled_float.reshape(c.ns, c.H, c.W)
            assert np.array_equal(tb == -1, r["targets"] == -1) and np.array_equal(do_ == -1, r["blurred"] == -1), what   # padding
            assert np.array_equal(tb >= 0, r["targets"] >= 0) and np.array_equal(do_ >= 0, r["blurred"] >= 0), what       # hit sets
            assert np.array_equal(o._temp_int[:a], r["cntA"][idx]) and np.array_equal(o._temp_int[a:2 * a], r["cntB"].sum(0)), what
            assert np.array_equal(so != 0, r["sim"] != 0), what
            sb, mom = o.last_stages()                                         # the oracle's own sums and moments within the device's bounds
            tol = cases.tol_rel(name)
            assert (np.abs(sb - r["sumB"]) <= tol * np.maximum(r["cntB"], 1) * scale).all(), what
            assert (np.abs(mom - r["mom"]) <= tol * np.maximum(r["pairs"], 1)[..., None] * scale * scale).all(), what
            d_slices = max(d_slices, np.abs(do_ - r["blurred"]).max() / scale, np.abs(tb - r["targets"]).max() / scale)
            d_sim = max(d_sim, np.abs(so - r["sim"]).max())
    rec = cases.MEASURED[name]
    print(f"{name}: oracle to float64: slices {d_slices:.2e} of the largest sample (recorded {rec['slices']:.2e}), "
          f"similarities {d_sim:.2e} (recorded {rec['sim']:.2e})")
    assert d_slices <= rec["slices"] * 1.01 and d_sim <= rec["sim"] * 1.01         # the record is an upper bound ...
    assert rec["slices"] <= 2 * d_slices and rec["sim"] <= max(2 * d_sim, 1e-7)    # ... and not a loose one
    assert d_slices < 8 * 2.0 ** -24                                                # a few float roundings, nothing else


@pytest.mark.parametrize("name", cases.NAMES)
def test_conditioning_of_whole_runs(name):
    """TRAJECTORY[name] is the longest listed schedule at which scaling the non-negative voxels by 1 + 2^-20, 1 - 2^-19 and
    1 + 3 * 2^-21 moves no counter and no matrix by more than 1e-5 (None: none of them).  The recorded schedule must pass; the
    next longer one is run and reported."""
    c = cases.get(name)
    want = cases.TRAJECTORY[name]

    def stable(schedule):
        t0, c0, a0, _ = cases.oracle_run(c, schedule)
        moved = []
        for f in cases.PERTURBATIONS:
            t, cn, a, _ = cases.oracle_run(c, schedule, cases.perturbed(c.vol, f))
            moved.append((int((np.abs(t - t0).reshape(c.ns, -1).max(1) > 1e-5).sum()), bool(np.array_equal(cn, c0))))
        print(name, schedule, "slices moved / counters equal:", moved, "counters", c0.tolist())
        return all(m == (0, True) for m in moved)
    i = len(cases.SCHEDULES) if want is None else cases.SCHEDULES.index(want)
    if want is not None:
        assert stable(want)
    if i > 0:                                                                # (reported, not asserted: instability is no property to pin)
        print(name, "next longer schedule", cases.SCHEDULES[i - 1], "stable:", stable(cases.SCHEDULES[i - 1]))
    if name == "ns_1100":
        assert want == (1, 1, 1) and cases.oracle_run(c, want)[3] > 1024          # the first line-search step keeps > 1024 slices
    if name in ("wide_37x5", "tall_5x37"):
        assert want is not None                                                   # a W != H case is compared as a whole run


@pytest.mark.parametrize("name", cases.PATCH_NAMES)
def test_patch_cost_reference_is_the_oracle(name, oracle_mod):
    worst = 0.0
    for integer in (True, False):
        c = cases.patch_case(name, integer)
        for level in range(3):
            no, so = oracle_mod.cc_patches(c.patches, c.ri2w, c.tm, c.w2i, c.vol, level)
            st = level + 1
            for k in range(c.n):
                nr, sr = ref.cc_patch(c.patches[k], c.ri2w[k], c.tm[k], c.w2i, c.vol, level)
                assert so[k, 0] == sr[0] <= 3 * -(-c.px // st) * -(-c.py // st), (integer, level, k)
                if integer:                                                  # (the oracle's float sums round from 2^24 on)
                    assert all(a == b for a, b in zip(so[k], sr) if b < 2 ** 24), (level, k, so[k], sr)
                else:
                    worst = max(worst, (np.abs(so[k, 1:] - sr[1:]) / np.maximum(np.abs(sr[1:]), 1)).max())
                if sr[0] > 2 and np.isfinite(nr):
                    assert abs(no[k] - nr) < 2e-5, (integer, level, k, no[k], nr)
            assert (so[:, 0] > 0).all() and (integer or (so[:, 0] < 3 * -(-c.px // st) * -(-c.py // st)).all())
    print(f"{name}: oracle sums to float64, relative: {worst:.2e} (recorded {cases.PATCH_MEASURED[name]:.2e})")
    assert worst <= cases.PATCH_MEASURED[name] * 1.01 <= 2.02 * worst
    assert c.px != c.py and c.px % 2 and c.px % 3 and c.py % 2 and (c.py % 3 or c.py == 3)


def test_patch_registration_case_and_its_conditioning(oracle_mod):
    """the 19 x 13 case: level 1 blurs with 13 taps (the second pass with the 14th, clamped one), level 0 with 7; the share of
    patches the oracle itself reproduces under the perturbations is what reg_cases.PATCH_REG_SHARE records"""
    c = cases.patch_reg_case()
    assert [ref.gauss_half(ref.level_sigma(c.vdim, lv))[0] for lv in (0, 1)] == [7, 13] and c.px != c.py and c.py < 14 <= c.px
    for level in (1, 0):                                                    # the oracle's patch blur is the reference's, quirk included
        sigma = ref.level_sigma(c.vdim, level)
        k, h = ref.gauss_half(sigma)
        quirk = np.append(h, h[-1]) if k == 13 else None                    # GaussYKernel<14>: one more tap with the last weight
        want = ref.blur(c.patches, h, quirk, outside_zero=True)
        got = oracle_mod.pvr_blur_patches(c.patches, sigma)
        assert np.array_equal(got == -1, want == -1) and np.abs(got - want).max() <= 4e-7 * float(c.vol.max())
        if k == 13:
            assert np.abs(ref.blur(c.patches, h, outside_zero=True) - want).max() > 1e-3 * float(c.vol.max())   # the 14th tap matters
    t, ti, cn = cases.oracle_patch_run(c)
    lv, st, it = c.schedule
    assert cn[0] == lv * st * it and cn[2] == c.n and cn[1] >= c.n * cn[0] * 14
    shares = []
    for f in cases.PERTURBATIONS:
        t2, _, c2 = cases.oracle_patch_run(c, cases.perturbed(c.vol, f))
        shares.append(float((np.abs(t2 - t).max(axis=1) < 1e-4).mean()))
        assert c2[0] == cn[0] and abs(int(c2[1]) - int(cn[1])) <= max(10, int(cn[1]) // 1000)
    print("share of patches within 1e-4 of the unperturbed run:", shares, "recorded", cases.PATCH_REG_SHARE)
    assert abs(min(shares) - cases.PATCH_REG_SHARE) < 1e-9
