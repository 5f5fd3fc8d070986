"""Structural slice exclusion (--structural: csrc/svr_ssim.inc, svr_structural_decide in csrc/svr_io.cpp, csrc/svr_host.cpp,
csrc/svr_cli.cpp) without a GPU: the numpy restatement of the windowed SSIM on hand-worked windows, the library's decision rule and
extended report writer against the restatement, the command line's refusals, how much the order of the window sums shows in the value
(the tolerance of tests/test_structural_gpu.py comes from here), and the fairness of the end-to-end case that file runs: on the CPU
oracle the restatement and the rule single the shifted slice out."""
import math
import subprocess

import numpy as np
import pytest

from fetalreconstruction_amd import build, host
from tests import slice_quality_ref as qref
from tests import ssim_ref as ref


def _map(s, y, R, sw=None, scale=1.0, c1=0.0, c2=0.0, bias=None, mode="ltr"):
    s, y = np.asarray(s, np.float32)[None], np.asarray(y, np.float32)[None]
    sw = np.ones_like(s) if sw is None else np.asarray(sw, np.float32)[None]
    counted, val, m = ref.ssim_map(s, y, sw, [scale], R, c1, c2, None if bias is None else np.asarray(bias, np.float32)[None], mode=mode)
    return counted[0], val[0], m[0]


# ---- hand-worked windows ---------------------------------------------------------------------------------------------------------

def test_a_single_pixel_is_not_counted():
    for R in (1, 3, 7):
        counted, val, m = _map([[5.0]], [[5.0]], R)
        assert m.tolist() == [[1]] and not counted.any() and np.isnan(val).all()     # 1 < ((2R+1)^2 + 1) / 2
    assert ref.slice_sums(counted[None], val[None]).tolist() == [[0.0, 0.0]]


def test_the_half_window_threshold_at_a_corner():
    # R = 1: the corner pixel of a grid sees 4 of its 9 window pixels -> m = 4 < 5, not counted; its neighbour along the edge sees 6
    a = np.arange(1.0, 13.0).reshape(3, 4)
    counted, val, m = _map(a, a, 1)
    assert m.tolist() == [[4, 6, 6, 4], [6, 9, 9, 6], [4, 6, 6, 4]]
    assert counted.tolist() == [[False, True, True, False], [True] * 4, [False, True, True, False]]
    # exactly 5 of 9: an interior pixel with four of its window's pixels outside the mask (-1) or under the simulated weight
    s = a.copy()
    s[0, 0] = s[0, 1] = s[0, 2] = -1.0
    sw = np.ones((3, 4))
    sw[2, 0] = 0.5
    counted, val, m = _map(s, a, 1, sw=sw)
    assert m[1, 1] == 5 and counted[1, 1]
    sw[2, 1] = 0.99                                        # float32(0.99) is not > 0.99f: one fewer, 4 of 9
    counted, val, m = _map(s, a, 1, sw=sw)
    assert m[1, 1] == 4 and not counted[1, 1] and math.isnan(val[1, 1])
    assert not counted[0, :3].any()                        # a pixel outside V is never counted, whatever its window holds


def test_identical_integer_slices_give_exactly_one():
    rng = np.random.default_rng(2)
    a = rng.integers(0, 256, (16, 17)).astype(np.float32)    # (R = 7 needs 113 pixels in a window)
    for R, c1, c2 in ((1, 0.0, 0.0), (3, 6.5, 58.5), (7, 0.25, 4.0)):
        counted, val, m = _map(a, a * 2, R, scale=2.0, c1=c1, c2=c2)
        assert counted.any() and (val[counted] == 1.0).all()
    # a constant window without constants: 0 / 0, reported as it comes out
    counted, val, m = _map(np.full((3, 3), 4.0), np.full((3, 3), 4.0), 1)
    assert counted[1, 1] and math.isnan(val[1, 1])
    counted, val, m = _map(np.full((3, 3), 4.0), np.full((3, 3), 4.0), 1, c1=1.0, c2=1.0)
    assert val[1, 1] == 1.0


def test_a_hand_worked_window():
    # 3 x 3, R = 1, the centre pixel: x = 1..9, y = 9..1  ->  means 5, 5; variances 60/9; covariance -60/9
    x = np.arange(1.0, 10.0).reshape(3, 3)
    counted, val, m = _map(x, 10.0 - x, 1, c1=1.0, c2=2.0)
    mx = my = 45 / 9
    vx = vy = 285 / 9 - mx * mx
    cxy = 165 / 9 - mx * my
    want = ((2 * mx * my + 1.0) * (2 * cxy + 2.0)) / ((mx * mx + my * my + 1.0) * (vx + vy + 2.0))
    assert counted[1, 1] and val[1, 1] == want and want < 0


def test_x_is_float32_before_it_is_widened():
    s, scale = np.float32(0.1), np.float32(3.0)
    a = np.full((3, 3), s, np.float32)
    x, y, V = ref.operands(a[None], a[None], np.ones((1, 3, 3), np.float32), [scale])
    assert x.dtype == np.float32 and x[0, 1, 1] == np.float32(s * scale) and float(x[0, 1, 1]) != float(s) * float(scale)
    m, S = ref.window_sums(x, y, V, 1)
    assert S[0, 0, 1, 1] == sum([float(np.float32(s * scale))] * 9) and S[2, 0, 1, 1] == sum([float(np.float32(s * scale)) ** 2] * 9)
    # with a bias field: s * exp(-b) * scale, left to right in float32, and the M-step's double comparison of the simulated weight
    b = np.full((1, 3, 3), 0.25, np.float32)
    sw = np.full((1, 3, 3), np.float32(0.99))
    xb, _, Vb = ref.operands(a[None], a[None], sw, [scale], b)
    assert Vb.all() and xb[0, 0, 0] == np.float32(np.float32(s * np.exp(-b[0, 0, 0])) * scale)
    assert not ref.operands(a[None], a[None], sw, [scale])[2].any()      # float32(0.99) is not above the float 0.99f of the other form


def test_the_three_summations_agree_on_integer_data():
    rng = np.random.default_rng(4)
    s = rng.integers(0, 256, (2, 13, 17)).astype(np.float32)
    s[rng.random(s.shape) < 0.2] = -1
    y = rng.integers(0, 256, s.shape).astype(np.float32)
    sw = rng.choice(np.array([0.5, 0.99, 1.0, 1.0], np.float32), s.shape)
    got = [ref.ssim_map(s, y, sw, [1.0, 2.0], 3, 6.5, 58.5, mode=mode) for mode in ("ltr", "fsum", "dd")]
    for c, v, m in got[1:]:
        assert np.array_equal(c, got[0][0]) and np.array_equal(v, got[0][1], equal_nan=True) and np.array_equal(m, got[0][2])


# ---- how much the order of the window sums shows (the device's tolerance) ----------------------------------------------------------

@pytest.mark.parametrize("name", ["general", "general_bias"])
def test_the_order_of_the_window_sums_shows_this_much(name):
    s, y, simw, scales = ref.general_case(seed=11 if name == "general" else 12)
    bias = ref.general_bias(s.shape) if name == "general_bias" else None
    c1, c2 = ref.GENERAL_C
    x, yy, V = ref.operands(s, y, simw, scales, bias, exp64=True)        # (the float64 exponential rounded to float32: the same on every host)
    m, S_ltr = ref.window_sums(x, yy, V, 3, "ltr")
    _, S_exact = ref.window_sums(x, yy, V, 3, "fsum")
    _, S_dd = ref.window_sums(x, yy, V, 3, "dd")
    assert np.array_equal(S_dd, S_exact)                   # the fast error-free summation the GPU tests use IS math.fsum on this input
    counted, a = ref.ssim_from_sums(m, S_ltr, V, 3, c1, c2)
    counted2, b = ref.ssim_from_sums(m, S_exact, V, 3, c1, c2)
    # the threshold is a comparison of integers: no window is at it ambiguously
    thr = (7 * 7 + 1) // 2
    assert m.dtype == np.int64 and np.array_equal(counted, counted2) and np.array_equal(counted, V & (m >= thr)) and ((m >= thr) | (m <= thr - 1)).all()
    assert counted.sum() > 100000 and (m[V] < thr).sum() > 1000   # (both sides of the threshold occur)
    gap = float(np.abs(a[counted] - b[counted]).max())
    print(f"{name}: largest per-pixel gap exact vs left-to-right window sums {gap:.3e} over {int(counted.sum())} pixels; ssim in "
          f"[{np.nanmin(b):.3f}, {np.nanmax(b):.3f}]")
    assert 0 < gap <= ref.MEASURED[name], (gap, ref.MEASURED[name])
    assert ref.MEASURED[name] <= 1.05 * gap                # ... and the recorded number is this input's, not a loose one


# ---- the decision rule ---------------------------------------------------------------------------------------------------------

def _sums(q, n=100.0):
    q = np.asarray(q, np.float64)
    return np.stack([np.full(len(q), n), q * n], 1)


def _both(stack, sums, eligible=None, **kw):
    eligible = np.ones(len(stack), bool) if eligible is None else eligible
    args = {k: kw.get(k, ref.DEFAULTS[k]) for k in ("min_pixels", "k_mad", "min_drop")}
    q, ex = host.structural_decide(stack, sums, eligible, **args)
    q2, ex2 = ref.decide(stack, sums, eligible, **args)
    assert np.array_equal(q, q2, equal_nan=True) and np.array_equal(ex, ex2), (q, q2, ex, ex2)
    return q, ex


def test_decide_on_an_even_and_an_odd_stack():
    q0 = [0.9, 0.85, 0.2, 0.88, 0.91, 0.87, 0.86, 0.89]                 # even: median (0.87 + 0.88) / 2
    q1 = [0.7, 0.72, 0.69, 0.71, 0.3, 0.73, 0.68]                       # odd: median 0.7
    stack = [0] * 8 + [1] * 7
    q, ex = _both(stack, _sums(q0 + q1))
    assert np.flatnonzero(ex).tolist() == [2, 12]
    # interleaved stacks: the same decision slice by slice
    perm = np.random.default_rng(0).permutation(15)
    q, ex2 = _both(np.asarray(stack)[perm], _sums(np.asarray(q0 + q1)[perm]))
    assert np.array_equal(ex2, ex[perm])
    # hand-worked, the even stack: |q - 0.875| sorted -> MAD = (0.015 + 0.025) / 2 up to rounding; k MAD 1.4826 < 0.1, so min_drop decides
    v = sorted(q0)
    med = (v[3] + v[4]) / 2.0
    d = sorted(abs(t - med) for t in q0)
    mad = (d[3] + d[4]) / 2.0
    assert 3.0 * 1.4826 * mad < 0.1 and [t < med - 0.1 for t in q0] == ex[:8].tolist()
    # ... and without a min_drop the MAD term decides
    q, ex = _both([0] * 8, _sums(q0), k_mad=0.5, min_drop=0.0)
    assert ex.tolist() == [t < med - 0.5 * 1.4826 * mad for t in q0] and ex.sum() == 3


def test_decide_with_a_mad_of_zero():
    qv = [0.8, 0.8, 0.8, 0.8, 0.8, 0.75, 0.69]                           # median 0.8, MAD 0: min_drop alone
    q, ex = _both([3] * 7, _sums(qv))
    assert ex.tolist() == [False] * 6 + [True]
    q, ex = _both([3] * 7, _sums(qv), min_drop=0.0)                     # q < median - 0: everything below the median
    assert ex.tolist() == [False] * 5 + [True, True]


def test_decide_needs_four_judged_slices():
    q, ex = _both([0, 0, 0], _sums([0.9, 0.9, 0.1]))
    assert not ex.any() and not np.isnan(q).any()
    sums = _sums([0.9, 0.9, 0.9, 0.1, 0.9])
    sums[1, 0] = 24                                        # below min_pixels: not judged, and then only ...
    sums[2] = [0, 0]                                       # ... three are left
    q, ex = _both([0] * 5, sums)
    assert np.isnan(q[[1, 2]]).all() and not ex.any()
    sums[1, 0] = 25
    sums[1, 1] = 0.9 * 25
    q, ex = _both([0] * 5, sums)
    assert ex.tolist() == [False, False, False, True, False]


def test_decide_nan_ties_and_eligibility():
    sums = _sums([0.9, 0.9, 0.1, 0.9, 0.9, 0.1])
    sums[4, 1] = np.nan                                    # a sum that is nan: not judged, never excluded, and it poisons no median
    q, ex = _both([0] * 6, sums)
    assert math.isnan(q[4]) and ex.tolist() == [False, False, True, False, False, True]
    el = np.array([1, 1, 0, 1, 1, 1], bool)                # the first bad slice is not eligible (outside, force-excluded): reported nan, kept
    q, ex = _both([0] * 6, _sums([0.9, 0.9, 0.1, 0.9, 0.9, 0.1]), eligible=el)
    assert math.isnan(q[2]) and ex.tolist() == [False] * 5 + [True]
    qv = [0.5, 0.9, 0.5, 0.9, 0.9, 0.5, 0.9, 0.9]                        # ties: equal values are excluded or kept together
    q, ex = _both([0] * 8, _sums(qv))
    assert ex.tolist() == [v == 0.5 for v in qv]
    assert host.structural_decide([], np.zeros((0, 2)), [])[1].shape == (0,)
    with pytest.raises(Exception):
        host.structural_decide([0], [[1.0, 1.0]], [1], k_mad=-1.0)


def test_report_writer_with_the_three_columns(tmp_path):
    n = 5
    sums = np.zeros((n, 10))
    for i in range(n):
        a = np.random.default_rng(i).integers(1, 200, (5, 6)).astype(np.float32)
        sums[i] = qref.sums(a[None], a[None] + 1, np.ones((1, 5, 6), np.float32), np.ones((1, 5, 6), np.float32), [1.0])[0]
    stack, weight = np.array([0, 0, 1, 1, 1]), np.array([1, 0, 1, 0.75, 0.2], np.float32)
    inside, scale, p6 = np.array([1, 1, 1, 0, 1], np.uint8), np.ones(n, np.float32), np.zeros((n, 6))
    ssim = np.array([[30, 24.0], [28, 7.0], [0, 0.0], [12, -3.0], [30, 30.0]])
    flag = np.array([0, 1, 0, 0, 1])
    host.write_slice_report_ex(tmp_path / "ex.tsv", stack, weight, inside, scale, p6, sums, ssim, flag)
    host.write_slice_report(tmp_path / "plain.tsv", stack, weight, inside, scale, p6, sums)
    names, rows = ref.read_report(tmp_path / "ex.tsv")
    names0, rows0 = ref.read_report(tmp_path / "plain.tsv")
    assert names == ref.HEADER_EX and len(names) == 21 and names0 == qref.HEADER and rows0.shape == (n, 18)
    assert np.array_equal(rows[:, :18], rows0, equal_nan=True)
    assert np.array_equal(rows[:, 19], ssim[:, 0]) and np.array_equal(rows[:, 20], flag)
    assert math.isnan(rows[2, 18]) and np.allclose(rows[[0, 1, 3, 4], 18], [0.8, 0.25, -0.25, 1.0], rtol=1e-8)
    assert (tmp_path / "ex.tsv").read_text().splitlines()[3].split("\t")[18] == "nan"


# ---- the command line's refusals ------------------------------------------------------------------------------------------------

def _run(args):
    build.build()
    return subprocess.run([build.CLI, *args], capture_output=True, text=True, timeout=120)


def test_help_lists_the_option():
    r = _run(["--help"])
    assert r.returncode == 0 and all(o in r.stdout for o in ("--structural", "--structuralRadius", "--structuralK", "--structuralMinDrop",
                                                              "--structuralMinPixels")) and "deviation" in r.stdout


def test_structural_is_refused_with_sfolder():
    r = _run(["-o", "x.nii.gz", "-i", "s.nii.gz", "--structural", "--sfolder", "slices"])
    assert r.returncode != 0 and "--sfolder" in r.stderr and "belong to no stack" in r.stderr and "not supported by this build" not in r.stderr, r.stderr


@pytest.mark.parametrize("radius", ["0", "8"])
def test_a_radius_outside_one_to_seven_is_refused(radius):
    r = _run(["-o", "x.nii.gz", "-i", "s.nii.gz", "--structural", "--structuralRadius", radius])
    assert r.returncode != 0 and "--structuralRadius" in r.stderr and "not supported by this build" not in r.stderr, r.stderr


# ---- the end-to-end case is fair ---------------------------------------------------------------------------------------------------

def test_the_end_to_end_case_is_fair_on_the_oracle(oracle_mod, tmp_path):
    """The case of tests/test_structural_gpu.py's command-line tests, through the Python pre-processing and the host twin over the CPU
    oracle with the command line's schedule (tests/test_slice_quality.py's, on the shifted slice): with the defaults the restatement and
    the rule exclude the shifted slice, every other excluded slice lies below its stack's median, and there are at most 2 of those.
    (What the GPU test asserts of the product.)"""
    from fetalreconstruction_amd import nifti
    from fetalreconstruction_amd import preprocess as pp
    from tests.twins.reconstruction import irtkReconstruction
    args = ref.write_cli_case(tmp_path)
    paths = args[1:4]
    stacks = []
    for p in paths:
        d, at = nifti.read(p)
        stacks.append(pp.Image(d.astype(np.float64), at))
    md, mat = nifti.read(tmp_path / "mask.nii.gz")
    mask = pp.Image(md.astype(np.float64), mat)
    T = [np.eye(4)] * 3
    stacks[0] = pp.CropImage(stacks[0], pp.TransformMask(stacks[0].attr, mask, T[0]))
    tattr, _ = pp.CreateTemplate(stacks[0].attr, 1.0)
    vol_mask = pp.SetMask(tattr, mask, 0.0)
    for k in (1, 2):
        stacks[k] = pp.CropImage(stacks[k], pp.TransformMask(stacks[k].attr, vol_mask, T[k]))
    pp.MatchStackIntensitiesWithMasking(stacks, T, vol_mask, 700.0, together=False)
    slices, attrs, slice_t, stack_index = pp.CreateSlicesAndTransformations(stacks, T, [2.2] * 3)
    slices = pp.MaskSlices(slices, attrs, slice_t, vol_mask)
    prob = pp.build_problem(tattr, vol_mask, slices, attrs, slice_t, stack_index)
    orc = oracle_mod.OracleReconstruction(prob, oracle_mod.CANON)
    drv = irtkReconstruction(orc, prob.ns, max_intensity=prob.max_intensity, min_intensity=prob.min_intensity)
    drv.SetSmoothingParameters(ref.SCHEDULE["delta"], ref.SCHEDULE["last_lambda"])
    drv.SpeedupOff()
    drv.reconstruct_iteration(ref.SCHEDULE["rec_last"])
    # where svrh_structural_evaluate stands: after the last SR iteration, before MaskVolume -- the slices are the last iteration's projection
    c1, c2 = ref.constants(prob.max_intensity, prob.min_intensity)
    counted, val, _ = ref.ssim_map(orc.slices, orc.simslices, orc.simweights, drv._scale_gpu, ref.DEFAULTS["radius"], c1, c2, mode="dd")
    sums = ref.slice_sums(counted, val)
    si = np.asarray(prob.stack_index)
    inside = np.asarray(drv._slice_inside_gpu, bool)       # (of that projection)
    q, ex = ref.decide(si, sums, inside, ref.DEFAULTS["min_pixels"], ref.DEFAULTS["k_mad"], ref.DEFAULTS["min_drop"])
    assert int((si == ref.CORRUPT_STACK).sum()) == 8, "the crop is expected to keep every slice of the stack"
    bad = int(np.flatnonzero(si == ref.CORRUPT_STACK)[0]) + ref.CORRUPT_SLICE
    for k in range(3):
        print("stack", k, "q", np.round(q[si == k], 4), "excluded", np.flatnonzero(ex[si == k]).tolist())
    assert ex[bad]
    others = [i for i in np.flatnonzero(ex) if i != bad]
    for i in others:
        assert q[i] < np.nanmedian(q[si == si[i]])
    assert len(others) <= 2
