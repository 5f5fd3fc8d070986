"""The per-slice quality report (csrc/svr_quality.inc, csrc/svr_io.cpp, --sliceReport / --simulatedStacks of csrc/svr_cli.cpp) without a
GPU: the numpy restatement of the ten sums and of the derived values on hand-worked slices, the derived values and the report writer of the
library against it, the command line's refusals, and the fairness of the end-to-end case tests/test_slice_quality_gpu.py runs: on the CPU
oracle the restatement singles the corrupted slice out."""
import math
import subprocess

import numpy as np
import pytest

from fetalreconstruction_amd import build, host
from tests import slice_quality_ref as ref


def _one(s, y, sw=None, w=None, scale=1.0, bias=None):
    s, y = np.asarray(s, np.float32)[None], np.asarray(y, np.float32)[None]
    sw = np.ones_like(s) if sw is None else np.asarray(sw, np.float32)[None]
    w = np.ones_like(s) if w is None else np.asarray(w, np.float32)[None]
    return ref.sums(s, y, sw, w, [scale], None if bias is None else np.asarray(bias, np.float32)[None])[0]


def _both(row):
    """the library's derived values; they must be the restatement's (same expressions in double)"""
    lib, mine = host.slice_quality_derive(row), ref.derive(row)
    assert np.array_equal(lib, mine, equal_nan=True), (lib, mine)
    return lib


def test_hand_worked_sums():
    # 2 x 3 pixels, scale 2: one pixel outside the mask (-1), one with a simulated weight of 0.5 (in n_px, not in n)
    s = [[1, 2, -1], [3, 4, 5]]
    y = [[2, 5, 9], [6, 7, 11]]
    sw = [[1, 1, 1], [1, 0.5, 1]]
    w = [[0.5, 0.25, 1], [1, 1, 0.75]]
    row = _one(s, y, sw, w, scale=2.0)
    x, yy, ww = np.array([2.0, 4, 6, 10]), np.array([2.0, 5, 6, 11]), np.array([0.5, 0.25, 1, 0.75])
    e = x - yy
    assert row.tolist() == [5, 4, x.sum(), yy.sum(), (x * x).sum(), (yy * yy).sum(), (x * yy).sum(), (e * e).sum(), np.abs(e).sum(), ww.sum()]
    d = _both(row)
    assert d[0] == pytest.approx(np.corrcoef(x, yy)[0, 1], abs=1e-14) and d[1] == math.sqrt(2 / 4) and d[2] == 0.5 and d[3] == 2.5 / 4


def test_x_and_e_are_float32_before_they_are_widened():
    s, scale, y = np.float32(0.1), np.float32(3.0), np.float32(0.3)
    row = _one([[s]], [[y]], scale=scale)
    x = np.float32(s * scale)
    assert row[2] == float(x) and row[2] != float(s) * float(scale)
    assert row[7] == float(np.float32(x - y)) ** 2
    # with a bias field: s * exp(-b) * scale, left to right in float32, and the M-step's double comparison of the simulated weight
    b = np.float32(0.25)
    rb = _one([[s, s]], [[y, y]], sw=[[np.float32(0.99), 1.0]], scale=scale, bias=[[b, b]])
    assert rb[0] == 2 and rb[1] == 2                       # float32(0.99) is above the double 0.99 the bias form compares with ...
    assert rb[2] == 2 * float(np.float32(np.float32(s * np.exp(-b)) * scale))
    assert _one([[s, s]], [[y, y]], sw=[[np.float32(0.99), 1.0]], scale=scale)[1] == 1    # ... and not above the float 0.99f of the other


def test_empty_slice():
    row = _one(np.full((3, 4), -1.0), np.zeros((3, 4)))
    assert row.tolist() == [0] * 10
    assert np.isnan(_both(row)).all()


def test_slice_with_one_pixel():
    row = _one([[-1, 7, -1]], [[0, 5, 0]], w=[[1, 0.5, 1]])
    assert row[0] == 1 and row[1] == 1
    d = _both(row)
    assert math.isnan(d[0]) and d[1] == 2.0 and d[2] == 2.0 and d[3] == 0.5


def test_constant_slice_has_no_ncc():
    row = _one(np.full((4, 4), 3.0), np.arange(16.0).reshape(4, 4))
    d = _both(row)
    assert row[1] == 16 and math.isnan(d[0]) and d[1] > 0
    row = _one(np.arange(16.0).reshape(4, 4), np.full((4, 4), 3.0))      # ... whichever of the two is constant
    assert math.isnan(_both(row)[0])


def test_identical_slices():
    a = np.arange(1.0, 21.0).reshape(4, 5)
    d = _both(_one(a, a))
    assert d[0] == pytest.approx(1.0, abs=1e-12) and d[1] == 0.0 and d[2] == 0.0 and d[3] == 1.0


def test_report_writer(tmp_path):
    rng = np.random.default_rng(5)
    n = 7
    sums = np.zeros((n, 10))
    for i in range(n):
        a = rng.integers(1, 200, (5, 6)).astype(np.float32)
        sums[i] = _one(a, a + rng.integers(-5, 6, a.shape), w=rng.integers(0, 257, a.shape) / 256.0)
    sums[2] = 0                                            # an empty slice: four nan
    sums[5] = _one([[-1, 7]], [[0, 5]])                    # one pixel: ncc nan
    stack = np.array([0, 0, 0, 1, 1, 2, 2])
    weight = np.array([1, 0.75, 0.5, 0.25, 0.9, 0.1, 1.0], np.float32)
    inside = np.array([1, 1, 0, 1, 1, 0, 1], np.uint8)
    scale = np.linspace(0.9, 1.1, n).astype(np.float32)
    p6 = rng.normal(size=(n, 6))
    path = tmp_path / "report.tsv"
    host.write_slice_report(path, stack, weight, inside, scale, p6, sums)
    text = path.read_text()
    lines = text.splitlines()
    assert lines[0].split("\t") == ref.HEADER and len(ref.HEADER) == 18
    assert len(lines) == 1 + n and all(len(ln.split("\t")) == 18 for ln in lines)
    assert lines[3].split("\t")[14:] == ["nan"] * 4 and lines[6].split("\t")[14] == "nan" and "-nan" not in text
    names, rows = ref.read_report(path)
    assert np.array_equal(rows[:, 0], stack)
    assert rows[:, 1].tolist() == [1, 1, 0, 0, 1, 0, 1] and rows[:, 2].tolist() == [0, 0, 0, 1, 0, 0, 0] and rows[:, 3].tolist() == [0, 0, 1, 0, 0, 1, 0]
    assert np.array_equal(rows[:, 1:4].sum(1), np.ones(n))
    assert np.allclose(rows[:, 4], weight, rtol=1e-8) and np.allclose(rows[:, 5], scale, rtol=1e-8) and np.allclose(rows[:, 6:12], p6, rtol=1e-8)
    assert np.array_equal(rows[:, 12:14], sums[:, :2])
    want = np.stack([ref.derive(s) for s in sums])
    assert np.array_equal(np.isnan(rows[:, 14:]), np.isnan(want)) and np.allclose(rows[:, 14:], want, rtol=1e-8, equal_nan=True)


def _run(args):
    build.build()
    return subprocess.run([build.CLI, *args], capture_output=True, text=True, timeout=120)


def test_help_lists_the_two_options():
    r = _run(["--help"])
    assert r.returncode == 0 and "--sliceReport" in r.stdout and "--simulatedStacks" in r.stdout


@pytest.mark.parametrize("option", [["--sliceReport", "r.tsv"], ["--simulatedStacks", "sim"]])
def test_both_options_are_refused_with_dry_run(option):
    r = _run(["-o", "x.nii.gz", "-i", "s.nii.gz", *option, "--dryRun"])
    assert r.returncode != 0 and "--dryRun" in r.stderr and "not supported by this build" not in r.stderr, r.stderr


def test_simulated_stacks_are_refused_with_sfolder():
    r = _run(["-o", "x.nii.gz", "-i", "s.nii.gz", "--simulatedStacks", "sim", "--sfolder", "slices"])
    assert r.returncode != 0 and "--sfolder" in r.stderr and "belong to no stack" in r.stderr and "not supported by this build" not in r.stderr, r.stderr


def test_the_end_to_end_case_is_fair_on_the_oracle(oracle_mod, tmp_path):
    """The case of tests/test_slice_quality_gpu.py's command-line test, through the Python pre-processing and the host twin over the CPU
    oracle with the command line's schedule: the restatement gives the corrupted slice the smallest ncc of its stack, or the robust
    statistics exclude it.  (What the GPU test asserts of the product.)"""
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
    factors = pp.MatchStackIntensitiesWithMasking(stacks, T, vol_mask, 700.0, together=False)
    slices, attrs, slice_t, stack_index = pp.CreateSlicesAndTransformations(stacks, T, [2.2] * 3)
    slices = pp.MaskSlices(slices, attrs, slice_t, vol_mask)
    prob = pp.build_problem(tattr, vol_mask, slices, attrs, slice_t, stack_index)
    orc = oracle_mod.OracleReconstruction(prob, oracle_mod.CANON)
    drv = irtkReconstruction(orc, prob.ns, max_intensity=prob.max_intensity, min_intensity=prob.min_intensity)
    drv.SetSmoothingParameters(ref.SCHEDULE["delta"], ref.SCHEDULE["last_lambda"])
    drv.SpeedupOff()
    drv.reconstruct_iteration(ref.SCHEDULE["rec_last"])
    orc.RestoreSliceIntensities(factors, prob.stack_index)
    drv.ScaleVolumeGPU()
    inside = np.asarray(orc.SimulateSlices(), bool)
    sums = ref.sums(orc.slices, orc.simslices, orc.simweights, orc.weights, drv._scale_gpu)
    ncc = np.array([ref.derive(s)[0] for s in sums])
    si = np.asarray(prob.stack_index)
    first = int(np.flatnonzero(si == ref.CORRUPT_STACK)[0])
    bad = first + ref.CORRUPT_SLICE                    # (cropping may drop leading slices: located below by its content instead)
    included = (drv._slice_weight_gpu >= 0.5) & inside
    mine = np.flatnonzero((si == ref.CORRUPT_STACK) & included & ~np.isnan(ncc))
    print("ncc of stack", ref.CORRUPT_STACK, np.round(ncc[si == ref.CORRUPT_STACK], 4), "weights", np.round(drv._slice_weight_gpu[si == ref.CORRUPT_STACK], 3))
    assert int((si == ref.CORRUPT_STACK).sum()) == 8, "the crop is expected to keep every slice of the stack"
    assert not included[bad] or (bad in mine and ncc[bad] == ncc[mine].min() and (ncc[mine] == ncc[bad]).sum() == 1)
