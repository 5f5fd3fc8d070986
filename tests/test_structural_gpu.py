"""svr_slice_ssim (csrc/svr_ssim.inc) on the device against the numpy restatement of tests/ssim_ref.py, and the command line's
--structural end to end on the tiny phantom with one slice shifted inside its plane.  The buffers are set through svr_debug_set: no
reconstruction is needed to test a window sum.

Tolerances.  Integer data: slices and simulation in 0..255, scale 1 or 2, dyadic c1 and c2 -- the six window sums are exact in double
whatever their order, the expressions after them are evaluated in the stated order by IEEE operations on both sides, so the map is
array_equal to the restatement's float32(ssim) and the counts are equal; the per-slice sum of up to n values is within n 2^-53 sum|ssim|
of the exactly rounded one.  Random floats: the variances are differences of large moments and the order of the window sums shows.
tests/test_structural.py measures, on this very input, the largest per-pixel gap between exactly rounded window sums and sums added left
to right (ssim_ref.MEASURED: 6.4e-15 and 5.3e-15); the device adds in a third order, rows then columns, and is allowed 4 x that per
pixel.  The restatement compared against has exactly rounded window sums ("dd", asserted bit-equal to math.fsum there).  In double the
allowance is checked on the per-slice sum: n_ssim x 4 x gap plus the summation bound.  Per pixel the device's value is only available as
the float32 map, so half a float32 ulp of the value (2^-24 |ssim|) is added there: the format's rounding, nothing of the kernel's.  With
a bias field device expf and numpy's float32 exp may round differently: as tests/test_slice_quality_gpu.py does for its sums, the gap
between the restatement with float32 exp and with the float64 exp rounded to float32 is measured on the test's input (the largest per
pixel) and ten times that gap is allowed on top.  Counts and the NaN pattern are always exact."""
import subprocess

import numpy as np
import pytest

from fetalreconstruction_amd import build, engine
from tests import slice_quality_ref as qref
from tests import ssim_ref as ref

pytestmark = pytest.mark.gpu

C1, C2 = 6.5, 58.5                                     # dyadic: (0.01 L)^2 and (0.03 L)^2 of L = 255 are 6.5025 and 58.5225


@pytest.fixture(scope="module")
def rec():
    r = engine.Reconstruction(0)
    yield r
    r.close()


def load(rec, slices, sim, simw, scales, bias=None, sizes=None):
    ns, sy, sx = slices.shape
    rec.initStorageVolumes((sx, sy, ns), (1.0, 1.0, 1.0))
    sizes = sizes if sizes is not None else [(sx, sy)] * ns
    rec.FillSlices(slices, [a for a, _ in sizes], [b for _, b in sizes])
    rec.UpdateScaleVector(scales, np.ones(ns, np.float32))
    rec.debug_set(engine.BUF_SIMSLICES, sim.astype(np.float32))
    rec.debug_set(engine.BUF_SIMWEIGHTS, simw.astype(np.float32))
    if bias is not None:
        rec.set_flags(disable_bias_correction=False)       # (allocates the bias buffers of the slice grid)
        rec.debug_set(engine.BUF_BIAS, bias.astype(np.float32))


def integer_case(ns, sx, sy, seed, sizes=None, holes=0.15):
    rng = np.random.default_rng(seed)
    shp = (ns, sy, sx)
    s = rng.integers(0, 256, shp).astype(np.float32)
    s[rng.random(shp) < holes] = -1.0
    if sizes is not None:                                  # a slice smaller than the grid: the rest of its rows and columns is padding
        for i, (a, b) in enumerate(sizes):
            s[i, b:, :] = -1.0
            s[i, :, a:] = -1.0
    y = rng.integers(0, 256, shp).astype(np.float32)
    simw = rng.choice(np.array([0.5, 0.99, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0], np.float32), shp)    # float32(0.99) is not > 0.99f
    if holes < 0.1:
        simw[rng.random(shp) < 0.9] = 1.0
    scales = rng.choice(np.array([1.0, 2.0], np.float32), ns)
    return s, y, simw, scales


EXACT = [
    ("1x7x5-R3", 1, 7, 5, 3, None),                        # the window is larger than the slice
    ("3x65x33-R3", 3, 65, 33, 3, None),                    # one past a tile both ways, and slices 1 and 2 start off a float4
    ("2x32x32-R3", 2, 32, 32, 3, None),                    # whole tiles
    ("1x130x97-R3", 1, 130, 97, 3, None),                  # several ragged tiles
    ("257x16x16-R3", 257, 16, 16, 3, None),                # many slices of one tile
    ("3x65x33-R1", 3, 65, 33, 1, None),                    # the smallest radius
    ("1x40x40-R7", 1, 40, 40, 7, None),                    # the largest
    ("5x40x24-mixed-R3", 5, 40, 24, 3, [(40, 24), (17, 24), (40, 9), (1, 1), (33, 23)]),   # per-slice sizes smaller than the grid
]


def _exact(e, name, ns, sx, sy, R, sizes):
    s, y, simw, scales = integer_case(ns, sx, sy, seed=ns * 1000 + sx + R, sizes=sizes, holes=0.04 if sx * sy < 100 else 0.15)
    if ns >= 3 and sizes is None:
        s[1] = -1.0                                        # a slice that is all padding
        simw[2] = np.where(simw[2] > 0.99, np.float32(0.99), simw[2])    # ... and one the volume never covers well enough
    load(e, s, y, simw, scales, sizes=sizes)
    got, gmap = e.slice_ssim(R, C1, C2, want_map=True)
    counted, val, m = ref.ssim_map(s, y, simw, scales, R, C1, C2)
    want = ref.slice_sums(counted, val)
    assert got.shape == (ns, 2) and got.dtype == np.float64 and gmap.shape == s.shape and gmap.dtype == np.float32
    if ns >= 3 and sizes is None:
        assert want[1].tolist() == [0, 0] and want[2].tolist() == [0, 0] and got[1].tolist() == [0, 0] and got[2].tolist() == [0, 0]
    thr = ((2 * R + 1) ** 2 + 1) // 2
    V = (s != -1) & (simw > np.float32(0.99))
    assert want[:, 0].sum() > 0 and (V & (m < thr)).any() and (V & (m >= thr)).any()   # pixels on both sides of the half-window threshold
    assert np.array_equal(got[:, 0], want[:, 0]), np.argwhere(got[:, 0] != want[:, 0])[:5]
    assert np.array_equal(np.isnan(gmap), ~counted), np.argwhere(np.isnan(gmap) == counted)[:5]
    assert np.array_equal(gmap, val.astype(np.float32), equal_nan=True), np.argwhere((gmap != val.astype(np.float32)) & counted)[:5]
    bound = want[:, 0] * 2.0 ** -53 * np.array([np.abs(val[i][counted[i]]).sum() for i in range(ns)])
    err = np.abs(got[:, 1] - want[:, 1])
    print(name, "counted", int(want[:, 0].sum()), "largest error of the slice sum / bound", float(np.max(err / np.maximum(bound, 1e-300))))
    assert (err <= bound).all(), np.argwhere(err > bound)[:5]
    again, amap = e.slice_ssim(R, C1, C2, want_map=True)
    assert np.array_equal(again, got) and np.array_equal(amap.view(np.uint32), gmap.view(np.uint32))      # two calls, the same bits
    assert np.array_equal(e.slice_ssim(R, C1, C2)[0], got)                                                 # ... with and without the map


@pytest.mark.parametrize("name,ns,sx,sy,R,sizes", EXACT, ids=[c[0] for c in EXACT])
def test_integer_data_gives_the_exact_map(rec, name, ns, sx, sy, R, sizes):
    _exact(rec, name, ns, sx, sy, R, sizes)


def test_a_patch_based_context_reads_the_same_buffers():
    r = engine.Reconstruction(0)
    try:
        r.set_option("pvr", 1)                             # units are patches
        _exact(r, *EXACT[1])
    finally:
        r.close()


@pytest.fixture(scope="module")
def general():
    """the random input and its restatements, made once: (inputs, bias) -> counted, exactly summed ssim"""
    out = {}
    for name, seed in (("general", 11), ("general_bias", 12)):
        s, y, simw, scales = ref.general_case(seed=seed)
        bias = ref.general_bias(s.shape) if name == "general_bias" else None
        counted, val, m = ref.ssim_map(s, y, simw, scales, 3, *ref.GENERAL_C, bias=bias, mode="dd")
        thr = (7 * 7 + 1) // 2
        assert m.dtype == np.int64 and ((m >= thr) | (m <= thr - 1)).all()       # integers: no window sits at the threshold ambiguously
        out[name] = (s, y, simw, scales, bias, counted, val)
    return out


def _general(r, name, data, expgap):
    s, y, simw, scales, bias, counted, val = data
    load(r, s, y, simw, scales, bias)
    got, gmap = r.slice_ssim(3, *ref.GENERAL_C, want_map=True)
    again, amap = r.slice_ssim(3, *ref.GENERAL_C, want_map=True)
    want = ref.slice_sums(counted, val)
    assert want[:, 0].min() > 1000 and (~counted & (s != -1)).any()
    assert np.array_equal(got[:, 0], want[:, 0]) and np.array_equal(np.isnan(gmap), ~counted)
    per_pixel = 4.0 * ref.MEASURED[name] + 10.0 * expgap
    v = np.where(counted, val, 0.0)
    d = np.where(counted, np.abs(gmap.astype(np.float64) - v), 0.0)
    tol = np.where(counted, per_pixel + 2.0 ** -24 * np.abs(v), 0.0)
    print(name, "largest per-pixel distance of the float32 map", float(d.max()), "allowed beyond the float32 rounding", per_pixel)
    assert (d <= tol).all(), np.argwhere(d > tol)[:5]
    abs_sum = np.array([np.abs(val[i][counted[i]]).sum() for i in range(len(want))])
    bound = want[:, 0] * per_pixel + want[:, 0] * 2.0 ** -53 * abs_sum
    err = np.abs(got[:, 1] - want[:, 1])
    print(name, "slice sums: largest error", float(err.max()), "per counted pixel", float((err / want[:, 0]).max()), "allowed per pixel", per_pixel,
          "largest error / bound", float((err / bound).max()))
    assert (err <= bound).all(), np.argwhere(err > bound)[:5]
    assert np.array_equal(again, got) and np.array_equal(amap.view(np.uint32), gmap.view(np.uint32))


def test_random_data_within_four_times_the_measured_gap(rec, general):
    _general(rec, "general", general["general"], 0.0)


def test_with_a_bias_field(general):
    s, y, simw, scales, bias, counted, val = general["general_bias"]
    c64, v64, _ = ref.ssim_map(s, y, simw, scales, 3, *ref.GENERAL_C, bias=bias, exp64=True, mode="dd")
    assert np.array_equal(c64, counted)
    expgap = float(np.abs(v64[counted] - val[counted]).max())
    print("float32 exp vs rounded float64 exp, largest per-pixel gap of ssim:", expgap)
    assert expgap > 0, "numpy's float32 exp is the rounded float64 exp on this input: no gap to scale the tolerance by"
    r = engine.Reconstruction(0)
    try:
        _general(r, "general_bias", general["general_bias"], expgap)
    finally:
        r.close()


def test_refusals_are_errors_not_faults():
    import ctypes as C
    r = engine.Reconstruction(0)
    try:
        lib = r._lib
        d = C.c_double
        assert lib.svr_slice_ssim(None, 3, d(C1), d(C2), None, None) == 10001             # SVR_E_ARG, no context to keep a message
        r.initStorageVolumes((8, 6, 2), (1.0, 1.0, 1.0))
        with pytest.raises(engine.SvrError, match="slices not filled"):
            r.slice_ssim(1, C1, C2)
        s, y, simw, scales = integer_case(2, 8, 6, seed=3, holes=0.04)
        r.FillSlices(s, [8, 8], [6, 6])
        with pytest.raises(engine.SvrError, match="scale vector not set"):
            r.slice_ssim(1, C1, C2)
        r.UpdateScaleVector(scales, np.ones(2, np.float32))
        with pytest.raises(engine.SvrError, match="no simulated slices"):
            r.slice_ssim(1, C1, C2)
        r.debug_set(engine.BUF_SIMSLICES, y)
        r.debug_set(engine.BUF_SIMWEIGHTS, simw)
        first, fmap = r.slice_ssim(1, C1, C2, want_map=True)
        counted, val, _ = ref.ssim_map(s, y, simw, scales, 1, C1, C2)
        assert first[:, 0].sum() > 0 and np.array_equal(first[:, 0], counted.sum((1, 2))) and np.array_equal(fmap, val.astype(np.float32), equal_nan=True)

        def same():
            again, amap = r.slice_ssim(1, C1, C2, want_map=True)
            assert np.array_equal(again, first) and np.array_equal(amap.view(np.uint32), fmap.view(np.uint32))

        out = np.zeros((2, 2))
        p = out.ctypes.data_as(C.c_void_p)
        assert lib.svr_slice_ssim(r._h, 1, d(C1), d(C2), None, None) == 10001 and b"no array" in lib.svr_last_error(r._h)
        same()
        for radius in (0, 8, -1):
            assert lib.svr_slice_ssim(r._h, radius, d(C1), d(C2), p, None) == 10001 and b"radius" in lib.svr_last_error(r._h)
            same()
        for c1, c2 in ((-1.0, C2), (C1, -0.5), (float("inf"), C2), (C1, float("nan")), (float("nan"), C2), (C1, float("inf"))):
            with pytest.raises(engine.SvrError, match="finite and not negative"):
                r.slice_ssim(1, c1, c2)
            same()
        assert not out.any()                               # a refused call writes nothing
        r.initStorageVolumes((8, 6, 2), (1.0, 1.0, 1.0))   # a new slice grid forgets the forward projection
        r.FillSlices(s, [8, 8], [6, 6])
        r.UpdateScaleVector(scales, np.ones(2, np.float32))
        with pytest.raises(engine.SvrError, match="no simulated slices"):
            r.slice_ssim(1, C1, C2)
    finally:
        r.close()


def test_the_host_object_evaluates_decides_and_puts_it_in_force(tiny):
    """svrh_set_structural / svrh_structural_evaluate / svrh_get_structural on the tiny problem, with k = 0 and no minimum drop so that
    every judged slice below its stack's median is excluded: the sets are not empty"""
    from fetalreconstruction_amd import host
    rec = engine.Reconstruction(0)
    try:
        engine.sync_gpu(rec, tiny)
        d = host.irtkReconstruction(rec, tiny.ns, max_intensity=tiny.max_intensity, min_intensity=tiny.min_intensity)
        d.SetSmoothingParameters(150, 0.02)
        with pytest.raises(engine.SvrError, match="svrh_set_structural first"):
            d.get_structural()
        with pytest.raises(engine.SvrError, match="radius"):
            d.set_structural(True, tiny.stack_index, radius=8)
        si = np.asarray(tiny.stack_index)
        d.set_structural(True, si, radius=3, k_mad=0.0, min_drop=0.0, min_pixels=25)
        d.reconstruct_iteration(2)
        st = d.get_structural()
        assert not st["in_force"].any()                    # nothing is in force in the first outer iteration
        # the evaluation stood before MaskVolume, which leaves the slice buffers alone: the same call now gives the same sums
        c1, c2 = ref.constants(tiny.max_intensity, tiny.min_intensity)
        sums, _ = rec.slice_ssim(3, c1, c2)
        q, ex = ref.decide(si, sums, d.state()["slice_inside"], 25, 0.0, 0.0)
        assert np.array_equal(st["n_ssim"], sums[:, 0]) and np.array_equal(st["q"], q, equal_nan=True) and np.array_equal(st["pending"], ex)
        assert 0 < ex.sum() < np.isfinite(q).sum()
        d.structural_evaluate()                            # on its own: the same buffers, the same answer
        again = d.get_structural()
        assert np.array_equal(again["q"], q, equal_nan=True) and np.array_equal(again["pending"], ex)
        d.reconstruct_iteration(2)
        st2 = d.get_structural()
        assert np.array_equal(st2["in_force"], ex)         # what the first iteration found holds for the second ...
        assert (d.state()["slice_weight"][ex] == 0).all()  # ... as a force-excluded slice: weight 0 to the end of the iteration
        assert np.isfinite(st2["q"][ex]).any()             # ... and judged again (where enough of it is still covered): the set is not sticky
        d.set_structural(False)
        with pytest.raises(engine.SvrError, match="svrh_set_structural first"):
            d.get_structural()
    finally:
        rec.close()


# ---- the command line, end to end, on the tiny phantom with one slice shifted inside its plane ----------------------------------------

def _cli(args):
    return subprocess.run(["timeout", "-k", "10", "240", build.CLI, *args], capture_output=True, text=True)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    build.build()
    d = tmp_path_factory.mktemp("structural")
    one = ref.write_cli_case(d, iterations=1)
    two = [("2" if one[i - 1] == "--iterations" else a) for i, a in enumerate(one)]
    out = {}
    for name, common, extra in (("plain1", one, []),
                                ("st1", one, ["--structural"]),
                                ("rep18", one, ["--sliceReport", str(d / "rep18.tsv")]),
                                ("plain2", two, []),
                                ("st2", two, ["--structural", "--sliceReport", str(d / "st2.tsv")]),
                                ("ranks", two, ["--structural", "--sliceReport", str(d / "ranks.tsv"), "-d", "0", "0"])):
        r = _cli(["-o", str(d / f"{name}.nii.gz"), *common, *extra])
        assert r.returncode == 0, (name, r.stderr[-3000:])                # (the parent refuses the option: "not supported by this build")
        out[name] = r
    return d, out


def test_one_iteration_writes_the_same_volume(runs):
    d, out = runs
    assert "structural, iteration 0:" in out["st1"].stderr                  # evaluated ...
    assert (d / "plain1.nii.gz").read_bytes() == (d / "st1.nii.gz").read_bytes()    # ... and nothing was in force in iteration 0


def _bad_row(rows):
    assert rows[:, 0].tolist() == [0] * 8 + [1] * 8 + [2] * 8
    return int(np.flatnonzero(rows[:, 0] == ref.CORRUPT_STACK)[ref.CORRUPT_SLICE])


def test_the_shifted_slice_is_left_out_of_the_second_iteration(runs):
    d, out = runs
    names, rows = ref.read_report(d / "st2.tsv")
    assert names == ref.HEADER_EX and rows.shape == (24, 21)
    bad = _bad_row(rows)
    for k in range(3):
        print("stack", k, "ssim", np.round(rows[rows[:, 0] == k, 18], 4), "structural", rows[rows[:, 0] == k, 20])
    assert rows[bad, 20] == 1 and rows[bad, 2] == 1 and rows[bad, 4] == 0
    others = [i for i in np.flatnonzero(rows[:, 20] == 1) if i != bad]
    for i in others:
        assert rows[i, 18] < np.nanmedian(rows[rows[:, 0] == rows[i, 0], 18])
    assert len(others) <= 2
    assert set(np.unique(rows[:, 20])) <= {0.0, 1.0} and (rows[:, 19] <= rows[:, 13]).all()      # n_ssim counts some of the M-step's pixels
    lines = [ln for ln in out["st2"].stderr.splitlines() if ln.startswith("structural, iteration")]
    assert len(lines) == 2 and lines[0].startswith("structural, iteration 0:")
    named = lines[0].split("excluded slices:")[1].split()
    assert str(bad) in named and sorted(int(v) for v in named) == sorted([bad, *others])        # what iteration 0 found is what was in force in iteration 1
    assert "stack 1 judged" in lines[0]
    assert (d / "plain2.nii.gz").read_bytes() != (d / "st2.nii.gz").read_bytes()


def test_two_ranks_on_one_device_decide_alike(runs):
    d, out = runs
    assert "2 ranks" in out["ranks"].stderr
    (n1, a), (n2, b) = ref.read_report(d / "st2.tsv"), ref.read_report(d / "ranks.tsv")
    assert n1 == n2 and a.shape == b.shape
    bad = _bad_row(a)
    assert a[bad, 20] == b[bad, 20] == 1
    assert np.array_equal(a[:, [0, 12, 19]], b[:, [0, 12, 19]])            # stack_index n_px n_ssim
    rest = [c for c in range(21) if c not in (0, 12, 19)]
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(a[:, rest] - b[:, rest]) / np.maximum(np.abs(a[:, rest]), 1e-30)
    print("two ranks vs one, largest relative difference per column:", dict(zip([n1[c] for c in rest], np.nanmax(rel, 0))))
    print("structural, one rank:", a[:, 20], "two ranks:", b[:, 20])


def test_without_the_option_the_report_keeps_its_eighteen_columns(runs):
    d, out = runs
    names, rows = ref.read_report(d / "rep18.tsv")
    assert names == qref.HEADER and rows.shape == (24, 18)
    assert "structural" not in out["rep18"].stderr and "structural" not in out["plain1"].stderr
