"""svr_slice_quality (csrc/svr_quality.inc) on the device against the numpy restatement of tests/slice_quality_ref.py, and the command
line's --sliceReport / --simulatedStacks end to end.  The buffers are set through svr_debug_set: no reconstruction is needed to test a
reduction.

Tolerances.  Exact cases: every value is a small integer (or a multiple of 1/256), so every product and every partial sum is exact in
double whatever the order -- array_equal.  General case: the products are exact (24 x 24 bits), the restatement's sums are exactly
rounded (math.fsum), so what is left is the device's summation error, at most (n - 1) 2^-53 sum|term| for n terms in any order; the
bound asserted is n 2^-53 sum|term|.  With a bias field device expf and numpy's float32 exp may round differently: the gap between the
restatement with float32 exp and with the float64 exp rounded to float32 is measured on the test's own input -- per sum, the largest
over the input's 40 slices -- and ten times that gap is allowed on top of the summation bound (the gap is zero for the sums x does not
enter); n_px and n are exact.  The gap is one number per sum for the whole input, as the auto-template tests take one number over all of
theirs: a single slice's gap is a sum of some 2 900 rounding differences of either sign and comes out anywhere between nothing and the
typical size, so it does not bound what another exponential may differ by on that slice.  (The first version of this test compared slice
by slice and failed where a slice's own gap happened to cancel, e.g. 0.035 against a typical 0.7 for sum xy; on the MI355X the device's
largest distance per sum is 0.92-0.99 of the gap, i.e. the device's expf sits next to the rounded float64 exp.)"""
import subprocess

import numpy as np
import pytest

from fetalreconstruction_amd import build, engine
from tests import slice_quality_ref as ref

pytestmark = pytest.mark.gpu

CHUNK_PIX, MAX_CHUNKS = 16384, 64                      # QUAL_CHUNK_PIX, QUAL_MAX_CHUNKS of csrc/svr_quality.inc


def chunks_of(n2):
    return min(MAX_CHUNKS, max(1, -(-n2 // CHUNK_PIX)))


@pytest.fixture(scope="module")
def rec():
    r = engine.Reconstruction(0)
    yield r
    r.close()


def load(rec, slices, sim, simw, w, scales, bias=None, sizes=None):
    ns, sy, sx = slices.shape
    rec.initStorageVolumes((sx, sy, ns), (1.0, 1.0, 1.0))
    sizes = sizes if sizes is not None else [(sx, sy)] * ns
    rec.FillSlices(slices, [a for a, _ in sizes], [b for _, b in sizes])
    rec.UpdateScaleVector(scales, np.ones(ns, np.float32))
    rec.debug_set(engine.BUF_SIMSLICES, sim.astype(np.float32))
    rec.debug_set(engine.BUF_SIMWEIGHTS, simw.astype(np.float32))
    rec.debug_set(engine.BUF_WEIGHTS, w.astype(np.float32))
    if bias is not None:
        rec.set_flags(disable_bias_correction=False)       # (allocates the bias buffers of the slice grid)
        rec.debug_set(engine.BUF_BIAS, bias.astype(np.float32))


def integer_case(ns, sx, sy, seed, sizes=None):
    rng = np.random.default_rng(seed)
    shp = (ns, sy, sx)
    s = rng.integers(0, 256, shp).astype(np.float32)
    s[rng.random(shp) < 0.2] = -1.0
    if sizes is not None:                                  # a slice smaller than the grid: the rest of its rows and columns is padding
        for i, (a, b) in enumerate(sizes):
            s[i, b:, :] = -1.0
            s[i, :, a:] = -1.0
    y = rng.integers(0, 256, shp).astype(np.float32)
    simw = rng.choice(np.array([0.0, 0.5, 0.99, 1.0, 1.0, 1.0], np.float32), shp)    # float32(0.99) is not > 0.99f
    w = (rng.integers(0, 257, shp) / 256.0).astype(np.float32)
    scales = rng.choice(np.array([1.0, 2.0], np.float32), ns)
    return s, y, simw, w, scales


EXACT = [
    ("1x7x5", 1, 7, 5, None),
    ("3x65x33", 3, 65, 33, None),                          # no multiple of 4, 64 or 256; slices 1 and 2 start off a float4
    ("257x16x16", 257, 16, 16, None),                      # one more than the EM kernels' 256 slices
    ("2x127x129", 2, 127, 129, None),                      # 16383 pixels: one below the second chunk
    ("2x128x128", 2, 128, 128, None),                      # 16384: the last size with one chunk
    ("2x145x113", 2, 145, 113, None),                      # 16385: two chunks, and slice 1 starts one float past a float4
    ("1x300x301", 1, 300, 301, None),                      # six chunks
    ("5x40x24-mixed", 5, 40, 24, [(40, 24), (17, 24), (40, 9), (1, 1), (33, 23)]),
]


def _exact(e, name, ns, sx, sy, sizes):
    s, y, simw, w, scales = integer_case(ns, sx, sy, seed=ns * 1000 + sx, sizes=sizes)
    if ns >= 3:
        s[1] = -1.0                                        # a slice that is all padding
        simw[2] = np.where(simw[2] > 0.99, np.float32(0.99), simw[2])    # ... and one the volume never covers well enough
    load(e, s, y, simw, w, scales, sizes=sizes)
    got = e.slice_quality()
    assert e.get_option("quality_chunks") == chunks_of(sx * sy)
    want = ref.sums(s, y, simw, w, scales)
    assert got.shape == (ns, 10) and got.dtype == np.float64
    if ns >= 3:
        assert want[1].tolist() == [0] * 10 and want[2, 0] > 0 and want[2, 1:].tolist() == [0] * 9
    assert want[:, 1].sum() > 0
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


@pytest.mark.parametrize("name,ns,sx,sy,sizes", EXACT, ids=[c[0] for c in EXACT])
def test_integer_data_gives_the_exact_sums(rec, name, ns, sx, sy, sizes):
    _exact(rec, name, ns, sx, sy, sizes)


@pytest.mark.parametrize("name,ns,sx,sy,sizes", [EXACT[1], EXACT[5]], ids=[EXACT[1][0], EXACT[5][0]])
def test_a_patch_based_context_reads_the_same_buffers(name, ns, sx, sy, sizes):
    r = engine.Reconstruction(0)
    try:
        r.set_option("pvr", 1)                             # units are patches
        _exact(r, name, ns, sx, sy, sizes)
    finally:
        r.close()


def test_the_chunk_count_changes_where_the_formula_says(rec):
    assert [chunks_of(n) for n in (1, 16383, 16384, 16385, 32768, 32769, 64 * 16384, 10 ** 8)] == [1, 1, 1, 2, 2, 3, 64, 64]
    for sx, sy, want in ((127, 129, 1), (128, 128, 1), (145, 113, 2)):
        s, y, simw, w, scales = integer_case(2, sx, sy, seed=7)
        load(rec, s, y, simw, w, scales)
        rec.slice_quality()
        assert rec.get_option("quality_chunks") == want


def general_case(seed=11, ns=40, sx=96, sy=80):
    rng = np.random.default_rng(seed)
    shp = (ns, sy, sx)
    s = rng.uniform(1.0, 1000.0, shp).astype(np.float32)
    s[rng.random(shp) < 0.1] = -1.0
    scales = rng.uniform(0.8, 1.2, ns).astype(np.float32)
    y = (np.abs(s) * scales[:, None, None] + rng.normal(0.0, 30.0, shp)).astype(np.float32)
    simw = rng.uniform(0.9, 1.0, shp).astype(np.float32)
    w = rng.uniform(0.0, 1.0, shp).astype(np.float32)
    return s, y, simw, w, scales


def test_random_data_within_the_summation_bound(rec):
    s, y, simw, w, scales = general_case()
    load(rec, s, y, simw, w, scales)
    got = rec.slice_quality()
    want = ref.sums(s, y, simw, w, scales)
    assert np.array_equal(got[:, :2], want[:, :2]) and want[:, 1].min() > 100
    bound = want[:, 1:2] * 2.0 ** -53 * ref.abs_sums(s, y, simw, w, scales)
    err = np.abs(got[:, 2:] - want[:, 2:])
    print("largest error / bound per sum:", np.round((err / bound).max(0), 4))
    assert (err <= bound).all()
    assert np.array_equal(rec.slice_quality(), got)                      # two calls, the same bits


def test_with_a_bias_field():
    s, y, simw, w, scales = general_case(seed=12)
    bias = np.random.default_rng(13).uniform(-0.3, 0.3, s.shape).astype(np.float32)
    want = ref.sums(s, y, simw, w, scales, bias)
    gap = np.abs(want - ref.sums(s, y, simw, w, scales, bias, exp64=True))
    bound = want[:, 1:2] * 2.0 ** -53 * ref.abs_sums(s, y, simw, w, scales, bias)
    r = engine.Reconstruction(0)
    try:
        load(r, s, y, simw, w, scales, bias)
        got = r.slice_quality()
        again = r.slice_quality()
    finally:
        r.close()
    err = np.abs(got - want)
    scale = np.abs(want).max(0)
    print("float32 exp vs rounded float64 exp, largest gap per sum / largest sum:", (gap.max(0) / scale)[2:])
    print("device vs float32 exp, largest distance per sum / largest sum:       ", (err.max(0) / scale)[2:])
    assert np.array_equal(got[:, :2], want[:, :2])
    assert gap[:, [2, 4, 6, 7, 8]].max() > 0, "numpy's float32 exp is the rounded float64 exp on this input: no gap to scale the tolerance by"
    d64 = np.abs(got - ref.sums(s, y, simw, w, scales, bias, exp64=True))
    print("device vs rounded float64 exp, largest distance per sum / largest sum:", (d64.max(0) / scale)[2:])
    tol = 10.0 * gap[:, 2:].max(0) + bound                 # the gap of this input per sum, not of one slice (module docstring)
    assert (err[:, 2:] <= tol).all(), np.argwhere(err[:, 2:] > tol)[:5]
    assert np.array_equal(got, again)


def test_refusals_are_errors_not_faults():
    r = engine.Reconstruction(0)
    try:
        lib = r._lib
        assert lib.svr_slice_quality(None, None) == 10001                # SVR_E_ARG, no context to keep a message
        out = np.zeros((2, 10))
        r.initStorageVolumes((8, 4, 2), (1.0, 1.0, 1.0))
        with pytest.raises(engine.SvrError, match="slices not filled"):
            r.slice_quality()
        s, y, simw, w, scales = integer_case(2, 8, 4, seed=3)
        r.FillSlices(s, [8, 8], [4, 4])
        with pytest.raises(engine.SvrError, match="scale vector not set"):
            r.slice_quality()
        r.UpdateScaleVector(scales, np.ones(2, np.float32))
        with pytest.raises(engine.SvrError, match="no simulated slices"):
            r.slice_quality()
        assert r.get_option("quality_chunks") == -1                      # nothing was launched
        r.debug_set(engine.BUF_SIMSLICES, y)
        r.debug_set(engine.BUF_SIMWEIGHTS, simw)
        r.debug_set(engine.BUF_WEIGHTS, w)
        assert lib.svr_slice_quality(r._h, None) == 10001 and b"no array" in lib.svr_last_error(r._h)
        assert np.array_equal(r.slice_quality(), ref.sums(s, y, simw, w, scales))     # the context is still usable
        r.initStorageVolumes((8, 4, 2), (1.0, 1.0, 1.0))                 # a new slice grid forgets the forward projection
        r.FillSlices(s, [8, 8], [4, 4])
        r.UpdateScaleVector(scales, np.ones(2, np.float32))
        with pytest.raises(engine.SvrError, match="no simulated slices"):
            r.slice_quality()
    finally:
        r.close()


# ---- the command line, end to end, on the corrupted tiny phantom of tests/test_slice_quality.py ---------------------------------------

def _cli(args):
    return subprocess.run(["timeout", "-k", "10", "240", build.CLI, *args], capture_output=True, text=True)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    build.build()
    d = tmp_path_factory.mktemp("slice_report")
    common = ref.write_cli_case(d)
    out = {}
    for name, extra in (("plain", []),
                        ("report", ["--sliceReport", str(d / "report.tsv"), "--simulatedStacks", str(d / "sim_"), "--dumpProblem", str(d / "dump.bin")]),
                        ("ranks", ["--sliceReport", str(d / "report2.tsv"), "--simulatedStacks", str(d / "sim2_"), "-d", "0", "0"])):
        r = _cli(["-o", str(d / f"{name}.nii.gz"), *common, *extra])
        assert r.returncode == 0, (name, r.stderr[-3000:])                # (the parent refuses the option: "not supported by this build")
        out[name] = r
    return d, out


def test_the_volume_does_not_depend_on_the_options(runs):
    d, out = runs
    assert (d / "plain.nii.gz").read_bytes() == (d / "report.nii.gz").read_bytes()


def test_the_report_of_a_run(runs):
    d, out = runs
    names, rows = ref.read_report(d / "report.tsv")
    assert names == ref.HEADER
    assert rows.shape == (24, 18) and rows[:, 0].tolist() == [0] * 8 + [1] * 8 + [2] * 8
    assert np.array_equal(rows[:, 1:4].sum(1), np.ones(24))
    assert (rows[:, 13] <= rows[:, 12]).all() and rows[:, 12].max() > 100
    mine = np.flatnonzero(rows[:, 0] == ref.CORRUPT_STACK)
    bad = mine[ref.CORRUPT_SLICE]
    inc = mine[rows[mine, 1] == 1]
    print("stack", ref.CORRUPT_STACK, "ncc", rows[mine, 14], "weight", rows[mine, 4], "included", rows[mine, 1])
    assert rows[bad, 2] == 1 or (rows[bad, 1] == 1 and rows[bad, 14] == np.nanmin(rows[inc, 14]) and (rows[inc, 14] == rows[bad, 14]).sum() == 1)
    err = out["report"].stderr
    assert f"Total: {int(rows[:, 1].sum())}" in err and "Included slices:" in err and "Excluded slices:" in err and "Outside slices:" in err
    assert all(f"stack {k}: median ncc" in err for k in range(3))


def test_the_simulated_stacks(runs):
    from fetalreconstruction_amd import geometry as geo, nifti
    from tests.test_prep_oracle import _read_svr_dump
    d, out = runs
    names, rows = ref.read_report(d / "report.tsv")
    D = _read_svr_dump(str(d / "dump.bin"))
    base = 0
    for k, sa in enumerate(D["sattrs"]):
        v, a = nifti.read(d / f"sim_{k}.nii.gz")
        assert v.shape == (sa.nz, sa.ny, sa.nx)
        assert np.allclose(geo.image_to_world(a), geo.image_to_world(sa), rtol=0, atol=1e-4)
        for j in range(sa.nz):
            row = rows[base + j]
            nz = int(np.count_nonzero(v[j]))
            if row[1] == 1:
                assert 0 < nz <= row[12]
            else:
                assert nz == 0
        base += sa.nz
    assert base == len(rows)


def test_two_ranks_on_one_device_give_the_same_rows(runs):
    d, out = runs
    assert "2 ranks" in out["ranks"].stderr
    (n1, a), (n2, b) = ref.read_report(d / "report.tsv"), ref.read_report(d / "report2.tsv")
    assert n1 == n2 and a.shape == b.shape
    same = [0, 1, 2, 3, 12]                                # stack_index included excluded outside n_px
    assert np.array_equal(a[:, same], b[:, same])
    rest = [c for c in range(18) if c not in same]
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(a[:, rest] - b[:, rest]) / np.maximum(np.abs(a[:, rest]), 1e-30)
    print("two ranks vs one, largest relative difference per column:", dict(zip([n1[c] for c in rest], np.nanmax(rel, 0))))
