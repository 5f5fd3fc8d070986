"""svr_resample_to_reconstruction (csrc/svr_seed.inc) on the device against the numpy restatement of tests/resample_ref.py, and the
command line's --referenceVolume end to end.

Tolerances.  Exact cases: the data are integers 0..255 and the matrix has only dyadic entries (0, +-1, +-0.5, 2, 2.5, offsets in
quarters), so every coordinate, weight, product and sum is exact in double; the cases are laid out so that a valid voxel's W is 0.5
or 1 (asserted on the restatement), so the one division is exact too, every value is a multiple of 1/64 below 256 and the statistics
are exact sums whatever the order: array_equal for the volume and all five statistics.  (Half-voxel shifts along three axes next to
padding give W = 0.625, 0.75 ...: quotients with 24 significant bits whose squares no longer add up exactly in double -- the volume is
still equal bit for bit there, the sum of squares depends on the order by its last bit.)
Oblique case: both sides evaluate the same expressions in double and round once, so a valid voxel may differ by at most one float ulp
(a coordinate difference of 1e-13 voxels times the largest neighbour difference is far below half an ulp, except at a rounding tie);
validity and n must be equal, which the test secures beforehand on the restatement: no voxel has |W - 0.5| < 1e-9 and no coordinate
lies within 1e-9 of an integer.  The three sums: the device's summation error, at most n 2^-53 sum|term|, plus the ulp each term may
differ by (for v^2: 2 |v| ulp + ulp^2)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from fetalreconstruction_amd import build, engine, geometry as geo
from tests import resample_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rec():
    r = engine.Reconstruction(0)
    yield r
    r.close()


def set_grid(r, shape, mask):
    vz, vy, vx = shape
    r.InitReconstructionVolume((vx, vy, vz), (1.0, 1.0, 1.0))
    if mask is not None:
        r.setMask((vx, vy, vz), (1.0, 1.0, 1.0), mask)


def random_mask(shape, seed, p=0.8):
    return (np.random.default_rng(seed).random(shape) < p).astype(np.float32)


def shell(n=16):
    """integers everywhere, with a shell of -1 two voxels thick well inside the grid"""
    v = ref.ints((n, n, n), 21)
    c = (np.arange(n) - (n - 1) / 2.0) ** 2
    r = np.sqrt(c[:, None, None] + c[None, :, None] + c[None, None, :])
    v[(r > 3.5) & (r < 5.5)] = -1.0
    return v


HALF = np.array([[1, 0, 0, 0.5], [0, 1, 0, 0.5], [0, 0, 1, 0.5]])
HALF_X = np.array([[1, 0, 0, 0.5], [0, 1, 0, 0], [0, 0, 1, 0]])       # next to padding W is 0, 0.5 or 1: the division stays exact
# name, target shape [vz][vy][vx], source, matrix, padding, mask (None = none set, on a context of its own)
EXACT = [
    ("5x4x3<-4x5x6-permuted-flipped", (3, 4, 5), ref.ints((6, 5, 4), 11), np.array([[0, -1, 0, 3], [1, 0, 0, 0], [0, 0, 1, 2.0]]), -1.0, random_mask((3, 4, 5), 12)),
    ("33x17x9<-20x20x20-half-voxel", (9, 17, 33), ref.ints((20, 20, 20), 13), HALF, -1.0, random_mask((9, 17, 33), 14, 0.9)),
    ("16x16x16<-8x8x40-anisotropic", (16, 16, 16), ref.ints((40, 8, 8), 15), np.array([[0.5, 0, 0, 0], [0, 0.5, 0, 0], [0, 0, 2.5, 0.25]]), -1.0,
     random_mask((16, 16, 16), 16)),
    ("16x16x16<-outside", (16, 16, 16), ref.ints((16, 16, 16), 17), np.array([[1, 0, 0, 100.0], [0, 1, 0, 0], [0, 0, 1, 0]]), -2.0, random_mask((16, 16, 16), 18)),
    ("16x16x16<-shell-of-padding", (16, 16, 16), shell(), HALF_X, -1.0, np.ones((16, 16, 16), np.float32)),
    ("16x16x16-no-mask", (16, 16, 16), ref.ball(), HALF_X, -1.0, None),
]


@pytest.mark.parametrize("name,shape,src,m,padding,mask", EXACT, ids=[c[0] for c in EXACT])
def test_dyadic_cases_are_exact(rec, name, shape, src, m, padding, mask):
    r = rec if mask is not None else engine.Reconstruction(0)
    try:
        set_grid(r, shape, mask)
        want, valid, wstats = ref.resample(src, m, shape, padding, mask)
        W, _ = ref.weights(src, m, shape, padding)
        assert np.isin(W[valid], (0.5, 1.0)).all()                 # the one division is by a power of two: every value a short dyadic number
        got, stats = r.resample_to_reconstruction(src, m, padding)
    finally:
        if r is not rec:
            r.close()
    print(name, "stats", stats.tolist(), "valid", int(valid.sum()), "of", valid.size)
    if "outside" in name:
        assert wstats.tolist() == [0, 0, 0, np.inf, -np.inf] and (want[mask != 0] == -2).all() and (want[mask == 0] == -1).all()
    elif "shell" in name:
        assert 0 < (~valid).sum() < valid.size // 4            # padding inside the mask
    else:
        assert valid.sum() > valid.size // 8
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert np.array_equal(stats, wstats), (stats, wstats)


def oblique_case(seed=31):
    sa, ra = ref.oblique_pair()
    rng = np.random.default_rng(seed)
    src = rng.uniform(1.0, 1000.0, (sa.nz, sa.ny, sa.nx)).astype(np.float32)
    src[rng.random(src.shape) < 0.05] = -1.0
    shape = (ra.nz, ra.ny, ra.nx)
    return src, ref.compose(sa, ra), shape, random_mask(shape, seed + 1, 0.85)


def test_oblique_grid_within_one_ulp(rec):
    src, m, shape, mask = oblique_case()
    # no ties on the restatement: validity and the base voxels cannot differ by a last bit of a coordinate
    W, _ = ref.weights(src, m, shape)
    p = np.stack(ref.coordinates(m, shape))
    assert np.abs(W - 0.5).min() >= 1e-9 and np.abs(p - np.round(p)).min() >= 1e-9
    want, valid, wstats = ref.resample(src, m, shape, -1.0, mask)
    assert valid.sum() > 5000 and ((W < 0.5) & (mask != 0)).sum() > 1000 and ((W >= 0.5) & (W < 1.0 - 1e-9)).sum() > 1000
    set_grid(rec, shape, mask)
    got, stats = rec.resample_to_reconstruction(src, m, -1.0)
    assert np.array_equal(got != -1, want != -1) and np.array_equal((got != -1) & (mask != 0), valid) and stats[0] == wstats[0]
    ulp = np.spacing(np.abs(want[valid])).astype(np.float64)
    d = np.abs(got[valid].astype(np.float64) - want[valid].astype(np.float64))
    print("voxels that differ:", int((d > 0).sum()), "of", int(valid.sum()), " largest difference / ulp:", float((d / ulp).max()))
    assert (d <= ulp).all()
    v = np.abs(want[valid].astype(np.float64))
    n = wstats[0]
    bound1 = n * 2.0 ** -53 * v.sum() + ulp.sum()
    bound2 = n * 2.0 ** -53 * (v * v).sum() + (2 * v * ulp + ulp * ulp).sum()
    print("sum errors / bounds:", abs(stats[1] - wstats[1]) / bound1, abs(stats[2] - wstats[2]) / bound2)
    assert abs(stats[1] - wstats[1]) <= bound1 and abs(stats[2] - wstats[2]) <= bound2
    assert abs(stats[3] - wstats[3]) <= np.spacing(np.float32(wstats[3])) and abs(stats[4] - wstats[4]) <= np.spacing(np.float32(wstats[4]))
    assert stats[3] == got[valid].min() and stats[4] == got[valid].max()           # the device's own result, exactly


def test_two_calls_give_the_same_bits(rec):
    src, m, shape, mask = oblique_case(seed=33)
    set_grid(rec, shape, mask)
    a, sa = rec.resample_to_reconstruction(src, m)
    b, sb = rec.resample_to_reconstruction(src, m)
    assert a.tobytes() == b.tobytes() and sa.tobytes() == sb.tobytes() and sa[0] > 0


def test_install_and_scale(rec):
    name, shape, src, m, padding, mask = EXACT[1]
    set_grid(rec, shape, mask)
    before = rec.syncCPU().copy()
    plain, stats = rec.resample_to_reconstruction(src, m, padding)
    assert np.array_equal(rec.syncCPU(), before)                          # without the flag the reconstructed volume is left alone
    out, _ = rec.resample_to_reconstruction(src, m, padding, install=True)
    assert np.array_equal(out, plain) and np.array_equal(rec.syncCPU().reshape(shape), plain)
    doubled, stats2 = rec.resample_to_reconstruction(src, m, padding, install=True, scale=2.0)
    valid = (mask != 0) & (plain != -1)
    assert 0 < valid.sum() < valid.size
    assert np.array_equal(doubled[valid], 2 * plain[valid]) and (doubled[~valid] == -1).all() and np.array_equal(stats2, stats)
    assert np.array_equal(rec.syncCPU().reshape(shape), doubled)
    _, _, wstats = ref.resample(src, m, shape, padding, mask, scale=2.0)
    assert np.array_equal(stats2, wstats)
    none, stats3 = rec.resample_to_reconstruction(src, m, padding, want_volume=False)
    assert none is None and np.array_equal(stats3, stats)


def test_refusals_are_errors_not_faults():
    r = engine.Reconstruction(0)
    try:
        lib, h = r._lib, r._h
        src = ref.ints((4, 4, 4), 41)
        m = np.ascontiguousarray(np.eye(4)[:3])
        st, out = np.zeros(5), np.zeros((4, 4, 4), np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        u3 = lambda *v: (C.c_uint32 * 3)(*v)
        call = lambda size, s, mm, flags, o, stats: lib.svr_resample_to_reconstruction(h, size, s, mm, C.c_float(-1.0), flags, C.c_float(1.0), o, stats)
        assert lib.svr_resample_to_reconstruction(None, u3(4, 4, 4), p(src), p(m), C.c_float(-1.0), 0, C.c_float(1.0), None, p(st)) == 10001
        assert call(u3(4, 4, 4), p(src), p(m), 0, p(out), p(st)) == 10002 and b"InitReconstructionVolume first" in lib.svr_last_error(h)
        set_grid(r, (4, 4, 4), None)
        for args, msg in (((u3(4, 4, 4), None, p(m), 0, p(out), p(st)), b"no source volume"),
                          ((None, p(src), p(m), 0, p(out), p(st)), b"no source volume"),
                          ((u3(4, 4, 4), p(src), None, 0, p(out), p(st)), b"no matrix"),
                          ((u3(4, 4, 4), p(src), p(m), 0, p(out), None), b"no array for the statistics"),
                          ((u3(4, 0, 4), p(src), p(m), 0, p(out), p(st)), b"a source size is zero"),
                          ((u3(2048, 2048, 512), p(src), p(m), 0, p(out), p(st)), b"more than 2^31 - 1 voxels"),      # 2^31: refused before a byte is read
                          ((u3(65536, 65536, 65536), p(src), p(m), 0, p(out), p(st)), b"more than 2^31 - 1 voxels"),
                          ((u3(4, 4, 4), p(src), p(m), 4, p(out), p(st)), b"unknown flag")):
            assert call(*args) == 10001 and msg in lib.svr_last_error(h), (msg, lib.svr_last_error(h))
        bad = m.copy()
        bad[1, 3] = np.nan
        assert call(u3(4, 4, 4), p(src), p(bad), 0, p(out), p(st)) == 10001 and b"not finite" in lib.svr_last_error(h)
        got, stats = r.resample_to_reconstruction(src, m)                 # the context is still usable
        assert np.array_equal(got, src) and stats[0] == 64
    finally:
        r.close()


# ---- the command line, end to end, on the tiny phantom (three stacks of 32 x 32 x 8) with every slice moved on its own ----------------

MOTION_MM, MOTION_DEG = 1.5, 3.0        # per slice, uniform in +-: enough that one iteration without slice registration shows it
REG_LINE = "slice-to-volume registration:"


def _cli(args):
    return subprocess.run(["timeout", "-k", "10", "300", build.CLI, *args], capture_output=True, text=True)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from fetalreconstruction_amd import nifti
    build.build()
    d = tmp_path_factory.mktemp("reference_volume")
    common, rattr, rmask = ref.write_cli_case(d, MOTION_MM, MOTION_DEG)
    out = {}

    def run(name, extra, ok=True):
        r = _cli(["-o", str(d / f"{name}.nii.gz"), *common, *extra])
        if ok:
            assert r.returncode == 0, (name, r.stderr[-3000:])            # (the parent refuses the option: "is not supported by this build")
        out[name] = r

    run("C", ["--iterations", "3"])
    seed = ["--referenceVolume", str(d / "C.nii.gz")]
    run("A", ["--iterations", "1"])
    run("A2", ["--iterations", "1"])
    run("B", ["--iterations", "1", *seed])
    run("B2", ["--iterations", "1", *seed, "-d", "0", "0"])
    run("P2", ["--iterations", "2"])
    run("S2", ["--iterations", "2", *seed])
    run("N", ["--iterations", "1", *seed, "--useNMI"])
    run("G", ["--iterations", "1", *seed, "--useGPUReg"])
    run("G2", ["--iterations", "1", *seed, "--useGPUReg", "-d", "0", "0"])
    # the seed on another grid: 1.5 x the voxel size, the axes permuted cyclically, shifted (written with the Python NIfTI binding)
    c, ca = nifti.read(d / "C.nii.gz")
    n = lambda k, dv: int(np.ceil(k * dv / (1.5 * dv))) + 2
    oa = geo.ImageAttributes(n(ca.ny, ca.dy), n(ca.nz, ca.dz), n(ca.nx, ca.dx), 1.5 * ca.dy, 1.5 * ca.dz, 1.5 * ca.dx, ca.yaxis.copy(), ca.zaxis.copy(),
                             ca.xaxis.copy(), origin=np.asarray(ca.origin) + np.array([1.3, -0.7, 0.9]))
    coarse, _, _ = ref.resample(c, ref.compose(ca, oa), (oa.nz, oa.ny, oa.nx), -1.0)
    nifti.write(d / "coarse.nii.gz", coarse, oa)
    run("D", ["--iterations", "1", "--referenceVolume", str(d / "coarse.nii.gz")])
    far = geo.ImageAttributes(ca.nx, ca.ny, ca.nz, ca.dx, ca.dy, ca.dz, ca.xaxis.copy(), ca.yaxis.copy(), ca.zaxis.copy(),
                              origin=np.asarray(ca.origin) + np.array([500.0, 0.0, 0.0]))
    nifti.write(d / "far.nii.gz", c, far)
    run("E", ["--iterations", "1", "--referenceVolume", str(d / "far.nii.gz")], ok=False)
    vols = {k: nifti.read(d / f"{k}.nii.gz")[0] for k in ("C", "A", "B", "D", "N", "G", "G2")}
    inside, _, _ = ref.resample(rmask, ref.compose(rattr, ca), c.shape, -1.0)
    return d, out, vols, inside >= 0.5


def test_the_option_is_accepted_and_reported(runs):
    d, out, vols, inside = runs
    err = out["S2"].stderr
    line = [ln for ln in err.splitlines() if ln.startswith("reference volume: n=")]
    assert len(line) == 1 and " mean=" in line[0] and " min=" in line[0] and " max=" in line[0] and " scale=" in line[0], err[-2000:]
    assert err.count(REG_LINE) == 2 and out["P2"].stderr.count(REG_LINE) == 1 and "similarity evaluations" in err
    assert "reference volume:" not in out["P2"].stderr
    assert out["B"].stderr.count(REG_LINE) == 1 and out["A"].stderr.count(REG_LINE) == 0


def test_registration_against_the_seed_helps(runs):
    d, out, vols, inside = runs
    assert inside.sum() > 5000
    a, b = ref.ncc(vols["A"], vols["C"], inside), ref.ncc(vols["B"], vols["C"], inside)
    print("NCC inside the mask against the 3-iteration run: 1 iteration", a, " 1 iteration seeded with it", b)
    assert b > a


def test_a_seed_on_another_grid(runs):
    d, out, vols, inside = runs
    a, dd = ref.ncc(vols["A"], vols["C"], inside), ref.ncc(vols["D"], vols["C"], inside)
    print("NCC against the 3-iteration run: 1 iteration", a, " seeded with it at 1.5 x the voxel size on a permuted, shifted grid", dd)
    assert out["D"].stderr.count(REG_LINE) == 1 and dd > a


def test_a_seed_outside_the_mask_is_an_error(runs):
    d, out, vols, inside = runs
    assert out["E"].returncode == 1 and "--referenceVolume does not overlap the mask" in out["E"].stderr, (out["E"].returncode, out["E"].stderr[-2000:])


def test_two_ranks_on_one_device_register_as_often(runs):
    d, out, vols, inside = runs
    assert "2 ranks" in out["B2"].stderr and out["B2"].stderr.count(REG_LINE) == out["B"].stderr.count(REG_LINE) == 1
    assert len([ln for ln in out["B2"].stderr.splitlines() if ln.startswith("reference volume: n=")]) == 1


def test_the_other_registrations_take_the_seed(runs):
    """--useNMI (the IRTK schedule on the joint histogram) and --useGPUReg (every rank registers its own slices against its own copy of the
    seed, -1 outside the mask) at iteration 0: accepted, the seed is reported, the registration ran and moved the slices (the volume is not
    the unseeded run's) and the volume is finite.  How much each helps on this phantom is printed, not asserted: the claim of these runs is
    that the pairing works, the claim that a seed helps is made of the default path above."""
    d, out, vols, inside = runs
    a = ref.ncc(vols["A"], vols["C"], inside)
    for k in ("N", "G", "G2"):
        assert len([ln for ln in out[k].stderr.splitlines() if ln.startswith("reference volume: n=")]) == 1
        assert np.isfinite(vols[k]).all() and vols[k].shape == vols["A"].shape and not np.array_equal(vols[k], vols["A"])
        print(k, "NCC against the 3-iteration run:", ref.ncc(vols[k], vols["C"], inside), " unseeded:", a)
    assert out["N"].stderr.count(REG_LINE) == 1 and "2 ranks" in out["G2"].stderr


def test_runs_without_the_option_repeat_bit_for_bit(runs):
    d, out, vols, inside = runs
    assert (d / "A.nii.gz").read_bytes() == (d / "A2.nii.gz").read_bytes()
