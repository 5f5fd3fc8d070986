"""The windowed cross correlation in the IRTK registration schedule (--useLNCC; csrc/irtk_reg.cpp with SVRH_SIM_LNCC, csrc/svr_lncc.inc
on the device).  No GPU here: the numpy restatement of the metric (tests/lncc_ref.py) checked against its own definition, the C++
schedule over that restatement on the case the metric exists for -- slices under a smooth multiplicative bias the volume does not
have --, packages, determinism, refusals and the command line."""
import numpy as np
import pytest

from fetalreconstruction_amd import geometry as geo, host
from tests import lncc_ref
from tests.test_nmi_registration import _analytic_slice_case, _max_error_mm, _package_case, _run, cli_case  # noqa: F401  (cli_case: a fixture)


# ---- the restatement against the definition -------------------------------------------------------------------------------------------
def _direct(valid, t, s, R):
    """the definition with python integers, window by window"""
    ty, tx = valid.shape
    need = ((2 * R + 1) ** 2 + 1) // 2
    N = S = 0
    kmap = np.full((ty, tx), lncc_ref.NOT_COUNTED, np.int64)
    for y in range(ty):
        for x in range(tx):
            if not valid[y, x]:
                continue
            w = (slice(max(0, y - R), y + R + 1), slice(max(0, x - R), x + R + 1))
            v = valid[w]
            tt, ss = [int(a) for a in t[w][v]], [int(a) for a in s[w][v]]
            m = len(tt)
            A = m * sum(a * b for a, b in zip(tt, ss)) - sum(tt) * sum(ss)
            B = m * sum(a * a for a in tt) - sum(tt) ** 2
            C = m * sum(b * b for b in ss) - sum(ss) ** 2
            if m < need or B <= 0:
                continue
            q = 0.0 if C == 0 else (float(A) / float(B)) * (float(A) / float(C)) * (-1.0 if A < 0 else 1.0)
            k = int(np.floor(q * 2.0 ** 24 + 0.5))
            N, S, kmap[y, x] = N + 1, S + k, k
    return N, S, kmap


@pytest.mark.parametrize("R", [1, 3, 7])
def test_restatement_is_the_definition(R):
    rng = np.random.default_rng(R)
    for ty, tx, top in ((5, 7, 300), (19, 23, 32768)):
        valid = rng.random((ty, tx)) < 0.85
        t = np.where(valid, rng.integers(0, top, (ty, tx)), 0)
        s = np.where(valid, rng.integers(0, top, (ty, tx)), 0)
        N, S, k = lncc_ref.lncc_from_samples(valid, t, s, R)
        wN, wS, wk = _direct(valid, t, s, R)
        assert (N, S) == (wN, wS) and np.array_equal(k, wk)
        assert N > 0 or (2 * R + 1 > min(ty, tx))


def test_restatement_is_invariant_to_a_linear_change_of_the_target_and_knows_flat_images():
    rng = np.random.default_rng(4)
    ty, tx, R = 30, 34, 3
    valid = np.ones((ty, tx), bool)
    t, s = rng.integers(0, 900, (ty, tx)), rng.integers(0, 900, (ty, tx))
    N, S, k = lncc_ref.lncc_from_samples(valid, t, s, R)
    inner = (slice(R, ty - R), slice(R, tx - R))                    # the windows that are not clipped
    # every pixel but the twenty at the corners whose clipped window holds fewer than 25 samples (4 x 4, 4 x 5, 4 x 6, 5 x 4, 6 x 4)
    assert N == ty * tx - 20 and (k[inner] != lncc_ref.NOT_COUNTED).all() and k[0, 0] == lncc_ref.NOT_COUNTED and k[1, 1] != lncc_ref.NOT_COUNTED
    for a, b in ((1, 17), (3, 0), (7, 250)):
        k2 = lncc_ref.lncc_from_samples(valid, a * t + b, s, R)[2]
        # A -> a A, B -> a^2 B: q = A^2 / (B C) keeps its value, to the rounding of the two quotients (2^-52 each) -- one step of
        # the 2^-24 grid at the very most
        assert np.abs(k2[inner].astype(np.int64) - k[inner]).max() <= 1
    # the same image on both sides: q = 1 exactly, every pixel scores 2^24
    same = lncc_ref.lncc_from_samples(valid, t, 5 * t + 3, R)
    assert same[0] == N and same[1] == N << 24
    anti = lncc_ref.lncc_from_samples(valid, t, 5000 - 5 * t, R)
    assert anti[1] == -(N << 24)
    flat_s = lncc_ref.lncc_from_samples(valid, t, np.full_like(s, 41), R)
    assert flat_s[0] == N and flat_s[1] == 0 and (flat_s[2][inner] == 0).all()   # counted, scores nothing
    flat_t = lncc_ref.lncc_from_samples(valid, np.full_like(t, 41), s, R)
    assert flat_t[0] == 0 and flat_t[1] == 0 and (flat_t[2] == lncc_ref.NOT_COUNTED).all()
    # fewer than half a window of samples: not counted
    few = np.zeros((ty, tx), bool)
    few[::3, ::3] = True
    assert lncc_ref.lncc_from_samples(few, np.where(few, t, 0), np.where(few, s, 0), R)[0] == 0
    assert lncc_ref.similarity([(0, 0)]) == 0.0 and lncc_ref.similarity([(2, 3 << 24), (1, 0)]) == 1.0


# ---- the case the metric exists for: a multiplicative bias over the slices ------------------------------------------------------------
def ramp(slices, ratio):
    """every slice times exp(ln(ratio) (i - 24) / 48) along x: a smooth gain that changes by `ratio` across the 48 columns"""
    i = np.arange(slices.shape[-1], dtype=np.float64)
    return (slices * np.exp(np.log(ratio) * (i - 24) / 48)).astype(np.float32)


def _lncc_backend(R=3):
    return host.NccBackend(lncc_ref.evaluator(R))


def _errors(ts):
    return np.array([_max_error_mm(m, np.eye(4)) for m in ts])


def test_lncc_registers_slices_under_a_bias_ramp_where_cc_makes_them_worse(oracle_mod):
    slices, attrs, P, ra, vol = _analytic_slice_case(seed=11)
    cc_be = lambda: host.NccBackend(lambda t, M, s: oracle_mod.ncc_evaluate(t, M, s)[1])   # noqa: E731
    before = _errors(P)
    biased = (ramp(slices, 10.0), attrs, P, ra, vol)
    be = _lncc_backend()
    ln, nev = host.SliceToVolumeRegistration(None, *biased, backend=be, similarity="lncc", radius=3)
    cc, _ = host.SliceToVolumeRegistration(None, *biased, backend=cc_be())
    e_ln, e_cc = _errors(ln), _errors(cc)
    print("ramp ratio 10: error before", np.round(before, 2), "LNCC", np.round(e_ln, 2), "CC", np.round(e_cc, 2), "evaluations", nev)
    assert nev > 100 and be.calls < nev / 3
    assert np.median(e_ln) < 0.5 * np.median(before)
    assert np.median(e_cc) > np.median(before)
    assert np.median(e_ln) < 0.4 * np.median(e_cc)
    # determinism: the same transformations and evaluation counts again; the default radius is 3
    ln2, nev2 = host.SliceToVolumeRegistration(None, *biased, backend=_lncc_backend(), similarity="lncc")
    assert np.array_equal(ln, ln2) and nev == nev2
    # the unbiased slices: both metrics register them
    plain = (slices, attrs, P, ra, vol)
    ln0, _ = host.SliceToVolumeRegistration(None, *plain, backend=_lncc_backend(), similarity="lncc")
    cc0, _ = host.SliceToVolumeRegistration(None, *plain, backend=cc_be())
    print("no ramp: LNCC", np.round(_errors(ln0), 2), "CC", np.round(_errors(cc0), 2))
    assert np.median(_errors(ln0)) < 1.5 and np.median(_errors(cc0)) < 1.5
    # another radius is another metric
    ln5, _ = host.SliceToVolumeRegistration(None, *biased, backend=_lncc_backend(5), similarity="lncc", radius=5)
    assert not np.array_equal(ln5, ln)


def test_package_to_volume_runs_the_schedule_with_lncc():
    a, data, t_pack, ra, vol = _package_case()
    start = np.tile(np.eye(4), (a.nz, 1, 1))
    be = _lncc_backend()
    t, nev = host.PackageToVolume(None, [data], [a], [2], start, ra, vol, backend=be, similarity="lncc")
    err = [_max_error_mm(t[k], t_pack[k % 2], 10.0) for k in range(a.nz)]
    before = [_max_error_mm(np.eye(4), t_pack[k % 2], 10.0) for k in range(a.nz)]
    print("LNCC package registration: error before", np.round(before[:2], 2), "after", np.round(err[:2], 2), "evaluations", nev)
    assert nev > 50 and be.calls < nev and max(err) < 0.6 * min(before)
    for k in range(2, a.nz):
        assert np.allclose(t[k], t[k % 2], atol=1e-12)
    t2, nev2 = host.PackageToVolume(None, [data], [a], [2], start, ra, vol, backend=_lncc_backend(), similarity="lncc")
    assert np.array_equal(t, t2) and nev == nev2


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_radius_and_backend_are_checked():
    args = (None, np.zeros((1, 2, 2), np.float32), [geo.ImageAttributes(2, 2, 1, 1, 1, 1)], np.eye(4)[None],
            geo.ImageAttributes(2, 2, 2, 1, 1, 1), np.zeros((2, 2, 2), np.float32))
    zero = host.NccBackend(lambda t, M, s: (0, 0))
    for bad in (0, 8, -1, 2.5):
        with pytest.raises(ValueError):
            host.SliceToVolumeRegistration(*args, backend=zero, similarity="lncc", radius=bad)
    with pytest.raises(ValueError):                                   # a radius without the metric it belongs to
        host.SliceToVolumeRegistration(*args, backend=zero, similarity="cc", radius=3)
    with pytest.raises(ValueError):                                   # a joint-histogram evaluator for LNCC
        host.SliceToVolumeRegistration(*args, backend=host.NmiBackend(lambda *a: np.zeros((64, 64), np.uint32)), similarity="lncc")
    assert host.SIMILARITY["lncc"] == 2
    # the C entry points refuse what the keyword cannot express: a radius beyond 7, a radius on another metric, an unknown metric
    import ctypes as C
    lib = host._reg_lib()
    g, t, v = np.full((1, 2, 2), -1, np.float32), np.eye(4).reshape(1, 16).copy(), np.zeros((2, 2, 2), np.float32)
    at, ra = (host.ImageAttr * 1)(host.ImageAttr.of(args[2][0])), host.ImageAttr.of(args[4])
    p = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731
    for sim, ok in ((2 | 8 << 8, False), (2 | 255 << 8, False), (0 | 3 << 8, False), (1 | 3 << 8, False), (3, False), (2 | 7 << 8, True),
                    (2, True)):
        err = C.create_string_buffer(256)
        rc = lib.svrh_slice_to_volume_registration_ex(None, C.byref(zero.struct), None, sim, 1, p(g), 2, 2, at, p(t), C.byref(ra), p(v), 0,
                                                      None, err)
        assert (rc == 0) == ok, (sim, rc, err.value)


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def test_help_lists_use_lncc_as_a_deviation():
    r = _run(["--help"])
    assert r.returncode == 0 and "--useLNCC" in r.stdout and "--lnccRadius" in r.stdout
    line = [ln for ln in r.stdout.splitlines() if ln.lstrip().startswith("--useLNCC")]
    assert line and "deviation from the reference" in line[0]


def test_use_lncc_does_not_change_the_problem(cli_case):   # noqa: F811
    d, common = cli_case
    a, b = d / "plain_l.bin", d / "lncc.bin"
    assert _run(["-o", str(d / "x.nii.gz"), *common, "--no_registration", "--dumpProblem", str(a), "--dryRun"]).returncode == 0
    r = _run(["-o", str(d / "x.nii.gz"), *common, "--no_registration", "--useLNCC", "--lnccRadius", "5", "--dumpProblem", str(b), "--dryRun"])
    assert r.returncode == 0, r.stderr
    assert a.read_bytes() == b.read_bytes()


def test_use_lncc_refusals(cli_case):   # noqa: F811
    d, common = cli_case
    r = _run(["-o", str(d / "x.nii.gz"), *common, "--useLNCC", "--useGPUReg"])
    assert r.returncode != 0 and "--useGPUReg" in r.stderr and "cross-correlation only" in r.stderr
    r = _run(["-o", str(d / "x.nii.gz"), *common, "--useLNCC", "--useNMI"])
    assert r.returncode != 0 and "--useNMI" in r.stderr and "--useLNCC" in r.stderr
    for bad in ("0", "8"):
        r = _run(["-o", str(d / "x.nii.gz"), *common, "--useLNCC", "--lnccRadius", bad])
        assert r.returncode != 0 and "--lnccRadius" in r.stderr
