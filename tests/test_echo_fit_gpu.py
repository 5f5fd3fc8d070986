"""The mono-exponential fit on the device (svr_monoexp_fit, csrc/svr_fit.inc) and --echoStacks / --fit* from the command line.

Tolerances, stated once:
  * count: equal.
  * rate and amplitude against the restatement (tests/echo_fit_ref.py, float64) rounded to float32: 4 float32 ulp (np.spacing).  Both sides
    compute in double, and the inputs keep the 2 x 2 system's condition number below about 1e4, so they differ by a few ulp of double in log / exp
    times that -- far below half a float ulp: a rounding boundary at most.
  * rmse: 1e-6 of max |C|, absolute.  On nearly exact fits it is a cancellation residue with no relative meaning.
  * with Gauss-Newton iterations the same, and rmse(5) <= rmse(0) + 1e-6 max |C| on every voxel.
  * between two calls and between chunkings: bit patterns.
  * the command line: files that must be another run's are compared as bytes; the fitted maps against the restatement applied to the written
    echoes under the tolerances above; T against the truth 40 within 2e-3 relative on the cover eroded by two voxels (the scatter is linear, so
    C_k = a_k C_ramp up to the rounding of float sums of at most 4096 positive taps: under 5e-4 in ln C, over R dx = 1); two ranks against one
    as stated on the test.
Observed on one MI355X (the bounds stay): rate and amplitude 0 ulp in every case, rmse within 8.4e-10 of max |C|; T against 40 within 4.8e-7
on 7000 voxels; two ranks against one 7.2e-7 (bound 1.07e-4).
"""
import subprocess

import numpy as np
import pytest

from fetalreconstruction_amd import build
from tests import channel_ref as ref
from tests import channel_sr_ref as sr
from tests import echo_fit_ref as fr

pytestmark = pytest.mark.gpu

ULPS = 4
FLOOR = 1.0
SIZES = (1, 3, 255, 256, 257, 1000)


def _inputs(n, K):
    """A in [50, 1000], R (x_max - x_min) in [0.3, 3], 2 % multiplicative noise, float32 [K][n]; salted voxels of every special kind"""
    rng = np.random.default_rng(1000 * K + n)
    x = 10.0 * np.arange(K)
    a = rng.uniform(50.0, 1000.0, n)
    r = rng.uniform(0.3, 3.0, n) / (x[-1] - x[0])
    c = (a * np.exp(-r * x[:, None]) * (1.0 + 0.02 * rng.standard_normal((K, n)))).astype(np.float32)
    assert c.min() > FLOOR

    def salt(i, kind):
        if kind == "all unusable":
            c[:, i] = 0.0
        elif kind == "one usable":
            c[1:, i] = -1.0
        elif kind == "two usable":
            c[1:K - 1, i] = np.nan
        elif kind == "a nan":
            c[1, i] = np.nan
        elif kind == "a negative":
            c[0, i] = -3.0
        elif kind == "the floor":
            c[K - 1, i] = FLOOR
        elif kind == "an inf":
            c[K - 1, i] = np.inf
    kinds = ("all unusable", "one usable", "two usable", "a nan", "a negative", "the floor", "an inf")
    if n == 3:
        salt(1, "all unusable"); salt(2, "one usable")
    elif n >= 255:                                           # spread over the array, the last voxel (the ragged chunk's end) among them
        for q, kind in enumerate(kinds):
            salt(7 + 31 * q, kind)
        salt(n - 1, "the floor"); salt(n - 2, "two usable"); salt(254, "a nan")
    return x, c


_REF = {}


def _reference(n, K, iterations):
    """computed once per case and shared, left unchanged"""
    key = (n, K, iterations)
    if key not in _REF:
        x, c = _inputs(n, K)
        _REF[key] = tuple(np.asarray(v) for v in fr.fit(c, x, iterations, FLOOR))
        for v in _REF[key]:
            v.setflags(write=False)
    return _REF[key]


@pytest.fixture(scope="module")
def rec():
    from fetalreconstruction_amd import engine as E
    r = E.Reconstruction(0)                                  # a created context and nothing else: no geometry
    yield r
    r.close()


def _check(got, want, cmax, what):
    rate, amp, rmse, count = got
    w_rate, w_amp, w_rmse, w_count = want
    assert np.array_equal(count, w_count.astype(np.float32)), what
    worst = {}
    for name, g, w in (("rate", rate, w_rate), ("amplitude", amp, w_amp)):
        w32 = w.astype(np.float32)
        ulp = np.spacing(np.abs(w32))
        worst[name] = float(np.max(np.abs(g.astype(np.float64) - w32.astype(np.float64)) / ulp)) if g.size else 0.0
    worst["rmse / max|C|"] = float(np.max(np.abs(rmse.astype(np.float64) - w_rmse))) / cmax if rmse.size else 0.0
    print(what, "worst deviation (ulp, ulp, of max|C|):", worst)
    assert worst["rate"] <= ULPS and worst["amplitude"] <= ULPS, (what, worst)
    assert worst["rmse / max|C|"] <= 1e-6, (what, worst)
    unfit = w_amp == 0
    assert (rate[unfit] == 0).all() and (amp[unfit] == 0).all() and (rmse[unfit] == 0).all(), what


@pytest.mark.parametrize("K", [2, 16])
@pytest.mark.parametrize("n", SIZES)
def test_kernel_against_the_restatement(rec, n, K):
    x, c = _inputs(n, K)
    cmax = float(np.abs(c[np.isfinite(c)]).max())
    rec.set_option("fit_chunk", 256 if n == 1000 else 1 << 20)            # 1000: three full chunks and a ragged one
    try:
        got0 = rec.monoexp_fit(c, x, 0, FLOOR)
        got5 = rec.monoexp_fit(c, x, 5, FLOOR)
    finally:
        rec.set_option("fit_chunk", 1 << 20)
    want0, want5 = _reference(n, K, 0), _reference(n, K, 5)
    if n >= 255:
        # the salt took: every count a salted voxel can have is there, and nearly every voxel is fitted
        assert set(want0[3].tolist()) >= ({0.0, 1.0, 2.0} if K == 2 else {0.0, 1.0, 2.0, 15.0, 16.0})
        assert (want0[1] == 0).sum() >= 2 and (want0[1] > 0).sum() >= n - 12
    _check(got0, want0, cmax, f"n {n} K {K} iterations 0")
    _check(got5, want5, cmax, f"n {n} K {K} iterations 5")
    assert (got5[2].astype(np.float64) <= got0[2].astype(np.float64) + 1e-6 * cmax).all()
    assert (want5[2] <= want0[2] + 1e-6 * cmax).all()


def test_refusals_are_errors_and_the_context_goes_on(rec):
    from fetalreconstruction_amd import engine as E
    x, c = _inputs(257, 16)
    usual = rec.monoexp_fit(c, x, 2, FLOOR)
    nan, inf = float("nan"), float("inf")
    for call, word in ((lambda: rec.monoexp_fit(None, x), "no abscissae or no volumes"), (lambda: rec.monoexp_fit(c, None), "no abscissae or no volumes"),
                       (lambda: rec.monoexp_fit(c[:1], x[:1]), "2 .. 16 volumes"), (lambda: rec.monoexp_fit(np.zeros((17, 5), np.float32), np.arange(17.0)), "2 .. 16 volumes"),
                       (lambda: rec.monoexp_fit(np.zeros((0, 5), np.float32), np.zeros(0)), "2 .. 16 volumes"),
                       (lambda: rec.monoexp_fit(c[:3], [0.0, nan, 2.0]), "not finite"), (lambda: rec.monoexp_fit(c[:3], [0.0, 1.0, inf]), "not finite"),
                       (lambda: rec.monoexp_fit(c[:3], [0.0, 1.0, 0.0]), "duplicate x"), (lambda: rec.monoexp_fit(c[:2], [-0.0, 0.0]), "duplicate x"),
                       (lambda: rec.monoexp_fit(c, x, -1), "iterations must be 0 .. 50"), (lambda: rec.monoexp_fit(c, x, 51), "iterations must be 0 .. 50"),
                       (lambda: rec.monoexp_fit(c, x, 0, -1.0), "floor"), (lambda: rec.monoexp_fit(c, x, 0, nan), "floor"),
                       (lambda: rec.monoexp_fit(c, x, 0, inf), "floor"), (lambda: rec.set_option("fit_chunk", 0), "fit_chunk")):
        with pytest.raises(E.SvrError, match=word):
            call()
    with pytest.raises(E.SvrError, match="abscissae for"):
        rec.monoexp_fit(c, x[:5])
    again = rec.monoexp_fit(c, x, 2, FLOOR)
    assert all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(usual, again))
    assert all(v.size == 0 for v in rec.monoexp_fit(np.zeros((3, 0), np.float32), [0.0, 1.0, 2.0]))     # n = 0 is fine and writes nothing
    assert rec.monoexp_fit(c, x, 50, FLOOR)[3].max() == 16                                               # the most iterations there are
    pv = E.Reconstruction(0)                                 # legal on a patch-based context
    pv.set_option("pvr", 1)
    got = pv.monoexp_fit(c, x, 2, FLOOR)
    pv.close()
    assert all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(usual, got))


def test_same_bits_again_and_with_another_chunking(rec):
    x, c = _inputs(1000, 16)
    assert rec.get_option("fit_chunk") == 1 << 20
    whole = rec.monoexp_fit(c, x, 5, FLOOR)
    again = rec.monoexp_fit(c, x, 5, FLOOR)
    rec.set_option("fit_chunk", 256)
    try:
        assert rec.get_option("fit_chunk") == 256
        cut = rec.monoexp_fit(c, x, 5, FLOOR)
    finally:
        rec.set_option("fit_chunk", 1 << 20)
    for u, v, w in zip(whole, again, cut):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32)) and np.array_equal(u.view(np.uint32), w.view(np.uint32))
    # shapes follow the volumes
    vol = rec.monoexp_fit(c[:, :990].reshape(16, 9, 10, 11), x, 5, FLOOR)
    assert all(v.shape == (9, 10, 11) and np.array_equal(v.reshape(-1).view(np.uint32), u[:990].view(np.uint32)) for u, v in zip(whole, vol))


# ---- the command line ---------------------------------------------------------------------------------------------------------------
X = (10.0, 30.0, 50.0)
T_TRUE = 40.0
T_CAP = 39.5            # run "sr": a cap below the truth


def _cli(args):
    return subprocess.run(["timeout", "-k", "10", "240", build.CLI, *args], capture_output=True, text=True)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """plain | three echoes a_k ramp with every fit output | echo 1's files as --channelStacks | the echoes with --echoIterations 2 and a cap |
    echo 1's files with --channelIterations 2 | the echoes on two ranks"""
    build.build()
    d = tmp_path_factory.mktemp("echo_fit")
    args, paths, stacks = ref.write_cli_case(d)
    err = {}

    def go(name, extra):
        r = _cli(["-o", str(d / f"{name}.nii.gz"), *args, *extra])
        assert r.returncode == 0, r.stderr[-3000:]
        err[name] = r.stderr
    ramp = lambda st: 100.0 + 2.0 * ref.pixel_world(st.attr)[..., 0] - 1.0 * ref.pixel_world(st.attr)[..., 2]
    files = [ref.write_like(d, f"echo{k}_", stacks, lambda _, st, k=k: np.exp(-X[k] / T_TRUE) * ramp(st)) for k in range(3)]
    echoes = sum((["--echoStacks", "%g" % X[k], *files[k]] for k in range(3)), [])
    fits = lambda tag: sum(([f"--fit{o}", str(d / f"{tag}_{o}.nii.gz")] for o in ("Rate", "T", "Amplitude", "Residual", "Count")), [])
    go("plain", [])
    go("echo", [*echoes, "--echoOutput", str(d / "e_"), *fits("fit")])
    go("ch1", ["--channelStacks", *files[1], "--channelOutput", str(d / "c1.nii.gz")])
    go("sr", [*echoes, "--echoOutput", str(d / "s_"), "--echoIterations", "2", *fits("sfit"), "--fitMaxT", str(T_CAP), "--fitIterations", "3"])
    go("ch1sr", ["--channelStacks", *files[1], "--channelOutput", str(d / "c1sr.nii.gz"), "--channelIterations", "2"])
    go("two", [*echoes, "--echoOutput", str(d / "t_"), *fits("tfit"), "-d", "0", "0"])
    return d, err


def _vol(d, name):
    from fetalreconstruction_amd import nifti
    return nifti.read(d / name)[0]


def test_cli_primary_volume_is_unchanged(runs):
    d, err = runs
    plain = (d / "plain.nii.gz").read_bytes()
    for name in ("echo", "ch1", "sr", "ch1sr"):
        assert (d / f"{name}.nii.gz").read_bytes() == plain, name
    for x in ("10", "30", "50"):
        assert f"--echoStacks {x} " in err["echo"] and "covered voxels" in err["echo"]
    assert "--fit over 3 echoes" in err["echo"] and "fitted voxels, median T" in err["echo"]


def test_cli_an_echo_is_the_channel_of_its_files(runs):
    d, err = runs
    assert (d / "e_1.nii.gz").read_bytes() == (d / "c1.nii.gz").read_bytes()
    assert (d / "s_1.nii.gz").read_bytes() == (d / "c1sr.nii.gz").read_bytes()
    assert (d / "e_1.nii.gz").read_bytes() != (d / "s_1.nii.gz").read_bytes()
    assert err["sr"].count("--echoIterations 2: delta") == 3 and "--channelIterations 2: delta" in err["ch1sr"]


@pytest.mark.parametrize("echo,fit,iterations,t_max", [("e_", "fit", 0, 10.0 * max(X)), ("s_", "sfit", 3, T_CAP)])
def test_cli_fit_files_are_the_restatement_of_the_written_echoes(runs, echo, fit, iterations, t_max):
    d, err = runs
    vols = np.stack([_vol(d, f"{echo}{k}.nii.gz") for k in range(3)])
    assert vols.dtype == np.float32
    want = fr.fit(vols, X, iterations, 0.0)
    got = tuple(_vol(d, f"{fit}_{o}.nii.gz") for o in ("Rate", "Amplitude", "Residual", "Count"))
    _check(got, want, float(np.abs(vols).max()), f"--fit* of {echo}")
    t = _vol(d, f"{fit}_T.nii.gz")
    assert np.array_equal(t, fr.t_map(got[0], got[1], t_max))
    fitted = got[1] > 0
    assert np.array_equal(fitted, (vols != 0).sum(0) >= 2) and fitted.sum() > 1000
    assert (t[~fitted] == 0).all() and (t[fitted] > 0).all() and t.max() <= np.float32(t_max)
    if t_max == T_CAP:
        print("capped voxels", int((t == np.float32(T_CAP)).sum()), "of", int(fitted.sum()))
        assert (t == np.float32(T_CAP)).sum() > 500


def test_cli_t_is_the_truth_inside_the_cover(runs):
    d, err = runs
    t, count = _vol(d, "fit_T.nii.gz"), _vol(d, "fit_Count.nii.gz")
    inner = sr.erode(count == 3, 2)
    worst = float(np.abs(t[inner] / T_TRUE - 1.0).max())
    print("T against 40 on the eroded cover (%d voxels): worst relative deviation %.3g" % (int(inner.sum()), worst))
    assert inner.sum() >= 500 and worst <= 2e-3


def test_cli_two_ranks_on_one_device(runs):
    """The existing two-rank channel tests allow a volume 2e-5 of its maximum.  On the eroded cover (12 mm from the centre at most) the ramp
    100 + 2 x - z lies in 100 +- sqrt(5) 12 = [73, 127] and the echo's maximum anywhere in the mask (15 mm) is below 134, so a voxel's value is more
    than half its echo's maximum and ln C_k moves by at most 2 * 2e-5.  R is linear in the ln C_k with coefficients c_k = w_k (x_k - xw) / sum w
    (x - xw)^2, w_k = a_k^2 (the data are an exact exponential, so the weights' own change is of second order), and dT / T = T dR:
    factor = 2 T sum |c_k|, about 5.3."""
    d, err = runs
    assert "2 ranks" in err["two"]
    w = np.exp(-2.0 * np.asarray(X) / T_TRUE)
    xw = (w * X).sum() / w.sum()
    coeff = w * (np.asarray(X) - xw) / (w * (np.asarray(X) - xw) ** 2).sum()
    factor = 2.0 * T_TRUE * np.abs(coeff).sum()
    c1, c2 = _vol(d, "fit_Count.nii.gz"), _vol(d, "tfit_Count.nii.gz")
    assert np.array_equal(c1, c2)
    for k in range(3):
        assert np.array_equal(_vol(d, f"e_{k}.nii.gz") != 0, _vol(d, f"t_{k}.nii.gz") != 0)
    t1, t2 = _vol(d, "fit_T.nii.gz"), _vol(d, "tfit_T.nii.gz")
    inner = sr.erode(c1 == 3, 2)
    worst = float(np.abs(t2[inner] / t1[inner] - 1.0).max())
    print("two ranks against one: T on the eroded cover, worst relative deviation %.3g (factor %.3f, bound %.3g)" % (worst, factor, factor * 2e-5))
    assert inner.sum() >= 500 and 5.0 < factor < 5.6 and worst <= factor * 2e-5
