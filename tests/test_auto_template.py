"""Automatic template selection (csrc/svr_cli.cpp --useAutoTemplate / --autoTemplateCentral over svr_stack_motion, csrc/svr_motion.inc):
the numpy restatement of the reference's score (stackMotionEstimator.cpp:67-164 + reconstruction.cc:565-591), the inputs the GPU tests
of tests/test_auto_template_gpu.py use, and what the command line does without a GPU.

The restatement exists in two formulations -- the singular values of A, and the square roots of the eigenvalues of A^T A in double,
which is what the engine computes -- and this file checks that they agree on every input of the GPU tests: their difference is what
squaring the condition number costs, independent of the code under test, and ten times it is the GPU tests' tolerance."""
import subprocess

import numpy as np
import pytest

from fetalreconstruction_amd import build, geometry as geo, nifti, phantom, preprocess as prep

THRESHOLD = 0.99
GUARD = 1e-6            # no error(r) of an input may lie this close to the threshold: r_min must not hang on round-off


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def rank_score(s):
    """steps 4-5: (errors, et, r_min, score) from descending singular values, in double"""
    s = np.asarray(s, np.float64)
    norm_all = np.sqrt(np.sum(s * s))
    errors = np.array([np.sqrt(np.sum(s[:r] * s[:r])) / norm_all for r in range(len(s))])     # r never reaches num_ev
    et, r_min = 0.0, -1
    for r, e in enumerate(errors):
        if e < THRESHOLD:
            et, r_min = float(e), r
    return errors, et, r_min, et * r_min


def singular_values_svd(a):
    """a: float32 [n][m] (slice after slice = the columns of the reference's column-major M x N matrix)"""
    return np.linalg.svd(a.astype(np.float64).T, compute_uv=False)


def singular_values_gram(a):
    a64 = a.astype(np.float64)
    ev = np.linalg.eigvalsh(a64 @ a64.T)[::-1]
    return np.sqrt(np.maximum(ev, 0.0))


def normalise(stack):
    """step 1: the whole (cropped) stack's min / max, in double, rounded to float once"""
    d = np.asarray(stack, np.float64)
    lo, hi = d.min(), d.max()
    return ((d - lo) / (hi - lo)).astype(np.float32)


def window(stack, central=False):
    """steps 1-2 on a cropped stack [nz][ny][nx]: float32 [N][M], N = int(nz / 3.0) slices from the first one (the reference's code)
    or from (nz - N) // 2 (its comment; --autoTemplateCentral)"""
    nz = stack.shape[0]
    n = int(nz / 3.0)
    first = (nz - n) // 2 if central else 0
    return normalise(stack)[first:first + n].reshape(n, -1)


def stack_score(cropped, central=False):
    return rank_score(singular_values_svd(window(cropped, central)))[3]


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def motion_stack(shape, in_plane, spacing, radius, shift_mm, seed, noise_sigma=5.0, average=700.0, origin=(0.37, 0.29, 0.2),
                 orientation="ax"):
    """An axial phantom stack whose slices were acquired at different in-plane positions: slice k is the phantom seen through a
    translation drawn from [-shift_mm, shift_mm]^2 (phantom.make_stacks only moves whole stacks).  shift_mm = 0: no motion.
    Returns (data float32 [nz][ny][nx], attributes)."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    attr = geo.ImageAttributes(nx, ny, nz, in_plane, in_plane, spacing, *phantom._ORIENT[orientation], origin=np.array(origin))
    kk, jj, ii = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    w = np.stack([ii, jj, kk, np.ones_like(ii)], -1).astype(np.float64) @ geo.image_to_world(attr).T
    ax = phantom._ORIENT[orientation]
    sh = rng.uniform(-shift_mm, shift_mm, (nz, 2)) if shift_mm > 0 else np.zeros((nz, 2))
    w3 = w[..., :3] + sh[:, 0, None, None, None] * ax[0] + sh[:, 1, None, None, None] * ax[1]
    val = phantom.phantom_intensity(w3, radius) * average / 0.55 + rng.normal(0.0, noise_sigma, w3.shape[:-1])
    return np.maximum(val, 0.0).astype(np.float32), attr


SHAPES = [((64, 64), 1), ((100, 93), 7), ((128, 128), 33), ((96, 96), 100), ((40, 40), 256)]      # ((nx, ny), N)
KINDS = ("still", "moving", "random")


def gpu_input(shape, n, kind, seed=11):
    """float32 [N][M] in [0, 1]: N phantom slices without / with inter-slice shifts, or uniform random numbers"""
    nx, ny = shape
    if kind == "random":
        return np.random.default_rng(seed).random((n, nx * ny), dtype=np.float32)
    fov = 0.8 * min(nx, ny)
    d, _ = motion_stack((nx, ny, n), 1.0, fov / max(n, 8), 0.45 * fov, 3.0 if kind == "moving" else 0.0, seed,
                        origin=(0.37, 0.29, 0.0))
    return normalise(d).reshape(n, -1)


def gpu_inputs():
    for shape, n in SHAPES:
        for kind in KINDS:
            yield f"{shape[0]}x{shape[1]}x{n}-{kind}", gpu_input(shape, n, kind)


def formulation_gap(a):
    """max |S_svd - S_gram| / S_max: what the Gram matrix costs on this input"""
    s, g = singular_values_svd(a), singular_values_gram(a)
    return float(np.max(np.abs(s - g)) / s[0])


# the largest formulation_gap over gpu_inputs() is 2.473e-14 (40x40x256-moving; the others lie between 0 and 1.1e-14):
# test_the_measured_gap_is_the_one_the_tolerance_was_made_from keeps this constant honest, the GPU tests allow the device ten times it
FORMULATION_GAP = 2.5e-14
DEVICE_TOLERANCE = 10.0 * FORMULATION_GAP


def fair(a):
    """the issue's condition: no error(r) within GUARD of the threshold"""
    return bool(np.all(np.abs(rank_score(singular_values_svd(a))[0] - THRESHOLD) > GUARD))


# ---- the command line's case: three stacks, the one that did not move is not the first --------------------------------------------
CLI_SHAPE, CLI_IN_PLANE, CLI_SPACING, CLI_RADIUS = (48, 48, 24), 1.1, 1.6, 16.0
CLI_SHIFTS = (4.0, 0.0, 4.0)                 # mm; stack 1 is motion-free
CLI_SEEDS = (41, 42, 43)


def cli_stacks():
    """[(data, attributes)]: the stacks' grids differ by sub-voxel offsets, so the template made from each is recognisable"""
    return [motion_stack(CLI_SHAPE, CLI_IN_PLANE, CLI_SPACING, CLI_RADIUS, s, seed, origin=(0.37 + 0.31 * k, 0.29 - 0.23 * k, 0.2 + 0.19 * k))
            for k, (s, seed) in enumerate(zip(CLI_SHIFTS, CLI_SEEDS))]


def cli_mask():
    """a ball of CLI_RADIUS mm around the origin on a 1 mm grid -> (data [z][y][x], attributes)"""
    n = int(np.ceil(2.0 * CLI_RADIUS + 6.0))
    a = geo.ImageAttributes(n, n, n, 1.0, 1.0, 1.0)
    c = (np.arange(n) - (n - 1) / 2.0) ** 2
    return ((c[:, None, None] + c[None, :, None] + c[None, None, :]) < CLI_RADIUS ** 2).astype(np.float32), a


def cli_scores(central):
    """what reconstruction.cc:569-586 computes for the three stacks (all -t id): TransformMask, CropImage, the score"""
    md, ma = cli_mask()
    mask = prep.Image(md.astype(np.float64), ma)
    out = []
    for d, a in cli_stacks():
        st = prep.Image(d.astype(np.float64), a)
        out.append(stack_score(prep.CropImage(st, prep.TransformMask(a, mask, np.eye(4))).data, central))
    return out


def write_cli_case(d):
    paths = []
    for k, (data, attr) in enumerate(cli_stacks()):
        nifti.write(d / f"stack{k}.nii.gz", data, attr)
        paths.append(str(d / f"stack{k}.nii.gz"))
    md, ma = cli_mask()
    nifti.write(d / "mask.nii.gz", md, ma)
    return ["-i", *paths, "-m", str(d / "mask.nii.gz"), "--resolution", "1.0", "--no_registration", "--iterations", "1"]


def run_cli(args, **kw):
    return subprocess.run([build.CLI, *args], capture_output=True, text=True, timeout=600, **kw)


# ---- tests (no GPU) --------------------------------------------------------------------------------------------------------------
def test_help_names_both_options():
    build.build()
    r = run_cli(["--help"])
    assert r.returncode == 0
    assert "--useAutoTemplate" in r.stdout and "--autoTemplateCentral" in r.stdout
    central = r.stdout[r.stdout.index("  --autoTemplateCentral"):]
    assert "deviation" in central.split("\n  --")[0]


@pytest.fixture(scope="module")
def bias_case(tmp_path_factory):
    """the fixture of tests/test_bias_cli.py"""
    build.build()
    d = tmp_path_factory.mktemp("auto_template_cli")
    stacks, mask, mattr, rattr, rmask = phantom.make_stacks(2, (24, 24, 6), 1.1, 2.2, None, 1.0, 10.0, seed=4,
                                                            stack_motion_mm=0.0, stack_motion_deg=0.0)
    paths = []
    for k, st in enumerate(stacks):
        nifti.write(d / f"stack{k}.nii.gz", st.data, st.attr)
        paths.append(str(d / f"stack{k}.nii.gz"))
    nifti.write(d / "mask.nii.gz", rmask, rattr)
    return d, ["-i", *paths, "-m", str(d / "mask.nii.gz"), "--resolution", "1.0", "--no_registration"]


@pytest.mark.parametrize("option", ["--useAutoTemplate", "--autoTemplateCentral"])
def test_dry_run_refuses_the_selection_and_says_why(bias_case, option):
    d, common = bias_case
    r = run_cli(["-o", str(d / "x.nii.gz"), *common, option, "--dryRun"])
    assert r.returncode != 0
    assert "--dryRun" in r.stderr and "engine context" in r.stderr and "not supported by this build" not in r.stderr


def test_the_default_path_is_untouched(bias_case):
    d, common = bias_case
    a, b = d / "plain.bin", d / "other.bin"
    assert run_cli(["-o", str(d / "x.nii.gz"), *common, "--dumpProblem", str(a), "--dryRun"]).returncode == 0
    assert run_cli(["-o", str(d / "x.nii.gz"), *common, "--useNMI", "--dumpProblem", str(b), "--dryRun"]).returncode == 0
    assert a.read_bytes() == b.read_bytes()


@pytest.mark.parametrize("name,a", list(gpu_inputs()), ids=[n for n, _ in gpu_inputs()])
def test_the_two_formulations_agree_on_the_gpu_tests_inputs(name, a):
    assert fair(a), "an error(r) of this input lies within 1e-6 of 0.99: choose another seed"
    e1, et1, r1, _ = rank_score(singular_values_svd(a))
    e2, et2, r2, _ = rank_score(singular_values_gram(a))
    print(f"{name}: r_min {r1}, et {et1:.9f}, formulation gap {formulation_gap(a):.3e}")
    assert r1 == r2 and abs(et1 - et2) < 1e-9


def test_the_measured_gap_is_the_one_the_tolerance_was_made_from():
    worst = max(formulation_gap(a) for _, a in gpu_inputs())
    print(f"largest formulation gap {worst:.3e}")
    assert worst <= 2.0 * FORMULATION_GAP      # (other LAPACK kernels move the last digit of the measurement, not its size)


def test_the_rank_loop_never_sums_every_singular_value():
    """the reference's quirks, kept: r stops at num_ev - 1; one slice scores 0 with r_min 0; equal singular values"""
    assert rank_score([3.0])[1:] == (0.0, 0, 0.0)
    errors, et, r_min, score = rank_score(np.ones(4))
    assert np.allclose(errors, [0.0, 0.5, np.sqrt(0.5), np.sqrt(0.75)]) and r_min == 3 and score == 3 * np.sqrt(0.75)


def test_the_window_is_the_first_third_and_the_stack_s_range_normalises_it():
    st = np.arange(7 * 2 * 3, dtype=np.float64).reshape(7, 2, 3)
    w = window(st)
    assert w.shape == (2, 6) and w[0, 0] == 0.0 and np.isclose(w[1, 5], 11.0 / 41.0)      # max is outside the window
    assert np.array_equal(window(st, central=True), normalise(st)[2:4].reshape(2, 6))


def test_the_cli_case_separates_the_motion_free_stack_on_the_central_window():
    """Central window (--autoTemplateCentral): the three stacks score 3.954, 0.986, 3.949 -- the motion-free stack 1 is the smallest
    by a factor of four.  First third (the reference's window): 2.935, 2.960, 2.924 -- there the motion-free stack scores worst and
    stack 2 is chosen: the first slices of a stack cropped to a ball show little of the phantom, and what separates them is
    noise.  That is the quirk; the command-line test asserts agreement with this restatement, not a wish.  The two smallest
    first-third scores differ by 0.011 (et by 0.0036), far above any round-off."""
    c, f = cli_scores(True), cli_scores(False)
    print("central", c, "first third", f)
    assert int(np.argmin(c)) == 1 and c[1] * 3.0 < min(c[0], c[2])
    assert int(np.argmin(f)) == 2 and np.sort(f)[1] - np.sort(f)[0] > 5e-3
