"""svr_stack_motion (csrc/svr_motion.inc) and the command line's --useAutoTemplate / --autoTemplateCentral on the GPU, against the numpy
restatement of tests/test_auto_template.py (which also checks, without a GPU, that these inputs are fair and what the Gram
formulation costs on them)."""
import numpy as np
import pytest

from fetalreconstruction_amd import engine, nifti, preprocess as prep
from tests.test_auto_template import (DEVICE_TOLERANCE, cli_scores, fair, gpu_inputs, rank_score, run_cli,
                                      singular_values_svd, write_cli_case)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rec():
    r = engine.Reconstruction(0)
    yield r
    r.close()


def test_the_gram_matrix_of_integer_slices_is_exact(rec):
    """Pins the lane maps of the f64 MFMA: small integers make every sum exact, so the singular values of slices that are scaled
    unit vectors e_k * (k + 1) plus an asymmetric coupling come out as those of the exact Gram matrix -- a row / column mix-up or
    a lost tile changes them grossly.  n = 70 crosses a band of 64 columns and a tile of 16."""
    n, m = 70, 300
    rng = np.random.default_rng(5)
    a = rng.integers(-3, 4, (n, m)).astype(np.float32)
    a[np.arange(n), np.arange(n)] += 2.0 * np.arange(1, n + 1)          # an asymmetric, well separated diagonal
    s, et, r_min, score = rec.stack_motion(a)
    ref = singular_values_svd(a)
    assert np.max(np.abs(s - ref)) / ref[0] < DEVICE_TOLERANCE
    assert r_min == rank_score(ref)[2]


@pytest.mark.parametrize("name,a", list(gpu_inputs()), ids=[n for n, _ in gpu_inputs()])
def test_stack_motion_matches_the_restatement(rec, name, a):
    """Measured on the MI355X (largest |S - S_ref| / S_max per input): see DESIGN section 9b; the bound is DEVICE_TOLERANCE =
    ten times the gap between the two numpy formulations."""
    assert fair(a)
    ref = singular_values_svd(a)
    _, et0, r0, score0 = rank_score(ref)
    s, et, r_min, score = rec.stack_motion(a)
    dev = float(np.max(np.abs(s - ref)) / ref[0])
    print(f"{name}: device vs SVD {dev:.3e} (bound {DEVICE_TOLERANCE:.1e}), r_min {r_min} / {r0}, et {et:.12f} / {et0:.12f}")
    assert s.shape == ref.shape and np.all(np.diff(s) <= 0)
    assert r_min == r0
    assert dev < DEVICE_TOLERANCE
    assert abs(et - et0) < 1e-9 and abs(score - score0) < 1e-9 * max(1, r0)


def test_two_calls_return_the_same_bits(rec):
    for name, a in gpu_inputs():
        if name in ("128x128x33-moving", "40x40x256-random"):
            s1, s2 = rec.stack_motion(a), rec.stack_motion(a)
            assert np.array_equal(s1[0], s2[0]) and s1[1:] == s2[1:]


def test_refusals_are_errors_not_faults(rec):
    with pytest.raises(engine.SvrError, match="no slice in the window"):
        rec.stack_motion(np.zeros((0, 16), np.float32))                  # N = 0
    with pytest.raises(engine.SvrError, match="more slices than pixels"):
        rec.stack_motion(np.ones((5, 4), np.float32))                    # N > M
    with pytest.raises(engine.SvrError, match="zero everywhere"):
        rec.stack_motion(np.zeros((2, 16), np.float32))
    s, et, r_min, score = rec.stack_motion(np.ones((1, 4), np.float32))  # the context is still usable
    assert s[0] == 2.0 and (et, r_min, score) == (0.0, 0, 0.0)


def _template_of_dump(path):
    """(nx, ny, nz), origin of the template attributes in a --dumpProblem file (8 int32, then one svr_image_attr)"""
    raw = open(path, "rb").read()
    return tuple(int(v) for v in np.frombuffer(raw, np.int32, 3, 32)), np.frombuffer(raw, np.float64, 15, 48)[12:15]


def _expected_template(d, k):
    """CreateTemplate of stack k cropped to the mask, from the files the command line reads (a NIfTI header keeps floats)"""
    md, ma = nifti.read(d / "mask.nii.gz")
    sd, sa = nifti.read(d / f"stack{k}.nii.gz")
    c = prep.CropImage(prep.Image(sd.astype(np.float64), sa), prep.TransformMask(sa, prep.Image(md.astype(np.float64), ma), np.eye(4)))
    t, _ = prep.CreateTemplate(c.attr, 1.0)
    return (t.nx, t.ny, t.nz), np.asarray(t.origin, np.float64)


@pytest.fixture(scope="module")
def cli_case(tmp_path_factory):
    d = tmp_path_factory.mktemp("auto_template")
    return d, write_cli_case(d)


@pytest.mark.parametrize("option,central", [(None, None), ("--autoTemplateCentral", True), ("--useAutoTemplate", False)])
def test_the_command_line_takes_the_stack_the_restatement_picks(cli_case, option, central):
    """Three stacks, all -t id; stacks 0 and 2 have per-slice shifts of up to 4 mm, stack 1 has none.  Central window: 3.954,
    0.986, 3.949 -> stack 1; first third: 2.935, 2.960, 2.924 -> stack 2 (the quirk); without the option: stack 0."""
    d, common = cli_case
    dump = d / f"dump{option}.bin"
    r = run_cli(["-o", str(d / "o.nii.gz"), *common, *([option] if option else []), "--dumpProblem", str(dump)])
    assert r.returncode == 0, r.stderr[-3000:]
    if option is None:
        want = 0
        assert "motion score" not in r.stderr and "as template" not in r.stderr
    else:
        scores = cli_scores(central)
        want = int(np.argmin(scores))
        assert want == (1 if central else 2)
        assert f"Determined stack {want} as template." in r.stderr, r.stderr[-3000:]
        lines = [ln for ln in r.stderr.splitlines() if "motion score" in ln]
        assert len(lines) == 3
        for k, ln in enumerate(lines):
            assert ln.startswith(f"stack {k}: motion score ")
            assert abs(float(ln.split("motion score ")[1].split()[0]) - scores[k]) < 1e-6
    size, origin = _template_of_dump(dump)
    esize, eorigin = _expected_template(d, want)
    assert size == esize and np.allclose(origin, eorigin, rtol=0, atol=1e-9)
    others = [_expected_template(d, k)[1] for k in range(3) if k != want]
    assert all(np.max(np.abs(origin - o)) > 1e-3 for o in others)
