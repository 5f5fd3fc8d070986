"""Bias correction from the command line (csrc/svr_cli.cpp --enableBiasCorrection, --sigma, --global_bias_correction,
--low_intensity_cutoff): the options parse, and a run without the switch receives the same problem as before.  No GPU: --dryRun
stops before the engine."""
import subprocess

import pytest

from fetalreconstruction_amd import build, nifti, phantom


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    build.build()
    d = tmp_path_factory.mktemp("bias_cli")
    stacks, mask, mattr, rattr, rmask = phantom.make_stacks(2, (24, 24, 6), 1.1, 2.2, None, 1.0, 10.0, seed=4,
                                                            stack_motion_mm=0.0, stack_motion_deg=0.0)
    paths = []
    for k, st in enumerate(stacks):
        p = d / f"stack{k}.nii.gz"
        nifti.write(p, st.data, st.attr)
        paths.append(str(p))
    nifti.write(d / "mask.nii.gz", rmask, rattr)
    return d, ["-i", *paths, "-m", str(d / "mask.nii.gz"), "--resolution", "1.0", "--no_registration"]


def _run(args, **kw):
    return subprocess.run([build.CLI, *args], capture_output=True, text=True, timeout=120, **kw)


def test_help_lists_the_bias_switch():
    r = _run(["--help"])
    assert r.returncode == 0
    assert "--enableBiasCorrection" in r.stdout and "--sigma" in r.stdout and "deviation from the reference" in r.stdout


@pytest.mark.parametrize("extra", [
    ["--enableBiasCorrection", "--sigma", "8"],
    ["--enableBiasCorrection", "--sigma", "0"],                                  # sigma <= 0: no bias step, as in the reference
    ["--enableBiasCorrection", "--global_bias_correction", "1", "--low_intensity_cutoff", "0.2"],
    ["--enableBiasCorrection", "--global_bias_correction"],                      # a bare po::value<bool> switch
    ["--disableBiasCorrection"],                                                 # accepted, changes nothing
])
def test_bias_options_are_accepted(case, extra):
    d, common = case
    r = _run(["-o", str(d / "x.nii.gz"), *common, *extra, "--dryRun"])
    assert r.returncode == 0, r.stderr


def test_the_problem_does_not_depend_on_the_bias_options(case):
    d, common = case
    a, b = d / "plain.bin", d / "bias.bin"
    assert _run(["-o", str(d / "x.nii.gz"), *common, "--dumpProblem", str(a), "--dryRun"]).returncode == 0
    assert _run(["-o", str(d / "x.nii.gz"), *common, "--enableBiasCorrection", "--sigma", "8", "--dumpProblem", str(b), "--dryRun"]).returncode == 0
    assert a.read_bytes() == b.read_bytes()


def test_cpu_reconstruction_is_still_refused(case):
    d, common = case
    r = _run(["-o", str(d / "x.nii.gz"), *common, "--enableBiasCorrection", "--useCPU"])
    assert r.returncode != 0 and "not supported" in r.stderr
