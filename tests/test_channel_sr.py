"""SR iterations on a channel (--channelIterations; svr_channel_sr_*) without a GPU: the restatement of tests/channel_sr_ref.py pinned by
facts that need no device, the recovery case on the oracle, whose two ratios are the yardstick of the device's leg
(tests/test_channel_sr_gpu.py), and the command line's option checks under --dryRun."""
import subprocess

import numpy as np
import pytest

from fetalreconstruction_amd import build
from tests import channel_sr_ref as sr
from tests.twins.reconstruction import irtkReconstruction
from tests.util import run_to_state


@pytest.fixture(scope="module")
def state(tiny, oracle_mod):
    """the oracle at state "scale" on the tiny problem: the motion and weights the iterations hold fixed"""
    orc = oracle_mod.OracleReconstruction(tiny, oracle_mod.CANON)
    d = irtkReconstruction(orc, tiny.ns, max_intensity=tiny.max_intensity, min_intensity=tiny.min_intensity)
    d.SetSmoothingParameters(150, 0.02)
    run_to_state(d, "scale")
    return tiny, orc


def test_no_iteration_is_the_seed(state, oracle_mod):
    prob, orc = state
    c = np.random.default_rng(5).integers(0, 256, prob.slices.shape).astype(np.float32)
    sw = orc.slice_weights
    c0, cover = sr.seed(oracle_mod, orc, prob, c, sw)
    vol, cov, res = sr.superresolve(oracle_mod, orc, prob, c, 0, sr.parameters(prob, orc, c), sw)
    assert cover.sum() > 1000 and (~cover).any() and not res
    assert np.array_equal(cov, cover) and np.array_equal(vol.view(np.uint32), c0.view(np.uint32))
    assert not vol[~cover].any() and 0 <= vol[cover].min() and vol[cover].max() <= 255


def test_a_pixel_without_sim_weight_contributes_nothing_whatever_its_value(state, oracle_mod):
    """The gate is the forward pass's sim-weight: where it is 0 the pixel's factors are 0 and its channel value is never read into the sums;
    where it is positive a simulated value <= 0 does not shut it."""
    prob, orc = state
    c = np.random.default_rng(6).integers(0, 256, prob.slices.shape).astype(np.float32) - np.float32(100)
    sw = orc.slice_weights
    vol, _ = sr.seed(oracle_mod, orc, prob, c, sw)
    sim, simw = sr.forward(oracle_mod, orc, prob, vol)
    P = sr.pixel_set(prob, orc)
    assert (P & (simw > 0) & (sim <= 0)).any()
    shut = P & (np.random.default_rng(7).random(P.shape) < 0.1)
    simw2 = np.where(shut, np.float32(0), simw)
    wild = np.where(shut, np.float32(1e30), c).astype(np.float32)
    g1, e1 = sr.factors(prob, orc, c, sim, simw2)
    g2, e2 = sr.factors(prob, orc, wild, sim, simw2)
    assert shut.sum() > 100 and not (g1 & shut).any() and np.array_equal(g1, g2) and np.array_equal(e1, e2) and not e1[shut].any()
    g0, e0 = sr.factors(prob, orc, c, sim, simw)
    assert (g0 & (sim <= 0)).any() and (e0[g0 & (sim <= 0)] != 0).any()
    a1, m1 = sr.scatter(oracle_mod, orc, prob, e1, g1, sw)
    a0, m0 = sr.scatter(oracle_mod, orc, prob, e0, g0, sw)
    assert not np.array_equal(m1, m0) and (m1 <= m0).all()      # the shut pixels' weights are gone from the sums too


def test_recovery_on_the_oracle(state, oracle_mod):
    """A step of 100 | 300 across an oblique plane, seen through the problem's slices: eight iterations bring the volume closer to the truth
    than the average is and shrink the weighted residual.  The two ratios are recorded for the device's leg."""
    prob, orc = state
    o = sr.oracle_recovery(oracle_mod, orc, prob, "tiny")
    print("oracle recovery: RMSE ratio %.9g, weighted residual ratio %.9g, parameters %r" % (o["rmse_ratio"], o["res_ratio"], o["p"]))
    assert o["rmse_ratio"] < 1.0 and o["res_ratio"] < 1.0
    assert abs(o["rmse_ratio"] / sr.ORACLE_RMSE_RATIO - 1) < 1e-3 and abs(o["res_ratio"] / sr.ORACLE_RESIDUAL_RATIO - 1) < 1e-3


# ---- the command line ------------------------------------------------------------------------------------------------------------------------
def _run(args):
    build.build()
    return subprocess.run([build.CLI, *args], capture_output=True, text=True, timeout=300)


def _refused(r, *words):
    assert r.returncode != 0 and "not supported by this build" not in r.stderr, r.stderr
    for w in words:
        assert w in r.stderr, (w, r.stderr)


CH = ["--channelStacks", "a.nii.gz", "--channelOutput", "c.nii.gz"]


def test_help_lists_the_options_as_deviations():
    r = _run(["--help"])
    assert r.returncode == 0
    for o in ("--channelIterations", "--channelDelta", "--channelLambda"):
        line = [l for l in r.stdout.splitlines() if l.strip().startswith(o)]
        assert line and "deviation from the reference" in line[0], o


@pytest.mark.parametrize("option", [["--channelIterations", "4"], ["--channelDelta", "10"], ["--channelLambda", "0.02"], ["--channelIterations", "0"]])
def test_refused_without_channel_stacks(option):
    _refused(_run(["-o", "x.nii.gz", "-i", "s.nii.gz", *option, "--dryRun"]), "--channelIterations", "--channelStacks")
    _refused(_run(["-o", "x.nii.gz", "-i", "s.nii.gz", "--labelStacks", "a.nii.gz", "--labelOutput", "l.nii.gz", *option, "--dryRun"]), "--channelStacks")


def test_refused_with_sfolder():
    _refused(_run(["-o", "x.nii.gz", "-i", "s.nii.gz", *CH, "--channelIterations", "4", "--sfolder", "slices", "--dryRun"]), "--sfolder", "belong to no stack")


@pytest.mark.parametrize("option,words", [(["--channelIterations", "-1"], ["--channelIterations", "negative"]),
                                          (["--channelDelta", "0"], ["--channelDelta", "positive"]),
                                          (["--channelDelta", "nan"], ["--channelDelta", "positive"]),
                                          (["--channelLambda", "-0.5"], ["--channelLambda", "positive"])])
def test_bad_values_are_refused_before_any_file_is_read(option, words):
    _refused(_run(["-o", "x.nii.gz", "-i", "s.nii.gz", *CH, *option, "--dryRun"]), *words)


def test_accepted_next_to_channel_stacks(tmp_path):
    from tests import channel_ref as ref
    args, paths, stacks = ref.write_cli_case(tmp_path)
    ch = ref.write_like(tmp_path, "ch", stacks, lambda k, st: np.full(st.data.shape, 8.0))
    r = _run(["-o", str(tmp_path / "x.nii.gz"), *args, "--channelStacks", *ch, "--channelOutput", str(tmp_path / "c.nii.gz"), "--channelIterations", "4",
              "--channelDelta", "12.5", "--channelLambda", "0.02", "--dryRun"])
    assert r.returncode == 0, r.stderr
