"""The guided volume update of a channel's SR iterations (--channelGuide; svr_channel_sr_guide) without a GPU: the numpy restatement of
tests/channel_guide_ref.py pinned against the oracle's own update where the two must agree, the noisy recovery case on the oracle leg, whose
three ratios are the yardstick of the device's leg (tests/test_channel_guide_gpu.py), and the command line's option checks under
--dryRun."""
import subprocess

import numpy as np
import pytest

from fetalreconstruction_amd import build
from tests import channel_guide_ref as gr
from tests import channel_sr_ref as sr
from tests.twins.reconstruction import irtkReconstruction
from tests.util import rel_err, run_to_state

TOL_A7 = 1e-6           # row a7: the volume update against the oracle's, of the volume's maximum (tests/test_channel_sr_gpu.py)


@pytest.fixture(scope="module")
def state(tiny, oracle_mod):
    """the oracle at state "scale" on the tiny problem: the motion and weights the iterations hold fixed"""
    orc = oracle_mod.OracleReconstruction(tiny, oracle_mod.CANON)
    d = irtkReconstruction(orc, tiny.ns, max_intensity=tiny.max_intensity, min_intensity=tiny.min_intensity)
    d.SetSmoothingParameters(150, 0.02)
    run_to_state(d, "scale")
    return tiny, orc


@pytest.mark.parametrize("adaptive", [False, True])
def test_restatement_without_a_guide_is_the_oracle_s_update(state, oracle_mod, adaptive):
    """(a) no guide, and a constant guide (only differences enter): orc_regularization's result to TOL_A7; the two restatements bit for bit"""
    po = oracle_mod
    prob, orc = state
    c = np.random.default_rng(5).integers(0, 256, prob.slices.shape).astype(np.float32)
    sw = orc.slice_weights
    p = dict(sr.parameters(prob, orc, c), adaptive=adaptive)
    vol, cover = sr.seed(po, orc, prob, c, sw)
    sim, simw = sr.forward(po, orc, prob, vol)
    gate, e = sr.factors(prob, orc, c, sim, simw)
    addon, cmap = sr.scatter(po, orc, prob, e, gate, sw)
    want = sr.update(po, prob, vol, addon, cmap, p)
    plain = gr.update(po, prob, vol, addon, cmap, p)
    const = gr.update(po, prob, vol, addon, cmap, p, guide=np.full(prob.nvox, 7.0, np.float32), delta_g=3.0)
    only = gr.update(po, prob, vol, addon, cmap, p, guide=vol, delta_g=p["delta"], guide_only=True)      # the channel itself as the guide
    moved = gr.update(po, prob, vol, addon, cmap, p, guide=gr.smooth_guide_with_a_step(prob), delta_g=20.0)
    print("adaptive", adaptive, "restatement against the oracle", rel_err(plain, want), "constant guide", rel_err(const, want), "a guide moves it by", rel_err(moved, want))
    assert cover.sum() > 1000 and rel_err(want, vol) > 1e-3
    assert rel_err(plain, want) <= TOL_A7 and rel_err(const, want) <= TOL_A7
    assert np.array_equal(plain.view(np.uint32), const.view(np.uint32))
    assert rel_err(only, want) <= TOL_A7
    assert rel_err(moved, want) > 1e-3


def test_guided_recovery_on_the_oracle_leg(state, oracle_mod):
    """(b) a noisy channel (sigma 40 on a 100 | 300 step), lambda_c 0.05, eight iterations: the guided update (delta 120, delta_g 20, the guide a
    200 | 800 step across the same plane) comes closer to the truth than the unguided one does at the default delta or at delta 120.  The three
    ratios are recorded (tests/channel_guide_ref.py) for the device's leg."""
    prob, orc = state
    d, w, g = (gr.oracle_leg(oracle_mod, orc, prob, which) for which in ("default", "wide", "guided"))
    case = gr.noisy_case(oracle_mod, orc, prob)
    print("oracle leg, RMSE after 8 iterations over the average's: unguided delta %.9g -> %.9g, unguided delta %.9g -> %.9g, guided -> %.9g"
          % (case["p_default"]["delta"], d, case["p_wide"]["delta"], w, g))
    assert g < d and g < w
    for got, rec in ((d, gr.ORACLE_UNGUIDED_DEFAULT), (w, gr.ORACLE_UNGUIDED_WIDE), (g, gr.ORACLE_GUIDED)):
        assert abs(got / rec - 1) < 1e-3, (got, rec)


# ---- the command line ------------------------------------------------------------------------------------------------------------------------
def _run(args):
    build.build()
    return subprocess.run([build.CLI, *args], capture_output=True, text=True, timeout=300)


def _refused(r, *words):
    assert r.returncode != 0 and "not supported by this build" not in r.stderr, r.stderr
    for w in words:
        assert w in r.stderr, (w, r.stderr)


CH = ["--channelStacks", "a.nii.gz", "--channelOutput", "c.nii.gz"]
BASE = ["-o", "x.nii.gz", "-i", "s.nii.gz"]


def test_help_lists_the_options_as_deviations():
    r = _run(["--help"])
    assert r.returncode == 0
    for o in ("--channelGuide ", "--channelGuideDelta", "--channelGuideOnly"):
        line = [l for l in r.stdout.splitlines() if l.strip().startswith(o)]
        assert line and "deviation from the reference" in line[0], o


@pytest.mark.parametrize("extra", [[], CH, [*CH, "--channelIterations", "0"], ["--labelStacks", "a.nii.gz", "--labelOutput", "l.nii.gz"]])
def test_guide_refused_without_channel_iterations(extra):
    _refused(_run([*BASE, *extra, "--channelGuide", "--dryRun"]), "--channelGuide", "--channelIterations", "--channelStacks")


@pytest.mark.parametrize("option", [["--channelGuideDelta", "10"], ["--channelGuideOnly"]])
def test_guide_options_refused_without_the_guide(option):
    _refused(_run([*BASE, *CH, "--channelIterations", "4", *option, "--dryRun"]), "--channelGuideDelta / --channelGuideOnly", "--channelGuide")


@pytest.mark.parametrize("value", ["0", "-3", "nan", "inf"])
def test_bad_guide_delta_is_refused_before_any_file_is_read(value):
    _refused(_run([*BASE, *CH, "--channelIterations", "4", "--channelGuide", "--channelGuideDelta", value, "--dryRun"]), "--channelGuideDelta", "positive")


def test_guide_refused_with_sfolder():
    _refused(_run([*BASE, *CH, "--channelIterations", "4", "--channelGuide", "--sfolder", "slices", "--dryRun"]), "--sfolder", "belong to no stack")


def test_accepted_next_to_channel_iterations(tmp_path):
    from tests import channel_ref as ref
    args, paths, stacks = ref.write_cli_case(tmp_path)
    ch = ref.write_like(tmp_path, "ch", stacks, lambda k, st: np.full(st.data.shape, 8.0))
    r = _run(["-o", str(tmp_path / "x.nii.gz"), *args, "--channelStacks", *ch, "--channelOutput", str(tmp_path / "c.nii.gz"), "--channelIterations", "4",
              "--channelGuide", "--channelGuideDelta", "12.5", "--channelGuideOnly", "--dryRun"])
    assert r.returncode == 0, r.stderr
