"""The guided volume update of a channel's SR iterations on the device (svr_channel_sr_guide, csrc/svr_channel.inc; the GUIDED kernels of
csrc/svr_regul.inc) and from the command line (--channelGuide).

The problems are tests/test_channel_gpu.py's: tiny (34^3) and awkward (31^3, stacks of 37 x 29 x 7).  Nothing there is a multiple of a tile and the
update runs in z-chunks of 4, so tile edges, chunk seams and the ring's wrap are all hit, for the three tiles of option reg_tile.

Tolerances, stated once (none is new):
  * a guide whose differences vanish (a constant), and the seed volume itself as a guide-only guide with delta_g = delta: the unguided update's
    bit patterns -- fma(0, 0, w) is w, and fma(t, t 0, 1) is 1.
  * the updated volume against the numpy restatement (tests/channel_guide_ref.py) of the SAME inputs (the device's seed and the device's
    addon | cmap): row a7's 1e-6 of the volume's maximum; the guide adds one fma in front of the same v_rsq.
  * between two calls, with the table on and off, NULL against a host pointer, and everything the call must leave alone: bit patterns.
  * recovery: within 5 % of the oracle leg's recorded ratio (the margin of tests/test_channel_sr_gpu.py::test_recovery_on_the_device: the two legs
    differ by float effects of order 1e-5, so 5 % only guards against a wrong sign, gate or constant), and below the device's own unguided ratios.
  * two ranks against one: 2e-5 of the maximum, as tests/test_channel_sr_gpu.py demands of the unguided channel.
"""
import subprocess

import numpy as np
import pytest

from fetalreconstruction_amd import build
from tests import channel_guide_ref as gr
from tests import channel_ref as ref
from tests import channel_sr_ref as sr
from tests.test_channel_gpu import _channel, _engine_at_scale, _num_den, _state
from tests.util import _snap, rel_err

pytestmark = pytest.mark.gpu

TOL_A7 = 1e-6           # row a7: the fused volume update against the restatement, of the volume's maximum


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _quot(num, den):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, num / den, np.float32(0)).astype(np.float32)


def _one_iteration(rec, c, sw, p, guide=False, delta_g=1.0, guide_only=False):
    """begin .. end with one iteration -> (the seed, cover, addon, cmap of the iteration, the volume).  guide: False = no svr_channel_sr_guide call,
    "seed" = the seed volume itself, None = the reconstruction (NULL), or a volume"""
    rec.channel_sr_begin(c, slice_weights=sw)
    num, den = _num_den(rec)
    c0 = _quot(num, den)
    rec.channel_sr_seed()
    if guide is not False:
        rec.channel_sr_guide(c0 if isinstance(guide, str) else guide, delta_g, guide_only)
    rec.channel_sr_backproject()
    addon, cmap = _num_den(rec)
    rec.channel_sr_update(p["adaptive"], p["alpha"], p["lo"], p["hi"], p["delta"], p["lam"])
    return c0, den > 0, addon, cmap, rec.channel_sr_end()


@pytest.mark.parametrize("name", ["tiny", "awkward"])
def test_a_guide_without_differences_gives_the_unguided_bits(tiny, oracle_mod, name):
    """a constant guide (joint and guide-only mode are then the unguided update and the update with b = f), and the seed volume as a guide-only guide
    with delta_g = delta: bit for bit, for both Prep forms and the three tiles"""
    prob, rec, orc = _state(name, tiny, oracle_mod)
    c = _channel(prob, 1) + np.float32(1)
    sw = orc.slice_weights.copy()
    const = np.full(prob.nvox, 123.5, np.float32)
    try:
        for adaptive in (False, True):
            p = dict(sr.parameters(prob, orc, c), adaptive=adaptive)
            for tile in (0, 1, 2):
                rec.set_option("reg_tile", tile)
                c0, cover, _, _, plain = _one_iteration(rec, c, sw, p)
                flat = _one_iteration(rec, c, sw, p, const, 7.0)[4]
                own = _one_iteration(rec, c, sw, p, "seed", p["delta"], True)[4]
                print(name, "adaptive", adaptive, "tile", tile, "cover", int(cover.sum()), "differing voxels: constant guide",
                      int((_bits(flat) != _bits(plain)).sum()), "the seed as its own guide", int((_bits(own)[cover] != _bits(plain)[cover]).sum()))
                assert cover.sum() > 1000 and rel_err(plain, c0) > 1e-3
                assert np.array_equal(_bits(flat), _bits(plain))
                assert np.array_equal(_bits(own)[cover], _bits(plain)[cover])
    finally:
        rec.set_option("reg_tile", -1)


@pytest.mark.parametrize("name", ["tiny", "awkward"])
@pytest.mark.parametrize("guide_only", [False, True])
def test_one_guided_iteration_against_the_restatement(tiny, oracle_mod, name, guide_only):
    """a random smooth guide plus a step, joint and guide-only: the restatement fed the device's own seed and the device's addon | cmap.
    Measured on one MI355X: see the printed figures (recorded in DESIGN 9e)."""
    po = oracle_mod
    prob, rec, orc = _state(name, tiny, oracle_mod)
    c = _channel(prob, 1) + np.float32(1)
    sw = orc.slice_weights.copy()
    guide, delta_g = gr.smooth_guide_with_a_step(prob), 25.0
    try:
        for adaptive, tile in ((False, -1), (True, 0), (False, 1)):
            rec.set_option("reg_tile", tile)
            p = dict(sr.parameters(prob, orc, c), adaptive=adaptive)
            plain = _one_iteration(rec, c, sw, p)[4]
            c0, cover, addon, cmap, vol = _one_iteration(rec, c, sw, p, guide, delta_g, guide_only)
            want = np.where(cover, gr.update(po, prob, c0, addon, cmap, p, guide, delta_g, guide_only), np.float32(0))
            ev = rel_err(vol, want)
            print(name, "guide only" if guide_only else "joint", "adaptive", adaptive, "tile", tile, "covered", int(cover.sum()), "rel_err volume", ev,
                  "differs from the unguided by", rel_err(vol, plain))
            assert cover.sum() > 1000
            assert ev <= TOL_A7
            assert not vol[~cover].any() and rel_err(vol, plain) > 1e-3
    finally:
        rec.set_option("reg_tile", -1)


def _iterate(rec, c, p, guide=False, delta_g=30.0, n=2):
    rec.channel_sr_begin(c)
    rec.channel_sr_seed()
    if guide is not False:
        rec.channel_sr_guide(guide, delta_g)
    for _ in range(n):
        rec.channel_sr_backproject()
        rec.channel_sr_update(p["adaptive"], p["alpha"], p["lo"], p["hi"], p["delta"], p["lam"])
    return rec.channel_sr_end()


def test_repeats_bit_for_bit_and_leaves_the_run_alone():
    """a NULL guide = the reconstruction: two calls, the table on and off, and the same volume as a host pointer give the same bits; the
    reconstruction, the simulated slices, the weights and the EM state keep theirs, and the next primary SR iteration is a twin's that never saw
    the call"""
    from fetalreconstruction_amd import engine as E
    prob = ref.awkward_problem()
    c = _channel(prob, 4) - np.float32(50)
    R_c = 255.0
    p = dict(adaptive=False, alpha=1.0, lo=-50 - 0.1 * R_c, hi=205 + 0.1 * R_c, delta=30.0, lam=0.01 * 30.0 * 30.0)
    engines = []
    for _ in range(2):                                       # the second one never sees the call
        rec, d = _engine_at_scale(prob)
        d.SuperresolutionGPU(1); d.SimulateSlicesGPU(); d.MStepGPU(1); d.EStepGPU(); d.ScaleGPU()
        engines.append((rec, d))
    (rec, d), (rec2, d2) = engines
    bufs = (E.BUF_RECONSTRUCTED, E.BUF_SIMSLICES, E.BUF_SIMWEIGHTS, E.BUF_SIMINSIDE, E.BUF_WEIGHTS, E.BUF_PSF_SUMS)

    def snapshot(r, dd):
        s = {b: r.debug_get(b).copy() for b in bufs}
        s["scale"] = np.asarray(r.GetScaleVector()).copy()
        s["driver"] = {k: v for k, (kind, v) in _snap(dd).items()}     # the slice weights, the scale vector's host copy and the EM scalars
        return s
    before = snapshot(rec, d)
    recon = rec.syncCPU().copy()
    delta_g = 0.1 * float(recon.max() - recon.min())
    assert delta_g > 0
    plain = _iterate(rec, c, p)
    v1 = _iterate(rec, c, p, None, delta_g)
    v2 = _iterate(rec, c, p, None, delta_g)
    host = _iterate(rec, c, p, recon, delta_g)
    rec.set_option("coeff_table", 0)
    fly = _iterate(rec, c, p, None, delta_g)
    rec.set_option("coeff_table", 1)
    # a second call replaces the guide: a constant one first, the reconstruction after it
    rec.channel_sr_begin(c)
    rec.channel_sr_guide(np.full(prob.nvox, 3.0, np.float32), 1.0)     # (legal before the seed)
    rec.channel_sr_seed()
    rec.channel_sr_guide(None, delta_g)
    for _ in range(2):
        rec.channel_sr_backproject()
        rec.channel_sr_update(p["adaptive"], p["alpha"], p["lo"], p["hi"], p["delta"], p["lam"])
    twice = rec.channel_sr_end()
    print("guided by the reconstruction: differs from the unguided by", rel_err(v1, plain))
    assert np.abs(v1).max() > 0 and rel_err(v1, plain) > 1e-4
    for other in (v2, host, fly, twice):
        assert np.array_equal(_bits(v1), _bits(other))
    assert np.array_equal(_bits(_iterate(rec, c, p)), _bits(plain))           # the guide went with its call
    fb = rec.fallbacks()
    assert fb["scatter_to_atomics"] == 0 and fb["gather_to_tiles"] == 0
    after = snapshot(rec, d)
    for b in bufs:
        assert np.array_equal(before[b].view(np.uint8), after[b].view(np.uint8)), b
    assert np.array_equal(before["scale"], after["scale"])
    for k, v in before["driver"].items():
        assert np.array_equal(np.asarray(v), np.asarray(after["driver"][k])), k
    rec2.set_option("coeff_table", 0); rec2.set_option("coeff_table", 1)     # (the twin's table goes through the same off / on)
    for dd in (d, d2):
        dd.SuperresolutionGPU(2)
    assert np.array_equal(_bits(rec.syncCPU()), _bits(rec2.syncCPU()))
    for dd in (d, d2):
        dd.SimulateSlicesGPU()
    assert np.array_equal(rec.debug_get(E.BUF_SIMSLICES), rec2.debug_get(E.BUF_SIMSLICES))
    rec.close(); rec2.close()


def test_refusals_are_errors_and_the_context_goes_on(tiny):
    from fetalreconstruction_amd import engine as E
    c = _channel(tiny, 9)
    rec, _ = _engine_at_scale(tiny)
    p = dict(adaptive=False, alpha=1.0, lo=0.0, hi=300.0, delta=20.0, lam=4.0)
    usual = _iterate(rec, c, p, n=1)
    g = np.linspace(0, 500, tiny.nvox).astype(np.float32)
    with pytest.raises(E.SvrError, match="svr_channel_sr_begin first"):      # no call in flight
        rec.channel_sr_guide(g, 10.0)
    rec.channel_sr_begin(c)
    rec.channel_sr_seed()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(E.SvrError, match="delta_g must be finite and positive"):
            rec.channel_sr_guide(g, bad)
    for flags in (2, 4, 3):
        with pytest.raises(E.SvrError, match="unknown flag"):
            rec.channel_sr_guide(g, 10.0, flags=flags)
    for bad in (np.nan, np.inf, -np.inf):
        h = g.copy()
        h[tiny.nvox // 2] = bad
        with pytest.raises(E.SvrError, match="not finite"):
            rec.channel_sr_guide(h, 10.0)
    with pytest.raises(E.SvrError, match="a value per voxel"):
        rec.channel_sr_guide(g[:-1], 10.0)
    rec.set_option("reg_mode", 0)
    with pytest.raises(E.SvrError, match="reg_mode 1"):
        rec.channel_sr_guide(g, 10.0)
    rec.set_option("reg_mode", 1)
    rec.channel_sr_backproject()
    with pytest.raises(E.SvrError, match="between a back-projection and its update"):   # the wrong stage
        rec.channel_sr_guide(g, 10.0)
    rec.channel_sr_update(p["adaptive"], p["alpha"], p["lo"], p["hi"], p["delta"], p["lam"])
    vol = rec.channel_sr_end()
    # none of the refused calls left a guide behind: the call in flight went on unguided, and so does the next one
    assert np.array_equal(_bits(vol), _bits(usual))
    with pytest.raises(E.SvrError, match="svr_channel_sr_begin first"):
        rec.channel_sr_guide(g, 10.0)
    assert np.array_equal(_bits(_iterate(rec, c, p, n=1)), _bits(usual))
    guided = _iterate(rec, c, p, g, 10.0, n=1)                               # ... and a guided one runs
    assert np.isfinite(guided).all() and rel_err(guided, usual) > 1e-4
    rec.close()


def test_recovery_on_the_device(tiny, oracle_mod):
    """tests/test_channel_guide.py's noisy recovery case: the guided ratio within 5 % of the oracle leg's recorded one and below the device's own
    unguided ratios"""
    po = oracle_mod
    prob, rec, orc = _state("tiny", tiny, oracle_mod)
    case = gr.noisy_case(po, orc, prob)
    c, sw = case["c"], case["sw"]

    def run(p, guided):
        rec.channel_sr_begin(c, slice_weights=sw)
        rec.channel_sr_seed()
        if guided:
            rec.channel_sr_guide(case["guide"], gr.DELTA_G)
        for _ in range(sr.RECOVERY_ITERATIONS):
            rec.channel_sr_backproject()
            rec.channel_sr_update(p["adaptive"], p["alpha"], p["lo"], p["hi"], p["delta"], p["lam"])
        return gr.rmse_ratio(prob, case, rec.channel_sr_end())
    d, w, g = run(case["p_default"], False), run(case["p_wide"], False), run(case["p_wide"], True)
    rec.UpdateSliceWeights(orc.slice_weights)
    print("device recovery, RMSE ratios: unguided default %.9g (oracle leg %.9g), unguided delta 120 %.9g (%.9g), guided %.9g (%.9g)"
          % (d, gr.ORACLE_UNGUIDED_DEFAULT, w, gr.ORACLE_UNGUIDED_WIDE, g, gr.ORACLE_GUIDED))
    assert g < d and g < w
    assert abs(g / gr.ORACLE_GUIDED - 1) <= 0.05


def test_the_host_object_s_guided_call_is_the_engine_s_sequence(tiny):
    """svrh_channel_superresolve_guided through its Python binding: the engine's begin, seed, guide, n x (backproject, update), end with the
    object's parameters, bit for bit; without a guide influence (a constant) it is svrh_channel_superresolve; a bad delta_g is refused and the
    object goes on"""
    from fetalreconstruction_amd import engine as E, host
    rec = E.Reconstruction(0)
    E.sync_gpu(rec, tiny)
    d = host.irtkReconstruction(rec, tiny.ns, max_intensity=tiny.max_intensity, min_intensity=tiny.min_intensity)
    d.SetSmoothingParameters(150, 0.02)
    d.reconstruct_iteration(1)
    c = _channel(tiny, 2)
    delta_c, lambda_c, lo, hi, n = 30.0, 0.02, -25.5, 280.5, 2
    recon = rec.syncCPU().copy()
    delta_g = 0.1 * float(recon.max() - recon.min())
    plain = d.ChannelSuperresolve(c, None, n, delta_c, lambda_c, lo, hi, tiny.nvox)
    flat = d.ChannelSuperresolveGuided(c, None, n, delta_c, lambda_c, lo, hi, tiny.nvox, guide=np.full(tiny.nvox, 7.0, np.float32), delta_g=3.0)
    null = d.ChannelSuperresolveGuided(c, None, n, delta_c, lambda_c, lo, hi, tiny.nvox, delta_g=delta_g)
    held = d.ChannelSuperresolveGuided(c, None, n, delta_c, lambda_c, lo, hi, tiny.nvox, guide=recon, delta_g=delta_g)
    only = d.ChannelSuperresolveGuided(c, None, n, delta_c, lambda_c, lo, hi, tiny.nvox, delta_g=delta_g, guide_only=True)
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(E.SvrError, match="delta_g"):
            d.ChannelSuperresolveGuided(c, None, n, delta_c, lambda_c, lo, hi, tiny.nvox, delta_g=bad)
    with pytest.raises(E.SvrError, match="svr_channel_sr_begin first"):       # the refused call left nothing in flight
        rec.channel_sr_end()
    assert np.array_equal(_bits(rec.syncCPU()), _bits(recon))
    p = dict(adaptive=False, alpha=min(1.0, 0.05 / lambda_c), lo=lo, hi=hi, delta=delta_c, lam=lambda_c * delta_c * delta_c)
    seq = _iterate(rec, c, p, None, delta_g, n=n)                              # (the object's calls left its slice weights on the device)
    print("host object: guided differs from the unguided by", rel_err(null, plain), "guide only from joint by", rel_err(only, null))
    assert np.abs(plain).max() > 0 and np.array_equal(_bits(flat), _bits(plain))
    assert rel_err(null, plain) > 1e-4 and rel_err(only, null) > 1e-4
    assert np.array_equal(_bits(null), _bits(held)) and np.array_equal(_bits(null), _bits(seq))
    assert np.array_equal(_bits(d.ChannelSuperresolve(c, None, n, delta_c, lambda_c, lo, hi, tiny.nvox)), _bits(plain))
    rec.close()


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def _cli(args):
    return subprocess.run(["timeout", "-k", "10", "240", build.CLI, *args], capture_output=True, text=True)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """plain | 4 iterations on a ramp | the same guided | guided on two ranks"""
    build.build()
    d = tmp_path_factory.mktemp("channel_guide")
    args, paths, stacks = ref.write_cli_case(d)
    err = {}

    def go(name, extra):
        r = _cli(["-o", str(d / f"{name}.nii.gz"), *args, *extra])
        assert r.returncode == 0, r.stderr[-3000:]
        err[name] = r.stderr
    ramp = ref.write_like(d, "ramp", stacks, lambda k, st: 50.0 + 2.0 * ref.pixel_world(st.attr)[..., 0] - 1.0 * ref.pixel_world(st.attr)[..., 2])
    ch = lambda out: ["--channelStacks", *ramp, "--channelOutput", str(d / out), "--channelIterations", "4"]
    go("plain", [])
    go("four", ch("c_four.nii.gz"))
    go("guided", [*ch("c_guided.nii.gz"), "--channelGuide"])
    go("two", [*ch("c_two.nii.gz"), "--channelGuide", "-d", "0", "0"])
    return d, err


def _vol(d, name):
    from fetalreconstruction_amd import nifti
    return nifti.read(d / name)[0]


def test_cli_primary_volume_is_unchanged(runs):
    """the -o bytes with and without --channelGuide; without it the channel's path is the parent commit's (no guide: the unguided kernels, whose
    code is unchanged) and says nothing about a guide"""
    d, err = runs
    plain = (d / "plain.nii.gz").read_bytes()
    assert (d / "four.nii.gz").read_bytes() == plain and (d / "guided.nii.gz").read_bytes() == plain
    assert "--channelGuide" not in err["four"]
    line = [l for l in err["guided"].splitlines() if l.startswith("--channelGuide: delta_g")]
    assert line and "guide range" in line[0] and "joint" in line[0], err["guided"][-2000:]
    print(line[0])


def test_cli_the_guide_changes_the_channel_and_keeps_its_cover(runs):
    d, err = runs
    f, g = _vol(d, "c_four.nii.gz"), _vol(d, "c_guided.nii.gz")
    print("--channelGuide moves the channel by", rel_err(g, f))
    assert np.array_equal(f != 0, g != 0) and rel_err(g, f) > 1e-4
    assert np.isfinite(g).all()


def test_cli_two_ranks_on_one_device(runs):
    d, err = runs
    assert "2 ranks" in err["two"]
    c1, c2 = _vol(d, "c_guided.nii.gz"), _vol(d, "c_two.nii.gz")
    assert np.array_equal(c1 != 0, c2 != 0)
    print("two ranks against one: guided channel after 4 iterations", rel_err(c2, c1))
    assert rel_err(c2, c1) < 2e-5
