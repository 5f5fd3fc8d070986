"""A second image through a run's motion and weights on the device (csrc/svr_channel.inc: svr_channel_scatter / _finish / _vote /
_vote_fetch, factor mode 3 of k_cell_factors) and from the command line (--channelStacks / --labelStacks / --manualMask).

Tolerances, stated once:
  * num | den against the oracle's SR scatter: the project's TOL_SUM (2e-5 of the buffer's maximum, tests/test_parity_gpu.py) -- it is the
    very scatter that bound was set for; the covered set (den > 0) exactly.
  * everything else is exact.  The library is built with -fno-fast-math and HIP's default correctly rounded float division, so
    svr_channel_finish is the float32 quotient numpy forms (no 1-ulp allowance is needed or made), and a channel that is 8 everywhere
    gives num = 8 den bit for bit (a power of two scales every product and every sum exactly) and a quotient of exactly 8.
  * two ranks against one: the ranks' sums meet in another order: 2e-5 of the maximum."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from fetalreconstruction_amd import build
from tests import channel_ref as ref
from tests.twins.reconstruction import irtkReconstruction
from tests.util import rel_err, run_to_state

pytestmark = pytest.mark.gpu

TOL_SUM = 2e-5          # tests/test_parity_gpu.py


def _driver(eng, prob):
    d = irtkReconstruction(eng, prob.ns, max_intensity=prob.max_intensity, min_intensity=prob.min_intensity)
    d.SetSmoothingParameters(150, 0.02)
    return d


def _engine_at_scale(prob):
    from fetalreconstruction_amd import engine as E
    rec = E.Reconstruction(0)
    E.sync_gpu(rec, prob)
    d = _driver(rec, prob)
    run_to_state(d, "scale")
    return rec, d


_PROBLEMS = {}


def _problem(name, tiny):
    if name not in _PROBLEMS:
        _PROBLEMS[name] = tiny if name == "tiny" else ref.awkward_problem()
    return _PROBLEMS[name]


_STATES = {}


def _state(name, tiny, oracle_mod):
    """engine and oracle at state "scale", the oracle's per-pixel state copied onto the device (as test_backprojection_parity): shared by
    the tests of a problem, which leave the engine's options and inputs as they found them"""
    if name not in _STATES:
        from fetalreconstruction_amd import engine as E
        prob = _problem(name, tiny)
        rec, _ = _engine_at_scale(prob)
        orc = oracle_mod.OracleReconstruction(prob, oracle_mod.CANON)
        run_to_state(_driver(orc, prob), "scale")
        rec.debug_set(E.BUF_WEIGHTS, orc.weights)
        rec.debug_set(E.BUF_PSF_SUMS, orc.psf_sums)
        rec.UpdateScaleVector(orc.d_scales, orc.slice_weights)
        _STATES[name] = (prob, rec, orc)
    return _STATES[name]


def _num_den(rec):
    from fetalreconstruction_amd import engine as E
    return rec.debug_get(E.BUF_ADDON), rec.debug_get(E.BUF_CONFIDENCE_MAP)


def _channel(prob, seed=0):
    """integer values in [0, 255] on the slice grid"""
    return np.random.default_rng(seed).integers(0, 256, prob.slices.shape).astype(np.float32)


def _oracle_num_den(po, orc, prob, c, slice_weights, off_slices=()):
    """The oracle's SR scatter, unchanged, on slices' = c + 256 (-1 where the slice is), scales 1, simulated slices 256: its residual
    e = slices' * 1 - 256 is exactly c, its weight the SR scatter's -- addon | cmap are num | den."""
    s2 = np.where(prob.slices == -1, np.float32(-1), c + np.float32(256)).astype(np.float32)
    for u in off_slices:
        s2[u] = -1
    sim = np.full(prob.slices.shape, 256, np.float32)
    one = np.ones(prob.ns, np.float32)
    sw = po._f32(slice_weights)
    nv = prob.nvox
    pair = np.zeros(2 * nv, np.float32)
    addon, cmap = pair[:nv], pair[nv:]
    po.lib().orc_superresolution_backproject(C.byref(orc.g), po._p(s2), po._p(orc.weights), po._p(sim), po._p(sw), po._p(one), po._p(orc.mask),
                                             po._p(orc.psf_sums), po._p(addon), po._p(cmap))
    return addon, cmap


@pytest.mark.parametrize("name,switch", [("tiny", False), ("awkward", False), ("awkward", True)])
def test_num_and_den_against_the_oracle_s_sr_scatter(tiny, oracle_mod, name, switch):
    """switch: unit_on switches one whole slice off and another slice's weight is 0; the oracle gets the first as a slice of -1 and the
    second as the same weight."""
    prob, rec, orc = _state(name, tiny, oracle_mod)
    c = _channel(prob, 1)
    sw = orc.slice_weights.copy()
    unit_on, off = None, ()
    if switch:
        live = [s for s in range(prob.ns) if (orc.psf_sums[s] != 0).any() and sw[s] > 0]
        off = (live[len(live) // 2],)
        sw[live[len(live) // 3]] = 0
        unit_on = np.ones(prob.ns, np.uint8)
        unit_on[off[0]] = 0
    rec.channel_scatter(c, unit_on=unit_on, slice_weights=sw)
    num, den = _num_den(rec)
    onum, oden = _oracle_num_den(oracle_mod, orc, prob, c, sw, off)
    rec.UpdateSliceWeights(orc.slice_weights)
    print(name, switch, "covered", int((den > 0).sum()), "rel_err num", rel_err(num, onum), "den", rel_err(den, oden))
    assert (oden > 0).sum() > 1000
    assert np.array_equal(den > 0, oden > 0)
    assert rel_err(num, onum) < TOL_SUM and rel_err(den, oden) < TOL_SUM
    if switch:                                              # the switches did something
        full_num, full_den = _oracle_num_den(oracle_mod, orc, prob, c, orc.slice_weights)
        assert not np.array_equal(full_den, oden)


@pytest.mark.parametrize("name", ["tiny", "awkward"])
def test_exact_invariants(tiny, oracle_mod, name):
    prob, rec, orc = _state(name, tiny, oracle_mod)
    nv = prob.nvox
    assert name == "tiny" or (nv % 4 and prob.slices.size % 4)
    # a constant channel of 8
    rec.channel_scatter(np.full(prob.slices.shape, 8, np.float32))
    num, den = _num_den(rec)
    assert (den > 0).sum() > 1000 and (den <= 0).any()
    assert np.array_equal(num.view(np.uint32), (np.float32(8) * den).view(np.uint32))
    out = rec.channel_finish(background=-3.0)
    assert np.array_equal(out, np.where(den > 0, np.float32(8), np.float32(-3)))
    # indicator mode with every pixel matching: num is den
    rec.channel_scatter(np.full(prob.slices.shape, 5, np.float32), indicator=True, match=5.0)
    num1, den1 = _num_den(rec)
    assert np.array_equal(num1.view(np.uint32), den1.view(np.uint32)) and np.array_equal(den1.view(np.uint32), den.view(np.uint32))
    # ... and with none matching it is 0
    rec.channel_scatter(np.full(prob.slices.shape, 5, np.float32), indicator=True, match=6.0)
    assert not _num_den(rec)[0].any()
    # the finish is the float32 quotient of the downloaded buffers (correctly rounded division: exact, no allowance)
    c = _channel(prob, 2) - np.float32(100)                 # zero and negative values count
    rec.channel_scatter(c)
    num, den = _num_den(rec)
    out = rec.channel_finish(background=0.5)
    with np.errstate(divide="ignore", invalid="ignore"):
        want = np.where(den > 0, num / den, np.float32(0.5)).astype(np.float32)
    assert want.dtype == np.float32 and np.array_equal(out.view(np.uint32), want.view(np.uint32))
    assert out[den > 0].min() < 0                           # a negative channel value never excluded its pixel
    from fetalreconstruction_amd import engine as E
    assert np.array_equal(rec.debug_get(E.BUF_ADDON), out)  # in place


@pytest.mark.parametrize("name", ["tiny", "awkward"])
def test_vote_is_the_first_maximum(tiny, oracle_mod, name):
    prob, rec, orc = _state(name, tiny, oracle_mod)
    labels = np.array([1, 2, 5], np.float32)
    lab = labels[np.random.default_rng(3).integers(0, 3, prob.slices.shape)]
    P = []
    for k, l in enumerate(labels):
        rec.channel_scatter(lab, indicator=True, match=float(l))
        den = _num_den(rec)[1]
        rec.channel_vote(float(l), k == 0)
        P.append(rec.channel_finish(background=-1.0))       # (after the vote: the finish divides in place)
    P = np.stack(P)
    got_l, got_c = rec.channel_vote_fetch(background_label=-7.0)
    cov = den > 0
    assert cov.sum() > 1000 and (~cov).any()
    assert np.array_equal(got_l[cov], labels[np.argmax(P[:, cov], 0)])       # numpy's argmax: the first maximum
    assert np.array_equal(got_c[cov], P[:, cov].max(0))
    assert (got_l[~cov] == -7.0).all() and (got_c[~cov] == 0).all()
    assert len(np.unique(got_l[cov])) == 3
    # a constructed tie: two labels with identical indicator images, through two calls
    a = np.where(lab == 1, np.float32(3), np.float32(0))
    b = np.where(lab == 1, np.float32(7), np.float32(0))
    rec.channel_scatter(a, indicator=True, match=3.0)
    rec.channel_vote(3.0, True)
    rec.channel_scatter(b, indicator=True, match=7.0)
    rec.channel_vote(7.0, False)
    tl, tc = rec.channel_vote_fetch(background_label=0.0)
    assert (tl[cov] == 3.0).all() and np.array_equal(tc[cov], P[0][cov])


def test_repeats_bit_for_bit_and_leaves_the_sr_iteration_alone():
    """Two calls, and the coefficient table on and off (what test_normalise_bias_scatter_on_the_cell_kernels_repeats_bit_for_bit asserts
    of factor mode 2): the same bits.  An SR iteration after a channel scatter gives the volume of one without it: addon | cmap are marked
    as clobbered and nothing the iteration caches is touched."""
    from fetalreconstruction_amd import engine as E
    prob = ref.awkward_problem()
    c = _channel(prob, 4)
    rec, d = _engine_at_scale(prob)
    rec.channel_scatter(c)                                   # before any SR iteration: no table yet, every tap evaluated
    early = _num_den(rec)
    d.SuperresolutionGPU(1)
    after_channel = rec.syncCPU()
    assert rec.get_option("coeff_table") == 1 and rec.get_option("coeff_valid") == 1
    rec.channel_scatter(c)
    t1 = _num_den(rec)
    rec.channel_scatter(c)
    t2 = _num_den(rec)
    rec.set_option("coeff_table", 0)
    rec.channel_scatter(c)
    fly = _num_den(rec)
    assert np.abs(t1[0]).max() > 0 and t1[1].max() > 0
    for k in (0, 1):
        assert np.array_equal(t1[k], t2[k]) and np.array_equal(t1[k], fly[k]) and np.array_equal(t1[k], early[k])
    assert rec.fallbacks()["scatter_to_atomics"] == 0
    rec2, d2 = _engine_at_scale(prob)
    d2.SuperresolutionGPU(1)
    assert np.array_equal(after_channel, rec2.syncCPU())
    # ... and a second iteration after scatters with the table and without it
    rec.set_option("coeff_table", 1)
    for r, dd in ((rec, d), (rec2, d2)):
        dd.SimulateSlicesGPU(); dd.MStepGPU(1); dd.EStepGPU(); dd.ScaleGPU(); dd.SuperresolutionGPU(2)
    assert np.array_equal(rec.syncCPU(), rec2.syncCPU())


def test_refusals_are_errors_not_faults(tiny):
    from fetalreconstruction_amd import engine as E
    c = np.zeros(tiny.slices.shape, np.float32)
    rec = E.Reconstruction(0)
    E.sync_gpu(rec, tiny)
    with pytest.raises(E.SvrError, match="EM weights"):      # no EM state
        rec.channel_scatter(c)
    with pytest.raises(E.SvrError, match="no vote in flight"):
        rec.channel_vote_fetch()
    with pytest.raises(E.SvrError, match="no vote in flight"):
        rec.channel_vote(1.0, False)
    rec2, _ = _engine_at_scale(tiny)
    with pytest.raises(E.SvrError, match="no channel"):      # NULL channel
        rec2.channel_scatter(None)
    assert rec2._lib.svr_channel_scatter(rec2._h, c.ctypes.data_as(C.c_void_p), None, None, 2, C.c_float(0)) != 0
    assert b"unknown flag" in rec2._lib.svr_last_error(rec2._h)
    rec2.set_option("back_mode", 4)                          # the atomic scatters: no channel path
    with pytest.raises(E.SvrError, match="no fallback"):
        rec2.channel_scatter(c)
    rec2.set_option("back_mode", 5)
    rec2.channel_scatter(c)                                  # ... and the context still works
    pv = E.Reconstruction(0)
    pv.set_option("pvr", 1)
    pv.sgrid = tiny.slices.shape
    with pytest.raises(E.SvrError, match="pvr"):
        pv.channel_scatter(c)


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def _cli(args):
    return subprocess.run(["timeout", "-k", "10", "240", build.CLI, *args], capture_output=True, text=True)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """plain | channel of 8 + labels split by a plane + confidence | --manualMask next to --channelStacks f none none | the second on two ranks"""
    from fetalreconstruction_amd import geometry as geo, nifti
    build.build()
    d = tmp_path_factory.mktemp("channels")
    args, paths, stacks = ref.write_cli_case(d)
    err = {}

    def go(name, extra):
        r = _cli(["-o", str(d / f"{name}.nii.gz"), *args, *extra])
        assert r.returncode == 0, r.stderr[-3000:]
        err[name] = r.stderr
    go("plain", [])
    vol, vattr = nifti.read(d / "plain.nii.gz")
    centre = geo.image_to_world(vattr) @ np.array([(vattr.nx - 1) / 2.0, (vattr.ny - 1) / 2.0, (vattr.nz - 1) / 2.0, 1.0])
    eight = ref.write_like(d, "eight", stacks, lambda k, st: np.full(st.data.shape, 8.0))
    split = ref.write_like(d, "split", stacks, lambda k, st: np.where(ref.pixel_world(st.attr)[..., 0] < centre[0], 1.0, 2.0))
    both = ["--channelStacks", *eight, "--channelOutput", str(d / "c8.nii.gz"), "--labelStacks", *split, "--labelOutput", str(d / "lab.nii.gz"),
            "--labelConfidence", str(d / "conf.nii.gz")]
    go("both", both)
    (d / "mm").mkdir()
    manual = ref.write_like(d / "mm", "manual", stacks, lambda k, st: (st.data > np.median(st.data)).astype(np.float32) if k == 0 else None)
    go("manual", ["--manualMask", manual[0], "--channelStacks", *manual, "--channelOutput", str(d / "manual_as_channel.nii.gz")])
    two = [a.replace(str(d / "c8"), str(d / "c8_2")).replace(str(d / "lab"), str(d / "lab_2")).replace(str(d / "conf"), str(d / "conf_2")) for a in both]
    go("two", [*two, "-d", "0", "0"])
    return d, err, centre, vattr


def _vol(d, name):
    from fetalreconstruction_amd import nifti
    return nifti.read(d / name)[0]


def _mask_on(vattr):
    """the case's mask on the reconstruction grid as SetMask puts it there (nearest neighbour, no smoothing), and every voxel's world x"""
    from fetalreconstruction_amd import geometry as geo
    _, rattr, rmask = ref.case_stacks()
    w = ref.pixel_world(vattr)
    q = np.concatenate([w, np.ones(w.shape[:-1] + (1,))], -1) @ geo.world_to_image(rattr).T
    i = np.floor(q[..., :3] + 0.5).astype(int)
    ok = ((i >= 0) & (i < [rattr.nx, rattr.ny, rattr.nz])).all(-1)
    i = np.clip(i, 0, [rattr.nx - 1, rattr.ny - 1, rattr.nz - 1])
    return ok & (rmask[i[..., 2], i[..., 1], i[..., 0]] > 0), w[..., 0]


def test_cli_volume_is_unchanged(runs):
    d, err, centre, vattr = runs
    assert (d / "plain.nii.gz").read_bytes() == (d / "both.nii.gz").read_bytes()
    assert (d / "plain.nii.gz").read_bytes() == (d / "manual.nii.gz").read_bytes()
    assert "--channelStacks" in err["both"] and "covered voxels" in err["both"] and "--labelConfidence" in err["both"]


def test_cli_constant_channel(runs):
    d, err, centre, vattr = runs
    c8, conf = _vol(d, "c8.nii.gz"), _vol(d, "conf.nii.gz")
    cov = c8 != 0
    inside, _ = _mask_on(vattr)
    print("covered", int(cov.sum()), "mask", int(inside.sum()))
    assert cov.sum() > 1000 and (c8[cov] == 8.0).all() and not (cov & ~inside).any()
    assert np.array_equal(cov, conf > 0)                    # the label run's covered set: the same slices, the same weights


def _far(vattr, centre, cov):
    inside, x = _mask_on(vattr)
    left = cov & (x < centre[0] - 9.0 * vattr.dx)
    right = cov & (x > centre[0] + 9.0 * vattr.dx)
    return left, right


def test_cli_labels_on_a_plane_split(runs):
    """A covered voxel more than 9 voxel widths from the plane (the scatter's 16-tap box reaches 8, plus one for the rounding of the
    centre) sees pixels of its own side only: its label is its side's and its confidence exactly 1."""
    d, err, centre, vattr = runs
    lab, conf = _vol(d, "lab.nii.gz"), _vol(d, "conf.nii.gz")
    cov = conf > 0
    left, right = _far(vattr, centre, cov)
    print("far voxels", int(left.sum()), int(right.sum()))
    assert left.sum() >= 500 and right.sum() >= 500
    assert (lab[left] == 1.0).all() and (lab[right] == 2.0).all()
    assert (conf[left] == 1.0).all() and (conf[right] == 1.0).all()
    near = cov & ~left & ~right
    assert np.isin(lab[near], (1.0, 2.0)).all() and (lab[~cov] == 0).all()
    _, x = _mask_on(vattr)
    side = np.where(x < centre[0], 1.0, 2.0)
    print("near the plane: %d voxels, %.4f disagree with their own side" % (int(near.sum()), float((lab[near] != side[near]).mean())))


def test_cli_manual_mask_is_the_channel_on_the_first_stack(runs):
    d, err, centre, vattr = runs
    out = d / "mm" / "PSFTransformed_manual0.nii.gz"
    assert out.exists()
    assert out.read_bytes() == (d / "manual_as_channel.nii.gz").read_bytes()
    v = _vol(d / "mm", "PSFTransformed_manual0.nii.gz")
    assert v.max() <= 1.0 and v.min() >= 0.0 and 0 < (v > 0.5).sum() < (v > 0).sum()


def test_cli_two_ranks_on_one_device(runs):
    d, err, centre, vattr = runs
    assert "2 ranks" in err["two"]
    c1, c2 = _vol(d, "c8.nii.gz"), _vol(d, "c8_2.nii.gz")
    l1, l2 = _vol(d, "lab.nii.gz"), _vol(d, "lab_2.nii.gz")
    f1, f2 = _vol(d, "conf.nii.gz"), _vol(d, "conf_2.nii.gz")
    assert np.array_equal(c1 != 0, c2 != 0) and np.array_equal(f1 > 0, f2 > 0)
    print("two ranks against one: channel", rel_err(c2, c1), "confidence", rel_err(f2, f1))
    assert rel_err(c2, c1) < 2e-5 and rel_err(f2, f1) < 2e-5
    left, right = _far(vattr, centre, f1 > 0)
    assert np.array_equal(l1[left | right], l2[left | right]) and np.array_equal(f1[left | right], f2[left | right])
