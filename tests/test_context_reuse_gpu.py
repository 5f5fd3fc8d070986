"""A live context handed a second problem gives the bits of a fresh context handed that problem (tests/reuse_cases.py: the problems
and the call sequence).  The kernels' arithmetic is pinned elsewhere, against the oracle and float64 restatements; this pins the
state around them -- which upload drops which buffer, what a kept grow-only block (csrc/svr_devbuf.h) still holds, and what the
per-call arenas of the registration entry points carry from one call to the next.  No comparison here has a tolerance: everything
runs on the default paths, whose sums have a fixed order, and the control shows that two fresh contexts agree on every array."""
import numpy as np
import pytest

from fetalreconstruction_amd import geometry as geo
from tests import reuse_cases as cases
from tests.test_nmi_gpu import _plane_matrices
from tests.test_nmi_registration import entropy_sums, joint_histogram, number_of_bins

pytestmark = pytest.mark.gpu

KEEP = object()               # _upload: leave the superpixel masks to whatever the upload does with them
_FRESH = {}


def _new(pvr=False, bias=False):
    from fetalreconstruction_amd import engine as E
    rec = E.Reconstruction(0)
    if pvr:
        rec.set_option("pvr", 1)
    if bias:
        rec.set_flags(disable_bias_correction=False)
    return rec


def _upload(rec, prob, masks=KEEP, bias=False):
    """the usual order, then every stage -> the fingerprint"""
    from fetalreconstruction_amd import engine as E
    E.sync_gpu(rec, prob)
    if masks is not KEEP:
        rec.set_spx_masks(masks)
    return cases.fingerprint(rec, prob, cases.inputs(prob), bias)


def _fresh(label, prob, pvr=False, masks=KEEP, bias=False):
    """the fingerprint of a fresh context on the problem, computed once per session and shared read-only"""
    key = (label, pvr, masks is not KEEP and masks is not None, bias)
    if key not in _FRESH:
        rec = _new(pvr, bias)
        fp = _upload(rec, prob, masks, bias)
        rec.close()
        for a in fp.values():
            a.setflags(write=False)
        _FRESH[key] = fp
    return _FRESH[key]


def _same(got, ref, what):
    bad = cases.differing(got, ref)
    assert not bad, (what, bad)


def _something_happened(fp, pvr=False):
    """the fingerprint is of a run that did its work on the default paths"""
    opts = dict(zip(cases.STATE_OPTIONS, fp["table.options"]))
    assert fp["gauss.voxel_num"][0] > 0 and (fp["gauss.psf_sums"] != 0).any() and (fp["sr.addon"] != 0).any() and fp["fwd.inside"].any()
    assert opts["psf_list_valid"] == 1 and opts["cells_valid"] == 1 and opts["coeff_state"] == (0 if pvr else 1), opts
    assert not fp["table.fallbacks"].any()


# ---- control ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pvr,bias", [("A", False, False), ("L16", True, False), ("A", False, True)], ids=["A", "L16 patch-based", "A with bias"])
def test_two_fresh_contexts_agree_on_every_array(name, pvr, bias):
    prob = cases.get(name)
    first = _fresh(name, prob, pvr, bias=bias)
    _something_happened(first, pvr)
    if bias:
        assert (first["bias.bias"] != 0).any()
    rec = _new(pvr, bias)
    _same(_upload(rec, prob, bias=bias), first, (name, "a second fresh context"))
    rec.close()


def test_the_fingerprint_tells_the_problems_apart():
    """(a comparison that passes must be able to fail: other pixels of the same shapes change every recorded stage)"""
    a, a2 = _fresh("A", cases.get("A")), _fresh("A2", cases.get("A2"))
    bad = {b[0] for b in cases.differing(a2, a)}
    same_by_design = {"gauss.voxel_num", "fwd.inside", "sr.confidence_map"}          # (the non-adaptive update sets the confidence map to one value)
    assert {k for k in a if k.split(".")[0] in ("gauss", "fwd", "em", "sr")} - same_by_design <= bad, bad
    assert {"table.simslices", "table.addon", "table.confidence_map"} <= bad, bad


# ---- whole re-uploads -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain,bias", [(("A", "B", "A"), False), (("B", "C", "B"), False), (("A", "A2", "A"), False), (("A", "B", "A"), True)],
                         ids=["A-B-A", "B-C-B", "A-A2-A", "A-B-A with bias"])
def test_whole_reuploads_on_one_context(chain, bias):
    """grow and back into the kept blocks; shrink first; the same sizes with other content (a cache keyed on shape)"""
    rec = _new(bias=bias)
    for step, name in enumerate(chain):
        prob = cases.get(name)
        _same(_upload(rec, prob, bias=bias), _fresh(name, prob, bias=bias), (chain, "step", step, name))
    rec.close()


# ---- partial re-uploads ---------------------------------------------------------------------------------------------------------------
def _set_matrices(rec, P):
    rec.SetSliceMatrices(P.slice_t, P.slice_tinv, P.slice_i2w, P.slice_w2i, P.slice_i2w, P.slice_w2i, P.recon_i2w, P.recon_w2i)


BIAS = pytest.mark.parametrize("bias", [False, True], ids=["no bias", "with bias"])


@BIAS
@pytest.mark.parametrize("radius", [12.0, 17.0])
def test_a_new_volume_grid_under_kept_slices(radius, bias):
    """(smaller and larger than the grid before; the slices stick out of the smaller one)"""
    a = cases.get("A")
    final = cases.with_volume_of(a, cases.volume_grid(radius))
    rec = _new(bias=bias)
    _upload(rec, a, bias=bias)
    rec.InitReconstructionVolume(final.vsize, final.vdim, None, 12.0)
    rec.setMask(final.vsize, final.vdim, final.mask, 12.0)
    _set_matrices(rec, final)
    got = cases.fingerprint(rec, final, cases.inputs(final), bias)
    _something_happened(got)
    _same(got, _fresh(f"A under {radius}", final, bias=bias), ("volume grid", radius, bias))
    rec.close()


@BIAS
@pytest.mark.parametrize("other", ["B", "C"])
def test_a_new_slice_grid_under_a_kept_volume(other, bias):
    a = cases.get("A")
    final = cases.with_slices_of(a, cases.get(other))
    rec = _new(bias=bias)
    _upload(rec, a, bias=bias)
    ns, sy, sx = final.slices.shape
    rec.initStorageVolumes((sx, sy, ns), tuple(final.slice_dim[0]))
    rec.FillSlices(final.slices, final.sizes_x, final.sizes_y)
    rec.setSliceDims(final.slice_dim, 2.0)
    _set_matrices(rec, final)
    got = cases.fingerprint(rec, final, cases.inputs(final), bias)
    _something_happened(got)
    _same(got, _fresh(f"{other} in A", final, bias=bias), ("slice grid", other, bias))
    rec.close()


@BIAS
def test_a_new_mask_only(bias):
    """(with bias: the blurred mask of the bias path is built again)"""
    a = cases.get("A")
    final = cases.with_mask(a, 10.0)
    rec = _new(bias=bias)
    _upload(rec, a, bias=bias)
    rec.setMask(final.vsize, final.vdim, final.mask, 12.0)
    got = cases.fingerprint(rec, final, cases.inputs(final), bias)
    _same(got, _fresh("A, mask 10", final, bias=bias), ("mask", bias))
    assert cases.differing(got, _fresh("A", a, bias=bias))                         # (the new mask was taken)
    rec.close()


# ---- patch-based ------------------------------------------------------------------------------------------------------------------------
LEVELS = ("L16", "L8", "L12x8", "L16")


@pytest.mark.parametrize("with_masks", [False, True], ids=["no masks", "superpixel masks"])
def test_the_hierarchical_levels_on_one_context(with_masks):
    """fewer large patches, many small ones, a non-square one and back, as setup_engines of the patch-based command line uploads them"""
    rec = _new(pvr=True)
    for step, name in enumerate(LEVELS):
        prob = cases.get(name)
        masks = cases.spx(prob) if with_masks else KEEP
        ref = _fresh(name, prob, True, masks)
        _something_happened(ref, pvr=True)
        _same(_upload(rec, prob, masks), ref, ("levels", "step", step, name, with_masks))
    if with_masks:                                                                 # (the masks do something)
        assert cases.differing(_fresh("L16", cases.get("L16"), True, cases.spx(cases.get("L16"))), _fresh("L16", cases.get("L16"), True))
    rec.close()


@pytest.mark.parametrize("explicitly", [False, True], ids=["no call", "set_spx_masks(None)"])
def test_masks_then_none(explicitly):
    """a new slice grid comes without the old grid's superpixel masks, with or without svr_set_spx_masks(NULL)"""
    first, second = cases.get("L8"), cases.get("L16")
    rec = _new(pvr=True)
    _upload(rec, first, cases.spx(first))
    got = _upload(rec, second, None if explicitly else KEEP)
    bad = cases.differing(got, _fresh("L16", second, True))
    stale = cases.spx(first).reshape(-1, 64, 64)[:second.ns, :second.slices.shape[1], :second.slices.shape[2]] == ord("0")
    zeroed = int(((got["gauss.psf_sums"] == 0) & (_fresh("L16", second, True)["gauss.psf_sums"] != 0) & stale).sum())
    assert not bad, ("masks, then none", explicitly, bad, "v_PSF_sums zero where the old masks say '0':", zeroed)
    rec.close()


def test_pvr_toggled_on_a_live_context():
    rec = _new()
    for step, (name, pvr) in enumerate((("A", 0), ("L16", 1), ("A", 0))):
        rec.set_option("pvr", pvr)
        prob = cases.get(name)
        _same(_upload(rec, prob), _fresh(name, prob, bool(pvr)), ("pvr toggled", "step", step, name))
    rec.close()


# ---- the grow-only arenas of the per-call entry points ----------------------------------------------------------------------------------
def test_nmi_merge_slots_grow_and_are_left_zero():
    """targets of 100 x 93: one plane per workgroup, so every evaluation of two planes or more is split and merged in a slot.  3 slots,
    then 71 (the slots and the term table grow; the counters move behind the new slots), then the 3 again"""
    from fetalreconstruction_amd import engine as E
    rec = E.Reconstruction(0)
    rng = np.random.default_rng(7)
    tx, ty, ssize = 100, 93, (60, 64, 58)
    src = rng.integers(-1, 3000, ssize[::-1]).astype(np.int16)
    src[:, :, :2] = -1
    nbs, ws = number_of_bins(0, 2999)
    nbt, wt = number_of_bins(0, 199)
    ppe_all = [2] * 70 + [5]
    starts = np.concatenate([[0], np.cumsum(ppe_all)])
    tg = rng.integers(-1, 200, (int(starts[-1]), ty, tx)).astype(np.int16)
    tg[:, :3] = -1
    mats = np.concatenate([_plane_matrices(rng, (tx, ty, k), ssize, k) for k in ppe_all])
    rec.ncc_set_targets(tg)
    rec.ncc_set_source(src)
    rec.nmi_bin_source(ws)
    src_b = np.where(src > 0, src // ws, src).astype(np.int16)
    want = {}

    def call(n_eval):
        ppe, n_planes = ppe_all[:n_eval], int(starts[n_eval])
        out, hist = rec.nmi_evaluate(ppe, np.arange(n_planes), mats[:n_planes], np.full(n_eval, wt), np.full(n_eval, nbt), nbs, histograms=True)
        for e in range(n_eval):
            if e not in want:
                h = joint_histogram(tg[starts[e]:starts[e + 1]], mats[starts[e]:starts[e + 1]], src_b, wt, nbt, nbs)
                want[e] = (h, entropy_sums(h, nbt, nbs)[0])
            assert np.array_equal(hist[e], want[e][0]), (n_eval, e, "histogram")
            assert tuple(out[e]) == want[e][1], (n_eval, e, out[e], want[e][1])
        assert out[:, 0].min() > 1000
        return out, hist

    first = call(3)
    call(len(ppe_all))
    third = call(3)
    assert np.array_equal(third[0], first[0]) and np.array_equal(third[1], first[1])
    plain, none = rec.nmi_evaluate(ppe_all[:3], np.arange(6), mats[:6], np.full(3, wt), np.full(3, nbt), nbs)      # without the histograms
    assert none is None and np.array_equal(plain, first[0])
    rec.close()


def _pyr_level(rec, c, n):
    """level 0 of the first n images of a case of tests/pyramid_cases.py, from element 0 of slot 1 -> (min, max, the target planes)"""
    import pyramid_ref as ref
    s = c.steps[0]
    rs = c.resamples(s)
    a0 = c.attrs[0]
    outs = [ref.resampled_attr(a, s.res) if rs else a for a in c.attrs[:n]]
    o = outs[0]
    rec.ncc_alloc_targets(n * o.nz, o.nx, o.ny)
    mn, mx = rec.pyr_level(1, 0, (a0.nx, a0.ny, a0.nz), c.kernels(s), rs, (o.nx, o.ny, o.nz), [geo.image_to_world(a) for a in outs],
                           [geo.world_to_image(a) for a in c.attrs[:n]], c.pads[:n], 0)
    return mn.copy(), mx.copy(), rec.ncc_get_targets()


def test_a_pyramid_level_ends_inside_the_last_upload():
    """a large image set, then a smaller one into the kept block: a level over the stale tail is refused, a level inside is a fresh context's"""
    from fetalreconstruction_amd import engine as E
    import pyramid_cases
    c = pyramid_cases.get("batch_mixed_padding")                                   # five images of 37 x 29, one grid
    n_all, small = len(c.pads), 2
    rec = E.Reconstruction(0)
    with pytest.raises(E.SvrError, match="svr_pyr_upload first"):
        _pyr_level(rec, c, 1)
    rec.pyr_upload(1, c.images)
    whole = _pyr_level(rec, c, n_all)
    rec.pyr_upload(1, c.images[:small])
    for n in (n_all, small + 1):
        with pytest.raises(E.SvrError, match="svr_pyr_upload first"):
            _pyr_level(rec, c, n)
    got = _pyr_level(rec, c, small)
    fresh = E.Reconstruction(0)
    fresh.pyr_upload(1, c.images[:small])
    want = _pyr_level(fresh, c, small)
    for g, w, h in zip(got, want, whole):
        assert np.array_equal(g, w) and np.array_equal(g, h[:len(g)])
    # the source slot: a volume, then its first planes
    v = pyramid_cases.get("source_slot").images[0]
    nz, ny, nx = v.shape
    eye = [np.eye(4)]
    level = lambda r, planes: r.pyr_level(0, 0, (nx, ny, planes), [None] * 3, False, (nx, ny, planes), eye, eye, [-32768])   # noqa: E731
    rec.pyr_upload(0, v)
    level(rec, nz)
    rec.pyr_upload(0, v[:5])
    with pytest.raises(E.SvrError, match="svr_pyr_upload first"):
        level(rec, nz)
    mn, mx = level(rec, 5)
    fresh.pyr_upload(0, v[:5])
    mn_f, mx_f = level(fresh, 5)
    assert np.array_equal(mn, mn_f) and np.array_equal(mx, mx_f)
    assert np.array_equal(rec.ncc_get_source(), fresh.ncc_get_source()) and rec.ncc_get_source().shape == (5, ny, nx)
    fresh.close()
    rec.close()


def _metric_case(seed, n, tx, ty, ssize):
    rng = np.random.default_rng(seed)
    src = (rng.integers(0, 400, ssize[::-1]) + np.indices(ssize[::-1]).sum(0) * 25).astype(np.int16)
    src[:, :, :2] = -1
    tg = rng.integers(-1, 200, (n, ty, tx)).astype(np.int16)
    tg[:, :2] = -1
    mats = np.concatenate([_plane_matrices(rng, (tx, ty, 1), ssize, 1) for _ in range(n)])
    return dict(src=src, tg=tg, mats=mats, n=n, bins=(number_of_bins(0, int(src.max())), number_of_bins(0, 199)))


def _metrics(rec, q):
    """targets and source up, one call of each metric -> what they returned"""
    rec.ncc_set_targets(q["tg"])
    rec.ncc_set_source(q["src"])
    idx = np.arange(q["n"])
    ncc, sums = rec.ncc_evaluate(idx, q["mats"])
    lncc, kmap = rec.lncc_evaluate(idx, q["mats"], 3, maps=True)
    (nbs, ws), (nbt, wt) = q["bins"]
    rec.nmi_bin_source(ws)
    ppe = [1] * (q["n"] - 2) + [2]                                                 # single planes and one split evaluation
    nmi, hist = rec.nmi_evaluate(ppe, idx, q["mats"], np.full(len(ppe), wt), np.full(len(ppe), nbt), nbs, histograms=True)
    assert sums[:, 0].min() > 50 and lncc[:, 0].max() > 50 and nmi[:, 0].min() > 50
    return [ncc, sums, lncc, kmap, nmi, hist, rec.ncc_get_targets(), rec.ncc_get_source()]


def test_registration_targets_and_source_at_a_large_a_small_and_the_large_grid_again():
    from fetalreconstruction_amd import engine as E
    large, small = _metric_case(21, 6, 100, 93, (40, 44, 38)), _metric_case(22, 3, 20, 17, (14, 16, 15))
    want = {}
    for key, q in (("large", large), ("small", small)):
        fresh = E.Reconstruction(0)
        want[key] = _metrics(fresh, q)
        fresh.close()
    rec = E.Reconstruction(0)
    for step, (key, q) in enumerate((("large", large), ("small", small), ("large", large))):
        for k, (g, w) in enumerate(zip(_metrics(rec, q), want[key])):
            assert np.array_equal(g, w, equal_nan=g.dtype.kind == "f"), (step, key, k)
    rec.close()


EYE = np.eye(4, dtype=np.float32).reshape(1, 16)
REG_SCHEDULE = (2, 1, 2)                                                           # both levels (what test_whole_runs_device_against_device runs from 1024 slices on)


def _register(rec, c):
    """a whole slice-to-volume registration of a case of tests/reg_cases.py on the context, everything uploaded again"""
    from fetalreconstruction_amd import engine as E
    rec.InitReconstructionVolume((c.vx, c.vy, c.vz), (c.vdim,) * 3, None, 12.0)
    rec.initStorageVolumes((1, 1, 1), (1.0, 1.0, 1.0))
    rec.SetSliceMatrices(EYE, EYE, EYE, EYE, EYE, EYE, EYE[0], c.w2i)
    rec.UpdateReconstructed((c.vx, c.vy, c.vz), c.vol)
    rec.initRegStorageVolumes(c.W, c.H, c.ns)
    rec.FillRegSlices(c.targets)
    rec.updateResampledSlicesI2W(c.ofs)
    rec.prepareSliceToVolumeReg()
    rec.set_schedule(*REG_SCHEDULE)
    t = rec.registerSlicesToVolume(c.start)
    act, ls_max, _ = rec.reg_get(E.REG_ACTIVE)
    return [t.view(np.uint32), rec.reg_counters(), act, np.array([ls_max]), rec.reg_get(E.REG_SIMILARITIES).view(np.uint32)]


def test_device_registration_state_large_small_large(oracle_mod):
    from fetalreconstruction_amd import engine as E
    import reg_cases
    pixels = lambda n: reg_cases.SPECS[n][2] * reg_cases.SPECS[n][3] * reg_cases.SPECS[n][4]   # noqa: E731
    large, small = max(reg_cases.NAMES, key=pixels), min(reg_cases.NAMES, key=pixels)
    assert (large, small) == ("ns_1100", "one_slice")
    want = {}
    for name in (large, small):
        fresh = E.Reconstruction(0)
        want[name] = _register(fresh, reg_cases.get(name))
        fresh.close()
        assert want[name][1][1] > 0 and not np.array_equal(want[name][0], reg_cases.get(name).start.reshape(-1, 4, 4).view(np.uint32))
    rec = E.Reconstruction(0)
    for step, name in enumerate((large, small, large)):
        for k, (g, w) in enumerate(zip(_register(rec, reg_cases.get(name)), want[name])):
            assert np.array_equal(g, w), (step, name, ("matrices", "counters", "active list", "line-search maximum", "similarities")[k])
    rec.close()
