"""The sharded volume update by z-slabs on the device (csrc/svr_slab.inc, the svr_slab_* entry points, the z-range form of
k_regul_fused), rank by rank in one process: W engine contexts play the W ranks and tests/slab_ranks.py does the reduce-scatter
and the all-gather in numpy, adding the ranks in rank order.  Against tests/twins/reconstruction.py::slab_plan_numpy (the plan and
both messages, voxel by voxel) and against the whole-volume SuperresolutionUpdate of one more context that is given the
rank-ordered sums (pinned to the oracle by test_regulariser_parity and tests/test_shape_sweep_gpu.py).  Every comparison is
array_equal: with the ranks added in rank order the slab form computes the replicated form's bits."""
import numpy as np
import pytest

from tests import slab_ranks as SR
from tests.twins.reconstruction import slab_plan_numpy

pytestmark = pytest.mark.gpu

MAX_RANK_CONTEXTS = 15          # + the replicated twin: 16 contexts open at once


def _start(mask, seed):
    """random positive inside the mask, zero outside"""
    rng = np.random.default_rng(1000 + seed)
    return np.where(mask != 0, rng.uniform(20.0, 120.0, mask.shape), 0.0).astype(np.float32).ravel()


def _inputs(mask, W, seed, kind):
    """per rank (addon, cmap), exactly zero outside the mask.  random: cmap in (0, 2) at a random 70 % of the mask's voxels, addon
    random there; eighths: small integers / 8, so that the ranks' sums are exact in any order (what an RCCL ring and the
    twice-reduced halo plane would give); index: addon[i] = i + 1, cmap[i] = -(i + 1) at the mask's voxels on every rank (exact in
    float32 below 2^24 / W): the reduce-scatter message then IS the index list"""
    m = mask.ravel() != 0
    out = []
    for r in range(W):
        rng = np.random.default_rng([seed, r, W])
        if kind == "index":
            i = np.arange(m.size, dtype=np.float32) + 1
            out.append((np.where(m, i, 0).astype(np.float32), np.where(m, -i, 0).astype(np.float32)))
            continue
        sel = m & (rng.random(m.size) < 0.7)
        if kind == "random":
            a, c = rng.normal(0.0, 30.0, m.size), rng.uniform(0.05, 1.95, m.size)
        else:
            a, c = rng.integers(-64, 65, m.size) / 8.0, rng.integers(1, 16, m.size) / 8.0
        out.append((np.where(sel, a, 0).astype(np.float32), np.where(sel, c, 0).astype(np.float32)))
    return out


def _args(start, mask, adaptive):
    """(adaptive, alpha, min, max, delta, lambda) with both clamps firing: min / max at the 25th / 60th percentile of the volume"""
    v = start[mask.ravel() != 0]
    lo, hi = (np.percentile(v, 25), np.percentile(v, 60)) if v.size else (0.0, 1.0)
    delta, alpha = 30.0, 1.0
    return (adaptive, alpha, float(lo), float(hi), delta, 0.05 * delta * delta / alpha)


def _check(ctxs, twin, mask, W, inputs, args, start=None, after_update=None):
    """one slab update of W ranks against the numpy plan (assertions 1, 2) and the replicated twin (assertion 3)"""
    plan = slab_plan_numpy(mask, W)
    midx, didx, CH, AG = plan["midx"], plan["didx"], plan["rs_chunk"], plan["ag_chunk"]
    if len(ctxs) < W:                               # more ranks than contexts may be open: a context plays several ranks
        assert after_update is None
        out = SR.run_slab_pooled(ctxs, W, inputs, args, start)
    else:
        out = SR.run_slab(ctxs, W, inputs, args, start=start, after_update=after_update)
    # 1. the plan: message sizes, and every rank's reduce-scatter message voxel by voxel (zero padded; an empty slab sends zeros)
    assert out["chunks"] == (2 * CH, AG)
    for q in range(W):
        want = np.zeros((W, 2, CH), np.float32)
        for r, (st, cnt) in enumerate(plan["rs"]):
            want[r, 0, :cnt] = inputs[q][0][midx[st:st + cnt]]
            want[r, 1, :cnt] = inputs[q][1][midx[st:st + cnt]]
        assert np.array_equal(out["sends"][q], want), f"world {W}: reduce-scatter message of rank {q}"
    ref = SR.run_replicated(twin, SR.rank_sum([a for a, _ in inputs]), SR.rank_sum([c for _, c in inputs]), args, recon=start)
    dil = np.zeros(mask.size, bool)
    dil[didx] = True
    assert np.array_equal(dil.reshape(mask.shape), SR.dilate(mask != 0))
    # 3. every rank ends with the same volume: the replicated update's on the dilated mask, exactly 0.0 outside
    vols = out["vols"]
    for r in range(W):
        assert np.array_equal(vols[r], vols[0]), f"world {W}: volume of rank {r}"
        assert np.array_equal(vols[r][dil], ref[dil]), f"world {W}: rank {r} against the replicated update"
        assert not vols[r][~dil].any(), f"world {W}: rank {r} outside the dilated mask"
    # 2. rank r's all-gather part is the new volume at its range of the dilated list, zero padded; the ranges partition the list
    cover = np.zeros(len(didx), int)
    for r, (st, cnt) in enumerate(plan["ag"]):
        want = np.zeros(AG, np.float32)
        want[:cnt] = vols[0][didx[st:st + cnt]]
        assert np.array_equal(out["parts"][r], want), f"world {W}: all-gather part of rank {r}"
        cover[st:st + cnt] += 1
    assert (cover == 1).all()
    return out, ref, plan


def _open(vsize, name, n_ranks, seed=0):
    mask = SR.make_mask(vsize, name)
    P = SR.make_case(vsize, mask, seed)
    return mask, P, SR.ranks(P, n_ranks), SR.open_context(P)


_CASES = [(v, m) for v in SR.VOLUMES for m in SR.MASKS]
_ids = lambda c: "-".join("x".join(map(str, p)) if isinstance(p, tuple) else str(p) for p in c)


@pytest.mark.parametrize("case", _CASES, ids=_ids)
def test_plan_messages_and_result_at_worlds_1_to_8(case):
    """every mask on every volume at worlds 1, 2, 3, 5, 8 (reg_tile -1), the contexts re-planned from world to world: the index leg
    (the message is the index list), the random leg (adaptive) and the exact-eighths leg (non-adaptive).  The all-zero mask plans,
    exchanges all-zero messages and gives an all-zero volume."""
    vsize, name = case
    mask, P, ctxs, twin = _open(vsize, name, 8)
    try:
        start = _start(mask, 1)
        for W in (1, 2, 3, 5, 8):
            for kind, adaptive in (("index", False), ("random", True), ("eighths", False)):
                ins = _inputs(mask, W, 7, kind)
                out, ref, _ = _check(ctxs[:W], twin, mask, W, ins, _args(start, mask, adaptive), start=start)
                if name == "g":
                    assert not any(s.any() for s in out["sends"]) and not any(v.any() for v in out["vols"]) and not ref.any()
                elif kind == "random" and SR.rank_sum([c for _, c in ins]).any():
                    assert out["vols"][0].any()
    finally:
        SR.close_all(ctxs + [twin])


_BIG = [(v, m, w) for v in SR.VOLUMES for m in ("a", "d", "e0", "e1") for w in (v[2], v[2] + 3)]


@pytest.mark.parametrize("case", _BIG, ids=_ids)
def test_more_ranks_than_planes(case):
    """worlds vz and vz + 3: empty slabs at the end and in the middle (a rank's share of the mask inside one fat plane), ranks that
    send and receive padding only.  More ranks than contexts may be open: a context plays several ranks (slab_ranks.run_slab)."""
    vsize, name, W = case
    mask, P, ctxs, twin = _open(vsize, name, min(W, MAX_RANK_CONTEXTS))
    try:
        start = _start(mask, 2)
        plan = slab_plan_numpy(mask, W)
        assert any(a == b for a, b in zip(plan["zb"], plan["zb"][1:]))              # the case has empty slabs
        for kind, adaptive in (("index", False), ("random", True)):
            _check(ctxs, twin, mask, W, _inputs(mask, W, 11, kind), _args(start, mask, adaptive), start=start)
    finally:
        SR.close_all(ctxs + [twin])


_TILE_CASES = [((19, 17, 23), "a"), ((33, 9, 5), "b"), ((65, 17, 6), "b"), ((8, 8, 37), "a")]


@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("case", _TILE_CASES, ids=_ids)
def test_every_tile_shape_on_slabs(case, adaptive):
    """reg_tile -1, 0, 1 (32 x 8, 64 x 8, 32 x 16) x adaptive on one mask per volume at worlds 2 and 3: partial tiles of each shape on
    planes [z_lo, z_hi) with z_lo > 0"""
    vsize, name = case
    mask, P, ctxs, twin = _open(vsize, name, 3)
    try:
        start = _start(mask, 3)
        for tile in (-1, 0, 1):
            for c in ctxs + [twin]:
                c.set_option("reg_tile", tile)
            for W in (2, 3):
                _check(ctxs[:W], twin, mask, W, _inputs(mask, W, 13 + tile, "random"), _args(start, mask, adaptive), start=start)
    finally:
        SR.close_all(ctxs + [twin])


@pytest.mark.parametrize("name", ["a", "b"])
def test_a_ranks_planes_before_finish_are_the_whole_volume_updates(name):
    """world 3 on (8, 8, 37): rank r's planes [zb_r, zb_r+1) of the buffer svr_slab_update wrote, read BEFORE svr_slab_finish, are the
    same planes of the whole-volume update: slabs of 6 - 16 planes in z-chunks of 4 (partial last chunks), the LDS ring starting at
    more than one z_lo & 3.  A first iteration tells the two volume buffers apart (the current volume's pointer before and after)."""
    from fetalreconstruction_amd import engine as E
    vsize, W = (8, 8, 37), 3
    mask, P, ctxs, twin = _open(vsize, name, W)
    try:
        start = _start(mask, 4)
        args = _args(start, mask, True)
        first = [c.device_ptr(E.BUF_RECONSTRUCTED) for c in ctxs]
        for c in ctxs:
            c.debug_set(E.BUF_RECONSTRUCTED, start)
        _check(ctxs, twin, mask, W, _inputs(mask, W, 17, "random"), args, start=start)
        assert all(c.device_ptr(E.BUF_RECONSTRUCTED) != p for c, p in zip(ctxs, first))      # the volume flipped: `first` is written next
        seen, zc = {}, {}

        def grab(r, h):
            seen[r] = h.read_floats(first[r], P.nvox)
            zc[r] = (h.get_option("reg_zc"), h.get_option("reg_chunks"))

        out, ref, plan = _check(ctxs, twin, mask, W, _inputs(mask, W, 19, "random"), args, after_update=grab)
        zb, plane = plan["zb"], vsize[0] * vsize[1]
        assert any((b - a) % 4 for a, b in zip(zb, zb[1:])) and len({z & 3 for z in zb[:-1]}) > 1, zb
        assert all(zc[r] == (4, (zb[r + 1] - zb[r] + 3) // 4) for r in range(W)), (zc, zb)
        for r in range(W):
            assert np.array_equal(seen[r][zb[r] * plane:zb[r + 1] * plane], ref[zb[r] * plane:zb[r + 1] * plane]), f"rank {r}"
    finally:
        SR.close_all(ctxs + [twin])


@pytest.mark.parametrize("name", ["b", "c", "e0", "e1"])
@pytest.mark.parametrize("vsize", [(5, 5, 5), (33, 9, 5)], ids=lambda v: "x".join(map(str, v)))
def test_the_scatter_writes_mask_voxels_only(vsize, name):
    """what the mask-only reduce-scatter and the mask-box shortcut rest on: after a real SuperresolutionBackproject addon != 0 and
    cmap != 0 lie inside mask != 0.  The harness's stack (6 x 6 x 4 mm around the centre) covers (5, 5, 5) up to all six faces and
    reaches both end planes of (33, 9, 5): with the one-plane masks e0 / e1, the full volume b and the two parts c (which touch
    opposite faces and leave voxels outside the mask next to written ones) the scatter writes at z = 0 and z = vz - 1 and is
    clipped there; every mask receives something."""
    from fetalreconstruction_amd import engine as E
    mask = SR.make_mask(vsize, name)
    P = SR.make_case(vsize, mask)
    c = SR.open_context(P)
    try:
        c.SuperresolutionBackproject(np.ones(P.ns, np.float32))
        addon, cmap, m = c.debug_get(E.BUF_ADDON), c.debug_get(E.BUF_CONFIDENCE_MAP), mask.ravel() != 0
        print(f"{vsize} {name}: cmap != 0 at {int((cmap != 0).sum())} of {int(m.sum())} mask voxels, addon != 0 at {int((addon != 0).sum())}")
        assert not addon[~m].any() and not cmap[~m].any()
        assert cmap[m].any() and addon[m].any()
        vx, vy, vz = vsize
        hit = (cmap != 0).reshape(vz, vy, vx)
        if name in ("b", "e0"):
            assert hit[0].any()                      # written at the face z = 0 ...
        if name in ("b", "e1"):
            assert hit[vz - 1].any()                 # ... and at z = vz - 1
    finally:
        c.close()


@pytest.mark.parametrize("seq", ["slab_x3", "whole_then_slab", "slab_whole_slab", "debug_set", "set_mask", "replan"])
def test_state_sequences_keep_ranks_and_twin_in_step(seq):
    """mask a on (19, 17, 23), world 3, the three rank contexts and the replicated twin in step; assertions 1-3 after every slab update.
    Every rank AND the twin start from the same volume, non-zero everywhere, and are given the same volumes later.  The slab form
    promises zeros outside the dilated mask whatever the old volume held there (svr_slab.inc: both buffers are kept zero there, a
    buffer somebody else wrote is cleared first); the comparison with the twin is on the dilated mask, where both forms read the
    same old volume.
    A whole-volume update does not carry the OLD VOLUME's values over: where no neighbour has confidence it writes 0 (valW = 0),
    and cmap is 0 outside the mask while it is the scatter's.  It leaves values outside the dilated mask when cmap itself is
    non-zero there, i.e. set by debug_set: `whole_dirty` does that on every context, checks that the buffer it wrote is then
    non-zero outside the dilated mask, and the second slab update after it writes that very buffer."""
    from fetalreconstruction_amd import engine as E
    vsize, W = (19, 17, 23), 3
    mask, P, ctxs, twin = _open(vsize, "a", W)
    try:
        dil = SR.dilate(mask != 0).ravel()
        dirty = np.random.default_rng(8).uniform(20.0, 120.0, P.nvox).astype(np.float32)
        args = _args(dirty, mask, True)
        for c in ctxs + [twin]:
            c.debug_set(E.BUF_RECONSTRUCTED, dirty)
        step = [0]

        def slab(w=W, m=mask):
            step[0] += 1
            return _check(ctxs[:w], twin, m, w, _inputs(m, w, 100 + step[0], "random"), args)

        def whole():                                 # addon | cmap the scatter's: the rank-ordered sums on every context
            step[0] += 1
            ins = _inputs(mask, W, 100 + step[0], "random")
            a, c = SR.rank_sum([x for x, _ in ins]), SR.rank_sum([x for _, x in ins])
            vols = [SR.run_replicated(h, a, c, args) for h in ctxs + [twin]]
            assert all(np.array_equal(v, vols[0]) for v in vols)

        def whole_dirty():                           # addon | cmap set by debug_set, cmap > 0 everywhere: values everywhere
            step[0] += 1
            rng = np.random.default_rng(200 + step[0])
            a, c = rng.normal(0.0, 30.0, P.nvox).astype(np.float32), rng.uniform(0.05, 1.95, P.nvox).astype(np.float32)
            vols = []
            for h in ctxs + [twin]:
                h.debug_set(E.BUF_ADDON, a)
                h.debug_set(E.BUF_CONFIDENCE_MAP, c)
                h.SuperresolutionUpdate(*args)
                vols.append(h.syncCPU())
            assert all(np.array_equal(v, vols[0]) for v in vols) and vols[0][~dil].all()

        if seq == "slab_x3":                         # both volume buffers written and reused
            slab(), slab(), slab()
        elif seq == "whole_then_slab":               # the second slab update writes the buffer the whole-volume update left dirty
            whole_dirty(), slab(), slab(), whole(), slab()          # (never known clean before: cleared in any case)
        elif seq == "slab_whole_slab":               # ... after both buffers have been known clean: the whole-volume update has to
            slab(), slab(), whole_dirty(), slab(), slab()           # say that it wrote one (invalidate(CH_VOLUME_VALUES))
        elif seq == "debug_set":
            slab()
            for c in ctxs + [twin]:
                c.debug_set(E.BUF_RECONSTRUCTED, dirty[::-1].copy())
            slab(), slab()
        elif seq == "set_mask":
            slab()
            m2 = SR.make_mask(vsize, "c")
            for c in ctxs + [twin]:
                c.setMask(P.vsize, P.vdim, m2, 12.0)
            slab(m=m2), slab(m=m2)
        else:                                        # world 2 after world 3 on the same contexts: the lists stay, the boundaries move
            slab()
            out, _, _ = slab(w=2)
            ctxs[2].debug_set(E.BUF_RECONSTRUCTED, out["vols"][0])       # (rank 2 sat the iteration out)
            slab()
    finally:
        SR.close_all(ctxs + [twin])


def test_refusals_are_error_codes_with_a_message():
    from fetalreconstruction_amd import engine as E
    vsize = (19, 17, 23)
    mask = SR.make_mask(vsize, "a")
    P = SR.make_case(vsize, mask)
    c = SR.open_context(P)
    try:
        with pytest.raises(E.SvrError, match="svr_slab_plan first"):
            c.slab_rs_pack()
        with pytest.raises(E.SvrError, match="svr_slab_plan first"):
            c.slab_update(*_args(_start(mask, 1), mask, True))
        with pytest.raises(E.SvrError, match="svr_slab_plan first"):
            c.slab_finish()
        for world, rank in ((0, 0), (2, 2), (3, 7), (2, -1), (-1, 0)):
            with pytest.raises(E.SvrError, match="rank / world"):
                c.slab_chunks(world, rank)
        c.slab_chunks(2, 1)
        with pytest.raises(E.SvrError, match="svr_superresolution_backproject"):      # addon | cmap are not the scatter's yet
            c.slab_rs_pack()
        c.SuperresolutionBackproject(np.ones(P.ns, np.float32))
        c.slab_rs_pack()
        c.debug_set(E.BUF_ADDON, np.zeros(P.nvox, np.float32))
        with pytest.raises(E.SvrError, match="svr_superresolution_backproject"):
            c.slab_rs_pack()
        c.set_option("reg_mode", 0)
        with pytest.raises(E.SvrError, match="reg_mode 1"):
            c.slab_update(*_args(_start(mask, 1), mask, True))
        c.set_option("reg_mode", 1)
        c.SuperresolutionBackproject(np.ones(P.ns, np.float32))                        # and the context still works
        c.slab_rs_pack()
    finally:
        c.close()


# ---- the replicated path's exchange: the mask's bounding box of a volume pair (svr_pair_pack / svr_pair_unpack, k_pair_pack) ----
@pytest.mark.parametrize("case", _CASES, ids=_ids)
def test_pair_pack_is_the_masks_bounding_box(case):
    """the packed buffer is the box of both volumes; unpack after editing it changes the box and nothing else; nothing is packed
    (null pointer, 0 floats: the caller reduces the whole pair) for a box over 80 % of the volume and for the empty mask"""
    from fetalreconstruction_amd import engine as E
    vsize, name = case
    vx, vy, vz = vsize
    mask = SR.make_mask(vsize, name)
    P = SR.make_case(vsize, mask)
    c = SR.open_context(P)
    try:
        nv = P.nvox
        pair = np.random.default_rng(21).normal(0.0, 10.0, 2 * nv).astype(np.float32)
        c.write_floats(c.device_ptr(E.BUF_ADDON), pair)
        ptr, n = c.pair_pack(E.BUF_ADDON, 2 * nv)
        nz = np.argwhere(mask != 0)
        box = np.zeros(mask.shape, bool)
        if len(nz):
            lo, hi = nz.min(0), nz.max(0)
            box[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = True
        nb = int(box.sum())
        if nb == 0 or nb * 5 > nv * 4:
            assert not ptr and n == 0
            assert np.array_equal(c.read_floats(c.device_ptr(E.BUF_ADDON), 2 * nv), pair)
            return
        assert ptr and n == 2 * nb
        b = box.ravel()
        packed = c.read_floats(ptr, 2 * nb)
        assert np.array_equal(packed, np.concatenate([pair[:nv][b], pair[nv:][b]]))
        c.write_floats(ptr, packed * 2 + 1)                                    # what the collective would leave there
        c.pair_unpack(E.BUF_ADDON, 2 * nv)
        want = pair.copy()
        want[:nv][b] = packed[:nb] * 2 + 1
        want[nv:][b] = packed[nb:] * 2 + 1
        assert np.array_equal(c.read_floats(c.device_ptr(E.BUF_ADDON), 2 * nv), want)
    finally:
        c.close()
