"""The ranks of a sharded run's volume update by z-slabs (csrc/svr_slab.inc) in ONE process: W engine contexts on one device play
the W ranks, and the two collectives between the entry points are done here in numpy, adding the ranks in rank order:

    svr_slab_rs_pack on every rank -> recv_r = sum over q = 0 .. W - 1 of send_q[r] (float32, in that order) -> svr_slab_update
    -> every rank's all-gather part, concatenated [W][ag_chunk], to every rank -> svr_slab_finish.

The masks and volumes of tests/test_slab_gpu.py live here too (numpy only: tests/test_distributed_cpu.py runs the numpy
restatement of the plan over the same masks).  No fixtures, no process spawn; importing this needs no GPU."""
import dataclasses

import numpy as np

VOLUMES = [(19, 17, 23), (33, 9, 5), (65, 17, 6), (8, 8, 37)]      # (vx, vy, vz)
MASKS = ["a", "b", "c", "d", "e0", "e1", "f", "g", "h"]
POISON = -7777.0       # what a rank finds in its own part of the all-gather's result: svr_slab_finish must not read it


def make_mask(vsize, name):
    """float32 [vz][vy][vx].  a: an ellipsoid with 40 voxels knocked out (at (19, 17, 23): the mask of
    test_slab_plan_covers_every_voxel_once); b: the full volume; c: two parts with two empty planes between them; d: one full plane
    that holds more than half of the mask, one voxel in every other plane; e0 / e1: the plane z = 0 / z = vz - 1 alone; f: one voxel
    in the far corner; g: empty; h: a with 25 entries of -1 scattered over the volume (the code tests != 0)."""
    vx, vy, vz = vsize
    z, y, x = np.mgrid[:vz, :vy, :vx]
    m = np.zeros((vz, vy, vx), np.float32)
    if name in ("a", "h"):
        rng = np.random.default_rng(3)
        m = ((((z - (vz - 1) / 2.0) / (9.0 / 23 * vz)) ** 2 + ((y - (vy - 1) / 2.0) / (6.5 / 17 * vy)) ** 2 +
              ((x - (vx - 1) / 2.0) / (7.0 / 19 * vx)) ** 2) < 1).astype(np.float32)
        m[rng.integers(0, vz, 40), rng.integers(0, vy, 40), rng.integers(0, vx, 40)] = 0
        if name == "h":
            m[rng.integers(0, vz, 25), rng.integers(0, vy, 25), rng.integers(0, vx, 25)] = -1
    elif name == "b":
        m[...] = 1
    elif name == "c":
        g0 = vz // 2 - 1                                    # planes g0, g0 + 1 stay empty
        m[(z < g0) & (y < 0.6 * vy) & (x < 0.7 * vx)] = 1
        m[(z >= g0 + 2) & (y >= 0.3 * vy) & (x >= 0.2 * vx)] = 1
    elif name == "d":
        m[vz // 2] = 1
        zz = np.array([k for k in range(vz) if k != vz // 2])
        m[zz, zz % vy, (2 * zz) % vx] = 1
    elif name == "e0":
        m[0] = 1
    elif name == "e1":
        m[vz - 1] = 1
    elif name == "f":
        m[vz - 1, vy - 1, vx - 1] = 1
    elif name != "g":
        raise ValueError(name)
    return m


def make_case(vsize, mask, seed=0):
    """a phantom.Problem on the volume grid (vx, vy, vz) at 1 mm with the given mask, and one stack of 8 slices of 12 x 12 at
    0.5 mm around the volume's centre: enough for a real SuperresolutionBackproject, which marks addon | cmap as the scatter's"""
    from fetalreconstruction_amd import geometry as geo, phantom
    vx, vy, vz = vsize
    P = phantom.make_problem(1, (12, 12, 8), 0.5, 0.5, None, 1.0, 4.0, motion_frac=0.0, seed=seed, orientations=("ax",))
    a = geo.ImageAttributes(vx, vy, vz, 1.0, 1.0, 1.0)
    return dataclasses.replace(P, vsize=(vx, vy, vz), vdim=(1.0, 1.0, 1.0), recon_i2w=geo.to_matrix4(geo.image_to_world(a)),
                               recon_w2i=geo.to_matrix4(geo.world_to_image(a)),
                               mask=np.ascontiguousarray(np.asarray(mask, np.float32).reshape(vz, vy, vx)))


def open_context(P):
    """one engine context synced with P and ready for SuperresolutionBackproject"""
    from fetalreconstruction_amd import engine as E
    rec = E.Reconstruction(0)
    E.sync_gpu(rec, P)
    ones = np.ones(P.ns, np.float32)
    rec.UpdateScaleVector(ones, ones)
    rec.GaussianReconstruction()           # (v_PSF_sums: the scatter's pixel list)
    rec.InitializeEMValues()
    rec.SimulateSlices()
    return rec


def ranks(P, W):
    """W contexts, context r planned as rank r of W"""
    out = []
    for r in range(W):
        out.append(open_context(P))
        out[-1].slab_chunks(W, r)
    return out


def close_all(ctxs):
    for c in ctxs:
        c.close()


def inject(ctx, addon, cmap):
    """addon | cmap of the context := the given volumes, which must be exactly zero outside the mask (what the mask-box shortcut and
    the mask-only reduce-scatter rest on), written behind the engine's back after a real back-projection: they stay `the scatter's`"""
    from fetalreconstruction_amd import engine as E
    ctx.SuperresolutionBackproject(np.ones(ctx.sgrid[0], np.float32))
    pair = np.concatenate([np.asarray(addon, np.float32).ravel(), np.asarray(cmap, np.float32).ravel()])
    ctx.write_floats(ctx.device_ptr(E.BUF_ADDON), pair)           # one allocation of 2 Nv floats


def rank_sum(arrays):
    """float32 sum in rank order 0 .. W - 1: what a collective that adds the ranks in rank order gives"""
    s = np.zeros_like(np.asarray(arrays[0], np.float32))
    for a in arrays:
        s = s + np.asarray(a, np.float32)
    return s


def _stage(h, W, r, inputs, start):
    """context h becomes rank r of W: `start` (if given) its volume, the rank's addon | cmap injected, planned, its message packed
    -> (message sizes, send, recv)"""
    from fetalreconstruction_amd import engine as E
    if start is not None:
        h.debug_set(E.BUF_RECONSTRUCTED, np.asarray(start, np.float32).ravel())
    inject(h, *inputs[r])
    chunks = h.slab_chunks(W, r)
    return (chunks,) + h.slab_rs_pack()


def _reduce_scatter(sends, W):
    """recv_r = sum over q = 0 .. W - 1 of send_q[r]"""
    return [rank_sum([sends[q][r] for q in range(W)]) for r in range(W)]


def _gathered(parts, r):
    """what rank r receives from the all-gather, its own part poisoned"""
    full = np.stack(parts).copy()
    full[r] = POISON
    return full


def run_slab(ctxs, W, inputs, args, start=None, after_update=None):
    """One slab update of W ranks on W contexts.  inputs[r] = (addon, cmap) of rank r.  A context keeps its volume (state sequences)
    unless `start` is given, which debug_set makes its volume first.  The own part of what a rank receives before svr_slab_finish
    is POISON.  after_update(r, ctx) runs between a rank's svr_slab_update and its svr_slab_finish.
    -> dict(chunks = (2 rs_chunk, ag_chunk), sends [W] of [W][2][rs_chunk], recvs [W] of [2][rs_chunk], parts [W] of [ag_chunk],
    vols [W] of [Nv])."""
    assert len(ctxs) == W
    sends, ptrs, chunks = [], [], set()
    for r, h in enumerate(ctxs):
        (rs2, ag), send, recv = _stage(h, W, r, inputs, start)
        chunks.add((rs2, ag))
        sends.append(h.read_floats(send, W * rs2).reshape(W, 2, rs2 // 2))
        ptrs.append(recv)
    assert len(chunks) == 1, chunks                 # every rank reports the same message sizes
    recvs = _reduce_scatter(sends, W)
    parts = []
    for r, h in enumerate(ctxs):
        h.write_floats(ptrs[r], recvs[r])
        send, ptrs[r] = h.slab_update(*args)
        if after_update is not None:
            after_update(r, h)
        parts.append(h.read_floats(send, ag))
    vols = []
    for r, h in enumerate(ctxs):
        h.write_floats(ptrs[r], _gathered(parts, r))
        h.slab_finish()
        vols.append(h.syncCPU())
    return dict(chunks=(rs2, ag), sends=sends, recvs=recvs, parts=parts, vols=vols)


def run_slab_pooled(ctxs, W, inputs, args, start):
    """run_slab for more ranks than contexts may be open at once: context r % K plays rank r, always from the volume `start`.  Three
    passes over the ranks, each staging the rank afresh: the messages; the update, for every all-gather part; the update again and
    svr_slab_finish.  Same result dict."""
    K = len(ctxs)
    sends, chunks = [], set()
    for r in range(W):
        h = ctxs[r % K]
        (rs2, ag), send, _ = _stage(h, W, r, inputs, start)
        chunks.add((rs2, ag))
        sends.append(h.read_floats(send, W * rs2).reshape(W, 2, rs2 // 2))
    assert len(chunks) == 1, chunks
    recvs = _reduce_scatter(sends, W)

    def update(r):
        h = ctxs[r % K]
        _, _, recv = _stage(h, W, r, inputs, start)
        h.write_floats(recv, recvs[r])
        return (h,) + h.slab_update(*args)

    parts = []
    for r in range(W):
        h, send, _ = update(r)
        parts.append(h.read_floats(send, ag))
    vols = []
    for r in range(W):
        h, send, recv = update(r)
        assert np.array_equal(h.read_floats(send, ag), parts[r])
        h.write_floats(recv, _gathered(parts, r))
        h.slab_finish()
        vols.append(h.syncCPU())
    return dict(chunks=(rs2, ag), sends=sends, recvs=recvs, parts=parts, vols=vols)


def run_replicated(ctx, addon_sum, cmap_sum, args, recon=None):
    """the replicated form on one more context: the rank-ordered sums of the ranks' addon | cmap, then the whole-volume update
    (pinned to the oracle by test_regulariser_parity and the shape sweep).  recon: the starting volume, or None to keep the context's."""
    from fetalreconstruction_amd import engine as E
    if recon is not None:
        ctx.debug_set(E.BUF_RECONSTRUCTED, np.asarray(recon, np.float32).ravel())
    inject(ctx, addon_sum, cmap_sum)
    ctx.SuperresolutionUpdate(*args)
    return ctx.syncCPU()


def dilate(m):
    """3 x 3 x 3 dilation of a boolean [vz][vy][vx] volume, clipped at the faces"""
    p = np.pad(m, 1)
    d = np.zeros_like(m)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                d |= p[dz:dz + m.shape[0], dy:dy + m.shape[1], dx:dx + m.shape[2]]
    return d
