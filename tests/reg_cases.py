"""Synthetic cases for the float slice-to-volume registration (csrc/svr_reg.inc) at the shapes where its kernels take another
path: no phantom, deterministic, named.  Used by tests/test_reg_ref.py (numpy reference against the C oracle, on the CPU) and
tests/test_reg_shapes_gpu.py (the device against both).

A case is a volume [vz][vy][vx] with -1 outside an ellipsoid mask and structure inside, its voxel size, a world-to-image
matrix, W x H x ns registration slices given by per-slice offset matrices (slice pixel -> world), targets sampled from the
volume at identity through the oracle (`evaluate_costs(identity, 0)[1][1]`, the blurred middle offset), and start matrices
knocked off by translations of +-0.7 voxel sizes (KNOCK: +-0.5 for the three large cases).

MEASURED[name] = the largest distance of the C oracle (float, the arithmetic of the device) from the float64 reference of
tests/reg_ref.py over both levels and the active lists of `active_lists`, as measured by tests/test_reg_ref.py, which fails when
a number here is no longer an upper bound within a factor 2: `slices` relative to the largest sample of the case, `sim`
absolute.  The device tolerances follow from them (tol_sim, tol_rel): the device accumulates in double, so it must not be
further from float64 than the float oracle is; the factor 2 covers the final float roundings.

TRAJECTORY[name] = a schedule (levels, steps, iterations) at which a whole registration run of the case is well-conditioned
(the oracle's counters and matrices do not move when the volume's non-negative voxels are scaled by 1 + 2^-20, 1 - 2^-19,
1 + 3 * 2^-21) or None: only the former are compared with the oracle as whole runs on the device."""
import functools
from types import SimpleNamespace

import numpy as np

#       name            volume (vx,vy,vz) vdim   W    H    ns   why
SPECS = {
    "wide_37x5":      ((9, 8, 12),   2.7,   37,  5,   3),    # W != H, H below the 7 half taps of level 1 (13 taps)
    "tall_5x37":      ((9, 8, 12),   2.7,   5,   37,  3),    # the transpose: W below the half kernel
    "one_slice":      ((9, 8, 12),   1.0,   11,  9,   1),    # ns = 1: the scratch aliasing wipes everything
    "wave_3x3":       ((9, 8, 12),   1.0,   3,   3,   65),   # fewer pixels than a wavefront; 65 slices
    "line_257":       ((30, 8, 12),  1.0,   257, 1,   2),    # one pixel more than a 256-lane workgroup; H = 1
    "red_4270":       ((20, 18, 12), 1.0,   70,  61,  2),    # above 4096 pixels, no multiple of 1024: 1024 lanes chosen
    "red_4096":       ((20, 18, 12), 1.0,   64,  64,  2),    # exactly 4096: stays on 256 lanes
    "ns_1024":        ((9, 8, 12),   1.0,   6,   5,   1024),  # one full chunk of the compaction
    "ns_1025":        ((9, 8, 12),   1.0,   6,   5,   1025),  # one slice into the second chunk
    "ns_1100":        ((9, 8, 12),   1.0,   6,   5,   1100),  # the second chunk
    "cap_63":         ((9, 8, 12),   12.8,  20,  9,   3),    # level 1 at the 63-tap cap (32 half taps), level 0 at 31 taps
    "skew_9x14x11":   ((9, 14, 11),  1.3,   13,  10,  4),    # three non-power-of-two sizes, rotated world-to-image, integer voxels
    "dead_slices":    ((9, 8, 12),   1.0,   12,  7,   5),    # slice 1: targets all -1; slice 3: entirely outside the volume
}
NAMES = list(SPECS)
INTEGER = ("skew_9x14x11", "wave_3x3")

MEASURED = {
    "wide_37x5":    dict(slices=2.49e-07, sim=1.14e-07),
    "tall_5x37":    dict(slices=2.81e-07, sim=1.08e-07),
    "one_slice":    dict(slices=2.17e-07, sim=2.90e-08),
    "wave_3x3":     dict(slices=2.45e-07, sim=1.23e-06),
    "line_257":     dict(slices=2.67e-07, sim=2.98e-07),
    "red_4270":     dict(slices=3.23e-07, sim=2.71e-07),
    "red_4096":     dict(slices=3.37e-07, sim=2.25e-07),
    "ns_1024":      dict(slices=3.16e-07, sim=3.92e-07),
    "ns_1025":      dict(slices=2.95e-07, sim=3.85e-07),
    "ns_1100":      dict(slices=2.93e-07, sim=5.88e-07),
    "cap_63":       dict(slices=2.28e-07, sim=1.84e-06),
    "skew_9x14x11": dict(slices=1.74e-07, sim=3.19e-07),
    "dead_slices":  dict(slices=2.63e-07, sim=5.02e-07),
}
# hence, with tol_sim / tol_rel below: similarities within 2e-6 (wave_3x3 2.46e-6, cap_63 3.68e-6), sums and moments within
# 3.5e-7 (skew_9x14x11) to 6.7e-7 (red_4096) of their magnitude

# A schedule of (2,4,20), (2,2,3), (2,1,2), (1,2,3), (1,1,2), (1,1,1) that passes: the longest one when the cases were made (the test
# asserts that the recorded one passes; it reruns the next longer one and reports it, without pinning an instability).  None: no schedule passes -- ns_1025 moves one
# slice of 1025 by 1.2e-5 at (1,1,1), cap_63 and skew_9x14x11 two to three of their slices; they are left to the stage tests and
# the device-against-device runs.
TRAJECTORY = {
    "wide_37x5": (1, 1, 1), "tall_5x37": (1, 1, 1), "one_slice": (1, 1, 2), "wave_3x3": (1, 1, 1), "line_257": (1, 1, 2),
    "red_4270": (1, 1, 1), "red_4096": (1, 1, 1), "ns_1024": (1, 1, 1), "ns_1025": None, "ns_1100": (1, 1, 1), "cap_63": None,
    "skew_9x14x11": None, "dead_slices": (1, 1, 2),
}
SCHEDULES = ((2, 4, 20), (2, 2, 3), (2, 1, 2), (1, 2, 3), (1, 1, 2), (1, 1, 1))

# Start translations in voxel sizes, +-0.7 unless listed.  With +-0.7 the 1100 slices of ns_1100 on THIS volume (its +-25 of voxel noise
# on 6 x 5 pixel images) are not well-conditioned at any schedule: at (1,1,1) the counters stay but 1-2 slices of 1100 move by
# 1.2e-5 to 3.9e-5 under the three perturbations, after up to 36 line-search steps along a normalised gradient.  At +-0.5 the line
# search is shorter (23 steps) and no slice moves, while the first step still keeps 1063 > 1024 slices.
KNOCK = {"ns_1024": 0.5, "ns_1025": 0.5, "ns_1100": 0.5}

PERTURBATIONS = (1 + 2.0 ** -20, 1 - 2.0 ** -19, 1 + 3 * 2.0 ** -21)


def tol_sim(name):
    """similarities, absolute: the project's 2e-6 or twice the oracle's own distance from float64"""
    return max(2e-6, 2 * MEASURED[name]["sim"])


def tol_rel(name):
    """sums and moments, relative to their magnitude (count x largest sample, pairs x its square: `slices` is recorded relative
    to the largest sample): twice the oracle's relative distance of the blurred slices"""
    return 2 * MEASURED[name]["slices"]


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
            @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def volume(name):
    (vx, vy, vz), vdim = SPECS[name][:2]
    rng = np.random.default_rng(sum(map(ord, name)))
    k, j, i = np.meshgrid(np.arange(vz), np.arange(vy), np.arange(vx), indexing="ij")
    u, v, w = (i - (vx - 1) / 2) / (vx / 2), (j - (vy - 1) / 2) / (vy / 2), (k - (vz - 1) / 2) / (vz / 2)
    val = 300 + 150 * np.sin(2.1 * u + 0.3) * np.cos(1.7 * v) + 120 * w * u + 80 * np.cos(2.9 * w + v) + rng.uniform(-25, 25, u.shape)
    if name in INTEGER:
        val = np.rint(val)
    return np.where(u * u + v * v + w * w < 0.92, val, -1.0).astype(np.float32)


def geometry(name):
    """-> (recon_w2i [16], ofs [ns][16], identity [ns][16], start [ns][16]) in float32"""
    (vx, vy, vz), vdim, W, H, ns = SPECS[name]
    w2i = np.eye(4)
    w2i[:3, :3] = np.eye(3) / vdim
    if name == "skew_9x14x11":
        w2i[:3, :3] = _rot(0.21, -0.17, 0.4) / vdim
    w2i[:3, 3] = (vx / 2, vy / 2, vz / 2)
    grow = 1.5 if name == "skew_9x14x11" else 0.9            # skew: the slices stick out of the volume on every side
    sx, sy = grow * vdim * vx / W, grow * vdim * vy / H
    ofs = np.zeros((ns, 4, 4))
    for s in range(ns):
        m = np.eye(4)
        m[:3, :3] = _rot(0.02 * (s % 5) - 0.04, 0.03 * (s % 3) - 0.03, 0.05 * (s % 7) - 0.15) @ np.diag([sx, sy, 0.5 * vdim])
        z = (((s * 7) % 11) / 10 - 0.5) * 0.6 * vz * vdim
        m[:3, 3] = m[:3, :3] @ (-(W - 1) / 2, -(H - 1) / 2, 0) + (0.1 * vdim * ((s % 4) - 1.5), 0.07 * vdim * ((s % 3) - 1), z)
        ofs[s] = m
    if name == "dead_slices":
        ofs[3, :3, 3] += (0, 0, 40 * vz * vdim)
    ident = np.tile(np.eye(4), (ns, 1, 1))
    rng = np.random.default_rng(ns * 1000 + W)
    start = ident.copy()
    start[:, :3, 3] = rng.choice([-1.0, 1.0], (ns, 3)) * KNOCK.get(name, 0.7) * vdim
    f = lambda a: np.ascontiguousarray(a, np.float32).reshape(-1, 16)
    return f(w2i)[0], f(ofs), f(ident), f(start)


def oracle_for(c, vol=None):
    """an OracleRegistration holding the case (targets included when the case has them already)"""
    from oracle import pyoracle as po
    o = po.OracleRegistration((c.vx, c.vy, c.vz), c.vdim, c.w2i)
    o.initRegStorageVolumes(c.W, c.H, c.ns)
    o.FillRegSlices(c.targets if getattr(c, "targets", None) is not None else np.zeros((c.ns, c.H, c.W), np.float32))
    o.updateResampledSlicesI2W(c.ofs)
    o.prepareSliceToVolumeReg(c.vol if vol is None else vol)
    return o


@functools.lru_cache(maxsize=None)
def get(name):
    (vx, vy, vz), vdim, W, H, ns = SPECS[name]
    c = SimpleNamespace(name=name, vx=vx, vy=vy, vz=vz, vdim=vdim, W=W, H=H, ns=ns, vol=volume(name), targets=None,
                        integer=name in INTEGER)
    c.w2i, c.ofs, c.ident, c.start = geometry(name)
    c.targets = oracle_for(c).evaluate_costs(c.ident, 0)[1][1].copy()
    if name == "dead_slices":
        c.targets[1] = -1.0
    c.targets.setflags(write=False)
    c.vol.setflags(write=False)
    return c


def active_lists(c):
    """all, a few, reversed, a single last slice, and from 1024 slices on a list that straddles 1024"""
    ns = c.ns
    out = [None, sorted({0, ns // 3, ns - 1}), list(range(ns - 1, -1, -1)), [ns - 1]]
    if ns >= 1024:
        out.append(list(range(ns - 1030, ns)) if ns >= 1030 else list(range(1, ns, 1)) + [0])
    return out


def perturbed(vol, f):
    """the volume with its non-negative voxels scaled by f"""
    return np.where(vol >= 0, (vol.astype(np.float64) * f).astype(np.float32), vol)


def oracle_run(c, schedule, vol=None):
    """a whole registration of the case on the oracle from its start matrices -> (matrices [ns][4][4], counters, active list
    left behind, the most slices a line-search step kept)"""
    o = oracle_for(c, vol)
    o.set_schedule(*schedule)
    t = o.registerSlicesToVolume(c.start)
    act, ls_max = o.final_active()
    return t, o.counters.copy(), act, ls_max


@functools.lru_cache(maxsize=None)
def reference(name, level, k):
    """the float64 reference of the case's evaluation at its start matrices, level and k-th active list (computed once)"""
    import reg_ref
    c = get(name)
    return reg_ref.evaluate(c.vol, c.vdim, c.w2i, c.ofs, c.targets, c.start, level, active_lists(c)[k])


# ---- the patch cost (k_cc_patch / k_pvr_patch_opt) at awkward patch shapes ------------------------------------------------------------
#                 px  py  n    nx*ny*3 at level 0: 105 / 207 (below a 256-lane workgroup) / 741; no size but one divisible by 2 or 3
PATCH_SPECS = {"p_7x5": (7, 5, 6), "p_23x3": (23, 3, 5), "p_19x13": (19, 13, 6)}
PATCH_NAMES = list(PATCH_SPECS)
# the largest relative distance of the oracle's six sums (sequential float sums, orc_cc_patch) from the float64 reference over
# levels 0-2 on the generic data, as tests/test_reg_ref.py measures it; the device sums in double and must stay within twice that
PATCH_MEASURED = {"p_7x5": 4.68e-07, "p_23x3": 3.10e-07, "p_19x13": 1.23e-06}


@functools.lru_cache(maxsize=None)
def patch_case(name, integer):
    """patches [n][py][px] cut from the volume of skew_9x14x11 (integer voxels, rotated world-to-image).  integer: the patches are
    integers, the world-to-image matrix the identity at 1 mm and every patch an integer translation, so that every sample is a
    voxel (or outside: some patches hang over each face) and every sum is exact; else generic rigid matrices."""
    px, py, n = PATCH_SPECS[name]
    vol = volume("skew_9x14x11")
    vz, vy, vx = vol.shape
    rng = np.random.default_rng(px * 100 + py + int(integer))
    w2i = np.eye(4)
    ri2w, tm = np.tile(np.eye(4), (n, 1, 1)), np.tile(np.eye(4), (n, 1, 1))
    if integer:
        vdim = 1.0
        for k in range(n):
            ri2w[k, :3, 3] = (rng.integers(-3, vx - 2), rng.integers(-3, vy - 2), rng.integers(-1, vz))
            tm[k, :3, 3] = rng.integers(-2, 3, 3)
        patches = rng.integers(-1, 900, (n, py, px)).astype(np.float32)
    else:
        vdim = 1.3
        w2i = geometry("skew_9x14x11")[0].reshape(4, 4).astype(np.float64)
        for k in range(n):
            m = np.eye(4)
            m[:3, :3] = _rot(*rng.uniform(-0.5, 0.5, 3)) @ np.diag([1.2 * vdim * vx / px, 1.2 * vdim * vy / py, vdim])
            m[:3, 3] = m[:3, :3] @ (-(px - 1) / 2, -(py - 1) / 2, 0) + rng.uniform(-1, 1, 3) * vdim * (1, 1, 3)
            ri2w[k] = m
            tm[k, :3, :3] = _rot(*rng.uniform(-0.05, 0.05, 3))
            tm[k, :3, 3] = rng.uniform(-1, 1, 3)
        patches = rng.uniform(0, 900, (n, py, px)).astype(np.float32)
        patches[rng.uniform(size=patches.shape) < 0.15] = -1.0
    f = lambda a: np.ascontiguousarray(a, np.float32).reshape(-1, 16)
    return SimpleNamespace(name=name, px=px, py=py, n=n, vol=vol, vdim=vdim, w2i=f(w2i)[0], ri2w=f(ri2w), tm=f(tm), patches=patches,
                           vsize=(vx, vy, vz))


# ---- one patch-to-volume registration run on a non-square patch whose level-1 kernel has 13 taps (the second pass takes 14) ---------
PATCH_REG = dict(px=19, py=13, n=24, vdim=2.7, levels=2, steps=2, iterations=3)
# the share of patches the oracle leaves within 1e-4 of its own result when the volume's non-negative voxels are scaled by
# PERTURBATIONS (the smallest of the three, measured by tests/test_reg_ref.py), and the margin the device is given below it
# (measured: 14, 13 and 11 of 24 patches; the optimiser's steps of 4 and 2 mm / degrees at level 1 amplify a last bit, and on
# this small volume most patches drift by millimetres -- the 0.97 of the 32 x 32 case is out of the oracle's own reach here)
PATCH_REG_SHARE, PATCH_REG_MARGIN = 11 / 24, 1 / 24


@functools.lru_cache(maxsize=None)
def patch_reg_case():
    import reg_ref
    q = PATCH_REG
    px, py, n, vdim = q["px"], q["py"], q["n"], q["vdim"]
    vol = volume("red_4270")
    vz, vy, vx = vol.shape
    w2i = np.eye(4)
    w2i[:3, :3] /= vdim
    w2i[:3, 3] = ((vx - 1) / 2, (vy - 1) / 2, (vz - 1) / 2)
    rng = np.random.default_rng(1913)
    ri2w, T = np.tile(np.eye(4), (n, 1, 1)), np.tile(np.eye(4), (n, 1, 1))
    ys, xs = np.meshgrid(np.arange(py), np.arange(px), indexing="ij")
    patches = np.zeros((n, py, px), np.float32)
    f = lambda a: np.ascontiguousarray(a, np.float32).reshape(-1, 16)
    for k in range(n):
        m = np.eye(4)
        m[:3, :3] = _rot(*rng.uniform(-0.4, 0.4, 3)) @ np.diag([0.7 * vdim * vx / px, 0.7 * vdim * vy / py, vdim])
        m[:3, 3] = m[:3, :3] @ (-(px - 1) / 2, -(py - 1) / 2, 0) + rng.uniform(-1, 1, 3) * vdim * (2, 2, 2.5)
        ri2w[k] = m
        b = reg_ref.patch_samples(vol, f(w2i)[0], f(m)[0], xs, ys, np.zeros_like(xs))
        patches[k] = np.where(b < 0, -1.0, b)
        if k % 3 == 0:                                       # every third patch knocked off
            T[k, :3, :3] = _rot(*np.deg2rad(rng.uniform(-2, 2, 3)))
            T[k, :3, 3] = rng.uniform(-1.5, 1.5, 3)
    eye = f(np.tile(np.eye(4), (n, 1, 1)))
    return SimpleNamespace(px=px, py=py, n=n, vdim=vdim, vol=vol, vsize=(vx, vy, vz), w2i=f(w2i)[0], ri2w=f(ri2w), T=f(T), mo=eye, invmo=eye,
                           patches=patches, schedule=(q["levels"], q["steps"], q["iterations"]))


def oracle_patch_run(c, vol=None):
    from oracle import pyoracle as po
    lv, st, it = c.schedule
    return po.pvr_register_patches(c.patches, c.ri2w, c.mo, c.invmo, c.T, c.w2i, c.vol if vol is None else vol, c.vdim, levels=lv, steps=st,
                                   iterations=it)
