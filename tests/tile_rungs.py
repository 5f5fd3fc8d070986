"""The fit rules of the tile kernels (csrc/svr_tile.inc) and of launch_scatter's ladder (csrc/svr_hip.hip), restated from their text: which
slice tile ends on which rung, counted on the CPU from the centre voxels (cell_limit_cases.centres).  numpy only, no device.

The ladder of a scatter over slice tiles (level 4: back_mode 4, and every patch-based scatter on tiles):
  "wave"      back_wave_kernel with a box of min(wave_cap, tile_cap) voxels.  It rejects a tile iff
              Dz > 64 or 4 * PP > cap or tw * th > WAVE_MAXPIX (32 evaluating, 64 with the coefficient table)
  "large"     with the table and a first box under 3696: back_wave_kernel once more with min(3696, tile_cap)
  "slot"      back_slot_kernel<8> with tile_cap.  It rejects iff Dz > SLOT_MAXP = 48 or vox > cap, vox = PL * Dy per plane that takes a live unit
              + PD * Dy per plane that takes dead units only.  Which unit is dead (unit_is_dead) is not restated here: vox lies between every used
              plane at the narrow pitch PD and every used plane at PL, a tile whose verdict the two bounds do not share is "slot?" (undecided);
              the patch-based kernel has no dead units, its vox is exact
  "last-lds"  back_tiled_kernel, the box in the LDS: the SATURATED box, Px = Dx | 1, Pxy = ((Px * Dy + 15) & ~31) + 16, Pxy * Dz <= tile_cap
  "last-mem"  back_tiled_kernel's direct-atomic branch (in_lds false)
  "last-pvr"  pvr_tiles_kernel (patch-based: MODE_BACK, or MODE_GAUSS2 in pass 2 of the Gaussian reconstruction)
  "out"       every kernel returns at once: lox > vx - 1 or Dy <= 0 or Dz <= 0
The wave and slot kernels share one box: per slice the owned axis z' (SliceConst::own) and the lane axis y', lo = min centre - NC unsaturated, hi = max
centre + NH capped at the volume's last plane on y' and z' (not on x), PL = (hix - lox + 1) | 1, PP = PL * Dy, PD = (max cx - min cx + 1) | 1.
The gather (fwd_unit_kernel, every instantiation): the box on the volume's own axes with the same lo / hi, Px = Dx | 1, Pxy = Px * Dy made odd, in the LDS
iff Pxy * Dz <= min(fwd_unit_cap, tile_cap), else every tap from memory.

tests/test_tile_rungs.py holds this file to hand-computed boxes and checks that every case below puts a tile, and an impulse, on every rung it is meant
to reach, for both sizes tile_cap can take; tests/test_tile_rungs_gpu.py runs the cases."""
import functools

import numpy as np

from tests import cell_limit_cases as C
from tests import operator_entries as O

SLOT_MAXP, LARGE_BOX = 48, 3696
WAVE_CAP, FWD_UNIT_CAP = 2096, 9300                      # the defaults of svr_ctx
TILE_CAPS = (6016, 18304)                                # svr_create: (64 KiB or 160 KiB of LDS - 1 KiB - 16 KiB of static LDS) / 8 bytes
RUNGS = ("wave", "large", "slot", "slot?", "last-lds", "last-mem", "last-pvr", "out")


def taps(pvr):
    ns = O.support(pvr)
    nc = (ns - 1) // 2
    return ns, nc, ns - 1 - nc


# ---- the boxes of one tile ------------------------------------------------------------------------------------------------------
def plane_box(c, own, vsize, pvr):
    """the box of back_wave_kernel and back_slot_kernel for the centres c [n][3] of a tile's active pixels -> dict, or None where they return at once"""
    ns, nc, nh = taps(pvr)
    vx, vy, vz = vsize
    cx = c[:, 0]
    cl, cz = (c[:, 2], c[:, 1]) if own == 1 else (c[:, 1], c[:, 2])
    vgl, vgz = (vz, vy) if own == 1 else (vy, vz)
    lox, hix = int(cx.min()) - nc, int(cx.max()) + nh
    loy, hiy = int(cl.min()) - nc, min(int(cl.max()) + nh, vgl - 1)
    loz, hiz = int(cz.min()) - nc, min(int(cz.max()) + nh, vgz - 1)
    dy, dz = hiy - loy + 1, hiz - loz + 1
    if lox > vx - 1 or dy <= 0 or dz <= 0:
        return None
    planes = loz + np.arange(min(dz, SLOT_MAXP))
    u = planes[:, None] - cz[None, :] + nc
    used = int(((u >= 0) & (u < ns)).any(1).sum())
    pl, pd = (hix - lox + 1) | 1, (int(cx.max()) - int(cx.min()) + 1) | 1
    return dict(Dy=dy, Dz=dz, PL=pl, PD=pd, PP=pl * dy, used=used)


def wave_rejects(b, cap, tile_pixels, table):
    return b["Dz"] > 64 or 4 * b["PP"] > cap or tile_pixels > (64 if table else 32)


def slot_verdict(b, cap, pvr):
    """-> "fit" | "reject" | "undecided" """
    if b["Dz"] > SLOT_MAXP:
        return "reject"
    hi = b["used"] * b["PL"] * b["Dy"]
    lo = hi if pvr else b["used"] * b["PD"] * b["Dy"]
    return "fit" if hi <= cap else "reject" if lo > cap else "undecided"


def tiled_box(c, vsize):
    """back_tiled_kernel (support 16): -> (Pxy, Dz) of the saturated box, or None"""
    d = []
    for k, size in enumerate(vsize):
        lo, hi = max(int(c[:, k].min()) - 7, 0), min(max(int(c[:, k].max()) + 8, 0), size - 1)
        d.append(hi - lo + 1)
    if min(d) <= 0:
        return None
    px = d[0] | 1
    return ((px * d[1] + 15) & ~31) + 16, d[2]


def unit_box(c, vsize, pvr):
    """fwd_unit_kernel: -> Pxy * Dz, or None where the kernel returns at once"""
    _, nc, nh = taps(pvr)
    vx, vy, vz = vsize
    lo, hi = c.min(0).astype(int) - nc, c.max(0).astype(int) + nh
    dx, dy, dz = hi[0] - lo[0] + 1, min(hi[1], vy - 1) - lo[1] + 1, min(hi[2], vz - 1) - lo[2] + 1
    if lo[0] > vx - 1 or dy <= 0 or dz <= 0:
        return None
    px = dx | 1
    return ((px * dy) | 1) * dz


def rung(c, own, vsize, pvr, tile_pixels, wave_cap, tile_cap, table):
    """the rung a tile with the active centres c ends on"""
    b = plane_box(c, own, vsize, pvr)
    if b is None:
        return "out"
    cap1 = min(wave_cap, tile_cap)
    if not wave_rejects(b, cap1, tile_pixels, table):
        return "wave"
    if table and cap1 < LARGE_BOX and not wave_rejects(b, min(LARGE_BOX, tile_cap), tile_pixels, table):
        return "large"
    v = slot_verdict(b, tile_cap, pvr)
    if v == "fit":
        return "slot"
    if v == "undecided":
        return "slot?"
    if pvr:
        return "last-pvr"
    t = tiled_box(c, vsize)
    return "out" if t is None else "last-lds" if t[0] * t[1] <= tile_cap else "last-mem"


# ---- a problem's tiles ------------------------------------------------------------------------------------------------------------
def tiles(P, tw, th, active=None):
    """-> [(slice, own, centres [n][3], pixels [n][2] = (px, py))] for every tw x th tile with an active pixel (slices != -1, and `active`
    [ns][sy][sx] bool where given: the pixels that pass pixel_active)"""
    out = []
    for sl in range(P.ns):
        c, xy = C.centres(P, sl)
        if active is not None:
            keep = active[sl, xy[:, 1], xy[:, 0]]
            c, xy = c[keep], xy[keep]
        if not len(c):
            continue
        own = C.owned_axis(P, sl)
        key = (xy[:, 1] // th) * 4096 + xy[:, 0] // tw
        for k in np.unique(key):
            out.append((sl, own, c[key == k], xy[key == k]))
    return out


def census(problem, pvr, tile, caps, table=False, active=None):
    """problem: a name of operator_entries or a Problem; tile = (tw, th); caps = dict(wave_cap, tile_cap) ->
    dict(tiles = {rung: count}, pixels = {rung: frozenset of (slice, px, py)}, rerun = tiles that leave the wave kernel(s) for the slot kernel
    (exact), fallback = (lo, hi) tiles the slot kernel rejects: an interval where tiles are undecided)"""
    P = O.problem(problem) if isinstance(problem, str) else problem
    tw, th = tile
    n = {r: 0 for r in RUNGS}
    px = {r: set() for r in RUNGS}
    for sl, own, c, xy in tiles(P, tw, th, active):
        r = rung(c, own, P.vsize, pvr, tw * th, caps.get("wave_cap", WAVE_CAP), caps["tile_cap"], table)
        n[r] += 1
        px[r].update((sl, int(x), int(y)) for x, y in xy)
    last = n["last-lds"] + n["last-mem"] + n["last-pvr"]
    return dict(tiles=n, pixels={r: frozenset(v) for r, v in px.items()}, rerun=n["slot"] + n["slot?"] + last,
                fallback=(last, last + n["slot?"]))


def if_rejected(problem, pvr, tile, tile_cap, pixels):
    """{"last-lds" | "last-mem" | "last-pvr": tiles}: where the undecided tiles that hold `pixels` (census()["pixels"]["slot?"]) end if the slot kernel
    rejects them"""
    P = O.problem(problem) if isinstance(problem, str) else problem
    out = {}
    for sl, own, c, xy in tiles(P, *tile):
        if (sl, int(xy[0, 0]), int(xy[0, 1])) in pixels:
            t = tiled_box(c, P.vsize)
            r = "last-pvr" if pvr else "last-lds" if t[0] * t[1] <= tile_cap else "last-mem"
            out[r] = out.get(r, 0) + 1
    return out


def gather_census(problem, pvr, tile, cap, active=None):
    """-> dict(tiles = {"lds", "mem", "out": count}, pixels = {...: frozenset}) for fwd_unit_kernel with the box `cap` = min(fwd_unit_cap, tile_cap)"""
    P = O.problem(problem) if isinstance(problem, str) else problem
    n = dict(lds=0, mem=0, out=0)
    px = dict(lds=set(), mem=set(), out=set())
    for sl, own, c, xy in tiles(P, tile[0], tile[1], active):
        v = unit_box(c, P.vsize, pvr)
        r = "out" if v is None else "lds" if v <= cap else "mem"
        n[r] += 1
        px[r].update((sl, int(x), int(y)) for x, y in xy)
    return dict(tiles=n, pixels={r: frozenset(v) for r, v in px.items()})


# ---- the cases --------------------------------------------------------------------------------------------------------------------
# id -> (problem, patch-based, scatter tile, wave_cap or None (the default), with the table, {tile_cap: the rungs the case is meant to reach})
def _both(*rungs):
    return {cap: rungs for cap in TILE_CAPS}


SCATTER_CASES = {
    # case one: the two problems of operator_entries, by options alone
    "tiny-16-wave1024": ("tiny", False, (6, 4), 1024, False, _both("slot")),
    "ones24-16-wave1024": ("ones24", False, (6, 4), 1024, False, _both("slot")),
    "tiny-16-8x8": ("tiny", False, (8, 8), None, False, _both("slot")),
    "ones24-16-8x8": ("ones24", False, (8, 8), None, False, _both("slot")),
    "tiny-12-8x8": ("tiny", True, (8, 8), None, False, _both("slot")),
    "ones24-12-8x8": ("ones24", True, (8, 8), None, False, _both("slot")),
    "tiny-16-wave1024-table": ("tiny", False, (6, 4), 1024, True, _both("large")),
    "ones24-16-wave1024-table": ("ones24", False, (6, 4), 1024, True, _both("large")),
    "tiny-16-8x8-table": ("tiny", False, (8, 8), None, True, _both("large")),
    "ones24-16-8x8-table": ("ones24", False, (8, 8), None, True, _both("large")),
    # case two: coarse slices over a fine volume
    "coarse-16-2x2": ("coarse", False, (2, 2), None, False, {6016: ("wave",), 18304: ("wave", "slot")}),
    "coarse-16-2x2-wave1024": ("coarse", False, (2, 2), 1024, False, _both("slot")),          # (the last slice's line: 2 pixels a tile, a sure fit)
    "coarse-16-2x2-table": ("coarse", False, (2, 2), None, True, _both("wave", "large")),
    "coarse-16-4x4": ("coarse", False, (4, 4), None, False, {6016: ("last-mem",), 18304: ("slot",)}),
    "coarse-16-4x4-table": ("coarse", False, (4, 4), None, True, _both("wave", "large")),
    "coarse-16-8x8": ("coarse", False, (8, 8), None, False, _both("last-lds", "last-mem")),
    "coarse-16-8x8-table": ("coarse", False, (8, 8), None, True, _both("wave", "large", "last-mem")),   # (rung 1 takes the line's 60 planes: 64 pixels are allowed)
    "coarse-12-2x2": ("coarse", True, (2, 2), None, False, _both("wave")),
    "coarse-12-2x2-wave1024": ("coarse", True, (2, 2), 1024, False, _both("slot")),
    "coarse-12-4x4": ("coarse", True, (4, 4), None, False, {6016: ("last-pvr",), 18304: ("slot",)}),
    "coarse-12-8x8": ("coarse", True, (8, 8), None, False, _both("last-pvr")),
}
# pass 2 of the Gaussian reconstruction down the ladder: scatter case -> {tile_cap: the rungs its sets reach between them} (a set's pixels are the
# only live ones there, so a tile's box is that of one or two pixels, or of a pair of gauss_pairs)
GAUSS_CASES = {
    "tiny-16-wave1024": _both("slot"), "ones24-16-wave1024": _both("slot"), "tiny-16-8x8": _both("slot"), "tiny-12-8x8": _both("slot"),
    "tiny-16-wave1024-table": _both("large"), "ones24-16-wave1024-table": _both("large"),
    "coarse-16-8x8": {6016: ("slot", "last-mem"), 18304: ("slot", "last-lds", "last-mem")},
    "coarse-12-8x8": _both("slot", "last-pvr"),
}
GATHER_CAP = 2048                                        # fwd_unit_cap of the memory-read cases (svr_set_option's floor)
GATHER_TILE = (6, 5)
# id -> (problem, patch-based, fwd_unit_cap or None, the kind of gather, the arms the case is meant to reach)
GATHER_CASES = {}
for _name in ("tiny", "ones24"):
    GATHER_CASES[f"{_name}-16-evaluated"] = (_name, False, GATHER_CAP, "evaluated", ("mem",))
    GATHER_CASES[f"{_name}-16-table"] = (_name, False, GATHER_CAP, "table", ("mem",))
    GATHER_CASES[f"{_name}-12-evaluated"] = (_name, True, GATHER_CAP, "evaluated", ("mem",))
GATHER_CASES["coarse-16-evaluated"] = ("coarse", False, None, "evaluated", ("lds", "mem"))
GATHER_CASES["coarse-12-evaluated"] = ("coarse", True, None, "evaluated", ("lds", "mem"))


def scatter_options(case):
    """the options of a scatter case, in the order they are set"""
    name, pvr, tile, wave_cap, table, _ = SCATTER_CASES[case]
    opt = [("coeff_table", 1 if table else 0)]
    if table and not pvr:
        opt.append(("coeff_lazy", 0))
    opt += [("back_mode", 4), ("tile_w", tile[0]), ("tile_h", tile[1])]
    if wave_cap is not None:
        opt.append(("wave_cap", wave_cap))
    return tuple(opt)


def scatter_census(case, tile_cap, active=None):
    name, pvr, tile, wave_cap, table, _ = SCATTER_CASES[case]
    return census(name, pvr, tile, dict(wave_cap=WAVE_CAP if wave_cap is None else wave_cap, tile_cap=tile_cap), table, active)


def gather_case_census(case, tile_cap, gauss1=False):
    """the gather's tiles are GATHER_TILE; pass 1 of the Gaussian reconstruction keeps 4-pixel-wide tiles where the gather's are 6 wide"""
    name, pvr, cap, _, _ = GATHER_CASES[case]
    tile = (4, GATHER_TILE[1]) if gauss1 else GATHER_TILE
    return gather_census(name, pvr, tile, min(FWD_UNIT_CAP if cap is None else cap, tile_cap))


# ---- the impulse sets: a pixel in a tile of every rung -------------------------------------------------------------------------------
def _alone(name, pvr, pixel):
    idx, _ = O.mask_taps(name, pvr, pixel)
    return len(idx) > 0 and np.bincount(idx).max() <= 2


@functools.lru_cache(maxsize=None)
def rung_pixels(name, pvr):
    """pixels to place first in operator_entries.impulse_pixel_sets: for every scatter case of (name, pvr), every tile_cap and every rung it is
    meant to reach, one pixel of a tile on that rung, unless a pixel picked before or one of the problem's own sets lies in one already"""
    have = {p for s in O.impulse_pixel_sets(name, pvr)[0] for p in s}
    first = []
    for case, (n, v, _, _, _, reach) in SCATTER_CASES.items():
        if (n, v) != (name, pvr):
            continue
        for cap, rungs in reach.items():
            cen = scatter_census(case, cap)
            for r in rungs:
                if cen["pixels"][r] & (have | set(first)):
                    continue
                pick = next((p for p in sorted(cen["pixels"][r]) if _alone(name, pvr, p)), None)
                assert pick is not None, (case, cap, r)
                first.append(pick)
    return tuple(first)


def pixel_sets(name, pvr):
    """the impulse sets of the rung tests -> (sets, classes) as operator_entries.impulse_pixel_sets"""
    return O.impulse_pixel_sets(name, pvr, first=rung_pixels(name, pvr))


@functools.lru_cache(maxsize=None)
def gauss_pairs(name, pvr):
    """Pass 2 of the Gaussian reconstruction runs on a copy of the problem where only the set's pixels are live, so a tile's box spans the SET's
    pixels.  Of one 8 x 8 tile of the coarse problem's first sagittal slice: two opposite corners (60 planes of the owned axis: a slot reject; the
    saturated box overflows every LDS), and the two ends of the edge that runs along the owned axis (a slot reject; 17 x 16 x 60 voxels fit the larger
    LDS).  (The last slice's line below the low face cannot serve here: its low pixels fold sixteen taps onto one voxel.) -> tuple of sets"""
    if name != "coarse":
        return ()
    P = O.problem(name)
    sl = 2
    c, xy = C.centres(P, sl)
    axis = C.owned_axis(P, sl)
    at = {(int(x), int(y)): int(k[axis]) for k, (x, y) in zip(c, xy)}
    edge = (7, 0) if abs(at[7, 0] - at[0, 0]) > abs(at[0, 7] - at[0, 0]) else (0, 7)
    return (((sl, 0, 0), (sl, 7, 7)), ((sl, 0, 0), (sl,) + edge))


def gauss_sets(name, pvr):
    return pixel_sets(name, pvr)[0] + gauss_pairs(name, pvr)
