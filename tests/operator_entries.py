"""Inputs and comparisons that hold the PSF operator to the oracle ENTRY BY ENTRY (test infrastructure: numpy and the oracle only).

The operator is a sparse matrix A[pixel, voxel] whose entries are the taps the epsilon-skip keeps.  Fed with impulses, every output element
of the scatter (an impulse per pixel of a set) or of the gather (an impulse per voxel of a set) is ONE entry or the sum of TWO: a lone entry
has no summation order, and the float32 sum of two floats is the correctly rounded exact sum in either order -- what the oracle's double
accumulation rounded once gives too.  With factors that are powers of two the products round nothing, so every correct kernel path has to
return the oracle's bits, however it associates its products.

Two problems carry the sets: "tiny" (phantom.problem_tiny: 34^3 voxels, a spherical mask, axial / coronal / sagittal stacks of 32 x 32 slices)
and "ones24" (cell_limit_cases.base, two of its slices moved by a voxel or two: 24^3 voxels under a mask of ones, so that the volume's faces
are seen, and slices whose first and last rows and columns are active).  tests/test_operator_entries.py guards this file on the CPU; tests/test_operator_entries_gpu.py runs the
device against it."""
import copy
import functools
import itertools

import numpy as np

from tests import cell_limit_cases as C

PROBLEMS = ("tiny", "ones24")
RUNG_PROBLEMS = ("coarse",)                              # tests/tile_rungs.py: the tile kernels' box fallbacks (no test of PROBLEMS runs it)
CELL = dict(cell_w=16, cell_h=16, cell_band=6)           # the cells of tests/test_scatter_ring_gpu.py
U = 2.0 ** -24                                           # the unit round-off of float32

# the classes a problem's pixel sets have to hold between them (pixel_classes)
ORIENTATIONS = {"tiny": ("axial", "coronal", "sagittal-own-y", "sagittal-own-z"), "ones24": ("axial", "coronal"),
                "coarse": ("axial", "coronal", "sagittal-own-y", "sagittal-own-z")}
CELL_EDGES = ("cell-first-col", "cell-last-col", "cell-first-row", "cell-last-row")
REQUIRED = {"tiny": ORIENTATIONS["tiny"] + ("mask-surface", "literal-flip") + CELL_EDGES,
            "ones24": ORIENTATIONS["ones24"] + ("first-row", "last-row", "first-col", "last-col", "low-face", "high-face") + CELL_EDGES,
            "coarse": ORIENTATIONS["coarse"] + ("first-row", "last-row", "first-col", "last-col")}
VOXEL_REQUIRED = {"tiny": ("x-first", "x-last", "y-first", "y-last", "z-first", "z-last", "inside-surface", "outside-surface"),
                  "ones24": ("x-first", "x-last", "y-first", "y-last", "z-first", "z-last"),
                  "coarse": ("x-first", "x-last", "y-first", "y-last", "z-first", "z-last")}


def support(pvr):
    return 12 if pvr else 16


def first_tap(pvr):
    """the offset of a footprint's first tap from the centre voxel is -first_tap (psf_centre of oracle/svr_oracle.c)"""
    return (support(pvr) - 1) // 2


@functools.lru_cache(maxsize=None)
def problem(name):
    from fetalreconstruction_amd import phantom
    if name == "tiny":
        P = phantom.problem_tiny()
    elif name == "coarse":
        P = _coarse()
    else:
        # the first axial slice one voxel up the volume's y, the first coronal one two up its z: their first rows then lie ONE voxel short
        # of a whole footprint from the low face (5 and 4 voxels from it, they would fold three and four taps onto the face's voxels)
        P = C.moved(C.moved(C.base(), (0,), (0.0, 1.0, 0.0)), (3,), (0.0, 0.0, 2.0))
    for a in (P.slices, P.mask):
        a.setflags(write=False)
    return P


COARSE_LINE = 6                                          # the one live line of the coarse problem's last slice (a pixel coordinate)


def _coarse():
    """The problem of tests/tile_rungs.py: 96^3 voxels of 1 mm under a mask of ones and four slices of 14 x 14 pixels of 6.3 mm, every pixel
    live: axial, coronal (it owns the volume's y) and two sagittal ones, whose pixel axes both run across x -- a tile of 8 pixels spans 44
    planes of the owned axis.  Of the last slice ONE line of pixels along the owned axis is live, moved down that axis until the largest
    centre of its first eight pixels is 8: the slot kernel's box of that tile starts 43 planes below the volume (60 planes: a reject),
    back_tiled_kernel's saturated box keeps the 17 inside, which fit the smallest LDS."""
    from fetalreconstruction_amd import phantom
    P = phantom.make_problem(4, (14, 14, 1), 6.3, 6.3, None, 1.0, 45.0, seed=5, orientations=("ax", "cor", "sag", "sag"), motion_frac=0.0, name="coarse")
    P = C._own(P)
    P.mask[...] = 1.0
    P.slices = np.where(P.slices > 0, P.slices, np.float32(100.0)).astype(np.float32)
    sl = P.ns - 1
    axis = C.owned_axis(P, sl)
    c, xy = C.centres(P, sl)
    along = int(np.ptp(c[xy[:, 1] == 0, axis]) > np.ptp(c[xy[:, 0] == 0, axis]))      # 1: the owned axis runs along px, 0: along py
    line = xy[:, along] == COARSE_LINE
    P.slices[sl][tuple(xy[~line].T[::-1])] = -1.0
    first8 = line & (xy[:, 1 - along] < 8)
    t = np.zeros(3)
    t[axis] = 8.0 - float(c[first8, axis].max())
    return C.moved(P, (sl,), t)


def _pyoracle():
    from oracle import pyoracle
    pyoracle.build()
    return pyoracle


@functools.lru_cache(maxsize=None)
def _oracle(name, pvr, mode):
    return _pyoracle().OracleReconstruction(problem(name), mode, pvr=pvr)


def canon():
    return _pyoracle().CANON


def literal():
    return _pyoracle().LITERAL


# ---- one pixel's entries ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def taps(name, pvr, pixel, mode=None):
    """the kept taps of pixel (slice, px, py) from the oracle's tap_census -> (voxel [n] int64, value [n] float32, aliased, dropped):
    the taps that land inside the volume by the oracle's index rule (a negative coordinate becomes 0, one beyond the high end is dropped;
    vol_index / f2u_sat), mask or not; aliased / dropped say whether the rule touched any kept tap"""
    P = problem(name)
    sl, px, py = pixel
    n, bits, vals, c = _oracle(name, pvr, canon() if mode is None else mode).tap_census(sl, px, py, with_vals=True)
    b = np.flatnonzero(np.unpackbits(bits.view(np.uint8), bitorder="little"))
    assert len(b) == n
    ofs = np.stack([b & 15, (b >> 4) & 15, b >> 8], -1).astype(np.int64) - first_tap(pvr)
    v = ofs + c.astype(np.int64)
    neg = v < 0
    v = np.where(neg, 0, v)
    inside = (v < np.asarray(P.vsize, np.int64)).all(1)
    vx, vy, _ = P.vsize
    idx = (v[:, 0] + v[:, 1] * vx + v[:, 2] * vx * vy)[inside]
    val = vals[b][inside].copy()
    for a in (idx, val):
        a.setflags(write=False)
    return idx, val, bool(neg[inside].any()), bool((~inside).any())


def mask_taps(name, pvr, pixel, mode=None):
    """the taps of `taps` that land on mask voxels: what the scatters add and the gather reads"""
    idx, val, _, _ = taps(name, pvr, pixel, mode)
    m = problem(name).mask.reshape(-1)[idx] != 0
    return idx[m], val[m]


def terms_per_voxel(name, pvr, pixels):
    """how many terms each voxel receives from a scatter of the pixels' impulses, recounted from the oracle's tap lists"""
    n = np.zeros(problem(name).nvox, np.int64)
    for p in pixels:
        np.add.at(n, mask_taps(name, pvr, p)[0], 1)
    return n


# ---- the classes of a pixel ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pool(name):
    """every active pixel: [n][6] = slice, px, py, centre voxel x, y, z"""
    P = problem(name)
    rows = []
    for sl in range(P.ns):
        c, xy = C.centres(P, sl)
        rows.append(np.column_stack([np.full(len(c), sl), xy, c]))
    out = np.concatenate(rows).astype(np.int64)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _slice_classes(name):
    """per slice: (orientation class, owned axis)"""
    P = problem(name)
    out = []
    for sl in range(P.ns):
        A = (P.slice_w2i[sl].reshape(4, 4).astype(np.float64) @ P.slice_tinv[sl].reshape(4, 4).astype(np.float64)
             @ np.asarray(P.recon_i2w, np.float64).reshape(4, 4))
        normal = int(np.argmax(np.abs(A[2, :3])))                     # the volume axis closest to the slice normal
        own = C.owned_axis(P, sl)
        out.append((("sagittal-own-y" if own == 1 else "sagittal-own-z") if normal == 0 else "coronal" if normal == 1 else "axial", own))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _cell_layout(name, pvr):
    nc = first_tap(pvr)
    return C.layout(problem(name), CELL["cell_w"], CELL["cell_h"], nc=nc, nh=nc + 1)["classes"]


@functools.lru_cache(maxsize=None)
def literal_flip_pixels(name, pvr):
    """the pixels of tests/census.py's seed-0 sample of 300 whose LITERAL and CANONICAL walks keep different taps"""
    P = problem(name)
    act = np.argwhere(P.slices != -1)
    pick = act[np.random.default_rng(0).choice(len(act), min(300, len(act)), replace=False)]
    flips, _, _ = _oracle(name, pvr, canon()).flip_pixels(pick)
    return tuple((int(sl), int(px), int(py)) for (sl, py, px), f in zip(pick, flips) if f > 0)


def _cheap_classes(name, pvr, row):
    """the classes that follow from the pixel's place and centre alone"""
    P = problem(name)
    sl, px, py, cx, cy, cz = (int(v) for v in row)
    ns, sy, sx = P.slices.shape
    orient, own = _slice_classes(name)[sl]
    out = {orient}
    for on, what in ((py == 0, "first-row"), (py == sy - 1, "last-row"), (px == 0, "first-col"), (px == sx - 1, "last-col")):
        if on:
            out.add(what)
    q = _cell_layout(name, pvr)[0 if own == 1 else 1]["q"]
    if q is not None:
        cl = cz if own == 1 else cy
        col, lane = (cx - q[0]) % CELL["cell_w"], (cl - q[2]) % CELL["cell_h"]
        for on, what in ((col == 0, "cell-first-col"), (col == CELL["cell_w"] - 1, "cell-last-col"),
                         (lane == 0, "cell-first-row"), (lane == CELL["cell_h"] - 1, "cell-last-row")):
            if on:
                out.add(what)
    return out


def pixel_classes(name, pvr, pixel):
    """every class of REQUIRED that the pixel (slice, px, py) belongs to"""
    pool = _pool(name)
    row = pool[(pool[:, 0] == pixel[0]) & (pool[:, 1] == pixel[1]) & (pool[:, 2] == pixel[2])][0]
    out = _cheap_classes(name, pvr, row)
    idx, _, aliased, dropped = taps(name, pvr, pixel)
    on_mask = problem(name).mask.reshape(-1)[idx] != 0
    if aliased:
        out.add("low-face")
    if dropped:
        out.add("high-face")
    if on_mask.any() and not on_mask.all():
        out.add("mask-surface")
    if pixel in literal_flip_pixels(name, pvr):
        out.add("literal-flip")
    return frozenset(out)


# ---- impulse sets -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def impulse_pixel_sets(name, pvr, seed=0, first=()):
    """-> (sets, classes): a tuple of tuples of pixels (slice, px, py) and {pixel: its classes}.  A pixel joins a set only while no mask voxel
    would receive more than two terms, counted from the pixels' own kept taps (a pixel whose footprint the low faces fold onto itself more than
    twice joins none).  The pixels of `first` (tests/tile_rungs.py: one per rung of the tile kernels' ladder) and one pixel of every class of
    REQUIRED[name] are placed first, then the sets are filled from a seeded shuffle of the active pixels."""
    P = problem(name)
    pool = _pool(name)
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(pool))
    sets, counts, classes = [], [], {}

    def place(pixel, may_open):
        idx, _ = mask_taps(name, pvr, pixel)
        if not len(idx) or any(pixel in s for s in sets):
            return False
        own = np.bincount(idx, minlength=P.nvox)
        if own.max() > 2:
            return False
        for s, n in zip(sets, counts):
            if (n[idx] + own[idx]).max() <= 2:
                s.append(pixel)
                n += own
                break
        else:
            if not may_open:
                return False
            sets.append([pixel])
            counts.append(own)
        classes[pixel] = pixel_classes(name, pvr, pixel)
        return True

    def as_pixel(row):
        return (int(row[0]), int(row[1]), int(row[2]))

    for p in first:
        assert place(tuple(int(v) for v in p), True), p
    lo, hi = first_tap(pvr), first_tap(pvr) + 1
    v = np.asarray(P.vsize, np.int64)
    for want in REQUIRED[name]:
        if any(want in c for c in classes.values()):
            continue
        if want == "literal-flip":
            cand = iter(literal_flip_pixels(name, pvr))
        else:
            rows = pool[order]
            if want == "low-face":                                   # ONE coordinate folded onto 0, on one axis: two terms on the face's voxels
                below = rows[:, 3:] - lo
                rows = rows[((below < 0).sum(1) == 1) & ((below == -1).sum(1) == 1)]
            elif want == "high-face":
                rows = rows[((rows[:, 3:] + hi) > v - 1).any(1)]
            cheap = want not in ("low-face", "high-face", "mask-surface")
            cand = itertools.islice((as_pixel(r) for r in rows if not cheap or want in _cheap_classes(name, pvr, r)), 40)
        for p in cand:
            if want in pixel_classes(name, pvr, p) and place(p, True):
                break
    for r in pool[order][:120]:
        place(as_pixel(r), False)
    return tuple(tuple(s) for s in sets), classes


def voxel_classes(name, voxel):
    P = problem(name)
    vx, vy, vz = P.vsize
    x, y, z = voxel % vx, (voxel // vx) % vy, voxel // (vx * vy)
    out = set()
    for k, n, a in ((x, vx, "x"), (y, vy, "y"), (z, vz, "z")):
        if k == 0:
            out.add(a + "-first")
        if k == n - 1:
            out.add(a + "-last")
    m = P.mask != 0
    near = [m[zz, yy, xx] for xx, yy, zz in ((x - 1, y, z), (x + 1, y, z), (x, y - 1, z), (x, y + 1, z), (x, y, z - 1), (x, y, z + 1))
            if 0 <= xx < vx and 0 <= yy < vy and 0 <= zz < vz]
    if m[z, y, x] and not all(near):
        out.add("inside-surface")
    if not m[z, y, x] and any(near):
        out.add("outside-surface")
    return frozenset(out)


@functools.lru_cache(maxsize=None)
def impulse_voxel_sets(name, pvr):
    """-> (sets, classes): lattices of flat voxel indices with spacing 17 (13 patch-based: the support, and one more for the eight-voxel
    average the patch-based gather reads the volume through), so that a pixel's footprint holds at most one impulse.  The lattice is shifted
    from set to set: offset 0 holds voxel 0 of every axis, the offset that ends on v - 1 holds the last, one more is fixed, and two
    are searched for that put a voxel just inside and one just outside the mask's surface (a full gather of the oracle per set: few sets)."""
    P = problem(name)
    vx, vy, vz = P.vsize
    d = support(pvr) + 1
    last = tuple((n - 1) % d for n in (vx, vy, vz))

    def lattice(o):
        g = np.meshgrid(*[np.arange(o[k], n, d) for k, n in enumerate((vx, vy, vz))], indexing="ij")
        return tuple(int(i) for i in (g[0] + g[1] * vx + g[2] * vx * vy).reshape(-1))

    offsets = [(0, 0, 0), last, (5, 11, 8)]
    for want in [w for w in VOXEL_REQUIRED[name] if w.endswith("surface")]:
        for o in np.ndindex(d, d, d):
            if any(want in voxel_classes(name, i) for i in lattice(o)):
                offsets.append(o)
                break
    sets = tuple(dict.fromkeys(lattice(o) for o in offsets))
    return sets, {i: voxel_classes(name, i) for s in sets for i in s}


# ---- what the oracle says -------------------------------------------------------------------------------------------------------
def padded(name, keep, value=None):
    """a copy of the problem in which every pixel outside `keep` ([ns][sy][sx] bool) is padding (-1); value: what the kept pixels hold"""
    P = problem(name)
    Q = copy.copy(P)
    Q.slices = np.where(keep, P.slices if value is None else np.float32(value), np.float32(-1.0)).astype(np.float32)
    return Q


def indicator(name, pixels):
    on = np.zeros(problem(name).slices.shape, bool)
    for sl, px, py in pixels:
        on[sl, py, px] = True
    return on


def _frozen(*arrays):
    out = tuple(np.array(a) for a in arrays)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected_scatter(name, pvr, pixels, slice_value=3.0, mode=None):
    """-> (addon, cmap): the oracle's scatter of unit weights at `pixels` with psf_sums 1, simslices 1, slices = slice_value (e = slice_value
    - 1), slice weights and scales 1, on a copy of the problem where every other pixel is padding.  A padding pixel adds nothing and a pixel of
    weight 0 adds exact zeros, so this is the full problem's result too (tests/test_operator_entries.py holds one set to that)."""
    po = _pyoracle()
    on = indicator(name, pixels)
    Q = padded(name, on, slice_value)
    orc = po.OracleReconstruction(Q, po.CANON if mode is None else mode, pvr=pvr)
    for a in (orc.psf_sums, orc.weights, orc.simslices):
        a[...] = on
    orc.SuperresolutionBackproject(np.ones(Q.ns, np.float32))
    return _frozen(orc.addon, orc.cmap)


def contributing(name, pvr, voxels):
    """[ns][sy][sx] bool: the pixels whose footprint box (folded at the low faces, one voxel wider each way for the patch-based average)
    holds a voxel of the set -- every other pixel gathers exact zeros from it"""
    P = problem(name)
    pool = _pool(name)
    vx, vy, _ = P.vsize
    v = np.asarray(voxels, np.int64)
    xyz = np.stack([v % vx, (v // vx) % vy, v // (vx * vy)], -1)
    lo = np.maximum(pool[:, 3:] - first_tap(pvr), 0) - 1
    hi = np.maximum(pool[:, 3:] + first_tap(pvr) + 1, 0) + 1
    hit = ((xyz[None] >= lo[:, None]) & (xyz[None] <= hi[:, None])).all(2).any(1)
    on = np.zeros(P.slices.shape, bool)
    on[pool[hit, 0], pool[hit, 2], pool[hit, 1]] = True
    return on


def impulse_volume(name, voxels, value=4.0):
    V = np.zeros(problem(name).nvox, np.float32)
    V[list(voxels)] = value
    return V


@functools.lru_cache(maxsize=None)
def expected_gather(name, pvr, voxels, mode=None):
    """-> (simslices, simweights, siminside, contributing): the oracle's gather of a volume that holds 4.0 at `voxels` with psf_sums 1, on a copy
    of the problem where every pixel that cannot reach a voxel of the set is padding; simweights / siminside are filled at the contributing
    pixels only (gather_weights has every pixel's)"""
    po = _pyoracle()
    on = contributing(name, pvr, voxels)
    orc = po.OracleReconstruction(padded(name, on), po.CANON if mode is None else mode, pvr=pvr)
    orc.psf_sums[...] = on
    orc.recon[...] = impulse_volume(name, voxels)
    orc.SimulateSlices()
    return _frozen(orc.simslices, orc.simweights, orc.siminside, on)


@functools.lru_cache(maxsize=None)
def gather_weights(name, pvr):
    """-> (simweights, siminside) of every active pixel with psf_sums 1: they do not depend on the volume (one full pass of the oracle)"""
    po = _pyoracle()
    P = problem(name)
    orc = po.OracleReconstruction(P, po.CANON, pvr=pvr)
    orc.psf_sums[...] = P.slices != -1
    orc.SimulateSlices()
    return _frozen(orc.simweights, orc.siminside)


@functools.lru_cache(maxsize=None)
def expected_gauss(name, pvr, pixels, mode=None):
    """-> (psf_sums, volw, recon, voxcount): the oracle's GaussianReconstructionLocal (passes 1 and 2, no equalisation) on a copy of the
    problem where the set's pixels hold 512.0 and every other pixel is padding"""
    po = _pyoracle()
    Q = padded(name, indicator(name, pixels), 512.0)
    orc = po.OracleReconstruction(Q, po.CANON if mode is None else mode, pvr=pvr)
    ones = np.ones(Q.ns, np.float32)
    orc.UpdateScaleVector(ones, ones)
    orc.GaussianReconstructionLocal()
    return _frozen(orc.psf_sums, orc.volw, orc.recon, orc.voxcount)


def gauss_from_taps(name, pvr, pixels, psf_sums):
    """-> float64 [voxels]: sum over the set's pixels of (tap / the pixel's psf_sums) at the mask voxels, from the oracle's tap lists, exact to
    float64: what pass 2 leaves in the volume weights, given the psf_sums of pass 1 (the device's own: its pass 1 is checked apart).  A pixel
    that pass 1 dropped (psf_sums 0) adds nothing."""
    out = np.zeros(problem(name).nvox, np.float64)
    for sl, px, py in pixels:
        s = float(psf_sums[sl, py, px])
        if s != 0:
            idx, val = mask_taps(name, pvr, (sl, px, py))
            np.add.at(out, idx, val.astype(np.float64) / s)
    return out


# ---- dense passes: a bound per element ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def terms_bound(name, pvr):
    """n_v [voxels]: the number of active pixels whose footprint box (folded at the low faces) holds the voxel -- an upper bound on the
    terms a scatter adds there, counted from cell_limit_cases.centres"""
    P = problem(name)
    pool = _pool(name)
    vx, vy, vz = P.vsize
    size = np.array([vx, vy, vz])
    lo = np.clip(pool[:, 3:] - first_tap(pvr), 0, size)
    hi = np.clip(np.maximum(pool[:, 3:] + first_tap(pvr) + 1, 0) + 1, 0, size)     # exclusive
    d = np.zeros((vz + 1, vy + 1, vx + 1), np.int64)
    for sx_, x in ((1, lo[:, 0]), (-1, hi[:, 0])):
        for sy_, y in ((1, lo[:, 1]), (-1, hi[:, 1])):
            for sz_, z in ((1, lo[:, 2]), (-1, hi[:, 2])):
                np.add.at(d, (z, y, x), sx_ * sy_ * sz_)
    n = d.cumsum(0).cumsum(1).cumsum(2)[:vz, :vy, :vx].reshape(-1)
    n.setflags(write=False)
    return n


@functools.lru_cache(maxsize=None)
def terms_folded(name, pvr):
    """n_v [voxels]: every tap of every active pixel's footprint counted at the voxel the index rule sends it to (a negative coordinate to 0,
    one beyond the high end nowhere) -- an upper bound on the terms of a scatter like terms_bound, and still one where a slice hangs far
    below a low face and folds a whole row of taps onto one voxel (terms_bound counts such a pixel once)"""
    P = problem(name)
    vx, vy, vz = P.vsize
    n = np.zeros((vz, vy, vx), np.int64)
    ofs = np.arange(-first_tap(pvr), first_tap(pvr) + 2)
    for row in _pool(name):
        m = []
        for c, size in zip(row[3:], (vx, vy, vz)):
            v = np.maximum(c + ofs, 0)
            m.append(np.bincount(v[v < size], minlength=size))
        (x0, x1), (y0, y1), (z0, z1) = ((np.flatnonzero(k)[[0, -1]] if k.any() else (0, -1)) for k in m)
        n[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1] += m[2][z0:z1 + 1, None, None] * m[1][None, y0:y1 + 1, None] * m[0][None, None, x0:x1 + 1]
    n = n.reshape(-1)
    n.setflags(write=False)
    return n


def fold_terms(name, pvr):
    """[ns][sy][sx] int: the most taps of the pixel's footprint that the index rule sends to ONE voxel (1 where no coordinate is negative)"""
    P = problem(name)
    out = np.ones(P.slices.shape, np.int64)
    pool = _pool(name)
    lo = pool[:, 3:] - first_tap(pvr)
    out[pool[:, 0], pool[:, 2], pool[:, 1]] = np.clip(1 - lo, 1, support(pvr)).prod(1)
    return out


def dense_inputs(name):
    """the scatter's inputs of a dense pass: cell_limit_cases.em_inputs (random weights with a fifth of them zero, simulated slices around the
    slices, slice weights with one zero)"""
    return C.em_inputs(problem(name))


@functools.lru_cache(maxsize=None)
def expected_dense(name, pvr):
    """The oracle's sequence on the full problem -> dict: psf_sums, volw, recon (passes 1 and 2, not equalised), voxcount; simslices,
    simweights, siminside of the equalised volume `volume`; cmap, addon of dense_inputs with the oracle's psf_sums, and addon_abs = the
    same scatter with every residual replaced by its magnitude: the sum of the magnitudes of addon's terms."""
    po = _pyoracle()
    P = problem(name)
    orc = po.OracleReconstruction(P, po.CANON, pvr=pvr)
    ones = np.ones(P.ns, np.float32)
    orc.UpdateScaleVector(ones, ones)
    orc.InitializeEMValues()
    orc.GaussianReconstructionLocal()
    out = dict(psf_sums=orc.psf_sums, volw=orc.volw, recon=orc.recon, voxcount=orc.voxcount)
    out = {k: np.array(v) for k, v in out.items()}
    orc.GaussianReconstructionFinish()
    out["volume"] = np.array(orc.recon)
    orc.SimulateSlices()
    out.update(simslices=np.array(orc.simslices), simweights=np.array(orc.simweights), siminside=np.array(orc.siminside))
    w, ss, sw = dense_inputs(name)
    orc.weights[...] = w
    orc.simslices[...] = ss
    orc.SuperresolutionBackproject(sw)
    out.update(cmap=np.array(orc.cmap), addon=np.array(orc.addon))
    # e = slice - simslice where simslice > 0, else 0 (scales 1): slices' = simslice + |e| gives |e| up to one rounding of the sum, which
    # the factor (1 + 2^-22) on the result covers
    e = np.where(ss > 0, np.abs(orc.slices.astype(np.float64) - ss), 0.0)
    orc.slices[...] = np.where(orc.slices != -1, (ss + e).astype(np.float32), np.float32(-1.0))
    orc.SuperresolutionBackproject(sw)
    out["addon_abs"] = np.array(orc.addon).astype(np.float64) * (1 + 2.0 ** -22)
    for v in out.values():
        v.setflags(write=False)
    return out


def warm(name, pvr):
    """the expectations that take a pass of the oracle over most pixels (seconds each), side by side: the oracle runs outside the interpreter's lock"""
    from concurrent.futures import ThreadPoolExecutor
    _pyoracle()
    problem(name)
    jobs = [lambda v=v: expected_gather(name, pvr, v) for v in impulse_voxel_sets(name, pvr)[0]]
    jobs += [lambda: gather_weights(name, pvr), lambda: expected_dense(name, pvr)]
    with ThreadPoolExecutor(max_workers=8) as pool:
        for f in [pool.submit(j) for j in jobs]:
            f.result()


# ---- comparisons: the offending elements, not a verdict -------------------------------------------------------------------------
def same_bits(got, want):
    """-> the flat indices where two float32 arrays differ in any bit"""
    g = np.ascontiguousarray(got, np.float32).reshape(-1).view(np.uint32)
    w = np.ascontiguousarray(want, np.float32).reshape(-1).view(np.uint32)
    assert g.shape == w.shape
    return np.flatnonzero(g != w)


def within_relative(got, want, k):
    """-> the flat indices where |got - want| <= k 2^-24 |want| does NOT hold, in float64, element by element (so want is 0 exactly where got
    is 0, and a NaN offends)"""
    g = np.asarray(got, np.float64).reshape(-1)
    w = np.asarray(want, np.float64).reshape(-1)
    assert g.shape == w.shape
    with np.errstate(invalid="ignore"):
        return np.flatnonzero(~(np.abs(g - w) <= k * U * np.abs(w)))


def within_terms(got, want, n, magnitude=None):
    """-> the flat indices where |got - want| <= (n + 6) 2^-24 S does NOT hold: n = an upper bound on the terms of each element, S = the sum
    of their magnitudes (`want` itself where no term is negative).  Recursive summation of n terms in any order, atomics included, loses at
    most (n - 1) u sum|terms|; the product orders of the device and the oracle differ by at most 6 roundings per term."""
    g = np.asarray(got, np.float64).reshape(-1)
    w = np.asarray(want, np.float64).reshape(-1)
    s = np.abs(w) if magnitude is None else np.asarray(magnitude, np.float64).reshape(-1)
    n = np.broadcast_to(np.asarray(n, np.float64).reshape(-1) if np.ndim(n) else np.float64(n), g.shape)
    with np.errstate(invalid="ignore"):
        return np.flatnonzero(~(np.abs(g - w) <= (n + 6) * U * s))


def describe(bad, got, want, limit=5):
    """a few offending elements for an assertion message"""
    g, w = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    return f"{len(bad)} of {g.size}: " + ", ".join(f"[{i}] {g[i]!r} != {w[i]!r}" for i in bad[:limit])
