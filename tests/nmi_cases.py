"""The cases that take the device NMI (csrc/svr_nmi.inc, k_nmi / svr_nmi_evaluate) to where its schedule splits, merges and regrows, and
the schedule itself restated.  numpy only: tests/test_nmi_cases.py proves without a GPU that every case reaches its edge (from this
restatement and the numpy reference of tests/test_nmi_registration.py), tests/test_nmi_limits_gpu.py then only compares the device with
that reference, exactly.

The schedule, from svr_nmi_evaluate:
  per_block = max(1, 16384 // (tx * ty))         planes one workgroup takes
  chunks(e) = ceil(planes(e) / per_block)        workgroups of evaluation e
  an evaluation takes a merge slot iff it has more than one chunk; slots are numbered in evaluation order
  cap       = max(64, slots * 3 // 2)            slots laid out (and zeroed once) when a call needs more than there are
  terms     = max(max_count + 1, 2 * previous)   entries of the c log c table when previous <= max_count,
                                                 max_count = max_e planes(e) * tx * ty
"""
import functools
import math

import numpy as np

BINS = 64
BLOCK_PIXELS = 16384


# ---- the schedule ---------------------------------------------------------------------------------------------------------------
def per_block(tx, ty):
    return max(1, BLOCK_PIXELS // (tx * ty))


def chunks(planes, tx, ty):
    return -(-int(planes) // per_block(tx, ty))


class Tables:
    """a context's grow-only merge slots and term table, as one svr_nmi_evaluate after another leaves them"""

    def __init__(self):
        self.slots, self.terms = 0, 0

    def call(self, ppe, tx, ty):
        ch = [chunks(p, tx, ty) for p in ppe]
        need = sum(c > 1 for c in ch)
        max_count = max(int(p) * tx * ty for p in ppe)
        slots_before, terms_before = self.slots, self.terms
        if self.terms <= max_count:
            self.terms = max(max_count + 1, 2 * self.terms)
        if need > self.slots:
            self.slots = max(64, need * 3 // 2)
        return dict(chunks=ch, slots=need, workgroups=sum(ch), max_count=max_count, slots_before=slots_before, slots_after=self.slots,
                    terms_before=terms_before, terms_after=self.terms)


# ---- a call and what it runs on -------------------------------------------------------------------------------------------------
class Setup:
    """target planes [n][ty][tx] and a source [vz][vy][vx] (int16), the source's bin width and bin count"""

    def __init__(self, targets, source, ws, nbs):
        self.targets, self.source, self.ws, self.nbs = np.ascontiguousarray(targets, np.int16), np.ascontiguousarray(source, np.int16), ws, nbs
        self.ty, self.tx = self.targets.shape[1:]
        self.binned = np.where(self.source > 0, self.source // ws, self.source).astype(np.int16)   # what nmi_bin_source leaves
        self.cache = {}                                                  # restatements of evaluations, by restate()


class Call:
    """one nmi_evaluate: evaluation e spans ppe[e] consecutive entries of idx / mats and has its own (width, nbt)"""

    def __init__(self, ppe, idx, mats, widths, nbts, nbs, hist=True):
        self.ppe, self.idx = np.asarray(ppe, np.int32), np.asarray(idx, np.int32)
        self.mats = np.asarray(mats, np.float64).reshape(-1, 4, 4)
        self.widths, self.nbts, self.nbs, self.hist = np.asarray(widths, np.int32), np.asarray(nbts, np.int32), int(nbs), hist
        assert len(self.idx) == len(self.mats) == int(self.ppe.sum()) and len(self.widths) == len(self.nbts) == len(self.ppe)
        self.starts = np.concatenate([[0], np.cumsum(self.ppe)[:-1]]).astype(int)

    def __len__(self):
        return len(self.ppe)

    def planes(self, e):
        return slice(int(self.starts[e]), int(self.starts[e] + self.ppe[e]))

    def take(self, order, hist=None):
        """the call of evaluations `order` of this one, in that order"""
        order = list(order)
        rows = np.concatenate([np.arange(self.starts[e], self.starts[e] + self.ppe[e]) for e in order])
        return Call(self.ppe[order], self.idx[rows], self.mats[rows], self.widths[order], self.nbts[order], self.nbs,
                    self.hist if hist is None else hist)

    def args(self):
        return self.ppe, self.idx, self.mats, self.widths, self.nbts, self.nbs


def join(calls, hist=True):
    return Call(np.concatenate([c.ppe for c in calls]), np.concatenate([c.idx for c in calls]), np.concatenate([c.mats for c in calls]),
                np.concatenate([c.widths for c in calls]), np.concatenate([c.nbts for c in calls]), calls[0].nbs, hist)


def sums_and_nmi(entropy_sums, h, nbt, nbs):
    """entropy_sums; where one joint bin holds every sample the three entropies are the same expression and 0, Python's division
    raises, and C's 0 / 0 is NaN"""
    try:
        return entropy_sums(h, nbt, nbs)
    except ZeroDivisionError:
        assert np.count_nonzero(h) == 1
        n = int(h.sum())
        t = float(n) * math.log(float(n))
        return (float(n), t, t, t), float("nan")


def restate(setup, call, joint_histogram, entropy_sums):
    """-> ({n, S_xy, S_x, S_y} [n_eval][4], joint histograms [n_eval][64][64], NMI [n_eval]) of the numpy reference; an evaluation that
    recurs (the same planes, matrices and bins) is computed once per setup"""
    n = len(call)
    out, hist, nmi = np.zeros((n, 4)), np.zeros((n, BINS, BINS), np.uint32), np.zeros(n)
    for e in range(n):
        rows, w, nbt = call.planes(e), int(call.widths[e]), int(call.nbts[e])
        key = (call.idx[rows].tobytes(), call.mats[rows].tobytes(), w, nbt, call.nbs)
        if key not in setup.cache:
            h = joint_histogram(setup.targets[call.idx[rows]], call.mats[rows], setup.binned, w, nbt, call.nbs)
            setup.cache[key] = (h, *sums_and_nmi(entropy_sums, h, nbt, call.nbs))
        hist[e], out[e], nmi[e] = setup.cache[key]
    return out, hist, nmi


# ---- builders -------------------------------------------------------------------------------------------------------------------
def _rotation(deg):
    ax, ay, az = np.deg2rad(deg)
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def plane_matrices(rng, tx, ty, ssize, nz, span=None):
    """per-plane source-from-target matrices of one evaluation of nz planes: a random rotation and scale that puts the middle of the
    stack near the middle of the source, plane k one step along the third column on; `span`: the planes' larger side covers at most
    that many source voxels, and the nz planes half as many"""
    R = _rotation(rng.uniform(-25, 25, 3)) @ np.diag(rng.uniform(0.6, 1.4, 3))
    if span is not None:
        R[:, :2] *= min(1.0, span / (1.4 * max(tx, ty)))
        R[:, 2] *= min(1.0, span / (2.8 * nz))
    ct, cs = np.array([tx - 1, ty - 1, nz - 1], float) / 2, (np.array(ssize, float) - 1) / 2
    t0 = cs - R @ ct + rng.uniform(-2, 2, 3)
    out = np.tile(np.eye(4), (nz, 1, 1))
    out[:, :3, :3] = R
    out[:, :3, 3] = t0 + np.arange(nz)[:, None] * R[:, 2]
    return out


SSIZE = (40, 44, 38)                                                      # (x, y, z) of the common source


def common_source(rng, top=3008, ssize=SSIZE):
    """values 0 .. top-1: blocks of 4 x 4 x 4 voxels of one value each (inside a block the interpolation returns it, so the first and
    the last source bin are reached), a fifth of the voxels redrawn, two columns of padding"""
    blocks = rng.integers(0, top, [(n + 3) // 4 for n in ssize[::-1]])
    src = np.kron(blocks, np.ones((4, 4, 4), np.int64))[:ssize[2], :ssize[1], :ssize[0]]
    noise = rng.random(src.shape) < 0.2
    src[noise] = rng.integers(0, top, int(noise.sum()))
    src = src.astype(np.int16)
    src[:, :, :2] = -1
    return src


def _evaluation(rng, setup_tx, setup_ty, idx, width, nbt, nbs, span=34, ssize=SSIZE):
    return Call([len(idx)], idx, plane_matrices(rng, setup_tx, setup_ty, ssize, len(idx), span), [width], [nbt], nbs)


# 1. bins per evaluation, mixed in one call ----------------------------------------------------------------------------------------
CASE1_KINDS = [(7, 1), (5, 2), (2, 33), (1, 64), (512, 64)]              # (width, nbt): the largest value a kind holds is nbt * width - 1,
CASE1_TOPS = [6, 9, 64, 63, 32766]                                       # except 64 = range 65 at width 2 and 32766 = range 32767 at 512
CASE1_EVALS = [(0, 1), (1, 5), (2, 9), (3, 4), (4, 6), (2, 1), (0, 8), (4, 1), (3, 5), (1, 2)]   # (kind, planes)
CASE1_CHUNKS = [1, 2, 3, 1, 2, 1, 2, 1, 2, 1]                            # 61 x 67 planes: 4 per workgroup


@functools.lru_cache(maxsize=None)
def case1():
    """-> (setup with 64 source bins, setup with 1, the call for the first, the call for the second): two stored planes per kind, the
    kind's largest value at the middle pixel of its first"""
    rng = np.random.default_rng(101)
    tx, ty = 61, 67
    planes = []
    for top in CASE1_TOPS:
        for k in range(2):
            p = rng.integers(-1, top + 1, (ty, tx)).astype(np.int16)
            p[:2] = -1
            if k == 0:
                p[ty // 2, tx // 2] = top
            planes.append(p)
    wide = Setup(planes, common_source(rng), 47, 64)                     # number_of_bins(0, 3007) = (64, 47)
    flat_src = rng.integers(1, 500, SSIZE[::-1]).astype(np.int16)        # every positive value below the width: one source bin
    flat_src[:, :3, :] = -1
    flat_src[rng.random(flat_src.shape) < 0.02] = -1
    flat = Setup(planes, flat_src, 500, 1)
    calls = []
    for nbs in (64, 1):
        evs = []
        for kind, n in CASE1_EVALS:
            w, nbt = CASE1_KINDS[kind]
            evs.append(_evaluation(rng, tx, ty, [2 * kind + p % 2 for p in range(n)], w, nbt, nbs))
        calls.append(join(evs))
    return wide, flat, calls[0], calls[1]


# 2. the compaction and the serial sums at their ends ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case2_full():
    """(a) every one of the 4096 joint bins non-zero, in 8 chunks of one 128 x 128 plane"""
    rng = np.random.default_rng(102)
    src = np.broadcast_to(np.minimum(np.arange(66), 63).astype(np.int16), (12, 20, 66))
    targets = rng.integers(0, 64, (8, 128, 128)).astype(np.int16)
    mats = np.tile(np.eye(4), (8, 1, 1))
    mats[:, 0, 0], mats[:, 1, 1] = 63.4 / 128, 18 / 128
    mats[:, :3, 3] = [[0.01, 0.5, 1 + k] for k in range(8)]
    return Setup(targets, src, 1, 64), Call([8], np.arange(8), mats, [1], [64], 64)


CASE2_NNZ = [5, 27, 16, 0, 0, 32]                                        # of the evaluations of case2_sparse


@functools.lru_cache(maxsize=None)
def case2_sparse():
    """(c), (d): planes with 5, 27 and 16 pixels of distinct values among padding, each pixel its own joint bin; a plane of padding
    only; a full plane whose matrix lies outside the source; the first two together"""
    rng = np.random.default_rng(103)
    tx = ty = 20
    src = rng.integers(0, 64, (28, 34, 30)).astype(np.int16)
    planes = np.full((5, ty, tx), -1, np.int16)
    for k, (n, first) in enumerate(((5, 0), (27, 10), (16, 40))):
        at = rng.choice(tx * ty, n, replace=False)
        planes[k].reshape(-1)[at] = first + np.arange(n)
    planes[4] = rng.integers(0, 64, (ty, tx))
    M = np.eye(4)
    M[0, 0] = M[1, 1] = 0.9
    M[:3, 3] = (5.3, 6.2, 10.4)
    away = M.copy()
    away[:3, 3] += 500.0
    up = M.copy()
    up[2, 3] += 1.0
    return (Setup(planes, src, 1, 64),
            Call([1, 1, 1, 1, 1, 2], [0, 1, 2, 3, 4, 0, 1], [M, M, M, M, away, M, up], [1] * 6, [64] * 6, 64))


# 3. plane sizes around per_block ---------------------------------------------------------------------------------------------------
CASE3_SIZES = [(5, 7), (128, 64), (129, 64), (128, 128), (130, 127)]
CASE3_PER_BLOCK = [468, 2, 1, 1, 1]


@functools.lru_cache(maxsize=None)
def case3(tx, ty):
    """evaluations of per_block, per_block + 1, 2 * per_block planes and of one plane, on three stored planes"""
    rng = np.random.default_rng(1000 * tx + ty)
    pb = per_block(tx, ty)
    targets = rng.integers(-1, 192, (3, ty, tx)).astype(np.int16)
    targets[1][rng.random((ty, tx)) < 0.3] = -1
    setup = Setup(targets, common_source(rng), 47, 64)
    evs = [_evaluation(rng, tx, ty, [(e + p) % 3 for p in range(n)], 3, 64, 64) for e, n in enumerate((pb, pb + 1, 2 * pb, 1))]
    return setup, join(evs)


# 4. many chunks, many slots, regrowth ----------------------------------------------------------------------------------------------
def _setup_129(rng, n=4):
    targets = rng.integers(-1, 192, (n, 64, 129)).astype(np.int16)
    targets[:, :2] = -1
    return Setup(targets, common_source(rng), 47, 64)


CASE4_CALLS = [3, 65, 150, 3]                                            # split evaluations of the calls of 4 (b)
CASE4_CAPS = [64, 97, 225, 225]


@functools.lru_cache(maxsize=None)
def case4():
    """-> (setup, the call of (a): 70 and 33 planes around three single ones, the calls of (b)); 129 x 64: every plane a chunk"""
    rng = np.random.default_rng(104)
    setup = _setup_129(rng)
    a = join([_evaluation(rng, 129, 64, [(e + p) % 4 for p in range(n)], 3, 64, 64) for e, n in enumerate((70, 1, 1, 1, 33))])
    pool = join([_evaluation(rng, 129, 64, [e % 4, (e + 1 + e // 4) % 4], 3, 64, 64) for e in range(150)])
    b = [pool.take(range(0, 3)), pool.take(range(3, 68)), pool, pool.take(range(0, 3))]
    return setup, a, b


@functools.lru_cache(maxsize=None)
def case4_batch():
    """(c) 3000 single-plane evaluations of 8 x 8 planes, 61 different ones in turn"""
    rng = np.random.default_rng(105)
    targets = rng.integers(-1, 8, (6, 8, 8)).astype(np.int16)
    ssize = (14, 15, 13)
    setup = Setup(targets, rng.integers(0, 64, ssize[::-1]).astype(np.int16), 8, 8)
    kinds = join([_evaluation(rng, 8, 8, [e % 6], 1, 8, 8, span=9, ssize=ssize) for e in range(61)])
    return setup, kinds.take([e % 61 for e in range(3000)], hist=False)


# 5. the term table's last entry ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case5():
    """-> (setup and call 1: one 5 x 7 plane, so the table holds entries 0 .. 35; setup and call 2: 36 samples in one joint bin)"""
    rng = np.random.default_rng(106)
    first = Setup(rng.integers(0, 60, (1, 7, 5)), rng.integers(0, 64, (9, 10, 11)).astype(np.int16), 1, 64)
    M1 = np.eye(4)
    M1[:3, 3] = (2.5, 1.25, 3.5)
    second = Setup(np.full((1, 6, 6), 3, np.int16), np.full((6, 8, 8), 5, np.int16), 1, 6)
    M2 = np.eye(4)
    M2[0, 0] = M2[1, 1] = 0.9
    M2[:3, 3] = (1, 1, 2)
    return (first, Call([1], [0], [M1], [1], [64], 64)), (second, Call([1], [0], [M2], [1], [4], 6))


# 6. a refused call leaves nothing behind -------------------------------------------------------------------------------------------
CASE6_BAD_AT = (32, 64)                                                  # (row, column) of the one value at nbt * width in plane 2


@functools.lru_cache(maxsize=None)
def case6():
    """-> (setup, {name: refused call}, the mended twin of each, the valid call).  Planes 0 and 1 fit 64 bins of width 3; plane 2 is
    plane 0 with one pixel at 192 = 64 * 3.  129 x 64: an evaluation of 5 planes is 5 chunks."""
    rng = np.random.default_rng(107)
    setup = _setup_129(rng, 3)
    setup.targets[0][CASE6_BAD_AT] = 100
    setup.targets[2] = setup.targets[0]
    setup.targets[2][CASE6_BAD_AT] = 192
    ev = lambda idx: _evaluation(rng, 129, 64, idx, 3, 64, 64)           # noqa: E731
    good = [ev([0, 1, 0, 1, 0]) for _ in range(4)]
    single = ev([0])
    mended = {"first chunk": join([good[0], good[1]]), "last chunk": join([good[1], good[0]]), "single block": join([good[2], single, good[3]])}
    refused = {}
    for name, bad_row in (("first chunk", 0), ("last chunk", 9), ("single block", 5)):
        c = mended[name]
        idx = c.idx.copy()
        assert idx[bad_row] == 0
        idx[bad_row] = 2
        refused[name] = Call(c.ppe, idx, c.mats, c.widths, c.nbts, c.nbs)
    c = mended["first chunk"]
    idx = c.idx.copy()
    idx[7] = 3                                                           # three planes are stored
    refused["index"] = Call(c.ppe, idx, c.mats, c.widths, c.nbts, c.nbs)
    valid = join([good[3], good[0], good[2], single])
    return setup, refused, mended, valid


# 7. the shared evaluation arena ----------------------------------------------------------------------------------------------------
CASE7_TARGET_BINS = (63, 29)                                             # number_of_bins(0, 1799)
CASE7_SOURCE_BINS = (63, 40)                                             # number_of_bins(0, 2499)
CASE7_LNCC = 210                                                         # evaluations whose k maps no longer fit what NMI's histograms grew


class Arena:
    """the evaluate calls' grow-only device buffer (sim_evaluate): inputs | outputs | test map at 8-byte alignment, grown to
    max(floor, need * 3 // 2 + 4096) when a call needs more than there is"""

    def __init__(self):
        self.capacity = 0

    def call(self, b_in, b_out, b_map=0, floor=0):
        o_out = (b_in + 7) // 8 * 8
        need = (o_out + b_out + 7) // 8 * 8 + b_map
        grew = need > self.capacity
        if grew:
            self.capacity = max(floor, need * 3 // 2 + 4096)
        return need, grew

    def ncc(self, n):                                                    # matrices | indices -> six int64 moments; the floor holds 256
        return self.call(n * (128 + 4), n * 48, 0, 256 * (128 + 4 + 48))

    def nmi(self, call, tx, ty):                                         # matrices | blocks | evaluations | indices -> 4 doubles, histograms
        planes, blocks = int(call.ppe.sum()), sum(chunks(p, tx, ty) for p in call.ppe)
        return self.call(planes * 128 + blocks * 24 + len(call) * 8 + planes * 4, len(call) * 32, len(call) * BINS * BINS * 4 if call.hist else 0)

    def lncc(self, n, tx, ty, maps):                                     # matrices | indices -> {N, S}, the k maps
        return self.call(n * (128 + 4), n * 16, n * tx * ty * 4 if maps else 0)


@functools.lru_cache(maxsize=None)
def case7():
    """-> (setup, [(metric, arguments)] in the order of the sequence): NCC and LNCC take one plane per evaluation"""
    rng = np.random.default_rng(108)
    tx, ty, ssize = 37, 33, (30, 34, 28)
    targets = rng.integers(0, 1800, (5, ty, tx)).astype(np.int16)
    targets[rng.random(targets.shape) < 0.08] = -1
    src = rng.integers(-1, 2500, ssize[::-1]).astype(np.int16)
    src = np.maximum(src, (np.indices(src.shape).sum(0) * 40 % 3000).astype(np.int16) // 2)
    src[:, :, :2] = -1
    nbt, wt = CASE7_TARGET_BINS
    nbs, ws = CASE7_SOURCE_BINS
    setup = Setup(targets, src, ws, nbs)

    def singles(n):
        idx = rng.integers(0, 5, n).astype(np.int32)
        return idx, np.concatenate([plane_matrices(rng, tx, ty, ssize, 1) for _ in idx])
    nmi = join([_evaluation(rng, tx, ty, [(e + p) % 5 for p in range(n)], wt, nbt, nbs, span=None, ssize=ssize)
                for e, n in enumerate([1] * 19 + [14] + [1] * 19 + [27])])
    lncc = singles(CASE7_LNCC)
    return setup, [("ncc", singles(10)), ("nmi", nmi), ("lncc maps", lncc), ("ncc", singles(300)), ("nmi", nmi.take(range(40), hist=False)),
                   ("lncc", lncc)]
