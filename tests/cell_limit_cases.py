"""Geometries at the layout limits of the cell lists (csrc/svr_cell.inc: cell_prepare_state), in pairs: `beyond` trips exactly one
limit, so the pass leaves the cell path for the tile kernels (cells_or_fallback, csrc/svr_hip.hip); its `inside` twin sits just
within that limit and has to stay on the cell path.  tests/test_cell_limit_cases.py checks on the CPU that every case is on its
side of its limit; tests/test_cell_limits_gpu.py runs them on the device against the oracle.

All cases but 4 start from one small problem (24^3 voxels of 1 mm, an axial and a coronal stack of three 16 x 16 slices) with the
mask set to ones: a slice far off the volume lands on the volume's low faces (negative coordinates alias to index 0, RC.cu:382 /
508), and the phantom's spherical mask would hide exactly those voxels.

The limits, as the code states them (line numbers of csrc/svr_cell.inc):
  1  centres           ok && q[k] > -32000 && q[k] < 32000 for the six bounds of a class      (:1546; CellRec / CellRun hold shorts)
  2  planes per class  C.ng <= 1024, ng = plast - pfirst + 1, pfirst = min cz - NC,
                       plast = min(max cz + NH, v - 1)                                         (:1550-1554; items[] = cell << 10 | g)
  3  cells             ncells < 2^18, the classes' ncx * ncl added up                          (:1548-1549, 1557, 1562; key bits 46..63)
  4  pixels per run    cnt[q] > CELL_RUN_MAX = 16384 pixels of one slice in one cell around one band of planes (k_cell_run_ranges; a slot adds
                       its quarter of a run in one chain of float adds -- the limit stood at the 65535 of CellRun::n until these tests measured
                       volw 4e-5 from the oracle there, twice the tolerance)
  5  slice grid        sx * sy > 2^20                                                          (:1476; key bits 0..19)
  6  slices            ns > 2^17                                                               (:1476; key bits 29..45)
  7  LDS boxes         (scatter: 4) * PP * 8 bytes > 64 KiB, PP = ((CX + 15) | 1) * (CL + 15)  (:1527-1533)
with NC = 7, NH = 8 for the support of 16 (NC = 5, NH = 6 for the patch-based support of 12).

Left out: the high side of the centre limit (q[k] < 32000) needs a centre that is not dropped, i.e. a volume side above 32 000
(k_cell_centres drops a pixel whose footprint starts beyond the high end); and the staging buffer that does not fit the device's
memory (:1712) depends on the machine the test runs on."""
import copy
import functools
from dataclasses import dataclass, field

import numpy as np

from fetalreconstruction_amd import phantom

NC, NH = 7, 8
RUN_MAX = 16384                      # CELL_RUN_MAX of csrc/svr_cell.inc


@dataclass
class Case:
    name: str
    limit: int                      # 1..7 above
    side: str                       # "beyond" | "inside"
    problem: phantom.Problem
    special: tuple                  # the slices that carry the case: moved, or at the top of a key field
    options: dict = field(default_factory=dict)
    split_gather: bool = False      # case 7: the gather's own lists stay usable while the scatter falls back


# ---- the arithmetic of the engine and the oracle, restated ------------------------------------------------------------------
def _matvec(M, x, y, z):
    """float32, left to right, no contraction: matvec3 of csrc/svr_hip.hip and oracle/svr_oracle.c"""
    M = M.astype(np.float32)
    return (M[0] * x + M[1] * y + M[2] * z + M[3], M[4] * x + M[5] * y + M[6] * z + M[7], M[8] * x + M[9] * y + M[10] * z + M[11])


def centres(P, sl):
    """centre voxels (int64 [n][3]) and pixel coordinates [n][2] = (px, py) of the pixels != -1 of slice sl:
    round(reconW2I * (T * (sliceI2W * p))) in float32, as pixel_setup has it (the CPU test holds it against the oracle's)"""
    py, px = np.nonzero(P.slices[sl] != -1)
    x, y = px.astype(np.float32), py.astype(np.float32)
    w = _matvec(P.slice_i2w[sl], x, y, np.float32(0))
    t = _matvec(P.slice_t[sl], *w)
    v = _matvec(np.asarray(P.recon_w2i), *t)
    c = np.stack([np.where(a >= 0, np.floor(a + np.float32(0.5)), np.ceil(a - np.float32(0.5))) for a in v], -1)     # roundf: half away from zero
    return c.astype(np.int64), np.stack([px, py], -1)


def owned_axis(P, sl):
    """SliceConst::own: 1 = the volume's y, 2 = its z, whichever is closer to the slice normal (row 2 of volume index -> slice pixel)"""
    A = (P.slice_w2i[sl].reshape(4, 4).astype(np.float64) @ P.slice_tinv[sl].reshape(4, 4).astype(np.float64)
         @ np.asarray(P.recon_i2w, np.float64).reshape(4, 4))
    return 1 if abs(A[2, 1]) > abs(A[2, 2]) else 2


def auto_cell(P, gather=False, pvr=False):
    """cell_auto_size (:1414-1425)"""
    d = float(P.vdim[0]) * float(P.vdim[1]) / (float(P.slice_dim[0, 0]) * float(P.slice_dim[0, 1]))
    d = min(1.0, max(d, 0.0625))
    area = min(192.0, 32.0 / d ** 1.35) if gather else min(96.0, (28.0 if pvr else 24.0) / d)
    cw = min(16, max(2, int(np.floor(np.sqrt(1.5 * area) + 0.5))))
    ch = min(16, max(2, int(np.floor(area / cw + 0.5))))
    if (cw & 1) and cw < 16:
        cw += 1
    return cw, ch


def layout(P, cell_w, cell_h, nc=NC, nh=NH):
    """what cell_prepare_state works out from the centres (:1539-1562): per class [own 1, own 2] the six bounds q, ncx, ncl, ng;
    ncells; the largest number of pixels of one slice in one cell"""
    vx, vy, vz = P.vsize
    cls = [dict(q=None, ncx=0, ncl=0, ng=0), dict(q=None, ncx=0, ncl=0, ng=0)]
    kept = []
    for sl in np.flatnonzero((P.slices != -1).reshape(P.ns, -1).any(1)):
        c, _ = centres(P, sl)
        k = 0 if owned_axis(P, sl) == 1 else 1
        cx, cl, cz = c[:, 0], (c[:, 2] if k == 0 else c[:, 1]), (c[:, 1] if k == 0 else c[:, 2])
        vgl, vgz = (vz, vy) if k == 0 else (vy, vz)
        keep = ~((cx - nc > vx - 1) | (cl - nc > vgl - 1) | (cz - nc > vgz - 1))         # k_cell_centres :165
        kept.append((k, sl, cx[keep], cl[keep], cz[keep]))
    for k in (0, 1):
        rows = [r for r in kept if r[0] == k and len(r[2])]
        if not rows:
            continue
        cx, cl, cz = (np.concatenate([r[i] for r in rows]) for i in (2, 3, 4))
        q = [int(cx.min()), int(cx.max()), int(cl.min()), int(cl.max()), int(cz.min()), int(cz.max())]
        vgz = vy if k == 0 else vz
        pfirst, plast = q[4] - nc, min(q[5] + nh, vgz - 1)
        cls[k] = dict(q=q, ncx=(q[1] - q[0]) // cell_w + 1, ncl=(q[3] - q[2]) // cell_h + 1, ng=max(plast - pfirst + 1, 0), pfirst=pfirst, plast=plast)
    most = 0
    for k, sl, cx, cl, cz in kept:
        if len(cx):
            q = cls[k]["q"]
            cell = ((cl - q[2]) // cell_h) * cls[k]["ncx"] + (cx - q[0]) // cell_w
            most = max(most, int(np.bincount(cell - cell.min()).max()))
    return dict(classes=cls, ncells=sum(c["ncx"] * c["ncl"] for c in cls), most_per_cell=most)


def lds_bytes(cell_w, cell_h, slots=4, ns=16):
    """:1527-1533"""
    return slots * (((cell_w + ns - 1) | 1) * (cell_h + ns - 1)) * 8


def blanked(P, special):
    """the same problem without the special slices"""
    Q = copy.copy(P)
    Q.slices = P.slices.copy()
    Q.slices[list(special)] = -1.0
    return Q


# ---- the builders -----------------------------------------------------------------------------------------------------------
def _own(P):
    Q = copy.copy(P)
    for n in ("slices", "slice_i2w", "slice_w2i", "slice_t", "slice_tinv", "slice_dim", "sizes_x", "sizes_y", "stack_index", "mask"):
        setattr(Q, n, getattr(P, n).copy())
    return Q


@functools.lru_cache(maxsize=None)
def _base_cached():
    P = phantom.make_problem(2, (16, 16, 3), 1.1, 2.4, None, 1.0, 9.0, seed=3, orientations=("ax", "cor"), motion_frac=0.5, name="cell-limits")
    P = _own(P)
    P.mask[...] = 1.0
    return P


def base():
    return _own(_base_cached())


def moved(P, slices, t):
    """the slices moved by t (mm, world = voxels here) after their own motion"""
    Q = _own(P)
    M = np.eye(4)
    M[:3, 3] = t
    for s in slices:
        T = M @ P.slice_t[s].reshape(4, 4).astype(np.float64)
        Q.slice_t[s] = T.astype(np.float32).reshape(16)
        Q.slice_tinv[s] = np.linalg.inv(T).astype(np.float32).reshape(16)
    return Q


def _shift_to(P, slices, axis, target):
    """move the slices along a volume axis so that their smallest centre on it is `target`"""
    lo = min(int(centres(P, s)[0][:, axis].min()) for s in slices)
    t = np.zeros(3)
    t[axis] = target - lo + 0.0                       # (whole voxels: the sub-voxel phase of the slices stays what it was)
    return moved(P, slices, t)


def _retile(P, ns, sy, sx, put):
    """a slice grid of another size: put = [(new slice, old slice, y0, x0, h, w, oy, ox)] copies the old slice's pixels [oy:oy+h, ox:ox+w] to
    [y0:y0+h, x0:x0+w] of the new one, with sliceI2W / sliceW2I moved along so that every pixel stays where it was in the world.  The other
    slices are padding (-1) with the geometry of old slice 0."""
    Q = copy.copy(P)
    Q.slices = np.full((ns, sy, sx), -1.0, np.float32)
    for n in ("slice_i2w", "slice_w2i", "slice_t", "slice_tinv", "slice_dim"):
        setattr(Q, n, np.ascontiguousarray(np.tile(getattr(P, n)[:1], (ns, 1))))
    Q.stack_index = np.zeros(ns, np.int32)
    Q.sizes_x, Q.sizes_y = np.full(ns, sx, np.int32), np.full(ns, sy, np.int32)
    Q.slice_attr = None
    Q.mask = P.mask.copy()
    for new, old, y0, x0, h, w, oy, ox in put:
        Q.slices[new, y0:y0 + h, x0:x0 + w] = P.slices[old, oy:oy + h, ox:ox + w]
        S = np.eye(4)
        S[0, 3], S[1, 3] = ox - x0, oy - y0           # new pixel -> old pixel
        i2w = P.slice_i2w[old].reshape(4, 4).astype(np.float64) @ S
        Q.slice_i2w[new] = i2w.astype(np.float32).reshape(16)
        Q.slice_w2i[new] = np.linalg.inv(i2w).astype(np.float32).reshape(16)
        for n in ("slice_t", "slice_tinv", "slice_dim"):
            getattr(Q, n)[new] = getattr(P, n)[old]
        Q.stack_index[new] = P.stack_index[old]
    return Q


AX, COR = (0, 1, 2), (3, 4, 5)          # the base problem's stacks


def _case1(side, which):
    P = base()
    target = -32110 if side == "beyond" else -31950
    if which == "x":                    # one axial slice along x: class 1 (own z), the x bounds q[0]
        return Case(f"centres-x-{side}", 1, side, _shift_to(P, (1,), 0, target), (1,))
    # the owned axis of the coronal class (own y: class 0, q[4]).  The whole stack moves: one slice alone that far off would also make
    # more than 1024 planes between itself and its stack (limit 2), and a case trips one limit
    return Case(f"centres-own-{side}", 1, side, _shift_to(P, COR, 1, target), COR)


def _case2(side, exact=False):
    P = base()
    want = (lambda ng: ng == 1024) if exact else (lambda ng: 1015 <= ng < 1024) if side == "inside" else (lambda ng: 1030 <= ng <= 1040)
    for lo in range(-1020, -970):
        Q = _shift_to(P, (1,), 2, lo)
        if want(layout(Q, *auto_cell(Q))["classes"][1]["ng"]):
            return Case(f"planes-{side}{'-1024' if exact else ''}", 2, side, Q, (1,))
    raise AssertionError("no shift gives the number of planes asked for")


def _case3(side):
    P = base()
    want = (lambda n: n >= 2 ** 18) if side == "beyond" else (lambda n: 0.9 * 2 ** 18 <= n < 2 ** 18)
    for s in ((1100,) if side == "beyond" else range(1000, 960, -1)):
        Q = moved(P, (1,), (-s - 0.3, -s - 0.6, 0.0))
        if want(layout(Q, 2, 2)["ncells"]):
            return Case(f"cells-{side}", 3, side, Q, (1,), dict(cell_w=2, cell_h=2))
    raise AssertionError("no shift gives the number of cells asked for")


def _case4(side):
    sy = 129 if side == "beyond" else 128                                       # 128 x 129 = 16 512 pixels / 128 x 128 = 16 384: exactly the limit
    P = phantom.make_problem(1, (128, sy, 1), 0.01, 2.4, None, 1.0, 9.0, seed=3, orientations=("ax",), motion_frac=0.0, name=f"run-{side}")
    P = _own(P)
    P.mask[...] = 1.0
    P.slices = np.where(P.slices > 0, P.slices, 100.0).astype(np.float32)       # all active
    return Case(f"run-{side}", 4, side, P, (0,), dict(cell_w=16, cell_h=16))


def _case5(side):
    P = phantom.make_problem(1, (16, 16, 3), 1.1, 2.4, None, 1.0, 9.0, seed=3, orientations=("ax",), motion_frac=0.5, name=f"grid-{side}")
    P.mask = np.ones_like(P.mask)
    P.slices = np.where(P.slices > 0, P.slices, 120.0).astype(np.float32)       # all active: the last pixel of the grid too
    sy, sx = (1025, 1024) if side == "beyond" else (1024, 1024)
    Q = _retile(P, 3, sy, sx, [(s, s, sy - 16, sx - 16, 16, 16, 0, 0) for s in range(3)])
    return Case(f"grid-{side}", 5, side, Q, (0, 1, 2))


def _case6(side):
    P = base()
    ns = 2 ** 17 + 1 if side == "beyond" else 2 ** 17
    put = [(s, s, 0, 0, 2, 2, 7, 7) for s in AX] + [(ns - 3 + k, s, 0, 0, 2, 2, 7, 7) for k, s in enumerate(COR)]
    Q = _retile(P, ns, 2, 2, put)
    return Case(f"slices-{side}", 6, side, Q, (ns - 3, ns - 2, ns - 1))


def _case7(side, split=False):
    c = 32 if side == "beyond" else 26
    opt = dict(cell_w=c, cell_h=c)
    if split:
        opt.update(cell_gw=16, cell_gh=16)
    return Case(f"lds-{side}{'-split' if split else ''}", 7, side, base(), (1,), opt, split_gather=split)


_BUILDERS = {
    "centres-x-beyond": lambda: _case1("beyond", "x"), "centres-x-inside": lambda: _case1("inside", "x"),
    "centres-own-beyond": lambda: _case1("beyond", "own"), "centres-own-inside": lambda: _case1("inside", "own"),
    "planes-beyond": lambda: _case2("beyond"), "planes-inside": lambda: _case2("inside"), "planes-inside-1024": lambda: _case2("inside", True),
    "cells-beyond": lambda: _case3("beyond"), "cells-inside": lambda: _case3("inside"),
    "run-beyond": lambda: _case4("beyond"), "run-inside": lambda: _case4("inside"),
    "grid-beyond": lambda: _case5("beyond"), "grid-inside": lambda: _case5("inside"),
    "slices-beyond": lambda: _case6("beyond"), "slices-inside": lambda: _case6("inside"),
    "lds-beyond": lambda: _case7("beyond"), "lds-inside": lambda: _case7("inside"), "lds-beyond-split": lambda: _case7("beyond", True),
}
NAMES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def build(name):
    """the case of that name; built once per session -- a test that edits a problem takes a copy"""
    return _BUILDERS[name]()


def sizes(case, gather=False, pvr=False):
    """the cell size the engine takes for the case: the options where set, else cell_auto_size (cell_sizes :1426-1433)"""
    w, h = auto_cell(case.problem, gather, pvr)
    w, h = case.options.get("cell_w", w), case.options.get("cell_h", h)
    if gather:
        w, h = case.options.get("cell_gw", w), case.options.get("cell_gh", h)
    return w, h


def em_inputs(P):
    """random EM weights (a fifth of them zero) and simulated slices as in tests/test_fuzz_gpu.py, and a slice weight vector with one zero
    (a problem of one slice keeps its weight) -> (weights, simslices, slice_weight); a function of the slices alone"""
    rng = np.random.default_rng(4242)
    act, pos = P.slices != -1, P.slices > 0
    w = np.zeros(P.slices.shape, np.float32)
    w[act] = (rng.uniform(0.0, 1.0, int(act.sum())) * (rng.uniform(0, 1, int(act.sum())) > 0.2)).astype(np.float32)
    ss = np.zeros(P.slices.shape, np.float32)
    ss[pos] = (P.slices[pos] * rng.uniform(0.8, 1.2, int(pos.sum()))).astype(np.float32)
    live = np.flatnonzero(act.reshape(P.ns, -1).any(1))
    sw = np.ones(P.ns, np.float32)
    sw[live] = rng.uniform(0.1, 1.0, len(live)).astype(np.float32)
    if len(live) > 1:
        sw[live[0]] = 0.0
    return w, ss, sw


# ---- the oracle's side, once per case -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_run(name, pvr=False):
    """UpdateScaleVector, InitializeEMValues, GaussianReconstruction; SimulateSlices; random EM weights and simulated slices, a slice weight
    vector with one zero, SuperresolutionBackproject -- the sequence of tests/test_fuzz_gpu.py -> copies of every buffer compared"""
    from oracle import pyoracle
    pyoracle.build()
    P = build(name).problem
    orc = pyoracle.OracleReconstruction(P, pyoracle.CANON, pvr=pvr)
    ones = np.ones(P.ns, np.float32)
    orc.UpdateScaleVector(ones, ones)
    orc.InitializeEMValues()
    orc.GaussianReconstruction()
    out = dict(psf_sums=orc.psf_sums.copy(), volw=orc.volw.copy(), recon=orc.recon.copy())
    orc.SimulateSlices()
    out.update(siminside=orc.siminside.copy(), simslices=orc.simslices.copy(), simweights=orc.simweights.copy())
    w, ss, sw = em_inputs(P)
    orc.weights[...] = w
    orc.simslices[...] = ss
    orc.SuperresolutionBackproject(sw)
    out.update(weights=w, sr_simslices=ss, slice_weight=sw, cmap=orc.cmap.copy(), addon=orc.addon.copy())
    for v in out.values():
        v.setflags(write=False)
    return out
