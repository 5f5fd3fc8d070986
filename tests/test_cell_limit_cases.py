"""The geometries of tests/cell_limit_cases.py, checked on the CPU: every case is on the intended side of its limit with the margin
asked for, the oracle's buffers are finite, and the slices that carry the case add to the volume (so a kernel that lost them would show).
The limits' arithmetic is restated next to each case with its line in csrc/svr_cell.inc (cell_prepare_state unless said otherwise)."""
import copy

import numpy as np
import pytest

from tests import cell_limit_cases as C

NC, NH = C.NC, C.NH


def _layout(case, gather=False):
    return C.layout(case.problem, *C.sizes(case, gather))


def _other_limits_hold(case, but):
    """the limits the case is not about, for the scatter's and the gather's lists: a `beyond` case trips ONE limit, an `inside` case none"""
    P = case.problem
    ns, sy, sx = P.slices.shape
    for gather in (False, True):
        w, h = C.sizes(case, gather)
        L = C.layout(P, w, h)
        if but != 1:
            assert all(-32000 < v < 32000 for c in L["classes"] if c["q"] for v in c["q"])            # :1546
        if but != 2:
            assert all(c["ng"] <= 1024 for c in L["classes"])                                          # :1554
        if but != 3:
            ngs = max(1, max(c["ng"] for c in L["classes"]))
            assert 0 < L["ncells"] < 2 ** 18 and L["ncells"] * ngs < 2 ** 28                           # :1562
        if but != 4:
            assert L["most_per_cell"] <= C.RUN_MAX                                                     # k_cell_run_ranges
        if but != 5:
            assert sx * sy <= 2 ** 20                                                                  # :1476
        if but != 6:
            assert ns <= 2 ** 17                                                                       # :1476
        if but != 7:
            assert C.lds_bytes(w, h, 1 if gather and (w, h) != C.sizes(case) else 4) <= 64 * 1024      # :1533
    assert ns * sy * sx < 2 ** 32                                                                      # slice-grid indices are uint32


@pytest.mark.parametrize("name", C.NAMES)
def test_case_is_on_its_side_of_its_limit(name):
    case = C.build(name)
    P = case.problem
    ns, sy, sx = P.slices.shape
    beyond = case.side == "beyond"
    _other_limits_hold(case, but=case.limit if beyond else 0)
    L = _layout(case)
    if case.limit == 1:
        # :1546  for (k < 6) ok = ok && q[k] > -32000 && q[k] < 32000 -- CellRec::cx/cl/cz, CellRun::czmin/czmax are shorts
        k, axis = (1, 0) if "-x-" in name else (0, 4)                  # class 1's x bounds (an axial slice) / class 0's owned axis (the coronal stack)
        assert [C.owned_axis(P, s) for s in case.special] == [2 if k == 1 else 1] * len(case.special)
        lo = L["classes"][k]["q"][axis]
        assert lo <= -32100 if beyond else -31990 <= lo <= -31900
    elif case.limit == 2:
        # :1550-1554  pfirst = q[4] - NC; plast = min(q[5] + NH, v - 1); ng = plast - pfirst + 1; ok = ok && ng <= 1024 (items[] = cell << 10 | g)
        c = L["classes"][1]
        assert C.owned_axis(P, case.special[0]) == 2
        assert c["ng"] == min(c["q"][5] + NH, P.vsize[2] - 1) - (c["q"][4] - NC) + 1
        assert c["ng"] >= 1030 if beyond else (c["ng"] == 1024 if name.endswith("1024") else 1015 <= c["ng"] <= 1024)
    elif case.limit == 3:
        # :1548-1549, 1557, 1562  ncx = (q[1] - q[0]) / CX + 1; ncl = (q[3] - q[2]) / CL + 1; ncells = sum of ncx * ncl; ok = ok && ncells < 2^18
        assert C.sizes(case) == C.sizes(case, True) == (2, 2)
        assert all(c["ncx"] * c["ncl"] > 0 for c in L["classes"])      # both classes add up
        assert L["ncells"] >= 2 ** 18 if beyond else 0.9 * 2 ** 18 <= L["ncells"] < 2 ** 18
    elif case.limit == 4:
        # k_cell_run_ranges  cnt[q] counts the records of a run (one slice, one cell, one band of planes); cnt > CELL_RUN_MAX (16384) -> fallback
        assert ns == 1 and (P.slices != -1).all() and C.sizes(case) == (16, 16)
        c, _ = C.centres(P, 0)
        assert len(np.unique(c[:, 2])) == 1                            # one plane, so one band: the slice's pixels are ONE run ...
        assert L["ncells"] == 1 and L["most_per_cell"] == sx * sy      # ... and every centre falls in one cell
        assert sx * sy == (128 * 129 if beyond else C.RUN_MAX)
    elif case.limit == 5:
        # :1476  (uint64_t)sx * sy > (1u << 20) -> unusable; rem = key & 0xFFFFF (k_cell_records :233)
        assert sx * sy == (1025 * 1024 if beyond else 2 ** 20)
        live = np.argwhere(P.slices != -1)
        assert (live[:, 1] * sx + live[:, 2]).max() == sx * sy - 1     # the patch reaches the top of the position field
        assert len(live) > 300 and live[:, 1].min() == sy - 16 and live[:, 2].min() == sx - 16
    elif case.limit == 6:
        # :1476  ns > (1u << 17) -> unusable; slice = (key >> 29) & 0x1FFFF (k_cell_records :233, k_cell_runs :271)
        assert ns == (2 ** 17 + 1 if beyond else 2 ** 17) and (sy, sx) == (2, 2)
        live = np.flatnonzero((P.slices != -1).reshape(ns, -1).any(1))
        assert list(live) == [0, 1, 2, ns - 3, ns - 2, ns - 1]
    elif case.limit == 7:
        # :1527-1533  PL = (CX + NS - 1) | 1; DL = CL + NS - 1; PP = PL * DL; (scatter: 4 slots, a gather of its own: 1) * PP * sizeof(f2) > 64 KiB
        w, h = C.sizes(case)
        assert (w, h) == ((32, 32) if beyond else (26, 26))
        assert C.lds_bytes(w, h) > 64 * 1024 if beyond else C.lds_bytes(w, h) <= 64 * 1024
        if case.split_gather:
            assert C.sizes(case, True) == (16, 16) and C.lds_bytes(16, 16, 1) <= 64 * 1024
        else:
            assert C.sizes(case, True) == (w, h)                       # one set of lists for both passes: the gather falls back with the scatter


def _oracle_sample(P, sl, pix):
    from oracle import pyoracle
    orc = pyoracle.OracleReconstruction(P, pyoracle.CANON)
    return np.array([orc.tap_census(sl, int(px), int(py))[3] for px, py in pix]).astype(np.int64)


@pytest.mark.parametrize("name", C.NAMES)
def test_centres_are_the_oracles(name, oracle_mod):
    """the centre voxels the limits are worked out from, against the oracle's pixel_setup on the special slices (every pixel up to 256 per slice,
    else the corners, the extremes and a random sample)"""
    case = C.build(name)
    P = case.problem
    rng = np.random.default_rng(5)
    for sl in case.special:
        c, pix = C.centres(P, sl)
        pick = np.arange(len(c))
        if len(c) > 256:
            pick = np.unique(np.concatenate([[0, len(c) - 1], c.argmin(0), c.argmax(0), rng.integers(0, len(c), 64)]))
        assert np.array_equal(_oracle_sample(P, sl, pix[pick]), c[pick])


def _cmap(P, pyoracle):
    orc = pyoracle.OracleReconstruction(P, pyoracle.CANON)
    ones = np.ones(P.ns, np.float32)
    orc.UpdateScaleVector(ones, ones)
    orc.InitializeEMValues()
    orc.GaussianReconstruction()
    orc.weights[...] = orc.slices != -1
    orc.simslices[...] = np.where(orc.slices > 0, 0.9 * orc.slices, 0)
    orc.SuperresolutionBackproject(ones)
    return orc


@pytest.mark.parametrize("name", C.NAMES)
def test_special_slices_reach_the_volume_and_the_oracle_stays_finite(name, oracle_mod):
    case = C.build(name)
    P = case.problem
    if case.limit == 4:
        # the oracle needs several seconds for the 16 k pixels of this slice: a 16 x 16 patch of them stands in here
        P = copy.copy(P)
        P.slices = np.full_like(case.problem.slices, -1.0)
        P.slices[:, 56:72, 56:72] = case.problem.slices[:, 56:72, 56:72]
    full, without = _cmap(P, oracle_mod), _cmap(C.blanked(P, case.special), oracle_mod)
    for a in (full.recon, full.volw, full.psf_sums, full.addon, full.cmap):
        assert np.isfinite(a).all()
    changed = int((full.cmap != without.cmap).sum())
    assert changed >= 10, changed
    if case.limit in (1, 2, 3):
        # the moved slices lie below the volume on one or two axes: what they add, they add on its low faces (RC.cu:508)
        vx, vy, vz = P.vsize
        d = (full.cmap != without.cmap).reshape(vz, vy, vx)
        z, y, x = np.nonzero(d)
        face = {"centres-x": x, "centres-own": y, "planes": z}.get(name.rsplit("-", 1)[0] if not name.endswith("1024") else "planes")
        if case.limit == 3:
            assert not x.any() and not y.any()
        else:
            assert not face.any()
