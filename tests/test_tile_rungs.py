"""tests/tile_rungs.py on the CPU: the fit rules against boxes worked out by hand, and the conditions its cases have to meet before the device
runs them (tests/test_tile_rungs_gpu.py) -- every rung a case is meant to reach holds a tile, and an impulse, for both sizes tile_cap can take;
the counts the device is held to exactly hold no undecided tile."""
import numpy as np
import pytest

from tests import cell_limit_cases as C
from tests import operator_entries as O
from tests import tile_rungs as T

V96 = (96, 96, 96)
# the cases whose slot rejects the device is held to EXACTLY where tile_cap is 18304 (the MI355X); the others are asserted as an interval
INTERVAL_AT_18304 = ("coarse-16-4x4", "coarse-16-4x4-table", "coarse-16-8x8", "coarse-16-8x8-table")


def test_boxes_by_hand():
    """three tiles of the coarse problem, with pencil and paper from the kernels' text"""
    # one pixel, axial (the slice owns z), centre (48, 48, 48): 16 taps an axis
    c = np.array([[48, 48, 48]])
    b = T.plane_box(c, 2, V96, False)
    assert b == dict(Dy=16, Dz=16, PL=17, PD=1, PP=272, used=16)
    assert T.wave_rejects(b, 1024, 4, False) and not T.wave_rejects(b, 2096, 4, False)        # 4 * 272 = 1088
    assert T.wave_rejects(b, 2096, 64, False) and not T.wave_rejects(b, 2096, 64, True)       # 64 pixels: with the table only
    assert T.slot_verdict(b, 6016, False) == "fit"                                            # 16 * 272 = 4352
    assert T.tiled_box(c, V96) == (272, 16)                                                   # ((17 * 16 + 15) & ~31) + 16
    assert T.unit_box(c, V96, False) == 273 * 16                                              # 17 * 16 made odd
    assert T.plane_box(c, 2, V96, True) == dict(Dy=12, Dz=12, PL=13, PD=1, PP=156, used=12)   # support 12: NC 5, NH 6
    # 2 x 2 pixels of 6.3 mm at the volume's low corner: x 7..13, y 7..14
    c = np.array([[7, 7, 48], [13, 7, 48], [7, 14, 48], [13, 14, 48]])
    b = T.plane_box(c, 2, V96, False)
    assert b == dict(Dy=23, Dz=16, PL=23, PD=7, PP=529, used=16)
    assert T.wave_rejects(b, 2096, 4, False) and not T.wave_rejects(b, 3696, 4, True)         # 4 * 529 = 2116
    assert T.slot_verdict(b, 18304, False) == "fit" and T.slot_verdict(b, 6016, False) == "undecided"    # 2576 .. 8464
    assert T.slot_verdict(b, 2000, False) == "reject"
    assert T.tiled_box(c, V96) == (560, 16)                                                   # Px 23, 23 * 23 = 529 -> 544 + 16
    assert T.rung(c, 2, V96, False, 4, 2096, 18304, False) == "slot" and T.rung(c, 2, V96, False, 4, 2096, 18304, True) == "large"
    assert T.rung(c, 2, V96, False, 4, 2096, 6016, False) == "slot?"
    # eight pixels in a line down the owned axis y from 8 to -36: the slot kernel's box starts at -43, the saturated one at 0
    c = np.array([[48, int(np.floor(8 - 6.3 * k + 0.5)), 45] for k in range(8)])
    assert c[:, 1].min() == -36
    b = T.plane_box(c, 1, V96, False)
    assert (b["Dz"], b["Dy"], b["PL"], b["PP"]) == (60, 16, 17, 272)
    assert T.slot_verdict(b, 18304, False) == "reject"                                        # 60 > SLOT_MAXP
    assert not T.wave_rejects(b, 2096, 32, False) and T.wave_rejects(b, 2096, 64, False)      # (60 <= 64 planes)
    assert T.tiled_box(c, V96) == (304, 16)                                                   # y 0..16: 17 * 17 = 289 -> 288 + 16
    assert T.rung(c, 1, V96, False, 64, 2096, 6016, False) == "last-lds" and T.rung(c, 1, V96, True, 64, 2096, 6016, False) == "last-pvr"
    # the high face caps the box, a footprint that starts beyond it leaves nothing
    assert T.plane_box(np.array([[48, 48, 93]]), 2, V96, False)["Dz"] == 10
    assert T.plane_box(np.array([[48, 48, 103]]), 2, V96, False) is None and T.rung(np.array([[104, 48, 48]]), 2, V96, False, 4, 2096, 6016, False) == "out"
    assert T.unit_box(np.array([[48, 48, 93]]), V96, False) == 273 * 10


def test_the_coarse_problem_is_what_the_cases_need():
    P = O.problem("coarse")
    assert P.vsize == V96 and P.mask.all() and P.slices.shape == (4, 14, 14)
    kinds = [k for k, _ in O._slice_classes("coarse")]
    assert kinds[0] == "axial" and kinds[1] == "coronal" and C.owned_axis(P, 1) == 1 and kinds[2].startswith("sagittal")
    d = float(P.slice_dim[0, 0]) / float(P.vdim[0])
    assert 6.0 <= d <= 6.5                                             # voxels per pixel
    c, xy = C.centres(P, 2)                                            # a tile's centres span more than 32 planes of the owned axis
    tile = (xy[:, 0] < 8) & (xy[:, 1] < 8)
    assert np.ptp(c[tile, C.owned_axis(P, 2)]) > 32
    c, _ = C.centres(P, 3)                                             # the line of the last slice hangs below the low face
    assert len(c) == 14 and c[:, C.owned_axis(P, 3)].min() < -30


@pytest.mark.parametrize("case", list(T.SCATTER_CASES))
def test_scatter_cases_reach_their_rungs(case):
    name, pvr, tile, wave_cap, table, reach = T.SCATTER_CASES[case]
    sets, _ = T.pixel_sets(name, pvr)
    impulses = {p for s in sets for p in s}
    assert set(reach) == set(T.TILE_CAPS)
    for cap in T.TILE_CAPS:
        cen = T.scatter_census(case, cap)
        print(case, cap, {r: n for r, n in cen["tiles"].items() if n}, "rerun", cen["rerun"], "slot rejects", cen["fallback"])
        for r in reach[cap]:
            assert cen["tiles"][r] > 0 and len(cen["pixels"][r]) > 0, (case, cap, r)
            assert cen["pixels"][r] & impulses, (case, cap, r, "no impulse in a tile of this rung")
        assert sum(cen["tiles"].values()) == len(T.tiles(O.problem(name), *tile))
        if pvr:
            assert cen["tiles"]["slot?"] == 0                           # no dead units: the slot rule is exact
    if case not in INTERVAL_AT_18304:
        lo, hi = T.scatter_census(case, 18304)["fallback"]
        assert lo == hi


def test_the_coarse_cases_cover_the_ladder():
    """support 16: rung 1, the large-box pass, the slot kernel and the last resort with the box in the LDS and without, for either tile_cap; support 12:
    the slot kernel and pvr_tiles_kernel"""
    for cap in T.TILE_CAPS:
        for pvr, want in ((False, {"wave", "large", "slot", "last-lds", "last-mem"}), (True, {"slot", "last-pvr"})):
            have = set()
            for case, (name, v, _, _, _, reach) in T.SCATTER_CASES.items():
                if name == "coarse" and v == pvr:
                    have |= set(reach[cap])
            assert want <= have, (cap, pvr, want - have)


@pytest.mark.parametrize("name,pvr", [(n, v) for n in O.PROBLEMS + O.RUNG_PROBLEMS for v in (False, True)])
def test_rung_sets_keep_the_impulse_design(name, pvr):
    """no voxel receives more than two terms; the problem's classes stay covered; the sets are those of operator_entries where they reach every rung already"""
    sets, classes = T.pixel_sets(name, pvr)
    if not T.rung_pixels(name, pvr):
        assert sets == O.impulse_pixel_sets(name, pvr)[0]
    for s in sets + T.gauss_pairs(name, pvr):
        assert O.terms_per_voxel(name, pvr, s).max() <= 2
    have = set().union(*classes.values())
    assert not [c for c in O.REQUIRED[name] if c not in have], sorted(have)
    print(name, pvr, [len(s) for s in sets], "placed first:", T.rung_pixels(name, pvr))


@pytest.mark.parametrize("case", list(T.GAUSS_CASES))
def test_gauss_sets_reach_their_rungs(case):
    """pass 2 runs on copies where only a set's pixels are live: the union of the rungs its sets reach"""
    name, pvr = T.SCATTER_CASES[case][:2]
    for cap in T.TILE_CAPS:
        have = set()
        for s in T.gauss_sets(name, pvr):
            cen = T.scatter_census(case, cap, O.indicator(name, s))
            assert cen["tiles"]["slot?"] == 0 or name == "coarse", (case, cap, s)
            have |= {r for r, n in cen["tiles"].items() if n}
        assert set(T.GAUSS_CASES[case][cap]) <= have, (case, cap, have)


@pytest.mark.parametrize("case", list(T.GATHER_CASES))
def test_gather_cases_reach_their_arms(case):
    name, pvr, cap, kind, arms = T.GATHER_CASES[case]
    vsets, _ = O.impulse_voxel_sets(name, pvr)
    P = O.problem(name)
    reached = np.zeros(P.slices.shape, bool)
    for v in vsets:
        reached |= O.contributing(name, pvr, v)
    for tile_cap in T.TILE_CAPS:
        for gauss1 in (False, True):
            cen = T.gather_case_census(case, tile_cap, gauss1)
            print(case, tile_cap, "pass 1" if gauss1 else "gather", cen["tiles"])
            for arm in arms:
                assert cen["tiles"][arm] > 0
                assert gauss1 or any(reached[sl, py, px] for sl, px, py in cen["pixels"][arm]), (case, arm)


def test_terms_folded_counts_every_tap():
    """on the coarse problem: at least terms_bound's count where nothing folds, the whole folded row where a slice hangs below the face, and never fewer
    than the oracle's own kept taps"""
    for pvr in (False, True):
        n = O.terms_folded("coarse", pvr)
        s = O.support(pvr)
        assert n.sum() == sum(np.prod([np.count_nonzero(np.maximum(c + np.arange(-O.first_tap(pvr), O.first_tap(pvr) + 2), 0) < 96) for c in row[3:]])
                              for row in O._pool("coarse"))
        assert n.max() > s                                             # the line below the low face
        sets, _ = T.pixel_sets("coarse", pvr)
        assert np.all(O.terms_per_voxel("coarse", pvr, sets[0]) <= n)
        assert O.fold_terms("coarse", pvr).max() >= s and O.fold_terms("coarse", pvr)[0].max() == 1
