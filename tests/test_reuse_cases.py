"""tests/reuse_cases.py reaches what tests/test_context_reuse_gpu.py relies on (no device)."""
import numpy as np

from tests import reuse_cases as cases


def _sizes(p):
    ns, sy, sx = p.slices.shape
    return ns, sy, sx, p.nvox


def test_the_shapes_are_the_ones_the_suite_names():
    want = {"A": ((24, 32, 32), 34, 1.0), "A2": ((24, 32, 32), 34, 1.0), "B": ((30, 36, 40), 46, 0.8), "C": ((10, 24, 20), 21, 1.2),
            "L16": ((40, 16, 16), 28, 1.0), "L8": ((184, 8, 8), 28, 1.0), "L12x8": ((133, 8, 12), 28, 1.0)}
    for name, (grid, nv, res) in want.items():
        p = cases.get(name)
        assert p.slices.shape == grid and tuple(p.vsize) == (nv,) * 3 and np.allclose(p.vdim, res), (name, p.slices.shape, p.vsize, p.vdim)
        assert p.mask.size == nv ** 3 and (p.slices > 0).any()


def test_b_exceeds_a_and_c_falls_below_it_on_every_axis():
    a, b, c = (_sizes(cases.get(k)) for k in "ABC")
    assert all(y > x for x, y in zip(a, b)) and all(y < x for x, y in zip(a, c))


def test_b_alone_is_below_the_density_at_which_the_gather_changes_tiles():
    d = {k: cases.density(cases.get(k)) for k in "ABC"}
    assert d["B"] < cases.TILE_RULE_DENSITY < min(d["A"], d["C"]), d
    assert abs(d["A"] - 0.83) < 0.01 and abs(d["B"] - 0.53) < 0.01


def test_a2_has_the_shapes_of_a_and_other_content():
    a, a2 = cases.get("A"), cases.get("A2")
    assert _sizes(a) == _sizes(a2) and np.array_equal(a.mask, a2.mask) and np.array_equal(a.recon_w2i, a2.recon_w2i)
    assert not np.array_equal(a.slices, a2.slices) and not np.array_equal(a.slice_t, a2.slice_t)
    assert not np.array_equal(a.slices != -1, a2.slices != -1)                    # another active set, not only other values


def test_the_patch_levels_share_the_volume_and_differ_in_the_patches():
    lv = [cases.get(k) for k in cases.PVR_LEVELS]
    for p in lv[1:]:
        assert tuple(p.vsize) == tuple(lv[0].vsize) and np.array_equal(p.mask, lv[0].mask) and np.array_equal(p.recon_i2w, lv[0].recon_i2w)
    assert len({p.ns for p in lv}) == 3 and len({p.slices.shape[1:] for p in lv}) == 3
    assert lv[0].ns < lv[2].ns < lv[1].ns                                         # fewer large patches, then many small ones
    sy, sx = lv[2].slices.shape[1:]
    assert sx != sy                                                               # the non-square level


def test_stale_masks_would_be_read_inside_their_allocation():
    """masks, then none: the second grid has no more patches than the first and both are at most 64 wide, so a context that
    kept the first grid's masks reads inside what it allocated -- a wrong result, never an out-of-range read"""
    first, second = cases.get("L8"), cases.get("L16")
    assert second.ns <= first.ns
    for p in (first, second):
        assert max(p.slices.shape[1:]) <= 64
    m = cases.spx(first)
    assert m.shape == (first.ns, 4096) and set(np.unique(m)) == {ord("0"), ord("1")}
    ns, sy, sx = second.slices.shape
    stale = m.reshape(-1, 64, 64)[:ns, :sy, :sx] == ord("0")
    assert (stale & (second.slices != -1)).sum() > 100                            # stale masks would switch active pixels off


def test_the_partial_upload_problems_mix_what_they_say():
    a, b = cases.get("A"), cases.get("B")
    for radius in (12.0, 17.0):
        g = cases.volume_grid(radius)
        q = cases.with_volume_of(a, g)
        assert q.slices is a.slices and q.mask is g.mask and tuple(q.vsize) == tuple(g.vsize) != tuple(a.vsize) and np.allclose(q.vdim, a.vdim)
    assert cases.volume_grid(12.0).nvox < a.nvox < cases.volume_grid(17.0).nvox
    q = cases.with_slices_of(a, b)
    assert q.slices is b.slices and q.mask is a.mask and q.slice_t is b.slice_t
    m = cases.with_mask(a, 10.0)
    assert m.mask.shape == a.mask.shape and 0 < m.mask.sum() < a.mask.sum() and not (m.mask > a.mask).any()
    assert np.array_equal(cases.with_mask(a, 14.0).mask, a.mask)                  # the same rule as make_problem's


def test_inputs_are_fixed_and_cover_the_active_pixels():
    a = cases.get("A")
    x, y = cases.inputs(a), cases.inputs(a)
    assert all(np.array_equal(x[k], y[k]) for k in x) and not np.array_equal(x["w"], cases.inputs(a, 12)["w"])
    on = a.slices != -1
    assert (x["w"][on] > 0).all() and (x["w"][~on] == 0).all() and x["vol"].size == a.nvox
