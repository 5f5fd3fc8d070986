"""The support-16 table scatter's register ring (back_cell_kernel<16, false, 1>) at the shapes where a ring can go wrong.

The kernel keeps two units per slot in flight in registers that it loads and waits for itself; every trip of its unit loop uses ring entry 0,
then entry 1, and lanes without a unit load the table's first bytes.  Each case cuts one slice of the tiny problem down to the few pixels that
make one run of a known length (cell_stats says so: one run, that many sorted pixels; a run deals its records to the four slots in turn, record
i to slot i mod 4), scatters it once from the coefficient table (coeff_table 1, back_mode 5: the first pass writes the table, the second one
streams it) and once with every tap evaluated (coeff_table 0) in the same build, and asks for the same bits of addon and the confidence map."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SLICE = 3            # an axial slice near the middle of the first stack: rows along x, lanes along y, planes along z
CELL = dict(cell_w=16, cell_h=16, cell_band=6)   # cells of 16 x 16 voxels from the first centre on, all planes in one band: a small block is ONE run


def cut(tiny, keep, tilt_deg=0.0):
    """slice SLICE of the tiny problem with the pixels of `keep` ([sy][sx] bool) and no others; tilt_deg: turned about the world's x axis"""
    from fetalreconstruction_amd import geometry as geo
    from fetalreconstruction_amd import phantom
    q = phantom.sub_problem(tiny, SLICE, SLICE + 1)
    s = q.slices[0]
    q.slices = np.where(keep, np.where(s > 0, s, np.float32(500.0)), np.float32(-1.0)).astype(np.float32)[None]
    if tilt_deg:
        t = geo.rigid_matrix(rx=tilt_deg) @ q.slice_t[0].astype(np.float64).reshape(4, 4)
        q.slice_t = geo.to_matrix4(t)[None]
        q.slice_tinv = geo.to_matrix4(np.linalg.inv(t))[None]
    return q


def block(x0, x1, y0, y1):
    keep = np.zeros((32, 32), bool)
    keep[y0:y1, x0:x1] = True
    return keep


def scatter_both_ways(prob, weight_of=None):
    """-> ([addon, cmap] from the table, the same with every tap evaluated, unit_counts, cell_stats)"""
    from fetalreconstruction_amd import engine as E
    rng = np.random.default_rng(5)
    on = prob.slices != -1
    ones = np.ones(prob.ns, np.float32)
    psf = np.where(on, rng.uniform(0.5, 1.5, on.shape), 0).astype(np.float32)
    w = np.where(on, rng.uniform(0.2, 1.0, on.shape), 0).astype(np.float32)
    if weight_of is not None:
        w = weight_of(w)
    sim = np.where(on, prob.slices * rng.uniform(0.8, 1.2, on.shape), 0).astype(np.float32)
    out = {}
    for table in (0, 1):
        rec = E.Reconstruction(0)
        E.sync_gpu(rec, prob)
        rec.timer_enable(True)
        rec.set_option("coeff_table", table)
        rec.set_option("back_mode", 5)
        for k, v in CELL.items():
            rec.set_option(k, v)
        rec.UpdateScaleVector(ones, ones)
        rec.debug_set(E.BUF_PSF_SUMS, psf)
        for _ in range(1 + table):                           # (the table's first pass evaluates and writes it)
            rec.debug_set(E.BUF_SIMSLICES, sim)
            rec.debug_set(E.BUF_WEIGHTS, w)
            rec.SuperresolutionBackproject(ones)
        out[table] = [rec.debug_get(b).copy() for b in (E.BUF_ADDON, E.BUF_CONFIDENCE_MAP)]
        tm = rec.timers()
        assert (tm["backproject_store"][1], tm["backproject_table"][1]) == (table, table), tm
        assert rec.get_option("back_mode") == 5 and not any(rec.fallbacks().values()), rec.fallbacks()
        units, cells = rec.unit_counts(), rec.cell_stats()
        rec.close()
    return out[1], out[0], units, cells


def check(prob, pixels, weight_of=None, runs=1):
    got, want, units, cells = scatter_both_ways(prob, weight_of)
    print(units, cells)
    assert cells["sorted_pixels"] == pixels and cells["runs"] == runs, cells          # the shape the case is about
    assert units["live_units"] >= 1, units                                             # ... and it streamed the table
    assert np.any(want[0] != 0) and np.any(want[1] != 0)
    for k, name in enumerate(("addon", "confidence map")):
        assert np.array_equal(got[k], want[k]), (name, int(np.sum(got[k] != want[k])))
    return units


def test_one_pixel(tiny):
    """(a) one slice with one active pixel: one unit in one slot per plane, ring entry 1 never holds a unit"""
    check(cut(tiny, block(16, 17, 16, 17)), 1)


def test_two_and_three_units_per_slot(tiny):
    """(b) a run of 11 pixels: slots 0..2 take three records, slot 3 two -- the odd tail (the last trip has entry 0 only) next to the even one"""
    check(cut(tiny, block(10, 21, 16, 17)), 11)


def test_run_of_65_pixels(tiny):
    """(c) 65 pixels in one cell, one more than SlotGeom<16>::CH: the second chunk holds ONE record, 63 lanes load the table's first bytes"""
    check(cut(tiny, block(10, 23, 14, 19)), 65)


def test_dead_units_in_one_slot_live_in_another(tiny):
    """(d) two pixels of a slice tilted by 8 degrees, 7.7 mm apart along the lanes: each has dead units at both ends of its 16, and their
    distances to a plane differ by 1.07 voxels, so the planes where the live units end hold a dead unit of one pixel (slot 0 or 1: the dead-unit
    loop only) and a live unit of the other (the ring)"""
    keep = block(16, 17, 12, 13) | block(16, 17, 19, 20)
    units = check(cut(tiny, keep, tilt_deg=8.0), 2)
    assert units["dead_units"] >= 4, units


def test_rows_beyond_the_far_edge(tiny):
    """(e) pixels whose centres lie 2..8 voxels from the volume's last y (the lane axis of an axial slice; outside the mask, whose voxels their
    footprints still reach): the footprint's upper rows are off the volume, rowok is false in those lanes"""
    check(cut(tiny, block(12, 20, 26, 30)), 32)


def test_every_second_pixel_at_weight_zero(tiny):
    """(f) records whose factors are both 0 are not active: they must not take a place in the ring or shift their neighbours'"""
    def weight_of(w):
        w = w.copy()
        w[..., 1::2] = 0.0
        return w
    check(cut(tiny, block(12, 20, 12, 20)), 64, weight_of)
