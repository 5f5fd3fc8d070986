"""The engine context's invalidation map (csrc/svr_hip.hip: enum Change, invalidate) driven through the public API.

Every input a caller can change raises one change; the read-only options psf_list_valid, cells_valid and coeff_state show what it left
standing.  For the slice-pixel, PSF-sum, slice-geometry and cell-shape changes, the next gather and scatter (cell path, coefficient
table on) must also give the bits of a fresh context handed the same inputs: a cache the map failed to drop would show up there."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _state(rec):
    return (rec.get_option("psf_list_valid"), rec.get_option("cells_valid"), rec.get_option("coeff_state"))


def _inputs(P):
    """what the passes read besides the problem: fixed v_PSF_sums, volume, weights and simulated slices"""
    rng = np.random.default_rng(11)
    on = P.slices != -1
    return {
        "psf": np.where(on, rng.uniform(0.5, 1.5, P.slices.shape), 0).astype(np.float32),
        "vol": rng.uniform(0.5, 1.5, P.mask.size).astype(np.float32),
        "w": np.where(on, rng.uniform(0.2, 1.0, P.slices.shape), 0).astype(np.float32),
        "sim": np.where(P.slices > 0, P.slices * rng.uniform(0.8, 1.2, P.slices.shape), 0).astype(np.float32),
    }


def _context(P, X, **options):
    from fetalreconstruction_amd import engine as E
    rec = E.Reconstruction(0)
    for k, v in options.items():
        rec.set_option(k, v)
    E.sync_gpu(rec, P)
    ones = np.ones(P.ns, np.float32)
    rec.UpdateScaleVector(ones, ones)
    rec.debug_set(E.BUF_PSF_SUMS, X["psf"])
    rec.debug_set(E.BUF_RECONSTRUCTED, X["vol"])
    return rec


def _passes(rec, X):
    """one gather and one scatter from the same inputs every time"""
    from fetalreconstruction_amd import engine as E
    shape = X["sim"].shape
    rec.debug_set(E.BUF_SIMSLICES, np.zeros(shape, np.float32))
    rec.debug_set(E.BUF_SIMWEIGHTS, np.zeros(shape, np.float32))
    rec.debug_set(E.BUF_SIMINSIDE, np.zeros(shape, np.uint8))
    rec.SimulateSlices()
    out = [rec.debug_get(b).copy() for b in (E.BUF_SIMSLICES, E.BUF_SIMWEIGHTS, E.BUF_SIMINSIDE)]
    rec.debug_set(E.BUF_SIMSLICES, X["sim"])
    rec.debug_set(E.BUF_WEIGHTS, X["w"])
    rec.SuperresolutionBackproject(np.ones(X["sim"].shape[0], np.float32))
    out += [rec.debug_get(b).copy() for b in (E.BUF_ADDON, E.BUF_CONFIDENCE_MAP)]
    return out


def _same(a, b):
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y, equal_nan=True), k


def _moved(P):
    """the tiny problem with every slice shifted by a fraction of a voxel"""
    Q = copy.copy(P)
    T = P.slice_t.reshape(-1, 4, 4).astype(np.float64).copy()
    T[:, 0, 3] += 0.37
    T[:, 1, 3] -= 0.21
    Q.slice_t = T.reshape(P.slice_t.shape).astype(P.slice_t.dtype)
    Q.slice_tinv = np.linalg.inv(T).reshape(P.slice_tinv.shape).astype(P.slice_tinv.dtype)
    return Q


def _set_matrices(rec, P):
    rec.SetSliceMatrices(P.slice_t, P.slice_tinv, P.slice_i2w, P.slice_w2i, P.slice_i2w, P.slice_w2i, P.recon_i2w, P.recon_w2i)


def test_the_passes_build_what_they_read(tiny):
    X = _inputs(tiny)
    rec = _context(tiny, X)
    assert _state(rec) == (0, 0, 0)
    _passes(rec, X)
    assert _state(rec) == (1, 1, 1)                          # the gather wrote the table (coeff_lazy): its PSF pixels
    assert rec.get_option("coeff_valid") == 1
    rec.close()


def test_new_slice_pixels_drop_the_list_the_cells_and_the_table(tiny):
    from fetalreconstruction_amd import engine as E
    X = _inputs(tiny)
    P = copy.copy(tiny)
    rng = np.random.default_rng(5)
    P.slices = tiny.slices.copy()
    on = np.argwhere(tiny.slices != -1)
    drop = on[rng.choice(len(on), len(on) // 10, replace=False)]
    P.slices[tuple(drop.T)] = -1                               # pixels leave the active set ...
    P.slices[P.slices > 0] *= np.float32(1.1)                  # ... and the rest change value
    rec = _context(tiny, X)
    _passes(rec, X)
    rec.FillSlices(P.slices, P.sizes_x, P.sizes_y)
    assert _state(rec) == (0, 0, 0)
    got = _passes(rec, X)
    ref = _context(P, X)
    _same(got, _passes(ref, X))
    ref.close()
    rec.debug_set(E.BUF_SLICES, tiny.slices)                   # the debug path: the same change
    assert _state(rec) == (0, 0, 0)
    ref = _context(tiny, X)
    _same(_passes(rec, X), _passes(ref, X))
    ref.close()
    rec.close()


def test_new_psf_sums_drop_a_table_of_psf_pixels(tiny):
    from fetalreconstruction_amd import engine as E
    X = _inputs(tiny)
    Y = dict(X)
    psf = X["psf"].copy()
    psf[:, ::3, :] = 0                                         # a third of the rows leave the PSF list ...
    Y["psf"] = psf
    rec = _context(tiny, Y)
    _passes(rec, Y)
    assert _state(rec) == (1, 1, 1)                            # a table of the PSF pixels of a third fewer rows
    rec.debug_set(E.BUF_PSF_SUMS, X["psf"])                    # ... and come back: the table does not hold them
    assert _state(rec) == (0, 1, 0)
    got = _passes(rec, X)
    assert _state(rec) == (1, 1, 1)
    ref = _context(tiny, X)
    _same(got, _passes(ref, X))
    ref.close()
    rec.close()


def test_a_full_table_outlives_new_psf_sums_but_not_new_slices(tiny):
    from fetalreconstruction_amd import engine as E
    X = _inputs(tiny)
    rec = _context(tiny, X, coeff_lazy=0)
    _passes(rec, X)
    assert _state(rec) == (1, 1, 2)                            # k_coeff_build: every active pixel
    rec.debug_set(E.BUF_PSF_SUMS, X["psf"] * np.float32(0.5))
    assert _state(rec) == (0, 1, 2)
    _passes(rec, X)
    assert _state(rec)[2] == 2
    rec.debug_set(E.BUF_SLICES, tiny.slices)
    assert _state(rec) == (0, 0, 0)
    rec.close()


def test_the_gaussian_pass_leaves_a_table_of_its_psf_pixels(tiny):
    """new v_PSF_sums: pass 2 writes the table when none is there, a table of an earlier pass's PSF pixels goes, a full one stays"""
    X = _inputs(tiny)
    for lazy, earlier, after in ((1, False, 1), (1, True, 0), (0, False, 2), (0, True, 2)):
        rec = _context(tiny, X, coeff_lazy=lazy)
        if earlier:
            _passes(rec, X)
        rec.InitializeEMValues()
        rec.GaussianReconstruction()
        assert _state(rec) == (1, 1, after), (lazy, earlier)
        rec.close()


def test_new_slice_geometry_is_taken_by_the_next_pass(tiny):
    X = _inputs(tiny)
    P = _moved(tiny)
    rec = _context(tiny, X)
    rec.timer_enable(True)
    _passes(rec, X)
    stores = rec.timers()["forward_store"][1]
    _set_matrices(rec, P)
    assert _state(rec) == (1, 1, 1)                            # (lazy: the slice constants are rebuilt by the next pass, which drops the rest)
    got = _passes(rec, X)
    assert _state(rec) == (1, 1, 1) and rec.timers()["forward_store"][1] == stores + 1
    ref = _context(P, X)
    _same(got, _passes(ref, X))
    ref.close()
    rec.setSliceDims(tiny.slice_dim, 2.0)
    assert _state(rec) == (1, 1, 1)
    _passes(rec, X)
    assert rec.timers()["forward_store"][1] == stores + 2
    rec.close()


def test_a_new_psf_volume_drops_the_cells_and_the_table(tiny):
    from fetalreconstruction_amd import geometry as geo
    X = _inputs(tiny)
    rec = _context(tiny, X)
    _passes(rec, X)
    a = geo.ImageAttributes(128, 128, 128, *[float(d) for d in tiny.vdim])
    rec.generatePSFVolume(None, (128, 128, 128), tuple(tiny.slice_dim[0]), tiny.vdim, geo.to_matrix4(geo.image_to_world(a)),
                          geo.to_matrix4(geo.world_to_image(a)), 2.0)
    assert _state(rec) == (1, 0, 0)
    rec.close()


def test_a_new_cell_shape_drops_the_cells_and_keeps_the_table(tiny):
    X = _inputs(tiny)
    for name in ("cell_w", "cell_h", "cell_gw", "cell_band", "cell_order", "cell_balance", "cell_split", "cell_qx"):
        value = {"cell_band": 2, "cell_order": 0, "cell_balance": 4, "cell_split": 2, "cell_qx": 2}.get(name, 6)
        rec = _context(tiny, X)
        _passes(rec, X)
        rec.set_option(name, value)
        assert _state(rec) == (1, 0, 1), name
        got = _passes(rec, X)
        assert _state(rec) == (1, 1, 1), name
        if name in ("cell_w", "cell_gw", "cell_order"):
            ref = _context(tiny, X, **{name: value})
            _same(got, _passes(ref, X))
            ref.close()
        rec.close()


def test_tile_shapes_drop_the_psf_list(tiny):
    X = _inputs(tiny)
    rec = _context(tiny, X)
    _passes(rec, X)
    for name, value in (("tile_w", 2), ("fwd_tile_w", 2)):
        rec.set_option(name, value)
        assert _state(rec) == (0, 1, 1), name
        _passes(rec, X)
        assert _state(rec) == (1, 1, 1), name
    rec.close()


def test_the_table_options(tiny):
    X = _inputs(tiny)
    rec = _context(tiny, X)
    _passes(rec, X)
    rec.set_option("coeff_invalidate", 1)
    assert _state(rec) == (1, 1, 0) and rec.get_option("coeff_valid") == 0
    _passes(rec, X)
    assert _state(rec) == (1, 1, 1)
    rec.set_option("coeff_table", 0)
    assert _state(rec) == (1, 0, 0)
    _passes(rec, X)
    assert _state(rec) == (1, 1, 0)
    rec.set_option("coeff_table", 1)
    _passes(rec, X)
    assert _state(rec) == (1, 1, 1)
    rec.close()


def test_new_volume_and_storage_drop_everything_slice_derived(tiny):
    X = _inputs(tiny)
    rec = _context(tiny, X)
    _passes(rec, X)
    rec.InitReconstructionVolume(tiny.vsize, tiny.vdim, None, 12.0)
    assert _state(rec) == (1, 0, 0)
    rec.close()
    rec = _context(tiny, X)
    _passes(rec, X)
    ns, sy, sx = tiny.slices.shape
    rec.initStorageVolumes((sx, sy, ns), tuple(tiny.slice_dim[0]))
    assert _state(rec) == (0, 0, 0)
    rec.close()


def test_the_volume_side_changes_leave_the_slice_side_alone(tiny):
    from fetalreconstruction_amd import engine as E
    X = _inputs(tiny)
    rec = _context(tiny, X)
    got = _passes(rec, X)
    rec.setMask(tiny.vsize, tiny.vdim, tiny.mask, 12.0)
    for b, v in ((E.BUF_MASK, tiny.mask), (E.BUF_RECONSTRUCTED, X["vol"]), (E.BUF_ADDON, got[3]), (E.BUF_CONFIDENCE_MAP, got[4])):
        rec.debug_set(b, v)
    rec.set_option("fwd_autotune", 0)
    assert _state(rec) == (1, 1, 1)
    _same(_passes(rec, X), got)
    rec.close()
