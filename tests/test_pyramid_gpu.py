"""The device pyramid (csrc/svr_pyr.inc: k_pyr_blur, k_pyr_resample, k_pyr_range, k_pyr_shift behind svr_pyr_level) level by
level against the independent numpy reference of tests/pyramid_ref.py, at the shapes of tests/pyramid_cases.py: the buffers
svr_ncc_evaluate reads are copied back and compared as int16, exactly, with the returned min / max.  For the target planes
the whole allocation is compared, so pitch borders, the planes before first_plane and the planes behind the last image must
still hold the -1 of svr_ncc_alloc_targets."""
import numpy as np
import pytest

from fetalreconstruction_amd import geometry as geo
from fetalreconstruction_amd import host, phantom

import pyramid_cases as cases
import pyramid_ref as ref

pytestmark = pytest.mark.gpu

JUNK = 7            # elements in front of the images in the upload slot: svr_pyr_level's `offset`


@pytest.fixture(scope="module")
def rec():
    from fetalreconstruction_amd import engine
    r = engine.Reconstruction(0)
    yield r
    r.close()


def _upload(rec, c):
    flat = c.images.reshape(-1)
    if c.slot == 0:
        rec.pyr_upload(0, flat)
        return 0
    rec.pyr_upload(1, np.concatenate([np.full(JUNK, 12345, np.int16), flat]))
    return JUNK


def _device_level(rec, c, k, offset):
    """step k of case c on the device -> (min, max, the buffer read back, the same buffer according to the reference)"""
    s = c.steps[k]
    rs = c.resamples(s)
    a0 = c.attrs[0]
    out_attrs = [ref.resampled_attr(a, s.res) if rs else a for a in c.attrs]
    o = out_attrs[0]
    n = len(c.pads)
    expect = c.reference(k)
    if c.slot == 1:
        tx, ty, planes = c.tx or o.nx, c.ty or o.ny, c.first_plane + n * o.nz + 2
        rec.ncc_alloc_targets(planes, tx, ty)
        want = np.full((planes, ty, tx), -1, np.int16)
        for i, e in enumerate(expect):
            want[c.first_plane + i * o.nz: c.first_plane + (i + 1) * o.nz, :o.ny, :o.nx] = e[0]
    else:
        want = expect[0][0]
    mn, mx = rec.pyr_level(c.slot, offset, (a0.nx, a0.ny, a0.nz), c.kernels(s), rs, (o.nx, o.ny, o.nz),
                           [geo.image_to_world(a) for a in out_attrs], [geo.world_to_image(a) for a in c.attrs], c.pads, c.first_plane)
    got = rec.ncc_get_targets() if c.slot == 1 else rec.ncc_get_source()
    return mn, mx, got, want


@pytest.mark.parametrize("name", cases.NAMES)
def test_device_level_is_the_reference(rec, name):
    c = cases.get(name)
    offset = _upload(rec, c)
    for k, s in enumerate(c.steps):
        mn, mx, got, want = _device_level(rec, c, k, offset)
        expect = c.reference(k)
        what = (name, "level", s.level, "axes", s.axes, "resample", c.resamples(s))
        assert list(mn) == [e[2] for e in expect] and list(mx) == [e[3] for e in expect], what
        assert got.shape == want.shape, what                                 # slot 0: reg_vx / vy / vz follow the level
        bad = np.argwhere(got != want)
        assert bad.size == 0, (*what, len(bad), "voxels differ, the first at [plane, y, x]", bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))


def test_empty_image_leaves_its_neighbours_alone(rec):
    """an image with nothing above its padding: min 32767 > max -32768 and planes of -1; the images around it in the same launch
    are the ones they are when they are processed alone"""
    c = cases.get("nothing_above_padding")
    offset = _upload(rec, c)
    for k in range(len(c.steps)):
        mn, mx, got, want = _device_level(rec, c, k, offset)
        assert (mn[1], mx[1]) == (32767, -32768) and (got[1] == -1).all()
        assert mn[2] == mx[2] == 1024 and sorted(set(got[2].ravel())) == [-1, 0]
        assert np.array_equal(got, want)
        for i in (0, 3):
            alone = ref.prepare_level(c.images[i], c.attrs[i], c.kernels(c.steps[k]), c.resamples(c.steps[k]), c.steps[k].res, c.pads[i])
            assert (mn[i], mx[i]) == alone[2:] and np.array_equal(got[i, :alone[0].shape[1], :alone[0].shape[2]], alone[0][0])


def test_read_back_refuses_without_a_buffer_and_changes_nothing():
    from fetalreconstruction_amd import engine
    r = engine.Reconstruction(0)
    for getter in (r.ncc_get_source, r.ncc_get_targets):
        with pytest.raises(engine.SvrError, match="svr_ncc_get: no (source|targets)"):
            getter()
    rng = np.random.default_rng(3)
    t = rng.integers(-1, 900, (3, 7, 5)).astype(np.int16)
    s = rng.integers(0, 900, (6, 8, 9)).astype(np.int16)
    r.ncc_set_targets(t)
    r.ncc_set_source(s)
    m = np.eye(4)
    m[:3, 3] = (2.25, 1.5, 2.75)
    before = r.ncc_evaluate([0, 1, 2], [m] * 3)[1]
    assert np.array_equal(r.ncc_get_targets(), t) and np.array_equal(r.ncc_get_source(), s)
    assert np.array_equal(r.ncc_get_targets(), t) and np.array_equal(r.ncc_get_source(), s)       # reading is repeatable ...
    assert np.array_equal(r.ncc_evaluate([0, 1, 2], [m] * 3)[1], before) and before[:, 0].min() > 0   # ... and leaves the evaluator's inputs alone
    r.close()


def _oracle_backend(oracle_mod):
    return host.NccBackend(lambda target, M, source: oracle_mod.ncc_evaluate(target, M, source)[1])


def test_two_grid_groups_give_the_oracle_trajectory(rec, oracle_mod):
    """Slices of two grids in one pass (3 of 37 x 29 at 1.17647 mm, 2 of 50 x 41 at 0.9 mm, one padded 50 x 41 grid): the device
    makes each group's levels in a launch of its own, into planes of the larger group's pitch.  Same integer moments as the host
    pyramid under the oracle evaluator, hence the same decisions: equal evaluation counts and identical matrices."""
    R = 13.0
    ra = geo.ImageAttributes(34, 34, 34, 1.0, 1.0, 1.0)
    kk, jj, ii = np.meshgrid(np.arange(34), np.arange(34), np.arange(34), indexing="ij")
    w = np.stack([ii, jj, kk, np.ones_like(ii)], -1).astype(np.float64) @ geo.image_to_world(ra).T
    vol = (phantom.phantom_intensity(w[..., :3], R) * 700 / 0.55).astype(np.float32)
    grids = [(37, 29, 1.17647)] * 3 + [(50, 41, 0.9)] * 2
    slices = np.full((5, 41, 50), -1.0, np.float32)
    attrs, start = [], []
    rng = np.random.default_rng(8)
    for k, (nx, ny, d) in enumerate(grids):
        a = geo.ImageAttributes(nx, ny, 1, d, d, 1.0, origin=np.array([0.4 * k - 1.0, 0.7 - 0.3 * k, -6.0 + 3.0 * k]))
        jj, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
        p = np.stack([ii, jj, np.zeros_like(ii), np.ones_like(ii)], -1).astype(np.float64) @ geo.image_to_world(a).T
        slices[k, :ny, :nx] = phantom.phantom_intensity(p[..., :3], R) * 700 / 0.55
        attrs.append(a)
        start.append(geo.rigid_matrix(*rng.uniform(-1.5, 1.5, 3), *rng.uniform(-2.5, 2.5, 3)))
    args = (slices, attrs, np.stack(start), ra, vol)
    dev, nev_d = host.SliceToVolumeRegistration(rec, *args)
    cpu, nev_c = host.SliceToVolumeRegistration(None, *args, backend=_oracle_backend(oracle_mod))
    assert nev_d == nev_c and nev_d > 100
    assert np.array_equal(dev, cpu) and not np.array_equal(dev, np.stack(start))
