"""The host restatement of irtkImageRegistrationWithPadding::Initialize(level) (csrc/irtk_reg.cpp: blur_with_padding,
resample_with_padding, prepare_level -- "the definition" the device pyramid follows) against the independent numpy reference of
tests/pyramid_ref.py, at every case of tests/pyramid_cases.py and every level: int16 equality, no tolerance.  And the
reference against itself with long-double sums, so that it cannot hide an ordering mistake of its own."""
import numpy as np
import pytest

from fetalreconstruction_amd import host

import pyramid_cases as cases
import pyramid_ref as ref


def test_blur_kernel_is_the_sampled_gaussian():
    """the host's taps: 2 round(4 sigma / voxel) + 1 of them, each the Gaussian's value.  Both sides make an exp (at most an ulp
    each) and five roundings of products and quotients: a relative 1e-14 is generous and still far below any mistake."""
    for sigma, voxel in ((0.588235, 1.17647), (1.1, 2.2), (4.4, 1.1), (2.2, 2.2), (0.5, 1.25), (3.7, 0.9)):
        k, r = host.irtk_blur_kernel(sigma, voxel), ref.gaussian_kernel(sigma, voxel)
        assert k.size == r.size == 2 * int(np.floor(4 * sigma / voxel + 0.5)) + 1
        assert np.allclose(k, r, rtol=1e-14, atol=0) and np.array_equal(k, k[::-1]) and k.argmax() == k.size // 2


def _attr_tuple(a):
    return (a.nx, a.ny, a.nz, a.dx, a.dy, a.dz, *a.xaxis, *a.yaxis, *a.zaxis, *a.origin)


@pytest.mark.parametrize("name", cases.SMALL)
def test_host_blur_is_the_reference(name):
    c = cases.get(name)
    done = 0
    for s in c.steps:
        if not c.host_can(s) or not s.blur > 0:
            continue
        for im, a, p in zip(c.images, c.attrs, c.pads):
            out = host.irtk_blur_with_padding(im, a, s.blur, p)
            assert np.array_equal(out, ref.blur(im, c.kernels(s), p)), (name, s.level, p)
            done += 1
    assert done or name == "kernel_sizes_of_zero"          # (its steps leave passes out, which the host code cannot)


@pytest.mark.parametrize("name", cases.NAMES)
def test_host_level_is_the_reference(name):
    c = cases.get(name)
    for k, s in enumerate(c.steps):
        if not c.host_can(s):
            continue
        for im, a, p, (rim, ra, rmn, rmx) in zip(c.images, c.attrs, c.pads, c.reference(k)):
            out, oa, mn, mx = host.irtk_prepare_level(im, a, s.blur, s.res, s.res0, s.level, p)
            assert _attr_tuple(oa) == _attr_tuple(ra), (name, s.level)
            assert (mn, mx) == (rmn, rmx), (name, s.level, p)
            assert np.array_equal(out, rim), (name, s.level, p)


def test_the_cases_reach_their_edges():
    """what the shapes were chosen for, checked on the reference so that a change of a case cannot silently lose it"""
    c = cases.get("batch_mixed_padding")
    assert sorted(set(c.pads)) == [-32768, -1, 0] and all((im == 32767).any() and (im < 0).any() for im in c.images)
    lvl = [c.reference(k) for k in range(3)]
    assert [(r[0][1].nx, r[0][1].ny) for r in lvl] == [(37, 29), (19, 15), (9, 7)] and c.tx > 37 and c.ty > 29 and c.first_plane == 3
    assert all((r[0] == -1).any() and (r[0] > 0).any() for l in lvl for r in l)
    c = cases.get("batch_3d")
    assert [c.reference(k)[0][1].nz for k in range(4)] == [5, 5, 5, 10]                           # level 0 of the volume schedule up-samples z
    assert host.irtk_blur_kernel(c.steps[2].blur, 2.2).size // 2 >= 4 and not c.resamples(c.steps[0]) and c.resamples(c.steps[3])
    c = cases.get("thin_3x3x1")
    assert [(r[0][1].nx, r[0][1].nz, r[0][1].dz) for r in (c.reference(k) for k in range(3))] == [(3, 1, 1.0), (2, 1, 2.0), (1, 1, 1.0)]   # n_new < 1 -> 1, old size
    c = cases.get("thin_9x7x2")
    assert [(r[0][1].nx, r[0][1].ny, r[0][1].nz) for r in (c.reference(k) for k in range(3))] == [(9, 7, 4), (5, 4, 2), (2, 2, 1)]
    c = cases.get("nothing_above_padding")
    for k in range(2):
        r = c.reference(k)
        assert (r[1][2], r[1][3]) == (32767, -32768) and (r[1][0] == -1).all()                     # nothing above the padding: max < min
        assert r[2][2] == r[2][3] and sorted(set(r[2][0].ravel())) == [-1, 0]                        # one voxel: a range of 0
        assert r[0][3] > r[0][2] and r[3][3] > r[3][2]
    c = cases.get("source_slot")
    assert [(r[0][1].nx, r[0][1].ny, r[0][1].nz) for r in (c.reference(k) for k in range(3))] == [(23, 31, 21), (12, 16, 11), (6, 8, 5)]
    c = cases.get("range_loop")
    flat = c.images.reshape(-1)
    assert flat.size > 1024 * 4096 and int(np.argmin(np.where(flat > -1, flat, 32767))) >= 1024 * 4096 and int(np.argmax(flat)) == flat.size - 1


def _count_last_bit_voxels(q64, qld, where):
    """voxels whose float64 and long-double quotients truncate to different shorts; each must be an integer to 1e-9"""
    differ = where & (ref.put_as_double(q64) != ref.put_as_double(qld))
    assert (np.abs(qld[differ] - np.rint(qld[differ])) < 1e-9).all()
    return int(differ.sum())


@pytest.mark.parametrize("name", cases.SMALL)
def test_reference_quotients_do_not_depend_on_the_order(name):
    """Every quotient of the reference again with 64-bit-mantissa sums (np.longdouble): the sums of at most 33 products of a
    53-bit tap and a 16-bit voxel are then exact to 2^-11 ulp of a double, whatever the order.  A voxel whose two quotients
    truncate to different shorts must have an exact quotient within 1e-9 of an integer, and at most 1 voxel in 10^4 of a case
    may be such a voxel.

    The blur passes are checked at every level of every case.  The resampler is checked on the same (blurred) images with two
    changes that keep exact integers out of its quotients, both confirmed on the CPU to keep every case under the cap:
    a ratio of 1.9 per axis and a grid shifted by a fraction of a voxel -- at the schedule's own levels, and in the middle of any
    centred grid, every sample sits on an integer or half-integer position up to the
    last bits of the two matrix products, the weights are 0, 1/2, 1 +- 1e-15 and a large share of the exact quotients are
    multiples of 1/8 +- 1e-12 -- and the padded voxels filled with noise -- inside a padded band the four corners are equal, and
    next to it the resampler writes voxels that only one corner contributes to: both quotients, g (w1 + ..) / (w1 + ..) and
    g w / w, are the integer g by construction.  Neither says anything about the order of the sums; both are covered exactly by
    test_host_level_is_the_reference."""
    assert np.finfo(np.longdouble).nmant >= 63               # x87 extended precision
    c = cases.get(name)
    rng = np.random.default_rng(21)
    voxels = found = 0
    for s in c.steps:
        for im, a, p in zip(c.images, c.attrs, c.pads):
            cur = np.asarray(im)
            for axis, ker in enumerate(c.kernels(s)):
                if ker is None:
                    continue
                q64, centre = ref.blur_quotient(cur, axis, ker, p)
                qld, _ = ref.blur_quotient(cur, axis, ker, p, acc=np.longdouble)
                found += _count_last_bit_voxels(q64, qld, centre)
                voxels += cur.size
                cur = ref.blur_pass(cur, axis, ker, p)
            oa = ref.resampled_attr(a, (1.9 * a.dx, 1.9 * a.dy, 1.9 * a.dz))
            oa.origin = np.asarray(a.origin) + 0.37 * a.dx * np.asarray(a.xaxis) + 0.41 * a.dy * np.asarray(a.yaxis) + 0.29 * a.dz * np.asarray(a.zaxis)
            filled = np.where(cur <= p, rng.integers(-200, 3001, cur.shape), cur).astype(np.int16)
            q64, written = ref.resample_quotient(filled, a, oa, -32768)
            qld, wld = ref.resample_quotient(filled, a, oa, -32768, acc=np.longdouble)
            assert np.array_equal(written, wld)
            found += _count_last_bit_voxels(q64, qld, written)
            voxels += q64.size
    print(f"{name}: {found} last-bit voxels of {voxels}")
    assert voxels > 0 and found * 10 ** 4 <= voxels
