"""The images, grids and levels that tests/test_pyramid_ref.py (host code against tests/pyramid_ref.py) and
tests/test_pyramid_gpu.py (device against tests/pyramid_ref.py) share: the smallest shapes that reach each edge of
csrc/svr_pyr.inc.  The reference of a (case, step) is computed once and cached; nobody writes into it."""
from __future__ import annotations

import copy
from dataclasses import dataclass, field

import numpy as np

from fetalreconstruction_amd import geometry as geo
from fetalreconstruction_amd import host

import pyramid_ref as ref


@dataclass
class Step:
    level: int
    blur: float                    # sigma in mm, 0 = none
    res: tuple                     # the level's resolution
    res0: tuple                    # the finest level's (decides whether level 0 resamples)
    axes: tuple = None             # which of the x, y, z passes run; None = the reference's rule (z only when nz > 1)
    resample: bool = None          # None = the reference's rule (level > 0 or res0 != voxel size)


@dataclass
class Case:
    name: str
    images: np.ndarray             # int16 [n][nz][ny][nx], one grid
    attrs: list
    pads: list
    steps: list
    slot: int = 1
    tx: int = 0                    # the pitch of the allocated target planes (slot 1); 0 = the level's own size
    ty: int = 0
    first_plane: int = 0
    _ref: dict = field(default_factory=dict)

    def kernels(self, step):
        """the host's own kernels for the image's voxel sizes, None where no pass runs"""
        a = self.attrs[0]
        axes = step.axes if step.axes is not None else (1, 1, 1 if a.nz != 1 else 0)
        if not step.blur > 0:
            return [None, None, None]
        return [host.irtk_blur_kernel(step.blur, d) if on else None for on, d in zip(axes, (a.dx, a.dy, a.dz))]

    def resamples(self, step):
        return bool(step.resample) if step.resample is not None else ref.needs_resampling(self.attrs[0], step.res0, step.level)

    def host_can(self, step):
        """the host's prepare_level takes a sigma and a level, not kernels: it cannot leave out a pass"""
        return step.axes is None and step.resample is None

    def reference(self, k):
        """[(image, attributes, min, max)] of step k, one per image"""
        if k not in self._ref:
            s = self.steps[k]
            out = [ref.prepare_level(im, a, self.kernels(s), self.resamples(s), s.res, p) for im, a, p in zip(self.images, self.attrs, self.pads)]
            for o in out:
                o[0].setflags(write=False)
            self._ref[k] = out
        return self._ref[k]


def _image(rng, shape, pad, spike=False, band=True, holes=0.04):
    """values from -200 to 3000 (negative ones are above a padding of -32768 and at or below -1 / 0), a padded band along x, padded
    holes in the interior, optionally one voxel at 32767"""
    v = rng.integers(-200, 3001, shape).astype(np.int16)
    if band and shape[2] > 8:
        v[:, :, :3] = pad
        v[:, -2:, :] = pad
    v[rng.random(shape) < holes] = pad
    if spike:
        v[shape[0] // 2, shape[1] // 2, (2 * shape[2]) // 3] = 32767
    return v


def _levels(attr, slice_to_volume, levels=(0, 1, 2)):
    sch = ref.schedule(attr, slice_to_volume)
    return [Step(l, sch[l][0], sch[l][1], sch[0][1]) for l in levels]


def moved_attr(a, G):
    """the same image seen from the frame G (a rigid map of the world)"""
    r = copy.copy(a)
    r.xaxis, r.yaxis, r.zaxis = (G[:3, :3] @ np.asarray(v, float) for v in (a.xaxis, a.yaxis, a.zaxis))
    r.origin = (G @ np.array([*np.asarray(a.origin, float), 1.0]))[:3]
    return r


def bundled_mask_frame():
    """the oblique frame of the bundled mask, 475 mm from the world origin (tests/real_mask.py)"""
    import real_mask as rm
    m, a, _ = rm.load()
    G = np.eye(4)
    G[:3, 0], G[:3, 1], G[:3, 2] = a.xaxis, a.yaxis, a.zaxis
    G[:3, 3] = rm.centre(m, a)
    return G


def _batch_mixed_padding():
    rng = np.random.default_rng(11)
    pads = [-1, -1, 0, -32768, -1]
    a = geo.ImageAttributes(37, 29, 1, 1.17647, 1.17647, 2.5, origin=np.array([3.1, -2.7, 1.9]))
    imgs = np.stack([_image(rng, (1, 29, 37), p, spike=True) for p in pads])
    return Case("batch, mixed padding", imgs, [copy.copy(a) for _ in pads], pads, _levels(a, False), tx=50, ty=41, first_plane=3)


def _far_frame():
    c = _batch_mixed_padding()
    G = bundled_mask_frame()
    return Case("oblique, far frame", c.images, [moved_attr(a, G) for a in c.attrs], c.pads, c.steps, tx=50, ty=41, first_plane=3)


def _batch_3d():
    rng = np.random.default_rng(12)
    pads = [-1, 0, -32768]
    a = geo.ImageAttributes(21, 18, 5, 1.1, 1.1, 2.2, origin=np.array([-1.3, 0.4, 2.2]))
    # (fewer holes than in the 2-D cases: a voxel whose only z neighbour within the 3 taps is a hole keeps its value g as k g / k,
    # an integer by construction, and five planes have many such voxels -- test_reference_quotients_do_not_depend_on_the_order)
    imgs = np.stack([_image(rng, (5, 18, 21), p, holes=0.02) for p in pads])
    steps = _levels(a, False) + _levels(a, True, (0,))          # (the volume's level 0 is isotropic: 5 planes become 10)
    return Case("3-D batch", imgs, [copy.copy(a) for _ in pads], pads, steps, tx=24, ty=18, first_plane=1)


def _kernel_sizes_of_zero():
    c = _batch_3d()
    a = c.attrs[0]
    steps = [Step(1, 1.1, (2.2, 2.2, 2.2) if rs else (a.dx, a.dy, a.dz), (a.dx, a.dy, a.dz), axes=ax, resample=bool(rs))
             for ax in ((0, 1, 1), (1, 0, 0), (0, 0, 0)) for rs in (0, 1)]
    return Case("kernel sizes of zero", c.images, c.attrs, c.pads, steps, tx=21, ty=18, first_plane=0)


def _thin(shape, voxel):
    rng = np.random.default_rng(13)
    a = geo.ImageAttributes(shape[2], shape[1], shape[0], *voxel)
    img = _image(rng, shape, -1, band=False, holes=0.0)[None]
    return Case("thin axis %dx%dx%d" % shape[::-1], img, [a], [-1], _levels(a, True))     # the volume's schedule: z doubles too, n_new < 1 -> 1


def _nothing_above_padding():
    rng = np.random.default_rng(14)
    a = geo.ImageAttributes(37, 29, 1, 1.17647, 1.17647, 2.5)
    full = _image(rng, (1, 29, 37), -1)
    none = rng.integers(-200, 0, (1, 29, 37)).astype(np.int16)
    one = np.full((1, 29, 37), -1, np.int16)
    one[0, 12, 20] = 1024                                         # (even coordinates: level 1 samples every other voxel)
    imgs = np.stack([full, none, one, _image(rng, (1, 29, 37), -1)])
    return Case("no voxel above padding", imgs, [copy.copy(a) for _ in range(4)], [-1] * 4, _levels(a, False, (0, 1)), tx=37, ty=29, first_plane=0)


def _source_slot():
    rng = np.random.default_rng(15)
    a = geo.ImageAttributes(23, 31, 17, 1.0, 1.0, 1.25, origin=np.array([0.3, 1.1, -0.6]))
    img = _image(rng, (17, 31, 23), -32768)[None]
    return Case("source slot", img, [a], [-32768], _levels(a, True), slot=0)      # level 0: 1.25 mm planes up-sampled to 1 mm


RANGE_DIMS = (160, 160, 168)      # [z][y][x]: 4 300 800 voxels, more than the 1024 x 4096 of one sweep of k_pyr_range's grid


def _range_loop():
    rng = np.random.default_rng(16)
    v = rng.integers(10, 3000, RANGE_DIMS).astype(np.int16)
    v.reshape(-1)[::7] = -1
    flat = v.reshape(-1)
    flat[1024 * 4096 + 12345] = 5                                 # the minimum: past the first 1024 x 4096 voxels
    flat[-1] = 32000                                              # the maximum: the last voxel of the last workgroup
    a = geo.ImageAttributes(RANGE_DIMS[2], RANGE_DIMS[1], RANGE_DIMS[0], 1.0, 1.0, 1.0)
    return Case("range loop", v[None], [a], [-1], [Step(0, 0.0, (1.0, 1.0, 1.0), (1.0, 1.0, 1.0))], slot=0)


_BUILDERS = {
    "batch_mixed_padding": _batch_mixed_padding, "batch_3d": _batch_3d, "thin_9x7x2": lambda: _thin((2, 7, 9), (1.1, 1.1, 2.2)),
    "thin_3x3x1": lambda: _thin((1, 3, 3), (1.0, 1.0, 1.0)), "kernel_sizes_of_zero": _kernel_sizes_of_zero,
    "nothing_above_padding": _nothing_above_padding, "far_frame": _far_frame, "source_slot": _source_slot, "range_loop": _range_loop,
}
NAMES = list(_BUILDERS)
SMALL = [n for n in NAMES if n != "range_loop"]
_CASES = {}


def get(name):
    if name not in _CASES:
        _CASES[name] = _BUILDERS[name]()
        _CASES[name].images.setflags(write=False)
    return _CASES[name]
