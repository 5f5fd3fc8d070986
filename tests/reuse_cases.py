"""The problems and the call sequence of tests/test_context_reuse_gpu.py: one engine context handed a second problem must give the
bits of a fresh context handed the same problem.  Device-free -- tests/test_reuse_cases.py checks on the CPU that the cases reach
what they claim (larger / smaller on every axis, the table's gather changing family, the hierarchical levels' patch counts).

fingerprint() drives a context through every stage that keeps state between calls and returns what the stages left, copied.  It
runs the default paths only (cell scatter and gather, coefficient table on): their sums have a fixed order, so two fresh
contexts agree bit for bit and no tolerance is needed."""
import copy
import functools
from collections import OrderedDict

import numpy as np

from fetalreconstruction_amd import phantom

TILE_RULE_DENSITY = 0.65          # tile_shape_rule (csrc/svr_hip.hip): below it the table's gather takes 6 x 5 tiles
PVR_STACKS = dict(n_stacks=2, stack_shape=(28, 24, 5), in_plane=1.1, spacing=2.2, thickness=None, recon_res=1.0, mask_radius=11.0, seed=101,
                  orientations=("ax", "cor"))
PVR_LEVELS = {"L16": ((16, 16), (8, 8)), "L8": ((8, 8), (4, 4)), "L12x8": ((12, 8), (6, 4))}      # patch size, stride: (x, y)
NAMES = ("A", "A2", "B", "C", *PVR_LEVELS)


def _build(name):
    if name == "A":
        return phantom.problem_tiny()
    if name == "A2":
        return phantom.problem_tiny(seed=2)
    if name == "B":
        return phantom.make_problem(3, (40, 36, 10), 1.1, 2.2, None, 0.8, 16.0, seed=2, orientations=("ax", "cor", "sag"), name="B")
    if name == "C":
        return phantom.make_problem(2, (20, 24, 5), 1.3, 2.6, None, 1.2, 9.0, seed=3, orientations=("ax", "sag"), name="C")
    from tests.twins import pvr
    q = PVR_STACKS
    stacks, mask, mattr, rattr, rmask = phantom.make_stacks(q["n_stacks"], q["stack_shape"], q["in_plane"], q["spacing"], q["thickness"], q["recon_res"],
                                                            q["mask_radius"], seed=q["seed"], orientations=q["orientations"])
    size, stride = PVR_LEVELS[name]
    return pvr.make_pvr_problem(stacks, mask, mattr, rattr, rmask, size, stride, name=name)


def _freeze(prob):
    for v in vars(prob).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return prob


@functools.lru_cache(maxsize=None)
def get(name):
    """the named problem, made once; nobody writes into it"""
    return _freeze(_build(name))


def density(prob):
    """pixel_density (csrc/svr_hip.hip): voxel area / pixel area in the slice plane"""
    return float(prob.vdim[0]) * float(prob.vdim[1]) / (float(prob.slice_dim[0][0]) * float(prob.slice_dim[0][1]))


def with_volume_of(prob, other):
    """prob's slices under other's volume grid and mask"""
    q = copy.copy(prob)
    for k in ("vsize", "vdim", "recon_i2w", "recon_w2i", "mask", "psf_c0"):
        setattr(q, k, getattr(other, k))
    return q


def with_slices_of(prob, other):
    """other's slice grid under prob's volume grid and mask"""
    return with_volume_of(other, prob)


@functools.lru_cache(maxsize=None)
def volume_grid(radius, res=1.0):
    """a volume grid and its spherical mask as make_problem lays them out (only the volume side of the result is meant)"""
    return _freeze(phantom.make_problem(1, (4, 4, 1), 1.0, 2.0, None, res, radius, seed=1, orientations=("ax",)))


def with_mask(prob, radius):
    """prob with a smaller spherical mask on its own grid"""
    q = copy.copy(prob)
    n = prob.vsize[0]
    c1 = ((np.arange(n) - (n - 1) / 2.0) * float(prob.vdim[0])) ** 2
    q.mask = ((c1[:, None, None] + c1[None, :, None] + c1[None, None, :]) < radius * radius).astype(np.float32)
    return q


def spx(prob, seed=0):
    """superpixel masks in the wire format, as _spx of tests/test_pvr.py: 64 * 64 chars per patch, index x + 64 y, '1' = inside"""
    rng = np.random.default_rng(seed)
    ns, sy, sx = prob.slices.shape
    m = np.full((ns, 64, 64), ord("0"), np.uint8)
    m[:, :sy, :sx] = np.where(rng.random((ns, sy, sx)) < 0.7, ord("1"), ord("0"))
    return m.reshape(ns, 4096)


def inputs(prob, seed=11):
    """what the passes read besides the problem: a volume, EM weights and simulated slices, fixed (as _inputs of tests/test_invalidation_gpu.py)"""
    rng = np.random.default_rng(seed)
    on = prob.slices != -1
    return {
        "vol": rng.uniform(0.5, 1.5, prob.mask.size).astype(np.float32) * np.float32(prob.max_intensity * 0.5),
        "w": np.where(on, rng.uniform(0.2, 1.0, prob.slices.shape), 0).astype(np.float32),
        "sim": np.where(prob.slices > 0, prob.slices * rng.uniform(0.8, 1.2, prob.slices.shape), 0).astype(np.float32),
    }


STATE_OPTIONS = ("psf_list_valid", "cells_valid", "coeff_state", "back_mode", "fwd_mode")


def fingerprint(rec, prob, X, bias=False):
    """Every stage of one context on an uploaded problem (sync_gpu is the caller's) -> an ordered dict of named arrays, all copies."""
    from fetalreconstruction_amd import engine as E
    out = OrderedDict()

    def put(name, value):
        out[name] = np.array(value, copy=True)

    ones = np.ones(prob.ns, np.float32)
    # upload and Gaussian reconstruction
    rec.UpdateScaleVector(ones, ones)
    rec.InitializeEMValues()
    put("gauss.voxel_num", rec.GaussianReconstruction())
    put("gauss.psf_sums", rec.debug_get(E.BUF_PSF_SUMS))
    put("gauss.voxel_count", rec.debug_get(E.BUF_VOXEL_COUNT))
    put("gauss.vol_weights", rec.getVolWeights())
    put("gauss.volume", rec.syncCPU())
    # forward projection
    rec.debug_set(E.BUF_RECONSTRUCTED, X["vol"])
    put("fwd.inside", rec.SimulateSlices())
    for name, b in (("simslices", E.BUF_SIMSLICES), ("simweights", E.BUF_SIMWEIGHTS), ("siminside", E.BUF_SIMINSIDE)):
        put("fwd." + name, rec.debug_get(b))
    # EM steps
    m = float(np.float32(1.0 / (float(np.float32(2.1)) * prob.max_intensity - float(np.float32(1.9)) * prob.min_intensity)))
    sigma = rec.InitializeRobustStatistics()
    put("em.potentials", rec.EStep(m, sigma, 0.9))
    put("em.weights", rec.debug_get(E.BUF_WEIGHTS))
    put("em.scale", rec.CalculateScaleVector())
    put("em.scalars", np.array([sigma, *rec.MStep(1, 0.0001, sigma, 0.9)], np.float32))
    # superresolution (SetSmoothingParameters(150, 0.02): delta 150, lambda 450, alpha 1)
    rec.debug_set(E.BUF_SIMSLICES, X["sim"])
    rec.debug_set(E.BUF_WEIGHTS, X["w"])
    rec.Superresolution(1, ones, False, 1.0, prob.min_intensity, prob.max_intensity, 150.0, 450.0)
    put("sr.addon", rec.debug_get(E.BUF_ADDON))
    put("sr.confidence_map", rec.debug_get(E.BUF_CONFIDENCE_MAP))
    put("sr.volume", rec.syncCPU())
    # the table written in the first round is streamed in the second
    put("table.inside", rec.SimulateSlices())
    for name, b in (("simslices", E.BUF_SIMSLICES), ("simweights", E.BUF_SIMWEIGHTS), ("siminside", E.BUF_SIMINSIDE)):
        put("table." + name, rec.debug_get(b))
    rec.debug_set(E.BUF_SIMSLICES, X["sim"])
    rec.SuperresolutionBackproject(ones)
    put("table.addon", rec.debug_get(E.BUF_ADDON))
    put("table.confidence_map", rec.debug_get(E.BUF_CONFIDENCE_MAP))
    put("table.options", [rec.get_option(k) for k in STATE_OPTIONS])
    put("table.fallbacks", list(rec.fallbacks().values()))
    if bias:
        rec.CorrectBias(12.0, False)
        rec.NormaliseBias(0, 12.0)
        put("bias.bias", rec.debug_get(E.BUF_BIAS))
        put("bias.volume", rec.syncCPU())
    return out


def differing(got, ref):
    """the names of the arrays that are not the same bits (NaN equal to NaN), with the number of elements that differ"""
    bad = []
    if list(got) != list(ref):
        return [("keys", list(got), list(ref))]
    for k in ref:
        a, b = got[k], ref[k]
        if a.shape != b.shape or a.dtype != b.dtype:
            bad.append((k, a.shape, b.shape))
        elif not np.array_equal(a, b, equal_nan=a.dtype.kind == "f"):
            both_nan = np.isnan(a) & np.isnan(b) if a.dtype.kind == "f" else False
            bad.append((k, int(((a != b) & ~both_nan).sum()), "of", a.size))
    return bad
