"""ctypes binding of libsvr_hip.so: `Reconstruction`, a method-for-method mirror of the reference's
`class Reconstruction` (source/reconstructionGPU2/include/reconstruction_cuda2.cuh:92-341).

Method names, argument meaning and call order are the reference's, so the parity tests read
like irtkReconstruction's own call sequence (irtkReconstructionGPU.cc:249-401, 2695-3440).
Errors raise `SvrError` instead of the reference's print + exit(-err).

There is no CPU fallback: if the HIP library is missing or no GPU is visible, construction fails.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SVR_HIP_LIB: tuning builds made by `build.py --variant` (tools/exp_*.py); the product is lib/libsvr_hip.so
LIB_PATH = os.environ.get("SVR_HIP_LIB") or os.path.join(_HERE, "lib", "libsvr_hip.so")

# enum svr_buffer / svr_timer (include/svr_hip.h)
BUF_RECONSTRUCTED, BUF_VOL_WEIGHTS, BUF_ADDON, BUF_CONFIDENCE_MAP, BUF_MASK = 0, 1, 2, 3, 4
BUF_BIAS_VOLUME, BUF_SMOOTH_MASK = 5, 6
BUF_SLICES, BUF_WEIGHTS, BUF_SIMSLICES, BUF_SIMWEIGHTS, BUF_PSF_SUMS, BUF_BIAS = 10, 11, 12, 13, 14, 15
BUF_SIMINSIDE, BUF_VOXEL_COUNT = 20, 21
T_BACKPROJECT, T_FORWARD, T_GAUSS, T_REGULARIZE, T_ESTEP, T_MSTEP, T_SCALE, T_REGISTER = range(8)
RESAMPLE_INSTALL, RESAMPLE_SCALE = 1, 2                # SVR_RESAMPLE_* (include/svr_hip.h)
CHANNEL_INDICATOR = 1                                  # SVR_CHANNEL_INDICATOR
CHANNEL_GUIDE_ONLY = 1                                 # SVR_CHANNEL_GUIDE_ONLY
REG_TARGETS, REG_SUM_A, REG_CNT_A, REG_SUM_B, REG_CNT_B, REG_MOMENTS, REG_SIMILARITIES, REG_GRADIENT, REG_ACTIVE = range(9)   # enum svr_reg_state
TIMER_NAMES = ("backproject", "forward", "gauss", "regularize", "estep", "mstep", "scale", "register", "allreduce", "exchange_host", "coeff_build", "reduce_scatter", "allgather",
               "backproject_table", "forward_table", "forward_store", "backproject_store")

EXPORTS = [
    "svr_create", "svr_destroy", "svr_last_error", "svr_set_flags", "svr_set_option", "svr_get_option", "svr_set_spx_masks", "svr_init_reconstruction_volume",
    "svr_set_mask", "svr_init_storage_volumes", "svr_fill_slices", "svr_set_slice_dims",
    "svr_set_slice_matrices", "svr_generate_psf_volume", "svr_update_scale_vector",
    "svr_update_slice_weights", "svr_update_reconstructed", "svr_sync_cpu", "svr_get_vol_weights",
    "svr_gaussian_reconstruction", "svr_simulate_slices", "svr_initialize_em_values",
    "svr_initialize_robust_statistics", "svr_estep", "svr_mstep", "svr_calculate_scale_vector",
    "svr_superresolution", "svr_mask_volume", "svr_scale_volume", "svr_restore_slice_intensities",
    "svr_debug_get", "svr_debug_set", "svr_debug_probe_pixel", "svr_device_ptr", "svr_volume_voxels", "svr_set_stream",
    "svr_gaussian_reconstruction_local", "svr_gaussian_reconstruction_finish",
    "svr_superresolution_backproject", "svr_superresolution_update", "svr_robust_statistics_sums",
    "svr_mstep_sums", "svr_scale_volume_sums", "svr_scale_volume_apply", "svr_timer_get",
    "svr_unit_counts", "svr_fallbacks", "svr_clock_probe", "svr_slice_em_setup", "svr_slice_em_set_state", "svr_mstep_estep_device", "svr_slice_em_run", "svr_slice_em_apply_weights", "svr_slice_em_fetch", "svr_slice_em_set_patch_form", "svr_cell_stats", "svr_pair_pack", "svr_pair_unpack", "svr_timer_reset", "svr_timer_enable", "svr_timer_begin", "svr_timer_end", "svr_timer_add", "svr_counters", "svr_get_stream", "svr_device", "svr_device_count", "svr_combine_weights", "svr_update_stack_sizes", "svr_ncc_set_targets", "svr_ncc_set_source",
    "svr_ncc_evaluate", "svr_ncc_get", "svr_ncc_alloc_targets","svr_pyr_upload", "svr_pyr_level", "svr_nmi_bin_source", "svr_nmi_evaluate", "svr_lncc_evaluate", "svr_stack_motion", "svr_slice_quality", "svr_slice_ssim", "svr_resample_to_reconstruction", "svr_correct_bias", "svr_normalise_bias", "svr_normalise_bias_local",
    "svr_normalise_bias_finish", "svr_init_reg_storage_volumes", "svr_fill_reg_slices",
    "svr_update_resampled_slices_i2w", "svr_prepare_slice_to_volume_reg", "svr_register_slices_to_volume",
    "svr_reg_set_schedule", "svr_reg_evaluate_costs", "svr_reg_counters", "svr_reg_get", "svr_pvr_cc_patches", "svr_pvr_register_patches",
    "svr_slab_plan", "svr_slab_rs_pack", "svr_slab_update", "svr_slab_finish", "svr_stream_sync",
    "svr_get_scale_vector", "svr_adopt_scale_vector", "svr_get_slice_inside", "svr_mstep_estep", "svr_mstep_sums_fetch", "svr_mstep_partial", "svr_mstep_estep_ranks",
    "svr_channel_scatter", "svr_channel_finish", "svr_channel_vote", "svr_channel_vote_fetch",
    "svr_channel_sr_begin", "svr_channel_sr_seed", "svr_channel_sr_backproject", "svr_channel_sr_update", "svr_channel_sr_end",
    "svr_channel_sr_guide", "svr_monoexp_fit",
]


class SvrError(RuntimeError):
    pass


class _PyrImage(C.Structure):
    """struct svr_pyr_image (include/svr_hip.h)"""
    _fields_ = [("i2w_out", C.c_double * 12), ("w2i_in", C.c_double * 12), ("pad", C.c_int)]


_lib = None


def load_library(path: str = LIB_PATH):
    """Load libsvr_hip.so (fails loudly if it was not built: run `python -m fetalreconstruction_amd.build`)."""
    global _lib
    if _lib is None:
        if not os.path.exists(path):
            raise SvrError(f"{path} not found: build the HIP engine first (fetalreconstruction_amd/build.py); "
                           "there is no CPU fallback")
        lib = C.CDLL(path)
        lib.svr_last_error.restype = C.c_char_p
        lib.svr_device_ptr.restype = C.c_void_p
        lib.svr_volume_voxels.restype = C.c_size_t
        lib.svr_destroy.restype = None
        _lib = lib
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


_hip = None


def _hip_memcpy(dst, src, nbytes, kind):
    """hipMemcpy (kind 1: host to device, 2: device to host; it returns when the copy is done) on the HIP runtime libsvr_hip.so
    is linked to: opened by its soname, the loader hands back the runtime that is already loaded"""
    global _hip
    if _hip is None:
        load_library()
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipMemcpy.restype = C.c_int
    rc = _hip.hipMemcpy(dst, src, nbytes, kind)
    if rc != 0:
        raise SvrError(f"hipMemcpy: HIP error {rc}")


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _u3(v):
    return (C.c_uint32 * 3)(*[int(x) for x in v])


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


class Reconstruction:
    """One GPU's SVR engine.  Mirrors `class Reconstruction` (RC.cuh:92-341)."""

    def __init__(self, device: int = 0):
        self._lib = load_library()
        h = C.c_void_p()
        rc = self._lib.svr_create(int(device), C.byref(h))
        if rc != 0 or not h:
            raise SvrError(f"svr_create(device={device}) failed with status {rc} (no usable MI355X / HIP device?)")
        self._h = h
        self.vsize = None
        self.sgrid = None   # (ns, sy, sx)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.svr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            msg = self._lib.svr_last_error(self._h)
            raise SvrError(f"status {rc}: {msg.decode() if msg else ''}")

    # ---- state upload (names as in RC.cuh) --------------------------------------------
    def InitReconstructionVolume(self, size, dim, data=None, sigma_bias=12.0):
        d = _f32(data) if data is not None else None
        self._ck(self._lib.svr_init_reconstruction_volume(self._h, _u3(size), _f3(dim), _p(d) if d is not None else None,
                                                          C.c_float(sigma_bias)))
        self.vsize = tuple(int(s) for s in size)

    def setMask(self, size, dim, data, sigma_bias=12.0):
        d = _f32(data)
        self._ck(self._lib.svr_set_mask(self._h, _u3(size), _f3(dim), _p(d), C.c_float(sigma_bias)))

    def initStorageVolumes(self, size, dim):
        self._ck(self._lib.svr_init_storage_volumes(self._h, _u3(size), _f3(dim)))
        self.sgrid = (int(size[2]), int(size[1]), int(size[0]))

    def FillSlices(self, sdata, sizes_x, sizes_y):
        d = _f32(sdata)
        sx = np.ascontiguousarray(sizes_x, np.int32)
        sy = np.ascontiguousarray(sizes_y, np.int32)
        self._ck(self._lib.svr_fill_slices(self._h, _p(d), _p(sx), _p(sy)))

    def setSliceDims(self, slice_dims, quality_factor):
        d = _f32(slice_dims)
        self._ck(self._lib.svr_set_slice_dims(self._h, _p(d), C.c_float(quality_factor)))

    def SetSliceMatrices(self, slice_transforms, inv_slice_transforms, i2w_init, w2i_init, i2w, w2i, recon_i2w, recon_w2i):
        arrs = [_f32(a) for a in (slice_transforms, inv_slice_transforms, i2w_init, w2i_init, i2w, w2i, recon_i2w, recon_w2i)]
        self._ck(self._lib.svr_set_slice_matrices(self._h, *[_p(a) for a in arrs]))

    def generatePSFVolume(self, cpu_psf, psf_size, slice_voxel_dim, psf_dim, psf_i2w, psf_w2i, quality_factor):
        i2w, w2i = _f32(psf_i2w), _f32(psf_w2i)
        self._ck(self._lib.svr_generate_psf_volume(self._h, None, _u3(psf_size), _f3(slice_voxel_dim), _f3(psf_dim),
                                                   _p(i2w), _p(w2i), C.c_float(quality_factor)))

    def UpdateScaleVector(self, scales, slice_weights):
        s, w = _f32(scales), _f32(slice_weights)
        self._ck(self._lib.svr_update_scale_vector(self._h, _p(s), _p(w)))

    def UpdateSliceWeights(self, slice_weights):
        w = _f32(slice_weights)
        self._ck(self._lib.svr_update_slice_weights(self._h, _p(w)))

    def UpdateReconstructed(self, size, data):
        d = _f32(data)
        self._ck(self._lib.svr_update_reconstructed(self._h, _u3(size), _p(d)))

    def syncCPU(self):
        out = np.empty(int(np.prod(self.vsize)), np.float32)
        self._ck(self._lib.svr_sync_cpu(self._h, _p(out)))
        return out

    def combineWeights(self):
        out = np.zeros(int(np.prod(self.vsize)), np.float32)
        self._ck(self._lib.svr_combine_weights(self._h, _p(out)))
        return out

    def updateStackSizes(self, stack_sizes):
        a = np.ascontiguousarray(stack_sizes, np.uint32).reshape(-1, 3)
        self._ck(self._lib.svr_update_stack_sizes(self._h, _p(a), len(a)))

    def getVolWeights(self):
        out = np.empty(int(np.prod(self.vsize)), np.float32)
        self._ck(self._lib.svr_get_vol_weights(self._h, _p(out)))
        return out

    # ---- compute ------------------------------------------------------------------------
    def GaussianReconstruction(self):
        n = C.c_int(0)
        self._ck(self._lib.svr_gaussian_reconstruction(self._h, C.byref(n)))
        return [n.value]          # voxel_num: one entry per device (RC.cu:2331)

    def SimulateSlices(self):
        inside = np.zeros(self.sgrid[0], np.uint8)
        self._ck(self._lib.svr_simulate_slices(self._h, _p(inside)))
        return inside.astype(bool)

    def InitializeEMValues(self):
        self._ck(self._lib.svr_initialize_em_values(self._h))

    def InitializeRobustStatistics(self):
        s = C.c_float(0)
        self._ck(self._lib.svr_initialize_robust_statistics(self._h, C.byref(s)))
        return s.value

    def EStep(self, m, sigma, mix):
        pot = np.zeros(self.sgrid[0], np.float32)
        self._ck(self._lib.svr_estep(self._h, C.c_float(m), C.c_float(sigma), C.c_float(mix), _p(pot)))
        return pot

    def MStep(self, it, step, sigma, mix):
        s, mx, m = C.c_float(sigma), C.c_float(mix), C.c_float(0)
        self._ck(self._lib.svr_mstep(self._h, int(it), C.c_float(step), C.byref(s), C.byref(mx), C.byref(m)))
        return s.value, mx.value, m.value

    def CalculateScaleVector(self):
        sc = np.zeros(self.sgrid[0], np.float32)
        self._ck(self._lib.svr_calculate_scale_vector(self._h, _p(sc)))
        return sc

    # the deferred forms (the C++ host objects use them: one wait for the device per SR iteration instead of four)
    def SimulateSlicesDeferred(self):
        self._ck(self._lib.svr_simulate_slices(self._h, None))

    def GetSliceInside(self):
        inside = np.zeros(self.sgrid[0], np.uint8)
        self._ck(self._lib.svr_get_slice_inside(self._h, _p(inside)))
        return inside.astype(bool)

    def CalculateScaleVectorDeferred(self):
        self._ck(self._lib.svr_calculate_scale_vector(self._h, None))

    def GetScaleVector(self):
        sc = np.zeros(self.sgrid[0], np.float32)
        self._ck(self._lib.svr_get_scale_vector(self._h, _p(sc)))
        return sc

    def AdoptScaleVector(self):
        self._ck(self._lib.svr_adopt_scale_vector(self._h))

    def MStepEStep(self, it, step, sigma, mix, want_scale=False, want_inside=False):
        """MStep + EStep with one wait -> (sigma, mix, m, slice_potential, scale_vec | None, slice_inside | None)"""
        em = np.array([sigma, mix, 0.0], np.float32)
        pot = np.zeros(self.sgrid[0], np.float32)
        sc = np.zeros(self.sgrid[0], np.float32) if want_scale else None
        ins = np.zeros(self.sgrid[0], np.uint8) if want_inside else None
        self._ck(self._lib.svr_mstep_estep(self._h, int(it), C.c_float(step), _p(em), _p(pot), None if sc is None else _p(sc),
                                           None if ins is None else _p(ins)))
        return float(em[0]), float(em[1]), float(em[2]), pot, sc, None if ins is None else ins.astype(bool)

    def Superresolution(self, it, slice_weight, adaptive, alpha, min_intensity, max_intensity, delta, lam,
                        global_bias_correction=False, sigma_bias=12.0, low_intensity_cutoff=0.01):
        w = _f32(slice_weight)
        self._ck(self._lib.svr_superresolution(self._h, int(it), _p(w), int(bool(adaptive)), C.c_float(alpha),
                                               C.c_float(min_intensity), C.c_float(max_intensity), C.c_float(delta),
                                               C.c_float(lam), int(bool(global_bias_correction)), C.c_float(sigma_bias),
                                               C.c_float(low_intensity_cutoff)))

    def set_flags(self, disable_bias_correction=True, debug_gpu=False):
        self._ck(self._lib.svr_set_flags(self._h, int(bool(disable_bias_correction)), int(bool(debug_gpu))))

    def CorrectBias(self, sigma_bias, global_bias_correction=False):
        self._ck(self._lib.svr_correct_bias(self._h, C.c_float(sigma_bias), int(bool(global_bias_correction))))

    def NormaliseBias(self, it, sigma_bias):
        self._ck(self._lib.svr_normalise_bias(self._h, int(it), C.c_float(sigma_bias)))

    def maskVolume(self):
        self._ck(self._lib.svr_mask_volume(self._h))

    def ScaleVolume(self):
        self._ck(self._lib.svr_scale_volume(self._h))

    def RestoreSliceIntensities(self, stack_factors, stack_index):
        f = _f32(stack_factors)
        i = np.ascontiguousarray(stack_index, np.int32)
        self._ck(self._lib.svr_restore_slice_intensities(self._h, _p(f), len(f), _p(i)))

    # ---- sharded halves -----------------------------------------------------------------
    def GaussianReconstructionLocal(self):
        self._ck(self._lib.svr_gaussian_reconstruction_local(self._h))

    def GaussianReconstructionFinish(self):
        n = C.c_int(0)
        self._ck(self._lib.svr_gaussian_reconstruction_finish(self._h, C.byref(n)))
        return n.value

    def SuperresolutionBackproject(self, slice_weight=None):
        w = _f32(slice_weight) if slice_weight is not None else None
        self._ck(self._lib.svr_superresolution_backproject(self._h, _p(w) if w is not None else None))

    def SuperresolutionUpdate(self, adaptive, alpha, min_intensity, max_intensity, delta, lam):
        self._ck(self._lib.svr_superresolution_update(self._h, int(bool(adaptive)), C.c_float(alpha),
                                                      C.c_float(min_intensity), C.c_float(max_intensity),
                                                      C.c_float(delta), C.c_float(lam)))

    def RobustStatisticsSums(self):
        o = np.zeros(2, np.float64)
        self._ck(self._lib.svr_robust_statistics_sums(self._h, _p(o)))
        return o

    def MStepSums(self):
        o = np.zeros(5, np.float64)
        self._ck(self._lib.svr_mstep_sums(self._h, _p(o)))
        return o

    def MStepSumsFetch(self, want_scale=False, want_inside=False):
        """the M-step's five sums with the deferred vectors in the same wait (what a sharded host calls)"""
        o = np.zeros(5, np.float64)
        sc = np.zeros(self.sgrid[0], np.float32) if want_scale else None
        ins = np.zeros(self.sgrid[0], np.uint8) if want_inside else None
        self._ck(self._lib.svr_mstep_sums_fetch(self._h, _p(o), None if sc is None else _p(sc), None if ins is None else _p(ins)))
        return o, sc, None if ins is None else ins.astype(bool)

    def ScaleVolumeSums(self):
        o = np.zeros(2, np.float64)
        self._ck(self._lib.svr_scale_volume_sums(self._h, _p(o)))
        return o

    def ScaleVolumeApply(self, scale):
        self._ck(self._lib.svr_scale_volume_apply(self._h, C.c_float(scale)))

    def set_stream(self, stream_handle):
        self._ck(self._lib.svr_set_stream(self._h, C.c_void_p(stream_handle)))

    def device_ptr(self, which):
        return self._lib.svr_device_ptr(self._h, int(which))

    def stream_sync(self):
        """wait for everything queued on the engine's stream"""
        self._ck(self._lib.svr_stream_sync(self._h))

    # ---- debug getters (debugWeights/Simslices/... RC.cuh:192-207) ------------------------
    def debug_get(self, which):
        ns, sy, sx = self.sgrid if self.sgrid else (0, 0, 0)
        if which < 10:
            out = np.empty(int(np.prod(self.vsize)), np.float32)
        elif which < 20:
            out = np.empty((ns, sy, sx), np.float32)
        elif which == BUF_SIMINSIDE:
            out = np.empty((ns, sy, sx), np.uint8)
        else:
            out = np.empty((ns, sy, sx), np.int32)
        self._ck(self._lib.svr_debug_get(self._h, int(which), _p(out), C.c_size_t(out.nbytes)))
        return out

    def debug_set(self, which, arr):
        a = np.ascontiguousarray(arr)
        self._ck(self._lib.svr_debug_set(self._h, int(which), _p(a), C.c_size_t(a.nbytes)))

    # ---- slice-to-volume registration cost ------------------------------------------------
    def ncc_set_targets(self, targets):
        t = np.ascontiguousarray(targets, np.int16)
        n, ty, tx = t.shape
        self._ck(self._lib.svr_ncc_set_targets(self._h, n, tx, ty, _p(t)))

    def ncc_set_source(self, source=None):
        if source is None:
            self._ck(self._lib.svr_ncc_set_source(self._h, None, None))
        else:
            s = np.ascontiguousarray(source, np.int16)
            self._ck(self._lib.svr_ncc_set_source(self._h, _u3(s.shape[::-1]), _p(s)))

    def ncc_evaluate(self, target_index, matrices):
        idx = np.ascontiguousarray(target_index, np.int32)
        m = np.ascontiguousarray(matrices, np.float64).reshape(len(idx), 16)
        sums = np.zeros((len(idx), 6), np.int64)
        ncc = np.zeros(len(idx), np.float64)
        self._ck(self._lib.svr_ncc_evaluate(self._h, len(idx), _p(idx), _p(m), _p(sums), _p(ncc)))
        return ncc, sums

    # ---- the image pyramid of that registration on the device (csrc/svr_pyr.inc) ------------------------------------------
    def ncc_alloc_targets(self, n, tx, ty):
        """n target planes of ty x tx, all -1, for pyr_level(slot 1) to write into"""
        self._ck(self._lib.svr_ncc_alloc_targets(self._h, int(n), int(tx), int(ty)))

    def pyr_upload(self, slot, images):
        """the unprocessed images of a registration pass: slot 0 the source volume, slot 1 the targets back to back (int16)"""
        a = np.ascontiguousarray(images, np.int16).reshape(-1)
        self._ck(self._lib.svr_pyr_upload(self._h, int(slot), _p(a), C.c_size_t(a.size)))

    def pyr_level(self, slot, offset, in_dims, kernels, resample, out_dims, i2w_out, w2i_in, pads, first_plane=0):
        """svr_pyr_level: one level of len(pads) images of one grid that start at element `offset` of the slot -> (min [n], max [n])
        int32, the range above each padding before the shift (max < min: none).  in_dims / out_dims: (nx, ny, nz); kernels: the
        three blur kernels (None or empty = no pass on that axis); i2w_out / w2i_in: per image the 4x4 (or its first three rows) of
        the level's image-to-world and of the unprocessed grid's world-to-image matrix."""
        n = len(pads)
        imgs = (_PyrImage * n)()
        a = np.asarray(i2w_out, np.float64).reshape(n, -1)[:, :12]
        b = np.asarray(w2i_in, np.float64).reshape(n, -1)[:, :12]
        for i in range(n):
            imgs[i].i2w_out[:] = a[i].tolist()
            imgs[i].w2i_in[:] = b[i].tolist()
            imgs[i].pad = int(pads[i])
        ker = [np.zeros(0) if k is None else np.ascontiguousarray(k, np.float64) for k in kernels]
        mn, mx = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self._ck(self._lib.svr_pyr_level(self._h, int(slot), C.c_size_t(offset), n, (C.c_int * 3)(*[int(v) for v in in_dims]),
                                         _p(ker[0]) if ker[0].size else None, int(ker[0].size), _p(ker[1]) if ker[1].size else None,
                                         int(ker[1].size), _p(ker[2]) if ker[2].size else None, int(ker[2].size), int(bool(resample)),
                                         (C.c_int * 3)(*[int(v) for v in out_dims]), imgs, int(first_plane), _p(mn), _p(mx)))
        return mn, mx

    def _ncc_get(self, which):
        dims = (C.c_int * 3)()
        self._ck(self._lib.svr_ncc_get(self._h, which, dims, None, C.c_size_t(0)))
        out = np.empty((dims[2], dims[1], dims[0]), np.int16)
        self._ck(self._lib.svr_ncc_get(self._h, which, dims, _p(out), C.c_size_t(out.size)))
        return out

    def ncc_get_source(self):
        """the source svr_ncc_evaluate reads, int16 [vz][vy][vx] (read-only copy)"""
        return self._ncc_get(0)

    def ncc_get_targets(self):
        """the whole allocation of target planes svr_ncc_evaluate reads, int16 [n][ty][tx] (read-only copy)"""
        return self._ncc_get(1)

    def nmi_bin_source(self, width):
        """irtkCalculateNumberOfBins' rescaling of the current source, in place (v > 0 -> v // width)"""
        self._ck(self._lib.svr_nmi_bin_source(self._h, int(width)))

    def nmi_evaluate(self, planes_per_eval, target_index, matrices, target_width, target_nbins, source_nbins, histograms=False):
        """svr_nmi_evaluate -> ({n, S_xy, S_x, S_y} float64 [n_eval][4], uint32 joint histograms [n_eval][64][64] or None).
        Evaluation e spans planes_per_eval[e] consecutive entries of target_index / matrices."""
        ppe = np.ascontiguousarray(planes_per_eval, np.int32)
        idx = np.ascontiguousarray(target_index, np.int32)
        m = np.ascontiguousarray(matrices, np.float64).reshape(len(idx), 16)
        w, nb = np.ascontiguousarray(target_width, np.int32), np.ascontiguousarray(target_nbins, np.int32)
        if len(idx) != int(ppe.sum()) or len(w) != len(ppe) or len(nb) != len(ppe):
            raise SvrError("nmi_evaluate: one width and bin count per evaluation, one index and matrix per plane")
        out = np.zeros((len(ppe), 4), np.float64)
        h = np.zeros((len(ppe), 64, 64), np.uint32) if histograms else None
        self._ck(self._lib.svr_nmi_evaluate(self._h, len(ppe), _p(ppe), _p(idx), _p(m), _p(w), _p(nb), int(source_nbins), _p(out),
                                            _p(h) if h is not None else None))
        return out, h

    def lncc_evaluate(self, target_index, matrices, radius=3, maps=False):
        """svr_lncc_evaluate -> ({N, S} int64 [n_eval][2], the k maps int32 [n_eval][ty][tx] (INT32_MIN = not counted) or None): the
        windowed cross correlation of one candidate matrix per target plane, (S / N) / 2^24."""
        idx = np.ascontiguousarray(target_index, np.int32)
        m = np.ascontiguousarray(matrices, np.float64).reshape(len(idx), 16)
        out = np.zeros((len(idx), 2), np.int64)
        k = None
        if maps:
            dims = (C.c_int * 3)()
            self._ck(self._lib.svr_ncc_get(self._h, 1, dims, None, C.c_size_t(0)))
            k = np.zeros((len(idx), dims[1], dims[0]), np.int32)
        self._ck(self._lib.svr_lncc_evaluate(self._h, len(idx), _p(idx), _p(m), int(radius), _p(out), _p(k) if k is not None else None))
        return out, k

    def stack_motion(self, slices):
        """svr_stack_motion on float32 slices [n][...] (already normalised; a slice is flattened to its pixels) ->
        (singular values float64 [n] descending, et, r_min, score): the reference's --useAutoTemplate score of a stack window."""
        a = _f32(slices)
        n = int(a.shape[0]) if a.ndim else 0
        a = a.reshape(n, int(np.prod(a.shape[1:])) if a.ndim > 1 else 1)
        s = np.zeros(max(n, 1), np.float64)
        et, r_min, score = C.c_double(0.0), C.c_int(0), C.c_double(0.0)
        self._ck(self._lib.svr_stack_motion(self._h, _p(a), int(a.shape[1]), n, _p(s), C.byref(et), C.byref(r_min), C.byref(score)))
        return s[:n], et.value, r_min.value, score.value

    def slice_quality(self):
        """svr_slice_quality -> float64 [ns][10]: per slice {n_px, n, sum x, sum y, sum x^2, sum y^2, sum xy, sum e^2, sum |e|, sum w}
        of x = the scaled (bias-corrected) slice against y = the simulated slice, over the M-step's pixels (include/svr_hip.h).
        SimulateSlices first; host.slice_quality_derive turns a row into ncc / rmse / mae / mean weight."""
        if not self.sgrid:
            raise SvrError("slice_quality: initStorageVolumes first")
        out = np.zeros((self.sgrid[0], 10), np.float64)
        self._ck(self._lib.svr_slice_quality(self._h, _p(out)))
        return out

    def slice_ssim(self, radius, c1, c2, want_map=False):
        """svr_slice_ssim -> (float64 [ns][2] = {n_ssim, sum ssim} per slice, the map float32 [ns][sy][sx] or None): the windowed
        structural similarity of the scaled (bias-corrected) slice against the simulated one over the M-step's pixels, box window of
        (2 radius + 1)^2 pixels; the map is NaN where a pixel is not counted (include/svr_hip.h).  SimulateSlices first."""
        if not self.sgrid:
            raise SvrError("slice_ssim: initStorageVolumes first")
        out = np.zeros((self.sgrid[0], 2), np.float64)
        m = np.zeros(self.sgrid, np.float32) if want_map else None
        self._ck(self._lib.svr_slice_ssim(self._h, int(radius), C.c_double(c1), C.c_double(c2), _p(out), _p(m) if m is not None else None))
        return out, m

    def resample_to_reconstruction(self, src, src_from_recon, padding=-1.0, install=False, scale=None, want_volume=True):
        """svr_resample_to_reconstruction: src float32 [nz][ny][nx] on any grid, src_from_recon = source world-to-image x reconstruction
        image-to-world (float64, 3x4 or 4x4) -> (the volume on the reconstruction grid [vz][vy][vx] or None, stats float64 [5] =
        {n, sum v, sum v^2, min, max} of the valid voxels before scaling).  scale: multiply the valid voxels; install: the result becomes
        the reconstructed volume (include/svr_hip.h)."""
        if not self.vsize:
            raise SvrError("resample_to_reconstruction: InitReconstructionVolume first")
        a = _f32(src)
        if a.ndim != 3:
            raise SvrError("resample_to_reconstruction: a [nz][ny][nx] array expected")
        m = np.ascontiguousarray(np.asarray(src_from_recon, np.float64).reshape(-1, 4)[:3])
        out = np.empty(self.vsize[::-1], np.float32) if want_volume else None
        stats = np.zeros(5, np.float64)
        flags = (RESAMPLE_INSTALL if install else 0) | (RESAMPLE_SCALE if scale is not None else 0)
        self._ck(self._lib.svr_resample_to_reconstruction(self._h, _u3(a.shape[::-1]), _p(a), _p(m), C.c_float(padding), int(flags),
                                                          C.c_float(1.0 if scale is None else scale), None if out is None else _p(out), _p(stats)))
        return out, stats

    # ---- a second image through the run's motion and weights (csrc/svr_channel.inc) ------------------------------------------
    def channel_scatter(self, channel, unit_on=None, slice_weights=None, indicator=False, match=0.0):
        """svr_channel_scatter: channel float32 [ns][sy][sx] -> num | den in BUF_ADDON | BUF_CONFIDENCE_MAP (read them with debug_get).
        unit_on: a byte per slice (0 = the slice has no such channel) or None; slice_weights: as SuperresolutionBackproject's;
        indicator: scatter (channel == match) instead of the channel's value."""
        if not self.sgrid:
            raise SvrError("channel_scatter: initStorageVolumes first")
        c = None if channel is None else _f32(channel)
        if c is not None and c.size != int(np.prod(self.sgrid)):
            raise SvrError(f"channel_scatter: expected {self.sgrid}, got {c.shape}")
        u = None if unit_on is None else np.ascontiguousarray(unit_on, np.uint8)
        if u is not None and u.size != self.sgrid[0]:
            raise SvrError("channel_scatter: one unit_on byte per slice expected")
        w = None if slice_weights is None else _f32(slice_weights)
        self._ck(self._lib.svr_channel_scatter(self._h, None if c is None else _p(c), None if u is None else _p(u), None if w is None else _p(w),
                                               CHANNEL_INDICATOR if indicator else 0, C.c_float(match)))

    def channel_finish(self, background=0.0, want_volume=True):
        """svr_channel_finish: num / den where den > 0, `background` elsewhere, in place in BUF_ADDON -> the volume (flat) or None"""
        out = np.empty(int(np.prod(self.vsize)), np.float32) if want_volume else None
        self._ck(self._lib.svr_channel_finish(self._h, C.c_float(background), None if out is None else _p(out)))
        return out

    def channel_vote(self, label, first):
        """svr_channel_vote: the label whose indicator scatter is in BUF_ADDON | BUF_CONFIDENCE_MAP takes the voxels where it beats the best so far"""
        self._ck(self._lib.svr_channel_vote(self._h, C.c_float(label), int(bool(first))))

    def channel_vote_fetch(self, background_label=0.0):
        """svr_channel_vote_fetch -> (labels, confidence), flat float32; ends the vote"""
        n = int(np.prod(self.vsize)) if self.vsize else 0
        lab, conf = np.empty(n, np.float32), np.empty(n, np.float32)
        self._ck(self._lib.svr_channel_vote_fetch(self._h, C.c_float(background_label), _p(lab), _p(conf)))
        return lab, conf

    # SR iterations on a channel with the run's motion and weights held fixed (svr_channel_sr_*): begin, [all-reduce], seed, then per iteration
    # backproject, [all-reduce], update; end hands the volume over and frees the call's buffers
    def channel_sr_begin(self, channel, unit_on=None, slice_weights=None, flags=0):
        """svr_channel_sr_begin: uploads and keeps the channel, svr_channel_scatter's scatter -> BUF_ADDON | BUF_CONFIDENCE_MAP"""
        if not self.sgrid:
            raise SvrError("channel_sr_begin: initStorageVolumes first")
        c = None if channel is None else _f32(channel)
        if c is not None and c.size != int(np.prod(self.sgrid)):
            raise SvrError(f"channel_sr_begin: expected {self.sgrid}, got {c.shape}")
        u = None if unit_on is None else np.ascontiguousarray(unit_on, np.uint8)
        if u is not None and u.size != self.sgrid[0]:
            raise SvrError("channel_sr_begin: one unit_on byte per slice expected")
        w = None if slice_weights is None else _f32(slice_weights)
        self._ck(self._lib.svr_channel_sr_begin(self._h, None if c is None else _p(c), None if u is None else _p(u), None if w is None else _p(w),
                                                int(flags)))

    def channel_sr_seed(self, seed=None):
        """svr_channel_sr_seed: C0 = num / den where den > 0, else 0; cover = den > 0.  seed: a volume that replaces C0's values"""
        s = None if seed is None else _f32(seed)
        if s is not None and s.size != int(np.prod(self.vsize)):
            raise SvrError("channel_sr_seed: a value per voxel expected")
        self._ck(self._lib.svr_channel_sr_seed(self._h, None if s is None else _p(s)))

    def channel_sr_guide(self, guide=None, delta_g=1.0, guide_only=False, flags=None):
        """svr_channel_sr_guide: every later update of this begin..end weighs a pair by the guide's differences too (delta_g: their edge scale;
        guide_only: without the channel's own).  guide: a value per voxel, or None = a copy of the reconstruction as the device holds it now"""
        g = None if guide is None else _f32(guide)
        if g is not None and g.size != int(np.prod(self.vsize)):
            raise SvrError("channel_sr_guide: a value per voxel expected")
        f = (CHANNEL_GUIDE_ONLY if guide_only else 0) if flags is None else int(flags)
        self._ck(self._lib.svr_channel_sr_guide(self._h, None if g is None else _p(g), C.c_float(delta_g), f))

    def channel_sr_backproject(self):
        """svr_channel_sr_backproject: forward projection of the channel volume, residuals, scatter -> BUF_ADDON | BUF_CONFIDENCE_MAP"""
        self._ck(self._lib.svr_channel_sr_backproject(self._h))

    def channel_sr_update(self, adaptive, alpha, lo, hi, delta, lam):
        """svr_channel_sr_update: the SR volume update on the channel volume, clamped to [lo, hi]"""
        self._ck(self._lib.svr_channel_sr_update(self._h, int(bool(adaptive)), C.c_float(alpha), C.c_float(lo), C.c_float(hi), C.c_float(delta),
                                                 C.c_float(lam)))

    def channel_sr_end(self, want_volume=True):
        """svr_channel_sr_end -> the channel volume (flat, 0 outside cover) or None; frees the call's buffers"""
        out = np.empty(int(np.prod(self.vsize)), np.float32) if want_volume else None
        self._ck(self._lib.svr_channel_sr_end(self._h, None if out is None else _p(out)))
        return out

    # ---- S(x) = A exp(-R x) over K volumes, voxel by voxel (csrc/svr_fit.inc) ------------------------------------------------------
    def monoexp_fit(self, vols, x, iterations=0, floor=0.0):
        """svr_monoexp_fit: vols float32 [K][...], x the K abscissae (echo times, b-values) -> (rate, amplitude, rmse, count), float32 arrays
        of vols[0]'s shape.  iterations: Gauss-Newton steps after the weighted log-linear fit; floor: samples at or below it do not count.
        Needs no geometry.  None for vols or x reaches the library as NULL (refused there)."""
        v = None if vols is None else _f32(vols)
        xs = None if x is None else np.ascontiguousarray(x, np.float64).reshape(-1)
        if v is not None and v.ndim < 1:
            raise SvrError("monoexp_fit: vols [K][...] expected")
        k = 0 if v is None else v.shape[0]
        if v is not None and xs is not None and xs.size != k:
            raise SvrError(f"monoexp_fit: {xs.size} abscissae for {k} volumes")
        shape = () if v is None else v.shape[1:]
        n = int(np.prod(shape)) if v is not None else 0
        out = [np.zeros(shape, np.float32) for _ in range(4)]
        self._ck(self._lib.svr_monoexp_fit(self._h, C.c_int(k), None if xs is None else _p(xs), None if v is None else _p(v), C.c_size_t(n),
                                           C.c_int(int(iterations)), C.c_float(floor), *[_p(o) for o in out]))
        return tuple(out)

    # ---- GPU slice-to-volume registration (RC.cuh:326-338) ------------------------------------
    def initRegStorageVolumes(self, W, H, ns, dim=(1.0, 1.0, 1.0)):
        self._reg_grid = (int(ns), int(H), int(W))
        self._ck(self._lib.svr_init_reg_storage_volumes(self._h, _u3((W, H, ns)), _f3(dim)))

    def FillRegSlices(self, sdata, slices_resampled_i2w=None):
        d = _f32(sdata)
        if d.shape != self._reg_grid:
            raise SvrError(f"FillRegSlices: expected {self._reg_grid}, got {d.shape}")
        m = None if slices_resampled_i2w is None else _f32(slices_resampled_i2w).reshape(-1)
        self._ck(self._lib.svr_fill_reg_slices(self._h, _p(d), None if m is None else _p(m)))

    def updateResampledSlicesI2W(self, ofs):
        m = _f32(ofs).reshape(-1)
        if m.size != 16 * self._reg_grid[0]:
            raise SvrError("updateResampledSlicesI2W: one Matrix4 per slice expected")
        self._ck(self._lib.svr_update_resampled_slices_i2w(self._h, _p(m)))

    def prepareSliceToVolumeReg(self, volume=None):
        """Snapshots the engine's current reconstruction (`volume` is ignored; the oracle twin takes it)."""
        self._ck(self._lib.svr_prepare_slice_to_volume_reg(self._h))

    def set_schedule(self, levels=None, steps=None, iterations=None):
        self._ck(self._lib.svr_reg_set_schedule(self._h, int(levels or 0), int(steps or 0), int(iterations or 0)))

    def registerSlicesToVolume(self, transf):
        t = _f32(transf).reshape(-1).copy()
        if t.size != 16 * self._reg_grid[0]:
            raise SvrError("registerSlicesToVolume: one Matrix4 per slice expected")
        self._ck(self._lib.svr_register_slices_to_volume(self._h, _p(t)))
        return t.reshape(-1, 4, 4)

    def evaluate_costs(self, transf, level, active=None):
        ns, H, W = self._reg_grid
        t = _f32(transf).reshape(-1)
        act = None if active is None else np.ascontiguousarray(active, np.int32)
        a = ns if act is None else len(act)
        sim = np.zeros(ns, np.float32)
        dbg = np.zeros((3, a, H, W), np.float32)
        self._ck(self._lib.svr_reg_evaluate_costs(self._h, _p(t), int(level), None if act is None else _p(act), a,
                                                  _p(sim), _p(dbg)))
        return sim, dbg

    def cc_patches(self, ri2w, tmats, level, buffers=None):
        """computeCCpatch for every patch (patchBased2D3DRegistration_gpu2.cu:130-190)."""
        n = self.sgrid[0]
        r, t = _f32(ri2w).reshape(n, 16), _f32(tmats).reshape(n, 16)
        b = None if buffers is None else _f32(buffers)
        out = np.zeros(n, np.float32)
        sums = np.zeros((n, 6), np.float64)
        self._ck(self._lib.svr_pvr_cc_patches(self._h, None if b is None else _p(b), _p(r), _p(t), int(level), _p(out),
                                              _p(sums)))
        return out, sums

    def register_patches(self, ri2w, mo, invmo, transformations):
        """PatchBased2D3DRegistration_gpu2<T>::run (patchBased2D3DRegistration_gpu2.cu:450-566) -> (T [n][16], Tinv [n][16],
        counters {launches, evaluations, patches})."""
        n = self.sgrid[0]
        r, m, mi = (_f32(a).reshape(n, 16) for a in (ri2w, mo, invmo))
        t = _f32(transformations).reshape(n, 16).copy()
        ti = np.zeros((n, 16), np.float32)
        c = np.zeros(3, np.int64)
        self._ck(self._lib.svr_pvr_register_patches(self._h, _p(r), _p(m), _p(mi), _p(t), _p(ti), _p(c)))
        return t, ti, c

    def reg_get(self, which):
        """svr_reg_get: a copy of the state the last evaluate_costs / registerSlicesToVolume left (REG_* above; read-only).
        REG_ACTIVE -> (the active list, the most slices a line-search step of the last run kept, the workgroup size of the
        per-image reductions)."""
        ns, H, W = self._reg_grid
        shape, dt = {REG_TARGETS: ((ns, H, W), np.float32), REG_SUM_A: ((ns,), np.float32), REG_CNT_A: ((ns,), np.int32),
                     REG_SUM_B: ((3, ns), np.float32), REG_CNT_B: ((3, ns), np.int32), REG_MOMENTS: ((3, ns, 3), np.float32),
                     REG_SIMILARITIES: ((5, ns), np.float32), REG_GRADIENT: ((7, ns), np.float32),
                     REG_ACTIVE: ((3 + ns,), np.int32)}[which]
        out = np.zeros(shape, dt)
        self._ck(self._lib.svr_reg_get(self._h, int(which), _p(out), C.c_size_t(out.nbytes)))
        if which == REG_ACTIVE:
            return out[3:3 + out[0]].copy(), int(out[1]), int(out[2])
        return out

    def reg_counters(self):
        c = np.zeros(4, np.int64)
        self._ck(self._lib.svr_reg_counters(self._h, _p(c)))
        return c

    def set_spx_masks(self, masks):
        if masks is None:
            self._ck(self._lib.svr_set_spx_masks(self._h, None))
        else:
            m = np.ascontiguousarray(masks, np.uint8)
            self._ck(self._lib.svr_set_spx_masks(self._h, _p(m)))

    def set_option(self, name, value):
        self._ck(self._lib.svr_set_option(self._h, name.encode(), int(value)))

    def get_option(self, name):
        v = C.c_int(0)
        self._ck(self._lib.svr_get_option(self._h, name.encode(), C.byref(v)))
        return v.value

    def probe_pixel(self, sl, px, py):
        v = np.zeros(4096, np.float32)
        c = np.zeros(3, np.int32)
        self._ck(self._lib.svr_debug_probe_pixel(self._h, int(sl), int(px), int(py), _p(v), _p(c)))
        return v, c

    # ---- measurement --------------------------------------------------------------------
    def timer_enable(self, on=True):
        self._ck(self._lib.svr_timer_enable(self._h, int(bool(on))))

    def timer_reset(self):
        self._ck(self._lib.svr_timer_reset(self._h))

    def timers(self):
        out = {}
        for i, name in enumerate(TIMER_NAMES):
            ms, n = C.c_double(0), C.c_long(0)
            self._ck(self._lib.svr_timer_get(self._h, i, C.byref(ms), C.byref(n)))
            out[name] = (ms.value, n.value)
        return out

    def unit_counts(self):
        o = (C.c_uint64 * 3)()
        self._ck(self._lib.svr_unit_counts(self._h, o))
        return dict(pixels=int(o[0]), live_units=int(o[1]), dead_units=int(o[2]))

    def slab_chunks(self, world, rank):
        """svr_slab_plan: floats per rank of the slab update's reduce-scatter and all-gather messages"""
        a, b = C.c_size_t(0), C.c_size_t(0)
        self._ck(self._lib.svr_slab_plan(self._h, int(world), int(rank), C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def pair_pack(self, which, n_floats):
        """svr_pair_pack: the mask's bounding box of the n_floats / Nv volumes that start at buffer `which`, packed -> (device
        pointer, floats), or (None, 0) where nothing is gained (no mask box, a box over 80 % of the volume): the caller then
        exchanges the whole buffer"""
        ptr, n = C.c_void_p(), C.c_size_t(0)
        self._ck(self._lib.svr_pair_pack(self._h, int(which), C.c_size_t(n_floats), C.byref(ptr), C.byref(n)))
        return ptr.value, int(n.value)

    def pair_unpack(self, which, n_floats):
        """svr_pair_unpack: the packed box (after the collective) back into the volumes"""
        self._ck(self._lib.svr_pair_unpack(self._h, int(which), C.c_size_t(n_floats)))

    def slab_rs_pack(self):
        """svr_slab_rs_pack: addon | cmap at the mask voxels of every rank's slab + halo -> (send, recv) device pointers: send holds
        [world][2][rs_chunk] floats; the reduce-scatter's result, [2][rs_chunk], belongs at recv"""
        s, r = C.c_void_p(), C.c_void_p()
        self._ck(self._lib.svr_slab_rs_pack(self._h, C.byref(s), C.byref(r)))
        return s.value, r.value

    def slab_update(self, adaptive, alpha, min_intensity, max_intensity, delta, lam):
        """svr_slab_update: the reduced sums at recv -> the rank's planes of the volume update -> (send, recv): send holds the rank's
        all-gather part, [ag_chunk] floats; every rank's part, [world][ag_chunk], belongs at recv"""
        s, r = C.c_void_p(), C.c_void_p()
        self._ck(self._lib.svr_slab_update(self._h, int(bool(adaptive)), C.c_float(alpha), C.c_float(min_intensity),
                                           C.c_float(max_intensity), C.c_float(delta), C.c_float(lam), C.byref(s), C.byref(r)))
        return s.value, r.value

    def slab_finish(self):
        """svr_slab_finish: the other ranks' parts at recv go into the new volume, which becomes the current one"""
        self._ck(self._lib.svr_slab_finish(self._h))

    def read_floats(self, ptr, n):
        """n floats at a raw device pointer of this engine (slab_rs_pack, slab_update, device_ptr), behind everything queued on its stream"""
        return self.device_read(ptr, n, np.float32)

    def write_floats(self, ptr, arr):
        """a float32 array to a raw device pointer of this engine, behind everything queued on its stream and complete on return"""
        self.device_write(ptr, _f32(arr))

    def device_read(self, ptr, n, dtype=np.float32):
        """n items of `dtype` at a raw device pointer of this engine, behind everything queued on its stream"""
        out = np.empty(int(n), dtype)
        self.stream_sync()
        _hip_memcpy(_p(out), ptr, out.nbytes, 2)
        return out

    def device_write(self, ptr, array):
        """an array (its own dtype) to a raw device pointer of this engine, behind everything queued on its stream and complete on return"""
        a = np.ascontiguousarray(array).reshape(-1)
        self.stream_sync()
        _hip_memcpy(ptr, _p(a), a.nbytes, 1)

    # ---- the unit-level EM on the device (csrc/svr_em.inc): what the C++ host objects drive, one call each ----------------
    def slice_em_setup(self, n_global, world, rank, rank_lo, order=None, step=0.0001):
        """svr_slice_em_setup: rank_lo[world + 1] = the ranks' ranges of the host numbering (this rank's must hold the context's
        slices), order[k] = the reference index of host unit k (None: the same numbering)"""
        lo = np.ascontiguousarray(rank_lo, np.int32)
        if len(lo) != int(world) + 1:
            raise ValueError("rank_lo must have world + 1 entries")
        o = None if order is None else np.ascontiguousarray(order, np.int32)
        if o is not None and len(o) != int(n_global):
            raise ValueError("order must have n_global entries")
        self._ck(self._lib.svr_slice_em_setup(self._h, int(n_global), int(world), int(rank), _p(lo), None if o is None else _p(o), C.c_double(step)))
        self._em_n = int(n_global)                             # (set on success only: a setup refused for its ranges leaves the previous one in force, one refused later leaves none)

    def slice_em_set_patch_form(self, source_ref=None):
        """svr_slice_em_set_patch_form: source_ref[t] = the reference index of the unit whose potential reference unit t reads, -1 = none"""
        s = None if source_ref is None else np.ascontiguousarray(source_ref, np.int32)
        if s is not None and len(s) != getattr(self, "_em_n", -1):
            raise ValueError("source_ref must have n_global entries")
        self._ck(self._lib.svr_slice_em_set_patch_form(self._h, None if s is None else _p(s)))

    def slice_em_set_state(self, weights, excluded, scalars5, em3):
        w, e = _f32(weights), np.ascontiguousarray(excluded, np.uint8)
        if len(w) != getattr(self, "_em_n", len(w)) or len(e) != len(w):
            raise ValueError("weights and excluded must have n_global entries")
        s5, e3 = np.ascontiguousarray(scalars5, np.float64), _f32(em3)
        if len(s5) != 5 or len(e3) != 3:
            raise ValueError("scalars5 / em3")
        self._ck(self._lib.svr_slice_em_set_state(self._h, _p(w), _p(e), _p(s5), _p(e3)))

    def mstep_estep_device(self, it, step=0.0001):
        """svr_mstep_estep_device -> (send, recv, floats per rank): the device pointers of the rank's packed {potential, scale,
        inside} and of where every rank's belong (one rank: the same buffer)"""
        s, r, n = C.c_void_p(), C.c_void_p(), C.c_size_t(0)
        self._ck(self._lib.svr_mstep_estep_device(self._h, int(it), C.c_float(step), C.byref(s), C.byref(r), C.byref(n)))
        return s.value, r.value, int(n.value)

    def slice_em_run(self):
        self._ck(self._lib.svr_slice_em_run(self._h))

    def slice_em_apply_weights(self):
        self._ck(self._lib.svr_slice_em_apply_weights(self._h))

    def slice_em_fetch(self):
        """svr_slice_em_fetch -> dict(scale, weight, potential, inside [n_global], scalars5 (float64), em3)"""
        n = self._em_n if getattr(self, "_em_n", 0) > 0 else 1
        sc, w, pot = (np.zeros(n, np.float32) for _ in range(3))
        ins, s5, e3 = np.zeros(n, np.uint8), np.zeros(5, np.float64), np.zeros(3, np.float32)
        self._ck(self._lib.svr_slice_em_fetch(self._h, _p(sc), _p(w), _p(pot), _p(ins), _p(s5), _p(e3)))
        return dict(scale=sc, weight=w, potential=pot, inside=ins.astype(bool), scalars5=s5, em3=e3)

    def mstep_partial(self, world):
        """svr_mstep_partial -> (send, recv): this rank's M-step sums (8 doubles, five used) and where the ranks' [world][8] belong"""
        s, r = C.c_void_p(), C.c_void_p()
        self._ck(self._lib.svr_mstep_partial(self._h, int(world), C.byref(s), C.byref(r)))
        return s.value, r.value

    def mstep_estep_ranks(self, world, it, step, sigma, mix):
        """svr_mstep_estep_ranks (after mstep_partial and the all-gather) -> (em3, slice potentials)"""
        em = np.array([sigma, mix, 0.0], np.float32)
        pot = np.zeros(self.sgrid[0], np.float32)
        self._ck(self._lib.svr_mstep_estep_ranks(self._h, int(world), int(it), C.c_float(step), _p(em), _p(pot), None, None))
        return em, pot

    def cell_stats(self):
        o = (C.c_uint64 * 8)()
        self._ck(self._lib.svr_cell_stats(self._h, o))
        return dict(items=int(o[0]), runs=int(o[1]), sorted_pixels=int(o[2]), staging_bytes=int(o[3]), gather_items=int(o[4]),
                    gather_runs=int(o[5]), gather_partial_bytes=int(o[6]), cell=(int(o[7]) >> 32, int(o[7]) & 0xFFFFFFFF))

    def fallbacks(self):
        """launches that left the cell path since the context was made (svr_fallbacks): zeros on every bench workload"""
        o = (C.c_uint64 * 4)()
        self._ck(self._lib.svr_fallbacks(self._h, o))
        return dict(scatter_to_atomics=int(o[0]), gather_to_tiles=int(o[1]), gauss1_to_tiles=int(o[2]), tiles_rerun=int(o[3]))

    def clock_probe(self, chain=1 << 20):
        """(ms, chain): the time of `chain` packed f32 fmas per lane (eight independent chains) on 4 wavefronts per SIMD of the whole chip
        (svr_clock_probe) -- a fixed number of shader cycles at the vector pipe's full issue rate: boxes compare by it"""
        ms = C.c_double()
        self._ck(self._lib.svr_clock_probe(self._h, int(chain), C.byref(ms)))
        return ms.value, int(chain)

    def counters(self):
        o = (C.c_uint64 * 8)()
        self._ck(self._lib.svr_counters(self._h, o))
        return dict(Vs=int(o[0]), active=int(o[1]), Va=int(o[2]), Nv=int(o[3]), slices=int(o[4]),
                    tiles=int(o[5]), fallback_tiles=int(o[6]), rerun8_tiles=int(o[7]))


def device_count():
    """HIP devices visible to this process (0 without a GPU)"""
    return int(load_library().svr_device_count())


def sync_gpu(rec: Reconstruction, prob, quality_factor: float = 2.0):
    """irtkReconstruction::SyncGPU + generatePSFVolume + UpdateGPUTranformationMatrices
    (irtkReconstructionGPU.cc:249-328, 1496-1610, 372-401): upload one problem to the engine."""
    from . import geometry as geo

    vs, vd = prob.vsize, prob.vdim
    rec.InitReconstructionVolume(vs, vd, None, 12.0)
    rec.setMask(vs, vd, prob.mask, 12.0)
    ns, sy, sx = prob.slices.shape
    rec.initStorageVolumes((sx, sy, ns), tuple(prob.slice_dim[0]))
    rec.FillSlices(prob.slices, prob.sizes_x, prob.sizes_y)
    rec.setSliceDims(prob.slice_dim, quality_factor)
    a = geo.ImageAttributes(128, 128, 128, *[float(d) for d in vd])   # PSF_SIZE 128, RC.cuh:56
    rec.generatePSFVolume(None, (128, 128, 128), tuple(prob.slice_dim[0]), vd,
                          geo.to_matrix4(geo.image_to_world(a)), geo.to_matrix4(geo.world_to_image(a)),
                          quality_factor)
    rec.SetSliceMatrices(prob.slice_t, prob.slice_tinv, prob.slice_i2w, prob.slice_w2i, prob.slice_i2w,
                         prob.slice_w2i, prob.recon_i2w, prob.recon_w2i)
