/*
 * svr_host.h -- the host algorithm object above the engine, in the reference's own language.
 *
 * C++ class `svr::irtkReconstruction`: the GPU-path operator surface of the reference's
 * irtkReconstruction (source/reconstructionGPU2/irtkReconstructionGPU.cc, "RG.cc";
 * include/irtkReconstructionGPU.h, "RG.h") with the same method and member names, driving one
 * engine context (include/svr_hip.h) per process:
 *   InitializeEMValuesGPU RG.cc:2905-2919      InitializeEMGPU RG.cc:2921-2953
 *   GaussianReconstructionGPU RG.cc:2695-2762  SimulateSlicesGPU RG.cc:1163-1175
 *   InitializeRobustStatisticsGPU RG.cc:2988-3019   EStepGPU RG.cc:3184-3440
 *   ScaleGPU RG.cc:3751-3757   SuperresolutionGPU RG.cc:4024-4036   MStepGPU RG.cc:4214-4223
 *   MaskVolumeGPU RG.cc:5319-5323   ScaleVolumeGPU / RestoreSliceIntensitiesGPU RG.cc:4216,4653
 *   SetSmoothingParameters RG.h:605-612
 * and the reconstruction part of main()'s loop (reconstruction.cc:930-1140) as
 * reconstruct_iteration() / sr_iteration().
 *
 * Multi-GPU: one process per GPU; the slices are sharded, the collectives are supplied by the
 * launcher through `svr_collectives` (bench.py plugs torch.distributed/RCCL in; NULL = one rank).
 * A plain C-ABI (svrh_*) over the class is exported for bindings and tests.
 */
#ifndef SVR_HOST_H
#define SVR_HOST_H

#include <stddef.h>

#include "svr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* collectives supplied by the launcher; every callback returns 0 on success.
 * struct_size (first member, since round 5): sizeof(svr_collectives) of the header the LAUNCHER was built against.  The host objects copy
 * that many bytes and take every member beyond them as NULL / 0 -- a launcher built against an older (shorter) version of this struct
 * keeps working and simply gets the all-reduce + replicated update; 0 or anything smaller than the members up to allgather_slices is
 * refused by svrh_create / pvrh_create_sharded.  (Rounds 1-4 had no such member: launchers of that age must be rebuilt, INTEGRATION.md.) */
typedef struct svr_collectives {
  size_t struct_size;
  void *user;
  int rank, world;
  /* in-place sum of the float[2*Nv] device buffer at `device_ptr` over all ranks */
  int (*allreduce_volume_pair)(void *user, void *device_ptr, size_t n_floats);
  /* in-place reduction of a small host vector; op: 0 sum, 1 min, 2 max */
  int (*allreduce_host)(void *user, double *data, int n, int op);
  /* gather the per-slice vectors of all ranks (rank order = slice order) into global[n_global] */
  int (*allgather_slices)(void *user, const float *local, int n_local, float *global_out, int n_global);
  /* device buffers, on the engine's stream or ordered behind it (NULL: the host objects all-reduce the volume pair and run the volume
   * update replicated instead of by z-slabs, csrc/svr_slab.inc):
   * recv[n] = sum over ranks r' of send_{r'}[rank * n .. rank * n + n)   (send = float[world * n]) */
  int (*reduce_scatter_device)(void *user, const void *send, void *recv, size_t n_floats_per_rank);
  /* recv[r * n .. r * n + n) = send_r[0 .. n) for every rank r   (recv = float[world * n]) */
  int (*allgather_device)(void *user, const void *send, void *recv, size_t n_floats_per_rank);
  /* 1: the three device-buffer callbacks enqueue on the engine's stream (svr_get_stream) -- the host objects then launch scatter,
   * collective and volume update back to back without waiting for the device.  0: the host objects synchronise the engine's stream
   * before every device-buffer callback (its input may still be in flight there), and the callback returns with its result complete. */
  int on_engine_stream;
} svr_collectives;
/* the smallest struct_size the host objects accept: everything up to and including allgather_slices */
#define SVR_COLLECTIVES_MIN_SIZE (offsetof(svr_collectives, allgather_slices) + sizeof(void *))

/* ---- the collectives on RCCL, bound directly (csrc/svr_rccl.cpp) ---------------------------------------------------
 * One communicator per rank = per GPU: a process of its own (bench.py) or a thread of the command line (`-d 0 1 ..`).
 * Replaces the reference's per-device worker threads with their reduce on GPU 0 (reconstruction_cuda2.cu:1413-1457,
 * 2225-2239).  The volume pair is all-reduced in place on the engine's stream.  id128 = ncclUniqueId made by ONE rank
 * (svr_comm_unique_id) and handed to all; svr_comm_create blocks until all `world` ranks have called it. */
typedef struct svr_comm svr_comm;
int svr_comm_unique_id(char id128[128]);
svr_comm *svr_comm_create(int rank, int world, const char id128[128], svr_ctx *engine);
int svr_comm_rebind(svr_comm *c, svr_ctx *engine);                  /* the same communicator for another engine context on the same device */
const svr_collectives *svr_comm_collectives(svr_comm *c);
int svr_comm_world(svr_comm *c);                                     /* ncclCommCount */
int svr_comm_allreduce_host(svr_comm *c, double *data, int n, int op); /* op: 0 sum, 1 min, 2 max */
const char *svr_comm_last_error(const svr_comm *c);
void svr_comm_destroy(svr_comm *c);
/* the ranks of ONE process (the command line's `-d 0 1 2 ..`, one thread and one engine context per rank): RCCL
 * communicators when the devices are distinct, an exchange through host memory under a thread barrier when a device is
 * named more than once (RCCL refuses that; a test mode for one-GPU boxes).  svr_group_join is called by every rank from its
 * own thread and blocks until all have joined; NULL for world 1. */
typedef struct svr_group svr_group;
svr_group *svr_group_create(int world, const int *devices);
int svr_group_uses_rccl(const svr_group *g);
const svr_collectives *svr_group_join(svr_group *g, int rank, svr_ctx *engine);
void svr_group_destroy(svr_group *g);

typedef struct svrh_recon svrh_recon;

/* irtkReconstruction(std::vector<int> dev, bool useCPUReg)  RG.cc:159-221; the engine context is
 * created and filled (SyncGPU, RG.cc:249-328) by the caller.  [slice_lo, slice_hi) = this rank's
 * slices out of n_slices_global. */
svrh_recon *svrh_create(svr_ctx *engine, int n_slices_global, int slice_lo, int slice_hi,
                        const svr_collectives *coll_or_null);
void svrh_destroy(svrh_recon *r);
const char *svrh_last_error(const svrh_recon *r);

void svrh_set_intensity_range(svrh_recon *r, double min_intensity, double max_intensity); /* RG.cc:2937-2951 */
void svrh_set_smoothing_parameters(svrh_recon *r, double delta, double lambda);             /* RG.h:605-612 */
void svrh_set_force_excluded(svrh_recon *r, const int *idx, int n);                         /* RG.h:614-617 */
/* `intensity_matching` of reconstruction.cc:114,183 (--no_intensity_matching 0): off = no Bias / Scale / NormaliseBias in the SR
 * iterations (reconstruction.cc:1018-1045, 1062-1076); the scales stay 1 */
void svrh_set_intensity_matching(svrh_recon *r, int on);

/* disableBiasCorrection() RG.cc:234-238 / SetSigma RG.h:376; BiasGPU RG.cc:3904-3913, NormaliseBiasGPU RG.cc:4653 */
int svrh_set_bias_correction(svrh_recon *r, int enable, double sigma_bias);
/* GlobalBiasCorrectionOn/Off and SetLowIntensityCutoff (RG.h:398-404, 596-602; reconstruction.cc:451, 775-778): global = 1
 * makes CorrectBias skip the per-slice mean (the reference's GPU path has no global correction) and skips NormaliseBias;
 * the cutoff (clamped to [0, 1]) reaches SuperresolutionGPU, which does not use it */
int svrh_set_bias_options(svrh_recon *r, int global_bias_correction, double low_intensity_cutoff);
int svrh_bias_gpu(svrh_recon *r);
int svrh_normalise_bias_gpu(svrh_recon *r, int iter);
/* svr_channel_scatter (include/svr_hip.h) over this rank's slices -- channel_local / unit_on_local: the rank's own part, in its own
 * numbering -- with the slice weights SuperresolutionGPU would scatter with; in a sharded run num | den (SVR_BUF_ADDON |
 * SVR_BUF_CONFIDENCE_MAP) are then all-reduced like the pair of the non-slab SR update, so every rank holds the same sums.  Collective.
 * The caller finishes (svr_channel_finish) or votes (svr_channel_vote) on the engine. */
int svrh_channel_reconstruct(svrh_recon *r, const float *channel_local, const unsigned char *unit_on_local, int flags, float match);
/* That average refined by n super-resolution iterations with the run's motion and weights held fixed (svr_channel_sr_*, include/svr_hip.h;
 * the command line's --channelIterations).  Collective: begin, all-reduce of addon | cmap as above, seed; then n times backproject, the same
 * all-reduce, and the volume update replicated on every rank (no slab update).  delta_c and lambda_c are the user's values, made into the
 * engine's the way svrh_set_smoothing_parameters makes the primary's (lambda_c delta_c^2, alpha = min(1, 0.05 / lambda_c), the object's
 * adaptive flag); [lo, hi] clamps the channel.  n = 0 returns the average.  out_or_null: the channel volume, 0 where no slice with a channel
 * reaches.  Whatever fails, the engine's call is ended and its buffers are freed. */
int svrh_channel_superresolve(svrh_recon *r, const float *channel_local, const unsigned char *unit_on_local, int n, double delta_c, double lambda_c,
                              float lo, float hi, float *out_or_null);
/* The same with the update guided by a volume's edges (svr_channel_sr_guide, include/svr_hip.h; the command line's --channelGuide), collective in the
 * same way: the guide is set after the seed on every rank -- guide_or_null [nvox] host floats, the same on every rank, or NULL = the rank's
 * reconstruction as the device holds it, which every rank holds alike -- and the update stays replicated.  delta_g: the guide's edge scale, in the
 * guide's units, finite and positive; guide_only != 0: the channel's own differences leave the weight (delta_c still scales lambda_c).
 * svrh_channel_superresolve is this call without a guide. */
int svrh_channel_superresolve_guided(svrh_recon *r, const float *channel_local, const unsigned char *unit_on_local, int n, double delta_c, double lambda_c,
                                     float lo, float hi, float *out_or_null, const float *guide_or_null, double delta_g, int guide_only);

int svrh_initialize_em_values_gpu(svrh_recon *r);
int svrh_gaussian_reconstruction_gpu(svrh_recon *r);
int svrh_simulate_slices_gpu(svrh_recon *r);
int svrh_initialize_robust_statistics_gpu(svrh_recon *r);
int svrh_estep_gpu(svrh_recon *r);
int svrh_scale_gpu(svrh_recon *r);
int svrh_superresolution_gpu(svrh_recon *r, int iter);
int svrh_mstep_gpu(svrh_recon *r, int iter);
int svrh_mask_volume_gpu(svrh_recon *r);
int svrh_scale_volume_gpu(svrh_recon *r);
/* one SR iteration of reconstruction.cc:1013-1108 (with BiasGPU / NormaliseBiasGPU when bias correction is enabled) */
int svrh_sr_iteration(svrh_recon *r, int i);
/* Gaussian init + robust-statistics init + rec_iterations SR iterations + MaskVolume
 * (reconstruction.cc:930-1140) */
int svrh_reconstruct_iteration(svrh_recon *r, int rec_iterations);

/* ---- GPU slice-to-volume registration, host side (irtkReconstructionGPU.cc:2104-2290) ------------
 * irtkImageAttributes subset of one slice (z size 1): voxel counts and sizes, axes, origin = world
 * position of the image centre (IRTKSimple2/image++/src/irtkBaseImage.cc:79-147). */
typedef struct svr_image_attr {
  int nx, ny, nz;
  double dx, dy, dz;
  double xaxis[3], yaxis[3], zaxis[3], origin[3];
} svr_image_attr;
/* PrepareRegistrationSlices RG.cc:2104-2181: resample this rank's slices to the reconstruction's voxel
 * size with irtkResamplingWithPadding (padding -1), pack plane 0 of each into the padded grid and hand it
 * to the engine (initRegStorageVolumes + FillRegSlices).  slices [n_local][sy][sx]. */
int svrh_prepare_registration_slices(svrh_recon *r, const float *slices, int sx, int sy, const svr_image_attr *attrs,
                                     double recon_voxel);
/* SliceToVolumeRegistrationGPU RG.cc:2214-2290: transformations = row-major double 4x4 per local slice
 * (`_transformations_gpu`), updated in place; the engine registers against its current reconstruction. */
int svrh_slice_to_volume_registration_gpu(svrh_recon *r, double *transformations);
/* resampled grid of the last svrh_prepare_registration_slices: {x, y, slices} and a copy of the packed data */
int svrh_get_registration_slices(svrh_recon *r, int size3[3], float *data_or_null);

/* ---- NIfTI-1 I/O with the reference's image conventions (csrc/svr_io.cpp) ------------
 * read : .nii / .nii.gz, any of uint8/int8/int16/uint16/int32/uint32/float32/float64, either byte order,
 *        scl_slope/scl_inter applied; geometry from the qform, else the sform, else the default matrix, as
 *        irtkFileNIFTIToImage::ReadHeader does (irtkFileNIFTIToImage.cc:168-345): axes = matrix columns /
 *        voxel size, origin = world position of the centre voxel.  *data is malloc'ed float[nx*ny*nz*nt]
 *        (x fastest), release with svr_free.
 * write: float32 single-file NIfTI-1, qform_code 1 from the image-to-world matrix, sform_code 0
 *        (irtkImageToFileNIFTI.cc:65-145, irtkNIFTI.h:84-160); ".gz" suffix = gzip. */
int svr_nifti_read(const char *path, svr_image_attr *attr, int *nt_or_null, float **data, char err[256]);
int svr_nifti_write(const char *path, const svr_image_attr *attr, const float *data, char err[256]);
void svr_free(void *p);
/* IRTK rigid transformation files (`dof`, the reference's -t option): big-endian {815007, 2, 6} + tx ty tz rx ry rz
 * as doubles (irtkRigidTransformation.cc:392-451); matrix16_or_null = UpdateMatrix's 4x4 (:26-53), row-major. */
int svr_dof_read(const char *path, double params6[6], double *matrix16_or_null, char err[256]);
int svr_dof_write(const char *path, const double params6[6], char err[256]);
/* The number of host threads worth starting: the CPUs of the affinity mask, cut to the cgroup's CPU quota (cpu.max, or
 * cpu.cfs_quota_us / cpu.cfs_period_us) -- a container with 256 visible CPUs and a quota of 16 loses whole scheduler
 * periods to throttling when a pool starts 128 threads.  SVR_HOST_THREADS overrides.  Used by the registration's work
 * pool, the pre-processing of the command lines and the NIfTI writer. */
int svr_host_threads(void);
/* The quality report of a finished run (the command line's --sliceReport; a deviation from the reference, whose
 * irtkReconstruction::SlicesInfo, irtkReconstructionGPU.cc:4937-4975, is never called by its main()).
 * svr_slice_quality_derive: one row of svr_slice_quality's sums -> derived4 = {ncc, rmse, mae, mean_weight}, in double:
 *   ncc = (Sxy - Sx Sy / n) / sqrt((Sxx - Sx^2 / n)(Syy - Sy^2 / n)), nan when n < 2 or the product under the root is <= 0;
 *   rmse = sqrt(See / n), mae = S|e| / n, mean_weight = Sw / n, all nan when n = 0.
 * svr_slice_report_write: a tab-separated file, a header and one row per slice in the order of the arrays: SlicesInfo's
 *   stack_index included excluded outside weight scale TranslationX TranslationY TranslationZ RotationX RotationY RotationZ
 * (included = weight >= 0.5 and inside, excluded = weight < 0.5 and inside, outside = not inside; params6 [n][6] as
 * svrh_irtk_rigid_parameters gives them), then n_px n ncc rmse mae mean_weight from sums [n][SVR_SLICE_QUALITY_SUMS].  nan is
 * written as `nan`. */
void svr_slice_quality_derive(const double sums[SVR_SLICE_QUALITY_SUMS], double derived4[4]);
int svr_slice_report_write(const char *path, int n_slices, const int *stack_index, const float *slice_weight, const unsigned char *slice_inside,
                           const float *scale, const double *params6, const double *sums, char err[256]);
/* svr_slice_report_write_ex: the same file; with ssim_sums [n][2] (svr_slice_ssim's {n_ssim, S ssim}) and structural [n] (both or
 * neither) three more columns follow mean_weight:  ssim (S ssim / n_ssim, nan when n_ssim = 0)  n_ssim  structural (0 / 1).  With both
 * NULL it writes what svr_slice_report_write writes. */
int svr_slice_report_write_ex(const char *path, int n_slices, const int *stack_index, const float *slice_weight, const unsigned char *slice_inside,
                              const float *scale, const double *params6, const double *sums, const double *ssim_sums_or_null,
                              const unsigned char *structural_or_null, char err[256]);

/* ---- Structural slice exclusion (the command line's --structural; a deviation from the reference) ----------------------
 * svr_structural_decide: the rule, pure host code in double.  sums [ns][2] = svr_slice_ssim's {n_ssim, S ssim};  q = S ssim / n_ssim.
 * A slice is judged iff eligible[i] and n_ssim >= min_pixels (and n_ssim > 0, and q is a number); otherwise q_out[i] = nan and the
 * slice is never excluded.  Per stack (stack_index), over its judged slices: median = the middle value, or the mean of the two middle
 * values for an even count;  MAD = the median of |q - median|;  exclude iff q < median - max((k_mad 1.4826) MAD, min_drop).  A stack
 * with fewer than 4 judged slices excludes nothing.  Deterministic: ties in the sort are broken by slice index.  SVR_E_ARG for a
 * missing array or a negative / nan k_mad or min_drop.
 * svrh_set_structural: switches the evaluation inside svrh_reconstruct_iteration on (off by default: nothing below then runs).
 *   stack_index_global [n_slices_global], in the object's numbering; copied.  radius 1 .. 7.
 * svrh_structural_evaluate (collective): svr_slice_ssim on this rank's slices as they stand -- c1 = (0.01 L)^2, c2 = (0.03 L)^2 with
 *   L = max - min intensity -- after settling the unit-level state; sharded, the ranks' rows are summed (every row has one non-zero
 *   contributor, so the sum is exact); then every rank decides alike.  eligible = inside the mask, not force-excluded, not a small
 *   slice; a slice that is structurally excluded now is judged again (the set is not sticky).  The result becomes `pending`.
 *   svrh_reconstruct_iteration runs it after its last SR iteration, before MaskVolume: that iteration's forward projection is the
 *   newest volume's, so none is made.  At its start `pending` becomes the set `in force`: merged into the slices the slice-level EM
 *   leaves out and given weight 0 where the force-excluded slices are, i.e. treated as --force_exclude treats a slice, for that outer
 *   iteration only.  Registration still moves such a slice.  In the first outer iteration nothing is in force.
 * svrh_get_structural: q (nan = not judged) and n_ssim of the last evaluation, and the two sets; any pointer may be NULL. */
int svr_structural_decide(int ns, const int *stack_index, const double *sums /* [ns][2] */, const unsigned char *eligible, int min_pixels,
                          double k_mad, double min_drop, double *q_out /* [ns] */, unsigned char *exclude_out /* [ns] */);
int svrh_set_structural(svrh_recon *r, int enable, int radius, double k_mad, double min_drop, int min_pixels, const int *stack_index_global);
int svrh_structural_evaluate(svrh_recon *r);
int svrh_get_structural(svrh_recon *r, double *q, double *n_ssim, unsigned char *in_force, unsigned char *pending);

/* The numbering of a sharded run (round 5).  A launcher may deal the units to the ranks in any order -- e.g. the r-th part of EVERY stack
 * to rank r, so that a rank's slices are neighbours in space and it stages 1/N of the volume's work items instead of those of whole
 * stacks (csrc/svr_shard.h spatial_order; fetalreconstruction_amd/sharding.py shard_units) -- by uploading them in that order and
 * telling the host object: order[k] = index in the REFERENCE's order (stack after stack, slice after slice) of unit k of the numbering
 * this object and its engine use (n_slices_global entries, a permutation; NULL = the same numbering).  Per-unit vectors handed to or
 * returned by svrh_* / pvrh_* (scale, weights, potentials, force-excluded indices, transformations) are in the object's numbering;
 * whatever the reference computes ACROSS units in unit order -- the sums of the slice-level EM (RG.cc:3282-3420), the patch-based
 * path's within-stack indexing of the potentials (patchBasedRobustStatistics_gpu.cu:256-276) -- is computed in the reference's order. */
int svrh_set_unit_order(svrh_recon *r, const int *order_or_null);
/* test hook: a world-1 run goes through the launcher's collectives like a sharded one (instead of an environment variable) */
void svrh_force_collectives(svrh_recon *r, int on);
/* sharded runs: 1 (default) = the volume update by z-slabs when the launcher supplies reduce_scatter_device / allgather_device
 * (csrc/svr_slab.inc), 0 = all-reduce of the pair + the update replicated on every rank.  Identical on every rank either way; the two
 * forms are bit-equal to each other when the collectives add the ranks in rank order (host-staged / gloo), equal to a float sum's last
 * bits over RCCL. */
void svrh_set_slab_update(svrh_recon *r, int on);

/* state read-back: global per-slice vectors (length n_slices_global) and the EM scalars
 * scalars8 = {sigma, mix, m, mean_s, mean_s2, sigma_s, sigma_s2, mix_s}.  Sharded runs: COLLECTIVE -- the scale vector and
 * slice_inside of the other ranks travel with a rank's next exchange, so every rank must call this together (it completes
 * them with one exchange if any are pending). */
int svrh_get_state(svrh_recon *r, float *scale, float *slice_weight, float *slice_potential,
                   unsigned char *slice_inside, double scalars8[8]);

/* ---- the reference's default (CPU / IRTK) registration schedule around the batched NCC cost (csrc/irtk_reg.cpp) ----
 * irtkImageRigidRegistrationWithPadding::Run (3 levels, Gaussian blurring + resampling with padding per level, gradient
 * descent with 4 step halvings and up to 20 iterations per step, cross correlation) restated on the host, with every
 * similarity evaluation going through svr_ncc_evaluate -- all targets that share a source advance in lock step, one
 * batched call per optimiser step.  `backend` NULL = the engine `ctx`; tests pass the CPU oracle's evaluator instead. */
typedef struct svr_ncc_backend {
  void *user;
  int (*set_targets)(void *user, int n, int tx, int ty, const int16_t *targets);
  int (*set_source)(void *user, const uint32_t size[3], const int16_t *source);
  int (*evaluate)(void *user, int n_eval, const int *target_index, const double *matrices, int64_t *sums6, double *ncc_or_null);
} svr_ncc_backend;
/* irtkReconstruction::StackRegistrations (irtkReconstructionGPU.cc:849-1001): every stack against the (masked) template
 * stack; transformations: row-major double [n][16], in/out.  stacks[i]: double [nz][ny][nx] of attrs[i].
 * flags: SVRH_STACKREG_KEEP_ORIGIN = irtkStack3D3DRegistration<T>::run of the patch-based command line
 * (irtkStack3D3DRegistration.cpp:164-228), whose ResetOrigin is a no-op (arguments by value). */
#define SVRH_STACKREG_KEEP_ORIGIN 1
int svrh_stack_registrations(svr_ctx *ctx, const svr_ncc_backend *backend, int n_stacks, const svr_image_attr *attrs,
                             const double *const *stacks, double *transformations, int template_number,
                             const svr_image_attr *mask_attr, const double *mask_or_null, int flags, long *n_evaluations_or_null,
                             char err[256]);
/* irtkReconstruction::SliceToVolumeRegistration (irtkReconstructionGPU.cc:1991-2059, 2291-2303): every slice against the
 * current reconstruction.  slices: the padded grid float [n][sy][sx] (-1 = padding), attrs[i]: slice i's attributes.
 * flags: SVRH_S2V_NO_RESAMPLE = the patch-to-volume registration the patch-based command line actually runs
 * (patchBased2D3DRegistration<T>::runHybrid + ParallelPatchToVolumeRegistration, patchBased2D3DRegistration.cpp:88-225): the
 * same schedule on the patches as they are. */
#define SVRH_S2V_NO_RESAMPLE 1
int svrh_slice_to_volume_registration(svr_ctx *ctx, const svr_ncc_backend *backend, int n_slices, const float *slices, int sx, int sy,
                                      const svr_image_attr *attrs, double *transformations, const svr_image_attr *recon_attr,
                                      const float *reconstructed, int flags, long *n_evaluations_or_null, char err[256]);
/* irtkReconstruction::PackageToVolume (irtkReconstructionGPU.cc:5096-5192) with SplitImage / SplitImageEvenOdd /
 * SplitImageEvenOddHalf / HalfImage (:4979-5094): the packages (interleaved sub-stacks) of every stack are registered to
 * the reconstruction as 3-D targets and their transformations handed to their slices.  pack_num[i]: packages of stack i;
 * transformations: one per slice, double [n_slices][16], in/out. */
int svrh_package_to_volume(svr_ctx *ctx, const svr_ncc_backend *backend, int n_stacks, const svr_image_attr *attrs, const double *const *stacks,
                           const int *pack_num, int evenodd, int half, int half_iter, double *transformations,
                           const svr_image_attr *recon_attr, const float *reconstructed, long *n_evaluations_or_null, char err[256]);
/* ---- normalised mutual information (the reference's --useNMI: GuessParameterSliceToVolume(true), IRRWP.cc:304-321) ----------
 * The same schedules with irtkNormalisedMutualInformationSimilarityMetric (64 bins, irtkCalculateNumberOfBins per image and
 * level) instead of cross correlation; similarity SVRH_SIM_CC = the entry points above.  `nmi_backend` NULL = the engine
 * (svr_nmi_evaluate); tests pass a CPU evaluator that returns one joint histogram per evaluation: hist[n_eval][64][64],
 * [source bin][target bin], zero outside target_nbins[e] x source_nbins.  Evaluation e spans planes_per_eval[e] consecutive
 * entries of target_index / matrices (as for svr_nmi_evaluate); the targets are handed over unbinned (the evaluator takes
 * v / target_width[e]), the source binned.  The schedule turns every histogram into {n, S_xy, S_x, S_y} with the serial loops
 * of irtkHistogram_2D (svrh_nmi_sums) -- the engine's sums equal them bit for bit. */
#define SVRH_SIM_CC 0
#define SVRH_SIM_NMI 1
/* Local (windowed) cross correlation (csrc/svr_lncc.inc; --useLNCC, a deviation: the reference has no local metric): invariant to
 * any intensity change that is linear inside a window, so a slice registers under a bias field the volume does not have.  The
 * radius R of the (2R+1)^2 window travels in the same int: similarity = SVRH_SIM_LNCC | (R << 8), R = 1..7, 0 meaning 3.  The
 * schedule, the optimiser, epsilon and the pyramids are those of CC and neither image is binned.  `backend` NULL = the engine
 * (svr_lncc_evaluate, include/svr_hip.h, where the metric is defined); an external evaluator is a svr_ncc_backend whose `evaluate`
 * fills sums6[0..1] = {N, S} of every plane -- the counted pixels and the sum of their k = floor(q 2^24 + 0.5) -- and whose other
 * four entries are ignored.  Requests are per plane, as for CC; the schedule adds the planes of an evaluation and takes
 * (sum S / sum N) / 2^24, 0 when sum N = 0.  `nmi_backend` is not used. */
#define SVRH_SIM_LNCC 2
typedef struct svr_nmi_backend {
  void *user;
  int (*set_targets)(void *user, int n, int tx, int ty, const int16_t *targets);
  int (*set_source)(void *user, const uint32_t size[3], const int16_t *source);
  int (*evaluate)(void *user, int n_eval, const int *planes_per_eval, const int *target_index, const double *matrices,
                  const int *target_width, const int *target_nbins, int source_nbins, uint32_t *hist);
} svr_nmi_backend;
int svrh_slice_to_volume_registration_ex(svr_ctx *ctx, const svr_ncc_backend *backend, const svr_nmi_backend *nmi_backend, int similarity,
                                         int n_slices, const float *slices, int sx, int sy, const svr_image_attr *attrs, double *transformations,
                                         const svr_image_attr *recon_attr, const float *reconstructed, int flags, long *n_evaluations_or_null,
                                         char err[256]);
int svrh_package_to_volume_ex(svr_ctx *ctx, const svr_ncc_backend *backend, const svr_nmi_backend *nmi_backend, int similarity, int n_stacks,
                              const svr_image_attr *attrs, const double *const *stacks, const int *pack_num, int evenodd, int half, int half_iter,
                              double *transformations, const svr_image_attr *recon_attr, const float *reconstructed, long *n_evaluations_or_null,
                              char err[256]);
/* irtkCalculateNumberOfBins(image, 64, min, max) (irtkUtil.cc:438-474): returns the number of bins, the width through
 * width_or_null, and bins data_or_null[n] in place (v > 0 -> int(v / width)); max < min gives 1 bin of width 1 */
int svrh_irtk_number_of_bins(int16_t *data_or_null, long n, int min, int max, int *width_or_null);
/* {n, S_xy, S_x, S_y} of one histogram [64][64] as above; returns NormalizedMutualInformation (0 when n = 0) */
double svrh_nmi_sums(const uint32_t *hist64, int target_nbins, int source_nbins, double sums4[4]);
/* building blocks (irtkResamplingWithPadding<short>, irtkGaussianBlurringWithPadding<short>, irtkRigidTransformation::
 * Matrix2Parameters / UpdateMatrix), exported for the tests */
int svrh_irtk_resample_with_padding(const svr_image_attr *attr, const int16_t *data, double rx, double ry, double rz, int padding,
                                    svr_image_attr *out_attr, int16_t *out_or_null, long capacity);
int svrh_irtk_blur_with_padding(const svr_image_attr *attr, int16_t *data, double sigma, int padding);
/* the sampled Gaussian of one pass of that blur (sigma in mm, voxel = the voxel size along the axis): returns its (odd) number
 * of taps and writes them when out_or_null holds `capacity` >= that many doubles (-1 when it does not) */
int svrh_irtk_blur_kernel(double sigma, double voxel, double *out_or_null, int capacity);
/* irtkImageRegistrationWithPadding::Initialize(level) for one image, the host definition that svr_pyr_level restates: blur
 * (sigma `blur` mm, none when 0), resample to res[3] when level > 0 or res0[3] is not the image's voxel size, the range
 * [*min_out, *max_out] of the values above `padding` (max < min: none), and the shift to v - min / -1.  out_or_null NULL gives
 * the attributes and the range only.  Returns 1 with a message when the range exceeds 32767, 2 on bad arguments. */
int svrh_irtk_prepare_level(const svr_image_attr *attr, const int16_t *data, double blur, const double res[3], const double res0[3], int level,
                            int padding, svr_image_attr *out_attr, int16_t *out_or_null, long capacity, int *min_out, int *max_out,
                            char err[256]);
void svrh_irtk_rigid_parameters(const double matrix16[16], double params6[6], double *rebuilt16_or_null);

/* ---- patch-to-volume reconstruction loop (csrc/pvr_host.cpp) ---------------------------
 * svr::irtkPatchBasedReconstruction: the reconstruction part of irtkPatchBasedReconstruction<T>::run
 * (irtkPatchBasedReconstruction.cpp:445-593) and the host halves of patchBasedRobustStatistics_gpu<T>
 * (patchBasedRobustStatistics_gpu.cu: initializeEMValues :78-95, EStep :224-556, MStep :570-640, Scale :672-745,
 * InitializeRobustStatistics :793-845).  The engine must have the option "pvr" set and the patches uploaded
 * as its slices; patches_per_stack is PatchBasedVolume::getXYZPatchGridSize().z per stack. */
typedef struct pvrh_recon pvrh_recon;
pvrh_recon *pvrh_create(svr_ctx *engine, const int *patches_per_stack, int n_stacks, float min_intensity, float max_intensity);
/* sharded over ranks ("identical with patches as the unit"; the reference's patch-based path is single-GPU,
 * patchBasedReconMain.cpp:78,177-179): the engine holds the patches [patch_lo, patch_hi) of the global numbering (stack
 * after stack, patches_per_stack = the GLOBAL counts), every rank the whole volume.  Exchanges per SR iteration: one
 * all-reduce of addon|cmap, the M-step's five scalars and the E-step's patch potentials (with the scale vector riding along);
 * the patch-level EM runs replicated on the global vectors -- including the reference's within-stack indexing of the patch
 * potentials (patchBasedRobustStatistics_gpu.cu:256-276). */
pvrh_recon *pvrh_create_sharded(svr_ctx *engine, const int *patches_per_stack, int n_stacks, float min_intensity, float max_intensity,
                                int patch_lo, int patch_hi, const svr_collectives *coll_or_null);
int pvrh_set_unit_order(pvrh_recon *r, const int *order_or_null);    /* as svrh_set_unit_order, with patches */
void pvrh_force_collectives(pvrh_recon *r, int on);
void pvrh_set_slab_update(pvrh_recon *r, int on);
void pvrh_destroy(pvrh_recon *r);
const char *pvrh_last_error(const pvrh_recon *r);
int pvrh_initialize_em_values(pvrh_recon *r);
int pvrh_initialize_robust_statistics(pvrh_recon *r);
int pvrh_estep(pvrh_recon *r);
int pvrh_mstep(pvrh_recon *r, int iter);
int pvrh_scale(pvrh_recon *r);
/* one outer iteration without the patch registration (irtkPatchBasedReconstruction.cpp:490-548) */
int pvrh_reconstruct_iteration(pvrh_recon *r, int rec_iterations);
int pvrh_sr_iteration(pvrh_recon *r, int i);   /* one SR iteration: Scale, scatter (+ all-reduce) + regulariser, simulate, M-step, E-step */
/* the patch-to-volume registration between the outer iterations (irtkPatchBasedReconstruction.cpp:452-489): svr_pvr_register_patches,
 * then the new transformations go to the engine.  T / Tinv [n][16] in/out; counters3 = {launches, evaluations, patches} */
int pvrh_register_patches(pvrh_recon *r, const float *ri2w, const float *mo, const float *invmo, float *T, float *Tinv, const float *i2w,
                          const float *w2i, const float *recon_i2w, const float *recon_w2i, long long counters3[3]);
/* scalars8 = {sigma, mix, m, mean_s, mean_s2, sigma_s, sigma_s2, mix_s}; vectors of length sum(patches_per_stack) */
int pvrh_get_state(pvrh_recon *r, float *scale, float *patch_weight, float *patch_potential, double scalars8[8]);

#ifdef __cplusplus
}
#endif
#endif /* SVR_HOST_H */
