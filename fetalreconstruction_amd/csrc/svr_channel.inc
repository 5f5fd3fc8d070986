// svr_channel.inc -- a second image on the slice grid carried into the volume with a finished run's motion and weights
// (svr_channel_scatter / _finish / _vote / _vote_fetch), included by svr_hip.hip.
//
// Not a step of the reconstruction: what a run knows when it ends -- every slice's transformation, the EM's weight of every pixel and
// slice, the coefficient table -- applied to values it was not estimated from: another co-registered acquisition, or a label map drawn on
// the acquired slices.  The reference has the narrow form, transformManualMaskwithPSF (reconstruction.cc:1240-1250: a manual mask on the
// first stack, one plain Gaussian pass).
//
// For a float c_p per slice pixel (the layout of svr_fill_slices), over the pixels p of slice s with
//     primary slice pixel != -1,  v_PSF_sums[p] != 0,  unit_on == NULL or unit_on[s] != 0
// (the channel's own value never decides: a quantitative map may be zero or negative):
//     f1_p = weights[p] * slice_weights[s] / v_PSF_sums[p]           the SR scatter's own weight
//     f0_p = f1_p * x_p,   x_p = c_p, or with SVR_CHANNEL_INDICATOR (c_p == match) ? 1 : 0
//     num(v) = S coeff(p, v) f0_p,   den(v) = S coeff(p, v) f1_p     -> addon | cmap
// k_cell_factors (svr_cell.inc) has the factors as its mode 3; the scatter is launch_cell_scatter as the SR iteration calls it: the same
// epsilon-skip, mask voxels only, the same fixed combine order, the coefficient table when it holds the PSF pixels.  No atomics anywhere, so
// the same bits on every call and with the table on or off.  There is no fallback onto the atomic scatters: a label vote compares sums
// that must not depend on the run, and a geometry the cell lists cannot hold is refused.
//
//   k_channel_finish   out = den > 0 ? num / den : background, in place in addon
//   k_channel_vote     P = den > 0 ? num / den : -inf;  first label, or P > best (strictly: ties stay with the label that came first,
//                      which is the smallest when the caller visits them in ascending order): best = P, label = this one
//   k_channel_settle   before the download: voxels nobody covered (best == -inf) get the background label and confidence 0
// Element-wise over nv.  addon starts an allocation; cmap starts nv floats behind it, and nv is rarely a multiple of four: the body takes
// four voxels per lane with 16-byte accesses to the arrays that start an allocation and a load of four floats at a float's alignment
// (f4u) from cmap, a scalar head runs up to the first 16-byte boundary of addon and a scalar tail takes the rest.
//
// The channel and the per-slice switches are uploaded into buffers of the call's own and freed before it returns, like svr_slice_quality's
// scratch: the coefficient table sizes itself by the memory that is free.  The two vote arrays live from the first vote to the fetch;
// the invalidation map drops them with the volume grid (CH_VOLUME_GRID).
//
// svr_channel_sr_begin .. _end (further down) refine that average by SR iterations with the weights held fixed: the run's gather, factor
// mode 4 of k_cell_factors, the run's scatter and the run's volume update on buffers that live from begin to end.  svr_channel_sr_guide adds a
// guide volume to them: the updates of that call then weigh a neighbour pair by the guide's differences too (the GUIDED kernels of svr_regul.inc).

namespace {

struct __attribute__((packed, aligned(4))) f4u { float x, y, z, w; };

__device__ __forceinline__ float channel_quot(float num, float den, float otherwise) { return den > 0.0f ? num / den : otherwise; }

// the split of [0, nv) into a scalar head up to the first 16-byte boundary of `base`, whole float4s, and a scalar tail
struct VecSplit { size_t head, nvec, tail0; };
__device__ __forceinline__ VecSplit vec_split(const float *base, size_t nv) {
  VecSplit s;
  const size_t h = (size_t)((4u - (unsigned)((reinterpret_cast<uintptr_t>(base) >> 2) & 3u)) & 3u);
  s.head = h < nv ? h : nv;
  s.nvec = (nv - s.head) >> 2;
  s.tail0 = s.head + 4 * s.nvec;
  return s;
}

__global__ __launch_bounds__(256) void k_channel_finish(float *__restrict__ num, const float *__restrict__ den, float background, size_t nv) {
  const VecSplit s = vec_split(num, nv);
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
  if (t < s.head) num[t] = channel_quot(num[t], den[t], background);
  for (size_t i = t; i < s.nvec; i += stride) {
    const size_t g = s.head + 4 * i;
    float4 n4 = *reinterpret_cast<const float4 *>(num + g);
    const f4u d4 = *reinterpret_cast<const f4u *>(den + g);
    n4.x = channel_quot(n4.x, d4.x, background); n4.y = channel_quot(n4.y, d4.y, background);
    n4.z = channel_quot(n4.z, d4.z, background); n4.w = channel_quot(n4.w, d4.w, background);
    *reinterpret_cast<float4 *>(num + g) = n4;
  }
  if (t < nv - s.tail0) num[s.tail0 + t] = channel_quot(num[s.tail0 + t], den[s.tail0 + t], background);
}

__device__ __forceinline__ void channel_vote_one(float num, float den, float label, bool first, float &best, float &lab) {
  const float p = channel_quot(num, den, -INFINITY);
  if (first || p > best) { best = p; lab = label; }
}

// best / lab start allocations of their own, as num does: the three share one split
__global__ __launch_bounds__(256) void k_channel_vote(const float *__restrict__ num, const float *__restrict__ den, float label, int first,
                                                      float *__restrict__ best, float *__restrict__ lab, size_t nv) {
  const VecSplit s = vec_split(num, nv);
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
  const bool f = first != 0;
  auto scalar = [&](size_t g) {
    float b = f ? 0.0f : best[g], l = f ? 0.0f : lab[g];
    channel_vote_one(num[g], den[g], label, f, b, l);
    best[g] = b; lab[g] = l;
  };
  if (t < s.head) scalar(t);
  for (size_t i = t; i < s.nvec; i += stride) {
    const size_t g = s.head + 4 * i;
    const float4 n4 = *reinterpret_cast<const float4 *>(num + g);
    const f4u d4 = *reinterpret_cast<const f4u *>(den + g);
    float4 b4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), l4 = b4;
    if (!f) { b4 = *reinterpret_cast<const float4 *>(best + g); l4 = *reinterpret_cast<const float4 *>(lab + g); }
    channel_vote_one(n4.x, d4.x, label, f, b4.x, l4.x); channel_vote_one(n4.y, d4.y, label, f, b4.y, l4.y);
    channel_vote_one(n4.z, d4.z, label, f, b4.z, l4.z); channel_vote_one(n4.w, d4.w, label, f, b4.w, l4.w);
    *reinterpret_cast<float4 *>(best + g) = b4;
    *reinterpret_cast<float4 *>(lab + g) = l4;
  }
  if (t < nv - s.tail0) scalar(s.tail0 + t);
}

__device__ __forceinline__ void channel_settle_one(float &best, float &lab, float background_label) {
  if (best == -INFINITY) { best = 0.0f; lab = background_label; }
}
__global__ __launch_bounds__(256) void k_channel_settle(float *__restrict__ best, float *__restrict__ lab, float background_label, size_t nv) {
  const VecSplit s = vec_split(best, nv);
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
  if (t < s.head) channel_settle_one(best[t], lab[t], background_label);
  for (size_t i = t; i < s.nvec; i += stride) {
    const size_t g = s.head + 4 * i;
    float4 b4 = *reinterpret_cast<const float4 *>(best + g), l4 = *reinterpret_cast<const float4 *>(lab + g);
    channel_settle_one(b4.x, l4.x, background_label); channel_settle_one(b4.y, l4.y, background_label);
    channel_settle_one(b4.z, l4.z, background_label); channel_settle_one(b4.w, l4.w, background_label);
    *reinterpret_cast<float4 *>(best + g) = b4;
    *reinterpret_cast<float4 *>(lab + g) = l4;
  }
  if (t < nv - s.tail0) channel_settle_one(best[s.tail0 + t], lab[s.tail0 + t], background_label);
}

// a lane takes four voxels per step; enough workgroups for one step each, at least one
inline unsigned channel_blocks(size_t nv) { return std::max(1u, nblk((nv + 3) / 4)); }
inline bool same_16(const void *a, const void *b) { return ((reinterpret_cast<uintptr_t>(a) ^ reinterpret_cast<uintptr_t>(b)) & 15u) == 0; }

// What a channel scatter needs before its buffers: the PSF list, addon | cmap no longer the SR scatter's, the cell lists.  *empty: no PSF pixel,
// addon | cmap are zero and there is nothing to launch
int channel_scatter_prepare(svr_ctx *ctx, const char *who, bool *empty) {
  int r = ensure_psf_list(ctx);
  if (r) return r;
  // the SR scatter's Prep may still be owed to addon | cmap (k_regul_fused leaves it to their next reader): what lands there now is not its
  ctx->prep_pending = false;
  invalidate(ctx, CH_SCATTER_TARGETS);
  *empty = !ctx->n_psf;
  if (*empty) {                                             // no PSF pixel: nothing covers any voxel
    HIPCHK(hipMemsetAsync(ctx->d_addon_cmap, 0, 2 * ctx->nv * sizeof(float), ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SVR_OK;
  }
  if ((r = cell_prepare(ctx))) return r;
  if (!ctx->cell || !ctx->cell->usable)
    return fail(ctx, SVR_E_STATE, std::string(who) + ": the cell lists cannot hold this geometry, and channels have no fallback onto the atomic scatters");
  return SVR_OK;
}
int channel_upload(svr_ctx *ctx, const float *channel, const unsigned char *unit_on, DevBuf<float> &d_channel, DevBuf<unsigned char> &d_unit_on) {
  HIPCHK(d_channel.reserve(ctx->np));
  HIPCHK(hipMemcpyAsync(d_channel, channel, ctx->np * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  if (unit_on) {
    HIPCHK(d_unit_on.reserve(ctx->ns));
    HIPCHK(hipMemcpyAsync(d_unit_on, unit_on, ctx->ns, hipMemcpyHostToDevice, ctx->stream));
  }
  return SVR_OK;
}
// the scatter itself, factor mode 3 (values) or 4 (residuals against the forward projection sim / simw) -> addon | cmap
int channel_scatter_launch(svr_ctx *ctx, const float *d_channel, const unsigned char *d_unit_on, int flags, float match, int mode, float *sim, float *simw) {
  PsfArgs a = make_args(ctx);
  a.list = ctx->d_psf_list;
  a.n = ctx->n_psf;
  a.channel = d_channel;
  a.unit_on = d_unit_on;
  a.ch_flags = flags;
  a.ch_match = match;
  if (sim) { a.simslices = sim; a.simweights = simw; }
  TableUse use;
  const int r = table_begin(ctx, table_plan_for(ctx, PASS_CHANNEL_SCATTER, pass_path(ctx, PASS_CHANNEL_SCATTER), true), a, &use);
  return r ? r : launch_cell_scatter(ctx, a, mode, ctx->addon(), ctx->cmap());
}

int channel_scatter_run(svr_ctx *ctx, const float *channel, const unsigned char *unit_on, int flags, float match) {
  bool empty = false;
  int r = channel_scatter_prepare(ctx, "svr_channel_scatter", &empty);
  if (r || empty) return r;
  DevBuf<float> d_channel;                                  // the channel and its per-slice switches: nothing is kept beyond the call (the
  DevBuf<unsigned char> d_unit_on;                          // coefficient table sizes itself by the memory that is free)
  if ((r = channel_upload(ctx, channel, unit_on, d_channel, d_unit_on))) return r;
  if ((r = channel_scatter_launch(ctx, d_channel, d_unit_on, flags, match, 3, nullptr, nullptr))) return r;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

// ---- SR iterations on a channel (svr_channel_sr_begin / _seed / _backproject / _update / _end) ------------------------------------------
// The run's SR loop on other values, the weights held fixed.  C0 = the average above (seed), cover = its den > 0; then per iteration
//   sim = the forward projection of C (svr_simulate_slices's cell gather, the table when it is valid) into the call's own buffers,
//   factor mode 4 of k_cell_factors + launch_cell_scatter -> addon | cmap,   C' = k_regul_fused(C, addon, cmap) with a clamp [lo, hi],
// and at the end C = 0 outside cover.  The halves are separate entry points so that a sharded run can all-reduce addon | cmap in between.

// C0 = den > 0 ? num / den : 0 (svr_channel_finish with background 0, not in place) and the cover mask
__global__ __launch_bounds__(256) void k_channel_seed(const float *__restrict__ num, const float *__restrict__ den, float *__restrict__ vol,
                                                      unsigned char *__restrict__ cover, size_t nv) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nv) return;
  const float d = den[i];
  vol[i] = channel_quot(num[i], d, 0.0f);
  cover[i] = d > 0.0f ? 1 : 0;
}
__global__ __launch_bounds__(256) void k_channel_uncover(float *__restrict__ vol, const unsigned char *__restrict__ cover, size_t nv) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < nv && !cover[i]) vol[i] = 0.0f;
}

// step 1: the channel volume through svr_simulate_slices's gather over the (cell, plane) items into d_csr_sim / d_csr_simw.  Nothing of the primary's
// forward projection is written; d_volm and the cell lists' staging are scratch that every pass refills
int channel_sr_forward(svr_ctx *ctx) {
  const float *vol = ctx->d_csr_vol[ctx->csr_cur];
  PsfArgs a = make_args(ctx);
  a.list = ctx->d_psf_list;
  a.n = ctx->n_psf;
  a.vol = vol;
  a.simslices = ctx->d_csr_sim; a.simweights = ctx->d_csr_simw;
  a.siminside = ctx->d_csr_inside; a.slice_inside = ctx->d_csr_slice_inside;
  // the table where svr_simulate_slices would stream it on the cells; a gather it would hand to the slice tiles evaluates here (the same bits)
  TableUse use;
  int r = table_begin(ctx, table_plan_for(ctx, PASS_CHANNEL_GATHER, pass_path(ctx, PASS_CHANNEL_GATHER), true), a, &use);
  if (r) return r;
  HIPCHK(hipMemsetAsync(ctx->d_csr_sim, 0, ctx->np * sizeof(float), ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->d_csr_simw, 0, ctx->np * sizeof(float), ctx->stream));
  if ((r = pack_volm(ctx, a, vol))) return r;
  CellState *gcs = nullptr;
  if ((r = cell_prepare_gather(ctx, gcs))) return r;
  if (!gcs || !gcs->usable)
    return fail(ctx, SVR_E_STATE, "svr_channel_sr_backproject: the cell lists cannot hold this geometry, and channels have no fallback onto the tile kernels");
  return launch_cell_gather(ctx, *gcs, a, false);
}

int channel_sr_refuse_order(svr_ctx *ctx, const char *who, const char *what) { return fail(ctx, SVR_E_ARG, std::string(who) + ": " + what); }

}  // namespace

extern "C" {

int svr_channel_scatter(svr_ctx *ctx, const float *channel, const unsigned char *unit_on, const float *slice_weights, int flags, float match) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  if (!channel) return fail(ctx, SVR_E_ARG, "svr_channel_scatter: no channel");
  if (flags & ~SVR_CHANNEL_INDICATOR) return fail(ctx, SVR_E_ARG, "svr_channel_scatter: unknown flag");
  if (ctx->pvr) return fail(ctx, SVR_E_STATE, "svr_channel_scatter: not for a patch-based (pvr) context");
  NEED(ctx->np > 0 && ctx->have_slices, "slices not filled");
  NEED(ctx->have_em, "no EM weights (svr_initialize_em_values first)");
  int r = ready(ctx);
  if (r) return r;
  if (pass_path(ctx, PASS_CHANNEL_SCATTER).family != FAM_CELLS)
    return fail(ctx, SVR_E_STATE, "svr_channel_scatter: needs the cell scatter (back_mode 5); channels have no fallback onto the atomic scatters");
  if (slice_weights && (r = svr_update_slice_weights(ctx, slice_weights))) return r;
  return channel_scatter_run(ctx, channel, unit_on, flags, match);
}

int svr_channel_finish(svr_ctx *ctx, float background, float *out_or_null) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  NEED(ctx->nv > 0, "reconstruction volume not initialised");
  ctx->prep_pending = false;
  invalidate(ctx, CH_SCATTER_TARGETS);
  hipLaunchKernelGGL(k_channel_finish, dim3(channel_blocks(ctx->nv)), dim3(256), 0, ctx->stream, ctx->addon(), ctx->cmap(), background, ctx->nv);
  KCHK("k_channel_finish");
  if (out_or_null) HIPCHK(hipMemcpyAsync(out_or_null, ctx->addon(), ctx->nv * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

int svr_channel_vote(svr_ctx *ctx, float label, int first) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  NEED(ctx->nv > 0, "reconstruction volume not initialised");
  if (first) {
    ctx->d_vote_best.reset(); ctx->d_vote_label.reset();
    HIPCHK(ctx->d_vote_best.reserve(ctx->nv));
    HIPCHK(ctx->d_vote_label.reserve(ctx->nv));
  }
  NEED(ctx->d_vote_best && ctx->d_vote_label, "no vote in flight (the first label's call says first = 1)");
  if (!same_16(ctx->addon(), ctx->d_vote_best) || !same_16(ctx->addon(), ctx->d_vote_label))
    return fail(ctx, SVR_E_STATE, "svr_channel_vote: the vote arrays do not share addon's 16-byte alignment");
  ctx->prep_pending = false;
  hipLaunchKernelGGL(k_channel_vote, dim3(channel_blocks(ctx->nv)), dim3(256), 0, ctx->stream, ctx->addon(), ctx->cmap(), label, first ? 1 : 0,
                     ctx->d_vote_best, ctx->d_vote_label, ctx->nv);
  KCHK("k_channel_vote");
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

int svr_channel_vote_fetch(svr_ctx *ctx, float background_label, float *labels_or_null, float *confidence_or_null) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  NEED(ctx->nv > 0 && ctx->d_vote_best && ctx->d_vote_label, "no vote in flight (svr_channel_vote first)");
  if (!same_16(ctx->d_vote_best, ctx->d_vote_label)) return fail(ctx, SVR_E_STATE, "svr_channel_vote_fetch: the vote arrays do not share one alignment");
  int r = SVR_OK;
  hipLaunchKernelGGL(k_channel_settle, dim3(channel_blocks(ctx->nv)), dim3(256), 0, ctx->stream, ctx->d_vote_best, ctx->d_vote_label, background_label, ctx->nv);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && labels_or_null) e = hipMemcpyAsync(labels_or_null, ctx->d_vote_label, ctx->nv * sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && confidence_or_null) e = hipMemcpyAsync(confidence_or_null, ctx->d_vote_best, ctx->nv * sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) r = fail(ctx, (int)e, std::string("svr_channel_vote_fetch: ") + hipGetErrorString(e));
  ctx->d_vote_best.reset(); ctx->d_vote_label.reset();     // the vote is over, whether the download worked or not
  return r;
}

int svr_channel_sr_begin(svr_ctx *ctx, const float *channel, const unsigned char *unit_on, const float *slice_weights, int flags) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  if (!channel) return fail(ctx, SVR_E_ARG, "svr_channel_sr_begin: no channel");
  if (flags & SVR_CHANNEL_INDICATOR) return fail(ctx, SVR_E_ARG, "svr_channel_sr_begin: label indicators have no SR iterations (they keep their vote)");
  if (flags) return fail(ctx, SVR_E_ARG, "svr_channel_sr_begin: unknown flag");
  if (ctx->pvr) return fail(ctx, SVR_E_STATE, "svr_channel_sr_begin: not for a patch-based (pvr) context");
  if (ctx->csr_stage) return channel_sr_refuse_order(ctx, "svr_channel_sr_begin", "a channel's SR iterations are in flight (svr_channel_sr_end first)");
  NEED(ctx->np > 0 && ctx->have_slices, "slices not filled");
  NEED(ctx->have_em, "no EM weights (svr_initialize_em_values first)");
  int r = ready(ctx);
  if (r) return r;
  if (pass_path(ctx, PASS_CHANNEL_SCATTER).family != FAM_CELLS || pass_path(ctx, PASS_CHANNEL_GATHER).family != FAM_CELLS)
    return fail(ctx, SVR_E_STATE, "svr_channel_sr_begin: needs the cell scatter and the cell gather (back_mode 5, fwd_mode 2); channels have no fallback onto the other kernels");
  if (ctx->reg_mode != 1) return fail(ctx, SVR_E_STATE, "svr_channel_sr_begin: needs the fused volume update (reg_mode 1)");
  if (slice_weights && (r = svr_update_slice_weights(ctx, slice_weights))) return r;
  bool empty = false;
  if ((r = channel_scatter_prepare(ctx, "svr_channel_sr_begin", &empty))) return r;
  // the call's memory, after whatever the passes of the run allocated (the coefficient table sizes itself by the memory that is free)
  hipError_t e = hipSuccess;
  if (e == hipSuccess) e = ctx->d_csr_vol[0].reserve(ctx->nv);
  if (e == hipSuccess) e = ctx->d_csr_vol[1].reserve(ctx->nv);
  if (e == hipSuccess) e = ctx->d_csr_cover.reserve(ctx->nv);
  if (e == hipSuccess) e = ctx->d_csr_sim.reserve(ctx->np);
  if (e == hipSuccess) e = ctx->d_csr_simw.reserve(ctx->np);
  if (e == hipSuccess) e = ctx->d_csr_inside.reserve(ctx->np);
  if (e == hipSuccess) e = ctx->d_csr_slice_inside.reserve(ctx->ns);
  if (e == hipSuccess && (r = channel_upload(ctx, channel, unit_on, ctx->d_csr_channel, ctx->d_csr_unit_on))) { channel_sr_drop(ctx); return r; }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    channel_sr_drop(ctx);
    return fail(ctx, (int)e, std::string("svr_channel_sr_begin: ") + hipGetErrorString(e));
  }
  ctx->csr_has_unit_on = unit_on != nullptr;
  ctx->csr_cur = 0;
  if (!empty && (r = channel_scatter_launch(ctx, ctx->d_csr_channel, ctx->csr_has_unit_on ? ctx->d_csr_unit_on.get() : nullptr, 0, 0.0f, 3, nullptr, nullptr))) {
    channel_sr_drop(ctx);
    return r;
  }
  e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) { channel_sr_drop(ctx); return fail(ctx, (int)e, std::string("svr_channel_sr_begin: ") + hipGetErrorString(e)); }
  ctx->csr_stage = 1;
  return SVR_OK;
}

int svr_channel_sr_seed(svr_ctx *ctx, const float *seed_or_null) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  if (ctx->csr_stage != 1) return channel_sr_refuse_order(ctx, "svr_channel_sr_seed", "svr_channel_sr_begin first, and one seed per call");
  float *vol = ctx->d_csr_vol[ctx->csr_cur];
  hipLaunchKernelGGL(k_channel_seed, dim3(nblk(ctx->nv)), dim3(256), 0, ctx->stream, ctx->addon(), ctx->cmap(), vol, ctx->d_csr_cover, ctx->nv);
  KCHK("k_channel_seed");
  if (seed_or_null) HIPCHK(hipMemcpyAsync(vol, seed_or_null, ctx->nv * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->csr_stage = 2;
  return SVR_OK;
}

int svr_channel_sr_guide(svr_ctx *ctx, const float *guide_or_null, float delta_g, int flags) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  if (ctx->csr_stage != 1 && ctx->csr_stage != 2)
    return channel_sr_refuse_order(ctx, "svr_channel_sr_guide", ctx->csr_stage ? "not between a back-projection and its update (svr_channel_sr_update first)"
                                                                               : "svr_channel_sr_begin first");
  if (!(std::isfinite(delta_g) && delta_g > 0.0f)) return fail(ctx, SVR_E_ARG, "svr_channel_sr_guide: delta_g must be finite and positive");
  if (flags & ~SVR_CHANNEL_GUIDE_ONLY) return fail(ctx, SVR_E_ARG, "svr_channel_sr_guide: unknown flag");
  if (ctx->reg_mode != 1) return fail(ctx, SVR_E_STATE, "svr_channel_sr_guide: needs the fused volume update (reg_mode 1)");
  if (guide_or_null)
    for (size_t i = 0; i < ctx->nv; ++i)
      if (!std::isfinite(guide_or_null[i])) return fail(ctx, SVR_E_ARG, "svr_channel_sr_guide: the guide holds a value that is not finite");
  // a buffer of the call's own: nothing the run does later changes the guide, and the reconstruction is only read
  hipError_t e = ctx->d_csr_guide.reserve(ctx->nv);
  if (e == hipSuccess)
    e = guide_or_null ? hipMemcpyAsync(ctx->d_csr_guide, guide_or_null, ctx->nv * sizeof(float), hipMemcpyHostToDevice, ctx->stream)
                      : hipMemcpyAsync(ctx->d_csr_guide, ctx->recon(), ctx->nv * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {                                    // no guide rather than half of one; the call in flight goes on unguided
    (void)hipGetLastError();
    ctx->d_csr_guide.reset();
    return fail(ctx, (int)e, std::string("svr_channel_sr_guide: ") + hipGetErrorString(e));
  }
  ctx->csr_delta_g = delta_g;
  ctx->csr_guide_only = (flags & SVR_CHANNEL_GUIDE_ONLY) != 0;
  return SVR_OK;
}

int svr_channel_sr_backproject(svr_ctx *ctx) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  if (ctx->csr_stage != 2) return channel_sr_refuse_order(ctx, "svr_channel_sr_backproject", "svr_channel_sr_seed first, and svr_channel_sr_update after every back-projection");
  bool empty = false;
  int r = channel_scatter_prepare(ctx, "svr_channel_sr_backproject", &empty);
  if (r) return r;
  if (!empty) {
    if ((r = channel_sr_forward(ctx))) return r;
    if ((r = channel_scatter_launch(ctx, ctx->d_csr_channel, ctx->csr_has_unit_on ? ctx->d_csr_unit_on.get() : nullptr, 0, 0.0f, 4, ctx->d_csr_sim, ctx->d_csr_simw))) return r;
    ctx->cmap_from_scatter = true;                          // (the cell scatter's combine wrote every voxel, 0 outside the mask: the update may skip the rest)
  }
  if (!ctx->sr_no_wait) HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->csr_stage = 3;
  return SVR_OK;
}

int svr_channel_sr_update(svr_ctx *ctx, int adaptive, float alpha, float lo, float hi, float delta, float lambda) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  if (ctx->csr_stage != 3) return channel_sr_refuse_order(ctx, "svr_channel_sr_update", "svr_channel_sr_backproject first");
  if (!(std::isfinite(delta) && delta > 0.0f) || !(std::isfinite(lambda) && lambda > 0.0f))
    return fail(ctx, SVR_E_ARG, "svr_channel_sr_update: delta and lambda must be finite and positive");
  if (!std::isfinite(alpha)) return fail(ctx, SVR_E_ARG, "svr_channel_sr_update: alpha must be finite");
  if (!(lo <= hi)) return fail(ctx, SVR_E_ARG, "svr_channel_sr_update: the clamp needs lo <= hi");
  if (ctx->reg_mode != 1) return fail(ctx, SVR_E_STATE, "svr_channel_sr_update: needs the fused volume update (reg_mode 1)");
  if (alpha * lambda / (delta * delta) > 0.068)
    fprintf(stderr, "Warning: regularization might not have smoothing effect! Ensure that alpha*lambda/delta^2 is below 0.068.");
  RegulArgs ra;
  ra.thr_lo = ra.val_lo = lo;                               // r < lo -> lo, r > hi -> hi: the channel's own range, not 0.9 min / 1.1 max
  ra.thr_hi = ra.val_hi = hi;
  ra.guide = ctx->d_csr_guide ? ctx->d_csr_guide.get() : nullptr;
  if (ra.guide) {                                           // svr_channel_sr_guide: the GUIDED kernels; delta still defines k = alpha lambda / delta^2
    const double g2 = (double)ctx->csr_delta_g * (double)ctx->csr_delta_g;
    ra.gkap1 = (float)(1.0 / g2); ra.gkap2 = (float)(0.5 / g2); ra.gkap3 = (float)((double)(1.0f / 3.0f) / g2);
    ra.omega = ctx->csr_guide_only ? 0.0f : 1.0f;
  }
  const int r = regul_fused_launch(ctx, ra, ctx->d_csr_vol[ctx->csr_cur], ctx->d_csr_vol[ctx->csr_cur ^ 1], adaptive, alpha, delta, lambda, 0, (int)ctx->vz);
  if (r) return r;
  ctx->csr_cur ^= 1;                                        // the update wrote the other buffer
  if (!ctx->sr_no_wait) HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->csr_stage = 2;
  return SVR_OK;
}

int svr_channel_sr_end(svr_ctx *ctx, float *out_or_null) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  if (!ctx->csr_stage) return channel_sr_refuse_order(ctx, "svr_channel_sr_end", "svr_channel_sr_begin first");
  int r = SVR_OK;
  hipError_t e = hipSuccess;
  if (out_or_null && ctx->csr_stage < 2) r = fail(ctx, SVR_E_ARG, "svr_channel_sr_end: no volume to hand over (svr_channel_sr_seed first); the call is over");
  if (ctx->csr_stage >= 2 && out_or_null) {
    float *vol = ctx->d_csr_vol[ctx->csr_cur];
    hipLaunchKernelGGL(k_channel_uncover, dim3(nblk(ctx->nv)), dim3(256), 0, ctx->stream, vol, ctx->d_csr_cover, ctx->nv);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out_or_null, vol, ctx->nv * sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) r = fail(ctx, (int)e, std::string("svr_channel_sr_end: ") + hipGetErrorString(e));
  // addon | cmap hold the last iteration's scatter, with Prep's changes neither applied nor owed
  ctx->prep_pending = false;
  invalidate(ctx, CH_SCATTER_TARGETS);
  channel_sr_drop(ctx);                                     // the call is over, whether the download worked or not
  return r;
}

}  // extern "C"
