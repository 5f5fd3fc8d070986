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

int channel_scatter_run(svr_ctx *ctx, const float *channel, const unsigned char *unit_on, int flags, float match) {
  int r = ensure_psf_list(ctx);
  if (r) return r;
  // the SR scatter's Prep may still be owed to addon | cmap (k_regul_fused leaves it to their next reader): what lands there now is not its
  ctx->prep_pending = false;
  invalidate(ctx, CH_SCATTER_TARGETS);
  if (!ctx->n_psf) {                                        // no PSF pixel: nothing covers any voxel
    HIPCHK(hipMemsetAsync(ctx->d_addon_cmap, 0, 2 * ctx->nv * sizeof(float), ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SVR_OK;
  }
  if ((r = cell_prepare(ctx))) return r;
  if (!ctx->cell || !ctx->cell->usable)
    return fail(ctx, SVR_E_STATE, "svr_channel_scatter: the cell lists cannot hold this geometry, and channels have no fallback onto the atomic scatters");
  DevBuf<float> d_channel;                                  // the channel and its per-slice switches: nothing is kept beyond the call (the
  DevBuf<unsigned char> d_unit_on;                          // coefficient table sizes itself by the memory that is free)
  HIPCHK(d_channel.reserve(ctx->np));
  HIPCHK(hipMemcpyAsync(d_channel, channel, ctx->np * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  if (unit_on) {
    HIPCHK(d_unit_on.reserve(ctx->ns));
    HIPCHK(hipMemcpyAsync(d_unit_on, unit_on, ctx->ns, hipMemcpyHostToDevice, ctx->stream));
  }
  PsfArgs a = make_args(ctx);
  a.list = ctx->d_psf_list;
  a.n = ctx->n_psf;
  a.channel = d_channel;
  a.unit_on = d_unit_on;
  a.ch_flags = flags;
  a.ch_match = match;
  if (table_holds(ctx, COEFF_PSF)) give_coeff(ctx, a);
  if ((r = launch_cell_scatter(ctx, a, 3, ctx->addon(), ctx->cmap()))) return r;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

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
  if (pass_path(ctx, PASS_BACK).family != FAM_CELLS)
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

}  // extern "C"
