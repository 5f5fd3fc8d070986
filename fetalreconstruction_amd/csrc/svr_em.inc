// svr_em.inc -- the slice-level EM of an SR iteration ON THE DEVICE (#included at the end of svr_hip.hip).
//
// irtkReconstruction::EStepGPU (irtkReconstructionGPU.cc:3184-3440) is a device half -- voxel posteriors and the slices' potentials,
// EStepKernel3D_tex, reconstruction_cuda2.cu:2766-2925 -- and a HOST half: the potentials come down, a two-class 1-D EM over the slices
// (means, variances, slice weights, mixing proportion; :3282-3420) runs on the host, the slice weights go back up.  That round trip is the
// one wait of an SR iteration that is left after the M-step's scalars moved to the device (round 3) and, in a sharded run, the one
// exchange that has to meet on the hosts (round 4).  Here the host half runs as ONE WORKGROUP behind the E-step's kernels:
//
//   svr_slice_em_setup      once: global slice count, the ranks' ranges of the host object's numbering, its unit order, the step
//   svr_slice_em_set_state  the host's copy of the state -> device, whenever the host changed it (InitializeEMValues,
//                           InitializeRobustStatistics, force-excluded slices): slice weights, exclusion flags, the five slice-level scalars, {sigma, mix, m}
//   svr_mstep_estep_device  [M-step: this rank's sums -> scalars, or the ranks' sums added up (svr_mstep_partial + the launcher's all-gather)]
//                           -> E-step kernels on the device's {sigma, mix, m} -> {potential, scale, slice_inside} of this rank's slices packed
//                           into *send (3 x maxn floats)
//   (the launcher's all-gather of *send into *recv: world x 3 x maxn floats; one rank: nothing)
//   svr_slice_em_run        unpack -> the EM (k_slice_em) -> the global slice weights, this rank's part of them into the vector the scatter reads
//   svr_slice_em_fetch      everything back to the host in ONE wait, when somebody asks (state read-back, the next outer iteration's preamble)
//
// No wait for the device and no host exchange inside an SR iteration: the host object only queues launches.
//
// The arithmetic is the host object's (csrc/svr_host.cpp EStepGPU: the reference's expressions with their float / double mix), in the
// REFERENCE's slice order, with one difference: the five sums over the slices are taken by 256 threads (thread k adds the slices k, k + 256,
// .. in order, then a fixed tree) instead of one after the other -- double sums of a few hundred floats, so the scalars agree with the host
// form to ~1e-15 relative before they are rounded to float.  Every rank runs the same kernel on the same gathered vectors: the same bits
// on every rank, whatever the sharding.
//
// What the tests pin (tests/test_unit_em_gpu.py against the numpy restatement tests/unit_em_ref.py, cases tests/unit_em_cases.py): the
// unpacked scales / inside flags / potentials with the exclusions and mean_s, mean_s2, sigma_s, sigma_s2 BIT FOR BIT in this 256-thread
// order (and within 1 float ulp of the reference's serial order); the slice form's weights within 1 float ulp of float64 arithmetic on the
// returned scalars, its branch zeros and ones exactly; the patch form's within four times the float Gaussian's own gap to float64 plus an
// ulp; mix_s bit for bit from the returned weights; every rank of a sharding the same bits; k_mstep_finish, k_potential_pack (its zero
// padding up to maxn included) and k_mstep_scalars_dev bit for bit against the separate calls and against mstep_scalars restated.
namespace {

struct SliceEm {
  int ns = 0, world = 1, rank = 0, maxn = 0;
  std::vector<int> rlo;                       // [world + 1] ranges of the host object's numbering
  std::vector<int> h_by_ref;                  // [ns] host index of the unit with reference index t
  DevBuf<int> d_rlo, d_by_ref;                // [world + 1]; [ns]: host index of the slice with reference index t
  DevBuf<unsigned char> d_excl;               // [ns] force-excluded (host numbering)
  DevBuf<float> d_send, d_recv;               // [3][maxn]; [world][3][maxn]
  DevBuf<float> d_pot, d_scale, d_w, d_inside;   // [ns] global vectors, host numbering
  DevBuf<float> d_raw;                        // [ns] the potentials as the ranks sent them (patch form: d_pot takes them through d_src)
  DevBuf<int> d_src;                          // patch form: host index of the unit whose potential unit g reads, -1 = none (0); NULL = its own
  int patch_form = 0;                         // irtkPatchBasedReconstruction's EM: float Gaussian, the potentials through d_src
  DevBuf<double> d_sc;                        // {mean_s, mean_s2, sigma_s, sigma_s2, mix_s}
  double step = 0.0001;
  bool ready = false;
};

void slice_em_invalidate(SliceEm *p) { if (p) p->ready = false; }   // svr_init_storage_volumes: new slice count, svr_slice_em_setup again
void slice_em_free(SliceEm *p) { delete p; }

// the M-step's scalars with the previous {sigma, mix} read from device memory (k_mstep_scalars / k_mstep_scalars_ranks take them as arguments)
__global__ void k_mstep_scalars_dev(const double *s5_or_all, int world, int iter, float step, int pvr, float *em) {
  double s5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (world <= 0) {
    for (int k = 0; k < 5; ++k) s5[k] = s5_or_all[k];
  } else {
    for (int r = 0; r < world; ++r) {                    // rank order: k_mstep_scalars_ranks
      for (int k = 0; k < 3; ++k) s5[k] += s5_or_all[8 * r + k];
      s5[3] = r ? fmin(s5[3], s5_or_all[8 * r + 3]) : s5_or_all[3];
      s5[4] = r ? fmax(s5[4], s5_or_all[8 * r + 4]) : s5_or_all[4];
    }
  }
  float sigma = em[0], mix = em[1], m = 0.0f;
  mstep_scalars(s5, iter, step, pvr, sigma, mix, m);
  em[0] = sigma; em[1] = mix; em[2] = m;
}

// Round 6: the M-step's tail as ONE workgroup -- k_reduce_chunks, k_reduce_slices and k_mstep_scalars_dev (world <= 0) one after the other in one
// launch: the same additions in the same order (per slice over its chunks in chunk order; over the slices by the 256-thread tree), so the same
// bits; three launches of 4-6 us each that were nothing but latency become one.  K = 5 quantities, minimum for k = 3, maximum for k = 4.
__global__ __launch_bounds__(256) void k_mstep_finish(const double *partial, int ns, int chunks, double *per_slice, double *out, int iter, float step, int pvr, float *em) {
  constexpr int K = 5;
  __shared__ double sm[K][256];
  const int t = threadIdx.x;
  for (int i = t; i < ns * K; i += 256) {                  // k_reduce_chunks
    const int sl = i / K, k = i - sl * K;
    const bool mn = k == 3, mx = k == 4;
    double x = partial[((size_t)sl * chunks) * K + k];
    for (int c = 1; c < chunks; ++c) {
      const double y = partial[((size_t)sl * chunks + c) * K + k];
      x = mn ? fmin(x, y) : (mx ? fmax(x, y) : x + y);
    }
    per_slice[i] = x;
  }
  __syncthreads();                                         // (this workgroup's own global writes, read back below)
  for (int k = 0; k < K; ++k) {                            // k_reduce_slices
    const bool mn = k == 3, mx = k == 4;
    double x = mn ? INFINITY : (mx ? -INFINITY : 0.0);
    for (int s_ = t; s_ < ns; s_ += 256) {
      const double y = per_slice[(size_t)s_ * K + k];
      x = mn ? fmin(x, y) : (mx ? fmax(x, y) : x + y);
    }
    sm[k][t] = x;
  }
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
      for (int k = 0; k < K; ++k) {
        const bool mn = k == 3, mx = k == 4;
        const double y = sm[k][t + o], z = sm[k][t];
        sm[k][t] = mn ? fmin(z, y) : (mx ? fmax(z, y) : z + y);
      }
    }
    __syncthreads();
  }
  if (t < K) out[t] = sm[t][0];
  if (t == 0) {                                            // k_mstep_scalars_dev, world <= 0
    double s5[5];
    for (int k = 0; k < 5; ++k) s5[k] = sm[k][0];
    float sigma = em[0], mix = em[1], m = 0.0f;
    mstep_scalars(s5, iter, step, pvr, sigma, mix, m);
    em[0] = sigma; em[1] = mix; em[2] = m;
  }
}
// ... and the E-step's: k_potential_finish and k_slice_em_pack in one launch (thread i: slice i's potential from its chunks, in chunk order, then
// the three packed words the slice-level EM reads)
__global__ void k_potential_pack(const double *partial, int ns, int chunks, float *potential, const float *scale, const unsigned char *inside, int maxn, float *send) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= maxn) return;
  float pot = 0.0f;
  if (i < ns) {
    const double *p = partial + (size_t)i * chunks * 2;
    double a = p[0], b = p[1];
    for (int c = 1; c < chunks; ++c) { a += p[2 * c]; b += p[2 * c + 1]; }
    pot = (b > 0) ? sqrtf((float)a / (float)b) : -1.0f;
    potential[i] = pot;
  }
  send[i] = i < ns ? pot : 0.0f;
  send[maxn + i] = i < ns ? scale[i] : 0.0f;
  send[2 * maxn + i] = i < ns ? (inside[i] ? 1.0f : 0.0f) : 0.0f;
}

__global__ void k_slice_em_pack(const float *pot, const float *scale, const unsigned char *inside, int n, int maxn, float *send) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= maxn) return;
  send[i] = i < n ? pot[i] : 0.0f;
  send[maxn + i] = i < n ? scale[i] : 0.0f;
  send[2 * maxn + i] = i < n ? (inside[i] ? 1.0f : 0.0f) : 0.0f;
}

// K quantities reduced side by side over the 256 threads: the fixed tree of one block reduction per quantity (the bits of reducing them one after
// the other), one set of barriers for all of them -- the kernel is one workgroup and nothing but latency.  op[k]: 0 = sum, 1 = max, 2 = min.
template <int K>
__device__ __forceinline__ void block_reduce256(double (&v)[K], const int (&op)[K], double (*sh)[256]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < K; ++k) sh[k][t] = v[k];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const double x = sh[k][t], y = sh[k][t + o];
        sh[k][t] = op[k] == 0 ? x + y : (op[k] == 1 ? fmax(x, y) : fmin(x, y));
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = sh[k][0];
  __syncthreads();
}

// svr::irtkReconstruction::EStepGPU's host half (RG.cc:3282-3420), one workgroup of 256
//
// PATCH: irtkPatchBasedReconstruction's EM (csrc/pvr_host.cpp EStep; patchBasedRobustStatistics_gpu.cu:224-556) is the same two-class EM with
// three differences, all kept: a patch reads the potential of ANOTHER patch (the reference copies the stacks' potentials without the stack
// offset on the left, :256-276 -- `src`, built by the host object in the reference's numbering), the Gaussian is evaluated in float with
// the literal 0.00001f (:97-101), and the variance floor is step * step in float.
template <bool PATCH>
__global__ __launch_bounds__(256) void k_slice_em(const float *recv, int world, const int *rlo, int maxn, int ns, const int *by_ref, const unsigned char *excl,
                                                   double step, float *pot_g, float *scale_g, float *inside_g, float *w_g, double *sc, int my_lo, int my_n,
                                                   float *w_local, float *raw_g, const int *src) {
  __shared__ double sh[6][256];
  const int t = threadIdx.x;
  const double floor_ = PATCH ? (double)((float)step * (float)step) / 6.28 : step * step / 6.28;
  // unpack the ranks' vectors into the global ones (host numbering), apply the exclusions (RG.cc:3288-3300)
  for (int g = t; g < ns; g += 256) {
    int r = 0;
    while (r + 1 < world && g >= rlo[r + 1]) ++r;
    const int l = g - rlo[r];
    const float *p = recv + (size_t)r * 3 * maxn;
    raw_g[g] = p[l]; scale_g[g] = p[maxn + l]; inside_g[g] = p[2 * maxn + l];
  }
  __syncthreads();
  for (int g = t; g < ns; g += 256) {
    float pot = raw_g[g];
    if (PATCH && src) pot = src[g] >= 0 ? raw_g[src[g]] : 0.0f;
    const float scale = scale_g[g];
    if (excl[g]) pot = -1.0f;
    if ((scale < 0.2) || (scale > 5)) pot = -1.0f;
    pot_g[g] = pot;
  }
  __syncthreads();
  // first pass: means (RG.cc:3302-3326)
  double sum = 0, den = 0, sum2 = 0, den2 = 0, maxs = 0, mins = 1;
  for (int k = t; k < ns; k += 256) {
    const int g = by_ref[k];
    const float pot = pot_g[g], w = w_g[g];
    if (pot >= 0) {
      sum += pot * w;
      den += w;
      sum2 += pot * (1.0 - w);
      den2 += (1.0 - w);
      if (pot > maxs) maxs = pot;
      if (pot < mins) mins = pot;
    }
  }
  {
    double v6[6] = {sum, den, sum2, den2, maxs, mins};
    const int op6[6] = {0, 0, 0, 0, 1, 2};
    block_reduce256<6>(v6, op6, sh);
    sum = v6[0]; den = v6[1]; sum2 = v6[2]; den2 = v6[3]; maxs = v6[4]; mins = v6[5];
  }
  float mean_s, mean_s2;
  if (den > 0) mean_s = (float)(sum / den);
  else mean_s = (float)mins;
  if (den2 > 0) mean_s2 = (float)(sum2 / den2);
  else mean_s2 = (float)((maxs + mean_s) / 2.0);
  // second pass: variances (RG.cc:3328-3366)
  sum = 0; den = 0; sum2 = 0; den2 = 0;
  for (int k = t; k < ns; k += 256) {
    const int g = by_ref[k];
    const float pot = pot_g[g], w = w_g[g];
    if (pot >= 0) {
      sum += (pot - mean_s) * (pot - mean_s) * w;
      den += w;
      sum2 += (pot - mean_s2) * (pot - mean_s2) * (1 - w);
      den2 += (1 - w);
    }
  }
  {
    double v4[4] = {sum, den, sum2, den2};
    const int op4[4] = {0, 0, 0, 0};
    block_reduce256<4>(v4, op4, sh);
    sum = v4[0]; den = v4[1]; sum2 = v4[2]; den2 = v4[3];
  }
  float sigma_s, sigma_s2;
  if ((sum > 0) && (den > 0)) {
    sigma_s = (float)(sum / den);
    if (sigma_s < floor_) sigma_s = (float)floor_;
  } else {
    sigma_s = 0.025f;
  }
  if ((sum2 > 0) && (den2 > 0)) {
    sigma_s2 = (float)(sum2 / den2);
    if (sigma_s2 < floor_) sigma_s2 = (float)floor_;
  } else {
    sigma_s2 = (mean_s2 - mean_s) * (mean_s2 - mean_s) / 4;
    if (sigma_s2 < floor_) sigma_s2 = (float)floor_;
  }
  const float mix_s = (float)sc[4];
  // the slice weights (RG.cc:3368-3398); G of RG.h:529-532
  double wsum = 0;
  int num = 0;
  for (int g = t; g < ns; g += 256) {
    const float pot = pot_g[g];
    float w = w_g[g];
    if (pot == -1) {
      w = 0;
    } else if ((den <= 0) || (mean_s2 <= mean_s)) {
      w = 1;
    } else {
      double gs1, gs2;
      if (PATCH) {                                       // G_ of csrc/pvr_host.cpp (PRS.cu:97-101): float throughout
        if (pot < mean_s2) { const float x = pot - mean_s, s = sigma_s; gs1 = 0.00001f * expf(-x * x / (2.0f * s)) / sqrtf(6.28f * s); }
        else gs1 = 0;
        if (pot > mean_s) { const float x = pot - mean_s2, s = sigma_s2; gs2 = 0.00001f * expf(-x * x / (2.0f * s)) / sqrtf(6.28f * s); }
        else gs2 = 0;
      } else {
        if (pot < mean_s2) { const double x = pot - mean_s, s = sigma_s; gs1 = step * exp(-x * x / (2 * s)) / (sqrt(6.28 * s)); }
        else gs1 = 0;
        if (pot > mean_s) { const double x = pot - mean_s2, s = sigma_s2; gs2 = step * exp(-x * x / (2 * s)) / (sqrt(6.28 * s)); }
        else gs2 = 0;
      }
      const double likelihood = gs1 * mix_s + gs2 * (1 - mix_s);
      if (likelihood > 0) w = (float)(gs1 * mix_s / likelihood);
      else {
        if (pot <= mean_s) w = 1;
        if (pot >= mean_s2) w = 0;
        if ((pot < mean_s2) && (pot > mean_s)) w = 1;
      }
    }
    w_g[g] = w;
    if (pot >= 0) { wsum += w; ++num; }
  }
  __syncthreads();
  // mixing proportion (RG.cc:3400-3408): in the reference's order again
  wsum = 0;
  for (int k = t; k < ns; k += 256) {
    const int g = by_ref[k];
    if (pot_g[g] >= 0) wsum += w_g[g];
  }
  double nn;
  {
    double v2[2] = {wsum, (double)num};
    const int op2[2] = {0, 0};
    block_reduce256<2>(v2, op2, sh);
    wsum = v2[0]; nn = v2[1];
  }
  if (t == 0) {
    sc[0] = mean_s; sc[1] = mean_s2; sc[2] = sigma_s; sc[3] = sigma_s2;
    sc[4] = nn > 0 ? (double)(float)(wsum / nn) : (double)0.9f;
  }
  for (int i = t; i < my_n; i += 256) w_local[i] = w_g[my_lo + i];
}

}  // namespace

extern "C" {

int svr_slice_em_setup(svr_ctx *ctx, int ns_global, int world, int rank, const int *rank_lo, const int *order_or_null, double step) {
  SVR_ENTER(ctx);
  if (!ctx || ns_global <= 0 || world < 1 || rank < 0 || rank >= world || !rank_lo) return SVR_E_ARG;
  NEED(ctx->ns > 0, "initStorageVolumes first");
  if (rank_lo[0] != 0 || rank_lo[world] != ns_global || rank_lo[rank + 1] - rank_lo[rank] != (int)ctx->ns)
    return fail(ctx, SVR_E_ARG, "svr_slice_em_setup: the ranks' ranges do not match the engine's slices");
  slice_em_free(ctx->sem);                              // a fresh object: the old buffers go before the new ones come
  SliceEm &p = *(ctx->sem = new SliceEm());
  ctx->sem_weights_current = false;
  p.ns = ns_global; p.world = world; p.rank = rank; p.step = step;
  p.rlo.assign(rank_lo, rank_lo + world + 1);
  p.maxn = 1;
  for (int r = 0; r < world; ++r) {
    if (rank_lo[r + 1] < rank_lo[r]) return fail(ctx, SVR_E_ARG, "svr_slice_em_setup: ranges out of order");
    p.maxn = std::max(p.maxn, rank_lo[r + 1] - rank_lo[r]);
  }
  std::vector<int> by_ref(ns_global);
  for (int k = 0; k < ns_global; ++k) by_ref[k] = k;
  if (order_or_null) {
    std::vector<char> seen(ns_global, 0);
    for (int k = 0; k < ns_global; ++k) {
      const int t = order_or_null[k];
      if (t < 0 || t >= ns_global || seen[t]) return fail(ctx, SVR_E_ARG, "svr_slice_em_setup: the unit order is not a permutation");
      seen[t] = 1;
      by_ref[t] = k;
    }
  }
  const size_t n = (size_t)ns_global;
  HIPCHK(p.d_rlo.reserve(world + 1));
  HIPCHK(p.d_by_ref.reserve(n));
  HIPCHK(p.d_excl.reserve(n));
  HIPCHK(p.d_send.reserve((size_t)3 * p.maxn));
  HIPCHK(p.d_recv.reserve((size_t)world * 3 * p.maxn));
  HIPCHK(p.d_pot.reserve(n));
  HIPCHK(p.d_scale.reserve(n));
  HIPCHK(p.d_w.reserve(n));
  HIPCHK(p.d_inside.reserve(n));
  HIPCHK(p.d_sc.reserve(8));
  HIPCHK(p.d_raw.reserve(n));
  p.h_by_ref = by_ref;
  HIPCHK(hipMemcpyAsync(p.d_rlo, p.rlo.data(), (world + 1) * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(p.d_by_ref, by_ref.data(), n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemsetAsync(p.d_excl, 0, n, ctx->stream));
  HIPCHK(hipMemsetAsync(p.d_pot, 0, n * sizeof(float), ctx->stream));
  HIPCHK(hipMemsetAsync(p.d_scale, 0, n * sizeof(float), ctx->stream));
  HIPCHK(hipMemsetAsync(p.d_inside, 0, n * sizeof(float), ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));            // (by_ref is this function's memory)
  HIPCHK(ctx->d_em.reserve(4));
  p.ready = true;
  return SVR_OK;
}

/* The patch-based host's form of the EM (csrc/pvr_host.cpp): source_ref[t] = the REFERENCE index of the patch whose potential the patch with
 * reference index t reads, or -1 for none (potential 0) -- the reference's copy without the stack offset, PRS.cu:256-276; NULL = its own.
 * After svr_slice_em_setup (which resets it). */
int svr_slice_em_set_patch_form(svr_ctx *ctx, const int *source_ref_or_null) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  NEED(ctx->sem && ctx->sem->ready, "svr_slice_em_setup first");
  SliceEm &p = *ctx->sem;
  p.patch_form = 1;
  p.d_src.reset();
  if (!source_ref_or_null) return SVR_OK;
  std::vector<int> src((size_t)p.ns, -1);
  for (int t = 0; t < p.ns; ++t) {
    const int u = source_ref_or_null[t];
    if (u >= p.ns) return fail(ctx, SVR_E_ARG, "svr_slice_em_set_patch_form: source out of range");
    src[p.h_by_ref[t]] = u < 0 ? -1 : p.h_by_ref[u];
  }
  HIPCHK(p.d_src.reserve((size_t)p.ns));
  HIPCHK(hipMemcpyAsync(p.d_src, src.data(), (size_t)p.ns * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

int svr_slice_em_set_state(svr_ctx *ctx, const float *slice_weights_global, const unsigned char *excluded_global, const double scalars5[5],
                           const float em3[3]) {
  SVR_ENTER(ctx);
  if (!ctx || !slice_weights_global || !excluded_global || !scalars5 || !em3) return SVR_E_ARG;
  NEED(ctx->sem && ctx->sem->ready, "svr_slice_em_setup first");
  SliceEm &p = *ctx->sem;
  // small, rare (once per outer iteration): plain copies through the stream, then a wait so that the caller's memory is free again
  ctx->sem_weights_current = false;                      // (the scatter's vector is not what p.d_w holds any more)
  HIPCHK(hipMemcpyAsync(p.d_w, slice_weights_global, (size_t)p.ns * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(p.d_excl, excluded_global, (size_t)p.ns, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(p.d_sc, scalars5, 5 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(ctx->d_em, em3, 3 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

int svr_mstep_estep_device(svr_ctx *ctx, int iter, float step, void **send, void **recv, size_t *n_floats_per_rank) {
  SVR_ENTER(ctx);
  if (!ctx || !send || !recv || !n_floats_per_rank) return SVR_E_ARG;
  NEED(ctx->have_slices && ctx->have_scales, "slices / scales not set");
  NEED(ctx->sem && ctx->sem->ready, "svr_slice_em_setup first");
  SliceEm &p = *ctx->sem;
  int r;
  if (iter > 0) {
    if (p.world > 1) {
      NEED((size_t)p.world * 8 <= ctx->d_em_all.capacity(), "svr_mstep_partial + the launcher's all-gather first");
      hipLaunchKernelGGL(k_mstep_scalars_dev, dim3(1), dim3(1), 0, ctx->stream, ctx->d_em_all, p.world, iter, step, ctx->pvr ? 1 : 0, ctx->d_em);
    } else {
      // (round 6: k_mstep, then ONE workgroup for the chunk sums, the slice sums and the scalars: k_mstep_finish)
      ScopedTimer tm(ctx, SVR_T_MSTEP);
      hipLaunchKernelGGL(k_mstep, dim3(ctx->chunks, ctx->ns), dim3(256), 0, ctx->stream, ctx->d_slices, ctx->d_weights,
                         ctx->d_simslices, ctx->d_simweights, ctx->d_scales_host_copy,
                         ctx->disable_bias ? (const float *)nullptr : ctx->d_bias, (int)(ctx->sx * ctx->sy), ctx->d_partial);
      KCHK("k_mstep");
      hipLaunchKernelGGL(k_mstep_finish, dim3(1), dim3(256), 0, ctx->stream, ctx->d_partial, (int)ctx->ns, ctx->chunks, ctx->d_per_slice, ctx->d_out, iter, step,
                         ctx->pvr ? 1 : 0, ctx->d_em);
      tm.stop();
    }
    KCHK("k_mstep_scalars_dev");
  }
  {
    // the E-step, its potentials and the slice-level EM's packed input: two launches (k_estep, k_potential_pack) instead of three
    ScopedTimer te(ctx, SVR_T_ESTEP);
    hipLaunchKernelGGL(k_estep, dim3(ctx->chunks, ctx->ns), dim3(256), 0, ctx->stream, ctx->d_slices, ctx->d_simslices,
                       ctx->d_simweights, ctx->d_scales, ctx->disable_bias ? (const float *)nullptr : ctx->d_bias, 0.0f, 0.0f,
                       0.0f, (int)(ctx->sx * ctx->sy), ctx->d_weights, ctx->d_partial, ctx->pvr, ctx->d_em);
    KCHK("k_estep");
    ctx->have_em = true;
    hipLaunchKernelGGL(k_potential_pack, dim3(nblk(p.maxn)), dim3(256), 0, ctx->stream, ctx->d_partial, (int)ctx->ns, ctx->chunks, ctx->d_tmp_ns,
                       ctx->d_scales_host_copy, ctx->d_slice_inside, p.maxn, p.d_send);
    KCHK("k_potential_pack");
    te.stop();
  }
  *send = p.d_send;
  *recv = p.world > 1 ? p.d_recv : p.d_send;
  *n_floats_per_rank = (size_t)3 * p.maxn;
  return SVR_OK;
}

int svr_slice_em_run(svr_ctx *ctx) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  NEED(ctx->sem && ctx->sem->ready, "svr_slice_em_setup first");
  SliceEm &p = *ctx->sem;
  ScopedTimer t(ctx, SVR_T_ESTEP);
  if (p.patch_form)
    hipLaunchKernelGGL(k_slice_em<true>, dim3(1), dim3(256), 0, ctx->stream, p.world > 1 ? p.d_recv : p.d_send, p.world, p.d_rlo, p.maxn, p.ns, p.d_by_ref,
                       p.d_excl, p.step, p.d_pot, p.d_scale, p.d_inside, p.d_w, p.d_sc, p.rlo[p.rank], (int)ctx->ns, ctx->d_slice_weights, p.d_raw, p.d_src);
  else
    hipLaunchKernelGGL(k_slice_em<false>, dim3(1), dim3(256), 0, ctx->stream, p.world > 1 ? p.d_recv : p.d_send, p.world, p.d_rlo, p.maxn, p.ns, p.d_by_ref,
                       p.d_excl, p.step, p.d_pot, p.d_scale, p.d_inside, p.d_w, p.d_sc, p.rlo[p.rank], (int)ctx->ns, ctx->d_slice_weights, p.d_raw, nullptr);
  KCHK("k_slice_em");
  t.stop();
  ctx->mir_slice_weights.clear();                        // the device vector no longer holds what the host last sent
  ctx->mir_scales_copy.clear();
  ctx->sem_weights_current = true;
  return SVR_OK;
}

/* this rank's part of the EM's slice weights -> the vector the scatter reads (svr_slice_em_run does it too; a caller that may have sent other
 * weights in between -- a warm-up scatter with unit weights -- asks again: one device-to-device copy of ns floats, no wait) */
int svr_slice_em_apply_weights(svr_ctx *ctx) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  NEED(ctx->sem && ctx->sem->ready, "svr_slice_em_setup first");
  SliceEm &p = *ctx->sem;
  if (ctx->sem_weights_current) return SVR_OK;           // still what svr_slice_em_run left there (every upload into the vector clears the flag)
  HIPCHK(hipMemcpyAsync(ctx->d_slice_weights, p.d_w + p.rlo[p.rank], (size_t)ctx->ns * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
  ctx->mir_slice_weights.clear();
  ctx->sem_weights_current = true;
  return SVR_OK;
}

int svr_slice_em_fetch(svr_ctx *ctx, float *scale_global, float *slice_weight_global, float *slice_potential_global, unsigned char *slice_inside_global,
                       double scalars5[5], float em3[3]) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  NEED(ctx->sem && ctx->sem->ready, "svr_slice_em_setup first");
  SliceEm &p = *ctx->sem;
  const size_t nb = (size_t)p.ns * sizeof(float);
  std::vector<float> inside(slice_inside_global ? p.ns : 0);
  int r;
  // the whole batch is reserved before its first copy is queued: the vectors have the GLOBAL slice count, the arena's first size follows the local one
  if ((r = down_reserve(ctx, 4 * ((nb + 63) & ~(size_t)63) + 128))) return r;
  if (scale_global && (r = down_queue(ctx, scale_global, p.d_scale, nb))) return r;
  if (slice_weight_global && (r = down_queue(ctx, slice_weight_global, p.d_w, nb))) return r;
  if (slice_potential_global && (r = down_queue(ctx, slice_potential_global, p.d_pot, nb))) return r;
  if (slice_inside_global && (r = down_queue(ctx, inside.data(), p.d_inside, nb))) return r;
  if (scalars5 && (r = down_queue(ctx, scalars5, p.d_sc, 5 * sizeof(double)))) return r;
  if (em3 && (r = down_queue(ctx, em3, ctx->d_em, 3 * sizeof(float)))) return r;
  if ((r = down_flush(ctx))) return r;
  if (slice_inside_global) for (int i = 0; i < p.ns; ++i) slice_inside_global[i] = inside[i] > 0.5f;
  return SVR_OK;
}

}  // extern "C"
