// svr_quality.inc -- per-slice agreement between the slices and the volume they built (svr_slice_quality), included by svr_hip.hip.
//
// Not a step of the reconstruction: a report on its result.  The reference keeps the pieces (irtkReconstruction::SlicesInfo,
// SimulateStacks, EvaluateGPU: irtkReconstructionGPU.cc:4937-4975, 1205-1262, 4503-4538) and its main() never calls the first two.
// After a forward projection everything the report needs is on the device; what is missing is one reduction per slice.
//
// Per pixel, with the float expressions of the M-step (k_mstep, svr_small.inc):
//   x = bias ? s * expf(-bias) * scale : s * scale        (scale: the vector the M-step reads, d_scales_host_copy)
//   y = simslices,  e = x - y  (float)
// and per slice the ten sums  {n_px, n, S x, S y, S x^2, S y^2, S xy, S e^2, S |e|, S w}:  n_px counts s != -1, the others run over
// the M-step's pixel set (s != -1 and simweight > 0.99, with k_mstep's bias-dependent comparison).  Every product is formed in double
// from the float operands (exact: 24 x 24 bits) and every sum is kept in double.
//
//   k_slice_quality         grid = ns x chunks workgroups of 256.  A workgroup owns a contiguous range of one slice's pixels; a lane adds
//                           its pixels into ten double registers in index order, the wavefront folds them with a fixed xor tree
//                           (offsets 32 .. 1), lane 0 of each wavefront puts its ten sums into the LDS and ten threads add the four
//                           wavefronts in wave order and store the (slice, chunk) partial.
//   k_slice_quality_finish  thread (slice, k) adds the slice's chunks in chunk order (as k_mstep_finish does for the M-step).
// No atomics and no order that depends on scheduling: the same bits on every call.  The chunks of a slice follow from sx * sy alone
// (quality_chunks: QUAL_CHUNK_PIX pixels each, at most QUAL_MAX_CHUNKS), readable afterwards as the option "quality_chunks".
// The five arrays share one alignment (hipMalloc, one index), so a range is a scalar head up to the next multiple of four
// floats, float4 loads, and a scalar tail.  One pass: 4 floats per pixel without bias, 5 with.  Units are slices or patches alike.
// The scratch (partials and the result) is allocated by the call and freed before it returns, like svr_stack_motion's: the
// coefficient table sizes itself by the memory that is free, and nothing here is cached, so the invalidation map has no line for it.

#define QUAL_K SVR_SLICE_QUALITY_SUMS
#define QUAL_CHUNK_PIX 16384              // pixels of a chunk: 64 per lane, 16 float4 loads per array and lane
#define QUAL_MAX_CHUNKS 64

namespace {

inline int quality_chunks(size_t n2) {
  return (int)std::min<size_t>(QUAL_MAX_CHUNKS, std::max<size_t>(1, (n2 + QUAL_CHUNK_PIX - 1) / QUAL_CHUNK_PIX));
}
// pixels per chunk: the slice's pixels dealt evenly, rounded up to whole float4s (no chunk of a slice is empty: a second chunk
// exists only above QUAL_CHUNK_PIX pixels)
inline int quality_chunk_len(size_t n2, int chunks) { return (int)((((n2 + chunks - 1) / chunks) + 3) & ~(size_t)3); }

template <bool BIAS>
__device__ __forceinline__ void qual_pixel(float s, float sw, float y, float w, float b, float scale, double v[QUAL_K]) {
  if (s == -1.0f) return;
  v[0] += 1.0;
  if (!(BIAS ? (double)sw > 0.99 : sw > 0.99f)) return;     // k_mstep's set (RC.cu:2947, 2985)
  const float x = BIAS ? s * expf(-b) * scale : s * scale;
  const float e = x - y;
  const double dx = (double)x, dy = (double)y, de = (double)e;
  v[1] += 1.0;
  v[2] += dx;
  v[3] += dy;
  v[4] += dx * dx;
  v[5] += dy * dy;
  v[6] += dx * dy;
  v[7] += de * de;
  v[8] += fabs(de);
  v[9] += (double)w;
}

template <bool BIAS>
__global__ __launch_bounds__(256) void k_slice_quality(const float *__restrict__ slices, const float *__restrict__ weights,
                                                       const float *__restrict__ simslices, const float *__restrict__ simweights,
                                                       const float *__restrict__ scales, const float *__restrict__ bias, int n2, int chunks,
                                                       int chunk_len, double *__restrict__ partial) {
  __shared__ double sm[4][QUAL_K];
  const int sl = (int)(blockIdx.x / (unsigned)chunks), c = (int)(blockIdx.x - (unsigned)sl * (unsigned)chunks);
  const float scale = scales[sl];
  const int p0 = min(n2, c * chunk_len), p1 = min(n2, p0 + chunk_len);
  const size_t g0 = (size_t)sl * n2 + p0;                    // first element of the range in the arrays
  const int len = p1 - p0;
  const int head = min(len, (int)((4 - (g0 & 3)) & 3)), nvec = (len - head) >> 2, tail = len - head - 4 * nvec;
  const int t = threadIdx.x;
  double v[QUAL_K];
#pragma unroll
  for (int k = 0; k < QUAL_K; ++k) v[k] = 0.0;
  if (t < head) {
    const size_t g = g0 + t;
    qual_pixel<BIAS>(slices[g], simweights[g], simslices[g], weights[g], BIAS ? bias[g] : 0.0f, scale, v);
  }
  const size_t gv = g0 + head;                               // a multiple of four floats
  for (int i = t; i < nvec; i += 256) {
    const size_t g = gv + 4 * (size_t)i;
    const float4 s4 = *reinterpret_cast<const float4 *>(slices + g), sw4 = *reinterpret_cast<const float4 *>(simweights + g);
    const float4 y4 = *reinterpret_cast<const float4 *>(simslices + g), w4 = *reinterpret_cast<const float4 *>(weights + g);
    float4 b4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (BIAS) b4 = *reinterpret_cast<const float4 *>(bias + g);
    qual_pixel<BIAS>(s4.x, sw4.x, y4.x, w4.x, b4.x, scale, v);
    qual_pixel<BIAS>(s4.y, sw4.y, y4.y, w4.y, b4.y, scale, v);
    qual_pixel<BIAS>(s4.z, sw4.z, y4.z, w4.z, b4.z, scale, v);
    qual_pixel<BIAS>(s4.w, sw4.w, y4.w, w4.w, b4.w, scale, v);
  }
  if (t < tail) {
    const size_t g = gv + 4 * (size_t)nvec + t;
    qual_pixel<BIAS>(slices[g], simweights[g], simslices[g], weights[g], BIAS ? bias[g] : 0.0f, scale, v);
  }
#pragma unroll
  for (int k = 0; k < QUAL_K; ++k) {
    double x = v[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    v[k] = x;
  }
  const int w = t >> 6, lane = t & 63;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < QUAL_K; ++k) sm[w][k] = v[k];
  }
  __syncthreads();
  if (t < QUAL_K) partial[(size_t)blockIdx.x * QUAL_K + t] = ((sm[0][t] + sm[1][t]) + sm[2][t]) + sm[3][t];   // wave order
}

__global__ void k_slice_quality_finish(const double *__restrict__ partial, int ns, int chunks, double *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ns * QUAL_K) return;
  const int sl = i / QUAL_K, k = i - sl * QUAL_K;
  double x = partial[((size_t)sl * chunks) * QUAL_K + k];
  for (int c = 1; c < chunks; ++c) x += partial[((size_t)sl * chunks + c) * QUAL_K + k];
  out[i] = x;
}

int slice_quality_run(svr_ctx *ctx, double *sums) {
  const size_t n2 = (size_t)ctx->sx * ctx->sy;
  const int chunks = quality_chunks(n2), chunk_len = quality_chunk_len(n2, chunks);
  const size_t blocks = (size_t)ctx->ns * chunks, nout = (size_t)ctx->ns * QUAL_K;
  if (blocks >= (1ull << 31) || nout >= (1ull << 31)) return fail(ctx, SVR_E_ARG, "svr_slice_quality: too many slices");
  const float *bias = ctx->disable_bias ? (const float *)nullptr : ctx->d_bias;
  DevBuf<double> d_partial, d_sums;                          // nothing is kept beyond the call: the coefficient table sizes itself by the memory that is free
  HIPCHK(d_partial.reserve(blocks * QUAL_K));
  HIPCHK(d_sums.reserve(nout));
  hipLaunchKernelGGL(bias ? k_slice_quality<true> : k_slice_quality<false>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, ctx->d_slices,
                     ctx->d_weights, ctx->d_simslices, ctx->d_simweights, ctx->d_scales_host_copy, bias, (int)n2, chunks, chunk_len,
                     d_partial.get());
  KCHK("k_slice_quality");
  hipLaunchKernelGGL(k_slice_quality_finish, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, ctx->stream, d_partial.get(), (int)ctx->ns,
                     chunks, d_sums.get());
  KCHK("k_slice_quality_finish");
  ctx->last_quality_chunks = chunks;
  HIPCHK(hipMemcpyAsync(sums, d_sums.get(), nout * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

}  // namespace

extern "C" {

int svr_slice_quality(svr_ctx *ctx, double *sums) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  if (!sums) return fail(ctx, SVR_E_ARG, "svr_slice_quality: no array for the sums");
  NEED(ctx->np > 0 && ctx->have_slices, "slices not filled");
  NEED(ctx->have_scales, "scale vector not set");
  NEED(ctx->have_sim, "no simulated slices (svr_simulate_slices first)");
  int r = ensure_bias_buffers(ctx);                          // (as every compute call: a bias path switched on before the slice grid existed)
  if (r) return r;
  return slice_quality_run(ctx, sums);
}

}  // extern "C"
