// svr_sim.inc -- the similarity of the default (IRTK) registration on the device: the one sampler of its three metrics, the one
// evaluation scratch and launch chain of their evaluate calls, and the cross correlation itself; included by svr_hip.hip before
// svr_nmi.inc and svr_lncc.inc.
//
// The sampler restates irtkImageRigidRegistrationWithPadding::Evaluate (IRRWP.cc:534-610) for one target pixel: the source position
// from the evaluation's 4 x 4 in double, the strict inside test, the double trilinear in EvaluateInside's operation order, value >= 0,
// IRTK's round().  V = the target pixels (tv >= 0) that pass all of it.  k_ncc below, k_nmi and k_lncc all take their samples from
// sim_sample, so the three metrics see the same V and the same rounded source values by construction; what each does with a sample
// (six moments, a joint histogram bin, a word of the window's LDS ring) is its own.  The library is built with -ffp-contract=off
// -fno-fast-math (build.py): inlining the sampler into three kernels can neither fuse nor re-associate any of its operations, and
// the bit-for-bit guarantees of the three metrics rest on that -- keep both flags.

namespace {

// What one (plane, candidate) needs to sample: the nine entries of its matrix that a plane (k = 0) uses, the source's upper
// bounds and strides.  Loaded once per (plane, candidate) from mats + 16 * e.
struct SimPlane {
  double m00, m01, m03, m10, m11, m13, m20, m21, m23;
  double sx2, sy2, sz2;
  size_t o3, o5;
  const short *source;
};

__device__ __forceinline__ SimPlane sim_plane(const double *mats, size_t e, const short *source, int vx, int vy, int vz) {
  const double *M = mats + 16 * e;
  return SimPlane{M[0], M[1], M[3], M[4], M[5], M[7], M[8], M[9], M[11], (double)(vx - 1), (double)(vy - 1), (double)(vz - 1),
                  (size_t)vx, (size_t)vx * vy, source};
}

// pixel (i, j) of a plane with target value tv: is it in V, and if so its rounded source value
__device__ __forceinline__ bool sim_sample(const SimPlane &P, int i, int j, int tv, int &sv) {
  if (tv < 0) return false;
  const double X = P.m00 * i + P.m01 * j + P.m03, Y = P.m10 * i + P.m11 * j + P.m13, Z = P.m20 * i + P.m21 * j + P.m23;
  if (!((X > 0) && (X < P.sx2) && (Y > 0) && (Y < P.sy2) && (Z > 0) && (Z < P.sz2))) return false;
  const int a = (int)X, b = (int)Y, c = (int)Z;
  const double t1 = X - a, u1 = Y - b, v1 = Z - c, t2 = 1 - t1, u2 = 1 - u1, v2 = 1 - v1;
  const size_t o3 = P.o3, o5 = P.o5;
  const short *q = P.source + a + (size_t)b * o3 + (size_t)c * o5;
  const double value = (t1 * (u2 * (v2 * q[1] + v1 * q[o5 + 1]) + u1 * (v2 * q[o3 + 1] + v1 * q[o5 + o3 + 1])) +
                        t2 * (u2 * (v2 * q[0] + v1 * q[o5]) + u1 * (v2 * q[o3] + v1 * q[o5 + o3])));
  if (!(value >= 0)) return false;
  sv = value > 0 ? (int)(value + 0.5) : (int)(value - 0.5);   // irtkCommon.h:85-88
  return true;
}

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- the evaluate calls' device scratch and launch chain ------------------------------------------------------------------------
// One grow-only arena of the context (d_sim_io, sim_staging) serves svr_ncc_evaluate, svr_nmi_evaluate and
// svr_lncc_evaluate: inputs | outputs | optional test map, each part at 8-byte alignment.  sim_evaluate checks the target indices,
// grows the arena (3/2 of the need, at least `floor` bytes), stages the inputs and uploads them in one copy, runs the caller's
// launch(d_in, d_out, d_map), downloads the outputs (and the map) and waits.
struct SimSeg { const void *p; size_t bytes; };

template <class Launch>
int sim_evaluate(svr_ctx *ctx, const char *name, const int *target_index, size_t n_planes, std::initializer_list<SimSeg> inputs, void *h_out,
                 size_t b_out, void *h_map, size_t b_map, size_t floor, Launch launch) {
  for (size_t i = 0; i < n_planes; ++i)
    if (target_index[i] < 0 || target_index[i] >= ctx->reg_n) return fail(ctx, SVR_E_ARG, "target index out of range");
  size_t b_in = 0;
  for (const SimSeg &s : inputs) b_in += s.bytes;
  const size_t o_out = (b_in + 7) / 8 * 8, o_map = (o_out + b_out + 7) / 8 * 8, need = o_map + b_map;
  if (need > ctx->d_sim_io.capacity()) HIPCHK(ctx->d_sim_io.reserve(std::max(floor, need * 3 / 2 + 4096)));
  ctx->sim_staging.resize(b_in);
  size_t at = 0;
  for (const SimSeg &s : inputs) { memcpy(ctx->sim_staging.data() + at, s.p, s.bytes); at += s.bytes; }
  unsigned char *d = ctx->d_sim_io;
  hipError_t e = hipMemcpyAsync(d, ctx->sim_staging.data(), b_in, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    launch(d, d + o_out, b_map ? d + o_map : nullptr);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(h_out, d + o_out, b_out, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && b_map) e = hipMemcpyAsync(h_map, d + o_map, b_map, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return fail(ctx, (int)e, name);
  return SVR_OK;
}

// ------------------------------------------------------------------------------------------
// slice-to-volume NCC cost (the CPU-default registration metric, SURVEY 8a16):
// irtkImageRigidRegistrationWithPadding::Evaluate + irtkCrossCorrelationSimilarityMetric.
// One workgroup per (target slice, candidate transform): the six integer moments of the samples are accumulated exactly in
// int64 and reduced with wavefront shuffles -- order-independent, so the moments equal the serial CPU loop's.
// ------------------------------------------------------------------------------------------
__global__ void k_f32_to_i16(const float *in, short *out, size_t n) {   // static_cast<short>(float): truncation
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (short)in[i];
}

__global__ __launch_bounds__(256) void k_ncc(const short *targets, int tx, int ty, const int *target_index,
                                             const double *mats, const short *source, int vx, int vy, int vz,
                                             long long *sums) {
  __shared__ long long sm[4][6];
  const int e = blockIdx.x;
  const short *tgt = targets + (size_t)target_index[e] * tx * ty;
  const SimPlane P = sim_plane(mats, e, source, vx, vy, vz);
  long long a_n = 0, a_x = 0, a_y = 0, a_x2 = 0, a_y2 = 0, a_xy = 0;
  for (int p = threadIdx.x; p < tx * ty; p += 256) {
    const int tv = tgt[p];
    if (tv < 0) continue;
    const int j = p / tx, i = p - j * tx;
    int sv;
    if (sim_sample(P, i, j, tv, sv)) {
      a_n += 1; a_x += tv; a_y += sv; a_x2 += (long long)tv * tv; a_y2 += (long long)sv * sv;
      a_xy += (long long)tv * sv;
    }
  }
  long long v[6] = {a_n, a_x, a_y, a_x2, a_y2, a_xy};
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    v[k] = wave_sum_i64(v[k]);
    if (lane == 0) sm[w][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < 6) sums[6 * (size_t)e + threadIdx.x] = sm[0][threadIdx.x] + sm[1][threadIdx.x] + sm[2][threadIdx.x] + sm[3][threadIdx.x];
}

}  // namespace

extern "C" {

int svr_ncc_set_targets(svr_ctx *ctx, int n, int tx, int ty, const int16_t *targets) {
  SVR_ENTER(ctx);
  if (!ctx || !targets || n <= 0 || tx <= 0 || ty <= 0) return SVR_E_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  ctx->d_reg_targets.reset();
  const size_t bytes = (size_t)n * tx * ty * sizeof(short);
  HIPCHK(ctx->d_reg_targets.reserve((size_t)n * tx * ty));
  HIPCHK(hipMemcpyAsync(ctx->d_reg_targets, targets, bytes, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->reg_n = n; ctx->reg_tx = tx; ctx->reg_ty = ty;
  return SVR_OK;
}

int svr_ncc_set_source(svr_ctx *ctx, const uint32_t size[3], const int16_t *source_or_null) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  if (!source_or_null) NEED(ctx->nv > 0, "no source given and no reconstruction volume");
  uint32_t sx = source_or_null ? size[0] : ctx->vx, sy = source_or_null ? size[1] : ctx->vy,
           sz = source_or_null ? size[2] : ctx->vz;
  const size_t n = (size_t)sx * sy * sz;
  if (n == 0) return SVR_E_ARG;
  ctx->d_reg_source.reset();
  HIPCHK(ctx->d_reg_source.reserve(n));
  if (source_or_null) {
    HIPCHK(hipMemcpyAsync(ctx->d_reg_source, source_or_null, n * sizeof(short), hipMemcpyHostToDevice, ctx->stream));
  } else {
    // irtkGreyImage source = _reconstructed  (RG.cc:2031): static_cast<short> of every voxel
    hipLaunchKernelGGL(k_f32_to_i16, dim3(nblk(n)), dim3(256), 0, ctx->stream, ctx->recon(), ctx->d_reg_source, n);
    KCHK("k_f32_to_i16");
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->reg_vx = sx; ctx->reg_vy = sy; ctx->reg_vz = sz;
  return SVR_OK;
}

int svr_ncc_evaluate(svr_ctx *ctx, int n_eval, const int *target_index, const double *matrices,
                     int64_t *sums6, double *ncc) {
  SVR_ENTER(ctx);
  if (!ctx || n_eval <= 0 || !target_index || !matrices) return SVR_E_ARG;
  NEED(ctx->d_reg_targets && ctx->d_reg_source, "svr_ncc_set_targets / svr_ncc_set_source first");
  // matrices | target indices in, the six moments out; the first allocation holds 256 evaluations (the optimiser calls this
  // ~60 k times per registration pass with growing batch sizes)
  const size_t b_mats = (size_t)n_eval * 16 * sizeof(double), per_eval = 16 * sizeof(double) + sizeof(int) + 6 * sizeof(long long);
  std::vector<long long> h((size_t)n_eval * 6);
  if (int rc = sim_evaluate(ctx, "svr_ncc_evaluate", target_index, n_eval, {{matrices, b_mats}, {target_index, n_eval * sizeof(int)}}, h.data(),
                            h.size() * sizeof(long long), nullptr, 0, 256 * per_eval, [&](unsigned char *d_in, unsigned char *d_out, unsigned char *) {
                              hipLaunchKernelGGL(k_ncc, dim3(n_eval), dim3(256), 0, ctx->stream, ctx->d_reg_targets, ctx->reg_tx, ctx->reg_ty,
                                                 reinterpret_cast<const int *>(d_in + b_mats), reinterpret_cast<const double *>(d_in), ctx->d_reg_source,
                                                 (int)ctx->reg_vx, (int)ctx->reg_vy, (int)ctx->reg_vz, reinterpret_cast<long long *>(d_out));
                            }))
    return rc;
  for (int i = 0; i < n_eval; ++i) {
    const long long *s = &h[6 * (size_t)i];
    if (sums6) for (int k = 0; k < 6; ++k) sums6[6 * (size_t)i + k] = s[k];
    if (ncc) {
      // irtkCrossCorrelationSimilarityMetric::Evaluate (…Metric.h:158-165)
      const double n = (double)s[0], x = (double)s[1], y = (double)s[2], x2 = (double)s[3], y2 = (double)s[4],
                   xy = (double)s[5];
      ncc[i] = n > 0 ? (xy - (x * y) / n) / (sqrt(x2 - x * x / n) * sqrt(y2 - y * y / n)) : 0.0;
    }
  }
  return SVR_OK;
}

}  // extern "C"
