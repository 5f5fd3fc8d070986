// svr_motion.inc -- the motion score of a stack (the reference's --useAutoTemplate, "matrix rank method":
// stackMotionEstimator.cpp:67-164), included by svr_hip.hip.
//
// The reference asks CULA's sgesvd for the singular values of the M x N matrix A whose columns are N slices of M pixels
// (no vectors: jobu = jobvt = 'N').  The singular values of A are the square roots of the eigenvalues of its N x N Gram
// matrix G = A^T A, so nothing of an SVD library is needed:
//   k_gram      G's upper triangle from the float slices, accumulated in double by v_mfma_f64_16x16x4_f64.  The pixels are
//               split into chunks (grid x), G into pairs (I <= J) of 64-column bands (grid y).  A workgroup walks its chunk
//               in steps of 64 pixels: the two bands' 64 x 64 floats go into the LDS, wavefront w multiplies tile row w of
//               band I with the (up to) four tiles of band J -- one LDS read per operand, one MFMA per tile and 4 pixels --
//               and writes its 16 x 16 double tiles into the chunk's partial matrix (not those below G's diagonal).
//   k_gram_sum  G[i][j] = the chunks' partial sums in chunk order, mirrored into the lower triangle.
// No atomics: the same bits from run to run.  The number of chunks is bounded so that the partial matrices stay within
// MOT_PARTIAL_BYTES whatever M is.  With N <= 64 the slices are read from memory once; a wider G reads a band once per pair it
// takes part in (ceil(N / 64) + 1 times at most), which the L2 / Infinity Cache serve: the window is a few tens of MB at most.
// The eigenvalues are cyclic Jacobi in double on the host side of the library (N is a few hundred at most), the rest of the
// score -- sqrt, the reference's rank loop -- follows in double.
//
// Lane maps of v_mfma_f64_16x16x4_f64 (D = A B + C, A 16 x 4, B 4 x 16): lane l holds A[l & 15][l >> 4] and
// B[l >> 4][l & 15] in one double each; register r of its four results is D[(l >> 4) + 4 r][l & 15] (not the f32 forms'
// row 4 (l >> 4) + r).  tests/test_auto_template_gpu.py pins them with integer slices whose Gram matrix is exact.

#include <functional>

#define MOT_T 64                          // columns of a band = pixels of an LDS step (4 x 4 MFMA tiles)
#define MOT_LD 68                         // floats per column in the LDS: lanes (column l & 15, pixel l >> 4) hit 64 different banks
#define MOT_MAX_CHUNKS 128
#define MOT_PARTIAL_BYTES ((size_t)4 << 20)

namespace {

typedef double mot_f64x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void k_gram(const float *__restrict__ x, int m, int n, int chunk_len, int bands, double *__restrict__ partial) {
  __shared__ float sa[MOT_T * MOT_LD], sb[MOT_T * MOT_LD];
  int bi = 0, bj = (int)blockIdx.y;                                 // pair blockIdx.y of the upper triangle, row after row
  while (bj >= bands - bi) { bj -= bands - bi; ++bi; }
  bj += bi;
  const bool diag = bi == bj;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int p_begin = (int)blockIdx.x * chunk_len, p_end = min(m, p_begin + chunk_len);
  const int lp = threadIdx.x & 63, lc = threadIdx.x >> 6;           // the loads: 64 consecutive pixels of 4 columns per pass
  const float *tb = diag ? sa : sb;
  const int oa = (w * 16 + (lane & 15)) * MOT_LD + (lane >> 4), ob = (lane & 15) * MOT_LD + (lane >> 4);
  mot_f64x4 acc[4];
  for (int t = 0; t < 4; ++t) acc[t] = mot_f64x4{0.0, 0.0, 0.0, 0.0};
  for (int p0 = p_begin; p0 < p_end; p0 += MOT_T) {
    const int p = p0 + lp;
#pragma unroll 4
    for (int c = lc; c < MOT_T; c += 4) {
      const int ca = bi * MOT_T + c, cb = bj * MOT_T + c;
      sa[c * MOT_LD + lp] = (ca < n && p < p_end) ? x[(size_t)ca * m + p] : 0.0f;
      if (!diag) sb[c * MOT_LD + lp] = (cb < n && p < p_end) ? x[(size_t)cb * m + p] : 0.0f;
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < MOT_T; k += 4) {
      const double a = (double)sa[oa + k];
#pragma unroll
      for (int t = 0; t < 4; ++t)                                   // (a diagonal band's tiles below the diagonal too: straight-line code, dropped at the store)
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, (double)tb[ob + t * 16 * MOT_LD + k], acc[t], 0, 0, 0);
    }
    __syncthreads();
  }
  const size_t np = (size_t)bands * MOT_T;
  double *out = partial + (size_t)blockIdx.x * np * np;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (diag && t < w) continue;                                    // below the diagonal: never read
#pragma unroll
    for (int r = 0; r < 4; ++r)
      out[((size_t)bi * MOT_T + w * 16 + (lane >> 4) + 4 * r) * np + (size_t)bj * MOT_T + t * 16 + (lane & 15)] = acc[t][r];
  }
}

__global__ void k_gram_sum(const double *__restrict__ partial, int n, int np, int chunks, double *__restrict__ g) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (j >= n || j < i) return;
  double s = 0.0;
  for (int c = 0; c < chunks; ++c) s += partial[((size_t)c * np + i) * np + j];
  g[(size_t)i * n + j] = g[(size_t)j * n + i] = s;
}

// eigenvalues of the symmetric n x n matrix a (destroyed) by cyclic Jacobi; false: no convergence
bool jacobi_eigenvalues(std::vector<double> &a, int n, std::vector<double> &ev) {
  double trace = 0.0;
  for (int i = 0; i < n; ++i) trace += fabs(a[(size_t)i * n + i]);
  // an off-diagonal entry this small moves no eigenvalue by more than n x floor: far below the rounding of G itself (2^-53 trace)
  const double floor_abs = 1e-22 * trace;
  bool done = n < 2;
  for (int sweep = 0; sweep < 64 && !done; ++sweep) {
    done = true;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = a[(size_t)p * n + q];
        if (fabs(apq) <= floor_abs) continue;
        done = false;
        const double app = a[(size_t)p * n + p], aqq = a[(size_t)q * n + q];
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < n; ++k) {
          if (k == p || k == q) continue;
          const double akp = a[(size_t)k * n + p], akq = a[(size_t)k * n + q];
          a[(size_t)k * n + p] = a[(size_t)p * n + k] = c * akp - s * akq;
          a[(size_t)k * n + q] = a[(size_t)q * n + k] = s * akp + c * akq;
        }
        a[(size_t)p * n + p] = app - t * apq;
        a[(size_t)q * n + q] = aqq + t * apq;
        a[(size_t)p * n + q] = a[(size_t)q * n + p] = 0.0;
      }
  }
  ev.resize(n);
  for (int i = 0; i < n; ++i) ev[i] = a[(size_t)i * n + i];
  return done;
}

int motion_gram(svr_ctx *ctx, const float *slices, int m, int n, std::vector<double> &g) {
  const int bands = (n + MOT_T - 1) / MOT_T, pairs = bands * (bands + 1) / 2;
  const size_t np = (size_t)bands * MOT_T, steps = ((size_t)m + MOT_T - 1) / MOT_T;
  const size_t chunks_fit = std::max<size_t>(1, MOT_PARTIAL_BYTES / (np * np * sizeof(double)));
  const size_t want = std::min<size_t>(std::min<size_t>(steps, MOT_MAX_CHUNKS), chunks_fit);
  const int chunk_len = (int)((steps + want - 1) / want) * MOT_T;
  const int chunks = (int)(((size_t)m + chunk_len - 1) / chunk_len);
  if (pairs > 65535) return fail(ctx, SVR_E_ARG, "svr_stack_motion: too many slices");
  // the slices, the chunks' partial Gram matrices and their sum: nothing is kept beyond the call (the coefficient table sizes itself by the
  // memory that is free)
  DevBuf<float> d_x;
  DevBuf<double> d_partial, d_g;
  HIPCHK(d_x.reserve((size_t)m * n));
  HIPCHK(d_partial.reserve((size_t)chunks * np * np));
  HIPCHK(d_g.reserve((size_t)n * n));
  HIPCHK(hipMemcpyAsync(d_x, slices, (size_t)m * n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_gram, dim3(chunks, pairs), dim3(256), 0, ctx->stream, d_x, m, n, chunk_len, bands, d_partial);
  KCHK("k_gram");
  hipLaunchKernelGGL(k_gram_sum, dim3((n + 63) / 64, n), dim3(64), 0, ctx->stream, d_partial, n, (int)np, chunks, d_g);
  KCHK("k_gram_sum");
  g.resize((size_t)n * n);
  HIPCHK(hipMemcpyAsync(g.data(), d_g, g.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

}  // namespace

extern "C" {

int svr_stack_motion(svr_ctx *ctx, const float *slices, int m, int n, double *singular_values_or_null, double *et, int *r_min, double *score) {
  SVR_ENTER(ctx);
  if (!ctx || !et || !r_min || !score) return SVR_E_ARG;
  if (m < 1 || n < 1) return fail(ctx, SVR_E_ARG, "svr_stack_motion: no slice in the window (a stack of fewer than 3 slices has no third)");
  if (!slices) return fail(ctx, SVR_E_ARG, "svr_stack_motion: no slices");
  if (n > m) return fail(ctx, SVR_E_ARG, "svr_stack_motion: more slices than pixels per slice (" + std::to_string(n) + " > " + std::to_string(m) + ")");
  if (n > 65535) return fail(ctx, SVR_E_ARG, "svr_stack_motion: too many slices");
  std::vector<double> g, ev;
  const int rc = motion_gram(ctx, slices, m, n, g);
  if (rc) return rc;
  if (!jacobi_eigenvalues(g, n, ev)) return fail(ctx, SVR_E_STATE, "svr_stack_motion: the eigenvalue iteration did not converge");
  std::sort(ev.begin(), ev.end(), std::greater<double>());
  std::vector<double> s(n);
  for (int i = 0; i < n; ++i) s[i] = sqrt(std::max(ev[i], 0.0));          // (round-off below zero)
  // stackMotionEstimator.cpp:124-163.  r stops at num_ev - 1: the sum never holds every singular value
  double norm_all = 0.0;
  for (int i = 0; i < n; ++i) norm_all += s[i] * s[i];
  norm_all = sqrt(norm_all);
  if (!(norm_all > 0.0)) return fail(ctx, SVR_E_ARG, "svr_stack_motion: the window is zero everywhere");
  double e_t = 0.0;
  int r_m = -1;
  for (int r = 0; r < n; ++r) {
    double norm_a = 0.0;
    for (int i = 0; i < r; ++i) norm_a += s[i] * s[i];
    const double error = sqrt(norm_a) / norm_all;
    if (error < 0.99) { e_t = error; r_m = r; }
  }
  if (singular_values_or_null) memcpy(singular_values_or_null, s.data(), (size_t)n * sizeof(double));
  *et = e_t; *r_min = r_m; *score = e_t * r_m;
  return SVR_OK;
}

}  // extern "C"
