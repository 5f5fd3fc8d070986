// svr_fit.inc -- the mono-exponential fit S(x) = A exp(-R x) over K co-registered volumes (svr_monoexp_fit), included by svr_hip.hip.
//
// What --echoStacks of the command line ends with: K motion-corrected echoes (x = TE: T2*, T2) or diffusion weightings (x = b: ADC) on the
// reconstruction grid, one parameter pair per voxel.  Not a step of the reconstruction and no reference equivalent; it needs a context for its
// device and stream, and nothing of a geometry.
//
// Per voxel, over the samples k = 0 .. K-1 in that order, everything in double (DESIGN 9e has the same lines):
//     usable_k = C_k finite and C_k > floor;   count = the number of usable samples;   count < 2 -> rate = amplitude = rmse = 0
//     y = ln C_k, w = C_k^2:   Sw, Swx, Swxx, Swy, Swxy   (the log-linear fit weighted by the squared signal, which undoes the log's noise gain)
//     D = Sw Swxx - Swx^2;   D not positive -> 0
//     R = -(Sw Swxy - Swx Swy) / D,   A = exp((Swxx Swy - Swx Swxy) / D);   not finite -> 0
//     iterations > 0: that many Gauss-Newton steps on C_k - a exp(-r x_k) from (A, R): J1 = e_k = exp(-r x_k), J2 = -a x_k e_k, the 2 x 2 normal
//       equations solved in closed form; stop when det <= 1e-30 a11 a22; back to (A, R) when a parameter stops being finite; the refined pair
//       is kept only if its sum of squares is not above (A, R)'s
//     rmse = sqrt(sum (C_k - A exp(-R x_k))^2 / count) for the pair returned
//     rounded to float once; an output that is not finite as a float -> rate = amplitude = rmse = 0 (count stays)
//
// k_monoexp_fit: one lane per voxel.  The K values of a voxel lie in K planes of a [K][stride] array, so a wavefront's 64 loads are 256
// contiguous bytes for every k.  A lane does not keep its samples: every pass (the sums, each Gauss-Newton step, the sums of squares) loads
// them again -- K <= 16 floats that stay in the cache -- which keeps the loop bounds compile-time (16, guarded by k < K) without an indexed
// register array.  x comes with the kernel arguments.  No LDS, no atomics, plain stores.  Blocks of 256: the kernel is element-wise and f64
// transcendental-bound, registers are far from binding, and nobody has measured it.
//
// The host cuts [0, n) into chunks of at most fit_chunk voxels (svr_set_option "fit_chunk", default 1 << 20), uploads a chunk's K rows,
// launches and downloads the wanted outputs.  The buffers are locals of the call, freed before it returns: by the time a run fits, the
// coefficient table has taken the memory that was free.  A chunk of 2^20 voxels costs 84 MB at K = 16 with four outputs (20 float planes).

namespace {

struct FitX { double x[16]; };

__device__ __forceinline__ bool fit_usable(float c, float floor) { return isfinite(c) && c > floor; }

// sum of squares of C_k - a exp(-r x_k) over the usable samples
__device__ __forceinline__ double fit_sum_squares(const float *__restrict__ in, size_t stride, size_t i, int K, const FitX &xs, float floor, double a, double r) {
  double ss = 0.0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    if (k >= K) break;
    const float c = in[(size_t)k * stride + i];
    if (!fit_usable(c, floor)) continue;
    const double d = (double)c - a * exp(-r * xs.x[k]);
    ss += d * d;
  }
  return ss;
}

__global__ __launch_bounds__(256) void k_monoexp_fit(const float *__restrict__ in, size_t stride, size_t len, int K, FitX xs, int iterations, float floor,
                                                     float *__restrict__ rate, float *__restrict__ amplitude, float *__restrict__ rmse,
                                                     float *__restrict__ count) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= len) return;
  int cnt = 0;
  double sw = 0.0, swx = 0.0, swxx = 0.0, swy = 0.0, swxy = 0.0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    if (k >= K) break;
    const float cf = in[(size_t)k * stride + i];
    if (!fit_usable(cf, floor)) continue;
    const double c = (double)cf, x = xs.x[k];
    const double y = log(c), w = c * c, wx = w * x;
    ++cnt;
    sw += w; swx += wx; swxx += wx * x; swy += w * y; swxy += wx * y;
  }
  float o_rate = 0.0f, o_amp = 0.0f, o_rmse = 0.0f;
  const double D = sw * swxx - swx * swx;
  if (cnt >= 2 && D > 0.0) {
    double R = -(sw * swxy - swx * swy) / D;
    double A = exp((swxx * swy - swx * swxy) / D);
    if (isfinite(R) && isfinite(A)) {
      if (iterations > 0) {
        double a = A, r = R;
        for (int it = 0; it < iterations; ++it) {
          double a11 = 0.0, a12 = 0.0, a22 = 0.0, g1 = 0.0, g2 = 0.0;
#pragma unroll
          for (int k = 0; k < 16; ++k) {
            if (k >= K) break;
            const float cf = in[(size_t)k * stride + i];
            if (!fit_usable(cf, floor)) continue;
            const double x = xs.x[k], e = exp(-r * x);
            const double j1 = e, j2 = -a * x * e, res = (double)cf - a * e;
            a11 += j1 * j1; a12 += j1 * j2; a22 += j2 * j2; g1 += j1 * res; g2 += j2 * res;
          }
          const double det = a11 * a22 - a12 * a12;
          if (!(det > 1e-30 * a11 * a22)) break;
          a = a + (a22 * g1 - a12 * g2) / det;
          r = r + (a11 * g2 - a12 * g1) / det;
          if (!(isfinite(a) && isfinite(r))) { a = A; r = R; break; }
        }
        if (fit_sum_squares(in, stride, i, K, xs, floor, a, r) <= fit_sum_squares(in, stride, i, K, xs, floor, A, R)) { A = a; R = r; }
      }
      const double ss = fit_sum_squares(in, stride, i, K, xs, floor, A, R);
      const float fr = (float)R, fa = (float)A, fe = (float)sqrt(ss / (double)cnt);
      if (isfinite(fr) && isfinite(fa) && isfinite(fe)) { o_rate = fr; o_amp = fa; o_rmse = fe; }
    }
  }
  if (rate) rate[i] = o_rate;
  if (amplitude) amplitude[i] = o_amp;
  if (rmse) rmse[i] = o_rmse;
  if (count) count[i] = (float)cnt;
}

}  // namespace

extern "C" int svr_monoexp_fit(svr_ctx *ctx, int K, const double *x, const float *vols, size_t n, int iterations, float floor, float *rate,
                               float *amplitude, float *rmse, float *count) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  if (!x || !vols) return fail(ctx, SVR_E_ARG, "svr_monoexp_fit: no abscissae or no volumes");
  if (K < 2 || K > 16) return fail(ctx, SVR_E_ARG, "svr_monoexp_fit: 2 .. 16 volumes expected");
  for (int k = 0; k < K; ++k) {
    if (!std::isfinite(x[k])) return fail(ctx, SVR_E_ARG, "svr_monoexp_fit: an abscissa is not finite");
    for (int j = 0; j < k; ++j)
      if (x[j] == x[k]) return fail(ctx, SVR_E_ARG, "svr_monoexp_fit: two volumes share an abscissa (a duplicate x)");
  }
  if (iterations < 0 || iterations > 50) return fail(ctx, SVR_E_ARG, "svr_monoexp_fit: iterations must be 0 .. 50");
  if (!(std::isfinite(floor) && floor >= 0.0f)) return fail(ctx, SVR_E_ARG, "svr_monoexp_fit: floor must be finite and not negative");
  if (!n || (!rate && !amplitude && !rmse && !count)) return SVR_OK;
  FitX xs;
  for (int k = 0; k < 16; ++k) xs.x[k] = k < K ? x[k] : 0.0;
  const size_t cap = std::min(n, (size_t)ctx->fit_chunk);
  // the call's memory: K input planes and a plane per wanted output.  84 MB for a chunk of 2^20 voxels at K = 16 with four outputs -- small
  // enough to find room after the coefficient table has sized itself by the free memory, and gone when the call returns
  DevBuf<float> d_in, d_out[4];
  float *host[4] = {rate, amplitude, rmse, count};
  HIPCHK(d_in.reserve((size_t)K * cap));
  for (int q = 0; q < 4; ++q)
    if (host[q]) HIPCHK(d_out[q].reserve(cap));
  for (size_t off = 0; off < n; off += cap) {
    const size_t len = std::min(cap, n - off);
    for (int k = 0; k < K; ++k)
      HIPCHK(hipMemcpyAsync(d_in.get() + (size_t)k * cap, vols + (size_t)k * n + off, len * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_monoexp_fit, dim3(nblk(len)), dim3(256), 0, ctx->stream, d_in.get(), cap, len, K, xs, iterations, floor, d_out[0].get(),
                       d_out[1].get(), d_out[2].get(), d_out[3].get());
    KCHK("k_monoexp_fit");
    for (int q = 0; q < 4; ++q)
      if (host[q]) HIPCHK(hipMemcpyAsync(host[q] + off, d_out[q].get(), len * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));              // the next chunk's upload overwrites d_in
  }
  return SVR_OK;
}
