// svr_ssim.inc -- a windowed structural similarity between every slice and its simulation (svr_slice_ssim), included by svr_hip.hip.
//
// Not a step of the reference: what the command line's --structural judges a slice by (DESIGN 9f).  The global correlation of the
// slice report (svr_quality.inc) cannot tell a rim slice from a displaced one; the mean of a local SSIM over the M-step's pixels can.
//
// Per pixel p, with qual_pixel's operands and set V (svr_quality.inc):
//   x = bias ? s * expf(-bias) * scale : s * scale   (float),   y = simslices,   p in V iff s != -1 and simweight > 0.99
// window = the (2R+1)^2 box around p clipped to the sx x sy grid; over its pixels in V, in double from the float operands:
//   m, Sx, Sy, Sxx, Syy, Sxy.   p is counted iff p in V and m >= ((2R+1)^2 + 1) / 2.   Then, in double and as written:
//   mx = Sx/m, my = Sy/m, vx = Sxx/m - mx*mx, vy = Syy/m - my*my, cxy = Sxy/m - mx*my
//   ssim = (((2*mx)*my + c1) * (2*cxy + c2)) / (((mx*mx + my*my) + c1) * ((vx + vy) + c2))
//
//   k_slice_ssim         grid = ns x tiles workgroups of 256, a tile = SSIM_T x SSIM_T pixels, one per thread.  The workgroup stages
//                        the tile and its R-wide halo once -- x, y (0 outside V) and the flag -- then forms the window sums separably
//                        through the LDS: thread (row of the staged region, column of the tile) adds its 2R+1 staged neighbours left
//                        to right, thread (pixel) adds the 2R+1 row sums above and below it top to bottom.  A pixel outside V adds
//                        +0.0, which changes no sum.  The tile's {n, S ssim}: a lane's value (0 when not counted), the xor tree
//                        (offsets 32 .. 1), the four wavefronts in wave order through the LDS.
//   k_slice_ssim_finish  thread (slice, k) adds the slice's tiles in tile order.
// No atomics; lane, fold, wave order and tile order follow from (ns, sx, sy, R) alone: the same bits on every call.  The loads are
// scalar: a staged row starts R pixels left of a tile, at no alignment worth a vector load, and the pass is bound by its double adds
// (5 (2R+1) per row sum and per pixel), not by the 3-4 floats per pixel it reads.  LDS: 2 x 30 x 31 floats, 30 x 32 flags, 5 x 30 x 16
// doubles, 30 x 16 counts, 4 x 2 doubles: 29 600 bytes by the compiler's report, at every R (sized for R = 7).  Scratch is the call's
// own and freed before it returns, like svr_slice_quality's; nothing is cached, so the invalidation map has no line for it.  Units are
// slices or patches alike.

#define SSIM_T 16                          // tile edge: one pixel per thread of a 256-thread workgroup
#define SSIM_H (SSIM_T + 2 * SVR_SSIM_MAX_RADIUS)   // the staged region's edge at the largest radius

namespace {

// the last step, kept apart so that nothing around it can be folded into it
__device__ __forceinline__ double ssim_value(double m, double sx, double sy, double sxx, double syy, double sxy, double c1, double c2) {
#pragma clang fp contract(off)
#pragma clang fp reassociate(off)
  const double mx = sx / m, my = sy / m;
  const double vx = sxx / m - mx * mx, vy = syy / m - my * my, cxy = sxy / m - mx * my;
  const double num = ((2.0 * mx) * my + c1) * (2.0 * cxy + c2);
  const double den = ((mx * mx + my * my) + c1) * ((vx + vy) + c2);
  return num / den;
}

template <bool BIAS>
__global__ __launch_bounds__(256) void k_slice_ssim(const float *__restrict__ slices, const float *__restrict__ simslices,
                                                    const float *__restrict__ simweights, const float *__restrict__ scales,
                                                    const float *__restrict__ bias, int sx, int sy, int tiles_x, int tiles, int R,
                                                    double c1, double c2, double *__restrict__ partial, float *__restrict__ map) {
  __shared__ float s_x[SSIM_H][SSIM_H + 1], s_y[SSIM_H][SSIM_H + 1];
  __shared__ unsigned char s_v[SSIM_H][SSIM_H + 2];
  __shared__ double r_s[5][SSIM_H][SSIM_T];
  __shared__ int r_m[SSIM_H][SSIM_T];
  __shared__ double w_s[4][2];
  const int sl = (int)(blockIdx.x / (unsigned)tiles), tile = (int)(blockIdx.x - (unsigned)sl * (unsigned)tiles);
  const int tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
  const int x0 = txi * SSIM_T - R, y0 = tyi * SSIM_T - R, hw = SSIM_T + 2 * R, win = 2 * R + 1;
  const size_t base = (size_t)sl * ((size_t)sx * sy);
  const float scale = scales[sl];
  const int t = threadIdx.x;
  for (int i = t; i < hw * hw; i += 256) {                   // the tile and its halo, once
    const int hy = i / hw, hx = i - hy * hw, gx = x0 + hx, gy = y0 + hy;
    float xv = 0.0f, yv = 0.0f;
    unsigned char v = 0;
    if (gx >= 0 && gx < sx && gy >= 0 && gy < sy) {
      const size_t g = base + (size_t)gy * sx + gx;
      const float s = slices[g];
      if (s != -1.0f) {
        const float sw = simweights[g];
        if (BIAS ? (double)sw > 0.99 : sw > 0.99f) {         // qual_pixel's set
          xv = BIAS ? s * expf(-bias[g]) * scale : s * scale;
          yv = simslices[g];
          v = 1;
        }
      }
    }
    s_x[hy][hx] = xv; s_y[hy][hx] = yv; s_v[hy][hx] = v;
  }
  __syncthreads();
  for (int i = t; i < hw * SSIM_T; i += 256) {               // row sums, left to right
    const int hy = i / SSIM_T, cx = i - hy * SSIM_T;
    int m = 0;
    double ax = 0.0, ay = 0.0, axx = 0.0, ayy = 0.0, axy = 0.0;
    for (int k = 0; k < win; ++k) {
      const double dx = (double)s_x[hy][cx + k], dy = (double)s_y[hy][cx + k];
      m += s_v[hy][cx + k];
      ax += dx; ay += dy; axx += dx * dx; ayy += dy * dy; axy += dx * dy;
    }
    r_m[hy][cx] = m;
    r_s[0][hy][cx] = ax; r_s[1][hy][cx] = ay; r_s[2][hy][cx] = axx; r_s[3][hy][cx] = ayy; r_s[4][hy][cx] = axy;
  }
  __syncthreads();
  const int cy = t / SSIM_T, cx = t - cy * SSIM_T, px = txi * SSIM_T + cx, py = tyi * SSIM_T + cy;
  double cnt = 0.0, val = 0.0;
  if (px < sx && py < sy) {
    float out = __builtin_nanf("");
    if (s_v[cy + R][cx + R]) {
      int m = 0;
      double ax = 0.0, ay = 0.0, axx = 0.0, ayy = 0.0, axy = 0.0;
      for (int k = 0; k < win; ++k) {                        // column sums, top to bottom
        m += r_m[cy + k][cx];
        ax += r_s[0][cy + k][cx]; ay += r_s[1][cy + k][cx]; axx += r_s[2][cy + k][cx]; ayy += r_s[3][cy + k][cx]; axy += r_s[4][cy + k][cx];
      }
      if (m >= (win * win + 1) / 2) {
        val = ssim_value((double)m, ax, ay, axx, ayy, axy, c1, c2);
        cnt = 1.0;
        out = (float)val;
      }
    }
    if (map) map[base + (size_t)py * sx + px] = out;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o, 64);
    val += __shfl_xor(val, o, 64);
  }
  const int w = t >> 6;
  if ((t & 63) == 0) { w_s[w][0] = cnt; w_s[w][1] = val; }
  __syncthreads();
  if (t < 2) partial[(size_t)blockIdx.x * 2 + t] = ((w_s[0][t] + w_s[1][t]) + w_s[2][t]) + w_s[3][t];   // wave order
}

__global__ void k_slice_ssim_finish(const double *__restrict__ partial, int ns, int tiles, double *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ns * 2) return;
  const int sl = i >> 1, k = i & 1;
  double x = partial[((size_t)sl * tiles) * 2 + k];
  for (int c = 1; c < tiles; ++c) x += partial[((size_t)sl * tiles + c) * 2 + k];
  out[i] = x;
}

int slice_ssim_run(svr_ctx *ctx, int R, double c1, double c2, double *sums, float *map) {
  const int sx = (int)ctx->sx, sy = (int)ctx->sy;
  const int tiles_x = (sx + SSIM_T - 1) / SSIM_T, tiles_y = (sy + SSIM_T - 1) / SSIM_T;
  const size_t tiles = (size_t)tiles_x * tiles_y, blocks = (size_t)ctx->ns * tiles, nout = (size_t)ctx->ns * 2;
  if (tiles >= (1ull << 31) || blocks >= (1ull << 31) || nout >= (1ull << 31)) return fail(ctx, SVR_E_ARG, "svr_slice_ssim: too many slices");
  const float *bias = ctx->disable_bias ? (const float *)nullptr : ctx->d_bias;
  DevBuf<double> d_partial, d_sums;                          // nothing is kept beyond the call
  DevBuf<float> d_map;
  HIPCHK(d_partial.reserve(blocks * 2));
  HIPCHK(d_sums.reserve(nout));
  if (map) HIPCHK(d_map.reserve(ctx->np));
  hipLaunchKernelGGL(bias ? k_slice_ssim<true> : k_slice_ssim<false>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, ctx->d_slices,
                     ctx->d_simslices, ctx->d_simweights, ctx->d_scales_host_copy, bias, sx, sy, tiles_x, (int)tiles, R, c1, c2,
                     d_partial.get(), d_map.get());
  KCHK("k_slice_ssim");
  hipLaunchKernelGGL(k_slice_ssim_finish, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, ctx->stream, d_partial.get(), (int)ctx->ns,
                     (int)tiles, d_sums.get());
  KCHK("k_slice_ssim_finish");
  HIPCHK(hipMemcpyAsync(sums, d_sums.get(), nout * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (map) HIPCHK(hipMemcpyAsync(map, d_map.get(), ctx->np * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

}  // namespace

extern "C" {

int svr_slice_ssim(svr_ctx *ctx, int radius, double c1, double c2, double *sums, float *map_or_null) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  if (!sums) return fail(ctx, SVR_E_ARG, "svr_slice_ssim: no array for the sums");
  if (radius < 1 || radius > SVR_SSIM_MAX_RADIUS) return fail(ctx, SVR_E_ARG, "svr_slice_ssim: the radius must be 1 .. 7");
  if (!(c1 >= 0.0 && c2 >= 0.0) || std::isinf(c1) || std::isinf(c2))
    return fail(ctx, SVR_E_ARG, "svr_slice_ssim: c1 and c2 must be finite and not negative");
  NEED(ctx->np > 0 && ctx->have_slices, "slices not filled");
  NEED(ctx->have_scales, "scale vector not set");
  NEED(ctx->have_sim, "no simulated slices (svr_simulate_slices first)");
  int r = ensure_bias_buffers(ctx);                          // (as every compute call: a bias path switched on before the slice grid existed)
  if (r) return r;
  return slice_ssim_run(ctx, radius, c1, c2, sums, map_or_null);
}

}  // extern "C"
