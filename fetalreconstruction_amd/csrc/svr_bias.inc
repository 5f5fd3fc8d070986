// svr_bias.inc -- the bias path's Gaussians through the LDS (option bias_mode 1, the default, takes the NormaliseBias tail here from
// BIAS_LDS_TAIL_MIN voxels on, bias_mode 2 at every size; bias_mode 0 keeps the stencils of svr_small.inc).  Included inside
// svr_hip.hip's anonymous namespace, after svr_small.inc.
//
// Every output keeps the stencils' arithmetic: the recursive weights g0 *= g1; g1 *= g2 in float (computed once per launch
// block instead of once per output), sum = g0 * in[c]; then sum += g_i * in[c + i]; sum += g_i * in[c - i] for i = 1 .. half,
// border repeat, sum / sum_coeff -- and the library is built with -ffp-contract=off, so the results are the stencils' bits.
//
// CorrectBias (RC.cu:1837-1942, k_bias_residual + 4 x k_gauss_conv_slices + k_bias_update): one workgroup per (slice, strip of
// BX columns).  Rows go through the LDS in batches: the residual pair (wb, wr) of the strip plus its halo is computed into a
// window, the horizontal pass of both lands in two [sy][BX] column stores; then the vertical passes read those and update
// the field.  The reference's buffer reuse (RC.cu:1886-1891) is kept: a pass writes only where its result != 0, so the wr
// horizontal pass leaves the wb pass's value where it gives 0, and each vertical pass leaves the residual itself.  The new
// field goes to a second buffer (the strips' halos read the old one), and the caller swaps the two.
//
// NormaliseBias tail (RC.cu:2553-2581, k_div_s + 3 x k_gauss_conv3d + copy + k_div_s + k_divexp): x lines through the LDS
// with the division by the volume weights folded in, y columns through the LDS, z columns through the LDS with the copy,
// the division by maskC and divexp folded in.  Each pass writes unless its result is NaN, as k_gauss_conv3d does.

constexpr size_t BIAS_LDS_TAIL_MIN = size_t(1) << 22;   // bias_mode 1: volumes from 4.2 M voxels take the LDS tail (S8, 20 M: 1.66 vs 4.11 ms)
constexpr int BIAS_HMAX = 255;          // largest half-width of the LDS kernels (sigma / voxel <= 63.75); wider goes to bias_mode 0

struct GaussTable { int half; float sum_coeff; };

// the recurrence of k_gauss_conv_slices / k_gauss_conv3d, written into g[0 .. half]; the same float operations in the same order
__device__ GaussTable gauss_table(float sigma, float dimd, float *g) {
  const float sigma2 = sigma / dimd;
  int klength = 2 * (int)roundf(4 * sigma2) + 1;
  klength -= 1 - klength % 2;
  const int half = (klength - 1) / 2;
  float g0 = (float)(1.0 / (sqrt(2.0 * M_PI) * sigma2));
  float g1 = (float)exp(-0.5 / (sigma2 * sigma2));
  const float g2 = g1 * g1;
  float sum_coeff = g0;
  g[0] = g0;
  for (int i = 1; i <= half; ++i) {
    g0 *= g1;
    g1 *= g2;
    g[i] = g0;
    sum_coeff += 2 * g0;
  }
  return {half, sum_coeff};
}
// the half-width the kernels will find (host side, to size the LDS and pick the path)
inline int gauss_half_host(float sigma, float dimd) {
  const float sigma2 = sigma / dimd;
  int klength = 2 * (int)roundf(4 * sigma2) + 1;
  klength -= 1 - klength % 2;
  return (klength - 1) / 2;
}

// calculateResidual3D_adv RC.cu:1687-1731 as k_bias_residual leaves it in the zeroed wb / wr
__device__ __forceinline__ void bias_residual_at(const float *slices, const float *bias, const float *weights, const float *simweights,
                                                 const float *simslices, float scale, size_t idx, float &wb, float &wr) {
  wb = 0.0f; wr = 0.0f;
  const float s = slices[idx];
  if (s == -1.0f) return;
  float wbo = 0.0f, wro = 0.0f;
  if ((double)simweights[idx] > 0.99) {
    float eb = expf(-bias[idx]);
    float sliceVal = s * (eb * scale);
    wbo = weights[idx] * sliceVal;
    float ss = simslices[idx];
    if (((double)ss > 1.0) && ((double)sliceVal > 1.0)) wro = logf(sliceVal / ss) * wbo;
  }
  if (wbo > 0) { wb = wbo; wr = wro; }
}

// LDS: g[BIAS_HMAX + 1] | hb[sy][bx] | hr[sy][bx] | win_b[rows][W] | win_r[rows][W], W = bx + 2 half, rows = 256 / bx
__global__ __launch_bounds__(256) void k_bias_field_lds(const float *slices, const float *bias, const float *weights,
                                                        const float *simweights, const float *simslices, const float *scales,
                                                        const SliceConst *sc, int sx, int sy, float sigma, int bx, float *bias_out) {
  extern __shared__ float lds[];
  const int sl = blockIdx.y, x0 = blockIdx.x * bx, t = threadIdx.x;
  const size_t base = (size_t)sl * sx * sy;
  float *g = lds, *hb = g + BIAS_HMAX + 1, *hr = hb + sy * bx;
  __shared__ GaussTable gt;
  if (t == 0) gt = gauss_table(sigma, sc[sl].dim[0], g);
  __syncthreads();
  const int half = gt.half, W = bx + 2 * half, rows = 256 / bx;
  const float sum_coeff = gt.sum_coeff, scale = scales[sl];
  float *wbw = hr + sy * bx, *wrw = wbw + rows * W;
  // horizontal passes, `rows` rows at a time: RC.cu:1886 (wb -> buffer) and 1889 (wr -> buffer, which keeps the wb result where 0)
  const int tr = t / bx, tx = t % bx;
  for (int y0 = 0; y0 < sy; y0 += rows) {
    for (int k = t; k < rows * W; k += 256) {
      const int r = k / W, j = k % W, y = y0 + r;
      float b = 0.0f, w = 0.0f;
      if (y < sy) bias_residual_at(slices, bias, weights, simweights, simslices, scale, base + (size_t)y * sx + reflect_(sx, x0 - half + j), b, w);
      wbw[k] = b; wrw[k] = w;
    }
    __syncthreads();
    const int y = y0 + tr;
    if (tr < rows && y < sy) {
      const float *pb = wbw + tr * W + half + tx, *pr = wrw + tr * W + half + tx;
      float sb = g[0] * pb[0], sr = g[0] * pr[0];
      for (int i = 1; i <= half; ++i) {
        const float gi = g[i];
        sb += gi * pb[i];
        sb += gi * pb[-i];
        sr += gi * pr[i];
        sr += gi * pr[-i];
      }
      const float ob = sb / sum_coeff, orr = sr / sum_coeff;
      const float vb = ob != 0 ? ob : 0.0f;              // the buffer was zeroed (RC.cu:1875)
      hb[y * bx + tx] = vb;
      hr[y * bx + tx] = orr != 0 ? orr : vb;
    }
    __syncthreads();
  }
  // vertical passes (RC.cu:1888, 1891: wb / wr keep the residual where the result is 0) and updateBiasField3D_adv RC.cu:1734-1758
  for (int k = t; k < sy * bx; k += 256) {
    const int y = k / bx, c = k % bx, x = x0 + c;
    if (x >= sx) continue;
    float sb = g[0] * hb[y * bx + c], sr = g[0] * hr[y * bx + c];
    for (int i = 1; i <= half; ++i) {
      const float gi = g[i];
      const int a = reflect_(sy, y + i) * bx + c, b = reflect_(sy, y - i) * bx + c;
      sb += gi * hb[a];
      sb += gi * hb[b];
      sr += gi * hr[a];
      sr += gi * hr[b];
    }
    const float ob = sb / sum_coeff, orr = sr / sum_coeff;
    const size_t idx = base + (size_t)y * sx + x;
    float b0, r0;
    bias_residual_at(slices, bias, weights, simweights, simslices, scale, idx, b0, r0);
    const float wbv = ob != 0 ? ob : b0, wrv = orr != 0 ? orr : r0;
    float v = bias[idx];
    if (slices[idx] != -1.0f && wbv > 0) v = v + wrv / wbv;
    bias_out[idx] = v;
  }
}
// LDS bytes of k_bias_field_lds for a strip of bx columns
inline size_t bias_field_lds_bytes(int sy, int bx, int half) {
  return sizeof(float) * ((size_t)BIAS_HMAX + 1 + 2 * (size_t)sy * bx + 2 * (size_t)(256 / bx) * (bx + 2 * half));
}

// x pass: `rows` lines of vx per workgroup.  bv <- bv / volw (divS RC.cu:2553-2556) in place, out <- X(bv) unless NaN, else 0
// (the zeroed mbuf).  LDS: g[BIAS_HMAX + 1] | line[rows][vx]
__global__ __launch_bounds__(256) void k_gauss3d_x_lds(float *bv, const float *volw, float *out, float sigma, float dimd, int vx, int nlines,
                                                       int rows) {
  extern __shared__ float lds[];
  float *g = lds, *line = g + BIAS_HMAX + 1;
  __shared__ GaussTable gt;
  if (threadIdx.x == 0) gt = gauss_table(sigma, dimd, g);
  const size_t l0 = (size_t)blockIdx.x * rows;
  const int nl = (int)min((size_t)rows, nlines - l0);
  for (int k = threadIdx.x; k < nl * vx; k += 256) {
    const size_t i = l0 * vx + k;
    const float d = volw[i];
    const float v = (d != 0) ? bv[i] / d : 0;
    bv[i] = v;
    line[k] = v;
  }
  __syncthreads();
  const int half = gt.half;
  for (int k = threadIdx.x; k < nl * vx; k += 256) {
    const int r = k / vx, x = k % vx;
    const float *p = line + r * vx;
    float sum = g[0] * p[x];
    for (int i = 1; i <= half; ++i) {
      sum += g[i] * p[reflect_(vx, x + i)];
      sum += g[i] * p[reflect_(vx, x - i)];
    }
    const float o = sum / gt.sum_coeff;
    out[l0 * vx + k] = (o == o) ? o : 0.0f;
  }
}

// y pass (dir 1) or z pass (dir 2): a workgroup takes a strip of bx consecutive x on one z plane (y) or one y row (z) and every
// position along the axis.  y: out <- Y(in) unless NaN (out keeps the divided value otherwise).  z (LAST): the stencil's
// result m = Z(in) unless NaN, else the x pass's value (mbuf); then bv <- maskC != 0 ? m / maskC : 0 (RC.cu:2575-2577) and
// recon <- recon / exp(-bv) where recon != -1 (divexp RC.cu:2579-2581).  LDS: g[BIAS_HMAX + 1] | col[n][bx]
template <bool LAST>
__global__ __launch_bounds__(256) void k_gauss3d_col_lds(const float *in, float *out, const float *xpass, const float *maskC, float *recon,
                                                         float sigma, float dimd, int vx, int vy, int vz, int bx) {
  extern __shared__ float lds[];
  float *g = lds, *col = g + BIAS_HMAX + 1;
  __shared__ GaussTable gt;
  if (threadIdx.x == 0) gt = gauss_table(sigma, dimd, g);
  const int x0 = blockIdx.x * bx, other = blockIdx.y;               // other = z (y pass) or y (z pass)
  const int n = LAST ? vz : vy;
  const size_t stride = LAST ? (size_t)vx * vy : (size_t)vx;
  const size_t base = LAST ? (size_t)other * vx + x0 : (size_t)other * vx * vy + x0;
  const int w = min(bx, vx - x0);
  for (int k = threadIdx.x; k < n * bx; k += 256) {
    const int p = k / bx, c = k % bx;
    if (c < w) col[k] = in[base + p * stride + c];
  }
  __syncthreads();
  const int half = gt.half;
  for (int k = threadIdx.x; k < n * bx; k += 256) {
    const int p = k / bx, c = k % bx;
    if (c >= w) continue;
    float sum = g[0] * col[k];
    for (int i = 1; i <= half; ++i) {
      sum += g[i] * col[reflect_(n, p + i) * bx + c];
      sum += g[i] * col[reflect_(n, p - i) * bx + c];
    }
    const float o = sum / gt.sum_coeff;
    const size_t idx = base + p * stride + c;
    if (!LAST) {
      if (o == o) out[idx] = o;
    } else {
      const float m = (o == o) ? o : xpass[idx];
      const float d = maskC[idx];
      const float b = (d != 0) ? m / d : 0;
      out[idx] = b;
      const float a = recon[idx];
      if (a != -1.0f) recon[idx] = a / expf(-b);
    }
  }
}
