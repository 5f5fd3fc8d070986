// svr_seed.inc -- a volume on any grid brought onto the reconstruction grid (svr_resample_to_reconstruction), included by svr_hip.hip.
//
// The command line's --referenceVolume: a previous reconstruction, one at another resolution or an atlas in the template's space
// becomes the volume the first outer iteration registers against.  The reference reads such a file (reconstruction.cc:253-258), lets
// iteration 0 register (:826) and, outside its T1 experiment, never hands the voxels to the registration; here they take effect.
// Voxel size, field of view, axis order and oblique axes may all differ: the caller composes
//   M = source world-to-image x reconstruction image-to-world      (double, rows 0..2, row-major)
// and target voxel (i, j, k) reads the source at p = M (i, j, k, 1), evaluated in double, left to right.
//
// Per target voxel, with base = floor(p), t = p - base and the eight neighbours base + (dx, dy, dz), x fastest:
//   w = (dx ? tx : 1 - tx) * (dy ? ty : 1 - ty) * (dz ? tz : 1 - tz)              (double)
//   a neighbour takes part if it lies inside the source grid and its value is > padding
//   W = sum w, A = sum w * value  (double, in that order)   ->   W >= 0.5 ? (float)(A / W) : padding
// which is the idea of irtkResamplingWithPadding: background (a previous output of this program holds -1 outside its mask) neither
// bleeds into the rim nor counts as data, and a voxel with less than half of its weight on data is background itself.  Where the
// context's mask is 0 the result is -1, as svr_mask_volume leaves it; without a mask every voxel counts as inside.
//
// Statistics over the valid voxels (inside the mask, W >= 0.5), v = the rounded float result held in double:
//   {n, sum v, sum v^2, min v, max v};   n = 0: sums 0, min = +infinity, max = -infinity.
//
//   k_seed_resample   SEED blocks of 256 threads, thread = target voxel, x fastest, grid-stride.  A lane adds its voxels in index order,
//                     the wavefront folds the five values with a fixed xor tree (offsets 32 .. 1), lane 0 of each wavefront puts them
//                     into the LDS and five threads fold the four wavefronts in wave order and store the workgroup's partial.
//   k_seed_finish     thread k folds value k of the workgroups' partials in index order (as k_slice_quality_finish does).
//   k_seed_scale      SVR_RESAMPLE_SCALE: a second pass over the result, valid voxels times `scale` in float.
// No atomics and no order that depends on scheduling: the same bits on every call.  The number of workgroups follows from the volume's
// size alone.  The eight reads of a voxel are gathers; the call runs once per run.  The source copy, the result and the partials are
// allocated by the call and freed before it returns, like svr_slice_quality's: the coefficient table sizes itself by the memory that
// is free, and nothing here is cached, so the invalidation map has no line for them.  Installing the result writes the current volume
// whole: CH_VOLUME_VALUES, the line svr_update_reconstructed and svr_debug_set(SVR_BUF_RECONSTRUCTED) raise.

#define SEED_MAX_BLOCKS 2048

namespace {

struct SeedArgs {
  const float *src;          // [nz][ny][nx]
  const float *mask;         // reconstruction grid, or null
  float *out;                // reconstruction grid
  double *partial;           // [blocks][5]
  double m[12];
  int nx, ny, nz;
  unsigned vx, vy;
  size_t nv;
  float padding;
};

__global__ __launch_bounds__(256) void k_seed_resample(SeedArgs a) {
  __shared__ double sm[4][5];
  double n = 0.0, s1 = 0.0, s2 = 0.0, lo = HUGE_VAL, hi = -HUGE_VAL;
  const size_t stride = (size_t)gridDim.x * 256;
  const double pad = (double)a.padding;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < a.nv; i += stride) {
    float r = -1.0f;
    bool valid = false;
    if (!a.mask || a.mask[i] != 0.0f) {
      const size_t row = i / a.vx;
      const double x = (double)(unsigned)(i - row * a.vx), y = (double)(unsigned)(row % a.vy), z = (double)(row / a.vy);
      const double px = a.m[0] * x + a.m[1] * y + a.m[2] * z + a.m[3];
      const double py = a.m[4] * x + a.m[5] * y + a.m[6] * z + a.m[7];
      const double pz = a.m[8] * x + a.m[9] * y + a.m[10] * z + a.m[11];
      r = a.padding;
      // outside (-1, n) no neighbour lies in the grid (and the conversions to int below stay in range; a NaN fails every comparison)
      if (px > -1.0 && px < (double)a.nx && py > -1.0 && py < (double)a.ny && pz > -1.0 && pz < (double)a.nz) {
        const double fx = floor(px), fy = floor(py), fz = floor(pz);
        const int ix = (int)fx, iy = (int)fy, iz = (int)fz;
        const double tx = px - fx, ty = py - fy, tz = pz - fz;
        double W = 0.0, A = 0.0;
#pragma unroll
        for (int dz = 0; dz < 2; ++dz) {
          const int zi = iz + dz;
          const double wz = dz ? tz : 1.0 - tz;
#pragma unroll
          for (int dy = 0; dy < 2; ++dy) {
            const int yi = iy + dy;
            const double wy = dy ? ty : 1.0 - ty;
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
              const int xi = ix + dx;
              const double w = ((dx ? tx : 1.0 - tx) * wy) * wz;
              if (xi >= 0 && xi < a.nx && yi >= 0 && yi < a.ny && zi >= 0 && zi < a.nz) {
                const double v = (double)a.src[((size_t)zi * a.ny + yi) * a.nx + xi];
                if (v > pad) { W += w; A += w * v; }
              }
            }
          }
        }
        if (W >= 0.5) { r = (float)(A / W); valid = true; }
      }
    }
    a.out[i] = r;
    if (valid) {
      const double v = (double)r;
      n += 1.0; s1 += v; s2 += v * v;
      lo = fmin(lo, v); hi = fmax(hi, v);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    n += __shfl_xor(n, o, 64);
    s1 += __shfl_xor(s1, o, 64);
    s2 += __shfl_xor(s2, o, 64);
    lo = fmin(lo, __shfl_xor(lo, o, 64));
    hi = fmax(hi, __shfl_xor(hi, o, 64));
  }
  const int t = threadIdx.x, w = t >> 6;
  if ((t & 63) == 0) { sm[w][0] = n; sm[w][1] = s1; sm[w][2] = s2; sm[w][3] = lo; sm[w][4] = hi; }
  __syncthreads();
  if (t < 5) {
    double x;
    if (t < 3) x = ((sm[0][t] + sm[1][t]) + sm[2][t]) + sm[3][t];                       // wave order
    else if (t == 3) x = fmin(fmin(fmin(sm[0][3], sm[1][3]), sm[2][3]), sm[3][3]);
    else x = fmax(fmax(fmax(sm[0][4], sm[1][4]), sm[2][4]), sm[3][4]);
    a.partial[(size_t)blockIdx.x * 5 + t] = x;
  }
}

__global__ void k_seed_finish(const double *__restrict__ partial, int blocks, double *__restrict__ out) {
  const int k = threadIdx.x;
  if (k >= 5) return;
  double x = partial[k];
  for (int b = 1; b < blocks; ++b) {
    const double p = partial[(size_t)b * 5 + k];
    x = k < 3 ? x + p : k == 3 ? fmin(x, p) : fmax(x, p);
  }
  out[k] = x;
}

__global__ void k_seed_scale(float *__restrict__ out, const float *__restrict__ mask, float padding, float scale, size_t nv) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += stride) {
    if (mask && mask[i] == 0.0f) continue;
    const float v = out[i];
    if (v != padding) out[i] = v * scale;                     // (a valid result is a mean of values above the padding: never the padding itself)
  }
}

int seed_run(svr_ctx *ctx, size_t ns, const uint32_t src_size[3], const float *src, const double m[12], float padding, int flags, float scale,
             float *out, double stats[5]) {
  const int blocks = (int)std::min<size_t>(SEED_MAX_BLOCKS, (ctx->nv + 255) / 256);
  DevBuf<float> d_src, d_out;                                  // nothing is kept beyond the call (see above)
  DevBuf<double> d_partial;
  HIPCHK(d_src.reserve(ns));
  HIPCHK(d_out.reserve(ctx->nv));
  HIPCHK(d_partial.reserve(((size_t)blocks + 1) * 5));
  HIPCHK(hipMemcpyAsync(d_src, src, ns * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  SeedArgs a;
  a.src = d_src; a.mask = ctx->have_mask ? ctx->d_mask.get() : nullptr; a.out = d_out; a.partial = d_partial;
  for (int k = 0; k < 12; ++k) a.m[k] = m[k];
  a.nx = (int)src_size[0]; a.ny = (int)src_size[1]; a.nz = (int)src_size[2];
  a.vx = ctx->vx; a.vy = ctx->vy; a.nv = ctx->nv; a.padding = padding;
  hipLaunchKernelGGL(k_seed_resample, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, a);
  KCHK("k_seed_resample");
  double *d_stats = d_partial + (size_t)blocks * 5;
  hipLaunchKernelGGL(k_seed_finish, dim3(1), dim3(64), 0, ctx->stream, d_partial, blocks, d_stats);
  KCHK("k_seed_finish");
  if (flags & SVR_RESAMPLE_SCALE) {
    hipLaunchKernelGGL(k_seed_scale, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, d_out, a.mask, padding, scale, ctx->nv);
    KCHK("k_seed_scale");
  }
  if (flags & SVR_RESAMPLE_INSTALL) {
    HIPCHK(hipMemcpyAsync(ctx->recon(), d_out, ctx->nv * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    invalidate(ctx, CH_VOLUME_VALUES);
  }
  if (out) HIPCHK(hipMemcpyAsync(out, d_out, ctx->nv * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(stats, d_stats, 5 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

}  // namespace

extern "C" {

int svr_resample_to_reconstruction(svr_ctx *ctx, const uint32_t src_size[3], const float *src, const double src_from_recon[12], float padding,
                                   int flags, float scale, float *out_or_null, double stats[5]) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  if (!src_size || !src) return fail(ctx, SVR_E_ARG, "svr_resample_to_reconstruction: no source volume");
  if (!src_from_recon) return fail(ctx, SVR_E_ARG, "svr_resample_to_reconstruction: no matrix");
  if (!stats) return fail(ctx, SVR_E_ARG, "svr_resample_to_reconstruction: no array for the statistics");
  if (flags & ~(SVR_RESAMPLE_INSTALL | SVR_RESAMPLE_SCALE)) return fail(ctx, SVR_E_ARG, "svr_resample_to_reconstruction: unknown flag");
  if (!src_size[0] || !src_size[1] || !src_size[2]) return fail(ctx, SVR_E_ARG, "svr_resample_to_reconstruction: a source size is zero");
  size_t ns = (size_t)src_size[0] * src_size[1];               // (below 2^64; then at most 2^31 x 2^32)
  if (ns <= (size_t)INT32_MAX) ns *= src_size[2];
  if (ns > (size_t)INT32_MAX) return fail(ctx, SVR_E_ARG, "svr_resample_to_reconstruction: a source of more than 2^31 - 1 voxels");
  for (int k = 0; k < 12; ++k)
    if (!std::isfinite(src_from_recon[k])) return fail(ctx, SVR_E_ARG, "svr_resample_to_reconstruction: the matrix is not finite");
  if (!std::isfinite(padding) || ((flags & SVR_RESAMPLE_SCALE) && !std::isfinite(scale)))
    return fail(ctx, SVR_E_ARG, "svr_resample_to_reconstruction: padding / scale not finite");
  NEED(ctx->nv > 0, "InitReconstructionVolume first");
  return seed_run(ctx, ns, src_size, src, src_from_recon, padding, flags, scale, out_or_null, stats);
}

}  // extern "C"
