// svr_pyr.inc -- the image pyramid of the default (IRTK) registration on the device; included by svr_hip.hip.
//
// irtkImageRegistrationWithPadding::Initialize(level) (IRTKSimple2/packages/registration/src/
// irtkImageRegistrationWithPadding.cc:28-334) blurs, resamples and re-ranges every target and the source at each of three
// levels.  csrc/irtk_reg.cpp restates that on the host (blur_with_padding, resample_with_padding, prepare_level) and stays
// the definition: the kernels below do the same double arithmetic operation for operation (the library is built with
// -ffp-contract=off, double division and the conversions are IEEE on gfx950), so a level made here is the level made
// there bit for bit (every voxel of every level against an independent reference: tests/test_pyramid_gpu.py, the host code
// against the same reference: tests/test_pyramid_ref.py; end to end: tests/test_irtk_registration.py::
// test_device_pyramid_is_the_host_pyramid).  What it buys: the host of
// a gpurun box has 16 CPUs' worth of quota -- the pyramids of 512 slices of 256 x 256 took 0.5 s of a 0.87 s pass, the
// pyramid of a 400 x 400 x 320 source 0.5 s of a 1.4 s pass -- and the levels no longer travel host -> device.

namespace {

struct PyrImg { double i2w[12], w2i[12]; int pad; int pad_; };

// irtkGaussianBlurringWithPadding<short>: one 1-D pass (irtkConvolutionWithPadding_1D.cc:45-70), truncated to short
__global__ void k_pyr_blur(const short *in, short *out, int nx, int ny, int nz, int axis, const double *ker, int half,
                           const PyrImg *imgs) {
  const size_t nvox = (size_t)nx * ny * nz;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nvox) return;
  const int img = blockIdx.y;
  const short pad = (short)imgs[img].pad;
  const short *p = in + (size_t)img * nvox;
  const short c = p[i];
  short r;
  if (c <= pad) {
    r = pad;
  } else {
    const int x = (int)(i % nx), y = (int)((i / nx) % ny), z = (int)(i / ((size_t)nx * ny));
    const int pos = axis == 0 ? x : axis == 1 ? y : z, n = axis == 0 ? nx : axis == 1 ? ny : nz;
    const ptrdiff_t stride = axis == 0 ? 1 : axis == 1 ? nx : (ptrdiff_t)nx * ny;
    double val = 0, sum = 0;
    for (int t = -half; t <= half; ++t) {
      const int q = pos + t;
      if (q < 0 || q >= n) continue;
      const short g = p[(ptrdiff_t)i + t * stride];
      if (g > pad) { val += ker[t + half] * g; sum += ker[t + half]; }
    }
    double v = sum > 0 ? val / sum : 0.0;
    if (v > 32767.0) v = 32767.0;
    if (v < -32768.0) v = -32768.0;
    r = (short)v;
  }
  out[(size_t)img * nvox + i] = r;
}

// irtkResamplingWithPadding<short>::Run, irtkResamplingWithPadding.cc:202-443
__global__ void k_pyr_resample(const short *in, int X, int Y, int Z, short *out, int ox, int oy, int oz, const PyrImg *imgs) {
  const size_t nout = (size_t)ox * oy * oz;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= nout) return;
  const int img = blockIdx.y;
  const PyrImg &g = imgs[img];
  const short pad = (short)g.pad;
  const short *p = in + (size_t)img * X * Y * Z;
  const int i = (int)(idx % ox), j = (int)((idx / ox) % oy), k = (int)(idx / ((size_t)ox * oy));
  const double wx = g.i2w[0] * i + g.i2w[1] * j + g.i2w[2] * k + g.i2w[3];
  const double wy = g.i2w[4] * i + g.i2w[5] * j + g.i2w[6] * k + g.i2w[7];
  const double wz = g.i2w[8] * i + g.i2w[9] * j + g.i2w[10] * k + g.i2w[11];
  const double x = g.w2i[0] * wx + g.w2i[1] * wy + g.w2i[2] * wz + g.w2i[3];
  const double y = g.w2i[4] * wx + g.w2i[5] * wy + g.w2i[6] * wz + g.w2i[7];
  const double z = g.w2i[8] * wx + g.w2i[9] * wy + g.w2i[10] * wz + g.w2i[11];
  const int u = (int)floor(x), v = (int)floor(y), w = (int)floor(z);
  const double dx = x - u, dy = y - v, dz = z - w;
  const double wt[8] = {(1 - dx) * (1 - dy) * (1 - dz), (1 - dx) * (1 - dy) * dz, (1 - dx) * dy * (1 - dz), (1 - dx) * dy * dz,
                        dx * (1 - dy) * (1 - dz),       dx * (1 - dy) * dz,       dx * dy * (1 - dz),       dx * dy * dz};
  double val = 0, sum = 0;
  int npad = 8;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int a = u + (c >> 2), b = v + ((c >> 1) & 1), e = w + (c & 1);
    if (a >= 0 && a < X && b >= 0 && b < Y && e >= 0 && e < Z) {
      const short s = p[((size_t)e * Y + b) * X + a];
      if (s != pad) { npad--; val += s * wt[c]; sum += wt[c]; }
    } else {
      npad--;
    }
  }
  short r = pad;
  if (npad < 4 && sum > 0) {
    double q = val / sum;
    if (q > 32767.0) q = 32767.0;
    if (q < -32768.0) q = -32768.0;
    r = (short)q;
  }
  out[(size_t)img * nout + idx] = r;
}

__global__ void k_pyr_range_init(int *mn, int *mx, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { mn[i] = 32767; mx[i] = -32768; }
}

// range of the values above the padding (Initialize, irtkImageRegistrationWithPadding.cc:120-160)
__global__ __launch_bounds__(256) void k_pyr_range(const short *in, size_t nvox, const PyrImg *imgs, int *mn, int *mx) {
  const int img = blockIdx.y;
  const short pad = (short)imgs[img].pad;
  const short *p = in + (size_t)img * nvox;
  int lo = 32767, hi = -32768;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvox; i += (size_t)gridDim.x * 256) {
    const int v = p[i];
    if (v > pad) { lo = min(lo, v); hi = max(hi, v); }
  }
  for (int off = 32; off > 0; off >>= 1) { lo = min(lo, __shfl_down(lo, off)); hi = max(hi, __shfl_down(hi, off)); }
  if ((threadIdx.x & 63) == 0) { atomicMin(&mn[img], lo); atomicMax(&mx[img], hi); }
}

// v > pad ? v - min : -1, written where svr_ncc_evaluate reads: the source volume, or the target planes (row pitch tx,
// plane pitch tx * ty, image i at plane first_plane + i * nz)
__global__ void k_pyr_shift(const short *in, int nx, int ny, int nz, const PyrImg *imgs, const int *mn, short *dst, int tx, int ty,
                            int first_plane) {
  const size_t nvox = (size_t)nx * ny * nz;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nvox) return;
  const int img = blockIdx.y;
  const short pad = (short)imgs[img].pad;
  const short v = in[(size_t)img * nvox + i];
  const short r = v > pad ? (short)(v - (short)mn[img]) : (short)-1;
  const int x = (int)(i % nx), y = (int)((i / nx) % ny), z = (int)(i / ((size_t)nx * ny));
  dst[(((size_t)first_plane + (size_t)img * nz + z) * ty + y) * tx + x] = r;
}

__global__ void k_pyr_fill(short *p, size_t n, short v) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

}  // namespace

extern "C" {

int svr_ncc_alloc_targets(svr_ctx *ctx, int n, int tx, int ty) {
  SVR_ENTER(ctx);
  if (!ctx || n <= 0 || tx <= 0 || ty <= 0) return SVR_E_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  ctx->d_reg_targets.reset();
  const size_t count = (size_t)n * tx * ty;
  HIPCHK(ctx->d_reg_targets.reserve(count));
  hipLaunchKernelGGL(k_pyr_fill, dim3(nblk(count)), dim3(256), 0, ctx->stream, ctx->d_reg_targets, count, (short)-1);
  KCHK("k_pyr_fill");
  ctx->reg_n = n; ctx->reg_tx = tx; ctx->reg_ty = ty;
  return SVR_OK;
}

int svr_pyr_upload(svr_ctx *ctx, int slot, const int16_t *images, size_t count) {
  SVR_ENTER(ctx);
  if (!ctx || !images || count == 0 || slot < 0 || slot > 1) return SVR_E_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  ctx->pyr_count[slot] = 0;                               // (the elements that were uploaded, not the block's size: none until the copy below is through)
  HIPCHK(ctx->d_pyr_full[slot].reserve(count));
  HIPCHK(hipMemcpyAsync(ctx->d_pyr_full[slot], images, count * sizeof(short), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->pyr_count[slot] = count;
  return SVR_OK;
}

int svr_pyr_level(svr_ctx *ctx, int slot, size_t offset, int n_images, const int in_dims[3], const double *kernel_x, int size_x,
                  const double *kernel_y, int size_y, const double *kernel_z, int size_z, int resample, const int out_dims[3],
                  const svr_pyr_image *images, int first_plane, int *min_out, int *max_out) {
  SVR_ENTER(ctx);
  if (!ctx || slot < 0 || slot > 1 || n_images <= 0 || !in_dims || !out_dims || !images) return SVR_E_ARG;
  if (slot == 0 && n_images != 1) return fail(ctx, SVR_E_ARG, "svr_pyr_level: one source");
  HIPCHK(hipSetDevice(ctx->device));
  const size_t nin = (size_t)in_dims[0] * in_dims[1] * in_dims[2], nout = (size_t)out_dims[0] * out_dims[1] * out_dims[2];
  if (nin == 0 || nout == 0 || nin >= (1ull << 31) || nout >= (1ull << 31)) return fail(ctx, SVR_E_ARG, "svr_pyr_level: image size out of range");
  if (n_images > 65535) return fail(ctx, SVR_E_ARG, "svr_pyr_level: at most 65535 images of one grid per call");
  // against what the last upload holds, not the block's capacity: a kept block keeps an earlier, larger upload's tail
  NEED(ctx->d_pyr_full[slot] && offset <= ctx->pyr_count[slot] && nin * n_images <= ctx->pyr_count[slot] - offset, "svr_pyr_upload first");
  if (!resample && nout != nin) return fail(ctx, SVR_E_ARG, "svr_pyr_level: a level that keeps the grid keeps its size");
  if (slot == 1) {
    NEED(ctx->d_reg_targets, "svr_ncc_alloc_targets first");
    if (out_dims[0] > ctx->reg_tx || out_dims[1] > ctx->reg_ty || first_plane < 0 ||
        (long long)first_plane + (long long)n_images * out_dims[2] > ctx->reg_n)
      return fail(ctx, SVR_E_ARG, "svr_pyr_level: the planes do not fit the allocated targets");
  }
  const size_t work = (size_t)n_images * std::max(nin, nout);
  HIPCHK(ctx->d_pyr_a.reserve(work));
  HIPCHK(ctx->d_pyr_b.reserve(work));
  // meta: the images' matrices and paddings, the three kernels, min / max
  const int sizes[3] = {size_x, size_y, size_z};
  const double *kers[3] = {kernel_x, kernel_y, kernel_z};
  size_t ker_total = 0;
  for (int a = 0; a < 3; ++a) {
    if (sizes[a] < 0 || (sizes[a] > 0 && (!kers[a] || sizes[a] % 2 == 0))) return fail(ctx, SVR_E_ARG, "svr_pyr_level: odd kernel sizes");
    ker_total += (size_t)sizes[a];
  }
  const size_t img_bytes = sizeof(PyrImg) * (size_t)n_images, ker_bytes = sizeof(double) * std::max<size_t>(ker_total, 1),
               mm_bytes = 2 * sizeof(int) * (size_t)n_images, meta = img_bytes + ker_bytes + mm_bytes;
  HIPCHK(ctx->d_pyr_meta.reserve(meta));
  std::vector<unsigned char> hmeta(img_bytes + ker_bytes, 0);
  PyrImg *hi = reinterpret_cast<PyrImg *>(hmeta.data());
  for (int i = 0; i < n_images; ++i) {
    memcpy(hi[i].i2w, images[i].i2w_out, sizeof(hi[i].i2w));
    memcpy(hi[i].w2i, images[i].w2i_in, sizeof(hi[i].w2i));
    hi[i].pad = images[i].pad; hi[i].pad_ = 0;
  }
  double *hk = reinterpret_cast<double *>(hmeta.data() + img_bytes);
  size_t koff[3], at = 0;
  for (int a = 0; a < 3; ++a) { koff[a] = at; if (sizes[a]) memcpy(hk + at, kers[a], sizeof(double) * sizes[a]); at += sizes[a]; }
  HIPCHK(hipMemcpyAsync(ctx->d_pyr_meta, hmeta.data(), hmeta.size(), hipMemcpyHostToDevice, ctx->stream));
  const PyrImg *d_img = reinterpret_cast<const PyrImg *>(ctx->d_pyr_meta.get());
  const double *d_ker = reinterpret_cast<const double *>(ctx->d_pyr_meta.get() + img_bytes);
  int *d_mn = reinterpret_cast<int *>(ctx->d_pyr_meta.get() + img_bytes + ker_bytes), *d_mx = d_mn + n_images;
  // blur: three passes, each from the previous one's shorts
  const short *cur = ctx->d_pyr_full[slot] + offset;
  short *bufs[2] = {ctx->d_pyr_a, ctx->d_pyr_b};
  int flip = 0;
  for (int a = 0; a < 3; ++a) {
    if (!sizes[a]) continue;
    hipLaunchKernelGGL(k_pyr_blur, dim3(nblk(nin), n_images), dim3(256), 0, ctx->stream, cur, bufs[flip], in_dims[0], in_dims[1], in_dims[2], a,
                       d_ker + koff[a], sizes[a] / 2, d_img);
    cur = bufs[flip]; flip ^= 1;
  }
  KCHK("k_pyr_blur");
  int lx = in_dims[0], ly = in_dims[1], lz = in_dims[2];
  if (resample) {
    hipLaunchKernelGGL(k_pyr_resample, dim3(nblk(nout), n_images), dim3(256), 0, ctx->stream, cur, in_dims[0], in_dims[1], in_dims[2], bufs[flip],
                       out_dims[0], out_dims[1], out_dims[2], d_img);
    KCHK("k_pyr_resample");
    cur = bufs[flip]; flip ^= 1;
    lx = out_dims[0]; ly = out_dims[1]; lz = out_dims[2];
  }
  hipLaunchKernelGGL(k_pyr_range_init, dim3(nblk(n_images)), dim3(256), 0, ctx->stream, d_mn, d_mx, n_images);
  const unsigned chunks = (unsigned)std::min<size_t>(1024, (nout + 4095) / 4096);
  hipLaunchKernelGGL(k_pyr_range, dim3(chunks, n_images), dim3(256), 0, ctx->stream, cur, nout, d_img, d_mn, d_mx);
  KCHK("k_pyr_range");
  short *dst;
  int tx, ty;
  if (slot == 0) {
    ctx->d_reg_source.reset();
    HIPCHK(ctx->d_reg_source.reserve(nout));
    ctx->reg_vx = lx; ctx->reg_vy = ly; ctx->reg_vz = lz;
    dst = ctx->d_reg_source; tx = lx; ty = ly; first_plane = 0;
  } else {
    dst = ctx->d_reg_targets; tx = ctx->reg_tx; ty = ctx->reg_ty;
  }
  hipLaunchKernelGGL(k_pyr_shift, dim3(nblk(nout), n_images), dim3(256), 0, ctx->stream, cur, lx, ly, lz, d_img, d_mn, dst, tx, ty, first_plane);
  KCHK("k_pyr_shift");
  std::vector<int> mm(2 * (size_t)n_images);
  HIPCHK(hipMemcpyAsync(mm.data(), d_mn, mm_bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < n_images; ++i) {
    if (min_out) min_out[i] = mm[i];
    if (max_out) max_out[i] = mm[n_images + i];
  }
  return SVR_OK;
}

// what svr_ncc_evaluate reads, copied to the host for the tests: which 0 = the source, short [vz][vy][vx], dims = {vx, vy, vz};
// 1 = the target planes, short [n][ty][tx], dims = {tx, ty, n}.  Reads only: no buffer, size or cached state changes.
int svr_ncc_get(svr_ctx *ctx, int which, int dims[3], int16_t *out_or_null, size_t count) {
  SVR_ENTER(ctx);
  if (!ctx || !dims || which < 0 || which > 1) return SVR_E_ARG;
  const short *src;
  if (which == 0) {
    NEED(ctx->d_reg_source, "no source: svr_ncc_set_source or svr_pyr_level (slot 0) first");
    dims[0] = (int)ctx->reg_vx; dims[1] = (int)ctx->reg_vy; dims[2] = (int)ctx->reg_vz;
    src = ctx->d_reg_source;
  } else {
    NEED(ctx->d_reg_targets, "no targets: svr_ncc_set_targets or svr_ncc_alloc_targets first");
    dims[0] = ctx->reg_tx; dims[1] = ctx->reg_ty; dims[2] = ctx->reg_n;
    src = ctx->d_reg_targets;
  }
  if (!out_or_null) return SVR_OK;
  const size_t n = (size_t)dims[0] * dims[1] * dims[2];
  if (count != n) return fail(ctx, SVR_E_ARG, "svr_ncc_get: size mismatch");
  HIPCHK(hipMemcpyAsync(out_or_null, src, n * sizeof(short), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

}  // extern "C"
