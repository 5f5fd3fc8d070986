// svr_small.inc -- the small kernels, #included by svr_hip.hip inside its first anonymous namespace: list compaction, the block reductions,
// the EM (E-step, M-step, scale, robust statistics), the volume kernels of the first rounds (Prep / regulariser reg_mode 0, equalize, mask, scale),
// the bias path and the NCC cost of the IRTK registration.  Moved out of svr_hip.hip in round 6 (nothing else changed).
// ------------------------------------------------------------------------------------------
// list compaction
// ------------------------------------------------------------------------------------------
// keep pixel i if slices[i] != -1 (and psf_sums[i] != 0 when psf_sums given)
// (one atomic on the counter per workgroup of 1024 and chunk, not per wavefront: 524 k wavefronts queueing on one address took
// 3.4 ms on S8's 33.5 M slice pixels, 0.34 ms on P4)
__global__ __launch_bounds__(1024) void k_compact(const float *slices, const float *psf_sums, uint32_t n, uint32_t *list,
                                                  uint32_t *counter) {
  __shared__ uint32_t sh_cnt[16], sh_base;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint64_t c0 = (uint64_t)blockIdx.x * 1024u; c0 < n; c0 += (uint64_t)gridDim.x * 1024u) {
    const uint64_t i = c0 + threadIdx.x;
    bool keep = false;
    if (i < n) {
      keep = slices[i] != -1.0f;
      if (keep && psf_sums) keep = psf_sums[i] != 0.0f;
    }
    const unsigned long long b = __ballot(keep);
    if (lane == 0) sh_cnt[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t tot = 0;
      for (int w = 0; w < 16; ++w) { const uint32_t t = sh_cnt[w]; sh_cnt[w] = tot; tot += t; }
      sh_base = tot ? atomicAdd(counter, tot) : 0u;
    }
    __syncthreads();
    if (keep) list[sh_base + sh_cnt[wave] + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = (uint32_t)i;
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------
// block reduction helpers (256 threads)
// ------------------------------------------------------------------------------------------
template <int K>
__device__ __forceinline__ void block_reduce_store(double v[K], const int op[K], double *out) {
  __shared__ double sm[4][K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double x = v[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      double y = __shfl_xor(x, o, 64);
      x = op[k] == 0 ? x + y : (op[k] == 1 ? fmin(x, y) : fmax(x, y));
    }
    v[k] = x;
  }
  int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0)
    for (int k = 0; k < K; ++k) sm[w][k] = v[k];
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 0; k < K; ++k) {
      double x = sm[0][k];
      for (int i = 1; i < 4; ++i) {
        double y = sm[i][k];
        x = op[k] == 0 ? x + y : (op[k] == 1 ? fmin(x, y) : fmax(x, y));
      }
      out[k] = x;
    }
  }
}

// sums partial[(sl*chunks + c)*K + k] over c (per slice) -> per_slice[sl*K + k]
__global__ void k_reduce_chunks(const double *partial, int ns, int chunks, int K, int opmask_min,
                                int opmask_max, double *per_slice) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ns * K) return;
  int sl = i / K, k = i - sl * K;
  bool mn = (opmask_min >> k) & 1, mx = (opmask_max >> k) & 1;
  double x = partial[((size_t)sl * chunks) * K + k];
  for (int c = 1; c < chunks; ++c) {
    double y = partial[((size_t)sl * chunks + c) * K + k];
    x = mn ? fmin(x, y) : (mx ? fmax(x, y) : x + y);
  }
  per_slice[i] = x;
}
constexpr int REDUCE_MAXK = 8;   // quantities reduce_partials takes side by side: k_reduce_slices' LDS rows, and what d_partial / d_per_slice are allocated for
// reduces per_slice[sl*K + k] over slices -> out[k]   (single block, 256 threads; K <= 8).  The K quantities go through the tree side by side --
// per quantity the order of one block reduction after the other (the same bits), one set of barriers for all: the kernel is nothing but latency
__global__ void k_reduce_slices(const double *per_slice, int ns, int K, int opmask_min,
                                int opmask_max, double *out) {
  __shared__ double sm[REDUCE_MAXK][256];
  const int t = threadIdx.x;
  for (int k = 0; k < K; ++k) {
    bool mn = (opmask_min >> k) & 1, mx = (opmask_max >> k) & 1;
    double x = mn ? INFINITY : (mx ? -INFINITY : 0.0);
    for (int s = t; s < ns; s += 256) {
      double y = per_slice[(size_t)s * K + k];
      x = mn ? fmin(x, y) : (mx ? fmax(x, y) : x + y);
    }
    sm[k][t] = x;
  }
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
      for (int k = 0; k < K; ++k) {
        bool mn = (opmask_min >> k) & 1, mx = (opmask_max >> k) & 1;
        double y = sm[k][t + o];
        double z = sm[k][t];
        sm[k][t] = mn ? fmin(z, y) : (mx ? fmax(z, y) : z + y);
      }
    }
    __syncthreads();
  }
  if (t < K) out[t] = sm[t][0];
}

// ------------------------------------------------------------------------------------------
// EM kernels over the slice grid: grid = (chunks, ns), 256 threads, CHUNK_PIX pixels per block
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float G_(float x, float s) {   // RC.cu:62-65
  return SVR_STEP * expf(-x * x / (2.0f * s)) / (sqrtf(6.28f * s));
}

// InitializeEMValuesKernel RC.cu:3241-3267
// pvr: InitializeEMValuesKernel of R2/patchBasedRobustStatistics_gpu.cu:55-76 also zeroes s == 0
__global__ void k_init_em(const float *slices, float *weights, size_t n, int pvr) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const float s = slices[i];
    weights[i] = (s != -1.0f && !(pvr && s == 0.0f)) ? 1.0f : 0.0f;
  }
}

// EStepKernel3D_tex RC.cu:2766-2813 fused with the slice-potential transform RC.cu:2816-2841
__global__ __launch_bounds__(256) void k_estep(const float *slices, const float *simslices,
                                               const float *simweights, const float *scales,
                                               const float *bias, float m_, float sigma_, float mix_, int n2,
                                               float *weights, double *partial, int pvr, const float *em) {
  if (em) { sigma_ = em[0]; mix_ = em[1]; m_ = em[2]; }   // svr_mstep_estep: the M-step's scalars never left the device
  const int sl = blockIdx.y;
  const float scale = scales[sl];
  if (pvr) {
    // EStepKernel of R2/patchBasedRobustStatistics_gpu.cu:106-150: gated on the pixel's current WEIGHT
    // (not the simulated weight), weights are not cleared first, __step = 1e-5f (reconConfig.cuh:120),
    // the mixture in double through the `1.0 - _mix` literal
    const float step = 0.00001f;
    const float m = m_ * step;
    double v[2] = {0.0, 0.0};
    const size_t base = (size_t)sl * n2;
    for (int i = blockIdx.x * CHUNK_PIX + threadIdx.x; i < min(n2, (int)(blockIdx.x + 1) * CHUNK_PIX); i += 256) {
      const float s = slices[base + i];
      float w = weights[base + i];
      if (!(s == -1.0f || w <= 0.0f)) {
        float patchVal = s * scale;
        patchVal -= simslices[base + i];
        const float g = step * expf(-patchVal * patchVal / (2.0f * sigma_)) / (sqrtf(6.28f * sigma_));
        w = (float)((double)(g * mix_) / ((double)(g * mix_) + (double)m * (1.0 - (double)mix_)));
        weights[base + i] = w;
      }
      if ((double)simweights[base + i] > 0.99) {        // transformPatchPotential :152-168
        const double t = 1.0 - (double)w;
        v[0] += (double)(float)(t * t);
        v[1] += 1.0;
      }
    }
    const int op[2] = {0, 0};
    block_reduce_store<2>(v, op, partial + ((size_t)sl * gridDim.x + blockIdx.x) * 2);
    return;
  }
  const float m = m_ * SVR_STEP;   // M_ RC.cu:67-70
  double v[2] = {0.0, 0.0};
  const size_t base = (size_t)sl * n2;
  for (int i = blockIdx.x * CHUNK_PIX + threadIdx.x; i < min(n2, (int)(blockIdx.x + 1) * CHUNK_PIX);
       i += 256) {
    float s = slices[base + i], sw = simweights[base + i];
    float w = 0.0f;                                    // weights are cleared first RC.cu:2881
    if (!(s == -1.0f || sw <= 0.0f)) {
      float sliceVal = bias ? s * expf(-bias[base + i]) * scale : s * scale;   // RC.cu:2792-2795
      sliceVal -= simslices[base + i];
      float g = G_(sliceVal, sigma_);
      w = (g * mix_) / (g * mix_ + m * (1.0f - mix_));
    }
    weights[base + i] = w;
    if ((double)sw > 0.99) {                           // transformSlicePotential RC.cu:2822
      double t = 1.0 - (double)w;
      v[0] += (double)(float)(t * t);
      v[1] += 1.0;
    }
  }
  const int op[2] = {0, 0};
  block_reduce_store<2>(v, op, partial + ((size_t)sl * gridDim.x + blockIdx.x) * 2);
}
// RC.cu:2903-2910
// (+ the sum over the slice's chunks, in chunk order like k_reduce_chunks: one launch instead of two -- these kernels last 4 us each and a
// rank of a sharded run has little else to hide them behind)
__global__ void k_potential_finish(const double *partial, int ns, int chunks, float *potential) {
  int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= ns) return;
  const double *p = partial + (size_t)s * chunks * 2;
  double a = p[0], b = p[1];
  for (int c = 1; c < chunks; ++c) { a += p[2 * c]; b += p[2 * c + 1]; }
  potential[s] = (b > 0) ? sqrtf((float)a / (float)b) : -1.0f;
}

// transformMStep3DNoBias RC.cu:2966-3000; reduce identity (0,0,0,0,0) RC.cu:3103
__global__ __launch_bounds__(256) void k_mstep(const float *slices, const float *weights,
                                               const float *simslices, const float *simweights,
                                               const float *scales, const float *bias, int n2,
                                               double *partial) {
  const int sl = blockIdx.y;
  const float scale = scales[sl];
  double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  const size_t base = (size_t)sl * n2;
  for (int i = blockIdx.x * CHUNK_PIX + threadIdx.x; i < min(n2, (int)(blockIdx.x + 1) * CHUNK_PIX);
       i += 256) {
    float s = slices[base + i];
    // transformMStep3D tests sw against the double 0.99, the NoBias twin against 0.99f (RC.cu:2947,2985)
    const float sw = simweights[base + i];
    if (s != -1.0f && (bias ? (double)sw > 0.99 : sw > 0.99f)) {
      float w = weights[base + i];
      float e = bias ? (s * expf(-bias[base + i]) * scale) - simslices[base + i] : (s * scale) - simslices[base + i];
      v[0] += (double)(e * e * w);
      v[1] += (double)w;
      v[2] += 1.0;
      v[3] = fmin(v[3], (double)e);
      v[4] = fmax(v[4], (double)e);
    }
  }
  const int op[5] = {0, 0, 0, 1, 2};
  block_reduce_store<5>(v, op, partial + ((size_t)sl * gridDim.x + blockIdx.x) * 5);
}

// transformScalenoBias RC.cu:3142-3165
__global__ __launch_bounds__(256) void k_scale(const float *slices, const float *weights,
                                               const float *simslices, const float *simweights,
                                               const float *bias, int n2, double *partial) {
  const int sl = blockIdx.y;
  double v[2] = {0.0, 0.0};
  const size_t base = (size_t)sl * n2;
  for (int i = blockIdx.x * CHUNK_PIX + threadIdx.x; i < min(n2, (int)(blockIdx.x + 1) * CHUNK_PIX);
       i += 256) {
    float s = slices[base + i];
    if (!(s == -1.0f || simweights[base + i] <= 0.99f)) {
      float w = weights[base + i], ss = simslices[base + i];
      if (bias) {                                        // transformScale RC.cu:3133-3136
        float eb = expf(-bias[base + i]);
        v[0] += (double)(w * s * eb * ss);
        v[1] += (double)(w * s * eb * s * eb);
      } else {
        v[0] += (double)(w * s * ss);
        v[1] += (double)(w * s * s);
      }
    }
  }
  const int op[2] = {0, 0};
  block_reduce_store<2>(v, op, partial + ((size_t)sl * gridDim.x + blockIdx.x) * 2);
}
// RC.cu:3229-3236
// (+ the two moves of the reference's one-call lag, svr_calculate_scale_vector: the device's scales take the PREVIOUS host copy, the host
// copy takes the new vector -- two device-to-device copies of ns floats until round 5, 5 us each on a stream that has nothing else to do)
// (+ the sum over the slice's chunks, in chunk order like k_reduce_chunks)
__global__ void k_scale_finish(const double *partial, int ns, int chunks, float *scale_vec, float *scales, float *scales_host_copy) {
  int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= ns) return;
  const double *p = partial + (size_t)s * chunks * 2;
  double a = p[0], b = p[1];
  for (int c = 1; c < chunks; ++c) { a += p[2 * c]; b += p[2 * c + 1]; }
  float num = (float)a, den = (float)b;
  const float v = (den != 0.0f) ? num / den : 1.0f;
  scale_vec[s] = v;
  scales[s] = scales_host_copy[s];
  scales_host_copy[s] = v;
}

// transformRS RC.cu:2243-2265
__global__ __launch_bounds__(256) void k_robust(const float *slices, const unsigned char *siminside,
                                                const float *simslices, const float *simweights, int n2,
                                                double *partial) {
  const int sl = blockIdx.y;
  double v[2] = {0.0, 0.0};
  const size_t base = (size_t)sl * n2;
  for (int i = blockIdx.x * CHUNK_PIX + threadIdx.x; i < min(n2, (int)(blockIdx.x + 1) * CHUNK_PIX);
       i += 256) {
    float s = slices[base + i];
    if (s != -1.0f && siminside[base + i] == 1 && (double)simweights[base + i] > 0.99) {
      float sval = s - simslices[base + i];
      v[0] += (double)(sval * sval);
      v[1] += 1.0;
    }
  }
  const int op[2] = {0, 0};
  block_reduce_store<2>(v, op, partial + ((size_t)sl * gridDim.x + blockIdx.x) * 2);
}

// ScaleVolumeKernel RC.cu:3386-3413
__global__ __launch_bounds__(256) void k_scalevol(const float *slices, const float *weights,
                                                  const float *simslices, const float *simweights,
                                                  const float *slice_weights, int n2, double *partial) {
  const int sl = blockIdx.y;
  const float slicew = slice_weights[sl];
  double v[2] = {0.0, 0.0};
  const size_t base = (size_t)sl * n2;
  for (int i = blockIdx.x * CHUNK_PIX + threadIdx.x; i < min(n2, (int)(blockIdx.x + 1) * CHUNK_PIX);
       i += 256) {
    float s = slices[base + i];
    if (s == -1.0f) continue;
    if ((double)simweights[base + i] <= 0.99) continue;
    float ss = simslices[base + i], w = weights[base + i];
    v[0] += (double)(w * slicew * s * ss);
    v[1] += (double)(w * slicew * ss * ss);
  }
  const int op[2] = {0, 0};
  block_reduce_store<2>(v, op, partial + ((size_t)sl * gridDim.x + blockIdx.x) * 2);
}

// per-slice any(siminside == 1)  (thrust::count per slice, RC.cu:2742-2752)
__global__ __launch_bounds__(256) void k_slice_inside(const unsigned char *siminside, int n2,
                                                      unsigned char *slice_inside) {
  const int sl = blockIdx.x;
  int any = 0;
  for (int i = threadIdx.x; i < n2; i += 256) any |= (siminside[(size_t)sl * n2 + i] == 1);
  any = __syncthreads_or(any);
  if (threadIdx.x == 0) slice_inside[sl] = any ? 1 : 0;
}
// count_if(sliceVoxel_count > 0) RC.cu:2472-2474
__global__ void k_count_positive(const int *v, size_t n, unsigned long long *out) {
  // grid-stride: a thread counts its own, a wavefront adds up and touches the counter once (an atomic per 64 elements: 3.5 ms on S8)
  unsigned int cnt = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) cnt += v[i] > 0 ? 1u : 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(out, (unsigned long long)cnt);
}
// RestoreSliceIntensitiesKernel RC.cu:3349-3367
__global__ void k_restore(float *slices, const float *stack_factors, const int *stack_index, int n2,
                          size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float factor = stack_factors[stack_index[i / n2]];
  float s = slices[i];
  if (s > 0) slices[i] = s / factor;
}

// ------------------------------------------------------------------------------------------
// volume kernels
// ------------------------------------------------------------------------------------------
// equalizeVol RC.cu:2312-2327
__global__ void k_equalize(float *recon, const float *volw, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float b = volw[i];
  float a = recon[i];
  recon[i] = (b != 0) ? a / b : a;
}
// AdaptiveRegularizationPrep RC.cu:1944-1969: recon is left untouched (it is the regulariser's
// `original`, RC.cu:2138-2141); the updated volume goes to snap.
__global__ void k_reg_prep(int adaptive, float alpha, const float *recon, float *addon, float *cmap,
                           float min_i, float max_i, float *snap, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float ad = addon[i];
  if (!adaptive) {
    float c = cmap[i];
    if (c != 0) {
      ad = ad / c;
      addon[i] = ad;
      cmap[i] = 1.0f;
    }
  }
  float r = recon[i] + ad * alpha;
  if ((double)r < (double)min_i * 0.9) r = (float)((double)min_i * 0.9);
  if ((double)r > (double)max_i * 1.1) r = (float)((double)max_i * 1.1);
  snap[i] = r;
}

__constant__ int c_dirs[13][3] = {{1, 0, -1}, {0, 1, -1}, {1, 1, -1}, {1, -1, -1}, {1, 0, 0},
                                  {0, 1, 0},  {1, 1, 0},  {1, -1, 0}, {1, 0, 1},   {0, 1, 1},
                                  {1, 1, 1},  {1, -1, 1}, {0, 0, 1}};   // RC.cu:666-680

__device__ __forceinline__ float reg_b(float f, float sqf, float o_p, float o_p2, float c_p, float c_p2,
                                       float delta) {
  // AdaptiveRegularization1 RC.cu:2046-2057
  if (c_p <= 0 || c_p2 <= 0) return 0.0f;
  float diff = (o_p2 - o_p) * sqf / delta;
  return (float)((double)f / sqrt(1.0 + (double)(diff * diff)));
}
// AdaptiveRegularizationKernel RC.cu:2061-2117; neighbours read `snap` (post-Prep snapshot)
__global__ __launch_bounds__(256) void k_regularize(int vx, int vy, int vz, float delta, float alpha,
                                                    float lambda, const float *snap,
                                                    const float *original, const float *cmap,
                                                    float *out) {
  int x = blockIdx.x * 64 + (threadIdx.x & 63);
  int y = blockIdx.y * 4 + (threadIdx.x >> 6);
  int z = blockIdx.z;
  if (x >= vx || y >= vy) return;
  size_t p = (size_t)x + (size_t)y * vx + (size_t)z * vx * vy;
  float val = 0, valW = 0, sum = 0;
  float o_p = original[p], c_p = cmap[p], r_p = snap[p];
#pragma unroll
  for (int i = 0; i < 13; ++i) {
    const int dx = c_dirs[i][0], dy = c_dirs[i][1], dz = c_dirs[i][2];
    const float f = 1.0f / (float)(abs(dx) + abs(dy) + abs(dz));   // RC.cu:682-692
    const float sqf = sqrtf(f);
    int x2 = x + dx, y2 = y + dy, z2 = z + dz;
    bool in2 = x2 >= 0 && x2 < vx && y2 >= 0 && y2 < vy && z2 >= 0 && z2 < vz;
    float o2 = 0, c2 = 0;
    if (in2) {
      size_t p2 = (size_t)x2 + (size_t)y2 * vx + (size_t)z2 * vx * vy;
      o2 = original[p2];
      c2 = cmap[p2];
      float bi = reg_b(f, sqf, o_p, o2, c_p, c2, delta);
      val += bi * snap[p2] * c2;
      valW += bi * c2;
      sum += bi;
    }
    int x3 = x - dx, y3 = y - dy, z3 = z - dz;
    bool in3 = x3 >= 0 && x3 < vx && y3 >= 0 && y3 < vy && z3 >= 0 && z3 < vz;
    if (in3 && in2) {
      size_t p3 = (size_t)x3 + (size_t)y3 * vx + (size_t)z3 * vx * vy;
      float o3 = original[p3], c3 = cmap[p3];
      float bi = reg_b(f, sqf, o3, o2, c3, c2, delta);   // (pos3, pos2): RC.cu:2095
      val += bi * snap[p3] * c3;
      valW += bi * c3;
      sum += bi;
    }
  }
  val -= sum * r_p * c_p;
  valW -= sum * c_p;
  float k = alpha * lambda / (delta * delta);
  val = r_p * c_p + k * val;
  valW = c_p + k * valW;
  out[p] = (valW > 0.0f) ? val / valW : 0.0f;
}
#include "svr_regul.inc"
// maskVolumeKernel RC.cu:3313-3326
// {V m, m} per voxel (m = 1 inside the mask, else 0): what the gather's LDS boxes hold, packed once per pass so that a
// box voxel is one 8-byte load instead of two loads and a select
__global__ void k_pack_volm(const float *vol, const float *mask, float2 *out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float m = mask[i] != 0.0f ? 1.0f : 0.0f;
  out[i] = make_float2(m != 0.0f ? vol[i] : 0.0f, m);
}

// the patch-based gather reads the volume through getReconValueFromTexture's 8-voxel average (pvr_tex, reconVolume.cu:170-187):
// taken once per voxel and pass here instead of once per box voxel of every tile (eight loads each); same operations, same bits
__global__ void k_pack_volm_pvr(const float *vol, const float *mask, float2 *out, VolGeom vg) {
  const size_t n = (size_t)vg.vx * vg.vy * vg.vz;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float m = mask[i] != 0.0f ? 1.0f : 0.0f;
  const int X = (int)(i % (size_t)vg.vx), Y = (int)((i / (size_t)vg.vx) % (size_t)vg.vy), Z = (int)(i / ((size_t)vg.vx * vg.vy));
  out[i] = make_float2(m != 0.0f ? pvr_tex(vol, vg, X, Y, Z) : 0.0f, m);
}

__global__ void k_mask_volume(float *recon, const float *mask, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && mask[i] == 0) recon[i] = -1.0f;
}
// scaleVolumeKernel RC.cu:3415-3423
__global__ void k_scale_volume(float *recon, float scale, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && recon[i] > 0) recon[i] = recon[i] * scale;
}


// ------------------------------------------------------------------------------------------
// bias correction (SURVEY 8a13): CorrectBias RC.cu:1837-1942, NormaliseBias RC.cu:2519-2652
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int reflect_(int M, int x) { return max(0, min(M - 1, x)); }   // RC.cu:53-56

// calculateResidual3D_adv RC.cu:1687-1731
__global__ void k_bias_residual(const float *slices, const float *bias, const float *weights,
                                const float *simweights, const float *simslices, const float *scales, int n2,
                                size_t n, float *wb, float *wr) {
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  float s = slices[idx];
  if (s == -1.0f) return;
  float wbo = 0.0f, wro = 0.0f;
  if ((double)simweights[idx] > 0.99) {
    float eb = expf(-bias[idx]);
    float sliceVal = s * (eb * scales[idx / n2]);
    wbo = weights[idx] * sliceVal;
    float ss = simslices[idx];
    if (((double)ss > 1.0) && ((double)sliceVal > 1.0)) wro = logf(sliceVal / ss) * wbo;
  }
  if (wbo > 0) { wb[idx] = wbo; wr[idx] = wro; }
}

// GaussianConvolutionKernel<float> RC.cu:909-985: one 1-D pass (recursive Gaussian weights, border
// repeat); the output is only written where the result != 0, so `out` keeps its previous content
// elsewhere -- the reference relies on that when it reuses its buffer (RC.cu:1886-1891).
__global__ void k_gauss_conv_slices(const float *in, float *out, const SliceConst *sc, int sx, int sy, int ns,
                                    float sigma, int horizontal) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), sl = blockIdx.z;
  if (x >= sx || y >= sy) return;
  const size_t base = (size_t)sl * sx * sy;
  const float sigma2 = sigma / sc[sl].dim[0];
  int klength = 2 * (int)roundf(4 * sigma2) + 1;
  klength -= 1 - klength % 2;
  const int half = (klength - 1) / 2;
  float g0 = (float)(1.0 / (sqrt(2.0 * M_PI) * sigma2));
  float g1 = (float)exp(-0.5 / (sigma2 * sigma2));
  const float g2 = g1 * g1;
  const size_t idx = base + x + (size_t)y * sx;
  float sum = g0 * in[idx];
  float sum_coeff = g0;
  for (int i = 1; i <= half; ++i) {
    g0 *= g1;
    g1 *= g2;
    const size_t a = horizontal ? base + reflect_(sx, x + i) + (size_t)y * sx : base + x + (size_t)reflect_(sy, y + i) * sx;
    sum += g0 * in[a];
    const size_t b = horizontal ? base + reflect_(sx, x - i) + (size_t)y * sx : base + x + (size_t)reflect_(sy, y - i) * sx;
    sum += g0 * in[b];
    sum_coeff += 2 * g0;
  }
  const float outv = sum / sum_coeff;
  if (outv != 0) out[idx] = outv;
}

// updateBiasField3D_adv RC.cu:1734-1758
__global__ void k_bias_update(const float *slices, float *bias, const float *wb, const float *wr, size_t n) {
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  if (slices[idx] == -1.0f) return;
  float w = wb[idx];
  if (w > 0) bias[idx] = bias[idx] + wr[idx] / w;
}
// per-slice {count(s > -1), sum(bias)}  (count_if + reduce, RC.cu:1904-1909)
__global__ __launch_bounds__(256) void k_bias_mean(const float *slices, const float *bias, int n2, double *partial) {
  const int sl = blockIdx.y;
  double v[2] = {0.0, 0.0};
  const size_t base = (size_t)sl * n2;
  for (int i = blockIdx.x * CHUNK_PIX + threadIdx.x; i < min(n2, (int)(blockIdx.x + 1) * CHUNK_PIX); i += 256) {
    if (slices[base + i] > -1.0f) v[0] += 1.0;
    v[1] += (double)bias[base + i];
  }
  const int op[2] = {0, 0};
  block_reduce_store<2>(v, op, partial + ((size_t)sl * gridDim.x + blockIdx.x) * 2);
}
// transformBiasMean RC.cu:1760-1783 with the mean of RC.cu:1911-1921
__global__ void k_bias_sub_mean(const float *slices, float *bias, const double *per_slice, int n2, size_t n) {
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  if (slices[idx] == -1.0f) return;
  const int sl = (int)(idx / n2);
  const double num = per_slice[2 * sl], sum = per_slice[2 * sl + 1];
  const float mean = num > 0 ? (float)(sum / num) : -1.0f;
  if (mean == -1.0f) return;
  if (mean != 0) bias[idx] = bias[idx] - mean;
}

// GaussianConvolutionKernel3D RC.cu:988-1093, one direction; written unless NaN
__global__ void k_gauss_conv3d(const float *in, float *out, float sigma, int dir, float dimd, int vx, int vy, int vz) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), z = blockIdx.z;
  if (x >= vx || y >= vy) return;
  const float sigma2 = sigma / dimd;
  int klength = 2 * (int)roundf(4 * sigma2) + 1;
  klength -= 1 - klength % 2;
  const int half = (klength - 1) / 2;
  float g0 = (float)(1.0 / (sqrt(2.0 * M_PI) * sigma2));
  float g1 = (float)exp(-0.5 / (sigma2 * sigma2));
  const float g2 = g1 * g1;
  const size_t sxy = (size_t)vx * vy;
  const size_t idx = x + (size_t)y * vx + (size_t)z * sxy;
  float sum = g0 * in[idx];
  float sum_coeff = g0;
  for (int i = 1; i <= half; ++i) {
    g0 *= g1;
    g1 *= g2;
    size_t a, b;
    if (dir == 0) { a = reflect_(vx, x + i) + (size_t)y * vx + (size_t)z * sxy; b = reflect_(vx, x - i) + (size_t)y * vx + (size_t)z * sxy; }
    else if (dir == 1) { a = x + (size_t)reflect_(vy, y + i) * vx + (size_t)z * sxy; b = x + (size_t)reflect_(vy, y - i) * vx + (size_t)z * sxy; }
    else { a = x + (size_t)y * vx + (size_t)reflect_(vz, z + i) * sxy; b = x + (size_t)y * vx + (size_t)reflect_(vz, z - i) * sxy; }
    sum += g0 * in[a];
    sum += g0 * in[b];
    sum_coeff += 2 * g0;
  }
  const float outv = sum / sum_coeff;
  if (outv == outv) out[idx] = outv;
}
// divS RC.cu:1786-1797
__global__ void k_div_s(float *a, const float *b, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { float d = b[i]; a[i] = (d != 0) ? a[i] / d : 0; }
}
// a += b (NormaliseBias on the cell path: dev_volume_weights_ accumulates over the calls, RC.cu:2633)
__global__ void k_add_to(float *a, const float *b, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) a[i] += b[i];
}
// divexp RC.cu:2505-2516
__global__ void k_divexp(float *recon, const float *bias, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { float a = recon[i]; if (a != -1.0f) recon[i] = a / expf(-bias[i]); }
}
