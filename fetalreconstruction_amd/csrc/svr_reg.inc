// svr_reg.inc -- GPU slice-to-volume registration (SURVEY 8a17, 8f1); included by svr_hip.hip.
//
// The reference's opt-in `--useGPUReg` path: registerMultipleSlicesToVolume (RC.cu:4001-4141) =
// batched gradient ascent over all slices of a device on the sum of three NCC values (blurred
// resampled slice vs the volume resampled at through-plane offsets -2, 0, +2 voxels of the slice
// plane), central differences in the 6 rigid parameters, line search with active-set compaction.
//
// MI355X layout: the three offsets of one evaluateCostsMultipleSlices call are one batch
// (grid z = offset), every per-(slot, offset) reduction is one workgroup with a fixed tree in
// double (deterministic; the reference uses float atomics), the volume snapshot (<= a few 10 MB)
// is gathered straight from L2/MALL.  The reference's temp-buffer aliasing (its memset of
// float[2*slices, 5*slices), RC.cu:4200, and the sampled-slice sums that are never reset between
// offsets, RC.cu:4195) changes the similarity values and is reproduced by a per-slot state
// machine in k_reg_combine instead of by aliasing memory.

struct RegState {
  int W = 0, H = 0, ns = 0;
  size_t wh = 0;
  DevBuf<float> resampled, target, tmp, reg;                                       // [ns][H][W], .., [3ns].., [3][ns][H][W]
  DevBuf<float> vol;                                                               // snapshot of the reconstruction
  DevBuf<float> ofs, mat, mat_orig;                                                // [ns][16]
  DevBuf<float> sim, grad;                                                         // [5][ns], [7][ns]
  DevBuf<int> active, active2, active_prev, count;
  // batched gradient: the twelve variants of every slice in one launch sequence
  DevBuf<float> regv, tmpv, matv, simv, sumBv, momv;   // [36][ns][H][W] x 2, [12][ns][16], [12][ns], [36][ns], [36][ns][3]
  DevBuf<int> cntBv;
  DevBuf<long long> dctr;                                                          // [5] device part of `counters` (blind line-search steps); [4]: ls_max
  int red_threads = 0;                                                             // 0: by image size; 256 / 1024 (option reg_red_threads, tests)
  int batch_state = 0;                                                             // 0 not tried, 1 ready, -1 no memory: literal sequence
  DevBuf<float> sumA, sumB, mom, half;                                             // [ns], [3][ns], [3][ns][3], [8][32]
  DevBuf<int> cntA, cntB;
  bool have_slices = false, have_ofs = false, prepared = false;
  int levels = 2, steps = 4, iterations = 20;
  float epsilon = 0.0001f;
  float blurring[8], length_of_steps[8];
  int klen[8];
  long long counters[4] = {0, 0, 0, 0};
  // svr_reg_get: the length of the active list the last evaluation / run left, and the most slices any line-search step of
  // the last run kept
  int last_active = 0, ls_max = 0;
  int red_used = 0;                                                                // the workgroup size the per-image reductions last ran with
};

struct RegVol {
  const float *vol;
  int vx, vy, vz;
  float W2I[12];
};

__device__ __forceinline__ void reg_matvec(const float *M, float x, float y, float z, float &a, float &b, float &c) {
  a = M[0] * x + M[1] * y + M[2] * z + M[3];     // RVH:134-145, literal order
  b = M[4] * x + M[5] * y + M[6] * z + M[7];
  c = M[8] * x + M[9] * y + M[10] * z + M[11];
}

__device__ __forceinline__ float reg_fetch(const RegVol &v, int x, int y, int z) {   // cudaAddressModeBorder
  if (x < 0 || y < 0 || z < 0 || x >= v.vx || y >= v.vy || z >= v.vz) return 0.0f;
  return v.vol[(size_t)x + (size_t)y * v.vx + (size_t)z * v.vx * v.vy];
}

__device__ __forceinline__ void reg_tex_axis(float p, float n, int &i, float &a) {
  const float u = p / n;               // normalised coordinate handed to tex3D (RC.cu:3525)
  const float xb = u * n - 0.5f;       // CUDA linear filtering: xB = N*u - 0.5
  const float fl = floorf(xb);
  const float fr = xb - fl;
  i = (int)fl;
  a = floorf(fr * 256.0f + 0.5f) / 256.0f;   // 8 fractional bits
}

// tex3D(reconstructedTex_, ...) with cudaFilterModeLinear, normalised coordinates, border 0
__device__ __forceinline__ float reg_tex3d(const RegVol &v, float px, float py, float pz) {
  int i, j, k;
  float a, b, c;
  reg_tex_axis(px, (float)v.vx, i, a);
  reg_tex_axis(py, (float)v.vy, j, b);
  reg_tex_axis(pz, (float)v.vz, k, c);
  const float oa = 1.0f - a, ob = 1.0f - b, oc = 1.0f - c;
  float t = oa * ob * oc * reg_fetch(v, i, j, k);
  t = t + a * ob * oc * reg_fetch(v, i + 1, j, k);
  t = t + oa * b * oc * reg_fetch(v, i, j + 1, k);
  t = t + a * b * oc * reg_fetch(v, i + 1, j + 1, k);
  t = t + oa * ob * c * reg_fetch(v, i, j, k + 1);
  t = t + a * ob * c * reg_fetch(v, i + 1, j, k + 1);
  t = t + oa * b * c * reg_fetch(v, i, j + 1, k + 1);
  t = t + a * b * c * reg_fetch(v, i + 1, j + 1, k + 1);
  return t;
}

// genenerateRegistrationSlices RC.cu:3504-3529, the three through-plane offsets in grid z
// blockIdx.z = 3 * variant + offset: the batched gradient (reg_evaluate_variants) samples the twelve central-difference
// matrices of every slice in one launch, variant v reading mat + v * mat_var_stride; a plain evaluation has gridDim.z = 3
__global__ void k_reg_generate(RegVol v, const int *active, const float *ofs, const float *mat, float *reg, int W,
                               int H, int ns, size_t mat_var_stride, const int *cnt) {
  const int pix = blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= W * H) return;
  const int slot = blockIdx.y, o = blockIdx.z % 3;
  if (cnt && slot >= *cnt) return;                       // blind line-search steps: the active count lives on the device
  mat += (size_t)(blockIdx.z / 3) * mat_var_stride;
  const int sl = active[slot];
  const int x = pix % W, y = pix / W;
  float wx, wy, wz, tx, ty, tz, vx, vy, vz;
  reg_matvec(ofs + 16 * (size_t)sl, (float)x, (float)y, (float)((o - 1) * 2), wx, wy, wz);
  reg_matvec(mat + 16 * (size_t)sl, wx, wy, wz, tx, ty, tz);
  reg_matvec(v.W2I, tx, ty, tz, vx, vy, vz);
  float val = reg_tex3d(v, vx, vy, vz);
  if (val < 0) val = -1.0f;
  reg[((size_t)blockIdx.z * ns + slot) * (size_t)W * H + pix] = val;
}

__device__ __forceinline__ float reg_max0(float v) { return v > 0.0f ? v : 0.0f; }

// GaussXKernel / GaussYKernel GF.cu:92-173.  layer = blockIdx.z * layer_stride + blockIdx.y
// ZERO: the patch-based variant (GPUGauss/patchBasedGaussfilter.cu:88-190), where a neighbour outside the image contributes 0
// instead of the clamped edge pixel
template <bool YDIR, bool ZERO = false>
__global__ void k_reg_blur(const float *in, float *out, int W, int H, int layer_stride, const float *half, int nh, const int *cnt = nullptr) {
  const int pix = blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= W * H) return;
  if (cnt && (int)blockIdx.y >= *cnt) return;
  const size_t base = ((size_t)blockIdx.z * layer_stride + blockIdx.y) * (size_t)W * H;
  const int x = pix % W, y = pix / W;
  float v = in[base + pix];
  if (v != -1) {
    v = v * half[0];
    for (int i = 1; i < nh; ++i) {
      float p, m;
      if (YDIR) {
        p = in[base + (size_t)min(y + i, H - 1) * W + x];
        m = in[base + (size_t)max(y - i, 0) * W + x];
      } else {
        p = in[base + (size_t)y * W + min(x + i, W - 1)];
        m = in[base + (size_t)y * W + max(x - i, 0)];
      }
      if (ZERO) {
        if (YDIR) { if (y + i >= H) p = 0.0f; if (y - i < 0) m = 0.0f; }
        else { if (x + i >= W) p = 0.0f; if (x - i < 0) m = 0.0f; }
      }
      v = v + half[i] * (reg_max0(p) + reg_max0(m));
    }
  }
  out[base + pix] = v;
}

__device__ __forceinline__ double reg_block_sum(double v, double *sh) {   // blockDim.x = 256 or 1024 threads, fixed tree (sh: one double per wavefront)
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  double t = sh[0];
  for (int k = 1; k < nw; ++k) t += sh[k];
  return t;
}

// averageIf RC.cu:4459-4496: sum and count of values > -1 of one layer per workgroup.
// layer = (active ? active[blockIdx.x] : blockIdx.x) + blockIdx.y * layer_stride; out index = blockIdx.y * out_stride + blockIdx.x
__global__ __launch_bounds__(1024) void k_reg_sums(const float *layers, const int *active, int layer_stride, int wh,
                                                    float *sum, int *count, int out_stride, const int *cnt = nullptr) {
  __shared__ double sh[16];
  __shared__ int shc[16];
  if (cnt && (int)blockIdx.x >= *cnt) return;
  const int sl = active ? active[blockIdx.x] : blockIdx.x;
  const float *p = layers + ((size_t)blockIdx.y * layer_stride + sl) * (size_t)wh;
  double acc = 0;
  int c = 0;
  for (int i = threadIdx.x; i < wh; i += blockDim.x) {
    const float v = p[i];
    if (v > -1.0f) { ++c; acc += (double)v; }
  }
  for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
  if ((threadIdx.x & 63) == 0) shc[threadIdx.x >> 6] = c;
  const double s = reg_block_sum(acc, sh);
  if (threadIdx.x == 0) {
    int ct = 0;
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) ct += shc[k];
    sum[(size_t)blockIdx.y * out_stride + blockIdx.x] = (float)s;
    count[(size_t)blockIdx.y * out_stride + blockIdx.x] = ct;
  }
}

// computeNCCAndReduce RC.cu:4498-4550 for (slot = blockIdx.x, offset = blockIdx.y); the sampled-slice
// mean is the running mean over offsets <= o (sums are not reset between offsets, RC.cu:4195)
__global__ __launch_bounds__(1024) void k_reg_ncc(const float *target, const int *active, const float *reg,
                                                  const float *sumA, const int *cntA, const float *sumB,
                                                  const int *cntB, float *mom, int wh, int ns, int lv, const int *cnt = nullptr) {
  __shared__ double sh[16];
  const int slot = blockIdx.x, o = blockIdx.y;
  if (cnt && slot >= *cnt) return;
  const size_t var = blockIdx.z;                         // batched gradient: the variant's block of [3][ns] layers
  sumB += var * 3 * ns; cntB += var * 3 * ns; reg += var * 3 * ns * (size_t)wh; mom += var * 9 * ns;
  const int sl = active[slot];
  float avg_a = sumA[sl], avg_b = 0.0f;
  int cb = 0;
  for (int k = 0; k <= o; ++k) { avg_b = avg_b + sumB[(size_t)k * ns + slot]; cb += cntB[(size_t)k * ns + slot]; }
  if (avg_a != 0) avg_a /= cntA[sl];
  if (avg_b != 0) avg_b /= cb;
  const float *A = target + (size_t)sl * wh, *B = reg + ((size_t)o * ns + slot) * (size_t)wh;
  double m0 = 0, m1 = 0, m2 = 0;
  for (int lin = threadIdx.x; lin < wh; lin += blockDim.x) {
    const float va = A[lin], vb = B[lin];
    if (va >= 0.0f && vb >= 0.0f && lin % lv == 0) {
      const float sa = va - avg_a, sb = vb - avg_b;
      m0 += (double)(sa * sb);
      m1 += (double)(sa * sa);
      m2 += (double)(sb * sb);
    }
  }
  m0 = reg_block_sum(m0, sh);
  m1 = reg_block_sum(m1, sh);
  m2 = reg_block_sum(m2, sh);
  if (threadIdx.x == 0) {
    float *R = mom + ((size_t)o * ns + slot) * 3;
    R[0] = (float)m0; R[1] = (float)m1; R[2] = (float)m2;
  }
}

// addNccValues + writeSimilarities RC.cu:4552-4575 with the literal effect of the
// memset(dev_temp_float + 2*slices, 0, 3*slices*sizeof(float)) of RC.cu:4200 on the buffer layout
// [2a,3a) = accumulated NCC, [3a,6a) = moments (a = active slices, s = slices).
__global__ void k_reg_combine(const float *mom, const int *active, float *sim, int a, int s, int writeoffset,
                              int writestep, int writenum, float *simv, const int *cnt = nullptr) {
  const int slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (cnt) a = *cnt;                                     // (the aliasing rule below depends on the number of active slices)
  if (slot >= a) return;
  mom += (size_t)blockIdx.y * 9 * s;                     // batched gradient: variant blockIdx.y, its similarity goes to simv
  float acc = 0.0f, R[3] = {0.0f, 0.0f, 0.0f};
  for (int o = 0; o < 3; ++o) {
    const int ia = 2 * a + slot;
    if (ia >= 2 * s && ia < 5 * s) acc = 0.0f;
    for (int k = 0; k < 3; ++k) {
      const int ir = 3 * a + 3 * slot + k;
      if (ir >= 2 * s && ir < 5 * s) R[k] = 0.0f;
      R[k] = R[k] + mom[((size_t)o * s + slot) * 3 + k];
    }
    const float norm = R[1] * R[2];
    float res = 0.0f;
    if (norm > 0) res = R[0] / sqrtf(norm);
    acc += res;
  }
  const int sl = active[slot];
  if (simv) { simv[(size_t)blockIdx.y * s + sl] = acc; return; }
  for (int i = 0; i < writenum; ++i) sim[(size_t)writeoffset * s + (size_t)s * writestep * i + sl] = acc;
}

// per-slice trigonometry in double, rounded to float (bit-reproducible on host and device)
__device__ __forceinline__ float reg_sin(float x) { return (float)sin((double)x); }
__device__ __forceinline__ float reg_cos(float x) { return (float)cos((double)x); }
__device__ __forceinline__ float reg_asin(float x) { return (float)asin((double)x); }
__device__ __forceinline__ float reg_atan2(float y, float x) { return (float)atan2((double)y, (double)x); }

__device__ void reg_euler_of(const float *m, float p_rot[3]) {      // RC.cu:4254-4269
  const float TOL = 0.000001f;
  const float tmp = reg_asin(-1.0f * m[2]);
  if (fabsf(reg_cos(tmp)) > TOL) {
    p_rot[0] = reg_atan2(m[6], m[10]);
    p_rot[1] = tmp;
    p_rot[2] = reg_atan2(m[1], m[0]);
  } else {
    p_rot[0] = reg_atan2(-m[2] * m[4], -m[2] * m[8]);
    p_rot[1] = tmp;
    p_rot[2] = 0;
  }
}

__device__ void reg_rot_of(const float p_rot[3], float *m) {        // RC.cu:4274-4291
  const float cosrx = reg_cos(p_rot[0]), cosry = reg_cos(p_rot[1]), cosrz = reg_cos(p_rot[2]);
  const float sinrx = reg_sin(p_rot[0]), sinry = reg_sin(p_rot[1]), sinrz = reg_sin(p_rot[2]);
  m[0] = cosry * cosrz;
  m[1] = cosry * sinrz;
  m[2] = -sinry;
  m[4] = (sinrx * sinry * cosrz - cosrx * sinrz);
  m[5] = (sinrx * sinry * sinrz + cosrx * cosrz);
  m[6] = sinrx * cosry;
  m[8] = (cosrx * sinry * cosrz + sinrx * sinrz);
  m[9] = (cosrx * sinry * sinrz - sinrx * cosrz);
  m[10] = cosrx * cosry;
}

// adjustSamplingMatrixForCentralDifferences RC.cu:4231-4293, one slice
__device__ void reg_adjust_one(const float *in, float *out, int part, float step) {
  const float pi = 3.14159265358979323846f;
  float m[16];
  for (int k = 0; k < 16; ++k) m[k] = in[k];
  if (part < 3) {
    m[4 * part + 3] = in[4 * part + 3] + step;
  } else {
    float p_rot[3];
    reg_euler_of(in, p_rot);
    p_rot[part - 3] += step * pi / 180.0f;
    reg_rot_of(p_rot, m);
  }
  for (int k = 0; k < 16; ++k) out[k] = m[k];
}

__global__ void k_reg_adjust(const float *in_m, float *out_m, const int *active, int a, int part, float step) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a) return;
  const int sl = active[i];
  reg_adjust_one(in_m + 16 * (size_t)sl, out_m + 16 * (size_t)sl, part, step);
}

// computeGradientCentralDiff RC.cu:4295-4308 (rows 3 and 4 of the similarity table)
__global__ void k_reg_grad(const float *sim, float *grad, const int *active, int a, int s, int p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a) return;
  const int sl = active[i];
  const float dx = sim[3 * (size_t)s + sl] - sim[4 * (size_t)s + sl];
  grad[(size_t)p * s + sl] = dx;
  if (p == 0) grad[6 * (size_t)s + sl] = dx * dx;
  else grad[6 * (size_t)s + sl] += dx * dx;
}

// normalizeGradient RC.cu:4309-4323
__global__ void k_reg_normalize(float *grad, const int *active, int a, int s) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a) return;
  const int sl = active[i];
  float norm = grad[6 * (size_t)s + sl];
  if (norm > 0) norm = 1.0f / sqrtf(norm);
  for (int j = 0; j < 6; ++j) grad[(size_t)j * s + sl] *= norm;
}

// The twelve matrices of a central-difference gradient at once: variant 2p = parameter p + step, 2p + 1 = parameter p - step
// (k_reg_adjust from mat_orig, as the literal loop calls it twelve times)
__global__ void k_reg_variants(const float *in_m, float *matv, const int *active, int a, int s, float step) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, var = blockIdx.y;
  if (i >= a) return;
  const int sl = active[i];
  reg_adjust_one(in_m + 16 * (size_t)sl, matv + ((size_t)var * s + sl) * 16, var >> 1, (var & 1) ? -step : step);
}

// k_reg_grad for p = 0..5 + k_reg_normalize from the similarities of the twelve variants, and what the literal loop leaves
// behind: rows 3 / 4 of the similarity table hold the last pair, the working matrix is the last variant (rz - step)
__global__ void k_reg_grad_all(const float *simv, float *sim, float *grad, const float *matv, float *mat, const int *active, int a, int s) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a) return;
  const int sl = active[i];
  for (int p = 0; p < 6; ++p) {
    const float sp = simv[(size_t)(2 * p) * s + sl], sm = simv[(size_t)(2 * p + 1) * s + sl];
    sim[3 * (size_t)s + sl] = sp; sim[4 * (size_t)s + sl] = sm;
    const float dx = sp - sm;
    grad[(size_t)p * s + sl] = dx;
    if (p == 0) grad[6 * (size_t)s + sl] = dx * dx;
    else grad[6 * (size_t)s + sl] += dx * dx;
  }
  float norm = grad[6 * (size_t)s + sl];
  if (norm > 0) norm = 1.0f / sqrtf(norm);
  for (int j = 0; j < 6; ++j) grad[(size_t)j * s + sl] *= norm;
  for (int k = 0; k < 16; ++k) mat[16 * (size_t)sl + k] = matv[((size_t)11 * s + sl) * 16 + k];
}

// copySimilarity RC.cu:4326-4333
__global__ void k_reg_copy_sim(float *sim, const int *active, int a, int s, int target, int source) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a) return;
  const int sl = active[i];
  sim[(size_t)target * s + sl] = sim[(size_t)source * s + sl];
}

// gradientStep RC.cu:4335-4391, one slice
__device__ void reg_step_one(float *m, const float *grad, int sl, int s, float step) {
  const float pi = 3.14159265358979323846f;
  for (int p = 0; p < 3; ++p) m[4 * p + 3] = m[4 * p + 3] + step * grad[(size_t)p * s + sl];
  float p_rot[3];
  reg_euler_of(m, p_rot);
  for (int p = 0; p < 3; ++p) p_rot[p] += grad[(size_t)(p + 3) * s + sl] * step * pi / 180.0f;
  float r[16];
  reg_rot_of(p_rot, r);
  m[0] = r[0]; m[1] = r[1]; m[2] = r[2];
  m[4] = r[4]; m[5] = r[5]; m[6] = r[6];
  m[8] = r[8]; m[9] = r[9]; m[10] = r[10];
}

__global__ void k_reg_step(float *mats, const float *grad, const int *active, int a, int s, float step) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a) return;
  const int sl = active[i];
  reg_step_one(mats + 16 * (size_t)sl, grad, sl, s, step);
}

// checkImprovement RC.cu:4393-4457: stable compaction of the slices whose similarity improved by
// more than eps; one workgroup of 1024 walks the list in chunks of 1024 (order-preserving for any size); the new count comes
// back in every lane
__device__ int reg_compact(int *new_mask, const int *mask, int n, int s, const float *sim, int cursim, int prev, float eps) {
  __shared__ int wave_tot[16];
  __shared__ int base;
  __syncthreads();
  if (threadIdx.x == 0) base = 0;
  __syncthreads();
  for (int start = 0; start < n; start += 1024) {
    const int i = start + threadIdx.x;
    int sl = -1, act = 0;
    if (i < n) {
      sl = mask[i];
      act = sim[(size_t)cursim * s + sl] > sim[(size_t)prev * s + sl] + eps ? 1 : 0;
    }
    const unsigned long long b = __ballot(act);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int before = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) wave_tot[w] = __popcll(b);
    __syncthreads();
    int off = base;
    for (int k = 0; k < w; ++k) off += wave_tot[k];
    if (act) new_mask[off + before] = sl;
    __syncthreads();
    if (threadIdx.x == 0) {
      int t = 0;
      for (int k = 0; k < 16; ++k) t += wave_tot[k];
      base += t;
    }
    __syncthreads();
  }
  return base;
}

__global__ __launch_bounds__(1024) void k_reg_check(int *new_mask, const int *mask, int n, int s, const float *sim,
                                                     int cursim, int prev, float eps, int *count) {
  const int c = reg_compact(new_mask, mask, n, s, sim, cursim, prev, eps);
  if (threadIdx.x == 0) *count = c;
}

__global__ void k_reg_set_count(int *count, int v) { *count = v; }

// One line-search step's bookkeeping with the active count on the device (blind steps): checkImprovement of the step just
// evaluated, then copySimilarity + gradientStep for the slices that go on (what the literal loop does at the top of its
// next pass).  A step whose count is already 0 does nothing, like the loop that would not have run it.
__global__ __launch_bounds__(1024) void k_reg_line_check(int *new_mask, const int *mask, int s, float *sim, float eps, int *count, float *mats,
                                                          const float *grad, float step, long long *dctr) {
  const int n = *count;
  if (n == 0) return;
  const int c = reg_compact(new_mask, mask, n, s, sim, 0, 2, eps);
  if (threadIdx.x == 0) { *count = c; dctr[0] += 1; dctr[1] += 1; dctr[3] += n; if (c > dctr[4]) dctr[4] = c; }
  __syncthreads();
  for (int i = threadIdx.x; i < c; i += 1024) {
    const int sl = new_mask[i];
    sim[2 * (size_t)s + sl] = sim[sl];                   // k_reg_copy_sim(2 <- 0)
    reg_step_one(mats + 16 * (size_t)sl, grad, sl, s, step);
  }
}

__global__ void k_reg_iota(int *buf, int n) {      // initActiveSlices RC.cu:4224-4229
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) buf[i] = i;
}

// computeCCpatch (R2/patchBased2D3DRegistration_gpu2.cu:130-190): raw-moment NCC of one patch of the slice
// grid against the volume through the software trilinear `interp` of R2/include/interpFunctions.cuh:81-96,
// through-plane offsets z = -1, 0, 1, every (level+1)-th pixel.  One workgroup per patch, double sums.
__device__ __forceinline__ float cc_vol(const RegVol &v, int x, int y, int z) {
  if ((unsigned)x < (unsigned)v.vx && (unsigned)y < (unsigned)v.vy && (unsigned)z < (unsigned)v.vz)
    return v.vol[(size_t)x + (size_t)y * v.vx + (size_t)z * v.vx * v.vy];
  return 0.0f;
}
__device__ __forceinline__ float cc_interp(const RegVol &v, float px, float py, float pz) {
  const float flx = floorf(px), fly = floorf(py), flz = floorf(pz);
  const float fx = px - flx, fy = py - fly, fz = pz - flz;
  const int bx = (int)flx, by = (int)fly, bz = (int)flz;
  const int lx = max(bx, 0), ly = max(by, 0), lz = max(bz, 0);            // lower = max(base, 0)
  const int ux = min(bx + 1, v.vx - 1), uy = min(by + 1, v.vy - 1), uz = min(bz + 1, v.vz - 1);
  return cc_vol(v, lx, ly, lz) * (1 - fx) * (1 - fy) * (1 - fz)
       + cc_vol(v, ux, ly, lz) * fx * (1 - fy) * (1 - fz)
       + cc_vol(v, lx, uy, lz) * (1 - fx) * fy * (1 - fz)
       + cc_vol(v, ux, uy, lz) * fx * fy * (1 - fz)
       + cc_vol(v, lx, ly, uz) * (1 - fx) * (1 - fy) * fz
       + cc_vol(v, ux, ly, uz) * fx * (1 - fy) * fz
       + cc_vol(v, lx, uy, uz) * (1 - fx) * fy * fz
       + cc_vol(v, ux, uy, uz) * fx * fy * fz;
}
__global__ __launch_bounds__(256) void k_cc_patch(RegVol v, const float *buffer, int px, int py, const float *M,
                                                   int level, double *sums6) {
  __shared__ double sh[4];
  const int patch = blockIdx.x;
  const float *m = M + 16 * (size_t)patch;
  const float *buf = buffer + (size_t)patch * px * py;
  const int st = level + 1;
  const int nx = (px + st - 1) / st, ny = (py + st - 1) / st;
  double acc[6] = {0, 0, 0, 0, 0, 0};
  for (int i = threadIdx.x; i < nx * ny * 3; i += 256) {
    const int z = i % 3 - 1, r = i / 3;
    const int x = (r % nx) * st, y = (r / nx) * st;
    const float a = buf[y * px + x];
    float wx, wy, wz, vx, vy, vz;
    reg_matvec(m, (float)x, (float)y, (float)z, wx, wy, wz);
    reg_matvec(v.W2I, wx, wy, wz, vx, vy, vz);
    const float b = cc_interp(v, vx, vy, vz);
    if (a >= 0.0f && b >= 0.0f && a == a && b == b) {
      acc[0] += 1.0; acc[1] += (double)a; acc[2] += (double)b;
      acc[3] += (double)(a * a); acc[4] += (double)(b * b); acc[5] += (double)(a * b);
    }
  }
  for (int k = 0; k < 6; ++k) {
    const double t = reg_block_sum(acc[k], sh);
    if (threadIdx.x == 0) sums6[6 * (size_t)patch + k] = t;
  }
}

// ---- patch-to-volume registration of the patch-based path (R2/patchBased2D3DRegistration_gpu2.cu) ---------------------
// Matrix2Parameters / Parameters2Matrix of R2/include/matrix4.cuh:189-260 (T = float): the inverse functions are float
// calls there (asinf, cosf, atan2f of CUDA, not reproducible elsewhere), the forward ones double calls on float x (pi/180)
// rounded to float; both are taken here as the correctly rounded float of the double function.
__device__ void pvr_m2p(const float *m, float p[6]) {
  const float TOL = 0.000001f;
  p[0] = m[3]; p[1] = m[7]; p[2] = m[11];
  const float tmp = reg_asin(-1.0f * m[2]);
  if (fabsf(reg_cos(tmp)) > TOL) {
    p[3] = reg_atan2(m[6], m[10]);
    p[4] = tmp;
    p[5] = reg_atan2(m[1], m[0]);
  } else {
    p[3] = reg_atan2(-1.0f * m[2] * m[4], -1.0f * m[2] * m[8]);
    p[4] = tmp;
    p[5] = 0;
  }
  for (int k = 3; k < 6; ++k) p[k] = (float)((double)p[k] * (180.0 / 3.14159265358979323846));
}
__device__ void pvr_p2m(const float p[6], float *m) {
  const double k = 3.14159265358979323846 / 180.0;
  const float cosrx = (float)cos((double)p[3] * k), cosry = (float)cos((double)p[4] * k), cosrz = (float)cos((double)p[5] * k);
  const float sinrx = (float)sin((double)p[3] * k), sinry = (float)sin((double)p[4] * k), sinrz = (float)sin((double)p[5] * k);
  m[0] = cosry * cosrz; m[1] = cosry * sinrz; m[2] = -sinry; m[3] = p[0];
  m[4] = (sinrx * sinry * cosrz - cosrx * sinrz); m[5] = (sinrx * sinry * sinrz + cosrx * cosrz); m[6] = sinrx * cosry; m[7] = p[1];
  m[8] = (cosrx * sinry * cosrz + sinrx * sinrz); m[9] = (cosrx * sinry * sinrz - sinrx * cosrz); m[10] = cosrx * cosry; m[11] = p[2];
  m[12] = 0; m[13] = 0; m[14] = 0; m[15] = 1.0f;
}

// computeCCpatch for the workgroup's patch with the matrix cur * RI2W; the value is returned to every thread
__device__ float pvr_block_cc(const RegVol &v, const float *buf, int px, int py, const float *cur, const float *ri2w, int level,
                              float *shM, double *sh, float *shv) {
  __syncthreads();
  if (threadIdx.x < 16) {                                   // Tmat * patch.RI2W (:152), the product order of matmul4
    const int i = threadIdx.x >> 2, j = threadIdx.x & 3;
    shM[threadIdx.x] = cur[4 * i] * ri2w[j] + cur[4 * i + 1] * ri2w[4 + j] + cur[4 * i + 2] * ri2w[8 + j] + cur[4 * i + 3] * ri2w[12 + j];
  }
  __syncthreads();
  const int st = level + 1;
  const int nx = (px + st - 1) / st, ny = (py + st - 1) / st;
  double acc[6] = {0, 0, 0, 0, 0, 0};
  for (int i = threadIdx.x; i < nx * ny * 3; i += 256) {
    const int z = i % 3 - 1, r = i / 3;
    const int x = (r % nx) * st, y = (r / nx) * st;
    const float a = buf[y * px + x];
    float wx, wy, wz, vx, vy, vz;
    reg_matvec(shM, (float)x, (float)y, (float)z, wx, wy, wz);
    reg_matvec(v.W2I, wx, wy, wz, vx, vy, vz);
    const float b = cc_interp(v, vx, vy, vz);
    if (a >= 0.0f && b >= 0.0f && a == a && b == b) {
      acc[0] += 1.0; acc[1] += (double)a; acc[2] += (double)b;
      acc[3] += (double)(a * a); acc[4] += (double)(b * b); acc[5] += (double)(a * b);
    }
  }
  double s[6];
  for (int k = 0; k < 6; ++k) s[k] = reg_block_sum(acc[k], sh);
  if (threadIdx.x == 0) {
    const float cnt = (float)s[0], x = (float)s[1], y = (float)s[2], x2 = (float)s[3], y2 = (float)s[4], xy = (float)s[5];
    *shv = s[0] > 0 ? (xy - (x * y) / cnt) / (sqrtf(x2 - x * x / cnt) * sqrtf(y2 - y * y / cnt)) : 0.0f;
  }
  __syncthreads();
  return *shv;
}

// parallelPatchRegOptimization (:198-291): one gradient-ascent run of one patch -- central differences over the six rigid
// parameters, then steps along the normalised gradient while the similarity grows (at most 50), then one step back.  The
// reference runs it in ONE THREAD per patch (3 x 1024 samples per evaluation, >= 14 evaluations, sequentially); here a
// workgroup shares every evaluation and thread 0 carries the parameters.  evals[patch] += evaluations made.
__global__ __launch_bounds__(256) void k_pvr_patch_opt(RegVol v, const float *buffer, int px, int py, const float *RI2W, float *mats,
                                                        int level, float step, int *evals) {
  __shared__ float shM[16], cur[16], ri2w[16], params[6], dxt[6], shv;
  __shared__ double sh[4];
  __shared__ int go;
  const int patch = blockIdx.x;
  const float *buf = buffer + (size_t)patch * px * py;
  float *mat = mats + 16 * (size_t)patch;
  if (threadIdx.x < 16) { cur[threadIdx.x] = mat[threadIdx.x]; ri2w[threadIdx.x] = RI2W[16 * (size_t)patch + threadIdx.x]; }
  __syncthreads();
  if (threadIdx.x == 0) pvr_m2p(cur, params);
  int n_eval = 0;
  for (int i = 0; i < 6; ++i) {
    float pv = 0;
    if (threadIdx.x == 0) { pv = params[i]; params[i] = pv + step; pvr_p2m(params, cur); }
    const float s1 = pvr_block_cc(v, buf, px, py, cur, ri2w, level, shM, sh, &shv);
    if (threadIdx.x == 0) { params[i] = pv - step; pvr_p2m(params, cur); }
    const float s2 = pvr_block_cc(v, buf, px, py, cur, ri2w, level, shM, sh, &shv);
    if (threadIdx.x == 0) { dxt[i] = s1 - s2; params[i] = pv; pvr_p2m(params, cur); }
    n_eval += 2;
  }
  if (threadIdx.x == 0) {
    float norm = 0;
    for (int i = 0; i < 6; ++i) norm += dxt[i] * dxt[i];
    norm = sqrtf(norm);
    for (int i = 0; i < 6; ++i) dxt[i] = norm > 0.0f ? dxt[i] / norm : 0.0f;
  }
  float similarity = pvr_block_cc(v, buf, px, py, cur, ri2w, level, shM, sh, &shv);
  float new_similarity = similarity;
  int count = 0;
  n_eval += 1;
  do {
    new_similarity = similarity;
    if (threadIdx.x == 0) {
      for (int i = 0; i < 6; ++i) params[i] = params[i] + step * dxt[i];
      pvr_p2m(params, cur);
    }
    similarity = pvr_block_cc(v, buf, px, py, cur, ri2w, level, shM, sh, &shv);
    count++;
    n_eval += 1;
    if (threadIdx.x == 0) go = (similarity > new_similarity + 0.0001f && count < 50) ? 1 : 0;
    __syncthreads();
  } while (go);
  if (threadIdx.x == 0) {                                   // last step was no improvement, so back track
    for (int i = 0; i < 6; ++i) params[i] = params[i] - step * dxt[i];
    pvr_p2m(params, cur);
    evals[patch] += n_eval;
  }
  __syncthreads();
  if (threadIdx.x < 16) mat[threadIdx.x] = cur[threadIdx.x];
}

namespace {

// inverse of a 4x4 in double (Gauss-Jordan with partial pivoting)
void invert4d(const double *a, double *out) {
  double w[4][8];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) { w[i][j] = a[4 * i + j]; w[i][4 + j] = (i == j) ? 1.0 : 0.0; }
  for (int c = 0; c < 4; ++c) {
    int p = c;
    for (int r = c + 1; r < 4; ++r) if (fabs(w[r][c]) > fabs(w[p][c])) p = r;
    for (int j = 0; j < 8; ++j) { const double t = w[c][j]; w[c][j] = w[p][j]; w[p][j] = t; }
    const double d = w[c][c];
    for (int j = 0; j < 8; ++j) w[c][j] /= d;
    for (int r = 0; r < 4; ++r)
      if (r != c) { const double f = w[r][c]; for (int j = 0; j < 8; ++j) w[r][j] -= f * w[c][j]; }
  }
  for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) out[4 * i + j] = w[i][4 + j];
}

void reg_free(RegState *r) { delete r; }

// generateGaussianKernel + the length rule of FilterGaussStack (GF.cu:56-87,195-196)
int reg_gauss_kernel(float sigma, float *half) {
  int klength = (int)(sigma * 5);
  if (klength > 64 - 1) klength = 64 - 1;
  if (klength < 7) klength = 7;
  klength -= 1 - klength % 2;
  float k[64];
  float sum = 0;
  const int mid = klength / 2;
  for (int i = 0; i < klength; ++i) {
    const int d = abs(i - mid);
    k[i] = expf(-(float)d * (float)d / (2 * sigma * sigma));
    sum += k[i];
  }
  for (int i = 0; i < klength; ++i) k[i] /= sum;
  for (int i = 0; i < (klength + 1) / 2; ++i) half[i] = k[mid + i];
  return klength;
}

RegVol reg_vol(svr_ctx *ctx) {
  RegVol v;
  v.vol = ctx->reg->vol;
  v.vx = (int)ctx->vx; v.vy = (int)ctx->vy; v.vz = (int)ctx->vz;
  memcpy(v.W2I, ctx->reconW2I, 12 * sizeof(float));
  return v;
}

// Workgroup size of the per-image reductions (k_reg_sums, k_reg_ncc): one workgroup walks a whole image, so its latency is
// pixels / lanes dependent steps; images beyond 4096 pixels take 1024 lanes (the fixed tree has 16 leaves then instead of 4)
inline int reg_red_threads(const RegState *r) { return r->red_threads ? r->red_threads : r->wh > 4096 ? 1024 : 256; }

// FilterGaussStack on `n` layers starting at `img` (in place through r->tmp)
int reg_blur_layers(svr_ctx *ctx, float *img, int n, int groups, int level, const int *cnt = nullptr) {
  RegState *r = ctx->reg;
  if (n == 0) return SVR_OK;
  const int nh = (r->klen[level] + 1) / 2;
  const dim3 grid(nblk(r->wh), n, groups);
  hipLaunchKernelGGL(k_reg_blur<false>, grid, dim3(256), 0, ctx->stream, img, r->tmp, r->W, r->H, r->ns,
                     r->half + 32 * level, nh, cnt);
  hipLaunchKernelGGL(k_reg_blur<true>, grid, dim3(256), 0, ctx->stream, r->tmp, img, r->W, r->H, r->ns,
                     r->half + 32 * level, nh, cnt);
  KCHK("k_reg_blur");
  return SVR_OK;
}

// start of a level (RC.cu:4016-4026): blurred copy of the resampled slices + their sums
int reg_begin_level(svr_ctx *ctx, int level) {
  RegState *r = ctx->reg;
  HIPCHK(hipMemcpyAsync(r->target, r->resampled, (size_t)r->ns * r->wh * sizeof(float), hipMemcpyDeviceToDevice,
                        ctx->stream));
  int rc = reg_blur_layers(ctx, r->target, r->ns, 1, level);
  if (rc) return rc;
  r->red_used = reg_red_threads(r);
  hipLaunchKernelGGL(k_reg_sums, dim3(r->ns, 1), dim3(reg_red_threads(r)), 0, ctx->stream, r->target, (const int *)nullptr, r->ns,
                     (int)r->wh, r->sumA, r->cntA, r->ns);
  KCHK("k_reg_sums(target)");
  return SVR_OK;
}

// evaluateCostsMultipleSlices RC.cu:4150-4221
// cnt: the active count on the device (blind line-search steps); `a` is then an upper bound that sizes the grids, the
// kernels take the slots below *cnt, and the evaluation is counted on the device (k_reg_line_check)
int reg_evaluate(svr_ctx *ctx, int a, int level, int writeoffset, int writestep, int writenum, const int *cnt = nullptr) {
  RegState *r = ctx->reg;
  if (a == 0) return SVR_OK;
  if (!cnt) {
    r->counters[0] += 1;
    r->counters[3] += a;
  }
  hipLaunchKernelGGL(k_reg_generate, dim3(nblk(r->wh), a, 3), dim3(256), 0, ctx->stream, reg_vol(ctx), r->active, r->ofs,
                     r->mat, r->reg, r->W, r->H, r->ns, (size_t)0, cnt);
  KCHK("k_reg_generate");
  int rc = reg_blur_layers(ctx, r->reg, a, 3, level, cnt);
  if (rc) return rc;
  hipLaunchKernelGGL(k_reg_sums, dim3(a, 3), dim3(reg_red_threads(r)), 0, ctx->stream, r->reg, (const int *)nullptr, r->ns, (int)r->wh,
                     r->sumB, r->cntB, r->ns, cnt);
  hipLaunchKernelGGL(k_reg_ncc, dim3(a, 3), dim3(reg_red_threads(r)), 0, ctx->stream, r->target, r->active, r->reg, r->sumA, r->cntA,
                     r->sumB, r->cntB, r->mom, (int)r->wh, r->ns, level + 1, cnt);
  hipLaunchKernelGGL(k_reg_combine, dim3(nblk(a)), dim3(256), 0, ctx->stream, r->mom, r->active, r->sim, a, r->ns,
                     writeoffset, writestep, writenum, (float *)nullptr, cnt);
  KCHK("k_reg_ncc");
  return SVR_OK;
}

// The twelve evaluateCostsMultipleSlices calls of one gradient (RC.cu:4060-4082) as one launch sequence: the same kernels
// with the variant as one more grid dimension, 36 layers per slice instead of 3.  Every evaluation is independent of the
// others (the state machine of k_reg_combine starts from zero in each), so the numbers are the literal loop's.
bool reg_batch_ready(svr_ctx *ctx) {
  RegState *r = ctx->reg;
  if (r->batch_state) return r->batch_state > 0;
  const size_t n = (size_t)36 * r->ns * r->wh;
  bool ok = r->regv.reserve(n) == hipSuccess && r->tmpv.reserve(n) == hipSuccess &&
            r->matv.reserve((size_t)12 * 16 * r->ns) == hipSuccess && r->simv.reserve((size_t)12 * r->ns) == hipSuccess &&
            r->sumBv.reserve((size_t)36 * r->ns) == hipSuccess && r->cntBv.reserve((size_t)36 * r->ns) == hipSuccess &&
            r->momv.reserve((size_t)108 * r->ns) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    r->regv.reset(); r->tmpv.reset(); r->matv.reset(); r->simv.reset(); r->sumBv.reset(); r->momv.reset(); r->cntBv.reset();
  }
  r->batch_state = ok ? 1 : -1;
  return ok;
}

int reg_evaluate_variants(svr_ctx *ctx, int a, int level, float step) {
  RegState *r = ctx->reg;
  if (a == 0) return SVR_OK;
  r->counters[0] += 12;
  r->counters[3] += 12LL * a;
  const int s = r->ns, nh = (r->klen[level] + 1) / 2;
  hipLaunchKernelGGL(k_reg_variants, dim3(nblk(a), 12), dim3(256), 0, ctx->stream, r->mat_orig, r->matv, r->active, a, s, step);
  hipLaunchKernelGGL(k_reg_generate, dim3(nblk(r->wh), a, 36), dim3(256), 0, ctx->stream, reg_vol(ctx), r->active, r->ofs,
                     r->matv, r->regv, r->W, r->H, s, (size_t)16 * s, (const int *)nullptr);
  KCHK("k_reg_generate(variants)");
  const dim3 grid(nblk(r->wh), a, 36);
  hipLaunchKernelGGL(k_reg_blur<false>, grid, dim3(256), 0, ctx->stream, r->regv, r->tmpv, r->W, r->H, s, r->half + 32 * level, nh);
  hipLaunchKernelGGL(k_reg_blur<true>, grid, dim3(256), 0, ctx->stream, r->tmpv, r->regv, r->W, r->H, s, r->half + 32 * level, nh);
  KCHK("k_reg_blur(variants)");
  hipLaunchKernelGGL(k_reg_sums, dim3(a, 36), dim3(reg_red_threads(r)), 0, ctx->stream, r->regv, (const int *)nullptr, s, (int)r->wh, r->sumBv, r->cntBv, s);
  hipLaunchKernelGGL(k_reg_ncc, dim3(a, 3, 12), dim3(reg_red_threads(r)), 0, ctx->stream, r->target, r->active, r->regv, r->sumA, r->cntA,
                     r->sumBv, r->cntBv, r->momv, (int)r->wh, s, level + 1);
  hipLaunchKernelGGL(k_reg_combine, dim3(nblk(a), 12), dim3(256), 0, ctx->stream, r->momv, r->active, r->sim, a, s, 0, 0, 0, r->simv);
  hipLaunchKernelGGL(k_reg_grad_all, dim3(nblk(a)), dim3(256), 0, ctx->stream, r->simv, r->sim, r->grad, r->matv, r->mat, r->active, a, s);
  KCHK("k_reg_grad_all");
  return SVR_OK;
}

int reg_check(svr_ctx *ctx, int *new_mask, const int *mask, int n, int cursim, int prev, int *out_count) {
  RegState *r = ctx->reg;
  hipLaunchKernelGGL(k_reg_check, dim3(1), dim3(1024), 0, ctx->stream, new_mask, mask, n, r->ns, r->sim, cursim, prev,
                     r->epsilon, r->count);
  KCHK("k_reg_check");
  HIPCHK(hipMemcpyAsync(out_count, r->count, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

}  // namespace

extern "C" {

int svr_init_reg_storage_volumes(svr_ctx *ctx, const uint32_t size[3], const float dim[3]) {
  SVR_ENTER(ctx);
  if (!ctx || !size) return SVR_E_ARG;
  (void)dim;
  if (size[0] == 0 || size[1] == 0 || size[2] == 0) return fail(ctx, SVR_E_ARG, "empty registration slice grid");
  reg_free(ctx->reg);
  RegState *r = ctx->reg = new RegState();
  r->W = (int)size[0]; r->H = (int)size[1]; r->ns = (int)size[2];
  r->wh = (size_t)r->W * r->H;
  const size_t n = (size_t)r->ns * r->wh;
  HIPCHK(r->resampled.reserve(n));
  HIPCHK(r->target.reserve(n));
  HIPCHK(r->tmp.reserve(3 * n));
  HIPCHK(r->reg.reserve(3 * n));
  HIPCHK(r->ofs.reserve(16 * r->ns));
  HIPCHK(r->mat.reserve(16 * r->ns));
  HIPCHK(r->mat_orig.reserve(16 * r->ns));
  HIPCHK(r->sim.reserve(5 * r->ns));
  HIPCHK(r->grad.reserve(7 * r->ns));
  HIPCHK(r->active.reserve(r->ns));
  HIPCHK(r->active2.reserve(r->ns));
  HIPCHK(r->active_prev.reserve(r->ns));
  HIPCHK(r->count.reserve(1));
  HIPCHK(r->dctr.reserve(5));
  HIPCHK(r->sumA.reserve(r->ns));
  HIPCHK(r->cntA.reserve(r->ns));
  HIPCHK(r->sumB.reserve(3 * r->ns));
  HIPCHK(r->cntB.reserve(3 * r->ns));
  HIPCHK(r->mom.reserve(9 * r->ns));
  HIPCHK(r->half.reserve(8 * 32));
  HIPCHK(hipMemsetAsync(r->sim, 0, 5 * sizeof(float) * r->ns, ctx->stream));
  HIPCHK(hipMemsetAsync(r->grad, 0, 7 * sizeof(float) * r->ns, ctx->stream));
  return SVR_OK;
}

int svr_fill_reg_slices(svr_ctx *ctx, const float *sdata, const float *slices_resampledI2W) {
  SVR_ENTER(ctx);
  if (!ctx || !sdata) return SVR_E_ARG;
  (void)slices_resampledI2W;   // uploaded but never read by the reference's kernels (RC.cu:3515)
  NEED(ctx->reg, "svr_init_reg_storage_volumes first");
  RegState *r = ctx->reg;
  HIPCHK(hipMemcpyAsync(r->resampled, sdata, (size_t)r->ns * r->wh * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  r->have_slices = true;
  return SVR_OK;
}

int svr_update_resampled_slices_i2w(svr_ctx *ctx, const float *ofsSlice) {
  SVR_ENTER(ctx);
  if (!ctx || !ofsSlice) return SVR_E_ARG;
  NEED(ctx->reg, "svr_init_reg_storage_volumes first");
  RegState *r = ctx->reg;
  HIPCHK(hipMemcpyAsync(r->ofs, ofsSlice, 16 * sizeof(float) * r->ns, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  r->have_ofs = true;
  return SVR_OK;
}

int svr_prepare_slice_to_volume_reg(svr_ctx *ctx) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  NEED(ctx->reg, "svr_init_reg_storage_volumes first");
  NEED(ctx->d_recon_volw, "svr_init_reconstruction_volume first");
  RegState *r = ctx->reg;
  HIPCHK(r->vol.reserve(ctx->nv));
  HIPCHK(hipMemcpyAsync(r->vol, ctx->recon(), ctx->nv * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
  // RC.cu:3884-3900
  r->levels = 2; r->steps = 4; r->iterations = 20; r->epsilon = 0.0001f;
  r->blurring[0] = ctx->vdim[0] / 2.0f;
  for (int i = 0; i < r->levels; ++i) r->length_of_steps[i] = (float)(0.1 * pow(2.0f, i));
  for (int i = 1; i < r->levels; ++i) r->blurring[i] = r->blurring[i - 1] * 2;
  float h[8 * 32];
  memset(h, 0, sizeof(h));
  for (int i = 0; i < r->levels; ++i) r->klen[i] = reg_gauss_kernel(r->blurring[i], h + 32 * i);
  HIPCHK(hipMemcpyAsync(r->half, h, sizeof(h), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  r->prepared = true;
  return SVR_OK;
}

int svr_reg_set_schedule(svr_ctx *ctx, int levels, int steps, int iterations) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  NEED(ctx->reg && ctx->reg->prepared, "svr_prepare_slice_to_volume_reg first");
  RegState *r = ctx->reg;
  if (levels > 0) { if (levels > 2) return fail(ctx, SVR_E_ARG, "at most 2 levels are prepared"); r->levels = levels; }
  if (steps > 0) r->steps = steps;
  if (iterations > 0) r->iterations = iterations;
  return SVR_OK;
}

int svr_register_slices_to_volume(svr_ctx *ctx, float *transf) {
  SVR_ENTER(ctx);
  if (!ctx || !transf) return SVR_E_ARG;
  NEED(ctx->reg && ctx->reg->prepared && ctx->reg->have_slices && ctx->reg->have_ofs,
       "FillRegSlices / updateResampledSlicesI2W / prepareSliceToVolumeReg first");
  RegState *r = ctx->reg;
  const int s = r->ns;
  const size_t mb = 16 * sizeof(float) * s;
  ScopedTimer t(ctx, SVR_T_REGISTER);
  for (int k = 0; k < 4; ++k) r->counters[k] = 0;
  HIPCHK(hipMemcpyAsync(r->mat, transf, mb, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(r->mat_orig, transf, mb, hipMemcpyHostToDevice, ctx->stream));
  int rc;
  r->red_threads = ctx->reg_red_threads;
  const bool batch = ctx->reg_batch && reg_batch_ready(ctx);   // the gradient's twelve evaluations as one launch sequence
  const int blind = std::max(0, ctx->reg_blind);               // line-search steps per host round trip (0: the literal loop)
  HIPCHK(hipMemsetAsync(r->dctr, 0, 5 * sizeof(long long), ctx->stream));
  r->ls_max = 0;
#define RCHK(x) do { rc = (x); if (rc) return rc; } while (0)
  for (int level = r->levels - 1; level >= 0; --level) {
    float step = r->length_of_steps[level];
    RCHK(reg_begin_level(ctx, level));
    for (int st = 0; st < r->steps; ++st) {
      hipLaunchKernelGGL(k_reg_iota, dim3(nblk(s)), dim3(256), 0, ctx->stream, r->active, s);
      int active = s;
      for (int iter = 0; iter < r->iterations; ++iter) {
        r->counters[2] += 1;
        RCHK(reg_evaluate(ctx, active, level, 0, 1, 3));
        if (batch) RCHK(reg_evaluate_variants(ctx, active, level, step));
        else {
        for (int p = 0; p < 6; ++p) {
          hipLaunchKernelGGL(k_reg_adjust, dim3(nblk(active)), dim3(256), 0, ctx->stream, r->mat_orig, r->mat, r->active,
                             active, p, step);
          RCHK(reg_evaluate(ctx, active, level, 3, 0, 1));
          hipLaunchKernelGGL(k_reg_adjust, dim3(nblk(active)), dim3(256), 0, ctx->stream, r->mat_orig, r->mat, r->active,
                             active, p, -step);
          RCHK(reg_evaluate(ctx, active, level, 4, 0, 1));
          hipLaunchKernelGGL(k_reg_grad, dim3(nblk(active)), dim3(256), 0, ctx->stream, r->sim, r->grad, r->active, active,
                             s, p);
        }
        hipLaunchKernelGGL(k_reg_normalize, dim3(nblk(active)), dim3(256), 0, ctx->stream, r->grad, r->active, active, s);
        KCHK("k_reg_normalize");
        }
        const int prev_active = active;
        HIPCHK(hipMemcpyAsync(r->active_prev, r->active, sizeof(int) * active, hipMemcpyDeviceToDevice, ctx->stream));
        if (blind > 0) {
          // the line search without a host round trip per step: the active count stays on the device, `blind` steps are
          // launched at a time over grids sized for the last count the host saw (a step whose count is 0 is a no-op, like
          // the loop that would not have run it), and the count is read once per chunk
          hipLaunchKernelGGL(k_reg_copy_sim, dim3(nblk(active)), dim3(256), 0, ctx->stream, r->sim, r->active, active, s, 2, 0);
          hipLaunchKernelGGL(k_reg_step, dim3(nblk(active)), dim3(256), 0, ctx->stream, r->mat, r->grad, r->active, active, s, step);
          hipLaunchKernelGGL(k_reg_set_count, dim3(1), dim3(1), 0, ctx->stream, r->count, active);
          do {
            for (int j = 0; j < blind; ++j) {
              RCHK(reg_evaluate(ctx, active, level, 0, 1, 1, r->count));
              hipLaunchKernelGGL(k_reg_line_check, dim3(1), dim3(1024), 0, ctx->stream, r->active2, r->active, s, r->sim, r->epsilon, r->count,
                                 r->mat, r->grad, step, r->dctr);
              std::swap(r->active, r->active2);
            }
            KCHK("k_reg_line_check");
            HIPCHK(hipMemcpyAsync(&active, r->count, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipStreamSynchronize(ctx->stream));
          } while (active > 0);
        } else
        do {
          hipLaunchKernelGGL(k_reg_copy_sim, dim3(nblk(active)), dim3(256), 0, ctx->stream, r->sim, r->active, active, s, 2,
                             0);
          hipLaunchKernelGGL(k_reg_step, dim3(nblk(active)), dim3(256), 0, ctx->stream, r->mat, r->grad, r->active, active,
                             s, step);
          RCHK(reg_evaluate(ctx, active, level, 0, 1, 1));
          r->counters[1] += 1;
          RCHK(reg_check(ctx, r->active2, r->active, active, 0, 2, &active));
          r->ls_max = std::max(r->ls_max, active);
          std::swap(r->active, r->active2);
        } while (active > 0);
        // the last step did not improve: back track (RC.cu:4118-4122)
        hipLaunchKernelGGL(k_reg_step, dim3(nblk(prev_active)), dim3(256), 0, ctx->stream, r->mat, r->grad, r->active_prev,
                           prev_active, s, -step);
        KCHK("k_reg_step");
        HIPCHK(hipMemcpyAsync(r->mat_orig, r->mat, mb, hipMemcpyDeviceToDevice, ctx->stream));
        RCHK(reg_check(ctx, r->active, r->active_prev, prev_active, 2, 1, &active));
        r->last_active = active;
        if (active == 0) break;
      }
      step /= 2.0f;
    }
  }
#undef RCHK
  long long dc[5] = {0, 0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(dc, r->dctr, sizeof(dc), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(transf, r->mat, mb, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < 4; ++k) r->counters[k] += dc[k];
  r->ls_max = std::max(r->ls_max, (int)dc[4]);
  t.stop();
  return SVR_OK;
}

/* debug / test hook: one evaluateCostsMultipleSlices(…, 0, 1, 1) on the blurred targets of `level`
 * for the given matrices and active list (NULL = all slices).  similarities_out[slices];
 * reg_slices_out (optional) = blurred sampled slices [3][n_active][H][W] (debugRegSlicesVolume, RC.cuh:207) */
int svr_reg_evaluate_costs(svr_ctx *ctx, const float *transf, int level, const int *active_or_null, int n_active,
                           float *similarities_out, float *reg_slices_out) {
  SVR_ENTER(ctx);
  if (!ctx || !transf || !similarities_out) return SVR_E_ARG;
  NEED(ctx->reg && ctx->reg->prepared && ctx->reg->have_slices && ctx->reg->have_ofs,
       "FillRegSlices / updateResampledSlicesI2W / prepareSliceToVolumeReg first");
  RegState *r = ctx->reg;
  if (level < 0 || level >= r->levels) return fail(ctx, SVR_E_ARG, "level out of range");
  r->red_threads = ctx->reg_red_threads;
  const int s = r->ns;
  int a = s;
  if (active_or_null) {
    if (n_active < 0 || n_active > s) return fail(ctx, SVR_E_ARG, "active list too long");
    for (int i = 0; i < n_active; ++i)
      if (active_or_null[i] < 0 || active_or_null[i] >= s) return fail(ctx, SVR_E_ARG, "active slice out of range");
    a = n_active;
  }
  HIPCHK(hipMemcpyAsync(r->mat, transf, 16 * sizeof(float) * s, hipMemcpyHostToDevice, ctx->stream));   // (nothing is touched before the arguments are checked)
  if (active_or_null) {
    HIPCHK(hipMemcpyAsync(r->active, active_or_null, sizeof(int) * a, hipMemcpyHostToDevice, ctx->stream));
  } else {
    hipLaunchKernelGGL(k_reg_iota, dim3(nblk(s)), dim3(256), 0, ctx->stream, r->active, s);
  }
  HIPCHK(hipMemsetAsync(r->sim, 0, 5 * sizeof(float) * s, ctx->stream));
  int rc = reg_begin_level(ctx, level);
  if (rc) return rc;
  r->last_active = a;
  rc = reg_evaluate(ctx, a, level, 0, 1, 1);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(similarities_out, r->sim, sizeof(float) * s, hipMemcpyDeviceToHost, ctx->stream));
  if (reg_slices_out)
    for (int o = 0; o < 3; ++o)
      HIPCHK(hipMemcpyAsync(reg_slices_out + (size_t)o * a * r->wh, r->reg + (size_t)o * s * r->wh,
                            (size_t)a * r->wh * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

/* test hook: a copy of the state the last svr_reg_evaluate_costs / svr_register_slices_to_volume left on the device.
 * which (enum svr_reg_state, include/svr_hip.h) picks the array; `bytes` must be its exact size.  Reads only. */
int svr_reg_get(svr_ctx *ctx, int which, void *out, size_t bytes) {
  SVR_ENTER(ctx);
  if (!ctx || !out) return SVR_E_ARG;
  NEED(ctx->reg && ctx->reg->prepared, "no registration state (svr_prepare_slice_to_volume_reg first)");
  RegState *r = ctx->reg;
  const size_t s = (size_t)r->ns;
  const void *src = nullptr;
  size_t n = 0;
  switch (which) {
    case SVR_REG_TARGETS: src = r->target; n = s * r->wh * sizeof(float); break;
    case SVR_REG_SUM_A: src = r->sumA; n = s * sizeof(float); break;
    case SVR_REG_CNT_A: src = r->cntA; n = s * sizeof(int); break;
    case SVR_REG_SUM_B: src = r->sumB; n = 3 * s * sizeof(float); break;
    case SVR_REG_CNT_B: src = r->cntB; n = 3 * s * sizeof(int); break;
    case SVR_REG_MOMENTS: src = r->mom; n = 9 * s * sizeof(float); break;
    case SVR_REG_SIMILARITIES: src = r->sim; n = 5 * s * sizeof(float); break;
    case SVR_REG_GRADIENT: src = r->grad; n = 7 * s * sizeof(float); break;
    case SVR_REG_ACTIVE: src = r->active; n = (3 + s) * sizeof(int); break;
    default: return fail(ctx, SVR_E_ARG, "svr_reg_get: unknown array");
  }
  if (bytes != n) return fail(ctx, SVR_E_ARG, "svr_reg_get: size mismatch");
  if (which == SVR_REG_ACTIVE) {
    int *o = (int *)out;
    o[0] = r->last_active; o[1] = r->ls_max; o[2] = r->red_used;
    HIPCHK(hipMemcpyAsync(o + 3, src, s * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  } else {
    HIPCHK(hipMemcpyAsync(out, src, n, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

int svr_reg_counters(svr_ctx *ctx, long long out4[4]) {
  SVR_ENTER(ctx);
  if (!ctx || !out4) return SVR_E_ARG;
  NEED(ctx->reg, "svr_init_reg_storage_volumes first");
  for (int k = 0; k < 4; ++k) out4[k] = ctx->reg->counters[k];
  return SVR_OK;
}

/* PVR patch-to-volume registration cost: computeCCpatch for every patch i of the slice grid (or of
 * `buffer`, e.g. the blurred patches, [n][pY][pX]) with its own matrix Tmat[i] and RI2W[i]
 * (R2/patchBased2D3DRegistration_gpu2.cu:130-190) against the current reconstruction. */
int svr_pvr_cc_patches(svr_ctx *ctx, const float *buffer_or_null, const float *RI2W, const float *Tmats, int level,
                       float *ncc_out, double *sums6_or_null) {
  SVR_ENTER(ctx);
  if (!ctx || !RI2W || !Tmats || !ncc_out || level < 0) return SVR_E_ARG;
  NEED(ctx->have_slices && ctx->d_recon_volw, "slice grid / reconstruction volume not set");
  const int n = (int)ctx->ns, px = (int)ctx->sx, py = (int)ctx->sy;
  std::vector<float> M(16 * (size_t)n);
  for (int i = 0; i < n; ++i) matmul4(Tmats + 16 * (size_t)i, RI2W + 16 * (size_t)i, &M[16 * (size_t)i]);   // Tmat * RI2W (:152)
  DevBuf<float> d_m, d_buf;
  DevBuf<double> d_s;
  std::vector<double> h(6 * (size_t)n);
  HIPCHK(d_m.reserve(M.size()));
  HIPCHK(d_s.reserve(h.size()));
  hipError_t e = hipMemcpyAsync(d_m, M.data(), M.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess && buffer_or_null) {
    e = d_buf.reserve(ctx->np);
    if (e == hipSuccess) e = hipMemcpyAsync(d_buf, buffer_or_null, ctx->np * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
  }
  if (e == hipSuccess) {
    RegVol v;
    v.vol = ctx->recon(); v.vx = (int)ctx->vx; v.vy = (int)ctx->vy; v.vz = (int)ctx->vz;
    memcpy(v.W2I, ctx->reconW2I, 12 * sizeof(float));
    hipLaunchKernelGGL(k_cc_patch, dim3(n), dim3(256), 0, ctx->stream, v, d_buf ? d_buf.get() : ctx->d_slices.get(), px, py, d_m, level,
                       d_s);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(h.data(), d_s, h.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return fail(ctx, (int)e, "svr_pvr_cc_patches");
  for (int i = 0; i < n; ++i) {
    const double *s = &h[6 * (size_t)i];
    if (sums6_or_null) for (int k = 0; k < 6; ++k) sums6_or_null[6 * (size_t)i + k] = s[k];
    // the closing expression of computeCCpatch in float (:180-188)
    const float cnt = (float)s[0], x = (float)s[1], y = (float)s[2], x2 = (float)s[3], y2 = (float)s[4], xy = (float)s[5];
    ncc_out[i] = s[0] > 0 ? (xy - (x * y) / cnt) / (sqrtf(x2 - x * x / cnt) * sqrtf(y2 - y * y / cnt)) : 0.0f;
  }
  return SVR_OK;
}


/* PatchBased2D3DRegistration_gpu2<T>::run (R2/patchBased2D3DRegistration_gpu2.cu:450-566) for every patch of the slice grid
 * against the current reconstruction.  T: the patches' transformations [n][16], in/out; Tinv_out: their inverses;
 * Mo / InvMo / RI2W: the origin-reset matrices of the patches (patchBasedObject.cuh:285-304).  The optimised matrix is
 * T * Mo (:96), levels 2, 1, 0 (every 3rd / 2nd / every pixel, blurring dim.x/2 * 2^level, steps 2 * 2^level halved 4
 * times, 20 runs per step size, no early exit); at the end T = (T * Mo) * InvMo (:110).
 * The reference's run() also iterates a level 3 whose blurring and step length are read past the end of two 3-element
 * arrays (:476-478 with m_NumberOfLevels = 3, :584-596): undefined there, omitted here.
 * counters3 = {kernel launches, cost evaluations, patches}. */
int svr_pvr_register_patches(svr_ctx *ctx, const float *RI2W, const float *Mo, const float *InvMo, float *T, float *Tinv_out,
                             long long *counters3_or_null) {
  SVR_ENTER(ctx);
  if (!ctx || !RI2W || !Mo || !InvMo || !T || !Tinv_out) return SVR_E_ARG;
  NEED(ctx->have_slices && ctx->d_recon_volw, "slice grid / reconstruction volume not set");
  ScopedTimer t(ctx, SVR_T_REGISTER);
  const int n = (int)ctx->ns, px = (int)ctx->sx, py = (int)ctx->sy;
  const size_t mb = 16 * sizeof(float) * (size_t)n;
  std::vector<float> M(16 * (size_t)n);
  for (int i = 0; i < n; ++i) matmul4(T + 16 * (size_t)i, Mo + 16 * (size_t)i, &M[16 * (size_t)i]);       // initDevReconMatrices2
  DevBuf<float> d_m, d_r, d_buf, d_tmp, d_half;
  DevBuf<int> d_ev;
  hipError_t e = d_m.reserve(16 * (size_t)n);
  if (e == hipSuccess) e = d_r.reserve(16 * (size_t)n);
  if (e == hipSuccess) e = d_buf.reserve(ctx->np);
  if (e == hipSuccess) e = d_tmp.reserve(ctx->np);
  if (e == hipSuccess) e = d_half.reserve(40);
  if (e == hipSuccess) e = d_ev.reserve(n);
  if (e == hipSuccess) e = hipMemcpyAsync(d_m, M.data(), mb, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_r, RI2W, mb, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_ev, 0, sizeof(int) * (size_t)n, ctx->stream);
  RegVol v;
  v.vol = ctx->recon(); v.vx = (int)ctx->vx; v.vy = (int)ctx->vy; v.vz = (int)ctx->vz;
  memcpy(v.W2I, ctx->reconW2I, 12 * sizeof(float));
  long long launches = 0;
  for (int level = ctx->pvr_reg_levels - 1; level >= 0 && e == hipSuccess; --level) {
    const float sigma = (ctx->vdim[0] / 2.0f) * (float)(1 << level);            // m_Blurring (:590-596)
    float half[40];
    memset(half, 0, sizeof(half));
    const int klen = reg_gauss_kernel(sigma, half);
    int nh = (klen + 1) / 2, nh_y = nh;
    if (klen == 13) { half[nh] = half[nh - 1]; nh_y = nh + 1; }                 // GaussYKernel<14> for klength 13 (PGF.cu:311): one more, clamped, tap
    e = hipMemcpyAsync(d_half, half, sizeof(half), hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) break;
    const dim3 grid(nblk((size_t)px * py), n, 1);
    hipLaunchKernelGGL((k_reg_blur<false, true>), grid, dim3(256), 0, ctx->stream, ctx->d_slices, d_tmp, px, py, 0, d_half, nh);
    hipLaunchKernelGGL((k_reg_blur<true, true>), grid, dim3(256), 0, ctx->stream, d_tmp, d_buf, px, py, 0, d_half, nh_y);
    float step = 2.0f * (float)(1 << level);                                    // m_LengthOfSteps
    for (int st = 0; st < ctx->pvr_reg_steps; ++st) {
      for (int iter = 0; iter < ctx->pvr_reg_iterations; ++iter) {
        hipLaunchKernelGGL(k_pvr_patch_opt, dim3(n), dim3(256), 0, ctx->stream, v, d_buf, px, py, d_r, d_m, level, step, d_ev);
        ++launches;
      }
      step /= 2.0f;
    }
    e = hipGetLastError();
  }
  std::vector<int> ev(n);
  if (e == hipSuccess) e = hipMemcpyAsync(M.data(), d_m, mb, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(ev.data(), d_ev, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return fail(ctx, (int)e, "svr_pvr_register_patches");
  long long evals = 0;
  for (int i = 0; i < n; ++i) {
    matmul4(&M[16 * (size_t)i], InvMo + 16 * (size_t)i, T + 16 * (size_t)i);                                  // resetOriginDevReconMatrices2
    double a[16], inv[16];
    for (int k = 0; k < 16; ++k) a[k] = T[16 * (size_t)i + k];
    invert4d(a, inv);                                                                                          // irtkMatrix::Invert on the host (:540-546)
    for (int k = 0; k < 16; ++k) Tinv_out[16 * (size_t)i + k] = (float)inv[k];
    evals += ev[i];
  }
  if (counters3_or_null) { counters3_or_null[0] = launches; counters3_or_null[1] = evals; counters3_or_null[2] = n; }
  t.stop();
  return SVR_OK;
}

}  // extern "C"
