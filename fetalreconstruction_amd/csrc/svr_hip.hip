// svr_hip.hip -- MI355X (gfx950) slice-to-volume super-resolution engine behind the C-ABI of
// include/svr_hip.h.  Written for CDNA4 only: 64-wide wavefronts; the PSF evaluated row per lane, two taps per lane-op
// (v_pk_fma_f32); the scatter with one wavefront owning four planes of a tile's LDS box (back_wave_kernel), the gather
// with a workgroup per tile over (pixel, plane) units (fwd_unit_kernel); optionally the evaluated taps kept in HBM and
// streamed (the coefficient table, k_coeff_build); hardware float atomics only at the flush.
//
// Reference behaviour being replaced (citations: RC.cu = source/reconstructionGPU2/
// reconstruction_cuda2.cu, RC.cuh = include/reconstruction_cuda2.cuh, RVH =
// include/recon_volumeHelper.cuh, RG.cc = irtkReconstructionGPU.cc).  See DESIGN.md for the
// canonical float32 PSF sequence and the list of reproduced / not reproduced quirks.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -munsafe-fp-atomics ... (build.py)
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "../../include/svr_hip.h"
#include "svr_devbuf.h"
#include "svr_plan.h"      // which kernel family runs a PSF pass and what it does with the coefficient table: plain C++ (pass_path, table_plan)

// csrc/svr_sort.hip: radix sort / prefix sum of the vendor's primitives library for the work lists of svr_cell.inc
int svr_sort_keys_u64(void *tmp, size_t *tmp_bytes, const uint64_t *keys_in, uint64_t *keys_out, size_t n, int end_bit, hipStream_t stream);
int svr_inclusive_sum_u32(void *tmp, size_t *tmp_bytes, const uint32_t *in, uint32_t *out, size_t n, hipStream_t stream);

// ------------------------------------------------------------------------------------------
// constants of the reference configuration section (RC.cuh:54-75)
// ------------------------------------------------------------------------------------------
#define SVR_STEP 0.0001f        // __step
#define PSF_SUPPORT 16          // MAX_PSF_SUPPORT with USE_INFINITE_PSF_SUPPORT 1
#define PSF_CENTRE 7            // (MAX_PSF_SUPPORT - 1) / 2   (RC.cu:219)
// `abs(oldPSF - psfval) < PSF_EPSILON` compares a float against the double 0.00001
// (RC.cuh:72, RC.cu:238); for a float f that is exactly  f <= 0.00001f  because 0.00001f is
// the largest float below 1e-5.
#define PSF_EPS_F 0.00001f
#define LDS_ROW 20              // floats per PSF row in LDS (16 + pad: conflict-free b128 stores)
#define WAVES_PER_BLOCK 4
#define CHUNK_PIX 2048          // slice-grid pixels per block in the EM kernels

namespace {

// ------------------------------------------------------------------------------------------
// host float helpers with the literal operation order of RVH:134-159 (no FMA contraction)
// ------------------------------------------------------------------------------------------
void matmul4(const float *A, const float *B, float *C) {
  float t[16];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j)
      t[i * 4 + j] = A[i * 4 + 0] * B[0 * 4 + j] + A[i * 4 + 1] * B[1 * 4 + j] +
                     A[i * 4 + 2] * B[2 * 4 + j] + A[i * 4 + 3] * B[3 * 4 + j];
  memcpy(C, t, sizeof(t));
}
void matvec3_host(const float *M, const float v[3], float out[3]) {
  out[0] = M[0] * v[0] + M[1] * v[1] + M[2] * v[2] + M[3];
  out[1] = M[4] * v[0] + M[5] * v[1] + M[6] * v[2] + M[7];
  out[2] = M[8] * v[0] + M[9] * v[1] + M[10] * v[2] + M[11];
}

// per-slice constants, 64 floats, read through the scalar cache (slice index is wave-uniform)
struct SliceConst {
  float I2W[12];   // rows 0..2 of sliceI2W
  float T[12];     // slice transformation
  float A[12];     // combInvTrans = sliceW2I * Tinv * reconI2W  (RC.cu:223)
  float Lp[9];     // linear part of A scaled to calcPSF's argument space
  float dim[3];    // slice voxel dims (dx, dy, thickness)
  float kx, ky, inv2s2;
  float dd, w;     // Gaussian recurrence along a row: (z' step)^2, and exp(-2 dd inv2s2) or -1 (see gauss_pairs)
  int own;         // volume axis whose planes the scatter's slots own: 1 = y, 2 = z (the one closer to the slice normal)
  float invD;      // 1 / determinant of the in-plane map over (x, lane axis), or 0 if degenerate (unit_is_dead)
  float pad[9];
};
static_assert(sizeof(SliceConst) == 256, "SliceConst layout");

struct VolGeom {
  int vx, vy, vz;
  float W2I[12];   // rows 0..2 of reconstructedW2I
  float c0[3];     // d_PSFI2W * ((PSFsize-1)/2)  (RC.cu:172)
  int pvr;         // patch-to-volume constants
};

// ------------------------------------------------------------------------------------------
// canonical PSF (bit-identical to oracle/svr_oracle.c psf_canon: IEEE fma/mul/add/rint + integer ops)
// ------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ float canon_exp_neg(float a) {
  const float LOG2E = 1.442695040888963407359924681001892137426645954152985934135449406931f;
  const float L2U = 0.693145751953125f;
  const float L2L = 1.428606765330187045e-06f;
  float d = -a;
  float q = __builtin_rintf(d * LOG2E);
  float s = __builtin_fmaf(q, -L2U, d);
  s = __builtin_fmaf(q, -L2L, s);
  float u = 0.000198527617612853646278381f;
  u = __builtin_fmaf(u, s, 0.00139304355252534151077271f);
  u = __builtin_fmaf(u, s, 0.00833336077630519866943359f);
  u = __builtin_fmaf(u, s, 0.0416664853692054748535156f);
  u = __builtin_fmaf(u, s, 0.166666671633720397949219f);
  u = __builtin_fmaf(u, s, 0.5f);
  u = __builtin_fmaf(s * s, u, s) + 1.0f;
  float r = ldexpf(u, (int)q);
  return (a > 87.0f) ? 0.0f : r;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ void matvec3(const float *M, float x, float y, float z, float &a,
                                        float &b, float &c) {
  a = M[0] * x + M[1] * y + M[2] * z + M[3];
  b = M[4] * x + M[5] * y + M[6] * z + M[7];
  c = M[8] * x + M[9] * y + M[10] * z + M[11];
}

enum { MODE_GAUSS = 0, MODE_FWD = 1, MODE_BACK = 2, MODE_BIAS = 3 };

struct PsfArgs {
  const SliceConst *sc;
  VolGeom vg;
  int sx, sy;               // slice grid
  const uint32_t *list;     // pixel indices to process
  uint32_t n;
  const float *slices;
  const float *mask;
  float *psf_sums;
  const float *scales;        // per slice
  const float *bias;          // per-pixel log bias field, NULL when _disableBiasC (RC.cu:200-203)
  const unsigned char *flag;  // optional per-pixel activity flag replacing `v_PSF_sums != 0` (Gaussian pass 2)
  unsigned char *flag_out;    // Gaussian pass 1: 1 where the pixel's sume passed the threshold
  const unsigned char *spx;   // PVR superpixel masks [ns][64*64] of '0'/'1' or NULL (ImagePatch2D.cuh:51)
  // gauss (MODE_BIAS reuses recon/volw for the bias volume / its accumulated weights)
  float *recon, *volw;
  int *voxcount;
  // forward
  const float *vol;
  const float2 *volm;       // SVR gather: {V m, m} per voxel, packed by k_pack_volm right before the pass (NULL: vol + mask)
  float *simslices, *simweights;
  unsigned char *siminside;
  unsigned char *slice_inside;  // [slice]: some pixel of the slice has siminside == 1 (k_slice_inside; the cell gather's finish sets it itself: siminside only ever
                                // goes from 0 to 1 between two Gaussian passes, so the per-slice flag needs no pass of its own)
  // back
  const float *weights, *slice_weights;
  float *addon, *cmap;
  // coefficient table (COEFF instantiations): the evaluated taps of every live unit of every PSF pixel, kept in HBM
  const float4 *coeff;        // [pixel id][16 units][4 tap quads][16 rows] float4
  const uint32_t *coeff_id;   // slice-grid index -> pixel id
  // channel scatter (k_cell_factors modes 3 and 4, svr_channel.inc): a float per slice pixel that is not the primary image
  const float *channel;
  const unsigned char *unit_on;   // [slice] 0 = the slice has no such channel; NULL = every slice has
  int ch_flags;                   // SVR_CHANNEL_INDICATOR: the scattered value is (channel == ch_match) ? 1 : 0
  float ch_match;
};

// per-pixel state shared by all modes
struct PixelState {
  int cxi, cyi, czi;   // rounded centre voxel psfxyz (RC.cu:225-226)
  float bx, by, bz;    // scaled residual at the centre (canonical form)
};

__device__ __forceinline__ int clampi(float f) {
  // |centre| beyond 2^20 is out of any volume; clamp so the int arithmetic cannot overflow
  f = fminf(fmaxf(f, -1048576.0f), 1048576.0f);
  return (int)f;   // NaN -> 0 after the clamp's fmin/fmax semantics
}

__device__ __forceinline__ PixelState pixel_setup(const SliceConst &S, const VolGeom &vg, int px,
                                                  int py) {
  PixelState P;
  float wx, wy, wz, tx, ty, tz, vx_, vy_, vz_;
  // d_reconstructedW2I * (slicesTransformation * (sliceI2W * slicePos))  RC.cu:225
  matvec3(S.I2W, (float)px, (float)py, 0.0f, wx, wy, wz);
  matvec3(S.T, wx, wy, wz, tx, ty, tz);
  matvec3(vg.W2I, tx, ty, tz, vx_, vy_, vz_);
  float cx = roundf(vx_), cy = roundf(vy_), cz = roundf(vz_);
  P.cxi = clampi(cx); P.cyi = clampi(cy); P.czi = clampi(cz);
  double d0 = (double)S.A[0] * cx + (double)S.A[1] * cy + (double)S.A[2] * cz + (double)S.A[3] - (double)(float)px;
  double d1 = (double)S.A[4] * cx + (double)S.A[5] * cy + (double)S.A[6] * cz + (double)S.A[7] - (double)(float)py;
  double d2 = (double)S.A[8] * cx + (double)S.A[9] * cy + (double)S.A[10] * cz + (double)S.A[11] - 0.0;
  P.bx = (float)((d0 * S.dim[0] - vg.c0[0]) * S.kx);
  P.by = (float)((d1 * S.dim[1] - vg.c0[1]) * S.ky);
  P.bz = vg.pvr ? (float)(d2 * S.dim[2] / 2.5 - vg.c0[2]) : (float)(d2 * S.dim[2] - vg.c0[2]);
  return P;
}

// hot per-slice constants held in registers (SGPRs: the slice index is wave-uniform)
struct RowConst {
  float Lp[9];
  float inv2s2;
  float dd, w;
  float invD;
};
__device__ __forceinline__ float uniform_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}
__device__ __forceinline__ RowConst load_row_const(const SliceConst &S) {
  RowConst R;
#pragma unroll
  for (int i = 0; i < 9; ++i) R.Lp[i] = S.Lp[i];
  // (through readfirstlane: the four values stay in scalar registers; read as plain struct fields the vectoriser fuses
  // them into one 16-byte load of a stack copy of the struct -- 32 bytes of scratch per lane for nothing)
  R.inv2s2 = uniform_f(S.inv2s2);
  R.dd = uniform_f(S.dd);
  R.w = uniform_f(S.w);
  R.invD = uniform_f(S.invD);
  return R;
}

// One (y,z) row of a pixel's footprint: walks the 16 x-taps sequentially with the
// epsilon-skip (RC.cu:233-239).  out[x] = psf, or -1 if skipped.  fy, fz = row offsets in
// [-7, 8] relative to the centre voxel.
// The PSF of the row's taps is evaluated STAGE BY STAGE over chunks of EVAL_CHUNK taps (arrays in
// registers): every stage is EVAL_CHUNK independent instructions, which is what lets one wave
// issue back to back -- evaluated tap after tap the dependent chains (sqrt, division, two
// polynomials) left the SIMDs latency-bound (forward time scaled 1:1 with occupancy).  The
// arithmetic per tap is exactly the oracle's psf_canon, so the values stay bit-identical.
// N = PSF support (16 for SVR, 12 for PVR), CENTRE = (N-1)/2; PVR selects the patch-to-volume
// constants (sinc_pi Taylor branch, strict float epsilon; R2/include/pointSpreadFunction.cuh:45-70,
// R2/include/reconConfig.cuh:138).
typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2 fma2(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f2 bc2(float c) { return (f2)(c); }

// H pairs of consecutive x-taps of one (y,z) row, first tap at lattice offset fx0: val2[i] = psf of taps
// (fx0 + 2i, fx0 + 2i + 1).  rowx/rowy/rowz = the row's part of the scaled lattice coordinates.
// psf of 2H taps given their scaled lattice coordinates (x', y', z') two per lane-op
// exp(-a) of two values: canon_exp_neg per component
__device__ __forceinline__ f2 exp_neg2(f2 a) {
  const f2 t = -a * bc2(1.442695040888963407359924681001892137426645954152985934135449406931f);
  const f2 k = (f2){__builtin_rintf(t.x), __builtin_rintf(t.y)};
  f2 r = fma2(k, bc2(-0.693145751953125f), -a);
  r = fma2(k, bc2(-1.428606765330187045e-06f), r);
  f2 s = fma2(bc2(0.000198527617612853646278381f), r, bc2(0.00139304355252534151077271f));
  s = fma2(s, r, bc2(0.00833336077630519866943359f));
  s = fma2(s, r, bc2(0.0416664853692054748535156f));
  s = fma2(s, r, bc2(0.166666671633720397949219f));
  s = fma2(s, r, bc2(0.5f));
  s = fma2(r * r, s, r) + bc2(1.0f);
  s = (f2){ldexpf(s.x, (int)k.x), ldexpf(s.y, (int)k.y)};
  return (f2){(a.x > 87.0f) ? 0.0f : s.x, (a.y > 87.0f) ? 0.0f : s.y};
}

// The Gaussian factor exp(-z'^2 inv2s2) of a row's taps, canonical definition (oracle: canon_gauss_row).  z' is
// linear along the row, so the factor of neighbouring taps differs by a ratio that itself changes by the constant
// w = exp(-2 dd inv2s2): from the two central taps (lattice offsets 0 and 1, where |z'| is smallest for every row
// that matters) the factors are stepped outwards,
//     g(-j) = g(-j+1) * rl,  rl *= w      g(1+j) = g(j) * rr,  rr *= w,
// two multiplications per tap instead of an exponential.  g[j] = {factor of tap -j, factor of tap 1+j}.
// A row whose central factors are too small to start from (a > GAUSS_AMAX: thin slices seen obliquely, far from
// the slice plane), and every row of a slice whose first ratio could overflow (S.w < 0, set by the host), takes
// the exponential per tap instead; which rows do is part of the definition, and the oracle applies the same test.
#define GAUSS_AMAX 60.0f
// the rare path of gauss_pairs, out of line so that it costs the common path no registers
__device__ __attribute__((noinline)) f2 gauss_direct2(float dz, float rowz, float inv2s2, float j, bool keep, f2 g) {
  const f2 z = fma2(bc2(dz), (f2){-j, 1.0f + j}, bc2(rowz));
  const f2 e = exp_neg2((z * z) * bc2(inv2s2));
  return keep ? g : e;
}
struct GaussStep {        // state of the recurrence between two chunks of pairs
  f2 g, r;
  bool ok;
};
__device__ __forceinline__ GaussStep gauss_start(const RowConst S, float rowz) {
  const f2 zc = fma2(bc2(S.Lp[6]), (f2){0.0f, 1.0f}, bc2(rowz));
  const f2 ac = (zc * zc) * bc2(S.inv2s2);
  const f2 t = fma2(((f2){-2.0f, 2.0f}) * zc, bc2(S.Lp[6]), bc2(S.dd)) * bc2(S.inv2s2);
  GaussStep st;
  st.r = exp_neg2(t);
  st.g = exp_neg2(ac);
  st.ok = ac.x <= GAUSS_AMAX && ac.y <= GAUSS_AMAX && S.w >= 0.0f;
  return st;
}
// factors of pairs j0 .. j0 + H - 1
template <int H>
__device__ __forceinline__ void gauss_pairs(const RowConst S, float rowz, GaussStep &st, int j0, f2 g[H]) {
#pragma unroll
  for (int i = 0; i < H; ++i) {
    if (j0 + i > 0) {
      st.g = st.g * st.r;
      st.r = st.r * bc2(S.w);
    }
    g[i] = st.g;
  }
#ifndef SVR_NO_GAUSS_FALLBACK
  if (!__all(st.ok)) {
#pragma unroll
    for (int i = 0; i < H; ++i)
      if (j0 + i > 0) g[i] = gauss_direct2(S.Lp[6], rowz, S.inv2s2, (float)(j0 + i), st.ok, g[i]);
  }
#endif
}
// the same for the first tap (lattice offset -CENTRE) of two rows at once: x = row A, y = row B
template <int CENTRE>
__device__ __forceinline__ f2 gauss_first_tap2(const RowConst S, f2 rowz) {
  const f2 zl = fma2(bc2(S.Lp[6]), bc2(0.0f), rowz), zr = fma2(bc2(S.Lp[6]), bc2(1.0f), rowz);
  const f2 al = (zl * zl) * bc2(S.inv2s2), ar = (zr * zr) * bc2(S.inv2s2);
  const f2 t = fma2(bc2(-2.0f) * zl, bc2(S.Lp[6]), bc2(S.dd)) * bc2(S.inv2s2);
  f2 r = exp_neg2(t), g = exp_neg2(al);
#pragma unroll
  for (int j = 1; j <= CENTRE; ++j) {
    g = g * r;
    r = r * bc2(S.w);
  }
  const bool okx = al.x <= GAUSS_AMAX && ar.x <= GAUSS_AMAX && S.w >= 0.0f;
  const bool oky = al.y <= GAUSS_AMAX && ar.y <= GAUSS_AMAX && S.w >= 0.0f;
  if (!__all(okx && oky)) {
    const f2 z = fma2(bc2(S.Lp[6]), bc2((float)(-CENTRE)), rowz);
    const f2 e = exp_neg2((z * z) * bc2(S.inv2s2));
    g.x = okx ? g.x : e.x;
    g.y = oky ? g.y : e.y;
  }
  return g;
}

// in-plane factor sinc^2 of 2H taps given their scaled in-plane lattice coordinates (x', y'), two per lane-op.
// The canonical sequence (oracle: canon_rsqrt / canon_sinc) is built from fma / mul / add / rint and one integer
// shift-subtract only -- no quarter-rate transcendental, no correctly rounded sqrt or division to emulate:
//   q = x'^2 + y'^2;  y ~ 1/sqrt(q) (bit-trick start + 2 Newton-form steps with tuned constants, round 3);  r = q y;  f = r - rint(r) (exact);
//   sin(pi r)/(pi r) = +-(f y) P(f^2), P = degree-4 fit of sinc on [0, 1/4];  the square removes the sign.
// q == 0 gives NaN like sin(0)/0 in the reference (RC.cu:129); PVR takes sinc_pi's Taylor branch there instead.
#define RSQRT_MAGIC 0x5f376686u
#define RSQRT_K1 1.5009000301361084f
#define RSQRT_K2 1.5000005960464478f
template <int H, bool PVR>
__device__ __forceinline__ void eval_pairs_xyz(const RowConst S, const f2 xs[H], const f2 ys[H], f2 val2[H]) {
#define EACH for (int i = 0; i < H; ++i)
    f2 q[H], y[H], h[H], r[H], f[H], p[H];
#pragma unroll
    EACH q[i] = fma2(ys[i], ys[i], xs[i] * xs[i]);
#pragma unroll
    EACH y[i] = (f2){__uint_as_float(RSQRT_MAGIC - (__float_as_uint(q[i].x) >> 1)),
                     __uint_as_float(RSQRT_MAGIC - (__float_as_uint(q[i].y) >> 1))};
#pragma unroll
    EACH h[i] = bc2(0.5f) * q[i];
#pragma unroll
    for (int it = 0; it < 2; ++it) {                       // two steps with centred errors (RSQRT_K1, RSQRT_K2): 7.1e-7
#pragma unroll
      EACH r[i] = h[i] * y[i];
#pragma unroll
      EACH r[i] = fma2(-r[i], y[i], bc2(it == 0 ? RSQRT_K1 : RSQRT_K2));
#pragma unroll
      EACH y[i] = y[i] * r[i];
    }
#pragma unroll
    EACH r[i] = q[i] * y[i];
#pragma unroll
    EACH f[i] = r[i] - (f2){__builtin_rintf(r[i].x), __builtin_rintf(r[i].y)};
#pragma unroll
    EACH h[i] = f[i] * f[i];
#pragma unroll
    EACH p[i] = fma2(bc2(0.024719201028347015f), h[i], bc2(-0.1904420256614685f));
#pragma unroll
    EACH p[i] = fma2(p[i], h[i], bc2(0.8117148876190186f));
#pragma unroll
    EACH p[i] = fma2(p[i], h[i], bc2(-1.6449332237243652f));
#pragma unroll
    EACH p[i] = fma2(p[i], h[i], bc2(1.0f));
#pragma unroll
    EACH p[i] = (f[i] * y[i]) * p[i];
    if (PVR) {
      // sinc_pi: Taylor branch below eps^(1/4) instead of the NaN at 0 (pointSpreadFunction.cuh:45-70).  Only a tap within
      // 0.006 voxels of the PSF centre takes it: the branch (two IEEE divisions per tap) is entered when some lane has one
      // (round 3: it used to run for every tap and was a third of the patch-based kernels' instructions)
      // (the test is on q, a superset: pi sqrt(q) < 1.858e-2 needs q < 3.5e-5; q == 0 makes r NaN, which a minimum of r would skip)
      float qmin = FLT_MAX;
#pragma unroll
      EACH qmin = __builtin_fminf(__builtin_fminf(qmin, q[i].x), q[i].y);
      if (__any(!(qmin >= 4.0e-5f))) {
#pragma unroll
      EACH {
        for (int c = 0; c < 2; ++c) {
          const float x = 3.14159265359f * (c ? r[i].y : r[i].x), x2 = x * x;
          float t = 1.0f;
          if (x >= 1.1920929e-07f) {
            t -= x2 / 6.0f;
            if (x >= 3.4526698300e-04f) t += (x2 * x2) / 120.0f;
          }
          if (c) p[i].y = (x >= 1.8581361323e-02f) ? p[i].y : t;
          else p[i].x = (x >= 1.8581361323e-02f) ? p[i].x : t;
        }
      }
      }
    } else {
      // the R = 0 tap: only a pixel that sits exactly on a voxel centre of an aligned slice has one.  One v_min3_f32 per pair and a
      // branch that is never taken on real data (the empty asm keeps it one)
      float qmin = FLT_MAX;
#pragma unroll
      EACH qmin = __builtin_fminf(__builtin_fminf(qmin, q[i].x), q[i].y);
      if (__builtin_expect(__any(qmin == 0.0f), 0)) {
        asm volatile("" ::: "memory");
#pragma unroll
        EACH {
          p[i].x = (q[i].x == 0.0f) ? __builtin_nanf("") : p[i].x;
          p[i].y = (q[i].y == 0.0f) ? __builtin_nanf("") : p[i].y;
        }
      }
    }
#pragma unroll
    EACH val2[i] = p[i] * p[i];                         // si * si; the caller multiplies by the Gaussian factor
#undef EACH
}

// ZERO: skipped taps come out as -0.0f instead of -1: adding them changes nothing, and a processed tap whose value is
// exactly +0 (an underflowed Gaussian factor, sin(pi r) at an integer r) can still be told from a skipped one by its bits
// HP: pairs evaluated side by side (0 = the default below); the cell kernels ask for a whole row at once (no pixel tables, no
// tile state: they have the registers, and the longer independent stages are worth 3-4 % of their time)
// (the two halves of eval_row_t: the values of a row's taps, and the epsilon-walk over them -- a kernel that has loads to issue in
// between calls them one after the other)
template <int N, bool PVR, int HP = 0>
__device__ __forceinline__ void eval_row_vals(const RowConst S, float bx, float by, float bz, float fy, float fz, float val[N]);
template <int N, bool PVR, bool ZERO>
__device__ __forceinline__ void eps_walk(const float val[N], float out[N]) {
  float old = FLT_MAX;
#pragma unroll
  for (int x = 0; x < N; ++x) {
    const float v = val[x];
    // SVR: |d| < 0.00001 (double) == |d| <= 0.00001f; PVR: |d| < 0.00001f.  NaN compares false -> processed
    const bool skip = PVR ? (__builtin_fabsf(old - v) < PSF_EPS_F) : (__builtin_fabsf(old - v) <= PSF_EPS_F);
    out[x] = skip ? (ZERO ? -0.0f : -1.0f) : v;
    old = skip ? old : v;
  }
}
template <int N, bool PVR, bool ZERO = false, int HP = 0>
__device__ __forceinline__ void eval_row_t(const RowConst S, float bx, float by, float bz, float fy,
                                           float fz, float out[N]) {
  float val[N];
  eval_row_vals<N, PVR, HP>(S, bx, by, bz, fy, fz, val);
  eps_walk<N, PVR, ZERO>(val, out);
}
template <int N, bool PVR, int HP>
__device__ __forceinline__ void eval_row_vals(const RowConst S, float bx, float by, float bz, float fy, float fz, float val[N]) {
  // Taps are evaluated two per lane in float2 registers: every fma / mul / add stage of eval_pairs_xyz
  // compiles to v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 (half the issue slots for the same cycles);
  // sqrt, rcp, rint and the selects stay per component.  Pair j holds the taps at lattice offsets -j and 1 + j
  // (the order of the Gaussian recurrence, gauss_pairs); the in-plane part is evaluated in two chunks of N/4 pairs.
  constexpr int NP = N / 2;
#ifndef SVR_EVAL_H16
#define SVR_EVAL_H16 4
#endif
  constexpr int H = HP ? HP : (N == 16 ? SVR_EVAL_H16 : NP / 2);   // pairs evaluated side by side (instruction-level parallelism against registers)
  constexpr int CENTRE = (N - 1) / 2;
  static_assert(NP % H == 0 && CENTRE == NP - 1, "pairs (-j, 1 + j) around the central taps");
  const float rowx = __builtin_fmaf(S.Lp[1], fy, __builtin_fmaf(S.Lp[2], fz, bx));
  const float rowy = __builtin_fmaf(S.Lp[4], fy, __builtin_fmaf(S.Lp[5], fz, by));
  const float rowz = __builtin_fmaf(S.Lp[7], fy, __builtin_fmaf(S.Lp[8], fz, bz));
  GaussStep st = gauss_start(S, rowz);
#pragma unroll
  for (int c0 = 0; c0 < NP; c0 += H) {
    f2 xs[H], ys[H], v2[H], g[H];
#pragma unroll
    for (int i = 0; i < H; ++i) {
      const f2 fx = (f2){(float)(-(c0 + i)), (float)(1 + c0 + i)};
      xs[i] = fma2(bc2(S.Lp[0]), fx, bc2(rowx));
      ys[i] = fma2(bc2(S.Lp[3]), fx, bc2(rowy));
    }
    eval_pairs_xyz<H, PVR>(S, xs, ys, v2);
    gauss_pairs<H>(S, rowz, st, c0, g);
#pragma unroll
    for (int i = 0; i < H; ++i) {
      const f2 v = v2[i] * g[i];                        // (si * si) * gz
      val[CENTRE - (c0 + i)] = v.x;
      val[CENTRE + 1 + c0 + i] = v.y;
    }
  }
}
// Can every tap of the (fy, fz) row be proven to lie below the epsilon of the skip test?  Then the
// reference processes only the row's first tap (oldPSF starts at FLT_MAX) and skips the other 15:
// |v0 - v| <= max(v0, v) < 1e-5.  Upper bound of the canonical value over the row:
//   exp(-a_min) * min(1, 1 / (pi^2 q_min)),
// a_min from the end taps (z' is monotone in x, and so is its rounded fma), q_min from the vertex of the
// quadratic x'^2 + y'^2 shrunk by 1 % (covers the roundings of x', y', q), both with the polynomial errors
// of the canonical sin / exp (< 1e-6) far inside the 2 % margin of the threshold.  A row that may contain
// the R = 0 tap (NaN, RC.cu:129) is never declared dead.
__host__ __device__ __forceinline__ bool row_is_dead(const RowConst S, float bx, float by, float bz, float fy, float fz) {
  const float rowx = __builtin_fmaf(S.Lp[1], fy, __builtin_fmaf(S.Lp[2], fz, bx));
  const float rowy = __builtin_fmaf(S.Lp[4], fy, __builtin_fmaf(S.Lp[5], fz, by));
  const float rowz = __builtin_fmaf(S.Lp[7], fy, __builtin_fmaf(S.Lp[8], fz, bz));
  const float z0 = __builtin_fmaf(S.Lp[6], (float)(-PSF_CENTRE), rowz);
  const float z1 = __builtin_fmaf(S.Lp[6], (float)(PSF_SUPPORT - 1 - PSF_CENTRE), rowz);
  const float zmin = (z0 > 0.0f) == (z1 > 0.0f) && z0 != 0.0f && z1 != 0.0f ? fminf(fabsf(z0), fabsf(z1)) : 0.0f;
  const float amin = (zmin * zmin) * S.inv2s2;
  const float qa = S.Lp[0] * S.Lp[0] + S.Lp[3] * S.Lp[3];
  const float qb = 2.0f * (S.Lp[0] * rowx + S.Lp[3] * rowy);
  const float qc = rowx * rowx + rowy * rowy;
  float fx = qa > 1e-12f ? -qb / (2.0f * qa) : 0.0f;
  fx = fminf(fmaxf(fx, (float)(-PSF_CENTRE)), (float)(PSF_SUPPORT - 1 - PSF_CENTRE));
  const float qe0 = (qa * (float)(PSF_CENTRE * PSF_CENTRE) - qb * (float)PSF_CENTRE) + qc;
  const float e1 = (float)(PSF_SUPPORT - 1 - PSF_CENTRE);
  const float qe1 = (qa * (e1 * e1) + qb * e1) + qc;
  const float qv = (qa * (fx * fx) + qb * fx) + qc;
  const float qmin = fmaxf(fminf(qv, fminf(qe0, qe1)), 0.0f) * 0.99f - 1e-5f;
  if (!(qmin > 1e-6f)) return false;   // may contain the R = 0 tap: keep the row live
  // ln(1e5 / 0.98) = 11.533
#ifndef SVR_DEAD_THR
#define SVR_DEAD_THR 11.56f
#endif
  return amin + logf(fmaxf(1.0f, 9.8696044f * qmin)) > SVR_DEAD_THR;
}

__device__ __forceinline__ void eval_row_at(const RowConst S, float bx, float by, float bz, float fy,
                                            float fz, float out[16]) {
  eval_row_t<16, false>(S, bx, by, bz, fy, fz, out);
}
// Phase 1 of the wave-per-pixel kernels: lane = one (y,z) row of quarter q (4 z-planes x 16 y)
__device__ __forceinline__ void eval_row(const RowConst S, const PixelState &P, int lane, int q,
                                         float out[16]) {
  eval_row_at(S, P.bx, P.by, P.bz, (float)((lane & 15) - PSF_CENTRE), (float)(4 * q + (lane >> 4) - PSF_CENTRE), out);
}

__device__ __forceinline__ uint32_t sat0(int i) { return (uint32_t)max(i, 0); }  // float->uint saturation

template <int MODE>
__global__ __launch_bounds__(WAVES_PER_BLOCK * 64) void psf_kernel(PsfArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[WAVES_PER_BLOCK][64 * LDS_ROW];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const uint32_t pi = blockIdx.x * WAVES_PER_BLOCK + wave;
  if (pi >= a.n) return;
  const uint32_t idx = __builtin_amdgcn_readfirstlane(a.list[pi]);
  const uint32_t n2 = (uint32_t)(a.sx * a.sy);
  const uint32_t sl = idx / n2;
  const uint32_t rem = idx - sl * n2;
  const int py = (int)(rem / (uint32_t)a.sx);
  const int px = (int)(rem - (uint32_t)py * (uint32_t)a.sx);
  const SliceConst &S = a.sc[sl];
  const VolGeom &vg = a.vg;
  const PixelState P = pixel_setup(S, vg, px, py);
  const RowConst RC = load_row_const(S);
  float *my = lds[wave];

  float s = a.slices[idx];
  float sume;
  if (MODE == MODE_GAUSS) {
    // pass 1 (RC.cu:228-258): sume over processed, in-bounds taps (truncating cast, no mask)
    double acc = 0.0;
    for (int q = 0; q < 4; ++q) {
      float out[16];
      eval_row(RC, P, lane, q, out);
      const uint32_t az = sat0(P.czi + 4 * q + (lane >> 4) - PSF_CENTRE);
      const uint32_t ay = sat0(P.cyi + (lane & 15) - PSF_CENTRE);
      const bool rowin = az < (uint32_t)vg.vz && ay < (uint32_t)vg.vy;
#pragma unroll
      for (int x = 0; x < 16; ++x) {
        const uint32_t ax = sat0(P.cxi + x - PSF_CENTRE);
        const bool use = rowin && ax < (uint32_t)vg.vx && !(out[x] < 0.0f);
        acc += use ? (double)out[x] : 0.0;
      }
    }
    sume = (float)wave_sum(acc);
    if (!(sume > 0.5f)) return;          // also drops NaN (RC.cu:251-258)
    if (lane == 0) a.psf_sums[idx] = sume;
    s = a.bias ? s * expf(-a.bias[idx]) * a.scales[sl] : s * a.scales[sl];   // RC.cu:200-203
  } else {
    sume = a.psf_sums[idx];
  }
  if (MODE == MODE_BIAS) {
    // normalizeBiasKernel3D_tex RC.cu:544-550: the scattered value is the pixel's log bias
    s = a.bias[idx];
    const float scale = a.scales[sl];
    if (scale > 0) s -= logf(scale);
  }

  float f0 = 0.0f, f1 = 0.0f;   // FWD: sim, weight partials.  BACK: (w*sw*e)/sume, (w*sw)/sume
  if (MODE == MODE_BACK) {
    float w = a.weights[idx];
    float ss = a.simslices[idx];
    float e = a.bias ? s * expf(-a.bias[idx]) * a.scales[sl] : s * a.scales[sl];   // RC.cu:439-442
    e = (ss > 0.0f) ? (e - ss) : 0.0f;   // RC.cu:444-447
    float ws = w * a.slice_weights[sl];
    f1 = ws / sume;
    f0 = f1 * e;
  }
  const float rsume = 1.0f / sume;
  bool hit = false;
  const int x2 = lane & 15, r4 = lane >> 4;
  const uint32_t ax = sat0(P.cxi + x2 - PSF_CENTRE);
  const bool xin = ax < (uint32_t)vg.vx;

  for (int q = 0; q < 4; ++q) {
    {
      float out[16];
      eval_row(RC, P, lane, q, out);
      float4 *dst = reinterpret_cast<float4 *>(my + lane * LDS_ROW);
      dst[0] = make_float4(out[0], out[1], out[2], out[3]);
      dst[1] = make_float4(out[4], out[5], out[6], out[7]);
      dst[2] = make_float4(out[8], out[9], out[10], out[11]);
      dst[3] = make_float4(out[12], out[13], out[14], out[15]);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // Phase 2: lane = (x, 4 consecutive y rows): coalesced 4 x 64 B volume accesses
    for (int j = 0; j < 16; ++j) {
      const int row = 4 * j + r4;
      const float val = my[row * LDS_ROW + x2];
      const uint32_t az = sat0(P.czi + 4 * q + (row >> 4) - PSF_CENTRE);
      const uint32_t ay = sat0(P.cyi + (row & 15) - PSF_CENTRE);
      const bool ok = xin && ay < (uint32_t)vg.vy && az < (uint32_t)vg.vz && !(val < 0.0f);
      if (ok) {
        const uint32_t vi = ax + ay * (uint32_t)vg.vx + az * (uint32_t)(vg.vx * vg.vy);
        if (a.mask[vi] != 0.0f) {
          if (MODE == MODE_GAUSS || MODE == MODE_BIAS) {
            float p = val / sume;                       // RC.cu:278, 591
            unsafeAtomicAdd(a.volw + vi, p);
            unsafeAtomicAdd(a.recon + vi, p * s);
          } else if (MODE == MODE_FWD) {
            float p = val * rsume;
            f0 += p * a.vol[vi];
            f1 += p;
          } else {
            unsafeAtomicAdd(a.addon + vi, val * f0);
            unsafeAtomicAdd(a.cmap + vi, val * f1);
          }
          hit = true;
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }

  if (MODE == MODE_GAUSS) {
    if (__ballot(hit) != 0ull && lane == 0) a.voxcount[idx] = 1;   // RC.cu:291-294
  } else if (MODE == MODE_FWD) {
    float sim = wave_sum(f0), w = wave_sum(f1);
    bool inside = __ballot(hit) != 0ull;
    if (lane == 0 && w > 0.0f) {                                    // RC.cu:398-403
      a.simslices[idx] = sim / w;
      a.simweights[idx] = w;
      a.siminside[idx] = inside ? 1 : 0;
    }
  }
}


// ------------------------------------------------------------------------------------------
// LDS-tiled back-projection (SuperresolutionKernel3D_tex RC.cu:408-522)
// ------------------------------------------------------------------------------------------
// One workgroup owns a TW x TH tile of slice pixels.  The union of their 16^3 footprints (after
// the float->uint saturation) is a small box of the volume; {addon, cmap} for that box live in
// LDS, every wave scatters its pixels' taps with ds_add_f32 straight from the row-per-lane
// layout (no transposition needed: LDS has no coalescing rule), and the box is flushed to HBM
// once with the mask test applied per voxel instead of per tap.  This removes ~95 % of the
// device-scope float atomics of the direct kernel, which are what bound it (profiles/r01_a).
#define TILE_WAVES 16

struct TileArgs {
  const uint32_t *tiles;   // tile ids: (slice * tiles_y + ty) * tiles_x + tx
  uint32_t ntiles;
  int tiles_x, tiles_y;
  int cap;                 // voxels of LDS accumulator available
  int tw, th;              // tile size in pixels, tw * th <= 64
  int gauss;               // scatter kernels: 1 = Gaussian-reconstruction pass 2 (recon|volw instead of addon|cmap)
};

// activity of a pixel for the tile kernels: s != -1 and (flag ? flag : v_PSF_sums != 0); both NULL: s != -1
__device__ __forceinline__ bool pixel_active(const float *slices, const float *psf_sums, const unsigned char *flag,
                                             size_t idx) {
  if (slices[idx] == -1.0f) return false;
  if (flag) return flag[idx] != 0;
  return psf_sums ? psf_sums[idx] != 0.0f : true;
}

__global__ void k_build_tiles(const float *slices, const float *psf_sums, const unsigned char *flag, int sx, int sy,
                              int ns, int tiles_x, int tiles_y, int TILE_W, int TILE_H, uint32_t *tiles,
                              uint32_t *counter, const unsigned char *slice_sel = nullptr, int want = 0, uint32_t t0 = 0u,
                              uint32_t t_end = 0xFFFFFFFFu) {
  const int lane = threadIdx.x & 63;
  const uint32_t t = t0 + blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);   // (t0 .. t_end: this dispatch's piece of the candidates)
  const uint32_t total = min((uint32_t)tiles_x * tiles_y * ns, t_end);
  const uint32_t tt = t < total ? t : 0u;                  // (every wavefront reaches the barriers below)
  const int sl = tt / (tiles_x * tiles_y);
  const bool skip = slice_sel && slice_sel[sl] != want;
  const int r = tt - sl * tiles_x * tiles_y;
  const int ty = r / tiles_x, tx = r - ty * tiles_x;
  const int px = tx * TILE_W + (lane % TILE_W), py = ty * TILE_H + (lane / TILE_W);
  bool act = false;
  if (lane < TILE_W * TILE_H && px < sx && py < sy) {
    size_t idx = (size_t)px + (size_t)py * sx + (size_t)sl * sx * sy;
    act = pixel_active(slices, psf_sums, flag, idx);
  }
  // one atomic on the global counter per workgroup, not per tile (168 k tiles on one address took 1.2 ms on P4)
  __shared__ uint32_t sh_n, sh_base, sh_t[16];
  if (threadIdx.x == 0) sh_n = 0;
  __syncthreads();
  const bool keep = t < total && !skip && __ballot(act) != 0ull;
  if (keep && lane == 0) sh_t[atomicAdd(&sh_n, 1u)] = t;
  __syncthreads();
  if (threadIdx.x == 0 && sh_n) sh_base = atomicAdd(counter, sh_n);
  __syncthreads();
  if (threadIdx.x < sh_n) tiles[sh_base + threadIdx.x] = sh_t[threadIdx.x];
}

// XCD-aware tile index.  Workgroups are handed to the eight XCDs round-robin by their index and every XCD has its own L2.
// The tile lists are (roughly) in raster order, so with the plain index an XCD sees every eighth tile and shares no box
// with its own previous tile; with this permutation every XCD takes runs of SVR_XCD_RUN neighbouring tiles, whose boxes of
// the volume overlap, while the eight XCDs still advance through the list together (measured on the gather of P4:
// 4.60 -> 4.47 ms with runs of 16; a coarser split -- whole slices per XCD -- lost to load imbalance).
#ifndef SVR_XCD_RUN
#define SVR_XCD_RUN 16
#endif
__device__ __forceinline__ uint32_t xcd_run_index(uint32_t b, uint32_t n) {
  if (SVR_XCD_RUN <= 0) return b;
  constexpr uint32_t R = SVR_XCD_RUN > 0 ? SVR_XCD_RUN : 1, G = 8u * R;
  const uint32_t base = b / G * G;
  if (base + G > n) return b;                             // the last, incomplete group keeps its order
  const uint32_t q = b - base;
  return base + (q & 7u) * R + (q >> 3);
}


struct PixelRec {      // per tile pixel, in LDS
  int cx, cy, cz;
  float bx, by, bz;
  float f0, f1;
};

#define SLOT_MAXP 48      // planes of a box the plane tables are sized for
struct RowWalk {       // i = y * P + x walked in steps of `stride` without a division per element
  int x, y, tx, ty, P;
  __device__ __forceinline__ void init(int i0, int stride, int P_) {
    P = P_;
    y = i0 / P; x = i0 - y * P;
    ty = stride / P; tx = stride - ty * P;
  }
  __device__ __forceinline__ void step() {
    x += tx; y += ty;
    if (x >= P) { x -= P; ++y; }
  }
};

// Is every tap of the unit (all x, all offsets of the lane axis, fixed offset `fo` of volume axis F in {1, 2}) provably
// below the epsilon of the skip test, and free of the R = 0 tap?  |z'| is bounded from below over the unit's lattice
// square (z' is affine), exp(-a_min) with sinc^2 <= 1 bounds the value; the R = 0 tap (NaN, RC.cu:129 -- it would be
// processed, and so would every tap after it in its row) is excluded by evaluating q at the lattice points around the
// real solution of x' = y' = 0.  A degenerate in-plane map (rows along the slice normal) never takes the shortcut.
__device__ __forceinline__ bool unit_is_dead(const RowConst S, float bx, float by, float bz, int F, float fo) {
  const bool f1 = F == 1;                               // (selects, not indexing: an index would put RowConst into scratch)
  const float LxF = f1 ? S.Lp[1] : S.Lp[2], LxG = f1 ? S.Lp[2] : S.Lp[1];
  const float LyF = f1 ? S.Lp[4] : S.Lp[5], LyG = f1 ? S.Lp[5] : S.Lp[4];
  const float LzF = f1 ? S.Lp[7] : S.Lp[8], LzG = f1 ? S.Lp[8] : S.Lp[7];
  const float lo_ = (float)(-PSF_CENTRE), hi_ = (float)(PSF_SUPPORT - 1 - PSF_CENTRE);
  const float c = __builtin_fmaf(LzF, fo, bz);
  const float zlo = c + fminf(S.Lp[6] * lo_, S.Lp[6] * hi_) + fminf(LzG * lo_, LzG * hi_);
  const float zhi = c + fmaxf(S.Lp[6] * lo_, S.Lp[6] * hi_) + fmaxf(LzG * lo_, LzG * hi_);
  if (!(zlo > 0.0f || zhi < 0.0f)) return false;
  const float zmin = fminf(fabsf(zlo), fabsf(zhi)) * 0.999f - 1e-4f;      // covers the roundings of the fma chains of z'
  if (!(zmin > 0.0f && (zmin * zmin) * S.inv2s2 > SVR_DEAD_THR)) return false;
  if (S.invD == 0.0f) return false;                     // degenerate in-plane map: no shortcut
  const float cx = __builtin_fmaf(LxF, fo, bx), cy = __builtin_fmaf(LyF, fo, by);
  const float ox = (cy * LxG - cx * LyG) * S.invD, og = (cx * S.Lp[3] - cy * S.Lp[0]) * S.invD;
  if (!(fabsf(ox) < 64.0f && fabsf(og) < 64.0f)) return true;             // the zero of (x', y') is far outside the lattice
  const float fx0 = floorf(ox), fg0 = floorf(og);
  bool zero = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float fx = fx0 + (float)(j & 1), fg = fg0 + (float)(j >> 1);
    const float fy = f1 ? fo : fg, fz = f1 ? fg : fo;
    const float xs = __builtin_fmaf(S.Lp[0], fx, __builtin_fmaf(S.Lp[1], fy, __builtin_fmaf(S.Lp[2], fz, bx)));
    const float ys = __builtin_fmaf(S.Lp[3], fx, __builtin_fmaf(S.Lp[4], fy, __builtin_fmaf(S.Lp[5], fz, by)));
    zero = zero || __builtin_fmaf(ys, ys, xs * xs) == 0.0f;
  }
  return !zero;
}

// 16 bytes of the coefficient table: read once per pass and never again before the next one, so the load is marked
// non-temporal (it should not push the volume, the mask and the slice data out of the L2 / the memory-side cache)
typedef float nt_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 load_stream(const float4 *p) {
  const nt_f4 v = __builtin_nontemporal_load(reinterpret_cast<const nt_f4 *>(p));
  return make_float4(v.x, v.y, v.z, v.w);
}

// 16 bytes per lane from global memory straight into the LDS (LDS-DMA, gfx950: global_load_lds_dwordx4): lane l's 16 bytes land at
// lds_dst + 16 l (lds_dst: wave-uniform LDS byte address).  No VGPR is the destination, so nothing the compiler can copy, spill or wait for:
// the data is in flight for as long as the kernel likes, and the kernel counts its completion itself (glds_wait) before it reads the LDS.
// M0 holds the destination and is compiler-reserved: saved and restored inside the statement.  (hipcc does not count this load in its
// own s_waitcnt bookkeeping; an uncounted older operation only makes the compiler's counted waits stricter, never looser: vmcnt is in order.)
// The stage written here is one the wavefront has read before (ds_read): the statement opens with s_waitcnt lgkmcnt(0), so that every LDS read
// issued so far has returned before the DMA can write over its source -- the "memory" clobber orders the issue only, not the completion.
__device__ __forceinline__ void glds16(const void *gsrc, uint32_t lds_dst) {
  unsigned keep;
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
// wait until at most N vector-memory operations of this wavefront are outstanding (N an immediate), then the LDS may be read
template <int N>
__device__ __forceinline__ void glds_wait() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); }

// 16 bytes per lane from global memory into a VGPR quad, non-temporal, OFF bytes beyond gsrc (an immediate), by a load that hipcc does not count:
// the compiler puts no s_waitcnt of its own in front of the registers' readers and has no reason to park them in copies behind one, so the data
// stay in flight until the kernel's own wait (gload_wait), which names every destination register of the unit about to be used as "+v" -- no
// consumer can be scheduled above it.  Until then `dst` is not to be read, copied or left to die: a unit that is not used is still waited for.
// (As with glds16: an operation hipcc does not count only makes its own counted waits stricter, vmcnt returns in order.)
template <int OFF>
__device__ __forceinline__ void gload16(const void *gsrc, nt_f4 &dst) {
  asm volatile("global_load_dwordx4 %0, %1, off offset:%2 nt" : "=&v"(dst) : "v"(gsrc), "n"(OFF) : "memory");
}
// wait until at most N vector-memory operations are outstanding; the four quads of one row (support 16) / of two rows become readable
template <int N>
__device__ __forceinline__ void gload_wait(nt_f4 (&r)[4]) {
  asm volatile("s_waitcnt vmcnt(%4)" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]) : "n"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void gload_wait(nt_f4 (&r)[4], nt_f4 (&s)[4]) {
  asm volatile("s_waitcnt vmcnt(%8)" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(s[0]), "+v"(s[1]), "+v"(s[2]), "+v"(s[3]) : "n"(N) : "memory");
}
__device__ __forceinline__ uint32_t lds_addr_of(const void *p) { return (uint32_t)(uintptr_t)p; }   // (a generic pointer into the LDS: aperture in the high half, LDS byte address in the low)

#ifndef SVR_COEFF_STORE_NT
#define SVR_COEFF_STORE_NT 1
#endif
__device__ __forceinline__ void store_stream(float4 *p, float a, float b, float c, float d) {
#if SVR_COEFF_STORE_NT
  __builtin_nontemporal_store((nt_f4){a, b, c, d}, reinterpret_cast<nt_f4 *>(p));
#else
  *p = make_float4(a, b, c, d);
#endif
}
#include "svr_coeff.h"     // the coefficient table's layout: CoeffLayout, coeff_row and the row loads / stores on the three functions above

// The coefficient table's writer: one wavefront per pixel, four of its NS units per pass -- slot = unit, lane = row.
template <int NS, bool PVR>
__global__ __launch_bounds__(256) void k_coeff_build(PsfArgs a, float4 *coeff, uint32_t *coeff_id, uint32_t base) {
  constexpr int NC = (NS - 1) / 2;
  const uint32_t wl = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (wl >= a.n) return;
  const int lane = threadIdx.x & 63;
  const uint32_t idx = a.list[wl];
  const uint32_t w = base + wl;                          // the pixel's id in the table (the list goes out in pieces)
  const uint32_t n2 = (uint32_t)(a.sx * a.sy);
  const uint32_t sl = idx / n2, rem = idx - sl * n2;
  const int py = (int)(rem / (uint32_t)a.sx), px = (int)(rem - (uint32_t)py * (uint32_t)a.sx);
  const SliceConst &S = a.sc[sl];
  const PixelState P = pixel_setup(S, a.vg, px, py);
  const RowConst RC = load_row_const(S);
  const bool swap = S.own == 1;
  const int F = swap ? 1 : 2;
  if (lane == 0) coeff_id[idx] = w;
  const int slot = lane >> 4, y = lane & 15;
  const float fyl = (float)(y - NC);
  for (int g = 0; 4 * g < NS; ++g) {
    const int u = 4 * g + slot;
    const float fu = (float)(u - NC);
    const bool dead = !PVR && unit_is_dead(RC, P.bx, P.by, P.bz, F, fu);   // (the bound is derived for the SVR constants)
    if (__all(dead)) continue;
    float out[NS];
    eval_row_t<NS, PVR, true>(RC, P.bx, P.by, P.bz, swap ? fu : fyl, swap ? fyl : fu, out);
    if (!dead && u < NS && y < NS) coeff_store_row<NS>(coeff_row<NS>(coeff, w, u, y), out);
  }
}



// getReconValueFromTexture (R2/reconVolume.cu:170-187): linear filter at the un-offset coordinate =
// 0.125 * sum over {p-1,p}^3 with zero border
__device__ __forceinline__ float pvr_tex(const float *vol, const VolGeom &vg, int X, int Y, int Z) {
  float v = 0.0f;
#pragma unroll
  for (int dz = -1; dz <= 0; ++dz)
#pragma unroll
    for (int dy = -1; dy <= 0; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 0; ++dx) {
        const int x = X + dx, y = Y + dy, z = Z + dz;
        const float t = (x >= 0 && y >= 0 && z >= 0) ? vol[(size_t)x + (size_t)y * vg.vx + (size_t)z * vg.vx * vg.vy] : 0.0f;
        v += 0.125f * t;
      }
  return v;
}

// Sum over the 16 lanes of a slot, result in the slot's first lane: four DPP row shifts folded into the additions
// (v_add_f32_dpp) instead of four dependent ds_bpermute round trips through the LDS crossbar.  Lanes shifted in from
// beyond the row read 0 (bound_ctrl), so the tree is ((v0 + v8) + (v4 + v12)) + ... -- fixed, the same for every unit.
template <int N> __device__ __forceinline__ int row_shl_i(int v) {
  return __builtin_amdgcn_update_dpp(0, v, 0x100 + N, 0xF, 0xF, true);
}
template <int N> __device__ __forceinline__ float row_shl_f(float v) {
  return __builtin_bit_cast(float, row_shl_i<N>(__builtin_bit_cast(int, v)));
}
template <int N> __device__ __forceinline__ double row_shl_d(double v) {
  const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)row_shl_i<N>((int)(unsigned)b), hi = (unsigned)row_shl_i<N>((int)(unsigned)(b >> 32));
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ float row_sum16(float v) {
  v += row_shl_f<8>(v); v += row_shl_f<4>(v); v += row_shl_f<2>(v); v += row_shl_f<1>(v);
  return v;
}
__device__ __forceinline__ double row_sum16(double v) {
  v += row_shl_d<8>(v); v += row_shl_d<4>(v); v += row_shl_d<2>(v); v += row_shl_d<1>(v);
  return v;
}
#include "svr_tile.inc"    // the tile kernels of rounds 1-2: back_tiled_kernel, back_slot_kernel, back_wave_kernel (back_mode 1 / 3 / 4), fwd_unit_kernel (fwd_mode 1)

// ------------------------------------------------------------------------------------------
// Patch-to-volume (PVR) PSF kernels -- first correct version
// ------------------------------------------------------------------------------------------
// patchBasedPSFReconstructionKernel (R2/patchBasedPSFReconstruction_gpu.cu:41-145),
// patchBasedSimulatePatchesKernel (R2/patchBasedSimulatePatches_gpu.cu:41-125),
// patchBasedSuperresolution_gpuKernel (R2/patchBasedSuperresolution_gpu.cu:34-111).
// Patches are the "slices" of the padded grid [nPatches][pY][pX]; support 12^3, sigma_z = dim.z,
// through-plane offset / 2.5, sinc_pi, pixel kept if sume > 1e-5 or NaN, optional superpixel mask.
// One wavefront per patch pixel; lane = one of the 144 (y,z) rows (3 passes), 12 x-taps each, the
// volume is accessed straight from the row-per-lane layout (not yet tiled like the SVR scatter).
#define PVR_N 12
#define PVR_CENTRE 5

#define MODE_GAUSS2 4      // pass 2 of the Gaussian reconstruction only (v_PSF_sums from the tiled pass 1)
template <int MODE>
__device__ __forceinline__ void pvr_pixel(const PsfArgs &a, uint32_t idx, int lane) {
  const uint32_t n2 = (uint32_t)(a.sx * a.sy);
  const uint32_t sl = idx / n2;
  const uint32_t rem = idx - sl * n2;
  const int py = (int)(rem / (uint32_t)a.sx);
  const int px = (int)(rem - (uint32_t)py * (uint32_t)a.sx);
  const SliceConst &S = a.sc[sl];
  const VolGeom &vg = a.vg;
  const PixelState P = pixel_setup(S, vg, px, py);
  const RowConst RC = load_row_const(S);
  float s = a.slices[idx] * a.scales[sl];                 // s * patch.scale
  float sume;
  if (MODE == MODE_GAUSS) {
    double acc = 0.0;
    const bool spx_ok = !a.spx || a.spx[(size_t)sl * 4096 + px + 64 * py] == '1';
    if (spx_ok) {
      for (int p = 0; p < 3; ++p) {
        const int r = p * 64 + lane;
        const bool valid = r < PVR_N * PVR_N;
        const int z = r / PVR_N, y = r - z * PVR_N;
        float out[PVR_N];
        eval_row_t<PVR_N, true>(RC, P.bx, P.by, P.bz, (float)(y - PVR_CENTRE), (float)(z - PVR_CENTRE), out);
        const uint32_t az = sat0(P.czi + z - PVR_CENTRE), ay = sat0(P.cyi + y - PVR_CENTRE);
        const bool rowin = valid && az < (uint32_t)vg.vz && ay < (uint32_t)vg.vy;
#pragma unroll
        for (int x = 0; x < PVR_N; ++x) {
          const uint32_t ax = sat0(P.cxi + x - PVR_CENTRE);
          acc += (rowin && ax < (uint32_t)vg.vx && !(out[x] < 0.0f)) ? (double)out[x] : 0.0;
        }
      }
    }
    sume = (float)wave_sum(acc);
    if (!((sume > 0.00001f) || (sume != sume))) return;   // patchBasedPSFReconstruction_gpu.cu:110
    if (lane == 0) a.psf_sums[idx] = sume;
  } else {
    sume = a.psf_sums[idx];
  }
  float f0 = 0.0f, f1 = 0.0f;
  if (MODE == MODE_BACK) {
    const float ss = a.simslices[idx];
    const float e = (ss > 0.0f) ? (s - ss) : 0.0f;         // patchBasedSuperresolution_gpu.cu:64-67
    f1 = a.weights[idx] * a.slice_weights[sl];             // w * patch_weight
    f0 = f1 * e;
  }
  bool hit = false;
  for (int p = 0; p < 3; ++p) {
    const int r = p * 64 + lane;
    const bool valid = r < PVR_N * PVR_N;
    const int z = r / PVR_N, y = r - z * PVR_N;
    float out[PVR_N];
    eval_row_t<PVR_N, true>(RC, P.bx, P.by, P.bz, (float)(y - PVR_CENTRE), (float)(z - PVR_CENTRE), out);
    const uint32_t az = sat0(P.czi + z - PVR_CENTRE), ay = sat0(P.cyi + y - PVR_CENTRE);
    const bool rowin = valid && az < (uint32_t)vg.vz && ay < (uint32_t)vg.vy;
    if (!rowin) continue;
#pragma unroll
    for (int x = 0; x < PVR_N; ++x) {
      const uint32_t ax = sat0(P.cxi + x - PVR_CENTRE);
      if (ax < (uint32_t)vg.vx && !(out[x] < 0.0f)) {
        const uint32_t vi = ax + ay * (uint32_t)vg.vx + az * (uint32_t)(vg.vx * vg.vy);
        if (a.mask[vi] != 0.0f) {
          const float pv = out[x] / sume;
          if (MODE == MODE_GAUSS || MODE == MODE_GAUSS2) {
            unsafeAtomicAdd(a.volw + vi, pv);
            unsafeAtomicAdd(a.recon + vi, s * pv);
          } else if (MODE == MODE_FWD) {
            f0 += pv * pvr_tex(a.vol, vg, (int)ax, (int)ay, (int)az);
            f1 += pv;
          } else {
            unsafeAtomicAdd(a.addon + vi, pv * f0);
            unsafeAtomicAdd(a.cmap + vi, pv * f1);
          }
          hit = true;
        }
      }
    }
  }
  if (MODE == MODE_GAUSS) {
    if (__ballot(hit) != 0ull && lane == 0) a.voxcount[idx] = 1;
  } else if (MODE == MODE_FWD) {
    const float sim = wave_sum(f0), w = wave_sum(f1);
    const bool inside = __ballot(hit) != 0ull;
    if (lane == 0 && w > 0.0f) {
      a.simslices[idx] = sim / w;
      a.simweights[idx] = w;
      a.siminside[idx] = inside ? 1 : 0;
    }
  }
}

template <int MODE>
__global__ __launch_bounds__(WAVES_PER_BLOCK * 64) void pvr_kernel(PsfArgs a) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const uint32_t pi = blockIdx.x * WAVES_PER_BLOCK + wave;
  if (pi >= a.n) return;
  pvr_pixel<MODE>(a, __builtin_amdgcn_readfirstlane(a.list[pi]), lane);
}

// fallback of the tiled PVR scatter: the pixels of the listed tiles with device atomics (MODE_BACK / MODE_GAUSS2)
template <int MODE>
__global__ __launch_bounds__(WAVES_PER_BLOCK * 64) void pvr_tiles_kernel(PsfArgs a, TileArgs ta) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const uint32_t t = ta.tiles[blockIdx.x];
  const int per_slice = ta.tiles_x * ta.tiles_y;
  const uint32_t sl = t / per_slice;
  const int r = t - sl * per_slice;
  const int ty = r / ta.tiles_x, tx = r - ty * ta.tiles_x;
  for (int k = wave; k < ta.tw * ta.th; k += WAVES_PER_BLOCK) {
    const int px = tx * ta.tw + k % ta.tw, py = ty * ta.th + k / ta.tw;
    if (px >= a.sx || py >= a.sy) continue;
    const uint32_t idx = (uint32_t)px + (uint32_t)py * a.sx + sl * (uint32_t)(a.sx * a.sy);
    if (pixel_active(a.slices, a.psf_sums, a.flag, idx)) pvr_pixel<MODE>(a, idx, lane);
  }
}

// test probe: one wave evaluates one pixel; out[x + 16*y + 256*z] = psf or -1 when skipped
__global__ __launch_bounds__(64) void k_probe_pixel(PsfArgs a, uint32_t idx, float *out, int *centre) {
  const int lane = threadIdx.x & 63;
  const uint32_t n2 = (uint32_t)(a.sx * a.sy);
  const uint32_t sl = idx / n2;
  const uint32_t rem = idx - sl * n2;
  const int py = (int)(rem / (uint32_t)a.sx);
  const int px = (int)(rem - (uint32_t)py * (uint32_t)a.sx);
  const SliceConst &S = a.sc[sl];
  const PixelState P = pixel_setup(S, a.vg, px, py);
  const RowConst RC = load_row_const(S);
  if (a.vg.pvr) {
    for (int p = 0; p < 3; ++p) {
      const int r = p * 64 + lane;
      if (r >= PVR_N * PVR_N) continue;
      const int z = r / PVR_N, y = r - z * PVR_N;
      float v[PVR_N];
      eval_row_t<PVR_N, true>(RC, P.bx, P.by, P.bz, (float)(y - PVR_CENTRE), (float)(z - PVR_CENTRE), v);
#pragma unroll
      for (int x = 0; x < PVR_N; ++x) out[x + 16 * y + 256 * z] = v[x];
    }
  } else {
    for (int q = 0; q < 4; ++q) {
      float v[16];
      eval_row(RC, P, lane, q, v);
      const int z = 4 * q + (lane >> 4), y = lane & 15;
#pragma unroll
      for (int x = 0; x < 16; ++x) out[x + 16 * y + 256 * z] = v[x];
    }
  }
  if (lane == 0) { centre[0] = P.cxi; centre[1] = P.cyi; centre[2] = P.czi; }
}

#include "svr_small.inc"   // list compaction, reductions, the EM / scale / bias / volume kernels
#include "svr_bias.inc"    // the bias path's Gaussians through the LDS (bias_mode 1)

}  // namespace

// ==========================================================================================
// context
// ==========================================================================================
struct RegState;   // GPU slice-to-volume registration state (svr_reg.inc)
namespace { struct CellState; struct SlabPlan; struct SliceEm; void slice_em_free(SliceEm *); void slice_em_invalidate(SliceEm *); }  // sorted pixels, runs, items and staging of the scatter without atomics (svr_cell.inc)
namespace {
// The coefficient table: what irtkReconstruction::CoeffInit keeps as _volcoeffs on the CPU path (RG.cc:2305-2673) --
// every PSF pixel's evaluated taps, 16 KiB per pixel, written once per slice geometry by k_coeff_build and streamed by
// the COEFF instantiations of the scatter and the gather instead of being re-evaluated in every SR iteration.  The
// reference's GPU path recomputes them (a 2015 GPU had 6-12 GB); 288 GB of HBM hold them for every workload of
// BASELINE.json (P4: 19 GB, S8: 174 GB).  Values are bit-identical to the on-the-fly evaluation by construction.
// svr_table.inc owns it: nobody else writes a field.
struct CoeffTable {
  DevBuf<float4> d_coeff;
  DevBuf<uint32_t> d_coeff_id;
  DevBuf<uint32_t> d_coeff_order;   // the active pixels in the order of their places in the table (coeff_order)
  CoeffState coeff_state = COEFF_NONE;
  int coeff_mode = 1;          // option "coeff_table": 0 = evaluate on the fly, 1 = stream the table (falls back to 0 if it does not fit).  Round 6: ON by
                               // default for slice-to-volume runs (written by the first gather of the SR iterations, coeff_lazy: P4 +7 %, S8 +5 % with one
                               // table per four SR iterations INSIDE the timed region), off for the patch-based path (no gain there: DESIGN 5.1b)
  bool coeff_user = false;     // svr_set_option("coeff_table") was called: the "pvr" option leaves the mode alone
  int coeff_lazy = 1;          // option "coeff_lazy" (round 6): 1 = the table is written by the first gather of the SR iterations after a new slice geometry
                               // (fwd_cell_kernel<.., 3>: the evaluation that pass needs anyway) instead of by k_coeff_build; passes before it evaluate
  const uint32_t *coeff_list = nullptr;   // (alias) the active pixels in table order (d_coeff_order, or d_active), while coeff_ids_valid
  bool coeff_ids_valid = false;   // d_coeff_order / d_coeff_id match the current cell lists (dropped with them): a table thrown away without a new
                                  // geometry (svr_set_option coeff_invalidate) keeps its pixels' places
  void want(bool on);             // option "coeff_table"
  void want_by_default(bool on);  // ... what the "pvr" option makes of it, unless the caller chose
  void set_lazy(bool on);         // option "coeff_lazy"
  void drop();                    // holds nothing any more
  void drop_psf_pixels();         // the PSF pixels changed: a table that holds only them holds nothing any more
  void free_rows();               // the table's memory
  void free_ids();                // ... and the ids' (a new slice grid)
  void ids_stale();               // the cell lists that gave the pixels their places are gone
};
}  // namespace

struct svr_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::string err;
  bool disable_bias = true, debug_gpu = false;

  // volume
  uint32_t vx = 0, vy = 0, vz = 0;
  float vdim[3] = {1, 1, 1};
  size_t nv = 0;
  DevBuf<float> d_recon_volw;   // recon | volw
  DevBuf<float> d_addon_cmap;   // addon | cmap
  DevBuf<float> d_mask, d_snap, d_recon_new;
  float *recon_cur = nullptr;   // (alias) the volume: d_recon_volw or d_recon_new (the fused volume update writes the other one, svr_regul.inc)
  int reg_tile = -1;            // k_regul_fused's tile: -1 = by the volume's extent, 0 = 64 x 8, 1 = 32 x 16, 2 = 32 x 8
  int reg_mode = 1;             // volume update: 1 = k_regul_fused (one kernel, LDS planes, float32 weights), 0 = k_reg_prep + k_regularize (fp64 weights)
  bool prep_pending = false;    // reg_mode 1, non-adaptive: Prep's own changes of addon / cmap are applied when somebody reads the buffers
  bool cmap_from_scatter = false;   // cmap is what the scatter wrote (zero outside the mask): the update skips tiles outside the mask's box
  DevBuf<float2> d_volm;   // {V m, m}, refreshed before every SVR forward projection
  bool have_mask = false;
  // bounding box of mask != 0 (inclusive), from the host copy handed to svr_set_mask: the scatter only ever writes mask voxels,
  // so a sharded run need not all-reduce the rest of a volume pair (svr_pair_pack / svr_pair_unpack)
  int mbox_lo[3] = {0, 0, 0}, mbox_hi[3] = {-1, -1, -1};
  bool mbox_valid = false;
  DevBuf<float> d_pair_pack;

  // slice grid
  uint32_t sx = 0, sy = 0, ns = 0;
  size_t np = 0;
  DevBuf<float> d_slices, d_weights, d_simslices, d_simweights, d_psf_sums;
  DevBuf<unsigned char> d_siminside;
  DevBuf<int> d_voxcount;
  bool have_slices = false;
  bool have_sim = false;                // d_simslices / d_simweights hold a forward projection (svr_simulate_slices, or a test's svr_debug_set)
  bool sem_weights_current = false;     // d_slice_weights holds the device-side EM's weights (svr_slice_em_run) and nobody has written it since
  DevBuf<float> d_scales, d_slice_weights, d_scales_host_copy, d_tmp_ns;
  DevBuf<unsigned char> d_slice_inside;
  std::vector<float> h_slice_weights;             // RC.cu:1346.  h_scales (RC.cu:1345) lives on the device: d_scales_host_copy
  bool have_scales = false;
  // per-slice vectors go up through pinned slots without a stream synchronisation (upload_ns); what each device vector holds
  // is mirrored on the host, and a vector that is already there is not sent again (the SR loop sends the slice weights twice
  // and the previous scale vector once per iteration: RC.cu:2123, 3238)
  static constexpr int UP_SLOTS = 4;
  float *h_up = nullptr;                          // [UP_SLOTS][ns], pinned
  hipEvent_t up_ev[UP_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
  bool up_busy[UP_SLOTS] = {false, false, false, false};
  int up_next = 0;
  std::vector<float> mir_scales, mir_slice_weights, mir_scales_copy;
  // small results come down through one pinned arena: the copies are queued on the stream, ONE synchronisation, then they
  // are handed to the caller's memory (down_queue / down_flush)
  unsigned char *h_down = nullptr;
  size_t down_cap = 0, down_used = 0;
  struct DownItem { void *dst; size_t off, bytes; };
  std::vector<DownItem> down_items;
  DevBuf<float> d_em;                             // {sigma, mix, m} of the fused M-step + E-step (svr_mstep_estep)

  // geometry
  std::vector<float> slice_dims;   // ns*3
  std::vector<uint32_t> stack_sizes;   // updateStackSizes (RC.cuh:210)
  std::vector<float> mI2W, mW2I, mT, mTinv;
  float reconI2W[16], reconW2I[16];
  float psf_c0[3] = {0, 0, 0};
  float quality_factor = 1.0f;
  bool have_dims = false, have_mats = false, have_psf = false, sc_dirty = true;
  DevBuf<SliceConst> d_sc;

  // work lists
  DevBuf<uint32_t> d_active, d_psf_list, d_counter, d_tiles, d_tiles_fb;
  uint32_t n_active = 0, n_psf = 0, n_tiles = 0;
  int tiles_x = 0, tiles_y = 0, tile_w = 4, tile_h = 4;
  int reg_blind = 4;        // GPU slice-to-volume registration: line-search steps per host round trip, the active count on the device (0: a round trip per step)
  int reg_red_threads = 0;  // workgroup size of the registration's per-image reductions: 0 = by image size, 256, 1024
  int reg_batch = 1;        // GPU slice-to-volume registration: the twelve evaluations of a gradient as one launch sequence (0: one by one)
  int pvr_reg_levels = 3, pvr_reg_steps = 4, pvr_reg_iterations = 20;   // PatchBased2D3DRegistration_gpu2 schedule (tests shorten it)
  bool psf_list_valid = false;
  DevBuf<unsigned char> d_gauss_flag;      // pixels whose sume passed in the current Gaussian pass
  DevBuf<uint32_t> d_tiles_tmp;            // tile list of the Gaussian passes (grows: the tile shapes can change between calls)
  int gauss_mode = 1;                      // 1 = unit-based pass 1 (fwd_unit_kernel<GAUSS1>) + the LDS scatter, 0 = psf_kernel<MODE_GAUSS>
  DevBuf<uint32_t> d_tiles_fwd;      // tiles of fwd_tw x fwd_th pixels for fwd_unit_kernel
  uint32_t n_tiles_fwd = 0;
  bool tiles_back_valid = false, tiles_fwd_valid = false;   // the tile lists belong to the current PSF list (ensure_tiles_back / ensure_tiles_fwd)
  int fwd_tw = 4, fwd_th = 4, fwd_tiles_x = 0, fwd_tiles_y = 0;
  int fwd_unit_cap = 9300;  // box voxels (float2) of fwd_unit_kernel: 72.7 KiB + up to 6.6 KiB static = 64 LDS granules of 1280 B -> 2 workgroups of 8 waves per CU (9400 would push the GAUSS1 table instantiation to 65)
  int fwd_mode = 2;         // 2 = the gather over (cell, plane) items (fwd_cell_kernel, svr_cell.inc; SVR on the fly -- patch-based runs and the
                            // coefficient table take 1), >= 1 = unit-based gather per slice tile (fwd_unit_kernel), 0 = wave-per-pixel kernel (psf_kernel<MODE_FWD>)
  // The tile shapes follow from the geometry (tile_shape_rule for the unit gather, 6 x 4 for the tiled scatters: every run, every rank the
  // same) unless the caller named one: fwd_tile_w / fwd_tile_h, tile_w / tile_h, SVR_TILE_PIN.  The results do not depend on the gather's
  // shape (per-pixel sums in a fixed order); the tiled scatters' sums are float atomics in run-dependent order with any shape.
  bool fwd_tile_user = false, tile_user = false;
  int pvr = 0;              // 1: patch-to-volume constants and kernels (svr_set_option "pvr")
  int pvr_mode = 1;         // PVR kernels: 1 = the unit-based gather / wave-owned scatter with support 12, 0 = wave-per-pixel (pvr_kernel)
  DevBuf<unsigned char> d_spx;
  int back_mode = 5;        // 5 = cell-owned planes, staged and combined in a fixed order: no atomics (svr_cell.inc; the default for SVR on the fly --
                            // patch-based runs and the coefficient table take 4 unless the mode was set explicitly),
                            // 4 = wave-owned LDS planes (back_wave_kernel), 3 = the workgroup kernel for every tile (back_slot_kernel<8>),
                            // 1 = LDS tiles with ds_add_f32 (back_tiled_kernel), 0 = direct device-scope atomics per tap (psf_kernel<MODE_BACK>)
  int tile_cap = 0;         // voxels of LDS accumulator per workgroup
  int n_cu = 0;             // compute units of the device (the grids of the persistent cell kernels)
  uint32_t n_tiles_fb = 0;
  uint32_t n_tiles_fb8 = 0;   // tiles of the last scatter that the wave-owned kernel handed to the workgroup kernel (box larger than wave_cap)
  // PSF launches that were asked for on the cell path (back_mode 5 / fwd_mode 2: no atomics, bit-identical from run to run) and left it
  // because the cell lists cannot hold the geometry (svr_cell.inc cell_prepare: `usable`): [0] scatters (-> back_mode 4: float atomics,
  // run-dependent last bits), [1] gathers, [2] pass 1 of the Gaussian reconstruction (-> the tile kernels: same bits, slower);
  // [3] tiles of tiled scatters re-run by a workgroup kernel.  svr_fallbacks() reads them; the first of each kind says so on stderr.
  uint64_t fallbacks[4] = {0, 0, 0, 0};
  void note_fallback(int kind, const char *what) {
    if (!fallbacks[kind]++) fprintf(stderr, "svr: %s -- counted in svr_fallbacks()[%d]\n", what, kind);
  }
  DevBuf<uint32_t> d_tiles_fb2;
  bool wave_cap_user = false;
  bool back_mode_user = false;   // svr_set_option("back_mode") was called: no automatic choice between 5 and 4
  bool fwd_mode_user = false;    // likewise "fwd_mode"
  bool sr_no_wait = false;       // inside svr_superresolution: its two halves do not wait for the device
  CoeffTable table;            // the coefficient table (svr_table.inc)
  bool legacy_ok = false;      // option "legacy_kernels": back_mode 0 / 1 / 3 and fwd_mode 0 may be asked for (tests)
  int wave_groups = 1, wave_cap = 2096;      // back_wave_kernel: wavefronts per tile, box voxels of a wavefront's four planes (14 LDS granules of 1280 B with the static part: 9 wavefronts per CU)

  // reductions
  DevBuf<double> d_partial, d_per_slice, d_out;
  DevBuf<double> d_em_all;          // [world][8]: every rank's M-step sums (svr_mstep_partial / svr_mstep_estep_ranks)
  int chunks = 0;

  // bias correction (allocated only when bias correction is enabled)
  DevBuf<float> d_bias, d_wb, d_wr, d_buffer;                        // slice grid
  DevBuf<float> d_bias_vol, d_volume_weights, d_maskC, d_mbuf;       // volume
  float mask_sigma_bias = 12.0f;
  // option "bias_mode": 1 (default) = NormaliseBias scatters on the cell kernels, CorrectBias on the LDS kernel of svr_bias.inc, the NormaliseBias
  // tail on its LDS kernels from BIAS_LDS_TAIL_MIN voxels on (below, the stencils are as fast: P4 0.18 vs 0.20 ms); 2 = the same with the LDS
  // tail at every size; 0 = round 1's kernels (psf_kernel<MODE_BIAS> with float atomics, the stencils of svr_small.inc).  The Gaussians give
  // the same bits in every mode
  int bias_mode = 1;
  int bias_corrections = 0, bias_normalisations = 0;   // CorrectBias / NormaliseBias (finish) calls that ran (svr_get_option)
  int bias_scatters = 0, bias_scatters_on_cells = 0;   // NormaliseBias scatters, and those of them that ran on the cell kernels
  // what the last launches chose (read-only options, so a test can tell which branch it reached; -1 = not launched yet):
  // CorrectBias's strip width (0 = the stencils), the NormaliseBias tail on the LDS kernels (0/1) with its x rows and y / z strip
  // widths (0 when the stencils ran), the fused volume update's planes per z-chunk and chunks
  int last_bias_bx = -1, last_tail_lds = -1, last_tail_rows = -1, last_tail_bxy = -1, last_tail_bxz = -1;
  int last_reg_zc = -1, last_reg_chunks = -1;
  bool maskC_valid = false;

  // registration cost (NCC)
  DevBuf<short> d_reg_targets, d_reg_source;
  DevBuf<short> d_pyr_full[2], d_pyr_a, d_pyr_b;   // device pyramid of the registration (svr_pyr_*)
  size_t pyr_count[2] = {0, 0};                    // the elements the last svr_pyr_upload put into each slot (a kept block may be larger and hold an older upload's tail)
  DevBuf<unsigned char> d_pyr_meta;
  DevBuf<unsigned char> d_sim_io;        // grow-only arena of svr_ncc / svr_nmi / svr_lncc_evaluate (sim_evaluate, svr_sim.inc): inputs | outputs | test map
  std::vector<unsigned char> sim_staging;
  DevBuf<double> d_nmi_terms;            // c log c for c = 0 .. nmi_terms_n - 1, from the host's libm
  size_t nmi_terms_n = 0;
  DevBuf<unsigned> d_nmi_merge;          // merge slots of split evaluations + their counters, all zero between calls
  size_t nmi_slots = 0;
  DevBuf<float> d_vote_best, d_vote_label;                    // svr_channel_vote: the running maximum and its label, [nv] each, from the first vote to svr_channel_vote_fetch
  // svr_channel_sr_begin .. _end (svr_channel.inc): the channel and its switches, the two channel volumes of the regulariser's flip, the channel's own
  // forward projection {simulated, sim-weight, inside flags} and the cover mask.  All of it belongs to the call: channel_sr_drop frees it
  DevBuf<float> d_csr_channel, d_csr_vol[2], d_csr_sim, d_csr_simw;
  DevBuf<unsigned char> d_csr_unit_on, d_csr_cover, d_csr_inside, d_csr_slice_inside;
  int csr_stage = 0;                     // 0 = no call in flight, 1 = begun (the seed scatter is in addon | cmap), 2 = a volume to project, 3 = back-projected
  int csr_cur = 0;                       // which of d_csr_vol is the channel volume
  bool csr_has_unit_on = false;
  DevBuf<float> d_csr_guide;             // svr_channel_sr_guide's volume, a copy of the call's own: set = every update of this begin..end is guided
  float csr_delta_g = 0.0f;
  bool csr_guide_only = false;
  bool have_em = false;                  // d_weights hold EM posteriors (svr_initialize_em_values or a later E-step; a test's svr_debug_set)
  int fit_chunk = 1 << 20;               // voxels per upload / launch / download of svr_monoexp_fit (svr_fit.inc; option "fit_chunk")
  int last_quality_chunks = -1;          // chunks per slice of the last svr_slice_quality (read-only option "quality_chunks"; -1 = not launched yet)
  int reg_tx = 0, reg_ty = 0, reg_n = 0;
  uint32_t reg_vx = 0, reg_vy = 0, reg_vz = 0;

  // GPU slice-to-volume registration (svr_reg.inc)
  RegState *reg = nullptr;

  // the scatter without atomics (back_mode 5, svr_cell.inc): cell size in voxels (x, lane axis), wavefronts per item
  SliceEm *sem = nullptr;         // the slice-level EM on the device (svr_em.inc)
  SlabPlan *slab = nullptr;       // sharded runs: the index lists and slab boundaries of reduce-scatter -> slab update -> all-gather (svr_slab.inc)
  bool vol_clean[2] = {false, false};   // d_recon_volw / d_recon_new known to be zero outside the dilated mask (svr_slab.inc)
  CellState *cell = nullptr;      // the scatter's cell lists
  CellState *cell_g = nullptr;    // the gather's, when it works on another cell size (cell_prepare_gather)
  DevBuf<int> d_cellc;            // centre voxel + class of every active pixel (k_cell_centres), shared by the two
  uint32_t cellc_n = 0;
  bool cellc_valid = false;
  int cellc_range[16] = {0};
  int cell_w = 0, cell_h = 0, cell_gw = 0, cell_gh = 0;   // 0: by the pixel density (cell_auto_size); cell_gw / cell_gh: the gather's own
  int cell_order = 1;       // > 0: items in order of falling work, in classes of 2^(cell_order - 1) pixels (0: (cell, plane) order)
  int cell_combine = 2;     // 2: one item_of load per wavefront and class, early out where nothing is staged (k_cell_combine_wave); 1: a voxel's slabs in two batches (k_cell_combine_fast); 0: the general form.  Same bits
  int cell_balance = 0;     // an item heavier than the launch's work / (1024 x cell_balance) is cut into parts (0: never)
  int cell_split = 1, cell_qx = 1, cell_band = 3;   // cell_qx: cells of a quad along x (1, 2 or 4; the other factor along the lane axis)

  // timers
  bool timers = false;
  // kernel timers: event pairs are recorded on the stream and read back later (svr_timer_get / reset / every TIMER_BATCH
  // pairs) -- timing a pass does not synchronise the stream
  struct TimedSpan { int which; hipEvent_t a, b; };
  std::vector<hipEvent_t> ev_free;
  std::vector<TimedSpan> ev_pending;
  hipEvent_t ev_open = nullptr;                   // svr_timer_begin .. svr_timer_end
  double t_ms[SVR_T_COUNT] = {0};
  long t_n[SVR_T_COUNT] = {0};

  float *recon() { return recon_cur; }
  float *volw() { return d_recon_volw + nv; }
  float *addon() { return d_addon_cmap; }
  float *cmap() { return d_addon_cmap + nv; }
};

namespace {

int fail(svr_ctx *c, int code, const std::string &msg) {
  if (c) c->err = msg;
  return code;
}
// Every public entry point selects the context's device first: the command lines run one host thread per device and start
// fresh threads per phase (a new thread's current device is 0), so hipMalloc / hipMemGetInfo / event calls inside an entry
// point would otherwise land on GPU 0 until the first call that happened to set the device.
#define SVR_ENTER(c)                                                                        \
  do {                                                                                      \
    if (c) (void)hipSetDevice((c)->device);                                                 \
  } while (0)
#define HIPCHK(expr)                                                                        \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return fail(ctx, (int)e_, std::string(#expr) + ": " + hipGetErrorString(e_));       \
  } while (0)
#define KCHK(name)                                                                          \
  do {                                                                                      \
    hipError_t e_ = hipGetLastError();                                                      \
    if (e_ != hipSuccess)                                                                   \
      return fail(ctx, (int)e_, std::string(name) + ": " + hipGetErrorString(e_));        \
  } while (0)
#define NEED(cond, what)                                                                    \
  do {                                                                                      \
    if (!(cond)) return fail(ctx, SVR_E_STATE, std::string(__func__) + ": " + what);      \
  } while (0)

void reg_free(RegState *r);
void cell_free(CellState *c);

// The changes of a context's inputs: invalidate (after the cell and slab includes) is the one place that drops cached state.  A new writer
// of an input raises the change it causes, a new cache adds its line there; whoever builds a cache marks it valid.  Buffers that
// live for one call are locals of their entry point; the vote arrays of svr_channel_vote live from the first vote to the fetch and have a line,
// and so do the buffers of a channel's SR iterations (svr_channel_sr_begin .. _end): dropped with either grid, never reused.
enum Change : unsigned {
  CH_SLICE_GEOMETRY = 1u << 0,    // slice dims / matrices: the slice constants, rebuilt by the next pass (prepare_slice_consts then raises CH_TAPS)
  CH_TAPS = 1u << 1,              // new slice constants, generatePSFVolume: the table and the cell lists
  CH_SLICE_PIXELS = 1u << 2,      // d_slices: the PSF list, the table and the cell lists (they cover the pixels with s != -1)
  CH_PSF_SUMS = 1u << 3,          // v_PSF_sums: the PSF list, the gather's 1 / v_PSF_sums, a table that holds the PSF pixels of an earlier pass
  CH_VOLUME_GRID = 1u << 4,       // a new volume: the table, the cell lists and what is known about the volume buffers
  CH_MASK = 1u << 5,              // the mask: clean buffers, the slab plan, the mask box
  CH_MASK_BLUR = 1u << 6,         // the inputs of the blurred mask maskC (svr_set_mask: the mask and sigma)
  CH_VOLUME_VALUES = 1u << 7,     // the current volume was written whole: no longer known to be clean
  CH_SCATTER_TARGETS = 1u << 8,   // addon | cmap hold something other than the scatter's result
  CH_CELL_SHAPE = 1u << 9,        // the cell options: the cell lists
  CH_TILE_SHAPE = 1u << 10,       // a tile shape: the PSF list, and with it the tile lists
  CH_TABLE = 1u << 11,            // the table thrown away (option coeff_invalidate: what a new slice geometry does to it)
  CH_TABLE_OFF = 1u << 12,        // the table's memory freed: the table and the cell lists
  CH_TABLE_IDS = 1u << 13,        // the pixels got new places in the table: the records' table ids
};
void invalidate(svr_ctx *ctx, unsigned changes);

constexpr size_t TIMER_BATCH = 256;
inline hipEvent_t timer_event(svr_ctx *c) {
  if (!c->ev_free.empty()) { hipEvent_t e = c->ev_free.back(); c->ev_free.pop_back(); return e; }
  hipEvent_t e = nullptr;
  // timing only: nobody reads device memory on the strength of these events, so they need not write the caches back to system scope when
  // they are recorded (hipEventDisableSystemFence: "for events that are only being used to measure timing") -- the default's fence is
  // what made every recorded event a 5.8 us hole in the stream (profiles/r05_step_timeline_p4.txt)
  if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) { e = nullptr; (void)hipEventCreate(&e); }
  return e;
}
// the recorded pairs -> t_ms / t_n (waits for the last one)
inline void timers_resolve(svr_ctx *c) {
  for (const auto &sp : c->ev_pending) {
    float ms = 0;
    if (sp.a && sp.b && hipEventSynchronize(sp.b) == hipSuccess && hipEventElapsedTime(&ms, sp.a, sp.b) == hipSuccess) {
      const int w = sp.which & 255, also = (sp.which >> 8) - 1;      // (ScopedTimer::also: the same pair counted under a second name)
      c->t_ms[w] += ms;
      c->t_n[w] += 1;
      if (also >= 0 && also < SVR_T_COUNT) { c->t_ms[also] += ms; c->t_n[also] += 1; }
    }
    if (sp.a) c->ev_free.push_back(sp.a);
    if (sp.b) c->ev_free.push_back(sp.b);
  }
  c->ev_pending.clear();
}
inline void timer_close(svr_ctx *c, int which, hipEvent_t a) {
  hipEvent_t b = timer_event(c);
  if (b) (void)hipEventRecord(b, c->stream);
  c->ev_pending.push_back({which, a, b});
  if (c->ev_pending.size() >= TIMER_BATCH) timers_resolve(c);
}
struct ScopedTimer {
  svr_ctx *c;
  int which;
  hipEvent_t a = nullptr;
  ScopedTimer(svr_ctx *c_, int w) : c(c_), which(w) {
    if (c->timers) {
      a = timer_event(c);
      if (a) (void)hipEventRecord(a, c->stream);
    }
  }
  void also(int w2) { which = (which & 255) | ((w2 + 1) << 8); }   // the same interval under a second name (what kind of pass it was)
  void stop() {
    if (a) timer_close(c, which, a);
    a = nullptr;
  }
  ~ScopedTimer() {                                  // an error path left before stop(): the event goes back unused
    if (a) c->ev_free.push_back(a);
  }
};

inline unsigned nblk(size_t n, unsigned b = 256) { return (unsigned)((n + b - 1) / b); }

void free_volume(svr_ctx *c) {
  c->recon_cur = nullptr;
  c->d_recon_volw.reset();
  c->d_addon_cmap.reset();
  c->d_snap.reset();
  c->d_recon_new.reset();
  c->d_volm.reset();
}
void free_slices(svr_ctx *c) {
  c->d_slices.reset(); c->d_weights.reset(); c->d_simslices.reset(); c->d_simweights.reset();
  c->d_psf_sums.reset(); c->d_siminside.reset(); c->d_voxcount.reset(); c->d_scales.reset();
  c->d_slice_weights.reset(); c->d_scales_host_copy.reset(); c->d_tmp_ns.reset();
  c->mir_scales.clear(); c->mir_slice_weights.clear(); c->mir_scales_copy.clear();
  if (c->h_up) { (void)hipStreamSynchronize(c->stream); (void)hipHostFree(c->h_up); c->h_up = nullptr; }
  if (c->h_down) { (void)hipStreamSynchronize(c->stream); (void)hipHostFree(c->h_down); c->h_down = nullptr; c->down_cap = c->down_used = 0; c->down_items.clear(); }
  c->d_em.reset();
  for (int k = 0; k < svr_ctx::UP_SLOTS; ++k) {
    if (c->up_ev[k]) { (void)hipEventDestroy(c->up_ev[k]); c->up_ev[k] = nullptr; }
    c->up_busy[k] = false;
  }
  c->d_slice_inside.reset(); c->d_sc.reset(); c->d_active.reset(); c->d_psf_list.reset();
  c->d_tiles.reset();
  c->d_tiles_fwd.reset();
  c->d_gauss_flag.reset();
  c->d_tiles_tmp.reset();
  c->d_tiles_fb.reset();
  c->d_tiles_fb2.reset();
  c->d_partial.reset(); c->d_per_slice.reset();
}

// builds the per-slice constants (host float math, literal order) and uploads them
int prepare_slice_consts(svr_ctx *ctx) {
  NEED(ctx->have_dims && ctx->have_mats && ctx->have_slices, "slice dims / matrices / storage not set");
  if (!ctx->sc_dirty) return SVR_OK;
  std::vector<SliceConst> h(ctx->ns);
  for (uint32_t s = 0; s < ctx->ns; ++s) {
    SliceConst &S = h[s];
    memset(&S, 0, sizeof(S));
    memcpy(S.I2W, &ctx->mI2W[16 * s], 12 * sizeof(float));
    memcpy(S.T, &ctx->mT[16 * s], 12 * sizeof(float));
    float tmp[16], A[16];
    matmul4(&ctx->mW2I[16 * s], &ctx->mTinv[16 * s], tmp);   // RC.cu:223 (left to right)
    matmul4(tmp, ctx->reconI2W, A);
    memcpy(S.A, A, 12 * sizeof(float));
    for (int k = 0; k < 3; ++k) S.dim[k] = ctx->slice_dims[3 * s + k];
    S.kx = S.dim[0] / 2.3548f;
    S.ky = S.dim[1] / 2.3548f;
    // SVR: sigma_z = dz / 2.3548 (RC.cu:114); PVR: sigma_z = dz and the offset is divided by 2.5
    // (pointSpreadFunction.cuh:76,112)
    float sigmaz = ctx->pvr ? S.dim[2] : S.dim[2] / 2.3548f;
    S.inv2s2 = 1.0f / (2.0f * sigmaz * sigmaz);
    for (int j = 0; j < 3; ++j) {
      S.Lp[0 * 3 + j] = (A[0 * 4 + j] * S.dim[0]) * S.kx;
      S.Lp[1 * 3 + j] = (A[1 * 4 + j] * S.dim[1]) * S.ky;
      S.Lp[2 * 3 + j] = ctx->pvr ? (A[2 * 4 + j] * S.dim[2]) / 2.5f : A[2 * 4 + j] * S.dim[2];
    }
    // Gaussian recurrence (gauss_pairs): the ratio of ratios, or -1 where the first ratio exp(+-2 z' dz' c - dd c)
    // of a row that passes the central test (a <= GAUSS_AMAX) could leave the float range
    S.dd = S.Lp[6] * S.Lp[6];
    const double tmax = 2.0 * sqrt((double)GAUSS_AMAX * (double)S.inv2s2) * fabs((double)S.Lp[6]) + (double)S.dd * (double)S.inv2s2;
    S.w = tmax <= 80.0 ? canon_exp_neg((2.0f * S.dd) * S.inv2s2) : -1.0f;
    S.own = fabsf(S.Lp[7]) > fabsf(S.Lp[8]) ? 1 : 2;
    {
      const int G = S.own == 1 ? 2 : 1;                    // the lane axis
      const float D = S.Lp[0] * S.Lp[3 + G] - S.Lp[G] * S.Lp[3];
      S.invD = fabsf(D) > 1e-4f ? 1.0f / D : 0.0f;
    }
  }
  HIPCHK(hipMemcpyAsync(ctx->d_sc, h.data(), h.size() * sizeof(SliceConst), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->sc_dirty = false;
  invalidate(ctx, CH_TAPS);
  return SVR_OK;
}

// A dispatch holds at most 2^32 - 1 work-items per dimension (launch_fwd_unit below tells how that was found): every kernel
// that takes one workgroup per entry of a tile list sends long lists out in pieces.  f(offset, count) launches one piece.
template <class F>
int in_pieces(uint32_t n, uint32_t threads_per_tile, F &&f) {
  const long env = getenv("SVR_LIST_PIECE") ? atol(getenv("SVR_LIST_PIECE")) : 0;     // test hook: short pieces on a small problem
  uint32_t piece = (uint32_t)((((1ull << 32) - 1) / threads_per_tile) & ~1023ull);
  if (env > 0) piece = (uint32_t)std::min<long>(env, piece);
  for (uint32_t off = 0; off < n; off += piece) {
    const int r = f(off, std::min(piece, n - off));
    if (r) return r;
  }
  return SVR_OK;
}
// one wavefront per entry of a pixel list (psf_kernel, pvr_kernel, k_coeff_build): launch(args of one piece, offset of the piece)
template <class L>
int pixel_list_in_pieces(const PsfArgs &a0, L &&launch) {
  return in_pieces(a0.n, 64, [&](uint32_t off, uint32_t cnt) {
    PsfArgs a = a0;
    a.list = a0.list + off;
    a.n = cnt;
    return launch(a, off);
  });
}
// tiles of tw x th pixels that hold at least one active pixel (k_build_tiles: a wavefront per candidate tile)
int build_tile_list(svr_ctx *ctx, const float *psf_sums, const unsigned char *flag, int tiles_x, int tiles_y, int tw, int th, uint32_t *tiles,
                    uint32_t *counter) {
  const uint64_t total64 = (uint64_t)tiles_x * tiles_y * ctx->ns;
  if (total64 >= (1ull << 32)) return fail(ctx, SVR_E_ARG, "more than 2^32 candidate tiles");
  return in_pieces((uint32_t)total64, 64, [&](uint32_t off, uint32_t cnt) {
    hipLaunchKernelGGL(k_build_tiles, dim3(nblk(cnt, 16)), dim3(1024), 0, ctx->stream, ctx->d_slices, psf_sums, flag, (int)ctx->sx, (int)ctx->sy,
                       (int)ctx->ns, tiles_x, tiles_y, tw, th, tiles, counter, (const unsigned char *)nullptr, 0, off, off + cnt);
    KCHK("k_build_tiles");
    return (int)SVR_OK;
  });
}

int build_list(svr_ctx *ctx, bool with_psf) {
  HIPCHK(hipMemsetAsync(ctx->d_counter, 0, sizeof(uint32_t), ctx->stream));
  uint32_t *list = with_psf ? ctx->d_psf_list : ctx->d_active;
  hipLaunchKernelGGL(k_compact, dim3(std::min(nblk(ctx->np, 1024), 4096u)), dim3(1024), 0, ctx->stream, ctx->d_slices,
                     with_psf ? ctx->d_psf_sums : (const float *)nullptr, (uint32_t)ctx->np, list, ctx->d_counter);
  KCHK("k_compact");
  uint32_t n = 0;
  HIPCHK(hipMemcpyAsync(&n, ctx->d_counter, sizeof(n), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (with_psf) {
    ctx->n_psf = n;
    ctx->psf_list_valid = true;
    // the tile lists of the tile kernels (the table's gather, the fallback modes) are built when one of them asks (round 4: the default
    // path works on (cell, plane) items and used to pay for both lists, two more waits and an allocation per slice geometry)
    ctx->tiles_back_valid = ctx->tiles_fwd_valid = false;
  } else {
    ctx->n_active = n;
  }
  return SVR_OK;
}
int ensure_psf_list(svr_ctx *ctx);
// tiles of tile_w x tile_h pixels that hold at least one pixel of the PSF list (the tiled scatters)
int ensure_tiles_back(svr_ctx *ctx) {
  int r = ensure_psf_list(ctx);
  if (r || ctx->tiles_back_valid) return r;
  uint32_t n = 0;
  HIPCHK(hipMemsetAsync(ctx->d_counter, 0, sizeof(uint32_t), ctx->stream));
  if ((r = build_tile_list(ctx, ctx->d_psf_sums, nullptr, ctx->tiles_x, ctx->tiles_y, ctx->tile_w, ctx->tile_h, ctx->d_tiles, ctx->d_counter))) return r;
  HIPCHK(hipMemcpyAsync(&n, ctx->d_counter, sizeof(n), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->n_tiles = n;
  ctx->tiles_back_valid = true;
  return SVR_OK;
}
// ... of fwd_tw x fwd_th pixels (fwd_unit_kernel)
int ensure_tiles_fwd(svr_ctx *ctx) {
  int r = ensure_psf_list(ctx);
  if (r || ctx->tiles_fwd_valid) return r;
  uint32_t n = 0;
  ctx->d_tiles_fwd.reset();
  ctx->fwd_tiles_x = (int)((ctx->sx + ctx->fwd_tw - 1) / ctx->fwd_tw);
  ctx->fwd_tiles_y = (int)((ctx->sy + ctx->fwd_th - 1) / ctx->fwd_th);
  const uint32_t total_f = (uint32_t)ctx->fwd_tiles_x * ctx->fwd_tiles_y * ctx->ns;
  HIPCHK(ctx->d_tiles_fwd.reserve((size_t)total_f));
  HIPCHK(hipMemsetAsync(ctx->d_counter, 0, sizeof(uint32_t), ctx->stream));
  if ((r = build_tile_list(ctx, ctx->d_psf_sums, nullptr, ctx->fwd_tiles_x, ctx->fwd_tiles_y, ctx->fwd_tw, ctx->fwd_th, ctx->d_tiles_fwd, ctx->d_counter))) return r;
  HIPCHK(hipMemcpyAsync(&n, ctx->d_counter, sizeof(n), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->n_tiles_fwd = n;
  ctx->tiles_fwd_valid = true;
  return SVR_OK;
}

PsfArgs make_args(svr_ctx *ctx) {
  PsfArgs a;
  memset(&a, 0, sizeof(a));
  a.sc = ctx->d_sc;
  a.vg.vx = (int)ctx->vx; a.vg.vy = (int)ctx->vy; a.vg.vz = (int)ctx->vz;
  memcpy(a.vg.W2I, ctx->reconW2I, 12 * sizeof(float));
  memcpy(a.vg.c0, ctx->psf_c0, 3 * sizeof(float));
  a.vg.pvr = ctx->pvr;
  a.spx = ctx->d_spx;
  a.sx = (int)ctx->sx; a.sy = (int)ctx->sy;
  a.slices = ctx->d_slices; a.mask = ctx->d_mask; a.psf_sums = ctx->d_psf_sums;
  a.scales = ctx->d_scales;
  a.bias = ctx->disable_bias ? nullptr : ctx->d_bias;
  a.recon = ctx->recon(); a.volw = ctx->volw(); a.voxcount = ctx->d_voxcount;
  a.vol = ctx->recon(); a.simslices = ctx->d_simslices; a.simweights = ctx->d_simweights;
  a.siminside = ctx->d_siminside;
  a.slice_inside = ctx->d_slice_inside;
  a.weights = ctx->d_weights; a.slice_weights = ctx->d_slice_weights;
  a.addon = ctx->addon(); a.cmap = ctx->cmap();
  return a;
}

// bias-path buffers: slice-grid {bias, wb, wresidual, buffer} (RC.cu:1510-1539) and volume
// {bias, volume_weights, maskC} (RC.cu:1203-1214, 1129-1157); created on first use after
// svr_set_flags(ctx, disable_bias_correction = 0, ...)
int ensure_bias_buffers(svr_ctx *ctx) {
  if (ctx->disable_bias) return SVR_OK;
  if (ctx->np && !ctx->d_bias) {
    const size_t fb = ctx->np * sizeof(float);
    HIPCHK(ctx->d_bias.reserve(ctx->np)); HIPCHK(ctx->d_wb.reserve(ctx->np));
    HIPCHK(ctx->d_wr.reserve(ctx->np)); HIPCHK(ctx->d_buffer.reserve(ctx->np));
    HIPCHK(hipMemsetAsync(ctx->d_bias, 0, fb, ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->d_wb, 0, fb, ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->d_wr, 0, fb, ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->d_buffer, 0, fb, ctx->stream));
  }
  if (ctx->nv && !ctx->d_bias_vol) {
    const size_t vb = ctx->nv * sizeof(float);
    HIPCHK(ctx->d_bias_vol.reserve(ctx->nv)); HIPCHK(ctx->d_volume_weights.reserve(ctx->nv));
    HIPCHK(ctx->d_maskC.reserve(ctx->nv)); HIPCHK(ctx->d_mbuf.reserve(ctx->nv));
    HIPCHK(hipMemsetAsync(ctx->d_bias_vol, 0, vb, ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->d_volume_weights, 0, vb, ctx->stream));
  }
  if (ctx->nv && ctx->have_mask && !ctx->maskC_valid) {
    // maskC_ = mask blurred with sigma_bias: x into a zeroed buffer, y back, z into the buffer, copy (RC.cu:1129-1157)
    const size_t vb = ctx->nv * sizeof(float);
    const dim3 grid((ctx->vx + 63) / 64, (ctx->vy + 3) / 4, ctx->vz);
    HIPCHK(hipMemcpyAsync(ctx->d_maskC, ctx->d_mask, vb, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->d_mbuf, 0, vb, ctx->stream));
    hipLaunchKernelGGL(k_gauss_conv3d, grid, dim3(256), 0, ctx->stream, ctx->d_maskC, ctx->d_mbuf, ctx->mask_sigma_bias, 0,
                       ctx->vdim[0], (int)ctx->vx, (int)ctx->vy, (int)ctx->vz);
    hipLaunchKernelGGL(k_gauss_conv3d, grid, dim3(256), 0, ctx->stream, ctx->d_mbuf, ctx->d_maskC, ctx->mask_sigma_bias, 1,
                       ctx->vdim[1], (int)ctx->vx, (int)ctx->vy, (int)ctx->vz);
    hipLaunchKernelGGL(k_gauss_conv3d, grid, dim3(256), 0, ctx->stream, ctx->d_maskC, ctx->d_mbuf, ctx->mask_sigma_bias, 2,
                       ctx->vdim[2], (int)ctx->vx, (int)ctx->vy, (int)ctx->vz);
    KCHK("k_gauss_conv3d(mask)");
    HIPCHK(hipMemcpyAsync(ctx->d_maskC, ctx->d_mbuf, vb, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->maskC_valid = true;
  }
  return SVR_OK;
}

int ready(svr_ctx *ctx) {
  NEED(ctx->nv > 0, "reconstruction volume not initialised");
  NEED(ctx->have_mask, "mask not set");
  NEED(ctx->have_slices, "slices not filled");
  NEED(ctx->have_scales, "scale vector not set");
  NEED(ctx->have_psf, "generatePSFVolume not called");
  int r = ensure_bias_buffers(ctx);
  if (r) return r;
  return prepare_slice_consts(ctx);
}

// The gather takes one workgroup of FWDU_WAVES wavefronts per tile, and a dispatch holds at most 2^32 - 1 work-items per
// dimension: beyond 8.4 M tiles (2 x 2-pixel tiles of a 0.5 mm patch-based case: 12.2 M) a single launch silently ran the
// tile count modulo 2^23 -- it looked 3.3 x faster in the tuner and left two thirds of the simulated slices stale.  Long
// lists go out in pieces of 2^22 tiles (a multiple of the XCD group of xcd_run_index).
template <bool GAUSS1>
void launch_fwd_unit(svr_ctx *ctx, const PsfArgs &a, TileArgs ta, size_t lds) {
  constexpr uint32_t PIECE_MAX = 1u << 22;
  static_assert((uint64_t)PIECE_MAX * FWDU_WAVES * 64 < (1ull << 32), "a piece must fit one dispatch");
  const char *env = getenv("SVR_FWD_PIECE");             // test hook: short pieces on a small problem
  const uint32_t PIECE = env && atol(env) > 0 ? (uint32_t)std::min<long>(atol(env), PIECE_MAX) : PIECE_MAX;
  const uint32_t *tiles = ta.tiles;
  const uint32_t total = ta.ntiles;
  for (uint32_t off = 0; off < total; off += PIECE) {
    ta.tiles = tiles + off;
    ta.ntiles = std::min(PIECE, total - off);
    const dim3 grid(ta.ntiles), block(FWDU_WAVES * 64);
    if (ctx->pvr && a.coeff) hipLaunchKernelGGL((fwd_unit_kernel<GAUSS1, PVR_N, true, true>), grid, block, lds, ctx->stream, a, ta);
    else if (ctx->pvr) hipLaunchKernelGGL((fwd_unit_kernel<GAUSS1, PVR_N, true>), grid, block, lds, ctx->stream, a, ta);
    else if (a.coeff) hipLaunchKernelGGL((fwd_unit_kernel<GAUSS1, PSF_SUPPORT, false, true>), grid, block, lds, ctx->stream, a, ta);
    else hipLaunchKernelGGL((fwd_unit_kernel<GAUSS1>), grid, block, lds, ctx->stream, a, ta);
  }
}

int ensure_psf_list(svr_ctx *ctx) {
  if (!ctx->psf_list_valid) return build_list(ctx, true);
  return SVR_OK;
}

// The scatter over a tile list (back-projection into addon|cmap, or pass 2 of the Gaussian reconstruction into
// recon|volw): the wave-owned kernel with a box of `wave_cap` voxels; tiles whose planes do not fit it are re-run by the
// workgroup kernel (8 wavefronts, the largest box the CU can hold); what fits neither -- strongly oblique tiles of very fine
// volumes -- takes LDS atomics (SVR: back_tiled_kernel) or device atomics per tap (PVR: pvr_tiles_kernel).
// level: 4 = start with the wave-owned kernel, 3 = with the workgroup kernel, 1 = the last resort for every tile.
int launch_slot(svr_ctx *ctx, bool pvr, const PsfArgs &a, const TileArgs &ta_, uint32_t *fb, uint32_t *cnt) {
  const size_t lds = (size_t)ta_.cap * 2 * sizeof(float);
  return in_pieces(ta_.ntiles, 8 * 64, [&](uint32_t off, uint32_t cntp) {
    TileArgs ta = ta_;
    ta.tiles = ta_.tiles + off; ta.ntiles = cntp;
    if (pvr) hipLaunchKernelGGL((back_slot_kernel<8, PVR_N, true>), dim3(ta.ntiles), dim3(8 * 64), lds, ctx->stream, a, ta, fb, cnt);
    else hipLaunchKernelGGL(back_slot_kernel<8>, dim3(ta.ntiles), dim3(8 * 64), lds, ctx->stream, a, ta, fb, cnt);
    KCHK("back_slot_kernel");
    return (int)SVR_OK;
  });
}
int launch_scatter(svr_ctx *ctx, int level, const PsfArgs &a_, const uint32_t *tiles, uint32_t n, int mode_last) {
  PsfArgs a = a_;
  TileArgs ta;
  ta.tiles_x = ctx->tiles_x; ta.tiles_y = ctx->tiles_y; ta.tw = ctx->tile_w; ta.th = ctx->tile_h; ta.gauss = mode_last == MODE_GAUSS2;
  const bool pvr = ctx->pvr != 0;
  uint32_t *cnt = ctx->d_counter;                         // [0]: did not fit the wavefront's box, [1]: did not fit the workgroup's
  HIPCHK(hipMemsetAsync(cnt, 0, 2 * sizeof(uint32_t), ctx->stream));
  ctx->n_tiles_fb8 = ctx->n_tiles_fb = 0;
  if (!n) return SVR_OK;
  int r;
  uint32_t nfb[2] = {0, 0};
  const uint32_t *cur = tiles;
  uint32_t ncur = n;
  if (level >= 4) {
    ta.tiles = cur; ta.ntiles = ncur; ta.cap = std::min(ctx->wave_cap, ctx->tile_cap);
    const size_t lds = (size_t)ta.cap * 2 * sizeof(float);
    {
      const TileArgs ta1 = ta;
      r = in_pieces(ncur, 64u * (uint32_t)ctx->wave_groups, [&](uint32_t off, uint32_t cntp) {
        TileArgs tp = ta1;
        tp.tiles = ta1.tiles + off; tp.ntiles = cntp;
        const dim3 grid(cntp * (uint32_t)ctx->wave_groups);
        if (pvr && a.coeff) hipLaunchKernelGGL((back_wave_kernel<PVR_N, true, true>), grid, dim3(64), lds, ctx->stream, a, tp, ctx->wave_groups, ctx->d_tiles_fb, cnt);
        else if (pvr) hipLaunchKernelGGL((back_wave_kernel<PVR_N, true>), grid, dim3(64), lds, ctx->stream, a, tp, ctx->wave_groups, ctx->d_tiles_fb, cnt);
        else if (a.coeff) hipLaunchKernelGGL((back_wave_kernel<PSF_SUPPORT, false, true>), grid, dim3(64), lds, ctx->stream, a, tp, ctx->wave_groups, ctx->d_tiles_fb, cnt);
        else hipLaunchKernelGGL(back_wave_kernel<>, grid, dim3(64), lds, ctx->stream, a, tp, ctx->wave_groups, ctx->d_tiles_fb, cnt);
        return (int)SVR_OK;
      });
      if (r) return r;
    }
    KCHK("back_wave_kernel");
    HIPCHK(hipMemcpyAsync(nfb, cnt, sizeof(nfb), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    cur = ctx->d_tiles_fb; ncur = nfb[0];
    if (ncur && a.coeff && ta.cap < 3696) {
      // table mode: the tiles whose planes did not fit go through the same kernel once more with the largest box worth
      // having (4 planes of 30 x 30 voxels: 5 wavefronts per CU) before the evaluating workgroup kernel gets them
      HIPCHK(hipMemsetAsync(cnt, 0, sizeof(uint32_t), ctx->stream));
      ta.tiles = cur; ta.ntiles = ncur; ta.cap = std::min(3696, ctx->tile_cap);
      if (pvr) hipLaunchKernelGGL((back_wave_kernel<PVR_N, true, true>), dim3(ncur * (uint32_t)ctx->wave_groups), dim3(64), (size_t)ta.cap * 2 * sizeof(float),
                                  ctx->stream, a, ta, ctx->wave_groups, ctx->d_tiles_fb2, cnt);
      else hipLaunchKernelGGL((back_wave_kernel<PSF_SUPPORT, false, true>), dim3(ncur * (uint32_t)ctx->wave_groups), dim3(64), (size_t)ta.cap * 2 * sizeof(float),
                              ctx->stream, a, ta, ctx->wave_groups, ctx->d_tiles_fb2, cnt);
      KCHK("back_wave_kernel (large box)");
      HIPCHK(hipMemcpyAsync(nfb, cnt, sizeof(nfb), hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));
      cur = ctx->d_tiles_fb2; ncur = nfb[0];
      if (ncur) {                                          // the workgroup kernel writes its own rejects to d_tiles_fb2: move the list
        HIPCHK(hipMemcpyAsync(ctx->d_tiles_fb, ctx->d_tiles_fb2, (size_t)ncur * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
        cur = ctx->d_tiles_fb;
      }
    }
    ctx->n_tiles_fb8 = ncur;
    ctx->fallbacks[3] += ncur;
  }
  if (ncur && level >= 3) {
    ta.tiles = cur; ta.ntiles = ncur; ta.cap = ctx->tile_cap;
    if ((r = launch_slot(ctx, pvr, a, ta, ctx->d_tiles_fb2, cnt + 1))) return r;
    HIPCHK(hipMemcpyAsync(nfb, cnt, sizeof(nfb), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    cur = ctx->d_tiles_fb2; ncur = nfb[1];
  }
  if (level >= 3) ctx->n_tiles_fb = ncur;
  if (ncur) {
    ta.tiles = cur; ta.ntiles = ncur; ta.cap = ctx->tile_cap;
    if (pvr && mode_last == MODE_GAUSS2) { a.recon = a.addon; a.volw = a.cmap; }
    const TileArgs ta0 = ta;
    r = in_pieces(ncur, pvr ? WAVES_PER_BLOCK * 64 : TILE_WAVES * 64, [&](uint32_t off, uint32_t cntp) {
      ta.tiles = ta0.tiles + off; ta.ntiles = cntp;
      if (pvr) {
        if (mode_last == MODE_GAUSS2) hipLaunchKernelGGL(pvr_tiles_kernel<MODE_GAUSS2>, dim3(cntp), dim3(WAVES_PER_BLOCK * 64), 0, ctx->stream, a, ta);
        else hipLaunchKernelGGL(pvr_tiles_kernel<MODE_BACK>, dim3(cntp), dim3(WAVES_PER_BLOCK * 64), 0, ctx->stream, a, ta);
      } else {
        hipLaunchKernelGGL(back_tiled_kernel, dim3(cntp), dim3(TILE_WAVES * 64), (size_t)ctx->tile_cap * 2 * sizeof(float), ctx->stream, a, ta);
      }
      KCHK("scatter (last resort)");
      return (int)SVR_OK;
    });
    if (r) return r;
  }
  return SVR_OK;
}

#include "svr_cell.inc"
#include "svr_table.inc"   // the coefficient table's owner: its memory, order and ids, and a pass's begin / end on a table_plan
#include "svr_slab.inc"

// What each Change leaves stale.  A table written by a pass of the SR iterations holds that pass's PSF pixels only: every change that can
// add one drops it.  Rebuilt cell lists reset their gather factors and table ids (cell_prepare_state): the lists take them along.
// every buffer of a channel's SR iterations (svr_channel_sr_begin .. _end, svr_channel.inc): the call is over
void channel_sr_drop(svr_ctx *ctx) {
  ctx->d_csr_channel.reset(); ctx->d_csr_vol[0].reset(); ctx->d_csr_vol[1].reset(); ctx->d_csr_sim.reset(); ctx->d_csr_simw.reset();
  ctx->d_csr_unit_on.reset(); ctx->d_csr_cover.reset(); ctx->d_csr_inside.reset(); ctx->d_csr_slice_inside.reset();
  ctx->d_csr_guide.reset();
  ctx->csr_stage = 0; ctx->csr_cur = 0; ctx->csr_has_unit_on = false; ctx->csr_delta_g = 0.0f; ctx->csr_guide_only = false;
}

void invalidate(svr_ctx *ctx, unsigned ch) {
  if (ch & CH_SLICE_GEOMETRY) ctx->sc_dirty = true;
  if (ch & (CH_VOLUME_GRID | CH_SLICE_PIXELS)) channel_sr_drop(ctx);   // (a channel's SR iterations in flight were over the old grids: nothing of them is cached)
  if (ch & (CH_SLICE_PIXELS | CH_PSF_SUMS | CH_TILE_SHAPE)) ctx->psf_list_valid = false;
  if (ch & (CH_TAPS | CH_SLICE_PIXELS | CH_VOLUME_GRID | CH_TABLE | CH_TABLE_OFF)) ctx->table.drop();
  if (ch & CH_PSF_SUMS) ctx->table.drop_psf_pixels();
  if (ch & CH_TABLE_OFF) ctx->table.free_rows();
  const bool cells = ch & (CH_TAPS | CH_SLICE_PIXELS | CH_VOLUME_GRID | CH_CELL_SHAPE | CH_TABLE_OFF);
  if (cells) { ctx->cellc_valid = false; ctx->table.ids_stale(); }   // (the pixels' places in the table follow the scatter's lists)
  for (CellState *cs : {ctx->cell, ctx->cell_g}) {
    if (!cs) continue;
    if (cells) cs->valid = false;
    if (cells || (ch & CH_PSF_SUMS)) cs->gf_valid = false;
    if (cells || (ch & CH_TABLE_IDS)) cs->pid_valid = false;
  }
  if (ch & (CH_VOLUME_GRID | CH_MASK)) { ctx->vol_clean[0] = ctx->vol_clean[1] = false; if (ctx->slab) ctx->slab->valid = false; }   // (zero outside the old mask)
  if (ch & CH_MASK) ctx->mbox_valid = false;
  if (ch & (CH_VOLUME_GRID | CH_MASK_BLUR)) ctx->maskC_valid = false;
  if (ch & CH_VOLUME_VALUES) ctx->vol_clean[ctx->recon_cur == ctx->d_recon_new ? 1 : 0] = false;
  if (ch & (CH_VOLUME_GRID | CH_SCATTER_TARGETS)) ctx->cmap_from_scatter = false;
  if (ch & CH_VOLUME_GRID) { ctx->d_vote_best.reset(); ctx->d_vote_label.reset(); }   // (a vote in flight was over the old grid)
}

// The tile shape of the unit gather (fwd_unit_kernel: fwd_mode 1, and the coefficient table's gather) from the geometry, not from a
// timed trial: what the trials of rounds 1-3 picked, as a rule of the pixel density d = voxel area / pixel area in the slice plane.
// With the table (the pass waits for HBM; 24-32 pixels per tile keep two workgroups per CU): P4 (d 0.72) 6 x 4 2.79 ms against 2.85 for
// 6 x 5 and 3.07 for 4 x 4; S8 (d 0.56) 6 x 5 26.8 against 28.6 / 28.4 for 6 x 4 / 8 x 4; patches (support 12: smaller boxes) 8 x 4
// 8.1 against 9.0-9.5 ms.  On the fly: 6 x 4 (round 2: 4.21 against 4.60 ms for 4 x 4 on P4).  Near-ties all (2-6 %): a rule that
// repeats is worth more than the last per cent -- the table line of round 3 moved by 4 % from run to run with the trials' picks.
double pixel_density(const svr_ctx *ctx) {              // voxel area / pixel area in the slice plane
  double d = 1.0;
  if (ctx->slice_dims.size() >= 3 && ctx->slice_dims[0] > 0 && ctx->slice_dims[1] > 0)
    d = (double)ctx->vdim[0] * ctx->vdim[1] / ((double)ctx->slice_dims[0] * ctx->slice_dims[1]);
  return d;
}
void tile_shape_rule(const svr_ctx *ctx, bool table, int &w, int &h) {
  const double d = pixel_density(ctx);
  if (ctx->pvr) { w = 8; h = 4; }
  else if (table && d < 0.65) { w = 6; h = 5; }
  else { w = 6; h = 4; }
}
// The tiled scatters' tile of w x h pixels (option tile_w / tile_h, and the 6 x 4 rule of svr_superresolution_backproject): the tile
// lists are sized for it and built again.
int set_scatter_tile(svr_ctx *ctx, int w, int h) {
  ctx->tile_w = w; ctx->tile_h = h;
  if (!ctx->np) return SVR_OK;
  ctx->d_tiles.reset(); ctx->d_tiles_fb.reset(); ctx->d_tiles_fb2.reset();
  ctx->tiles_x = (int)((ctx->sx + w - 1) / w);
  ctx->tiles_y = (int)((ctx->sy + h - 1) / h);
  const size_t nb = (size_t)ctx->tiles_x * ctx->tiles_y * ctx->ns;
  HIPCHK(ctx->d_tiles.reserve(nb));
  HIPCHK(ctx->d_tiles_fb.reserve(nb));
  HIPCHK(ctx->d_tiles_fb2.reserve(nb));
  invalidate(ctx, CH_TILE_SHAPE);
  return SVR_OK;
}

// pass_path's inputs (svr_plan.h) from the context
PassOptions pass_options(const svr_ctx *ctx) {
  int sw, sh, gw, gh;
  cell_sizes(ctx, sw, sh, gw, gh);
  return {ctx->pvr, ctx->pvr_mode, ctx->back_mode, ctx->fwd_mode, ctx->gauss_mode, ctx->bias_mode, ctx->fwd_mode_user, pixel_density(ctx), gw * gh};
}
PassPath pass_path(const svr_ctx *ctx, Pass pass) { return pass_path(pass_options(ctx), pass); }
// The cell lists for a pass on FAM_CELLS (gather: the gather's own when it works on another cell size) -> cs; nullptr where they cannot
// hold the geometry (CellState::usable), with the fallback counted and, the first time, said.
int cells_or_fallback(svr_ctx *ctx, bool gather, int kind, const char *what, CellState *&cs) {
  cs = nullptr;
  int r;
  if (gather) r = cell_prepare_gather(ctx, cs);
  else if (!(r = cell_prepare(ctx))) cs = ctx->cell;
  if (r) return r;
  if (cs && cs->usable) return SVR_OK;
  cs = nullptr;
  ctx->note_fallback(kind, what);
  return SVR_OK;
}
const char *const SCATTER_LEFT_CELLS = "the scatter left the cell path (the cell lists cannot hold this geometry): back_mode 4, float atomics, last bits depend on the run";

// FAM_PIXELS: a wavefront per entry of the pixel list (psf_kernel<MODE> / pvr_kernel<MODE>)
int launch_pixels(svr_ctx *ctx, const PsfArgs &a, void (*kernel)(PsfArgs), const char *name) {
  return pixel_list_in_pieces(a, [&](const PsfArgs &ap, uint32_t) {
    hipLaunchKernelGGL(kernel, dim3(nblk(ap.n, WAVES_PER_BLOCK)), dim3(WAVES_PER_BLOCK * 64), 0, ctx->stream, ap);
    KCHK(name);
    return (int)SVR_OK;
  });
}
// {V m, m} per voxel for the gathers' boxes (patch-based: V through the 8-voxel average) -> a.volm
// (vol: the volume the pass projects -- the reconstruction, or a channel volume of svr_channel.inc)
int pack_volm(svr_ctx *ctx, PsfArgs &a, const float *vol) {
  HIPCHK(ctx->d_volm.reserve(ctx->nv));
  if (ctx->pvr) hipLaunchKernelGGL(k_pack_volm_pvr, dim3(nblk(ctx->nv)), dim3(256), 0, ctx->stream, vol, ctx->d_mask, ctx->d_volm, a.vg);
  else hipLaunchKernelGGL(k_pack_volm, dim3(nblk(ctx->nv)), dim3(256), 0, ctx->stream, vol, ctx->d_mask, ctx->d_volm, ctx->nv);
  KCHK(ctx->pvr ? "k_pack_volm_pvr" : "k_pack_volm");
  a.volm = ctx->d_volm;
  return SVR_OK;
}
// FAM_TILES, the gathers: fwd_unit_kernel over a list of tw x th-pixel tiles (GAUSS1: pass 1 of the Gaussian reconstruction)
template <bool GAUSS1>
int launch_unit_gather(svr_ctx *ctx, const PsfArgs &a, const uint32_t *tiles, uint32_t ntiles, int tiles_x, int tiles_y, int tw, int th) {
  if (!ntiles) return SVR_OK;
  TileArgs ta;
  ta.tiles = tiles; ta.ntiles = ntiles; ta.tiles_x = tiles_x; ta.tiles_y = tiles_y; ta.tw = tw; ta.th = th; ta.gauss = GAUSS1 ? 1 : 0;
  ta.cap = std::min(ctx->fwd_unit_cap, ctx->tile_cap);
  launch_fwd_unit<GAUSS1>(ctx, a, ta, (size_t)ta.cap * 2 * sizeof(float));
  KCHK(GAUSS1 ? "fwd_unit_kernel<GAUSS1>" : "fwd_unit_kernel");
  return SVR_OK;
}

// reduce partial[ns*chunks][K] -> per_slice[ns][K] (+ optionally -> d_out[K])
int reduce_partials(svr_ctx *ctx, int K, int mn, int mx, bool global) {
  if (K < 1 || K > REDUCE_MAXK) return fail(ctx, SVR_E_ARG, "reduce_partials: 1..8 quantities (k_reduce_slices holds them side by side; d_partial / d_per_slice are sized for them)");
  hipLaunchKernelGGL(k_reduce_chunks, dim3(nblk((size_t)ctx->ns * K)), dim3(256), 0, ctx->stream,
                     ctx->d_partial, (int)ctx->ns, ctx->chunks, K, mn, mx, ctx->d_per_slice);
  KCHK("k_reduce_chunks");
  if (global) {
    hipLaunchKernelGGL(k_reduce_slices, dim3(1), dim3(256), 0, ctx->stream, ctx->d_per_slice, (int)ctx->ns, K,
                       mn, mx, ctx->d_out);
    KCHK("k_reduce_slices");
  }
  return SVR_OK;
}

// a per-slice vector to the device, asynchronously: through a pinned slot (the caller's memory is free again on return), no
// stream synchronisation; `mirror` = what the device vector holds, an identical vector is not sent again
int upload_ns(svr_ctx *ctx, float *dst, const float *src, std::vector<float> &mirror) {
  const size_t n = ctx->ns;
  if (dst == ctx->d_slice_weights) ctx->sem_weights_current = false;
  if (mirror.size() == n && !memcmp(mirror.data(), src, n * sizeof(float))) return SVR_OK;
  if (!ctx->h_up) {
    HIPCHK(hipHostMalloc((void **)&ctx->h_up, (size_t)svr_ctx::UP_SLOTS * n * sizeof(float), hipHostMallocDefault));
    for (int k = 0; k < svr_ctx::UP_SLOTS; ++k) HIPCHK(hipEventCreateWithFlags(&ctx->up_ev[k], hipEventDisableTiming));
  }
  const int k = ctx->up_next;
  ctx->up_next = (k + 1) % svr_ctx::UP_SLOTS;
  if (ctx->up_busy[k]) HIPCHK(hipEventSynchronize(ctx->up_ev[k]));       // the copy that last used the slot (long done)
  float *slot = ctx->h_up + (size_t)k * n;
  memcpy(slot, src, n * sizeof(float));
  HIPCHK(hipMemcpyAsync(dst, slot, n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipEventRecord(ctx->up_ev[k], ctx->stream));
  ctx->up_busy[k] = true;
  mirror.assign(src, src + n);
  return SVR_OK;
}

// queue a small device -> host copy; nothing is in `dst` before down_flush.  A call that fails drops everything queued so far
// (the destinations are the caller's memory: a later, unrelated down_flush must not write to them)
// make room for `total` more bytes of queued copies.  With copies already in flight into the arena the stream is waited for and what
// has arrived moves into the larger arena (round 5 refused here: a batch whose LATER items were larger than its first -- the
// slice-level EM's vectors of the GLOBAL slice count on a rank that holds a fraction of the slices -- failed with SVR_E_STATE)
int down_reserve(svr_ctx *ctx, size_t total) {
  auto drop = [&](int code, const std::string &msg) { ctx->down_items.clear(); ctx->down_used = 0; return fail(ctx, code, msg); };
  const size_t need = ctx->down_used + total;
  if (need <= ctx->down_cap) return SVR_OK;
  const size_t cap = std::max<size_t>(need + need / 2, (size_t)ctx->ns * 12 + 4096);
  unsigned char *fresh = nullptr;
  hipError_t e = hipHostMalloc((void **)&fresh, cap, hipHostMallocDefault);
  if (e != hipSuccess) return drop((int)e, std::string("down_queue: hipHostMalloc: ") + hipGetErrorString(e));
  if (!ctx->down_items.empty()) {
    e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { (void)hipHostFree(fresh); return drop((int)e, std::string("down_queue: hipStreamSynchronize: ") + hipGetErrorString(e)); }
    memcpy(fresh, ctx->h_down, ctx->down_used);
  }
  if (ctx->h_down) (void)hipHostFree(ctx->h_down);
  ctx->h_down = fresh;
  ctx->down_cap = cap;
  return SVR_OK;
}
int down_queue(svr_ctx *ctx, void *dst, const void *src, size_t bytes) {
  auto drop = [&](int code, const std::string &msg) { ctx->down_items.clear(); ctx->down_used = 0; return fail(ctx, code, msg); };
  const size_t padded = (bytes + 63) & ~(size_t)63;
  { const int r = down_reserve(ctx, padded); if (r) return r; }
  const hipError_t e = hipMemcpyAsync(ctx->h_down + ctx->down_used, src, bytes, hipMemcpyDeviceToHost, ctx->stream);
  if (e != hipSuccess) return drop((int)e, std::string("down_queue: hipMemcpyAsync: ") + hipGetErrorString(e));
  ctx->down_items.push_back({dst, ctx->down_used, bytes});
  ctx->down_used += padded;
  return SVR_OK;
}
int down_flush(svr_ctx *ctx) {
  const hipError_t e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess)
    for (const auto &it : ctx->down_items) memcpy(it.dst, ctx->h_down + it.off, it.bytes);
  ctx->down_items.clear();
  ctx->down_used = 0;
  if (e != hipSuccess) return fail(ctx, (int)e, std::string("down_flush: ") + hipGetErrorString(e));
  return SVR_OK;
}

}  // namespace

// ==========================================================================================
// C-ABI
// ==========================================================================================
extern "C" {

int svr_create(int device, svr_ctx **out) {
  if (!out) return SVR_E_ARG;
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return (int)e;
  if (device < 0 || device >= n) return SVR_E_ARG;
  e = hipSetDevice(device);
  if (e != hipSuccess) return (int)e;
  svr_ctx *ctx = new svr_ctx();
  ctx->device = device;
  e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
  if (e != hipSuccess) { delete ctx; return (int)e; }
  ctx->own_stream = true;
  if (ctx->d_counter.reserve(16) != hipSuccess || ctx->d_out.reserve(16) != hipSuccess) {
    svr_destroy(ctx);
    return (int)hipErrorOutOfMemory;
  }
  {
    // LDS accumulator of the tiled scatter: everything the CU has minus the static part
    int lds_max = 0;
    (void)hipDeviceGetAttribute(&ctx->n_cu, hipDeviceAttributeMultiprocessorCount, device);
    if (ctx->n_cu <= 0) ctx->n_cu = 256;
    (void)hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, device);
    if (lds_max <= 0) lds_max = 65536;
    int dyn = lds_max - 1024;
    dyn -= 16384;  // static LDS of the kernels (pixel table, unit lists, partial sums: fwd_unit_kernel<GAUSS1> 14.6 KiB)
    const void *big_lds[] = {reinterpret_cast<const void *>(back_tiled_kernel),
                             reinterpret_cast<const void *>(fwd_unit_kernel<false>), reinterpret_cast<const void *>(fwd_unit_kernel<true>),
                             reinterpret_cast<const void *>(fwd_unit_kernel<false, PSF_SUPPORT, false, true>),
                             reinterpret_cast<const void *>(fwd_unit_kernel<false, PVR_N, true>), reinterpret_cast<const void *>(fwd_unit_kernel<true, PVR_N, true>),
                             reinterpret_cast<const void *>(back_wave_kernel<>), reinterpret_cast<const void *>(back_wave_kernel<PVR_N, true>),
                             reinterpret_cast<const void *>(back_wave_kernel<PSF_SUPPORT, false, true>), reinterpret_cast<const void *>(back_wave_kernel<PVR_N, true, true>),
                             reinterpret_cast<const void *>(fwd_unit_kernel<false, PVR_N, true, true>), reinterpret_cast<const void *>(fwd_unit_kernel<true, PVR_N, true, true>),
                             reinterpret_cast<const void *>(fwd_unit_kernel<true, PSF_SUPPORT, false, true>),
                             reinterpret_cast<const void *>(back_slot_kernel<8>), reinterpret_cast<const void *>(back_slot_kernel<8, PVR_N, true>)};
    bool ok = true;
    for (const void *f : big_lds) ok = ok && hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, dyn) == hipSuccess;
    if (!ok) {
      (void)hipGetLastError();
      dyn = 65536 - 1024 - 16384;  // the default 64 KiB minus the kernels' static LDS
    }
    ctx->tile_cap = dyn / (2 * (int)sizeof(float));
  }
  // SVR_TILE_PIN="GWxGH,SWxSH,BOX": the gather's tile, the tiled scatter's tile and its LDS box fixed instead of following the geometry, so that a
  // run can be repeated with the same shapes (on every rank, in every process); bench.py prints the shapes in config.tuned
  if (const char *v = getenv("SVR_CELL_ORDER")) ctx->cell_order = std::min(20, std::max(0, atoi(v)));   // (experiments: the options' defaults)
  if (const char *v = getenv("SVR_CELL_BALANCE")) ctx->cell_balance = std::min(1024, std::max(0, atoi(v)));
  if (const char *pin = getenv("SVR_TILE_PIN")) {
    int gw, gh, sw, sh, box;
    if (sscanf(pin, "%dx%d,%dx%d,%d", &gw, &gh, &sw, &sh, &box) == 5 && gw > 0 && gh > 0 && gw * gh <= 32 && sw > 0 && sh > 0 && sw * sh <= 64 && box >= 1024) {
      ctx->fwd_tw = gw; ctx->fwd_th = gh; ctx->fwd_tile_user = true;
      ctx->tile_w = sw; ctx->tile_h = sh; ctx->tile_user = true;
      ctx->wave_cap = box; ctx->wave_cap_user = true;
    } else {
      fprintf(stderr, "svr_create: SVR_TILE_PIN=\"%s\" ignored (expected e.g. 6x5,6x4,2096)\n", pin);
    }
  }
  *out = ctx;
  return SVR_OK;
}

int svr_set_option(svr_ctx *ctx, const char *name, int value) {
  SVR_ENTER(ctx);
  if (!ctx || !name) return SVR_E_ARG;
  // Round 6: the scatter generations before the wave-owned tile kernel (0 = a wavefront per pixel with device atomics per tap, 1 = LDS atomics per tile,
  // 3 = the workgroup's slot kernel as a mode of its own) and the wave-per-pixel gather (fwd_mode 0) stay in the library for the tests that pin the
  // generations against each other and as the tile path's own re-run kernels -- asking for one by option needs "legacy_kernels" 1 first.
  if (!strcmp(name, "legacy_kernels")) { ctx->legacy_ok = value != 0; return SVR_OK; }
  if (!strcmp(name, "back_mode")) {
    if (value < 0 || value > 5 || value == 2) return fail(ctx, SVR_E_ARG, "back_mode: 5 (cells), 4 (tile fallback); 0 / 1 / 3 behind legacy_kernels");
    if (value < 4 && !ctx->legacy_ok && !ctx->pvr) return fail(ctx, SVR_E_ARG, "back_mode 0 / 1 / 3: set option legacy_kernels 1 first (kept for the tests; the product runs 5 with 4 as its fallback)");
    ctx->back_mode = value; ctx->back_mode_user = true; return SVR_OK;
  }
  if (!strcmp(name, "sr_no_wait")) { ctx->sr_no_wait = value != 0; return SVR_OK; }   // svr_superresolution_backproject / _update / svr_slab_finish return without waiting for the device (a sharded run whose collectives share the stream)
  if (!strcmp(name, "reg_tile")) { if (value < -1 || value > 2) return fail(ctx, SVR_E_ARG, "reg_tile: -1 .. 2"); ctx->reg_tile = value; return SVR_OK; }
  if (!strcmp(name, "reg_mode")) { if (value < 0 || value > 1) return fail(ctx, SVR_E_ARG, "reg_mode: 0 or 1"); ctx->reg_mode = value; return SVR_OK; }
  if (!strcmp(name, "fwd_mode")) {                         // 2: cell gather, 1: unit-based gather per slice tile (fallback), 0: wave-per-pixel kernel (legacy_kernels)
    if (value < 0 || value > 2) return fail(ctx, SVR_E_ARG, "fwd_mode: 2 (cells), 1 (tile fallback); 0 behind legacy_kernels");
    if (value == 0 && !ctx->legacy_ok && !ctx->pvr) return fail(ctx, SVR_E_ARG, "fwd_mode 0: set option legacy_kernels 1 first (kept for the tests; the product runs 2 with 1 as its fallback)");
    ctx->fwd_mode = value; ctx->fwd_mode_user = true; return SVR_OK;
  }
  if (!strcmp(name, "pvr_mode")) { ctx->pvr_mode = value; return SVR_OK; }
  if (!strcmp(name, "gauss_mode")) { ctx->gauss_mode = value; return SVR_OK; }
  if (!strcmp(name, "fwd_unit_cap")) { ctx->fwd_unit_cap = std::max(2048, value); return SVR_OK; }
  if (!strcmp(name, "fwd_tile_w") || !strcmp(name, "fwd_tile_h")) {
    int w = !strcmp(name, "fwd_tile_w") ? value : ctx->fwd_tw, h = !strcmp(name, "fwd_tile_h") ? value : ctx->fwd_th;
    if (w < 1 || h < 1 || w * h > 32) return fail(ctx, SVR_E_ARG, "fwd tile must hold 1..32 pixels");   // FWDU_MAXPIX: the gather's pixel tables
    ctx->fwd_tw = w; ctx->fwd_th = h; invalidate(ctx, CH_TILE_SHAPE);
    ctx->fwd_tile_user = true;                           // an explicit shape is left alone
    return SVR_OK;
  }
  if (!strcmp(name, "fwd_autotune")) {                     // (the name stays readable; 0 is all it can be)
    if (value) return fail(ctx, SVR_E_ARG, "fwd_autotune: the timed trial launches were removed; the tile shapes follow from the geometry (0 is accepted and changes nothing)");
    return SVR_OK;
  }
  if (!strcmp(name, "pvr")) { ctx->pvr = value ? 1 : 0; ctx->table.want_by_default(!value); invalidate(ctx, CH_SLICE_GEOMETRY | CH_TILE_SHAPE | CH_TABLE_OFF); return SVR_OK; }
  if (!strcmp(name, "coeff_lazy")) { ctx->table.set_lazy(value != 0); return SVR_OK; }
  if (!strcmp(name, "coeff_invalidate")) { invalidate(ctx, CH_TABLE); return SVR_OK; }   // (what a new slice geometry does to the table: bench.py's outer iterations)
  if (!strcmp(name, "coeff_table")) {
    ctx->table.want(value != 0);
    if (!value) invalidate(ctx, CH_TABLE_OFF);
    return SVR_OK;
  }
  if (!strcmp(name, "cell_combine")) { if (value < 0 || value > 2) return fail(ctx, SVR_E_ARG, "cell_combine: 0, 1 or 2"); ctx->cell_combine = value; return SVR_OK; }
  // the options of the cell lists' layout: the lists are built again
  static const char *cwh = "cell_w / cell_h / cell_gw / cell_gh: 1..32, 0 = by the pixel density";
  static const struct { const char *n; int lo, hi; int svr_ctx::*f; const char *what; } cell_opts[] = {
      {"cell_band", 0, 10, &svr_ctx::cell_band, "cell_band: 0..10 (a run holds 2^cell_band centre planes)"},
      {"cell_qx", 1, 4, &svr_ctx::cell_qx, "cell_qx: 1, 2 or 4"},
      {"cell_w", 0, 32, &svr_ctx::cell_w, cwh}, {"cell_h", 0, 32, &svr_ctx::cell_h, cwh},
      {"cell_gw", 0, 32, &svr_ctx::cell_gw, cwh}, {"cell_gh", 0, 32, &svr_ctx::cell_gh, cwh},
      {"cell_order", 0, 20, &svr_ctx::cell_order, "cell_order: 0..20"},
      {"cell_balance", 0, 1024, &svr_ctx::cell_balance, "cell_balance: 0..1024"},
      {"cell_split", 1, 32, &svr_ctx::cell_split, "cell_split: 1..32"}};
  for (const auto &o : cell_opts) {
    if (strcmp(name, o.n)) continue;
    if (value < o.lo || value > o.hi || (o.f == &svr_ctx::cell_qx && value == 3)) return fail(ctx, SVR_E_ARG, o.what);
    ctx->*o.f = value;
    invalidate(ctx, CH_CELL_SHAPE);
    return SVR_OK;
  }
  if (!strcmp(name, "wave_groups")) { ctx->wave_groups = std::max(1, value); return SVR_OK; }
  if (!strcmp(name, "wave_cap")) { ctx->wave_cap = std::max(1024, value); ctx->wave_cap_user = true; return SVR_OK; }
  if (!strcmp(name, "reg_blind")) { ctx->reg_blind = std::max(0, value); return SVR_OK; }
  if (!strcmp(name, "reg_red_threads")) {
    if (value != 0 && value != 256 && value != 1024) return fail(ctx, SVR_E_ARG, "reg_red_threads: 0, 256 or 1024");
    ctx->reg_red_threads = value;
    return SVR_OK;
  }
  if (!strcmp(name, "reg_batch")) { ctx->reg_batch = value ? 1 : 0; return SVR_OK; }
  if (!strcmp(name, "bias_mode")) { if (value < 0 || value > 2) return fail(ctx, SVR_E_ARG, "bias_mode: 0, 1 or 2"); ctx->bias_mode = value; return SVR_OK; }
  if (!strcmp(name, "fit_chunk")) { if (value < 1 || value > (1 << 24)) return fail(ctx, SVR_E_ARG, "fit_chunk: 1 .. 16777216 voxels"); ctx->fit_chunk = value; return SVR_OK; }
  if (!strcmp(name, "pvr_reg_levels")) { ctx->pvr_reg_levels = std::min(3, std::max(1, value)); return SVR_OK; }
  if (!strcmp(name, "pvr_reg_steps")) { ctx->pvr_reg_steps = std::max(1, value); return SVR_OK; }
  if (!strcmp(name, "pvr_reg_iterations")) { ctx->pvr_reg_iterations = std::max(1, value); return SVR_OK; }
  if (!strcmp(name, "tile_w") || !strcmp(name, "tile_h")) {
    int w = !strcmp(name, "tile_w") ? value : ctx->tile_w, h = !strcmp(name, "tile_h") ? value : ctx->tile_h;
    if (w < 1 || h < 1 || w * h > 64) return fail(ctx, SVR_E_ARG, "tile_w * tile_h must be in 1..64");
    ctx->tile_user = true;                               // an explicit shape is left alone
    return set_scatter_tile(ctx, w, h);
  }
  return fail(ctx, SVR_E_ARG, std::string("unknown option ") + name);
}

int svr_get_option(svr_ctx *ctx, const char *name, int *value) {
  SVR_ENTER(ctx);
  if (!ctx || !name || !value) return SVR_E_ARG;
  int csw, csh, cgw, cgh;
  cell_sizes(ctx, csw, csh, cgw, cgh);                   // the cell sizes in effect (0 = automatic resolved)
  const bool cells_valid = ctx->cell && ctx->cell->valid && ((cgw == csw && cgh == csh) || !ctx->cell_g || ctx->cell_g->valid);   // (+ the gather's own)
  const struct { const char *n; int v; } tab[] = {
      {"back_mode", ctx->back_mode}, {"reg_mode", ctx->reg_mode}, {"fwd_mode", ctx->fwd_mode}, {"gauss_mode", ctx->gauss_mode}, {"pvr_mode", ctx->pvr_mode},
      {"pvr", ctx->pvr}, {"coeff_table", ctx->table.coeff_mode}, {"coeff_lazy", ctx->table.coeff_lazy}, {"coeff_valid", ctx->table.coeff_state != COEFF_NONE}, {"coeff_state", ctx->table.coeff_state}, {"tile_w", ctx->tile_w}, {"tile_h", ctx->tile_h},
      {"fwd_tile_w", ctx->fwd_tw}, {"fwd_tile_h", ctx->fwd_th}, {"wave_cap", ctx->wave_cap}, {"tile_cap", ctx->tile_cap}, {"cell_w", csw}, {"cell_h", csh}, {"cell_gw", cgw}, {"cell_gh", cgh}, {"cell_split", ctx->cell_split}, {"cell_order", ctx->cell_order}, {"cell_balance", ctx->cell_balance}, {"cell_combine", ctx->cell_combine}, {"fwd_autotune", 0}, {"cell_qx", ctx->cell_qx}, {"fwd_unit_cap", ctx->fwd_unit_cap}, {"reg_batch", ctx->reg_batch}, {"reg_blind", ctx->reg_blind},
      {"bias_mode", ctx->bias_mode}, {"bias_corrections", ctx->bias_corrections}, {"bias_normalisations", ctx->bias_normalisations},
      {"bias_scatters", ctx->bias_scatters}, {"bias_scatters_on_cells", ctx->bias_scatters_on_cells},
      {"bias_field_bx", ctx->last_bias_bx}, {"bias_tail_lds", ctx->last_tail_lds}, {"bias_tail_rows", ctx->last_tail_rows},
      {"bias_tail_bxy", ctx->last_tail_bxy}, {"bias_tail_bxz", ctx->last_tail_bxz}, {"reg_zc", ctx->last_reg_zc}, {"reg_chunks", ctx->last_reg_chunks},
      {"psf_list_valid", ctx->psf_list_valid}, {"cells_valid", cells_valid}, {"quality_chunks", ctx->last_quality_chunks}, {"fit_chunk", ctx->fit_chunk}};
  for (const auto &e : tab)
    if (!strcmp(name, e.n)) { *value = e.v; return SVR_OK; }
  return fail(ctx, SVR_E_ARG, std::string("unknown option ") + name);
}

void svr_destroy(svr_ctx *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipDeviceSynchronize();
  free_slices(ctx);              // (the pinned slots and their events; the device buffers go with the context's members)
  reg_free(ctx->reg);
  cell_free(ctx->cell);
  cell_free(ctx->cell_g);
  slab_free(ctx->slab);
  slice_em_free(ctx->sem);
  timers_resolve(ctx);
  if (ctx->ev_open) (void)hipEventDestroy(ctx->ev_open);
  for (hipEvent_t e : ctx->ev_free) (void)hipEventDestroy(e);
  ctx->ev_free.clear();
  if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

const char *svr_last_error(const svr_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int svr_set_flags(svr_ctx *ctx, int disable_bias_correction, int debug_gpu) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  ctx->disable_bias = disable_bias_correction != 0;
  ctx->debug_gpu = debug_gpu != 0;
  // with the geometry known, the bias buffers come now, before a coefficient table sizes itself on the free memory
  if (!ctx->disable_bias) { HIPCHK(hipSetDevice(ctx->device)); return ensure_bias_buffers(ctx); }
  return SVR_OK;
}

int svr_set_stream(svr_ctx *ctx, void *hip_stream) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
  ctx->stream = (hipStream_t)hip_stream;
  ctx->own_stream = false;
  return SVR_OK;
}

void *svr_get_stream(svr_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }
int svr_stream_sync(svr_ctx *ctx) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}
int svr_device(svr_ctx *ctx) { return ctx ? ctx->device : -1; }
int svr_device_count(void) {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

int svr_init_reconstruction_volume(svr_ctx *ctx, const uint32_t size[3], const float dim[3],
                                   const float *data, float sigma_bias) {
  SVR_ENTER(ctx);
  if (!ctx || !size || !dim) return SVR_E_ARG;
  (void)sigma_bias;
  HIPCHK(hipSetDevice(ctx->device));
  size_t nv = (size_t)size[0] * size[1] * size[2];
  if (nv == 0 || nv >= 0xFFFFFFFFull) return fail(ctx, SVR_E_ARG, "volume size out of range");
  free_volume(ctx);
  ctx->d_bias_vol.reset(); ctx->d_volume_weights.reset(); ctx->d_maskC.reset(); ctx->d_mbuf.reset();
  ctx->vx = size[0]; ctx->vy = size[1]; ctx->vz = size[2];
  memcpy(ctx->vdim, dim, 3 * sizeof(float));
  ctx->nv = nv;
  invalidate(ctx, CH_VOLUME_GRID);
  HIPCHK(ctx->d_recon_volw.reserve(2 * nv));
  HIPCHK(ctx->d_addon_cmap.reserve(2 * nv));
  HIPCHK(ctx->d_recon_new.reserve(nv));
  ctx->recon_cur = ctx->d_recon_volw;
  ctx->prep_pending = false;
  HIPCHK(hipMemsetAsync(ctx->d_recon_volw, 0, 2 * nv * sizeof(float), ctx->stream));   // RC.cu:1199-1229
  HIPCHK(hipMemsetAsync(ctx->d_addon_cmap, 0, 2 * nv * sizeof(float), ctx->stream));
  if (data) HIPCHK(hipMemcpyAsync(ctx->recon(), data, nv * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

int svr_set_mask(svr_ctx *ctx, const uint32_t size[3], const float dim[3], const float *data,
                 float sigma_bias) {
  SVR_ENTER(ctx);
  if (!ctx || !size || !data) return SVR_E_ARG;
  (void)dim;   // the blurred maskC_ (RC.cu:1129-1157) is built lazily: it only feeds NormaliseBias
  NEED(ctx->nv > 0, "InitReconstructionVolume first");
  if ((size_t)size[0] * size[1] * size[2] != ctx->nv || size[0] != ctx->vx || size[1] != ctx->vy)
    return fail(ctx, SVR_E_ARG, "mask grid differs from the reconstruction volume");
  ctx->d_mask.reset();
  HIPCHK(ctx->d_mask.reserve(ctx->nv));
  HIPCHK(hipMemcpyAsync(ctx->d_mask, data, ctx->nv * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->have_mask = true;
  ctx->mask_sigma_bias = sigma_bias;
  invalidate(ctx, CH_MASK | CH_MASK_BLUR);
  {
    int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {-1, -1, -1};
    const size_t sxy = (size_t)ctx->vx * ctx->vy;
    for (uint32_t z = 0; z < ctx->vz; ++z)
      for (uint32_t y = 0; y < ctx->vy; ++y) {
        const float *row = data + z * sxy + (size_t)y * ctx->vx;
        int x0 = -1, x1 = -1;
        for (uint32_t x = 0; x < ctx->vx; ++x)
          if (row[x] != 0.0f) { if (x0 < 0) x0 = (int)x; x1 = (int)x; }
        if (x0 >= 0) {
          lo[0] = std::min(lo[0], x0); hi[0] = std::max(hi[0], x1);
          lo[1] = std::min(lo[1], (int)y); hi[1] = std::max(hi[1], (int)y);
          lo[2] = std::min(lo[2], (int)z); hi[2] = std::max(hi[2], (int)z);
        }
      }
    ctx->mbox_valid = hi[0] >= 0;
    for (int k = 0; k < 3; ++k) { ctx->mbox_lo[k] = lo[k]; ctx->mbox_hi[k] = hi[k]; }
  }
  return SVR_OK;
}

// ---- the part of a volume pair a sharded run has to exchange -------------------------------------------------------------
__global__ void k_pair_pack(const float *vol, float *packed, int nvols, size_t nv, int vx, int vy, int lx, int ly, int lz, int bx, int by, int bz, int unpack,
                            float *vol_out) {
  const size_t nb = (size_t)bx * by * bz;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nb * nvols) return;
  const int v = (int)(i / nb);
  const size_t r = i - (size_t)v * nb;
  const int z = (int)(r / ((size_t)bx * by)), y = (int)((r / bx) % by), x = (int)(r % bx);
  const size_t g = (size_t)v * nv + (size_t)(x + lx) + (size_t)(y + ly) * vx + (size_t)(z + lz) * vx * vy;
  if (unpack) vol_out[g] = packed[i];
  else packed[i] = vol[g];
}
int svr_pair_pack(svr_ctx *ctx, int which, size_t n_floats, void **packed, size_t *n_packed) {
  SVR_ENTER(ctx);
  if (!ctx || !packed || !n_packed) return SVR_E_ARG;
  *packed = nullptr; *n_packed = 0;
  float *vol = static_cast<float *>(svr_device_ptr(ctx, which));
  if (!vol || !ctx->mbox_valid || !ctx->nv || n_floats % ctx->nv) return SVR_OK;          // nothing to gain: the caller reduces the whole buffer
  const int nvols = (int)(n_floats / ctx->nv);
  const int bx = ctx->mbox_hi[0] - ctx->mbox_lo[0] + 1, by = ctx->mbox_hi[1] - ctx->mbox_lo[1] + 1, bz = ctx->mbox_hi[2] - ctx->mbox_lo[2] + 1;
  const size_t nb = (size_t)bx * by * bz;
  if (nb * 5 > ctx->nv * 4) return SVR_OK;                // the box is more than 80 % of the volume: not worth two copies
  HIPCHK(ctx->d_pair_pack.reserve(nb * nvols));
  hipLaunchKernelGGL(k_pair_pack, dim3(nblk(nb * nvols)), dim3(256), 0, ctx->stream, vol, ctx->d_pair_pack, nvols, ctx->nv, (int)ctx->vx, (int)ctx->vy,
                     ctx->mbox_lo[0], ctx->mbox_lo[1], ctx->mbox_lo[2], bx, by, bz, 0, (float *)nullptr);
  KCHK("k_pair_pack");
  *packed = ctx->d_pair_pack;
  *n_packed = nb * nvols;
  return SVR_OK;
}
int svr_pair_unpack(svr_ctx *ctx, int which, size_t n_floats) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  float *vol = static_cast<float *>(svr_device_ptr(ctx, which));
  NEED(vol && ctx->mbox_valid && ctx->d_pair_pack && ctx->nv && n_floats % ctx->nv == 0, "svr_pair_pack first");
  const int nvols = (int)(n_floats / ctx->nv);
  const int bx = ctx->mbox_hi[0] - ctx->mbox_lo[0] + 1, by = ctx->mbox_hi[1] - ctx->mbox_lo[1] + 1, bz = ctx->mbox_hi[2] - ctx->mbox_lo[2] + 1;
  const size_t nb = (size_t)bx * by * bz;
  hipLaunchKernelGGL(k_pair_pack, dim3(nblk(nb * nvols)), dim3(256), 0, ctx->stream, (const float *)nullptr, ctx->d_pair_pack, nvols, ctx->nv, (int)ctx->vx,
                     (int)ctx->vy, ctx->mbox_lo[0], ctx->mbox_lo[1], ctx->mbox_lo[2], bx, by, bz, 1, vol);
  KCHK("k_pair_unpack");
  return SVR_OK;
}

int svr_init_storage_volumes(svr_ctx *ctx, const uint32_t size[3], const float dim[3]) {
  SVR_ENTER(ctx);
  if (!ctx || !size) return SVR_E_ARG;
  (void)dim;
  HIPCHK(hipSetDevice(ctx->device));
  size_t np = (size_t)size[0] * size[1] * size[2];
  // slice-grid indices are 32-bit; every launch that takes a wavefront per pixel or per tile goes out in pieces of < 2^32
  // work-items (in_pieces), like the reference's MAX_SLICES_PER_RUN chunks (RC.cu:2207-2219, 2414-2432, 2701-2716)
  if (np == 0 || np >= (1ull << 31)) return fail(ctx, SVR_E_ARG, "slice grid out of range: 1 .. 2^31 - 1 pixels per context (shard the slices over more ranks)");
  free_slices(ctx);
  ctx->d_bias.reset(); ctx->d_wb.reset(); ctx->d_wr.reset(); ctx->d_buffer.reset();
  ctx->d_spx.reset();                                     // the superpixel masks are indexed by the old grid's slices: svr_set_spx_masks comes after the grid
  ctx->sx = size[0]; ctx->sy = size[1]; ctx->ns = size[2];
  ctx->np = np;
  ctx->have_slices = false; ctx->have_sim = false; ctx->have_scales = false; ctx->have_dims = false; ctx->have_mats = false;
  ctx->have_em = false;
  ctx->n_active = ctx->n_psf = 0;
  invalidate(ctx, CH_SLICE_GEOMETRY | CH_SLICE_PIXELS | CH_TABLE_OFF);
  ctx->table.free_ids();
  const size_t fb = np * sizeof(float);
  HIPCHK(ctx->d_slices.reserve(np));
  HIPCHK(ctx->d_weights.reserve(np));
  HIPCHK(ctx->d_simslices.reserve(np));
  HIPCHK(ctx->d_simweights.reserve(np));
  HIPCHK(ctx->d_psf_sums.reserve(np));
  HIPCHK(ctx->d_siminside.reserve(np));
  HIPCHK(ctx->d_voxcount.reserve(np));
  HIPCHK(ctx->d_active.reserve(np));
  HIPCHK(ctx->d_psf_list.reserve(np));
  ctx->tiles_x = (int)((ctx->sx + ctx->tile_w - 1) / ctx->tile_w);
  ctx->tiles_y = (int)((ctx->sy + ctx->tile_h - 1) / ctx->tile_h);
  HIPCHK(ctx->d_tiles.reserve((size_t)ctx->tiles_x * ctx->tiles_y * ctx->ns));
  HIPCHK(ctx->d_tiles_fb.reserve((size_t)ctx->tiles_x * ctx->tiles_y * ctx->ns));
  HIPCHK(ctx->d_tiles_fb2.reserve((size_t)ctx->tiles_x * ctx->tiles_y * ctx->ns));
  HIPCHK(ctx->d_scales.reserve(ctx->ns));
  HIPCHK(ctx->d_slice_weights.reserve(ctx->ns));
  ctx->sem_weights_current = false;
  slice_em_invalidate(ctx->sem);                          // the slice-level EM's arrays and rank ranges were set up for the old slice count
  HIPCHK(ctx->d_scales_host_copy.reserve(ctx->ns));
  HIPCHK(ctx->d_tmp_ns.reserve(ctx->ns));
  HIPCHK(ctx->d_slice_inside.reserve(ctx->ns));
  HIPCHK(ctx->d_sc.reserve(ctx->ns));
  ctx->chunks = (int)(((size_t)ctx->sx * ctx->sy + CHUNK_PIX - 1) / CHUNK_PIX);
  HIPCHK(ctx->d_partial.reserve((size_t)ctx->ns * ctx->chunks * REDUCE_MAXK));    // (reduce_partials' guard is the same constant)
  HIPCHK(ctx->d_per_slice.reserve((size_t)ctx->ns * REDUCE_MAXK));
  // RC.cu:1555-1568: everything cleared once at allocation (v_PSF_sums is never cleared again)
  HIPCHK(hipMemsetAsync(ctx->d_slices, 0, fb, ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->d_weights, 0, fb, ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->d_simslices, 0, fb, ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->d_simweights, 0, fb, ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->d_psf_sums, 0, fb, ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->d_siminside, 0, np, ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->d_slice_inside, 0, ctx->ns, ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->d_voxcount, 0, np * sizeof(int), ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

int svr_fill_slices(svr_ctx *ctx, const float *sdata, const int *sizes_x, const int *sizes_y) {
  SVR_ENTER(ctx);
  if (!ctx || !sdata) return SVR_E_ARG;
  (void)sizes_x; (void)sizes_y;   // only used by the reference's dead code (RC.cu:3252-3253)
  NEED(ctx->np > 0, "initStorageVolumes first");
  HIPCHK(hipMemcpyAsync(ctx->d_slices, sdata, ctx->np * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  ctx->have_slices = true;
  invalidate(ctx, CH_SLICE_PIXELS);
  return build_list(ctx, false);
}

int svr_set_slice_dims(svr_ctx *ctx, const float *slice_dims, float quality_factor) {
  SVR_ENTER(ctx);
  if (!ctx || !slice_dims) return SVR_E_ARG;
  NEED(ctx->ns > 0, "initStorageVolumes first");
  ctx->slice_dims.assign(slice_dims, slice_dims + 3 * (size_t)ctx->ns);
  ctx->quality_factor = quality_factor;   // only sizes the (unused) finite-support dim, RC.cu:772-784
  ctx->have_dims = true;
  invalidate(ctx, CH_SLICE_GEOMETRY);
  return SVR_OK;
}

int svr_set_slice_matrices(svr_ctx *ctx, const float *T, const float *Tinv, const float *i2w_init,
                           const float *w2i_init, const float *i2w, const float *w2i,
                           const float recon_i2w[16], const float recon_w2i[16]) {
  SVR_ENTER(ctx);
  if (!ctx || !T || !Tinv || !i2w || !w2i || !recon_i2w || !recon_w2i) return SVR_E_ARG;
  (void)i2w_init; (void)w2i_init;   // registration-only in the reference (RC.cu:3486)
  NEED(ctx->ns > 0, "initStorageVolumes first");
  const size_t n = 16 * (size_t)ctx->ns;
  ctx->mT.assign(T, T + n);
  ctx->mTinv.assign(Tinv, Tinv + n);
  ctx->mI2W.assign(i2w, i2w + n);
  ctx->mW2I.assign(w2i, w2i + n);
  memcpy(ctx->reconI2W, recon_i2w, 16 * sizeof(float));
  memcpy(ctx->reconW2I, recon_w2i, 16 * sizeof(float));
  ctx->have_mats = true;
  invalidate(ctx, CH_SLICE_GEOMETRY);
  return SVR_OK;
}

int svr_generate_psf_volume(svr_ctx *ctx, const float *cpu_psf, const uint32_t psf_size[3],
                            const float slice_voxel_dim[3], const float psf_dim[3],
                            const float psf_i2w[16], const float psf_w2i[16], float quality_factor) {
  SVR_ENTER(ctx);
  if (!ctx || !psf_size || !psf_i2w) return SVR_E_ARG;
  (void)cpu_psf; (void)slice_voxel_dim; (void)psf_dim; (void)psf_w2i;
  // d_PSFI2W * ((PSFsize - 1) * 0.5f)   RC.cu:172
  float v[3] = {((float)psf_size[0] - 1) * 0.5f, ((float)psf_size[1] - 1) * 0.5f, ((float)psf_size[2] - 1) * 0.5f};
  matvec3_host(psf_i2w, v, ctx->psf_c0);
  invalidate(ctx, CH_TAPS);                                // the taps' residuals carry c0
  ctx->quality_factor = quality_factor;
  ctx->have_psf = true;
  return SVR_OK;
}

int svr_update_scale_vector(svr_ctx *ctx, const float *scales, const float *slice_weights) {
  SVR_ENTER(ctx);
  if (!ctx || !scales || !slice_weights) return SVR_E_ARG;
  NEED(ctx->ns > 0, "initStorageVolumes first");
  ctx->h_slice_weights.assign(slice_weights, slice_weights + ctx->ns);
  int r = upload_ns(ctx, ctx->d_scales, scales, ctx->mir_scales);
  if (r) return r;
  r = upload_ns(ctx, ctx->d_scales_host_copy, scales, ctx->mir_scales_copy);    // the device's copy of h_scales (below)
  if (r) return r;
  r = upload_ns(ctx, ctx->d_slice_weights, slice_weights, ctx->mir_slice_weights);
  if (r) return r;
  ctx->have_scales = true;
  return SVR_OK;
}

int svr_update_slice_weights(svr_ctx *ctx, const float *slice_weights) {
  SVR_ENTER(ctx);
  if (!ctx || !slice_weights) return SVR_E_ARG;
  NEED(ctx->have_scales, "UpdateScaleVector first");
  ctx->h_slice_weights.assign(slice_weights, slice_weights + ctx->ns);
  return upload_ns(ctx, ctx->d_slice_weights, slice_weights, ctx->mir_slice_weights);
}

int svr_update_reconstructed(svr_ctx *ctx, const uint32_t size[3], const float *data) {
  SVR_ENTER(ctx);
  if (!ctx || !size || !data) return SVR_E_ARG;
  NEED(ctx->nv > 0, "InitReconstructionVolume first");
  if ((size_t)size[0] * size[1] * size[2] != ctx->nv) return fail(ctx, SVR_E_ARG, "size mismatch");
  HIPCHK(hipMemcpyAsync(ctx->recon(), data, ctx->nv * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  invalidate(ctx, CH_VOLUME_VALUES);                       // (as svr_debug_set(SVR_BUF_RECONSTRUCTED): the caller's volume need not be zero outside the mask)
  return SVR_OK;
}

int svr_sync_cpu(svr_ctx *ctx, float *out) {
  SVR_ENTER(ctx);
  if (!ctx || !out) return SVR_E_ARG;
  NEED(ctx->nv > 0, "InitReconstructionVolume first");
  HIPCHK(hipMemcpyAsync(out, ctx->recon(), ctx->nv * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

// Reconstruction::updateStackSizes (RC.cuh:210): the sizes are stored; nothing in the reference reads them back
int svr_update_stack_sizes(svr_ctx *ctx, const uint32_t *sizes3, int n_stacks) {
  SVR_ENTER(ctx);
  if (!ctx || n_stacks < 0 || (n_stacks > 0 && !sizes3)) return SVR_E_ARG;
  ctx->stack_sizes.assign(sizes3, sizes3 + 3 * (size_t)n_stacks);
  return SVR_OK;
}

// Reconstruction::combineWeights (RC.cu:5091-5097): the bias path's accumulated volume weights (dev_volume_weights_) of device 0;
// zeros while no NormaliseBias has run (the reference's buffer is cleared at allocation, RC.cu:1214)
int svr_combine_weights(svr_ctx *ctx, float *out) {
  SVR_ENTER(ctx);
  if (!ctx || !out) return SVR_E_ARG;
  NEED(ctx->nv > 0, "InitReconstructionVolume first");
  if (!ctx->d_volume_weights) { memset(out, 0, ctx->nv * sizeof(float)); return SVR_OK; }
  HIPCHK(hipMemcpyAsync(out, ctx->d_volume_weights, ctx->nv * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

int svr_get_vol_weights(svr_ctx *ctx, float *out) {
  SVR_ENTER(ctx);
  if (!ctx || !out) return SVR_E_ARG;
  NEED(ctx->nv > 0, "InitReconstructionVolume first");
  HIPCHK(hipMemcpyAsync(out, ctx->volw(), ctx->nv * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

// ---- Gaussian reconstruction -----------------------------------------------------------
int svr_gaussian_reconstruction_local(svr_ctx *ctx) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  int r = ready(ctx);
  if (r) return r;
  const size_t fb = ctx->np * sizeof(float);
  // RC.cu:2401-2411.  PVR: ReconVolume::reset() clears only the volume and its weights
  // (R2/include/reconVolume.cuh:93-98); the patch buffers keep their values between outer iterations.
  if (!ctx->pvr) {
    HIPCHK(hipMemsetAsync(ctx->d_weights, 0, fb, ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->d_simweights, 0, fb, ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->d_simslices, 0, fb, ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->d_siminside, 0, ctx->np, ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->d_slice_inside, 0, ctx->ns, ctx->stream));
  }
  HIPCHK(hipMemsetAsync(ctx->d_voxcount, 0, ctx->np * sizeof(int), ctx->stream));
  ctx->recon_cur = ctx->d_recon_volw;      // recon | volw as one allocation again (the pair a sharded run all-reduces); the old volume is not read
  HIPCHK(hipMemsetAsync(ctx->d_recon_volw, 0, 2 * ctx->nv * sizeof(float), ctx->stream));
  const PassPath p1 = pass_path(ctx, PASS_GAUSS1), p2 = pass_path(ctx, PASS_GAUSS2);
  PsfArgs a = make_args(ctx);
  a.list = ctx->d_active;
  a.n = ctx->n_active;
  // one plan for both passes.  Both stream, or pass 2 stores what pass 1 evaluated too -- if its cell lists, built below, hold the geometry
  TablePlan tp = table_plan_for(ctx, PASS_GAUSS2, p2, true);
  TableUse use = TABLE_EVALUATE;
  if (tp.use != TABLE_STORE && (r = table_begin(ctx, tp, a, &use))) return r;
  ScopedTimer t(ctx, SVR_T_GAUSS);
  if (a.n && p1.family != FAM_PIXELS) {
    // pass 1 = the unit-based walk of the gather (sume, gate, v_PSF_sums, voxel-count flag), pass 2 = the scatter of the
    // back-projection with {recon|volw} as targets and unit voxel / slice weights
    HIPCHK(ctx->d_gauss_flag.reserve(ctx->np));
    HIPCHK(hipMemsetAsync(ctx->d_gauss_flag, 0, ctx->np, ctx->stream));
    // pass 1 keeps 4-pixel-wide tiles when the gather of the SR iterations chose 6 x 4 (measured: 6 x 4 costs pass 1 1.6 ms on P4)
    const int gtw = ctx->fwd_tw == 6 ? 4 : ctx->fwd_tw, gth = ctx->fwd_th;
    const int ftx = (int)((ctx->sx + gtw - 1) / gtw), fty = (int)((ctx->sy + gth - 1) / gth);
    const size_t max_tiles = std::max((size_t)ftx * fty, (size_t)ctx->tiles_x * ctx->tiles_y) * ctx->ns;
    HIPCHK(ctx->d_tiles_tmp.reserve(max_tiles));
    uint32_t n1 = 0, n2 = 0;
    a.flag = nullptr; a.flag_out = ctx->d_gauss_flag;
    CellState *gcs = nullptr;
    if (p1.family == FAM_CELLS && gather_stays_on_cells(p1, use) &&
        (r = cells_or_fallback(ctx, true, 2, "pass 1 of the Gaussian reconstruction left the cell path (the cell lists cannot hold this geometry): tile kernel, same bits", gcs))) return r;
    if (gcs) {
      if ((r = launch_cell_gauss1(ctx, *gcs, a))) return r;
    } else {
      HIPCHK(hipMemsetAsync(ctx->d_counter, 0, sizeof(uint32_t), ctx->stream));
      if ((r = build_tile_list(ctx, nullptr, nullptr, ftx, fty, gtw, gth, ctx->d_tiles_tmp, ctx->d_counter))) return r;
      HIPCHK(hipMemcpyAsync(&n1, ctx->d_counter, sizeof(n1), hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));
      if ((r = launch_unit_gather<true>(ctx, a, ctx->d_tiles_tmp, n1, ftx, fty, gtw, gth))) return r;
    }
    a.flag = ctx->d_gauss_flag;
    a.addon = ctx->recon(); a.cmap = ctx->volw();       // scatter targets of pass 2 (RC.cu:279-282)
    CellState *scs = nullptr;
    if (p2.family == FAM_CELLS && (r = cells_or_fallback(ctx, false, 0, SCATTER_LEFT_CELLS, scs))) return r;
    if (tp.use == TABLE_STORE) {
      // (coeff_lazy: pass 2 evaluates every unit the SR iterations will read -- it writes the table, and the SimulateSlices that follows streams it)
      if (!scs) tp = table_plan_for(ctx, PASS_GAUSS2, p2, false);
      if ((r = table_begin(ctx, tp, a, &use))) return r;
    }
    if (scs) {
      r = launch_cell_scatter(ctx, a, 1, ctx->recon(), ctx->volw(), use == TABLE_STORE);
    } else {
      // the tiles of the pixels that passed the gate (the tiled scatters only)
      HIPCHK(hipMemsetAsync(ctx->d_counter, 0, sizeof(uint32_t), ctx->stream));
      if ((r = build_tile_list(ctx, nullptr, ctx->d_gauss_flag, ctx->tiles_x, ctx->tiles_y, ctx->tile_w, ctx->tile_h, ctx->d_tiles_tmp, ctx->d_counter))) return r;
      HIPCHK(hipMemcpyAsync(&n2, ctx->d_counter, sizeof(n2), hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));
      r = launch_scatter(ctx, p2.scatter_level, a, ctx->d_tiles_tmp, n2, MODE_GAUSS2);
    }
    if (r) return r;
  } else if (a.n) {
    if ((r = launch_pixels(ctx, a, ctx->pvr ? pvr_kernel<MODE_GAUSS> : psf_kernel<MODE_GAUSS>, "psf_kernel / pvr_kernel<GAUSS>"))) return r;
  }
  t.stop();
  invalidate(ctx, CH_PSF_SUMS);
  table_end(ctx, use);                                     // (written by pass 2 for the new v_PSF_sums)
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

int svr_gaussian_reconstruction_finish(svr_ctx *ctx, int *voxel_num) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  NEED(ctx->nv > 0 && ctx->have_slices, "volume / slices not set");
  hipLaunchKernelGGL(k_equalize, dim3(nblk(ctx->nv)), dim3(256), 0, ctx->stream, ctx->recon(), ctx->volw(), ctx->nv);
  KCHK("k_equalize");
  unsigned long long cnt = 0;
  unsigned long long *d_cnt = reinterpret_cast<unsigned long long *>(ctx->d_out.get());
  HIPCHK(hipMemsetAsync(d_cnt, 0, sizeof(cnt), ctx->stream));
  hipLaunchKernelGGL(k_count_positive, dim3(std::min(nblk(ctx->np), 2048u)), dim3(256), 0, ctx->stream, ctx->d_voxcount, ctx->np, d_cnt);
  KCHK("k_count_positive");
  HIPCHK(hipMemcpyAsync(&cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (voxel_num) *voxel_num = (int)cnt;
  return build_list(ctx, true);
}

int svr_gaussian_reconstruction(svr_ctx *ctx, int *voxel_num) {
  SVR_ENTER(ctx);
  int r = svr_gaussian_reconstruction_local(ctx);
  if (r) return r;
  return svr_gaussian_reconstruction_finish(ctx, voxel_num);
}

// ---- forward projection ----------------------------------------------------------------
int svr_simulate_slices(svr_ctx *ctx, uint8_t *slice_inside) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  int r = ready(ctx);
  if (r) return r;
  r = ensure_psf_list(ctx);
  if (r) return r;
  const PassPath p = pass_path(ctx, PASS_FORWARD);
  // Round 6 (coeff_lazy): with the table wanted and not there, THIS pass writes it -- it evaluates every tap of every PSF pixel anyway
  // (fwd_cell_kernel<.., 3>); needs the cell gather.  Otherwise k_coeff_build, as before.
  CellState *gcs = nullptr;
  TablePlan tp = table_plan_for(ctx, PASS_FORWARD, p, true);
  if (tp.use == TABLE_STORE) {
    if ((r = cell_prepare_gather(ctx, gcs))) return r;
    if (!gcs->usable) tp = table_plan_for(ctx, PASS_FORWARD, p, false);
  }
  PsfArgs a = make_args(ctx);
  a.list = ctx->d_psf_list;
  a.n = ctx->n_psf;
  TableUse use;
  if ((r = table_begin(ctx, tp, a, &use))) return r;
  const bool store = use == TABLE_STORE;
  if (a.n && p.family != FAM_PIXELS && (r = pack_volm(ctx, a, ctx->recon()))) return r;
  gcs = nullptr;
  if (a.n && p.family == FAM_CELLS && gather_stays_on_cells(p, use) &&
      (r = cells_or_fallback(ctx, true, 1, "the gather left the cell path (the cell lists cannot hold this geometry): tile kernel, same bits", gcs))) return r;
  if (a.n && p.family != FAM_PIXELS && !gcs && !ctx->fwd_tile_user) {
    int w, h;
    tile_shape_rule(ctx, a.coeff != nullptr, w, h);
    if (w != ctx->fwd_tw || h != ctx->fwd_th) {
      ctx->fwd_tw = w; ctx->fwd_th = h; invalidate(ctx, CH_TILE_SHAPE);
      r = ensure_psf_list(ctx);
      if (r) return r;
      a.list = ctx->d_psf_list; a.n = ctx->n_psf;
    }
  }
  ScopedTimer t(ctx, SVR_T_FORWARD);
  if (store) t.also(SVR_T_FORWARD_STORE); else if (a.coeff) t.also(SVR_T_FORWARD_TABLE);
  if (gcs) {
    if ((r = launch_cell_gather(ctx, *gcs, a, store))) return r;
  } else if (a.n && p.family != FAM_PIXELS) {
    if ((r = ensure_tiles_fwd(ctx))) return r;
    if ((r = launch_unit_gather<false>(ctx, a, ctx->d_tiles_fwd, ctx->n_tiles_fwd, ctx->fwd_tiles_x, ctx->fwd_tiles_y, ctx->fwd_tw, ctx->fwd_th))) return r;
  } else if (a.n) {
    if ((r = launch_pixels(ctx, a, ctx->pvr ? pvr_kernel<MODE_FWD> : psf_kernel<MODE_FWD>, "psf_kernel / pvr_kernel<FWD>"))) return r;
  }
  t.stop();
  table_end(ctx, use);
  ctx->have_sim = true;
  if (!gcs) {                                              // (the cell gather's finish raises the slices' flags itself)
    hipLaunchKernelGGL(k_slice_inside, dim3(ctx->ns), dim3(256), 0, ctx->stream, ctx->d_siminside,
                       (int)(ctx->sx * ctx->sy), ctx->d_slice_inside);
    KCHK("k_slice_inside");
  }
  // slice_inside == NULL: the flags stay on the device (svr_get_slice_inside, svr_mstep_estep) and the call does not wait
  if (slice_inside) {
    if ((r = down_queue(ctx, slice_inside, ctx->d_slice_inside, ctx->ns))) return r;
    return down_flush(ctx);
  }
  return SVR_OK;
}

int svr_get_slice_inside(svr_ctx *ctx, uint8_t *slice_inside) {
  SVR_ENTER(ctx);
  if (!ctx || !slice_inside) return SVR_E_ARG;
  NEED(ctx->have_slices, "slices not filled");
  int r = down_queue(ctx, slice_inside, ctx->d_slice_inside, ctx->ns);
  if (r) return r;
  return down_flush(ctx);
}

// ---- EM --------------------------------------------------------------------------------
int svr_initialize_em_values(svr_ctx *ctx) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  NEED(ctx->have_slices, "slices not filled");
  hipLaunchKernelGGL(k_init_em, dim3(nblk(ctx->np)), dim3(256), 0, ctx->stream, ctx->d_slices, ctx->d_weights, ctx->np, ctx->pvr);
  KCHK("k_init_em");
  ctx->have_em = true;
  if (!ctx->disable_bias) {                              // RC.cu:3305-3309
    int r = ensure_bias_buffers(ctx);
    if (r) return r;
    HIPCHK(hipMemsetAsync(ctx->d_bias, 0, ctx->np * sizeof(float), ctx->stream));
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

int svr_robust_statistics_sums(svr_ctx *ctx, double out2[2]) {
  SVR_ENTER(ctx);
  if (!ctx || !out2) return SVR_E_ARG;
  NEED(ctx->have_slices, "slices not filled");
  hipLaunchKernelGGL(k_robust, dim3(ctx->chunks, ctx->ns), dim3(256), 0, ctx->stream, ctx->d_slices, ctx->d_siminside,
                     ctx->d_simslices, ctx->d_simweights, (int)(ctx->sx * ctx->sy), ctx->d_partial);
  KCHK("k_robust");
  int r = reduce_partials(ctx, 2, 0, 0, true);
  if (r) return r;
  HIPCHK(hipMemcpyAsync(out2, ctx->d_out, 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

int svr_initialize_robust_statistics(svr_ctx *ctx, float *sigma) {
  SVR_ENTER(ctx);
  if (!ctx || !sigma) return SVR_E_ARG;
  double s2[2];
  int r = svr_robust_statistics_sums(ctx, s2);
  if (r) return r;
  *sigma = (float)s2[0] / (float)s2[1];   // RC.cu:2301-2305
  return SVR_OK;
}

namespace {
// the E-step's kernels; em = NULL: (m, sigma, mix) by value, else {sigma, mix, m} read from the device (svr_mstep_estep)
int launch_estep(svr_ctx *ctx, float m, float sigma, float mix, const float *em) {
  ScopedTimer t(ctx, SVR_T_ESTEP);
  hipLaunchKernelGGL(k_estep, dim3(ctx->chunks, ctx->ns), dim3(256), 0, ctx->stream, ctx->d_slices, ctx->d_simslices,
                     ctx->d_simweights, ctx->d_scales, ctx->disable_bias ? (const float *)nullptr : ctx->d_bias, m, sigma,
                     mix, (int)(ctx->sx * ctx->sy), ctx->d_weights, ctx->d_partial, ctx->pvr, em);
  KCHK("k_estep");
  ctx->have_em = true;
  hipLaunchKernelGGL(k_potential_finish, dim3(nblk(ctx->ns, 64)), dim3(64), 0, ctx->stream, ctx->d_partial,
                     (int)ctx->ns, ctx->chunks, ctx->d_tmp_ns);
  KCHK("k_potential_finish");
  t.stop();
  return SVR_OK;
}
// the M-step's sums -> d_out[5]
int launch_mstep(svr_ctx *ctx) {
  // the reference fills its per-pixel scale buffer from the HOST copy h_scales (RC.cu:3091-3094): d_scales_host_copy
  ScopedTimer t(ctx, SVR_T_MSTEP);
  hipLaunchKernelGGL(k_mstep, dim3(ctx->chunks, ctx->ns), dim3(256), 0, ctx->stream, ctx->d_slices, ctx->d_weights,
                     ctx->d_simslices, ctx->d_simweights, ctx->d_scales_host_copy,
                     ctx->disable_bias ? (const float *)nullptr : ctx->d_bias, (int)(ctx->sx * ctx->sy), ctx->d_partial);
  KCHK("k_mstep");
  int r = reduce_partials(ctx, 5, 1 << 3, 1 << 4, true);
  if (r) return r;
  t.stop();
  return SVR_OK;
}
// Reconstruction::MStep's host part RC.cu:3016-3071 (patch-based: patchBasedRobustStatistics_gpu.cu:570-640, no FLT_MAX /
// FLT_MIN clamps), the same float operations on either side
__host__ __device__ inline void mstep_scalars(const double s5[5], int iter, float step, int pvr, float &sigma_io, float &mix_io, float &m_out) {
  const float sigma = (float)s5[0], mix = (float)s5[1], num = (float)s5[2];
  float min_ = (float)s5[3], max_ = (float)s5[4];
  if (!pvr) {
    min_ = min_ < 3.402823466e+38f ? min_ : 3.402823466e+38f;       // std::min(FLT_MAX, .), std::max(FLT_MIN, .)
    max_ = 1.175494351e-38f < max_ ? max_ : 1.175494351e-38f;
  }
  if (mix > 0) sigma_io = sigma / mix;
  if (sigma_io < step * step / 6.28f) sigma_io = step * step / 6.28f;
  if (iter > 1) mix_io = mix / num;
  m_out = 1.0f / (max_ - min_);
}
__global__ void k_mstep_scalars(const double *s5, int iter, float step, int pvr, float sigma, float mix, float *em) {
  float m = 0.0f;
  mstep_scalars(s5, iter, step, pvr, sigma, mix, m);
  em[0] = sigma; em[1] = mix; em[2] = m;
}
// ... of a sharded run: all[world][8] = every rank's five sums (an all-gather on the device), added up in rank order exactly like
// the hosts do after their exchange (csrc/svr_unit_em.h UnitState::mstep_now) -- the same bits on every rank
__global__ void k_mstep_scalars_ranks(const double *all, int world, int iter, float step, int pvr, float sigma, float mix, float *em) {
  double s5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int r = 0; r < world; ++r) {
    for (int k = 0; k < 3; ++k) s5[k] += all[8 * r + k];
    s5[3] = r ? fmin(s5[3], all[8 * r + 3]) : all[3];
    s5[4] = r ? fmax(s5[4], all[8 * r + 4]) : all[4];
  }
  float m = 0.0f;
  mstep_scalars(s5, iter, step, pvr, sigma, mix, m);
  em[0] = sigma; em[1] = mix; em[2] = m;
}
}  // namespace

int svr_estep(svr_ctx *ctx, float m, float sigma, float mix, float *slice_potential) {
  SVR_ENTER(ctx);
  if (!ctx || !slice_potential) return SVR_E_ARG;
  NEED(ctx->have_slices && ctx->have_scales, "slices / scales not set");
  int r = launch_estep(ctx, m, sigma, mix, nullptr);
  if (r) return r;
  if ((r = down_queue(ctx, slice_potential, ctx->d_tmp_ns, ctx->ns * sizeof(float)))) return r;
  return down_flush(ctx);
}

int svr_mstep_sums(svr_ctx *ctx, double out5[5]) {
  SVR_ENTER(ctx);
  if (!ctx || !out5) return SVR_E_ARG;
  NEED(ctx->have_slices && ctx->have_scales, "slices / scales not set");
  int r = launch_mstep(ctx);
  if (r) return r;
  if ((r = down_queue(ctx, out5, ctx->d_out, 5 * sizeof(double)))) return r;
  return down_flush(ctx);
}

// svr_mstep_sums plus what deferred calls left on the device (each may be NULL), in the same wait: for a sharded host, which needs
// the sums on the host for its exchange anyway
int svr_mstep_sums_fetch(svr_ctx *ctx, double out5[5], float *scale_vec, uint8_t *slice_inside) {
  SVR_ENTER(ctx);
  if (!ctx || !out5) return SVR_E_ARG;
  NEED(ctx->have_slices && ctx->have_scales, "slices / scales not set");
  int r = launch_mstep(ctx);
  if (r) return r;
  if ((r = down_queue(ctx, out5, ctx->d_out, 5 * sizeof(double)))) return r;
  if (scale_vec && (r = down_queue(ctx, scale_vec, ctx->d_scales_host_copy, ctx->ns * sizeof(float)))) return r;
  if (slice_inside && (r = down_queue(ctx, slice_inside, ctx->d_slice_inside, ctx->ns))) return r;
  if ((r = down_flush(ctx))) return r;
  if (scale_vec) ctx->mir_scales_copy.assign(scale_vec, scale_vec + ctx->ns);
  return SVR_OK;
}

int svr_mstep(svr_ctx *ctx, int iter, float step, float *sigma_io, float *mix_io, float *m_out) {
  SVR_ENTER(ctx);
  if (!ctx || !sigma_io || !mix_io || !m_out) return SVR_E_ARG;
  double s5[5];
  int r = svr_mstep_sums(ctx, s5);
  if (r) return r;
  if (!((float)s5[1] > 0)) fprintf(stderr, "Something went wrong: sigma= %f mix= %f\n", (float)s5[0], (float)s5[1]);
  mstep_scalars(s5, iter, step, 0, *sigma_io, *mix_io, *m_out);
  return SVR_OK;
}

// MStep followed by EStep (reconstruction.cc:1093-1108, irtkPatchBasedReconstruction.cpp:540-545) with ONE wait for the
// device: the M-step's scalars are worked out by a one-thread kernel with the host's float operations and read by the
// E-step's kernel from device memory.  em3 = {sigma, mix, m} in/out.  scale_vec / slice_inside (each may be NULL): what
// a deferred svr_calculate_scale_vector(ctx, NULL) / svr_simulate_slices(ctx, NULL) left on the device, in the same wait.
int svr_mstep_estep(svr_ctx *ctx, int iter, float step, float em3[3], float *slice_potential, float *scale_vec, uint8_t *slice_inside) {
  SVR_ENTER(ctx);
  if (!ctx || !em3 || !slice_potential) return SVR_E_ARG;
  NEED(ctx->have_slices && ctx->have_scales, "slices / scales not set");
  HIPCHK(ctx->d_em.reserve(4));
  int r = launch_mstep(ctx);
  if (r) return r;
  hipLaunchKernelGGL(k_mstep_scalars, dim3(1), dim3(1), 0, ctx->stream, ctx->d_out, iter, step, ctx->pvr ? 1 : 0, em3[0], em3[1], ctx->d_em);
  KCHK("k_mstep_scalars");
  if ((r = launch_estep(ctx, 0.0f, 0.0f, 0.0f, ctx->d_em))) return r;
  if ((r = down_queue(ctx, slice_potential, ctx->d_tmp_ns, ctx->ns * sizeof(float)))) return r;
  if ((r = down_queue(ctx, em3, ctx->d_em, 3 * sizeof(float)))) return r;
  if (scale_vec && (r = down_queue(ctx, scale_vec, ctx->d_scales_host_copy, ctx->ns * sizeof(float)))) return r;
  if (slice_inside && (r = down_queue(ctx, slice_inside, ctx->d_slice_inside, ctx->ns))) return r;
  if ((r = down_flush(ctx))) return r;
  if (scale_vec) ctx->mir_scales_copy.assign(scale_vec, scale_vec + ctx->ns);
  return SVR_OK;
}

// The same for a SHARDED run without a wait in between: svr_mstep_partial leaves this rank's five sums in *send (8 doubles = 16
// floats, device memory) and names the buffer the launcher's all-gather fills (*recv: world x 8 doubles); svr_mstep_estep_ranks
// adds the ranks' sums up on the device in rank order, works the scalars out there, runs the E-step on them and fetches this rank's
// potentials, the scalars and the deferred vectors in ONE wait.  The host's exchange of the M-step's sums is gone.
int svr_mstep_partial(svr_ctx *ctx, int world, void **send, void **recv) {
  SVR_ENTER(ctx);
  if (!ctx || !send || !recv || world < 1) return SVR_E_ARG;
  NEED(ctx->have_slices && ctx->have_scales, "slices / scales not set");
  HIPCHK(ctx->d_em_all.reserve((size_t)world * 8));
  int r = launch_mstep(ctx);
  if (r) return r;
  *send = ctx->d_out;
  *recv = ctx->d_em_all;
  return SVR_OK;
}
int svr_mstep_estep_ranks(svr_ctx *ctx, int world, int iter, float step, float em3[3], float *slice_potential, float *scale_vec, uint8_t *slice_inside) {
  SVR_ENTER(ctx);
  if (!ctx || !em3 || !slice_potential || world < 1) return SVR_E_ARG;
  NEED(ctx->have_slices && ctx->have_scales && (size_t)world * 8 <= ctx->d_em_all.capacity(), "svr_mstep_partial first");
  HIPCHK(ctx->d_em.reserve(4));
  hipLaunchKernelGGL(k_mstep_scalars_ranks, dim3(1), dim3(1), 0, ctx->stream, ctx->d_em_all, world, iter, step, ctx->pvr ? 1 : 0, em3[0], em3[1], ctx->d_em);
  KCHK("k_mstep_scalars_ranks");
  int r;
  if ((r = launch_estep(ctx, 0.0f, 0.0f, 0.0f, ctx->d_em))) return r;
  if ((r = down_queue(ctx, slice_potential, ctx->d_tmp_ns, ctx->ns * sizeof(float)))) return r;
  if ((r = down_queue(ctx, em3, ctx->d_em, 3 * sizeof(float)))) return r;
  if (scale_vec && (r = down_queue(ctx, scale_vec, ctx->d_scales_host_copy, ctx->ns * sizeof(float)))) return r;
  if (slice_inside && (r = down_queue(ctx, slice_inside, ctx->d_slice_inside, ctx->ns))) return r;
  if ((r = down_flush(ctx))) return r;
  if (scale_vec) ctx->mir_scales_copy.assign(scale_vec, scale_vec + ctx->ns);
  return SVR_OK;
}

int svr_calculate_scale_vector(svr_ctx *ctx, float *scale_vec) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  NEED(ctx->have_slices && ctx->have_scales, "slices / scales not set");
  ScopedTimer t(ctx, SVR_T_SCALE);
  hipLaunchKernelGGL(k_scale, dim3(ctx->chunks, ctx->ns), dim3(256), 0, ctx->stream, ctx->d_slices, ctx->d_weights,
                     ctx->d_simslices, ctx->d_simweights, ctx->disable_bias ? (const float *)nullptr : ctx->d_bias,
                     (int)(ctx->sx * ctx->sy), ctx->d_partial);
  KCHK("k_scale");
  int r;
  hipLaunchKernelGGL(k_scale_finish, dim3(nblk(ctx->ns, 64)), dim3(64), 0, ctx->stream, ctx->d_partial, (int)ctx->ns, ctx->chunks,
                     ctx->d_tmp_ns, ctx->d_scales, ctx->d_scales_host_copy);
  KCHK("k_scale_finish");
  t.stop();
  // Reference quirk, reproduced: CalculateScaleVectorOnX uploads h_scales -- still the PREVIOUS
  // scale vector -- to the device (RC.cu:3238) and only afterwards h_scales = scale_vec
  // (RC.cu:3195).  The E-step / back-projection kernels therefore see scales that lag one call
  // behind; the M-step reads h_scales (RC.cu:3093) and sees the new ones.  h_scales is d_scales_host_copy here: both
  // moves are device-to-device, and with scale_vec == NULL (svr_get_scale_vector / svr_mstep_estep fetch it later) the
  // call does not wait for the device.  (Both moves happen in k_scale_finish.)
  ctx->mir_scales = ctx->mir_scales_copy;          // (empty = unknown: the next upload is not skipped)
  ctx->mir_scales_copy.clear();
  if (scale_vec) {
    if ((r = down_queue(ctx, scale_vec, ctx->d_scales_host_copy, ctx->ns * sizeof(float)))) return r;
    if ((r = down_flush(ctx))) return r;
    ctx->mir_scales_copy.assign(scale_vec, scale_vec + ctx->ns);
  }
  return SVR_OK;
}

int svr_get_scale_vector(svr_ctx *ctx, float *scale_vec) {
  SVR_ENTER(ctx);
  if (!ctx || !scale_vec) return SVR_E_ARG;
  NEED(ctx->have_slices && ctx->have_scales, "slices / scales not set");
  int r = down_queue(ctx, scale_vec, ctx->d_scales_host_copy, ctx->ns * sizeof(float));
  if (r) return r;
  if ((r = down_flush(ctx))) return r;
  ctx->mir_scales_copy.assign(scale_vec, scale_vec + ctx->ns);
  return SVR_OK;
}

// the scale vector last calculated becomes the one the kernels see (the patch-based loop's copyToScales: no lag,
// patchBasedRobustStatistics_gpu.cu:672-745) -- svr_update_scale_vector(scale_vec, unchanged weights) without the host
int svr_adopt_scale_vector(svr_ctx *ctx) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  NEED(ctx->have_slices && ctx->have_scales, "slices / scales not set");
  HIPCHK(hipMemcpyAsync(ctx->d_scales, ctx->d_scales_host_copy, ctx->ns * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
  ctx->mir_scales = ctx->mir_scales_copy;
  return SVR_OK;
}

// ---- super-resolution ------------------------------------------------------------------
int svr_superresolution_backproject(svr_ctx *ctx, const float *slice_weight) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  int r = ready(ctx);
  if (r) return r;
  if (slice_weight) {
    r = svr_update_slice_weights(ctx, slice_weight);   // RC.cu:2123
    if (r) return r;
  }
  const PassPath p = pass_path(ctx, PASS_BACK);
  if (p.family == FAM_TILES && p.scatter_level >= 3 && !ctx->tile_user && (ctx->tile_w != 6 || ctx->tile_h != 4)) {
    // the tiled scatters (back_mode 3 / 4: fallbacks of the cell scatter, and what a caller names) without trials: 6 x 4 pixels with
    // the 2096-voxel box -- the trials' pick or within 2 % of it on P4 (4.97 ms against 4.96-5.08) and S8 (6 x 5 / 2096: 50.5 against 52.2)
    if ((r = set_scatter_tile(ctx, 6, 4))) return r;
  }
  r = ensure_psf_list(ctx);
  if (r) return r;
  PsfArgs a = make_args(ctx);
  a.list = ctx->d_psf_list;
  a.n = ctx->n_psf;
  // (coeff_lazy: a scatter that finds no table evaluates -- and, on the cell path, writes it: whichever PSF pass comes first after a new geometry does)
  TablePlan tp = table_plan_for(ctx, PASS_BACK, p, true);
  TableUse use = TABLE_EVALUATE;
  if (tp.use != TABLE_STORE && (r = table_begin(ctx, tp, a, &use))) return r;
  ctx->prep_pending = false;
  ctx->cmap_from_scatter = true;
  CellState *cs = nullptr;
  if (a.n && p.family == FAM_CELLS && (r = cells_or_fallback(ctx, false, 0, SCATTER_LEFT_CELLS, cs))) return r;
  if (tp.use == TABLE_STORE) {                             // (the cell lists have spoken)
    if (!cs) tp = table_plan_for(ctx, PASS_BACK, p, false);
    if ((r = table_begin(ctx, tp, a, &use))) return r;
  }
  const bool store = use == TABLE_STORE;
  ScopedTimer t(ctx, SVR_T_BACKPROJECT);
  if (store) t.also(SVR_T_BACKPROJECT_STORE); else if (a.coeff) t.also(SVR_T_BACKPROJECT_TABLE);
  // RC.cu:2202-2203 -- not needed where the cell scatter runs: its combine writes EVERY voxel of addon | cmap (0 outside the mask)
  if (!cs) HIPCHK(hipMemsetAsync(ctx->d_addon_cmap, 0, 2 * ctx->nv * sizeof(float), ctx->stream));
  if (cs) {
    if ((r = launch_cell_scatter(ctx, a, 0, ctx->addon(), ctx->cmap(), store))) return r;
  } else if (a.n && p.family != FAM_PIXELS) {
    if ((r = ensure_tiles_back(ctx))) return r;
    if ((r = launch_scatter(ctx, p.scatter_level, a, ctx->d_tiles, ctx->n_tiles, MODE_BACK))) return r;
  } else if (a.n) {
    if ((r = launch_pixels(ctx, a, ctx->pvr ? pvr_kernel<MODE_BACK> : psf_kernel<MODE_BACK>, "psf_kernel / pvr_kernel<BACK>"))) return r;
  }
  t.stop();
  table_end(ctx, use);
  if (!ctx->sr_no_wait) HIPCHK(hipStreamSynchronize(ctx->stream));   // (svr_superresolution: the update follows on the same stream)
  return SVR_OK;
}

// (double)r < (double)min * 0.9 and (double)r > (double)max * 1.1 (RC.cu:1964-1967) for a float r, as float comparisons
static void regul_thresholds(float min_i, float max_i, RegulArgs &ra) {
  const double dlo = (double)min_i * 0.9, dhi = (double)max_i * 1.1;
  ra.val_lo = (float)dlo;
  ra.val_hi = (float)dhi;
  ra.thr_lo = (double)ra.val_lo >= dlo ? ra.val_lo : nextafterf(ra.val_lo, INFINITY);
  ra.thr_hi = (double)ra.val_hi <= dhi ? ra.val_hi : nextafterf(ra.val_hi, -INFINITY);
}

// Prep's own changes of addon / cmap, left out by k_regul_fused, for whoever reads the two buffers
static int regul_settle(svr_ctx *ctx) {
  if (!ctx->prep_pending) return SVR_OK;
  ctx->prep_pending = false;
  hipLaunchKernelGGL(k_regul_settle, dim3(nblk(ctx->nv)), dim3(256), 0, ctx->stream, ctx->addon(), ctx->cmap(), ctx->nv);
  KCHK("k_regul_settle");
  return SVR_OK;
}

static int regul_fused_launch(svr_ctx *ctx, RegulArgs &ra, const float *recon, float *out, int adaptive, float alpha, float delta, float lambda, int z_lo,
                              int z_hi);
static int superresolution_update_planes(svr_ctx *ctx, int adaptive, float alpha, float min_intensity, float max_intensity, float delta,
                                         float lambda, int z_lo, int z_hi) {
  if (ctx->reg_mode == 0) {
    HIPCHK(ctx->d_snap.reserve(ctx->nv));
    if (z_lo != 0 || z_hi != (int)ctx->vz) return fail(ctx, SVR_E_ARG, "reg_mode 0 updates whole volumes only");
    float *out = ctx->recon_cur == ctx->d_recon_volw ? ctx->d_recon_new : ctx->d_recon_volw;
    hipLaunchKernelGGL(k_reg_prep, dim3(nblk(ctx->nv)), dim3(256), 0, ctx->stream, adaptive, alpha, ctx->recon(),
                       ctx->addon(), ctx->cmap(), min_intensity, max_intensity, ctx->d_snap, ctx->nv);
    KCHK("k_reg_prep");
    hipLaunchKernelGGL(k_regularize, dim3((ctx->vx + 63) / 64, (ctx->vy + 3) / 4, ctx->vz), dim3(256), 0, ctx->stream,
                       (int)ctx->vx, (int)ctx->vy, (int)ctx->vz, delta, alpha, lambda, ctx->d_snap, ctx->recon(),
                       ctx->cmap(), out);
    KCHK("k_regularize");
    return SVR_OK;
  }
  RegulArgs ra;
  ra.guide = nullptr;
  regul_thresholds(min_intensity, max_intensity, ra);
  return regul_fused_launch(ctx, ra, ctx->recon(), ctx->recon_cur == ctx->d_recon_volw ? ctx->d_recon_new : ctx->d_recon_volw, adaptive, alpha, delta, lambda,
                            z_lo, z_hi);
}

// k_regul_fused on planes [z_lo, z_hi) of `recon` with the context's addon | cmap -> out; ra brings the clamp (thr / val) and the guide (NULL: the
// unguided kernels; else gkap1..3 and omega with it), everything else is set here
static int regul_fused_launch(svr_ctx *ctx, RegulArgs &ra, const float *recon, float *out, int adaptive, float alpha, float delta, float lambda, int z_lo,
                              int z_hi) {
  ra.recon = recon; ra.addon = ctx->addon(); ra.cmap = ctx->cmap();
  ra.out = out;
  ra.vx = (int)ctx->vx; ra.vy = (int)ctx->vy; ra.vz = (int)ctx->vz;
  ra.z_lo = z_lo; ra.z_hi = z_hi;
  // tile of a workgroup (option reg_tile).  Measured on one MI355X (tools/exp_regul_tile.py; 64 x 8 / 32 x 16 / 32 x 8): P4 19.4 / 20.2 /
  // 18.2 us, S8 (273^3) 189 / 177 / 164 us, PVR8spx (400 x 400 x 320) 429 / 394 / 395 us: the small tile wastes the fewest lanes
  // beyond the volume's extent and keeps more workgroups per CU between its barriers
  static const int shapes[3][2] = {{64, 8}, {32, 16}, {32, 8}};
  const int pick = ctx->reg_tile < 0 ? 2 : ctx->reg_tile;
  const int TW = shapes[pick][0], TH = shapes[pick][1];
  const int tiles = (int)((ctx->vx + TW - 1) / TW * ((ctx->vy + TH - 1) / TH));
  const int nz = z_hi - z_lo;
  const int want = std::max(1, (2048 * 512 / (TW * TH) + tiles - 1) / tiles);   // chunks along z for >= 2048 workgroups of 512 lanes
  ra.zc = std::min(32, std::max(4, (nz + want - 1) / want));
  const int chunks = (nz + ra.zc - 1) / ra.zc;
  ctx->last_reg_zc = ra.zc; ctx->last_reg_chunks = chunks;
  for (int k = 0; k < 3; ++k) { ra.blo[k] = 0; ra.bhi[k] = -1; }
  if (ctx->mbox_valid && ctx->cmap_from_scatter) {
    const int dims[3] = {ra.vx, ra.vy, ra.vz};
    for (int k = 0; k < 3; ++k) { ra.blo[k] = std::max(0, ctx->mbox_lo[k] - 1); ra.bhi[k] = std::min(dims[k] - 1, ctx->mbox_hi[k] + 1); }
  }
  ra.alpha = alpha;
  ra.k = alpha * lambda / (delta * delta);                                // RC.cu:2107 (float)
  const double d2 = (double)delta * (double)delta;
  ra.kap1 = (float)(1.0 / d2); ra.kap2 = (float)(0.5 / d2); ra.kap3 = (float)((double)(1.0f / 3.0f) / d2);
  if (nz > 0) {
    const dim3 grid((ctx->vx + TW - 1) / TW, (ctx->vy + TH - 1) / TH, chunks);
    const dim3 block(TW * TH);
#define REGUL_LAUNCH(AD, W, H)                                                                               \
  do {                                                                                                       \
    if (ra.guide) hipLaunchKernelGGL((k_regul_fused<AD, W, H, true>), grid, block, 0, ctx->stream, ra);      \
    else hipLaunchKernelGGL((k_regul_fused<AD, W, H>), grid, block, 0, ctx->stream, ra);                     \
  } while (0)
    if (adaptive) { if (pick == 0) REGUL_LAUNCH(true, 64, 8); else if (pick == 1) REGUL_LAUNCH(true, 32, 16); else REGUL_LAUNCH(true, 32, 8); }
    else { if (pick == 0) REGUL_LAUNCH(false, 64, 8); else if (pick == 1) REGUL_LAUNCH(false, 32, 16); else REGUL_LAUNCH(false, 32, 8); }
#undef REGUL_LAUNCH
    KCHK("k_regul_fused");
  }
  if (!adaptive) ctx->prep_pending = true;
  return SVR_OK;
}

int svr_superresolution_update(svr_ctx *ctx, int adaptive, float alpha, float min_intensity,
                               float max_intensity, float delta, float lambda) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  NEED(ctx->nv > 0, "volume not set");
  if (alpha * lambda / (delta * delta) > 0.068)   // RC.cu:2124-2127
    fprintf(stderr, "Warning: regularization might not have smoothing effect! Ensure that alpha*lambda/delta^2 is below 0.068.");
  ScopedTimer t(ctx, SVR_T_REGULARIZE);
  int r = superresolution_update_planes(ctx, adaptive, alpha, min_intensity, max_intensity, delta, lambda, 0, (int)ctx->vz);
  if (r) return r;
  ctx->recon_cur = ctx->recon_cur == ctx->d_recon_volw ? ctx->d_recon_new : ctx->d_recon_volw;   // the update wrote the other buffer
  // a whole-volume update carries whatever the old volume held outside the dilated mask over into the buffer it wrote: the slab update
  // (svr_slab.inc), which only writes inside it, must clear that buffer before it uses it next
  invalidate(ctx, CH_VOLUME_VALUES);
  t.stop();
  if (!ctx->sr_no_wait) HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

// ---- the volume update of a sharded run: reduce-scatter -> the rank's z-slab -> all-gather (svr_slab.inc) ----------------
int svr_slab_plan(svr_ctx *ctx, int world, int rank, size_t *rs_floats_per_rank, size_t *ag_floats_per_rank) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  const int r = slab_plan(ctx, world, rank);
  if (r) return r;
  if (rs_floats_per_rank) *rs_floats_per_rank = (size_t)2 * ctx->slab->rs_chunk;
  if (ag_floats_per_rank) *ag_floats_per_rank = ctx->slab->ag_chunk;
  return SVR_OK;
}
int svr_slab_rs_pack(svr_ctx *ctx, void **send, void **recv) {
  SVR_ENTER(ctx);
  if (!ctx || !send || !recv) return SVR_E_ARG;
  NEED(ctx->slab && ctx->slab->valid && ctx->slab->world > 0, "svr_slab_plan first");
  NEED(ctx->cmap_from_scatter, "svr_slab_rs_pack: addon | cmap must come from svr_superresolution_backproject");
  SlabPlan &p = *ctx->slab;
  hipLaunchKernelGGL(k_slab_rs_pack, dim3(nblk((size_t)p.world * 2 * p.rs_chunk)), dim3(256), 0, ctx->stream, ctx->addon(), ctx->cmap(), p.d_midx, p.d_tab,
                     p.world, p.rs_chunk, p.d_send);
  KCHK("k_slab_rs_pack");
  *send = p.d_send; *recv = p.d_recv;
  return SVR_OK;
}
int svr_slab_update(svr_ctx *ctx, int adaptive, float alpha, float min_intensity, float max_intensity, float delta, float lambda,
                    void **send, void **recv) {
  SVR_ENTER(ctx);
  if (!ctx || !send || !recv) return SVR_E_ARG;
  NEED(ctx->slab && ctx->slab->valid && ctx->slab->world > 0, "svr_slab_plan first");
  if (ctx->reg_mode == 0) return fail(ctx, SVR_E_STATE, "svr_slab_update needs reg_mode 1");
  SlabPlan &p = *ctx->slab;
  const int R = p.rank;
  ScopedTimer t(ctx, SVR_T_REGULARIZE);
  if (p.rs_count[R]) {
    hipLaunchKernelGGL(k_slab_rs_unpack, dim3(nblk((size_t)2 * p.rs_count[R])), dim3(256), 0, ctx->stream, ctx->addon(), ctx->cmap(), p.d_midx, p.rs_start[R],
                       p.rs_count[R], p.rs_chunk, p.d_recv);
    KCHK("k_slab_rs_unpack");
  }
  const int ob = ctx->recon_cur == ctx->d_recon_volw ? 1 : 0;           // the buffer the update writes
  float *out = ob ? ctx->d_recon_new : ctx->d_recon_volw;
  if (!ctx->vol_clean[ob]) {
    HIPCHK(hipMemsetAsync(out, 0, ctx->nv * sizeof(float), ctx->stream));
    ctx->vol_clean[ob] = true;
  }
  int r = superresolution_update_planes(ctx, adaptive, alpha, min_intensity, max_intensity, delta, lambda, p.zb[R], p.zb[R + 1]);
  if (r) return r;
  hipLaunchKernelGGL(k_slab_ag_pack, dim3(nblk(p.ag_chunk)), dim3(256), 0, ctx->stream, out, p.d_didx, p.ag_start[R], p.ag_count[R], p.ag_chunk, p.d_send);
  KCHK("k_slab_ag_pack");
  t.stop();
  *send = p.d_send; *recv = p.d_recv;
  return SVR_OK;
}
int svr_slab_finish(svr_ctx *ctx) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  NEED(ctx->slab && ctx->slab->valid && ctx->slab->world > 0, "svr_slab_plan first");
  SlabPlan &p = *ctx->slab;
  float *out = ctx->recon_cur == ctx->d_recon_volw ? ctx->d_recon_new : ctx->d_recon_volw;
  hipLaunchKernelGGL(k_slab_ag_unpack, dim3(nblk((size_t)p.world * p.ag_chunk)), dim3(256), 0, ctx->stream, out, p.d_didx, p.d_tab, p.world, p.rank, p.ag_chunk, p.d_recv);
  KCHK("k_slab_ag_unpack");
  ctx->recon_cur = out;
  // addon | cmap now hold the sums of this rank's slab only: not a state a reader should see as "the scatter's result"
  invalidate(ctx, CH_SCATTER_TARGETS);
  ctx->prep_pending = false;
  if (!ctx->sr_no_wait) HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

int svr_superresolution(svr_ctx *ctx, int iter, const float *slice_weight, int adaptive, float alpha,
                        float min_intensity, float max_intensity, float delta, float lambda,
                        int global_bias_correction, float sigma_bias, float low_intensity_cutoff) {
  SVR_ENTER(ctx);
  (void)iter; (void)sigma_bias; (void)low_intensity_cutoff;
  // back-projection and update without a wait for the device in between or after: whatever reads the volume next is ordered
  // behind them on the stream, and every call that hands results to the host waits itself (down_flush, svr_sync_cpu, debug_get)
  ctx->sr_no_wait = true;
  int r = svr_superresolution_backproject(ctx, slice_weight);
  if (!r) r = svr_superresolution_update(ctx, adaptive, alpha, min_intensity, max_intensity, delta, lambda);
  ctx->sr_no_wait = false;
  if (r) return r;
  if (global_bias_correction) printf("_global_bias_correction not implemented\n");   // RC.cu:2182-2185
  return SVR_OK;
}

int svr_mask_volume(svr_ctx *ctx) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  NEED(ctx->nv > 0 && ctx->have_mask, "volume / mask not set");
  hipLaunchKernelGGL(k_mask_volume, dim3(nblk(ctx->nv)), dim3(256), 0, ctx->stream, ctx->recon(), ctx->d_mask, ctx->nv);
  KCHK("k_mask_volume");
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

int svr_scale_volume_sums(svr_ctx *ctx, double out2[2]) {
  SVR_ENTER(ctx);
  if (!ctx || !out2) return SVR_E_ARG;
  NEED(ctx->have_slices && ctx->have_scales, "slices / scales not set");
  hipLaunchKernelGGL(k_scalevol, dim3(ctx->chunks, ctx->ns), dim3(256), 0, ctx->stream, ctx->d_slices, ctx->d_weights,
                     ctx->d_simslices, ctx->d_simweights, ctx->d_slice_weights, (int)(ctx->sx * ctx->sy),
                     ctx->d_partial);
  KCHK("k_scalevol");
  int r = reduce_partials(ctx, 2, 0, 0, true);
  if (r) return r;
  HIPCHK(hipMemcpyAsync(out2, ctx->d_out, 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

int svr_scale_volume_apply(svr_ctx *ctx, float scale) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  NEED(ctx->nv > 0, "volume not set");
  hipLaunchKernelGGL(k_scale_volume, dim3(nblk(ctx->nv)), dim3(256), 0, ctx->stream, ctx->recon(), scale, ctx->nv);
  KCHK("k_scale_volume");
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

int svr_scale_volume(svr_ctx *ctx) {
  SVR_ENTER(ctx);
  double s2[2];
  int r = svr_scale_volume_sums(ctx, s2);
  if (r) return r;
  float scale = (float)(s2[0] / s2[1]);   // RC.cu:3459
  printf("Volume scale GPU: %f\n", scale);
  return svr_scale_volume_apply(ctx, scale);
}

int svr_restore_slice_intensities(svr_ctx *ctx, const float *stack_factors, int n_stacks,
                                  const int *stack_index) {
  SVR_ENTER(ctx);
  if (!ctx || !stack_factors || !stack_index || n_stacks <= 0) return SVR_E_ARG;
  NEED(ctx->have_slices, "slices not filled");
  for (uint32_t i = 0; i < ctx->ns; ++i)
    if (stack_index[i] < 0 || stack_index[i] >= n_stacks) return fail(ctx, SVR_E_ARG, "stack index out of range");
  DevBuf<float> d_f;
  DevBuf<int> d_i;
  HIPCHK(d_f.reserve(n_stacks));
  HIPCHK(d_i.reserve(ctx->ns));
  HIPCHK(hipMemcpyAsync(d_f, stack_factors, n_stacks * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(d_i, stack_index, ctx->ns * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_restore, dim3(nblk(ctx->np)), dim3(256), 0, ctx->stream, ctx->d_slices, d_f, d_i,
                     (int)(ctx->sx * ctx->sy), ctx->np);
  hipError_t e = hipGetLastError();
  (void)hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return fail(ctx, (int)e, "k_restore");
  return SVR_OK;
}

// ---- buffers ---------------------------------------------------------------------------
static int buffer_info(svr_ctx *ctx, int which, void **ptr, size_t *bytes) {
  if ((which == SVR_BUF_ADDON || which == SVR_BUF_CONFIDENCE_MAP) && ctx->nv) {
    const int rs = regul_settle(ctx);      // (the fused volume update leaves Prep's changes of the two buffers to their readers)
    if (rs) return rs;
  }
  switch (which) {
    case SVR_BUF_RECONSTRUCTED: *ptr = ctx->nv ? ctx->recon() : nullptr; *bytes = ctx->nv * 4; break;
    case SVR_BUF_VOL_WEIGHTS: *ptr = ctx->nv ? ctx->volw() : nullptr; *bytes = ctx->nv * 4; break;
    case SVR_BUF_ADDON: *ptr = ctx->nv ? ctx->addon() : nullptr; *bytes = ctx->nv * 4; break;
    case SVR_BUF_CONFIDENCE_MAP: *ptr = ctx->nv ? ctx->cmap() : nullptr; *bytes = ctx->nv * 4; break;
    case SVR_BUF_MASK: *ptr = ctx->d_mask; *bytes = ctx->nv * 4; break;
    case SVR_BUF_BIAS_VOLUME: *ptr = ctx->d_bias_vol; *bytes = ctx->nv * 4; break;
    case SVR_BUF_SMOOTH_MASK: *ptr = ctx->d_maskC; *bytes = ctx->nv * 4; break;
    case SVR_BUF_BIAS: *ptr = ctx->d_bias; *bytes = ctx->np * 4; break;
    case SVR_BUF_SLICES: *ptr = ctx->d_slices; *bytes = ctx->np * 4; break;
    case SVR_BUF_WEIGHTS: *ptr = ctx->d_weights; *bytes = ctx->np * 4; break;
    case SVR_BUF_SIMSLICES: *ptr = ctx->d_simslices; *bytes = ctx->np * 4; break;
    case SVR_BUF_SIMWEIGHTS: *ptr = ctx->d_simweights; *bytes = ctx->np * 4; break;
    case SVR_BUF_PSF_SUMS: *ptr = ctx->d_psf_sums; *bytes = ctx->np * 4; break;
    case SVR_BUF_SIMINSIDE: *ptr = ctx->d_siminside; *bytes = ctx->np; break;
    case SVR_BUF_VOXEL_COUNT: *ptr = ctx->d_voxcount; *bytes = ctx->np * 4; break;
    default: return SVR_E_ARG;
  }
  return *ptr ? SVR_OK : SVR_E_STATE;
}

int svr_debug_get(svr_ctx *ctx, int which, void *host_out, size_t bytes) {
  SVR_ENTER(ctx);
  if (!ctx || !host_out) return SVR_E_ARG;
  void *p; size_t b;
  int r = buffer_info(ctx, which, &p, &b);
  if (r) return fail(ctx, r, "svr_debug_get: buffer not available");
  if (bytes != b) return fail(ctx, SVR_E_ARG, "svr_debug_get: size mismatch");
  HIPCHK(hipMemcpyAsync(host_out, p, b, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

int svr_debug_set(svr_ctx *ctx, int which, const void *host_in, size_t bytes) {
  SVR_ENTER(ctx);
  if (!ctx || !host_in) return SVR_E_ARG;
  void *p; size_t b;
  int r = buffer_info(ctx, which, &p, &b);
  if (r) return fail(ctx, r, "svr_debug_set: buffer not available");
  if (bytes != b) return fail(ctx, SVR_E_ARG, "svr_debug_set: size mismatch");
  HIPCHK(hipMemcpyAsync(p, host_in, b, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (which == SVR_BUF_SIMINSIDE) {                      // (the per-slice flags follow: the cell gather only ever raises them)
    hipLaunchKernelGGL(k_slice_inside, dim3(ctx->ns), dim3(256), 0, ctx->stream, ctx->d_siminside, (int)(ctx->sx * ctx->sy), ctx->d_slice_inside);
    KCHK("k_slice_inside");
  }
  // (a mask set behind svr_set_mask's back: no mask box, the whole pair is exchanged; maskC stays as it was)
  invalidate(ctx, which == SVR_BUF_SLICES ? CH_SLICE_PIXELS : which == SVR_BUF_PSF_SUMS ? CH_PSF_SUMS : which == SVR_BUF_MASK ? CH_MASK
                  : which == SVR_BUF_RECONSTRUCTED ? CH_VOLUME_VALUES : which == SVR_BUF_ADDON || which == SVR_BUF_CONFIDENCE_MAP ? CH_SCATTER_TARGETS : 0u);
  if (which == SVR_BUF_SIMSLICES) ctx->have_sim = true;   // (a test's own forward projection: svr_slice_quality takes it)
  if (which == SVR_BUF_WEIGHTS) ctx->have_em = true;      // (a test's own posteriors: svr_channel_scatter takes them)
  if (which == SVR_BUF_SLICES) return build_list(ctx, false);
  return SVR_OK;
}

void *svr_device_ptr(svr_ctx *ctx, int which) {
  SVR_ENTER(ctx);
  if (!ctx) return nullptr;
  void *p; size_t b;
  if (buffer_info(ctx, which, &p, &b)) return nullptr;
  return p;
}

size_t svr_volume_voxels(const svr_ctx *ctx) { return ctx ? ctx->nv : 0; }

int svr_debug_probe_pixel(svr_ctx *ctx, int slice, int px, int py, float *vals4096, int *centre3) {
  SVR_ENTER(ctx);
  if (!ctx || !vals4096 || !centre3) return SVR_E_ARG;
  int r = ready(ctx);
  if (r) return r;
  if (slice < 0 || slice >= (int)ctx->ns || px < 0 || px >= (int)ctx->sx || py < 0 || py >= (int)ctx->sy)
    return fail(ctx, SVR_E_ARG, "pixel out of range");
  DevBuf<float> d_v;
  DevBuf<int> d_c;
  HIPCHK(d_v.reserve(4096));
  HIPCHK(d_c.reserve(3));
  PsfArgs a = make_args(ctx);
  uint32_t idx = (uint32_t)px + (uint32_t)py * ctx->sx + (uint32_t)slice * ctx->sx * ctx->sy;
  hipLaunchKernelGGL(k_probe_pixel, dim3(1), dim3(64), 0, ctx->stream, a, idx, d_v, d_c);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(vals4096, d_v, 4096 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(centre3, d_c, 3 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return fail(ctx, (int)e, "svr_debug_probe_pixel");
  return SVR_OK;
}

// ---- PVR superpixel masks (ImagePatch2D::spxMask, R2/include/ImagePatch2D.cuh:51) ----------
int svr_set_spx_masks(svr_ctx *ctx, const char *masks_or_null) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  NEED(ctx->ns > 0, "initStorageVolumes first");
  ctx->d_spx.reset();
  if (!masks_or_null) return SVR_OK;
  const size_t bytes = (size_t)ctx->ns * 4096;
  HIPCHK(ctx->d_spx.reserve(bytes));
  HIPCHK(hipMemcpyAsync(ctx->d_spx, masks_or_null, bytes, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

// ---- bias correction --------------------------------------------------------------------
int svr_correct_bias(svr_ctx *ctx, float sigma_bias, int global_bias_correction) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  NEED(!ctx->disable_bias, "bias correction is disabled (svr_set_flags)");
  NEED(ctx->have_slices && ctx->have_scales && ctx->have_dims, "slices / scales / slice dims not set");
  int r = ensure_bias_buffers(ctx);
  if (r) return r;
  r = prepare_slice_consts(ctx);
  if (r) return r;
  const size_t fb = ctx->np * sizeof(float);
  const int n2 = (int)(ctx->sx * ctx->sy);
  ++ctx->bias_corrections;
  // bias_mode 1: residual, the four passes and the update in one kernel, a strip of bx columns per workgroup (svr_bias.inc); the
  // widest strip whose LDS fits 64 KiB, else the stencils.  The new field lands in d_buffer, which becomes d_bias.
  int bx = 0, half = 0;
  if (ctx->bias_mode >= 1) {
    for (uint32_t sl = 0; sl < ctx->ns; ++sl) half = std::max(half, gauss_half_host(sigma_bias, ctx->slice_dims[3 * (size_t)sl]));
    for (int b = 64; b >= 8 && !bx; b /= 2)
      if (half <= BIAS_HMAX && bias_field_lds_bytes((int)ctx->sy, b, half) <= 65536) bx = b;
  }
  ctx->last_bias_bx = bx;
  if (bx) {
    const dim3 grid(((int)ctx->sx + bx - 1) / bx, ctx->ns);
    hipLaunchKernelGGL(k_bias_field_lds, grid, dim3(256), bias_field_lds_bytes((int)ctx->sy, bx, half), ctx->stream,
                       ctx->d_slices, ctx->d_bias, ctx->d_weights, ctx->d_simweights, ctx->d_simslices, ctx->d_scales, ctx->d_sc,
                       (int)ctx->sx, (int)ctx->sy, sigma_bias, bx, ctx->d_buffer);
    KCHK("k_bias_field_lds");
    std::swap(ctx->d_bias, ctx->d_buffer);
  } else {
  HIPCHK(hipMemsetAsync(ctx->d_wb, 0, fb, ctx->stream));       // RC.cu:1873-1875
  HIPCHK(hipMemsetAsync(ctx->d_wr, 0, fb, ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->d_buffer, 0, fb, ctx->stream));
  hipLaunchKernelGGL(k_bias_residual, dim3(nblk(ctx->np)), dim3(256), 0, ctx->stream, ctx->d_slices, ctx->d_bias,
                     ctx->d_weights, ctx->d_simweights, ctx->d_simslices, ctx->d_scales, n2, ctx->np, ctx->d_wb, ctx->d_wr);
  KCHK("k_bias_residual");
  const dim3 grid((ctx->sx + 63) / 64, (ctx->sy + 3) / 4, ctx->ns);
#define CONV(in, out, horiz) \
  hipLaunchKernelGGL(k_gauss_conv_slices, grid, dim3(256), 0, ctx->stream, in, out, ctx->d_sc, (int)ctx->sx, (int)ctx->sy, \
                     (int)ctx->ns, sigma_bias, horiz)
  CONV(ctx->d_wb, ctx->d_buffer, 1);       // RC.cu:1886
  CONV(ctx->d_buffer, ctx->d_wb, 0);       // RC.cu:1888
  CONV(ctx->d_wr, ctx->d_buffer, 1);       // RC.cu:1889 (buffer still holds the first pass where the result is 0)
  CONV(ctx->d_buffer, ctx->d_wr, 0);       // RC.cu:1891
#undef CONV
  KCHK("k_gauss_conv_slices");
  hipLaunchKernelGGL(k_bias_update, dim3(nblk(ctx->np)), dim3(256), 0, ctx->stream, ctx->d_slices, ctx->d_bias, ctx->d_wb,
                     ctx->d_wr, ctx->np);
  KCHK("k_bias_update");
  }
  if (!global_bias_correction) {
    hipLaunchKernelGGL(k_bias_mean, dim3(ctx->chunks, ctx->ns), dim3(256), 0, ctx->stream, ctx->d_slices, ctx->d_bias, n2,
                       ctx->d_partial);
    KCHK("k_bias_mean");
    r = reduce_partials(ctx, 2, 0, 0, false);
    if (r) return r;
    hipLaunchKernelGGL(k_bias_sub_mean, dim3(nblk(ctx->np)), dim3(256), 0, ctx->stream, ctx->d_slices, ctx->d_bias,
                       ctx->d_per_slice, n2, ctx->np);
    KCHK("k_bias_sub_mean");
  } else {
    printf("_global_bias_correction is not implemented in CUDA yet\n");   // RC.cu:1932
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

int svr_normalise_bias_local(svr_ctx *ctx) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  NEED(!ctx->disable_bias, "bias correction is disabled (svr_set_flags)");
  int r = ready(ctx);
  if (r) return r;
  r = ensure_psf_list(ctx);
  if (r) return r;
  ++ctx->bias_scatters;
  PsfArgs a = make_args(ctx);
  a.list = ctx->d_psf_list;
  a.n = ctx->n_psf;
  // bias_mode >= 1: the SR scatter's cell kernels (no atomics: the same bits from run to run, with the coefficient table or without) --
  // factors f1 = 1 / sume, f0 = f1 (bias - log scale) over the PSF pixels, back_cell_kernel (streaming the table when it is valid:
  // NormaliseBias follows SuperresolutionGPU on the same geometry), the combine writes bias_vol and this call's weights, which are
  // then added to the never-cleared dev_volume_weights_.  A sharded rank scatters its own slices through its own cell lists.
  const PassPath p = pass_path(ctx, PASS_BIAS);
  CellState *cs = nullptr;
  if (a.n && p.family == FAM_CELLS &&
      (r = cells_or_fallback(ctx, false, 0, "the NormaliseBias scatter left the cell path (the cell lists cannot hold this geometry): float atomics, last bits depend on the run", cs))) return r;
  if (cs) {
    TableUse use;
    if ((r = table_begin(ctx, table_plan_for(ctx, PASS_BIAS, p, true), a, &use))) return r;
    if ((r = launch_cell_scatter(ctx, a, 2, ctx->d_bias_vol, ctx->d_mbuf))) return r;
    hipLaunchKernelGGL(k_add_to, dim3(nblk(ctx->nv)), dim3(256), 0, ctx->stream, ctx->d_volume_weights, ctx->d_mbuf, ctx->nv);
    KCHK("k_add_to");
    ++ctx->bias_scatters_on_cells;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SVR_OK;
  }
  HIPCHK(hipMemsetAsync(ctx->d_bias_vol, 0, ctx->nv * sizeof(float), ctx->stream));   // RC.cu:2621
  a.recon = ctx->d_bias_vol;            // scattered value: psf/sume * (bias - log scale)
  a.volw = ctx->d_volume_weights;       // dev_volume_weights_: accumulates, never cleared (RC.cu:2633)
  if (a.n && (r = launch_pixels(ctx, a, psf_kernel<MODE_BIAS>, "psf_kernel<BIAS>"))) return r;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

int svr_normalise_bias_finish(svr_ctx *ctx, float sigma_bias) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  NEED(!ctx->disable_bias && ctx->d_bias_vol && ctx->maskC_valid, "bias buffers not ready");
  const size_t nv = ctx->nv;
  ++ctx->bias_normalisations;
  if (ctx->bias_mode == 2 || (ctx->bias_mode == 1 && nv >= BIAS_LDS_TAIL_MIN)) {
    // svr_bias.inc: x lines (with divS by the weights), y and z columns (with the copy, divS by maskC and divexp)
    // through the LDS; the widest strips whose LDS fits 64 KiB, else the stencils below
    const int vx = (int)ctx->vx, vy = (int)ctx->vy, vz = (int)ctx->vz;
    int half = 0;
    for (int d = 0; d < 3; ++d) half = std::max(half, gauss_half_host(sigma_bias, ctx->vdim[d]));
    const size_t gb = (BIAS_HMAX + 1) * sizeof(float), cap = 65536;
    int rows = 0, bxy = 0, bxz = 0;
    for (int r = 16; r >= 1 && !rows; r /= 2) if (gb + (size_t)r * vx * 4 <= cap) rows = r;
    for (int b = 64; b >= 4 && !bxy; b /= 2) if (gb + (size_t)vy * b * 4 <= cap) bxy = b;
    for (int b = 64; b >= 4 && !bxz; b /= 2) if (gb + (size_t)vz * b * 4 <= cap) bxz = b;
    if (half <= BIAS_HMAX && rows && bxy && bxz) {
      ctx->last_tail_lds = 1; ctx->last_tail_rows = rows; ctx->last_tail_bxy = bxy; ctx->last_tail_bxz = bxz;
      const int nlines = vy * vz;
      hipLaunchKernelGGL(k_gauss3d_x_lds, dim3((nlines + rows - 1) / rows), dim3(256), gb + (size_t)rows * vx * 4, ctx->stream,
                         ctx->d_bias_vol, ctx->volw(), ctx->d_mbuf, sigma_bias, ctx->vdim[0], vx, nlines, rows);
      hipLaunchKernelGGL(k_gauss3d_col_lds<false>, dim3((vx + bxy - 1) / bxy, vz), dim3(256), gb + (size_t)vy * bxy * 4, ctx->stream,
                         ctx->d_mbuf, ctx->d_bias_vol, (const float *)nullptr, (const float *)nullptr, (float *)nullptr, sigma_bias,
                         ctx->vdim[1], vx, vy, vz, bxy);
      hipLaunchKernelGGL(k_gauss3d_col_lds<true>, dim3((vx + bxz - 1) / bxz, vy), dim3(256), gb + (size_t)vz * bxz * 4, ctx->stream,
                         ctx->d_bias_vol, ctx->d_bias_vol, ctx->d_mbuf, ctx->d_maskC, ctx->recon(), sigma_bias, ctx->vdim[2], vx, vy, vz, bxz);
      KCHK("k_gauss3d_*_lds");
      HIPCHK(hipStreamSynchronize(ctx->stream));
      return SVR_OK;
    }
  }
  ctx->last_tail_lds = 0; ctx->last_tail_rows = ctx->last_tail_bxy = ctx->last_tail_bxz = 0;
  const dim3 grid((ctx->vx + 63) / 64, (ctx->vy + 3) / 4, ctx->vz);
  hipLaunchKernelGGL(k_div_s, dim3(nblk(nv)), dim3(256), 0, ctx->stream, ctx->d_bias_vol, ctx->volw(), nv);   // RC.cu:2553-2556
  // the reference's mbuf is uninitialised device memory (RC.cu:2563-2564); zero it so a NaN result is defined
  HIPCHK(hipMemsetAsync(ctx->d_mbuf, 0, nv * sizeof(float), ctx->stream));
  hipLaunchKernelGGL(k_gauss_conv3d, grid, dim3(256), 0, ctx->stream, ctx->d_bias_vol, ctx->d_mbuf, sigma_bias, 0,
                     ctx->vdim[0], (int)ctx->vx, (int)ctx->vy, (int)ctx->vz);
  hipLaunchKernelGGL(k_gauss_conv3d, grid, dim3(256), 0, ctx->stream, ctx->d_mbuf, ctx->d_bias_vol, sigma_bias, 1,
                     ctx->vdim[1], (int)ctx->vx, (int)ctx->vy, (int)ctx->vz);
  hipLaunchKernelGGL(k_gauss_conv3d, grid, dim3(256), 0, ctx->stream, ctx->d_bias_vol, ctx->d_mbuf, sigma_bias, 2,
                     ctx->vdim[2], (int)ctx->vx, (int)ctx->vy, (int)ctx->vz);
  KCHK("k_gauss_conv3d");
  HIPCHK(hipMemcpyAsync(ctx->d_bias_vol, ctx->d_mbuf, nv * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
  hipLaunchKernelGGL(k_div_s, dim3(nblk(nv)), dim3(256), 0, ctx->stream, ctx->d_bias_vol, ctx->d_maskC, nv);   // RC.cu:2575-2577
  hipLaunchKernelGGL(k_divexp, dim3(nblk(nv)), dim3(256), 0, ctx->stream, ctx->recon(), ctx->d_bias_vol, nv);  // RC.cu:2579-2581
  KCHK("k_divexp");
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

int svr_normalise_bias(svr_ctx *ctx, int iter, float sigma_bias) {
  SVR_ENTER(ctx);
  (void)iter;
  int r = svr_normalise_bias_local(ctx);
  if (r) return r;
  return svr_normalise_bias_finish(ctx, sigma_bias);
}

// ---- measurement -----------------------------------------------------------------------
int svr_timer_enable(svr_ctx *ctx, int enable) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  timers_resolve(ctx);
  ctx->timers = enable != 0;
  return SVR_OK;
}
int svr_timer_reset(svr_ctx *ctx) {
  SVR_ENTER(ctx);
  if (!ctx) return SVR_E_ARG;
  timers_resolve(ctx);
  for (int i = 0; i < SVR_T_COUNT; ++i) { ctx->t_ms[i] = 0; ctx->t_n[i] = 0; }
  return SVR_OK;
}
int svr_timer_get(svr_ctx *ctx, int which, double *ms_total, long *launches) {
  SVR_ENTER(ctx);
  if (!ctx || which < 0 || which >= SVR_T_COUNT) return SVR_E_ARG;
  timers_resolve(ctx);
  if (ms_total) *ms_total = ctx->t_ms[which];
  if (launches) *launches = ctx->t_n[which];
  return SVR_OK;
}
int svr_unit_counts(svr_ctx *ctx, uint64_t out3[3]) {
  SVR_ENTER(ctx);
  if (!ctx || !out3) return SVR_E_ARG;
  int r = ready(ctx);
  if (r) return r;
  if ((r = cell_prepare(ctx))) return r;
  const CellState &cs = *ctx->cell;
  const uint64_t ns = ctx->pvr ? PVR_N : PSF_SUPPORT;
  out3[0] = cs.n_sorted;
  out3[1] = (uint64_t)cs.n_sorted * ns - cs.dead_units;
  out3[2] = cs.dead_units;
  return SVR_OK;
}
// what the cell lists of the current slice geometry hold (the per-item fixed costs of a sharded run: bench.py --shard)
int svr_cell_stats(svr_ctx *ctx, uint64_t out8[8]) {
  SVR_ENTER(ctx);
  if (!ctx || !out8) return SVR_E_ARG;
  int r = ready(ctx);
  if (r) return r;
  for (int k = 0; k < 8; ++k) out8[k] = 0;
  if ((r = cell_prepare(ctx))) return r;
  const CellState &cs = *ctx->cell;
  out8[0] = cs.a.nitems; out8[1] = cs.n_runs; out8[2] = cs.n_sorted;
  out8[3] = (uint64_t)cs.a.nents * cs.a.PP * sizeof(f2);      // staging bytes written by the scatter, read by the combine
  CellState *g = nullptr;
  if ((r = cell_prepare_gather(ctx, g))) return r;
  if (g) { out8[4] = g->a.nitems; out8[5] = g->n_runs; out8[6] = (uint64_t)g->n_sorted * (ctx->pvr ? PVR_N : PSF_SUPPORT) * sizeof(f2); }
  out8[7] = (uint64_t)cs.a.CX << 32 | (uint64_t)cs.a.CL;
  return SVR_OK;
}
int svr_timer_begin(svr_ctx *ctx, int which) {
  SVR_ENTER(ctx);
  if (!ctx || which < 0 || which >= SVR_T_COUNT) return SVR_E_ARG;
  if (ctx->timers) {
    if (!ctx->ev_open) ctx->ev_open = timer_event(ctx);
    if (ctx->ev_open) HIPCHK(hipEventRecord(ctx->ev_open, ctx->stream));
  }
  return SVR_OK;
}
int svr_timer_end(svr_ctx *ctx, int which) {
  SVR_ENTER(ctx);
  if (!ctx || which < 0 || which >= SVR_T_COUNT) return SVR_E_ARG;
  if (ctx->timers && ctx->ev_open) {
    timer_close(ctx, which, ctx->ev_open);
    ctx->ev_open = nullptr;
  }
  return SVR_OK;
}
int svr_timer_add(svr_ctx *ctx, int which, double ms) {
  if (!ctx || which < 0 || which >= SVR_T_COUNT) return SVR_E_ARG;
  if (ctx->timers) { ctx->t_ms[which] += ms; ctx->t_n[which] += 1; }
  return SVR_OK;
}
// A fixed amount of dependent f32 work on every SIMD of the chip (4 wavefronts per SIMD, each a chain of `n` fmas): its time is a fixed number of
// cycles over the shader clock the device sustains under a full vector load -- what differs between the boxes of a pool (power caps, temperature)
// when the same binary reads 158 on one and 189 MVoxels/s on another.  bench.py reports it next to the headline.
__global__ __launch_bounds__(256) void k_clock_probe(float *out, int n) {
  // eight independent chains of packed fmas per lane: the vector pipe at its full issue rate, i.e. the power draw of the PSF kernels -- a box
  // that holds its clock on a light load and drops it on this one is what the probe is there to show
  f2 x[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) x[k] = (f2){1.0f + 1.0e-7f * (float)(threadIdx.x + k), 1.0f - 1.0e-7f * (float)(threadIdx.x + k)};
  const f2 a = (f2){0.99999994f, 1.00000012f}, b = (f2){1.0e-9f, -1.0e-9f};
  for (int i = 0; i < n; i += 8) {
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = fma2(x[k], a, b);
  }
  f2 t = x[0];
#pragma unroll
  for (int k = 1; k < 8; ++k) t = t + x[k];
  if (t.x == 12345.678f && t.y == 1.0f) out[blockIdx.x] = t.x;   // (never: keeps the chains)
}
int svr_clock_probe(svr_ctx *ctx, int chain, double *ms) {
  SVR_ENTER(ctx);
  if (!ctx || !ms || chain <= 0) return SVR_E_ARG;
  DevBuf<float> d;
  HIPCHK(d.reserve(4096));
  hipEvent_t a = nullptr, b = nullptr;
  hipError_t e = hipEventCreate(&a);
  if (e == hipSuccess) e = hipEventCreate(&b);
  float best = 3.0e38f;
  for (int rep = 0; rep < 4 && e == hipSuccess; ++rep) {   // the first launch warms the clocks up; the shortest of the rest
    e = hipEventRecord(a, ctx->stream);
    hipLaunchKernelGGL(k_clock_probe, dim3(1024), dim3(256), 0, ctx->stream, d, chain);   // 256 CUs x 4 workgroups of 4 wavefronts: 4 per SIMD
    if (e == hipSuccess) e = hipEventRecord(b, ctx->stream);
    if (e == hipSuccess) e = hipEventSynchronize(b);
    float t = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&t, a, b);
    if (rep > 0 && t < best) best = t;
  }
  if (a) (void)hipEventDestroy(a);
  if (b) (void)hipEventDestroy(b);
  if (e != hipSuccess) return fail(ctx, (int)e, std::string("svr_clock_probe: ") + hipGetErrorString(e));
  *ms = best;
  return SVR_OK;
}
int svr_fallbacks(svr_ctx *ctx, uint64_t out4[4]) {
  SVR_ENTER(ctx);
  if (!ctx || !out4) return SVR_E_ARG;
  for (int k = 0; k < 4; ++k) out4[k] = ctx->fallbacks[k];
  return SVR_OK;
}

int svr_counters(svr_ctx *ctx, uint64_t out5[8]) {
  SVR_ENTER(ctx);
  if (!ctx || !out5) return SVR_E_ARG;
  if (ctx->have_slices) {
    int r = ensure_tiles_back(ctx);
    if (r) return r;
  }
  out5[0] = ctx->np; out5[1] = ctx->n_active; out5[2] = ctx->n_psf; out5[3] = ctx->nv; out5[4] = ctx->ns;
  out5[5] = ctx->n_tiles; out5[6] = ctx->n_tiles_fb; out5[7] = ctx->n_tiles_fb8;
  return SVR_OK;
}

}  // extern "C"

#include "svr_reg.inc"
#include "svr_pyr.inc"
#include "svr_sim.inc"
#include "svr_nmi.inc"
#include "svr_lncc.inc"
#include "svr_motion.inc"
#include "svr_quality.inc"
#include "svr_ssim.inc"
#include "svr_seed.inc"
#include "svr_channel.inc"
#include "svr_fit.inc"
#include "svr_em.inc"
