// The coefficient table's layout (CoeffTable::d_coeff, svr_hip.hip): the one definition for its writers, its readers and the host allocation.
//
// The table holds, for every pixel that has a place in it (its id: d_coeff_id), the evaluated PSF taps of its NS units -- a unit = one
// plane of the pixel's NS x NS x NS footprint along the axis the slice's cells own, NS rows of NS taps, what eval_row_t returns per row,
// skipped taps as -0.0f.  The kernels work on a unit with the 16 lanes of a slot, lane = row, exactly the decomposition of the scatter
// and the gather, so the table is
//
//     float4 coeff[pixel][plane][quad][row]          plane < NS, quad < NS / 4 (taps 4 quad .. 4 quad + 3 of the row), row < 16
//
// with the row innermost: the 16 lanes of a slot write and later read 256 contiguous bytes per instruction, one instruction per tap quad.
// The row pitch is the slot's 16 lanes whatever the support: support 16 (slice-to-volume) fills 16 units of 1 KiB per pixel, support 12
// (patch-based) has 12 units of 768 bytes of which rows 12 .. 15 of every quad are never written or read.
// Dead units (unit_is_dead) are not stored: the kernels evaluate their first taps themselves.
//
// The first part is plain C++ (tests/coeff_layout_check.cpp compiles it with g++); the device helpers follow under __HIPCC__.
#pragma once

#include <stddef.h>
#include <stdint.h>

template <int NS>
struct CoeffLayout {
  static_assert(NS % 4 == 0 && NS <= 16, "tap quads, one row per lane of a 16-lane slot");
  static constexpr int QUADS = NS / 4;                   // tap quads (float4) per row
  static constexpr int ROW_PITCH = 16;                   // float4 from one quad to the next: the lanes of a slot
  static constexpr int UNIT_F4 = QUADS * ROW_PITCH;      // float4 per unit
  static constexpr int UNITS = NS;                       // units (planes) per pixel
  static constexpr size_t PIXEL_F4 = (size_t)UNITS * UNIT_F4;
  static constexpr size_t PIXEL_BYTES = PIXEL_F4 * 16;   // 16384 for support 16, 9216 for support 12

  // Row `row` of unit (pid, plane), counted in float4 from `base`: a pointer into the table, or 0 for the row's index.  The sum is
  // base + unit + row in this order: the compiler keeps the association, and the kernels' address arithmetic was tuned with this one.
  // A tap quad's float4 of the row lies quad * ROW_PITCH further on.
  template <class T>
  static constexpr T row_at(T base, uint32_t pid, int plane, int row) { return base + ((size_t)pid * NS + (size_t)plane) * UNIT_F4 + row; }
  static constexpr size_t index(uint32_t pid, int plane, int quad, int row) { return row_at<size_t>(0, pid, plane, row) + (size_t)(quad * ROW_PITCH); }

  // The landing stage of a row that travels by LDS-DMA (fwd_cell_kernel, COEFF == 2): a wavefront's 64 lanes (four slots of 16 rows) put
  // one float4 per lane and quad, lane-linear, so a stage is [quad][lane] float4 and QUADS * 1024 bytes
  static constexpr int STAGE_QUAD_F4 = 64;
  static constexpr uint32_t STAGE_QUAD_BYTES = STAGE_QUAD_F4 * 16;
  static constexpr uint32_t STAGE_BYTES = QUADS * STAGE_QUAD_BYTES;
};

#ifdef __HIPCC__
// Row `y` of unit (pid, plane).  Whether a lane beyond the support reads row 0 instead (y < NS ? y : 0) or stays out is the caller's decision.
template <int NS>
__device__ __forceinline__ const float4 *coeff_row(const float4 *base, uint32_t pid, int plane, int y) {
  return CoeffLayout<NS>::row_at(base, pid, plane, y);
}
template <int NS>
__device__ __forceinline__ void coeff_load_row(const float4 *row, float4 (&dst)[NS / 4]) {
#pragma unroll
  for (int q = 0; q < NS / 4; ++q) dst[q] = load_stream(row + q * CoeffLayout<NS>::ROW_PITCH);
}
// Tap x of a loaded row.  (An accessor, so that the caller's out[x] = coeff_tap(row, x) stays a plain store to its own array: an unpack
// that writes the caller's array through a reference compiles back_wave_kernel<12> differently.)
template <int NS>
__device__ __forceinline__ float coeff_tap(const float4 (&row)[NS / 4], int x) {
  const float4 c = row[x >> 2];
  return (x & 3) == 0 ? c.x : (x & 3) == 1 ? c.y : (x & 3) == 2 ? c.z : c.w;
}
template <int NS>
__device__ __forceinline__ void coeff_store_row(const float4 *row, const float (&out)[NS]) {
  float4 *dst = const_cast<float4 *>(row);
#pragma unroll
  for (int q = 0; q < NS / 4; ++q) store_stream(dst + q * CoeffLayout<NS>::ROW_PITCH, out[4 * q], out[4 * q + 1], out[4 * q + 2], out[4 * q + 3]);
}
// a row on its way into the stage at LDS byte address `stage` (wave-uniform): NS / 4 loads in flight, counted by the caller (glds_wait)
template <int NS>
__device__ __forceinline__ void coeff_dma_row(const float4 *row, uint32_t stage) {
#pragma unroll
  for (int q = 0; q < NS / 4; ++q) glds16(row + q * CoeffLayout<NS>::ROW_PITCH, stage + q * CoeffLayout<NS>::STAGE_QUAD_BYTES);
}
#endif
