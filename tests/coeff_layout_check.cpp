// The coefficient table's layout (csrc/svr_coeff.h, its plain C++ part) checked on the host: no engine, no GPU.
// Run by tests/test_coeff_layout_cpu.py; exits 0 when every property holds, prints the first one that does not.
#include <cstdio>
#include <vector>

#include "../fetalreconstruction_amd/csrc/svr_coeff.h"

#define CHECK(cond, ...) do { if (!(cond)) { std::printf("NS %d: ", NS); std::printf(__VA_ARGS__); std::printf("\n"); return 1; } } while (0)

template <int NS>
static int check(size_t bytes_per_pixel) {
  typedef CoeffLayout<NS> L;
  const uint32_t pixels = 3;
  const size_t total = pixels * L::PIXEL_F4;
  CHECK(L::QUADS == NS / 4 && L::ROW_PITCH == 16 && L::UNITS == NS, "constants");
  CHECK(L::UNIT_F4 == NS / 4 * 16 && L::PIXEL_F4 == (size_t)NS * (NS / 4 * 16), "float4 per unit / per pixel");
  CHECK(L::PIXEL_BYTES == bytes_per_pixel, "%zu bytes per pixel, not %zu", (size_t)L::PIXEL_BYTES, bytes_per_pixel);
  CHECK(L::STAGE_QUAD_BYTES == 1024u && L::STAGE_BYTES == (uint32_t)(NS / 4) * 1024u, "LDS-DMA stage");
  std::vector<int> seen(total, 0);
  size_t covered = 0;
  for (uint32_t pid = 0; pid < pixels; ++pid)
    for (int plane = 0; plane < NS; ++plane)
      for (int q = 0; q < NS / 4; ++q)
        for (int row = 0; row < NS; ++row) {
          const size_t i = L::index(pid, plane, q, row);
          // the specification: the expression the nine users carried before the layout had a definition
          const size_t spec = ((size_t)pid * NS + plane) * (NS / 4 * 16) + row + q * 16;
          CHECK(i == spec, "index(%u, %d, %d, %d) = %zu, specified %zu", pid, plane, q, row, i, spec);
          CHECK(i < total, "index(%u, %d, %d, %d) = %zu beyond %zu", pid, plane, q, row, i, total);
          CHECK(!seen[i], "index(%u, %d, %d, %d) = %zu taken twice", pid, plane, q, row, i);
          seen[i] = 1;
          ++covered;
          // the rows of one (pid, plane, quad): consecutive float4, 256 bytes for the 16 lanes of a slot
          CHECK(i == L::index(pid, plane, q, 0) + (size_t)row, "rows of (%u, %d, %d) not consecutive at %d", pid, plane, q, row);
          CHECK(L::row_at((size_t)0, pid, plane, row) + (size_t)q * L::ROW_PITCH == i, "row_at and index disagree");
        }
  CHECK(covered * 16 == total * NS, "%zu of %zu float4 covered", covered, total);
  // what is not covered: rows NS .. 15 of every quad, nothing else (support 16: nothing)
  for (size_t i = 0; i < total; ++i) {
    const int row = (int)(i % L::ROW_PITCH);
    CHECK(seen[i] == (row < NS), "float4 %zu (row %d of its quad) %s", i, row, seen[i] ? "covered" : "not covered");
  }
  return 0;
}

int main() {
  if (check<16>(16384) || check<12>(9216)) return 1;
  std::printf("ok\n");
  return 0;
}
