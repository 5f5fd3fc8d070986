// Driver of the host two-class EM over units (csrc/svr_unit_em.h unit_em) for tests/test_unit_em_cpu.py: g++, no engine, no GPU.
//   unit_em_check IN OUT
// IN:  int32 form (0 = slices, 1 = patches), int32 n, float64 var_floor, float64 step, float32 classes[5] = {mean, mean2, var, var2, mix},
//      float32 pot[n], float32 w[n], float32 scale[n], uint8 excluded[n], int32 n_stacks, int32 counts[n_stacks]
//      (patches: the potentials are read through stack_potential_sources(counts) first, as the patch host object does)
// OUT: float32 pot[n], float32 w[n], float32 classes[5]
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../fetalreconstruction_amd/csrc/svr_unit_em.h"

template <class T> static bool get(FILE *f, T *v, size_t n) { return fread(v, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: unit_em_check IN OUT\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t form, n, n_stacks;
  double floor_, step;
  float c5[5];
  bool ok = get(f, &form, 1) && get(f, &n, 1) && get(f, &floor_, 1) && get(f, &step, 1) && get(f, c5, 5);
  if (!ok || n < 0) return 3;
  std::vector<float> pot(n), w(n), scale(n);
  std::vector<unsigned char> excl(n);
  ok = get(f, pot.data(), n) && get(f, w.data(), n) && get(f, scale.data(), n) && get(f, excl.data(), n) && get(f, &n_stacks, 1);
  if (!ok || n_stacks < 0) return 3;
  std::vector<int32_t> counts(n_stacks);
  if (!get(f, counts.data(), n_stacks)) return 3;
  fclose(f);

  svr::UnitClasses c = {c5[0], c5[1], c5[2], c5[3], c5[4]};
  if (form == 0) {
    svr::unit_em(n, pot.data(), w.data(), scale.data(), excl.data(), floor_, c, svr::SliceGauss{step});
  } else {
    const std::vector<int> src = svr::stack_potential_sources(std::vector<int>(counts.begin(), counts.end()));
    if ((int)src.size() != n) return 4;
    pot = svr::gather_potentials(src, pot);
    svr::unit_em(n, pot.data(), w.data(), scale.data(), excl.data(), floor_, c, svr::PatchGauss{});
  }
  const float out5[5] = {c.mean, c.mean2, c.var, c.var2, c.mix};
  FILE *o = fopen(argv[2], "wb");
  if (!o) return 2;
  ok = fwrite(pot.data(), 4, n, o) == (size_t)n && fwrite(w.data(), 4, n, o) == (size_t)n && fwrite(out5, 4, 5, o) == 5;
  return fclose(o) == 0 && ok ? 0 : 5;
}
