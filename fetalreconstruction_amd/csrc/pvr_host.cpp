// pvr_host.cpp -- the host side of the patch-to-volume reconstruction loop in C++:
// svr::irtkPatchBasedReconstruction mirrors the reconstruction part of irtkPatchBasedReconstruction<T>::run
// (source/reconstructionGPU2/irtkPatchBasedReconstruction.cpp = "PBR.cpp" :445-593) and the host halves of
// patchBasedRobustStatistics_gpu<T> ("PRS.cu" = patchBasedRobustStatistics_gpu.cu): initializeEMValues :78-95,
// EStep :224-556, MStep :570-640, Scale :672-745, InitializeRobustStatistics :793-845, with T = float.
// Device work goes through the engine's C-ABI (include/svr_hip.h) with the engine option "pvr" set.
//
// Sharded over ranks (svr_shard.h): the engine of a rank holds the patches [lo, hi) of the global numbering; the patch vectors
// (scale, weight, potential: svr_unit_em.h UnitState) stay GLOBAL on every rank and the patch-level EM runs replicated on them.
//
// Kept quirks: the patch potentials of stack i are written at the patch index inside the stack, without the
// stack offset (PRS.cu:256-276, svr_unit_em.h stack_potential_sources); the Gaussian's step is 0.00001f (:97-101,
// svr_unit_em.h PatchGauss) while m_step is 0.0001; delta 1, lambda 0.1 (patchBasedSuperresolution_gpu.cu:291-295).
#include <math.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/svr_host.h"
#include "svr_unit_em.h"

namespace svr {

class irtkPatchBasedReconstruction {
 public:
  svr_ctx *e;
  std::vector<int> counts;             // patches per stack
  int n;
  UnitState em;                        // the patches' vectors and EM scalars, the numbering, the device EM, the exchanges (svr_unit_em.h)
  Shard &sh = em.sh;
  std::string &err = em.err;
  float m_min_intensity, m_max_intensity;
  bool m_adaptive;
  float m_delta, m_lambda, m_alpha, m_step;
  int lo, hi;

  irtkPatchBasedReconstruction(svr_ctx *engine, const int *patches_per_stack, int n_stacks, float min_i, float max_i, int lo_ = 0,
                               int hi_ = -1, const svr_collectives *c = nullptr)
      : e(engine), counts(patches_per_stack, patches_per_stack + n_stacks), n(0), m_min_intensity(min_i),
        m_max_intensity(max_i), m_adaptive(false) {
    for (int c_ : counts) n += c_;
    lo = lo_; hi = hi_ < 0 ? n : hi_;
    em.init(engine, n, lo, hi, c, false);
    m_delta = 1.0f;
    m_lambda = 0.1f;
    m_alpha = (0.05f / m_lambda) * m_delta * m_delta;
    m_step = 0.0001f;
    em.step = m_step;
    em.var_floor = m_step * m_step / 6.28;
    em.src = stack_potential_sources(counts);   // PRS.cu:256-276: no stack offset on the left
  }

#define PENG(call) do { int rc_ = (call); if (rc_) return em.fail(rc_, #call); } while (0)

  int initializeEMValues() { return em.init_em_values(); }                 // PRS.cu:78-95

  int InitializeRobustStatistics() {                                         // PRS.cu:793-845
    if (int rc = em.settle()) return rc;
    double s2[2];
    PENG(svr_robust_statistics_sums(e, s2));
    if (sh.on) {
      std::vector<double> all;
      if (int rc = em.exchange(s2, 2, all, nullptr)) return rc;
      s2[0] = s2[1] = 0;
      for (int r = 0; r < sh.coll.world; ++r) { s2[0] += all[2 * r]; s2[1] += all[2 * r + 1]; }   // rank order: the same bits everywhere
    }
    if (s2[1] == 0) { err = "ERROR: sb = 0!! no sigma computed!"; return 10001; }   // the reference exits here
    em.sigma = (float)s2[0] / (float)s2[1];
    em.cls.var = 0.025f;
    em.mix = 0.9f;
    em.cls.mix = 0.9f;
    em.m = (float)(1.0f / (2.1f * m_max_intensity - 1.9f * m_min_intensity));
    return 0;
  }

  // PRS.cu:224-556; the patch-level EM :256-468 on the device or on the host (svr_unit_em.h), then copyToWeightsAndScales :486-491
  int EStep() { return em.estep(PatchGauss{}, std::vector<unsigned char>(n, 0)); }

  int MStep(int iter) { return em.mstep(iter); }                            // PRS.cu:570-640; PBR.cpp:540-545

  int Scale() {                                                              // PRS.cu:672-745
    PENG(svr_calculate_scale_vector(e, nullptr));                            // stays on the device: fetched with the E-step's potentials
    PENG(svr_adopt_scale_vector(e));                                         // (sharded: with the M-step's sums), or by settle.  copyToScales: no lag
    em.scale_pending = true;
    em.scale_stale = sh.on;                                                  // read next in the E-step, whose exchange completes it
    return 0;
  }

  // patchBased2D3DRegistration<T>::run for all patches (PBR.cpp:452-489): registers them against the current reconstruction and
  // hands the new transformations back to the engine.  T / Tinv [n][16] in/out, the other matrices as uploaded.
  int registerPatches(const float *ri2w, const float *mo, const float *invmo, float *T, float *Tinv, const float *i2w, const float *w2i,
                      const float *recon_i2w, const float *recon_w2i, long long counters3[3]) {
    PENG(svr_pvr_register_patches(e, ri2w, mo, invmo, T, Tinv, counters3));
    PENG(svr_set_slice_matrices(e, T, Tinv, i2w, w2i, i2w, w2i, recon_i2w, recon_w2i));
    return 0;
  }

  // one outer iteration without the patch registration (PBR.cpp:490-548)
  int reconstruct_iteration(int rec_iterations) {
    int rc;
    if ((rc = initializeEMValues())) return rc;
    int nvox = 0;
    if (!sh.on) {
      PENG(svr_gaussian_reconstruction(e, &nvox));     // reset + patchBasedPSFReconstruction_gpu + equalize
    } else {
      PENG(svr_gaussian_reconstruction_local(e));
      PENG(sh.allreduce_pair(SVR_BUF_RECONSTRUCTED, 2 * svr_volume_voxels(e)));
      PENG(svr_gaussian_reconstruction_finish(e, &nvox));
    }
    PENG(svr_simulate_slices(e, nullptr));          // (the patch-based loop never reads the inside flags: no wait)
    if ((rc = InitializeRobustStatistics())) return rc;
    if ((rc = EStep())) return rc;
    for (int i = 0; i < rec_iterations; ++i) {
      if ((rc = sr_iteration(i))) return rc;
    }
    return 0;
  }

  // one SR iteration (PBR.cpp:505-546): Scale, resetAddonCmap + run + regularize, simulate, M-step, E-step
  int sr_iteration(int i) {
    int rc;
    {
      if ((rc = Scale())) return rc;
      const float *pw;
      if ((rc = em.scatter_weights(&pw))) return rc;
      if (!sh.on) {
        PENG(svr_superresolution(e, i + 1, pw, m_adaptive, m_alpha, m_min_intensity, m_max_intensity, m_delta,
                                 m_lambda, 0, 12.0f, 0.01f));
      } else {
        PENG(sh.superresolution(pw, m_adaptive, m_alpha, m_min_intensity, m_max_intensity, m_delta, m_lambda));
      }
      PENG(svr_simulate_slices(e, nullptr));
      if ((rc = MStep(i + 1))) return rc;
      if ((rc = EStep())) return rc;
    }
    return 0;
  }
#undef PENG
};

}  // namespace svr

struct pvrh_recon {
  svr::irtkPatchBasedReconstruction impl;
  pvrh_recon(svr_ctx *e, const int *c, int ns, float mn, float mx, int lo, int hi, const svr_collectives *coll) : impl(e, c, ns, mn, mx, lo, hi, coll) {}
};

extern "C" {

pvrh_recon *pvrh_create(svr_ctx *engine, const int *patches_per_stack, int n_stacks, float min_intensity, float max_intensity) {
  if (!engine || !patches_per_stack || n_stacks <= 0) return nullptr;
  return new pvrh_recon(engine, patches_per_stack, n_stacks, min_intensity, max_intensity, 0, -1, nullptr);
}
pvrh_recon *pvrh_create_sharded(svr_ctx *engine, const int *patches_per_stack, int n_stacks, float min_intensity, float max_intensity,
                                int patch_lo, int patch_hi, const svr_collectives *coll) {
  if (!engine || !patches_per_stack || n_stacks <= 0) return nullptr;
  long total = 0;
  for (int k = 0; k < n_stacks; ++k) total += patches_per_stack[k];
  if (patch_lo < 0 || patch_hi < patch_lo || patch_hi > total) return nullptr;
  if (coll && coll->struct_size < SVR_COLLECTIVES_MIN_SIZE) return nullptr;
  if (coll && coll->world > 1 && (!coll->allreduce_volume_pair || !coll->allreduce_host)) return nullptr;
  return new pvrh_recon(engine, patches_per_stack, n_stacks, min_intensity, max_intensity, patch_lo, patch_hi, coll);
}
int pvrh_set_unit_order(pvrh_recon *r, const int *order_or_null) {
  return r ? r->impl.em.set_order(order_or_null, "pvrh_set_unit_order: not a permutation of the patches") : SVR_E_ARG;
}
void pvrh_force_collectives(pvrh_recon *r, int on) { if (r) { (void)r->impl.em.settle(); r->impl.sh.force(on != 0); } }
void pvrh_set_slab_update(pvrh_recon *r, int on) { if (r) r->impl.sh.slabs = on != 0; }
int pvrh_sr_iteration(pvrh_recon *r, int i) { return r->impl.sr_iteration(i); }
void pvrh_destroy(pvrh_recon *r) { delete r; }
const char *pvrh_last_error(const pvrh_recon *r) { return r ? r->impl.err.c_str() : "null"; }
int pvrh_initialize_em_values(pvrh_recon *r) { return r->impl.initializeEMValues(); }
int pvrh_initialize_robust_statistics(pvrh_recon *r) { return r->impl.InitializeRobustStatistics(); }
int pvrh_estep(pvrh_recon *r) { return r->impl.EStep(); }
int pvrh_mstep(pvrh_recon *r, int iter) { return r->impl.MStep(iter); }
int pvrh_scale(pvrh_recon *r) { return r->impl.Scale(); }
int pvrh_reconstruct_iteration(pvrh_recon *r, int rec_iterations) { return r->impl.reconstruct_iteration(rec_iterations); }
int pvrh_register_patches(pvrh_recon *r, const float *ri2w, const float *mo, const float *invmo, float *T, float *Tinv, const float *i2w,
                          const float *w2i, const float *recon_i2w, const float *recon_w2i, long long counters3[3]) {
  return r->impl.registerPatches(ri2w, mo, invmo, T, Tinv, i2w, w2i, recon_i2w, recon_w2i, counters3);
}
int pvrh_get_state(pvrh_recon *r, float *scale, float *patch_weight, float *patch_potential, double scalars8[8]) {
  svr::UnitState &u = r->impl.em;
  if (int rc = u.flush()) return rc;       // sharded: collective (the other ranks' scales may still be on their way)
  if (scale) std::copy(u.scale.begin(), u.scale.end(), scale);
  if (patch_weight) std::copy(u.weight.begin(), u.weight.end(), patch_weight);
  if (patch_potential) std::copy(u.potential.begin(), u.potential.end(), patch_potential);
  if (scalars8) u.scalars(scalars8);
  return 0;
}

}  // extern "C"
