// svr_unit_em.h -- the unit-level EM that both host objects (svr::irtkReconstruction, csrc/svr_host.cpp: slices;
// svr::irtkPatchBasedReconstruction, csrc/pvr_host.cpp: patches) drive.  A "unit" is a slice or a patch.
//
//   unit_em()     the two-class EM over the units on the host: pure, no engine calls (tests/unit_em_check.cpp builds it with g++)
//   UnitState     what the two objects share around it: the unit vectors and the eight EM scalars, the numbering of a sharded
//                 run, the device-side EM (csrc/svr_em.inc) and the host-side bookkeeping of the M-step and the exchanges
//
// The two forms differ in data only: the Gaussian (a template parameter of unit_em), the variance floor, the exclusion mask, the
// map of where each unit's potential comes from (`src`), and `slice_form` (slice_inside, and the M-step's engine calls).
#ifndef SVR_UNIT_EM_H
#define SVR_UNIT_EM_H

#include <float.h>
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "svr_shard.h"

namespace svr {

// ---- the pure two-class EM -----------------------------------------------------------------------------------------------------
// The units' potentials split into an inlier class (low potential: mean, var) and an outlier class (mean2, var2); a unit's weight
// is its posterior of the inlier class, `mix` the inliers' share.
struct UnitClasses { float mean, mean2, var, var2, mix; };

// The two forms' Gaussians: a zero-mean Gaussian of variance s at x, times the form's step
struct SliceGauss {          // slices: in double (irtkReconstructionGPU.h:529-532)
  double step;
  double operator()(float x, float s) const { const double d = x, v = s; return step * exp(-d * d / (2 * v)) / (sqrt(6.28 * v)); }
};
struct PatchGauss {          // patches: in float, 0.00001 for the step (patchBasedRobustStatistics_gpu.cu:97-101)
  double operator()(float x, float s) const { return 0.00001f * expf(-x * x / (2.0f * s)) / sqrtf(6.28f * s); }
};

// Sums over the units that take part (potential >= 0): a term weighted by the inlier weight w and by 1 - w, and those weights
struct ClassSums { double in = 0, in_w = 0, out = 0, out_w = 0; };

// One pass of the EM over n units in the reference's unit order; the host part of EStepGPU (irtkReconstructionGPU.cc) and of the
// patch-based EStep (patchBasedRobustStatistics_gpu.cu:224-556).  pot[n] in/out: comes back with the excluded units at -1 --
// excluded[i] != 0 (may be NULL), or a scale outside [0.2, 5].  w[n] in/out: the weights.  var_floor: the least variance of a class
// (each form rounds step^2 / 6.28 its own way: the caller's).
template <class Gauss>
void unit_em(int n, float *pot, float *w, const float *scale, const unsigned char *excluded, double var_floor, UnitClasses &c,
             const Gauss &gauss) {
  for (int i = 0; i < n; ++i)
    if ((excluded && excluded[i]) || scale[i] < 0.2 || scale[i] > 5) pot[i] = -1;

  ClassSums s;                                         // the class means
  double top = 0, bottom = 1;
  for (int i = 0; i < n; ++i)
    if (pot[i] >= 0) {
      s.in += pot[i] * w[i];
      s.in_w += w[i];
      s.out += pot[i] * (1.0 - w[i]);
      s.out_w += (1.0 - w[i]);
      if (pot[i] > top) top = pot[i];
      if (pot[i] < bottom) bottom = pot[i];
    }
  c.mean = s.in_w > 0 ? (float)(s.in / s.in_w) : (float)bottom;
  c.mean2 = s.out_w > 0 ? (float)(s.out / s.out_w) : (float)((top + c.mean) / 2.0);

  ClassSums v;                                         // the class variances
  for (int i = 0; i < n; ++i)
    if (pot[i] >= 0) {
      v.in += (pot[i] - c.mean) * (pot[i] - c.mean) * w[i];
      v.in_w += w[i];
      v.out += (pot[i] - c.mean2) * (pot[i] - c.mean2) * (1 - w[i]);
      v.out_w += (1 - w[i]);
    }
  c.var = 0.025f;
  if (v.in > 0 && v.in_w > 0) {
    c.var = (float)(v.in / v.in_w);
    if (c.var < var_floor) c.var = (float)var_floor;
  }
  c.var2 = v.out > 0 && v.out_w > 0 ? (float)(v.out / v.out_w) : (c.mean2 - c.mean) * (c.mean2 - c.mean) / 4;
  if (c.var2 < var_floor) c.var2 = (float)var_floor;

  const bool one_class = v.in_w <= 0 || c.mean2 <= c.mean;   // every unit that takes part is an inlier
  for (int i = 0; i < n; ++i) {
    const float p = pot[i];
    if (p == -1) { w[i] = 0; continue; }
    if (one_class) { w[i] = 1; continue; }
    const double g_in = p < c.mean2 ? gauss(p - c.mean, c.var) : 0;
    const double g_out = p > c.mean ? gauss(p - c.mean2, c.var2) : 0;
    const double likelihood = g_in * c.mix + g_out * (1 - c.mix);
    if (likelihood > 0) w[i] = (float)(g_in * c.mix / likelihood);
    else if (p >= c.mean2) w[i] = 0;                                      // both underflow: by where the unit lies
    else if (p <= c.mean || (p > c.mean && p < c.mean2)) w[i] = 1;        // (NaNs keep the weight)
  }

  double inliers = 0;
  int m = 0;
  for (int i = 0; i < n; ++i)
    if (pot[i] >= 0) { inliers += w[i]; ++m; }
  c.mix = m > 0 ? (float)(inliers / m) : 0.9f;
}

// Where the patch form reads each unit's potential: the reference copies the potentials of stack k to the patch indices
// 0 .. count[k]-1, without the stack's offset, a later stack overwriting an earlier one (patchBasedRobustStatistics_gpu.cu:256-276).
// src[i] = the index of the potential unit i ends up with, -1 = none (0).  The device EM reads the same map (svr_slice_em_set_patch_form).
inline std::vector<int> stack_potential_sources(const std::vector<int> &counts) {
  int n = 0;
  for (int k : counts) n += k;
  std::vector<int> src(n, -1);
  int ofs = 0;
  for (int k : counts) {
    for (int j = 0; j < k; ++j) src[j] = ofs + j;
    ofs += k;
  }
  return src;
}
// pot read through src (empty: each unit its own)
inline std::vector<float> gather_potentials(const std::vector<int> &src, const std::vector<float> &pot) {
  if (src.empty()) return pot;
  std::vector<float> out(src.size());
  for (size_t i = 0; i < src.size(); ++i) out[i] = src[i] < 0 ? 0.0f : pot[src[i]];
  return out;
}

// ---- the state both host objects own -------------------------------------------------------------------------------------------
struct UnitState {
  svr_ctx *e = nullptr;
  Shard sh;                            // this rank's unit range, the collectives, the one exchange per step (svr_shard.h)
  int n = 0, lo = 0, hi = 0;           // units: global count, this rank's range
  std::string err;

  // the form: set by the owner
  bool slice_form = false;             // slices: slice_inside is part of the state, and the M-step's calls differ (mstep_now)
  double step = 0;                     // the M-step's and the device EM's step
  double var_floor = 0;                // unit_em's least class variance
  std::vector<int> src;                // where unit i's potential comes from (stack_potential_sources); empty: unit i

  // the unit vectors, GLOBAL on every rank, and the eight scalars: the voxel-level EM's (sigma, mix, m) and the unit-level EM's
  std::vector<float> scale, weight, potential;
  std::vector<unsigned char> inside;   // slices only
  float sigma = 0, mix = 0, m = 0;
  UnitClasses cls = {0, 0, 0, 0, 0};

  // SVR_DEVICE_SLICE_EM: the unit-level EM on the device.  SVR_DEVICE_EM: a sharded M-step's sums meet on the device.
  bool dev_unit_em = true, device_em = true;

  void init(svr_ctx *engine, int n_global, int lo_, int hi_, const svr_collectives *c, bool slices) {
    e = engine; n = n_global; lo = lo_; hi = hi_; slice_form = slices;
    sh.init(engine, n_global, lo_, hi_, c);
    if (const char *v = getenv("SVR_DEVICE_SLICE_EM")) dev_unit_em = atoi(v) != 0;
    if (const char *v = getenv("SVR_DEVICE_EM")) device_em = atoi(v) != 0;
    scale.assign(n, 1.0f);
    weight.assign(n, 1.0f);
    potential.assign(n, 0.0f);
    if (slice_form) inside.assign(n, 1);
  }

  int fail(int rc, const char *what) {
    err = std::string(what) + ": " + (rc >= 10000 || rc < 0 ? "" : "hip error ") + std::to_string(rc) + " " + svr_last_error(e);
    return rc;
  }
#define UENG(call) do { int rc_ = (call); if (rc_) return fail(rc_, #call); } while (0)

  // -- the numbering ---------------------------------------------------------------------------------------------------------
  // The numbering of a sharded run need not be the reference's (set_order): a launcher that deals the r-th part of EVERY stack to rank
  // r (spatially compact shards, sharding.shard_units / svr_shard.h spatial_order) uploads the units rank after rank.  order[k] = the
  // reference's index of unit k of this object's numbering; empty = the same numbering.  Everything per unit is indifferent to the
  // numbering; what the reference does ACROSS units -- the sums of the unit-level EM, and the patch form's within-stack indexing of the
  // potentials, which only means something in its own numbering -- is done in the reference's order (to_ref / from_ref), so a permuted
  // run adds the same numbers in the same order as an unpermuted one.
  std::vector<int> order;
  template <class T> std::vector<T> to_ref(const std::vector<T> &v) const {
    if (order.empty()) return v;
    std::vector<T> r(v.size());
    for (size_t k = 0; k < v.size(); ++k) r[order[k]] = v[k];
    return r;
  }
  template <class T> std::vector<T> from_ref(const std::vector<T> &r) const {
    if (order.empty()) return r;
    std::vector<T> v(r.size());
    for (size_t k = 0; k < r.size(); ++k) v[k] = r[order[k]];
    return v;
  }
  // a new numbering (NULL: the reference's); one that is not a permutation changes nothing
  int set_order(const int *order_or_null, const char *what) {
    if (order_or_null) {
      std::vector<char> seen(n, 0);
      for (int k = 0; k < n; ++k) {
        const int i = order_or_null[k];
        if (i < 0 || i >= n || seen[i]) { err = what; return SVR_E_ARG; }
        seen[i] = 1;
      }
    }
    if (int rc = settle()) return rc;                  // (the device's copy of the state, if it is the current one, in the old numbering)
    if (order_or_null) order.assign(order_or_null, order_or_null + n);
    else order.clear();
    sem_ready = false;                                 // the device-side EM learns the new numbering at its next use
    return SVR_OK;
  }

  // -- the unit-level EM on the device (csrc/svr_em.inc) ---------------------------------------------------------------------
  // The host half of the E-step -- potentials down, the two-class EM over the units, weights up -- was the one wait of an SR iteration
  // and, sharded, its one host exchange.  With SVR_DEVICE_SLICE_EM (default on; sharded: when the launcher supplies allgather_device)
  // the E-step's potentials, the scale vector [and slice_inside] of every rank meet on the device (one all-gather of 3 x maxn floats)
  // and the EM runs there as one workgroup: an SR iteration only queues launches.  `on_host` says whose copy of the state (the unit
  // vectors, the eight scalars) is current: pull_state() brings the device's over in one wait when somebody reads it, push_state()
  // sends the host's when the host changed it.
  bool sem_ready = false, on_host = true;
  bool use_device_unit_em() const { return dev_unit_em && device_em && (!sh.on || sh.coll.allgather_device); }
  int push_state(const std::vector<unsigned char> &excluded) {
    if (!sem_ready) {
      const int W = sh.on ? sh.coll.world : 1, R = sh.on ? sh.coll.rank : 0;
      std::vector<double> b((size_t)W + 1, 0.0);      // every rank's range of this numbering: one small exchange, once
      b[R] = lo;
      if (R == W - 1) b[W] = hi;
      if (sh.on && W > 1) UENG(sh.coll.allreduce_host(sh.coll.user, b.data(), W + 1, 0));
      std::vector<int> rlo((size_t)W + 1);
      for (int r = 0; r <= W; ++r) rlo[r] = (int)b[r];
      UENG(svr_slice_em_setup(e, n, W, R, rlo.data(), order.empty() ? nullptr : order.data(), step));
      if (!src.empty()) UENG(svr_slice_em_set_patch_form(e, src.data()));
      sem_ready = true;
      on_host = true;
    }
    if (on_host) {
      const double s5[5] = {cls.mean, cls.mean2, cls.var, cls.var2, cls.mix};
      const float em3[3] = {sigma, mix, m};
      UENG(svr_slice_em_set_state(e, weight.data(), excluded.data(), s5, em3));
    }
    return 0;
  }
  int pull_state() {
    if (on_host) return 0;
    double s5[5];
    float em3[3];
    UENG(svr_slice_em_fetch(e, scale.data(), weight.data(), potential.data(), slice_form ? inside.data() : nullptr, s5, em3));
    cls = {(float)s5[0], (float)s5[1], (float)s5[2], (float)s5[3], (float)s5[4]};
    sigma = em3[0]; mix = em3[1]; m = em3[2];
    on_host = true;
    return 0;
  }
  // the weights for the scatter: this rank's part of the host's, or NULL = keep the device EM's (whatever anybody sent the engine in
  // between is replaced by them, device to device)
  int scatter_weights(const float **w) {
    *w = on_host ? weight.data() + lo : nullptr;
    if (!*w) UENG(svr_slice_em_apply_weights(e));
    return 0;
  }

  // -- host-side bookkeeping -------------------------------------------------------------------------------------------------
  // One rank, nothing to exchange: the scale vector, slice_inside and the M-step's scalars stay on the device until the E-step fetches
  // them with its potentials in one wait (svr_mstep_estep) -- one wait per SR iteration instead of four.  `settle` brings over whatever
  // is still there when something else wants to read it.  Sharded, the n-sized vectors a rank holds only its own part of (`*_stale`)
  // ride along with the next exchange that every rank makes anyway (Shard::exchange: one collective): the M-step's sums, the E-step's
  // potentials, the robust-statistics sums.
  bool scale_pending = false, inside_pending = false, scale_stale = false, inside_stale = false;
  int mstep_pending = 0;                               // iteration number of an M-step not yet run, or 0

  //   mine[n_mine] -> all[world][n_mine];  pot (or NULL): the potentials, this rank's range filled -> complete
  int exchange(const double *mine, int n_mine, std::vector<double> &all, std::vector<float> *pot) {
    if (int rc = settle()) return rc;                  // this rank's own parts of the vectors that travel
    std::vector<float> in;
    if (inside_stale) in.assign(inside.begin(), inside.end());
    std::vector<float> *vec[3] = {scale_stale ? &scale : nullptr, inside_stale ? &in : nullptr, pot};
    const int rc = sh.exchange(mine, n_mine, all, vec);
    if (rc) { err = rc == SVR_E_STATE ? "exchange: the ranks are not in the same step of the reconstruction" : "exchange: the collective failed"; return rc; }
    if (inside_stale) for (int i = 0; i < n; ++i) inside[i] = in[i] > 0.5f;
    scale_stale = inside_stale = false;
    return 0;
  }
  // this rank's part of the vectors that were pending, as the device returned them
  void take_pending(const std::vector<float> &sc, const std::vector<unsigned char> &in) {
    if (scale_pending) std::copy(sc.begin(), sc.end(), scale.begin() + lo);
    if (inside_pending) for (int i = 0; i < hi - lo; ++i) inside[lo + i] = in[i] != 0;
    scale_pending = inside_pending = false;
  }
  int settle() {
    if (int rc = pull_state()) return rc;              // (the device's unit-level state, if it is the current one)
    if (mstep_pending) {
      const int iter = mstep_pending;
      mstep_pending = 0;
      if (int rc = mstep_now(iter)) return rc;         // (sharded: collective, the ranks run the same operator sequence)
    }
    if (scale_pending) {
      UENG(svr_get_scale_vector(e, scale.data() + lo));
      scale_pending = false;
    }
    if (inside_pending) {
      std::vector<unsigned char> in(hi - lo);
      UENG(svr_get_slice_inside(e, in.data()));
      for (int i = 0; i < hi - lo; ++i) inside[lo + i] = in[i] != 0;
      inside_pending = false;
    }
    return 0;
  }
  // completes the vectors of which a rank only holds its own part (collective: every rank calls it); the state getters do
  int flush() {
    if (int rc = settle()) return rc;
    if (!sh.on || (!scale_stale && !inside_stale)) return 0;
    std::vector<double> none;
    return exchange(nullptr, 0, none, nullptr);
  }

  int init_em_values() {
    if (int rc = settle()) return rc;
    weight.assign(n, 1.0f);
    scale.assign(n, 1.0f);
    UENG(svr_update_scale_vector(e, scale.data() + lo, weight.data() + lo));
    UENG(svr_initialize_em_values(e));
    return 0;
  }

  // -- the M-step ------------------------------------------------------------------------------------------------------------
  // iter > 0 runs with the E-step that follows (one rank; sharded: when the ranks' sums can meet on the device there), or in settle
  int mstep(int iter) {
    if (iter > 0 && (!sh.on || (device_em && sh.coll.allgather_device))) {
      if (mstep_pending) { if (int rc = settle()) return rc; }   // (an M-step after an M-step; the vectors stay pending for the fused fetch)
      mstep_pending = iter;
      return 0;
    }
    if (slice_form && !sh.on) { if (int rc = settle()) return rc; }   // (the host's sigma / mix are the engine's M-step's inputs)
    return mstep_now(iter);
  }
  // Slices on one rank: the engine's M-step.  Otherwise: this rank's five sums [+ one exchange], the scalars on the host (the slice
  // form clamps the extremes to the float range first).
  int mstep_now(int iter) {
    if (slice_form && !sh.on) { UENG(svr_mstep(e, iter, (float)step, &sigma, &mix, &m)); return 0; }
    if (!slice_form) { if (int rc = pull_state()) return rc; }
    double s5[5];
    {
      std::vector<float> sc(scale_pending ? hi - lo : 0);
      std::vector<unsigned char> in(inside_pending ? hi - lo : 0);
      UENG(svr_mstep_sums_fetch(e, s5, scale_pending ? sc.data() : nullptr, inside_pending ? in.data() : nullptr));
      take_pending(sc, in);
    }
    if (sh.on) {
      std::vector<double> all;
      if (int rc = exchange(s5, 5, all, nullptr)) return rc;   // three sums, a minimum, a maximum: one collective
      s5[0] = s5[1] = s5[2] = 0;
      for (int r = 0; r < sh.coll.world; ++r) {              // rank order: the same bits everywhere
        for (int k = 0; k < 3; ++k) s5[k] += all[5 * r + k];
        s5[3] = r ? std::min(s5[3], all[5 * r + 3]) : all[3];
        s5[4] = r ? std::max(s5[4], all[5 * r + 4]) : all[4];
      }
    }
    const float s_sigma = (float)s5[0], s_mix = (float)s5[1], s_num = (float)s5[2];
    float mn = (float)s5[3], mx = (float)s5[4];
    if (slice_form) { mn = std::min(FLT_MAX, mn); mx = std::max(FLT_MIN, mx); }
    const float fstep = (float)step;
    if (s_mix > 0) sigma = s_sigma / s_mix;
    if (sigma < fstep * fstep / 6.28f) sigma = fstep * fstep / 6.28f;
    if (iter > 1) mix = s_mix / s_num;
    m = 1.0f / (mx - mn);
    return 0;
  }

  // -- the E-step ------------------------------------------------------------------------------------------------------------
  // [the pending M-step +] the voxel posteriors, then the unit-level EM: on the device (no wait, no host exchange) or on the host
  // (unit_em).  excluded[n]: the units of this numbering that the EM leaves out.
  template <class Gauss> int estep(const Gauss &gauss, const std::vector<unsigned char> &excluded) {
    void *send = nullptr, *recv = nullptr;
    if (use_device_unit_em()) {
      if (int rc = push_state(excluded)) return rc;
      const int iter = mstep_pending;
      mstep_pending = 0;
      if (iter > 0 && sh.on) {                         // the ranks' M-step sums meet on the device
        UENG(svr_mstep_partial(e, sh.coll.world, &send, &recv));
        if (int rc = sh.before_device_collective()) return fail(rc, "svr_stream_sync");
        if (int rc = sh.coll.allgather_device(sh.coll.user, send, recv, 16)) return fail(rc, "allgather_device (M-step sums)");
      }
      size_t nf = 0;
      UENG(svr_mstep_estep_device(e, iter, (float)step, &send, &recv, &nf));
      if (sh.on) {                                     // every rank's potentials, scales [and slice_inside]: one all-gather of 3 x maxn floats
        if (int rc = sh.before_device_collective()) return fail(rc, "svr_stream_sync");
        if (int rc = sh.coll.allgather_device(sh.coll.user, send, recv, nf)) return fail(rc, "allgather_device (unit potentials)");
      }
      UENG(svr_slice_em_run(e));
      on_host = false;
      scale_pending = inside_pending = scale_stale = inside_stale = false;   // (they travelled with the gather)
      return 0;
    }
    std::vector<float> pot(n, 0.0f);
    if (const int iter = mstep_pending) {
      // M-step + E-step + whatever is still on the device, one wait.  Sharded, the ranks' M-step sums meet ON THE DEVICE first (the
      // launcher's all-gather on the engine's stream) and are added up there in rank order: one wait and one host exchange (the
      // potentials') per SR iteration instead of two of each.
      mstep_pending = 0;
      float em3[3] = {sigma, mix, m};
      std::vector<float> sc(scale_pending ? hi - lo : 0);
      std::vector<unsigned char> in(inside_pending ? hi - lo : 0);
      float *psc = scale_pending ? sc.data() : nullptr;
      unsigned char *pin = inside_pending ? in.data() : nullptr;
      if (sh.on) {
        UENG(svr_mstep_partial(e, sh.coll.world, &send, &recv));
        if (int rc = sh.before_device_collective()) return fail(rc, "svr_stream_sync");
        if (int rc = sh.coll.allgather_device(sh.coll.user, send, recv, 16)) return fail(rc, "allgather_device (M-step sums)");
        UENG(svr_mstep_estep_ranks(e, sh.coll.world, iter, (float)step, em3, pot.data() + lo, psc, pin));
      } else {
        UENG(svr_mstep_estep(e, iter, (float)step, em3, pot.data() + lo, psc, pin));
      }
      sigma = em3[0]; mix = em3[1]; m = em3[2];
      take_pending(sc, in);
    } else {
      if (int rc = settle()) return rc;
      UENG(svr_estep(e, m, sigma, mix, pot.data() + lo));
    }
    if (sh.on) { std::vector<double> none; if (int rc = exchange(nullptr, 0, none, &pot)) return rc; }   // (and the scale vector)
    // the EM in the reference's unit order (the identity unless set_order)
    std::vector<float> p = gather_potentials(src, to_ref(pot));
    std::vector<float> w = to_ref(weight);
    const std::vector<float> sc = to_ref(scale);
    const std::vector<unsigned char> ex = to_ref(excluded);
    unit_em(n, p.data(), w.data(), sc.data(), ex.data(), var_floor, cls, gauss);
    weight = from_ref(w);
    potential = from_ref(p);
    if (slice_form) UENG(svr_update_slice_weights(e, weight.data() + lo));
    else UENG(svr_update_scale_vector(e, scale.data() + lo, weight.data() + lo));   // (patches: the scales go down with the weights)
    return 0;
  }

  // {sigma, mix, m, mean, mean2, var, var2, mix of the units}: the order of svrh_get_state / pvrh_get_state
  void scalars(double s[8]) const {
    const double v[8] = {sigma, mix, m, cls.mean, cls.mean2, cls.var, cls.var2, cls.mix};
    for (int k = 0; k < 8; ++k) s[k] = v[k];
  }
#undef UENG
};

}  // namespace svr
#endif
