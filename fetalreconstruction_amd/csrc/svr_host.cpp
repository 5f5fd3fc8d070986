// svr_host.cpp -- svr::irtkReconstruction: the reference's host algorithm object (GPU operator
// surface of irtkReconstruction, irtkReconstructionGPU.cc = "RG.cc") in C++ above the C-ABI engine.
// Plain host C++: no HIP calls here, everything device-side goes through include/svr_hip.h.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "../../include/svr_host.h"
#include "svr_unit_em.h"

namespace svr {

class irtkReconstruction {
 public:
  // engine + the unit-level state (svr_unit_em.h: the slices' vectors and EM scalars, the numbering, the device EM, the exchanges)
  svr_ctx *reconstructionGPU;          // RG.h: Reconstruction* reconstructionGPU
  int ns, lo, hi;
  UnitState em;
  Shard &sh = em.sh;                   // this rank's slice range, the collectives, the one exchange per step (svr_shard.h)
  std::string &err = em.err;

  // members named as in RG.h / RG.cc:159-221
  double _step;
  int _quality_factor;
  float _sigma_bias;
  double _delta, _lambda, _alpha;
  float _low_intensity_cutoff;
  bool _global_bias_correction, _adaptive, _disableBiasC;
  bool _intensity_matching;            // reconstruction.cc:114,183: false skips Bias / Scale / NormaliseBias in every SR iteration
  double _max_intensity, _min_intensity;
  std::vector<int> _force_excluded, _small_slices;

  irtkReconstruction(svr_ctx *engine, int n_global, int lo_, int hi_, const svr_collectives *c)
      : reconstructionGPU(engine), ns(n_global), lo(lo_), hi(hi_) {
    em.init(engine, n_global, lo_, hi_, c, true);
    _step = 0.0001;
    em.step = _step;
    em.var_floor = _step * _step / 6.28;
    _quality_factor = 2;
    _sigma_bias = 12;
    em.cls.var = 0.025f;
    em.cls.var2 = 0.025f;
    em.cls.mix = 0.9f;
    em.mix = 0.9f;
    _delta = 1;
    _lambda = 0.1f;
    _alpha = (0.05f / _lambda) * _delta * _delta;
    _low_intensity_cutoff = 0.01f;
    _global_bias_correction = false;
    _adaptive = false;
    _disableBiasC = true;   // reconstruction.cc:121,202
    _intensity_matching = true;
    _max_intensity = 1; _min_intensity = 0;
  }

#define ENG(call) do { int rc_ = (call); if (rc_) return em.fail(rc_, #call); } while (0)
  const float *local(const std::vector<float> &v) const { return v.data() + lo; }

  // the slices the slice-level EM leaves out, in this object's numbering
  std::vector<unsigned char> excluded() const {
    std::vector<unsigned char> x(ns, 0);
    for (int i : _force_excluded) if (i >= 0 && i < ns) x[i] = 1;
    for (int i : _small_slices) if (i >= 0 && i < ns) x[i] = 1;
    for (size_t i = 0; i < _st_in_force.size(); ++i) if (_st_in_force[i]) x[i] = 1;
    return x;
  }

  // ---- structural slice exclusion (--structural; not in the reference: include/svr_host.h) ---------------------
  bool _structural = false;
  int _st_radius = 3, _st_min_pixels = 25;
  double _st_k_mad = 3, _st_min_drop = 0.1;
  std::vector<int> _st_stack;                          // the stack of every slice, this object's numbering
  std::vector<unsigned char> _st_in_force, _st_pending;
  std::vector<double> _st_q, _st_n;                    // the last evaluation: mean SSIM (nan: not judged) and the pixels counted

  int StructuralEvaluate() {
    if (!_structural) { err = "svrh_structural_evaluate: svrh_set_structural first"; return SVR_E_STATE; }
    if (int rc = em.flush()) return rc;                // (settle: the device's scale vector is the newest; sharded: every rank's slice_inside)
    const double L = _max_intensity - _min_intensity, c1 = (0.01 * L) * (0.01 * L), c2 = (0.03 * L) * (0.03 * L);
    std::vector<double> sums(2 * (size_t)ns, 0.0);
    const auto t0 = std::chrono::steady_clock::now();
    if (hi > lo) ENG(svr_slice_ssim(reconstructionGPU, _st_radius, c1, c2, sums.data() + 2 * (size_t)lo, nullptr));
    if (getenv("SVR_CLI_TIMING"))                      // (the call blocks: the host clock around it is its cost)
      fprintf(stderr, "[timing] svr_slice_ssim, %d slices, radius %d: %.3f ms (host clock)\n", hi - lo, _st_radius,
              1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    if (sh.on) ENG(sh.coll.allreduce_host(sh.coll.user, sums.data(), 2 * ns, 0));   // one non-zero contributor per entry: exact
    std::vector<unsigned char> eligible(ns);
    for (int i = 0; i < ns; ++i) eligible[i] = em.inside[i] ? 1 : 0;
    for (int i : _force_excluded) if (i >= 0 && i < ns) eligible[i] = 0;
    for (int i : _small_slices) if (i >= 0 && i < ns) eligible[i] = 0;
    _st_q.assign(ns, 0.0);
    _st_pending.assign(ns, 0);
    for (int i = 0; i < ns; ++i) _st_n[i] = sums[2 * (size_t)i];
    if (int rc = svr_structural_decide(ns, _st_stack.data(), sums.data(), eligible.data(), _st_min_pixels, _st_k_mad, _st_min_drop,
                                       _st_q.data(), _st_pending.data())) {
      err = "svr_structural_decide: bad argument";
      return rc;
    }
    return 0;
  }

  // RG.h:605-612
  void SetSmoothingParameters(double delta, double lambda) {
    _delta = delta;
    _lambda = lambda * delta * delta;
    _alpha = 0.05 / lambda;
    if (_alpha > 1) _alpha = 1;
  }

  int InitializeEMValuesGPU() { return em.init_em_values(); }   // RG.cc:2905-2919

  // RG.cc:2695-2762.  voxel_num has one entry per device and its median indexes out of range for
  // one device (RG.cc:2714-2726), so no slice is ever "small" on the GPU path.
  int GaussianReconstructionGPU() {
    if (!sh.on) {
      int n = 0;
      ENG(svr_gaussian_reconstruction(reconstructionGPU, &n));
    } else {
      ENG(svr_gaussian_reconstruction_local(reconstructionGPU));
      ENG(sh.allreduce_pair(SVR_BUF_RECONSTRUCTED, 2 * svr_volume_voxels(reconstructionGPU)));
      int n = 0;
      ENG(svr_gaussian_reconstruction_finish(reconstructionGPU, &n));
    }
    _small_slices.clear();
    return 0;
  }

  // RG.cc:1163-1175.  Sharded: this rank's flags come over with the M-step's sums, the other ranks' with the exchange that follows.
  int SimulateSlicesGPU() {
    ENG(svr_simulate_slices(reconstructionGPU, nullptr));
    em.inside_pending = true;
    if (sh.on) em.inside_stale = true;
    return 0;
  }

  // RG.cc:2988-3019
  int InitializeRobustStatisticsGPU() {
    if (int rc = em.settle()) return rc;
    if (!sh.on) {
      ENG(svr_initialize_robust_statistics(reconstructionGPU, &em.sigma));
    } else {
      double s2[2], t[2] = {0, 0};
      ENG(svr_robust_statistics_sums(reconstructionGPU, s2));
      std::vector<double> all;
      ENG(em.exchange(s2, 2, all, nullptr));      // (brings the other ranks' slice_inside along)
      for (int r = 0; r < sh.coll.world; ++r) { t[0] += all[2 * r]; t[1] += all[2 * r + 1]; }
      em.sigma = (float)t[0] / (float)t[1];
    }
    for (int i = 0; i < ns; ++i)
      if (!em.inside[i]) em.weight[i] = 0;
    for (size_t i = 0; i < _force_excluded.size(); i++) em.weight[_force_excluded[i]] = 0;
    for (size_t i = 0; i < _st_in_force.size(); ++i) if (_st_in_force[i]) em.weight[i] = 0;   // --structural: as a force-excluded slice
    em.cls.var = 0.025f;
    em.mix = 0.9f;
    em.cls.mix = 0.9f;
    em.m = (float)(1.0f / (2.1f * _max_intensity - 1.9f * _min_intensity));
    ENG(svr_update_scale_vector(reconstructionGPU, local(em.scale), local(em.weight)));
    return 0;
  }

  // RG.cc:3184-3440: voxel posteriors on the GPU, the slice-level EM on the device or on the host (svr_unit_em.h)
  int EStepGPU() { return em.estep(SliceGauss{_step}, excluded()); }

  // RG.cc:3751-3757.  Fetched with the M-step's sums / the E-step's potentials, or by settle; sharded, read next in the E-step,
  // whose exchange completes it.
  int ScaleGPU() {
    ENG(svr_calculate_scale_vector(reconstructionGPU, nullptr));
    em.scale_pending = true;
    if (sh.on) em.scale_stale = true;
    return 0;
  }

  // RG.cc:4024-4036
  int SuperresolutionGPU(int iter) {
    const float *sw;
    if (int rc = em.scatter_weights(&sw)) return rc;
    if (!sh.on) {
      ENG(svr_superresolution(reconstructionGPU, iter, sw, _adaptive, (float)_alpha,
                              (float)_min_intensity, (float)_max_intensity, (float)_delta, (float)_lambda,
                              _global_bias_correction, _sigma_bias, _low_intensity_cutoff));
    } else {
      ENG(sh.superresolution(sw, _adaptive, (float)_alpha, (float)_min_intensity, (float)_max_intensity, (float)_delta,
                             (float)_lambda));
    }
    return 0;
  }

  // RG.cc:4214-4223 + Reconstruction::MStep host part (reconstruction_cuda2.cu:3016-3071)
  int MStepGPU(int iter) { return em.mstep(iter); }

  // RG.cc:3904-3913, 4653-4655
  int BiasGPU() { ENG(svr_correct_bias(reconstructionGPU, _sigma_bias, _global_bias_correction)); return 0; }
  int NormaliseBiasGPU(int iter) {
    if (!sh.on) { ENG(svr_normalise_bias(reconstructionGPU, iter, _sigma_bias)); return 0; }
    ENG(svr_normalise_bias_local(reconstructionGPU));
    // the bias volume is a single float[Nv] message
    ENG(sh.allreduce_pair(SVR_BUF_BIAS_VOLUME, svr_volume_voxels(reconstructionGPU)));
    ENG(svr_normalise_bias_finish(reconstructionGPU, _sigma_bias));
    return 0;
  }

  // A channel through this rank's slices with the weights SuperresolutionGPU would scatter with; sharded, num | den are then summed over
  // the ranks the way the non-slab SR update sums addon | cmap: every rank holds the same pair and finishes or votes on its own
  int ChannelReconstruct(const float *channel_local, const unsigned char *unit_on_local, int flags, float match) {
    const float *sw;
    if (int rc = em.scatter_weights(&sw)) return rc;
    ENG(svr_channel_scatter(reconstructionGPU, channel_local, unit_on_local, sw, flags, match));
    if (sh.on) ENG(sh.allreduce_pair(SVR_BUF_ADDON, 2 * svr_volume_voxels(reconstructionGPU)));
    return 0;
  }

  // n SR iterations on a channel (svr_channel_sr_*, include/svr_hip.h) with the weights ChannelReconstruct scatters with: the seed scatter and
  // every iteration's addon | cmap are summed over the ranks like ChannelReconstruct's pair, the volume update runs replicated on every rank.
  // delta_c / lambda_c become the engine's parameters the way SetSmoothingParameters makes the primary's.  guided: svr_channel_sr_guide after the
  // seed on every rank (guide_or_null = NULL: the rank's reconstruction, which every rank holds alike), so the replicated update stays replicated
  int ChannelSuperresolve(const float *channel_local, const unsigned char *unit_on_local, int n, double delta_c, double lambda_c, float clamp_lo, float clamp_hi,
                          float *out_or_null, bool guided = false, const float *guide_or_null = nullptr, double delta_g = 0, int guide_only = 0) {
    if (n < 0 || !std::isfinite(delta_c) || !(delta_c > 0) || !std::isfinite(lambda_c) || !(lambda_c > 0) || !(clamp_lo <= clamp_hi)) {
      err = "svrh_channel_superresolve: n >= 0, delta and lambda finite and positive, lo <= hi";
      return SVR_E_ARG;
    }
    if (guided && (!std::isfinite(delta_g) || !(delta_g > 0) || !std::isfinite((float)delta_g))) {
      err = "svrh_channel_superresolve_guided: delta_g finite and positive";
      return SVR_E_ARG;
    }
    const float *sw;
    if (int rc = em.scatter_weights(&sw)) return rc;
    const size_t pair = 2 * svr_volume_voxels(reconstructionGPU);
    const float alpha = (float)std::min(1.0, 0.05 / lambda_c), lambda_eng = (float)(lambda_c * delta_c * delta_c);
    double ms = 0;
    auto run = [&]() -> int {
      ENG(svr_channel_sr_begin(reconstructionGPU, channel_local, unit_on_local, sw, 0));
      if (sh.on) ENG(sh.allreduce_pair(SVR_BUF_ADDON, pair));
      ENG(svr_channel_sr_seed(reconstructionGPU, nullptr));
      if (guided) ENG(svr_channel_sr_guide(reconstructionGPU, guide_or_null, (float)delta_g, guide_only ? SVR_CHANNEL_GUIDE_ONLY : 0));
      const auto t0 = std::chrono::steady_clock::now();
      for (int k = 0; k < n; ++k) {
        ENG(svr_channel_sr_backproject(reconstructionGPU));
        if (sh.on) ENG(sh.allreduce_pair(SVR_BUF_ADDON, pair));
        ENG(svr_channel_sr_update(reconstructionGPU, _adaptive, alpha, clamp_lo, clamp_hi, (float)delta_c, lambda_eng));
      }
      ms = 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      ENG(svr_channel_sr_end(reconstructionGPU, out_or_null));
      return 0;
    };
    const int rc = run();
    if (rc) (void)svr_channel_sr_end(reconstructionGPU, nullptr);       // (the call is over either way: its buffers go, the message stays)
    else if (n > 0 && getenv("SVR_CLI_TIMING"))                           // (every engine call blocks: the host clock around them is their cost)
      fprintf(stderr, "[timing] channel SR iteration (gather, scatter%s, %supdate), %d slices: %.3f ms each over %d (host clock)\n",
              sh.on ? ", all-reduce" : "", guided ? "guided " : "", hi - lo, ms / n, n);
    return rc;
  }

  int MaskVolumeGPU() { ENG(svr_mask_volume(reconstructionGPU)); return 0; }   // RG.cc:5319-5323

  int ScaleVolumeGPU() {
    if (!sh.on) { ENG(svr_scale_volume(reconstructionGPU)); return 0; }
    double s2[2];
    ENG(svr_scale_volume_sums(reconstructionGPU, s2));
    ENG(sh.coll.allreduce_host(sh.coll.user, s2, 2, 0));
    ENG(svr_scale_volume_apply(reconstructionGPU, (float)(s2[0] / s2[1])));
    return 0;
  }

  // reconstruction.cc:1013-1108; the bias steps run when bias correction is enabled (svrh_set_bias_correction)
  int sr_iteration(int i) {
    int rc;
    if (_intensity_matching) {                                               // reconstruction.cc:1018-1045
      if (!_disableBiasC && _sigma_bias > 0)                                 // reconstruction.cc:1032-1037
        if ((rc = BiasGPU())) return rc;
      if ((rc = ScaleGPU())) return rc;
    }
    if ((rc = SuperresolutionGPU(i + 1))) return rc;
    if (_intensity_matching && !_disableBiasC && _sigma_bias > 0 && !_global_bias_correction)   // reconstruction.cc:1062-1076
      if ((rc = NormaliseBiasGPU(i))) return rc;
    if ((rc = SimulateSlicesGPU())) return rc;
    if ((rc = MStepGPU(i + 1))) return rc;
    return EStepGPU();
  }

  // ---- GPU slice-to-volume registration, host side ------------------------------------------
  struct M4 { double m[16]; };
  static M4 mul(const M4 &a, const M4 &b) {
    M4 c;
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) {
        double t = 0;
        for (int k = 0; k < 4; ++k) t += a.m[4 * i + k] * b.m[4 * k + j];
        c.m[4 * i + j] = t;
      }
    return c;
  }
  static M4 ident() { M4 c; for (int i = 0; i < 16; ++i) c.m[i] = (i % 5 == 0) ? 1.0 : 0.0; return c; }
  // irtkBaseImage::GetImageToWorldMatrix / GetWorldToImageMatrix (irtkBaseImage.cc:79-147)
  static M4 image_to_world(const svr_image_attr &a) {
    M4 t1 = ident(), sc = ident(), rot = ident(), t2 = ident();
    t1.m[3] = -(a.nx - 1) / 2.0; t1.m[7] = -(a.ny - 1) / 2.0; t1.m[11] = -(a.nz - 1) / 2.0;
    sc.m[0] = a.dx; sc.m[5] = a.dy; sc.m[10] = a.dz;
    for (int k = 0; k < 3; ++k) { rot.m[4 * k] = a.xaxis[k]; rot.m[4 * k + 1] = a.yaxis[k]; rot.m[4 * k + 2] = a.zaxis[k]; }
    for (int k = 0; k < 3; ++k) t2.m[4 * k + 3] = a.origin[k];
    return mul(t2, mul(rot, mul(sc, t1)));
  }
  static M4 world_to_image(const svr_image_attr &a) {
    M4 t1 = ident(), rot = ident(), sc = ident(), t2 = ident();
    for (int k = 0; k < 3; ++k) t1.m[4 * k + 3] = -a.origin[k];
    for (int k = 0; k < 3; ++k) { rot.m[k] = a.xaxis[k]; rot.m[4 + k] = a.yaxis[k]; rot.m[8 + k] = a.zaxis[k]; }
    sc.m[0] = 1.0 / a.dx; sc.m[5] = 1.0 / a.dy; sc.m[10] = 1.0 / a.dz;
    t2.m[3] = (a.nx - 1) / 2.0; t2.m[7] = (a.ny - 1) / 2.0; t2.m[11] = (a.nz - 1) / 2.0;
    return mul(t2, mul(sc, mul(rot, t1)));
  }
  static int irtk_round(double x) { return x > 0 ? (int)(x + 0.5) : (int)(x - 0.5); }   // irtkCommon.h:85-88

  std::vector<svr_image_attr> _slices_resampled_attr;   // attributes of `_slices_resampled` (RG.cc:2104-2119)
  std::vector<float> _reg_combined;                     // combinedStacks (RG.cc:2134-2160)
  int _reg_size[3] = {0, 0, 0};

  // irtkResamplingWithPadding<irtkRealPixel>(d, d, d, -1).Run() on one slice, plane 0 of the result
  // (IRTKSimple2/image++/src/irtkResamplingWithPadding.cc:198-252, 254-443)
  static void resample_plane0(const float *img, int row_pitch, const svr_image_attr &a, double d, svr_image_attr &oa,
                              std::vector<double> &out) {
    oa = a;
    oa.nx = irtk_round(a.nx * a.dx / d); oa.ny = irtk_round(a.ny * a.dy / d); oa.nz = irtk_round(a.nz * a.dz / d);
    oa.dx = oa.dy = oa.dz = d;
    if (oa.nx < 1) { oa.nx = 1; oa.dx = a.dx; }
    if (oa.ny < 1) { oa.ny = 1; oa.dy = a.dy; }
    if (oa.nz < 1) { oa.nz = 1; oa.dz = a.dz; }
    const M4 m = mul(world_to_image(a), image_to_world(oa));
    out.assign((size_t)oa.nx * oa.ny, -1.0);
    for (int j = 0; j < oa.ny; ++j)
      for (int i = 0; i < oa.nx; ++i) {
        const double x = m.m[0] * i + m.m[1] * j + m.m[3], y = m.m[4] * i + m.m[5] * j + m.m[7],
                     z = m.m[8] * i + m.m[9] * j + m.m[11];               // output k = 0
        const int u = (int)floor(x), v = (int)floor(y), w = (int)floor(z);
        const double fx = x - u, fy = y - v, fz = z - w;
        double val = 0, sum = 0;
        int pad = 8;
        for (int du = 0; du < 2; ++du)                                     // the reference's order w1..w8
          for (int dv = 0; dv < 2; ++dv)
            for (int dw = 0; dw < 2; ++dw) {
              const double wt = (du ? fx : 1 - fx) * (dv ? fy : 1 - fy) * (dw ? fz : 1 - fz);
              const int p = u + du, q = v + dv, r = w + dw;
              if (p >= 0 && p < a.nx && q >= 0 && q < a.ny && r >= 0 && r < a.nz) {
                const double g = img[(size_t)q * row_pitch + p];            // nz == 1
                if (g != -1.0) { --pad; val += g * wt; sum += wt; }
              } else {
                --pad;
              }
            }
        if (pad < 4 && sum > 0) out[(size_t)j * oa.nx + i] = val / sum;
      }
  }

  // PrepareRegistrationSlices RG.cc:2104-2181
  int PrepareRegistrationSlices(const float *slices, int sx, int sy, const svr_image_attr *attrs, double d) {
    const int n = hi - lo;
    _slices_resampled_attr.resize(n);
    std::vector<std::vector<double>> res(n);
    int mx = 0, my = 0;
    for (int i = 0; i < n; ++i) {
      if (attrs[i].nz != 1) { err = "PrepareRegistrationSlices: slices must have one plane"; return SVR_E_ARG; }
      resample_plane0(slices + (size_t)i * sx * sy, sx, attrs[i], d, _slices_resampled_attr[i], res[i]);
      mx = std::max(mx, _slices_resampled_attr[i].nx);
      my = std::max(my, _slices_resampled_attr[i].ny);
    }
    _reg_size[0] = mx; _reg_size[1] = my; _reg_size[2] = n;
    _reg_combined.assign((size_t)n * mx * my, -1.0f);                       // combinedStacks = -1 (RG.cc:2143)
    std::vector<float> i2w(16 * (size_t)n);
    for (int i = 0; i < n; ++i) {
      const svr_image_attr &a = _slices_resampled_attr[i];
      for (int y = 0; y < a.ny; ++y)
        for (int x = 0; x < a.nx; ++x)
          _reg_combined[((size_t)i * my + y) * mx + x] = (float)res[i][(size_t)y * a.nx + x];
      const M4 m = image_to_world(a);
      for (int k = 0; k < 16; ++k) i2w[16 * (size_t)i + k] = (float)m.m[k];
    }
    const uint32_t size[3] = {(uint32_t)mx, (uint32_t)my, (uint32_t)n};
    const float dim[3] = {(float)d, (float)d, (float)d};
    ENG(svr_init_reg_storage_volumes(reconstructionGPU, size, dim));
    ENG(svr_fill_reg_slices(reconstructionGPU, _reg_combined.data(), i2w.data()));
    return 0;
  }

  // SliceToVolumeRegistrationGPU RG.cc:2214-2290
  int SliceToVolumeRegistrationGPU(double *transformations) {
    const int n = hi - lo;
    if ((int)_slices_resampled_attr.size() != n) { err = "SliceToVolumeRegistrationGPU: PrepareRegistrationSlices first"; return SVR_E_STATE; }
    std::vector<float> transf(16 * (size_t)n), ofs(16 * (size_t)n);
    std::vector<M4> mos(n);
    for (int i = 0; i < n; ++i) {
      svr_image_attr a0 = _slices_resampled_attr[i];
      M4 mo = ident();
      for (int k = 0; k < 3; ++k) { mo.m[4 * k + 3] = a0.origin[k]; a0.origin[k] = 0.0; }   // RG.cc:2226-2236
      mos[i] = mo;
      M4 t;
      for (int k = 0; k < 16; ++k) t.m[k] = transformations[16 * (size_t)i + k];
      const M4 tm = mul(t, mo), o = image_to_world(a0);
      for (int k = 0; k < 16; ++k) { transf[16 * (size_t)i + k] = (float)tm.m[k]; ofs[16 * (size_t)i + k] = (float)o.m[k]; }
    }
    ENG(svr_update_resampled_slices_i2w(reconstructionGPU, ofs.data()));
    ENG(svr_prepare_slice_to_volume_reg(reconstructionGPU));
    ENG(svr_register_slices_to_volume(reconstructionGPU, transf.data()));
    for (int i = 0; i < n; ++i) {                                            // mat * mo^-1 (RG.cc:2262-2267)
      M4 t, moi = ident();
      for (int k = 0; k < 16; ++k) t.m[k] = (double)transf[16 * (size_t)i + k];
      for (int k = 0; k < 3; ++k) moi.m[4 * k + 3] = -mos[i].m[4 * k + 3];
      const M4 rres = mul(t, moi);
      for (int k = 0; k < 16; ++k) transformations[16 * (size_t)i + k] = rres.m[k];
    }
    return 0;
  }

  // reconstruction.cc:930-1140 (one outer iteration after registration)
  int reconstruct_iteration(int rec_iterations) {
    int rc;
    if (_structural) _st_in_force = _st_pending;         // what the last outer iteration found holds for this one
    if ((rc = InitializeEMValuesGPU())) return rc;
    if ((rc = GaussianReconstructionGPU())) return rc;
    if ((rc = SimulateSlicesGPU())) return rc;
    if ((rc = InitializeRobustStatisticsGPU())) return rc;
    if ((rc = EStepGPU())) return rc;
    for (int i = 0; i < rec_iterations; ++i)
      if ((rc = sr_iteration(i))) return rc;
    if (_structural && (rc = StructuralEvaluate())) return rc;   // (the slices were projected from the newest volume by the last SR iteration)
    return MaskVolumeGPU();
  }
#undef ENG
};

}  // namespace svr

struct svrh_recon {
  svr::irtkReconstruction impl;
  svrh_recon(svr_ctx *e, int n, int lo, int hi, const svr_collectives *c) : impl(e, n, lo, hi, c) {}
};

extern "C" {

svrh_recon *svrh_create(svr_ctx *engine, int n_slices_global, int slice_lo, int slice_hi,
                        const svr_collectives *coll) {
  if (!engine || n_slices_global <= 0 || slice_lo < 0 || slice_hi > n_slices_global || slice_lo > slice_hi) return nullptr;
  if (coll && coll->struct_size < SVR_COLLECTIVES_MIN_SIZE) return nullptr;      // (a launcher built against the struct of rounds 1-4)
  if (coll && coll->world > 1 && (!coll->allreduce_volume_pair || !coll->allreduce_host || !coll->allgather_slices))
    return nullptr;
  return new svrh_recon(engine, n_slices_global, slice_lo, slice_hi, coll);
}
void svrh_destroy(svrh_recon *r) { delete r; }
const char *svrh_last_error(const svrh_recon *r) { return r ? r->impl.err.c_str() : "null"; }
void svrh_set_intensity_range(svrh_recon *r, double mn, double mx) { r->impl._min_intensity = mn; r->impl._max_intensity = mx; }
void svrh_set_smoothing_parameters(svrh_recon *r, double delta, double lambda) { r->impl.SetSmoothingParameters(delta, lambda); }
void svrh_set_force_excluded(svrh_recon *r, const int *idx, int n) { (void)r->impl.em.settle(); r->impl._force_excluded.assign(idx, idx + n); }
int svrh_set_bias_correction(svrh_recon *r, int enable, double sigma_bias) {
  r->impl._disableBiasC = !enable;
  r->impl._sigma_bias = (float)sigma_bias;
  return svr_set_flags(r->impl.reconstructionGPU, !enable, 0);
}
int svrh_set_bias_options(svrh_recon *r, int global_bias_correction, double low_intensity_cutoff) {
  if (!r) return SVR_E_ARG;
  r->impl._global_bias_correction = global_bias_correction != 0;                      // GlobalBiasCorrectionOn/Off
  r->impl._low_intensity_cutoff = (float)std::min(1.0, std::max(0.0, low_intensity_cutoff));   // SetLowIntensityCutoff RG.h:596-602
  return SVR_OK;
}
int svrh_bias_gpu(svrh_recon *r) { return r->impl.BiasGPU(); }
int svrh_normalise_bias_gpu(svrh_recon *r, int iter) { return r->impl.NormaliseBiasGPU(iter); }
int svrh_channel_reconstruct(svrh_recon *r, const float *channel_local, const unsigned char *unit_on_local, int flags, float match) {
  if (!r) return SVR_E_ARG;
  return r->impl.ChannelReconstruct(channel_local, unit_on_local, flags, match);
}
int svrh_channel_superresolve(svrh_recon *r, const float *channel_local, const unsigned char *unit_on_local, int n, double delta_c, double lambda_c,
                              float lo, float hi, float *out_or_null) {
  if (!r) return SVR_E_ARG;
  return r->impl.ChannelSuperresolve(channel_local, unit_on_local, n, delta_c, lambda_c, lo, hi, out_or_null);
}
int svrh_channel_superresolve_guided(svrh_recon *r, const float *channel_local, const unsigned char *unit_on_local, int n, double delta_c, double lambda_c,
                                     float lo, float hi, float *out_or_null, const float *guide_or_null, double delta_g, int guide_only) {
  if (!r) return SVR_E_ARG;
  return r->impl.ChannelSuperresolve(channel_local, unit_on_local, n, delta_c, lambda_c, lo, hi, out_or_null, true, guide_or_null, delta_g, guide_only);
}
int svrh_initialize_em_values_gpu(svrh_recon *r) { return r->impl.InitializeEMValuesGPU(); }
int svrh_gaussian_reconstruction_gpu(svrh_recon *r) { return r->impl.GaussianReconstructionGPU(); }
int svrh_simulate_slices_gpu(svrh_recon *r) { return r->impl.SimulateSlicesGPU(); }
int svrh_initialize_robust_statistics_gpu(svrh_recon *r) { return r->impl.InitializeRobustStatisticsGPU(); }
int svrh_estep_gpu(svrh_recon *r) { return r->impl.EStepGPU(); }
int svrh_scale_gpu(svrh_recon *r) { return r->impl.ScaleGPU(); }
int svrh_superresolution_gpu(svrh_recon *r, int iter) { return r->impl.SuperresolutionGPU(iter); }
void svrh_set_intensity_matching(svrh_recon *r, int on) { if (r) r->impl._intensity_matching = on != 0; }
int svrh_mstep_gpu(svrh_recon *r, int iter) { return r->impl.MStepGPU(iter); }
int svrh_mask_volume_gpu(svrh_recon *r) { return r->impl.MaskVolumeGPU(); }
int svrh_scale_volume_gpu(svrh_recon *r) { return r->impl.ScaleVolumeGPU(); }
int svrh_sr_iteration(svrh_recon *r, int i) { return r->impl.sr_iteration(i); }
int svrh_reconstruct_iteration(svrh_recon *r, int n) { return r->impl.reconstruct_iteration(n); }

int svrh_set_structural(svrh_recon *r, int enable, int radius, double k_mad, double min_drop, int min_pixels, const int *stack_index_global) {
  if (!r) return SVR_E_ARG;
  svr::irtkReconstruction &o = r->impl;
  if (enable && (!stack_index_global || radius < 1 || radius > SVR_SSIM_MAX_RADIUS || !(k_mad >= 0.0) || !(min_drop >= 0.0) || min_pixels < 0)) {
    o.err = "svrh_set_structural: a stack index per slice, a radius of 1 .. 7 and a k, drop and pixel count that are not negative";
    return SVR_E_ARG;
  }
  o._structural = enable != 0;
  o._st_in_force.assign(o.ns, 0);
  o._st_pending.assign(o.ns, 0);
  o._st_q.assign(o.ns, NAN);
  o._st_n.assign(o.ns, 0.0);
  if (!enable) { o._st_in_force.clear(); return SVR_OK; }
  o._st_radius = radius; o._st_k_mad = k_mad; o._st_min_drop = min_drop; o._st_min_pixels = min_pixels;
  o._st_stack.assign(stack_index_global, stack_index_global + o.ns);
  return SVR_OK;
}
int svrh_structural_evaluate(svrh_recon *r) { return r ? r->impl.StructuralEvaluate() : SVR_E_ARG; }
int svrh_get_structural(svrh_recon *r, double *q, double *n_ssim, unsigned char *in_force, unsigned char *pending) {
  if (!r) return SVR_E_ARG;
  svr::irtkReconstruction &o = r->impl;
  if (!o._structural) { o.err = "svrh_get_structural: svrh_set_structural first"; return SVR_E_STATE; }
  if (q) std::copy(o._st_q.begin(), o._st_q.end(), q);
  if (n_ssim) std::copy(o._st_n.begin(), o._st_n.end(), n_ssim);
  if (in_force) std::copy(o._st_in_force.begin(), o._st_in_force.end(), in_force);
  if (pending) std::copy(o._st_pending.begin(), o._st_pending.end(), pending);
  return SVR_OK;
}

int svrh_prepare_registration_slices(svrh_recon *r, const float *slices, int sx, int sy, const svr_image_attr *attrs,
                                     double recon_voxel) {
  if (!r || !slices || !attrs || sx <= 0 || sy <= 0 || !(recon_voxel > 0)) return SVR_E_ARG;
  return r->impl.PrepareRegistrationSlices(slices, sx, sy, attrs, recon_voxel);
}
int svrh_slice_to_volume_registration_gpu(svrh_recon *r, double *transformations) {
  if (!r || !transformations) return SVR_E_ARG;
  return r->impl.SliceToVolumeRegistrationGPU(transformations);
}
int svrh_get_registration_slices(svrh_recon *r, int size3[3], float *data_or_null) {
  if (!r || !size3) return SVR_E_ARG;
  for (int k = 0; k < 3; ++k) size3[k] = r->impl._reg_size[k];
  if (data_or_null) std::copy(r->impl._reg_combined.begin(), r->impl._reg_combined.end(), data_or_null);
  return 0;
}

int svrh_set_unit_order(svrh_recon *r, const int *order_or_null) {
  return r ? r->impl.em.set_order(order_or_null, "svrh_set_unit_order: not a permutation of the slices") : SVR_E_ARG;
}
void svrh_force_collectives(svrh_recon *r, int on) { if (r) { (void)r->impl.em.settle(); r->impl.sh.force(on != 0); } }
void svrh_set_slab_update(svrh_recon *r, int on) { if (r) r->impl.sh.slabs = on != 0; }

int svrh_get_state(svrh_recon *r, float *scale, float *slice_weight, float *slice_potential,
                   unsigned char *slice_inside, double s[8]) {
  if (!r) return SVR_E_ARG;
  svr::UnitState &u = r->impl.em;
  if (int rc = u.flush()) return rc;   // sharded: the scale vector / slice_inside of the other ranks may still be on their way
  if (scale) std::copy(u.scale.begin(), u.scale.end(), scale);
  if (slice_weight) std::copy(u.weight.begin(), u.weight.end(), slice_weight);
  if (slice_potential) std::copy(u.potential.begin(), u.potential.end(), slice_potential);
  if (slice_inside) std::copy(u.inside.begin(), u.inside.end(), slice_inside);
  if (s) u.scalars(s);
  return SVR_OK;
}

}  // extern "C"
