// irtk_reg.cpp -- the reference's default (CPU / IRTK) rigid registration schedule around the batched NCC cost of the
// engine (SURVEY 8a16 + 8f1 "the IRTK schedule" + 8f2 "stack-to-stack registration"), host C++.
//
// Restated, each function citing the lines it follows (IRTK = source/IRTKSimple2, RG.cc = source/reconstructionGPU2/
// irtkReconstructionGPU.cc):
//   irtkImageRigidRegistrationWithPadding::GuessParameterThickSlices / GuessParameterSliceToVolume
//                                             IRTK/packages/registration/src/irtkImageRigidRegistrationWithPadding.cc:110-205, 304-400
//   irtkImageRegistrationWithPadding::Initialize(level)      .../src/irtkImageRegistrationWithPadding.cc:28-334
//   irtkImageRegistration::Run, EvaluateGradient             .../src/irtkImageRegistration.cc:414-568
//   irtkGradientDescentOptimizer::Run, irtkOptimizer::Run    .../src/irtkGradientDescentOptimizer.cc:25-69, irtkOptimizer.cc:107-131
//   irtkGaussianBlurringWithPadding, irtkConvolutionWithPadding_1D, irtkScalarGaussian
//                                             IRTK/image++/src/irtkGaussianBlurringWithPadding.cc:35-121, irtkConvolutionWithPadding_1D.cc:38-125
//   irtkResamplingWithPadding                 IRTK/image++/src/irtkResamplingWithPadding.cc:202-443
//   irtkRigidTransformation::UpdateMatrix / Matrix2Parameters   IRTK/packages/transformation/src/irtkRigidTransformation.cc:26-53, 119-148
//   irtkReconstruction::StackRegistrations (+ ParallelStackRegistrations, ResetOrigin, InvertStackTransformations)   RG.cc:823-1001
//   irtkReconstruction::SliceToVolumeRegistration (+ ParallelSliceToVolumeRegistration)                               RG.cc:1991-2059, 2291-2303
// The similarity itself (irtkImageRigidRegistrationWithPadding::Evaluate + irtkCrossCorrelationSimilarityMetric) is the
// engine's svr_ncc_evaluate: exact integer moments, so the accept / reject decisions of the optimiser do not depend on
// where the cost is evaluated.  With SVRH_SIM_NMI (the reference's --useNMI) it is irtkNormalisedMutualInformationSimilarity-
// Metric: the levels are binned (irtkCalculateNumberOfBins) and svr_nmi_evaluate returns integer joint histograms' entropy
// sums added in the reference's order, equal to nmi_sums below bit for bit -- the same guarantee.  With SVRH_SIM_LNCC (a
// deviation: the reference has no local metric) it is the windowed cross correlation of svr_lncc_evaluate, per plane the
// integers {N, S} added over the planes of an evaluation -- again independent of where it is evaluated.  All targets that share a source are optimised in lock step: one optimiser step of every
// target (its similarity, its 12 finite differences, or one line-search probe) is ONE batched evaluate call.  A 3-D target
// (a stack) is handed to the engine as its z-planes, each with the start position the reference's iterator reaches by
// repeated addition (irtkHomogeneousTransformationIterator.h:96-199), and the six moments are added up.
#include <float.h>
#include <stdint.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <map>
#include <tuple>
#include <condition_variable>
#include <mutex>
#include <thread>

#include "svr_prep.h"

namespace {

// Rows of an image, and the targets of a registration pass, are independent in every filter below: they are split over a
// pool of host threads that lives as long as the library (starting threads per call cost more than the 280 small pyramids
// of a slice-to-volume pass).  Results do not depend on the split.  A call from inside a pool task, or while another
// host thread (an in-process rank) owns the pool, runs inline.
class WorkPool {
 public:
  static WorkPool &get() { static WorkPool p; return p; }
  template <class F> void run(int n, int max_threads, F &fn) {
    // (a forked child inherits the object but not the threads: it works inline)
    if (n < 2 || max_threads < 2 || inside() || workers_->empty() || getpid() != pid_ || !owner_.try_lock()) { fn(0, n); return; }
    const int nt = std::min<int>({max_threads, (int)workers_->size() + 1, n});
    {
      std::lock_guard<std::mutex> g(m_);
      call_ = [](void *f, int a, int b) { (*static_cast<F *>(f))(a, b); };
      fn_ = &fn; n_ = n; chunk_ = std::max(1, n / (nt * 4)); next_ = 0; wanted_ = nt - 1; running_ = nt - 1; ++gen_;
    }
    cv_.notify_all();
    inside() = true;
    work();
    inside() = false;
    std::unique_lock<std::mutex> g(m_);
    done_.wait(g, [&] { return running_ == 0; });
    g.unlock();
    owner_.unlock();
  }
  int size() const { return (int)workers_->size() + 1; }

 private:
  WorkPool() {
    const int n = std::min(svr_host_threads(), 128);          // the CPUs this process may actually use (affinity, cgroup quota)
    pid_ = getpid();
    for (int i = 1; i < n; ++i) workers_->emplace_back([this] { loop(); });
  }
  ~WorkPool() {
    if (getpid() != pid_) return;                          // forked child: the thread objects name threads it never had (leaked on purpose)
    { std::lock_guard<std::mutex> g(m_); stop_ = true; }
    cv_.notify_all();
    for (auto &t : *workers_) t.join();
    delete workers_;
  }
  static bool &inside() { static thread_local bool in = false; return in; }
  void work() {
    for (;;) {
      const int a = next_.fetch_add(chunk_);
      if (a >= n_) break;
      call_(fn_, a, std::min(n_, a + chunk_));
    }
  }
  void loop() {
    inside() = true;
    uint64_t seen = 0;
    std::unique_lock<std::mutex> g(m_);
    for (;;) {
      cv_.wait(g, [&] { return stop_ || (gen_ != seen && wanted_ > 0); });
      if (stop_) return;
      seen = gen_;
      --wanted_;
      g.unlock();
      work();
      g.lock();
      if (--running_ == 0) done_.notify_one();
    }
  }
  std::vector<std::thread> *workers_ = new std::vector<std::thread>();
  std::mutex m_, owner_;
  std::condition_variable cv_, done_;
  void (*call_)(void *, int, int) = nullptr;
  void *fn_ = nullptr;
  int n_ = 0, chunk_ = 1, wanted_ = 0, running_ = 0;
  std::atomic<int> next_{0};
  uint64_t gen_ = 0;
  bool stop_ = false;
  pid_t pid_ = 0;
};
template <class F> void parallel_rows(int n, size_t work_per_row, F fn) {
  const int nt = (int)std::min<size_t>(128, (size_t)n * work_per_row / 50000 + 1);
  WorkPool::get().run(n, nt, fn);
}

template <class T> struct Vol {
  svr_image_attr a;
  std::vector<T> d;                                      // [z][y][x]
  T &at(int x, int y, int z) { return d[((size_t)z * a.ny + y) * a.nx + x]; }
  T at(int x, int y, int z) const { return d[((size_t)z * a.ny + y) * a.nx + x]; }
  size_t n() const { return (size_t)a.nx * a.ny * a.nz; }
};

template <class T> T put_as_double(double v);             // irtkGenericImage::PutAsDouble, irtkGenericImage.h:303-333
template <> short put_as_double<short>(double v) {
  if (v > 32767.0) v = 32767.0;
  if (v < -32768.0) v = -32768.0;
  return (short)v;                                        // static_cast: truncation
}
template <> double put_as_double<double>(double v) { return v; }

// irtkResamplingWithPadding<T>(rx, ry, rz, pad).Run(), RWP.cc:202-443
// the grid irtkResamplingWithPadding gives an image (RWP.cc:202-240)
svr_image_attr resampled_attr(const svr_image_attr &in, double rx, double ry, double rz) {
  svr_image_attr out = in;
  const double want[3] = {rx, ry, rz}, old[3] = {in.dx, in.dy, in.dz};
  const int n_old[3] = {in.nx, in.ny, in.nz};
  int n_new[3];
  double d_new[3];
  for (int k = 0; k < 3; ++k) {
    n_new[k] = (int)irtk_round(n_old[k] * old[k] / want[k]);
    d_new[k] = want[k];
    if (n_new[k] < 1) { n_new[k] = 1; d_new[k] = old[k]; }
  }
  out.nx = n_new[0]; out.ny = n_new[1]; out.nz = n_new[2];
  out.dx = d_new[0]; out.dy = d_new[1]; out.dz = d_new[2];
  return out;
}

template <class T> Vol<T> resample_with_padding(const Vol<T> &in, double rx, double ry, double rz, T pad) {
  Vol<T> out;
  out.a = resampled_attr(in.a, rx, ry, rz);
  out.d.assign(out.n(), pad);
  const M4 o_i2w = image_to_world(out.a), i_w2i = world_to_image(in.a);
  const int X = in.a.nx, Y = in.a.ny, Z = in.a.nz;
  parallel_rows(out.a.nz * out.a.ny, (size_t)out.a.nx * 40, [&](int r0, int r1) {
  for (int r = r0; r < r1; ++r) {
      const int k = r / out.a.ny, j = r % out.a.ny;
      for (int i = 0; i < out.a.nx; ++i) {
        // ImageToWorld then WorldToImage, two separate matrix applications like the reference
        const double wx = o_i2w.m[0] * i + o_i2w.m[1] * j + o_i2w.m[2] * k + o_i2w.m[3];
        const double wy = o_i2w.m[4] * i + o_i2w.m[5] * j + o_i2w.m[6] * k + o_i2w.m[7];
        const double wz = o_i2w.m[8] * i + o_i2w.m[9] * j + o_i2w.m[10] * k + o_i2w.m[11];
        const double x = i_w2i.m[0] * wx + i_w2i.m[1] * wy + i_w2i.m[2] * wz + i_w2i.m[3];
        const double y = i_w2i.m[4] * wx + i_w2i.m[5] * wy + i_w2i.m[6] * wz + i_w2i.m[7];
        const double z = i_w2i.m[8] * wx + i_w2i.m[9] * wy + i_w2i.m[10] * wz + i_w2i.m[11];
        const int u = (int)floor(x), v = (int)floor(y), w = (int)floor(z);
        const double dx = x - u, dy = y - v, dz = z - w;
        const double wt[8] = {(1 - dx) * (1 - dy) * (1 - dz), (1 - dx) * (1 - dy) * dz, (1 - dx) * dy * (1 - dz), (1 - dx) * dy * dz,
                              dx * (1 - dy) * (1 - dz),       dx * (1 - dy) * dz,       dx * dy * (1 - dz),       dx * dy * dz};
        static const int off[8][3] = {{0, 0, 0}, {0, 0, 1}, {0, 1, 0}, {0, 1, 1}, {1, 0, 0}, {1, 0, 1}, {1, 1, 0}, {1, 1, 1}};
        double val = 0, sum = 0;
        int npad = 8;
        for (int c = 0; c < 8; ++c) {
          const int a = u + off[c][0], b = v + off[c][1], e = w + off[c][2];
          if (a >= 0 && a < X && b >= 0 && b < Y && e >= 0 && e < Z) {
            const T g = in.at(a, b, e);
            if (g != pad) { npad--; val += g * wt[c]; sum += wt[c]; }
          } else {
            npad--;
          }
        }
        if (npad < 4 && sum > 0) out.at(i, j, k) = put_as_double<T>(val / sum);
      }
  }
  });
  return out;
}

// the sampled Gaussian of one pass of irtkGaussianBlurringWithPadding (GBWP.cc:60-120): sigma in mm, vs = the voxel size along the axis
std::vector<double> blur_kernel(double sigma, double vs) {
  const double s = sigma / vs;
  const int size = 2 * (int)irtk_round(4 * sigma / vs) + 1;
  std::vector<double> ker(size);                          // irtkScalarGaussian(s, 1, 1, 0, 0, 0) sampled at i - (size-1)/2
  const double norm = 1.0 / (sqrt(2.0 * M_PI) * s * sqrt(2.0 * M_PI) * 1 * sqrt(2.0 * M_PI) * 1);
  for (int i = 0; i < size; ++i) {
    const double x = i - (size - 1) / 2.0;
    ker[i] = norm * exp(-(x * x) / (2.0 * s * s) - 0.0 - 0.0);
    if (fabs(ker[i]) < FLT_MIN) ker[i] = 0;               // irtkScalarFunctionToImage.cc:89-92
  }
  return ker;
}

// irtkGaussianBlurringWithPadding<short>(sigma, pad).Run(): three 1-D passes, each rounded (truncated) back to short
void blur_with_padding(Vol<short> &im, double sigma, short pad) {
  const int n[3] = {im.a.nx, im.a.ny, im.a.nz};
  const double vs[3] = {im.a.dx, im.a.dy, im.a.dz};
  const ptrdiff_t stride[3] = {1, (ptrdiff_t)im.a.nx, (ptrdiff_t)im.a.nx * im.a.ny};
  for (int axis = 0; axis < 3; ++axis) {
    if (axis == 2 && im.a.nz == 1) continue;             // GBWP.cc:90
    const std::vector<double> ker = blur_kernel(sigma, vs[axis]);
    const int size = (int)ker.size(), half = size / 2;
    std::vector<short> out(im.d.size());
    parallel_rows(n[2] * n[1], (size_t)n[0] * size, [&](int r0, int r1) {
    for (int r = r0; r < r1; ++r) {
        const int z = r / n[1], y = r % n[1];
        for (int x = 0; x < n[0]; ++x) {
          const int p[3] = {x, y, z};
          const size_t base = ((size_t)z * n[1] + y) * n[0] + x;
          if (im.d[base] <= pad) { out[base] = pad; continue; }        // CWP_1D.cc:45
          double val = 0, sum = 0;
          for (int t = -half; t <= half; ++t) {
            const int q = p[axis] + t;
            if (q < 0 || q >= n[axis]) continue;
            const short g = im.d[base + t * stride[axis]];
            if (g > pad) { val += ker[t + half] * g; sum += ker[t + half]; }
          }
          out[base] = put_as_double<short>(sum > 0 ? val / sum : 0.0);
        }
    }
    });
    im.d.swap(out);
  }
}

// the eight-corner padding guess of GuessParameter*, IRRWP.cc:183-204
short guess_padding(const Vol<short> &v) {
  const int X = v.a.nx - 1, Y = v.a.ny - 1, Z = v.a.nz - 1;
  const short c = v.at(0, 0, 0);
  if (v.at(X, 0, 0) == c && v.at(0, Y, 0) == c && v.at(0, 0, Z) == c && v.at(X, Y, 0) == c && v.at(0, Y, Z) == c && v.at(X, 0, Z) == c &&
      v.at(X, Y, Z) == c)
    return c;
  return (short)-32768;                                    // MIN_GREY
}

// irtkCalculateNumberOfBins (irtkUtil.cc:438-474) with GuessParameterSliceToVolume's _NumberOfBins = 64 (IRRWP.cc:316), which
// Initialize(level) calls for NMI (IRWP.cc:239-246) with the range [mn, mx] of the level before its shift to 0: the smallest
// width that puts range = mx - mn + 1 into at most 64 bins.  A level without a voxel above the padding (mx < mn) has no
// samples; it gets one bin of width 1 (the reference would size its histogram by the negative range).
int nmi_number_of_bins(int mn, int mx, int &width) {
  const int range = mx - mn + 1;
  width = 1;
  if (range < 1) return 1;
  while ((int)ceil(range / (double)width) > 64) width++;
  return (int)ceil(range / (double)width);
}
void nmi_bin(short *d, size_t n, int width) {              // ... and its rescaling of the voxels
  for (size_t i = 0; i < n; ++i)
    if (d[i] > 0) d[i] = (short)(int)(d[i] / (double)width);
}
// The sums of irtkHistogram_2D::JointEntropy / EntropyX / EntropyY (H2D.cc:443-523) over h[source bin][target bin] (row pitch
// 64): {n, S_xy, S_x, S_y}, each S the serial sum of c log c over the nonzero bins in the reference's visit order.  The
// engine's entropy pass (csrc/svr_nmi.inc) adds the same terms, from a table of the same expression, in the same order.
void nmi_sums(const uint32_t *h, int nbt, int nbs, double out[4]) {
  auto term = [](uint64_t c) { return (double)c * log((double)c); };
  double sxy = 0, sx = 0, sy = 0;
  uint64_t n = 0;
  for (int j = 0; j < nbs; ++j)
    for (int i = 0; i < nbt; ++i) {
      const uint32_t c = h[j * 64 + i];
      if (c > 0) sxy += term(c);
      n += c;
    }
  for (int i = 0; i < nbt; ++i) {
    uint64_t m = 0;
    for (int j = 0; j < nbs; ++j) m += h[j * 64 + i];
    if (m > 0) sx += term(m);
  }
  for (int j = 0; j < nbs; ++j) {
    uint64_t m = 0;
    for (int i = 0; i < nbt; ++i) m += h[j * 64 + i];
    if (m > 0) sy += term(m);
  }
  out[0] = (double)n; out[1] = sxy; out[2] = sx; out[3] = sy;
}
// irtkHistogram_2D::NormalizedMutualInformation, H2D.cc:617-624: (EntropyX + EntropyY) / JointEntropy, entropy = -S / n + log(n)
double nmi_from_sums(const double s[4]) {
  const double n = s[0];
  if (n == 0) return 0;
  const double ex = -s[2] / n + log(n), ey = -s[3] / n + log(n), exy = -s[1] / n + log(n);
  return (ex + ey) / exy;
}

struct Schedule {                                          // GuessParameterThickSlices / GuessParameterSliceToVolume
  int levels = 3, iterations[3], steps[3];
  double epsilon = 0.0001, t_blur[3], s_blur[3], t_res[3][3], s_res[3][3], length[3], delta[3];
};

Schedule guess_parameters(const svr_image_attr &t, const svr_image_attr &s, int slice_to_volume) {
  Schedule p;
  double size = t.dy < t.dx ? t.dy : t.dx;
  p.t_blur[0] = size / 2.0;
  p.t_res[0][0] = size; p.t_res[0][1] = size; p.t_res[0][2] = t.dz;
  for (int i = 1; i < 3; ++i) {
    p.t_blur[i] = p.t_blur[i - 1] * 2;
    p.t_res[i][0] = p.t_res[i - 1][0] * 2; p.t_res[i][1] = p.t_res[i - 1][1] * 2; p.t_res[i][2] = p.t_res[i - 1][2];
  }
  size = s.dy < s.dx ? s.dy : s.dx;
  if (slice_to_volume && s.dz < size) size = s.dz;         // IRRWP.cc:355-356
  p.s_blur[0] = size / 2.0;
  p.s_res[0][0] = size; p.s_res[0][1] = size; p.s_res[0][2] = slice_to_volume ? size : s.dz;
  for (int i = 1; i < 3; ++i) {
    p.s_blur[i] = p.s_blur[i - 1] * 2;
    p.s_res[i][0] = p.s_res[i - 1][0] * 2; p.s_res[i][1] = p.s_res[i - 1][1] * 2;
    p.s_res[i][2] = slice_to_volume ? p.s_res[i - 1][2] * 2 : p.s_res[i - 1][2];
  }
  for (int i = 0; i < 3; ++i) { p.iterations[i] = 20; p.steps[i] = 4; p.length[i] = 2 * pow(2.0, i); p.delta[i] = 0; }
  return p;
}

// irtkImageRegistrationWithPadding::Initialize(level) for one image: blur, resample, shift the range, pad with -1
// (mn_out / mx_out: the range before the shift, max < min when no voxel is above the padding)
int prepare_level(const Vol<short> &in, double blur, const double res[3], const double res0[3], int level, short pad, Vol<short> &out,
                  std::string &err, int *mn_out = nullptr, int *mx_out = nullptr) {
  out = in;
  if (blur > 0) blur_with_padding(out, blur, pad);
  const double temp = fabs(res0[0] - out.a.dx) + fabs(res0[1] - out.a.dy) + fabs(res0[2] - out.a.dz);
  if (level > 0 || temp > 0.000001) out = resample_with_padding<short>(out, res[0], res[1], res[2], pad);
  double vmax = -32768.0, vmin = 32767.0;
  for (short &v : out.d) {
    if (v > pad) { if (v > vmax) vmax = v; if (v < vmin) vmin = v; }
    else v = pad;
  }
  if (vmax - vmin > 32767.0) { err = "Initialize: dynamic range of an image is too large"; return 1; }
  for (short &v : out.d) v = v > pad ? (short)(v - (short)vmin) : (short)-1;
  if (mn_out) *mn_out = (int)vmin;
  if (mx_out) *mx_out = (int)vmax;
  return 0;
}

// irtkRigidTransformation::UpdateMatrix, RT.cc:26-53
M4 params_to_matrix(const double p[6]) {
  const double k = M_PI / 180.0;
  const double cosrx = cos(p[3] * k), cosry = cos(p[4] * k), cosrz = cos(p[5] * k);
  const double sinrx = sin(p[3] * k), sinry = sin(p[4] * k), sinrz = sin(p[5] * k);
  M4 m = ident();
  m.m[0] = cosry * cosrz; m.m[1] = cosry * sinrz; m.m[2] = -sinry; m.m[3] = p[0];
  m.m[4] = (sinrx * sinry * cosrz - cosrx * sinrz); m.m[5] = (sinrx * sinry * sinrz + cosrx * cosrz); m.m[6] = sinrx * cosry; m.m[7] = p[1];
  m.m[8] = (cosrx * sinry * cosrz + sinrx * sinrz); m.m[9] = (cosrx * sinry * sinrz - sinrx * cosrz); m.m[10] = cosrx * cosry; m.m[11] = p[2];
  return m;
}

// irtkRigidTransformation::Matrix2Parameters, RT.cc:119-148
void matrix_to_params(const M4 &m, double p[6]) {
  const double TOL = 0.000001;
  p[0] = m.m[3]; p[1] = m.m[7]; p[2] = m.m[11];
  const double tmp = asin(-1 * m.m[2]);
  if (fabs(cos(tmp)) > TOL) {
    p[3] = atan2(m.m[6], m.m[10]);
    p[4] = tmp;
    p[5] = atan2(m.m[1], m.m[0]);
  } else {
    p[3] = atan2(-1.0 * m.m[2] * m.m[4], -1.0 * m.m[2] * m.m[8]);
    p[4] = tmp;
    p[5] = 0;
  }
  p[3] *= 180.0 / M_PI; p[4] *= 180.0 / M_PI; p[5] *= 180.0 / M_PI;
}

struct Backend {                                           // where the images go: the engine, or whatever the caller supplies
  svr_ctx *ctx;
  const svr_ncc_backend *be;
  const svr_nmi_backend *nbe = nullptr;                    // NMI: the caller's joint histograms instead of the engine's sums
  bool external() const { return be || nbe; }
  int set_targets(int n, int tx, int ty, const int16_t *t) const {
    return nbe ? nbe->set_targets(nbe->user, n, tx, ty, t) : be ? be->set_targets(be->user, n, tx, ty, t) : svr_ncc_set_targets(ctx, n, tx, ty, t);
  }
  int set_source(const uint32_t size[3], const int16_t *s) const {
    return nbe ? nbe->set_source(nbe->user, size, s) : be ? be->set_source(be->user, size, s) : svr_ncc_set_source(ctx, size, s);
  }
};

struct Target {                                            // one registration: a target image and its transformation
  const Vol<short> *full;                                  // the unprocessed target
  Vol<short> lvl;                                          // this level's image
  int first_plane = 0;                                     // index of its plane 0 among the backend's targets
  int own_padding = 0;                                     // 1: `padding` replaces the call's target padding (GuessParameter's corner rule)
  short padding = 0;
  int bin_width = 1, nbins = 1;                            // NMI: irtkCalculateNumberOfBins of this level
  M4 matrix;                                               // irtkRigidTransformation::_matrix
  double p[6];                                             // ... and its parameters
  // optimiser state (irtkImageRegistration::Run + irtkGradientDescentOptimizer::Run)
  int phase = 0, step_i = 0, iter_j = 0, grad_k = 0;
  double step = 0, delta = 0, old_sim = 0, new_sim = 0, sim = 0, start[6], s1 = 0;
  float dx[6];
  bool done = false;
};

enum { PH_START = 0, PH_GRAD, PH_LINE };

double ncc_from_sums(const int64_t s[6]) {                 // irtkCrossCorrelationSimilarityMetric::Evaluate, CCSM.h:158-165
  const double n = (double)s[0], x = (double)s[1], y = (double)s[2], x2 = (double)s[3], y2 = (double)s[4], xy = (double)s[5];
  if (n > 0) return (xy - (x * y) / n) / (sqrt(x2 - x * x / n) * sqrt(y2 - y * y / n));
  return 0;
}

// The similarity of a pass: everything between the optimiser's requests and the values it gets back that depends on which of
// the three metrics runs, and on whether the engine or a caller's backend evaluates it.  The schedule and the optimiser see
// requests and value(): CC is the six moments added over the planes of a request; NMI (the levels binned, irtkCalculateNumber-
// OfBins) one {n, S_xy, S_x, S_y} per request, the engine's or nmi_sums of the caller's histograms; LNCC (neither image binned)
// the integers {N, S} per plane -- the engine's pairs, or the first two of a caller's six -- added over the planes.
struct Metric {
  const Backend &be;
  int kind, radius;                                        // SVRH_SIM_*; the LNCC window
  int src_nbins = 1;                                       // NMI: bins of this level's source
  std::vector<int> req_planes, req_width, req_nbins;       // NMI: what a request records
  std::vector<double> out4;
  std::vector<int64_t> sums;
  std::vector<uint32_t> hist;
  bool nmi() const { return kind == SVRH_SIM_NMI; }
  bool lncc() const { return kind == SVRH_SIM_LNCC; }
  const char *name() const { return nmi() ? "NMI" : lncc() ? "LNCC" : "CC"; }
  int stride() const { return lncc() && !be.be ? 2 : 6; }  // entries per plane in `sums`
  // the level's source: binned before it is interpolated (IRWP.cc:243-244), [mn, mx] its range before the shift
  int prepare_source(Vol<short> &src, int mn, int mx, bool dev, std::string &err) {
    if (!nmi()) return 0;
    int width = 1;
    src_nbins = nmi_number_of_bins(mn, mx, width);
    if (!dev) nmi_bin(src.d.data(), src.d.size(), width);
    else if (svr_nmi_bin_source(be.ctx, width)) { err = std::string("svr_nmi_bin_source: ") + svr_last_error(be.ctx); return 2; }
    return 0;
  }
  void prepare_target(Target &t, int mn, int mx) const { t.nbins = nmi_number_of_bins(mn, mx, t.bin_width); }   // binned on the fly
  void size_round(int n_req, int n_planes) {
    if (nmi()) { req_planes.resize(n_req); req_width.resize(n_req); req_nbins.resize(n_req); out4.resize(4 * (size_t)n_req); }
    else sums.resize(stride() * (size_t)n_planes);
  }
  void record(int rq, const Target &t) {
    if (nmi()) { req_planes[rq] = t.lvl.a.nz; req_width[rq] = t.bin_width; req_nbins[rq] = t.nbins; }
  }
  int call(int n_req, int n_planes, const int *idx, const double *m) {
    if (nmi()) {
      const int *ppe = req_planes.data(), *width = req_width.data(), *nbins = req_nbins.data();
      if (!be.nbe) return svr_nmi_evaluate(be.ctx, n_req, ppe, idx, m, width, nbins, src_nbins, out4.data(), nullptr);
      hist.assign((size_t)n_req * 4096, 0);
      if (int rc = be.nbe->evaluate(be.nbe->user, n_req, ppe, idx, m, width, nbins, src_nbins, hist.data())) return rc;
      for (int e = 0; e < n_req; ++e) nmi_sums(&hist[(size_t)e * 4096], nbins[e], src_nbins, &out4[4 * (size_t)e]);
      return 0;
    }
    if (be.be) return be.be->evaluate(be.be->user, n_planes, idx, m, sums.data(), nullptr);
    return lncc() ? svr_lncc_evaluate(be.ctx, n_planes, idx, m, radius, sums.data(), nullptr) : svr_ncc_evaluate(be.ctx, n_planes, idx, m, sums.data(), nullptr);
  }
  int evaluate(int n_req, int n_planes, const int *idx, const double *m, std::string &err) {
    if (!call(n_req, n_planes, idx, m)) return 0;
    const std::string fn = nmi() ? "svr_nmi_evaluate" : lncc() ? "svr_lncc_evaluate" : "svr_ncc_evaluate";
    err = (kind == SVRH_SIM_CC || be.external()) ? fn + " failed" : fn + ": " + svr_last_error(be.ctx);
    return 2;
  }
  // request rq, whose nz planes start at plane `at` of the round
  double value(size_t rq, size_t at, int nz) const {
    if (nmi()) return nmi_from_sums(&out4[4 * rq]);
    int64_t s[6] = {0, 0, 0, 0, 0, 0};
    const int st = stride(), n = lncc() ? 2 : 6;
    for (int c = 0; c < nz; ++c) for (int k = 0; k < n; ++k) s[k] += sums[st * (at + c) + k];
    if (lncc()) return s[0] > 0 ? ((double)s[1] / (double)s[0]) / 16777216.0 : 0.0;   // (sum S / sum N) / 2^24
    return ncc_from_sums(s);
  }
};

// One level of prepare_level on the device (csrc/svr_pyr.inc) for `n` images of one grid whose unprocessed voxels sit at
// `offset` of the upload slot: the attributes of the level come back in out[i], the voxels stay on the device as the NCC
// source (slot 0) or as the target planes first_plane, first_plane + nz, ...
int device_level(svr_ctx *ctx, int slot, size_t offset, int n, const svr_image_attr *const *in, const short *pads, double blur, const double res[3],
                 const double res0[3], int level, int first_plane, svr_image_attr *out, std::string &err, int *mn_out = nullptr,
                 int *mx_out = nullptr) {
  const svr_image_attr &a0 = *in[0];
  std::vector<double> ker[3];
  if (blur > 0) {
    ker[0] = blur_kernel(blur, a0.dx); ker[1] = blur_kernel(blur, a0.dy);
    if (a0.nz != 1) ker[2] = blur_kernel(blur, a0.dz);     // GBWP.cc:90
  }
  const double temp = fabs(res0[0] - a0.dx) + fabs(res0[1] - a0.dy) + fabs(res0[2] - a0.dz);
  const int resample = level > 0 || temp > 0.000001;
  std::vector<svr_pyr_image> imgs(n);
  for (int i = 0; i < n; ++i) {
    out[i] = resample ? resampled_attr(*in[i], res[0], res[1], res[2]) : *in[i];
    const M4 o_i2w = image_to_world(out[i]), i_w2i = world_to_image(*in[i]);
    memcpy(imgs[i].i2w_out, o_i2w.m, sizeof(imgs[i].i2w_out));
    memcpy(imgs[i].w2i_in, i_w2i.m, sizeof(imgs[i].w2i_in));
    imgs[i].pad = pads[i];
  }
  const int in_dims[3] = {a0.nx, a0.ny, a0.nz}, out_dims[3] = {out[0].nx, out[0].ny, out[0].nz};
  std::vector<int> mn(n), mx(n);
  if (svr_pyr_level(ctx, slot, offset, n, in_dims, ker[0].data(), (int)ker[0].size(), ker[1].data(), (int)ker[1].size(), ker[2].data(),
                    (int)ker[2].size(), resample, out_dims, imgs.data(), first_plane, mn.data(), mx.data())) {
    err = std::string("svr_pyr_level: ") + svr_last_error(ctx);
    return 2;
  }
  for (int i = 0; i < n; ++i) {
    if ((double)mx[i] - (double)mn[i] > 32767.0) { err = "Initialize: dynamic range of an image is too large"; return 1; }
    if (mn_out) mn_out[i] = mn[i];
    if (mx_out) mx_out[i] = mx[i];
  }
  return 0;
}

struct GridKey {
  int nx, ny, nz;
  double dx, dy, dz;
  bool operator<(const GridKey &o) const { return std::tie(nx, ny, nz, dx, dy, dz) < std::tie(o.nx, o.ny, o.nz, o.dx, o.dy, o.dz); }
};
struct GridGroup { std::vector<int> members; size_t offset = 0; };

// SVRH_SIM_* and the LNCC radius of the `similarity` of the _ex entry points (radius 0 = 3); false = refused
bool parse_similarity(int similarity, int &sim, int &radius) {
  sim = similarity & 0xff;
  radius = (similarity >> 8) & 0xffffff;
  if (similarity < 0 || (sim != SVRH_SIM_CC && sim != SVRH_SIM_NMI && sim != SVRH_SIM_LNCC)) return false;
  if (sim != SVRH_SIM_LNCC) return radius == 0;
  if (radius == 0) radius = 3;
  return radius >= 1 && radius <= 7;
}

// ---- a pass = irtkImageRegistration::Run for every target against one source, in lock step, stage by stage ------------------------
struct Pass {                                              // what the stages share
  const Backend &be;
  std::vector<Target> &targets;
  const Vol<short> &source;
  int slice_to_volume;
  short target_padding, source_padding;
  // The engine makes the pyramids itself (csrc/svr_pyr.inc: the same arithmetic, no host pass over the voxels, no upload
  // per level); another backend (the oracle evaluator of the tests), or SVR_HOST_PYRAMID=1, takes the host code.
  bool dev;
  std::map<GridKey, GridGroup> groups;                     // dev: targets of one grid go through the kernels together
  Schedule schedule(const Target &t) const { return guess_parameters(t.full->a, source.a, slice_to_volume); }
  short padding_of(const Target &t) const { return t.own_padding ? t.padding : target_padding; }
};
struct Level {
  int level;
  Schedule ps;                                             // of the first target: the optimiser's iterations, steps and epsilon
  Vol<short> src;                                          // the source of the level (dev: its attributes only)
  int tx = 0, ty = 0, planes = 0;                          // the backend's target planes
};
struct Round {                                             // one batched evaluation: the requests of every target still running
  std::vector<int> live, req_off, plane_off, idx;
  std::vector<double> mats, value;
  int n_req = 0, n_planes = 0;
};
struct Times { double src = 0, tgt = 0, pack = 0, opt = 0, eval = 0; long rounds = 0; };   // SVR_REG_TIMING
double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// a target enters a level: its optimiser starts over, its planes follow those of the targets before it
void enter_level(Target &t, const Schedule &p, Level &lv) {
  t.phase = PH_START; t.step_i = 0; t.iter_j = 0; t.done = false;
  t.step = p.length[lv.level]; t.delta = p.delta[lv.level];
}
void place_planes(Target &t, Level &lv) {
  lv.tx = std::max(lv.tx, t.lvl.a.nx); lv.ty = std::max(lv.ty, t.lvl.a.ny);
  t.first_plane = lv.planes;
  lv.planes += t.lvl.a.nz;
}

// dev: the unprocessed source (slot 0) and targets (slot 1, grid by grid) go up once per pass
int upload_pyramid_inputs(Pass &ps, std::string &err) {
  if (svr_pyr_upload(ps.be.ctx, 0, ps.source.d.data(), ps.source.n())) { err = std::string("svr_pyr_upload: ") + svr_last_error(ps.be.ctx); return 2; }
  size_t total = 0;
  for (size_t r = 0; r < ps.targets.size(); ++r) {
    const svr_image_attr &a = ps.targets[r].full->a;
    ps.groups[GridKey{a.nx, a.ny, a.nz, a.dx, a.dy, a.dz}].members.push_back((int)r);
    total += ps.targets[r].full->n();
  }
  std::vector<int16_t> all(total);
  size_t at = 0;
  for (auto &g : ps.groups) {
    g.second.offset = at;
    for (int r : g.second.members) { memcpy(&all[at], ps.targets[r].full->d.data(), sizeof(int16_t) * ps.targets[r].full->n()); at += ps.targets[r].full->n(); }
  }
  if (svr_pyr_upload(ps.be.ctx, 1, all.data(), total)) { err = std::string("svr_pyr_upload: ") + svr_last_error(ps.be.ctx); return 2; }
  return 0;
}

// Initialize(level) of the source, on the device or on the host
int level_source(Pass &ps, Metric &metric, Level &lv, std::string &err) {
  const int level = lv.level;
  int smn = 0, smx = -1;
  if (ps.dev) {
    const svr_image_attr *in = &ps.source.a;
    if (int rc = device_level(ps.be.ctx, 0, 0, 1, &in, &ps.source_padding, lv.ps.s_blur[level], lv.ps.s_res[level], lv.ps.s_res[0], level, 0, &lv.src.a,
                              err, &smn, &smx))
      return rc;
  } else if (prepare_level(ps.source, lv.ps.s_blur[level], lv.ps.s_res[level], lv.ps.s_res[0], level, ps.source_padding, lv.src, err, &smn, &smx)) return 1;
  return metric.prepare_source(lv.src, smn, smx, ps.dev, err);
}

// Initialize(level) of every target on the device: the grids of the level first (the planes must be allocated before the kernels
// write them), then the kernels group by group
int level_targets_device(Pass &ps, const Metric &metric, Level &lv, std::string &err) {
  const int level = lv.level;
  for (auto &g : ps.groups)
    for (int r : g.second.members) {
      Target &t = ps.targets[r];
      const Schedule p = ps.schedule(t);
      const double temp = fabs(p.t_res[0][0] - t.full->a.dx) + fabs(p.t_res[0][1] - t.full->a.dy) + fabs(p.t_res[0][2] - t.full->a.dz);
      t.lvl.a = (level > 0 || temp > 0.000001) ? resampled_attr(t.full->a, p.t_res[level][0], p.t_res[level][1], p.t_res[level][2]) : t.full->a;
      t.lvl.d.clear();
      enter_level(t, p, lv);
      place_planes(t, lv);
    }
  if (svr_ncc_alloc_targets(ps.be.ctx, lv.planes, lv.tx, lv.ty)) { err = std::string("svr_ncc_alloc_targets: ") + svr_last_error(ps.be.ctx); return 2; }
  for (auto &g : ps.groups) {
    const std::vector<int> &mem = g.second.members;
    const Schedule p = ps.schedule(ps.targets[mem[0]]);
    const size_t nvox = ps.targets[mem[0]].full->n();
    for (size_t c0 = 0; c0 < mem.size(); c0 += 32768) {                        // the grid's y dimension holds 65535 images
      const int n = (int)std::min<size_t>(32768, mem.size() - c0);
      std::vector<const svr_image_attr *> in(n);
      std::vector<short> pads(n);
      std::vector<svr_image_attr> outa(n);
      for (int i = 0; i < n; ++i) {
        const Target &t = ps.targets[mem[c0 + i]];
        in[i] = &t.full->a;
        pads[i] = ps.padding_of(t);
      }
      std::vector<int> tmn(n), tmx(n);
      if (int rc = device_level(ps.be.ctx, 1, g.second.offset + c0 * nvox, n, in.data(), pads.data(), p.t_blur[level], p.t_res[level], p.t_res[0], level,
                                ps.targets[mem[c0]].first_plane, outa.data(), err, tmn.data(), tmx.data()))
        return rc;
      for (int i = 0; i < n; ++i) metric.prepare_target(ps.targets[mem[c0 + i]], tmn[i], tmx[i]);
    }
  }
  return 0;
}

// ... and on the host, by the host threads
int level_targets_host(Pass &ps, const Metric &metric, Level &lv, std::string &err) {
  std::vector<Target> &targets = ps.targets;
  std::vector<int> bad(targets.size(), 0);
  std::vector<std::string> errs(targets.size());
  size_t pixels = 0;
  for (const Target &t : targets) pixels += t.full->n();
  parallel_rows((int)targets.size(), pixels / targets.size() * 60, [&](int r0, int r1) {
    for (int r = r0; r < r1; ++r) {
      Target &t = targets[r];
      const Schedule p = ps.schedule(t);
      int mn = 0, mx = -1;
      bad[r] = prepare_level(*t.full, p.t_blur[lv.level], p.t_res[lv.level], p.t_res[0], lv.level, ps.padding_of(t), t.lvl, errs[r], &mn, &mx);
      metric.prepare_target(t, mn, mx);
      enter_level(t, p, lv);
    }
  });
  for (size_t r = 0; r < targets.size(); ++r)
    if (bad[r]) { err = errs[r]; return 1; }
  return 0;
}

// host: the level's planes packed into one array and handed, with the source, to the backend
int pack_level_host(Pass &ps, Level &lv, std::string &err) {
  for (Target &t : ps.targets) place_planes(t, lv);
  const int tx = lv.tx, ty = lv.ty;
  std::vector<int16_t> packed((size_t)lv.planes * tx * ty, (int16_t)-1);
  for (const Target &t : ps.targets)
    for (int k = 0; k < t.lvl.a.nz; ++k)
      for (int y = 0; y < t.lvl.a.ny; ++y)
        memcpy(&packed[((size_t)(t.first_plane + k) * ty + y) * tx], &t.lvl.d[((size_t)k * t.lvl.a.ny + y) * t.lvl.a.nx], sizeof(int16_t) * t.lvl.a.nx);
  if (ps.be.set_targets(lv.planes, tx, ty, packed.data())) { err = "svr_ncc_set_targets failed"; return 2; }
  const uint32_t ssz[3] = {(uint32_t)lv.src.a.nx, (uint32_t)lv.src.a.ny, (uint32_t)lv.src.a.nz};
  if (ps.be.set_source(ssz, lv.src.d.data())) { err = "svr_ncc_set_source failed"; return 2; }
  return 0;
}

// the requests of a round by a prefix sum over the targets still running; false = none is
bool lay_out_round(const std::vector<Target> &targets, Round &rd) {
  rd.live.clear(); rd.req_off.clear(); rd.plane_off.clear();
  rd.n_req = rd.n_planes = 0;
  for (size_t ti = 0; ti < targets.size(); ++ti) {
    const Target &t = targets[ti];
    if (t.done) continue;
    const int nr = t.phase == PH_GRAD ? 12 : 1;             // START: old_similarity = Evaluate(), GDO.cc:31; GRAD: IR.cc:530-568; LINE: one probe
    rd.live.push_back((int)ti); rd.req_off.push_back(rd.n_req); rd.plane_off.push_back(rd.n_planes);
    rd.n_req += nr; rd.n_planes += nr * t.lvl.a.nz;
  }
  rd.idx.resize(rd.n_planes); rd.mats.resize(16 * (size_t)rd.n_planes); rd.value.resize(rd.n_req);
  return !rd.live.empty();
}

// the requests of live target l: its similarity or probe at t.matrix, or its 12 finite differences
void write_requests(const Target &t, const M4 &s_w2i, int l, Metric &metric, Round &rd) {
  int at = rd.plane_off[l], rq = rd.req_off[l];
  auto request = [&](const M4 &tm) {                         // the per-plane matrices of one evaluation (push_request)
    metric.record(rq++, t);
    const M4 m = mul(mul(s_w2i, tm), image_to_world(t.lvl.a));
    double zx = m.m[3], zy = m.m[7], zz = m.m[11];
    for (int k = 0; k < t.lvl.a.nz; ++k, ++at) {
      rd.idx[at] = t.first_plane + k;
      M4 q = m;
      q.m[3] = zx; q.m[7] = zy; q.m[11] = zz;
      memcpy(&rd.mats[16 * (size_t)at], q.m, sizeof(q.m));
      zx += m.m[2]; zy += m.m[6]; zz += m.m[10];             // NextZ()
    }
  };
  if (t.phase != PH_GRAD) { request(t.matrix); return; }
  for (int i = 0; i < 6; ++i) {
    double q[6];
    for (int k = 0; k < 6; ++k) q[k] = t.p[k];
    q[i] = t.p[i] + t.step; request(params_to_matrix(q));
    q[i] = t.p[i] - t.step; request(params_to_matrix(q));
  }
}

// One step of irtkImageRegistration::Run + irtkGradientDescentOptimizer::Run for a target whose requests came back as value[]:
// START took the similarity, GRAD the 12 finite differences, LINE one probe of the line search.
void advance(Target &t, const double *value, const Schedule &p0, int level) {
  auto take_step = [&](double sign) {                        // Put(i, Get(i) +- StepSize * dx[i]) for every i
    for (int i = 0; i < 6; ++i) t.p[i] = t.p[i] + sign * (t.step * t.dx[i]);
    t.matrix = params_to_matrix(t.p);
  };
  if (t.phase == PH_START) {
    t.old_sim = t.new_sim = t.sim = value[0];
    for (int i = 0; i < 6; ++i) t.start[i] = t.p[i];         // irtkOptimizer::Run stores the parameters, O.cc:113-116
    t.phase = PH_GRAD;
    return;
  }
  if (t.phase == PH_GRAD) {
    double norm = 0;
    for (int i = 0; i < 6; ++i) { const double s1 = value[2 * i], s2 = value[2 * i + 1]; t.dx[i] = (float)(s1 - s2); }
    t.matrix = params_to_matrix(t.p);                        // Put(i, parameterValue) rebuilt the matrix from the parameters
    for (int i = 0; i < 6; ++i) norm += t.dx[i] * t.dx[i];
    norm = sqrt(norm);
    for (int i = 0; i < 6; ++i) t.dx[i] = norm > 0 ? (float)(t.dx[i] / norm) : 0.0f;
    t.new_sim = t.sim;                                       // first pass of the do-while, GDO.cc:47-54
    take_step(+1);
    t.phase = PH_LINE;
    return;
  }
  t.sim = value[0];
  if (t.sim > t.new_sim + p0.epsilon) {                      // keep stepping
    t.new_sim = t.sim;
    take_step(+1);
    return;
  }
  take_step(-1);                                             // last step was no improvement: back track, GDO.cc:58-61
  const double eps = t.new_sim > t.old_sim ? t.new_sim - t.old_sim : 0;
  double max_change = 0;
  for (int i = 0; i < 6; ++i) max_change = std::max(max_change, fabs(t.p[i] - t.start[i]));
  bool next_step = true;                                     // IR.cc:482-506
  if (eps > p0.epsilon && max_change > t.delta) {
    if (++t.iter_j < p0.iterations[level]) next_step = false;
  }
  if (next_step) {
    t.iter_j = 0;
    t.step = t.step / 2;
    t.delta = t.delta / 2.0;
    if (++t.step_i >= p0.steps[level]) t.done = true;
  }
  t.phase = PH_START;
}

// The optimiser of a level, one round = one batched evaluation.  A round costs the host a few double trigonometric calls per
// target; with tens of thousands of targets (the patches of the patch-based path) that was 1.6 s of a 2.8 s pass, so the requests
// are laid out by a prefix sum and written, and the answers consumed, by the host threads -- every target touches only its own
// state and its own slots.
int optimise_level(Pass &ps, Metric &metric, const Level &lv, Times &tm, long *n_eval, std::string &err) {
  const M4 s_w2i = world_to_image(lv.src.a);
  Round rd;
  auto over_live = [&](size_t work, const std::function<void(int, int)> &fn) {
    if (rd.live.size() >= 2048) parallel_rows((int)rd.live.size(), work, fn);
    else fn(0, (int)rd.live.size());
  };
  while (lay_out_round(ps.targets, rd)) {
    metric.size_round(rd.n_req, rd.n_planes);
    over_live(3000, [&](int l0, int l1) {
      for (int l = l0; l < l1; ++l) write_requests(ps.targets[rd.live[l]], s_w2i, l, metric, rd);
    });
    const double te = now();
    if (int rc = metric.evaluate(rd.n_req, rd.n_planes, rd.idx.data(), rd.mats.data(), err)) return rc;
    tm.eval += now() - te; ++tm.rounds;
    if (n_eval) *n_eval += (long)rd.n_req;
    over_live(600, [&](int l0, int l1) {
      for (int l = l0; l < l1; ++l) {
        Target &t = ps.targets[rd.live[l]];
        const int nz = t.lvl.a.nz, nr = t.phase == PH_GRAD ? 12 : 1;
        double *v = &rd.value[rd.req_off[l]];
        for (int q = 0; q < nr; ++q) v[q] = metric.value((size_t)rd.req_off[l] + q, (size_t)rd.plane_off[l] + (size_t)q * nz, nz);
        advance(t, v, lv.ps, lv.level);
      }
    });
  }
  return 0;
}

// sim: the similarity is NMI instead of CC (GuessParameterSliceToVolume(useNMI), IRRWP.cc:319-321: the schedule, the optimiser
// and epsilon are the same), or the windowed cross correlation of radius lncc_radius
int run_registrations(const Backend &be, std::vector<Target> &targets, const Vol<short> &source, int slice_to_volume, short target_padding,
                      int sim, int lncc_radius, long *n_eval, std::string &err) {
  if (targets.empty()) return 0;
  Pass ps{be, targets, source, slice_to_volume, target_padding, guess_padding(source), !be.external() && be.ctx && !getenv("SVR_HOST_PYRAMID"), {}};
  Metric metric{be, sim, lncc_radius};
  Times tm;                                                 // dev: where a registration pass spends its wall time
  if (ps.dev)
    if (int rc = upload_pyramid_inputs(ps, err)) return rc;
  for (int level = 2; level >= 0; --level) {
    Level lv;
    lv.level = level;
    lv.ps = ps.schedule(targets[0]);
    double t0 = now();
    if (int rc = level_source(ps, metric, lv, err)) return rc;
    tm.src += now() - t0; t0 = now();
    if (int rc = ps.dev ? level_targets_device(ps, metric, lv, err) : level_targets_host(ps, metric, lv, err)) return rc;
    tm.tgt += now() - t0; t0 = now();
    if (!ps.dev)
      if (int rc = pack_level_host(ps, lv, err)) return rc;
    tm.pack += now() - t0; t0 = now();
    if (int rc = optimise_level(ps, metric, lv, tm, n_eval, err)) return rc;
    tm.opt += now() - t0;
  }
  if (getenv("SVR_REG_TIMING"))
    fprintf(stderr, "[svr reg timing] %s: source pyramid %.1f ms, target pyramids %.1f ms, pack + upload %.1f ms, optimiser %.1f ms (%ld rounds, %.1f ms in the batched evaluations)\n",
            metric.name(), 1e3 * tm.src, 1e3 * tm.tgt, 1e3 * tm.pack, 1e3 * tm.opt, tm.rounds, 1e3 * tm.eval);
  return 0;
}

template <class T> Vol<short> to_grey(const svr_image_attr &a, const T *d) {   // irtkGreyImage = irtkRealImage: static_cast per voxel
  Vol<short> v;
  v.a = a;
  v.d.resize(v.n());
  for (size_t i = 0; i < v.d.size(); ++i) v.d[i] = (short)d[i];
  return v;
}

void reset_origin(svr_image_attr &a, M4 &offset) {                       // ResetOrigin, RG.cc:823-834
  offset = ident();
  offset.m[3] = a.origin[0]; offset.m[7] = a.origin[1]; offset.m[11] = a.origin[2];
  a.origin[0] = a.origin[1] = a.origin[2] = 0;
}

void set_err(char err[256], const std::string &m) { if (err) { strncpy(err, m.c_str(), 255); err[255] = 0; } }

// The opening of the two _ex entry points: the similarity taken apart, a place to evaluate it (the engine, or the caller's backend
// of that similarity's kind) and the entry point's own arguments (`args_ok`) required, the evaluation count zeroed; false = refused
bool open_registration(svr_ctx *ctx, const svr_ncc_backend *backend, const svr_nmi_backend *nmi_backend, int similarity, bool args_ok,
                       long *n_evaluations_or_null, Backend &be, int &sim, int &radius) {
  if (!parse_similarity(similarity, sim, radius)) return false;
  const bool nmi = sim == SVRH_SIM_NMI;
  be = Backend{ctx, nmi ? nullptr : backend, nmi ? nmi_backend : nullptr};
  if ((!ctx && !be.external()) || !args_ok) return false;
  if (n_evaluations_or_null) *n_evaluations_or_null = 0;
  return true;
}

}  // namespace

extern "C" {

int svrh_stack_registrations(svr_ctx *ctx, const svr_ncc_backend *backend, int n_stacks, const svr_image_attr *attrs,
                             const double *const *stacks, double *transformations, int template_number,
                             const svr_image_attr *mask_attr, const double *mask_or_null, int flags, long *n_evaluations_or_null,
                             char err[256]) {
  if ((!ctx && !backend) || n_stacks < 1 || !attrs || !stacks || !transformations || template_number < 0 || template_number >= n_stacks) {
    set_err(err, "svrh_stack_registrations: bad arguments");
    return 1;
  }
  if (n_evaluations_or_null) *n_evaluations_or_null = 0;
  const Backend be{ctx, backend};
  std::vector<M4> T(n_stacks);
  for (int s = 0; s < n_stacks; ++s) {                                   // InvertStackTransformations, RG.cc:946
    M4 m;
    for (int q = 0; q < 16; ++q) m.m[q] = transformations[16 * s + q];
    T[s] = inverse_rigid_or_affine(m);
  }
  Vol<short> target = to_grey(attrs[template_number], stacks[template_number]);
  if (mask_or_null) {                                                     // RG.cc:959-984: outside the mask -> 0
    Vol<double> mask;
    mask.a = *mask_attr;
    mask.d.assign(mask_or_null, mask_or_null + mask.n());
    const M4 t_i2w = image_to_world(target.a), m_w2i = world_to_image(mask.a);
    for (int k = 0; k < target.a.nz; ++k)
      for (int j = 0; j < target.a.ny; ++j)
        for (int i = 0; i < target.a.nx; ++i) {
          const double wx = t_i2w.m[0] * i + t_i2w.m[1] * j + t_i2w.m[2] * k + t_i2w.m[3], wy = t_i2w.m[4] * i + t_i2w.m[5] * j + t_i2w.m[6] * k + t_i2w.m[7],
                       wz = t_i2w.m[8] * i + t_i2w.m[9] * j + t_i2w.m[10] * k + t_i2w.m[11];
          const double x = irtk_round(m_w2i.m[0] * wx + m_w2i.m[1] * wy + m_w2i.m[2] * wz + m_w2i.m[3]);
          const double y = irtk_round(m_w2i.m[4] * wx + m_w2i.m[5] * wy + m_w2i.m[6] * wz + m_w2i.m[7]);
          const double z = irtk_round(m_w2i.m[8] * wx + m_w2i.m[9] * wy + m_w2i.m[10] * wz + m_w2i.m[11]);
          if (x >= 0 && x < mask.a.nx && y >= 0 && y < mask.a.ny && z >= 0 && z < mask.a.nz) {
            if (mask.at((int)x, (int)y, (int)z) == 0) target.at(i, j, k) = 0;
          } else {
            target.at(i, j, k) = 0;
          }
        }
  }
  M4 mo = ident();
  // irtkStack3D3DRegistration<T>::ResetOrigin takes its arguments by value (irtkStack3D3DRegistration.cpp:151-162): the
  // patch-based command line registers with the target's origin in place and an identity offset
  if (!(flags & SVRH_STACKREG_KEEP_ORIGIN)) reset_origin(target.a, mo);   // RG.cc:987-988
  const M4 mo_inv = inverse_rigid_or_affine(mo);
  for (int s = 0; s < n_stacks; ++s) {                                    // ParallelStackRegistrations, RG.cc:877-911
    if (s == template_number) continue;
    const Vol<short> source = to_grey(attrs[s], stacks[s]);
    std::vector<Target> one(1);
    one[0].full = &target;
    one[0].matrix = mul(T[s], mo);                                        // include the offset: PutMatrix(m * mo)
    matrix_to_params(one[0].matrix, one[0].p);
    std::string e;
    const int rc = run_registrations(be, one, source, 0, (short)0, SVRH_SIM_CC, 0, n_evaluations_or_null, e);   // ThickSlices, SetTargetPadding(0)
    if (rc) { set_err(err, e); return rc; }
    T[s] = mul(params_to_matrix(one[0].p), mo_inv);                       // undo the offset
  }
  for (int s = 0; s < n_stacks; ++s) {                                    // InvertStackTransformations, RG.cc:1000
    const M4 inv = inverse_rigid_or_affine(T[s]);
    for (int q = 0; q < 16; ++q) transformations[16 * s + q] = inv.m[q];
  }
  return 0;
}

int svrh_slice_to_volume_registration(svr_ctx *ctx, const svr_ncc_backend *backend, int n_slices, const float *slices, int sx, int sy,
                                      const svr_image_attr *attrs, double *transformations, const svr_image_attr *recon_attr,
                                      const float *reconstructed, int flags, long *n_evaluations_or_null, char err[256]) {
  return svrh_slice_to_volume_registration_ex(ctx, backend, nullptr, SVRH_SIM_CC, n_slices, slices, sx, sy, attrs, transformations, recon_attr,
                                              reconstructed, flags, n_evaluations_or_null, err);
}

int svrh_slice_to_volume_registration_ex(svr_ctx *ctx, const svr_ncc_backend *backend, const svr_nmi_backend *nmi_backend, int similarity,
                                         int n_slices, const float *slices, int sx, int sy, const svr_image_attr *attrs, double *transformations,
                                         const svr_image_attr *recon_attr, const float *reconstructed, int flags, long *n_evaluations_or_null,
                                         char err[256]) {
  Backend be{nullptr, nullptr};
  int sim = 0, radius = 0;
  if (!open_registration(ctx, backend, nmi_backend, similarity, n_slices >= 1 && slices && attrs && transformations && recon_attr && reconstructed,
                         n_evaluations_or_null, be, sim, radius)) {
    set_err(err, "svrh_slice_to_volume_registration: bad arguments");
    return 1;
  }
  const Vol<short> source = to_grey(*recon_attr, reconstructed);          // irtkGreyImage source = _reconstructed, RG.cc:2031
  std::vector<Vol<short>> grey(n_slices);
  std::vector<M4> mo_inv(n_slices);
  std::vector<Target> targets;
  std::vector<int> which;
  targets.reserve(n_slices);
  std::vector<char> live(n_slices, 0);
  std::vector<M4> mo_all(n_slices);
  parallel_rows(n_slices, (size_t)sx * sy * 60, [&](int s0, int s1) {       // ParallelSliceToVolumeRegistration, RG.cc:2002-2050
    for (int s = s0; s < s1; ++s) {
      Vol<double> sl;
      sl.a = attrs[s];
      sl.d.resize(sl.n());
      for (int y = 0; y < sl.a.ny; ++y)
        for (int x = 0; x < sl.a.nx; ++x) sl.at(x, y, 0) = slices[((size_t)s * sy + y) * sx + x];
      // the patch-based caller (ParallelPatchToVolumeRegistration, patchBased2D3DRegistration.cpp:113-122) resamples into a variable
      // that shadows the patch and goes out of scope: its targets are registered as they are
      const Vol<double> t = (flags & SVRH_S2V_NO_RESAMPLE) ? sl : resample_with_padding<double>(sl, recon_attr->dx, recon_attr->dx, recon_attr->dx, -1.0);
      grey[s].a = t.a;
      grey[s].d.resize(t.d.size());
      short smax = -32768;
      for (size_t i = 0; i < t.d.size(); ++i) { grey[s].d[i] = (short)t.d[i]; smax = std::max(smax, grey[s].d[i]); }
      if (!(smax > -1)) continue;                                           // nothing to register
      reset_origin(grey[s].a, mo_all[s]);
      live[s] = 1;
    }
  });
  for (int s = 0; s < n_slices; ++s) {
    if (!live[s]) continue;
    M4 m;
    for (int q = 0; q < 16; ++q) m.m[q] = transformations[16 * s + q];
    mo_inv[s] = inverse_rigid_or_affine(mo_all[s]);
    Target tg;
    tg.full = &grey[s];
    tg.matrix = mul(m, mo_all[s]);
    matrix_to_params(tg.matrix, tg.p);
    targets.push_back(tg);
    which.push_back(s);
  }
  std::string e;
  const int rc = run_registrations(be, targets, source, 1, (short)-1, sim, radius, n_evaluations_or_null, e);   // SliceToVolume, SetTargetPadding(-1)
  if (rc) { set_err(err, e); return rc; }
  for (size_t k = 0; k < targets.size(); ++k) {
    const M4 m = mul(params_to_matrix(targets[k].p), mo_inv[which[k]]);
    for (int q = 0; q < 16; ++q) transformations[16 * which[k] + q] = m.m[q];
  }
  return 0;
}

// SplitImage, RG.cc:4979-5035: every `packages`-th slice, starting at l = 0 .. packages-1
static void split_image(const Vol<double> &image, int packages, std::vector<Vol<double>> &out) {
  const int pkg_z = image.a.nz / packages;
  const M4 i2w = image_to_world(image.a);
  for (int l = 0; l < packages; ++l) {
    Vol<double> st;
    st.a = image.a;
    st.a.nz = (pkg_z * packages + l) < image.a.nz ? pkg_z + 1 : pkg_z;
    st.a.dz = image.a.dz * packages;
    st.d.resize(st.n());
    for (int k = 0; k < st.a.nz; ++k)
      for (int j = 0; j < st.a.ny; ++j)
        for (int i = 0; i < st.a.nx; ++i) st.at(i, j, k) = image.at(i, j, k * packages + l);
    // adjust the origin so that voxel (0,0,0) of the package sits on voxel (0,0,l) of the image
    const double x = i2w.m[2] * l + i2w.m[3], y = i2w.m[6] * l + i2w.m[7], z = i2w.m[10] * l + i2w.m[11];
    const M4 s = image_to_world(st.a);
    st.a.origin[0] += x - s.m[3]; st.a.origin[1] += y - s.m[7]; st.a.origin[2] += z - s.m[11];
    out.push_back(st);
  }
}
static Vol<double> z_region(const Vol<double> &im, int z1, int z2) {     // GetRegion(0, 0, z1, nx, ny, z2)
  Vol<double> o;
  o.a = im.a;
  o.a.nz = z2 - z1;
  const M4 i2w = image_to_world(im.a);
  const double c[3] = {(im.a.nx - 1) / 2.0, (im.a.ny - 1) / 2.0, z1 + (o.a.nz - 1) / 2.0};
  for (int k = 0; k < 3; ++k) o.a.origin[k] = i2w.m[4 * k] * c[0] + i2w.m[4 * k + 1] * c[1] + i2w.m[4 * k + 2] * c[2] + i2w.m[4 * k + 3];
  o.d.assign(im.d.begin() + (size_t)z1 * im.a.nx * im.a.ny, im.d.begin() + (size_t)z2 * im.a.nx * im.a.ny);
  return o;
}
static void split_even_odd(const Vol<double> &image, int packages, std::vector<Vol<double>> &out) {      // RG.cc:5037-5055
  std::vector<Vol<double>> packs;
  split_image(image, packages, packs);
  for (const Vol<double> &p : packs) split_image(p, 2, out);
}
static void split_even_odd_half(const Vol<double> &image, int packages, std::vector<Vol<double>> &out, int iter) {   // RG.cc:5057-5093
  std::vector<Vol<double>> packs;
  if (iter > 1) split_even_odd_half(image, packages, packs, iter - 1);
  else split_even_odd(image, packages, packs);
  for (const Vol<double> &p : packs) {
    if (p.a.nz >= 4) { out.push_back(z_region(p, 0, p.a.nz / 2)); out.push_back(z_region(p, p.a.nz / 2, p.a.nz)); }   // HalfImage
    else out.push_back(p);
  }
}

// irtkReconstruction::PackageToVolume, RG.cc:5096-5192: every package of every stack is registered to the reconstruction as
// one 3-D target (GuessParameterSliceToVolume; the target padding is the corner guess, no SetTargetPadding) and its
// transformation is given to all of its slices.  transformations: one per slice, stacks in order.
int svrh_package_to_volume(svr_ctx *ctx, const svr_ncc_backend *backend, int n_stacks, const svr_image_attr *attrs, const double *const *stacks,
                           const int *pack_num, int evenodd, int half, int half_iter, double *transformations,
                           const svr_image_attr *recon_attr, const float *reconstructed, long *n_evaluations_or_null, char err[256]) {
  return svrh_package_to_volume_ex(ctx, backend, nullptr, SVRH_SIM_CC, n_stacks, attrs, stacks, pack_num, evenodd, half, half_iter, transformations,
                                   recon_attr, reconstructed, n_evaluations_or_null, err);
}

int svrh_package_to_volume_ex(svr_ctx *ctx, const svr_ncc_backend *backend, const svr_nmi_backend *nmi_backend, int similarity, int n_stacks,
                              const svr_image_attr *attrs, const double *const *stacks, const int *pack_num, int evenodd, int half, int half_iter,
                              double *transformations, const svr_image_attr *recon_attr, const float *reconstructed, long *n_evaluations_or_null,
                              char err[256]) {
  Backend be{nullptr, nullptr};
  int sim = 0, radius = 0;
  if (!open_registration(ctx, backend, nmi_backend, similarity, n_stacks >= 1 && attrs && stacks && pack_num && transformations && recon_attr && reconstructed,
                         n_evaluations_or_null, be, sim, radius)) {
    set_err(err, "svrh_package_to_volume: bad arguments");
    return 1;
  }
  const Vol<short> source = to_grey(*recon_attr, reconstructed);
  struct Pack { Vol<short> grey; M4 mo_inv; int first; std::vector<int> slices; };
  std::vector<Pack> packs;
  int first_slice = 0;
  for (int s = 0; s < n_stacks; ++s) {
    if (pack_num[s] < 1) { set_err(err, "svrh_package_to_volume: package counts must be positive"); return 1; }
    Vol<double> st;
    st.a = attrs[s];
    st.d.assign(stacks[s], stacks[s] + st.n());
    std::vector<Vol<double>> pk;
    if (evenodd) { if (half) split_even_odd_half(st, pack_num[s], pk, half_iter); else split_even_odd(st, pack_num[s], pk); }
    else split_image(st, pack_num[s], pk);
    const M4 s_w2i = world_to_image(st.a);
    for (const Vol<double> &p : pk) {
      if (p.a.nz < 1) continue;
      Pack q;
      const M4 p_i2w = image_to_world(p.a);
      for (int k = 0; k < p.a.nz; ++k) {                                    // which slices of the stack the package holds
        const double wx = p_i2w.m[2] * k + p_i2w.m[3], wy = p_i2w.m[6] * k + p_i2w.m[7], wz = p_i2w.m[10] * k + p_i2w.m[11];
        const double z = s_w2i.m[8] * wx + s_w2i.m[9] * wy + s_w2i.m[10] * wz + s_w2i.m[11];
        q.slices.push_back((int)irtk_round(z) + first_slice);
      }
      q.first = q.slices[0];
      q.grey.a = p.a;
      q.grey.d.resize(p.d.size());
      for (size_t i = 0; i < p.d.size(); ++i) q.grey.d[i] = (short)p.d[i];
      packs.push_back(q);
    }
    first_slice += st.a.nz;
  }
  std::vector<Target> targets(packs.size());
  for (size_t k = 0; k < packs.size(); ++k) {
    Pack &q = packs[k];
    Target &tg = targets[k];
    tg.own_padding = 1;
    tg.padding = guess_padding(q.grey);                                    // before ResetOrigin: values only
    M4 mo, m;
    reset_origin(q.grey.a, mo);
    q.mo_inv = inverse_rigid_or_affine(mo);
    for (int c = 0; c < 16; ++c) m.m[c] = transformations[16 * (size_t)q.first + c];
    tg.full = &q.grey;
    tg.matrix = mul(m, mo);
    matrix_to_params(tg.matrix, tg.p);
  }
  std::string e;
  const int rc = run_registrations(be, targets, source, 1, (short)0, sim, radius, n_evaluations_or_null, e);
  if (rc) { set_err(err, e); return rc; }
  for (size_t k = 0; k < packs.size(); ++k) {
    const M4 m = mul(params_to_matrix(targets[k].p), packs[k].mo_inv);      // PutMatrix: the first slice keeps this matrix
    double p6[6];
    matrix_to_params(m, p6);
    const M4 rebuilt = params_to_matrix(p6);                                // the other slices: parameters copied, UpdateMatrix
    for (size_t j = 0; j < packs[k].slices.size(); ++j) {
      const int sl = packs[k].slices[j];
      const M4 &use = sl == packs[k].first ? m : rebuilt;
      for (int c = 0; c < 16; ++c) transformations[16 * (size_t)sl + c] = use.m[c];
    }
  }
  return 0;
}

// building blocks, exported for the tests
int svrh_irtk_resample_with_padding(const svr_image_attr *attr, const int16_t *data, double rx, double ry, double rz, int padding,
                                    svr_image_attr *out_attr, int16_t *out_or_null, long capacity) {
  Vol<short> v;
  v.a = *attr;
  v.d.assign(data, data + v.n());
  const Vol<short> o = resample_with_padding<short>(v, rx, ry, rz, (short)padding);
  *out_attr = o.a;
  if (out_or_null) {
    if ((long)o.d.size() > capacity) return 1;
    memcpy(out_or_null, o.d.data(), sizeof(int16_t) * o.d.size());
  }
  return 0;
}

int svrh_irtk_blur_with_padding(const svr_image_attr *attr, int16_t *data, double sigma, int padding) {
  Vol<short> v;
  v.a = *attr;
  v.d.assign(data, data + v.n());
  blur_with_padding(v, sigma, (short)padding);
  memcpy(data, v.d.data(), sizeof(int16_t) * v.d.size());
  return 0;
}

int svrh_irtk_blur_kernel(double sigma, double voxel, double *out_or_null, int capacity) {
  const std::vector<double> ker = blur_kernel(sigma, voxel);
  if (out_or_null) {
    if ((int)ker.size() > capacity) return -1;
    memcpy(out_or_null, ker.data(), sizeof(double) * ker.size());
  }
  return (int)ker.size();
}

int svrh_irtk_prepare_level(const svr_image_attr *attr, const int16_t *data, double blur, const double res[3], const double res0[3], int level,
                            int padding, svr_image_attr *out_attr, int16_t *out_or_null, long capacity, int *min_out, int *max_out,
                            char err[256]) {
  if (!attr || !data || !res || !res0 || !out_attr) { set_err(err, "svrh_irtk_prepare_level: bad arguments"); return 2; }
  Vol<short> v, o;
  v.a = *attr;
  v.d.assign(data, data + v.n());
  std::string e;
  if (int rc = prepare_level(v, blur, res, res0, level, (short)padding, o, e, min_out, max_out)) { set_err(err, e); return rc; }
  *out_attr = o.a;
  if (out_or_null) {
    if ((long)o.d.size() > capacity) { set_err(err, "svrh_irtk_prepare_level: the output does not fit"); return 2; }
    memcpy(out_or_null, o.d.data(), sizeof(int16_t) * o.d.size());
  }
  return 0;
}

int svrh_irtk_number_of_bins(int16_t *data_or_null, long n, int min, int max, int *width_or_null) {
  int width = 1;
  const int nbins = nmi_number_of_bins(min, max, width);
  if (data_or_null) nmi_bin(data_or_null, (size_t)n, width);
  if (width_or_null) *width_or_null = width;
  return nbins;
}

double svrh_nmi_sums(const uint32_t *hist64, int target_nbins, int source_nbins, double sums4[4]) {
  nmi_sums(hist64, target_nbins, source_nbins, sums4);
  return nmi_from_sums(sums4);
}

void svrh_irtk_rigid_parameters(const double matrix16[16], double params6[6], double *rebuilt16_or_null) {
  M4 m;
  for (int q = 0; q < 16; ++q) m.m[q] = matrix16[q];
  matrix_to_params(m, params6);
  if (rebuilt16_or_null) { const M4 r = params_to_matrix(params6); for (int q = 0; q < 16; ++q) rebuilt16_or_null[q] = r.m[q]; }
}

}  // extern "C"
