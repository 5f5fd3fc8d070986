// svr_launch.h -- the launch plumbing shared by the two command lines (csrc/svr_cli.cpp, csrc/pvr_cli.cpp), next to what they
// share in pre-processing (svr_prep.h) and in the sharded numbering (svr_shard.h): the argument cursor of the option loops, the
// marshalling around svrh_stack_registrations, the PSF volume's matrices, a unit's normal in volume axes for the work estimates,
// and `Ranks`: one engine context per device of -d, the rank group, a thread per rank, the matrices of every rank's units.
// Included by one translation unit per program, hence the unnamed namespace.
#ifndef SVR_LAUNCH_H
#define SVR_LAUNCH_H
#include "svr_prep.h"
#include "svr_shard.h"

namespace {

// ---- the argument cursor: `while (a.next())`, then a.o is the option and the value readers move past what they take -------------
struct Args {
  int argc;
  char **argv;
  int i = 0;
  std::string o;
  // -0.5 and -.5 are values, not options
  static bool is_opt(const char *s) { return s[0] == '-' && !(s[1] >= '0' && s[1] <= '9') && s[1] != '.'; }
  bool next() { if (++i >= argc) return false; o = argv[i]; return true; }
  bool is(const char *a, const char *b = nullptr) const { return o == a || (b && o == b); }
  std::string one() { if (i + 1 >= argc) die("missing value for " + o); return argv[++i]; }
  int one_int() { return atoi(one().c_str()); }
  double one_double() { return atof(one().c_str()); }
  void multi(std::vector<std::string> &dst) { while (i + 1 < argc && !is_opt(argv[i + 1])) dst.push_back(argv[++i]); }   // all following non-options
  void ints(std::vector<int> &dst) { while (i + 1 < argc && !is_opt(argv[i + 1])) dst.push_back(atoi(argv[++i])); }
  void doubles(std::vector<double> &dst) { while (i + 1 < argc && !is_opt(argv[i + 1])) dst.push_back(atof(argv[++i])); }
  // po::value<bool> options of the reference take a value (--debug 1); a bare flag is accepted as `bare`
  bool opt_bool(bool bare) {
    if (i + 1 < argc) {
      const std::string v = argv[i + 1];
      if (v == "1" || v == "true" || v == "yes" || v == "on") { ++i; return true; }
      if (v == "0" || v == "false" || v == "no" || v == "off") { ++i; return false; }
    }
    return bare;
  }
};

// StackRegistrations (RG.cc:849-1001; irtkStack3D3DRegistration<T>::run, PBR.cpp:280-285): every stack to the template, ts in and out
void stack_registrations(svr_ctx *ctx, const std::vector<Image> &stacks, std::vector<M4> &ts, size_t tmpl, const Image *mask, int flags) {
  const size_t n = stacks.size();
  std::vector<svr_image_attr> at(n);
  std::vector<const double *> ptr(n);
  std::vector<double> tm(16 * n);
  for (size_t k = 0; k < n; ++k) { at[k] = stacks[k].a; ptr[k] = stacks[k].d.data(); for (int q = 0; q < 16; ++q) tm[16 * k + q] = ts[k].m[q]; }
  long evals = 0;
  char e[256] = {0};
  if (svrh_stack_registrations(ctx, nullptr, (int)n, at.data(), ptr.data(), tm.data(), (int)tmpl, mask ? &mask->a : nullptr, mask ? mask->d.data() : nullptr,
                               flags, &evals, e))
    die(std::string("stack registration: ") + e);
  for (size_t k = 0; k < n; ++k) for (int q = 0; q < 16; ++q) ts[k].m[q] = tm[16 * k + q];
  fprintf(stderr, "stack-to-stack registration: %ld similarity evaluations\n", evals);
}

// the PSF volume's image-to-world / world-to-image matrices: PSF_SIZE 128 (RC.cuh:56) at the volume's voxel size, RG.cc:1534-1551
void psf_volume_matrices(const svr_image_attr &tattr, float pi2w[16], float pw2i[16]) {
  svr_image_attr pa;
  memset(&pa, 0, sizeof(pa));
  pa.nx = pa.ny = pa.nz = 128; pa.dx = tattr.dx; pa.dy = tattr.dy; pa.dz = tattr.dz;
  pa.xaxis[0] = pa.yaxis[1] = pa.zaxis[2] = 1.0;
  to_f16(image_to_world(pa), pi2w); to_f16(world_to_image(pa), pw2i);
}

// A unit's normal in volume axes for the sharding work estimates: reconW2I * T * unitI2W applied to the unit's z direction; nv is not
// normalised, len = |nv|^2.  The two work formulas stay with their callers and differ in the last bit (they feed spatial_order's cut
// points), so nothing here may change a caller's arithmetic: t keeps the caller's type (SVR: the double T, PVR: the float st; a float
// operand is promoted to double exactly, as in the expressions this restates) and the sums keep their order.
template <class TT> void normal_in_volume_axes(const float *i2w, const TT *t, const M4 &rw, double nv[3], double &len) {
  double nw[3], nt[3];
  len = 0;
  for (int k = 0; k < 3; ++k) nw[k] = i2w[4 * k + 2];
  for (int k = 0; k < 3; ++k) nt[k] = t[4 * k] * nw[0] + t[4 * k + 1] * nw[1] + t[4 * k + 2] * nw[2];
  for (int k = 0; k < 3; ++k) { nv[k] = rw.m[4 * k] * nt[0] + rw.m[4 * k + 1] * nt[1] + rw.m[4 * k + 2] * nt[2]; len += nv[k] * nv[k]; }
}

// ---- ranks: one engine context per device of -d.  Rank r holds the units [rlo[r], rhi[r]) of the SHARDED numbering (rank after rank);
// order[k] = unit k's index in the reference's order, inv_order its inverse.  The host objects (svrh_recon* / pvrh_recon*) differ in
// type and stay with each program, one vector beside this. ------------------------------------------------------------------------
struct Ranks {
  int nr = 1;
  std::vector<int> rlo, rhi, order, inv_order;
  std::vector<svr_ctx *> ctxs;
  svr_group *group = nullptr;

  void init(int ranks, int units) {                     // one rank's worth: everything in the reference's order
    nr = ranks;
    rlo.assign(nr, 0); rhi.assign(nr, units); order.resize(units); inv_order.resize(units);
    for (int s = 0; s < units; ++s) order[s] = inv_order[s] = s;
    ctxs.assign(nr, nullptr);
  }
  void create_context(int r, int device) {
    if (svr_create(device, &ctxs[r]) || !ctxs[r]) die("no usable HIP device " + std::to_string(device) + " (svr_create failed)");
  }
  void create_group(const std::vector<int> &devices) {
    group = nr > 1 ? svr_group_create(nr, devices.data()) : nullptr;
    if (nr > 1 && !group) die("cannot set up the rank group (librccl not found?)");
  }
  // every rank in its own thread (the collectives inside block until all ranks have arrived)
  void par(const std::function<void(int)> &fn) const {
    if (nr == 1) { fn(0); return; }
    std::vector<std::thread> th;
    for (int r = 0; r < nr; ++r) th.emplace_back(fn, r);
    for (auto &t : th) t.join();
  }
  void check(int r, int rc, const char *what) const { if (rc) die(std::string(what) + ": " + svr_last_error(ctxs[r])); }
  // rank r's rows of the per-unit matrices (sharded numbering) and the volume's own
  void set_matrices(int r, const std::vector<float> &st, const std::vector<float> &sti, const std::vector<float> &i2w, const std::vector<float> &w2i,
                    const float *ri2w, const float *rw2i) const {
    const size_t o = 16 * (size_t)rlo[r];
    check(r, svr_set_slice_matrices(ctxs[r], st.data() + o, sti.data() + o, i2w.data() + o, w2i.data() + o, i2w.data() + o, w2i.data() + o, ri2w, rw2i),
          "svr_set_slice_matrices");
  }
  // UpdateGPUTranformationMatrices RG.cc:372-401, updateTransformationMatrices patchBasedObject.cuh:151-169: T (double) -> st / sti, every rank
  void update_matrices(const std::vector<double> &T, std::vector<float> &st, std::vector<float> &sti, const std::vector<float> &i2w,
                       const std::vector<float> &w2i, const float *ri2w, const float *rw2i) const {
    for (size_t s = 0; s < T.size() / 16; ++s) {
      M4 t;
      for (int q = 0; q < 16; ++q) t.m[q] = T[16 * s + q];
      to_f16(t, &st[16 * s]); to_f16(inverse_rigid_or_affine(t), &sti[16 * s]);
    }
    for (int r = 0; r < nr; ++r) set_matrices(r, st, sti, i2w, w2i, ri2w, rw2i);
  }
  // `between`: what a program adds between the device list and the collectives (PVR: the patches per rank)
  void describe(const std::vector<int> &devices, const std::string &between) const {
    if (nr < 2) return;
    std::string t;
    for (int d : devices) t += " " + std::to_string(d);
    fprintf(stderr, "%d ranks on devices%s%s, collectives: %s\n", nr, t.c_str(), between.c_str(),
            svr_group_uses_rccl(group) ? "RCCL" : "host memory (a device is named more than once: test mode)");
  }
  void destroy() {                                      // after the program's host objects
    svr_group_destroy(group);
    for (int r = 0; r < nr; ++r) svr_destroy(ctxs[r]);
  }
};
// an engine call of rank r that must not fail: dies with `<the call's text>: <svr_last_error>`
#define ENGR(R, r, call) (R).check(r, (call), #call)

}  // namespace
#endif
