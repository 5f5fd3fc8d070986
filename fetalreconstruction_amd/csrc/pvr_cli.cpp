// pvr_cli.cpp -- `PVRreconstructionGPU`: the reference's patch-to-volume command line (source/reconstructionGPU2/
// patchBasedReconMain.cpp, "pvrmain") over the MI355X engine, in C++ like the reference's own main().
//
//   PVRreconstructionGPU -o recon.nii.gz -i s1.nii.gz s2.nii.gz ... -m mask.nii.gz [--patchSize 32 32]
//                        [--patchStride 16 16] [--resolution 0.75] [--iterations 7] [--sr_iterations 7] ...
//
// Option names and defaults: pvrmain:108-131.  Set-up (irtkPatchBasedReconstruction<T>::run,
// irtkPatchBasedReconstruction.cpp = "PBR.cpp" :193-310): binarise the mask, crop every stack to it, resample the
// mask to the isotropic voxel size (nearest neighbour), match the stack intensities (:656-790, target = mean of all
// positive voxels), min/max intensities (:792-814), CreateTemplate (:941-965), the reconstruction mask (:303-304);
// then PatchBasedVolume::generate2DPatches per stack (patchBasedObject.cuh:176-342) and `iterations + 1` passes of
// the loop in csrc/pvr_host.cpp (PBR.cpp:445-593).  The Python twin is tests/twins/pvr_cli.py.
//
// The stack-to-stack registration (irtkStack3D3DRegistration, :280-285) runs through csrc/irtk_reg.cpp with every similarity
// on the GPU; between the outer passes every patch is registered to the volume with the same schedule
// (patchBased2D3DRegistration<T>::runHybrid, what PBR.cpp:472-476 calls); --no_registration (not a reference option) skips both.
// -s / --superpixel cuts SLICO superpixel patches (csrc/svr_slic.h).  --useFullSlices makes every slice one patch (patchBasedObject.cuh:183-189).
// --existingReconTarget starts from a given volume (and its grid); --hierarchical runs iterations + 1 levels of shrinking patches (pvrmain:359-432).
// --dilateMask n dilates the mask n times, --packages p_1 .. p_N splits every stack into its interleaved packages (PBR.cpp:134-146).
// --resample resamples the cropped stacks to the output voxel size with IRTK's cubic B-spline interpolator.
//
// Where things are.  Plain structs: Options (what the command line says; const after parse_options), Problem (the stacks, masks and
// template of the set-up, the same for every level), Level (what one run of the loop is asked for) with its LevelPatches (what it
// cuts and uploads), and Ranks (svr_launch.h) with one pvrh_recon* per rank.
//   pre-processing     resample_attr, match_stack_intensities_pvr, dilate_mask, resample_bspline, split_packages
//   patches            generate_2d_patches, append; cut_patches (square, full-slice, superpixel)
//   options            usage, parse_options
//   set-up             read_inputs, crop_to_mask, register_stacks, make_template
//   one level          run_level: cut_patches, dump_problem, shard_patches, setup_engines, run_iterations (register_patches)
// main() is the set-up, then one level or the hierarchical driver (first_level, the shrinking patch sizes), then the volume.
#include <float.h>

#include <future>

#include "svr_launch.h"
#include "svr_slic.h"

namespace {

// irtkResampling::Initialize (irtkResampling.cc:74-130): int(n d_old / d) voxels of size d, same axes and origin
svr_image_attr resample_attr(const svr_image_attr &in, double d) {
  svr_image_attr a = in;
  int n[3] = {(int)(a.nx * a.dx / d), (int)(a.ny * a.dy / d), (int)(a.nz * a.dz / d)};
  double s[3] = {d, d, d};
  const double old[3] = {a.dx, a.dy, a.dz};
  for (int k = 0; k < 3; ++k) if (n[k] < 1) { n[k] = 1; s[k] = old[k]; }
  a.nx = n[0]; a.ny = n[1]; a.nz = n[2]; a.dx = s[0]; a.dy = s[1]; a.dz = s[2];
  return a;
}

// MatchStackIntensitiesWithMasking PBR.cpp:656-790
void match_stack_intensities_pvr(std::vector<Image> &stacks, const std::vector<M4> &ts, const Image &mask) {
  float average = 0;                                    // T m_average_value, accumulated voxel by voxel
  unsigned long long count = 0;
  for (const Image &s : stacks)
    for (double v : s.d)
      if (v > 0) { average += (float)v; count++; }
  if (count) average /= count;
  const M4 mw2i = world_to_image(mask.a);
  std::vector<double> avg(stacks.size());
  parallel_for((int)stacks.size(), [&](int s) {             // a stack per host thread; the sums of a stack keep the reference's order
    const Image &st = stacks[s];
    const M4 s_i2w = image_to_world(st.a);
    double sum = 0, num = 0;
    for (int z = 0; z < st.a.nz; ++z)
      for (int y = 0; y < st.a.ny; ++y)
        for (int x = 0; x < st.a.nx; ++x) {
          double qx = x, qy = y, qz = z;
          apply_point(s_i2w, qx, qy, qz); apply_point(ts[s], qx, qy, qz); apply_point(mw2i, qx, qy, qz);
          const long i = (long)irtk_round(qx), j = (long)irtk_round(qy), k = (long)irtk_round(qz);
          if (i >= 0 && i < mask.a.nx && j >= 0 && j < mask.a.ny && k >= 0 && k < mask.a.nz &&
              mask.at((int)i, (int)j, (int)k) == 1 && st.at(x, y, z) > 0) {
            sum += st.at(x, y, z);
            num += 1;
          }
        }
    if (!(num > 0)) die("a stack has no overlap with the ROI");
    avg[s] = sum / num;
  });
  for (size_t s = 0; s < stacks.size(); ++s) {
    const double f = average / avg[s];
    for (double &v : stacks[s].d) if (v > 0) v = (double)(float)(v * f);      // float voxels times a double factor
  }
}

// irtkDilation<T> with CONNECTIVITY_26 (irtkDilation.cc:50-78): an interior voxel becomes the maximum of its 26 neighbours and
// itself, the voxels on the faces of the image keep their value
void dilate_mask(Image &m, int iterations) {
  const int nx = m.a.nx, ny = m.a.ny, nz = m.a.nz;
  for (int it = 0; it < iterations; ++it) {
    const std::vector<double> in = m.d;
    for (int z = 1; z + 1 < nz; ++z)
      for (int y = 1; y + 1 < ny; ++y)
        for (int x = 1; x + 1 < nx; ++x) {
          double v = in[((size_t)z * ny + y) * nx + x];
          for (int dz = -1; dz <= 1; ++dz)
            for (int dy = -1; dy <= 1; ++dy)
              for (int dx = -1; dx <= 1; ++dx) v = std::max(v, in[((size_t)(z + dz) * ny + (y + dy)) * nx + (x + dx)]);
          m.d[((size_t)z * ny + y) * nx + x] = v;
        }
  }
}

// ConvertToInterpolationCoefficients, cubic spline, mirror boundaries (irtkBSplineInterpolateImageFunction.cc:68-144)
void bspline_coefficients(double *c, int n) {
  if (n == 1) return;
  const double z = sqrt(3.0) - 2.0;
  const double lambda = (1.0 - z) * (1.0 - 1.0 / z);
  for (int k = 0; k < n; ++k) c[k] *= lambda;
  const int horizon = (int)ceil(log(DBL_EPSILON) / log(fabs(z)));
  double zn = z, sum;
  if (horizon < n) {
    sum = c[0];
    for (int k = 1; k < horizon; ++k) { sum += zn * c[k]; zn *= z; }
    c[0] = sum;
  } else {
    const double iz = 1.0 / z;
    double z2n = pow(z, (double)(n - 1));
    sum = c[0] + z2n * c[n - 1];
    z2n *= z2n * iz;
    for (int k = 1; k <= n - 2; ++k) { sum += (zn + z2n) * c[k]; zn *= z; z2n *= iz; }
    c[0] = sum / (1.0 - zn * zn);
  }
  for (int k = 1; k < n; ++k) c[k] += z * c[k - 1];
  c[n - 1] = (z / (z * z - 1.0)) * (z * c[n - 2] + c[n - 1]);
  for (int k = n - 2; k >= 0; --k) c[k] = z * (c[k + 1] - c[k]);
}

// irtkResampling<T> with irtkBSplineInterpolateImageFunction (cubic, clamped to the input's range): what --resample does to every
// cropped stack (PBR.cpp:225-246; irtkResampling.cc:74-175, irtkBSplineInterpolateImageFunction.cc:146-433); float voxels
Image resample_bspline(const Image &img, double d) {
  const svr_image_attr &a = img.a;
  const int nx = a.nx, ny = a.ny, nz = a.nz;
  std::vector<double> coeff = img.d, line((size_t)std::max(nx, std::max(ny, nz)));
  auto C = [&](int x, int y, int z) -> double & { return coeff[((size_t)z * ny + y) * nx + x]; };
  for (int z = 0; z < nz; ++z)
    for (int y = 0; y < ny; ++y) bspline_coefficients(&C(0, y, z), nx);
  for (int z = 0; z < nz; ++z)
    for (int x = 0; x < nx; ++x) {
      for (int y = 0; y < ny; ++y) line[y] = C(x, y, z);
      bspline_coefficients(line.data(), ny);
      for (int y = 0; y < ny; ++y) C(x, y, z) = line[y];
    }
  for (int y = 0; y < ny; ++y)
    for (int x = 0; x < nx; ++x) {
      for (int z = 0; z < nz; ++z) line[z] = C(x, y, z);
      bspline_coefficients(line.data(), nz);
      for (int z = 0; z < nz; ++z) C(x, y, z) = line[z];
    }
  double vmin = img.d[0], vmax = img.d[0];
  for (double v : img.d) { vmin = std::min(vmin, v); vmax = std::max(vmax, v); }
  Image out;
  out.a = resample_attr(a, d);
  out.d.resize((size_t)out.a.nx * out.a.ny * out.a.nz);
  const M4 m = mul(world_to_image(a), image_to_world(out.a));
  const int dims[3] = {nx, ny, nz};
  for (int k = 0; k < out.a.nz; ++k)
    for (int j = 0; j < out.a.ny; ++j)
      for (int i = 0; i < out.a.nx; ++i) {
        int idx[3][4];
        double wgt[3][4];
        for (int r = 0; r < 3; ++r) {
          const double x = m.m[4 * r] * i + m.m[4 * r + 1] * j + m.m[4 * r + 2] * k + m.m[4 * r + 3];
          const int i0 = (int)floor(x) - 1;
          const double w = x - (double)(i0 + 1);
          wgt[r][3] = (1.0 / 6.0) * w * w * w;
          wgt[r][0] = (1.0 / 6.0) + (1.0 / 2.0) * w * (w - 1.0) - wgt[r][3];
          wgt[r][2] = w + wgt[r][0] - 2.0 * wgt[r][3];
          wgt[r][1] = 1.0 - wgt[r][0] - wgt[r][2] - wgt[r][3];
          const int n = dims[r], half = 2 * n - 2;
          for (int q = 0; q < 4; ++q) {
            int v = i0 + q;
            v = (n == 1) ? 0 : (v < 0 ? -v - half * ((-v) / half) : v - half * (v / half));
            if (n <= v) v = half - v;
            idx[r][q] = v;
          }
        }
        double value = 0.0;
        for (int c = 0; c < 4; ++c)
          for (int b = 0; b < 4; ++b)
            for (int e = 0; e < 4; ++e) value += wgt[0][e] * wgt[1][b] * wgt[2][c] * C(idx[0][e], idx[1][b], idx[2][c]);
        value = std::min(std::max(value, vmin), vmax);
        out.d[((size_t)k * out.a.ny + j) * out.a.nx + i] = (double)(float)value;
      }
  return out;
}

// patchBasedPackageSplitter<T>::makePackageVolumes (patchBasedPackageSplitter.cpp:76-146): package l holds slices l, l + packages, ...
// of the stack at `packages` times the slice spacing, with its first voxel where slice l's first voxel was
std::vector<Image> split_packages(const Image &stack, int packages) {
  std::vector<Image> out;
  const svr_image_attr &a = stack.a;
  const int pkg_z = a.nz / packages;
  const M4 i2w = image_to_world(a);
  for (int l = 0; l < packages; ++l) {
    Image p;
    p.a = a;
    p.a.nz = (pkg_z * packages + l < a.nz) ? pkg_z + 1 : pkg_z;
    p.a.dz = a.dz * packages;
    const M4 first = image_to_world(p.a);
    for (int k = 0; k < 3; ++k) p.a.origin[k] += (i2w.m[4 * k + 2] * l + i2w.m[4 * k + 3]) - first.m[4 * k + 3];
    p.d.resize((size_t)p.a.nx * p.a.ny * p.a.nz);
    const size_t plane = (size_t)a.nx * a.ny;
    for (int k = 0; k < p.a.nz; ++k) memcpy(&p.d[(size_t)k * plane], &stack.d[(size_t)(k * packages + l) * plane], plane * sizeof(double));
    out.push_back(std::move(p));
  }
  return out;
}

struct Patches {
  std::vector<float> data, i2w, w2i;                   // [n][py][px], [n][16], [n][16]
  std::vector<float> ri2w, mo, invmo;                  // the origin-reset matrices (patchBasedObject.cuh:285-304), [n][16] each
  std::vector<svr_image_attr> attr;                    // the patches as images (targets of the patch-to-volume registration)
  int n = 0;
};

// A patch pixel sits exactly on a slice pixel (and, for a mask drawn on the stack's grid, on a mask voxel): its coordinate is an
// integer in exact arithmetic, and the reference truncates what the double arithmetic makes of it (patchBasedObject.cuh:262-277),
// so on an oblique grid 19.999999999999996 reads pixel 19 or 20 depending on the last bit.  Here a coordinate within 1e-6 of an
// integer IS that integer; everything else is untouched.
inline double snap(double v) { const double r = nearbyint(v); return fabs(v - r) < 1e-6 ? r : v; }

// PatchBasedVolume<T>::generate2DPatches, patchBasedObject.cuh:176-342
template <class From> void append(Patches &to, const From &from) {     // From: Patches, or the superpixel cutter's SpxPatches
  to.data.insert(to.data.end(), from.data.begin(), from.data.end());
  to.i2w.insert(to.i2w.end(), from.i2w.begin(), from.i2w.end()); to.w2i.insert(to.w2i.end(), from.w2i.begin(), from.w2i.end());
  to.ri2w.insert(to.ri2w.end(), from.ri2w.begin(), from.ri2w.end()); to.mo.insert(to.mo.end(), from.mo.begin(), from.mo.end());
  to.invmo.insert(to.invmo.end(), from.invmo.begin(), from.invmo.end());
  to.attr.insert(to.attr.end(), from.attr.begin(), from.attr.end());
  to.n += from.n;
}

void generate_2d_patches(const Image &stack, double thickness, const Image &mask, int px, int py, int sx, int sy, Patches &result) {
  const svr_image_attr &a = stack.a;
  const M4 m_w2i = world_to_image(mask.a);
  std::vector<Patches> per_slice(a.nz);                  // the slices are cut on the host threads and appended in slice order
  parallel_for(a.nz, [&](int z) {
    Patches &out = per_slice[z];
    std::vector<float> patch((size_t)px * py);
    {
    svr_image_attr sl = a;                               // GetRegion(0, 0, z, x, y, z + 1) + PutPixelSize :202-203
    sl.nz = 1;
    sl.dz = thickness * 2;
    region_origin(a, 0, 0, z, sl);
    const M4 sl_i2w = image_to_world(sl), sl_w2i = world_to_image(sl);
    svr_image_attr p0 = sl;
    p0.nx = px; p0.ny = py;
    p0.origin[0] = p0.origin[1] = p0.origin[2] = 0;
    const M4 p0_i2w = image_to_world(p0);
    for (int y = 0; y < a.ny + py; y += sy)
      for (int x = 0; x < a.nx + px; x += sx) {
        svr_image_attr pa = p0;                          // shift the origin so that pixel (0,0) sits on slice pixel (x,y) :232-246
        for (int k = 0; k < 3; ++k) pa.origin[k] = (sl_i2w.m[4 * k] * x + sl_i2w.m[4 * k + 1] * y + sl_i2w.m[4 * k + 3]) - p0_i2w.m[4 * k + 3];
        const M4 p_i2w = image_to_world(pa);
        int set_count = 0;
        for (int j = 0; j < py; ++j)
          for (int i = 0; i < px; ++i) {
            double wx = i, wy = j, wz = 0;                 // patch.ImageToWorld, then slice / mask WorldToImage (:262-277)
            apply_point(p_i2w, wx, wy, wz);
            double xx = wx, yy = wy, zz = wz, x1 = wx, y1 = wy, z1 = wz;
            apply_point(sl_w2i, xx, yy, zz);
            apply_point(m_w2i, x1, y1, z1);
            xx = snap(xx); yy = snap(yy); x1 = snap(x1); y1 = snap(y1); z1 = snap(z1);
            float v = 0;                                 // a patch starts as an all-zero image
            if (xx >= 0 && yy >= 0 && xx < a.nx && yy < a.ny && x1 >= 0 && y1 >= 0 && z1 >= 0 && x1 < mask.a.nx && y1 < mask.a.ny &&
                z1 < mask.a.nz && mask.at((int)x1, (int)y1, (int)z1) > 0) {
              v = (float)stack.at((int)xx, (int)yy, z);
              if (v != 0 && v != -1) set_count++;
            }
            patch[(size_t)j * px + i] = v;
          }
        if (set_count > 1.0f / 3.0f * py * px) {         // :318
          out.data.insert(out.data.end(), patch.begin(), patch.end());
          float f[16];
          to_f16(p_i2w, f); out.i2w.insert(out.i2w.end(), f, f + 16);
          to_f16(world_to_image(pa), f); out.w2i.insert(out.w2i.end(), f, f + 16);
          to_f16(p0_i2w, f); out.ri2w.insert(out.ri2w.end(), f, f + 16);           // RI2W: the patch with its origin at 0
          M4 mo = ident();
          for (int k = 0; k < 3; ++k) mo.m[4 * k + 3] = pa.origin[k];
          to_f16(mo, f); out.mo.insert(out.mo.end(), f, f + 16);
          to_f16(inverse_rigid_or_affine(mo), f); out.invmo.insert(out.invmo.end(), f, f + 16);
          out.attr.push_back(pa);
          out.n++;
        }
      }
    }
  });
  for (const Patches &p : per_slice) append(result, p);
}

// ---- options (pvrmain:108-131) -----------------------------------------------------------------------
struct Options {
  std::string output, mask_name;
  std::vector<std::string> inputs, tspecs;
  std::vector<double> thickness;
  std::vector<int> devices, psize, pstride, packages;
  int iterations = 7, sr_iterations = 7, dilate = 0;
  double resolution = 0.75;
  bool no_matching = false, dry_run = false, no_registration = false, superpixel = false, full_slices = false, hierarchical = false, resample = false, coeff_table = false;
  int spx_size = 16, spx_extend = 50;                    // pvrmain:104-106
  std::string existing_name;                             // --existingReconTarget (pvrmain:118)
  std::string dump_name;                                 // test hooks: --dumpProblem <file> [--dryRun]
};

// the set-up's result (pvrmain:184-257, PBR.cpp:193-310): the same for every level
struct Problem {
  std::vector<Image> stacks;                             // the packages, where --packages splits them; cropped (and resampled)
  std::vector<M4> ts;
  std::vector<double> half_thickness;                    // m_thickness: dz, or the given thickness / 2 (pvrmain:209-217)
  size_t tmpl = 0;
  Image mask, iso_mask, recon_mask;
  svr_image_attr tattr;
  float vmin = 3.402823466e38f, vmax = 1.175494351e-38f;
  std::vector<float> existing;                           // setExistingReconstructionTarget :185-191: the volume and its grid
};

// one irtkPatchBasedReconstruction<T>::run from the patch extraction on
struct Level {
  std::vector<int> psize, pstride;
  int spx_size, iterations;
  std::vector<float> existing;                           // the volume it starts from, or none
  bool dump;                                             // --dumpProblem describes the first level
};

// what a level cuts and uploads; the per-patch arrays are in the global numbering (stack after stack) until shard_patches
struct LevelPatches {
  Patches P;
  int px = 0, py = 0;
  std::vector<char> spx_masks;
  std::vector<int> counts;                               // patches per stack
  std::vector<float> st, sti, dims;
  std::vector<double> Td;                                // the registrators' m_transformations, one per patch
  float vol_i2w[16], vol_w2i[16];                        // the volume's own matrices
};

void host_check(pvrh_recon *h, int rc, const char *what) { if (rc) die(std::string(what) + ": " + pvrh_last_error(h)); }
#define PVRHR(r, call) host_check(hosts[r], (call), #call)

void usage() {
  printf("usage: PVRreconstructionGPU -o <volume> -i <stack_1> .. <stack_N> -m <mask> [-t id|<dof>|<4x4.txt> ..]\n"
         "       [--thickness th_1 ..] [--patchSize 32 32] [--patchStride 16 16] [--resolution 0.75] [--iterations 7]\n"
         "       [--sr_iterations 7] [--noMatchIntensities] [--no_registration] [-s [--spxSize 16] [--spxExtend 50]] [--useFullSlices] [-d device]\n");
}

Options parse_options(int argc, char **argv) {
  Options p;
  Args a{argc, argv};
  while (a.next()) {
    if (a.is("-o", "--output")) p.output = a.one();
    else if (a.is("-m", "--mask")) p.mask_name = a.one();
    else if (a.is("-i", "--input")) a.multi(p.inputs);
    else if (a.is("-t", "--transformation")) a.multi(p.tspecs);
    else if (a.is("--thickness")) a.doubles(p.thickness);
    else if (a.is("--useFullSlices")) p.full_slices = true;
    else if (a.is("--hierarchical")) p.hierarchical = true;
    else if (a.is("--resample")) p.resample = true;
    else if (a.is("--packages")) a.ints(p.packages);
    else if (a.is("--dilateMask")) p.dilate = a.one_int();
    else if (a.is("--existingReconTarget")) p.existing_name = a.one();
    else if (a.is("--patchSize")) a.ints(p.psize);
    else if (a.is("--patchStride")) a.ints(p.pstride);
    else if (a.is("--resolution")) p.resolution = a.one_double();
    else if (a.is("--iterations")) p.iterations = a.one_int();
    else if (a.is("--sr_iterations")) p.sr_iterations = a.one_int();
    else if (a.is("--noMatchIntensities")) p.no_matching = true;
    else if (a.is("--coeffTable")) p.coeff_table = true;                   // not a reference option: keep the PSF taps in HBM
    else if (a.is("-d", "--devices")) a.ints(p.devices);
    else if (a.is("--dumpProblem")) p.dump_name = a.one();
    else if (a.is("--dryRun")) p.dry_run = true;
    else if (a.is("--no_registration")) p.no_registration = true;
    else if (a.is("-s", "--superpixel")) p.superpixel = true;
    else if (a.is("--spxSize")) p.spx_size = a.one_int();
    else if (a.is("--spxExtend")) p.spx_extend = a.one_int();
    else if (a.is("-h", "--help")) { usage(); exit(0); }
    else die("option " + a.o + " is not supported by this build (see csrc/pvr_cli.cpp)");
  }
  if (p.output.empty() || p.inputs.empty() || p.mask_name.empty()) die("-o, -i and -m are required (try --help)");
  if (p.psize.empty()) p.psize = {32, 32};
  if (p.pstride.empty()) p.pstride = {16, 16};
  if (p.psize.size() != 2 || p.pstride.size() != 2 || p.psize[0] < 1 || p.psize[1] < 1 || p.pstride[0] < 1 || p.pstride[1] < 1)
    die("--patchSize and --patchStride take two positive integers");
  if (p.tspecs.empty()) p.tspecs.assign(p.inputs.size(), "id");
  if (p.tspecs.size() != p.inputs.size()) die("one transformation per stack expected");
  return p;
}

// ---- set-up (pvrmain:184-257, PBR.cpp:193-310) --------------------------------------------------------
// the stacks and their transformations, the thicknesses, the template's number; with --packages every package becomes a stack
void read_inputs(const Options &opt, Problem &S) {
  size_t n = opt.inputs.size();
  S.stacks.resize(n);
  parallel_for((int)n, [&](int k) { S.stacks[k] = read_image(opt.inputs[k]); });                 // gunzip is serial per file
  for (size_t k = 0; k < n; ++k) S.ts.push_back(load_transformation(opt.tspecs[k]));
}

void split_stacks(const Options &opt, Problem &S) {
  const size_t n = S.stacks.size();
  if (opt.thickness.empty()) for (auto &s : S.stacks) S.half_thickness.push_back(s.a.dz);
  else { if (opt.thickness.size() != n) die("one thickness per stack expected"); for (double t : opt.thickness) S.half_thickness.push_back(t / 2.0); }
  for (size_t k = 0; k < n; ++k) if (opt.tspecs[k] == "id") { S.tmpl = k; break; }
  if (opt.packages.size() != n) return;
  std::vector<Image> ps;                                 // setImageStacks, PBR.cpp:134-146: every package becomes a stack of its own;
  std::vector<M4> pt;                                    // m_template_num keeps indexing the new list
  std::vector<double> ph;
  for (size_t k = 0; k < n; ++k) {
    if (opt.packages[k] < 1) die("--packages takes positive integers");
    for (Image &p : split_packages(S.stacks[k], opt.packages[k])) { ps.push_back(std::move(p)); pt.push_back(S.ts[k]); ph.push_back(S.half_thickness[k]); }
  }
  S.stacks.swap(ps); S.ts.swap(pt); S.half_thickness.swap(ph);
}

void crop_to_mask(const Options &opt, Problem &S) {
  S.mask = read_image(opt.mask_name);
  for (double &v : S.mask.d) v = ((long long)v == 0) ? 0.0 : 1.0;                                // PBR.cpp:201-209
  if (opt.dilate > 0) dilate_mask(S.mask, opt.dilate);                                           // :212-223
  for (size_t k = 0; k < S.stacks.size(); ++k) {                                                 // :229-236
    const Image m = transform_nn(S.mask, S.stacks[k].a, S.ts[k], 0.0);
    S.stacks[k] = crop_image(S.stacks[k], m);
    if (opt.resample) S.stacks[k] = resample_bspline(S.stacks[k], opt.resolution);             // :237-246
  }
}

void register_stacks(const Options &opt, Problem &S) {   // irtkStack3D3DRegistration<T>::run, :280-285
  svr_ctx *rctx = nullptr;
  if (svr_create(opt.devices.empty() ? 0 : opt.devices[0], &rctx) || !rctx) die("no usable HIP device (svr_create failed)");
  stack_registrations(rctx, S.stacks, S.ts, S.tmpl, &S.iso_mask, SVRH_STACKREG_KEEP_ORIGIN);
  svr_destroy(rctx);
}

void make_template(const Options &opt, Problem &S) {
  for (const Image &s : S.stacks)                                                                // computeMinMaxIntensities :792-814
    for (double v : s.d)
      if (v > 0) { S.vmax = std::max(S.vmax, (float)v); S.vmin = std::min(S.vmin, (float)v); }
  S.tattr = resample_attr(S.stacks[S.tmpl].a, opt.resolution);                                   // CreateTemplate :941-965
  if (!opt.existing_name.empty()) {
    const Image ex = read_image(opt.existing_name);
    S.tattr = ex.a;
    S.existing.assign(ex.d.begin(), ex.d.end());
  }
  S.recon_mask = transform_nn(S.iso_mask, S.tattr, S.ts[S.tmpl], 0.0);                           // :303-304
}

// ---- one level -------------------------------------------------------------------------------------------
// patches (PBR.cpp:385-399): square patches, every slice as one patch, or superpixels; per patch its stack's transformation and voxel size
void cut_patches(const Options &opt, const Problem &S, const Level &lv, LevelPatches &C) {
  Patches &P = C.P;
  const size_t n = S.stacks.size();
  int &px = C.px, &py = C.py;
  px = lv.psize[0]; py = lv.psize[1];
  if (opt.full_slices) {                                 // the patch is the slice; stacks of different sizes share a grid padded with -1
    px = py = 0;
    for (size_t k = 0; k < n; ++k) { px = std::max(px, S.stacks[k].a.nx); py = std::max(py, S.stacks[k].a.ny); }
  }
  for (size_t k = 0; k < n; ++k) {
    const int before = P.n;
    if (opt.superpixel) {                                // pvrmain:291-296: patch size = spxSize, stride = spxExtend
      SpxPatches sp;
      slic_superpixel_patches(S.stacks[k], S.half_thickness[k], S.iso_mask, lv.spx_size, lv.spx_size, opt.spx_extend, sp);
      if (P.n > 0 && (sp.px != px || sp.py != py)) die("superpixel patches of different sizes (slices narrower than 64 pixels differ between the stacks)");
      px = sp.px; py = sp.py;
      append(P, sp);
      C.spx_masks.insert(C.spx_masks.end(), sp.masks.begin(), sp.masks.end());
    } else if (opt.full_slices) {                        // patchBasedObject.cuh:183-189: size = the slice, stride = size + 1
      const int nx = S.stacks[k].a.nx, ny = S.stacks[k].a.ny;
      Patches one;
      generate_2d_patches(S.stacks[k], S.half_thickness[k], S.iso_mask, nx, ny, nx + 1, ny + 1, one);
      std::vector<float> padded((size_t)one.n * px * py, -1.0f);
      for (int q = 0; q < one.n; ++q)
        for (int j = 0; j < ny; ++j) memcpy(&padded[((size_t)q * py + j) * px], &one.data[((size_t)q * ny + j) * nx], nx * sizeof(float));
      one.data.swap(padded);
      append(P, one);
    } else {
      generate_2d_patches(S.stacks[k], S.half_thickness[k], S.iso_mask, px, py, lv.pstride[0], lv.pstride[1], P);
    }
    C.counts.push_back(P.n - before);
    float t[16], ti[16];
    to_f16(S.ts[k], t); to_f16(inverse_rigid_or_affine(S.ts[k]), ti);
    for (int q = before; q < P.n; ++q) {
      C.st.insert(C.st.end(), t, t + 16); C.sti.insert(C.sti.end(), ti, ti + 16);
      C.Td.insert(C.Td.end(), S.ts[k].m, S.ts[k].m + 16);
      C.dims.push_back((float)S.stacks[k].a.dx); C.dims.push_back((float)S.stacks[k].a.dy); C.dims.push_back((float)S.stacks[k].a.dz);   // getDim()
    }
  }
}

// what the engine is about to receive, for the CPU tests
void dump_problem(const std::string &name, bool superpixel, const Problem &S, const LevelPatches &C) {
  const Patches &P = C.P;
  const svr_image_attr &tattr = S.tattr;
  FILE *f = fopen(name.c_str(), "wb");
  if (!f) die("cannot write " + name);
  const int hdr[8] = {P.n, C.px, C.py, (int)S.stacks.size(), tattr.nx, tattr.ny, tattr.nz, 1};   // [7] = 1: the geometry block at the end
  const float mm[2] = {S.vmin, S.vmax};
  std::vector<float> mf(S.recon_mask.d.begin(), S.recon_mask.d.end());
  fwrite(hdr, sizeof(int), 8, f); fwrite(C.counts.data(), sizeof(int), S.stacks.size(), f); fwrite(mm, sizeof(float), 2, f);
  fwrite(P.data.data(), sizeof(float), P.data.size(), f); fwrite(P.i2w.data(), sizeof(float), P.i2w.size(), f);
  fwrite(mf.data(), sizeof(float), mf.size(), f);
  if (superpixel) fwrite(C.spx_masks.data(), 1, C.spx_masks.size(), f);
  // everything else svr_set_slice_matrices / svr_set_slice_dims / svr_init_reconstruction_volume receive: per patch
  // w2i, T, Tinv, dims; the volume's image-to-world / world-to-image matrices and voxel size
  float gi2w[16], gw2i[16];
  to_f16(image_to_world(tattr), gi2w); to_f16(world_to_image(tattr), gw2i);
  const float gdim[3] = {(float)tattr.dx, (float)tattr.dy, (float)tattr.dz};
  fwrite(P.w2i.data(), sizeof(float), P.w2i.size(), f); fwrite(C.st.data(), sizeof(float), C.st.size(), f);
  fwrite(C.sti.data(), sizeof(float), C.sti.size(), f); fwrite(C.dims.data(), sizeof(float), C.dims.size(), f);
  fwrite(gi2w, sizeof(float), 16, f); fwrite(gw2i, sizeof(float), 16, f); fwrite(gdim, sizeof(float), 3, f);
  fclose(f);
}

// Ranks: one engine context per device of -d.  Rank r takes the r-th of nr work-balanced segments of EVERY stack's patches
// (svr_shard.h spatial_order: a rank's patches are neighbours in space), work = the pixels that carry data, weighted by orientation.
// From here on the per-patch arrays are in the SHARDED numbering (rank after rank); order[k] = patch k's index in the global numbering
// (stack after stack), which the host object keeps using where the reference's arithmetic depends on it (pvrh_set_unit_order).  The
// reference's patch-based path is single-GPU (patchBasedReconMain.cpp:78,177-179, irtkPatchBasedReconstruction.cpp:402); SURVEY 8e:
// "identical with patches as the unit"
void shard_patches(const Options &opt, const Problem &S, LevelPatches &C, Ranks &R) {
  Patches &P = C.P;
  const int ns = P.n, nr = (int)std::max<size_t>(1, opt.devices.size());
  if (ns < nr) die("fewer patches than devices");
  R.init(nr, ns);
  if (nr == 1) return;
  std::vector<double> work(ns, 0.0);
  const size_t pp = (size_t)C.px * C.py;
  const M4 rw = world_to_image(S.tattr);
  parallel_for(ns, [&](int q) {
    long c = 0;
    for (size_t i = 0; i < pp; ++i) c += P.data[(size_t)q * pp + i] > 0.0f;
    // a patch whose normal is the volume's x axis costs more per pixel (its runs span a band of centre planes, csrc/svr_cell.inc;
    // measured per rank: tools/shard_probe.py, sharding.py slice_cost_weights): x (1 + 0.2 n_x^2)
    double nv[3], len;
    normal_in_volume_axes(&P.i2w[16 * (size_t)q], &C.st[16 * (size_t)q], rw, nv, len);
    const double ax2 = len > 0 ? nv[0] * nv[0] / len : 0.0;
    work[q] = (double)c * (1.0 + 0.2 * ax2);
  });
  std::vector<int> stack_of;
  for (size_t k = 0; k < C.counts.size(); ++k) stack_of.insert(stack_of.end(), C.counts[k], (int)k);
  svr::spatial_order(work, stack_of, nr, R.order, R.rlo, R.rhi);
  for (int r = 0; r < nr; ++r) if (R.rhi[r] <= R.rlo[r]) die("a device would get no patch: fewer devices, please");
  for (int k = 0; k < ns; ++k) R.inv_order[R.order[k]] = k;
  svr::permute_rows(P.data, pp, R.order);
  svr::permute_rows(P.i2w, 16, R.order); svr::permute_rows(P.w2i, 16, R.order); svr::permute_rows(P.attr, 1, R.order);
  if (opt.superpixel) svr::permute_rows(C.spx_masks, 4096, R.order);
  svr::permute_rows(C.st, 16, R.order); svr::permute_rows(C.sti, 16, R.order); svr::permute_rows(C.dims, 3, R.order); svr::permute_rows(C.Td, 16, R.order);
}

// upload (the engine in PVR mode; m_quality_factor = 1, PBR.cpp:415), per rank, and every rank's host object
void setup_engines(const Options &opt, const Problem &S, const Level &lv, LevelPatches &C, const Ranks &R, std::vector<pvrh_recon *> &hosts) {
  const Patches &P = C.P;
  const svr_image_attr &tattr = S.tattr;
  const int px = C.px, py = C.py;
  const uint32_t vsize[3] = {(uint32_t)tattr.nx, (uint32_t)tattr.ny, (uint32_t)tattr.nz};
  const float vdim[3] = {(float)tattr.dx, (float)tattr.dy, (float)tattr.dz};
  const std::vector<float> maskf(S.recon_mask.d.begin(), S.recon_mask.d.end());
  to_f16(image_to_world(tattr), C.vol_i2w); to_f16(world_to_image(tattr), C.vol_w2i);
  if (!lv.existing.empty() && lv.existing.size() != (size_t)tattr.nx * tattr.ny * tattr.nz) die("existing reconstruction target of the wrong size");
  float pi2w[16], pw2i[16];
  psf_volume_matrices(tattr, pi2w, pw2i);
  hosts.assign(R.nr, nullptr);
  R.par([&](int r) {
    svr_ctx *c = R.ctxs[r];
    const int nl = R.rhi[r] - R.rlo[r];
    const size_t o = (size_t)R.rlo[r];
    ENGR(R, r, svr_set_option(c, "pvr", 1));
    if (opt.coeff_table) ENGR(R, r, svr_set_option(c, "coeff_table", 1));
    ENGR(R, r, svr_init_reconstruction_volume(c, vsize, vdim, lv.existing.empty() ? nullptr : lv.existing.data(), 12.0f));   // copyFromHost :310-314
    ENGR(R, r, svr_set_mask(c, vsize, vdim, maskf.data(), 12.0f));
    const uint32_t ssize[3] = {(uint32_t)px, (uint32_t)py, (uint32_t)nl};
    std::vector<int> sizes_x(nl, px), sizes_y(nl, py);
    ENGR(R, r, svr_init_storage_volumes(c, ssize, &C.dims[3 * o]));
    ENGR(R, r, svr_fill_slices(c, P.data.data() + o * px * py, sizes_x.data(), sizes_y.data()));
    if (opt.superpixel) ENGR(R, r, svr_set_spx_masks(c, C.spx_masks.data() + o * 4096));
    ENGR(R, r, svr_set_slice_dims(c, C.dims.data() + 3 * o, 1.0f));
    const uint32_t psz[3] = {128, 128, 128};
    ENGR(R, r, svr_generate_psf_volume(c, nullptr, psz, &C.dims[3 * o], vdim, pi2w, pw2i, 1.0f));
    R.set_matrices(r, C.st, C.sti, P.i2w, P.w2i, C.vol_i2w, C.vol_w2i);
    hosts[r] = pvrh_create_sharded(c, C.counts.data(), (int)C.counts.size(), S.vmin, S.vmax, R.rlo[r], R.rhi[r], R.group ? svr_group_join(R.group, r, c) : nullptr);
    if (!hosts[r]) die("pvrh_create_sharded failed" + std::string(R.group ? " (the rank group could not be joined)" : ""));
    if (R.nr > 1 && pvrh_set_unit_order(hosts[r], R.order.data())) die("pvrh_set_unit_order failed");
  });
  std::string per_rank = ", patches per rank";
  for (int r = 0; r < R.nr; ++r) per_rank += " " + std::to_string(R.rhi[r] - R.rlo[r]);
  R.describe(opt.devices, per_rank);
}

// PBR.cpp:452-489: runHybrid, the IRTK schedule on every patch; every rank registers its own patches against the shared volume
void register_patches(const Problem &S, LevelPatches &C, const Ranks &R) {
  const Patches &P = C.P;
  const int px = C.px, py = C.py;
  std::vector<float> vol((size_t)S.tattr.nx * S.tattr.ny * S.tattr.nz);
  ENGR(R, 0, svr_sync_cpu(R.ctxs[0], vol.data()));       // m_GPURecon.copyToHost (every rank holds the same volume)
  std::vector<long> evals(R.nr, 0);
  R.par([&](int r) {
    char e[256] = {0};
    const size_t o = (size_t)R.rlo[r];
    if (svrh_slice_to_volume_registration(R.ctxs[r], nullptr, R.rhi[r] - R.rlo[r], P.data.data() + o * px * py, px, py, P.attr.data() + o,
                                          C.Td.data() + 16 * o, &S.tattr, vol.data(), SVRH_S2V_NO_RESAMPLE, &evals[r], e))
      die(std::string("patch-to-volume registration: ") + e);
  });
  R.update_matrices(C.Td, C.st, C.sti, P.i2w, P.w2i, C.vol_i2w, C.vol_w2i);   // updateTransformationMatrices (patchBasedObject.cuh:151-169)
  long total = 0;
  for (long v : evals) total += v;
  fprintf(stderr, "patch-to-volume registration: %ld similarity evaluations\n", total);
}

// the loop (PBR.cpp:445-593)
void run_iterations(const Options &opt, const Problem &S, const Level &lv, LevelPatches &C, const Ranks &R, const std::vector<pvrh_recon *> &hosts,
                    StageClock &clk) {
  for (int it = 0; it < lv.iterations + 1; ++it) {
    const bool have_volume = it > 0 || !lv.existing.empty();                                   // PBR.cpp:456
    if (have_volume && !opt.no_registration && opt.superpixel) {
      // runHybrid registers the square CPU patches of generatePatchesCPU and updateTransformationMatrices then reads one
      // transformation per GPU patch from that shorter list: undefined in the reference for superpixel patches, not done
      fprintf(stderr, "superpixel mode: the patch-to-volume registration is skipped\n");
    } else if (have_volume && !opt.no_registration) {
      register_patches(S, C, R);
    }
    if (have_volume && !opt.no_registration) clk.mark("registration of the patches");
    R.par([&](int r) { PVRHR(r, pvrh_reconstruct_iteration(hosts[r], opt.sr_iterations)); });
    clk.mark("reconstruction iteration");
    double sc[8];
    pvrh_get_state(hosts[0], nullptr, nullptr, nullptr, sc);
    fprintf(stderr, "iteration %d: sigma %.4g mix %.3f\n", it, sc[0], sc[1]);
  }
}

// one level from the patch extraction on (the set-up gives the same result every time); false: --dryRun stopped it
bool run_level(const Options &opt, const Problem &S, const Level &lv, StageClock &clk, std::vector<float> &vol_out) {
  const svr_image_attr &tattr = S.tattr;
  LevelPatches C;
  cut_patches(opt, S, lv, C);
  clk.mark("patch generation");
  if (C.P.n == 0) die("no patch overlaps the mask");
  fprintf(stderr, "%zu stacks, %d patches of %dx%d, volume %dx%dx%d at %g mm\n", S.stacks.size(), C.P.n, C.px, C.py, tattr.nx, tattr.ny, tattr.nz, opt.resolution);
  if (!opt.dump_name.empty() && lv.dump) dump_problem(opt.dump_name, opt.superpixel, S, C);
  if (opt.dry_run) return false;

  Ranks R;
  std::vector<pvrh_recon *> hosts;
  shard_patches(opt, S, C, R);
  for (int r = 0; r < R.nr; ++r) R.create_context(r, opt.devices.empty() ? 0 : opt.devices[r]);
  R.create_group(opt.devices);
  setup_engines(opt, S, lv, C, R, hosts);
  clk.mark("engine set-up and upload");
  run_iterations(opt, S, lv, C, R, hosts, clk);
  vol_out.resize((size_t)tattr.nx * tattr.ny * tattr.nz);
  ENGR(R, 0, svr_sync_cpu(R.ctxs[0], vol_out.data()));
  if (clk.on) {
    int o[6] = {0, 0, 0, 0, 0, 0};
    const char *names[6] = {"tile_w", "tile_h", "wave_cap", "fwd_tile_w", "fwd_tile_h", "fwd_unit_cap"};
    for (int k = 0; k < 6; ++k) (void)svr_get_option(R.ctxs[0], names[k], &o[k]);
    fprintf(stderr, "[timing] tuned: scatter tiles %dx%d box %d, gather tiles %dx%d box %d\n", o[0], o[1], o[2], o[3], o[4], o[5]);
  }
  clk.mark("volume download");
  for (pvrh_recon *h : hosts) pvrh_destroy(h);
  R.destroy();
  return true;
}

// pvrmain:359-432: iterations + 1 levels of one registration-reconstruction iteration each; a level starts from the volume of
// the level before (its "reconimage1_<size>_<stride>.nii.gz") and cuts patches 4 pixels smaller (stride 2 smaller, not for superpixels)
bool run_hierarchical(const Options &opt, const Problem &S, StageClock &clk, std::vector<float> &vol) {
  Level lv{opt.psize, opt.pstride, opt.spx_size, 1, S.existing, true};
  std::vector<int> &ps = lv.psize, &pt = lv.pstride;
  for (int level = 0; level <= opt.iterations; ++level) {
    if (opt.superpixel ? lv.spx_size < 1 : (ps[0] < 1 || ps[1] < 1 || pt[0] < 1 || pt[1] < 1))
      die("hierarchical mode: the patch size reached zero at level " + std::to_string(level) + " (--patchSize - 4 * --iterations must stay positive)");
    fprintf(stderr, "hierarchical level %d: patch size %d stride %d\n", level, opt.superpixel ? lv.spx_size : ps[0], opt.superpixel ? opt.spx_extend : pt[0]);
    if (!run_level(opt, S, lv, clk, vol)) return false;
    lv.existing = vol;
    lv.dump = false;
    if (opt.superpixel) lv.spx_size -= 4;
    else { ps[0] -= 4; ps[1] -= 4; pt[0] -= 2; pt[1] -= 2; }
  }
  return true;
}

}  // namespace

int main(int argc, char **argv) {
  prog_name = "PVRreconstructionGPU";
  const Options opt = parse_options(argc, argv);
  StageClock clk;
  // the HIP runtime comes up on a second thread while the stacks are read: a first context (the stack-to-stack registration
  // makes one, the reconstruction another) then costs milliseconds instead of 75
  std::future<void> runtime_up = std::async(std::launch::async, [&] {
    svr_ctx *warm = nullptr;
    if (!opt.dry_run && svr_create(opt.devices.empty() ? 0 : opt.devices[0], &warm) == 0 && warm) svr_destroy(warm);
  });
  before_exit = [&] { if (runtime_up.valid()) runtime_up.wait(); };
  Problem S;
  read_inputs(opt, S);
  clk.mark("read stacks");
  split_stacks(opt, S);
  crop_to_mask(opt, S);
  clk.mark("mask, crop (resample)");
  S.iso_mask = transform_nn(S.mask, resample_attr(S.mask.a, opt.resolution), ident(), 0.0);      // :258-266
  clk.mark("isotropic mask");
  if (runtime_up.valid()) runtime_up.wait();
  if (!opt.no_registration && S.stacks.size() > 1) register_stacks(opt, S);
  clk.mark("registration of the stacks");
  if (!opt.no_matching) match_stack_intensities_pvr(S.stacks, S.ts, S.iso_mask);                 // :288-294
  clk.mark("match stack intensities");
  make_template(opt, S);
  clk.mark("template, reconstruction mask");
  if (opt.superpixel && opt.full_slices) die("--superpixel with --useFullSlices is not supported by this build");
  std::vector<float> vol;
  if (opt.hierarchical && !opt.full_slices) {            // (with --useFullSlices: pvrmain:282-285 "SVR ON", one level)
    if (!run_hierarchical(opt, S, clk, vol)) return 0;
  } else {
    if (!run_level(opt, S, Level{opt.psize, opt.pstride, opt.spx_size, opt.iterations, S.existing, true}, clk, vol)) return 0;
  }
  clk.mark("engine teardown");
  char err[256] = {0};
  if (svr_nifti_write(opt.output.c_str(), &S.tattr, vol.data(), err)) die(opt.output + ": " + err);
  clk.mark("write the volume");
  return 0;
}

