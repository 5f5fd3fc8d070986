// svr_cli.cpp -- `SVRreconstructionGPU`: the reference's command line (source/reconstructionGPU2/
// reconstruction.cc, "main.cc") over the MI355X engine, in C++ like the reference's own main().
//
//   SVRreconstructionGPU -o recon.nii.gz -i s1.nii.gz s2.nii.gz ... -m mask.nii.gz [--thickness t1 t2 ...]
//                        [--resolution 0.75] [--iterations 4] [--useGPUReg] ...
//
// Option names and defaults: main.cc:164-211.  Set-up (main.cc:386-815): read the stacks, crop them to the
// mask, CreateTemplate, SetMask, MatchStackIntensitiesWithMasking, CreateSlicesAndTransformations,
// MaskSlices, SyncGPU.  Loop (main.cc:816-1237): [slice-to-volume registration] -> smoothing schedule ->
// Gaussian reconstruction -> robust statistics -> SR iterations -> mask; finally RestoreSliceIntensities +
// ScaleVolume and the volume is written.  The pre-processing functions restate irtkReconstruction's
// (irtkReconstructionGPU.cc = "RG.cc"; the line ranges are on each function) and agree with the Python
// mirror fetalreconstruction_amd/preprocess.py, which the tests compare them with.
//
// Transformations (-t) are `id`, IRTK rigid `dof` files or 4x4 text matrices; like the reference they are the start of the
// stack-to-stack registration (StackRegistrations, before and after the other stacks are cropped, main.cc:661,711).
// Slice-to-volume registration is the reference's default IRTK schedule (csrc/irtk_reg.cpp, every similarity evaluation
// on the GPU) or, with --useGPUReg, the reference's GPU registration.  --no_registration (not a reference option) skips
// both.  --useNMI makes the IRTK schedule's slice-to-volume and package-to-volume registrations use normalised mutual
// information (csrc/svr_nmi.inc), as GuessParameterSliceToVolume(true) would; the reference parses it and never passes it
// on (main.cc:210), so this is a deviation; the GPU registration stays CC-only and refuses it.  --enableBiasCorrection (not a reference option either: the reference hard-wires its bias correction off) runs
// BiasGPU / NormaliseBiasGPU in every SR iteration with --sigma, --global_bias_correction and --low_intensity_cutoff as the
// reference's main() would pass them.  --packages runs PackageToVolume with the schedule of main.cc:832-864; --tfolder reads transformation<i>.dof per
// slice and --debug writes them next to the output.  --useAutoTemplate picks the template stack by the reference's matrix rank
// method (main.cc:565-591, stackMotionEstimator.cpp:67-164; there only in builds with CULA): every stack, cropped to the
// mask, gets the motion score of its first nz / 3 slices (svr_stack_motion, csrc/svr_motion.inc) and the smallest score replaces
// the stack found from `-t id`; --autoTemplateCentral (a deviation) scores the middle third instead, which is what the
// reference's comment describes.  --sliceReport <file> and --simulatedStacks <prefix> (deviations: the reference keeps SlicesInfo and
// SimulateStacks, RG.cc:4937-4975, 1205-1262, and its main() calls neither) say how the run went, after the volume has been written:
// one forward projection of the final volume, per slice the reference's twelve columns plus n_px, n, ncc, rmse, mae and mean_weight
// (svr_slice_quality, csrc/svr_quality.inc), and the simulated slices put back into the cropped stacks.  --referenceVolume <file> (a
// deviation: the reference reads the file, main.cc:253-258, lets iteration 0 register, :826, and outside its T1 experiment never hands
// the voxels to the registration) seeds the run with a volume in the template's world space on any grid: resampled onto the
// reconstruction grid on the device (svr_resample_to_reconstruction, csrc/svr_seed.inc), brought to the stacks' intensity scale, it is
// every rank's reconstructed volume when the loop starts, and iteration 0 registers against it like any later one.  --channelStacks /
// --labelStacks (deviations) and the reference's --manualMask (reconstruction.cc:1240-1250) carry a second image per stack -- another
// co-registered acquisition, a label map, a manual mask -- into the reconstructed space after the volume has been written, with the final
// slice transformations and the EM's weights (svr_channel_scatter, csrc/svr_channel.inc): cropped with their stack, cut into slices and
// packed like the primaries, scattered through the SR iteration's scatter, divided by the weights (channels) or voted label by label.
// --structural (a deviation: the reference leaves a slice out by its intensity residuals or --force_exclude only) lets every outer
// iteration end with the slices' mean windowed SSIM against their simulation (svr_slice_ssim, csrc/svr_ssim.inc) and treats a slice that
// falls out of its stack (svr_structural_decide) like a --force_exclude slice during the next one; it lives in svrh_reconstruct_iteration.
// Not built, refused loudly: patch/superpixel modes, the CPU reconstruction path.
#include <functional>
#include <set>
#include <thread>

#include <future>

#include "svr_prep.h"
#include "svr_shard.h"


int main(int argc, char **argv) {
  std::string output, mask_name, tfolder, sfolder;
  bool debug = false, dry_run = false, save_slice_transformations = false;
  std::string dump_name;
  std::vector<std::string> inputs, tspecs;
  std::vector<double> thickness;
  std::vector<int> force_excluded, devices, packages;
  int iterations = 4, levels = 3, rec_first = 4, rec_last = 13, num_stacks_tuner = 0;
  double resolution = 0.75, average = 700, delta = 150, lambda = 0.02, last_lambda = 0.01, smooth_mask = 4;
  bool no_matching = false, use_gpu_reg = false, no_registration = false, use_nmi = false;
  bool auto_template = false, auto_central = false;                      // --useAutoTemplate (main.cc:199), --autoTemplateCentral (not a reference option)
  double sigma = 12.0, low_intensity_cutoff = 0.01;                      // main.cc:172, 181
  bool enable_bias = false, global_bias = false;                         // --enableBiasCorrection (not a reference option), --global_bias_correction
  std::string reference_name;                                             // --referenceVolume (main.cc:207; takes effect here)
  std::string report_name, sim_prefix;                                   // --sliceReport, --simulatedStacks (not reference options)
  bool structural = false;                                                // --structural (not a reference option) and its four parameters
  int st_radius = 3, st_min_pixels = 25;
  double st_k = 3.0, st_min_drop = 0.1;
  std::vector<std::string> channel_names, label_names;                   // --channelStacks, --labelStacks (not reference options): a file or `none` per -i stack
  std::string channel_out, label_out, label_conf, manual_name, channels_dump;   // --channelOutput, --labelOutput, --labelConfidence, --manualMask, --dumpChannels
  bool have_channel_opt = false, have_label_opt = false;
  int coeff_table = -1;                                                   // -1: the engine's default (on since round 6), 1 / 0: --coeffTable / --noCoeffTable
  // ---- options (main.cc:164-211) ---------------------------------------------------------------------
  auto is_opt = [](const char *s) { return s[0] == '-' && !(s[1] >= '0' && s[1] <= '9') && s[1] != '.'; };
  for (int i = 1; i < argc; ++i) {
    const std::string o = argv[i];
    auto multi = [&](std::vector<std::string> &dst) { while (i + 1 < argc && !is_opt(argv[i + 1])) dst.push_back(argv[++i]); };
    auto one = [&]() -> std::string { if (i + 1 >= argc) die("missing value for " + o); return argv[++i]; };
    // po::value<bool> options of the reference take a value (--debug 1); a bare flag is accepted as `true`
    auto opt_bool = [&](bool bare) -> bool {
      if (i + 1 < argc) {
        const std::string v = argv[i + 1];
        if (v == "1" || v == "true" || v == "yes" || v == "on") { ++i; return true; }
        if (v == "0" || v == "false" || v == "no" || v == "off") { ++i; return false; }
      }
      return bare;
    };
    if (o == "-o" || o == "--output") output = one();
    else if (o == "-m" || o == "--mask") mask_name = one();
    else if (o == "-i" || o == "--input") multi(inputs);
    else if (o == "-t" || o == "--transformation") multi(tspecs);
    else if (o == "--thickness") { std::vector<std::string> v; multi(v); for (auto &s : v) thickness.push_back(atof(s.c_str())); }
    else if (o == "--iterations") iterations = atoi(one().c_str());
    else if (o == "--sigma") sigma = atof(one().c_str());              // bias field stdev (main.cc:172); used with --enableBiasCorrection
    else if (o == "--resolution") resolution = atof(one().c_str());
    else if (o == "--multires") levels = atoi(one().c_str());
    else if (o == "--average") average = atof(one().c_str());
    else if (o == "--delta") delta = atof(one().c_str());
    else if (o == "--lambda") lambda = atof(one().c_str());
    else if (o == "--lastIterLambda") last_lambda = atof(one().c_str());
    else if (o == "--smooth_mask") smooth_mask = atof(one().c_str());
    else if (o == "--no_intensity_matching") no_matching = !opt_bool(false);   // the value lands in `intensity_matching` (main.cc:186): 0 switches it off
    else if (o == "--num_stacks_tuner") num_stacks_tuner = atoi(one().c_str());
    else if (o == "--low_intensity_cutoff") low_intensity_cutoff = atof(one().c_str());   // passed to SuperresolutionGPU, which does not use it (as in the reference)
    else if (o == "--global_bias_correction") global_bias = opt_bool(true);
    else if (o == "--enableBiasCorrection") enable_bias = true;          // not a reference option: the reference hard-wires disableBiasCorr (main.cc:121,202)
    else if (o == "--log_prefix" || o == "--patchSize" || o == "--patchStride") (void)one();   // no log files; patch modes are off
    else if (o == "--no_log") (void)opt_bool(true);
    else if (o == "--force_exclude") { std::vector<std::string> v; multi(v); for (auto &s : v) force_excluded.push_back(atoi(s.c_str())); }
    else if (o == "--rec_iterations_first") rec_first = atoi(one().c_str());
    else if (o == "--rec_iterations_last") rec_last = atoi(one().c_str());
    else if (o == "--useGPUReg") use_gpu_reg = true;
    else if (o == "--useNMI") use_nmi = true;                             // main.cc:210 parses it and never calls setUseNMI(): here it takes effect
    else if (o == "--useAutoTemplate") auto_template = true;              // main.cc:199, 565-591 (there: HAVE_CULA builds only)
    else if (o == "--autoTemplateCentral") auto_template = auto_central = true;   // the middle third of the slices instead of the first
    else if (o == "-p" || o == "--packages") { std::vector<std::string> v; multi(v); for (auto &x : v) packages.push_back(atoi(x.c_str())); }
    else if (o == "--no_registration") no_registration = true;
    else if (o == "--tfolder") tfolder = one();
    else if (o == "--sfolder") sfolder = one();
    else if (o == "--coeffTable") coeff_table = 1;                        // not a reference option: keep the PSF taps in HBM (CoeffInit on the GPU path); the default since round 6
    else if (o == "--noCoeffTable") coeff_table = 0;                      // ... every tap evaluated in every pass, like the reference's GPU kernels: same volume, bit for bit
    else if (o == "--debug") debug = opt_bool(true);
    else if (o == "--saveSliceTransformations") save_slice_transformations = true;   // main.cc:211, 1213-1217
    else if (o == "--dumpProblem") dump_name = one();                     // test hooks: what the engine is about to receive [--dryRun: stop there]
    else if (o == "--dryRun") dry_run = true;
    else if (o == "--sliceReport") report_name = one();                   // not reference options: the reference's main() never calls SlicesInfo / SimulateStacks
    else if (o == "--simulatedStacks") sim_prefix = one();
    else if (o == "--structural") structural = true;                      // not reference options: the reference leaves slices out by intensity residuals only
    else if (o == "--structuralRadius") st_radius = atoi(one().c_str());
    else if (o == "--structuralK") st_k = atof(one().c_str());
    else if (o == "--structuralMinDrop") st_min_drop = atof(one().c_str());
    else if (o == "--structuralMinPixels") st_min_pixels = atoi(one().c_str());
    else if (o == "--referenceVolume") reference_name = one();            // main.cc:207, 253-258: read there and (outside the T1 experiment) never used
    else if (o == "--channelStacks") { have_channel_opt = true; multi(channel_names); }   // not reference options: a second image per stack through the run's motion and weights
    else if (o == "--channelOutput") channel_out = one();
    else if (o == "--labelStacks") { have_label_opt = true; multi(label_names); }
    else if (o == "--labelOutput") label_out = one();
    else if (o == "--labelConfidence") label_conf = one();
    else if (o == "--manualMask") manual_name = one();                    // main.cc:208; reconstruction.cc:1240-1250 transformManualMaskwithPSF
    else if (o == "--dumpChannels") channels_dump = one();                // test hook: the packed channel / label grids [--dryRun: stop there]
    else if (o == "--useCPUReg" || o == "--disableBiasCorrection" || o == "--debug_gpu") {}
    else if (o == "-d" || o == "--devices") { std::vector<std::string> v; multi(v); for (auto &s : v) devices.push_back(atoi(s.c_str())); }
    else if (o == "-h" || o == "--help") {
      printf("usage: SVRreconstructionGPU -o <volume> -i <stack_1> .. <stack_N> [-m <mask>] [-t id|<4x4.txt> ..] [--thickness th_1 ..]\n"
             "       [--iterations 4] [--resolution 0.75] [--multires 3] [--average 700] [--delta 150] [--lambda 0.02]\n"
             "       [--lastIterLambda 0.01] [--smooth_mask 4] [--no_intensity_matching] [--force_exclude i ..]\n"
             "       [--rec_iterations_first 4] [--rec_iterations_last 13] [--packages p_1 ..] [--useGPUReg] [--no_registration] [--tfolder dir] [--sfolder dir]\n"
             "       [--saveSliceTransformations] [--coeffTable | --noCoeffTable] [-d device_1 .. device_N]\n"
             "       [--enableBiasCorrection] [--sigma 12] [--global_bias_correction 0] [--low_intensity_cutoff 0.01] [--disableBiasCorrection] [--useNMI]\n"
             "       [--useAutoTemplate] [--autoTemplateCentral] [--sliceReport file] [--simulatedStacks prefix] [--referenceVolume file]\n"
             "       [--channelStacks f_1 .. f_N --channelOutput file] [--labelStacks f_1 .. f_N --labelOutput file [--labelConfidence file]]\n"
             "       [--manualMask file]\n"
             "       [--structural [--structuralRadius 3] [--structuralK 3] [--structuralMinDrop 0.1] [--structuralMinPixels 25]]\n"
             "  --structural            deviation from the reference, which leaves a slice out by its intensity residuals (or --force_exclude)\n"
             "                          only: after the last SR iteration of every outer iteration, the mean of a windowed structural\n"
             "                          similarity (SSIM; box window of (2 radius + 1)^2 pixels, radius 1 .. 7) between each slice and its\n"
             "                          simulation is taken over the pixels the M-step counts, where at least half the window holds data.  A\n"
             "                          slice with at least --structuralMinPixels such pixels whose mean lies further below its stack's median\n"
             "                          than max(K 1.4826 MAD, MinDrop) is treated like a --force_exclude slice during the NEXT outer iteration,\n"
             "                          and judged again at its end: registration still moves it, so a slice that registration repairs comes\n"
             "                          back.  Stacks with fewer than 4 judged slices exclude nothing.  One stderr line per outer iteration\n"
             "                          lists what was found.  With --sliceReport the report gets three more columns: ssim n_ssim structural\n"
             "                          (1 = left out during the last outer iteration).  Not with --sfolder.  Without the option nothing changes.\n"
             "  --channelStacks f_1 .. f_N --channelOutput <file>\n"
             "                          deviation from the reference, which has no such option: a second image per -i stack (another echo, a\n"
             "                          quantitative or probability map), on its stack's grid; `none` = the stack has none.  After the volume\n"
             "                          is written the files, cropped and cut into slices with their stacks, are scattered into the volume with\n"
             "                          the final slice transformations and the robust weights of the run and divided by the scattered weights:\n"
             "                          the robust PSF-weighted average of the channel, in its own units (no intensity matching, no bias field,\n"
             "                          no super-resolution iterations), 0 where no slice with a channel reaches.  Its own value never excludes\n"
             "                          a pixel: zero and negative values count.  The -o volume is the same with and without it.\n"
             "  --labelStacks f_1 .. f_N --labelOutput <file> [--labelConfidence <file>]\n"
             "                          deviation from the reference: a label map per -i stack (integers in 0..65535, at most 64 different\n"
             "                          ones; 0 competes like any other label; `none` = the stack has none).  Each label's indicator image is\n"
             "                          scattered like a channel; a voxel gets the label with the largest weighted share (ties: the smallest\n"
             "                          label) and --labelConfidence that share.  Both are float volumes on the reconstruction grid, 0 where\n"
             "                          no labelled slice reaches.\n"
             "  --manualMask <file>     the reference's option: a manual mask on the FIRST stack's grid is written PSF-transformed into the\n"
             "                          reconstructed space as PSFTransformed_<name> next to <file>.  The same as --channelStacks <file> none ..\n"
             "                          none.  Deviation from the reference in the weighting: the robust weights of the run instead of one\n"
             "                          plain Gaussian pass.\n"
             "                          None of the three with --sfolder (the slices then no longer come from the stacks).\n"
             "  --referenceVolume <file> deviation from the reference (the reference reads the file and, outside its T1 experiment, never uses\n"
             "                          its voxels): use the volume as the initial reconstruction.  It must be in the template stack's world\n"
             "                          space, roughly aligned, like every stack given with -t; its grid (voxel size, field of view, axis\n"
             "                          order, oblique axes) is free: it is resampled onto the reconstruction grid (values <= -1 are background),\n"
             "                          masked, and scaled to --average unless --no_intensity_matching 0.  The first iteration then registers\n"
             "                          the slices (and packages) against it instead of reconstructing from unregistered slices; the volume\n"
             "                          itself is overwritten by the first reconstruction.  Only the first volume of a 4D file is used.\n"
             "  --sliceReport <file>    deviation from the reference, which has SlicesInfo and never calls it: after the volume is written,\n"
             "                          project it into the slices once more and write one tab-separated row per slice, in slice order:\n"
             "                          SlicesInfo's stack_index included excluded outside weight scale Translation{X,Y,Z} Rotation{X,Y,Z},\n"
             "                          then n_px (pixels in the mask), n (pixels the M-step counts) and over those the correlation ncc, rmse,\n"
             "                          mae of the scaled slice against its simulation and the mean posterior weight (nan: too few pixels).\n"
             "                          Totals and the median ncc per stack go to stderr.  The volume is the same with and without it.\n"
             "  --simulatedStacks <pfx> deviation from the reference, which has SimulateStacks and never calls it: write <pfx><k>.nii.gz for\n"
             "                          every stack k in the geometry of the cropped stack: the simulated slice where the slice has a pixel\n"
             "                          and is included, 0 elsewhere.  Not with --sfolder.  Neither option with --dryRun.\n"
             "  --useAutoTemplate       select the 3D registration template stack automatically with the reference's matrix rank method:\n"
             "                          every stack is cropped to the mask and the first third of its slices is scored by the rank its\n"
             "                          singular values need for 99 %% of their norm; the smallest score becomes the template instead of the\n"
             "                          first stack whose -t is id.  All transformations stay as given, only the template's number changes\n"
             "                          (the chosen stack's -t need not be id; like the reference this build does not look at it).\n"
             "  --autoTemplateCentral   deviation from the reference, whose code scores the FIRST third of the slices although its comment\n"
             "                          says the central ones: score the middle third.  Implies --useAutoTemplate.\n"
             "  --useNMI                deviation from the reference, whose --useNMI is parsed and never takes effect: slice-to-volume and\n"
             "                          package-to-volume registration use normalised mutual information (64 bins, IRTK's histogram metric)\n"
             "                          instead of cross correlation -- for stacks whose contrast differs.  Not with --useGPUReg (CC only).\n"
             "  --enableBiasCorrection  deviation from the reference, whose bias correction cannot be switched on: run BiasGPU and\n"
             "                          NormaliseBiasGPU in every SR iteration (bias field stdev --sigma mm; sigma <= 0: no bias step).\n"
             "                          Without it bias correction is off, as in the reference; --disableBiasCorrection is accepted and changes nothing.\n");
      return 0;
    } else {
      die("option " + o + " is not supported by this build (see csrc/svr_cli.cpp)");
    }
  }
  if (output.empty() || inputs.empty()) die("-o and -i are required (try --help)");
  if (dry_run && (!report_name.empty() || !sim_prefix.empty()))
    die("--dryRun stops before the reconstruction; --sliceReport / --simulatedStacks describe a finished one: drop one or the other");
  if (!sim_prefix.empty() && !sfolder.empty())
    die("--simulatedStacks puts every simulated slice back into the stack it was cut from; with --sfolder the slices come from files of "
        "their own and belong to no stack: use --sliceReport, or drop --sfolder");
  if (structural && !sfolder.empty())
    die("--structural compares every slice with the other slices of its stack; with --sfolder the slices come from files of their own and "
        "belong to no stack: drop one or the other");
  if (structural && (st_radius < 1 || st_radius > SVR_SSIM_MAX_RADIUS))
    die("--structuralRadius must be 1 .. " + std::to_string(SVR_SSIM_MAX_RADIUS) + " (the window is (2 radius + 1)^2 pixels)");
  if (structural && (!(st_k >= 0.0) || !(st_min_drop >= 0.0) || st_min_pixels < 0))
    die("--structuralK, --structuralMinDrop and --structuralMinPixels must not be negative");
  if (dry_run && !reference_name.empty()) die("--dryRun makes no engine context and cannot resample a volume: drop --referenceVolume");
  if (use_nmi && use_gpu_reg)
    die("--useNMI selects normalised mutual information for the IRTK registration; the reference's GPU registration (--useGPUReg) is "
        "cross-correlation only: use one or the other");
  if (num_stacks_tuner > 0 && (size_t)num_stacks_tuner < inputs.size()) {      // main.cc:406-419: only the first stacks are used
    inputs.resize(num_stacks_tuner);
    if (tspecs.size() > (size_t)num_stacks_tuner) tspecs.resize(num_stacks_tuner);
    if (thickness.size() > (size_t)num_stacks_tuner) thickness.resize(num_stacks_tuner);
    if (packages.size() > (size_t)num_stacks_tuner) packages.resize(num_stacks_tuner);
  }
  const size_t n = inputs.size();
  // ---- second images per stack: what can be refused without reading a file -----------------------------
  struct ExtraSet {
    std::string what;                    // the option, for messages
    bool labels = false;
    std::vector<std::string> names;      // per stack; "none" = the stack has none
    std::string out, conf;
    std::vector<Image> imgs;             // per stack (empty image where none)
    std::vector<float> grid;             // [ns][my][mx], 0 outside a slice's extent
    std::vector<unsigned char> unit_on;  // [ns]
    std::vector<float> label_values;     // ascending
  };
  std::vector<ExtraSet> extras;
  {
    if (have_channel_opt && channel_out.empty()) die("--channelStacks needs --channelOutput <file> for the reconstructed channel");
    if (!have_channel_opt && !channel_out.empty()) die("--channelOutput needs --channelStacks f_1 .. f_N (a file or `none` per -i stack)");
    if (have_label_opt && label_out.empty()) die("--labelStacks needs --labelOutput <file> for the reconstructed labels");
    if (!have_label_opt && !label_out.empty()) die("--labelOutput needs --labelStacks f_1 .. f_N (a file or `none` per -i stack)");
    if (!have_label_opt && !label_conf.empty()) die("--labelConfidence needs --labelStacks f_1 .. f_N and --labelOutput");
    auto add = [&](const char *what, bool labels, const std::vector<std::string> &names, const std::string &out, const std::string &conf) {
      if (!sfolder.empty())
        die(std::string(what) + " cuts its files into slices with the stacks; with --sfolder the slices come from files of their own and belong to no "
            "stack: drop one or the other");
      if (names.size() != n)
        die(std::string(what) + ": " + std::to_string(names.size()) + " files for " + std::to_string(n) + " stacks: one file (or `none`) per -i stack expected");
      if (std::all_of(names.begin(), names.end(), [](const std::string &f) { return f == "none"; }))
        die(std::string(what) + ": every stack is `none`: nothing to reconstruct");
      ExtraSet e;
      e.what = what; e.labels = labels; e.names = names; e.out = out; e.conf = conf;
      extras.push_back(e);
    };
    if (have_channel_opt) add("--channelStacks", false, channel_names, channel_out, "");
    if (have_label_opt) add("--labelStacks", true, label_names, label_out, label_conf);
    if (!manual_name.empty()) {
      std::vector<std::string> names(n, "none");
      names[0] = manual_name;
      const size_t cut = manual_name.find_last_of('/');                  // reconstruction.cc:1243-1249: "PSFTransformed_" + the file's name, in its directory
      const std::string out = cut == std::string::npos ? "PSFTransformed_" + manual_name
                                                       : manual_name.substr(0, cut + 1) + "PSFTransformed_" + manual_name.substr(cut + 1);
      add("--manualMask", false, names, out, "");
    }
    if (!channels_dump.empty() && extras.empty()) die("--dumpChannels writes the packed grids of --channelStacks / --labelStacks / --manualMask: give one of them");
  }
  if (tspecs.empty()) tspecs.assign(n, "id");
  if (tspecs.size() != n) die("one transformation per stack expected");
  if (!packages.empty() && packages.size() != n) die("one package count per stack expected");

  size_t tmpl = n;
  for (size_t k = 0; k < n; ++k) if (tspecs[k] == "id") { tmpl = k; break; }
  if (tmpl == n) die("Please identify the template by assigning id transformation.");          // main.cc:452-457

  StageClock clk;
  // the HIP runtime and the context come up (75 ms) while the stacks are read and cropped; first use: the stack registrations
  svr_ctx *ctx = nullptr;
  std::future<int> ctx_ready = std::async(std::launch::async, [&] { return dry_run ? 1 : svr_create(devices.empty() ? 0 : devices[0], &ctx); });
  before_exit = [&] { if (ctx_ready.valid()) ctx_ready.wait(); };     // an error while reading must not exit under the runtime's feet
  auto need_ctx = [&] {
    if (ctx_ready.valid() && (ctx_ready.get() || !ctx)) die("no usable HIP device (svr_create failed)");
  };

  // ---- set-up (main.cc:386-815) ----------------------------------------------------------------------
  std::vector<Image> stacks;
  std::vector<M4> ts;
  stacks.resize(n);
  parallel_for((int)n, [&](int k) { stacks[k] = read_image(inputs[k]); });                        // gunzip is serial per file
  for (size_t k = 0; k < n; ++k) ts.push_back(load_transformation(tspecs[k]));
  for (auto &e : extras) {
    e.imgs.resize(n);
    for (size_t k = 0; k < n; ++k) {
      if (e.names[k] == "none") continue;
      e.imgs[k] = read_image(e.names[k]);
      // on its stack's grid as read: the same dimensions, the same image-to-world matrix
      const svr_image_attr &a = e.imgs[k].a, &b = stacks[k].a;
      bool same = a.nx == b.nx && a.ny == b.ny && a.nz == b.nz;
      if (same) {
        const M4 ma = image_to_world(a), mb = image_to_world(b);
        for (int q = 0; q < 16; ++q) same = same && fabs(ma.m[q] - mb.m[q]) <= 1e-3;
      }
      if (!same)
        die(e.what + ": " + e.names[k] + " is not on the grid of its stack " + inputs[k] + " (" + std::to_string(a.nx) + "x" + std::to_string(a.ny) + "x" +
            std::to_string(a.nz) + " against " + std::to_string(b.nx) + "x" + std::to_string(b.ny) + "x" + std::to_string(b.nz) +
            ", or another image-to-world matrix): resample it onto the stack first");
    }
  }
  clk.mark("read stacks");
  if (thickness.empty()) for (auto &s : stacks) thickness.push_back(2.0 * s.a.dz);            // main.cc:422-431
  if (thickness.size() != n) die("one thickness per stack expected");
  Image mask_img;
  const bool have_mask = !mask_name.empty() || sfolder.empty();          // main.cc:461: no mask is made up when --sfolder is given
  if (!mask_name.empty()) {
    mask_img = read_image(mask_name);
  } else if (have_mask) {
    // no mask given: CreateMask(stacks[templateNumber]) binarises the template stack (> 0), in case it was padded; the
    // normal mask path follows (main.cc:458-480, RG.cc:736-748)
    mask_img = stacks[tmpl];
    for (auto &v : mask_img.d) v = v > 0.0 ? 1.0 : 0.0;
  }
  if (auto_template) {                                                                           // main.cc:565-591
    if (!have_mask) die("--useAutoTemplate crops every stack to the mask before it scores it: give -m (the reference skips the selection without a mask)");
    if (dry_run) die("--dryRun makes no engine context and cannot score the stacks' motion: drop --useAutoTemplate / --autoTemplateCentral");
    need_ctx();
    double best = 1e300;                                                                         // tmp_motionestimate, main.cc:271
    size_t best_k = tmpl;
    for (size_t k = 0; k < n; ++k) {
      // on a copy: TransformMask + CropImage with the -t transformations as given (the stack registrations come later)
      const Image c = crop_image(stacks[k], transform_nn(mask_img, stacks[k].a, ts[k], 0.0));
      const int m = c.a.nx * c.a.ny, nw = (int)(c.a.nz / 3.0), first = auto_central ? (c.a.nz - nw) / 2 : 0;
      if (nw < 1) die("--useAutoTemplate: stack " + std::to_string(k) + " has " + std::to_string(c.a.nz) + " slices inside the mask; a third of them is none");
      const auto mm = std::minmax_element(c.d.begin(), c.d.end());                               // the whole cropped stack's, not the window's
      const double lo = *mm.first, hi = *mm.second;
      if (!(hi > lo)) die("--useAutoTemplate: stack " + std::to_string(k) + " is constant inside the mask");
      std::vector<float> win((size_t)m * nw);
      for (size_t i = 0; i < win.size(); ++i) win[i] = (float)((c.d[(size_t)first * m + i] - lo) / (hi - lo));
      double et = 0, score = 0;
      int r_min = 0;
      if (svr_stack_motion(ctx, win.data(), m, nw, nullptr, &et, &r_min, &score))
        die("--useAutoTemplate: stack " + std::to_string(k) + ": " + svr_last_error(ctx));
      fprintf(stderr, "stack %zu: motion score %.9g (r_min %d, et %.9g)\n", k, score, r_min, et);
      if (score < best) { best = score; best_k = k; }                                            // strictly smaller: the first one on ties
    }
    tmpl = best_k;
    fprintf(stderr, "Determined stack %zu as template.\n", tmpl);
    clk.mark("motion measurement");
  }
  if (have_mask) {
    const Image m = transform_nn(mask_img, stacks[tmpl].a, ts[tmpl], 0.0);                     // TransformMask RG.cc:805-821
    stacks[tmpl] = crop_image(stacks[tmpl], m);
    for (auto &e : extras) if (!e.imgs[tmpl].d.empty()) e.imgs[tmpl] = crop_image(e.imgs[tmpl], m);   // (the crop depends on the mask alone)
  }
  const svr_image_attr tattr = create_template(stacks[tmpl].a, resolution);
  const Image vol_mask = set_mask(tattr, have_mask ? &mask_img : nullptr, smooth_mask);
  clk.mark("mask, crop, template");
  auto stack_registrations = [&]() {                                                             // StackRegistrations, RG.cc:849-1001
    if (no_registration || n < 2 || !sfolder.empty()) return;                                    // main.cc:658, 708
    if (dry_run) die("--dryRun makes no engine context and cannot register the stacks: add --no_registration (or --sfolder)");
    need_ctx();
    std::vector<svr_image_attr> at(n);
    std::vector<const double *> ptr(n);
    std::vector<double> tm(16 * n);
    for (size_t k = 0; k < n; ++k) { at[k] = stacks[k].a; ptr[k] = stacks[k].d.data(); for (int q = 0; q < 16; ++q) tm[16 * k + q] = ts[k].m[q]; }
    long evals = 0;
    char e[256] = {0};
    if (svrh_stack_registrations(ctx, nullptr, (int)n, at.data(), ptr.data(), tm.data(), (int)tmpl, have_mask ? &vol_mask.a : nullptr,
                                 have_mask ? vol_mask.d.data() : nullptr, 0, &evals, e))
      die(std::string("stack registration: ") + e);
    for (size_t k = 0; k < n; ++k) for (int q = 0; q < 16; ++q) ts[k].m[q] = tm[16 * k + q];
    fprintf(stderr, "stack-to-stack registration: %ld similarity evaluations\n", evals);
  };
  stack_registrations();                                                                         // main.cc:657-662
  for (size_t k = 0; k < n; ++k) {                                                               // main.cc:676-700
    if (k == tmpl) continue;
    const Image m = transform_nn(vol_mask, stacks[k].a, ts[k], 0.0);
    stacks[k] = crop_image(stacks[k], m);
    for (auto &e : extras) if (!e.imgs[k].d.empty()) e.imgs[k] = crop_image(e.imgs[k], m);
  }
  stack_registrations();                                                                         // main.cc:707-713
  clk.mark("stack registrations, crops");
  const std::vector<float> factors = match_stack_intensities(stacks, ts, vol_mask, average, no_matching);
  clk.mark("match stack intensities");
  // CreateSlicesAndTransformations RG.cc:1835-1880 + MaskSlices RG.cc:1940-1988 + the packing of SyncGPU RG.cc:249-328
  struct SliceSrc { Image r; M4 t; int stack; };
  std::vector<SliceSrc> srcs;
  for (size_t k = 0; k < n; ++k)
    for (int j = 0; j < stacks[k].a.nz; ++j) {
      SliceSrc q{get_region(stacks[k], 0, 0, j, stacks[k].a.nx, stacks[k].a.ny, j + 1), ts[k], (int)k};
      q.r.a.dz = thickness[k];
      srcs.push_back(q);
    }
  if (!sfolder.empty()) {
    // replaceSlices, RG.cc:4767-4822: every file of the folder is one slice that is already in place -- identity
    // transformation, stack 0, 4 mm thickness, "equally many as loaded from stacks".  The reference takes the files in
    // directory_iterator order (unspecified); here they are taken in the order of their names.
    std::vector<std::string> files = list_directory(sfolder);
    if (files.size() != srcs.size())
      die("--sfolder: " + std::to_string(files.size()) + " files, but the stacks hold " + std::to_string(srcs.size()) + " slices");
    for (size_t i = 0; i < files.size(); ++i) {
      SliceSrc q{read_image(sfolder + "/" + files[i]), ident(), 0};
      if (q.r.a.nz != 1) die("--sfolder: " + files[i] + " is not a single slice");
      q.r.a.dz = 4.0;
      srcs[i] = q;
    }
  }
  int ns = (int)srcs.size(), mx = 0, my = 0;
  for (auto &q : srcs) { mx = std::max(mx, q.r.a.nx); my = std::max(my, q.r.a.ny); }
  std::vector<float> grid((size_t)ns * mx * my, -1.0f), i2w(16 * (size_t)ns), w2i(16 * (size_t)ns), st(16 * (size_t)ns),
      sti(16 * (size_t)ns), dims(3 * (size_t)ns);
  std::vector<int> sizes_x(ns), sizes_y(ns), stack_index(ns);
  std::vector<svr_image_attr> sattr(ns);
  std::vector<double> T(16 * (size_t)ns);
  const M4 mw2i = world_to_image(vol_mask.a);
  double vmin = 1e300, vmax = -1e300;
  for (int sl = 0; sl < ns; ++sl) {
      const Image &r = srcs[sl].r;
      const M4 &tk = srcs[sl].t;
      const M4 si2w = image_to_world(r.a);
      for (int y = 0; y < r.a.ny; ++y)
        for (int x = 0; x < r.a.nx; ++x) {
          double v = r.at(x, y, 0);
          if (v < 0.01) v = -1;
          double qx = x, qy = y, qz = 0;                   // ImageToWorld, Transform, WorldToImage: three applications (RG.cc:1961-1972)
          apply_point(si2w, qx, qy, qz); apply_point(tk, qx, qy, qz); apply_point(mw2i, qx, qy, qz);
          const long i = (long)irtk_round(qx), jj = (long)irtk_round(qy), kk = (long)irtk_round(qz);
          if (!(i >= 0 && i < vol_mask.a.nx && jj >= 0 && jj < vol_mask.a.ny && kk >= 0 && kk < vol_mask.a.nz) ||
              vol_mask.at((int)i, (int)jj, (int)kk) == 0)
            v = -1;
          grid[((size_t)sl * my + y) * mx + x] = (float)v;
          if (v > 0) { vmin = std::min(vmin, (double)(float)v); vmax = std::max(vmax, (double)(float)v); }
        }
      to_f16(si2w, &i2w[16 * (size_t)sl]); to_f16(world_to_image(r.a), &w2i[16 * (size_t)sl]);
      to_f16(tk, &st[16 * (size_t)sl]); to_f16(inverse_rigid_or_affine(tk), &sti[16 * (size_t)sl]);
      for (int q = 0; q < 16; ++q) T[16 * (size_t)sl + q] = tk.m[q];
      dims[3 * (size_t)sl] = (float)r.a.dx; dims[3 * (size_t)sl + 1] = (float)r.a.dy; dims[3 * (size_t)sl + 2] = (float)r.a.dz;
      sizes_x[sl] = r.a.nx; sizes_y[sl] = r.a.ny; stack_index[sl] = srcs[sl].stack; sattr[sl] = r.a;
  }
  // the second images, cut and packed like the primaries: slice sl = plane j of stack k, in the same order.  Their values are kept as they
  // are: no `v < 0.01 -> -1`, no mask, no stack factor -- which pixels count is the primary's business (svr_channel_scatter's pixel set)
  for (auto &e : extras) {
    e.grid.assign((size_t)ns * mx * my, 0.0f);
    e.unit_on.assign(ns, 0);
    int sl = 0;
    for (size_t k = 0; k < n; ++k)
      for (int j = 0; j < stacks[k].a.nz; ++j, ++sl) {
        const Image &c = e.imgs[k];
        if (c.d.empty()) continue;
        if (c.a.nx != stacks[k].a.nx || c.a.ny != stacks[k].a.ny || c.a.nz != stacks[k].a.nz) die(e.what + ": " + e.names[k] + " was not cropped like its stack");
        e.unit_on[sl] = 1;
        for (int y = 0; y < c.a.ny; ++y)
          for (int x = 0; x < c.a.nx; ++x) e.grid[((size_t)sl * my + y) * mx + x] = (float)c.at(x, y, j);
      }
    if (e.labels) {
      // the labels: the distinct values over the pixels that can count (the primary pixel is not -1, the stack has a label map)
      std::set<float> seen;
      for (int s = 0; s < ns; ++s) {
        if (!e.unit_on[s]) continue;
        for (size_t i = 0; i < (size_t)mx * my; ++i) {
          const size_t g = (size_t)s * mx * my + i;
          if (grid[g] == -1.0f) continue;
          const float v = e.grid[g];
          if (!(v >= 0.0f && v <= 65535.0f) || v != floorf(v))
            die(e.what + ": " + e.names[srcs[s].stack] + " holds the value " + std::to_string(v) + ": labels are integers in 0..65535");
          if (seen.insert(v).second && seen.size() > 64) die(e.what + ": more than 64 different labels");
        }
      }
      e.label_values.assign(seen.begin(), seen.end());                   // ascending: ties go to the smallest label
      if (e.label_values.empty()) die(e.what + ": no labelled pixel lies inside the mask");
    }
  }
  if (!channels_dump.empty()) {
    // test hook (tests/test_channel.py): {sets, ns, mx, my}, then per set {labels, number of labels}, unit_on [ns], the packed grid, the labels
    FILE *f = fopen(channels_dump.c_str(), "wb");
    if (!f) die("cannot write " + channels_dump);
    const int hdr[4] = {(int)extras.size(), ns, mx, my};
    fwrite(hdr, sizeof(int), 4, f);
    for (auto &e : extras) {
      const int h2[2] = {e.labels ? 1 : 0, (int)e.label_values.size()};
      fwrite(h2, sizeof(int), 2, f);
      fwrite(e.unit_on.data(), 1, e.unit_on.size(), f);
      fwrite(e.grid.data(), sizeof(float), e.grid.size(), f);
      fwrite(e.label_values.data(), sizeof(float), e.label_values.size(), f);
    }
    fclose(f);
  }
  if (!dump_name.empty()) {
    // what the engine is about to receive, for the CPU tests (tests/test_prep_oracle.py compares it with the oracle's restatement
    // of CreateTemplate / SetMask / TransformMask / CropImage / MatchStackIntensities / MaskSlices): header, the template's
    // attributes, the volume mask, the cropped stacks' attributes, the slice grid, the slices' transformations, the factors
    FILE *f = fopen(dump_name.c_str(), "wb");
    if (!f) die("cannot write " + dump_name);
    const int hdr[8] = {ns, mx, my, (int)n, tattr.nx, tattr.ny, tattr.nz, 2};
    fwrite(hdr, sizeof(int), 8, f);
    fwrite(&tattr, sizeof(svr_image_attr), 1, f);
    fwrite(vol_mask.d.data(), sizeof(double), vol_mask.d.size(), f);
    for (size_t k = 0; k < n; ++k) fwrite(&stacks[k].a, sizeof(svr_image_attr), 1, f);
    fwrite(grid.data(), sizeof(float), grid.size(), f);
    fwrite(T.data(), sizeof(double), T.size(), f);
    fwrite(factors.data(), sizeof(float), factors.size(), f);
    fwrite(sizes_x.data(), sizeof(int), sizes_x.size(), f);
    fwrite(sizes_y.data(), sizeof(int), sizes_y.size(), f);
    fclose(f);
  }
  if (dry_run) { fflush(nullptr); _exit(0); }             // (no context was made; skip the teardown of a runtime that never came up)
  if (!(vmax > 0)) die("no slice pixel lies inside the mask");
  fprintf(stderr, "%zu stacks, %d slices of up to %dx%d, volume %dx%dx%d at %g mm, stack factors", n, ns, mx, my, tattr.nx, tattr.ny, tattr.nz,
          resolution);
  for (float f : factors) fprintf(stderr, " %.9g", f);
  fprintf(stderr, "\n");

  // ---- ranks: one engine context per device of -d (main.cc:191).  Rank r takes the r-th of nr work-balanced segments of EVERY stack
  // (svr_shard.h spatial_order: a rank's slices are neighbours in space), work = estimated PSF work = active pixels x (9.4 + live
  // planes of the 16) x (1 + 0.2 n_x^2), see sharding.py slice_cost_weights.  (reconstruction_cuda2.cu:1413-1457 shards by slice count
  // in slice order and drops the remainder.)  From here on every per-slice array is in the SHARDED numbering -- rank after rank --
  // and `order[k]` is slice k's index in the reference's order: files named by slice number (--tfolder, --debug), --force_exclude
  // and the package registration, which works on whole stacks, go through it. -----------------------------------------------
  const int nr = (int)std::max<size_t>(1, devices.size());
  std::vector<int> rlo(nr, 0), rhi(nr, ns), order(ns), inv_order(ns);
  for (int s = 0; s < ns; ++s) order[s] = inv_order[s] = s;
  if (nr > 1) {
    if (ns < nr) die("fewer slices than devices");
    std::vector<double> work(ns, 0.0);
    const M4 rw = world_to_image(tattr);
    for (int s = 0; s < ns; ++s) {
      long c = 0;
      for (size_t i = 0; i < (size_t)mx * my; ++i) c += grid[(size_t)s * mx * my + i] != -1.0f;
      // slice normal in volume axes: reconW2I * T * sliceI2W applied to the slice's z direction
      double nw[3], nt[3], nv[3], len = 0;
      for (int k = 0; k < 3; ++k) nw[k] = i2w[16 * (size_t)s + 4 * k + 2];
      for (int k = 0; k < 3; ++k) nt[k] = T[16 * (size_t)s + 4 * k] * nw[0] + T[16 * (size_t)s + 4 * k + 1] * nw[1] + T[16 * (size_t)s + 4 * k + 2] * nw[2];
      for (int k = 0; k < 3; ++k) { nv[k] = rw.m[4 * k] * nt[0] + rw.m[4 * k + 1] * nt[1] + rw.m[4 * k + 2] * nt[2]; len += nv[k] * nv[k]; }
      len = std::max(sqrt(len), 1e-12);
      const double ax = fabs(nv[0]) / len, ay = fabs(nv[1]) / len, az = fabs(nv[2]) / len;
      const double ne = std::max(ay, az), no = std::min(ay, az), sigma = dims[3 * (size_t)s + 2] / 2.3548 / tattr.dx;
      const double live = std::min(16.0, 2.0 * (5.1 * sigma + 8.0 * (ax + no)) / std::max(ne, 1e-3) + 1.0);
      work[s] = (double)c * (9.4 + live) * (1.0 + 0.2 * ax * ax);
    }
    svr::spatial_order(work, stack_index, nr, order, rlo, rhi);
    for (int r = 0; r < nr; ++r) if (rhi[r] <= rlo[r]) die("a device would get no slice: fewer devices, please");
    for (int k = 0; k < ns; ++k) inv_order[order[k]] = k;
    svr::permute_rows(grid, (size_t)mx * my, order);
    svr::permute_rows(i2w, 16, order); svr::permute_rows(w2i, 16, order); svr::permute_rows(st, 16, order); svr::permute_rows(sti, 16, order);
    svr::permute_rows(dims, 3, order); svr::permute_rows(sizes_x, 1, order); svr::permute_rows(sizes_y, 1, order);
    svr::permute_rows(stack_index, 1, order); svr::permute_rows(sattr, 1, order); svr::permute_rows(T, 16, order);
    for (auto &e : extras) { svr::permute_rows(e.grid, (size_t)mx * my, order); svr::permute_rows(e.unit_on, 1, order); }
    for (int &s : force_excluded) if (s >= 0 && s < ns) s = inv_order[s];
  }
  need_ctx();
  std::vector<svr_ctx *> ctxs(nr, nullptr);
  std::vector<svrh_recon *> hosts(nr, nullptr);
  ctxs[0] = ctx;
  for (int r = 1; r < nr; ++r)
    if (svr_create(devices[r], &ctxs[r]) || !ctxs[r]) die("no usable HIP device " + std::to_string(devices[r]) + " (svr_create failed)");
  svr_group *group = nr > 1 ? svr_group_create(nr, devices.data()) : nullptr;
  if (nr > 1 && !group) die("cannot set up the rank group (librccl not found?)");
  // every rank in its own thread (the collectives inside block until all ranks have arrived)
  auto par = [&](const std::function<void(int)> &fn) {
    if (nr == 1) { fn(0); return; }
    std::vector<std::thread> th;
    for (int r = 0; r < nr; ++r) th.emplace_back(fn, r);
    for (auto &t : th) t.join();
  };
#define ENGR(r, call) do { int rc_ = (call); if (rc_) die(std::string(#call) + ": " + svr_last_error(ctxs[r])); } while (0)
#define HOSTR(r, call) do { int rc_ = (call); if (rc_) die(std::string(#call) + ": " + svrh_last_error(hosts[r])); } while (0)
  float ri2w[16], rw2i[16];
  to_f16(image_to_world(tattr), ri2w); to_f16(world_to_image(tattr), rw2i);
  auto set_matrices = [&](int r) {
    const size_t o = 16 * (size_t)rlo[r];
    ENGR(r, svr_set_slice_matrices(ctxs[r], st.data() + o, sti.data() + o, i2w.data() + o, w2i.data() + o, i2w.data() + o, w2i.data() + o, ri2w, rw2i));
  };

  // ---- SyncGPU + generatePSFVolume + UpdateGPUTranformationMatrices (RG.cc:249-401, 1496-1610), per rank ----------
  const uint32_t vsize[3] = {(uint32_t)tattr.nx, (uint32_t)tattr.ny, (uint32_t)tattr.nz};
  const float vdim[3] = {(float)tattr.dx, (float)tattr.dy, (float)tattr.dz};
  std::vector<float> maskf(vol_mask.d.begin(), vol_mask.d.end());
  float pi2w[16], pw2i[16];
  {
    svr_image_attr pa;                                                   // PSF_SIZE 128 (RC.cuh:56), RG.cc:1534-1551
    memset(&pa, 0, sizeof(pa));
    pa.nx = pa.ny = pa.nz = 128; pa.dx = tattr.dx; pa.dy = tattr.dy; pa.dz = tattr.dz;
    pa.xaxis[0] = pa.yaxis[1] = pa.zaxis[2] = 1.0;
    to_f16(image_to_world(pa), pi2w); to_f16(world_to_image(pa), pw2i);
  }
  par([&](int r) {
    const int nl = rhi[r] - rlo[r];
    const size_t o = (size_t)rlo[r];
    if (coeff_table >= 0) ENGR(r, svr_set_option(ctxs[r], "coeff_table", coeff_table));
    ENGR(r, svr_init_reconstruction_volume(ctxs[r], vsize, vdim, nullptr, 12.0f));
    ENGR(r, svr_set_mask(ctxs[r], vsize, vdim, maskf.data(), 12.0f));
    const uint32_t ssize[3] = {(uint32_t)mx, (uint32_t)my, (uint32_t)nl};
    ENGR(r, svr_init_storage_volumes(ctxs[r], ssize, &dims[3 * o]));
    ENGR(r, svr_fill_slices(ctxs[r], grid.data() + o * mx * my, sizes_x.data() + o, sizes_y.data() + o));
    ENGR(r, svr_set_slice_dims(ctxs[r], dims.data() + 3 * o, 2.0f));
    const uint32_t psize[3] = {128, 128, 128};
    ENGR(r, svr_generate_psf_volume(ctxs[r], nullptr, psize, &dims[3 * o], vdim, pi2w, pw2i, 2.0f));
    set_matrices(r);
    hosts[r] = svrh_create(ctxs[r], ns, rlo[r], rhi[r], group ? svr_group_join(group, r, ctxs[r]) : nullptr);
    if (!hosts[r]) die("svrh_create failed");
    svrh_set_intensity_range(hosts[r], vmin, vmax);                      // InitializeEMGPU RG.cc:2937-2951
    svrh_set_intensity_matching(hosts[r], no_matching ? 0 : 1);         // main.cc:1018, 1062
    // SetSigma / GlobalBiasCorrectionOn / SetLowIntensityCutoff (main.cc:451, 764-778); the steps themselves are gated on the option
    // sigma > 0 (main.cc:1025,1035,1069), so sigma <= 0 leaves the member at 20 and runs no bias step
    HOSTR(r, svrh_set_bias_correction(hosts[r], enable_bias && sigma > 0, sigma > 0 ? sigma : 20.0));
    HOSTR(r, svrh_set_bias_options(hosts[r], global_bias ? 1 : 0, low_intensity_cutoff));
    if (nr > 1 && svrh_set_unit_order(hosts[r], order.data())) die("svrh_set_unit_order failed");
    if (!force_excluded.empty()) svrh_set_force_excluded(hosts[r], force_excluded.data(), (int)force_excluded.size());
    if (structural) HOSTR(r, svrh_set_structural(hosts[r], 1, st_radius, st_k, st_min_drop, st_min_pixels, stack_index.data()));
    if (use_gpu_reg) HOSTR(r, svrh_prepare_registration_slices(hosts[r], grid.data() + o * mx * my, mx, my, sattr.data() + o, resolution));
  });
  if (nr > 1)
    fprintf(stderr, "%d ranks on devices%s, collectives: %s\n", nr, [&] { std::string t; for (int d : devices) t += " " + std::to_string(d); return t; }().c_str(),
            svr_group_uses_rccl(group) ? "RCCL" : "host memory (a device is named more than once: test mode)");
  svrh_recon *host = hosts[0];
  auto update_matrices_from_T = [&]() {                                  // UpdateGPUTranformationMatrices RG.cc:372-401
    for (int s = 0; s < ns; ++s) {
      M4 t;
      for (int q = 0; q < 16; ++q) t.m[q] = T[16 * (size_t)s + q];
      to_f16(t, &st[16 * (size_t)s]); to_f16(inverse_rigid_or_affine(t), &sti[16 * (size_t)s]);
    }
    for (int r = 0; r < nr; ++r) set_matrices(r);
  };

  if (!tfolder.empty()) {                                                // ReadTransformation, RG.cc:4733-4765
    for (int s = 0; s < ns; ++s) {
      double p6[6];
      char e[256] = {0};
      const std::string path = tfolder + "/transformation" + std::to_string(order[s]) + ".dof";       // (files are named in the reference's slice order)
      if (svr_dof_read(path.c_str(), p6, &T[16 * (size_t)s], e)) die(path + ": " + e);
    }
    update_matrices_from_T();
  }

  clk.mark("slices, engine set-up, upload");
  const bool have_reference = !reference_name.empty();
  if (have_reference) {
    // The seed on its own grid -> the reconstruction grid, on rank 0's device: once to learn its mean inside the mask, once more to
    // scale and install it; the other ranks get the result.  -1 is this program's own background (MaskVolume) and must not bleed in.
    svr_image_attr ra;
    float *rdata = nullptr;
    int rnt = 1;
    char e[256] = {0};
    if (svr_nifti_read(reference_name.c_str(), &ra, &rnt, &rdata, e)) die(reference_name + ": " + e);   // (4D: the first volume comes first)
    const M4 m = mul(world_to_image(ra), image_to_world(tattr));
    const uint32_t rsize[3] = {(uint32_t)ra.nx, (uint32_t)ra.ny, (uint32_t)ra.nz};
    double rs[5];
    ENGR(0, svr_resample_to_reconstruction(ctx, rsize, rdata, m.m, -1.0f, 0, 1.0f, nullptr, rs));
    if (rs[0] == 0) die("--referenceVolume does not overlap the mask");
    const double rmean = rs[1] / rs[0];
    // the stacks were matched to --average, and the default registration casts the volume to short: a seed in [0, 1] would have two levels
    double rscale = 1.0;
    if (!no_matching) {
      if (!(rmean > 0)) die("--referenceVolume: the mean inside the mask is " + std::to_string(rmean) + ", it cannot be scaled to --average");
      rscale = average / rmean;
    }
    std::vector<float> seed(nr > 1 ? (size_t)tattr.nx * tattr.ny * tattr.nz : 0);
    ENGR(0, svr_resample_to_reconstruction(ctx, rsize, rdata, m.m, -1.0f, SVR_RESAMPLE_INSTALL | (no_matching ? 0 : SVR_RESAMPLE_SCALE), (float)rscale,
                                           nr > 1 ? seed.data() : nullptr, rs));
    svr_free(rdata);
    for (int r = 1; r < nr; ++r) ENGR(r, svr_update_reconstructed(ctxs[r], vsize, seed.data()));
    fprintf(stderr, "reference volume: n=%.0f mean=%.9g min=%.9g max=%.9g scale=%.9g\n", rs[0], rmean, rs[3], rs[4], rscale);
    clk.mark("reference volume");
  }
  // ---- registration-reconstruction loop (main.cc:816-1237) ---------------------------------------------
  for (int it = 0; it < iterations; ++it) {
    bool slice_reg = (it > 0 || have_reference) && !no_registration;      // main.cc:826
    if (slice_reg && !packages.empty() && it <= iterations * (levels - 1) / levels && it < iterations - 1) {
      // packages first (main.cc:832-864): plain, even/odd, even/odd halves; from iteration 4 on also the slices
      std::vector<svr_image_attr> at(n);
      std::vector<const double *> ptr(n);
      for (size_t k = 0; k < n; ++k) { at[k] = stacks[k].a; ptr[k] = stacks[k].d.data(); }
      std::vector<float> vol((size_t)tattr.nx * tattr.ny * tattr.nz);
      ENG(svr_sync_cpu(ctx, vol.data()));
      long evals = 0;
      char e[256] = {0};
      svr::unpermute_rows(T, 16, order);                                   // (packages are sub-stacks: one transformation per slice, stack after stack)
      if (svrh_package_to_volume_ex(ctx, nullptr, nullptr, use_nmi ? SVRH_SIM_NMI : SVRH_SIM_CC, (int)n, at.data(), ptr.data(), packages.data(),
                                    it >= 2, it >= 3, it >= 4 ? it - 2 : 1, T.data(), &tattr, vol.data(), &evals, e))
        die(std::string("package-to-volume registration: ") + e);
      svr::permute_rows(T, 16, order);
      fprintf(stderr, "package-to-volume registration: %ld similarity evaluations\n", evals);
      slice_reg = it >= 4;
      if (!slice_reg) update_matrices_from_T();
    }
    if (slice_reg) {                                                      // main.cc:829-880
      if (use_gpu_reg) {                                                  // every rank registers its own slices
        par([&](int r) { HOSTR(r, svrh_slice_to_volume_registration_gpu(hosts[r], T.data() + 16 * (size_t)rlo[r])); });
      } else {                                                            // SliceToVolumeRegistration, RG.cc:2291-2303
        std::vector<float> vol((size_t)tattr.nx * tattr.ny * tattr.nz);
        ENG(svr_sync_cpu(ctx, vol.data()));                               // _reconstructed after SyncCPU, main.cc:1189
        long evals = 0;
        char e[256] = {0};
        if (svrh_slice_to_volume_registration_ex(ctx, nullptr, nullptr, use_nmi ? SVRH_SIM_NMI : SVRH_SIM_CC, ns, grid.data(), mx, my, sattr.data(),
                                                 T.data(), &tattr, vol.data(), 0, &evals, e))
          die(std::string("slice-to-volume registration: ") + e);
        fprintf(stderr, "slice-to-volume registration: %ld similarity evaluations\n", evals);
      }
      update_matrices_from_T();
    }
    for (int r = 0; r < nr; ++r) {
      if (it == iterations - 1) {                                         // main.cc:884-896
        svrh_set_smoothing_parameters(hosts[r], delta, last_lambda);
      } else {
        double l = lambda;
        for (int i = 0; i < levels; ++i) {
          if (it == iterations * (levels - i - 1) / levels) svrh_set_smoothing_parameters(hosts[r], delta, l);
          l *= 2;
        }
      }
    }
    if (slice_reg) clk.mark("registration");
    par([&](int r) { HOSTR(r, svrh_reconstruct_iteration(hosts[r], it == iterations - 1 ? rec_last : rec_first)); });   // main.cc:930-1140
    double sc[8];
    svrh_get_state(host, nullptr, nullptr, nullptr, nullptr, sc);
    fprintf(stderr, "iteration %d: sigma %.4g mix %.3f\n", it, sc[0], sc[1]);
    clk.mark("reconstruction iteration");
    if (structural) {                                                     // what this iteration's evaluation found: in force during the next one
      std::vector<double> q(ns);
      std::vector<unsigned char> pend(ns);
      HOSTR(0, svrh_get_structural(host, q.data(), nullptr, nullptr, pend.data()));
      std::vector<int> judged(n, 0), left_out(n, 0), named;
      for (int i = 0; i < ns; ++i) {                                      // slice i of the reference's order
        const int s = inv_order[i];
        if (q[s] == q[s]) ++judged[stack_index[s]];
        if (pend[s]) { ++left_out[stack_index[s]]; named.push_back(i); }
      }
      fprintf(stderr, "structural, iteration %d:", it);
      for (size_t k = 0; k < n; ++k) fprintf(stderr, " stack %zu judged %d excluded %d%s", k, judged[k], left_out[k], k + 1 < n ? "," : ";");
      fprintf(stderr, " excluded slices:");
      for (int i : named) fprintf(stderr, " %d", i);
      fprintf(stderr, "%s\n", named.empty() ? " none" : "");
    }
    if (save_slice_transformations) {
      // SaveSlices + SaveTransformations after every iteration (main.cc:1213-1217; RG.cc:4884-4892, 4903-4919), into the working
      // directory like the reference: slice<i>.nii.gz (the masked slice), croppedSliceTransformation<i>.dof (the slice's transformation)
      // and croppedSliceToVolumeTransformation<i>.dof (reconstructed W2I x transformation x slice I2W squeezed into a rigid
      // transformation by PutMatrix, as the reference does) -- <i> = the slice's index in the reference's order
      const M4 rw2i = world_to_image(tattr);
      for (int s = 0; s < ns; ++s) {
        const int i = order[s];
        const svr_image_attr &a = sattr[s];
        std::vector<float> img((size_t)a.nx * a.ny);
        for (int y = 0; y < a.ny; ++y) memcpy(&img[(size_t)y * a.nx], &grid[((size_t)s * my + y) * mx], a.nx * sizeof(float));
        char e[256] = {0};
        if (svr_nifti_write(("slice" + std::to_string(i) + ".nii.gz").c_str(), &a, img.data(), e)) die(std::string("slice file: ") + e);
        M4 t;
        for (int q = 0; q < 16; ++q) t.m[q] = T[16 * (size_t)s + q];
        double p6[6];
        svrh_irtk_rigid_parameters(t.m, p6, nullptr);
        if (svr_dof_write(("croppedSliceTransformation" + std::to_string(i) + ".dof").c_str(), p6, e)) die(std::string("dof file: ") + e);
        const M4 c = mul(rw2i, mul(t, image_to_world(a)));
        svrh_irtk_rigid_parameters(c.m, p6, nullptr);
        if (svr_dof_write(("croppedSliceToVolumeTransformation" + std::to_string(i) + ".dof").c_str(), p6, e)) die(std::string("dof file: ") + e);
      }
    }
  }
  if (clk.on && enable_bias && sigma > 0) {                              // which bias stages ran (rank 0)
    int nb = 0, nn = 0;
    ENG(svr_get_option(ctx, "bias_corrections", &nb));
    ENG(svr_get_option(ctx, "bias_normalisations", &nn));
    fprintf(stderr, "[timing] bias correction: %d CorrectBias, %d NormaliseBias\n", nb, nn);
  }
  par([&](int r) {                                                       // main.cc:1189-1193
    ENGR(r, svr_restore_slice_intensities(ctxs[r], factors.data(), (int)factors.size(), stack_index.data() + rlo[r]));
    HOSTR(r, svrh_scale_volume_gpu(hosts[r]));
  });
  std::vector<float> vol((size_t)tattr.nx * tattr.ny * tattr.nz);
  ENG(svr_sync_cpu(ctx, vol.data()));
  char err[256] = {0};
  clk.mark("restore, scale, download");
  if (svr_nifti_write(output.c_str(), &tattr, vol.data(), err)) die(output + ": " + err);
  clk.mark("write the volume");
  if (!report_name.empty() || !sim_prefix.empty()) {
    // How the run went (not in the reference's main(); SlicesInfo RG.cc:4937-4975, SimulateStacks :1205-1262, EvaluateGPU :4503-4538).
    // The volume is on disk: nothing from here on can reach it.  Every rank projects the final volume into its slices once and
    // reduces them (svr_slice_quality); rows and stacks are written in the reference's slice order, through order[].
    std::vector<float> scale_g(ns), weight_g(ns), sim;
    std::vector<unsigned char> inside(ns);
    std::vector<double> sums((size_t)ns * SVR_SLICE_QUALITY_SUMS, 0.0);
    const bool report_ex = structural && !report_name.empty();           // three more columns: ssim n_ssim structural
    std::vector<double> ssim_sums(report_ex ? 2 * (size_t)ns : 0, 0.0);
    if (!sim_prefix.empty()) sim.resize((size_t)ns * mx * my);
    par([&](int r) {                                                     // (collective: the other ranks' vectors may still be on their way)
      HOSTR(r, svrh_get_state(hosts[r], r ? nullptr : scale_g.data(), r ? nullptr : weight_g.data(), nullptr, nullptr, nullptr));
    });
    std::vector<double> t_sim(nr, 0.0), t_qual(nr, 0.0);
    par([&](int r) {
      const size_t o = (size_t)rlo[r], nl = (size_t)(rhi[r] - rlo[r]);
      const auto t0 = std::chrono::steady_clock::now();
      ENGR(r, svr_simulate_slices(ctxs[r], inside.data() + o));
      const auto t1 = std::chrono::steady_clock::now();
      if (!report_name.empty()) ENGR(r, svr_slice_quality(ctxs[r], sums.data() + o * SVR_SLICE_QUALITY_SUMS));
      const auto t2 = std::chrono::steady_clock::now();
      if (report_ex && nl > 0) {                                          // the run's own window and constants (svrh_structural_evaluate)
        const double L = (double)vmax - (double)vmin;
        ENGR(r, svr_slice_ssim(ctxs[r], st_radius, (0.01 * L) * (0.01 * L), (0.03 * L) * (0.03 * L), ssim_sums.data() + 2 * o, nullptr));
      }
      if (!sim_prefix.empty()) ENGR(r, svr_debug_get(ctxs[r], SVR_BUF_SIMSLICES, sim.data() + o * mx * my, nl * mx * my * sizeof(float)));
      t_sim[r] = std::chrono::duration<double>(t1 - t0).count(); t_qual[r] = std::chrono::duration<double>(t2 - t1).count();
    });
    if (clk.on)
      fprintf(stderr, "[timing] forward projection of the final volume %.3f ms, svr_slice_quality %.3f ms (slowest rank, host clock)\n",
              1e3 * *std::max_element(t_sim.begin(), t_sim.end()), 1e3 * *std::max_element(t_qual.begin(), t_qual.end()));
    auto included = [&](int s) { return weight_g[s] >= 0.5f && inside[s]; };
    if (!report_name.empty()) {
      std::vector<int> r_stack(ns);
      std::vector<float> r_weight(ns), r_scale(ns);
      std::vector<unsigned char> r_inside(ns);
      std::vector<double> r_p6(6 * (size_t)ns), r_sums(sums.size()), r_ssim(ssim_sums.size());
      std::vector<unsigned char> in_force(report_ex ? ns : 0), r_force(report_ex ? ns : 0);
      if (report_ex) HOSTR(0, svrh_get_structural(host, nullptr, nullptr, in_force.data(), nullptr));
      for (int i = 0; i < ns; ++i) {                                     // row i = slice i of the reference's order
        const int s = inv_order[i];
        r_stack[i] = stack_index[s]; r_weight[i] = weight_g[s]; r_scale[i] = scale_g[s]; r_inside[i] = inside[s];
        svrh_irtk_rigid_parameters(&T[16 * (size_t)s], &r_p6[6 * (size_t)i], nullptr);
        std::copy(sums.begin() + (size_t)s * SVR_SLICE_QUALITY_SUMS, sums.begin() + (size_t)(s + 1) * SVR_SLICE_QUALITY_SUMS,
                  r_sums.begin() + (size_t)i * SVR_SLICE_QUALITY_SUMS);
        if (report_ex) { r_ssim[2 * (size_t)i] = ssim_sums[2 * (size_t)s]; r_ssim[2 * (size_t)i + 1] = ssim_sums[2 * (size_t)s + 1]; r_force[i] = in_force[s]; }
      }
      if (report_ex ? svr_slice_report_write_ex(report_name.c_str(), ns, r_stack.data(), r_weight.data(), r_inside.data(), r_scale.data(),
                                                r_p6.data(), r_sums.data(), r_ssim.data(), r_force.data(), err)
                    : svr_slice_report_write(report_name.c_str(), ns, r_stack.data(), r_weight.data(), r_inside.data(), r_scale.data(), r_p6.data(),
                                             r_sums.data(), err))
        die(report_name + ": " + err);
      // the three lists of EvaluateGPU, then what the weights alone do not say: how well each stack's kept slices match the volume
      const char *names[3] = {"Included", "Excluded", "Outside"};
      for (int kind = 0; kind < 3; ++kind) {
        int total = 0;
        fprintf(stderr, "%s slices:", names[kind]);
        for (int i = 0; i < ns; ++i) {
          const bool in = r_inside[i] != 0, kept = r_weight[i] >= 0.5f;
          if (kind == 0 ? (kept && in) : kind == 1 ? (!kept && in) : !in) { fprintf(stderr, " %d", i); ++total; }
        }
        fprintf(stderr, "\nTotal: %d\n", total);
      }
      for (size_t k = 0; k < n; ++k) {
        std::vector<double> v;
        for (int i = 0; i < ns; ++i) {
          if (r_stack[i] != (int)k || !(r_weight[i] >= 0.5f && r_inside[i])) continue;
          double d4[4];
          svr_slice_quality_derive(&r_sums[(size_t)i * SVR_SLICE_QUALITY_SUMS], d4);
          if (d4[0] == d4[0]) v.push_back(d4[0]);
        }
        std::sort(v.begin(), v.end());
        const double med = v.empty() ? NAN : (v.size() % 2 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]));
        if (v.empty()) fprintf(stderr, "stack %zu: no included slice with a defined ncc\n", k);
        else fprintf(stderr, "stack %zu: median ncc %.6f over %zu included slices\n", k, med, v.size());
      }
    }
    if (!sim_prefix.empty()) {
      int base = 0;                                                      // the stack's first slice in the reference's order
      for (size_t k = 0; k < n; ++k) {
        const svr_image_attr &a = stacks[k].a;
        std::vector<float> out((size_t)a.nx * a.ny * a.nz, 0.0f);       // excluded and outside slices stay zero, as SimulateStacks leaves them
        for (int j = 0; j < a.nz; ++j) {
          const int s = inv_order[base + j];
          if (!included(s)) continue;
          for (int y = 0; y < a.ny; ++y)
            for (int x = 0; x < a.nx; ++x) {
              const size_t g = ((size_t)s * my + y) * mx + x;
              if (grid[g] != -1.0f) out[((size_t)j * a.ny + y) * a.nx + x] = sim[g];
            }
        }
        base += a.nz;
        const std::string path = sim_prefix + std::to_string(k) + ".nii.gz";
        if (svr_nifti_write(path.c_str(), &a, out.data(), err)) die(path + ": " + err);
      }
    }
    clk.mark("slice report, simulated stacks");
  }
  if (!extras.empty()) {
    // The second images into the reconstructed space (not in the reference's main() but for --manualMask, reconstruction.cc:1240-1250).  The
    // volume is on disk: nothing from here on can reach it.  Every rank scatters its own slices with the weights the last SR iteration
    // would scatter with, the ranks' sums are brought together (svrh_channel_reconstruct), and rank 0 divides or votes.
    const size_t nvv = (size_t)tattr.nx * tattr.ny * tattr.nz;
    double t_sr = 0.0, t_scatter = 0.0;
    int n_scatter = 0;
    if (clk.on) {
      // the yardstick, from the same run: one SR scatter of rank 0's slices (host clock around the blocking call; addon | cmap are free now)
      const auto t0 = std::chrono::steady_clock::now();
      ENG(svr_superresolution_backproject(ctx, nullptr));
      t_sr = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    auto scatter = [&](ExtraSet &e, int flags, float match) {
      std::vector<double> t(nr, 0.0);
      par([&](int r) {
        const size_t o = (size_t)rlo[r];
        const auto t0 = std::chrono::steady_clock::now();
        HOSTR(r, svrh_channel_reconstruct(hosts[r], e.grid.data() + o * mx * my, e.unit_on.data() + o, flags, match));
        t[r] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      });
      t_scatter += *std::max_element(t.begin(), t.end());
      ++n_scatter;
    };
    // covered voxels (cover[v] > 0) and the values there, from the downloaded volumes
    auto say = [&](const std::string &what, const std::string &path, const std::vector<float> &v, const std::vector<float> &cover) {
      size_t cnt = 0;
      double lo = INFINITY, hi = -INFINITY, sum = 0;
      for (size_t i = 0; i < v.size(); ++i)
        if (cover[i] > 0.0f) { ++cnt; lo = std::min(lo, (double)v[i]); hi = std::max(hi, (double)v[i]); sum += v[i]; }
      if (cnt) fprintf(stderr, "%s %s: %zu covered voxels, min %.9g max %.9g mean %.9g\n", what.c_str(), path.c_str(), cnt, lo, hi, sum / (double)cnt);
      else fprintf(stderr, "%s %s: no covered voxel\n", what.c_str(), path.c_str());
    };
    for (auto &e : extras) {
      std::vector<float> out(nvv), cover(nvv);
      if (!e.labels) {
        scatter(e, 0, 0.0f);
        ENG(svr_channel_finish(ctx, 0.0f, out.data()));
        ENG(svr_debug_get(ctx, SVR_BUF_CONFIDENCE_MAP, cover.data(), nvv * sizeof(float)));          // den: where it is positive a slice reached
        if (svr_nifti_write(e.out.c_str(), &tattr, out.data(), err)) die(e.out + ": " + err);
        say(e.what, e.out, out, cover);
      } else {
        for (size_t k = 0; k < e.label_values.size(); ++k) {
          scatter(e, SVR_CHANNEL_INDICATOR, e.label_values[k]);
          ENG(svr_channel_vote(ctx, e.label_values[k], k == 0));
        }
        ENG(svr_channel_vote_fetch(ctx, 0.0f, out.data(), cover.data()));                            // (the confidence is positive exactly where a slice reached)
        if (svr_nifti_write(e.out.c_str(), &tattr, out.data(), err)) die(e.out + ": " + err);
        say(e.what + " (" + std::to_string(e.label_values.size()) + " labels)", e.out, out, cover);
        if (!e.conf.empty()) {
          if (svr_nifti_write(e.conf.c_str(), &tattr, cover.data(), err)) die(e.conf + ": " + err);
          say("--labelConfidence", e.conf, cover, cover);
        }
      }
    }
    if (clk.on)
      fprintf(stderr, "[timing] %d channel / label scatters, %.3f ms each (upload, scatter%s; slowest rank, host clock); one SR scatter of rank 0's slices %.3f ms\n",
              n_scatter, 1e3 * t_scatter / std::max(1, n_scatter), nr > 1 ? ", all-reduce" : "", 1e3 * t_sr);
    clk.mark("channels, labels");
  }
  if (debug) {                                                           // SaveTransformations, RG.cc:4903-4915
    const size_t cut = output.find_last_of('/');
    const std::string folder = cut == std::string::npos ? "." : output.substr(0, cut);
    for (int s = 0; s < ns; ++s) {
      double p6[6];
      svrh_irtk_rigid_parameters(&T[16 * (size_t)s], p6, nullptr);
      char e[256] = {0};
      const std::string path = folder + "/transformation" + std::to_string(order[s]) + ".dof";
      if (svr_dof_write(path.c_str(), p6, e)) die(path + ": " + e);
    }
  }
  for (int r = 0; r < nr; ++r) svrh_destroy(hosts[r]);
  svr_group_destroy(group);
  for (int r = 0; r < nr; ++r) svr_destroy(ctxs[r]);
  clk.mark("teardown");
  return 0;
}
