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
// both.  --useLNCC [--lnccRadius 3] makes the same two registrations use a windowed cross correlation (csrc/svr_lncc.inc), which
// tolerates the bias field that is only estimated after the slices are registered; the reference has no such metric.  --useNMI makes the IRTK schedule's slice-to-volume and package-to-volume registrations use normalised mutual
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
// --echoStacks <x> f_1 .. f_N (a deviation), given 2 to 16 times, carries a multi-echo or diffusion series through one run: every echo is a channel
// set of its own (the same reading, cropping, packing and reconstruction), written as --echoOutput <prefix><k>.nii.gz, and --fitRate / --fitT /
// --fitAmplitude / --fitResidual / --fitCount fit S(x) = A exp(-R x) to the reconstructed echoes voxel by voxel (svr_monoexp_fit, csrc/svr_fit.inc).
// Not built, refused loudly: patch/superpixel modes, the CPU reconstruction path.
//
// Where things are.  Three plain structs: Options (what the command line says; const after parse_options), Problem (the host-side
// data: stacks, mask, template, the packed slices, the second images) and Ranks (svr_launch.h) with one svrh_recon* per rank.
//   usage
//   second images      declare_extras, read_extras, crop_extras_with, pack_extras, dump_channels, superresolve_extra, reconstruct_extras,
//                      fit_echoes -- all of --channelStacks / --labelStacks / --manualMask / --echoStacks, next to each other
//   options            parse_options (with every refusal that needs no file, in a fixed order)
//   set-up             read_inputs, make_mask, select_template_by_motion, make_template, crop_and_register_stacks, pack_slices (--sfolder)
//   engines            dump_problem, shard_slices, setup_engines, read_tfolder, seed_reference_volume
//   the loop           run_iterations: register_packages, register_slices, set_smoothing_for_iteration, structural_line,
//                      save_slice_transformations
//   afterwards         write_volume, report_final_slices (write_slice_report, write_simulated_stacks), save_debug_transformations
// main() is the sequence of these, with the stage clock's marks between them.
#include <functional>
#include <set>
#include <thread>

#include <future>

#include "svr_launch.h"

namespace {

// ---- options (main.cc:164-211) -----------------------------------------------------------------------
struct Options {
  std::string output, mask_name, tfolder, sfolder;
  bool debug = false, dry_run = false, save_slice_transformations = false;
  std::string dump_name;
  std::vector<std::string> inputs, tspecs;
  std::vector<double> thickness;
  std::vector<int> force_excluded, devices, packages;
  int iterations = 4, levels = 3, rec_first = 4, rec_last = 13, num_stacks_tuner = 0;
  double resolution = 0.75, average = 700, delta = 150, lambda = 0.02, last_lambda = 0.01, smooth_mask = 4;
  bool no_matching = false, use_gpu_reg = false, no_registration = false, use_nmi = false, use_lncc = false;
  int lncc_radius = 3;
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
  int channel_iterations = 0;                                             // --channelIterations (not a reference option): SR iterations on the --channelStacks set
  double channel_delta = 0, channel_lambda = 0;                           // --channelDelta, --channelLambda; 0 = not given (from --delta and the ranges / --lastIterLambda)
  bool have_channel_sr_opt = false;                                       // one of the three was named
  bool channel_guide = false, channel_guide_only = false;                 // --channelGuide, --channelGuideOnly (not reference options): the -o volume's edges
  double channel_guide_delta = 0;                                         // --channelGuideDelta; 0 = not given (from --delta and the ranges)
  bool have_channel_guide_opt = false;                                    // --channelGuideDelta or --channelGuideOnly was named
  std::vector<std::string> echo_x;                                       // --echoStacks <x> f_1 .. f_N (not reference options), once per echo: the abscissa as given,
  std::vector<std::vector<std::string>> echo_names;                      // ... and a file or `none` per -i stack
  std::string echo_out;                                                   // --echoOutput <prefix>: echo k is written as <prefix><k>.nii.gz
  int echo_iterations = 0;                                                // --echoIterations: SR iterations on every echo, as --channelIterations on the channel
  bool echo_guide = false;                                                // --echoGuide: as --channelGuide
  std::string fit_rate, fit_t, fit_amplitude, fit_residual, fit_count;   // --fitRate, --fitT, --fitAmplitude, --fitResidual, --fitCount: S(x) = A exp(-R x) over the echoes
  int fit_iterations = 0;                                                 // --fitIterations: Gauss-Newton steps after the log-linear fit
  double fit_floor = 0, fit_max_t = 0;                                    // --fitFloor; --fitMaxT (0 = not given: ten times the largest |x|)
  bool have_echo_dep_opt = false;                                         // an --echo* / --fit* option other than --echoStacks was named
  int coeff_table = -1;                                                   // -1: the engine's default (on since round 6), 1 / 0: --coeffTable / --noCoeffTable
  size_t tmpl = 0;                                                        // the first stack whose -t is id (main.cc:452-457)
};

// a second image per stack (--channelStacks, --labelStacks, --manualMask)
struct ExtraSet {
  std::string what;                    // the option, for messages
  bool labels = false;
  std::vector<std::string> names;      // per stack; "none" = the stack has none
  std::string out, conf;
  std::vector<Image> imgs;             // per stack (empty image where none)
  std::vector<float> grid;             // [ns][my][mx], 0 outside a slice's extent
  std::vector<unsigned char> unit_on;  // [ns]
  std::vector<float> label_values;     // ascending
  int echo = -1;                       // --echoStacks: which echo, in the order given (-1: not an echo)
  double x = 0;                        // ... and its abscissa
};

// the host-side data.  The per-slice arrays are in the reference's order (stack after stack) until shard_slices, in the sharded
// numbering afterwards
struct Problem {
  std::vector<Image> stacks;           // cropped in place
  std::vector<M4> ts;
  size_t tmpl = 0;
  std::vector<double> thickness;
  bool have_mask = false;
  Image mask_img, vol_mask;
  svr_image_attr tattr;
  double resolution = 0;               // --resolution, or the smallest voxel size it stood for (CreateTemplate)
  std::vector<float> factors;
  int ns = 0, mx = 0, my = 0;
  std::vector<float> grid, i2w, w2i, st, sti, dims;
  std::vector<int> sizes_x, sizes_y, stack_index;
  std::vector<svr_image_attr> sattr;
  std::vector<double> T;
  double vmin = 1e300, vmax = -1e300;
  float ri2w[16], rw2i[16];            // the volume's own matrices
  std::vector<int> force_excluded;     // --force_exclude, in the numbering of the arrays above
  std::vector<ExtraSet> extras;
};

void host_check(svrh_recon *h, int rc, const char *what) { if (rc) die(std::string(what) + ": " + svrh_last_error(h)); }
#define HOSTR(r, call) host_check(hosts[r], (call), #call)

void usage() {
  printf("usage: SVRreconstructionGPU -o <volume> -i <stack_1> .. <stack_N> [-m <mask>] [-t id|<4x4.txt> ..] [--thickness th_1 ..]\n"
         "       [--iterations 4] [--resolution 0.75] [--multires 3] [--average 700] [--delta 150] [--lambda 0.02]\n"
         "       [--lastIterLambda 0.01] [--smooth_mask 4] [--no_intensity_matching] [--force_exclude i ..]\n"
         "       [--rec_iterations_first 4] [--rec_iterations_last 13] [--packages p_1 ..] [--useGPUReg] [--no_registration] [--tfolder dir] [--sfolder dir]\n"
         "       [--saveSliceTransformations] [--coeffTable | --noCoeffTable] [-d device_1 .. device_N]\n"
         "       [--enableBiasCorrection] [--sigma 12] [--global_bias_correction 0] [--low_intensity_cutoff 0.01] [--disableBiasCorrection] [--useNMI]\n"
         "       [--useLNCC] [--lnccRadius 3]\n"
         "       [--useAutoTemplate] [--autoTemplateCentral] [--sliceReport file] [--simulatedStacks prefix] [--referenceVolume file]\n"
         "       [--channelStacks f_1 .. f_N --channelOutput file [--channelIterations 0] [--channelDelta d] [--channelLambda l]\n"
         "        [--channelGuide [--channelGuideDelta d] [--channelGuideOnly]]]\n"
         "       [--echoStacks x_1 f_1 .. f_N --echoStacks x_2 f_1 .. f_N [--echoStacks ..] [--echoOutput prefix] [--echoIterations 0] [--echoGuide]\n"
         "        [--fitRate file] [--fitT file] [--fitAmplitude file] [--fitResidual file] [--fitCount file] [--fitMaxT Tmax] [--fitIterations 0]\n"
         "        [--fitFloor 0]]\n"
         "       [--labelStacks f_1 .. f_N --labelOutput file [--labelConfidence file]]\n"
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
         "                          no super-resolution iterations unless --channelIterations asks for them), 0 where no slice with a channel\n"
         "                          reaches.  Its own value never excludes a pixel: zero and negative values count.  The -o volume is the same\n"
         "                          with and without it.\n"
         "  --channelIterations n   deviation from the reference: refine that average by n super-resolution iterations [0] with the run's final\n"
         "                          slice transformations and robust weights held fixed, so that the channel gets the through-plane resolution\n"
         "                          of the -o volume instead of the slice profile's blur.  Every iteration projects the channel volume into the\n"
         "                          slices, scatters the weighted residuals against the channel's pixels and runs the edge-preserving volume\n"
         "                          update; nothing is estimated, no intensity scale or bias field is applied, values are clamped to the\n"
         "                          channel's range widened by a tenth on either side.  A constant channel is returned as the average.  Voxels of\n"
         "                          the mask that no slice with a channel reaches (stacks given as `none`) hold 0 and count as 0 for their\n"
         "                          neighbours.  Needs --channelStacks; --labelStacks and --manualMask keep their vote / average.  Not with\n"
         "                          --sfolder.  With 0 or without the option nothing changes.  One stderr line reports the parameters.\n"
         "  --channelDelta d        deviation from the reference: the edge scale of that update in the channel's units [--delta times the\n"
         "                          channel's range over the primary's intensity range].\n"
         "  --channelLambda l       deviation from the reference: its smoothing weight [--lastIterLambda]; the step is min(1, 0.05 / l).\n"
         "  --channelGuide          deviation from the reference: the volume update of --channelIterations also weighs every pair of neighbours\n"
         "                          by the difference of the -o volume between them (the reconstruction as the device holds it when the channel\n"
         "                          stage starts): b = f / sqrt(1 + f (dC / delta)^2 + f (dG / delta_g)^2).  A noisy map is smoothed inside\n"
         "                          the tissues the anatomy shows and not across their boundaries, and --channelDelta can be large.  Needs\n"
         "                          --channelStacks and --channelIterations > 0.  The -o volume is the same with and without it; --labelStacks\n"
         "                          and --manualMask are untouched.  A constant -o volume guides nothing: the option is dropped with a message.\n"
         "                          One stderr line reports delta_g, the guide's range and the mode.\n"
         "  --channelGuideDelta d   deviation from the reference: the guide's edge scale delta_g in the -o volume's units [--delta times the\n"
         "                          written volume's range inside the mask over the run's intensity range].  Needs --channelGuide.\n"
         "  --channelGuideOnly      deviation from the reference: the channel's own differences leave the weight (--channelDelta still scales\n"
         "                          --channelLambda).  Needs --channelGuide.\n"
         "  --echoStacks <x> f_1 .. f_N\n"
         "                          deviation from the reference, which has no such option: one acquisition of a multi-echo or diffusion series,\n"
         "                          given 2 to 16 times in one run.  <x> is its abscissa (echo time, b-value): a finite number, all different; then a\n"
         "                          file or `none` per -i stack under the rules of --channelStacks.  Every echo is reconstructed like a channel of its\n"
         "                          own with the run's one motion estimate and its robust weights, after the -o volume and the other second images\n"
         "                          are written.  Needs --echoOutput or a --fit* output.  Not with --sfolder.  The -o volume, --channelOutput and\n"
         "                          --labelOutput are the same with and without it.  One stderr line per echo.\n"
         "  --echoOutput <prefix>   deviation from the reference: write echo k (from 0, in the order given) as <prefix><k>.nii.gz.\n"
         "  --echoIterations n      deviation from the reference: refine every echo by n super-resolution iterations [0], exactly as\n"
         "                          --channelIterations n refines the channel: delta from the echo's own range, lambda from --lastIterLambda, the clamp\n"
         "                          widened by a tenth.  --echoGuide: as --channelGuide, with delta_g by the same rule; needs --echoIterations > 0.\n"
         "  --fitRate <file> --fitT <file> --fitAmplitude <file> --fitResidual <file> --fitCount <file>\n"
         "                          deviation from the reference: fit S(x) = A exp(-R x) to the reconstructed echoes, voxel by voxel on the device, and\n"
         "                          write R (R2*, R2, ADC), T = 1 / R, A, the root mean square residual of the fit and the number of echoes that\n"
         "                          counted, on the reconstruction grid.  An echo counts in a voxel when its value is finite and above --fitFloor v\n"
         "                          [0, not negative]; with fewer than two, or a degenerate system, every map is 0 there.  The fit is the log-linear\n"
         "                          one weighted by the squared signal; --fitIterations n [0, at most 50] adds n Gauss-Newton steps on the signal\n"
         "                          itself, kept where they do not raise the residual.  --fitT is 1 / R where R > 1 / Tmax, Tmax where a fitted\n"
         "                          voxel has R <= 1 / Tmax, 0 where nothing was fitted; --fitMaxT Tmax [ten times the largest |x|].  No Rician\n"
         "                          bias handling, no second component.  One stderr line reports the fitted voxels and their median T.\n"
         "                          All of these need --echoStacks.\n"
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
         "  --useLNCC               deviation from the reference, which has no local metric: slice-to-volume and package-to-volume\n"
         "                          registration use a windowed normalised cross correlation -- the signed squared correlation of every\n"
         "                          (2 radius + 1)^2 window, averaged -- instead of the global one.  It ignores any intensity change that is\n"
         "                          linear inside a window, so slices register under a bias field (coil falloff, differing receive fields)\n"
         "                          that --enableBiasCorrection only estimates afterwards.  Stack-to-stack registration stays CC.\n"
         "                          Not with --useNMI, not with --useGPUReg (CC only).\n"
         "  --lnccRadius            radius of that window in pixels of the registration level, 1 .. 7 [3].\n"
         "  --enableBiasCorrection  deviation from the reference, whose bias correction cannot be switched on: run BiasGPU and\n"
         "                          NormaliseBiasGPU in every SR iteration (bias field stdev --sigma mm; sigma <= 0: no bias step).\n"
         "                          Without it bias correction is off, as in the reference; --disableBiasCorrection is accepted and changes nothing.\n");
}

// ---- second images per stack (--channelStacks, --labelStacks, --manualMask), from the option checks to the written volumes ----------
// what can be refused without reading a file
void declare_extras(const Options &p, std::vector<ExtraSet> &extras) {
  const size_t n = p.inputs.size();
  if (p.have_channel_opt && p.channel_out.empty()) die("--channelStacks needs --channelOutput <file> for the reconstructed channel");
  if (!p.have_channel_opt && !p.channel_out.empty()) die("--channelOutput needs --channelStacks f_1 .. f_N (a file or `none` per -i stack)");
  if (p.have_label_opt && p.label_out.empty()) die("--labelStacks needs --labelOutput <file> for the reconstructed labels");
  if (!p.have_label_opt && !p.label_out.empty()) die("--labelOutput needs --labelStacks f_1 .. f_N (a file or `none` per -i stack)");
  if (!p.have_label_opt && !p.label_conf.empty()) die("--labelConfidence needs --labelStacks f_1 .. f_N and --labelOutput");
  auto add = [&](const char *what, bool labels, const std::vector<std::string> &names, const std::string &out, const std::string &conf) {
    if (!p.sfolder.empty())
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
  if (p.have_channel_opt) add("--channelStacks", false, p.channel_names, p.channel_out, "");
  if (p.have_label_opt) add("--labelStacks", true, p.label_names, p.label_out, p.label_conf);
  if (!p.manual_name.empty()) {
    std::vector<std::string> names(n, "none");
    names[0] = p.manual_name;
    const size_t cut = p.manual_name.find_last_of('/');                  // reconstruction.cc:1243-1249: "PSFTransformed_" + the file's name, in its directory
    const std::string out = cut == std::string::npos ? "PSFTransformed_" + p.manual_name
                                                     : p.manual_name.substr(0, cut + 1) + "PSFTransformed_" + p.manual_name.substr(cut + 1);
    add("--manualMask", false, names, out, "");
  }
  // --echoStacks: a set per echo, after the others, in the order given
  const size_t K = p.echo_x.size();
  if (K && (K < 2 || K > 16)) die("--echoStacks: " + std::to_string(K) + " echo sets; a run takes 2 to 16 (one --echoStacks <x> f_1 .. f_N per echo)");
  const bool any_fit = !p.fit_rate.empty() || !p.fit_t.empty() || !p.fit_amplitude.empty() || !p.fit_residual.empty() || !p.fit_count.empty();
  if (K && p.echo_out.empty() && !any_fit)
    die("--echoStacks needs --echoOutput <prefix> for the reconstructed echoes or a --fitRate / --fitT / --fitAmplitude / --fitResidual / --fitCount <file>");
  std::vector<double> xs;
  for (size_t k = 0; k < K; ++k) {
    char *end = nullptr;
    const double x = strtod(p.echo_x[k].c_str(), &end);
    if (p.echo_x[k].empty() || *end || !std::isfinite(x))
      die("--echoStacks: `" + p.echo_x[k] + "` is not a finite number: the first value is the echo's abscissa (echo time, b-value), then a file or `none` per -i stack");
    if (std::find(xs.begin(), xs.end(), x) != xs.end()) die("--echoStacks: the abscissa " + p.echo_x[k] + " is given twice: a duplicate x fits nothing");
    xs.push_back(x);
  }
  for (size_t k = 0; k < K; ++k) {
    add(("--echoStacks " + p.echo_x[k]).c_str(), false, p.echo_names[k], p.echo_out.empty() ? "" : p.echo_out + std::to_string(k) + ".nii.gz", "");
    extras.back().echo = (int)k;
    extras.back().x = xs[k];
  }
  if (!p.channels_dump.empty() && extras.empty()) die("--dumpChannels writes the packed grids of --channelStacks / --labelStacks / --manualMask / --echoStacks: give one of them");
}

void read_extras(const Options &opt, Problem &P) {
  const size_t n = P.stacks.size();
  for (auto &e : P.extras) {
    e.imgs.resize(n);
    for (size_t k = 0; k < n; ++k) {
      if (e.names[k] == "none") continue;
      e.imgs[k] = read_image(e.names[k]);
      // on its stack's grid as read: the same dimensions, the same image-to-world matrix
      const svr_image_attr &a = e.imgs[k].a, &b = P.stacks[k].a;
      bool same = a.nx == b.nx && a.ny == b.ny && a.nz == b.nz;
      if (same) {
        const M4 ma = image_to_world(a), mb = image_to_world(b);
        for (int q = 0; q < 16; ++q) same = same && fabs(ma.m[q] - mb.m[q]) <= 1e-3;
      }
      if (!same)
        die(e.what + ": " + e.names[k] + " is not on the grid of its stack " + opt.inputs[k] + " (" + std::to_string(a.nx) + "x" + std::to_string(a.ny) + "x" +
            std::to_string(a.nz) + " against " + std::to_string(b.nx) + "x" + std::to_string(b.ny) + "x" + std::to_string(b.nz) +
            ", or another image-to-world matrix): resample it onto the stack first");
    }
  }
}

// stack k was cropped with m: its second images follow (the crop depends on the mask alone)
void crop_extras_with(std::vector<ExtraSet> &extras, size_t k, const Image &m) {
  for (auto &e : extras) if (!e.imgs[k].d.empty()) e.imgs[k] = crop_image(e.imgs[k], m);
}

// The second images, cut and packed like the primaries: slice sl = plane j of stack k, in the same order.  Their values are kept as they
// are: no `v < 0.01 -> -1`, no mask, no stack factor -- which pixels count is the primary's business (svr_channel_scatter's pixel set)
void pack_extras(Problem &P) {
  const int ns = P.ns, mx = P.mx, my = P.my;
  for (auto &e : P.extras) {
    e.grid.assign((size_t)ns * mx * my, 0.0f);
    e.unit_on.assign(ns, 0);
    int sl = 0;
    for (size_t k = 0; k < P.stacks.size(); ++k)
      for (int j = 0; j < P.stacks[k].a.nz; ++j, ++sl) {
        const Image &c = e.imgs[k];
        const svr_image_attr &a = P.stacks[k].a;
        if (c.d.empty()) continue;
        if (c.a.nx != a.nx || c.a.ny != a.ny || c.a.nz != a.nz) die(e.what + ": " + e.names[k] + " was not cropped like its stack");
        e.unit_on[sl] = 1;
        for (int y = 0; y < c.a.ny; ++y)
          for (int x = 0; x < c.a.nx; ++x) e.grid[((size_t)sl * my + y) * mx + x] = (float)c.at(x, y, j);
      }
    if (!e.labels) continue;
    // the labels: the distinct values over the pixels that can count (the primary pixel is not -1, the stack has a label map)
    std::set<float> seen;
    for (int s = 0; s < ns; ++s) {
      if (!e.unit_on[s]) continue;
      for (size_t i = 0; i < (size_t)mx * my; ++i) {
        const size_t g = (size_t)s * mx * my + i;
        if (P.grid[g] == -1.0f) continue;
        const float v = e.grid[g];
        if (!(v >= 0.0f && v <= 65535.0f) || v != floorf(v))
          die(e.what + ": " + e.names[P.stack_index[s]] + " holds the value " + std::to_string(v) + ": labels are integers in 0..65535");
        if (seen.insert(v).second && seen.size() > 64) die(e.what + ": more than 64 different labels");
      }
    }
    e.label_values.assign(seen.begin(), seen.end());                     // ascending: ties go to the smallest label
    if (e.label_values.empty()) die(e.what + ": no labelled pixel lies inside the mask");
  }
}

// test hook (tests/test_channel.py): {sets, ns, mx, my}, then per set {labels, number of labels}, unit_on [ns], the packed grid, the labels
void dump_channels(const std::string &name, const Problem &P) {
  FILE *f = fopen(name.c_str(), "wb");
  if (!f) die("cannot write " + name);
  const int hdr[4] = {(int)P.extras.size(), P.ns, P.mx, P.my};
  fwrite(hdr, sizeof(int), 4, f);
  for (auto &e : P.extras) {
    const int h2[2] = {e.labels ? 1 : 0, (int)e.label_values.size()};
    fwrite(h2, sizeof(int), 2, f);
    fwrite(e.unit_on.data(), 1, e.unit_on.size(), f);
    fwrite(e.grid.data(), sizeof(float), e.grid.size(), f);
    fwrite(e.label_values.data(), sizeof(float), e.label_values.size(), f);
  }
  fclose(f);
}

// What the SR iterations on a second image are asked: --channelIterations and its companions for the channel, --echoIterations / --echoGuide with
// every default for an echo.  The two names head the stderr lines
struct ExtraSr {
  const char *iterations_name, *guide_name;
  int iterations;
  double delta, lambda, guide_delta;     // 0 = not given
  bool guide, guide_only;
};

// --channelIterations / --echoIterations: the average of a second image refined by SR iterations with the run's final motion and weights
// (svrh_channel_superresolve; collective) -> out on rank 0
void superresolve_extra(const ExtraSr &q, const Options &opt, const Problem &P, const Ranks &R, const std::vector<svrh_recon *> &hosts, const ExtraSet &e,
                        std::vector<float> &out) {
  const size_t nvv = (size_t)P.tattr.nx * P.tattr.ny * P.tattr.nz, slice = (size_t)P.mx * P.my;
  svr_ctx *ctx = R.ctxs[0];
  // the channel's range over the pixels that can count -- the primary pixel is not -1, the stack has a channel --, over every rank's slices
  double c_min = INFINITY, c_max = -INFINITY;
  for (int s = 0; s < P.ns; ++s) {
    if (!e.unit_on[s]) continue;
    for (size_t i = 0; i < slice; ++i) {
      const size_t g = (size_t)s * slice + i;
      if (P.grid[g] == -1.0f) continue;
      c_min = std::min(c_min, (double)e.grid[g]); c_max = std::max(c_max, (double)e.grid[g]);
    }
  }
  if (!(c_max >= c_min) || !std::isfinite(c_min) || !std::isfinite(c_max)) die(e.what + ": no finite channel value lies inside the mask");
  const double R_c = c_max - c_min, R_s = P.vmax - P.vmin;
  const double lambda_c = q.lambda > 0 ? q.lambda : opt.last_lambda;
  const double delta_c = q.delta > 0 ? q.delta : (R_s > 0 ? opt.delta * R_c / R_s : 0.0);
  // a constant channel has nothing to refine (and no scale for delta): the average is the answer
  const int n_it = R_c > 0 && delta_c > 0 ? q.iterations : 0;
  fprintf(stderr, "%s %d%s: delta %.9g lambda %.9g alpha %.9g, channel range [%.9g, %.9g], clamp [%.9g, %.9g]\n", q.iterations_name, q.iterations,
          n_it ? "" : " (constant channel: none run)", delta_c, lambda_c, std::min(1.0, 0.05 / lambda_c), c_min, c_max, c_min - 0.1 * R_c, c_max + 0.1 * R_c);
  // the guide: the written volume, which every rank's device still holds (NULL = a copy of it).  Its range over the mask's voxels gives
  // delta_g the way the channel's range gives delta_c
  bool guided = q.guide && n_it > 0;
  double delta_g = 0.0;
  if (guided) {
    std::vector<float> vol(nvv);
    ENGR(R, 0, svr_sync_cpu(ctx, vol.data()));
    double g_min = INFINITY, g_max = -INFINITY;
    for (size_t i = 0; i < nvv; ++i)
      if (P.vol_mask.d[i] != 0) { g_min = std::min(g_min, (double)vol[i]); g_max = std::max(g_max, (double)vol[i]); }
    const double R_g = g_max >= g_min && std::isfinite(g_min) && std::isfinite(g_max) ? g_max - g_min : 0.0;
    delta_g = q.guide_delta > 0 ? q.guide_delta : (R_s > 0 ? opt.delta * R_g / R_s : 0.0);
    if (!(R_g > 0) || !(delta_g > 0) || !std::isfinite(delta_g)) {
      fprintf(stderr, "%s: the written volume is constant inside the mask (range %.9g) and guides nothing: dropped\n", q.guide_name, R_g);
      guided = false;
    } else {
      fprintf(stderr, "%s: delta_g %.9g, guide range %.9g [%.9g, %.9g], %s\n", q.guide_name, delta_g, R_g, g_min, g_max,
              q.guide_only ? "guide only" : "joint with the channel's differences");
    }
  }
  R.par([&](int r) {
    const size_t o = (size_t)R.rlo[r];
    if (guided)
      HOSTR(r, svrh_channel_superresolve_guided(hosts[r], e.grid.data() + o * slice, e.unit_on.data() + o, n_it, delta_c, lambda_c,
                                                (float)(c_min - 0.1 * R_c), (float)(c_max + 0.1 * R_c), r == 0 ? out.data() : nullptr, nullptr,
                                                delta_g, q.guide_only ? 1 : 0));
    else
      HOSTR(r, svrh_channel_superresolve(hosts[r], e.grid.data() + o * slice, e.unit_on.data() + o, n_it, n_it ? delta_c : 1.0, lambda_c,
                                         (float)(c_min - 0.1 * R_c), (float)(c_max + 0.1 * R_c), r == 0 ? out.data() : nullptr));
  });
}

// The second images into the reconstructed space (not in the reference's main() but for --manualMask, reconstruction.cc:1240-1250).  The
// volume is on disk: nothing from here on can reach it.  Every rank scatters its own slices with the weights the last SR iteration
// would scatter with, the ranks' sums are brought together (svrh_channel_reconstruct), and rank 0 divides or votes.  The echoes of
// --echoStacks come last, in the order given, and stay in `echoes` ([K][nvv]) for the fit.
void reconstruct_extras(const Options &opt, const Problem &P, const Ranks &R, const std::vector<svrh_recon *> &hosts, bool timing, std::vector<float> &echoes) {
  const size_t nvv = (size_t)P.tattr.nx * P.tattr.ny * P.tattr.nz, slice = (size_t)P.mx * P.my;
  svr_ctx *ctx = R.ctxs[0];
  char err[256] = {0};
  const ExtraSr channel_sr{"--channelIterations", "--channelGuide", opt.channel_iterations, opt.channel_delta, opt.channel_lambda, opt.channel_guide_delta,
                           opt.channel_guide, opt.channel_guide_only};
  const ExtraSr echo_sr{"--echoIterations", "--echoGuide", opt.echo_iterations, 0.0, 0.0, 0.0, opt.echo_guide, false};
  echoes.assign(opt.echo_x.size() * nvv, 0.0f);
  double t_sr = 0.0, t_scatter = 0.0;
  int n_scatter = 0;
  if (timing) {
    // the yardstick, from the same run: one SR scatter of rank 0's slices (host clock around the blocking call; addon | cmap are free now)
    const auto t0 = std::chrono::steady_clock::now();
    ENGR(R, 0, svr_superresolution_backproject(ctx, nullptr));
    t_sr = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }
  auto scatter = [&](const ExtraSet &e, int flags, float match) {
    std::vector<double> t(R.nr, 0.0);
    R.par([&](int r) {
      const size_t o = (size_t)R.rlo[r];
      const auto t0 = std::chrono::steady_clock::now();
      HOSTR(r, svrh_channel_reconstruct(hosts[r], e.grid.data() + o * slice, e.unit_on.data() + o, flags, match));
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
  for (auto &e : P.extras) {
    std::vector<float> out(nvv), cover(nvv);
    const bool sr = !e.labels && (e.echo >= 0 ? opt.echo_iterations > 0 : opt.channel_iterations > 0 && e.what == "--channelStacks");
    if (sr) {
      // --channelIterations on the channel, --echoIterations on every echo: the same refinement, the echoes with the defaults
      superresolve_extra(e.echo >= 0 ? echo_sr : channel_sr, opt, P, R, hosts, e, out);
      if (!e.out.empty() && svr_nifti_write(e.out.c_str(), &P.tattr, out.data(), err)) die(e.out + ": " + err);
      for (size_t i = 0; i < nvv; ++i) cover[i] = out[i] != 0.0f ? 1.0f : 0.0f;                          // (0 where no slice with a channel reaches)
      say(e.what + " (non-zero voxels)", e.out.empty() ? "(not written)" : e.out, out, cover);
    } else if (!e.labels) {
      scatter(e, 0, 0.0f);
      ENGR(R, 0, svr_channel_finish(ctx, 0.0f, out.data()));
      ENGR(R, 0, svr_debug_get(ctx, SVR_BUF_CONFIDENCE_MAP, cover.data(), nvv * sizeof(float)));        // den: where it is positive a slice reached
      if (!e.out.empty() && svr_nifti_write(e.out.c_str(), &P.tattr, out.data(), err)) die(e.out + ": " + err);
      say(e.what, e.out.empty() ? "(not written)" : e.out, out, cover);
    } else {
      for (size_t k = 0; k < e.label_values.size(); ++k) {
        scatter(e, SVR_CHANNEL_INDICATOR, e.label_values[k]);
        ENGR(R, 0, svr_channel_vote(ctx, e.label_values[k], k == 0));
      }
      ENGR(R, 0, svr_channel_vote_fetch(ctx, 0.0f, out.data(), cover.data()));                          // (the confidence is positive exactly where a slice reached)
      if (svr_nifti_write(e.out.c_str(), &P.tattr, out.data(), err)) die(e.out + ": " + err);
      say(e.what + " (" + std::to_string(e.label_values.size()) + " labels)", e.out, out, cover);
      if (!e.conf.empty()) {
        if (svr_nifti_write(e.conf.c_str(), &P.tattr, cover.data(), err)) die(e.conf + ": " + err);
        say("--labelConfidence", e.conf, cover, cover);
      }
    }
    if (e.echo >= 0) std::copy(out.begin(), out.end(), echoes.begin() + (size_t)e.echo * nvv);         // what was (or would have been) written: the fit's input
  }
  if (timing && !n_scatter)                                               // (only a channel with --channelIterations: its own line gave the iterations' time)
    fprintf(stderr, "[timing] one SR scatter of rank 0's slices %.3f ms (host clock)\n", 1e3 * t_sr);
  else if (timing)
    fprintf(stderr, "[timing] %d channel / label scatters, %.3f ms each (upload, scatter%s; slowest rank, host clock); one SR scatter of rank 0's slices %.3f ms\n",
            n_scatter, 1e3 * t_scatter / std::max(1, n_scatter), R.nr > 1 ? ", all-reduce" : "", 1e3 * t_sr);
}

// --fitRate / --fitT / --fitAmplitude / --fitResidual / --fitCount: S(x) = A exp(-R x) over the echoes as they were (or would have been) written,
// voxel by voxel on rank 0's device (svr_monoexp_fit, csrc/svr_fit.inc).  The echoes are on disk: nothing from here on can reach them.
void fit_echoes(const Options &opt, const Problem &P, const Ranks &R, const std::vector<float> &echoes, bool timing) {
  const size_t nvv = (size_t)P.tattr.nx * P.tattr.ny * P.tattr.nz;
  std::vector<double> x;
  for (auto &e : P.extras) if (e.echo >= 0) x.push_back(e.x);
  const int K = (int)x.size();
  double x_abs = 0;
  for (double v : x) x_abs = std::max(x_abs, fabs(v));
  const double t_max = opt.fit_max_t > 0 ? opt.fit_max_t : 10.0 * x_abs;
  std::vector<float> rate(nvv), amplitude(nvv), rmse(nvv), count(nvv), t(nvv);
  const auto t0 = std::chrono::steady_clock::now();
  ENGR(R, 0, svr_monoexp_fit(R.ctxs[0], K, x.data(), echoes.data(), nvv, opt.fit_iterations, (float)opt.fit_floor, rate.data(), amplitude.data(), rmse.data(),
                             count.data()));
  const double t_fit = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  // T = 1 / R where R > 1 / Tmax, Tmax where a fitted voxel has a smaller (or negative) rate, 0 where nothing was fitted: an amplitude is the
  // exponential of something, so 0 only where the fit was refused
  std::vector<float> fitted_t;
  for (size_t i = 0; i < nvv; ++i) {
    if (!(amplitude[i] > 0.0f)) { t[i] = 0.0f; continue; }
    const double r = (double)rate[i];
    t[i] = (float)(r > 1.0 / t_max ? 1.0 / r : t_max);
    fitted_t.push_back(t[i]);
  }
  char err[256] = {0};
  const std::pair<const std::string *, const std::vector<float> *> files[5] = {
      {&opt.fit_rate, &rate}, {&opt.fit_t, &t}, {&opt.fit_amplitude, &amplitude}, {&opt.fit_residual, &rmse}, {&opt.fit_count, &count}};
  for (auto &f : files)
    if (!f.first->empty() && svr_nifti_write(f.first->c_str(), &P.tattr, f.second->data(), err)) die(*f.first + ": " + err);
  std::sort(fitted_t.begin(), fitted_t.end());
  const size_t m = fitted_t.size();
  if (m)
    fprintf(stderr, "--fit over %d echoes: %zu fitted voxels, median T %.9g (Tmax %.9g, %d Gauss-Newton iterations, floor %.9g)\n", K, m,
            m % 2 ? (double)fitted_t[m / 2] : 0.5 * ((double)fitted_t[m / 2 - 1] + (double)fitted_t[m / 2]), t_max, opt.fit_iterations, opt.fit_floor);
  else
    fprintf(stderr, "--fit over %d echoes: no fitted voxel\n", K);
  if (timing) fprintf(stderr, "[timing] mono-exponential fit of %d volumes of %zu voxels %.3f ms (upload, kernel, download; host clock)\n", K, nvv, 1e3 * t_fit);
}

// ---- the option loop and, in this order, every refusal that needs no file; the second images are declared on the way --------------
Options parse_options(int argc, char **argv, std::vector<ExtraSet> &extras) {
  Options p;
  Args a{argc, argv};
  while (a.next()) {
    if (a.is("-o", "--output")) p.output = a.one();
    else if (a.is("-m", "--mask")) p.mask_name = a.one();
    else if (a.is("-i", "--input")) a.multi(p.inputs);
    else if (a.is("-t", "--transformation")) a.multi(p.tspecs);
    else if (a.is("--thickness")) a.doubles(p.thickness);
    else if (a.is("--iterations")) p.iterations = a.one_int();
    else if (a.is("--sigma")) p.sigma = a.one_double();                   // bias field stdev (main.cc:172); used with --enableBiasCorrection
    else if (a.is("--resolution")) p.resolution = a.one_double();
    else if (a.is("--multires")) p.levels = a.one_int();
    else if (a.is("--average")) p.average = a.one_double();
    else if (a.is("--delta")) p.delta = a.one_double();
    else if (a.is("--lambda")) p.lambda = a.one_double();
    else if (a.is("--lastIterLambda")) p.last_lambda = a.one_double();
    else if (a.is("--smooth_mask")) p.smooth_mask = a.one_double();
    else if (a.is("--no_intensity_matching")) p.no_matching = !a.opt_bool(false);   // the value lands in `intensity_matching` (main.cc:186): 0 switches it off
    else if (a.is("--num_stacks_tuner")) p.num_stacks_tuner = a.one_int();
    else if (a.is("--low_intensity_cutoff")) p.low_intensity_cutoff = a.one_double();   // passed to SuperresolutionGPU, which does not use it (as in the reference)
    else if (a.is("--global_bias_correction")) p.global_bias = a.opt_bool(true);
    else if (a.is("--enableBiasCorrection")) p.enable_bias = true;        // not a reference option: the reference hard-wires disableBiasCorr (main.cc:121,202)
    else if (a.is("--log_prefix", "--patchSize") || a.is("--patchStride")) (void)a.one();   // no log files; patch modes are off
    else if (a.is("--no_log")) (void)a.opt_bool(true);
    else if (a.is("--force_exclude")) a.ints(p.force_excluded);
    else if (a.is("--rec_iterations_first")) p.rec_first = a.one_int();
    else if (a.is("--rec_iterations_last")) p.rec_last = a.one_int();
    else if (a.is("--useGPUReg")) p.use_gpu_reg = true;
    else if (a.is("--useNMI")) p.use_nmi = true;                          // main.cc:210 parses it and never calls setUseNMI(): here it takes effect
    else if (a.is("--useLNCC")) p.use_lncc = true;                        // not reference options: a local metric for the IRTK registration
    else if (a.is("--lnccRadius")) p.lncc_radius = a.one_int();
    else if (a.is("--useAutoTemplate")) p.auto_template = true;           // main.cc:199, 565-591 (there: HAVE_CULA builds only)
    else if (a.is("--autoTemplateCentral")) p.auto_template = p.auto_central = true;   // the middle third of the slices instead of the first
    else if (a.is("-p", "--packages")) a.ints(p.packages);
    else if (a.is("--no_registration")) p.no_registration = true;
    else if (a.is("--tfolder")) p.tfolder = a.one();
    else if (a.is("--sfolder")) p.sfolder = a.one();
    else if (a.is("--coeffTable")) p.coeff_table = 1;                     // not a reference option: keep the PSF taps in HBM (CoeffInit on the GPU path); the default since round 6
    else if (a.is("--noCoeffTable")) p.coeff_table = 0;                   // ... every tap evaluated in every pass, like the reference's GPU kernels: same volume, bit for bit
    else if (a.is("--debug")) p.debug = a.opt_bool(true);
    else if (a.is("--saveSliceTransformations")) p.save_slice_transformations = true;   // main.cc:211, 1213-1217
    else if (a.is("--dumpProblem")) p.dump_name = a.one();                // test hooks: what the engine is about to receive [--dryRun: stop there]
    else if (a.is("--dryRun")) p.dry_run = true;
    else if (a.is("--sliceReport")) p.report_name = a.one();              // not reference options: the reference's main() never calls SlicesInfo / SimulateStacks
    else if (a.is("--simulatedStacks")) p.sim_prefix = a.one();
    else if (a.is("--structural")) p.structural = true;                   // not reference options: the reference leaves slices out by intensity residuals only
    else if (a.is("--structuralRadius")) p.st_radius = a.one_int();
    else if (a.is("--structuralK")) p.st_k = a.one_double();
    else if (a.is("--structuralMinDrop")) p.st_min_drop = a.one_double();
    else if (a.is("--structuralMinPixels")) p.st_min_pixels = a.one_int();
    else if (a.is("--referenceVolume")) p.reference_name = a.one();       // main.cc:207, 253-258: read there and (outside the T1 experiment) never used
    else if (a.is("--channelStacks")) { p.have_channel_opt = true; a.multi(p.channel_names); }   // not reference options: a second image per stack through the run's motion and weights
    else if (a.is("--channelOutput")) p.channel_out = a.one();
    else if (a.is("--channelIterations")) { p.have_channel_sr_opt = true; p.channel_iterations = a.one_int(); }   // not reference options: SR iterations on the channel
    else if (a.is("--channelDelta")) { p.have_channel_sr_opt = true; p.channel_delta = a.one_double(); if (!(p.channel_delta > 0) || !std::isfinite(p.channel_delta)) die("--channelDelta must be positive"); }
    else if (a.is("--channelLambda")) { p.have_channel_sr_opt = true; p.channel_lambda = a.one_double(); if (!(p.channel_lambda > 0) || !std::isfinite(p.channel_lambda)) die("--channelLambda must be positive"); }
    else if (a.is("--channelGuide")) p.channel_guide = true;              // not reference options: the channel's update guided by the -o volume's edges
    else if (a.is("--channelGuideDelta")) { p.have_channel_guide_opt = true; p.channel_guide_delta = a.one_double(); if (!(p.channel_guide_delta > 0) || !std::isfinite(p.channel_guide_delta)) die("--channelGuideDelta must be positive"); }
    else if (a.is("--channelGuideOnly")) { p.have_channel_guide_opt = true; p.channel_guide_only = true; }
    else if (a.is("--echoStacks")) {                                      // not reference options: K echoes through the run's motion and weights, and their fit
      std::vector<std::string> tok;
      a.multi(tok);
      if (tok.empty()) die("--echoStacks needs the echo's abscissa (echo time, b-value) and then a file or `none` per -i stack");
      p.echo_x.push_back(tok[0]);
      p.echo_names.emplace_back(tok.begin() + 1, tok.end());
    }
    else if (a.is("--echoOutput")) { p.have_echo_dep_opt = true; p.echo_out = a.one(); }
    else if (a.is("--echoIterations")) { p.have_echo_dep_opt = true; p.echo_iterations = a.one_int(); }
    else if (a.is("--echoGuide")) { p.have_echo_dep_opt = true; p.echo_guide = true; }
    else if (a.is("--fitRate")) { p.have_echo_dep_opt = true; p.fit_rate = a.one(); }
    else if (a.is("--fitT")) { p.have_echo_dep_opt = true; p.fit_t = a.one(); }
    else if (a.is("--fitAmplitude")) { p.have_echo_dep_opt = true; p.fit_amplitude = a.one(); }
    else if (a.is("--fitResidual")) { p.have_echo_dep_opt = true; p.fit_residual = a.one(); }
    else if (a.is("--fitCount")) { p.have_echo_dep_opt = true; p.fit_count = a.one(); }
    else if (a.is("--fitIterations")) { p.have_echo_dep_opt = true; p.fit_iterations = a.one_int(); }
    else if (a.is("--fitFloor")) { p.have_echo_dep_opt = true; p.fit_floor = a.one_double(); }
    else if (a.is("--fitMaxT")) { p.have_echo_dep_opt = true; p.fit_max_t = a.one_double(); if (!(p.fit_max_t > 0) || !std::isfinite(p.fit_max_t)) die("--fitMaxT must be positive"); }
    else if (a.is("--labelStacks")) { p.have_label_opt = true; a.multi(p.label_names); }
    else if (a.is("--labelOutput")) p.label_out = a.one();
    else if (a.is("--labelConfidence")) p.label_conf = a.one();
    else if (a.is("--manualMask")) p.manual_name = a.one();               // main.cc:208; reconstruction.cc:1240-1250 transformManualMaskwithPSF
    else if (a.is("--dumpChannels")) p.channels_dump = a.one();           // test hook: the packed channel / label grids [--dryRun: stop there]
    else if (a.is("--useCPUReg", "--disableBiasCorrection") || a.is("--debug_gpu")) {}
    else if (a.is("-d", "--devices")) a.ints(p.devices);
    else if (a.is("-h", "--help")) { usage(); exit(0); }
    else die("option " + a.o + " is not supported by this build (see csrc/svr_cli.cpp)");
  }
  if (p.output.empty() || p.inputs.empty()) die("-o and -i are required (try --help)");
  if (p.dry_run && (!p.report_name.empty() || !p.sim_prefix.empty()))
    die("--dryRun stops before the reconstruction; --sliceReport / --simulatedStacks describe a finished one: drop one or the other");
  if (!p.sim_prefix.empty() && !p.sfolder.empty())
    die("--simulatedStacks puts every simulated slice back into the stack it was cut from; with --sfolder the slices come from files of "
        "their own and belong to no stack: use --sliceReport, or drop --sfolder");
  if (p.channel_iterations < 0) die("--channelIterations must not be negative (0 = the robust PSF-weighted average alone)");
  if (p.have_channel_sr_opt && !p.have_channel_opt)
    die("--channelIterations / --channelDelta / --channelLambda refine the channel of --channelStacks f_1 .. f_N --channelOutput <file>: give them");
  if (p.have_channel_sr_opt && !p.sfolder.empty())
    die("--channelIterations / --channelDelta / --channelLambda belong to --channelStacks, which cuts its files into slices with the stacks; with "
        "--sfolder the slices come from files of their own and belong to no stack: drop one or the other");
  if (p.have_channel_guide_opt && !p.channel_guide) die("--channelGuideDelta / --channelGuideOnly describe the guide of --channelGuide: give it");
  if (p.channel_guide && (!p.have_channel_opt || p.channel_iterations <= 0))
    die("--channelGuide guides the volume update of --channelIterations n (n > 0) on the channel of --channelStacks f_1 .. f_N --channelOutput <file>: "
        "give them");
  if (p.echo_x.empty() && p.have_echo_dep_opt)
    die("--echoOutput / --echoIterations / --echoGuide / --fit* belong to the echoes of --echoStacks <x> f_1 .. f_N, given once per echo: give them");
  if (p.echo_iterations < 0) die("--echoIterations must not be negative (0 = the robust PSF-weighted average of every echo alone)");
  if (p.fit_iterations < 0 || p.fit_iterations > 50) die("--fitIterations must be 0 .. 50 (0 = the weighted log-linear fit alone; negative or larger counts are refused)");
  if (!(p.fit_floor >= 0) || !std::isfinite(p.fit_floor)) die("--fitFloor must be finite and not negative");
  if (p.echo_guide && p.echo_iterations <= 0) die("--echoGuide guides the volume update of --echoIterations n (n > 0): give it");
  if (p.structural && !p.sfolder.empty())
    die("--structural compares every slice with the other slices of its stack; with --sfolder the slices come from files of their own and "
        "belong to no stack: drop one or the other");
  if (p.structural && (p.st_radius < 1 || p.st_radius > SVR_SSIM_MAX_RADIUS))
    die("--structuralRadius must be 1 .. " + std::to_string(SVR_SSIM_MAX_RADIUS) + " (the window is (2 radius + 1)^2 pixels)");
  if (p.structural && (!(p.st_k >= 0.0) || !(p.st_min_drop >= 0.0) || p.st_min_pixels < 0))
    die("--structuralK, --structuralMinDrop and --structuralMinPixels must not be negative");
  if (p.dry_run && !p.reference_name.empty()) die("--dryRun makes no engine context and cannot resample a volume: drop --referenceVolume");
  if (p.use_nmi && p.use_gpu_reg)
    die("--useNMI selects normalised mutual information for the IRTK registration; the reference's GPU registration (--useGPUReg) is "
        "cross-correlation only: use one or the other");
  if (p.use_lncc && p.use_nmi) die("--useLNCC and --useNMI each select the similarity of the IRTK registration: use one or the other");
  if (p.use_lncc && p.use_gpu_reg)
    die("--useLNCC selects the windowed cross correlation for the IRTK registration; the reference's GPU registration (--useGPUReg) is "
        "cross-correlation only: use one or the other");
  if (p.use_lncc && (p.lncc_radius < 1 || p.lncc_radius > 7)) die("--lnccRadius must be 1 .. 7 (the window is (2 radius + 1)^2 pixels)");
  if (p.num_stacks_tuner > 0 && (size_t)p.num_stacks_tuner < p.inputs.size()) {      // main.cc:406-419: only the first stacks are used
    p.inputs.resize(p.num_stacks_tuner);
    if (p.tspecs.size() > (size_t)p.num_stacks_tuner) p.tspecs.resize(p.num_stacks_tuner);
    if (p.thickness.size() > (size_t)p.num_stacks_tuner) p.thickness.resize(p.num_stacks_tuner);
    if (p.packages.size() > (size_t)p.num_stacks_tuner) p.packages.resize(p.num_stacks_tuner);
  }
  const size_t n = p.inputs.size();
  declare_extras(p, extras);
  if (p.tspecs.empty()) p.tspecs.assign(n, "id");
  if (p.tspecs.size() != n) die("one transformation per stack expected");
  if (!p.packages.empty() && p.packages.size() != n) die("one package count per stack expected");
  p.tmpl = n;
  for (size_t k = 0; k < n; ++k) if (p.tspecs[k] == "id") { p.tmpl = k; break; }
  if (p.tmpl == n) die("Please identify the template by assigning id transformation.");          // main.cc:452-457
  return p;
}

// ---- set-up (main.cc:386-815) ------------------------------------------------------------------------
void read_inputs(const Options &opt, Problem &P) {
  const size_t n = opt.inputs.size();
  P.tmpl = opt.tmpl;
  P.force_excluded = opt.force_excluded;
  P.stacks.resize(n);
  parallel_for((int)n, [&](int k) { P.stacks[k] = read_image(opt.inputs[k]); });                 // gunzip is serial per file
  for (size_t k = 0; k < n; ++k) P.ts.push_back(load_transformation(opt.tspecs[k]));
}

// the thicknesses (main.cc:422-431) and the mask as given or made up (main.cc:458-480)
void make_mask(const Options &opt, Problem &P) {
  P.thickness = opt.thickness;
  if (P.thickness.empty()) for (auto &s : P.stacks) P.thickness.push_back(2.0 * s.a.dz);
  if (P.thickness.size() != P.stacks.size()) die("one thickness per stack expected");
  P.have_mask = !opt.mask_name.empty() || opt.sfolder.empty();            // main.cc:461: no mask is made up when --sfolder is given
  if (!opt.mask_name.empty()) {
    P.mask_img = read_image(opt.mask_name);
  } else if (P.have_mask) {
    // no mask given: CreateMask(stacks[templateNumber]) binarises the template stack (> 0), in case it was padded; the
    // normal mask path follows (main.cc:458-480, RG.cc:736-748)
    P.mask_img = P.stacks[P.tmpl];
    for (auto &v : P.mask_img.d) v = v > 0.0 ? 1.0 : 0.0;
  }
}

// --useAutoTemplate, main.cc:565-591: the stack with the smallest motion score becomes the template
void select_template_by_motion(const Options &opt, Problem &P, const std::function<svr_ctx *()> &need_ctx) {
  if (!P.have_mask) die("--useAutoTemplate crops every stack to the mask before it scores it: give -m (the reference skips the selection without a mask)");
  if (opt.dry_run) die("--dryRun makes no engine context and cannot score the stacks' motion: drop --useAutoTemplate / --autoTemplateCentral");
  svr_ctx *ctx = need_ctx();
  double best = 1e300;                                                                           // tmp_motionestimate, main.cc:271
  size_t best_k = P.tmpl;
  for (size_t k = 0; k < P.stacks.size(); ++k) {
    // on a copy: TransformMask + CropImage with the -t transformations as given (the stack registrations come later)
    const Image c = crop_image(P.stacks[k], transform_nn(P.mask_img, P.stacks[k].a, P.ts[k], 0.0));
    const int m = c.a.nx * c.a.ny, nw = (int)(c.a.nz / 3.0), first = opt.auto_central ? (c.a.nz - nw) / 2 : 0;
    if (nw < 1) die("--useAutoTemplate: stack " + std::to_string(k) + " has " + std::to_string(c.a.nz) + " slices inside the mask; a third of them is none");
    const auto mm = std::minmax_element(c.d.begin(), c.d.end());                                 // the whole cropped stack's, not the window's
    const double lo = *mm.first, hi = *mm.second;
    if (!(hi > lo)) die("--useAutoTemplate: stack " + std::to_string(k) + " is constant inside the mask");
    std::vector<float> win((size_t)m * nw);
    for (size_t i = 0; i < win.size(); ++i) win[i] = (float)((c.d[(size_t)first * m + i] - lo) / (hi - lo));
    double et = 0, score = 0;
    int r_min = 0;
    if (svr_stack_motion(ctx, win.data(), m, nw, nullptr, &et, &r_min, &score))
      die("--useAutoTemplate: stack " + std::to_string(k) + ": " + svr_last_error(ctx));
    fprintf(stderr, "stack %zu: motion score %.9g (r_min %d, et %.9g)\n", k, score, r_min, et);
    if (score < best) { best = score; best_k = k; }                                              // strictly smaller: the first one on ties
  }
  P.tmpl = best_k;
  fprintf(stderr, "Determined stack %zu as template.\n", P.tmpl);
}

// crop the template stack to the mask, CreateTemplate, SetMask
void make_template(const Options &opt, Problem &P) {
  if (P.have_mask) {
    const Image m = transform_nn(P.mask_img, P.stacks[P.tmpl].a, P.ts[P.tmpl], 0.0);             // TransformMask RG.cc:805-821
    P.stacks[P.tmpl] = crop_image(P.stacks[P.tmpl], m);
    crop_extras_with(P.extras, P.tmpl, m);
  }
  P.resolution = opt.resolution;
  const svr_image_attr t = create_template(P.stacks[P.tmpl].a, P.resolution);
  memcpy(&P.tattr, &t, sizeof(t));                       // (--dumpProblem writes the struct as it lies in memory, padding included)
  P.vol_mask = set_mask(P.tattr, P.have_mask ? &P.mask_img : nullptr, opt.smooth_mask);
}

// StackRegistrations before and after the other stacks are cropped to the volume mask (main.cc:657-713)
void crop_and_register_stacks(const Options &opt, Problem &P, const std::function<svr_ctx *()> &need_ctx) {
  const size_t n = P.stacks.size();
  auto register_stacks = [&]() {
    if (opt.no_registration || n < 2 || !opt.sfolder.empty()) return;                            // main.cc:658, 708
    if (opt.dry_run) die("--dryRun makes no engine context and cannot register the stacks: add --no_registration (or --sfolder)");
    stack_registrations(need_ctx(), P.stacks, P.ts, P.tmpl, P.have_mask ? &P.vol_mask : nullptr, 0);
  };
  register_stacks();                                                                             // main.cc:657-662
  for (size_t k = 0; k < n; ++k) {                                                               // main.cc:676-700
    if (k == P.tmpl) continue;
    const Image m = transform_nn(P.vol_mask, P.stacks[k].a, P.ts[k], 0.0);
    P.stacks[k] = crop_image(P.stacks[k], m);
    crop_extras_with(P.extras, k, m);
  }
  register_stacks();                                                                             // main.cc:707-713
}

// CreateSlicesAndTransformations RG.cc:1835-1880 + MaskSlices RG.cc:1940-1988 + the packing of SyncGPU RG.cc:249-328
void pack_slices(const Options &opt, Problem &P) {
  struct SliceSrc { Image r; M4 t; int stack; };
  std::vector<SliceSrc> srcs;
  for (size_t k = 0; k < P.stacks.size(); ++k)
    for (int j = 0; j < P.stacks[k].a.nz; ++j) {
      SliceSrc q{get_region(P.stacks[k], 0, 0, j, P.stacks[k].a.nx, P.stacks[k].a.ny, j + 1), P.ts[k], (int)k};
      q.r.a.dz = P.thickness[k];
      srcs.push_back(std::move(q));
    }
  if (!opt.sfolder.empty()) {
    // replaceSlices, RG.cc:4767-4822: every file of the folder is one slice that is already in place -- identity
    // transformation, stack 0, 4 mm thickness, "equally many as loaded from stacks".  The reference takes the files in
    // directory_iterator order (unspecified); here they are taken in the order of their names.
    const std::vector<std::string> files = list_directory(opt.sfolder);
    if (files.size() != srcs.size())
      die("--sfolder: " + std::to_string(files.size()) + " files, but the stacks hold " + std::to_string(srcs.size()) + " slices");
    for (size_t i = 0; i < files.size(); ++i) {
      SliceSrc q{read_image(opt.sfolder + "/" + files[i]), ident(), 0};
      if (q.r.a.nz != 1) die("--sfolder: " + files[i] + " is not a single slice");
      q.r.a.dz = 4.0;
      srcs[i] = std::move(q);
    }
  }
  const int ns = P.ns = (int)srcs.size();
  for (auto &q : srcs) { P.mx = std::max(P.mx, q.r.a.nx); P.my = std::max(P.my, q.r.a.ny); }
  const int mx = P.mx, my = P.my;
  P.grid.assign((size_t)ns * mx * my, -1.0f);
  for (std::vector<float> *v : {&P.i2w, &P.w2i, &P.st, &P.sti}) v->resize(16 * (size_t)ns);
  P.dims.resize(3 * (size_t)ns);
  P.sizes_x.resize(ns); P.sizes_y.resize(ns); P.stack_index.resize(ns);
  P.sattr.resize(ns);
  P.T.resize(16 * (size_t)ns);
  const Image &vol_mask = P.vol_mask;
  const M4 mw2i = world_to_image(vol_mask.a);
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
        P.grid[((size_t)sl * my + y) * mx + x] = (float)v;
        if (v > 0) { P.vmin = std::min(P.vmin, (double)(float)v); P.vmax = std::max(P.vmax, (double)(float)v); }
      }
    to_f16(si2w, &P.i2w[16 * (size_t)sl]); to_f16(world_to_image(r.a), &P.w2i[16 * (size_t)sl]);
    to_f16(tk, &P.st[16 * (size_t)sl]); to_f16(inverse_rigid_or_affine(tk), &P.sti[16 * (size_t)sl]);
    for (int q = 0; q < 16; ++q) P.T[16 * (size_t)sl + q] = tk.m[q];
    P.dims[3 * (size_t)sl] = (float)r.a.dx; P.dims[3 * (size_t)sl + 1] = (float)r.a.dy; P.dims[3 * (size_t)sl + 2] = (float)r.a.dz;
    P.sizes_x[sl] = r.a.nx; P.sizes_y[sl] = r.a.ny; P.stack_index[sl] = srcs[sl].stack; P.sattr[sl] = r.a;
  }
}

// ---- engines -------------------------------------------------------------------------------------------
// What the engine is about to receive, for the CPU tests (tests/test_prep_oracle.py compares it with the oracle's restatement
// of CreateTemplate / SetMask / TransformMask / CropImage / MatchStackIntensities / MaskSlices): header, the template's
// attributes, the volume mask, the cropped stacks' attributes, the slice grid, the slices' transformations, the factors
void dump_problem(const std::string &name, const Problem &P) {
  FILE *f = fopen(name.c_str(), "wb");
  if (!f) die("cannot write " + name);
  const int hdr[8] = {P.ns, P.mx, P.my, (int)P.stacks.size(), P.tattr.nx, P.tattr.ny, P.tattr.nz, 2};
  fwrite(hdr, sizeof(int), 8, f);
  fwrite(&P.tattr, sizeof(svr_image_attr), 1, f);
  fwrite(P.vol_mask.d.data(), sizeof(double), P.vol_mask.d.size(), f);
  for (const Image &s : P.stacks) fwrite(&s.a, sizeof(svr_image_attr), 1, f);
  fwrite(P.grid.data(), sizeof(float), P.grid.size(), f);
  fwrite(P.T.data(), sizeof(double), P.T.size(), f);
  fwrite(P.factors.data(), sizeof(float), P.factors.size(), f);
  fwrite(P.sizes_x.data(), sizeof(int), P.sizes_x.size(), f);
  fwrite(P.sizes_y.data(), sizeof(int), P.sizes_y.size(), f);
  fclose(f);
}

// Ranks: one engine context per device of -d (main.cc:191).  Rank r takes the r-th of nr work-balanced segments of EVERY stack
// (svr_shard.h spatial_order: a rank's slices are neighbours in space), work = estimated PSF work = active pixels x (9.4 + live
// planes of the 16) x (1 + 0.2 n_x^2), see sharding.py slice_cost_weights.  (reconstruction_cuda2.cu:1413-1457 shards by slice count
// in slice order and drops the remainder.)  From here on every per-slice array is in the SHARDED numbering -- rank after rank --
// and `order[k]` is slice k's index in the reference's order: files named by slice number (--tfolder, --debug), --force_exclude
// and the package registration, which works on whole stacks, go through it.
void shard_slices(const Options &opt, Problem &P, Ranks &R) {
  const int ns = P.ns, nr = (int)std::max<size_t>(1, opt.devices.size());
  const size_t slice = (size_t)P.mx * P.my;
  R.init(nr, ns);
  if (nr == 1) return;
  if (ns < nr) die("fewer slices than devices");
  std::vector<double> work(ns, 0.0);
  const M4 rw = world_to_image(P.tattr);
  for (int s = 0; s < ns; ++s) {
    long c = 0;
    for (size_t i = 0; i < slice; ++i) c += P.grid[(size_t)s * slice + i] != -1.0f;
    double nv[3], len;
    normal_in_volume_axes(&P.i2w[16 * (size_t)s], &P.T[16 * (size_t)s], rw, nv, len);
    len = std::max(sqrt(len), 1e-12);
    const double ax = fabs(nv[0]) / len, ay = fabs(nv[1]) / len, az = fabs(nv[2]) / len;
    const double ne = std::max(ay, az), no = std::min(ay, az), sigma = P.dims[3 * (size_t)s + 2] / 2.3548 / P.tattr.dx;
    const double live = std::min(16.0, 2.0 * (5.1 * sigma + 8.0 * (ax + no)) / std::max(ne, 1e-3) + 1.0);
    work[s] = (double)c * (9.4 + live) * (1.0 + 0.2 * ax * ax);
  }
  svr::spatial_order(work, P.stack_index, nr, R.order, R.rlo, R.rhi);
  for (int r = 0; r < nr; ++r) if (R.rhi[r] <= R.rlo[r]) die("a device would get no slice: fewer devices, please");
  for (int k = 0; k < ns; ++k) R.inv_order[R.order[k]] = k;
  svr::permute_rows(P.grid, slice, R.order);
  svr::permute_rows(P.i2w, 16, R.order); svr::permute_rows(P.w2i, 16, R.order); svr::permute_rows(P.st, 16, R.order); svr::permute_rows(P.sti, 16, R.order);
  svr::permute_rows(P.dims, 3, R.order); svr::permute_rows(P.sizes_x, 1, R.order); svr::permute_rows(P.sizes_y, 1, R.order);
  svr::permute_rows(P.stack_index, 1, R.order); svr::permute_rows(P.sattr, 1, R.order); svr::permute_rows(P.T, 16, R.order);
  for (auto &e : P.extras) { svr::permute_rows(e.grid, slice, R.order); svr::permute_rows(e.unit_on, 1, R.order); }
  for (int &s : P.force_excluded) if (s >= 0 && s < ns) s = R.inv_order[s];
}

// SyncGPU + generatePSFVolume + UpdateGPUTranformationMatrices (RG.cc:249-401, 1496-1610), per rank, and every rank's host object
void setup_engines(const Options &opt, Problem &P, const Ranks &R, std::vector<svrh_recon *> &hosts) {
  const svr_image_attr &tattr = P.tattr;
  const int mx = P.mx, my = P.my;
  to_f16(image_to_world(tattr), P.ri2w); to_f16(world_to_image(tattr), P.rw2i);
  const uint32_t vsize[3] = {(uint32_t)tattr.nx, (uint32_t)tattr.ny, (uint32_t)tattr.nz};
  const float vdim[3] = {(float)tattr.dx, (float)tattr.dy, (float)tattr.dz};
  const std::vector<float> maskf(P.vol_mask.d.begin(), P.vol_mask.d.end());
  float pi2w[16], pw2i[16];
  psf_volume_matrices(tattr, pi2w, pw2i);
  hosts.assign(R.nr, nullptr);
  R.par([&](int r) {
    svr_ctx *c = R.ctxs[r];
    const int nl = R.rhi[r] - R.rlo[r];
    const size_t o = (size_t)R.rlo[r];
    if (opt.coeff_table >= 0) ENGR(R, r, svr_set_option(c, "coeff_table", opt.coeff_table));
    ENGR(R, r, svr_init_reconstruction_volume(c, vsize, vdim, nullptr, 12.0f));
    ENGR(R, r, svr_set_mask(c, vsize, vdim, maskf.data(), 12.0f));
    const uint32_t ssize[3] = {(uint32_t)mx, (uint32_t)my, (uint32_t)nl};
    ENGR(R, r, svr_init_storage_volumes(c, ssize, &P.dims[3 * o]));
    ENGR(R, r, svr_fill_slices(c, P.grid.data() + o * mx * my, P.sizes_x.data() + o, P.sizes_y.data() + o));
    ENGR(R, r, svr_set_slice_dims(c, P.dims.data() + 3 * o, 2.0f));
    const uint32_t psize[3] = {128, 128, 128};
    ENGR(R, r, svr_generate_psf_volume(c, nullptr, psize, &P.dims[3 * o], vdim, pi2w, pw2i, 2.0f));
    R.set_matrices(r, P.st, P.sti, P.i2w, P.w2i, P.ri2w, P.rw2i);
    hosts[r] = svrh_create(c, P.ns, R.rlo[r], R.rhi[r], R.group ? svr_group_join(R.group, r, c) : nullptr);
    if (!hosts[r]) die("svrh_create failed");
    svrh_set_intensity_range(hosts[r], P.vmin, P.vmax);                  // InitializeEMGPU RG.cc:2937-2951
    svrh_set_intensity_matching(hosts[r], opt.no_matching ? 0 : 1);     // main.cc:1018, 1062
    // SetSigma / GlobalBiasCorrectionOn / SetLowIntensityCutoff (main.cc:451, 764-778); the steps themselves are gated on the option
    // sigma > 0 (main.cc:1025,1035,1069), so sigma <= 0 leaves the member at 20 and runs no bias step
    HOSTR(r, svrh_set_bias_correction(hosts[r], opt.enable_bias && opt.sigma > 0, opt.sigma > 0 ? opt.sigma : 20.0));
    HOSTR(r, svrh_set_bias_options(hosts[r], opt.global_bias ? 1 : 0, opt.low_intensity_cutoff));
    if (R.nr > 1 && svrh_set_unit_order(hosts[r], R.order.data())) die("svrh_set_unit_order failed");
    if (!P.force_excluded.empty()) svrh_set_force_excluded(hosts[r], P.force_excluded.data(), (int)P.force_excluded.size());
    if (opt.structural) HOSTR(r, svrh_set_structural(hosts[r], 1, opt.st_radius, opt.st_k, opt.st_min_drop, opt.st_min_pixels, P.stack_index.data()));
    if (opt.use_gpu_reg) HOSTR(r, svrh_prepare_registration_slices(hosts[r], P.grid.data() + o * mx * my, mx, my, P.sattr.data() + o, P.resolution));
  });
  R.describe(opt.devices, "");
}

void update_matrices_from_T(Problem &P, const Ranks &R) { R.update_matrices(P.T, P.st, P.sti, P.i2w, P.w2i, P.ri2w, P.rw2i); }

void read_tfolder(const Options &opt, Problem &P, const Ranks &R) {     // ReadTransformation, RG.cc:4733-4765
  for (int s = 0; s < P.ns; ++s) {
    double p6[6];
    char e[256] = {0};
    const std::string path = opt.tfolder + "/transformation" + std::to_string(R.order[s]) + ".dof";   // (files are named in the reference's slice order)
    if (svr_dof_read(path.c_str(), p6, &P.T[16 * (size_t)s], e)) die(path + ": " + e);
  }
  update_matrices_from_T(P, R);
}

// The seed on its own grid -> the reconstruction grid, on rank 0's device: once to learn its mean inside the mask, once more to
// scale and install it; the other ranks get the result.  -1 is this program's own background (MaskVolume) and must not bleed in.
void seed_reference_volume(const Options &opt, const Problem &P, const Ranks &R) {
  const svr_image_attr &tattr = P.tattr;
  const int nr = R.nr;
  svr_ctx *ctx = R.ctxs[0];
  svr_image_attr ra;
  float *rdata = nullptr;
  int rnt = 1;
  char e[256] = {0};
  if (svr_nifti_read(opt.reference_name.c_str(), &ra, &rnt, &rdata, e)) die(opt.reference_name + ": " + e);   // (4D: the first volume comes first)
  const M4 m = mul(world_to_image(ra), image_to_world(tattr));
  const uint32_t rsize[3] = {(uint32_t)ra.nx, (uint32_t)ra.ny, (uint32_t)ra.nz}, vsize[3] = {(uint32_t)tattr.nx, (uint32_t)tattr.ny, (uint32_t)tattr.nz};
  double rs[5];
  ENGR(R, 0, svr_resample_to_reconstruction(ctx, rsize, rdata, m.m, -1.0f, 0, 1.0f, nullptr, rs));
  if (rs[0] == 0) die("--referenceVolume does not overlap the mask");
  const double rmean = rs[1] / rs[0];
  // the stacks were matched to --average, and the default registration casts the volume to short: a seed in [0, 1] would have two levels
  double rscale = 1.0;
  if (!opt.no_matching) {
    if (!(rmean > 0)) die("--referenceVolume: the mean inside the mask is " + std::to_string(rmean) + ", it cannot be scaled to --average");
    rscale = opt.average / rmean;
  }
  std::vector<float> seed(nr > 1 ? (size_t)tattr.nx * tattr.ny * tattr.nz : 0);
  ENGR(R, 0, svr_resample_to_reconstruction(ctx, rsize, rdata, m.m, -1.0f, SVR_RESAMPLE_INSTALL | (opt.no_matching ? 0 : SVR_RESAMPLE_SCALE), (float)rscale,
                                            nr > 1 ? seed.data() : nullptr, rs));
  svr_free(rdata);
  for (int r = 1; r < nr; ++r) ENGR(R, r, svr_update_reconstructed(R.ctxs[r], vsize, seed.data()));
  fprintf(stderr, "reference volume: n=%.0f mean=%.9g min=%.9g max=%.9g scale=%.9g\n", rs[0], rmean, rs[3], rs[4], rscale);
}

// the similarity of the IRTK schedule's slice- and package-to-volume registrations, and what the registration lines call it
int reg_similarity(const Options &opt) { return opt.use_nmi ? SVRH_SIM_NMI : opt.use_lncc ? SVRH_SIM_LNCC | (opt.lncc_radius << 8) : SVRH_SIM_CC; }
std::string reg_metric(const Options &opt) { return opt.use_lncc ? " (LNCC, radius " + std::to_string(opt.lncc_radius) + ")" : ""; }

// ---- registration-reconstruction loop (main.cc:816-1237) ---------------------------------------------
// packages first (main.cc:832-864): plain, even/odd, even/odd halves; from iteration 4 on also the slices
void register_packages(const Options &opt, Problem &P, const Ranks &R, int it) {
  const size_t n = P.stacks.size();
  std::vector<svr_image_attr> at(n);
  std::vector<const double *> ptr(n);
  for (size_t k = 0; k < n; ++k) { at[k] = P.stacks[k].a; ptr[k] = P.stacks[k].d.data(); }
  std::vector<float> vol((size_t)P.tattr.nx * P.tattr.ny * P.tattr.nz);
  ENGR(R, 0, svr_sync_cpu(R.ctxs[0], vol.data()));
  long evals = 0;
  char e[256] = {0};
  svr::unpermute_rows(P.T, 16, R.order);                                 // (packages are sub-stacks: one transformation per slice, stack after stack)
  if (svrh_package_to_volume_ex(R.ctxs[0], nullptr, nullptr, reg_similarity(opt), (int)n, at.data(), ptr.data(), opt.packages.data(),
                                it >= 2, it >= 3, it >= 4 ? it - 2 : 1, P.T.data(), &P.tattr, vol.data(), &evals, e))
    die(std::string("package-to-volume registration: ") + e);
  svr::permute_rows(P.T, 16, R.order);
  fprintf(stderr, "package-to-volume registration%s: %ld similarity evaluations\n", reg_metric(opt).c_str(), evals);
}

void register_slices(const Options &opt, Problem &P, const Ranks &R, const std::vector<svrh_recon *> &hosts) {   // main.cc:829-880
  if (opt.use_gpu_reg) {                                                  // every rank registers its own slices
    R.par([&](int r) { HOSTR(r, svrh_slice_to_volume_registration_gpu(hosts[r], P.T.data() + 16 * (size_t)R.rlo[r])); });
  } else {                                                                // SliceToVolumeRegistration, RG.cc:2291-2303
    std::vector<float> vol((size_t)P.tattr.nx * P.tattr.ny * P.tattr.nz);
    ENGR(R, 0, svr_sync_cpu(R.ctxs[0], vol.data()));                      // _reconstructed after SyncCPU, main.cc:1189
    long evals = 0;
    char e[256] = {0};
    if (svrh_slice_to_volume_registration_ex(R.ctxs[0], nullptr, nullptr, reg_similarity(opt), P.ns, P.grid.data(), P.mx, P.my,
                                             P.sattr.data(), P.T.data(), &P.tattr, vol.data(), 0, &evals, e))
      die(std::string("slice-to-volume registration: ") + e);
    fprintf(stderr, "slice-to-volume registration%s: %ld similarity evaluations\n", reg_metric(opt).c_str(), evals);
  }
  update_matrices_from_T(P, R);
}

void set_smoothing_for_iteration(const Options &opt, const std::vector<svrh_recon *> &hosts, int it) {   // main.cc:884-896
  for (svrh_recon *h : hosts) {
    if (it == opt.iterations - 1) {
      svrh_set_smoothing_parameters(h, opt.delta, opt.last_lambda);
    } else {
      double l = opt.lambda;
      for (int i = 0; i < opt.levels; ++i) {
        if (it == opt.iterations * (opt.levels - i - 1) / opt.levels) svrh_set_smoothing_parameters(h, opt.delta, l);
        l *= 2;
      }
    }
  }
}

// --structural: what this iteration's evaluation found, in force during the next one
void structural_line(const Problem &P, const Ranks &R, const std::vector<svrh_recon *> &hosts, int it) {
  const size_t n = P.stacks.size();
  std::vector<double> q(P.ns);
  std::vector<unsigned char> pend(P.ns);
  HOSTR(0, svrh_get_structural(hosts[0], q.data(), nullptr, nullptr, pend.data()));
  std::vector<int> judged(n, 0), left_out(n, 0), named;
  for (int i = 0; i < P.ns; ++i) {                                        // slice i of the reference's order
    const int s = R.inv_order[i];
    if (q[s] == q[s]) ++judged[P.stack_index[s]];
    if (pend[s]) { ++left_out[P.stack_index[s]]; named.push_back(i); }
  }
  fprintf(stderr, "structural, iteration %d:", it);
  for (size_t k = 0; k < n; ++k) fprintf(stderr, " stack %zu judged %d excluded %d%s", k, judged[k], left_out[k], k + 1 < n ? "," : ";");
  fprintf(stderr, " excluded slices:");
  for (int i : named) fprintf(stderr, " %d", i);
  fprintf(stderr, "%s\n", named.empty() ? " none" : "");
}

// SaveSlices + SaveTransformations after every iteration (main.cc:1213-1217; RG.cc:4884-4892, 4903-4919), into the working
// directory like the reference: slice<i>.nii.gz (the masked slice), croppedSliceTransformation<i>.dof (the slice's transformation)
// and croppedSliceToVolumeTransformation<i>.dof (reconstructed W2I x transformation x slice I2W squeezed into a rigid
// transformation by PutMatrix, as the reference does) -- <i> = the slice's index in the reference's order
void save_slice_transformations(const Problem &P, const Ranks &R) {
  const M4 rw2i = world_to_image(P.tattr);
  for (int s = 0; s < P.ns; ++s) {
    const int i = R.order[s];
    const svr_image_attr &a = P.sattr[s];
    std::vector<float> img((size_t)a.nx * a.ny);
    for (int y = 0; y < a.ny; ++y) memcpy(&img[(size_t)y * a.nx], &P.grid[((size_t)s * P.my + y) * P.mx], a.nx * sizeof(float));
    char e[256] = {0};
    if (svr_nifti_write(("slice" + std::to_string(i) + ".nii.gz").c_str(), &a, img.data(), e)) die(std::string("slice file: ") + e);
    M4 t;
    for (int q = 0; q < 16; ++q) t.m[q] = P.T[16 * (size_t)s + q];
    double p6[6];
    svrh_irtk_rigid_parameters(t.m, p6, nullptr);
    if (svr_dof_write(("croppedSliceTransformation" + std::to_string(i) + ".dof").c_str(), p6, e)) die(std::string("dof file: ") + e);
    const M4 c = mul(rw2i, mul(t, image_to_world(a)));
    svrh_irtk_rigid_parameters(c.m, p6, nullptr);
    if (svr_dof_write(("croppedSliceToVolumeTransformation" + std::to_string(i) + ".dof").c_str(), p6, e)) die(std::string("dof file: ") + e);
  }
}

void run_iterations(const Options &opt, Problem &P, const Ranks &R, const std::vector<svrh_recon *> &hosts, StageClock &clk) {
  const int iterations = opt.iterations, levels = opt.levels;
  for (int it = 0; it < iterations; ++it) {
    bool slice_reg = (it > 0 || !opt.reference_name.empty()) && !opt.no_registration;             // main.cc:826
    if (slice_reg && !opt.packages.empty() && it <= iterations * (levels - 1) / levels && it < iterations - 1) {
      register_packages(opt, P, R, it);
      slice_reg = it >= 4;
      if (!slice_reg) update_matrices_from_T(P, R);
    }
    if (slice_reg) register_slices(opt, P, R, hosts);
    set_smoothing_for_iteration(opt, hosts, it);
    if (slice_reg) clk.mark("registration");
    R.par([&](int r) { HOSTR(r, svrh_reconstruct_iteration(hosts[r], it == iterations - 1 ? opt.rec_last : opt.rec_first)); });   // main.cc:930-1140
    double sc[8];
    svrh_get_state(hosts[0], nullptr, nullptr, nullptr, nullptr, sc);
    fprintf(stderr, "iteration %d: sigma %.4g mix %.3f\n", it, sc[0], sc[1]);
    clk.mark("reconstruction iteration");
    if (opt.structural) structural_line(P, R, hosts, it);
    if (opt.save_slice_transformations) save_slice_transformations(P, R);
  }
  if (clk.on && opt.enable_bias && opt.sigma > 0) {                       // which bias stages ran (rank 0)
    int nb = 0, nn = 0;
    ENGR(R, 0, svr_get_option(R.ctxs[0], "bias_corrections", &nb));
    ENGR(R, 0, svr_get_option(R.ctxs[0], "bias_normalisations", &nn));
    fprintf(stderr, "[timing] bias correction: %d CorrectBias, %d NormaliseBias\n", nb, nn);
  }
}

// ---- afterwards ----------------------------------------------------------------------------------------
// RestoreSliceIntensities + ScaleVolume (main.cc:1189-1193), and the volume is written
void write_volume(const Options &opt, const Problem &P, const Ranks &R, const std::vector<svrh_recon *> &hosts, StageClock &clk) {
  R.par([&](int r) {
    ENGR(R, r, svr_restore_slice_intensities(R.ctxs[r], P.factors.data(), (int)P.factors.size(), P.stack_index.data() + R.rlo[r]));
    HOSTR(r, svrh_scale_volume_gpu(hosts[r]));
  });
  std::vector<float> vol((size_t)P.tattr.nx * P.tattr.ny * P.tattr.nz);
  ENGR(R, 0, svr_sync_cpu(R.ctxs[0], vol.data()));
  char err[256] = {0};
  clk.mark("restore, scale, download");
  if (svr_nifti_write(opt.output.c_str(), &P.tattr, vol.data(), err)) die(opt.output + ": " + err);
  clk.mark("write the volume");
}

// --sliceReport: rows in the reference's slice order; the three lists of EvaluateGPU and the median ncc per stack on stderr
void write_slice_report(const Options &opt, const Problem &P, const Ranks &R, const std::vector<svrh_recon *> &hosts, const std::vector<float> &scale_g,
                        const std::vector<float> &weight_g, const std::vector<unsigned char> &inside, const std::vector<double> &sums,
                        const std::vector<double> &ssim_sums) {
  const int ns = P.ns;
  const bool report_ex = opt.structural;                                  // three more columns: ssim n_ssim structural
  char err[256] = {0};
  std::vector<int> r_stack(ns);
  std::vector<float> r_weight(ns), r_scale(ns);
  std::vector<unsigned char> r_inside(ns);
  std::vector<double> r_p6(6 * (size_t)ns), r_sums(sums.size()), r_ssim(ssim_sums.size());
  std::vector<unsigned char> in_force(report_ex ? ns : 0), r_force(report_ex ? ns : 0);
  if (report_ex) HOSTR(0, svrh_get_structural(hosts[0], nullptr, nullptr, in_force.data(), nullptr));
  for (int i = 0; i < ns; ++i) {                                          // row i = slice i of the reference's order
    const int s = R.inv_order[i];
    r_stack[i] = P.stack_index[s]; r_weight[i] = weight_g[s]; r_scale[i] = scale_g[s]; r_inside[i] = inside[s];
    svrh_irtk_rigid_parameters(&P.T[16 * (size_t)s], &r_p6[6 * (size_t)i], nullptr);
    std::copy(sums.begin() + (size_t)s * SVR_SLICE_QUALITY_SUMS, sums.begin() + (size_t)(s + 1) * SVR_SLICE_QUALITY_SUMS,
              r_sums.begin() + (size_t)i * SVR_SLICE_QUALITY_SUMS);
    if (report_ex) { r_ssim[2 * (size_t)i] = ssim_sums[2 * (size_t)s]; r_ssim[2 * (size_t)i + 1] = ssim_sums[2 * (size_t)s + 1]; r_force[i] = in_force[s]; }
  }
  if (report_ex ? svr_slice_report_write_ex(opt.report_name.c_str(), ns, r_stack.data(), r_weight.data(), r_inside.data(), r_scale.data(),
                                            r_p6.data(), r_sums.data(), r_ssim.data(), r_force.data(), err)
                : svr_slice_report_write(opt.report_name.c_str(), ns, r_stack.data(), r_weight.data(), r_inside.data(), r_scale.data(), r_p6.data(),
                                         r_sums.data(), err))
    die(opt.report_name + ": " + err);
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
  for (size_t k = 0; k < P.stacks.size(); ++k) {
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

// --simulatedStacks: the simulated slices back in the cropped stacks' geometry
void write_simulated_stacks(const Options &opt, const Problem &P, const Ranks &R, const std::vector<float> &weight_g, const std::vector<unsigned char> &inside,
                            const std::vector<float> &sim) {
  char err[256] = {0};
  int base = 0;                                                           // the stack's first slice in the reference's order
  for (size_t k = 0; k < P.stacks.size(); ++k) {
    const svr_image_attr &a = P.stacks[k].a;
    std::vector<float> out((size_t)a.nx * a.ny * a.nz, 0.0f);            // excluded and outside slices stay zero, as SimulateStacks leaves them
    for (int j = 0; j < a.nz; ++j) {
      const int s = R.inv_order[base + j];
      if (!(weight_g[s] >= 0.5f && inside[s])) continue;
      for (int y = 0; y < a.ny; ++y)
        for (int x = 0; x < a.nx; ++x) {
          const size_t g = ((size_t)s * P.my + y) * P.mx + x;
          if (P.grid[g] != -1.0f) out[((size_t)j * a.ny + y) * a.nx + x] = sim[g];
        }
    }
    base += a.nz;
    const std::string path = opt.sim_prefix + std::to_string(k) + ".nii.gz";
    if (svr_nifti_write(path.c_str(), &a, out.data(), err)) die(path + ": " + err);
  }
}

// How the run went (not in the reference's main(); SlicesInfo RG.cc:4937-4975, SimulateStacks :1205-1262, EvaluateGPU :4503-4538).
// The volume is on disk: nothing from here on can reach it.  Every rank projects the final volume into its slices once and
// reduces them (svr_slice_quality); rows and stacks are written in the reference's slice order, through order[].
void report_final_slices(const Options &opt, const Problem &P, const Ranks &R, const std::vector<svrh_recon *> &hosts, bool timing) {
  const int ns = P.ns, nr = R.nr;
  const size_t slice = (size_t)P.mx * P.my;
  const bool report = !opt.report_name.empty(), simulate = !opt.sim_prefix.empty();
  std::vector<float> scale_g(ns), weight_g(ns), sim;
  std::vector<unsigned char> inside(ns);
  std::vector<double> sums((size_t)ns * SVR_SLICE_QUALITY_SUMS, 0.0);
  const bool report_ex = opt.structural && report;
  std::vector<double> ssim_sums(report_ex ? 2 * (size_t)ns : 0, 0.0);
  if (simulate) sim.resize((size_t)ns * slice);
  R.par([&](int r) {                                                      // (collective: the other ranks' vectors may still be on their way)
    HOSTR(r, svrh_get_state(hosts[r], r ? nullptr : scale_g.data(), r ? nullptr : weight_g.data(), nullptr, nullptr, nullptr));
  });
  std::vector<double> t_sim(nr, 0.0), t_qual(nr, 0.0);
  R.par([&](int r) {
    const size_t o = (size_t)R.rlo[r], nl = (size_t)(R.rhi[r] - R.rlo[r]);
    const auto t0 = std::chrono::steady_clock::now();
    ENGR(R, r, svr_simulate_slices(R.ctxs[r], inside.data() + o));
    const auto t1 = std::chrono::steady_clock::now();
    if (report) ENGR(R, r, svr_slice_quality(R.ctxs[r], sums.data() + o * SVR_SLICE_QUALITY_SUMS));
    const auto t2 = std::chrono::steady_clock::now();
    if (report_ex && nl > 0) {                                            // the run's own window and constants (svrh_structural_evaluate)
      const double L = (double)P.vmax - (double)P.vmin;
      ENGR(R, r, svr_slice_ssim(R.ctxs[r], opt.st_radius, (0.01 * L) * (0.01 * L), (0.03 * L) * (0.03 * L), ssim_sums.data() + 2 * o, nullptr));
    }
    if (simulate) ENGR(R, r, svr_debug_get(R.ctxs[r], SVR_BUF_SIMSLICES, sim.data() + o * slice, nl * slice * sizeof(float)));
    t_sim[r] = std::chrono::duration<double>(t1 - t0).count(); t_qual[r] = std::chrono::duration<double>(t2 - t1).count();
  });
  if (timing)
    fprintf(stderr, "[timing] forward projection of the final volume %.3f ms, svr_slice_quality %.3f ms (slowest rank, host clock)\n",
            1e3 * *std::max_element(t_sim.begin(), t_sim.end()), 1e3 * *std::max_element(t_qual.begin(), t_qual.end()));
  if (report) write_slice_report(opt, P, R, hosts, scale_g, weight_g, inside, sums, ssim_sums);
  if (simulate) write_simulated_stacks(opt, P, R, weight_g, inside, sim);
}

void save_debug_transformations(const Options &opt, const Problem &P, const Ranks &R) {   // --debug: SaveTransformations, RG.cc:4903-4915
  const size_t cut = opt.output.find_last_of('/');
  const std::string folder = cut == std::string::npos ? "." : opt.output.substr(0, cut);
  for (int s = 0; s < P.ns; ++s) {
    double p6[6];
    svrh_irtk_rigid_parameters(&P.T[16 * (size_t)s], p6, nullptr);
    char e[256] = {0};
    const std::string path = folder + "/transformation" + std::to_string(R.order[s]) + ".dof";
    if (svr_dof_write(path.c_str(), p6, e)) die(path + ": " + e);
  }
}

}  // namespace

int main(int argc, char **argv) {
  Problem P;
  const Options opt = parse_options(argc, argv, P.extras);
  StageClock clk;
  // the HIP runtime and the context come up (75 ms) while the stacks are read and cropped; first use: the stack registrations
  svr_ctx *ctx = nullptr;
  std::future<int> ctx_ready = std::async(std::launch::async, [&] { return opt.dry_run ? 1 : svr_create(opt.devices.empty() ? 0 : opt.devices[0], &ctx); });
  before_exit = [&] { if (ctx_ready.valid()) ctx_ready.wait(); };     // an error while reading must not exit under the runtime's feet
  const std::function<svr_ctx *()> need_ctx = [&] {
    if (ctx_ready.valid() && (ctx_ready.get() || !ctx)) die("no usable HIP device (svr_create failed)");
    return ctx;
  };

  read_inputs(opt, P);
  read_extras(opt, P);
  clk.mark("read stacks");
  make_mask(opt, P);
  if (opt.auto_template) {
    select_template_by_motion(opt, P, need_ctx);
    clk.mark("motion measurement");
  }
  make_template(opt, P);
  clk.mark("mask, crop, template");
  crop_and_register_stacks(opt, P, need_ctx);
  clk.mark("stack registrations, crops");
  P.factors = match_stack_intensities(P.stacks, P.ts, P.vol_mask, opt.average, opt.no_matching);
  clk.mark("match stack intensities");
  pack_slices(opt, P);
  pack_extras(P);
  if (!opt.channels_dump.empty()) dump_channels(opt.channels_dump, P);
  if (!opt.dump_name.empty()) dump_problem(opt.dump_name, P);
  if (opt.dry_run) { fflush(nullptr); _exit(0); }         // (no context was made; skip the teardown of a runtime that never came up)
  if (!(P.vmax > 0)) die("no slice pixel lies inside the mask");
  fprintf(stderr, "%zu stacks, %d slices of up to %dx%d, volume %dx%dx%d at %g mm, stack factors", P.stacks.size(), P.ns, P.mx, P.my, P.tattr.nx, P.tattr.ny,
          P.tattr.nz, P.resolution);
  for (float f : P.factors) fprintf(stderr, " %.9g", f);
  fprintf(stderr, "\n");

  Ranks R;
  std::vector<svrh_recon *> hosts;
  shard_slices(opt, P, R);
  R.ctxs[0] = need_ctx();                                  // rank 0 adopts the context that came up beside the set-up
  for (int r = 1; r < R.nr; ++r) R.create_context(r, opt.devices[r]);
  R.create_group(opt.devices);
  setup_engines(opt, P, R, hosts);
  if (!opt.tfolder.empty()) read_tfolder(opt, P, R);
  clk.mark("slices, engine set-up, upload");
  if (!opt.reference_name.empty()) {
    seed_reference_volume(opt, P, R);
    clk.mark("reference volume");
  }
  run_iterations(opt, P, R, hosts, clk);
  write_volume(opt, P, R, hosts, clk);
  if (!opt.report_name.empty() || !opt.sim_prefix.empty()) {
    report_final_slices(opt, P, R, hosts, clk.on);
    clk.mark("slice report, simulated stacks");
  }
  if (!P.extras.empty()) {
    std::vector<float> echoes;
    reconstruct_extras(opt, P, R, hosts, clk.on, echoes);
    clk.mark("channels, labels");
    if (!opt.fit_rate.empty() || !opt.fit_t.empty() || !opt.fit_amplitude.empty() || !opt.fit_residual.empty() || !opt.fit_count.empty()) {
      fit_echoes(opt, P, R, echoes, clk.on);
      clk.mark("fit of the echoes");
    }
  }
  if (opt.debug) save_debug_transformations(opt, P, R);
  for (svrh_recon *h : hosts) svrh_destroy(h);
  R.destroy();
  clk.mark("teardown");
  return 0;
}
