// What a PSF pass runs on and what it does with the coefficient table: two decisions, each made once, in plain C++ -- options, geometry
// and the table's state in, a plain value out.  No HIP, no svr_ctx: tests/plan_check.cpp compiles this header with g++ and enumerates both.
// svr_hip.hip fills PassOptions (pass_options), svr_table.inc fills TableInputs and carries a plan out (table_plan_for / table_begin / table_end).
#pragma once

#include <algorithm>

// what the coefficient table holds (CoeffTable::coeff_state): nothing, the PSF pixels of the pass that wrote it (coeff_lazy: a gather or
// scatter of the SR iterations, pass 2 of a Gaussian reconstruction), or every pixel with s != -1 (k_coeff_build)
enum CoeffState { COEFF_NONE = 0, COEFF_PSF = 1, COEFF_FULL = 2 };

// Which kernel family runs a PSF pass: the one place that reads pvr, pvr_mode, back_mode, fwd_mode, gauss_mode and bias_mode for it.  Device-free:
// the options and the geometry in, a plain value out.  What only the built cell lists can tell (CellState::usable) is cells_or_fallback's.
enum Family {
  FAM_CELLS,    // svr_cell.inc: (cell, plane) items, no atomics -- the default
  FAM_TILES,    // svr_tile.inc: slice tiles -- the audible fallback, and the table's gather on coarse slices
  FAM_PIXELS,   // psf_kernel / pvr_kernel: a wavefront per pixel, kept for the parity tests
};
// (the Gaussian reconstruction: pass 1 gathers, pass 2 scatters; a channel's passes take the SR passes' kernels and only ever run on FAM_CELLS)
enum Pass { PASS_GAUSS1, PASS_GAUSS2, PASS_FORWARD, PASS_BACK, PASS_BIAS, PASS_CHANNEL_SCATTER, PASS_CHANNEL_GATHER };
struct PassPath {
  Family family;           // what the options ask for
  int scatter_level;       // launch_scatter's level for a scatter on FAM_TILES: 4 = wave-owned planes first, 3 = the workgroup kernel, 1 = LDS atomics
  bool may_stream_table;   // the family's kernels have a COEFF instantiation: the pass streams the table when it holds the pass's pixels
  bool table_on_cells;     // a gather on FAM_CELLS stays there when it streams the table (else it takes FAM_TILES, silently; a pass that writes
                           // the table is the cell gather)
};
struct PassOptions {
  int pvr, pvr_mode, back_mode, fwd_mode, gauss_mode, bias_mode;   // the options of the same names
  bool fwd_mode_user;      // "fwd_mode" was set by the caller
  double density;          // voxel area / pixel area in the slice plane (pixel_density)
  int gather_cell_area;    // gw * gh of the gather's cells (cell_sizes)
};
inline PassPath pass_path(const PassOptions &o, Pass pass) {
  const bool pvr = o.pvr != 0;
  const bool pvr_units = o.pvr_mode == 1;                // patch-based runs: the unit-based kernels of either family, else pvr_kernel
  PassPath p = {FAM_PIXELS, 0, false, false};
  switch (pass) {
    case PASS_GAUSS1:      // pass 1 follows the gather: over the (cell, plane) items when that is the gather's mode (fwd_mode 2; round 4), per slice
    case PASS_GAUSS2:      // tile otherwise; pass 2 follows the scatter.  The same bits
      if (o.gauss_mode != 1 || (pvr && !pvr_units)) break;
      p.may_stream_table = true;
      if (pass == PASS_GAUSS1) p.family = o.fwd_mode == 2 ? FAM_CELLS : FAM_TILES;
      else p.family = o.back_mode == 5 ? FAM_CELLS : FAM_TILES;
      p.scatter_level = pvr ? 4 : std::min(4, std::max(1, o.back_mode));
      break;
    case PASS_FORWARD:
    case PASS_CHANNEL_GATHER:
      if (pvr ? !pvr_units : o.fwd_mode < 1) break;
      p.may_stream_table = true;
      p.family = o.fwd_mode == 2 ? FAM_CELLS : FAM_TILES;
      // fwd_mode 2 (the default for SVR on the fly): the gather over the (cell, plane) items of the scatter without atomics
      // (with the coefficient table: the cell gather for support 12 only -- PVR8spx 24.5 -> 20.7 ms; for support 16 its ring and its 16
      // box values do not fit the registers and the unit gather streams the table faster: P4 2.76 against 3.04 ms)
      // ... and there only on large cells, i.e. fine volumes: PVR4 (9 x 6) 8.1 ms on tiles against 8.5 ms on cells)
      // Round 6: support 16 takes the cell gather too -- the table's rows land in the LDS by LDS-DMA instead of in a ring of registers (fwd_cell_kernel,
      // COEFF == 2): P4 2.39 against 2.84 ms; option fwd_mode 1 keeps the tile kernel reachable
      // ... where the slices' pixels are not much coarser than the voxels (the density of tile_shape_rule): S8 (d 0.56, a 174 GB table) 28.1 ms on the
      // cells whatever their size (6 x 4 .. 12 x 6) against 26.9 ms on 6 x 5 slice tiles
      if (pvr) p.table_on_cells = o.gather_cell_area >= 96 || o.fwd_mode_user;
      else p.table_on_cells = o.fwd_mode_user || o.density >= 0.65;
      break;
    case PASS_BACK:
    case PASS_CHANNEL_SCATTER:
      if (pvr ? !pvr_units : o.back_mode < 1) break;
      p.family = o.back_mode == 5 ? FAM_CELLS : FAM_TILES;
      p.scatter_level = pvr ? 4 : std::min(4, o.back_mode);
      p.may_stream_table = pvr || o.back_mode >= 4;        // (back_tiled_kernel and back_slot_kernel evaluate)
      break;
    case PASS_BIAS:        // the NormaliseBias scatter: the SR scatter's cell kernels, or round 1's psf_kernel<MODE_BIAS>
      if (o.bias_mode >= 1 && !pvr && o.back_mode == 5) { p.family = FAM_CELLS; p.may_stream_table = true; }
      break;
  }
  return p;
}

// What a pass does with the table: evaluate every tap, stream the table's rows, or evaluate and store them (the COEFF instantiations 0, 1 / 2, 3)
enum TableUse { TABLE_EVALUATE, TABLE_STREAM, TABLE_STORE };
struct TablePlan {
  bool build_first;        // k_coeff_build fills the table for every active pixel before the pass (-> COEFF_FULL)
  TableUse use;
};
struct TableInputs {
  bool wanted;             // option "coeff_table", until a table did not fit
  CoeffState state;
  bool lazy_ok;            // the table may be left to the first evaluating cell pass: option "coeff_lazy", support 16, the cell gather (fwd_mode 2)
  bool n_active, n_psf;    // there are pixels with s != -1 / PSF pixels (a subset)
  bool cells_usable;       // the pass's own cell lists hold the geometry (CellState::usable): means something on FAM_CELLS only.  A caller that
                           // has not built them yet plans with `true` and again with what they said where the plan was TABLE_STORE
};
// Pending: wanted, not there, and left to the evaluating cell pass that writes it -- whichever PSF pass comes first after a new geometry,
// every other pass evaluates meanwhile.  A pass streams when the table holds its pixels: the passes of the SR iterations read the PSF pixels
// (either written state has them), the Gaussian pass every pixel with s != -1 (COEFF_FULL).  The Gaussian reconstruction's two passes share
// one decision: pass 1 streams or evaluates, pass 2 streams, evaluates or stores.  Never TABLE_STORE with build_first.
inline TablePlan table_plan(Pass pass, const PassPath &p, const TableInputs &t) {
  const bool cells = p.family == FAM_CELLS && t.cells_usable;
  const bool absent = t.wanted && t.state == COEFF_NONE;
  const bool pending = absent && t.lazy_ok;
  bool store = false, may_stream = p.may_stream_table;
  CoeffState need = COEFF_PSF;
  TablePlan tp = {false, TABLE_EVALUATE};
  switch (pass) {
    case PASS_GAUSS1:
    case PASS_GAUSS2:
      need = COEFF_FULL;
      store = cells && pending && t.n_active;
      tp.build_first = p.may_stream_table && !pending && absent && t.n_active;
      break;
    case PASS_FORWARD:     // the gather that cannot store builds, whether it may stream or not, lazy or not
      store = cells && pending && t.n_psf && t.n_active;
      tp.build_first = !store && absent && t.n_active;
      break;
    case PASS_BACK:        // the scatter that cannot store a pending table leaves it to a later pass
      store = cells && pending && t.n_psf && t.n_active;
      tp.build_first = !pending && absent && t.n_active;
      break;
    case PASS_BIAS:        // on the cell kernels only, and readers only
    case PASS_CHANNEL_SCATTER:
      may_stream = true;
      break;
    case PASS_CHANNEL_GATHER:   // has no slice tiles to go to: where svr_simulate_slices would stream there, it evaluates (the same bits)
      may_stream = p.may_stream_table && p.table_on_cells;
      break;
  }
  const CoeffState state = tp.build_first ? COEFF_FULL : t.state;
  if (store) tp.use = TABLE_STORE;
  else if (may_stream && t.wanted && state >= need) tp.use = TABLE_STREAM;
  return tp;
}
// A gather on FAM_CELLS (the forward projection, pass 1 of the Gaussian reconstruction -- whose table_on_cells is never set) stays there
// unless it streams a table the slice tiles stream faster; `use` = what the pass ends up doing (table_begin)
inline bool gather_stays_on_cells(const PassPath &p, TableUse use) { return use != TABLE_STREAM || p.table_on_cells; }
