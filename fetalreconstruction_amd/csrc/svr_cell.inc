// svr_cell.inc -- the scatter WITHOUT float atomics (back_mode 5): cell-owned planes + a fixed-order combine.
// #included by svr_hip.hip inside its second anonymous namespace (after the launch helpers, before the C-ABI).
//
// Replaces the flush of back_wave_kernel (SuperresolutionKernel3D_tex RC.cu:408-522; pass 2 of
// gaussianReconstructionKernel3D_tex RC.cu:260-295): there a wavefront owns four planes of the box of ONE SLICE TILE and
// adds them to the volume with device-scope float atomics when the tile is done -- 55 k tiles x 17 planes on P4, each box
// voxel flushed by every tile whose footprints cover it: 3.3 GB of atomic traffic per launch against 38 MB of algorithmic
// bytes (profiles/r02_pmc_p4.txt), in run-dependent order.  Here the box belongs to a piece of the VOLUME instead:
//
//   * the slices are split into two classes by their owned axis (SliceConst::own: the volume axis y or z closest to the
//     slice normal; the planes a wavefront owns are planes of that axis, the lanes run over the other one, rows along x);
//   * per class the (x, lane axis) plane is cut into CELLS of CX x CL voxels; a pixel belongs to the cell of its centre
//     voxel.  The pixels (s != -1) are sorted by (class, cell, slice, band of centre planes, position): a RUN is the pixels
//     of one slice in one cell around one plane -- what a slice tile was, cut in volume space -- built once per slice
//     geometry (cell_prepare);
//   * a work item is (cell, ONE plane of the owned axis): one wavefront walks every run of its cell whose footprints reach the
//     plane and evaluates their (pixel, plane) units exactly like back_wave_kernel (row per lane, plain LDS read-add-write,
//     dead units: first taps only).  Its four 16-lane slots each keep a PRIVATE copy of the cell's box of (CX + 15) x
//     (CL + 15) voxels and take every fourth pixel of a run: the slots work on the same slice and the same plane, so a unit
//     is live or dead in all of them alike and they carry the same number of units to within one.  (Two earlier versions
//     are in DESIGN 5.3: four consecutive planes of one cell had one slot evaluating live units while the others held dead
//     ones; four cells of a quad got 4 or 5 pixel rows each and waited for the fullest.)  The four copies are added up in LDS
//     in a fixed order and the box goes out once per item, as plain coalesced float2 rows into the item's own slab of a
//     staging buffer: no atomics, no mask test, no scan for non-zeros;
//   * k_cell_combine, one thread per volume voxel, adds the <= (1 + 15/CX)(1 + 15/CL) slabs per class that cover the voxel in
//     a fixed order (class, plane, lane cell, x cell), applies the mask and the float->uint saturation of RC.cu:508
//     (negative coordinates alias to index 0: voxel 0 of an axis sums every staged coordinate <= 0) and writes addon|cmap.
//
// The result does not depend on the launch, the run or the hardware's atomic order: bit-identical from run to run.
// Staging traffic: 8 bytes written + 8 read per box voxel of an item (P4: ~0.1 GB + 0.1 GB per launch).

struct CellRec {            // one sorted pixel, 32 bytes
  short cx, cl, cz;         // centre voxel: x, lane axis, owned axis
  unsigned short dead;      // unit_is_dead of the 16 units (SVR)
  float bx, by, bz;         // scaled residual at the centre (pixel_setup)
  float f0, f1;             // per launch: {psf -> addon, psf -> cmap} factors; both 0 = nothing to add
  uint32_t idx;             // slice-grid index
};
static_assert(sizeof(CellRec) == 32, "CellRec layout");

struct CellRun {            // the pixels of one slice in one quad
  uint32_t start, count;    // range of the sorted records
  uint32_t cell, slice;     // cell = the quad's global index
  short czmin, czmax;
  unsigned short n[4];      // pixels in each of the quad's four cells (the records of a run are sorted by cell).  A slice whose
  int pad;                  // normal is the x axis lies IN the owned axis: its run is a whole column of the slice
};
static_assert(sizeof(CellRun) == 32, "CellRun layout");
// The most pixels of one slice in one cell (around one band of planes) the lists take.  CellRun::n could say 65535, but a slot adds its quarter of a
// run to a voxel in ONE chain of float adds: with the 16 k adds per slot of a 65 535-pixel run (0.01 mm pixels, regular terms) pass 2 of the Gaussian
// reconstruction left volw 4e-5 from the oracle, twice the 2e-5 the parity tests allow, where the short chains of the slice tiles leave 7e-6
// (tests/test_cell_limits_gpu.py).  16384 is still beyond anything the lists are laid out for: cell_auto_size stops at 16 pixels per voxel area, and the
// largest cell whose boxes fit the LDS (26 x 26) then holds 10 816 pixels of a slice.
constexpr uint32_t CELL_RUN_MAX = 16384u;

struct CellClass {
  int x0, l0;               // first centre coordinate of cell (0, 0)
  int ncx, ncl;             // QUADS along x / the lane axis
  int pfirst, plast;        // first / last absolute plane that can receive a tap (plast <= volume - 1; pfirst may be negative)
  int ng;                   // planes: plast - pfirst + 1
  int cell_base;            // global index of the class's first quad
  int row_base, col_base;   // the class's first entry in CellArgs::rowcol: its rows of quads (ncl), its columns (ncx)
};

struct CellArgs {
  CellClass cls[2];         // [0]: own == 1 (planes = y, lanes = z), [1]: own == 2 (planes = z, lanes = y)
  int CX, CL, PL, DL, PP;   // cell size; box pitch / rows / voxels of one cell's plane
  uint32_t mCX, mCL;        // ceil(2^32 / CX), ceil(2^32 / CL) (0 for a size of 1): floordiv_m, the combine's divisions without the divider sequence
  int qCX, qCL;             // ceil(2^16 / size): size * q is added before and q taken off after, so that the dividend is never negative
  int QX, QL;               // cells of a quad along x / the lane axis (QX * QL == 4: one per slot)
  int band_shift;           // a run holds the pixels of 2^band_shift consecutive centre planes
  int ngs;                  // stride of the (quad, plane) tables = max ng
  int split;                // least number of parts per item (option cell_split; cell_prepare)
  int dbg;                  // dev experiments: 1 = walk and list, no evaluation; 2 = also count into stats
  unsigned long long *trace; // dev experiment (SVR_CELL_TRACE=file): per entry {start, end (s_memrealtime, 100 MHz), HW_ID | XCC_ID << 32} of the scatter's wavefronts
  unsigned long long *stats; // dbg 2: [0] chunk visits, [1] chunks with work, [2] sum over chunks of the longest live list, [3] live units, [4] dead units, [5] run visits
  const CellRec *recs;
  const CellRun *runs;
  const uint32_t *cell_first, *cell_last;   // [cell] run range
  const uint32_t *items;    // quad << 10 | plane index, in launch order (heaviest first)
  uint32_t nitems;
  const uint4 *ents;        // what a workgroup takes: {item, part | parts << 16, the cell's run range} -- an item whose runs would keep one wavefront busy for
  uint32_t nents;           // much longer than the launch's fair share is cut into parts (every parts-th run that reaches the plane each)
  const int *item_of;       // [quad * ngs + plane index] -> the item's first entry | (parts - 1) << 28, or -1 (entries < 2^28)
  f2 *stage;                // [entry][DL][PL]
  const unsigned char *rowcol; // [CellClass::row_base + row of quads] / [col_base + column]: 1 = some run lies in it (combine_class skips the rest; NULL: none skipped)
  const unsigned char *act; // COEFF == 3 (the scatter that writes the table): [sorted record] 1 = a PSF pixel -- its units are evaluated and stored whatever its
                            // factors are this time (NULL: the factors decide, as in every other launch)
  const uint32_t *pid;      // [sorted record] -> the pixel's id in the coefficient table (cell_pids; COEFF launches only): travels with the record,
};                          // where PsfArgs::coeff_id[record's idx] was one more dependent load at the head of every chunk

struct CellState {
  bool valid = false, usable = true;
  CellArgs a;
  int *d_centres = nullptr;            // (alias) int4 per active pixel (svr_ctx::d_cellc: shared by the scatter's and the gather's lists)
  DevBuf<uint64_t> d_keys, d_keys2;
  DevBuf<uint32_t> d_head, d_runid;
  DevBuf<CellRec> d_recs;
  DevBuf<CellRun> d_runs;
  DevBuf<uint32_t> d_cell_first, d_cell_last, d_items, d_item_flag, d_item_pos;
  DevBuf<uint4> d_ents;
  DevBuf<int> d_item_of;
  DevBuf<f2> d_stage;
  DevBuf<unsigned char> d_rowcol;
  DevBuf<float> d_gf;                  // gather: 1 / v_PSF_sums per sorted pixel, 0 = not a PSF pixel
  DevBuf<f2> d_part;                   // gather: the units' partial sums [unit][sorted pixel] (a run's pixels of one plane: neighbours)
  DevBuf<uint32_t> d_pid;              // table ids of the sorted records (cell_pids)
  DevBuf<unsigned char> d_act;         // PSF-pixel flags of the sorted records for the scatter that writes the table (k_cell_factors)
  bool pid_valid = false;
  bool gf_valid = false;               // d_gf matches v_PSF_sums (it changes with a Gaussian pass, not with an SR iteration: CH_PSF_SUMS)
  DevBuf<unsigned char> d_tmp;         // the sorts' and scans' temporary storage (bytes)
  DevBuf<int> d_range;                 // [2][6] min / max of the centres, [12] dropped pixels
  uint32_t n_sorted = 0, n_runs = 0, n_cells = 0;
  uint64_t dead_units = 0;             // (pixel, plane) units of the sorted pixels that are dead (unit_is_dead)
  int ns_support = 0;
};

void cell_free(CellState *c) { delete c; }

__device__ __forceinline__ int floordiv(int a, int b) { return (a >= 0) ? a / b : -((-a + b - 1) / b); }
// floordiv(a, b) for -2^16 <= a < 2^16 and b <= 1024 by multiplication: m = ceil(2^32 / b), q = ceil(2^16 / b); a + b q is in [0, 2^18), where
// mulhi(n, m) == n / b (Granlund-Montgomery: exact for n < 2^32 / b).  Volume and cell coordinates are far inside the range (cell_prepare
// checks).  A runtime `/` costs ~35 VALU instructions; k_cell_combine_wave made eight of them per class and was instruction bound.
__device__ __forceinline__ int floordiv_m(int a, int b, uint32_t m, int q) {
  const uint32_t n = (uint32_t)(a + b * q);
  return (int)(m ? __umulhi(n, m) : n) - q;
}

// ---- once per slice geometry ---------------------------------------------------------------------------------------
// centre voxel and class of every pixel with s != -1; the ranges of the centres per class.  A pixel whose footprint lies
// entirely beyond the high end of the volume on some axis contributes nothing (RC.cu:509) and is dropped (class -1).
__global__ __launch_bounds__(256) void k_cell_centres(PsfArgs a, int NC, int *centres, int *range) {
  // a grid-stride loop: a thread keeps the bounds of its pixels in registers, a workgroup adds its wavefronts' up in the LDS and
  // touches the twelve global words once (one pixel per thread and one set of atomics per wavefront took 1.15 ms on P4's
  // 1.15 M pixels, nearly all of it the 15 k wavefronts queueing on twelve addresses)
  __shared__ int sh[4][13];
  int v[2][6];
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int q = 0; q < 6; ++q) v[k][q] = (q & 1) ? INT_MIN : INT_MAX;
  int ndrop = 0;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += gridDim.x * blockDim.x) {
    const uint32_t idx = a.list[i];
    const uint32_t n2 = (uint32_t)(a.sx * a.sy);
    const uint32_t sl = idx / n2, rem = idx - sl * n2;
    const int py = (int)(rem / (uint32_t)a.sx), px = (int)(rem - (uint32_t)py * (uint32_t)a.sx);
    const SliceConst &S = a.sc[sl];
    const PixelState P = pixel_setup(S, a.vg, px, py);
    const bool swap = S.own == 1;
    int c = swap ? 0 : 1;
    const int cx = P.cxi, cl = swap ? P.czi : P.cyi, cz = swap ? P.cyi : P.czi;
    const int vgl = swap ? a.vg.vz : a.vg.vy, vgz = swap ? a.vg.vy : a.vg.vz;
    if (cx - NC > a.vg.vx - 1 || cl - NC > vgl - 1 || cz - NC > vgz - 1) c = -1;
    reinterpret_cast<int4 *>(centres)[i] = make_int4(cx, cl, cz, c);
    ndrop += c == -1;
#pragma unroll
    for (int k = 0; k < 2; ++k)
      if (c == k) {
        v[k][0] = min(v[k][0], cx); v[k][1] = max(v[k][1], cx);
        v[k][2] = min(v[k][2], cl); v[k][3] = max(v[k][3], cl);
        v[k][4] = min(v[k][4], cz); v[k][5] = max(v[k][5], cz);
      }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ndrop += __shfl_xor(ndrop, o, 64);
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        const int w = __shfl_xor(v[k][q], o, 64);
        v[k][q] = (q & 1) ? max(v[k][q], w) : min(v[k][q], w);
      }
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int q = 0; q < 6; ++q) sh[wave][6 * k + q] = v[k][q];
    sh[wave][12] = ndrop;
  }
  __syncthreads();
  if (threadIdx.x < 13) {
    const int q = threadIdx.x;
    int r = sh[0][q];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r = q == 12 ? r + sh[w][q] : (q & 1) ? max(r, sh[w][q]) : min(r, sh[w][q]);
    if (q == 12) { if (r) atomicAdd(range + 12, r); }
    else if (q & 1) { if (r != INT_MIN) atomicMax(range + q, r); }
    else if (r != INT_MAX) atomicMin(range + q, r);
  }
}

// sort key: quad (classes apart) | slice | band of planes | cell of the quad | position in the slice: 18 + 17 + 7 + 2 + 20 bits
// (dropped pixels: all ones, they sort to the end)
__global__ void k_cell_keys(PsfArgs a, CellArgs ca, const int *centres, uint64_t *keys) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const int4 c = reinterpret_cast<const int4 *>(centres)[i];
  if (c.w < 0) { keys[i] = ~0ull; return; }
  const CellClass &C = ca.cls[c.w];
  const uint32_t idx = a.list[i];
  const uint32_t n2 = (uint32_t)(a.sx * a.sy);
  const uint32_t sl = idx / n2, rem = idx - sl * n2;
  const int jl = (c.y - C.l0) / ca.CL, ix = (c.x - C.x0) / ca.CX;             // the pixel's cell
  const uint32_t cell = (uint32_t)C.cell_base + (uint32_t)(jl / ca.QL) * (uint32_t)C.ncx + (uint32_t)(ix / ca.QX);   // its quad
  const uint32_t sub = (uint32_t)((jl % ca.QL) * ca.QX + ix % ca.QX);          // ... and which of the quad's four cells = which slot
  // band: a slice whose normal is the x axis lies IN the owned axis, a quad holds a whole column of it; cut into bands of a few
  // planes a run is again a handful of pixels around one plane, and an item only visits the bands near its own plane
  const uint32_t band = (uint32_t)(c.z - (C.pfirst)) >> ca.band_shift;
  keys[i] = ((uint64_t)cell << 46) | ((uint64_t)sl << 29) | ((uint64_t)band << 22) | ((uint64_t)sub << 20) | (uint64_t)rem;
}

// the geometry half of the records, in sorted order, and the heads of the runs
template <int NS, bool PVR>
__global__ void k_cell_records(PsfArgs a, const uint64_t *keys, uint32_t n, CellRec *recs, uint32_t *head, unsigned int *dead_units) {
  constexpr int NC = (NS - 1) / 2;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t k = keys[i];
  const uint32_t sl = (uint32_t)(k >> 29) & 0x1FFFFu, rem = (uint32_t)k & 0xFFFFFu;
  const int py = (int)(rem / (uint32_t)a.sx), px = (int)(rem - (uint32_t)py * (uint32_t)a.sx);
  const SliceConst &S = a.sc[sl];
  const PixelState P = pixel_setup(S, a.vg, px, py);
  const bool swap = S.own == 1;
  CellRec R;
  R.cx = (short)P.cxi; R.cl = (short)(swap ? P.czi : P.cyi); R.cz = (short)(swap ? P.cyi : P.czi);
  R.bx = P.bx; R.by = P.by; R.bz = P.bz;
  R.f0 = R.f1 = 0.0f;
  R.idx = sl * (uint32_t)(a.sx * a.sy) + rem;
  unsigned dead = 0;
  if (!PVR) {
    // (not load_row_const: that reads four fields through readfirstlane for kernels whose wavefronts work on ONE slice; here
    // neighbouring threads hold pixels of different slices -- the first lane's inv2s2 / invD decided the dead bits of all 64)
    RowConst RC;
#pragma unroll
    for (int q = 0; q < 9; ++q) RC.Lp[q] = S.Lp[q];
    RC.inv2s2 = S.inv2s2; RC.dd = S.dd; RC.w = S.w; RC.invD = S.invD;
    const int F = swap ? 1 : 2;
#pragma unroll 1
    for (int z = 0; z < NS; ++z) dead |= unit_is_dead(RC, P.bx, P.by, P.bz, F, (float)(z - NC)) ? (1u << z) : 0u;
  }
  R.dead = (unsigned short)dead;
  recs[i] = R;
  {                                                       // (measurement only: svr_unit_counts) one atomic per wavefront
    unsigned int tot = 0;
    for (int z = 0; z < NS; ++z) tot += (unsigned int)__popcll(__ballot((dead >> z) & 1u));
    const unsigned long long active = __ballot(true);
    if ((int)(threadIdx.x & 63) == (int)__builtin_ctzll(active) && tot) atomicAdd(dead_units, tot);
  }
  head[i] = (i == 0 || (keys[i - 1] >> 22) != (k >> 22)) ? 1u : 0u;
}

__global__ void k_cell_runs(const uint64_t *keys, const uint32_t *head, const uint32_t *runid, uint32_t n, CellRun *runs) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !head[i]) return;
  CellRun r;
  r.start = i; r.count = 0;
  r.cell = (uint32_t)(keys[i] >> 46); r.slice = (uint32_t)(keys[i] >> 29) & 0x1FFFFu;
  r.czmin = r.czmax = 0; r.n[0] = r.n[1] = r.n[2] = r.n[3] = 0; r.pad = 0;
  runs[runid[i] - 1] = r;
}
__global__ void k_cell_run_ranges(CellRun *runs, uint32_t nruns, uint32_t n, const CellRec *recs, const uint64_t *keys, uint32_t *cell_first,
                                  uint32_t *cell_last, uint32_t *overflow) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nruns) return;
  CellRun R = runs[r];
  const uint32_t end = r + 1 < nruns ? runs[r + 1].start : n;
  R.count = end - R.start;
  int mn = 32767, mx = -32768;
  uint32_t cnt[4] = {0, 0, 0, 0};
  for (uint32_t i = R.start; i < end; ++i) {
    const int z = recs[i].cz;
    mn = min(mn, z); mx = max(mx, z);
    ++cnt[(uint32_t)(keys[i] >> 20) & 3u];
  }
  R.czmin = (short)mn; R.czmax = (short)mx;
  for (int q = 0; q < 4; ++q) {
    if (cnt[q] > CELL_RUN_MAX) atomicAdd(overflow, 1u);  // a cell holds more pixels of one slice than a run may: the caller falls back
    R.n[q] = (unsigned short)min(cnt[q], 65535u);
  }
  runs[r] = R;
  if (r == 0 || runs[r - 1].cell != R.cell) cell_first[R.cell] = r;
  if (r + 1 == nruns || runs[r + 1].cell != R.cell) cell_last[R.cell] = r + 1;
}

// the rows and the columns of quads that hold a run, per class.  The voxels of a low face add up every staged source coordinate <= 0 (combine_class); a slice
// far below the volume on two axes leaves the voxels of a low edge ~10^6 of them, nearly all in rows and columns of cells nothing lies in
__global__ void k_cell_rowcol(CellArgs ca, const CellRun *runs, uint32_t nruns, unsigned char *rowcol) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nruns) return;
  const uint32_t cell = runs[r].cell;
  const CellClass &C = ca.cls[cell >= (uint32_t)ca.cls[1].cell_base ? 1 : 0];
  const int lq = (int)cell - C.cell_base;
  const int ql = lq / C.ncx, qx = lq - ql * C.ncx;
  rowcol[C.row_base + ql] = 1;
  rowcol[C.col_base + qx] = 1;
}

// the work items: (cell, plane) pairs some run reaches, IN (cell, plane) ORDER -- flags, a prefix sum, then the list: the planes of
// a cell are neighbouring workgroups, so the 16 partial sums of a pixel (the gather) and the slabs a voxel's combine reads are
// written close together in time.  item_of[] is -1 elsewhere (the combine skips those slabs).
__global__ void k_cell_item_flags(CellArgs ca, int NC, int NH, uint32_t ncells, uint32_t *flag) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t cell = t / (uint32_t)ca.ngs;
  if (cell >= ncells) return;
  const int g = (int)(t - cell * (uint32_t)ca.ngs);
  bool any = false;
  const CellClass &C = ca.cls[cell >= (uint32_t)ca.cls[1].cell_base ? 1 : 0];
  if (g < C.ng) {
    const int P = C.pfirst + g;
    for (uint32_t r = ca.cell_first[cell]; r < ca.cell_last[cell] && !any; ++r)
      any = ca.runs[r].czmin - NC <= P && ca.runs[r].czmax + NH >= P;
  }
  flag[t] = any ? 1u : 0u;
}
__global__ void k_cell_items(CellArgs ca, uint32_t ntab, const uint32_t *flag, const uint32_t *pos, uint32_t *items, int *item_of) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntab) return;
  if (flag[t]) {
    const uint32_t cell = t / (uint32_t)ca.ngs;
    const uint32_t g = t - cell * (uint32_t)ca.ngs;
    const uint32_t at = pos[t] - 1u;                       // inclusive sum
    items[at] = cell << 10 | g;
    item_of[t] = (int)at;
  } else {
    item_of[t] = -1;
  }
}

// The launch order and the parts.  The workgroups of a launch are handed out in list order and a wavefront works through one entry:
// a launch of a few thousand entries per CU-slot ends when its last heavy entry does (P4: the items in (cell, plane) order left
// 9 % of the scatter's and the gather's time to the tail, a rank's eighth of P4 15-20 %).  So (i) the items go out in order of
// FALLING WORK (work ~ the pixels of the runs that reach the plane + a fixed cost per run; stable inside classes of 2^shift), and
// (ii) an item heavier than `target` (the launch's work / (cell_balance x 1024)) is cut into parts: part p takes every parts-th
// run that reaches the plane, stages its own slab (scatter; the combine adds an item's slabs in part order) or writes the
// partial sums of its own (pixel, plane) units (gather).  The lists depend on the geometry only: runs repeat bit for bit.
__global__ void k_cell_item_work(CellArgs ca, int NC, int NH, uint32_t nitems, int shift, uint32_t *work, uint64_t *keys) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nitems) return;
  const uint32_t item = ca.items[t];
  const uint32_t cell = item >> 10;
  const CellClass &C = ca.cls[cell >= (uint32_t)ca.cls[1].cell_base ? 1 : 0];
  const int P = C.pfirst + (int)(item & 1023u);
  uint32_t w = 0;
  for (uint32_t r = ca.cell_first[cell]; r < ca.cell_last[cell]; ++r) {
    const CellRun R = ca.runs[r];
    if (R.czmin - NC <= P && R.czmax + NH >= P) w += R.count + 8u;       // (+ a run's fixed cost)
  }
  work[t] = w;
  keys[t] = ((uint64_t)(~(w >> shift)) << 32) | (uint64_t)t;
}
// items in launch order and the number of parts of each
__global__ void k_cell_items_reorder(uint32_t nitems, const uint64_t *keys, const uint32_t *items_in, const uint32_t *work, uint32_t target,
                                     uint32_t least, uint32_t *items_out, uint32_t *parts) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nitems) return;
  const uint32_t from = keys ? (uint32_t)keys[t] : t;
  items_out[t] = items_in[from];
  uint32_t np = target ? (work[from] + target - 1u) / target : 1u;
  parts[t] = min(max(np, least), 16u);
}
__global__ void k_cell_entries(CellArgs ca, uint32_t nitems, const uint32_t *items, const uint32_t *parts, const uint32_t *pos, uint4 *ents, int *item_of) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nitems) return;
  const uint32_t item = items[t], np = parts[t], base = pos[t] - np;       // inclusive sum
  const uint32_t cell = item >> 10;
  for (uint32_t p = 0; p < np; ++p) ents[base + p] = make_uint4(item, p | np << 16, ca.cell_first[cell], ca.cell_last[cell]);   // (one dependent load less per wavefront)
  item_of[(size_t)(item >> 10) * ca.ngs + (item & 1023u)] = (int)(base | (np - 1u) << 28);
}

// ---- per launch ------------------------------------------------------------------------------------------------------
// the factors of every sorted pixel: what back_wave_kernel's "lane = pixel" part works out (RC.cu:439-447 / 278-282).
// gauss: 0 = the SR scatter, 1 = pass 2 of the Gaussian reconstruction, 2 = NormaliseBias (normalizeBiasKernel3D_tex RC.cu:544-550, 591:
// weight psf / sume, value the pixel's log bias minus the log of its slice's scale), 3 = a channel (svr_channel_scatter: the SR scatter's weight, the
// value read from a.channel), 4 = an SR iteration on a channel (svr_channel_sr_backproject: that weight where the channel's forward projection has a
// sim-weight > 0, the value a.channel minus that projection)
__global__ void k_cell_factors(PsfArgs a, int gauss, CellRec *recs, uint32_t n, unsigned char *act) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t idx = recs[i].idx;
  float f0 = 0.0f, f1 = 0.0f;
  if (gauss == 3) {
    // a channel (svr_channel.inc): the SR scatter's pixel set without the flag, minus the slices switched off; the SR scatter's own weight; the value
    // is the channel's (or the indicator of one label), never the primary image's -- no scale, no bias, no simulated slice
    const uint32_t sl = idx / (uint32_t)(a.sx * a.sy);
    if (pixel_active(a.slices, a.psf_sums, nullptr, idx) && (!a.unit_on || a.unit_on[sl] != 0)) {
      const float c = a.channel[idx];
      const float x = (a.ch_flags & SVR_CHANNEL_INDICATOR) ? (c == a.ch_match ? 1.0f : 0.0f) : c;
      f1 = (a.weights[idx] * a.slice_weights[sl]) / a.psf_sums[idx];
      f0 = f1 * x;
    }
    recs[i].f0 = f0; recs[i].f1 = f1;    // (never the pass that writes the table: act is NULL)
    return;
  }
  if (gauss == 4) {
    // an SR iteration on a channel (svr_channel_sr_backproject): mode 3's pixel set and weight, the residual against the channel's own forward
    // projection (a.simslices / a.simweights are the call's buffers).  The gate is the sim-weight, not the sign of the simulated value
    const uint32_t sl = idx / (uint32_t)(a.sx * a.sy);
    if (pixel_active(a.slices, a.psf_sums, nullptr, idx) && (!a.unit_on || a.unit_on[sl] != 0) && a.simweights[idx] > 0.0f) {
      f1 = (a.weights[idx] * a.slice_weights[sl]) / a.psf_sums[idx];
      f0 = f1 * (a.channel[idx] - a.simslices[idx]);
    }
    recs[i].f0 = f0; recs[i].f1 = f1;    // (never the pass that writes the table: act is NULL)
    return;
  }
  const bool on = pixel_active(a.slices, a.psf_sums, a.flag, idx);
  // (the table is for the SR iterations' PSF pixels: s != -1 and v_PSF_sums != 0 -- in pass 2 of the Gaussian reconstruction a superset of the
  // flagged ones: v_PSF_sums is never cleared between Gaussian passes, RC.cu:2401-2411)
  if (act) act[i] = pixel_active(a.slices, a.psf_sums, nullptr, idx) ? 1 : 0;
  if (on) {
    const uint32_t sl = idx / (uint32_t)(a.sx * a.sy);
    const float sume = a.psf_sums[idx];
    const float ss = a.simslices[idx];
    float e = a.bias ? a.slices[idx] * expf(-a.bias[idx]) * a.scales[sl] : a.slices[idx] * a.scales[sl];
    if (gauss == 2) {
      e = a.bias[idx];
      const float scale = a.scales[sl];
      if (scale > 0) e -= logf(scale);
      f1 = 1.0f / sume;
    } else if (gauss) {
      f1 = 1.0f / sume;
    } else {
      e = (ss > 0.0f) ? (e - ss) : 0.0f;
      f1 = (a.weights[idx] * a.slice_weights[sl]) / sume;
    }
    f0 = f1 * e;
  }
  recs[i].f0 = f0; recs[i].f1 = f1;
}

// Slot geometry of the cell kernels: a unit's rows sit in the lanes of a SLOT.  Support 16: four slots of 16 lanes.  Support 12
// (patch-based): FIVE slots of 12 lanes (lanes 60..63 idle) instead of four slots with 12 of 16 lanes at work -- 94 % of the
// lanes against 75 %.  Records of a chunk of NSLOT x SL pixels: lane (slot q, row j) holds record NSLOT j + q.
template <int NS> struct SlotGeom {
  static constexpr int SL = NS == 12 ? 12 : 16;
  static constexpr int NSLOT = 64 / SL;
  static constexpr int CH = NSLOT * SL;             // records per chunk (64 or 60)
};
// sum over the SL lanes of a slot, valid in its first lane.  SL == 16: DPP row shifts.  SL == 12: the slots are not DPP rows;
// the same tree as row_sum16 over 12 values and four zeros (what fwd_unit_kernel<.., 12, ..> adds up), by ds_bpermute: the two
// gathers give the same bits.  The byte addresses of the four partners and the two lane tests are worked out once per kernel
// (SlotSum::init), not once per unit: 14 instead of ~50 VALU instructions per unit for the two sums.
template <int SL>
struct SlotSum {
  int a8, a4, a2, a1;
  bool m4, m2;
  __device__ __forceinline__ void init(int lane) {
    const int y = lane % 12;
    a8 = ((lane + 8) & 63) << 2; a4 = ((lane + 4) & 63) << 2; a2 = ((lane + 2) & 63) << 2; a1 = ((lane + 1) & 63) << 2;
    m4 = y < 4; m2 = y < 2;
  }
  __device__ __forceinline__ float sum(float v) const {
    if (SL == 16) return row_sum16(v);
    float t = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(a8, __builtin_bit_cast(int, v)));
    v += m4 ? t : 0.0f;
    t = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(a4, __builtin_bit_cast(int, v)));
    v += m4 ? t : 0.0f;
    t = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(a2, __builtin_bit_cast(int, v)));
    v += m2 ? t : 0.0f;
    t = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(a1, __builtin_bit_cast(int, v)));
    return v + t;
  }
  // the same tree over doubles (pass 1 of the Gaussian reconstruction adds its taps in double, like fwd_unit_kernel<GAUSS1>)
  __device__ __forceinline__ double perm(int addr, double x) const {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, x);
    const unsigned lo = (unsigned)__builtin_amdgcn_ds_bpermute(addr, (int)(unsigned)b), hi = (unsigned)__builtin_amdgcn_ds_bpermute(addr, (int)(unsigned)(b >> 32));
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
  }
  __device__ __forceinline__ double sum(double v) const {
    if (SL == 16) return row_sum16(v);
    double t = perm(a8, v);
    v += m4 ? t : 0.0;
    t = perm(a4, v);
    v += m4 ? t : 0.0;
    t = perm(a2, v);
    v += m2 ? t : 0.0;
    t = perm(a1, v);
    return v + t;
  }
};

#ifndef SVR_CELL_EVAL_H
#define SVR_CELL_EVAL_H(NS) ((NS) / 2)   // pairs of taps evaluated side by side in the cell kernels: the whole row
#endif
#ifndef SVR_CELL_EVAL_H_FWD
#define SVR_CELL_EVAL_H_FWD(NS) SVR_CELL_EVAL_H(NS)   // ... in the gather (experiments: fewer pairs, fewer registers, a fourth wavefront)
#endif
#ifndef SVR_CELL_DMA_DEPTH
#define SVR_CELL_DMA_DEPTH 2   // gather, COEFF == 2: stages of the table's landing area in the LDS (a stage = one unit per slot, 4 KiB); the loads run
#endif                         // DEPTH - 1 steps ahead of their use and DEPTH steps ahead of the LDS reads (P4: 2 -> 2.39 ms, 3 -> 2.44, 4 -> 2.60)
#ifndef SVR_CELL_RING
#define SVR_CELL_RING 2   // table rows in flight per slot (three: 168 VGPRs and 272 bytes of scratch)
#endif
#ifndef SVR_CELL_RING_ASM
#define SVR_CELL_RING_ASM 1   // support-16 table scatter: the ring's loads issued and waited for by the kernel itself (gload16 / gload_wait); 0: the counted ring
#endif
// Wavefronts per SIMD the support-12 (patch-based) instantiations are compiled for.  They need 134-135 VGPRs when left at 3; at 4 the compiler
// fits them into 128 with 48 bytes of scratch in the per-run set-up code (none in the row loop).  The issue rate of packed f32 rises from
// 0.433 to 0.465e9 per SIMD with the fourth wavefront (profiles/r04_issue_rate.txt): the gather takes it (PVR4 8.27 -> 8.03 ms, PVR8spx
// 21.5 -> 20.6 ms); the scatter does not -- its five private boxes hold a CU at 9-13 wavefronts whatever the registers allow, and the
// spills then only cost (PVR4 6.42 -> 6.71 ms, PVR8spx 23.1 -> 24.8 ms): it stays at 3.  Support 16 needs 162-167 VGPRs: 3.
#ifndef SVR_WPE_PVR_FWD
#define SVR_WPE_PVR_FWD 4
#endif
#ifndef SVR_WPE_PVR_BACK
#define SVR_WPE_PVR_BACK 3
#endif
#ifndef SVR_WPE_SVR_FWD
#define SVR_WPE_SVR_FWD SVR_WPE_WAVE
#endif
// COEFF: 0 = every tap evaluated, 1 = every tap of a live unit from the coefficient table, 3 = every tap evaluated AND stored: the pass that writes the table
template <int NS = PSF_SUPPORT, bool PVR = false, int COEFF = 0>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu((NS == 12 ? SVR_WPE_PVR_BACK : SVR_WPE_WAVE), (NS == 12 ? SVR_WPE_PVR_BACK : SVR_WPE_WAVE))))
void back_cell_kernel(PsfArgs a, CellArgs ca, uint32_t b0) {
  constexpr int NC = (NS - 1) / 2, NH = NS - 1 - NC;
  constexpr int SL = SlotGeom<NS>::SL, NSLOT = SlotGeom<NS>::NSLOT, CH = SlotGeom<NS>::CH;
  extern __shared__ __attribute__((aligned(16))) float tile[];
  f2 *box = reinterpret_cast<f2 *>(tile);               // {addon, cmap}: plane P of the quad's four cells, one box per slot
  const int lane = threadIdx.x;
  const VolGeom &vg = a.vg;
  const uint32_t bid = b0 + blockIdx.x;                  // (the entry list goes out in pieces of < 2^32 work-items)
  unsigned long long t_start = 0;
  if (ca.trace) t_start = __builtin_amdgcn_s_memrealtime();
  const uint4 ent = ca.ents[bid];
  const uint32_t item = ent.x;
  const uint32_t rep = ent.y & 0xFFFFu, nparts = ent.y >> 16;     // this wavefront takes every nparts-th run that reaches the plane
  const uint32_t quad = item >> 10;
  const int ci = quad >= (uint32_t)ca.cls[1].cell_base ? 1 : 0;
  const CellClass &C = ca.cls[ci];
  const int P = C.pfirst + (int)(item & 1023u);         // the item's plane (absolute, may be negative: aliases to 0 in the combine)
  const bool swap = ci == 0;                            // the planes are y-planes, lanes run over z
  const int vgy = swap ? vg.vz : vg.vy;
  const int lq = (int)quad - C.cell_base;
  const int ql = lq / C.ncx, qx = lq - ql * C.ncx;
  const int cx0 = C.x0 + qx * ca.CX, cl0 = C.l0 + ql * ca.CL;   // first centre coordinate of the cell
  const int PL = ca.PL, PP = ca.PP;
  const bool idle = lane >= CH;                          // (support 12: lanes 60..63)
  const int slot = idle ? NSLOT - 1 : lane / SL, y = lane % SL;
  const float fyl = (float)(y - NC);
  const int lox = cx0 - NC, loy = cl0 - NC;             // origin of the cell's box (unsaturated coordinates)
  f2 *pb = box + slot * PP - lox;                       // this slot's private copy
  for (int i = lane; i < NSLOT * PP; i += 64) box[i] = (f2){0.0f, 0.0f};
  __syncthreads();

  const uint32_t rfirst = ent.z, r1 = ent.w;
  uint32_t nreach = 0;                                   // runs that reach the plane so far
  for (uint32_t rb = rfirst; rb < r1; rb += 64) {
    // lane = run: does it reach the plane?  (the descriptors stay in the lanes: the walk below reads them with v_readlane)
    CellRun Rl;
    Rl.start = Rl.count = Rl.slice = 0u;
    bool hit = false;
    if (rb + lane < r1) {
      Rl = ca.runs[rb + lane];
      hit = Rl.czmin - NC <= P && Rl.czmax + NH >= P;
    }
    unsigned long long todo = __ballot(hit);
    if (nparts > 1u) {
      const uint32_t ord = nreach + (uint32_t)__popcll(todo & ((1ull << lane) - 1ull));
      nreach += (uint32_t)__popcll(todo);
      todo = __ballot(hit && ord % nparts == rep);
    }
    // the first 64 records of a run are requested while the run before it is evaluated; lane (q, j) takes record 4 j + q:
    // every slot gets every fourth pixel
    const int mine = idle ? 0x7fffffff : NSLOT * y + slot;
    CellRec nrec;
    uint32_t npid = 0u;
    bool nact = false;
    nrec.f0 = nrec.f1 = 0.0f; nrec.cz = 0; nrec.dead = 0;
    auto request_run = [&](int rl) {
      const uint32_t st = (uint32_t)__builtin_amdgcn_readlane((int)Rl.start, rl), cn = (uint32_t)__builtin_amdgcn_readlane((int)Rl.count, rl);
      if ((uint32_t)mine < cn) {
        nrec = ca.recs[st + (uint32_t)mine];
        if (COEFF) npid = ca.pid[st + (uint32_t)mine];
        if (COEFF == 3) nact = ca.act[st + (uint32_t)mine] != 0;
      }
    };
    if (todo) request_run((int)__builtin_ctzll(todo));
    while (todo) {
      const int rl = (int)__builtin_ctzll(todo);
      todo &= todo - 1ull;
      const uint32_t sl = (uint32_t)__builtin_amdgcn_readlane((int)Rl.slice, rl);
      const uint32_t rstart = (uint32_t)__builtin_amdgcn_readlane((int)Rl.start, rl), rcount = (uint32_t)__builtin_amdgcn_readlane((int)Rl.count, rl);
      const SliceConst &S = a.sc[sl];
      const RowConst RC = load_row_const(S);
      for (uint32_t c0 = 0; c0 < rcount; c0 += CH) {
        CellRec r0;
        bool act0 = false;
        int pid0 = 0;
        if (c0 + (uint32_t)mine < rcount) {
          bool on0 = nact;
          if (c0 == 0) { r0 = nrec; pid0 = (int)npid; }
          else {
            r0 = ca.recs[rstart + c0 + (uint32_t)mine];
            if (COEFF) pid0 = (int)ca.pid[rstart + c0 + (uint32_t)mine];
            if (COEFF == 3) on0 = ca.act[rstart + c0 + (uint32_t)mine] != 0;
          }
          // (COEFF == 3: every PSF pixel's units are evaluated and stored; one whose factors are both 0 this time adds 0 to the box)
          act0 = (COEFF == 3 ? on0 : (r0.f0 != 0.0f || r0.f1 != 0.0f)) && r0.cz - NC <= P && r0.cz + NH >= P;
        }
        if (c0 + CH >= rcount && todo) request_run((int)__builtin_ctzll(todo));   // the next run's records, in flight during this chunk
        if (ca.dbg == 2 && lane == 0) atomicAdd(ca.stats + 0, 1ull);
        if (!__any(act0)) continue;
        const bool dead0 = act0 && !PVR && ((r0.dead >> (P - r0.cz + NC)) & 1u);
        const int sh = SL * slot;
        unsigned ml = idle ? 0u : (unsigned)(__ballot(act0 && !dead0) >> sh) & ((1u << SL) - 1u);
        unsigned md = idle ? 0u : (unsigned)(__ballot(dead0) >> sh) & ((1u << SL) - 1u);
        if (ca.dbg == 2) {
          int mx = __popc(ml);
          for (int o = 16; o < 64; o <<= 1) mx = max(mx, __shfl_xor(mx, o, 64));
          if (y == 0 && !idle) { atomicAdd(ca.stats + 3, (unsigned long long)__popc(ml)); atomicAdd(ca.stats + 4, (unsigned long long)__popc(md)); }
          if (lane == 0) { atomicAdd(ca.stats + 1, 1ull); atomicAdd(ca.stats + 2, (unsigned long long)mx); }
        }
        // the words a unit needs: {cx | cl << 16, cz, bx, by, bz, f0, f1, table id}
        const int w0a = (int)((unsigned short)r0.cx | ((unsigned)(unsigned short)r0.cl << 16));
        struct Unit { int cx, cy, cz; float bx, by, bz, f0, f1; int pid; };
        auto fetch = [&](int j) -> Unit {                  // record j (0..15) of this slot, whichever of its lanes holds it
          const int src = slot * SL + (j & 15);
          Unit u;
          const int w0 = __shfl(w0a, src, 64);
          u.cx = (int)(short)(w0 & 0xFFFF); u.cy = w0 >> 16;
          u.cz = __shfl((int)r0.cz, src, 64);
          u.f0 = __shfl(r0.f0, src, 64); u.f1 = __shfl(r0.f1, src, 64);
          u.pid = COEFF ? __shfl(pid0, src, 64) : 0;
          u.bx = u.by = u.bz = 0.0f;
          return u;
        };
        auto fetch_b = [&](int j, Unit &u) {               // ... and its residuals, for the units that are evaluated
          const int src = slot * SL + (j & 15);
          u.bx = __shfl(r0.bx, src, 64); u.by = __shfl(r0.by, src, 64); u.bz = __shfl(r0.bz, src, 64);
        };
        if (ca.dbg == 0) {
          if constexpr (COEFF == 1 && NS == 16 && !PVR && SVR_CELL_RING_ASM) {
            // The support-16 table scatter (§5.1h): two units per slot in flight in a register ring the compiler cannot shorten.  The rows are loaded
            // by gload16 (inline asm, not counted by hipcc: no s_waitcnt of its in front of the ring's readers, no copies of the ring parked behind
            // one at the loop header -- what it makes of the counted ring of the branch below) and the kernel counts its own waits.  One back edge, no
            // break: a trip uses entry 0, reissues it, uses entry 1, reissues it, and EVERY issue is four loads from every lane -- a lane whose slot has
            // no further live unit reads the table's first bytes (as the gather's issue() does) and, its rowok false, writes nothing -- so the number
            // of operations in flight depends neither on the lane nor on the trip.  The units of a slot are taken in the order of the branch below and
            // added with the same fma2 into the same private box: the same bits.
            constexpr int HQ = NS / 4;
            nt_f4 ring[2][HQ];
            Unit ru[2];
            bool rv[2];
            auto issue = [&](Unit &u, bool &valid, nt_f4 (&dst)[HQ]) {
              valid = ml != 0u;
              const int j = valid ? __builtin_ctz(ml) : 0;
              ml &= ml - 1u;
              u = fetch(j);
              const float4 *row = valid ? coeff_row<NS>(a.coeff, (uint32_t)u.pid, P - u.cz + NC, y) : a.coeff + lane;
              gload16<0 * CoeffLayout<NS>::ROW_PITCH * 16>(row, dst[0]);
              gload16<1 * CoeffLayout<NS>::ROW_PITCH * 16>(row, dst[1]);
              gload16<2 * CoeffLayout<NS>::ROW_PITCH * 16>(row, dst[2]);
              gload16<3 * CoeffLayout<NS>::ROW_PITCH * 16>(row, dst[3]);
            };
            // (the ring lives inside this one condition, from its first issue to its drain, and the loop leaves from its bottom only: no path on
            // which the compiler has to carry ring registers next to their successors, which it does by copying them -- while they are in flight)
            if (__any(ml != 0u)) {
            issue(ru[0], rv[0], ring[0]);
            issue(ru[1], rv[1], ring[1]);
            do {
#pragma unroll
              for (int r3 = 0; r3 < 2; ++r3) {
                // this entry's four loads: the other entry's four, issued after them, stay in flight.  The kernel's other vector-memory operations
                // around here are the next run's or chunk's recs / pid loads (request_run); wherever the compiler puts them, an operation younger
                // than the loads waited for makes this wait stricter by itself at most, an older one has returned with them: never looser.
                gload_wait<HQ>(ring[r3]);
                const Unit u = ru[r3];
                const bool valid = rv[r3];
                if (r3 == 0 || __any(valid)) {              // (the odd tail: the last trip has entry 0 only)
                  const int ay = u.cy + y - NC;
                  const bool rowok = valid && ay < vgy;
                  const int rbx = rowok ? (ay - loy) * PL + u.cx - NC : lox;
                  // (the row in two halves -- the accumulators of a whole row next to the ring do not fit 168 registers)
                  constexpr int PARTS = 2, PT = NS / PARTS;
                  const f2 ff = (f2){u.f0, u.f1};
#pragma unroll
                  for (int hq = 0; hq < PARTS; ++hq) {
                    f2 acc[PT];
#pragma unroll
                    for (int x = 0; x < PT; ++x) acc[x] = pb[rbx + hq * PT + x];
                    if (rowok) {
#pragma unroll
                      for (int q = 0; q < PT / 4; ++q) {
                        const nt_f4 c = ring[r3][hq * (PT / 4) + q];
                        pb[rbx + hq * PT + 4 * q] = fma2(bc2(c.x), ff, acc[4 * q]);
                        pb[rbx + hq * PT + 4 * q + 1] = fma2(bc2(c.y), ff, acc[4 * q + 1]);
                        pb[rbx + hq * PT + 4 * q + 2] = fma2(bc2(c.z), ff, acc[4 * q + 2]);
                        pb[rbx + hq * PT + 4 * q + 3] = fma2(bc2(c.w), ff, acc[4 * q + 3]);
                      }
                    }
                  }
                }
                issue(ru[r3], rv[r3], ring[r3]);
              }
            } while (__any(rv[0]));
            // the end of the chunk's lists: the ring is drained (its last two issues carry no unit) before its registers go to anybody else
            gload_wait<0>(ring[0], ring[1]);
            }
          } else if (COEFF == 1) {
            // the taps come from the coefficient table: a ring of RING units per slot in flight (support 12, PVR4: two 5.8 ms, three
            // 6.1 ms, four spill: 9.5 ms)
            constexpr int RING = SVR_CELL_RING;
            float4 ring[RING][NS / 4];
            Unit ru[RING];
            bool rv[RING];
            auto request = [&](Unit &u, bool &valid, float4 (&dst)[NS / 4]) {
              valid = ml != 0u;
              const int j = valid ? __builtin_ctz(ml) : 0;
              ml &= ml - 1u;
              u = fetch(j);
              if (valid) coeff_load_row<NS>(coeff_row<NS>(a.coeff, (uint32_t)u.pid, P - u.cz + NC, y < NS ? y : 0), dst);
            };
#pragma unroll
            for (int r3 = 0; r3 < RING; ++r3) request(ru[r3], rv[r3], ring[r3]);
            while (__any(rv[0])) {
#pragma unroll
              for (int r3 = 0; r3 < RING; ++r3) {
                if (!__any(rv[r3])) break;
                const Unit u = ru[r3];
                const bool valid = rv[r3];
                const int ay = u.cy + y - NC;
                const bool rowok = valid && y < NS && ay < vgy;
                const int rbx = rowok ? (ay - loy) * PL + u.cx - NC : lox;
                // (support 16: the row in two halves -- the accumulators of a whole row next to the ring do not fit 168 registers)
                constexpr int PARTS = NS == 16 ? 2 : 1, PT = NS / PARTS;
                static_assert(PT % 4 == 0, "whole float4 per part");
                const f2 ff = (f2){u.f0, u.f1};
#pragma unroll
                for (int hq = 0; hq < PARTS; ++hq) {
                  f2 acc[PT];
#pragma unroll
                  for (int x = 0; x < PT; ++x) acc[x] = pb[rbx + hq * PT + x];
                  if (rowok) {
#pragma unroll
                    for (int q = 0; q < PT / 4; ++q) {
                      const float4 c = ring[r3][hq * (PT / 4) + q];
                      pb[rbx + hq * PT + 4 * q] = fma2(bc2(c.x), ff, acc[4 * q]);
                      pb[rbx + hq * PT + 4 * q + 1] = fma2(bc2(c.y), ff, acc[4 * q + 1]);
                      pb[rbx + hq * PT + 4 * q + 2] = fma2(bc2(c.z), ff, acc[4 * q + 2]);
                      pb[rbx + hq * PT + 4 * q + 3] = fma2(bc2(c.w), ff, acc[4 * q + 3]);
                    }
                  }
                }
                request(ru[r3], rv[r3], ring[r3]);
              }
            }
          } else {
            // the next unit's record is fetched (seven ds_bpermute) while the current one is evaluated
            bool nvalid = ml != 0u;
            int jn = nvalid ? __builtin_ctz(ml) : 0;
            ml &= ml - 1u;
            Unit un = fetch(jn);
            fetch_b(jn, un);
            while (__any(nvalid)) {
              const bool valid = nvalid;
              const Unit u = un;
              nvalid = ml != 0u;
              jn = nvalid ? __builtin_ctz(ml) : 0;
              ml &= ml - 1u;
              un = fetch(jn);
              fetch_b(jn, un);
              const float fzu = (float)(P - u.cz);
              const int ay = u.cy + y - NC;               // may be negative: aliases to 0 in the combine
              const bool rowok = valid && y < NS && ay < vgy;
              const int rbx = rowok ? (ay - loy) * PL + u.cx - NC : lox;
              float out[NS];
              eval_row_t<NS, PVR, true, SVR_CELL_EVAL_H(NS)>(RC, u.bx, u.by, u.bz, swap ? fzu : fyl, swap ? fyl : fzu, out);
              if (COEFF == 3) {
                // the pass that evaluates writes the coefficient table (fwd_cell_kernel<.., 3> does the same; whichever PSF pass comes first after a
                // new slice geometry -- pass 2 of the Gaussian reconstruction in the reconstruction loop, the scatter in bench.py's steps)
                if (valid && y < NS) coeff_store_row<NS>(coeff_row<NS>(a.coeff, (uint32_t)u.pid, P - u.cz + NC, y), out);
              }
              // all NS x positions are inside the box by construction: unconditional read-add-write (skipped taps add 0);
              // the reads first, together, then the sums, then the writes.  (Issued before the epsilon-walk instead of after it --
              // eval_row_vals, reads, eps_walk -- they change nothing: measured again in round 4, P4 / S8 / PVR4 within 0.3 %.)
              f2 acc[NS];
#pragma unroll
              for (int x = 0; x < NS; ++x) acc[x] = pb[rbx + x];
              if (rowok) {
                const f2 ff = (f2){u.f0, u.f1};
#pragma unroll
                for (int x = 0; x < NS; ++x) acc[x] = fma2(bc2(out[x]), ff, acc[x]);
#pragma unroll
                for (int x = 0; x < NS; ++x) pb[rbx + x] = acc[x];
              }
            }
          }
          if (!PVR) {
            // dead units: the first tap of every row, two units per pass in the two halves of the packed evaluator
            while (__any(md != 0u)) {
              const bool va = md != 0u;
              const int ja = va ? __builtin_ctz(md) : 0;
              md &= md - 1u;
              const bool vb = md != 0u;
              const int jb = vb ? __builtin_ctz(md) : 0;
              md &= md - 1u;
              Unit Ra = fetch(ja), Rb = fetch(jb);
              fetch_b(ja, Ra); fetch_b(jb, Rb);
              const float fua = (float)(P - Ra.cz), fub = (float)(P - Rb.cz);
              const float fya = swap ? fua : fyl, fza = swap ? fyl : fua, fyb = swap ? fub : fyl, fzb = swap ? fyl : fub;
              const f2 rowx = (f2){__builtin_fmaf(RC.Lp[1], fya, __builtin_fmaf(RC.Lp[2], fza, Ra.bx)),
                                   __builtin_fmaf(RC.Lp[1], fyb, __builtin_fmaf(RC.Lp[2], fzb, Rb.bx))};
              const f2 rowy = (f2){__builtin_fmaf(RC.Lp[4], fya, __builtin_fmaf(RC.Lp[5], fza, Ra.by)),
                                   __builtin_fmaf(RC.Lp[4], fyb, __builtin_fmaf(RC.Lp[5], fzb, Rb.by))};
              const f2 rowz = (f2){__builtin_fmaf(RC.Lp[7], fya, __builtin_fmaf(RC.Lp[8], fza, Ra.bz)),
                                   __builtin_fmaf(RC.Lp[7], fyb, __builtin_fmaf(RC.Lp[8], fzb, Rb.bz))};
              f2 xs[1], ys[1], t0[1];
              xs[0] = fma2(bc2(RC.Lp[0]), bc2((float)(-NC)), rowx);
              ys[0] = fma2(bc2(RC.Lp[3]), bc2((float)(-NC)), rowy);
              eval_pairs_xyz<1, false>(RC, xs, ys, t0);
              const f2 v = t0[0] * gauss_first_tap2<NC>(RC, rowz);      // always processed: |FLT_MAX - v| is not <= eps
              const int aya = Ra.cy + y - NC, ayb = Rb.cy + y - NC;
              if (va && aya < vgy) {
                f2 *q = pb + (aya - loy) * PL + Ra.cx - NC;
                *q = fma2(bc2(v.x), (f2){Ra.f0, Ra.f1}, *q);
              }
              if (vb && ayb < vgy) {
                f2 *q = pb + (ayb - loy) * PL + Rb.cx - NC;
                *q = fma2(bc2(v.y), (f2){Rb.f0, Rb.f1}, *q);
              }
            }
          }
        }
      }
    }
  }
  __syncthreads();
  // the four copies are added in a fixed order; the box goes out as plain coalesced rows into the item's own slab
  f2 *dst = ca.stage + (size_t)bid * (size_t)PP;
  for (int i = lane; i < PP; i += 64) {
    f2 v = (box[i] + box[PP + i]) + (box[2 * PP + i] + box[3 * PP + i]);
    if (NSLOT == 5) v = v + box[4 * PP + i];
    dst[i] = v;
  }
  if (ca.trace && lane == 0) {
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    ca.trace[3 * (size_t)bid] = t_start;
    ca.trace[3 * (size_t)bid + 1] = __builtin_amdgcn_s_memrealtime();
    ca.trace[3 * (size_t)bid + 2] = (unsigned long long)hw | (unsigned long long)xcc << 32;
  }
}

// One thread per volume voxel: the slabs that cover it, added in a fixed order; the mask test and the float->uint
// saturation of the reference's scatter (RC.cu:508-510: negative -> 0, beyond the high end -> dropped) are applied here.
// combine_class: the slabs of one class that cover voxel (x, y, z), in the order (plane, lane coordinate, x coordinate, lane cell, x cell, part)
// -- the general form: voxel 0 of an axis sums every staged source coordinate <= 0.
__device__ __forceinline__ f2 combine_class(const CellArgs &ca, const CellClass &C, int c, int x, int y, int z, int NC, int NH, f2 acc) {
  const int Pv = c == 0 ? y : z, Lv = c == 0 ? z : y;
  // source coordinates that land on this voxel: itself, or everything <= 0 for index 0
  const int pa = Pv > 0 ? Pv : min(C.pfirst, 0), pe = Pv > 0 ? Pv : 0;
  const int la = Lv > 0 ? Lv : min(C.l0 - NC, 0), le = Lv > 0 ? Lv : 0;
  const int xa = x > 0 ? x : min(C.x0 - NC, 0), xe = x > 0 ? x : 0;
  for (int Ps = max(pa, C.pfirst); Ps <= min(pe, C.plast); ++Ps) {
    const int g = Ps - C.pfirst;
    for (int Ls = la; Ls <= le; ++Ls) {
      // cells jl with l0 + jl CL - NC <= Ls <= l0 + jl CL + CL - 1 + NH
      const int jlo = max(-floordiv(-(Ls - C.l0 - NH - (ca.CL - 1)), ca.CL), 0);     // ceil
      const int jhi = min(floordiv(Ls - C.l0 + NC, ca.CL), C.ncl * ca.QL - 1);
      // (rows and columns of cells without a run hold no item: skipping them adds the same terms in the same order)
      if (ca.rowcol) {
        bool any = false;
        for (int jl = jlo; jl <= jhi && !any; ++jl) any = ca.rowcol[C.row_base + jl / ca.QL] != 0;
        if (!any) continue;
      }
      for (int Xs = xa; Xs <= xe; ++Xs) {
        const int ilo = max(-floordiv(-(Xs - C.x0 - NH - (ca.CX - 1)), ca.CX), 0);
        const int ihi = min(floordiv(Xs - C.x0 + NC, ca.CX), C.ncx * ca.QX - 1);
        if (ca.rowcol) {
          bool any = false;
          for (int ix = ilo; ix <= ihi && !any; ++ix) any = ca.rowcol[C.col_base + ix / ca.QX] != 0;
          if (!any) continue;
        }
        for (int jl = jlo; jl <= jhi; ++jl)
          for (int ix = ilo; ix <= ihi; ++ix) {
            const uint32_t quad = (uint32_t)(C.cell_base + (jl / ca.QL) * C.ncx + ix / ca.QX);
            const uint32_t it = (uint32_t)ca.item_of[(size_t)quad * ca.ngs + g];
            if (it == 0xFFFFFFFFu) continue;
            const int bl = Ls - (C.l0 + jl * ca.CL - NC), bx = Xs - (C.x0 + ix * ca.CX - NC);
            const uint32_t e0 = it & 0x0FFFFFFFu, np = (it >> 28) + 1u;             // the item's parts, in part order
            for (uint32_t rep = 0; rep < np; ++rep) {
              const f2 v = ca.stage[(size_t)(e0 + rep) * (size_t)ca.PP + (size_t)bl * ca.PL + bx];
              acc = acc + v;
            }
          }
      }
    }
  }
  return acc;
}
__global__ __launch_bounds__(256) void k_cell_combine(CellArgs ca, VolGeom vg, int NC, int NH, const float *mask, float *out0, float *out1) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), z = blockIdx.z;
  if (x >= vg.vx || y >= vg.vy) return;
  const size_t vi = (size_t)x + (size_t)y * vg.vx + (size_t)z * vg.vx * vg.vy;
  f2 acc = (f2){0.0f, 0.0f};
  if (mask[vi] != 0.0f) {
    for (int c = 0; c < 2; ++c) {
      const CellClass &C = ca.cls[c];
      if (C.ng <= 0) continue;
      acc = combine_class(ca, C, c, x, y, z, NC, NH, acc);
    }
  }
  out0[vi] = acc.x;
  out1[vi] = acc.y;
}
// The same sums in the same order with the loads in two batches.  The general form above is a chain of dependent loads per covering
// cell (item_of -> slab: ~12 cells per class, one after the other: S8 0.79 ms, PVR8spx 1.6 ms per pass, and a sharded rank pays the
// whole of it for an eighth of the scatter).  A voxel away from index 0 has ONE source coordinate per axis and at most MJ x MI
// covering cells per class (MJ = (NS - 2) / CL + 2, MI likewise): all their item_of entries are asked for at once, then all their
// slabs, then the values are added in the general form's order.  Voxels on the low faces and items cut into parts take the general
// form (combine_class); cell sizes with more than 4 x 4 covering cells take k_cell_combine.
template <int MJ, int MI>
__global__ __launch_bounds__(256) void k_cell_combine_fast(CellArgs ca, VolGeom vg, int NC, int NH, const float *mask, float *out0, float *out1) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), z = blockIdx.z;
  if (x >= vg.vx || y >= vg.vy) return;
  const size_t vi = (size_t)x + (size_t)y * vg.vx + (size_t)z * vg.vx * vg.vy;
  f2 acc = (f2){0.0f, 0.0f};
  if (mask[vi] != 0.0f) {
    const bool inner = x > 0 && y > 0 && z > 0;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const CellClass &C = ca.cls[c];
      if (C.ng <= 0) continue;
      const int Pv = c == 0 ? y : z, Lv = c == 0 ? z : y;
      if (!inner) { acc = combine_class(ca, C, c, x, y, z, NC, NH, acc); continue; }
      if (Pv < C.pfirst || Pv > C.plast) continue;
      const int g = Pv - C.pfirst;
      const int jlo = max(-floordiv(-(Lv - C.l0 - NH - (ca.CL - 1)), ca.CL), 0);
      const int jhi = min(floordiv(Lv - C.l0 + NC, ca.CL), C.ncl * ca.QL - 1);
      const int ilo = max(-floordiv(-(x - C.x0 - NH - (ca.CX - 1)), ca.CX), 0);
      const int ihi = min(floordiv(x - C.x0 + NC, ca.CX), C.ncx * ca.QX - 1);
      uint32_t it[MJ][MI];
      bool parts = false;
#pragma unroll
      for (int a = 0; a < MJ; ++a)
#pragma unroll
        for (int b = 0; b < MI; ++b) {
          const int jl = jlo + a, ix = ilo + b;
          it[a][b] = 0xFFFFFFFFu;
          if (jl <= jhi && ix <= ihi) it[a][b] = (uint32_t)ca.item_of[(size_t)(C.cell_base + (jl / ca.QL) * C.ncx + ix / ca.QX) * ca.ngs + g];
        }
      f2 v[MJ][MI];
#pragma unroll
      for (int a = 0; a < MJ; ++a)
#pragma unroll
        for (int b = 0; b < MI; ++b) {
          v[a][b] = (f2){0.0f, 0.0f};
          if (it[a][b] != 0xFFFFFFFFu) {
            const int bl = Lv - (C.l0 + (jlo + a) * ca.CL - NC), bx = x - (C.x0 + (ilo + b) * ca.CX - NC);
            v[a][b] = ca.stage[(size_t)(it[a][b] & 0x0FFFFFFFu) * (size_t)ca.PP + (size_t)bl * ca.PL + bx];
            parts = parts || (it[a][b] >> 28) != 0u;
          }
        }
      if (parts || jhi - jlo >= MJ || ihi - ilo >= MI) { acc = combine_class(ca, C, c, x, y, z, NC, NH, acc); continue; }   // (never for the sizes this kernel is launched with)
#pragma unroll
      for (int a = 0; a < MJ; ++a)
#pragma unroll
        for (int b = 0; b < MI; ++b)
          if (it[a][b] != 0xFFFFFFFFu) acc = acc + v[a][b];
    }
  }
  out0[vi] = acc.x;
  out1[vi] = acc.y;
}

// Round 5: the same sums in the same order, one item_of load per WAVEFRONT and class.  A wavefront holds 64 consecutive x of one (y, z):
// the plane and the covering lane cells are the same for all of them and their x cells span at most 16 columns, so the <= 4 x 16
// item_of entries the 64 voxels need between them are ONE load (lane = (lane cell, x cell column)), a voxel's own MJ x MI come out of
// the lanes with ds_bpermute, and a wavefront around which nothing is staged leaves after that one load.  What made this worth doing:
// a rank of a sharded run stages the items of its own slices only, but k_cell_combine_fast walked the whole volume with 2 x 12 loads
// per mask voxel whether or not anything was there -- 0.56 ms on S8 for a rank exactly as for the whole run, 8 x 0.56 ms next to a
// scatter of 8 x 4.7 ms.  Voxels on the low faces and items cut into parts take the general form, like there.
template <int MJ, int MI>
__global__ __launch_bounds__(256) void k_cell_combine_wave(CellArgs ca, VolGeom vg, int NC, int NH, const float *mask, float *out0, float *out1) {
  const int lane = threadIdx.x & 63;
  const int x0 = blockIdx.x * 64, y = blockIdx.y * 4 + (threadIdx.x >> 6), z = blockIdx.z;
  if (y >= vg.vy) return;                                   // (the whole wavefront)
  const int x = x0 + lane;
  const bool inb = x < vg.vx;
  const int xc = inb ? x : vg.vx - 1;
  const size_t vi = (size_t)xc + (size_t)y * vg.vx + (size_t)z * vg.vx * vg.vy;
  const bool m = inb && mask[vi] != 0.0f;
  f2 acc = (f2){0.0f, 0.0f};
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const CellClass &C = ca.cls[c];
    if (C.ng <= 0) continue;
    const int Pv = c == 0 ? y : z, Lv = c == 0 ? z : y;
    if (y == 0 || z == 0) {                                 // a low face: every staged coordinate <= 0 lands here (uniform over the wavefront)
      if (m) acc = combine_class(ca, C, c, x, y, z, NC, NH, acc);
      continue;
    }
    if (Pv < C.pfirst || Pv > C.plast) continue;
    const int g = Pv - C.pfirst;
    const int jlo = max(-floordiv_m(-(Lv - C.l0 - NH - (ca.CL - 1)), ca.CL, ca.mCL, ca.qCL), 0);
    const int jhi = min(floordiv_m(Lv - C.l0 + NC, ca.CL, ca.mCL, ca.qCL), C.ncl - 1);
    const int xl = min(x0 + 63, vg.vx - 1);
    const int IX0 = max(-floordiv_m(-(x0 - C.x0 - NH - (ca.CX - 1)), ca.CX, ca.mCX, ca.qCX), 0);
    const int IX1 = min(floordiv_m(xl - C.x0 + NC, ca.CX, ca.mCX, ca.qCX), C.ncx - 1);
    int itl = -1;
    {
      const int a_ = lane >> 4, b_ = lane & 15;
      if (a_ < MJ && jlo + a_ <= jhi && IX0 + b_ <= IX1) itl = ca.item_of[(size_t)(C.cell_base + (jlo + a_) * C.ncx + IX0 + b_) * ca.ngs + g];
    }
    if (!__any(itl != -1)) continue;                        // nothing staged around these 64 voxels
    const int ilo = max(-floordiv_m(-(xc - C.x0 - NH - (ca.CX - 1)), ca.CX, ca.mCX, ca.qCX), 0);
    const int ihi = min(floordiv_m(xc - C.x0 + NC, ca.CX, ca.mCX, ca.qCX), C.ncx - 1);
    uint32_t it[MJ][MI];
#pragma unroll
    for (int a = 0; a < MJ; ++a)
#pragma unroll
      for (int b = 0; b < MI; ++b) {
        const int col = min(max(ilo + b - IX0, 0), 15);
        const int v = __shfl(itl, a * 16 + col, 64);
        it[a][b] = (jlo + a <= jhi && ilo + b <= ihi) ? (uint32_t)v : 0xFFFFFFFFu;
      }
    if (!m) continue;
    if (x == 0) { acc = combine_class(ca, C, c, x, y, z, NC, NH, acc); continue; }
    f2 v[MJ][MI];
    bool parts = false;
#pragma unroll
    for (int a = 0; a < MJ; ++a)
#pragma unroll
      for (int b = 0; b < MI; ++b) {
        v[a][b] = (f2){0.0f, 0.0f};
        if (it[a][b] != 0xFFFFFFFFu) {
          const int bl = Lv - (C.l0 + (jlo + a) * ca.CL - NC), bx = x - (C.x0 + (ilo + b) * ca.CX - NC);
          v[a][b] = ca.stage[(uint64_t)(it[a][b] & 0x0FFFFFFFu) * (uint64_t)(uint32_t)ca.PP + (uint32_t)(bl * ca.PL + bx)];   // (one v_mad_u64_u32)
          parts = parts || (it[a][b] >> 28) != 0u;
        }
      }
    if (parts || jhi - jlo >= MJ || ihi - ilo >= MI) { acc = combine_class(ca, C, c, x, y, z, NC, NH, acc); continue; }   // (never for the sizes this kernel is launched with)
#pragma unroll
    for (int a = 0; a < MJ; ++a)
#pragma unroll
      for (int b = 0; b < MI; ++b)
        if (it[a][b] != 0xFFFFFFFFu) acc = acc + v[a][b];
  }
  if (inb) {
    out0[vi] = acc.x;
    out1[vi] = acc.y;
  }
}


// ---- the gather over the same items (fwd_mode 2) ------------------------------------------------------------------------
// simulateSlicesKernel3D_tex (RC.cu:298-404) on the cell structures: an item is again (cell, plane); the box holds {V m, m} of
// the cell's plane (one copy, read only: 3.6 KiB of LDS, the registers set the occupancy), the wavefront walks the runs that
// reach the plane, a slot evaluates a (pixel, plane) unit and leaves its partial sums {sum psf V m, sum psf m} in the pixel's
// row of a staging array; k_cell_gather_finish adds a pixel's partial sums in unit order.  Per unit and per pixel the
// operations and their order are fwd_unit_kernel's (x taps in order, the DPP tree over the 16 rows, units 0 .. NS-1), so the
// simulated slices are the same bits; what goes is the workgroup: no barrier between fill, evaluation and reduction, no
// wavefront waiting for the slowest of eight, and the box is filled once per (cell, plane) instead of once per slice tile.
__global__ void k_cell_gfactors(PsfArgs a, const CellRec *recs, uint32_t n, float *gf) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t idx = recs[i].idx;
  gf[i] = pixel_active(a.slices, a.psf_sums, a.flag, idx) ? 1.0f / a.psf_sums[idx] : 0.0f;   // 0: not a PSF pixel (1 / sume is never 0)
}

// G1: pass 1 of the Gaussian reconstruction on the same walk (gaussianReconstructionKernel3D_tex RC.cu:228-258; what fwd_unit_kernel<GAUSS1>
// does per slice tile): the box holds {in bounds, in mask}, a unit leaves its sum of psf over the in-bounds taps -- added in double in
// fwd_unit_kernel's order: x taps, the tree over the rows -- with the sign bit set when a processed tap fell on a mask voxel (the sums
// are >= 0 or NaN); k_cell_gauss1_finish adds a pixel's units in order and applies the gate.  The same bits as the tile kernel.
#ifndef SVR_WPE_DMA
#define SVR_WPE_DMA 4       // the table's gather through the LDS (COEFF == 2): 89 VGPRs
#endif
template <int NS = PSF_SUPPORT, bool PVR = false, int COEFF = 0, bool G1 = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu((NS == 12 ? SVR_WPE_PVR_FWD : COEFF == 2 ? SVR_WPE_DMA : SVR_WPE_SVR_FWD), (NS == 12 ? SVR_WPE_PVR_FWD : COEFF == 2 ? SVR_WPE_DMA : SVR_WPE_SVR_FWD))))
void fwd_cell_kernel(PsfArgs a, CellArgs ca, const float *gf, f2 *part, uint32_t npart, uint32_t b0) {
  static_assert(!(G1 && COEFF), "pass 1 with the coefficient table stays on fwd_unit_kernel");
  // COEFF: 0 = every tap evaluated, 1 = the table's rows through a ring of registers (support 12), 2 = through the LDS (support 16, LDS-DMA),
  // 3 = every tap evaluated AND stored: the pass that builds the table (round 6)
  double *partd = reinterpret_cast<double *>(part);
  constexpr int NC = (NS - 1) / 2, NH = NS - 1 - NC;
  constexpr int SL = SlotGeom<NS>::SL, NSLOT = SlotGeom<NS>::NSLOT, CH = SlotGeom<NS>::CH;
  extern __shared__ __attribute__((aligned(16))) float tile[];
  f2 *box = reinterpret_cast<f2 *>(tile);               // {V m, m} of the cell's box on plane P
  const int lane = threadIdx.x;
  const VolGeom &vg = a.vg;
  const uint32_t bid = b0 + blockIdx.x;
  const uint4 ent = ca.ents[bid];
  const uint32_t item = ent.x;
  const uint32_t rep = ent.y & 0xFFFFu, nparts = ent.y >> 16;
  const uint32_t quad = item >> 10;
  const int ci = quad >= (uint32_t)ca.cls[1].cell_base ? 1 : 0;
  const CellClass &C = ca.cls[ci];
  const int P = C.pfirst + (int)(item & 1023u);
  const bool swap = ci == 0;                            // the planes are y-planes, lanes run over z
  const int vgy = swap ? vg.vz : vg.vy;
  const int lq = (int)quad - C.cell_base;
  const int ql = lq / C.ncx, qx = lq - ql * C.ncx;
  const int lox = C.x0 + qx * ca.CX - NC, loy = C.l0 + ql * ca.CL - NC;
  const int PL = ca.PL, PP = ca.PP;
  const bool idle = lane >= CH;                          // (support 12: lanes 60..63)
  const int slot = idle ? NSLOT - 1 : lane / SL, y = lane % SL;
  const float fyl = (float)(y - NC);
  SlotSum<SL> ssum;
  ssum.init(lane);
  {
    // the box: the float->uint saturation of the reference (negative -> 0, RC.cu:382) is applied here; beyond the high end: 0
    const uint32_t sty = swap ? (uint32_t)(vg.vx * vg.vy) : (uint32_t)vg.vx, stz = swap ? (uint32_t)vg.vx : (uint32_t)(vg.vx * vg.vy);
    const uint32_t zoff = sat0(P) * stz;
    RowWalk w;
    w.init(lane, 64, PL);
    for (int i = lane; i < PP; i += 64, w.step()) {
      const int gx = w.x + lox, gy = w.y + loy;
      f2 v = (f2){0.0f, 0.0f};
      if (gx < vg.vx && gy < vgy) {
        const uint32_t vi = sat0(gx) + sat0(gy) * sty + zoff;
        if (G1) {
          v = (f2){1.0f, a.mask[vi] != 0.0f ? 1.0f : 0.0f};
        } else if (!PVR || a.volm) {                       // (patch-based: the texture average, packed once per pass)
          const float2 t = a.volm[vi];
          v = (f2){t.x, t.y};
        } else {
          const float m = a.mask[vi] != 0.0f ? 1.0f : 0.0f;
          const int X = (int)sat0(gx), L = (int)sat0(gy), Z = (int)sat0(P);
          v = (f2){m != 0.0f ? pvr_tex(a.vol, vg, X, swap ? Z : L, swap ? L : Z) : 0.0f, m};
        }
      }
      box[i] = v;
    }
  }
  __syncthreads();
  const f2 *pb = box - lox;
  // COEFF == 2: the landing area of the table's rows behind the box, SVR_CELL_DMA_DEPTH stages of [quad][lane] float4 (lane-linear: LDS-DMA)
  const float4 *stage = reinterpret_cast<const float4 *>(tile + 2 * ((PP + 1) & ~1)) + lane;
  const uint32_t stage_lds = COEFF == 2 ? (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_addr_of(tile + 2 * ((PP + 1) & ~1))) : 0u;

  const uint32_t rfirst = ent.z, r1 = ent.w;
  uint32_t nreach = 0;
  for (uint32_t rb = rfirst; rb < r1; rb += 64) {
    CellRun Rl;
    Rl.start = Rl.count = Rl.slice = 0u;
    bool hit = false;
    if (rb + lane < r1) {
      Rl = ca.runs[rb + lane];
      hit = Rl.czmin - NC <= P && Rl.czmax + NH >= P;
    }
    unsigned long long todo = __ballot(hit);
    if (nparts > 1u) {
      const uint32_t ord = nreach + (uint32_t)__popcll(todo & ((1ull << lane) - 1ull));
      nreach += (uint32_t)__popcll(todo);
      todo = __ballot(hit && ord % nparts == rep);
    }
    const int mine = idle ? 0x7fffffff : NSLOT * y + slot;
    CellRec nrec;
    float ngf = 0.0f;
    uint32_t npid = 0u;
    nrec.cz = 0; nrec.dead = 0;
    auto request_run = [&](int rl) {
      const uint32_t st = (uint32_t)__builtin_amdgcn_readlane((int)Rl.start, rl), cn = (uint32_t)__builtin_amdgcn_readlane((int)Rl.count, rl);
      if ((uint32_t)mine < cn) { nrec = ca.recs[st + (uint32_t)mine]; ngf = G1 ? 1.0f : gf[st + (uint32_t)mine]; if (COEFF) npid = ca.pid[st + (uint32_t)mine]; }
    };
    if (todo) request_run((int)__builtin_ctzll(todo));
    while (todo) {
      const int rl = (int)__builtin_ctzll(todo);
      todo &= todo - 1ull;
      const uint32_t sl = (uint32_t)__builtin_amdgcn_readlane((int)Rl.slice, rl);
      const uint32_t rstart = (uint32_t)__builtin_amdgcn_readlane((int)Rl.start, rl), rcount = (uint32_t)__builtin_amdgcn_readlane((int)Rl.count, rl);
      const SliceConst &S = a.sc[sl];
      const RowConst RC = load_row_const(S);
      for (uint32_t c0 = 0; c0 < rcount; c0 += CH) {
        CellRec r0;
        float g0 = 0.0f;
        bool act0 = false;
        int pid0 = 0;
        if (c0 + (uint32_t)mine < rcount) {
          if (c0 == 0) { r0 = nrec; g0 = ngf; pid0 = (int)npid; }
          else { r0 = ca.recs[rstart + c0 + (uint32_t)mine]; g0 = G1 ? 1.0f : gf[rstart + c0 + (uint32_t)mine]; if (COEFF) pid0 = (int)ca.pid[rstart + c0 + (uint32_t)mine]; }
          act0 = g0 != 0.0f && r0.cz - NC <= P && r0.cz + NH >= P;
        }
        if (c0 + CH >= rcount && todo) request_run((int)__builtin_ctzll(todo));
        if (!__any(act0)) continue;
        const bool dead0 = act0 && !PVR && ((r0.dead >> (P - r0.cz + NC)) & 1u);
        const int sh = SL * slot;
        unsigned ml = idle ? 0u : (unsigned)(__ballot(act0 && !dead0) >> sh) & ((1u << SL) - 1u);
        unsigned md = idle ? 0u : (unsigned)(__ballot(dead0) >> sh) & ((1u << SL) - 1u);
        const int w0a = (int)((unsigned short)r0.cx | ((unsigned)(unsigned short)r0.cl << 16));
        const uint32_t myrec = rstart + c0 + (uint32_t)mine;
        struct Unit { int cx, cy, cz; float bx, by, bz; uint32_t rec; int pid; };
        auto fetch = [&](int j) -> Unit {
          const int src = slot * SL + (j & 15);
          Unit u;
          const int w0 = __shfl(w0a, src, 64);
          u.cx = (int)(short)(w0 & 0xFFFF); u.cy = w0 >> 16;
          u.cz = __shfl((int)r0.cz, src, 64);
          u.bx = __shfl(r0.bx, src, 64); u.by = __shfl(r0.by, src, 64); u.bz = __shfl(r0.bz, src, 64);
          u.rec = (uint32_t)__shfl((int)myrec, src, 64);
          u.pid = COEFF ? __shfl(pid0, src, 64) : 0;
          return u;
        };
        if (COEFF == 2) {
          // Round 6: the table's rows travel HBM -> LDS by LDS-DMA (glds16: global_load_lds_dwordx4), DD - 1 steps ahead of their use; a step = the
          // next live unit of each slot.  No VGPR is a load's destination: nothing the compiler can park in copies behind s_waitcnt vmcnt(0) (what it
          // does with the ring of the loop below), 89 registers instead of 168, four wavefronts per SIMD, and the kernel counts the loads in flight
          // itself (glds_wait).  P4: 2.84 ms (fwd_unit_kernel<.., COEFF> on slice tiles, the table's gather until round 5) -> 2.39 ms = 5.9 TB/s.
          static_assert(COEFF != 2 || NS == 16, "the landing stages are laid out for support 16");
          constexpr int DD = SVR_CELL_DMA_DEPTH, HQ = NS / 4;
          unsigned mli = ml;                                 // the issue cursor runs DD - 1 steps ahead of ml
          int s_issue = 0, s_use = 0;
          auto issue = [&]() -> bool {
            const bool vi = mli != 0u;
            if (!__any(vi)) return false;
            const int j = vi ? __builtin_ctz(mli) : 0;
            mli &= mli - 1u;
            const int src = slot * SL + (j & 15);
            const int pid = __shfl(pid0, src, 64), czk = __shfl((int)r0.cz, src, 64);
            // (lanes without a unit read the table's first bytes into their part of the stage: the loads are issued whatever the lanes hold, so
            // that the wavefront's count of operations in flight does not depend on them)
            const float4 *srcp = vi ? coeff_row<NS>(a.coeff, (uint32_t)pid, P - czk + NC, y) : a.coeff + lane;
            coeff_dma_row<NS>(srcp, stage_lds + (uint32_t)s_issue * CoeffLayout<NS>::STAGE_BYTES);
            s_issue = s_issue + 1 == DD ? 0 : s_issue + 1;
            return true;
          };
#pragma unroll
          for (int k = 0; k < DD - 1; ++k) issue();
          // (the next unit's record travels -- ds_bpermute -- while this one is added up, like on the fly)
          bool nvalid = ml != 0u;
          int jn = nvalid ? __builtin_ctz(ml) : 0;
          ml &= ml - 1u;
          Unit un = fetch(jn);
          while (__any(nvalid)) {
            const bool ahead = issue();                      // the step DD - 1 ahead (if the lists go that far)
            const bool valid = nvalid;
            const Unit u = un;
            nvalid = ml != 0u;
            jn = nvalid ? __builtin_ctz(ml) : 0;
            ml &= ml - 1u;
            un = fetch(jn);
            const int ay = u.cy + y - NC;
            const bool rowok = valid && ay < vgy;
            f2 acc = (f2){0.0f, 0.0f};
            {
              const f2 *q = pb + (rowok ? (ay - loy) * PL + u.cx - NC : lox);
              // this step's stage: DD - 1 younger steps of HQ loads each stay in flight (or, at the end of the lists, everything is waited for).
              // The wavefront's own stores (one per step, younger than the loads waited for) only make the count stricter: vmcnt is in order.
              if (ahead) glds_wait<(DD - 1) * HQ>(); else glds_wait<0>();
              const float4 *st = stage + s_use * (HQ * CoeffLayout<NS>::STAGE_QUAD_F4);
              s_use = s_use + 1 == DD ? 0 : s_use + 1;
#pragma unroll
              for (int qq = 0; qq < HQ; ++qq) {
                const float4 c = st[qq * CoeffLayout<NS>::STAGE_QUAD_F4];
                acc = fma2(bc2(c.x), q[4 * qq], acc);
                acc = fma2(bc2(c.y), q[4 * qq + 1], acc);
                acc = fma2(bc2(c.z), q[4 * qq + 2], acc);
                acc = fma2(bc2(c.w), q[4 * qq + 3], acc);
              }
            }
            if (!rowok) acc = (f2){0.0f, 0.0f};
            acc.x = ssum.sum(acc.x); acc.y = ssum.sum(acc.y);
            if (valid && y == 0) part[(size_t)(P - u.cz + NC) * npart + u.rec] = acc;
          }
        } else if (COEFF == 1) {
          // the taps come from the coefficient table (what eval_row_t returns, written by k_coeff_build): two units per slot in flight
          constexpr int RING = SVR_CELL_RING;
          float4 ring[RING][NS / 4];
          Unit ru[RING];
          bool rv[RING];
          auto request = [&](Unit &u, bool &valid, float4 (&dst)[NS / 4]) {
            valid = ml != 0u;
            const int j = valid ? __builtin_ctz(ml) : 0;
            ml &= ml - 1u;
            u = fetch(j);
            if (valid) coeff_load_row<NS>(coeff_row<NS>(a.coeff, (uint32_t)u.pid, P - u.cz + NC, y < NS ? y : 0), dst);
          };
#pragma unroll
          for (int r3 = 0; r3 < RING; ++r3) request(ru[r3], rv[r3], ring[r3]);
          while (__any(rv[0])) {
#pragma unroll
            for (int r3 = 0; r3 < RING; ++r3) {
              if (!__any(rv[r3])) break;
              const Unit u = ru[r3];
              const bool valid = rv[r3];
              const int ay = u.cy + y - NC;
              const bool rowok = valid && y < NS && ay < vgy;
              f2 acc = (f2){0.0f, 0.0f};
              {
                const f2 *q = pb + (rowok ? (ay - loy) * PL + u.cx - NC : lox);
#pragma unroll
                for (int qq = 0; qq < NS / 4; ++qq) {
                  const float4 c = ring[r3][qq];
                  acc = fma2(bc2(c.x), q[4 * qq], acc);
                  acc = fma2(bc2(c.y), q[4 * qq + 1], acc);
                  acc = fma2(bc2(c.z), q[4 * qq + 2], acc);
                  acc = fma2(bc2(c.w), q[4 * qq + 3], acc);
                }
              }
              request(ru[r3], rv[r3], ring[r3]);
              if (!rowok) acc = (f2){0.0f, 0.0f};
              acc.x = ssum.sum(acc.x); acc.y = ssum.sum(acc.y);
              if (valid && y == 0) part[(size_t)(P - u.cz + NC) * npart + u.rec] = acc;
            }
          }
        }
        if (COEFF == 0 || COEFF == 3) {
        // the next unit's record travels (ds_bpermute) while this one is evaluated
        bool nvalid = ml != 0u;
        int jn = nvalid ? __builtin_ctz(ml) : 0;
        ml &= ml - 1u;
        Unit un = fetch(jn);
        while (__any(nvalid)) {
          const bool valid = nvalid;
          const Unit u = un;
          nvalid = ml != 0u;
          jn = nvalid ? __builtin_ctz(ml) : 0;
          ml &= ml - 1u;
          un = fetch(jn);
          const float fzu = (float)(P - u.cz);
          const int ay = u.cy + y - NC;
          const bool rowok = valid && y < NS && ay < vgy;
          float out[NS];
          eval_row_t<NS, PVR, true, SVR_CELL_EVAL_H_FWD(NS)>(RC, u.bx, u.by, u.bz, swap ? fzu : fyl, swap ? fyl : fzu, out);
          if (COEFF == 3) {
            // Round 6: the pass that evaluates WRITES the table (what k_coeff_build writes: the unit's taps as [tap quad][row] float4): the first
            // gather after a new slice geometry is CoeffInit (irtkReconstruction::CoeffInit, RG.cc:2617-2673), and the evaluation it needs anyway
            // is the table's -- no second evaluation of every tap, the stores leave while the next unit is evaluated
            if (valid && y < NS) coeff_store_row<NS>(coeff_row<NS>(a.coeff, (uint32_t)u.pid, P - u.cz + NC, y), out);
          }
          f2 acc = (f2){0.0f, 0.0f};
          double accd = 0.0;
          bool hit = false;
          {
            const f2 *q = pb + (rowok ? (ay - loy) * PL + u.cx - NC : lox);
            f2 v[NS];
#pragma unroll
            for (int x = 0; x < NS; ++x) v[x] = q[x];
#pragma unroll
            for (int x = 0; x < NS; ++x) {
              if (G1) {
                accd += (double)(out[x] * v[x].x);                   // RC.cu:241-245 (in bounds, no mask test)
                hit = hit | ((v[x].y != 0.0f) & (__float_as_uint(out[x]) != 0x80000000u));   // processed, on a mask voxel
              } else {
                acc = fma2(bc2(out[x]), v[x], acc);
              }
            }
          }
          if (G1) {
            if (!rowok) { accd = 0.0; hit = false; }
            accd = ssum.sum(accd);
            const bool anyhit = idle ? false : (((uint32_t)(__ballot(hit) >> (SL * slot)) & ((1u << SL) - 1u)) != 0u);
            if (valid && y == 0) partd[(size_t)(P - u.cz + NC) * npart + u.rec] = anyhit ? -accd : accd;
          } else {
            if (!rowok) acc = (f2){0.0f, 0.0f};
            acc.x = ssum.sum(acc.x); acc.y = ssum.sum(acc.y);
            if (valid && y == 0) part[(size_t)(P - u.cz + NC) * npart + u.rec] = acc;
          }
        }
        }
        if (!PVR) {
          while (__any(md != 0u)) {
            const bool va = md != 0u;
            const int ja = va ? __builtin_ctz(md) : 0;
            md &= md - 1u;
            const bool vb = md != 0u;
            const int jb = vb ? __builtin_ctz(md) : 0;
            md &= md - 1u;
            const Unit Ra = fetch(ja), Rb = fetch(jb);
            const float fua = (float)(P - Ra.cz), fub = (float)(P - Rb.cz);
            const float fya = swap ? fua : fyl, fza = swap ? fyl : fua, fyb = swap ? fub : fyl, fzb = swap ? fyl : fub;
            const f2 rowx = (f2){__builtin_fmaf(RC.Lp[1], fya, __builtin_fmaf(RC.Lp[2], fza, Ra.bx)),
                                 __builtin_fmaf(RC.Lp[1], fyb, __builtin_fmaf(RC.Lp[2], fzb, Rb.bx))};
            const f2 rowy = (f2){__builtin_fmaf(RC.Lp[4], fya, __builtin_fmaf(RC.Lp[5], fza, Ra.by)),
                                 __builtin_fmaf(RC.Lp[4], fyb, __builtin_fmaf(RC.Lp[5], fzb, Rb.by))};
            const f2 rowz = (f2){__builtin_fmaf(RC.Lp[7], fya, __builtin_fmaf(RC.Lp[8], fza, Ra.bz)),
                                 __builtin_fmaf(RC.Lp[7], fyb, __builtin_fmaf(RC.Lp[8], fzb, Rb.bz))};
            f2 xs[1], ys[1], t0[1];
            xs[0] = fma2(bc2(RC.Lp[0]), bc2((float)(-NC)), rowx);
            ys[0] = fma2(bc2(RC.Lp[3]), bc2((float)(-NC)), rowy);
            eval_pairs_xyz<1, false>(RC, xs, ys, t0);
            const f2 v = t0[0] * gauss_first_tap2<NC>(RC, rowz);
            const int aya = Ra.cy + y - NC, ayb = Rb.cy + y - NC;
            f2 wa = (f2){0.0f, 0.0f}, wb = (f2){0.0f, 0.0f};
            if (va && aya < vgy) wa = pb[(aya - loy) * PL + Ra.cx - NC];
            if (vb && ayb < vgy) wb = pb[(ayb - loy) * PL + Rb.cx - NC];
            f2 acca = bc2(v.x) * wa, accb = bc2(v.y) * wb;
            if (G1) {
              double da = row_sum16((double)acca.x), db = row_sum16((double)accb.x);
              const bool anya = ((uint32_t)(__ballot(wa.y != 0.0f) >> (16 * slot)) & 0xFFFFu) != 0u;   // the processed first tap lands on a mask voxel
              const bool anyb = ((uint32_t)(__ballot(wb.y != 0.0f) >> (16 * slot)) & 0xFFFFu) != 0u;
              if (y == 0) {
                if (va) partd[(size_t)(P - Ra.cz + NC) * npart + Ra.rec] = anya ? -da : da;
                if (vb) partd[(size_t)(P - Rb.cz + NC) * npart + Rb.rec] = anyb ? -db : db;
              }
            } else {
              acca.x = row_sum16(acca.x); acca.y = row_sum16(acca.y);
              accb.x = row_sum16(accb.x); accb.y = row_sum16(accb.y);
              if (y == 0) {
                if (va) part[(size_t)(P - Ra.cz + NC) * npart + Ra.rec] = acca;
                if (vb) part[(size_t)(P - Rb.cz + NC) * npart + Rb.rec] = accb;
              }
            }
          }
        }
      }
    }
  }
}

// a pixel's partial sums in unit order, then simulateSlicesKernel3D_tex's tail (RC.cu:396-403).  A unit whose plane lies beyond the
// volume took no part (fwd_unit_kernel: `inb`): its slot of the staging row was never written and is not read.
template <int NS>
__global__ void k_cell_gather_finish(PsfArgs a, CellArgs ca, const CellRec *recs, const float *gf, const f2 *part, uint32_t n) {
  constexpr int NC = (NS - 1) / 2;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float f1 = gf[i];
  if (f1 == 0.0f) return;
  const CellRec R = recs[i];
  const uint32_t sl = R.idx / (uint32_t)(a.sx * a.sy);
  const int plast = ca.cls[a.sc[sl].own == 1 ? 0 : 1].plast;
  f2 sm = (f2){0.0f, 0.0f};
  for (int u = 0; u < NS; ++u)
    if (R.cz + u - NC <= plast) sm = sm + part[(size_t)u * n + i];
  const float w = sm.y * f1;
  if (w > 0.0f) {
    a.simslices[R.idx] = sm.x / sm.y;
    a.simweights[R.idx] = w;
    a.siminside[R.idx] = 1;
    a.slice_inside[sl] = 1;                                // (k_slice_inside's answer: raised where a pixel's flag is; cleared with siminside)
  }
}

// pass 1's tail (fwd_unit_kernel<GAUSS1>'s: RC.cu:251-258, 291-294; patch-based: R2/patchBasedPSFReconstruction_gpu.cu:95-110)
template <int NS, bool PVR>
__global__ void k_cell_gauss1_finish(PsfArgs a, CellArgs ca, const CellRec *recs, const double *partd, uint32_t n) {
  constexpr int NC = (NS - 1) / 2;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const CellRec R = recs[i];
  const uint32_t idx = R.idx;
  const uint32_t sl = idx / (uint32_t)(a.sx * a.sy);
  const int plast = ca.cls[a.sc[sl].own == 1 ? 0 : 1].plast;
  double sd = 0.0;
  bool inside = false;
  for (int u = 0; u < NS; ++u)
    if (R.cz + u - NC <= plast) {
      const double p = partd[(size_t)u * n + i];
      sd += __builtin_fabs(p);
      inside = inside || __builtin_signbit(p);
    }
  float sume = (float)sd;
  bool pass = sume > 0.5f;                                // also drops NaN (RC.cu:251-258)
  if (PVR) {
    const uint32_t rem = idx % (uint32_t)(a.sx * a.sy);
    const uint32_t ppx = rem % (uint32_t)a.sx, ppy = rem / (uint32_t)a.sx;
    if (a.spx && a.spx[(size_t)sl * 4096 + ppx + 64 * ppy] != '1') sume = 0.0f;   // superpixel test of pass 1
    pass = (sume > 0.00001f) || (sume != sume);
  }
  a.flag_out[idx] = pass ? 1 : 0;
  if (pass) {
    a.psf_sums[idx] = sume;
    if (inside) a.voxcount[idx] = 1;                      // RC.cu:291-294
  }
}

// (Re)build the cell structures for the current slice geometry.  On anything the layout cannot hold (centres beyond +-32000: the records
// keep them as shorts; more than 1024 planes in a class, 2^18 cells or more, more than 16384 pixels of one slice in one cell around one
// band of planes, a slice grid of more than 2^20 pixels, more than 2^17 slices: the fields of items[] and of the sort key; LDS boxes
// beyond 64 KiB; a staging buffer that does not fit) the state is marked unusable and the caller takes the tile kernels -- the atomic
// flush of back_mode 4, fwd_unit_kernel, the tile form of pass 1 (cells_or_fallback).
//
// The cell size follows the density of slice pixels in the volume, d = voxel area / pixel area in the slice plane: a run (the
// pixels of one slice in one cell) should fill the records of the 64 (60) lanes.  Measured (scatter / gather, ms; DESIGN 5.1c):
// P4 (d = 0.7) 6x4 3.88 / 3.50, 8x6 4.12 / 3.47; S8 (d = 0.56) 6x4 38.3 / 38.2, 10x6 37.2 / 32.9, 16x8 40.9 / 31.9; PVR4 (d = 0.7)
// 6x4 9.8 / 9.9, 8x6 9.4 / 9.3, 14x9 - / 10.6; PVR8spx (d = 0.25) 6x4 38.1 / 37.2, 12x8 27.3 / 23.5, 16x12 32.1 / 21.8.  The scatter
// keeps one private box per slot in the LDS and stops gaining earlier than the gather, which keeps one: the gather works on
// larger cells, from a second set of lists (same code, another size).  Areas: scatter 24 / d voxels (28 / d for the smaller
// boxes of support 12), at most 96; gather 32 / d^1.35, at most 192 (the finer the volume the more it gains); sides 3 : 2.
// Within +-30 % of these areas the times move by 1-3 %, which is also what two runs of the same size differ by.
void cell_auto_size(const svr_ctx *ctx, bool gather, int &cw, int &ch) {
  double d = 1.0;
  if (ctx->slice_dims.size() >= 3 && ctx->slice_dims[0] > 0 && ctx->slice_dims[1] > 0)
    d = (double)ctx->vdim[0] * ctx->vdim[1] / ((double)ctx->slice_dims[0] * ctx->slice_dims[1]);
  d = std::min(1.0, std::max(d, 0.0625));
  const double area = gather ? std::min(192.0, 32.0 / std::pow(d, 1.35)) : std::min(96.0, (ctx->pvr ? 28.0 : 24.0) / d);
  cw = std::min(16, std::max(2, (int)std::lround(std::sqrt(1.5 * area))));
  ch = std::min(16, std::max(2, (int)std::lround(area / cw)));
  // the box pitch is (cw + support - 1) | 1: an odd width pays for the next even one's box -- take it (same LDS, 14 % more cell: P4's
  // scatter 7 x 5 -> 8 x 5 3.19 -> 3.13 ms, round 4)
  if ((cw & 1) && cw < 16) ++cw;
}
void cell_sizes(const svr_ctx *ctx, int &sw, int &sh, int &gw, int &gh) {
  cell_auto_size(ctx, false, sw, sh);
  cell_auto_size(ctx, true, gw, gh);
  if (ctx->cell_w > 0) sw = gw = ctx->cell_w;           // an explicit size holds for both (svr_set_option cell_w / cell_h) ...
  if (ctx->cell_h > 0) sh = gh = ctx->cell_h;
  if (ctx->cell_gw > 0) gw = ctx->cell_gw;             // ... unless the gather has one of its own (cell_gw / cell_gh)
  if (ctx->cell_gh > 0) gh = ctx->cell_gh;
}

int cell_prepare_state(svr_ctx *ctx, CellState *&slot, int cell_w, int cell_h, bool need_stage);
// the scatter's lists (and the gather's when both work on the same cell size)
int cell_prepare(svr_ctx *ctx) {
  int sw, sh, gw, gh;
  cell_sizes(ctx, sw, sh, gw, gh);
  return cell_prepare_state(ctx, ctx->cell, sw, sh, true);
}
// the gather's lists -> cs (ctx->cell when the sizes agree, else a second state of its own without a staging buffer)
int cell_prepare_gather(svr_ctx *ctx, CellState *&cs) {
  int sw, sh, gw, gh;
  cell_sizes(ctx, sw, sh, gw, gh);
  int r;
  if (gw == sw && gh == sh) {
    if ((r = cell_prepare_state(ctx, ctx->cell, sw, sh, true))) return r;
    cs = ctx->cell;
    return SVR_OK;
  }
  if ((r = cell_prepare_state(ctx, ctx->cell_g, gw, gh, false))) return r;
  cs = ctx->cell_g;
  return SVR_OK;
}

int cell_prepare_state(svr_ctx *ctx, CellState *&slot, int cell_w, int cell_h, bool need_stage) {
  if (!slot) slot = new CellState();
  CellState &cs = *slot;
  if (cs.valid && cs.a.CX == cell_w && cs.a.CL == cell_h) return SVR_OK;
  cs.usable = false;
  cs.pid_valid = false;
  cs.gf_valid = false;
  const bool dbg = getenv("SVR_TUNE_DEBUG") != nullptr;
  auto t_last = std::chrono::steady_clock::now();
  auto mark = [&](const char *what) {
    if (!dbg) return;
    (void)hipStreamSynchronize(ctx->stream);
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "[cell prepare] %-28s %7.2f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
    t_last = now;
  };
  const int NS = ctx->pvr ? PVR_N : PSF_SUPPORT, NC = (NS - 1) / 2, NH = NS - 1 - NC;
  const uint32_t n = ctx->n_active;
  if (!n) { cs.valid = true; return SVR_OK; }
  if ((uint64_t)ctx->sx * ctx->sy > (1u << 20) || ctx->ns > (1u << 17)) { cs.valid = true; return SVR_OK; }   // the sort key's fields
  PsfArgs a = make_args(ctx);
  a.list = ctx->d_active;
  a.n = n;
  HIPCHK(cs.d_keys.reserve(n));
  HIPCHK(cs.d_keys2.reserve(n));
  HIPCHK(cs.d_head.reserve(n));
  HIPCHK(cs.d_runid.reserve(n));
  HIPCHK(cs.d_recs.reserve(n));
  HIPCHK(cs.d_range.reserve(16));
  int hr[16];
  for (int c = 0; c < 2; ++c) for (int k = 0; k < 3; ++k) { hr[6 * c + 2 * k] = INT_MAX; hr[6 * c + 2 * k + 1] = INT_MIN; }
  hr[12] = hr[13] = hr[14] = hr[15] = 0;
  HIPCHK(hipMemcpyAsync(cs.d_range, hr, sizeof(hr), hipMemcpyHostToDevice, ctx->stream));
  // the centres and their ranges do not depend on the cell size: the scatter's and the gather's lists share one pass (invalidate
  // drops it with the lists)
  if (!ctx->cellc_valid || ctx->cellc_n != n) {
    HIPCHK(ctx->d_cellc.reserve((size_t)n * 4));
    hipLaunchKernelGGL(k_cell_centres, dim3(std::min<size_t>(nblk(n), 2048)), dim3(256), 0, ctx->stream, a, NC, ctx->d_cellc, cs.d_range);
    KCHK("k_cell_centres");
    HIPCHK(hipMemcpyAsync(ctx->cellc_range, cs.d_range, sizeof(hr), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemsetAsync(cs.d_range, 0, sizeof(hr), ctx->stream));      // ([13]: the dead-unit count of k_cell_records)
    ctx->cellc_valid = true;
    ctx->cellc_n = n;
  }
  memcpy(hr, ctx->cellc_range, sizeof(hr));
  cs.d_centres = ctx->d_cellc;
  mark("allocations, centres");
  CellArgs &ca = cs.a;
  memset(&ca, 0, sizeof(ca));
  ca.CX = cell_w; ca.CL = cell_h;
  ca.mCX = cell_w > 1 ? (uint32_t)((0x100000000ull + (uint64_t)cell_w - 1) / (uint64_t)cell_w) : 0u;
  ca.mCL = cell_h > 1 ? (uint32_t)((0x100000000ull + (uint64_t)cell_h - 1) / (uint64_t)cell_h) : 0u;
  ca.qCX = (65536 + cell_w - 1) / cell_w; ca.qCL = (65536 + cell_h - 1) / cell_h;
  ca.QX = ca.QL = 1;                                    // (quads of cells: tried and dropped, DESIGN 5.3)
  ca.band_shift = ctx->cell_band;
  ca.PL = (ca.CX + NS - 1) | 1;                         // (odd: with an even pitch the gather's rows collide in the LDS banks -- P4 gather 2.97 -> 3.65 ms, round 4)
  ca.DL = ca.CL + NS - 1;
  ca.PP = ca.PL * ca.DL;
  // the kernels' LDS boxes: one private copy per slot in the scatter, one read-only copy in the gather; a cell size whose boxes
  // do not fit the 64 KiB a workgroup may hold (svr_set_option cell_w / cell_h beyond ~24 x 24 at support 16) leaves the state
  // unusable and the fallback modes take over, instead of a launch that fails
  if ((size_t)(need_stage ? (ctx->pvr ? SlotGeom<PVR_N>::NSLOT : 4) : 1) * ca.PP * sizeof(f2) > 64 * 1024) { cs.valid = true; return SVR_OK; }
  ca.split = std::max(1, ctx->cell_split);
  uint64_t ncells = 0;
  size_t nrowcol = 0;
  int ngs = 0;
  bool ok = true;
  for (int c = 0; c < 2; ++c) {
    CellClass &C = ca.cls[c];
    const int *q = hr + 6 * c;
    C.cell_base = (int)ncells;
    C.row_base = C.col_base = (int)nrowcol;
    if (q[0] > q[1]) { C.ng = 0; C.ncx = C.ncl = 0; continue; }          // no pixel of this class
    const int vgz = c == 0 ? (int)ctx->vy : (int)ctx->vz;
    for (int k = 0; k < 6; ++k) ok = ok && q[k] > -32000 && q[k] < 32000;
    C.x0 = q[0]; C.l0 = q[2];
    C.ncx = (q[1] - q[0]) / (ca.CX * ca.QX) + 1;
    C.ncl = (q[3] - q[2]) / (ca.CL * ca.QL) + 1;
    C.pfirst = q[4] - NC;
    C.plast = std::min(q[5] + NH, vgz - 1);
    const int np = C.plast - C.pfirst + 1;
    C.ng = np > 0 ? np : 0;
    ok = ok && C.ng <= 1024;
    while (((q[5] - q[4] + NC) >> ca.band_shift) >= 128) ++ca.band_shift;      // the band field of the sort key has 7 bits
    ngs = std::max(ngs, C.ng);
    ncells += (uint64_t)C.ncx * C.ncl;
    C.col_base = C.row_base + C.ncl;
    nrowcol += (size_t)C.ncl + (size_t)C.ncx;
  }
  ca.ngs = std::max(ngs, 1);
  ok = ok && ncells > 0 && ncells < (1u << 18) && ncells * (uint64_t)ca.ngs < (1ull << 28);
  if (!ok) { if (getenv("SVR_TUNE_DEBUG")) fprintf(stderr, "[cell] layout limits exceeded (%llu quads, %d planes): fallback\n", (unsigned long long)ncells, ngs); cs.valid = true; return SVR_OK; }
  cs.n_cells = (uint32_t)ncells;
  cs.n_sorted = n - (uint32_t)hr[12];
  if (!cs.n_sorted) { cs.valid = true; return SVR_OK; }
  hipLaunchKernelGGL(k_cell_keys, dim3(nblk(n)), dim3(256), 0, ctx->stream, a, ca, cs.d_centres, cs.d_keys);
  KCHK("k_cell_keys");
  size_t tb = 0, tb2 = 0;
  if (svr_sort_keys_u64(nullptr, &tb, cs.d_keys, cs.d_keys2, n, 64, ctx->stream)) return fail(ctx, SVR_E_STATE, "cell_prepare: sort (size query)");
  if (svr_inclusive_sum_u32(nullptr, &tb2, cs.d_head, cs.d_runid, n, ctx->stream)) return fail(ctx, SVR_E_STATE, "cell_prepare: scan (size query)");
  tb = std::max(tb, tb2);
  HIPCHK(cs.d_tmp.reserve(tb));
  size_t tbs = cs.d_tmp.capacity();
  if (svr_sort_keys_u64(cs.d_tmp, &tbs, cs.d_keys, cs.d_keys2, n, 64, ctx->stream)) return fail(ctx, SVR_E_STATE, "cell_prepare: sort");
  mark("keys, sort");
  const uint32_t ns_ = cs.n_sorted;
  if (ctx->pvr) hipLaunchKernelGGL((k_cell_records<PVR_N, true>), dim3(nblk(ns_)), dim3(256), 0, ctx->stream, a, cs.d_keys2, ns_, cs.d_recs, cs.d_head, reinterpret_cast<unsigned int *>(cs.d_range + 13));
  else hipLaunchKernelGGL((k_cell_records<PSF_SUPPORT, false>), dim3(nblk(ns_)), dim3(256), 0, ctx->stream, a, cs.d_keys2, ns_, cs.d_recs, cs.d_head, reinterpret_cast<unsigned int *>(cs.d_range + 13));
  KCHK("k_cell_records");
  tbs = cs.d_tmp.capacity();
  if (svr_inclusive_sum_u32(cs.d_tmp, &tbs, cs.d_head, cs.d_runid, ns_, ctx->stream)) return fail(ctx, SVR_E_STATE, "cell_prepare: scan");
  uint32_t nruns = 0;
  HIPCHK(hipMemcpyAsync(&nruns, cs.d_runid + (ns_ - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  cs.n_runs = nruns;
  {
    unsigned int du = 0;
    HIPCHK(hipMemcpyAsync(&du, cs.d_range + 13, sizeof(du), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    cs.dead_units = du;
  }
  mark("records, scan");
  HIPCHK(cs.d_runs.reserve(nruns));
  HIPCHK(cs.d_cell_first.reserve(ncells));
  HIPCHK(cs.d_cell_last.reserve(ncells));
  const size_t tab = (size_t)ncells * ca.ngs;
  HIPCHK(cs.d_item_of.reserve(tab));
  HIPCHK(cs.d_items.reserve(tab));
  HIPCHK(hipMemsetAsync(cs.d_cell_first, 0, ncells * sizeof(uint32_t), ctx->stream));
  HIPCHK(hipMemsetAsync(cs.d_cell_last, 0, ncells * sizeof(uint32_t), ctx->stream));
  hipLaunchKernelGGL(k_cell_runs, dim3(nblk(ns_)), dim3(256), 0, ctx->stream, cs.d_keys2, cs.d_head, cs.d_runid, ns_, cs.d_runs);
  KCHK("k_cell_runs");
  HIPCHK(hipMemsetAsync(ctx->d_counter, 0, 2 * sizeof(uint32_t), ctx->stream));
  hipLaunchKernelGGL(k_cell_run_ranges, dim3(nblk(nruns)), dim3(256), 0, ctx->stream, cs.d_runs, nruns, ns_, cs.d_recs, cs.d_keys2, cs.d_cell_first,
                     cs.d_cell_last, ctx->d_counter + 1);
  KCHK("k_cell_run_ranges");
  if (need_stage) {
    HIPCHK(cs.d_rowcol.reserve(nrowcol));
    HIPCHK(hipMemsetAsync(cs.d_rowcol, 0, nrowcol, ctx->stream));
    hipLaunchKernelGGL(k_cell_rowcol, dim3(nblk(nruns)), dim3(256), 0, ctx->stream, ca, cs.d_runs, nruns, cs.d_rowcol);
    KCHK("k_cell_rowcol");
    ca.rowcol = cs.d_rowcol;
  }
  ca.recs = cs.d_recs; ca.runs = cs.d_runs; ca.cell_first = cs.d_cell_first; ca.cell_last = cs.d_cell_last;
  ca.items = cs.d_items; ca.item_of = cs.d_item_of;
  {
    HIPCHK(cs.d_item_flag.reserve(tab));
    HIPCHK(cs.d_item_pos.reserve(tab));
    hipLaunchKernelGGL(k_cell_item_flags, dim3(nblk(tab)), dim3(256), 0, ctx->stream, ca, NC, NH, (uint32_t)ncells, cs.d_item_flag);
    KCHK("k_cell_item_flags");
    size_t tb3 = 0;
    if (svr_inclusive_sum_u32(nullptr, &tb3, cs.d_item_flag, cs.d_item_pos, tab, ctx->stream)) return fail(ctx, SVR_E_STATE, "cell_prepare: scan (size query)");
    HIPCHK(cs.d_tmp.reserve(tb3));
    tb3 = cs.d_tmp.capacity();
    if (svr_inclusive_sum_u32(cs.d_tmp, &tb3, cs.d_item_flag, cs.d_item_pos, tab, ctx->stream)) return fail(ctx, SVR_E_STATE, "cell_prepare: scan of the item flags");
    hipLaunchKernelGGL(k_cell_items, dim3(nblk(tab)), dim3(256), 0, ctx->stream, ca, (uint32_t)tab, cs.d_item_flag, cs.d_item_pos, cs.d_items, cs.d_item_of);
    KCHK("k_cell_items");
  }
  mark("runs, run ranges, items");
  uint32_t two[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(two + 1, ctx->d_counter + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(two, cs.d_item_pos + (tab - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const uint32_t nitems = two[0];
  if (two[1]) { if (getenv("SVR_TUNE_DEBUG")) fprintf(stderr, "[cell] %u runs with > %u pixels of a slice in one cell: fallback\n", two[1], CELL_RUN_MAX); cs.valid = true; return SVR_OK; }         // > CELL_RUN_MAX pixels of one slice in one cell
  ca.nitems = nitems;
  uint32_t nents = 0;
  {
    // launch order (heaviest first) and parts (see k_cell_item_work)
    DevBuf<uint64_t> k1, k2;
    DevBuf<uint32_t> it2, work, parts, epos;
    const bool order = ctx->cell_order > 0 && nitems > 1;
    if (k1.reserve(nitems) != hipSuccess || k2.reserve(nitems) != hipSuccess || it2.reserve(nitems) != hipSuccess ||
        work.reserve(nitems) != hipSuccess || parts.reserve(nitems) != hipSuccess || epos.reserve(nitems) != hipSuccess) {
      (void)hipGetLastError();
      return fail(ctx, SVR_E_STATE, "cell_prepare: out of device memory (item order)");
    }
    hipLaunchKernelGGL(k_cell_item_work, dim3(nblk(nitems)), dim3(256), 0, ctx->stream, ca, NC, NH, nitems, order ? ctx->cell_order - 1 : 0, work, k1);
    size_t tb4 = 0, tb5 = 0;
    if (svr_sort_keys_u64(nullptr, &tb4, k1, k2, nitems, 64, ctx->stream) || svr_inclusive_sum_u32(nullptr, &tb5, parts, epos, nitems, ctx->stream)) return fail(ctx, SVR_E_STATE, "cell_prepare: item sort (size query)");
    tb4 = std::max(tb4, tb5);
    if (cs.d_tmp.reserve(tb4) != hipSuccess) { (void)hipGetLastError(); return fail(ctx, SVR_E_STATE, "cell_prepare: out of device memory (item order)"); }
    size_t tbs2 = cs.d_tmp.capacity();
    if (order && svr_sort_keys_u64(cs.d_tmp, &tbs2, k1, k2, nitems, 64, ctx->stream)) return fail(ctx, SVR_E_STATE, "cell_prepare: item sort");
    // the launch's work ~ every sorted pixel on the NS planes of its footprint; its fair share per wavefront slot / cell_balance
    const double total = (double)cs.n_sorted * NS;
    const uint32_t target = ctx->cell_balance > 0 ? (uint32_t)std::min(4.0e9, std::max(64.0, total / (1024.0 * ctx->cell_balance))) : 0u;
    if (hipMemcpyAsync(it2, cs.d_items, (size_t)nitems * 4, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) return fail(ctx, SVR_E_STATE, "cell_prepare: copy");
    hipLaunchKernelGGL(k_cell_items_reorder, dim3(nblk(nitems)), dim3(256), 0, ctx->stream, nitems, order ? k2 : (const uint64_t *)nullptr, it2, work, target, (uint32_t)ca.split, cs.d_items, parts);
    tbs2 = cs.d_tmp.capacity();
    if (svr_inclusive_sum_u32(cs.d_tmp, &tbs2, parts, epos, nitems, ctx->stream)) return fail(ctx, SVR_E_STATE, "cell_prepare: scan of the parts");
    if (hipMemcpyAsync(&nents, epos + (nitems - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) return fail(ctx, SVR_E_STATE, "cell_prepare: item order");
    if (nents >= (1u << 28)) { if (getenv("SVR_TUNE_DEBUG")) fprintf(stderr, "[cell] %u entries: beyond item_of's 28 bits, fallback\n", nents); cs.valid = true; return SVR_OK; }
    if (cs.d_ents.reserve(nents) != hipSuccess) { (void)hipGetLastError(); return fail(ctx, SVR_E_STATE, "cell_prepare: out of device memory (entries)"); }
    hipLaunchKernelGGL(k_cell_entries, dim3(nblk(nitems)), dim3(256), 0, ctx->stream, ca, nitems, cs.d_items, parts, epos, cs.d_ents, cs.d_item_of);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return fail(ctx, SVR_E_STATE, "cell_prepare: entries");
    if (!nents) { cs.valid = true; return SVR_OK; }         // (unusable: the atomic flush takes over)
    ca.ents = cs.d_ents; ca.nents = nents;
    mark("items by work, parts");
  }
  const size_t stage = need_stage ? (size_t)nents * ca.PP : 0;
  if (stage > cs.d_stage.capacity()) {
    cs.d_stage.reset();
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess || stage * sizeof(f2) + (size_t(1) << 30) > fr || cs.d_stage.reserve(stage) != hipSuccess) {
      (void)hipGetLastError();
      cs.valid = true;                                   // does not fit: the atomic flush takes over
      return SVR_OK;
    }
  }
  mark("staging buffer");
  ca.stage = cs.d_stage;
  cs.ns_support = NS;
  cs.usable = nitems > 0;
  cs.valid = true;
  if (getenv("SVR_TUNE_DEBUG"))
    fprintf(stderr, "[cell] %u pixels in %u runs, %llu quads of %dx%d cells of %dx%d voxels (classes %dx%d + %dx%d quads, %d + %d planes), %u items in %d entries, staging %.1f MB\n",
            ns_, nruns, (unsigned long long)ncells, ca.QX, ca.QL, ca.CX, ca.CL, ca.cls[0].ncx, ca.cls[0].ncl, ca.cls[1].ncx, ca.cls[1].ncl, ca.cls[0].ng, ca.cls[1].ng,
            nitems, (int)nents, stage * sizeof(f2) / 1048576.0);
  return SVR_OK;
}

int cell_pids(svr_ctx *ctx, CellState &cs, const PsfArgs &a, CellArgs &ca);   // the records' table ids for a COEFF launch (svr_table.inc)

// the scatter of one pass: factors, items, combine.  out0 | out1 = addon | cmap (or recon | volw in the Gaussian pass).
// store: the pass evaluates every tap of every PSF pixel and writes the coefficient table (support 16; a.coeff = the table to fill, a.coeff_id filled)
int launch_cell_scatter(svr_ctx *ctx, const PsfArgs &a, int gauss, float *out0, float *out1, bool store = false) {
  CellState &cs = *ctx->cell;
  CellArgs ca = cs.a;
  const int NS = cs.ns_support, NC = (NS - 1) / 2, NH = NS - 1 - NC;
  { const int rp = cell_pids(ctx, cs, a, ca); if (rp) return rp; }
  if (store) {
    HIPCHK(cs.d_act.reserve(cs.n_sorted));
    ca.act = cs.d_act;
  }
  hipLaunchKernelGGL(k_cell_factors, dim3(nblk(cs.n_sorted)), dim3(256), 0, ctx->stream, a, gauss, cs.d_recs, cs.n_sorted, store ? cs.d_act : (unsigned char *)nullptr);
  KCHK("k_cell_factors");
  const size_t lds = (size_t)(ctx->pvr ? SlotGeom<PVR_N>::NSLOT : 4) * ca.PP * sizeof(f2);
  const dim3 block(64);
  ca.dbg = getenv("SVR_CELL_DBG") ? atoi(getenv("SVR_CELL_DBG")) : 0;
  const char *trace_file = getenv("SVR_CELL_TRACE");
  DevBuf<unsigned long long> trace, stats;
  if (trace_file) { HIPCHK(trace.reserve((size_t)ca.nents * 3)); ca.trace = trace; }
  if (ca.dbg == 2) {
    HIPCHK(stats.reserve(8));
    ca.stats = stats;
    HIPCHK(hipMemsetAsync(ca.stats, 0, 8 * sizeof(unsigned long long), ctx->stream));
  }
  {
    const int rr = in_pieces(ca.nents, 64, [&](uint32_t off, uint32_t cnt) {
      const dim3 g(cnt);
      if (ctx->pvr && a.coeff) hipLaunchKernelGGL((back_cell_kernel<PVR_N, true, 1>), g, block, lds, ctx->stream, a, ca, off);
      else if (ctx->pvr) hipLaunchKernelGGL((back_cell_kernel<PVR_N, true>), g, block, lds, ctx->stream, a, ca, off);
      else if (a.coeff && store) hipLaunchKernelGGL((back_cell_kernel<PSF_SUPPORT, false, 3>), g, block, lds, ctx->stream, a, ca, off);
      else if (a.coeff) hipLaunchKernelGGL((back_cell_kernel<PSF_SUPPORT, false, 1>), g, block, lds, ctx->stream, a, ca, off);
      else hipLaunchKernelGGL(back_cell_kernel<>, g, block, lds, ctx->stream, a, ca, off);
      return (int)SVR_OK;
    });
    if (rr) return rr;
  }
  KCHK("back_cell_kernel");
  if (trace_file) {
    std::vector<unsigned long long> h((size_t)ca.nents * 3);
    HIPCHK(hipMemcpyAsync(h.data(), ca.trace, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (FILE *f = fopen(trace_file, "wb")) { fwrite(h.data(), sizeof(unsigned long long), h.size(), f); fclose(f); }
  }
  if (ca.dbg == 2) {
    unsigned long long h[8];
    HIPCHK(hipMemcpyAsync(h, ca.stats, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    fprintf(stderr, "[cell stats] chunk visits %llu, with work %llu, sum of longest live lists %llu (ideal %llu), live units %llu, dead units %llu\n", h[0], h[1], h[2], (h[3] + 3) / 4, h[3], h[4]);
  }
  {
    // covering cells per axis: a source coordinate lies in the boxes of floor((NS - 2 + C) / C) + 1 cells at most
    const int mj = (NS - 2 + ca.CL) / ca.CL + 1, mi = (NS - 2 + ca.CX) / ca.CX + 1;
    const dim3 g((ctx->vx + 63) / 64, (ctx->vy + 3) / 4, ctx->vz), b(256);
    const bool general = ctx->cell_combine == 0 || mj > 4 || mi > 4 || ca.QX != 1 || ca.QL != 1;
    // the x cells that 64 consecutive voxels can need between them: one wavefront load if they fit 16 columns
    // (and its divisions by multiplication hold for coordinates inside +-2^15: floordiv_m)
    const bool wave = !general && ctx->cell_combine == 2 && (63 + NS - 1 + ca.CX - 1) / ca.CX + 1 <= 16 &&
                      std::max(ctx->vx, std::max(ctx->vy, ctx->vz)) < 32768 && ca.CX <= 1024 && ca.CL <= 1024;
    if (general) hipLaunchKernelGGL(k_cell_combine, g, b, 0, ctx->stream, ca, a.vg, NC, NH, a.mask, out0, out1);
    else if (wave && mj <= 3 && mi <= 3) hipLaunchKernelGGL((k_cell_combine_wave<3, 3>), g, b, 0, ctx->stream, ca, a.vg, NC, NH, a.mask, out0, out1);
    else if (wave && mj <= 4 && mi <= 3) hipLaunchKernelGGL((k_cell_combine_wave<4, 3>), g, b, 0, ctx->stream, ca, a.vg, NC, NH, a.mask, out0, out1);
    else if (wave && mj <= 3) hipLaunchKernelGGL((k_cell_combine_wave<3, 4>), g, b, 0, ctx->stream, ca, a.vg, NC, NH, a.mask, out0, out1);
    else if (wave) hipLaunchKernelGGL((k_cell_combine_wave<4, 4>), g, b, 0, ctx->stream, ca, a.vg, NC, NH, a.mask, out0, out1);
    else if (mj <= 3 && mi <= 3) hipLaunchKernelGGL((k_cell_combine_fast<3, 3>), g, b, 0, ctx->stream, ca, a.vg, NC, NH, a.mask, out0, out1);
    else if (mj <= 4 && mi <= 3) hipLaunchKernelGGL((k_cell_combine_fast<4, 3>), g, b, 0, ctx->stream, ca, a.vg, NC, NH, a.mask, out0, out1);
    else if (mj <= 3) hipLaunchKernelGGL((k_cell_combine_fast<3, 4>), g, b, 0, ctx->stream, ca, a.vg, NC, NH, a.mask, out0, out1);
    else hipLaunchKernelGGL((k_cell_combine_fast<4, 4>), g, b, 0, ctx->stream, ca, a.vg, NC, NH, a.mask, out0, out1);
  }
  KCHK("k_cell_combine");
  return SVR_OK;
}

// pass 1 of the Gaussian reconstruction over the gather's cell structures (a.flag_out = the gate's flags; a.list is not used: the
// sorted records hold every pixel with s != -1 whose footprint reaches the volume, the others keep flag 0)
int launch_cell_gauss1(svr_ctx *ctx, CellState &cs, const PsfArgs &a) {
  CellArgs ca = cs.a;
  const int NS = cs.ns_support;
  int r;
  HIPCHK(cs.d_part.reserve((size_t)cs.n_sorted * NS));
  const size_t lds = (size_t)ca.PP * sizeof(f2);
  r = in_pieces(ca.nents, 64, [&](uint32_t off, uint32_t cnt) {
    if (ctx->pvr) hipLaunchKernelGGL((fwd_cell_kernel<PVR_N, true, 0, true>), dim3(cnt), dim3(64), lds, ctx->stream, a, ca, (const float *)nullptr, cs.d_part, (uint32_t)cs.n_sorted, off);
    else hipLaunchKernelGGL((fwd_cell_kernel<PSF_SUPPORT, false, 0, true>), dim3(cnt), dim3(64), lds, ctx->stream, a, ca, (const float *)nullptr, cs.d_part, (uint32_t)cs.n_sorted, off);
    KCHK("fwd_cell_kernel<G1>");
    return (int)SVR_OK;
  });
  if (r) return r;
  const double *pd = reinterpret_cast<const double *>(cs.d_part.get());
  if (ctx->pvr) hipLaunchKernelGGL((k_cell_gauss1_finish<PVR_N, true>), dim3(nblk(cs.n_sorted)), dim3(256), 0, ctx->stream, a, ca, cs.d_recs, pd, cs.n_sorted);
  else hipLaunchKernelGGL((k_cell_gauss1_finish<PSF_SUPPORT, false>), dim3(nblk(cs.n_sorted)), dim3(256), 0, ctx->stream, a, ca, cs.d_recs, pd, cs.n_sorted);
  KCHK("k_cell_gauss1_finish");
  return SVR_OK;
}

// the gather of one pass over the cell structures (svr_simulate_slices with fwd_mode 2)
// store: the pass evaluates every tap and writes the coefficient table (support 16; a.coeff = the table to fill, a.coeff_id filled)
int launch_cell_gather(svr_ctx *ctx, CellState &cs, const PsfArgs &a, bool store = false) {
  CellArgs ca = cs.a;
  const int NS = cs.ns_support;
  int r;
  HIPCHK(cs.d_gf.reserve(cs.n_sorted));
  HIPCHK(cs.d_part.reserve((size_t)cs.n_sorted * NS));
  if ((r = cell_pids(ctx, cs, a, ca))) return r;
  if (!cs.gf_valid || a.flag) {                            // (1 / v_PSF_sums per sorted pixel: once per Gaussian pass, not once per SR iteration)
    hipLaunchKernelGGL(k_cell_gfactors, dim3(nblk(cs.n_sorted)), dim3(256), 0, ctx->stream, a, cs.d_recs, cs.n_sorted, cs.d_gf);
    KCHK("k_cell_gfactors");
    cs.gf_valid = !a.flag;
  }
  const bool dma = a.coeff && !ctx->pvr && !store;         // support 16: the table's rows land in the LDS (COEFF == 2)
  const size_t lds = (size_t)ca.PP * sizeof(f2) + (dma ? 16 + (size_t)SVR_CELL_DMA_DEPTH * CoeffLayout<PSF_SUPPORT>::STAGE_BYTES : 0);
  r = in_pieces(ca.nents, 64, [&](uint32_t off, uint32_t cnt) {
    if (ctx->pvr && a.coeff) hipLaunchKernelGGL((fwd_cell_kernel<PVR_N, true, 1>), dim3(cnt), dim3(64), lds, ctx->stream, a, ca, cs.d_gf, cs.d_part, (uint32_t)cs.n_sorted, off);
    else if (ctx->pvr) hipLaunchKernelGGL((fwd_cell_kernel<PVR_N, true>), dim3(cnt), dim3(64), lds, ctx->stream, a, ca, cs.d_gf, cs.d_part, (uint32_t)cs.n_sorted, off);
    else if (a.coeff && store) hipLaunchKernelGGL((fwd_cell_kernel<PSF_SUPPORT, false, 3>), dim3(cnt), dim3(64), lds, ctx->stream, a, ca, cs.d_gf, cs.d_part, (uint32_t)cs.n_sorted, off);
    else if (a.coeff) hipLaunchKernelGGL((fwd_cell_kernel<PSF_SUPPORT, false, 2>), dim3(cnt), dim3(64), lds, ctx->stream, a, ca, cs.d_gf, cs.d_part, (uint32_t)cs.n_sorted, off);
    else hipLaunchKernelGGL(fwd_cell_kernel<>, dim3(cnt), dim3(64), lds, ctx->stream, a, ca, cs.d_gf, cs.d_part, (uint32_t)cs.n_sorted, off);
    KCHK("fwd_cell_kernel");
    return (int)SVR_OK;
  });
  if (r) return r;
  if (ctx->pvr) hipLaunchKernelGGL(k_cell_gather_finish<PVR_N>, dim3(nblk(cs.n_sorted)), dim3(256), 0, ctx->stream, a, ca, cs.d_recs, cs.d_gf, cs.d_part, cs.n_sorted);
  else hipLaunchKernelGGL(k_cell_gather_finish<PSF_SUPPORT>, dim3(nblk(cs.n_sorted)), dim3(256), 0, ctx->stream, a, ca, cs.d_recs, cs.d_gf, cs.d_part, cs.n_sorted);
  KCHK("k_cell_gather_finish");
  return SVR_OK;
}
