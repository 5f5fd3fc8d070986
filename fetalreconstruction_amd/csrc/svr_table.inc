// The coefficient table's owner (svr_ctx::table, CoeffTable): every write to its fields is in this file.  The others go through the named
// methods (invalidate, svr_set_option) or through a pass's three steps --
//   table_plan_for   what the pass does with the table (svr_plan.h: table_plan), from the context's options and the table's state
//   table_begin      carries the plan out: k_coeff_build first where it says so, memory / places / ids for a store, the table into PsfArgs
//   table_end        commits what a storing pass wrote
// Included after svr_cell.inc: the table's order follows the scatter's cell lists.

void CoeffTable::want(bool on) { coeff_mode = on ? 1 : 0; coeff_user = true; }
void CoeffTable::want_by_default(bool on) { if (!coeff_user) coeff_mode = on ? 1 : 0; }
void CoeffTable::set_lazy(bool on) { coeff_lazy = on ? 1 : 0; }
void CoeffTable::drop() { coeff_state = COEFF_NONE; }
void CoeffTable::drop_psf_pixels() { if (coeff_state == COEFF_PSF) coeff_state = COEFF_NONE; }   // (a COEFF_FULL table holds whatever pixels become PSF pixels)
void CoeffTable::free_rows() { d_coeff.reset(); }
void CoeffTable::free_ids() { d_coeff_id.reset(); }
void CoeffTable::ids_stale() { coeff_ids_valid = false; }

// ---- the order of the coefficient table (coeff_prepare) -------------------------------------------------------------------
__global__ void k_coeff_order_sorted(const CellRec *recs, uint32_t n, uint32_t *order, unsigned char *mark) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t idx = recs[i].idx;
  order[i] = idx;
  mark[idx] = 1;
}
__global__ void k_coeff_order_rest(const uint32_t *active, uint32_t n, const unsigned char *mark, uint32_t *order, uint32_t first, uint32_t *counter) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool rest = i < n && !mark[active[i]];
  const unsigned long long b = __ballot(rest);
  const int lane = threadIdx.x & 63;
  uint32_t base = 0;
  if (lane == 0 && b) base = atomicAdd(counter, (uint32_t)__popcll(b));
  base = __shfl(base, 0, 64);
  if (rest) order[first + base + __popcll(b & ((1ull << lane) - 1ull))] = active[i];
}
// *list = d_coeff_order[n_active]: the sorted pixels of the scatter's cell lists, then the active pixels the lists
// dropped; left as it is when the geometry has no usable cell lists
int coeff_order(svr_ctx *ctx, uint32_t n_active, const uint32_t **list) {
  int r = cell_prepare(ctx);
  if (r) return r;
  if (!ctx->cell || !ctx->cell->usable || !ctx->cell->n_sorted) return SVR_OK;
  CellState &cs = *ctx->cell;
  DevBuf<uint32_t> &order = ctx->table.d_coeff_order;
  HIPCHK(order.reserve(n_active));
  DevBuf<unsigned char> mark;
  HIPCHK(mark.reserve(ctx->np));
  HIPCHK(hipMemsetAsync(mark, 0, ctx->np, ctx->stream));
  hipLaunchKernelGGL(k_coeff_order_sorted, dim3(nblk(cs.n_sorted)), dim3(256), 0, ctx->stream, cs.d_recs, cs.n_sorted, order, mark);
  KCHK("k_coeff_order_sorted");
  if (cs.n_sorted < n_active) {
    HIPCHK(hipMemsetAsync(ctx->d_counter, 0, sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(k_coeff_order_rest, dim3(nblk(n_active)), dim3(256), 0, ctx->stream, ctx->d_active, n_active, mark, order, cs.n_sorted, ctx->d_counter);
    KCHK("k_coeff_order_rest");
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  *list = order;
  return SVR_OK;
}

// the table ids of a cell state's sorted records, for the COEFF launches (after table_begin; again when either the lists or the table are new)
__global__ void k_cell_pids(const CellRec *recs, uint32_t n, const uint32_t *coeff_id, uint32_t *pid) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) pid[i] = coeff_id[recs[i].idx];
}
int cell_pids(svr_ctx *ctx, CellState &cs, const PsfArgs &a, CellArgs &ca) {
  if (!a.coeff) return SVR_OK;
  if (!cs.pid_valid) {
    HIPCHK(cs.d_pid.reserve(cs.n_sorted));
    hipLaunchKernelGGL(k_cell_pids, dim3(nblk(cs.n_sorted)), dim3(256), 0, ctx->stream, cs.d_recs, cs.n_sorted, a.coeff_id, cs.d_pid);
    KCHK("k_cell_pids");
    cs.pid_valid = true;
  }
  ca.pid = cs.d_pid;
  return SVR_OK;
}

__global__ void k_coeff_ids(const uint32_t *list, uint32_t n, uint32_t *coeff_id) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) coeff_id[list[i]] = i;
}
// The table's memory and the pixels' places in it (*list = the active pixels in table order).  Returns with d_coeff set, or with the mode
// switched off when the table does not fit the free memory.
int coeff_prepare(svr_ctx *ctx, const uint32_t **list) {
  CoeffTable &t = ctx->table;
  // every pixel with s != -1: the Gaussian pass walks them all, the PSF pixels of the SR iterations are a subset
  const size_t npx = ctx->n_active;
  const size_t bytes = npx * (ctx->pvr ? CoeffLayout<PVR_N>::PIXEL_BYTES : CoeffLayout<PSF_SUPPORT>::PIXEL_BYTES);   // (whole float4s)
  if (bytes / sizeof(float4) > t.d_coeff.capacity()) {         // more pixels than the allocation holds (one layout per allocation: the "pvr" option raises CH_TABLE_OFF)
    t.d_coeff.reset();
    size_t fr = 0, tot = 0;
    const char *cap_gb = getenv("SVR_COEFF_MAX_GB");     // optional ceiling on the table (GiB): a deployment knob, and how the tests reach the fallback
    const bool over = cap_gb && (double)bytes > atof(cap_gb) * 1073741824.0;
    // the bias buffers are allocated before the first pass (svr_set_flags / ready); any still missing count in the headroom
    const size_t bias_later = ctx->disable_bias ? 0 : (ctx->d_bias ? 0 : 4 * ctx->np * sizeof(float)) + (ctx->d_bias_vol ? 0 : 4 * ctx->nv * sizeof(float));
    if (over || hipMemGetInfo(&fr, &tot) != hipSuccess || bytes + bias_later + (size_t(2) << 30) > fr || t.d_coeff.reserve(bytes / sizeof(float4)) != hipSuccess) {
      (void)hipGetLastError();
      t.coeff_mode = 0;                                    // does not fit: evaluate on the fly (svr_get_option tells)
      return SVR_OK;
    }
  }
  HIPCHK(t.d_coeff_id.reserve(ctx->np));      // (freed by svr_init_storage_volumes, whose changes drop the ids)
  if (t.coeff_ids_valid && t.coeff_list) { *list = t.coeff_list; return SVR_OK; }
  *list = ctx->d_active;
  // The pixels get their places in the table in the order of the scatter's cell lists (cell, slice, band, position): what a
  // (cell, plane) item of the scatter or a slice tile of the gather reads next then lies within a few megabytes instead of one
  // KiB per slice all over the table (a TLB miss per unit); pixels the cell lists dropped (footprint beyond the volume) follow.
  if (!getenv("SVR_COEFF_UNSORTED")) {
    const int r = coeff_order(ctx, (uint32_t)npx, list);
    if (r) return r;
  }
  t.coeff_list = *list;
  return SVR_OK;
}
// k_coeff_build over every active pixel (a plan's build_first: the table is wanted, there is none, there are pixels).
// Returns with coeff_state COEFF_FULL, or with the mode switched off when the table does not fit the free memory.
int coeff_build(svr_ctx *ctx) {
  CoeffTable &t = ctx->table;
  PsfArgs a = make_args(ctx);
  a.n = ctx->n_active;
  { const int r = coeff_prepare(ctx, &a.list); if (r) return r; }
  if (!t.coeff_mode) return SVR_OK;
  ScopedTimer tb(ctx, SVR_T_COEFF_BUILD);
  {
    const int rr = pixel_list_in_pieces(a, [&](const PsfArgs &ap, uint32_t off) {
      if (ctx->pvr) hipLaunchKernelGGL((k_coeff_build<PVR_N, true>), dim3(nblk(ap.n, 4)), dim3(256), 0, ctx->stream, ap, t.d_coeff, t.d_coeff_id, off);
      else hipLaunchKernelGGL((k_coeff_build<PSF_SUPPORT, false>), dim3(nblk(ap.n, 4)), dim3(256), 0, ctx->stream, ap, t.d_coeff, t.d_coeff_id, off);
      KCHK("k_coeff_build");
      return (int)SVR_OK;
    });
    if (rr) return rr;
  }
  tb.stop();
  t.coeff_state = COEFF_FULL;
  if (!t.coeff_ids_valid) invalidate(ctx, CH_TABLE_IDS);   // (k_coeff_build gave the pixels their places: cell_pids)
  t.coeff_ids_valid = true;
  return SVR_OK;
}

// ---- a pass and the table ----------------------------------------------------------------------------------------------------
// cells_usable: what the pass's own cell lists said, or true while they are not built (svr_plan.h TableInputs)
TablePlan table_plan_for(const svr_ctx *ctx, Pass pass, const PassPath &p, bool cells_usable) {
  const CoeffTable &t = ctx->table;
  // Can the table be left to the first gather of the SR iterations (coeff_lazy)?  Support 16 on the cell gather.
  const bool lazy_ok = t.coeff_lazy && !ctx->pvr && ctx->fwd_mode == 2;
  return table_plan(pass, p, {t.coeff_mode != 0, t.coeff_state, lazy_ok, ctx->n_active != 0, ctx->n_psf != 0, cells_usable});
}
// Before the pass's launches.  *use = what the pass does: the plan's use with the table in a.coeff / a.coeff_id, or TABLE_EVALUATE where
// the table turned out not to fit the memory (the mode is off from then on).  A storing pass evaluates every unit the SR iterations will
// read (fwd_cell_kernel / back_cell_kernel<.., 3>: the evaluation it needs anyway) into the places k_coeff_ids gives the active pixels.
int table_begin(svr_ctx *ctx, const TablePlan &tp, PsfArgs &a, TableUse *use) {
  CoeffTable &t = ctx->table;
  *use = TABLE_EVALUATE;
  int r;
  if (tp.build_first && (r = coeff_build(ctx))) return r;
  if (tp.use == TABLE_STORE) {
    const uint32_t *order = nullptr;
    if ((r = coeff_prepare(ctx, &order))) return r;
    if (t.coeff_mode && !t.coeff_ids_valid) {
      hipLaunchKernelGGL(k_coeff_ids, dim3(nblk(ctx->n_active)), dim3(256), 0, ctx->stream, order, (uint32_t)ctx->n_active, t.d_coeff_id);
      KCHK("k_coeff_ids");
      invalidate(ctx, CH_TABLE_IDS);
      t.coeff_ids_valid = true;
    }
  }
  if (tp.use == TABLE_EVALUATE || !t.coeff_mode) return SVR_OK;
  a.coeff = t.d_coeff; a.coeff_id = t.d_coeff_id;
  *use = tp.use;
  return SVR_OK;
}
// After the launches of a pass that ran: what a store wrote are the PSF pixels' live units -- what the SR iterations' passes read
void table_end(svr_ctx *ctx, TableUse use) {
  if (use == TABLE_STORE) ctx->table.coeff_state = COEFF_PSF;
}
