// svr_slab.inc -- the volume update of a sharded run by z-slabs (#included by svr_hip.hip after svr_regul.inc).
//
// The reference adds the per-device addon / cmap volumes up on GPU 0 and regularises there (reconstruction_cuda2.cu:2225-2239,
// 2138-2181).  Rounds 1-3 here all-reduced the pair (2 Nv floats) and ran the update replicated on every rank: the collective
// carried the whole volume twice and the update's time did not divide by the number of ranks.  Now:
//
//   scatter (rank's slices, whole volume)
//     -> svr_slab_rs_pack:   addon | cmap at the MASK's voxels only (the scatter writes nothing else: 48 % of P4 / S8), cut into
//                            `world` z-slabs of equal mask-voxel count, each with one halo plane on either side
//     -> reduce-scatter      (the launcher's collective: ncclReduceScatter on the engine's stream): a rank receives the sums of its slab + halo
//     -> svr_slab_update:    the sums go back into addon / cmap, k_regul_fused runs on the rank's planes only (Prep of the halo planes
//                            is evaluated from the reduced halo), the rank's part of the new volume is packed at the voxels where
//                            it can be non-zero (the mask dilated by one voxel: a weight needs a neighbour with cmap > 0)
//     -> all-gather          (ncclAllGather): every rank receives every slab of the new volume
//     -> svr_slab_finish:    unpacked into the other volume buffer; recon() flips.
//
// Bytes a rank sends per SR iteration (N ranks, Nm mask voxels, Nd dilated): 4 (N-1)/N (2 Nm + Nd) + halos, against
// 2 x 4 (N-1)/N 2 Nv for the ring all-reduce of the pair: S8 (Nv 20.3 M, Nm 9.9 M) 111 MB instead of 285 MB at N = 8.
// Results: identical on every rank (a rank's slab is updated by one rank and all-gathered), and -- with collectives that add the ranks in
// rank order (the host-staged exchanges of a `-d 0 0 0` group, gloo) -- the same bits as the replicated update: the update itself is
// deterministic (tests/test_distributed_cpu.py, `-d 0 0 0` command lines).  RCCL may add the ranks of a ring in another order per
// element, and a halo plane is reduced twice (in its owner's chunk and in the neighbour's): with ncclReduceScatter / ncclAllReduce the
// two forms agree to the last bits of a float sum over the ranks, not bit for bit.
//
// The index lists depend on the mask only (built on the device once per mask: flags -> prefix sum -> compaction); the slab
// boundaries on (mask, world).  Outside the dilated mask the new volume is zero: both volume buffers are kept zero there
// (vol_clean), a buffer somebody else wrote is cleared first.

struct SlabPlan {
  bool valid = false;
  DevBuf<uint32_t> d_midx, d_didx;                   // voxel indices of mask != 0 / of its 3x3x3 dilation, natural order
  uint32_t nm = 0, nd = 0;
  std::vector<uint32_t> mcum, dcum;                  // [vz + 1] mask / dilated voxels in the planes below z
  int world = 0, rank = -1;
  std::vector<int> zb;                               // [world + 1] slab r = planes [zb[r], zb[r + 1])
  std::vector<uint32_t> rs_start, rs_count, ag_start, ag_count;   // per rank: range of d_midx (slab + halo planes) / of d_didx (slab)
  uint32_t rs_chunk = 0, ag_chunk = 0;               // floats per rank and volume (padded to the largest rank's)
  DevBuf<float> d_send, d_recv;                      // [world][2][rs_chunk] | [2][rs_chunk]; then [ag_chunk] | [world][ag_chunk]
  DevBuf<uint32_t> d_tab;                            // [4][world] rs_start, rs_count, ag_start, ag_count on the device
};

void slab_free(SlabPlan *p) { delete p; }

__global__ void k_slab_flags(const float *mask, int vx, int vy, int vz, uint32_t *fm, uint32_t *fd) {
  const size_t n = (size_t)vx * vy * vz;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int x = (int)(i % vx), y = (int)((i / vx) % vy), z = (int)(i / ((size_t)vx * vy));
  fm[i] = mask[i] != 0.0f ? 1u : 0u;
  uint32_t d = 0;
  for (int dz = -1; dz <= 1; ++dz)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int X = x + dx, Y = y + dy, Z = z + dz;
        if (X >= 0 && X < vx && Y >= 0 && Y < vy && Z >= 0 && Z < vz && mask[(size_t)X + (size_t)Y * vx + (size_t)Z * vx * vy] != 0.0f) d = 1u;
      }
  fd[i] = d;
}
// inclusive scan -> index list; the counts below every plane
__global__ void k_slab_compact(const uint32_t *scan, size_t n, uint32_t *idx) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t s = scan[i], prev = i ? scan[i - 1] : 0u;
  if (s != prev) idx[prev] = (uint32_t)i;
}
__global__ void k_slab_plane_cum(const uint32_t *scan, size_t plane, int vz, uint32_t *cum) {
  const int z = blockIdx.x * blockDim.x + threadIdx.x;
  if (z > vz) return;
  cum[z] = z ? scan[(size_t)z * plane - 1] : 0u;
}
// addon | cmap at the mask voxels of every rank's slab + halo -> send[rank][vol][rs_chunk] (zero padded)
__global__ void k_slab_rs_pack(const float *addon, const float *cmap, const uint32_t *midx, const uint32_t *tab, int world, uint32_t chunk, float *send) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)world * 2 * chunk) return;
  const uint32_t r = (uint32_t)(i / (2 * (size_t)chunk)), rem = (uint32_t)(i - (size_t)r * 2 * chunk), v = rem / chunk, k = rem - v * chunk;
  float val = 0.0f;
  if (k < tab[world + r]) val = (v ? cmap : addon)[midx[tab[r] + k]];
  send[i] = val;
}
__global__ void k_slab_rs_unpack(float *addon, float *cmap, const uint32_t *midx, uint32_t start, uint32_t count, uint32_t chunk, const float *recv) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * (size_t)count) return;
  const uint32_t v = (uint32_t)(i / count), k = (uint32_t)(i - (size_t)v * count);
  (v ? cmap : addon)[midx[start + k]] = recv[(size_t)v * chunk + k];
}
__global__ void k_slab_ag_pack(const float *vol, const uint32_t *didx, uint32_t start, uint32_t count, uint32_t chunk, float *send) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= chunk) return;
  send[k] = k < count ? vol[didx[start + k]] : 0.0f;
}
__global__ void k_slab_ag_unpack(float *vol, const uint32_t *didx, const uint32_t *tab, int world, int skip, uint32_t chunk, const float *recv) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)world * chunk) return;
  const uint32_t r = (uint32_t)(i / chunk), k = (uint32_t)(i - (size_t)r * chunk);
  if ((int)r == skip || k >= tab[3 * world + r]) return;
  vol[didx[tab[2 * world + r] + k]] = recv[i];
}

static int slab_lists(svr_ctx *ctx, SlabPlan &p) {
  const size_t n = ctx->nv, plane = (size_t)ctx->vx * ctx->vy;
  DevBuf<uint32_t> fm, fd, sc, d_cum;
  DevBuf<unsigned char> tmp;
  size_t tb = 0;
  if (fm.reserve(n) != hipSuccess || fd.reserve(n) != hipSuccess || sc.reserve(n) != hipSuccess ||
      d_cum.reserve((size_t)ctx->vz + 1) != hipSuccess) return fail(ctx, SVR_E_STATE, "slab plan: out of device memory");
  hipLaunchKernelGGL(k_slab_flags, dim3(nblk(n)), dim3(256), 0, ctx->stream, ctx->d_mask, (int)ctx->vx, (int)ctx->vy, (int)ctx->vz, fm, fd);
  if (svr_inclusive_sum_u32(nullptr, &tb, fm, sc, n, ctx->stream)) return fail(ctx, SVR_E_STATE, "slab plan: scan (size query)");
  if (tmp.reserve(tb ? tb : 1) != hipSuccess) return fail(ctx, SVR_E_STATE, "slab plan: out of device memory");
  for (int pass = 0; pass < 2; ++pass) {
    DevBuf<uint32_t> &idx = pass ? p.d_didx : p.d_midx;
    std::vector<uint32_t> &cum = pass ? p.dcum : p.mcum;
    size_t t2 = tb;
    if (svr_inclusive_sum_u32(tmp, &t2, pass ? fd : fm, sc, n, ctx->stream)) return fail(ctx, SVR_E_STATE, "slab plan: scan");
    hipLaunchKernelGGL(k_slab_plane_cum, dim3(nblk((size_t)ctx->vz + 1)), dim3(256), 0, ctx->stream, sc, plane, (int)ctx->vz, d_cum);
    cum.assign((size_t)ctx->vz + 1, 0u);
    if (hipMemcpyAsync(cum.data(), d_cum, cum.size() * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess) return fail(ctx, SVR_E_STATE, "slab plan: copy");
    const uint32_t cnt = cum.back();
    (pass ? p.nd : p.nm) = cnt;
    idx.reset();
    if (idx.reserve(std::max(cnt, 1u)) != hipSuccess) return fail(ctx, SVR_E_STATE, "slab plan: out of device memory");
    hipLaunchKernelGGL(k_slab_compact, dim3(nblk(n)), dim3(256), 0, ctx->stream, sc, n, idx);
  }
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return fail(ctx, SVR_E_STATE, "slab plan: kernels");
  return SVR_OK;
}

// the plan of (mask, world, rank); chunk sizes in floats per rank (rs: both volumes of a rank's slab + halo; ag: a rank's slab)
static int slab_plan(svr_ctx *ctx, int world, int rank) {
  NEED(ctx->nv > 0 && ctx->have_mask, "volume / mask not set");
  if (world < 1 || rank < 0 || rank >= world) return fail(ctx, SVR_E_ARG, "slab plan: rank / world");
  if (!ctx->slab) ctx->slab = new SlabPlan();
  SlabPlan &p = *ctx->slab;
  if (!p.valid) {
    p.world = 0;
    const int rc = slab_lists(ctx, p);
    if (rc) return rc;
    p.valid = true;
  }
  if (p.world == world && p.rank == rank) return SVR_OK;
  const int vz = (int)ctx->vz;
  p.zb.assign((size_t)world + 1, 0);
  for (int r = 1; r < world; ++r) {                        // equal shares of the mask's voxels, whole planes
    const uint64_t target = (uint64_t)p.nm * r / world;
    int z = p.zb[r - 1];
    while (z < vz && p.mcum[z] < target) ++z;
    p.zb[r] = z;
  }
  p.zb[world] = vz;
  p.rs_start.assign(world, 0); p.rs_count.assign(world, 0); p.ag_start.assign(world, 0); p.ag_count.assign(world, 0);
  p.rs_chunk = p.ag_chunk = 1;
  for (int r = 0; r < world; ++r) {
    const int lo = std::max(0, p.zb[r] - 1), hi = std::min(vz, p.zb[r + 1] + 1);
    const bool empty = p.zb[r] >= p.zb[r + 1];
    p.rs_start[r] = p.mcum[lo]; p.rs_count[r] = empty ? 0u : p.mcum[hi] - p.mcum[lo];
    p.ag_start[r] = p.dcum[p.zb[r]]; p.ag_count[r] = p.dcum[p.zb[r + 1]] - p.dcum[p.zb[r]];
    p.rs_chunk = std::max(p.rs_chunk, p.rs_count[r]);
    p.ag_chunk = std::max(p.ag_chunk, p.ag_count[r]);
  }
  std::vector<uint32_t> tab;
  tab.insert(tab.end(), p.rs_start.begin(), p.rs_start.end()); tab.insert(tab.end(), p.rs_count.begin(), p.rs_count.end());
  tab.insert(tab.end(), p.ag_start.begin(), p.ag_start.end()); tab.insert(tab.end(), p.ag_count.begin(), p.ag_count.end());
  p.d_tab.reset();
  HIPCHK(p.d_tab.reserve(tab.size()));
  HIPCHK(hipMemcpyAsync(p.d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const size_t need_send = std::max((size_t)world * 2 * p.rs_chunk, (size_t)p.ag_chunk), need_recv = std::max((size_t)2 * p.rs_chunk, (size_t)world * p.ag_chunk);
  HIPCHK(p.d_send.reserve(need_send));
  HIPCHK(p.d_recv.reserve(need_recv));
  p.world = world; p.rank = rank;
  return SVR_OK;
}
