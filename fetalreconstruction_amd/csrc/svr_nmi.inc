// svr_nmi.inc -- normalised mutual information of the default (IRTK) registration on the device; included by svr_hip.hip.
//
// irtkImageRigidRegistrationWithPadding::Evaluate (IRRWP.cc:534-610) with irtkNormalisedMutualInformationSimilarityMetric
// over irtkHistogram_2D<double>: the samples are sim_sample's (svr_sim.inc), and every sample adds one to the joint bin (target
// bin, source bin) instead of six moments.  The source was binned before it is interpolated (irtkCalculateNumberOfBins,
// irtkUtil.cc:438-474: v > 0 -> int(v / width)); the target's bin is taken on the fly (tv / width).
//
// One evaluation = one candidate matrix on all planes of a target (1 for a slice, nz for a package): the entropies are not
// additive over planes, so the histogram spans them all.  A workgroup builds the histogram of a run of planes in LDS with
// integer atomics (u32 [source bin][target bin], at most 64 x 64 = 16 KB); an evaluation with more planes than one
// workgroup takes is split over several, which add their LDS histograms into a merge slot in global memory with integer
// atomics; the last of them to arrive (a per-slot counter) takes the slot back with atomic exchanges, which leaves slot and
// counter zero for the next call -- no memset per call.  Counts are integers: the histogram does not depend on the schedule.
//
// The entropy pass then restates irtkHistogram_2D::EntropyX / EntropyY / JointEntropy (H2D.cc:443-523) serially: the
// terms c * log(c) of the nonzero bins (joint: source-major visit order; the two marginals in bin order) are added one
// after another in that order, by one lane each.  The terms come from a table the host fills with its own libm
// (svr_nmi_evaluate), so {n, S_xy, S_x, S_y} equal the host's serial loops bit for bit and the NMI finished on the host
// equals irtkHistogram_2D::NormalizedMutualInformation of the same counts.  The nonzero joint bins are compacted (a block
// scan) so the serial lane only walks those.

namespace {

constexpr int NMI_B = 64;                     // irtkImageRigidRegistrationWithPadding::_NumberOfBins
constexpr int NMI_H = NMI_B * NMI_B;
constexpr int NMI_PER_THREAD = NMI_H / 256;   // visit-order bins per lane in the entropy pass

struct NmiBlock { int e, p0, p1, slot, nchunks, pad_; };   // planes [p0, p1) of evaluation e; slot -1 = the only block of e
struct NmiEval { int width, nbt; };

// v > 0 -> v / width (int(v / (double)width) for the shorts of a level: no quotient lies within 2^-30 of an integer)
__global__ void k_nmi_bin(short *p, size_t n, int width) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { const short v = p[i]; if (v > 0) p[i] = (short)(v / width); }
}

// the serial sum of c log c over v[0..n) in order, zero counts skipped (the table loads of 8 terms in flight, the adds in order)
__device__ double nmi_serial(const unsigned *v, int n, const double *terms) {
  double s = 0;
  int k = 0;
  for (; k + 8 <= n; k += 8) {
    double y[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) y[u] = terms[v[k + u]];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (v[k + u]) s += y[u];
  }
  for (; k < n; ++k)
    if (v[k]) s += terms[v[k]];
  return s;
}

__global__ __launch_bounds__(256) void k_nmi(const short *targets, int tx, int ty, const int *target_index, const double *mats,
                                             const short *source, int vx, int vy, int vz, const NmiBlock *blocks,
                                             const NmiEval *evals, int nbs, const double *terms, unsigned *merge,
                                             unsigned *counters, double *out4, unsigned *hist_out) {
  __shared__ unsigned h[NMI_H];
  __shared__ unsigned marg_x[NMI_B], marg_y[NMI_B];
  __shared__ int wave_nz[4];
  __shared__ unsigned bad;
  __shared__ int last;
  const NmiBlock b = blocks[blockIdx.x];
  const NmiEval ev = evals[b.e];
  const int width = ev.width, nbt = ev.nbt;
  for (int k = threadIdx.x; k < NMI_H; k += 256) h[k] = 0;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  // ---- the samples of planes [p0, p1) --------------------------------------------------------------------------------------
  const int npix = tx * ty;
  for (int pl = b.p0; pl < b.p1; ++pl) {
    const short *tgt = targets + (size_t)target_index[pl] * npix;
    const SimPlane P = sim_plane(mats, pl, source, vx, vy, vz);
    for (int p = threadIdx.x; p < npix; p += 256) {
      const int tv = tgt[p];
      if (tv < 0) continue;
      const int j = p / tx, i = p - j * tx;
      int sb;                                                  // the sampler's two-sided round(): a sample has value >= 0, where it
      if (sim_sample(P, i, j, tv, sb)) {                       // gives the same integer as (int)(value + 0.5) (irtkCommon.h:85-88)
        const int tb = tv / width;
        if (tb < nbt && sb < nbs) atomicAdd(&h[sb * nbt + tb], 1u);
        else bad = 1;                                          // irtkHistogram_2D::Add would exit: the caller's bins are wrong
      }
    }
  }
  __syncthreads();
  // ---- an evaluation split over several workgroups: merge, the last one goes on -------------------------------------------
  // Payload in and out by agent-scope integer atomics; the counter's add is released behind every wave's wait and a barrier,
  // the last arriver acquires before it takes the slot back (the counter form of the split-K hand-off).
  if (b.slot >= 0) {
    unsigned *g = merge + (size_t)b.slot * (NMI_H + 1);
    for (int k = threadIdx.x; k < nbt * nbs; k += 256) {
      const unsigned c = h[k];
      if (c) atomicAdd(&g[k], c);
    }
    if (threadIdx.x == 0 && bad) atomicOr(&g[NMI_H], 1u);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      last = atomicAdd(&counters[b.slot], 1u) == (unsigned)(b.nchunks - 1);
      if (last) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
    }
    __syncthreads();
    if (!last) return;
    for (int k = threadIdx.x; k < nbt * nbs; k += 256) h[k] = atomicExch(&g[k], 0u);
    if (threadIdx.x == 0) {
      bad = atomicExch(&g[NMI_H], 0u);
      atomicExch(&counters[b.slot], 0u);
    }
    __syncthreads();
  }
  // ---- marginals, the histogram for the tests, the nonzero joint bins in visit order ---------------------------------------
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, nb = nbt * nbs;
  if (t < nbt) {
    unsigned s = 0;
    for (int j = 0; j < nbs; ++j) s += h[j * nbt + t];
    marg_x[t] = s;
  } else if (t >= 64 && t - 64 < nbs) {
    unsigned s = 0;
    for (int i = 0; i < nbt; ++i) s += h[(t - 64) * nbt + i];
    marg_y[t - 64] = s;
  }
  unsigned c[NMI_PER_THREAD];
  int nz = 0;
#pragma unroll
  for (int q = 0; q < NMI_PER_THREAD; ++q) {
    const int k = t * NMI_PER_THREAD + q;
    c[q] = k < nb ? h[k] : 0u;
    nz += c[q] != 0;
  }
  if (hist_out) {
    unsigned *ho = hist_out + (size_t)b.e * NMI_H;
    for (int k = t; k < NMI_H; k += 256) {
      const int j = k / NMI_B, i = k % NMI_B;
      ho[k] = (j < nbs && i < nbt) ? h[j * nbt + i] : 0u;
    }
  }
  int incl = nz;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(incl, o, 64);
    if (lane >= o) incl += u;
  }
  if (lane == 63) wave_nz[w] = incl;
  __syncthreads();                                             // every lane has read h: it may be overwritten
  int at = incl - nz, nnz = 0;
  for (int q = 0; q < 4; ++q) {
    if (q < w) at += wave_nz[q];
    nnz += wave_nz[q];
  }
#pragma unroll
  for (int q = 0; q < NMI_PER_THREAD; ++q)
    if (c[q]) h[at++] = c[q];
  __syncthreads();
  // ---- three serial sums, one lane each of three wavefronts ---------------------------------------------------------------
  double *o = out4 + 4 * (size_t)b.e;
  if (t == 0) {
    o[1] = nmi_serial(h, nnz, terms);
  } else if (t == 64) {
    unsigned long long n = 0;
    for (int i = 0; i < nbt; ++i) n += marg_x[i];
    o[0] = bad ? -1.0 : (double)n;
    o[2] = nmi_serial(marg_x, nbt, terms);
  } else if (t == 128) {
    o[3] = nmi_serial(marg_y, nbs, terms);
  }
}

}  // namespace

extern "C" {

int svr_nmi_bin_source(svr_ctx *ctx, int width) {
  SVR_ENTER(ctx);
  if (!ctx || width < 1) return SVR_E_ARG;
  NEED(ctx->d_reg_source, "svr_ncc_set_source or svr_pyr_level first");
  if (width == 1) return SVR_OK;
  const size_t n = (size_t)ctx->reg_vx * ctx->reg_vy * ctx->reg_vz;
  hipLaunchKernelGGL(k_nmi_bin, dim3(nblk(n)), dim3(256), 0, ctx->stream, ctx->d_reg_source, n, width);
  KCHK("k_nmi_bin");
  return SVR_OK;
}

int svr_nmi_evaluate(svr_ctx *ctx, int n_eval, const int *planes_per_eval, const int *target_index, const double *matrices,
                     const int *target_width, const int *target_nbins, int source_nbins, double *out4, uint32_t *hist_or_null) {
  SVR_ENTER(ctx);
  if (!ctx || n_eval <= 0 || !planes_per_eval || !target_index || !matrices || !target_width || !target_nbins || !out4) return SVR_E_ARG;
  NEED(ctx->d_reg_targets && ctx->d_reg_source, "svr_ncc_set_targets / svr_ncc_set_source first");
  if (source_nbins < 1 || source_nbins > NMI_B) return fail(ctx, SVR_E_ARG, "svr_nmi_evaluate: source bins out of range");
  const size_t npix = (size_t)ctx->reg_tx * ctx->reg_ty;
  // planes per workgroup: about 16 k target pixels (a slice is always one workgroup)
  const int per_block = (int)std::max<size_t>(1, 16384 / npix);
  std::vector<NmiBlock> blocks;
  std::vector<NmiEval> evs(n_eval);
  size_t planes = 0, max_count = 0;
  int slots = 0;
  for (int e = 0; e < n_eval; ++e) {
    const int np = planes_per_eval[e];
    if (np < 1 || target_width[e] < 1 || target_nbins[e] < 1 || target_nbins[e] > NMI_B)
      return fail(ctx, SVR_E_ARG, "svr_nmi_evaluate: bad planes, width or bins of an evaluation");
    evs[e].width = target_width[e];
    evs[e].nbt = target_nbins[e];
    const int chunks = (np + per_block - 1) / per_block;
    const int slot = chunks > 1 ? slots++ : -1;
    for (int k = 0; k < chunks; ++k)
      blocks.push_back(NmiBlock{e, (int)planes + k * per_block, (int)planes + std::min(np, (k + 1) * per_block), slot, chunks, 0});
    planes += np;
    max_count = std::max(max_count, (size_t)np * npix);        // no count of an evaluation exceeds its target pixels
  }
  if (max_count >= (1ull << 32)) return fail(ctx, SVR_E_ARG, "svr_nmi_evaluate: an evaluation of 2^32 pixels or more");
  // the term table t[c] = c log c with the host's libm (the values of the host restatement), grown with the counts
  if (ctx->nmi_terms_n <= max_count) {
    const size_t n = std::max(max_count + 1, ctx->nmi_terms_n * 2);
    std::vector<double> tt(n);
    tt[0] = 0;
    for (size_t k = 1; k < n; ++k) tt[k] = (double)k * log((double)k);
    ctx->nmi_terms_n = 0;                                  // (the entries that were uploaded, not the allocation's size: none until the copy below is through)
    HIPCHK(ctx->d_nmi_terms.reserve(n));
    HIPCHK(hipMemcpyAsync(ctx->d_nmi_terms, tt.data(), n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->nmi_terms_n = n;
  }
  // merge slots and their counters: zeroed once when they grow, left zero by every call
  if ((size_t)slots > ctx->nmi_slots) {
    ctx->nmi_slots = 0;                                    // (the slots that are laid out and zeroed: where the counters start)
    const size_t cap = std::max<size_t>(64, (size_t)slots * 3 / 2);
    const size_t bytes = cap * (NMI_H + 1) * sizeof(unsigned) + cap * sizeof(unsigned);
    HIPCHK(ctx->d_nmi_merge.reserve(bytes / sizeof(unsigned)));
    HIPCHK(hipMemsetAsync(ctx->d_nmi_merge, 0, bytes, ctx->stream));
    ctx->nmi_slots = cap;
  }
  unsigned *d_merge = ctx->d_nmi_merge, *d_counters = d_merge ? d_merge + ctx->nmi_slots * (NMI_H + 1) : nullptr;
  // matrices | blocks | evaluations | target indices in; the results and (tests) the histograms out
  const size_t b_mats = planes * 16 * sizeof(double), b_blocks = blocks.size() * sizeof(NmiBlock), b_evs = evs.size() * sizeof(NmiEval),
               b_out = (size_t)n_eval * 4 * sizeof(double), b_hist = hist_or_null ? (size_t)n_eval * NMI_H * sizeof(unsigned) : 0;
  std::vector<double> h4((size_t)n_eval * 4);
  if (int rc = sim_evaluate(ctx, "svr_nmi_evaluate", target_index, planes,
                            {{matrices, b_mats}, {blocks.data(), b_blocks}, {evs.data(), b_evs}, {target_index, planes * sizeof(int)}}, h4.data(), b_out,
                            hist_or_null, b_hist, 0, [&](unsigned char *d, unsigned char *d_out, unsigned char *d_hist) {
                              hipLaunchKernelGGL(k_nmi, dim3((unsigned)blocks.size()), dim3(256), 0, ctx->stream, ctx->d_reg_targets, ctx->reg_tx, ctx->reg_ty,
                                                 reinterpret_cast<const int *>(d + b_mats + b_blocks + b_evs), reinterpret_cast<const double *>(d),
                                                 ctx->d_reg_source, (int)ctx->reg_vx, (int)ctx->reg_vy, (int)ctx->reg_vz,
                                                 reinterpret_cast<const NmiBlock *>(d + b_mats), reinterpret_cast<const NmiEval *>(d + b_mats + b_blocks),
                                                 source_nbins, ctx->d_nmi_terms, d_merge, d_counters, reinterpret_cast<double *>(d_out),
                                                 reinterpret_cast<unsigned *>(d_hist));
                            }))
    return rc;
  for (int i = 0; i < n_eval; ++i)
    if (h4[4 * (size_t)i] < 0) return fail(ctx, SVR_E_ARG, "svr_nmi_evaluate: a sample fell outside the bins (wrong widths or bin counts)");
  memcpy(out4, h4.data(), b_out);
  return SVR_OK;
}

}  // extern "C"
