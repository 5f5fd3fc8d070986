// svr_lncc.inc -- local (windowed) normalised cross correlation of the default (IRTK) registration on the device; included by
// svr_hip.hip.  A deviation from the reference, which has no local metric (--useLNCC, DESIGN 9).
//
// The samples are sim_sample's (svr_sim.inc): V = the target pixels it keeps; both operands are then integers in 0..32767.  With
// radius R the window of pixel p is the (2R+1)^2 box around it, clipped to the plane and restricted to V.  Over the window, in
// exact integers,
//   m, St, Ss, Stt, Sss, Sts,   A = m Sts - St Ss,   B = m Stt - St^2,   C = m Sss - Ss^2      (all below 2^53)
// p is counted iff p in V, m >= ((2R+1)^2 + 1) / 2 and B > 0 (the target window has structure).  A counted pixel scores q = 0 if
// C == 0, else q = (A / B) * (A / C) negated when A < 0 -- the signed squared local correlation, two IEEE double divisions and one
// multiplication -- and k = (int64) floor(q 2^24 + 0.5).  A plane's result is {N, S} = {counted pixels, sum of k}: everything
// added is an integer, so no order of summation matters and the result equals a serial restatement's bit for bit.
//
// One 256-thread workgroup per (plane, candidate), as k_ncc.  The plane is walked in bands of 32 rows (and, beyond 256 columns,
// in strips of 256 columns); every pixel of a band is sampled ONCE into LDS as one 32-bit word t | valid << 15 | s << 16 (0 = not in
// V, and 0 too for the halo outside the plane, so the window loops do not clip).  The rows live in a ring of 32 + 2R slots: a band
// samples only the rows the band before it did not, its R-row halo stays where it is.  The window sums are separable: a thread owns
// one column of a run of rows, forms the 2R+1-wide row sums of a row from LDS (consecutive lanes read consecutive words) and slides
// them down its column -- add the row entering the window, subtract the row leaving it, exact in integers -- so a pixel costs two
// row sums instead of (2R+1)^2 taps and nothing but the samples is ever stored.  m, St, Ss are 32-bit (at most 225 x 32767), the
// three product sums 64-bit (a product of two shorts fits 32 bits, 225 of them do not).  {N, S} are reduced with wave_sum_i64.
// LDS: (32 + 2R) x (columns + 2R) words, sized per launch: 15 KB for a 100-pixel-wide slice at R = 3, 49 KB at most (R = 7, 256
// columns) -- within the 64 KB a workgroup may declare statically.

namespace {

constexpr int LNCC_BH = 32;                   // output rows of a band
constexpr int LNCC_RMAX = 7;

struct LnccRow { unsigned m, st, ss; unsigned long long tt, sss, ts; };

// the 2R+1-wide sums of one ring row, window starting at word `w` (the halo columns hold 0)
__device__ __forceinline__ LnccRow lncc_row(const unsigned *w, int R) {
  LnccRow r = {0u, 0u, 0u, 0ull, 0ull, 0ull};
  for (int d = 0; d <= 2 * R; ++d) {
    const unsigned pk = w[d], t = pk & 0x7fffu, s = pk >> 16;
    r.m += (pk >> 15) & 1u; r.st += t; r.ss += s;
    r.tt += t * t; r.sss += s * s; r.ts += t * s;              // 32767^2 < 2^32
  }
  return r;
}

__global__ __launch_bounds__(256) void k_lncc(const short *targets, int tx, int ty, const int *target_index, const double *mats,
                                              const short *source, int vx, int vy, int vz, int R, int cw_log2, long long *sums2,
                                              int *kmap) {
  extern __shared__ unsigned lncc_pk[];                        // [LNCC_BH + 2R][CW + 2R], row r of the plane in slot (r + R) % NR
  __shared__ long long red[4][2];
  const int e = blockIdx.x;
  const short *tgt = targets + (size_t)target_index[e] * tx * ty;
  const SimPlane P = sim_plane(mats, e, source, vx, vy, vz);
  const int CW = 1 << cw_log2, WIN = CW + 2 * R, NR = LNCC_BH + 2 * R, SEG = (LNCC_BH * CW) >> 8;   // rows a thread walks per band
  const int c = threadIdx.x & (CW - 1), g = threadIdx.x >> cw_log2;
  const int need = ((2 * R + 1) * (2 * R + 1) + 1) / 2;
  int *km = kmap ? kmap + (size_t)e * tx * ty : nullptr;
  long long acc_n = 0, acc_s = 0;
  for (int x0 = 0; x0 < tx; x0 += CW) {                        // strips: one for every plane up to 256 columns
    for (int y0 = 0; y0 < ty; y0 += LNCC_BH) {
      // ---- sample the rows this band adds to the ring: [-R, BH + R) for the first band, [y0 + R, y0 + BH + R) after it ----
      const int r_lo = y0 == 0 ? -R : y0 + R, n_new = y0 + LNCC_BH + R - r_lo;
      for (int p = threadIdx.x; p < n_new * WIN; p += 256) {
        const int rr = p / WIN, cc = p - rr * WIN, j = r_lo + rr, i = x0 - R + cc;
        unsigned pk = 0;
        if (j >= 0 && j < ty && i >= 0 && i < tx) {
          const int tv = tgt[(size_t)j * tx + i];
          int sv;
          if (sim_sample(P, i, j, tv, sv)) pk = (unsigned)tv | 0x8000u | ((unsigned)sv << 16);
        }
        lncc_pk[((j + R) % NR) * WIN + cc] = pk;
      }
      __syncthreads();
      // ---- the windows of rows [ya, ya + SEG) of column x0 + c: row sums slid down the column -----------------------------
      const int ya = y0 + g * SEG, x = x0 + c;
      if (x < tx && ya < ty) {
        unsigned m = 0, st = 0, ss = 0;
        unsigned long long tt = 0, sss = 0, ts = 0;
        for (int j = ya - R; j < ya + R; ++j) {                // rows ya - R .. ya + R - 1; row ya + R enters below
          const LnccRow r = lncc_row(&lncc_pk[((j + R) % NR) * WIN + c], R);
          m += r.m; st += r.st; ss += r.ss; tt += r.tt; sss += r.sss; ts += r.ts;
        }
        const int yb = min(ya + SEG, ty);
        for (int y = ya; y < yb; ++y) {
          {
            const LnccRow r = lncc_row(&lncc_pk[((y + 2 * R) % NR) * WIN + c], R);     // row y + R
            m += r.m; st += r.st; ss += r.ss; tt += r.tt; sss += r.sss; ts += r.ts;
          }
          const unsigned own = lncc_pk[((y + R) % NR) * WIN + c + R];
          int k = INT_MIN;
          if ((own & 0x8000u) && (int)m >= need) {
            const long long B = (long long)m * (long long)tt - (long long)st * (long long)st;
            if (B > 0) {
              const long long A = (long long)m * (long long)ts - (long long)st * (long long)ss;
              const long long C = (long long)m * (long long)sss - (long long)ss * (long long)ss;
              double q = 0;
              if (C != 0) {
                q = ((double)A / (double)B) * ((double)A / (double)C);
                if (A < 0) q = -q;
              }
              k = (int)(long long)floor(q * 16777216.0 + 0.5);
              acc_n += 1; acc_s += k;
            }
          }
          if (km) km[(size_t)y * tx + x] = k;
          {
            const LnccRow r = lncc_row(&lncc_pk[(y % NR) * WIN + c], R);               // row y - R leaves
            m -= r.m; st -= r.st; ss -= r.ss; tt -= r.tt; sss -= r.sss; ts -= r.ts;
          }
        }
      }
      __syncthreads();                                         // the next band overwrites rows this one has read
    }
  }
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  acc_n = wave_sum_i64(acc_n);
  acc_s = wave_sum_i64(acc_s);
  if (lane == 0) { red[w][0] = acc_n; red[w][1] = acc_s; }
  __syncthreads();
  if (threadIdx.x < 2) sums2[2 * (size_t)e + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

}  // namespace

extern "C" {

int svr_lncc_evaluate(svr_ctx *ctx, int n_eval, const int *target_index, const double *matrices, int radius, int64_t *sums2,
                      int32_t *k_or_null) {
  SVR_ENTER(ctx);
  if (!ctx || n_eval <= 0 || !target_index || !matrices || !sums2) return SVR_E_ARG;
  NEED(ctx->d_reg_targets && ctx->d_reg_source, "svr_ncc_set_targets / svr_ncc_set_source first");
  if (radius < 1 || radius > LNCC_RMAX) return fail(ctx, SVR_E_ARG, "svr_lncc_evaluate: radius out of range (1..7)");
  const int tx = ctx->reg_tx, ty = ctx->reg_ty;
  const size_t npix = (size_t)tx * ty;
  // columns a workgroup takes at once: the plane's width rounded up to a power of two, 32..256 (wider planes go in strips)
  int cw_log2 = 5;
  while (cw_log2 < 8 && (1 << cw_log2) < tx) ++cw_log2;
  const size_t lds = (size_t)(LNCC_BH + 2 * radius) * ((1 << cw_log2) + 2 * radius) * sizeof(unsigned);
  static_assert((LNCC_BH + 2 * LNCC_RMAX) * (256 + 2 * LNCC_RMAX) * sizeof(unsigned) + 64 <= 65536, "k_lncc: LDS beyond a static allocation");
  // matrices | target indices in; {N, S} and (tests) the k maps out
  const size_t b_mats = (size_t)n_eval * 16 * sizeof(double), b_map = k_or_null ? (size_t)n_eval * npix * sizeof(int) : 0;
  std::vector<long long> h((size_t)n_eval * 2);
  if (int rc = sim_evaluate(ctx, "svr_lncc_evaluate", target_index, n_eval, {{matrices, b_mats}, {target_index, n_eval * sizeof(int)}}, h.data(),
                            h.size() * sizeof(long long), k_or_null, b_map, 0, [&](unsigned char *d, unsigned char *d_out, unsigned char *d_map) {
                              hipLaunchKernelGGL(k_lncc, dim3(n_eval), dim3(256), lds, ctx->stream, ctx->d_reg_targets, tx, ty,
                                                 reinterpret_cast<const int *>(d + b_mats), reinterpret_cast<const double *>(d), ctx->d_reg_source,
                                                 (int)ctx->reg_vx, (int)ctx->reg_vy, (int)ctx->reg_vz, radius, cw_log2,
                                                 reinterpret_cast<long long *>(d_out), reinterpret_cast<int *>(d_map));
                            }))
    return rc;
  for (size_t i = 0; i < h.size(); ++i) sums2[i] = h[i];
  return SVR_OK;
}

}  // extern "C"
