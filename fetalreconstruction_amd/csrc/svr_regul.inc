// svr_regul.inc -- the volume update of one SR iteration as ONE kernel (#included by svr_hip.hip, inside its anonymous namespace).
//
// Replaces AdaptiveRegularizationPrep + AdaptiveRegularizationKernel (reconstruction_cuda2.cu:1944-1969, 2046-2117; the
// directions and factors of :666-695).  The reference runs it on GPU 0 only and a sharded run here used to run it replicated on
// every rank, so its time does not divide by the number of ranks: round 3 measured it at 5 % of its 24 B/voxel HBM roofline
// (S8 1.16 ms, PVR8spx 2.94 ms) -- two passes, 81 uncached neighbour loads and 26 fp64 sqrt + fp64 divisions per voxel.
//
// k_regul_fused<ADAPTIVE>:
//  * a workgroup of 512 lanes owns a tile of 64 x 8 voxels and marches along z over `zc` planes.  Four planes of the tile + halo
//    (66 x 10) live in a ring in the LDS as float2 {o', s c} per voxel: o' = original, or NaN where the post-Prep confidence is
//    <= 0 or the voxel lies outside the volume; s c = post-Prep value x confidence.  Every voxel is loaded (and its Prep
//    evaluated) once per workgroup instead of 27 x per launch; plane z + 2 travels from HBM while plane z is evaluated; one
//    barrier per plane.
//  * the weight of a neighbour pair, b = f / sqrt(1 + diff^2) (RC.cu:2046-2057: float diff, double sqrt and division), is
//    f * v_rsq_f32(fma(t, t f/delta^2, 1)) in float32 -- two pairs per packed instruction (v_pk_add / v_pk_mul / v_pk_fma).  The
//    conditions `cmap <= 0 -> b = 0` and `neighbour outside the volume -> no term` are the NaN of o': a NaN difference gives a NaN
//    b, and the multiplication's clamp modifier writes 0 for NaN (DX10_CLAMP; b lies in (0, 1] otherwise) -- no compare, no branch.
//    Relative error of b <= 2e-7, entering the result scaled by alpha lambda / delta^2 <= 0.068: the stated tolerance of row a7
//    is 1e-6 of the volume's maximum (tests/test_parity_gpu.py::test_regulariser_parity; observed ~1e-7).
//  * Prep's in-place changes of addon / cmap (non-adaptive: addon /= cmap, cmap = 1 where cmap != 0) are NOT written by this
//    kernel (neighbouring workgroups read the same voxels: an in-place write would race, and nothing on the path reads them
//    again -- the next back-projection clears both).  A reader of the two buffers (svr_debug_get, svr_device_ptr) gets them
//    settled first (k_regul_settle); the product path never pays for it.
//  * the output goes to the other of two volume buffers (svr_ctx::recon() flips): no copy back.
//  * workgroups whose tile lies outside the mask's bounding box grown by one voxel write zeros without loading anything: the
//    scatter writes mask voxels only, so cmap is 0 there and every weight vanishes (valW = 0 -> 0, RC.cu:2113-2116).  Only while
//    cmap is the scatter's own (svr_ctx::cmap_from_scatter; a debug_set of the buffer switches the shortcut off).
//  * z range [z_lo, z_hi): a sharded run regularises its own slab (reduce-scatter -> slab -> all-gather, svr_shard.h).
//
//  * GUIDED (a channel's update under svr_channel_sr_guide, svr_channel.inc): a fourth array in the ring holds the guide G as loaded -- it
//    never gates, so it is not folded into o' --, loaded with the other three per halo voxel and read as ds_read2_b32 pairs like o'; the
//    weight becomes f * v_rsq_f32(fma(tg, tg f/delta_g^2, fma(t, t omega f/delta^2, 1))), omega = 0 for "guide only" (a constant, not a
//    branch).  The unguided kernels reference neither the array nor the arguments (`if constexpr`): their code is unchanged.
//
// A voxel of `original` that is NaN where the confidence is positive poisons its neighbourhood in the reference and is treated as
// "no confidence" here; volumes with NaNs are outside the contract.

struct RegulArgs {
  const float *recon, *addon, *cmap;   // original (pre-update volume), scatter results
  float *out;                          // updated volume
  int vx, vy, vz;
  int z_lo, z_hi, zc;                  // output planes [z_lo, z_hi), planes per workgroup
  int blo[3], bhi[3];                  // outputs outside this box (inclusive) are 0 (bhi < blo: no shortcut)
  float alpha, thr_lo, val_lo, thr_hi, val_hi;
  float k;                             // alpha * lambda / delta^2
  float kap1, kap2, kap3;              // f / delta^2 for f = 1, 1/2, 1/3
  // read by the GUIDED kernels only (a channel's update under svr_channel_sr_guide): the weight of a pair becomes
  // f / sqrt(1 + omega f (dC / delta)^2 + f (dG / delta_g)^2), G = `guide` on the volume's grid
  const float *guide;
  float gkap1, gkap2, gkap3;           // f / delta_g^2 for f = 1, 1/2, 1/3
  float omega;                         // 1: joint, 0: the guide's differences alone (kap1..3 enter as omega * kap: no branch)
};

// tile of a workgroup: TX x TY voxels, one lane per voxel; the halo plane is (TX + 2) x (TY + 2)
template <int TX, int TY>
struct RegulTile {
  static constexpr int NT = TX * TY, PW = TX + 2, PH = TY + 2, PE = PW * PH;
  static_assert(PE <= 2 * NT && 2 * PW + 2 < 256, "two halo voxels per lane; ds_read2_b32 offsets");
};

__device__ __forceinline__ f2 mk2(float a, float b) { f2 v = {a, b}; return v; }
__device__ __forceinline__ f2 regul_rsq2(f2 w) { return mk2(__builtin_amdgcn_rsqf(w.x), __builtin_amdgcn_rsqf(w.y)); }
// y * f with NaN -> 0 (the clamp modifier under DX10_CLAMP, the default of compute kernels); y * f lies in (0, 1]
__device__ __forceinline__ f2 regul_mul_clamp(f2 y, f2 f) {
  f2 b;
  asm("v_pk_mul_f32 %0, %1, %2 clamp" : "=v"(b) : "v"(y), "v"(f));
  return b;
}

// One voxel of a halo plane on its way from HBM to the LDS: the three loads are issued early (from an always valid address:
// no divergent branch; the plane's base is wave-uniform, the lane's in-plane offset fixed), Prep (RC.cu:1944-1969) is evaluated
// when the plane is stored, i.e. after the plane in between has been worked on.
struct RegulRaw { float o, ad, c; };
struct RegulLane { uint32_t off; bool ok; };            // in-plane element offset (clamped into the volume), inside the volume in x and y
__device__ __forceinline__ RegulLane regul_lane(const RegulArgs &a, int gx, int gy) {
  RegulLane l;
  l.ok = gx >= 0 && gx < a.vx && gy >= 0 && gy < a.vy;
  l.off = (uint32_t)min(max(gx, 0), a.vx - 1) + (uint32_t)min(max(gy, 0), a.vy - 1) * (uint32_t)a.vx;
  return l;
}
__device__ __forceinline__ RegulRaw regul_load(const RegulArgs &a, const RegulLane &l, int z) {
  const size_t pl = (size_t)min(max(z, 0), a.vz - 1) * ((size_t)a.vx * a.vy);      // wave-uniform
  RegulRaw r;
  r.o = (a.recon + pl)[l.off];
  r.ad = (a.addon + pl)[l.off];
  r.c = (a.cmap + pl)[l.off];
  return r;
}
// GUIDED: the guide's voxel, in flight with the three.  It never gates: outside the volume the clamped address's value, next to a NaN o'
__device__ __forceinline__ float regul_load_guide(const RegulArgs &a, const RegulLane &l, int z) {
  const size_t pl = (size_t)min(max(z, 0), a.vz - 1) * ((size_t)a.vx * a.vy);
  return (a.guide + pl)[l.off];
}
// -> o' (NaN: no confidence / outside), s c, and the post-Prep confidence
template <bool ADAPTIVE>
__device__ __forceinline__ void regul_prep(const RegulArgs &a, const RegulRaw &w, bool ok, float &o, float &sc, float &c) {
  float ad = w.ad;
  c = w.c;
  if (!ADAPTIVE) {
    // addon / cmap (RC.cu:1955) as addon * rcp(cmap): 1 ulp of v_rcp_f32 on a term that enters scaled by alpha (the reference
    // binary's own division is the approximate one of --use_fast_math); k_regul_settle hands readers of addon the IEEE quotient
    const bool nz = c != 0.0f;
    ad = nz ? ad * __builtin_amdgcn_rcpf(c) : ad;
    c = nz ? 1.0f : c;
  }
  float r = w.o + ad * a.alpha;
  r = r < a.thr_lo ? a.val_lo : r;       // (double)r < (double)min * 0.9 with the threshold worked out on the host: regul_thresholds
  r = r > a.thr_hi ? a.val_hi : r;
  c = ok ? c : 0.0f;
  o = c > 0.0f ? w.o : __builtin_nanf("");
  sc = ok ? r * c : 0.0f;
}

// the weights of two neighbour pairs and their terms: t = the two differences of `original` (RC.cu:2052), s2 = the two s c;
// GUIDED: tg = the two differences of the guide, one more fma in front of the same v_rsq (a NaN of t still switches the pair off)
template <bool ADAPTIVE, bool GUIDED = false>
__device__ __forceinline__ void regul_terms(f2 t, f2 kap, f2 f, f2 s2, f2 c2, f2 &acc, f2 &accw, f2 &sum2, f2 tg = f2{}, f2 kapg = f2{}) {
  f2 w = fma2(t, t * kap, bc2(1.0f));
  if constexpr (GUIDED) w = fma2(tg, tg * kapg, w);
  const f2 b = regul_mul_clamp(regul_rsq2(w), f);
  acc = fma2(b, s2, acc);
  if (ADAPTIVE) accw = fma2(b, c2, accw);
  sum2 = sum2 + b;
}

template <bool ADAPTIVE, int TX, int TY, bool GUIDED = false>
__global__ __launch_bounds__(TX * TY) void k_regul_fused(const RegulArgs a) {
  using T = RegulTile<TX, TY>;
  constexpr int PW = T::PW, PE = T::PE, NT = T::NT;
  // four planes in a ring, structure of arrays: two neighbours of one plane come out of one ds_read2_b32 as a register pair
  __shared__ float sho[4][PE], shs[4][PE];
  __shared__ float shc[ADAPTIVE ? 4 : 1][ADAPTIVE ? PE : 1];
  __shared__ float shg[GUIDED ? 4 : 1][GUIDED ? PE : 1];     // the guide, as loaded (referenced by the GUIDED kernels only)
  const int tid = threadIdx.x, tx = tid % TX, ty = tid / TX;
  const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
  const int zs = a.z_lo + blockIdx.z * a.zc, ze = min(zs + a.zc, a.z_hi);
  const int x = x0 + tx, y = y0 + ty;
  const bool mine = x < a.vx && y < a.vy;
  float *outp = a.out + ((size_t)min(x, a.vx - 1) + (size_t)min(y, a.vy - 1) * a.vx);
  const size_t plane = (size_t)a.vx * a.vy;
  if (a.bhi[0] >= a.blo[0] &&
      (x0 > a.bhi[0] || x0 + TX - 1 < a.blo[0] || y0 > a.bhi[1] || y0 + TY - 1 < a.blo[1] || zs > a.bhi[2] || ze - 1 < a.blo[2])) {
    if (mine)
      for (int z = zs; z < ze; ++z) outp[(size_t)z * plane] = 0.0f;
    return;
  }
  // the two halo-plane voxels this lane brings in per plane
  const int i0 = tid, i1 = tid + NT;
  const bool has1 = i1 < PE;
  const RegulLane l0 = regul_lane(a, x0 + i0 % PW - 1, y0 + i0 / PW - 1);
  const RegulLane l1 = regul_lane(a, x0 + (has1 ? i1 % PW : 0) - 1, y0 + (has1 ? i1 / PW : 0) - 1);
  auto stash_raw = [&](int z, const RegulRaw &r0, const RegulRaw &r1) {
    const int s = z & 3;
    const bool zok = z >= 0 && z < a.vz;
    float o, sc, c;
    regul_prep<ADAPTIVE>(a, r0, l0.ok && zok, o, sc, c);
    sho[s][i0] = o; shs[s][i0] = sc;
    if (ADAPTIVE) shc[s][i0] = c;
    if (has1) {
      regul_prep<ADAPTIVE>(a, r1, l1.ok && zok, o, sc, c);
      sho[s][i1] = o; shs[s][i1] = sc;
      if (ADAPTIVE) shc[s][i1] = c;
    }
  };
  auto stash_guide = [&](int z, float g0, float g1) {         // GUIDED: as loaded
    shg[z & 3][i0] = g0;
    if (has1) shg[z & 3][i1] = g1;
  };
  {                                                          // the first three planes: all loads in flight together
    RegulRaw p0[3], p1[3];
    float pg0[3], pg1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      p0[k] = regul_load(a, l0, zs - 1 + k);
      p1[k] = regul_load(a, l1, zs - 1 + k);
      if constexpr (GUIDED) { pg0[k] = regul_load_guide(a, l0, zs - 1 + k); pg1[k] = regul_load_guide(a, l1, zs - 1 + k); }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      stash_raw(zs - 1 + k, p0[k], p1[k]);
      if constexpr (GUIDED) stash_guide(zs - 1 + k, pg0[k], pg1[k]);
    }
  }
  __syncthreads();
  // d_directions (RC.cu:666-680) by plane: in the plane dz, A = {(1,0), (0,1)} and B = {(1,1), (1,-1)} as pairs (one weight class
  // each: |d|_1 = 1 + |dz| and 2 + |dz|), and (0,0,1) on its own.  `base` + these offsets = the neighbours; the opposite
  // neighbours (pos3 = pos - d) sit in the plane -dz at the mirrored offsets.
  const int base = ty * PW + tx;                             // halo voxel (tx - 1 + 1, ty - 1 + 1) - (PW + 1)
  constexpr int C = PW + 1, A0 = C + 1, A1 = C + PW, B0 = C + PW + 1, B1 = C - PW + 1;          // (1,0) (0,1) (1,1) (1,-1)
  constexpr int mA0 = C - 1, mA1 = C - PW, mB0 = C - PW - 1, mB1 = C + PW - 1;                  // mirrored
  const f2 f1 = bc2(1.0f), f2_ = bc2(0.5f), f3 = bc2(1.0f / 3.0f);
  f2 k1 = bc2(a.kap1), k2 = bc2(a.kap2), k3 = bc2(a.kap3);
  f2 g1 = bc2(0.0f), g2 = g1, g3 = g1;
  if constexpr (GUIDED) {
    k1 = bc2(a.kap1 * a.omega); k2 = bc2(a.kap2 * a.omega); k3 = bc2(a.kap3 * a.omega);
    g1 = bc2(a.gkap1); g2 = bc2(a.gkap2); g3 = bc2(a.gkap3);
  }
  for (int z = zs; z < ze; ++z) {
    const bool more = z + 1 < ze;
    RegulRaw w0, w1;
    if (more) { w0 = regul_load(a, l0, z + 2); w1 = regul_load(a, l1, z + 2); }
    float wg0, wg1;
    if constexpr (GUIDED) if (more) { wg0 = regul_load_guide(a, l0, z + 2); wg1 = regul_load_guide(a, l1, z + 2); }     // in flight while plane z is evaluated
    const int sm = (z - 1) & 3, s0 = z & 3, sp = (z + 1) & 3;
    const float *om = sho[sm] + base, *o0 = sho[s0] + base, *op = sho[sp] + base;
    const float *qm = shs[sm] + base, *q0 = shs[s0] + base, *qp = shs[sp] + base;
    const float *cm = shc[ADAPTIVE ? sm : 0] + (ADAPTIVE ? base : 0), *c0 = shc[ADAPTIVE ? s0 : 0] + (ADAPTIVE ? base : 0),
                *cp = shc[ADAPTIVE ? sp : 0] + (ADAPTIVE ? base : 0);
    // every neighbour pair of the three planes first, in the order in which their loads pair up as ds_read2_b32 (two neighbours
    // of one plane -> one register pair, no moves), the centre column last
    struct PairIn { f2 o2, o3, q2, q3, c2, c3, g2, g3; };
    PairIn in[6];
#define REGUL_LOAD(k, P_o, P_q, P_c, M_o, M_q, M_c, i, j, mi, mj)                                       \
    in[k].o2 = mk2(P_o[i], P_o[j]); in[k].o3 = mk2(M_o[mi], M_o[mj]);                                   \
    in[k].q2 = mk2(P_q[i], P_q[j]); in[k].q3 = mk2(M_q[mi], M_q[mj]);                                   \
    if (ADAPTIVE) { in[k].c2 = mk2(P_c[i], P_c[j]); in[k].c3 = mk2(M_c[mi], M_c[mj]); }
    REGUL_LOAD(0, om, qm, cm, op, qp, cp, A0, A1, mA0, mA1)             // (1,0,-1) (0,1,-1)
    REGUL_LOAD(1, om, qm, cm, op, qp, cp, B0, B1, mB0, mB1)             // (1,1,-1) (1,-1,-1)
    REGUL_LOAD(2, o0, q0, c0, o0, q0, c0, A0, A1, mA0, mA1)             // (1,0,0) (0,1,0)
    REGUL_LOAD(3, o0, q0, c0, o0, q0, c0, B0, B1, mB0, mB1)             // (1,1,0) (1,-1,0)
    REGUL_LOAD(4, op, qp, cp, om, qm, cm, A0, A1, mA0, mA1)             // (1,0,1) (0,1,1)
    REGUL_LOAD(5, op, qp, cp, om, qm, cm, B0, B1, mB0, mB1)             // (1,1,1) (1,-1,1)
#undef REGUL_LOAD
    f2 gz = bc2(0.0f), gp2 = gz, gz2 = gz;                             // the guide's pairs, read like sho's
    if constexpr (GUIDED) {
      const float *gm = shg[sm] + base, *g0 = shg[s0] + base, *gp = shg[sp] + base;
#define REGUL_LOAD_G(k, P_g, M_g, i, j, mi, mj) in[k].g2 = mk2(P_g[i], P_g[j]); in[k].g3 = mk2(M_g[mi], M_g[mj]);
      REGUL_LOAD_G(0, gm, gp, A0, A1, mA0, mA1)
      REGUL_LOAD_G(1, gm, gp, B0, B1, mB0, mB1)
      REGUL_LOAD_G(2, g0, g0, A0, A1, mA0, mA1)
      REGUL_LOAD_G(3, g0, g0, B0, B1, mB0, mB1)
      REGUL_LOAD_G(4, gp, gm, A0, A1, mA0, mA1)
      REGUL_LOAD_G(5, gp, gm, B0, B1, mB0, mB1)
#undef REGUL_LOAD_G
      gz = mk2(g0[C], gm[C]); gp2 = bc2(g0[C]); gz2 = bc2(gp[C]);
    }
    const f2 oz = mk2(o0[C], om[C]), qz = mk2(qp[C], qm[C]);            // (0,0,1): (pos, pos3) and the two s c
    const float o_p = oz.x, o2z = op[C], sc_p = q0[C];
    const f2 op2 = bc2(o_p);
    f2 acc = bc2(0.0f), accw = bc2(0.0f), sum2 = bc2(0.0f);
    // (pos, pos2): t = o2 - o_p; (pos3, pos2): t = o2 - o3 (RC.cu:2082, 2095)
    const f2 kaps[6] = {k2, k3, k1, k2, k2, k3}, fs[6] = {f2_, f3, f1, f2_, f2_, f3};
    if constexpr (GUIDED) {
      const f2 gks[6] = {g2, g3, g1, g2, g2, g3};
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        regul_terms<ADAPTIVE, true>(in[k].o2 - op2, kaps[k], fs[k], in[k].q2, in[k].c2, acc, accw, sum2, in[k].g2 - gp2, gks[k]);
        regul_terms<ADAPTIVE, true>(in[k].o2 - in[k].o3, kaps[k], fs[k], in[k].q3, in[k].c3, acc, accw, sum2, in[k].g2 - in[k].g3, gks[k]);
      }
      regul_terms<ADAPTIVE, true>(bc2(o2z) - oz, k1, f1, qz, ADAPTIVE ? mk2(cp[C], cm[C]) : op2, acc, accw, sum2, gz2 - gz, g1);
    } else {
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        regul_terms<ADAPTIVE>(in[k].o2 - op2, kaps[k], fs[k], in[k].q2, in[k].c2, acc, accw, sum2);
        regul_terms<ADAPTIVE>(in[k].o2 - in[k].o3, kaps[k], fs[k], in[k].q3, in[k].c3, acc, accw, sum2);
      }
      regul_terms<ADAPTIVE>(bc2(o2z) - oz, k1, f1, qz, ADAPTIVE ? mk2(cp[C], cm[C]) : op2, acc, accw, sum2);   // (0,0,1): its two terms as one pair
    }
    const float sum = sum2.x + sum2.y;
    const float c_p = ADAPTIVE ? c0[C] : (o_p == o_p ? 1.0f : 0.0f);
    float val = (acc.x + acc.y) - sum * sc_p;               // RC.cu:2104-2105
    float valW = (ADAPTIVE ? accw.x + accw.y : sum) - sum * c_p;
    val = sc_p + a.k * val;                                 // RC.cu:2107-2111
    valW = c_p + a.k * valW;
    if (mine) outp[(size_t)z * plane] = valW > 0.0f ? val / valW : 0.0f;
    if (more) stash_raw(z + 2, w0, w1);                      // slot of plane z - 2: last read before the previous barrier
    if constexpr (GUIDED) if (more) stash_guide(z + 2, wg0, wg1);
    __syncthreads();
  }
}

// Prep's own changes of addon / cmap (RC.cu:1952-1960), for a reader of the two buffers
__global__ void k_regul_settle(float *addon, float *cmap, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float c = cmap[i];
  if (c != 0.0f) { addon[i] = addon[i] / c; cmap[i] = 1.0f; }
}
