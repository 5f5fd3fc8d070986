"""The launch-geometry choices of the kernels that retile themselves by the data's shape, restated from the host code of
csrc/svr_hip.hip and csrc/svr_bias.inc, for the shape sweeps (tests/test_shape_sweep_gpu.py) and their CPU checks
(tests/test_shape_refs.py), and the numpy references the sweeps compare with.  Each sweep case derives its boundary shapes from these and asserts, through the read-only
options the library records (bias_field_bx, bias_tail_*, reg_zc, reg_chunks), that it reached the branch it was built for."""
import numpy as np

BIAS_HMAX = 255                 # svr_bias.inc: the widest half-width of the LDS kernels
BIAS_LDS_TAIL_MIN = 1 << 22     # svr_bias.inc: bias_mode 1 takes the LDS tail from this many voxels on
LDS_CAP = 65536                 # bytes of LDS a workgroup may use
CHUNK_PIX = 2048                # svr_small.inc: pixels per block of the per-slice EM reductions
REG_TILES = ((64, 8), (32, 16), (32, 8))   # reg_tile 0, 1, 2 (-1 = 2)


def gauss_half(sigma, dim):
    """half-width of k_gauss_conv_slices / k_gauss3d / gauss_half_host: the float arithmetic of the kernels"""
    sigma2 = np.float32(np.float32(sigma) / np.float32(dim))
    klength = 2 * int(np.floor(float(np.float32(4) * sigma2) + 0.5)) + 1     # roundf (sigma2 > 0)
    klength -= 1 - klength % 2
    return (klength - 1) // 2


def gauss_weights(sigma, dim):
    """the kernels' float32 recurrence g0 *= g1; g1 *= g2 -> (g[0 .. half], sum_coeff), both float32"""
    sigma2 = np.float32(np.float32(sigma) / np.float32(dim))
    half = gauss_half(sigma, dim)
    g0 = np.float32(1.0 / (np.sqrt(2.0 * np.pi) * float(sigma2)))
    g1 = np.float32(np.exp(-0.5 / float(np.float32(sigma2 * sigma2))))
    g2 = np.float32(g1 * g1)
    g = [g0]
    sum_coeff = g0
    for _ in range(half):
        g0 = np.float32(g0 * g1)
        g1 = np.float32(g1 * g2)
        g.append(g0)
        sum_coeff = np.float32(sum_coeff + np.float32(2) * g0)
    return np.array(g, np.float32), sum_coeff


# ---- CorrectBias: k_bias_field_lds (svr_correct_bias) -----------------------------------------------------------------
def bias_field_lds_bytes(sy, bx, half):
    return 4 * (BIAS_HMAX + 1 + 2 * sy * bx + 2 * (256 // bx) * (bx + 2 * half))


def bias_field_bx(sy, half):
    """the strip width CorrectBias launches with for slices of sy rows and the largest per-slice half-width; 0 = the stencils"""
    for b in (64, 32, 16, 8):
        if half <= BIAS_HMAX and bias_field_lds_bytes(sy, b, half) <= LDS_CAP:
            return b
    return 0


def bias_field_max_sy(bx, half):
    """the most rows a strip of bx columns takes at this half-width"""
    return (LDS_CAP // 4 - (BIAS_HMAX + 1) - 2 * (256 // bx) * (bx + 2 * half)) // (2 * bx)


# ---- NormaliseBias tail: k_gauss3d_x_lds / k_gauss3d_col_lds (svr_normalise_bias_finish) ------------------------------
_TAIL_FLOATS = (LDS_CAP - (BIAS_HMAX + 1) * 4) // 4      # floats of LDS beside the weight table


def tail_rows(vx):
    return next((r for r in (16, 8, 4, 2, 1) if r * vx <= _TAIL_FLOATS), 0)


def tail_strip(n):
    """y / z strip width for an axis of n voxels (0: none fits)"""
    return next((b for b in (64, 32, 16, 8, 4) if n * b <= _TAIL_FLOATS), 0)


def tail_strip_max(b):
    return _TAIL_FLOATS // b


def tail_rows_max(r):
    return _TAIL_FLOATS // r


def tail_choice(vsize, vdim, sigma, bias_mode):
    """-> (lds, rows, bxy, bxz) as svr_normalise_bias_finish picks them; lds 0 = the stencils (rows = bxy = bxz = 0)"""
    vx, vy, vz = vsize
    if bias_mode == 0 or (bias_mode == 1 and vx * vy * vz < BIAS_LDS_TAIL_MIN):
        return 0, 0, 0, 0
    half = max(gauss_half(sigma, d) for d in vdim)
    rows, bxy, bxz = tail_rows(vx), tail_strip(vy), tail_strip(vz)
    if half <= BIAS_HMAX and rows and bxy and bxz:
        return 1, rows, bxy, bxz
    return 0, 0, 0, 0


# ---- the fused volume update: k_regul_fused (superresolution_update_planes) --------------------------------------------
def reg_tile_shape(reg_tile):
    return REG_TILES[2 if reg_tile < 0 else reg_tile]


def reg_chunking(vx, vy, nz, reg_tile):
    """-> (zc, chunks): planes per workgroup and workgroups along z"""
    tw, th = reg_tile_shape(reg_tile)
    tiles = -(-vx // tw) * -(-vy // th)
    want = max(1, (2048 * 512 // (tw * th) + tiles - 1) // tiles)
    zc = min(32, max(4, -(-nz // want)))
    return zc, -(-nz // zc)


# ---- the per-slice EM reductions ------------------------------------------------------------------------------------------
def em_chunks(sx, sy):
    return -(-(sx * sy) // CHUNK_PIX)


# ---- numpy references of the NormaliseBias tail and the EM reductions ------------------------------------------------------
# (checked against the C oracle by tests/test_shape_refs.py, so that a sweep failure points at a kernel, not at its reference)
def conv_axis(a, sigma, dim, axis):
    """one pass of k_gauss_conv3d in float64 with the kernels' float32 weights and border repeat (clamped indices)"""
    g, sc = gauss_weights(sigma, dim)
    a = np.asarray(a, np.float64)
    n = a.shape[axis]
    idx = np.arange(n)
    out = float(g[0]) * a
    for i in range(1, len(g)):
        out = out + float(g[i]) * np.take(a, np.minimum(idx + i, n - 1), axis=axis)
        out = out + float(g[i]) * np.take(a, np.maximum(idx - i, 0), axis=axis)
    return out / float(sc)


def smooth3d(a, sigma, vdim):
    """X -> Y -> Z of a (z, y, x) volume, vdim = (dx, dy, dz)"""
    a = conv_axis(a, sigma, vdim[0], 2)
    a = conv_axis(a, sigma, vdim[1], 1)
    return conv_axis(a, sigma, vdim[2], 0)


def normalise_tail(field, volw, maskC, recon, sigma, vdim):
    """divS by the weights -> X -> Y -> Z -> divS by maskC -> divexp, NaN-free inputs -> (bias_vol, recon), float64"""
    f = np.asarray(field, np.float64)
    bv = np.where(volw != 0, f / np.where(volw != 0, volw, 1), 0.0)
    m = smooth3d(bv, sigma, vdim)
    b = np.where(maskC != 0, m / np.where(maskC != 0, maskC, 1), 0.0)
    r = np.asarray(recon, np.float64)
    return b, np.where(recon != -1, r / np.exp(-b), r)


F32 = np.float32


def _valid(slices, simweights, double_compare):
    sw = simweights
    return (slices != F32(-1)) & ((sw.astype(np.float64) > 0.99) if double_compare else (sw > F32(0.99)))


def _ebias(slices, bias):
    return slices if bias is None else slices * np.exp(-bias).astype(F32)


def mstep_sums(slices, weights, simslices, simweights, scales, bias=None):
    """transformMStep3D(NoBias) + the reduce, identities (0, 0, 0, 0, 0): {sum e^2 w, sum w, count, min e, max e}; the
    per-pixel terms in float32 in the kernels' order"""
    ok = _valid(slices, simweights, bias is not None)
    e = (_ebias(slices, bias) * scales[:, None, None].astype(F32)) - simslices
    e, w = e[ok], weights[ok]
    t = (e * e) * w
    return np.array([np.sum(t, dtype=np.float64), np.sum(w, dtype=np.float64), float(ok.sum()),
                     min(0.0, float(e.min())) if e.size else 0.0, max(0.0, float(e.max())) if e.size else 0.0])


def scale_vector(slices, weights, simslices, simweights, bias=None):
    """transformScale(noBias) per slice: den != 0 ? (float)num / (float)den : 1"""
    ok = (slices != F32(-1)) & (simweights > F32(0.99))
    if bias is None:
        num, den = (weights * slices) * simslices, (weights * slices) * slices
    else:
        eb = np.exp(-bias).astype(F32)
        num, den = ((weights * slices) * eb) * simslices, (((weights * slices) * eb) * slices) * eb
    num = np.where(ok, num, 0).sum(axis=(1, 2), dtype=np.float64).astype(F32)
    den = np.where(ok, den, 0).sum(axis=(1, 2), dtype=np.float64).astype(F32)
    return np.where(den != 0, num / np.where(den != 0, den, 1), F32(1)).astype(F32)


def robust_sums(slices, siminside, simslices, simweights):
    ok = (slices != F32(-1)) & (siminside == 1) & (simweights.astype(np.float64) > 0.99)
    d = (slices - simslices)[ok]
    return np.array([np.sum(d * d, dtype=np.float64), float(ok.sum())])


def scalevol_sums(slices, weights, simslices, simweights, slice_weights):
    ok = (slices != F32(-1)) & (simweights.astype(np.float64) > 0.99)
    ws = weights * slice_weights[:, None, None].astype(F32)
    return np.array([np.sum(((ws * slices) * simslices)[ok], dtype=np.float64), np.sum(((ws * simslices) * simslices)[ok], dtype=np.float64)])


def estep(slices, simslices, simweights, scales, m, sigma, mix, bias=None, step=F32(0.0001)):
    """EStepKernel3D + the slice potentials -> (weights, potential) in float32"""
    m, sigma, mix = F32(m), F32(sigma), F32(mix)
    ok = (slices != F32(-1)) & (simweights > F32(0))
    v = (_ebias(slices, bias) * scales[:, None, None].astype(F32)) - simslices
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        g = step * np.exp(-v * v / (F32(2) * sigma)).astype(F32) / np.sqrt(F32(6.28) * sigma)
        w = (g * mix) / (g * mix + (m * step) * (F32(1) - mix))
    w = np.where(ok, w, F32(0)).astype(F32)
    pot_ok = simweights.astype(np.float64) > 0.99
    t = 1.0 - w.astype(np.float64)
    a = np.where(pot_ok, (t * t).astype(F32).astype(np.float64), 0).sum(axis=(1, 2))
    b = pot_ok.sum(axis=(1, 2)).astype(np.float64)
    pot = np.where(b > 0, np.sqrt(a.astype(F32) / np.where(b > 0, b, 1).astype(F32)), F32(-1)).astype(F32)
    return w, pot
