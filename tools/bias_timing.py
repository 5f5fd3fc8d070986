"""Time the bias path: one SR iteration of the C++ host object with bias correction on and off, and CorrectBias / the NormaliseBias
tail with the new kernels (bias_mode 2) against round 1's (bias_mode 0), and the NormaliseBias scatter in both modes, on P4 and S8 with a smooth multiplicative field on the
slices.  Times are HIP events recorded on the engine's stream around the call alone (its inputs are uploaded before the start
event): the stream's span from the first kernel's launch to the last one's end, gaps between launches included.  Warm-up first,
then median and spread (min .. max) over repeats.
usage: python tools/bias_timing.py [P4 S8 ...] [--repeats 7] [--out profiles/bias_timing.json]
For per-kernel times run it under `rocprofv3 --kernel-trace --stats -- python tools/bias_timing.py P4 --kernels-only`, one workload
per trace."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from fetalreconstruction_amd import engine, host, workloads  # noqa: E402

_hip = C.CDLL("libamdhip64.so")


def _sync():
    assert _hip.hipDeviceSynchronize() == 0


def _biased(P):
    import copy
    Q = copy.copy(P)
    ns, sy, sx = P.slices.shape
    yy, xx = np.meshgrid(np.linspace(-1, 1, sy), np.linspace(-1, 1, sx), indexing="ij")
    field = np.exp(0.25 * xx - 0.15 * yy)[None] * (1 + 0.05 * np.sin(np.arange(ns))[:, None, None])
    Q.slices = np.where(P.slices > 0, P.slices * field, P.slices).astype(np.float32)
    return Q


_STREAM = [None]


def _timed(fn, repeats, warmup=2, setup=None):
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert _hip.hipEventCreate(C.byref(ev0)) == 0 and _hip.hipEventCreate(C.byref(ev1)) == 0
    for _ in range(warmup):
        if setup:
            setup()
        fn()
    t = []
    for _ in range(repeats):
        if setup:
            setup()
        _sync()
        assert _hip.hipEventRecord(ev0, _STREAM[0]) == 0
        fn()
        assert _hip.hipEventRecord(ev1, _STREAM[0]) == 0
        assert _hip.hipEventSynchronize(ev1) == 0
        ms = C.c_float()
        assert _hip.hipEventElapsedTime(C.byref(ms), ev0, ev1) == 0
        t.append(ms.value)
    _hip.hipEventDestroy(ev0)
    _hip.hipEventDestroy(ev1)
    return {"median_ms": float(np.median(t)), "min_ms": float(np.min(t)), "max_ms": float(np.max(t)), "repeats": repeats}


def run(name, repeats, kernels_only):
    P = _biased(workloads.get(name))
    rec = engine.Reconstruction(0)
    rec.set_flags(disable_bias_correction=False)
    engine.sync_gpu(rec, P)
    d = host.irtkReconstruction(rec, P.ns, max_intensity=P.max_intensity, min_intensity=P.min_intensity)
    d.SetSmoothingParameters(150, 0.02)
    d.set_bias_correction(True, 12.0)
    rec._lib.svr_get_stream.restype = C.c_void_p
    _STREAM[0] = C.c_void_p(rec._lib.svr_get_stream(rec._h))
    d.reconstruct_iteration(1)                        # a running reconstruction: EM weights, a field, the coefficient table
    res = {"workload": name, "slices": list(P.slices.shape), "volume": list(rec.vsize), "coeff_table": rec.get_option("coeff_table")}
    np_px, nv = int(np.prod(P.slices.shape)), int(np.prod(rec.vsize))
    # HBM bytes each kernel group must move at least (from the shapes): CorrectBias reads slices, bias, weights, simweights, simslices
    # and writes bias (6 x 4 B per slice pixel); the tail reads the field, the weights, maskC, recon and writes field, recon
    # (the three passes: 4 B in + 4 B out each, plus 3 x 4 B of the fused divisions / divexp)
    res["hbm_bytes_correct_bias"] = 6 * 4 * np_px
    res["hbm_bytes_normalise_tail"] = (3 * 2 + 4) * 4 * nv
    bias0 = rec.debug_get(engine.BUF_BIAS)
    field = rec.debug_get(engine.BUF_BIAS_VOLUME)
    recon = rec.debug_get(engine.BUF_RECONSTRUCTED)
    # bias_mode 0: round 1's kernels; 2: the new ones at every size (1, the default, takes the stencil tail below 4.2 M voxels)
    for mode in (2, 0):
        rec.set_option("bias_mode", mode)
        res[f"correct_bias_mode{mode}"] = _timed(lambda: rec.CorrectBias(12.0, False), repeats,
                                                 setup=lambda: rec.debug_set(engine.BUF_BIAS, bias0))
        res[f"normalise_tail_mode{mode}"] = _timed(lambda: rec._lib.svr_normalise_bias_finish(rec._h, C.c_float(12.0)), repeats,
                                                   setup=lambda: (rec.debug_set(engine.BUF_BIAS_VOLUME, field),
                                                                  rec.debug_set(engine.BUF_RECONSTRUCTED, recon)))
        res[f"normalise_scatter_mode{mode}"] = _timed(lambda: rec._lib.svr_normalise_bias_local(rec._h), repeats)
    rec.set_option("bias_mode", 1)
    rec.debug_set(engine.BUF_RECONSTRUCTED, recon)
    if not kernels_only:
        it = [1]

        def sr():
            d.sr_iteration(it[0])
            it[0] += 1
        d.set_bias_correction(True, 12.0)
        res["sr_iteration_bias_on"] = _timed(sr, repeats)
        d.set_bias_correction(False, 12.0)
        res["sr_iteration_bias_off"] = _timed(sr, repeats)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("workloads", nargs="*", default=["P4", "S8"])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args(argv)
    out = [run(w, a.repeats, a.kernels_only) for w in a.workloads]
    for r in out:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
