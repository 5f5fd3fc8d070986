"""Time the quality report's device work on a bench workload: svr_slice_quality (the whole call: two allocations, two kernels, the copy
of ns x 10 doubles, one wait), the forward projection --sliceReport runs before it, and one SR iteration of the same run for scale.
Times are HIP events on the engine's stream around the call; warm-up first, then median and spread (min .. max) over repeats.  The
kernel reads four floats per slice-grid pixel (five with a bias field): `hbm_bytes` over the kernel's own time is its share of the
HBM peak -- the kernel's time comes from a trace,
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/slice_quality_timing.py P4 --quality-only
usage: python tools/slice_quality_timing.py [P4 S8 ...] [--repeats 9] [--bias] [--out file.json]"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from fetalreconstruction_amd import engine, host, workloads  # noqa: E402

_hip = C.CDLL("libamdhip64.so")


def _timed(stream, fn, repeats, warmup=2):
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert _hip.hipEventCreate(C.byref(ev0)) == 0 and _hip.hipEventCreate(C.byref(ev1)) == 0
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(repeats):
        assert _hip.hipDeviceSynchronize() == 0
        assert _hip.hipEventRecord(ev0, stream) == 0
        fn()
        assert _hip.hipEventRecord(ev1, stream) == 0
        assert _hip.hipEventSynchronize(ev1) == 0
        ms = C.c_float()
        assert _hip.hipEventElapsedTime(C.byref(ms), ev0, ev1) == 0
        t.append(ms.value)
    _hip.hipEventDestroy(ev0)
    _hip.hipEventDestroy(ev1)
    return {"median_ms": float(np.median(t)), "min_ms": float(np.min(t)), "max_ms": float(np.max(t)), "repeats": repeats}


def run(name, repeats, bias, quality_only):
    P = workloads.get(name)
    rec = engine.Reconstruction(0)
    if bias:
        rec.set_flags(disable_bias_correction=False)
    engine.sync_gpu(rec, P)
    d = host.irtkReconstruction(rec, P.ns, max_intensity=P.max_intensity, min_intensity=P.min_intensity)
    d.SetSmoothingParameters(150, 0.02)
    if bias:
        d.set_bias_correction(True, 12.0)
    rec._lib.svr_get_stream.restype = C.c_void_p
    stream = C.c_void_p(rec._lib.svr_get_stream(rec._h))
    d.reconstruct_iteration(1)                        # a running reconstruction: EM weights, scales, the coefficient table
    px = int(np.prod(P.slices.shape))
    res = {"workload": name, "slices": list(P.slices.shape), "volume": list(rec.vsize), "bias": bool(bias),
           "hbm_bytes": (5 if bias else 4) * 4 * px}
    rec.SimulateSlices()
    res["slice_quality_call"] = _timed(stream, rec.slice_quality, repeats)
    res["quality_chunks"] = rec.get_option("quality_chunks")
    if not quality_only:
        res["forward_projection"] = _timed(stream, rec.SimulateSlices, repeats)
        it = [1]

        def sr():
            d.sr_iteration(it[0])
            it[0] += 1
        res["sr_iteration"] = _timed(stream, sr, repeats)
    rec.close()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("workloads", nargs="*", default=["P4", "S8"])
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--bias", action="store_true")
    ap.add_argument("--quality-only", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args(argv)
    out = [run(w, a.repeats, a.bias, a.quality_only) for w in a.workloads]
    for r in out:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
