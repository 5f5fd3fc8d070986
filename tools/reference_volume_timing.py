"""Time what --referenceVolume adds to a run on a bench workload: the whole of svr_resample_to_reconstruction (three allocations, the
upload of the source, k_seed_resample, k_seed_finish, the copy of the volume and of five doubles, one wait, three frees) on the
workload's reconstruction grid from a source of the same size on an oblique, shifted grid, and one SR iteration of the same run for scale.
The call is blocking: host clock around it; warm-up first, then median and spread (min .. max) over repeats.
usage: python tools/reference_volume_timing.py [P4 S8 ...] [--repeats 9] [--out file.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from fetalreconstruction_amd import engine, geometry as geo, host, workloads  # noqa: E402


def _timed(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return {"median_ms": float(np.median(t)), "min_ms": float(np.min(t)), "max_ms": float(np.max(t)), "repeats": repeats}


def run(name, repeats):
    P = workloads.get(name)
    rec = engine.Reconstruction(0)
    engine.sync_gpu(rec, P)
    d = host.irtkReconstruction(rec, P.ns, max_intensity=P.max_intensity, min_intensity=P.min_intensity)
    d.SetSmoothingParameters(150, 0.02)
    d.reconstruct_iteration(1)                        # a running reconstruction: its volume is the seed
    vx, vy, vz = rec.vsize
    src = rec.syncCPU().reshape(vz, vy, vx).copy()
    # the same number of voxels, turned by a few degrees about every axis and shifted by a fraction of a voxel: every read is a gather
    m = geo.rigid_matrix(0.3, -0.4, 0.2, 2.0, -3.0, 4.0)
    c = np.array([(vx - 1) / 2.0, (vy - 1) / 2.0, (vz - 1) / 2.0])
    m[:3, 3] += c - m[:3, :3] @ c
    res = {"workload": name, "volume": list(rec.vsize), "source": [vx, vy, vz], "bytes_moved_host": 8 * src.size}
    res["resample_call"] = _timed(lambda: rec.resample_to_reconstruction(src, m, -1.0), repeats)
    res["resample_call_install_scale_no_download"] = _timed(lambda: rec.resample_to_reconstruction(src, m, -1.0, install=True, scale=1.0, want_volume=False), repeats)
    it = [1]

    def sr():
        d.sr_iteration(it[0])
        rec.stream_sync()                             # (the host object does not wait inside an SR iteration)
        it[0] += 1
    res["sr_iteration"] = _timed(sr, repeats)
    rec.close()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("workloads", nargs="*", default=["P4", "S8"])
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out")
    a = ap.parse_args(argv)
    out = [run(w, a.repeats) for w in a.workloads]
    for r in out:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
