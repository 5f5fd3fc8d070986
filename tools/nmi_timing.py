"""One slice-to-volume pass of the IRTK schedule with CC and with NMI (--useNMI), every similarity on the GPU: P4s (280 slices) and
S8 (configs[3]: 512 slices of 256^2 against the 0.75 mm volume).  Reconstructs once per case, then registers from the true
transformations; prints wall time, evaluations and the schedule's own split (SVR_REG_TIMING=1 on stderr).
usage: nmi_timing.py [p4|s8 ...]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("SVR_REG_TIMING", "1")
import numpy as np  # noqa: E402

from fetalreconstruction_amd import engine, geometry as geo, host, phantom  # noqa: E402
from tests.twins.reconstruction import irtkReconstruction  # noqa: E402

for which in sys.argv[1:] or ["p4", "s8"]:
    P = phantom.problem_p4() if which == "p4" else phantom.problem_s8()
    rec = engine.Reconstruction(0)
    engine.sync_gpu(rec, P)
    d = irtkReconstruction(rec, P.ns, max_intensity=P.max_intensity, min_intensity=P.min_intensity)
    d.SetSmoothingParameters(150, 0.02)
    d.reconstruct_iteration(2)
    vol = rec.syncCPU().reshape(P.vsize[::-1])
    rattr = geo.ImageAttributes(*P.vsize, *P.vdim)
    T = P.slice_t.reshape(-1, 4, 4).astype(np.float64)
    for sim in ("cc", "nmi", "cc", "nmi"):                # the second pair is the measurement (first calls allocate)
        t0 = time.time()
        Tn, nev = host.SliceToVolumeRegistration(rec, P.slices, P.slice_attr, T, rattr, vol, similarity=sim)
        wall = time.time() - t0
        print(f"{which} {sim}: {P.ns} slices, wall {wall:.3f} s, {nev} similarity evaluations", flush=True)
