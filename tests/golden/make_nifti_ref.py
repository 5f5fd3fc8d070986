"""Regenerates tests/golden/nifti_ref.npz: what the reference's own NIfTI-1 library (oracle/_ref/libnifti_ref.so, built by
`make -C oracle` where the reference's sources lie) makes of the cases of tests/test_nifti.py, so that those tests pin the
engine's reader and writer on a checkout without that library:

  parse_<ext>_<left_handed>_*  the file the engine writes (after gzip) and the reference's parse of it (nifti_image_read)
  quat_<seed>_q / _mat         nifti_mat44_to_quatern and back of the image-to-world matrix
  write_<case>                 the file the reference writes (nifti_image_write), as written

Needs the engine library (build()) as well.  Run from the repo root:  python tests/golden/make_nifti_ref.py
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from fetalreconstruction_amd import nifti  # noqa: E402
from tests import test_nifti as tn  # noqa: E402


def main():
    ref = tn._ref()
    if ref is None:
        raise SystemExit(f"{tn.REF_LIB} not built (`make -C oracle` where the reference's sources are present)")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for ext in (".nii", ".nii.gz"):
            for lh in (False, True):
                a, d = tn._parse_case(lh)
                p = os.path.join(tmp, "w" + ext)
                nifti.write(p, d, a)
                r = tn._ref_read(ref, p)
                key = tn._parse_key(ext, lh)
                out[key + "_file"] = np.frombuffer(tn._file_body(p, ext), np.uint8)
                out[key + "_dims"] = np.array(r["dims"], np.int32)
                out[key + "_pix"] = np.array(r["pix"], np.float32)
                out[key + "_codes"] = np.array([r["qform"], r["sform"], r["datatype"]], np.int32)
                out[key + "_qto"] = r["qto"].astype(np.float32)
                out[key + "_sto"] = r["sto"].astype(np.float32)
                out[key + "_scl"] = np.array(r["scl"], np.float32)
                out[key + "_data"] = r["data"].view(np.uint8).copy()
        for seed, a in tn._quat_cases():
            out[f"quat_{seed}_q"], out[f"quat_{seed}_mat"] = tn._ref_quatern(ref, a)
        for case in tn.WRITE_CASES:
            raw, dt, name, nt, kw, _, _ = tn._write_case(case)
            p = os.path.join(tmp, case + "_" + name)
            tn._ref_write(ref, p, raw, (1.2, 0.9, 2.5), dt, nt=nt, **kw)
            out[f"write_{case}"] = np.frombuffer(open(p, "rb").read(), np.uint8)
    path = os.path.join(ROOT, "tests", "golden", "nifti_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, sum(v.nbytes for v in out.values()), "bytes")


if __name__ == "__main__":
    main()
