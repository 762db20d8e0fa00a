"""tests/golden/epnp_input_data_noise.npz and epnp_kat.json from the EPnP solver's own input file (data only):

    python tests/golden/make_epnp_fixture.py <reference>/matlab_code/aux_code/EPnP_matlab/data/input_data_noise.mat

The .mat holds 50 points (struct array `point`: Xworld, Xcam, Ximg_pix, Ximg_pix_true, ...), the 3 x 4 intrinsics A = [800 0 320 0; 0 800 240 0; 0 0 1 0]
and the true pose Rt (4 x 4).  The npz keeps Xworld (50, 3), Xcam (50, 3), Ximg_pix (50, 2), Ximg_pix_true (50, 2), A = A[:, :3] and Rt.  The json
records what tests/epnp_ref.py (LAPACK) answers on the noisy pixels; tests/test_epnp_ref.py holds the restatement to it to 1e-6 relative.
Needs scipy to read the .mat; the tests need only the two files written here.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def main(mat):
    from scipy.io import loadmat
    import epnp_ref as ref
    d = loadmat(mat)
    pt = d["point"][0]

    def col(name, k):
        return np.array([np.asarray(p[name], np.float64).ravel()[:k] for p in pt])

    out = dict(Xworld=col("Xworld", 3), Xcam=col("Xcam", 3), Ximg_pix=col("Ximg_pix", 2), Ximg_pix_true=col("Ximg_pix_true", 2),
               A=np.asarray(d["A"], np.float64)[:, :3], Rt=np.asarray(d["Rt"], np.float64))
    np.savez(os.path.join(HERE, "epnp_input_data_noise.npz"), **out)
    cam = [out["A"][0, 0], out["A"][0, 2], out["A"][1, 2], 0.0, 0.0, 480.0, 640.0]
    r = ref.epnp(out["Xworld"], out["Ximg_pix"], cam)
    kat = {"cam": cam, "noisy": {"err": [None if not np.isfinite(e) else float(e) for e in r["err"]], "best": r["best"], "sta": r["sta"]}}
    with open(os.path.join(HERE, "epnp_kat.json"), "w") as f:
        json.dump(kat, f, indent=1)
        f.write("\n")
    print(kat)


if __name__ == "__main__":
    main(sys.argv[1])
