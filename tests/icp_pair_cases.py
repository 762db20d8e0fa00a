"""A frame pair on which both the VO pair and the dense ICP behind it find the planted pose (tests/test_gpu_predict_icp_pair.py, tools/time_icp_cov.py;
DESIGN.md section 34): tests/icp_frame_cases.py's surface seen from two poses, with matched keypoints planted as tests/vo_pair_cases.py plants them."""
import numpy as np

import icp_ref as R
import sr_frame_ref as sr
import vo_pair_cases as vp


def planted_pair(rows=36, cols=45, K=28, seed=77):
    """dict(rows, cols, fr1, fr2, frm1, des1, frm2, des2, expect_pnum, R_true, T_true).  The raw planes are constant over each keypoint's 3 x 3 block;
    cur's keypoint carries its own surface point, prev's the same point moved by the true pose, so every one of the K matches is an inlier."""
    rng = np.random.default_rng(seed)
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    R_true, T_true = R.rotvec(rng.normal(0, 0.03, 3)), rng.normal(0, 0.02, 3)
    frames = []
    for shift, moved in ((0.0, False), (0.5, True)):
        X, Y = (c + shift - cols / 2) / (cols / 2), 0.8 * (r + shift - rows / 2) / (rows / 2)
        Z = 2.0 + 0.25 * np.sin(2.1 * X + 0.3) * np.cos(1.7 * Y) + 0.15 * X * Y + 0.1 * np.cos(3.3 * X - 1.1 * Y)
        P = np.stack([X.ravel(), Y.ravel(), Z.ravel()])
        if moved:
            P = R_true.T @ (P - T_true[:, None])
        frames.append(dict(x=-P[0].reshape(rows, cols), y=-P[1].reshape(rows, cols), z=P[2].reshape(rows, cols),
                           amp=np.floor(rng.uniform(100.0, 30000.0, (rows, cols))), conf=np.full((rows, cols), sr.CMAX)))
    fr1, fr2 = frames
    lat = vp.lattice(rows, cols)
    px1 = [lat[i] for i in rng.permutation(len(lat))[:K]]
    px2 = [lat[i] for i in rng.permutation(len(lat))[:K]]
    des2 = vp.unit(rng, K)
    des1 = des2 + rng.normal(0.0, 1e-3, (128, K))
    des1 /= np.linalg.norm(des1, axis=0)
    for (r1, c1), (r2, c2) in zip(px1, px2):
        P2 = np.array([-fr2["x"][r2, c2], -fr2["y"][r2, c2], fr2["z"][r2, c2]])
        P1 = R_true @ P2 + T_true
        for fr, (rr, cc), Pt in ((fr1, (r1, c1), P1), (fr2, (r2, c2), P2)):
            fr["x"][rr - 1:rr + 2, cc - 1:cc + 2] = -Pt[0]; fr["y"][rr - 1:rr + 2, cc - 1:cc + 2] = -Pt[1]; fr["z"][rr - 1:rr + 2, cc - 1:cc + 2] = Pt[2]
    frm = []
    for px in (px1, px2):
        f = np.zeros((4, K), order="F")
        f[0] = [cc + 1 for (rr, cc) in px]; f[1] = [rr + 1 for (rr, cc) in px]
        f[2] = 2.0
        frm.append(f)
    return dict(rows=rows, cols=cols, fr1={k: np.asfortranarray(v) for k, v in fr1.items()}, fr2={k: np.asfortranarray(v) for k, v in fr2.items()},
                frm1=frm[0], des1=np.asfortranarray(des1), frm2=frm[1], des2=np.asfortranarray(des2), expect_pnum=K, R_true=R_true, T_true=T_true)
