"""The synthetic frame pairs of the pair suites (tests/test_vo_pair_ref.py on the CPU, tests/test_gpu_vo_pair.py on the device).

A pair is two mode-1 frames with a confidence map and a SIFT set each.  Keypoints sit on a 3-pixel lattice and the raw planes are constant over each
keypoint's 3 x 3 neighbourhood, so the filtered pixel is the planted point to a few ulp (the nine weights sum to 1 within 2 ulp).  cur's points are random
and farther than 0.4 m; prev's are R p + T for the matched keypoints, a share of them displaced (outliers).  Descriptors are unit-norm 128-vectors:
a matched prev keypoint carries its partner's descriptor plus noise of 1e-3 per entry (squared distance about 1e-4 against about 2 to any other one, so
siftmatch.c:122 accepts it at any sensible threshold), every other keypoint an unrelated one (best and second best both near 2: rejected).  Some
keypoints of either frame lie under a confidence of 0: gate 1 drops them, and kept positions differ from the caller's indices.

CASES names, per case, the kept counts (n1, n2) and the pnum it must land on; tests/test_vo_pair_ref.py checks every one through the restatement and the
oracle alone."""
import numpy as np

import sr_frame_ref as sr
from test_vo_oracle import rotm

THRESH = 1.5


def lattice(rows, cols):
    """0-based (row, column) centres of disjoint 3 x 3 blocks inside the image"""
    return [(3 * i + 1, 3 * j + 1) for i in range(rows // 3) for j in range(cols // 3)]


def unit(rng, n):
    d = rng.normal(0.0, 1.0, (128, n))
    return d / np.linalg.norm(d, axis=0)


def make_pair(rows, cols, n1, n2, pnum, seed, drop1=0, drop2=0, outliers=0.3, near=False, special=None):
    """dict(fr1, fr2, frm1, des1, frm2, des2, R, T, n1, n2, pnum): n1 / n2 keypoints survive gate 1 in prev / cur, drop1 / drop2 more are planted under
    zero confidence; the first `pnum` surviving prev keypoints (in a shuffled order) are matched to distinct surviving cur keypoints.
    special: 'shared' (5 -> 1 style: every matched prev keypoint takes the SAME cur keypoint), 'dup' (duplicated cur descriptors, see the tests)."""
    rng = np.random.default_rng(seed)
    R, T = rotm(rng.normal(0, 0.1, 3)), rng.normal(0, 0.05, 3)
    K1, K2 = n1 + drop1, n2 + drop2
    lat = lattice(rows, cols)
    assert max(K1, K2) <= len(lat), "the lattice of a %d x %d frame holds %d keypoints" % (rows, cols, len(lat))
    out = dict(R=R, T=T, n1=n1, n2=n2, pnum=pnum, rows=rows, cols=cols)
    frames = []
    for K in (K1, K2):
        fr = dict(z=rng.uniform(0.8, 4.0, (rows, cols)), x=rng.uniform(-1.5, 1.5, (rows, cols)), y=rng.uniform(-1.0, 1.0, (rows, cols)),
                  amp=np.floor(rng.uniform(100.0, 30000.0, (rows, cols))), conf=np.full((rows, cols), sr.CMAX))
        px = [lat[i] for i in rng.permutation(len(lat))[:K]]
        frames.append((fr, px))
    (fr1, px1), (fr2, px2) = frames
    # which keypoints gate 1 drops: conf 0 at the pixel (strictly below half of CMAX)
    dropped1 = set(rng.permutation(K1)[:drop1].tolist()); dropped2 = set(rng.permutation(K2)[:drop2].tolist())
    for fr, px, dr in ((fr1, px1, dropped1), (fr2, px2, dropped2)):
        for k in dr:
            fr["conf"][px[k]] = 0.0
    kept1 = [k for k in range(K1) if k not in dropped1]; kept2 = [k for k in range(K2) if k not in dropped2]
    # cur's points, planted over the 3 x 3 blocks: pset = [-x; -y; z]
    P2 = np.stack([rng.uniform(-1.5, 1.5, K2), rng.uniform(-1.0, 1.0, K2), rng.uniform(0.05, 0.2, K2) if near else rng.uniform(0.8, 4.0, K2)])
    if near:
        P2[:2] *= 0.05
    P1 = np.stack([rng.uniform(-1.5, 1.5, K1), rng.uniform(-1.0, 1.0, K1), rng.uniform(0.8, 4.0, K1)])
    des1, des2 = unit(rng, K1), unit(rng, K2)
    a = [kept1[i] for i in rng.permutation(n1)[:pnum]]                    # matched prev keypoints (caller's indices)
    if special == "shared":
        b = [kept2[0]] * pnum
    else:
        b = [kept2[i] for i in rng.permutation(n2)[:pnum]]
    n_out = int(outliers * pnum) if pnum >= 8 else 0
    for i, (k1, k2) in enumerate(zip(a, b)):
        P1[:, k1] = R @ P2[:, k2] + T
        if i < n_out:
            P1[:, k1] += rng.normal(0, 0.5, 3)
        d = des2[:, k2] + rng.normal(0.0, 1e-3, 128)
        des1[:, k1] = d / np.linalg.norm(d)
    if special == "dup":
        # cur keypoint j2 repeats j (j < j2): prev a[0] carries j's descriptor EXACTLY (distance 0 to both: accepted, first index kept);
        # cur keypoint m2 repeats m: prev a[1] is m's descriptor plus noise (best == second > 0: rejected)
        j, m = sorted(b[:2])
        free = [k for k in kept2 if k not in b and k > m]
        j2, m2 = free[0], free[1]
        des1[:, a[b.index(j)]] = des2[:, j]
        des2[:, j2] = des2[:, j]; des2[:, m2] = des2[:, m]
        out.update(dup=dict(exact_prev=a[b.index(j)], exact_cur=j, exact_copy=j2, noisy_prev=a[b.index(m)], noisy_cur=m, noisy_copy=m2))
    for fr, px, P in ((fr1, px1, P1), (fr2, px2, P2)):
        for k, (r, c) in enumerate(px):
            fr["x"][r - 1:r + 2, c - 1:c + 2] = -P[0, k]; fr["y"][r - 1:r + 2, c - 1:c + 2] = -P[1, k]; fr["z"][r - 1:r + 2, c - 1:c + 2] = P[2, k]
    frm = []
    for px in (px1, px2):
        f = np.zeros((4, len(px)), order="F")
        f[0] = [c + 1 for (r, c) in px]; f[1] = [r + 1 for (r, c) in px]
        f[:2] += rng.uniform(-0.3, 0.3, (2, len(px)))                     # off the pixel centre: round() brings them back
        f[2] = rng.uniform(1.0, 3.0, len(px)); f[3] = rng.uniform(-3.0, 3.0, len(px))
        frm.append(f)
    out.update(fr1={k: np.asfortranarray(v) for k, v in fr1.items()}, fr2={k: np.asfortranarray(v) for k, v in fr2.items()},
               frm1=frm[0], des1=np.asfortranarray(des1), frm2=frm[1], des2=np.asfortranarray(des2), kept1=np.array(kept1, np.int32),
               kept2=np.array(kept2, np.int32), planted=(a, b), P1=P1, P2=P2)
    return out


SMALL, FULL = (36, 45), (144, 176)
# name: (shape, n1, n2, pnum, extra keyword arguments).  pnum covers rst = 0 (below 4), 1, 5, 495, 700 and the 64-bit mask word boundary; (n1, n2) the
# edges of the 32 x 32 tile, several column tiles (n2 = 65: three, 280: nine) and more than one pass of nothing (n1 <= 1024: one pass of the pairs launch)
CASES = {
    "n1x1":        (SMALL, 1, 1, 1, dict(seed=1)),                                # one scan keypoint: second stays at the maximum, the test passes
    "n5x1_shared": (SMALL, 5, 1, 5, dict(seed=2, special="shared", drop1=2)),      # five prev keypoints on ONE cur keypoint: every draw shares it
    "p0":          (SMALL, 31, 33, 0, dict(seed=3, drop1=3, drop2=2)),             # every match rejected by the ratio test
    "p3":          (SMALL, 32, 32, 3, dict(seed=4, drop1=1, drop2=4)),
    "p4":          (SMALL, 33, 65, 4, dict(seed=5, drop1=2, drop2=3)),             # rst = 1: the one hypothesis is the only one
    "p5":          (SMALL, 33, 65, 5, dict(seed=6, drop2=5)),
    "p12":         (SMALL, 31, 33, 12, dict(seed=7, drop1=4)),                     # rst = 495
    "p13":         (SMALL, 32, 32, 13, dict(seed=8, drop1=2, drop2=2)),            # rst = 700
    "p12_dup":     (SMALL, 31, 33, 12, dict(seed=9, special="dup", drop1=3, drop2=3)),   # ... 11 after the noisy duplicate's rejection
    "p63":         (SMALL, 100, 90, 63, dict(seed=10, drop1=10, drop2=10)),
    "p64":         (SMALL, 100, 90, 64, dict(seed=11, drop1=10, drop2=10)),
    "p65":         (SMALL, 100, 90, 65, dict(seed=12, drop1=10, drop2=10)),
    "p129":        (FULL, 300, 280, 129, dict(seed=13, drop1=40, drop2=30)),       # the planted motion is checked here
}


def case(name):
    shape, n1, n2, pnum, kw = CASES[name]
    c = make_pair(shape[0], shape[1], n1, n2, pnum, **kw)
    c["name"] = name
    c["expect_pnum"] = pnum - 1 if kw.get("special") == "dup" else pnum
    return c


def restated_chain(c, orc, w):
    """the case through code that is not under test: the restatement's conditioning and gate 1, then the oracle's siftmatch and gather.
    dict(k1, k2 (the restatement's keypoint dicts), match (2, pnum), p1, p2)"""
    c1, c2 = sr.condition(c["fr1"], 1, w), sr.condition(c["fr2"], 1, w)
    k1, k2 = sr.keypoints(c1, c["frm1"], c["des1"], 1), sr.keypoints(c2, c["frm2"], c["des2"], 1)
    mt, _ = orc.siftmatch(np.asfortranarray(k1["descriptors"]), np.asfortranarray(k2["descriptors"]), THRESH)
    out = dict(c1=c1, c2=c2, k1=k1, k2=k2, match=mt)
    if mt.shape[1]:
        out["p1"] = orc.vo_gather(c1["x"], c1["y"], c1["z"], k1["frames"], mt[0])
        out["p2"] = orc.vo_gather(c2["x"], c2["y"], c2["z"], k2["frames"], mt[1])
    return out
