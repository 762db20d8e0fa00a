"""The synthetic frame pairs and maps of the frame-policy suites (tests/test_frame_policy_ref.py on the CPU, tests/test_gpu_frame_policy.py on the device;
DESIGN.md section 22).

A pair is tests/vo_pair_cases.py's: keypoints on a 3-pixel lattice, raw planes constant over each keypoint's 3 x 3 neighbourhood (the filtered pixel is the
planted point to a few ulp in either mode -- no lattice block touches the border), unit-norm 128-descriptors shared with 1e-3 noise between matched
keypoints, some keypoints under a confidence of 0 so that the depth gate drops them and kept positions differ from the caller's indices.  Here both
frames are loaded in mode 0 and go through gate 0, as SIFT_extract_save.m does for both scans.  The map, its book and the last frame's flags are
tests/test_gpu_map_policy.py's (_case with no candidates of its own).

CASES names, per case, the frame size, the kept counts (n1, n2), the pnum it must land on, the map size N, the spare capacity, min_features and what the
walk must end on with strict_reference 1 and 0 ('exhausted': the drawn order runs out below the goal; 'goal': the goal is met inside a chunk of 64
positions; 'capacity': the map is full).  tests/test_frame_policy_ref.py checks every one -- the pnum, the ending and the margins -- through the restatements alone, in both quirk modes and
for both precisions of P, so that no GPU case needs to be skipped."""
import numpy as np

import cand_order_ref as cr
import map_policy_ref as mp
import sr_frame_ref as sr
import vo_pair_cases as vp
from test_gpu_map_policy import _case, _margin_ok

THRESH = vp.THRESH
MODE = 0                                  # read_xyz_sr4000.m: sigma = 2, zero padding
SEED, SEQ = 20261018, 5
SMALL, FULL = (17, 70), (144, 176)
# name: (shape, n1, n2, pnum, N, spare capacity, min_features, ending, make_pair keywords)
E = ("exhausted", "exhausted")
CASES = {
    "n0x5":   (SMALL, 0, 5, 0, 21, 40, 50, E, dict(seed=101, drop1=3)),                  # prev keeps nothing: nothing is queued for the match
    "n5x0":   (SMALL, 5, 0, 0, 0, 40, 50, E, dict(seed=102, drop2=2)),                  # cur keeps nothing
    "n1x1":   (SMALL, 1, 1, 1, 0, 40, 50, E, dict(seed=103, drop1=1)),
    "n5x1":   (SMALL, 5, 1, 5, 21, 40, 50, E, dict(seed=104, special="shared", drop1=2)),   # one scan keypoint: every prev keypoint passes the test
    "p0":     (SMALL, 33, 65, 0, 65, 40, 50, E, dict(seed=105, drop1=3, drop2=2)),       # every match rejected: K = 0 behind a real launch
    "p1":     (SMALL, 33, 65, 1, 21, 40, 50, E, dict(seed=106, drop2=5)),
    "p63":    (SMALL, 64, 64, 63, 21, 40, 50, ("goal", "exhausted"), dict(seed=107, drop1=5, drop2=4)),
    "p64":    (SMALL, 64, 64, 64, 0, 40, 50, ("goal", "exhausted"), dict(seed=108, drop1=2, drop2=6)),
    "p20":    (SMALL, 65, 31, 20, 65, 40, 50, E, dict(seed=109, drop1=4, drop2=3)),
    "p65":    (FULL, 300, 280, 65, 21, 2, 50, ("capacity", "capacity"), dict(seed=110, drop1=40, drop2=30)),
    "p129":   (FULL, 300, 280, 129, 65, 40, 40, ("goal", "exhausted"), dict(seed=111, drop1=25, drop2=35)),
    "p129_0": (FULL, 300, 280, 129, 0, 40, 30, ("goal", "goal"), dict(seed=112, drop1=30, drop2=20)),
}
GATE_CUR = {"p1": 1}                      # cur may come through either gate: one case takes gate 1 (the same keypoints survive: the drops sit at confidence 0)


def case(name):
    shape, n1, n2, pnum, N, spare, mf, ending, kw = CASES[name]
    c = vp.make_pair(shape[0], shape[1], n1, n2, pnum, **kw)
    x, P, cam, step, book, meas, li, hi, _, _, _ = _case(N, 0, 7 + N + kw["seed"], N + spare)
    c.update(name=name, expect_pnum=pnum, N=N, cap=N + spare, min_features=mf, ending=ending, gate_cur=GATE_CUR.get(name, 0),
             x=x, P=P, cam=cam, step=step, book=book, meas=meas, li=li, hi=hi)
    return c


def gather(k1, mt):
    """initialize_features.m:97-99 vectorised: (uv (K, 2), xyz (K, 3), desc (128, K)) of the previous scan's kept keypoints match[0] names"""
    idx = mt[0].astype(np.int64) - 1
    return np.ascontiguousarray(k1["frames"][:2, idx].T), np.ascontiguousarray(k1["xyz"][:, idx].T), np.asfortranarray(k1["descriptors"][:, idx])


def literal_candidates(SCAN_SIFT_pre, DataCurrent_Descriptor, orc):
    """SIFT_match_save.m:33 and initialize_features.m:95-99 line by line, indices 1-based as written"""
    matches, _ = orc.siftmatch(np.asfortranarray(SCAN_SIFT_pre["Descriptor"]), np.asfortranarray(DataCurrent_Descriptor), THRESH)      # siftmatch(DataPre.Descriptor, DataCurrent.Descriptor)
    UV, XYZ, DESCRIPTOR = [], [], []
    for col in range(matches.shape[1]):
        m1 = int(matches[0, col])                                                  # matches(1, :)
        UV.append([SCAN_SIFT_pre["SCALE_ORIENT_POS"][0, m1 - 1], SCAN_SIFT_pre["SCALE_ORIENT_POS"][1, m1 - 1]])      # SCALE_ORIENT_POS(1:2, matches(1,:))'
        XYZ.append([SCAN_SIFT_pre["XYZ_DATA"][r, m1 - 1] for r in range(3)])        # XYZ_DATA(:, matches(1,:))
        DESCRIPTOR.append([SCAN_SIFT_pre["Descriptor"][r, m1 - 1] for r in range(128)])
    return matches, np.array(UV).reshape(-1, 2), np.array(XYZ).reshape(-1, 3).T, np.array(DESCRIPTOR).reshape(-1, 128).T


def restated_keypoints(c, w):
    """both scans through restatement (a): conditioning in MODE, gate 0 on prev, the case's gate on cur"""
    c1, c2 = sr.condition(c["fr1"], MODE, w), sr.condition(c["fr2"], MODE, w)
    return sr.keypoints(c1, c["frm1"], c["des1"], 0), sr.keypoints(c2, c["frm2"], c["des2"], c["gate_cur"])


def landmark_flags(c):
    N = c["N"]
    ic, li, hi = np.zeros(N, int), np.zeros(N, int), np.zeros(N, int)
    ic[c["meas"]] = 1; li[c["meas"]] = c["li"]; hi[c["meas"]] = c["hi"]
    return ic, li, hi


def restated_policy(c, uv, xyz, predicted, strict, dtype, seed=SEED, seq=SEQ):
    """cand_order_ref -> map_policy_ref on gathered candidates: dict(order, ref (map_policy_ref.policy on the permuted arrays), accepted (candidate
    indices), margin_ok)"""
    o = cr.order(uv, seed, seq) if len(uv) else np.zeros(0, np.int32)
    if len(uv) > 1:
        assert cr.min_relative_gap(cr.keys(uv, seed, seq)) >= 1e-9
    Pd = c["P"].astype(np.float32).astype(np.float64) if dtype == "f32" else c["P"]
    ic, li, hi = landmark_flags(c)
    ref = mp.policy(c["step"], np.zeros(c["N"], np.int32), c["x"], Pd, c["cam"], c["book"], ic, li, hi, predicted, uv[o], xyz[o],
                    min_features=c["min_features"], threshold=0.1, strict=strict, cap=c["cap"])
    return dict(order=o, ref=ref, accepted=o[ref["accepted"]] if len(o) else np.zeros(0, np.int32), margin_ok=_margin_ok(ref, uv[o], c["cam"]))


def check_ending(c, ref, K, strict):
    """the walk ended the way the case names for this quirk mode"""
    n_acc, n_surv = len(ref["accepted"]), c["N"] - len(ref["deleted"])
    goal = (ref["T"] + 1) // 2 if strict else ref["T"]              # quirk Q13
    ending = c["ending"][0 if strict else 1]
    if ending == "exhausted":
        assert ref["examined"] == K and n_acc < goal and n_surv + n_acc < c["cap"]
    elif ending == "capacity":
        assert n_surv + n_acc == c["cap"] and ref["examined"] < K and n_acc < goal
    else:
        assert ending == "goal" and n_acc == goal > 0 and ref["examined"] < K and ref["examined"] % 64 != 0 and n_surv + n_acc < c["cap"]
