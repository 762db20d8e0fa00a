"""CPU restatement of map_management.m:27-79 with its policy (the truth of pre3_map_policy).

    decide()        steps 1-5 on given inputs: the book, last frame's flags, what was predicted, the survivors' h at x_k_k,
                    the candidates and the h each one would have once added
    policy()        the same from a filter state: conversion flags and points (np_twin.map_convert's arithmetic), projection at x_k_k
                    (np_twin.project), the new features' h (hinv_my_version.m's geometry, np_twin.undistort)
    literal()       a list-of-structs transliteration of the .m loops (delete_features.m:31-49, update_features_info.m:30-44,
                    initialize_features.m:110-142 -> initialize_a_feature_sift_3.m:72-138), the double count of quirk Q13 included

Book rows are [times_predicted, times_measured, init_frame, last_visible].
"""
import numpy as np

from oracle import np_twin as tw

SEMI_U, SEMI_V = 15.0, 10.0          # initialize_a_feature_sift_3.m:58-60: [60,40]/2 halved
INVDEPTH, CARTESIAN = 0, 1


def in_box(pu, pv, cu, cv, strict):
    """initialize_a_feature_sift_3.m:92-98; strict: the centre is (UV(c,2), UV(c,1)) (quirk Q14)."""
    bu, bv = (cv, cu) if strict else (cu, cv)
    return pu > bu - SEMI_U and pu < bu + SEMI_U and pv > bv - SEMI_V and pv < bv + SEMI_V


def target(measured, min_features):
    return min_features if measured == 0 else max(0, min_features - measured)     # map_management.m:58-66


def decide(step, book, ic, li, hi, predicted, h_surv, vis_surv, cand_uv, new_h, min_features=50, strict=True, cap=None):
    """book (N, 4); ic / li / hi / predicted (N,) last frame's flags and ~isempty(h); h_surv (N, 2) / vis_surv (N,) every landmark's projection
    at x_k_k after the conversion (only survivors are read); cand_uv (K, 2); new_h(c) -> (u, v) or None for candidate c once added.
    Returns dict(deleted, accepted, measured, T, examined, book)."""
    book = np.array(book, np.int64).reshape(-1, 4).copy()
    N = book.shape[0]
    book[:, 3] = np.where(np.asarray(ic)[:N] != 0, step - 1, book[:, 3])          # matching_sift_based.m:133 for last frame's IC
    tp, tm, init, lv = book.T
    dele = ((tm < 0.5 * tp) & (tp > 5)) | (step - init > 20) | ((N > 20) & (step - lv > 20))
    surv = np.nonzero(~dele)[0]
    meas = (np.asarray(li)[:N] != 0) | (np.asarray(hi)[:N] != 0)
    measured = int(meas[surv].sum())
    nb = book[surv].copy()
    nb[:, 0] += np.asarray(predicted)[:N][surv] != 0
    nb[:, 1] += meas[surv]
    T = target(measured, min_features)
    goal = (T + 1) // 2 if strict else T
    if cap is not None:
        goal = min(goal, cap - len(surv))
    hs = [tuple(h_surv[i]) for i in surv if vis_surv[i]]
    acc, examined = [], 0
    for c in range(len(cand_uv)):
        if len(acc) >= goal:
            break
        examined = c + 1
        cu, cv = cand_uv[c]
        if any(in_box(pu, pv, cu, cv, strict) for pu, pv in hs):
            continue
        acc.append(c)
        h = new_h(c)
        if h is not None:
            hs.append(tuple(h))
    nb = np.vstack([nb, np.tile([0, 0, step - 1, step - 1], (len(acc), 1))]) if acc else nb
    return dict(deleted=np.nonzero(dele)[0], accepted=np.array(acc, int), measured=measured, T=T, examined=examined,
                book=nb.astype(np.int32))


def new_feature_y(uvd, rho, x, cam):
    """hinv_my_version.m:26-53: the inverse-depth landmark a candidate becomes."""
    f, Cx, Cy = cam[0], cam[1], cam[2]
    uv = tw.undistort(np.asarray(uvd, float), cam)
    nw = tw.q2r(x[3:7]) @ np.array([-(Cx - uv[0]) / f, -(Cy - uv[1]) / f, 1.0])
    return np.array([x[0], x[1], x[2], np.arctan2(nw[0], nw[2]), np.arctan2(-nw[1], np.hypot(nw[0], nw[2])), rho])


def convert(types, off, x, P, threshold):
    """inversedepth_2_cartesian.m:38-57 (the arithmetic of np_twin.map_convert) without the covariance: a landmark's linearity index reads
    only its own block, which the earlier conversions leave as it is.  -> (x with the converted points, types, flags)"""
    N = len(types)
    conv = np.zeros(N, np.int32)
    tc = np.array(types, np.int32).copy()
    parts = [x[:13]]
    for i in range(N):
        o = off[i]
        if types[i] != INVDEPTH:
            parts.append(x[o:o + 3])
            continue
        y = x[o:o + 6]
        if threshold is not None and threshold >= 0:
            rho, theta, phi = y[5], y[3], y[4]
            std_d = np.sqrt(P[o + 5, o + 5]) / rho ** 2
            p = y[0:3] + tw.m_dir(theta, phi) / rho
            a, c2 = p - y[0:3], p - x[0:3]
            li = 4 * std_d * (a @ c2) / (np.linalg.norm(a) * np.linalg.norm(c2)) / np.linalg.norm(c2)
            if li < threshold:
                conv[i], tc[i] = 1, CARTESIAN
                parts.append(p)
                continue
        parts.append(y)
    return np.concatenate(parts), tc, conv


def offsets(types):
    off, o = [], 13
    for t in types:
        off.append(o)
        o += 6 if t == INVDEPTH else 3
    return np.array(off, int), o


def policy(step, types, x, P, cam, book, ic, li, hi, predicted, cand_uv, cand_xyz, min_features=50, threshold=0.1, strict=True, cap=None):
    """decide() on a filter state (x_k_k, p_k_k).  Returns decide()'s dict plus converted (per landmark before the call), rho (K,) and the
    survivors' types after the conversion."""
    types = np.asarray(types, np.int32)
    cand_uv = np.asarray(cand_uv, float).reshape(-1, 2)
    cand_xyz = np.asarray(cand_xyz, float).reshape(-1, 3)
    rho = np.array([1.0 / np.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]) for p in cand_xyz])      # initialize_a_feature_sift_3.m:116-117
    N = len(types)
    # the deletion does not move the other landmarks: convert on the whole map, project every landmark, read the survivors
    off, _ = offsets(types)
    xc, tc, conv = convert(types, off, x, P, threshold)
    offc, _ = offsets(tc)
    h, has = tw.project(tc, offc, xc, cam) if N else (np.zeros((0, 2)), np.zeros(0, np.int32))
    r_wc = tw.q2r(x[3:7])

    def new_h(c):
        return tw.hi_landmark(INVDEPTH, new_feature_y(cand_uv[c], rho[c], x, cam), x[0:3], r_wc, cam)

    out = decide(step, book, ic, li, hi, predicted, h, has, cand_uv, new_h, min_features, strict, cap)
    conv = np.array(conv, np.int32)
    conv[out["deleted"]] = 0
    # every pixel the decisions read, before the field-of-view and image-bound tests (tests check their distance to every edge they meet)
    raw = [raw_uv(tc[i], xc[offc[i]:offc[i] + (6 if tc[i] == INVDEPTH else 3)], xc, cam)[0] for i in range(N)]
    raw += [raw_uv(INVDEPTH, new_feature_y(cand_uv[c], rho[c], x, cam), x, cam)[0] for c in out["accepted"]]
    out.update(converted=conv, rho=rho, types=np.array([tc[i] for i in range(N) if i not in set(out["deleted"].tolist())], np.int32),
               h=h, has_h=has, acc_h=[new_h(c) for c in out["accepted"]], raw_uv=np.array(raw).reshape(-1, 2))
    return out


def literal(step, info, cand_uv, new_h, min_features=50, strict=True):
    """The .m loops on a list of dicts (times_predicted, times_measured, init_frame, last_visible, individually_compatible,
    low_innovation_inlier, high_innovation_inlier, h (None or (u, v) of the last frame), h_kk (None or (u, v) at x_k_k)).
    Returns (deletion_list 0-based, accepted candidate indices, measured, T, the resulting list)."""
    info = [dict(a) for a in info]
    for a in info:                                              # matching_sift_based.m:133, in the frame before
        if a["individually_compatible"]:
            a["last_visible"] = step - 1
    deletion_list = []                                          # delete_features.m:31-49
    for i in range(len(info)):
        a = info[i]
        if a["times_measured"] < 0.5 * a["times_predicted"] and a["times_predicted"] > 5:
            deletion_list.append(i)
            continue
        if step - a["init_frame"] > 20:
            deletion_list.append(i)
            continue
        if len(info) > 20:
            if step - a["last_visible"] > 20:
                deletion_list.append(i)
    for i in reversed(deletion_list):
        info = info[:i] + info[i + 1:]
    measured = 0                                                # map_management.m:37-40
    for a in info:
        if a["low_innovation_inlier"] or a["high_innovation_inlier"]:
            measured += 1
    for a in info:                                              # update_features_info.m:30-44
        if a["h"] is not None:
            a["times_predicted"] += 1
        if a["low_innovation_inlier"] or a["high_innovation_inlier"]:
            a["times_measured"] += 1
        a["individually_compatible"] = a["low_innovation_inlier"] = a["high_innovation_inlier"] = 0
        a["h"] = None
    if measured == 0:                                           # map_management.m:58-66
        T = min_features
    else:
        T = min_features - measured
        if T < 0:
            T = 0
    initialized, idx, accepted = 0, 0, []                       # initialize_features.m:110-142
    while initialized < T:
        if idx >= len(cand_uv):                                 # flag_no_more_features
            break
        uv_pred = [a["h_kk"] for a in info if a["h_kk"] is not None]
        center = (cand_uv[idx][1], cand_uv[idx][0]) if strict else (cand_uv[idx][0], cand_uv[idx][1])
        there = any(p[0] > center[0] - SEMI_U and p[0] < center[0] + SEMI_U and p[1] > center[1] - SEMI_V and p[1] < center[1] + SEMI_V
                    for p in uv_pred)
        uv = None if there else cand_uv[idx]
        if uv is not None:
            info.append(dict(times_predicted=0, times_measured=0, init_frame=step - 1, last_visible=step - 1, individually_compatible=0,
                             low_innovation_inlier=0, high_innovation_inlier=0, h=None, h_kk=new_h(idx)))
            accepted.append(idx)
            if strict:
                initialized += 1                                # :127-129
        idx += 1
        if uv is not None:
            initialized += 1                                    # :138-140
    return deletion_list, accepted, measured, T, info


def features_info_book(features_info):
    return np.array([[int(np.asarray(a[k]).reshape(-1)[0]) if np.size(a[k]) else 0
                      for k in ("times_predicted", "times_measured", "init_frame", "last_visible")] for a in features_info], np.int32).reshape(-1, 4)


def raw_uv(t, y, x, cam):
    """hi_landmark's distorted pixel without the field-of-view and image-bound tests (np_twin.hi_landmark's arithmetic)."""
    r_wc = tw.q2r(x[3:7])
    hrl = r_wc.T @ ((y[0:3] - x[0:3]) * y[5] + tw.m_dir(y[3], y[4])) if t == INVDEPTH else np.linalg.inv(r_wc) @ (y[0:3] - x[0:3])
    uv_u = np.array([[cam[1] + (hrl[0] / hrl[2]) * cam[0]], [cam[2] + (hrl[1] / hrl[2]) * cam[0]]])
    return tw.distort(uv_u, cam)[:, 0], hrl


def point_entering_view(x1, x2, cam, depth=2.0, margin=0.05):
    """A Cartesian point that is outside the image at pose x1 and inside it at pose x2, both by at least `margin` px (None if the two poses
    do not differ enough): the landmark a rescue at x2 sees and the projection at x1 does not."""
    W, H = cam[6], cam[5]
    R2 = tw.q2r(x2[3:7])
    for a in np.linspace(0.2, 30, 150):
        for (ud, vd) in [(W - a, H / 2), (a, H / 2), (W / 2, H - a), (W / 2, a), (W - a, H / 4), (a, 3 * H / 4), (W / 4, H - a), (3 * W / 4, a)]:
            uv = tw.undistort(np.array([ud, vd]), cam)
            p = x2[0:3] + R2 @ np.array([(uv[0] - cam[1]) / cam[0], (uv[1] - cam[2]) / cam[0], 1.0]) * depth
            u1, _ = raw_uv(CARTESIAN, p, x1, cam)
            u2, _ = raw_uv(CARTESIAN, p, x2, cam)
            inside2 = min(u2[0], W - u2[0], u2[1], H - u2[1])
            outside1 = max(-u1[0], u1[0] - W, -u1[1], u1[1] - H)
            if inside2 > margin and outside1 > margin and tw.hi_landmark(CARTESIAN, p, x1[0:3], tw.q2r(x1[3:7]), cam) is None \
                    and tw.hi_landmark(CARTESIAN, p, x2[0:3], R2, cam) is not None:
                return p
    return None
