"""Checkpoint files of the reference: `snapshot%d.mat`, one struct `snapshot%d` = {features_info, filter, step}.

    mono_slam.m:251-262   writer:  snapshotK.features_info / .filter / .step, save([DATA_FOLDER 'DataSnapshots/snapshotK'])
    mono_slam.m:266-270   reader
    @ekf_filter/ekf_filter.m:27-52                       the 20 fields of the filter object
    add_feature_to_info_vector_my_version_sift.m         the 24 fields of a features_info entry

Host-side IO through scipy.io (MATLAB v5 MAT-files).  `filter` is an old-style MATLAB object in the reference; MAT readers
outside MATLAB see it as a struct with the same fields, and that is also what `save_snapshot` writes -- in MATLAB,
`ekf_filter(s.x_k_k, s.p_k_k, s.std_a, s.std_alpha, s.std_z, s.type)` (ekf_filter.m:61-86) turns it back into an object.
The numerical work never happens here: `filter_from_snapshot` uploads the state to the device-resident EkfFilter.
"""
import re

import numpy as np
import scipy.io as sio
import scipy.sparse as sp

from . import _lib

FILTER_FIELDS = ("type", "x_k_k", "p_k_k", "std_a", "std_alpha", "std_z", "x_k_km1", "p_k_km1", "predicted_measurements",
                 "H_predicted", "R_predicted", "S_predicted", "S_matching", "z", "h", "H_matching", "measurements", "R_matching",
                 "x_k_k_mixing_estimate", "p_k_k_mixing_covariance")
FEATURE_FIELDS = ("r_wc_when_initialized", "R_wc_when_initialized", "uv_when_initialized", "half_patch_size_when_initialized",
                  "half_patch_size_when_matching", "times_predicted", "times_measured", "init_frame", "init_measurement", "type",
                  "yi", "individually_compatible", "low_innovation_inlier", "high_innovation_inlier", "z", "h", "H", "S",
                  "state_size", "measurement_size", "R", "Feature3d_in_code_coordinate", "Descriptor", "last_visible")
_COLUMN = ("x_k_k", "x_k_km1", "yi", "z", "Descriptor", "uv_when_initialized", "init_measurement", "r_wc_when_initialized")
_ROW = ("h", "Feature3d_in_code_coordinate")


def snapshot_path(data_folder, step):
    """mono_slam.m:256-262."""
    return "%sDataSnapshots/snapshot%d.mat" % (data_folder, step)


def _plain(v):
    if sp.issparse(v):
        return v
    if isinstance(v, np.ndarray) and v.dtype.kind in "US" and v.ndim == 0:
        return str(v)
    return v


def _struct_to_dict(s, fields):
    return {k: _plain(getattr(s, k)) for k in fields if hasattr(s, k)}


def load_snapshot(path, step=None):
    """-> dict(step, features_info=[dict, ...], filter=dict).  Values keep MATLAB's meaning: empty arrays stay empty
    (a landmark without z has z.size == 0), H is a scipy sparse matrix as MATLAB stores it (2 x n)."""
    m = sio.loadmat(path, squeeze_me=True, struct_as_record=False)
    names = [k for k in m if re.fullmatch(r"snapshot\d+", k)]
    if step is not None:
        names = [k for k in names if k == "snapshot%d" % step]
    if not names:
        raise KeyError("%s holds no snapshot%s struct" % (path, "" if step is None else str(step)))
    s = m[sorted(names, key=lambda k: int(k[8:]))[0]]
    fi = np.atleast_1d(s.features_info) if np.size(s.features_info) else []
    return dict(step=int(s.step), features_info=[_struct_to_dict(a, FEATURE_FIELDS) for a in fi],
                filter=_struct_to_dict(s.filter, FILTER_FIELDS))


def _shape_for_matlab(k, v):
    if sp.issparse(v):
        return v.tocsc()
    if isinstance(v, str):
        return v
    a = np.asarray(v)
    if a.size == 0:
        return np.zeros((0, 0))
    if a.dtype.kind in "iub":
        a = a.astype(np.float64)                      # MATLAB doubles throughout, as in the reference's own files
    if k in _COLUMN:
        return a.reshape(-1, 1)
    if k in _ROW:
        return a.reshape(1, -1)
    return a


def save_snapshot(path, snap, compress=True):
    fi = snap["features_info"]
    arr = np.zeros((1, len(fi)), dtype=[(k, object) for k in FEATURE_FIELDS])
    for i, a in enumerate(fi):
        for k in FEATURE_FIELDS:
            arr[0, i][k] = _shape_for_matlab(k, a.get(k, np.zeros((0, 0))))
    flt = {k: _shape_for_matlab(k, snap["filter"].get(k, np.zeros((0, 0)))) for k in FILTER_FIELDS}
    name = "snapshot%d" % int(snap["step"])
    sio.savemat(path, {name: {"features_info": arr, "filter": flt, "step": float(snap["step"])}}, format="5",
                do_compression=compress, oned_as="column", long_field_names=True)


def map_types(features_info):
    """features_info(i).type -> the ABI's landmark codes (map order = state order)."""
    t = []
    for a in features_info:
        if a["type"] not in ("inversedepth", "cartesian"):
            raise ValueError("unknown landmark type %r" % (a["type"],))
        t.append(_lib.INVDEPTH if a["type"] == "inversedepth" else _lib.CARTESIAN)
    return np.asarray(t, np.int32)


def filter_from_snapshot(snap, cam, which="k_k", dtype="f32", device=0, max_hyp=1000, max_landmarks=None):
    """Device-resident filter holding the snapshot's (x_k_k, p_k_k) or (x_k_km1, p_k_km1), descriptors included."""
    from .ekf import EkfFilter
    types = map_types(snap["features_info"])
    f = EkfFilter(cam, types, dtype=dtype, device=device, max_hyp=max_hyp, max_landmarks=max_landmarks,
                  std_z=float(np.asarray(snap["filter"].get("std_z", 1.0)).reshape(-1)[0]) if np.size(snap["filter"].get("std_z", 1.0)) else 1.0)
    x, P = snap["filter"]["x_" + which], snap["filter"]["p_" + which]
    if np.size(x) != f.n or np.shape(P) != (f.n, f.n):
        f.close()
        raise ValueError("snapshot state size %s does not match its features_info (n=%d)" % (np.shape(x), f.n))
    (f.set_x_p_k_k if which == "k_k" else f.set_x_p_k_km1)(np.asarray(x, float).reshape(-1), np.asarray(P, float))
    desc = [np.asarray(a.get("Descriptor", []), float).reshape(-1) for a in snap["features_info"]]
    if desc and all(d.size == 128 for d in desc):
        f.set_descriptors(np.stack(desc, 1))
    f.set_book(features_info_book(snap["features_info"]))
    return f


BOOK_FIELDS = ("times_predicted", "times_measured", "init_frame", "last_visible")
FLAG_FIELDS = ("individually_compatible", "low_innovation_inlier", "high_innovation_inlier")


def _int(v):
    return int(np.asarray(v).reshape(-1)[0]) if np.size(v) else 0


def features_info_book(features_info):
    """The device book (pre3_set_book): [times_predicted, times_measured, init_frame, last_visible] per entry."""
    return np.array([[_int(a.get(k, 0)) for k in BOOK_FIELDS] for a in features_info], np.int32).reshape(-1, 4)


def apply_policy_result(features_info, result, step, cand_uv, cand_xyz, cand_desc=None, book=None):
    """features_info after EkfFilter.map_management_policy: the deleted entries dropped (delete_features.m:63-74, without the reference's
    extra drop of a 2-entry list), one entry per accepted candidate appended with the fields of
    add_feature_to_info_vector_my_version_sift.m:37-60 (init_frame = last_visible = step - 1), per-frame fields emptied
    (update_features_info.m:30-44).  book (N, 4) -- EkfFilter.book() after the call -- overwrites the four counters of every entry."""
    gone = set(int(i) for i in result["deleted"])
    out = [dict(a) for i, a in enumerate(features_info) if i not in gone]
    cand_uv, cand_xyz = np.asarray(cand_uv, float).reshape(-1, 2), np.asarray(cand_xyz, float).reshape(-1, 3)
    conv = [c for i, c in enumerate(result.get("converted", np.zeros(len(features_info), int))) if i not in gone]
    for a, cv in zip(out, conv):
        if cv:
            a["type"] = "cartesian"
    for c in result["accepted"]:
        c = int(c)
        e = {k: np.zeros((0, 0)) for k in FEATURE_FIELDS}
        e.update(uv_when_initialized=cand_uv[c].copy(), half_patch_size_when_initialized=20, half_patch_size_when_matching=6,
                 times_predicted=0, times_measured=0, init_frame=step - 1, type="inversedepth", state_size=6, measurement_size=2,
                 individually_compatible=0, low_innovation_inlier=0, high_innovation_inlier=0, last_visible=step - 1,
                 Feature3d_in_code_coordinate=cand_xyz[c].copy())
        if cand_desc is not None:
            e["Descriptor"] = np.asarray(cand_desc, float).reshape(128, -1)[:, c].copy()
        out.append(e)
    for a in out:
        for k in FLAG_FIELDS:
            a[k] = 0
        for k in ("z", "h", "H", "S"):
            a[k] = np.zeros((0, 0))
    if book is not None:
        book = np.asarray(book).reshape(-1, 4)
        if len(book) != len(out):
            raise ValueError("book has %d rows, features_info %d entries" % (len(book), len(out)))
        for a, b in zip(out, book):
            for k, v in zip(BOOK_FIELDS, b):
                a[k] = int(v)
    return out


def update_snapshot_from_filter(snap, f, step=None):
    """The writer side of mono_slam.m:251-254: x_k_k / p_k_k, the landmark types, the last frame's IC / LI / HI flags and, on a booked filter,
    the book (times_predicted, times_measured, init_frame, last_visible) from the device."""
    out = dict(step=int(snap["step"] if step is None else step), features_info=[dict(a) for a in snap["features_info"]],
               filter=dict(snap["filter"]))
    if len(out["features_info"]) != f.N:
        raise ValueError("features_info has %d entries, the device map %d" % (len(out["features_info"]), f.N))
    out["filter"]["x_k_k"], out["filter"]["p_k_k"] = f.get_x_k_k(), f.get_p_k_k()
    for a, t in zip(out["features_info"], f.lm_type):
        a["type"] = "inversedepth" if t == _lib.INVDEPTH else "cartesian"
    try:
        book = f.book()
    except _lib.Pre3Error:                            # a filter without a book (pre3_set_book) keeps the snapshot's counters
        book = None
    if book is not None:
        for a, b in zip(out["features_info"], book):
            for k, v in zip(BOOK_FIELDS, b):
                a[k] = int(v)
    # the last frame's flags: IC = the installed measurements (matching_sift_based.m:131-134), LI / HI as the updates left them
    ic, lm_li, lm_hi = np.zeros(f.N, np.int32), np.zeros(f.N, np.int32), np.zeros(f.N, np.int32)
    meas = np.asarray(f.meas_idx, np.int64)
    if meas.size:
        li, hi = f.get_flags()
        ic[meas], lm_li[meas], lm_hi[meas] = 1, li, hi
    for a, i1, l1, h1 in zip(out["features_info"], ic, lm_li, lm_hi):
        a["individually_compatible"], a["low_innovation_inlier"], a["high_innovation_inlier"] = int(i1), int(l1), int(h1)
    return out
