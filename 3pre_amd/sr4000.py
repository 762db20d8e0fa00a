"""The SR4000 frame conditioned on the device: the .dat reader, the resident frame handle and mirrors of the reference's
readers and keypoint filters over the C ABI.

    read_xyz_sr4000.m:8-21                                   -> read_xyz_sr4000        (sigma = 2, zero padding)
    read_image_sr4000.m:10-24, normalzie_image.m:4           -> read_image_sr4000
    code_from_dr_ye/read_sr4000_data_dr_ye.m:8-90            -> read_sr4000_data_dr_ye (sigma = 1, replicated border)
    code_from_dr_ye/confidence_filtering.m:1-13              -> confidence_filtering
    SIFT_extract_save.m:68-88 over inittialize_depth_my_version.m:16-92 -> sift_extract (the SCAN_SIFT dict scanio.save_sift_result writes)
    code_from_dr_ye/vodometry_dr_ye.m:139-236                -> vodometry_dr_ye        (two resident frames, gate 1 on each, then vo.vo_pair_seeded)
    Calculate_V_Omega_RANSAC_dr_ye.m:25-50                   -> calculate_v_omega      (T, q, R, sta)
    initialize_features.m:95-99 + map_management.m:27-79     -> initialize_features_frames (two resident frames, gate 0 on each, then the policy)
    plane_fit_to_data.m:7-149                                -> plane_fit_to_data      (the fit on a resident frame, plane.plane_fit_frame_seeded)
    fv.m:41-48 + ekf_prediction.m                            -> fv_pair, ekf_prediction_frames (the VO pair and the prediction, u on the device)
    sift/sift_vedal.m:127-323 (+ the five MEX files)         -> SrFrame.sift, sift_vedal, sift_plan (the SIFT set made on the device)
    SIFT_extract_save.m:44-88                                -> sift_extract_frame     (sift + gate 0 on a resident frame, nothing uploaded)

    read_xyz_sr4000.m:2-3,25-42 (load of d1_%04d.dat)        -> loadtxt_device, SrFrame.load_text, parse="device" (the text parsed on the device, section 26)

    aux_code/compensate_badpixel_soonhac.m:5-14              -> SrFrame.set_compensation(COMP_BADPIXEL, cutoff), compensate_badpixel_soonhac (section 32)
    code_from_dr_ye/read_image_sr4000_dr_ye.m:21-24          -> SrFrame.set_compensation(COMP_IMAGE_MEDIAN), read_image_sr4000_dr_ye
    medfilt2(A, [3 3]) / medfilt2(A, [3 3], 'symmetric')     -> medfilt2

All compute runs in libpre3.so on the GPU; this module reads the file's bytes -- parsed on the host (numpy.loadtxt, the default) or handed to the device
as they are (parse="device") -- and marshals numpy arrays.
"""
import ctypes as C

import numpy as np

from ._lib import Pre3Error, check, dptr, f64, lib

ROWS, COLS = 144, 176                     # a d1_%04d.dat frame
MAX_KEYPOINTS = 8192                      # PRE3_SR_MAX_KEYPOINTS
MODE_XYZ, MODE_DR_YE = 0, 1               # read_xyz_sr4000.m / read_image_sr4000.m; read_sr4000_data_dr_ye.m
GATE_DEPTH, GATE_CONFIDENCE = 0, 1        # inittialize_depth_my_version.m:40,74; confidence_filtering.m:8
SIFT_LEVELS, SIFT_MAX_TAPS = 6, 32        # PRE3_SIFT_LEVELS, PRE3_SIFT_MAX_TAPS
COMP_NONE, COMP_BADPIXEL, COMP_IMAGE_MEDIAN = 0, 1, 2      # PRE3_SR_COMP_*: nothing; compensate_badpixel_soonhac.m; read_image_sr4000_dr_ye.m:21-24
PADDING = {"zeros": 0, "symmetric": 1}    # medfilt2's default, and its 'symmetric'


def gauss3(sigma):
    """fspecial('gaussian', [3 3], sigma) as the library forms it: (3, 3), G[i + 1, j + 1] = h(i, j)."""
    w = np.zeros(9)
    check(lib.pre3_sr_gauss3(float(sigma), dptr(w)))
    return w.reshape(3, 3).T.copy()


def medfilt2(A, padding="zeros", device=0):
    """medfilt2(A, [3 3]) (padding="zeros", MATLAB's default) or medfilt2(A, [3 3], 'symmetric') on the device (pre3_sr_medfilt3): the fifth smallest of
    each 3 x 3 window; a NaN in the window makes the pixel NaN.  Returns doubles of A's shape (uint8 values stay uint8 values: a median selects)."""
    if padding not in PADDING:
        raise ValueError("padding must be 'zeros' or 'symmetric', not %r" % (padding,))
    A = np.asfortranarray(f64(A))
    if A.ndim != 2:
        raise Pre3Error(-1, "medfilt2: A must be a matrix")
    out = np.zeros(A.shape, order="F")
    check(lib.pre3_sr_medfilt3(int(device), A.shape[0], A.shape[1], dptr(A), PADDING[padding], dptr(out)))
    return out


def compensate_badpixel_soonhac(img, x, y, z, c, confidence_cut_off, device=0):
    """[img, x, y, z, c] = compensate_badpixel_soonhac(img, x, y, z, c, confidence_cut_off) (aux_code/compensate_badpixel_soonhac.m:5-14): four symmetric
    medians on the device, taken on the planes as given, selected where c < confidence_cut_off.  img keeps its dtype."""
    e_index = f64(c) < float(confidence_cut_off)
    out = []
    for p in (img, x, y, z):
        p = np.array(p)
        q = p.copy()
        q[e_index] = medfilt2(p, "symmetric", device)[e_index].astype(p.dtype)
        out.append(q)
    return out[0], out[1], out[2], out[3], c


def sift_plan(rows, cols):
    """pre3_sift_plan_get: dict(O, rows (O,), cols (O,), sigma0, pow2 (5,), sigma (O, 6), W (O, 6), taps (O, 6, 32)) -- the bits the launches use"""
    O = C.c_int32(0)
    orows, ocols = np.zeros(32, np.int32), np.zeros(32, np.int32)
    sigma0, pow2 = C.c_double(0), np.zeros(5)
    sigma, W, taps = np.zeros((32, SIFT_LEVELS)), np.zeros((32, SIFT_LEVELS), np.int32), np.zeros((32, SIFT_LEVELS, SIFT_MAX_TAPS))
    check(lib.pre3_sift_plan_get(int(rows), int(cols), C.byref(O), dptr(orows), dptr(ocols), C.byref(sigma0), dptr(pow2), dptr(sigma), dptr(W), dptr(taps)))
    O = O.value
    return dict(O=O, rows=orows[:O].copy(), cols=ocols[:O].copy(), sigma0=sigma0.value, pow2=pow2, sigma=sigma[:O].copy(), W=W[:O].copy(),
                taps=taps[:O].copy())


def load_dat(path, rows=ROWS):
    """A d1_%04d.dat frame (numpy.loadtxt): rows 1-144 z, 145-288 x, 289-432 y, 433-576 amplitude, 577-720 confidence (when the file has them),
    row 721 the timestamp in its first entry (when the file has it).  Returns dict(z, x, y, amp, conf or None, timestamp or -1)."""
    a = np.loadtxt(path, dtype=np.float64, ndmin=2)
    if a.shape[0] < 4 * rows:
        raise ValueError("%s: %d rows, fewer than the %d of z, x, y and the amplitude" % (path, a.shape[0], 4 * rows))
    out = {k: np.asfortranarray(a[i * rows:(i + 1) * rows]) for i, k in enumerate(("z", "x", "y", "amp"))}
    out["conf"] = np.asfortranarray(a[4 * rows:5 * rows]) if a.shape[0] >= 5 * rows else None      # read_xyz_sr4000.m:25-34
    out["timestamp"] = float(a[5 * rows, 0]) if a.shape[0] == 5 * rows + 1 else -1.0                # :36-42
    return out


TEXT_STATUS = ("ok", "bad token", "ragged rows", "wrong shape for this handle", "undecided token", "negative or non-finite amplitude", "empty text")


class TextInfo(C.Structure):
    """pre3_sr_text_info"""
    _fields_ = [(k, C.c_int32) for k in ("status", "rows", "cols", "has_conf", "has_timestamp", "n_tokens", "n_undecided", "bad_row", "bad_col")] + [
        ("bad_offset", C.c_int64), ("timestamp", C.c_double)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["status_text"] = TEXT_STATUS[self.status] if 0 <= self.status < len(TEXT_STATUS) else "?"
        return d


def text_limits():
    """(chunk_bytes, max_bytes) of the device parse"""
    chunk, top = C.c_int32(0), C.c_int64(0)
    check(lib.pre3_sr_text_limits(C.byref(chunk), C.byref(top)))
    return chunk.value, top.value


def _text_bytes(data):
    """the bytes themselves, or the contents of the file `data` names"""
    if isinstance(data, (bytes, bytearray, memoryview)):
        return bytes(data)
    with open(data, "rb") as fh:
        return fh.read()


def _text_check(rc, info):
    if rc != 0:
        e = Pre3Error(rc, lib.pre3_last_error().decode(errors="replace"))
        e.info = info.as_dict()
        raise e


def loadtxt_device(data, device=0):
    """MATLAB's load / numpy.loadtxt of a rectangular ASCII matrix, parsed on the device (pre3_sr_text_parse): data is bytes or a path.  Returns
    (ndarray (rows, cols), info dict); a refused text raises Pre3Error with the status text, its .info the same dict."""
    text = _text_bytes(data)
    info = TextInfo()
    cap = (len(text) + 1) // 2                                # a token and its separator take two bytes
    out = np.zeros(max(cap, 1))
    _text_check(lib.pre3_sr_text_parse(int(device), text, len(text), dptr(out), cap, C.byref(info)), info)
    return out[:info.rows * info.cols].reshape((info.rows, info.cols), order="F").copy(), info.as_dict()


class SrFrame:
    """One resident, conditioned frame (pre3_sr_frame): load(planes, mode) queues the upload and the two conditioning launches and returns;
    planes(), image(), maxima() and keypoints() wait for them."""

    def __init__(self, rows=ROWS, cols=COLS, device=0):
        self.rows, self.cols = int(rows), int(cols)
        self._h = C.c_void_p()
        self.has_conf = False
        self.n_kept = 0                       # of the last keypoints() call: sizes vo.vo_pair_seeded's outputs
        check(lib.pre3_sr_frame_create(C.byref(self._h), int(device), self.rows, self.cols))

    def close(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.pre3_sr_frame_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _plane(self, a, name):
        a = np.asfortranarray(f64(a))
        if a.shape != (self.rows, self.cols):
            raise Pre3Error(-1, "SrFrame.load: %s is %s, the handle holds %d x %d frames" % (name, a.shape, self.rows, self.cols))
        return a

    def set_compensation(self, form, cutoff=1.0):
        """the compensation of every load() / load_text() that follows (pre3_sr_frame_set_compensation; the resident frame stays as it is): COMP_NONE,
        COMP_BADPIXEL (x, y, z and the image replaced by their 3 x 3 symmetric median where conf < cutoff) or COMP_IMAGE_MEDIAN (the uint8 image
        median-filtered with zero padding), in front of the mode's Gaussian"""
        check(lib.pre3_sr_frame_set_compensation(self._h, int(form), float(cutoff)))
        return self

    @property
    def compensation(self):
        """(form, cutoff): the setting the next load takes"""
        form, cutoff = C.c_int32(0), C.c_double(0)
        check(lib.pre3_sr_frame_get_compensation(self._h, C.byref(form), C.byref(cutoff)))
        return form.value, cutoff.value

    def bad_pixels(self):
        """(form_of_frame, n_bad): the form the resident frame was conditioned with and how many of its pixels were compensated (0 unless the form is
        COMP_BADPIXEL and the frame has a confidence map); waits"""
        form, n = C.c_int32(0), C.c_int32(0)
        check(lib.pre3_sr_frame_bad_pixels(self._h, C.byref(form), C.byref(n)))
        return form.value, n.value

    def load(self, planes, mode=MODE_XYZ):
        """planes: dict(z, x, y, amp, conf or None) as load_dat returns it; mode 0: sigma = 2, zero padding; 1: sigma = 1, replicate"""
        p = [self._plane(planes[k], k) for k in ("z", "x", "y", "amp")]
        conf = planes.get("conf")
        conf = None if conf is None else self._plane(conf, "conf")
        check(lib.pre3_sr_frame_load(self._h, int(mode), dptr(p[0]), dptr(p[1]), dptr(p[2]), dptr(p[3]), dptr(conf)))
        self.has_conf = conf is not None
        return self

    def load_text(self, data, mode=MODE_XYZ):
        """load() from the .dat file's bytes (or its path), parsed on the device (pre3_sr_frame_load_text): one wait for the status, then the
        conditioning launches are queued as in load().  Returns dict(has_conf, timestamp (-1 without one), rows); a refused file raises Pre3Error
        with the status text and leaves the handle as it was."""
        text = _text_bytes(data)
        info = TextInfo()
        _text_check(lib.pre3_sr_frame_load_text(self._h, int(mode), text, len(text), C.byref(info)), info)
        self.has_conf = bool(info.has_conf)
        return dict(has_conf=self.has_conf, timestamp=float(info.timestamp), rows=int(info.rows))

    def _new(self):
        return np.zeros((self.rows, self.cols), order="F")

    def planes(self):
        """(x, y, z, confidence_map or None): the filtered planes, the confidence map as loaded"""
        x, y, z = self._new(), self._new(), self._new()
        conf = self._new() if self.has_conf else None
        check(lib.pre3_sr_frame_get(self._h, dptr(x), dptr(y), dptr(z), None, dptr(conf), None, None))
        return x, y, z, conf

    def image(self):
        """the filtered amplitude image, uint8"""
        img = self._new()
        check(lib.pre3_sr_frame_get(self._h, None, None, None, dptr(img), None, None, None))
        return img.astype(np.uint8)

    def feed_image(self, filt):
        """this frame's filtered image as the frame an ekf.EkfFilter's patch search reads (pre3_set_image_frame): on the device, no wait"""
        filt.set_image_frame(self)

    def maxima(self):
        """(imax, cmax)"""
        imax, cmax = C.c_double(0), C.c_double(0)
        check(lib.pre3_sr_frame_get(self._h, None, None, None, None, None, C.byref(imax), C.byref(cmax)))
        return imax.value, cmax.value

    def keypoints(self, frm, des=None, gate=GATE_DEPTH):
        """frm (ldf, K): SIFT frames, row 1 the pixel column, row 2 the pixel row (1-based); des (ND, K) or None.  Returns dict(keep_idx (0-based),
        frames (ldf, n), descriptors (ND, n), and for gate 0 xyz (3, n) = [-x; -y; z] and rho (n,) = 1 / range)."""
        frm = np.asfortranarray(f64(frm))
        if frm.ndim != 2:
            raise Pre3Error(-1, "SrFrame.keypoints: frm must be ldf x K")
        ldf, K = frm.shape
        des = np.zeros((0, K), order="F") if des is None else np.asfortranarray(f64(des))
        if des.ndim != 2 or des.shape[1] != K:
            raise Pre3Error(-1, "SrFrame.keypoints: des must be ND x K")
        ND = des.shape[0]
        n = C.c_int32(0)
        Kb = min(max(K, 1), MAX_KEYPOINTS)
        idx, frm_o, des_o = np.zeros(Kb, np.int32), np.zeros((ldf, Kb), order="F"), np.zeros((ND, Kb), order="F")
        xyz, rho = np.zeros((3, Kb), order="F"), np.zeros(Kb)
        check(lib.pre3_sr_frame_keypoints(self._h, int(gate), ldf, K, dptr(frm), ND, dptr(des), C.byref(n), dptr(idx), dptr(frm_o), dptr(des_o),
                                          dptr(xyz), dptr(rho)))
        n = self.n_kept = n.value
        return self._gate_outputs(gate, n, idx, frm_o, des_o, xyz, rho)

    @staticmethod
    def _gate_outputs(gate, n, idx, frm_o, des_o, xyz, rho):
        out = dict(keep_idx=idx[:n].copy(), frames=frm_o[:, :n].copy(order="F"), descriptors=des_o[:, :n].copy(order="F"))
        if int(gate) == GATE_DEPTH:
            out["xyz"], out["rho"] = xyz[:, :n].copy(order="F"), rho[:n].copy()
        return out

    def sift(self, image=None, strict_reference=1, one_based=True, want_arrays=True):
        """sift_vedal on `image` (rows x cols) or on the frame's own filtered image; the set stays in the handle's keypoint block as the raw set
        (1-based frames), ready for gate().  Returns dict(frames (4, K), descriptors (128, K), counts (O, 4) = maxima, inside the boundary, refined,
        oriented per octave); one_based=False: sift_vedal's own 0-based x, y in `frames`.  want_arrays=False brings back the counts only."""
        img = None if image is None else self._plane(image, "image")
        K = C.c_int32(0)
        counts = np.zeros((32, 4), np.int32)
        frm = np.zeros((4, MAX_KEYPOINTS), order="F") if want_arrays else None
        des = np.zeros((128, MAX_KEYPOINTS), order="F") if want_arrays else None
        check(lib.pre3_sr_frame_sift(self._h, dptr(img), int(strict_reference), int(bool(one_based)), C.byref(K), dptr(frm), dptr(des), dptr(counts)))
        K = K.value
        O = sift_plan(self.rows, self.cols)["O"]
        out = dict(K=K, counts=counts[:O].astype(np.int64))
        if want_arrays:
            out["frames"], out["descriptors"] = frm[:, :K].copy(order="F"), des[:, :K].copy(order="F")
        return out

    def gate(self, gate=GATE_DEPTH):
        """keypoints()' gate over the raw set already in the block -- sift()'s, or a keypoints() upload of (4, K) frames and (128, K) descriptors; any
        other shape is refused by the library (the outputs are sized for 4 and 128): nothing is uploaded.  Returns what keypoints() returns."""
        n = C.c_int32(0)
        Kb = MAX_KEYPOINTS
        idx, frm_o, des_o = np.zeros(Kb, np.int32), np.zeros((4, Kb), order="F"), np.zeros((128, Kb), order="F")
        xyz, rho = np.zeros((3, Kb), order="F"), np.zeros(Kb)
        check(lib.pre3_sr_frame_gate(self._h, int(gate), C.byref(n), dptr(idx), dptr(frm_o), dptr(des_o), dptr(xyz), dptr(rho)))
        n = self.n_kept = n.value
        return self._gate_outputs(gate, n, idx, frm_o, des_o, xyz, rho)

    def sift_refined(self):
        """the refined points of the last sift(), before the orientations: (4, n) = x, y, s, octave (0-based, octave coordinates), all octaves in order"""
        n = C.c_int32(0)
        check(lib.pre3_sr_frame_sift_refined(self._h, C.byref(n), None))
        out = np.zeros((4, max(n.value, 1)), order="F")
        check(lib.pre3_sr_frame_sift_refined(self._h, C.byref(n), dptr(out)))
        return out[:, :n.value].copy(order="F")

    def sift_level(self, o, s, dog=False):
        """level s (0-based) of octave o of gss (dog=False) or dogss (dog=True) of the last sift()"""
        pl = sift_plan(self.rows, self.cols)
        if not 0 <= int(o) < pl["O"]:
            raise Pre3Error(-1, "SrFrame.sift_level: octave %d outside %d octaves" % (o, pl["O"]))
        out = np.zeros((pl["rows"][o], pl["cols"][o]), order="F")
        check(lib.pre3_sr_frame_sift_level(self._h, int(o), int(s), int(bool(dog)), dptr(out)))
        return out


def sift_vedal(I, strict_reference=1, device=0):
    """[frames, descriptors] = sift_vedal(I) (0-based frames, as the reference returns them) on a handle of I's size, used once"""
    I = np.asfortranarray(f64(I))
    with SrFrame(I.shape[0], I.shape[1], device) as f:
        out = f.sift(I, strict_reference, one_based=False)
    return out["frames"], out["descriptors"]


def sift_extract_frame(frame, idx_scan):
    """SIFT_extract_save.m:44-88 on a resident frame: sift on its own image, :55-56's 1-based frames, the depth gate -- the SCAN_SIFT dict of
    sift_extract, with no SIFT array uploaded"""
    raw = frame.sift()
    out = frame.gate(GATE_DEPTH)
    return dict(idxScan=int(idx_scan), Image=frame.image(), Descriptor_RAW=raw["descriptors"], SCALE_ORIENT_POS_RAW=raw["frames"],
                Descriptor=out["descriptors"], SCALE_ORIENT_POS=out["frames"], XYZ_DATA=out["xyz"], initial_rho=out["rho"], keep_idx=out["keep_idx"])


def _check_parse(parse):
    if parse not in ("host", "device"):
        raise ValueError("parse must be 'host' or 'device', not %r" % (parse,))
    return parse == "device"


def _load_into(f, path, mode, parse):
    """the file `path` into the handle f, parsed on the host or on the device: dict(conf (None without a map), timestamp)"""
    if _check_parse(parse):
        r = f.load_text(path, mode)
        return dict(conf=True if r["has_conf"] else None, timestamp=r["timestamp"])
    d = load_dat(path, f.rows)
    f.load(d, mode)
    return d


def _compensated(f, compensation):
    """a handle this module created, with the caller's compensation=(form, cutoff) set on it (None: the default, none)"""
    if compensation is not None:
        try:
            f.set_compensation(*compensation)
        except Exception:
            f.close()
            raise
    return f


def _conditioned(path, mode, device, parse="host", compensation=None):
    if _check_parse(parse):                                   # a d1_%04d.dat frame (the handle's size is fixed before the text is seen)
        f = _compensated(SrFrame(ROWS, COLS, device), compensation)
        try:
            return _load_into(f, path, mode, parse), f
        except Exception:
            f.close()
            raise
    d = load_dat(path)
    f = _compensated(SrFrame(d["z"].shape[0], d["z"].shape[1], device), compensation).load(d, mode)
    return d, f


def read_xyz_sr4000(path, with_timestamp=False, device=0, parse="host", compensation=None):
    """[x, y, z, confidence_map (, timestamp)] = read_xyz_sr4000(...) on the file `path`; confidence_map is None for a frame without one.
    parse="device": the text is parsed on the device (a 144 x 176 frame).  compensation=(form, cutoff): SrFrame.set_compensation on the frame."""
    d, f = _conditioned(path, MODE_XYZ, device, parse, compensation)
    with f:
        out = f.planes()
    return out + (d["timestamp"],) if with_timestamp else out


def read_image_sr4000(path, device=0, parse="host", compensation=None):
    """im = read_image_sr4000(...) on the file `path`: uint8"""
    d, f = _conditioned(path, MODE_XYZ, device, parse, compensation)
    with f:
        return f.image()


def read_image_sr4000_dr_ye(path, device=0, parse="host"):
    """img = read_image_sr4000_dr_ye(...) on the file `path` (code_from_dr_ye/read_image_sr4000_dr_ye.m): read_image_sr4000 with the uint8 image
    median-filtered (:21-24, zero padding) in front of the Gaussian -- mode 0 under COMP_IMAGE_MEDIAN"""
    return read_image_sr4000(path, device, parse, compensation=(COMP_IMAGE_MEDIAN, 1.0))


def read_sr4000_data_dr_ye(path, with_timestamp=False, device=0, parse="host", compensation=None):
    """[x, y, z, confidence_map, img1 (, timestamp)] = read_sr4000_data_dr_ye(path).  Deviation: a frame without confidence rows gets the same
    normalised image as one with them (the reference leaves it un-normalised, :34-59).  compensation=(COMP_BADPIXEL, 1.0) switches on the call its
    author left commented out at :44."""
    d, f = _conditioned(path, MODE_DR_YE, device, parse, compensation)
    with f:
        out = f.planes() + (f.image(),)
    return out + (d["timestamp"],) if with_timestamp else out


def confidence_filtering(frm, des, frame):
    """[frm, des] = confidence_filtering(frm, des, confidence_map), the map being the resident frame's"""
    out = frame.keypoints(frm, des, GATE_CONFIDENCE)
    return out["frames"], out["descriptors"]


def sift_extract(frames, descriptors, frame, idx_scan, image=None):
    """SIFT_extract_save.m:44-45,68-88: the SCAN_SIFT dict of scan idx_scan from its 1-based SIFT frames (4, K) (as :55-56 leave them) and descriptors
    (128, K), the depth gate run on the resident frame.  image: SCAN_SIFT.Image (default: the frame's own)."""
    out = frame.keypoints(frames, descriptors, GATE_DEPTH)
    return dict(idxScan=int(idx_scan), Image=frame.image() if image is None else np.asarray(image),
                Descriptor_RAW=np.array(descriptors, dtype=np.float64), SCALE_ORIENT_POS_RAW=np.array(frames, dtype=np.float64),
                Descriptor=out["descriptors"], SCALE_ORIENT_POS=out["frames"], XYZ_DATA=out["xyz"], initial_rho=out["rho"], keep_idx=out["keep_idx"])


def plane_fit_to_data(frame, seed, seq=0, n_draw=1001, box=None, t=0.02):
    """[R, T] = plane_fit_to_data(idx) with the scan already resident (plane_fit_to_data.m:13 reads read_xyz_sr4000: a frame loaded in mode 0): the box
    is gathered from the frame's filtered planes on the device and nothing is read back to be sent again.  Returns
    plane.plane_fit_frame_seeded's dict; R = out["R"], and mono_slam.m:192 passes R' to the heading update (EkfFilter.heading_from_frame_seeded does
    both in one call)."""
    from . import plane
    return plane.plane_fit_frame_seeded(frame, seed, seq, n_draw, box, t)


def vodometry_dr_ye(dat1, dat2, sift1, sift2, seed, seq=0, thresh=1.5, device=0, frames=None):
    """vodometry_dr_ye.m:139-236 on the files dat1, dat2 (frame 1 the earlier one) and their SIFT sets sift1, sift2 = (frames (>=2, K), descriptors
    (128, K)): each file is conditioned on the device in mode 1 and stays there, confidence_filtering (gate 1) drops the keypoints of low confidence --
    the depth gate (gate 0) stands in on a frame without confidence rows --, then vo.vo_pair_seeded runs siftmatch, rst and the seeded RANSAC between
    the two resident frames.  Returns vo_pair_seeded's dict plus kept1 / kept2 (the keep_idx of each frame: match holds positions in those lists).
    frames: an optional (SrFrame, SrFrame) pair to reuse instead of creating two."""
    from . import vo
    d1, d2 = load_dat(dat1), load_dat(dat2)
    own = frames is None
    f1, f2 = (SrFrame(d1["z"].shape[0], d1["z"].shape[1], device), SrFrame(d2["z"].shape[0], d2["z"].shape[1], device)) if own else frames
    try:
        kept = []
        for f, d, (frm, des) in ((f1, d1, sift1), (f2, d2, sift2)):
            f.load(d, MODE_DR_YE)
            kept.append(f.keypoints(frm, des, GATE_CONFIDENCE if d["conf"] is not None else GATE_DEPTH)["keep_idx"])
        out = vo.vo_pair_seeded(f1, f2, seed, seq, thresh)
    finally:
        if own:
            f1.close(); f2.close()
    out["kept1"], out["kept2"] = kept
    return out


def calculate_v_omega(dat1, dat2, sift1, sift2, seed, seq=0, **kw):
    """[T, q, R, sta] of Calculate_V_Omega_RANSAC_dr_ye.m:25-50: the translation, R2q(R), the rotation and the solution state; the identity motion unless
    sta == 1 (:41-50) -- u = [T; q] is what EkfFilter.ekf_prediction takes"""
    out = vodometry_dr_ye(dat1, dat2, sift1, sift2, seed, seq, **kw)
    ok = out["sta"] == 1
    return out["u"][:3].copy(), out["u"][3:].copy(), (out["rot"].copy() if ok else np.eye(3)), out["sta"]


def fv_pair(step):
    """fv.m:41-48's index rule: None for the frames whose prediction takes the identity motion (step - 1 <= 1), else the scans (step - 2, step - 1)
    whose VO increment Calculate_V_Omega_RANSAC_dr_ye(step - 2, step - 1) supplies"""
    step = int(step)
    return None if step - 1 <= 1 else (step - 2, step - 1)


def ekf_prediction_frames(filt, step, frames, seed, seq=0, thresh=1.5, wait=True):
    """fv.m:41-48 + ekf_prediction.m for frame `step` with the scans resident: frames maps a scan number to its SrFrame, each with a keypoint record
    (gate 1, as vodometry_dr_ye).  The first frames are predicted with the identity motion; from then on EkfFilter.ekf_prediction_pair_seeded runs the VO
    front end between frames[step - 2] and frames[step - 1] and the prediction behind it, u staying on the device.  Returns that
    call's result (None for the identity frames, or with wait=False).  The process noise is the filter's own (the reference's constant, or
    EkfFilter.set_process_noise); ekf_prediction_frames_cov takes the pair's."""
    return _prediction_frames(filt, step, frames, seed, seq, thresh, wait, "context")


def ekf_prediction_frames_cov(filt, step, frames, seed, seq=0, thresh=1.5, wait=True):
    """ekf_prediction_frames with the pair's covariance, computed on the device from its inliers, as that prediction's process noise
    (predict_state_and_covariance.m:115; EkfFilter.ekf_prediction_pair_cov_seeded).  The identity frames, and a pair whose
    covariance is not valid or whose u is not taken, are predicted with the filter's own noise."""
    return _prediction_frames(filt, step, frames, seed, seq, thresh, wait, "pair")


def ekf_prediction_frames_icp(filt, step, frames, seed, seq=0, thresh=1.5, stride=1, res=0.02, max_error=float("inf"), noise=0, wait=True):
    """ekf_prediction_frames with the dense ICP refining the pair's pose on the same two resident frames in front of the prediction
    (EkfFilter.ekf_prediction_icp_pair_seeded): the ICP's u when it ended by the reference's rule within max_error, with the
    process noise `noise` names (0 the filter's own, 1 the pair's covariance, 2 the ICP's closed-form covariance, 3 that plus the filter's own).  The
    identity frames are predicted with the filter's own noise."""
    pair = fv_pair(step)
    if pair is None:
        filt.ekf_prediction([0, 0, 0, 1, 0, 0, 0])
        return None
    return filt.ekf_prediction_icp_pair_seeded(frames[pair[0]], frames[pair[1]], seed, seq, thresh, stride, res, max_error, noise, wait)


def _prediction_frames(filt, step, frames, seed, seq, thresh, wait, noise):
    pair = fv_pair(step)
    if pair is None:
        filt.ekf_prediction([0, 0, 0, 1, 0, 0, 0])
        return None
    call = filt.ekf_prediction_pair_cov_seeded if noise == "pair" else filt.ekf_prediction_pair_seeded
    return call(frames[pair[0]], frames[pair[1]], seed, seq, thresh, wait)


def initialize_features_frames(filt, step, dat_prev, dat_cur, sift_prev, sift_cur, seed, seq=0, thresh=1.5, mode=MODE_XYZ, device=0, frames=None, **policy):
    """initialize_features.m:95-99 in front of map_management.m:27-79 on the files dat_prev, dat_cur (the previous and the current scan) and their SIFT
    sets = (frames (>=2, K), descriptors (128, K)): each file is conditioned on the device and stays there, the depth gate (gate 0,
    SIFT_extract_save.m:71-88) keeps Descriptor / SCALE_ORIENT_POS / XYZ_DATA of each scan, then
    EkfFilter.map_management_policy_frames_seeded matches the two kept sets, takes the candidates from the previous scan and runs the policy on `filt`.
    Returns that call's dict plus kept_prev / kept_cur (each scan's keep_idx: match holds 1-based positions in those lists) and cand_idx, the caller's
    index into sift_prev of every candidate.  frames: an optional (SrFrame, SrFrame) pair to reuse; policy: min_features, box, std_pxl, ..."""
    d1, d2 = load_dat(dat_prev), load_dat(dat_cur)
    own = frames is None
    f1, f2 = (SrFrame(d1["z"].shape[0], d1["z"].shape[1], device), SrFrame(d2["z"].shape[0], d2["z"].shape[1], device)) if own else frames
    try:
        kept = []
        for f, d, (frm, des) in ((f1, d1, sift_prev), (f2, d2, sift_cur)):
            f.load(d, mode)
            kept.append(f.keypoints(frm, des, GATE_DEPTH)["keep_idx"])
        out = filt.map_management_policy_frames_seeded(step, f1, f2, seed, seq, thresh, **policy)
    finally:
        if own:
            f1.close(); f2.close()
    out["kept_prev"], out["kept_cur"] = kept
    out["cand_idx"] = kept[0][out["match"][0].astype(np.int64) - 1] if out["K"] else np.zeros(0, np.int32)
    return out


def _own_pair(shape1, shape2, device, compensation):
    """two handles of this module's own, the caller's compensation set on both"""
    f1 = _compensated(SrFrame(shape1[0], shape1[1], device), compensation)
    try:
        return f1, _compensated(SrFrame(shape2[0], shape2[1], device), compensation)
    except Exception:
        f1.close()
        raise


def _two_frames(d1, d2, device, frames, compensation=None):
    own = frames is None
    f1, f2 = _own_pair(d1["z"].shape, d2["z"].shape, device, compensation) if own else frames
    return own, f1, f2


def _two_frames_for(dat1, dat2, device, frames, parse, compensation=None):
    """(own, f1, f2, d1, d2): the pair of handles and, for the host parse, the two files' planes (None for the device parse: _load_into reads them).
    compensation=(form, cutoff) is set on the handles made here; a caller's frames= keep what the caller set on them."""
    if _check_parse(parse):
        own = frames is None
        f1, f2 = _own_pair((ROWS, COLS), (ROWS, COLS), device, compensation) if own else frames
        return own, f1, f2, None, None
    d1, d2 = load_dat(dat1), load_dat(dat2)
    return _two_frames(d1, d2, device, frames, compensation) + (d1, d2)


def _load_pair_member(f, path, d, mode, parse):
    if d is None:
        return _load_into(f, path, mode, parse)
    f.load(d, mode)
    return d


def vodometry_frames_pnp(dat1, dat2, seed, cam, seq=0, thresh=1.5, undistort=True, device=0, frames=None, parse="host", compensation=None):
    """vodometry_frames with RANSAC_CALC_VER2.m:191 behind it (vo.vo_pair_pnp_seeded): out["pnp"] is the pose of the pair's
    inliers from prev's range points and cur's pixels alone -- no depth of the current frame.  cam = [f, Cx, Cy, k1, k2, nRows, nCols]; the pixels
    go through undistort_fm_my_version.m first unless undistort=False."""
    return vodometry_frames(dat1, dat2, seed, seq, thresh, device, frames, parse, compensation, _pnp=(cam, undistort))


def vodometry_frames(dat1, dat2, seed, seq=0, thresh=1.5, device=0, frames=None, parse="host", compensation=None, _pnp=None):
    """vodometry_dr_ye with the SIFT sets made on the device: each file is conditioned in mode 1, SrFrame.sift runs on its filtered image, gate 1 (gate 0
    on a frame without confidence rows) drops keypoints, then vo.vo_pair_seeded.  The gated set is 1-based, as vodometry_dr_ye.m:73-74,120-122 make
    it before confidence_filtering.  parse="device": the two texts are parsed on the device too (SrFrame.load_text).  compensation=(form, cutoff):
    SrFrame.set_compensation on the two frames made here (a caller's frames= keep their own setting)."""
    from . import vo
    own, f1, f2, d1, d2 = _two_frames_for(dat1, dat2, device, frames, parse, compensation)
    try:
        kept = []
        for f, path, d in ((f1, dat1, d1), (f2, dat2, d2)):
            d = _load_pair_member(f, path, d, MODE_DR_YE, parse)
            f.sift(want_arrays=False)
            kept.append(f.gate(GATE_CONFIDENCE if d["conf"] is not None else GATE_DEPTH)["keep_idx"])
        out = vo.vo_pair_seeded(f1, f2, seed, seq, thresh) if _pnp is None else vo.vo_pair_pnp_seeded(f1, f2, seed, _pnp[0], seq, thresh, _pnp[1])
    finally:
        if own:
            f1.close(); f2.close()
    out["kept1"], out["kept2"] = kept
    return out


def initialize_features_scans(filt, step, dat_prev, dat_cur, seed, seq=0, thresh=1.5, mode=MODE_XYZ, device=0, frames=None, parse="host", compensation=None,
                              **policy):
    """initialize_features_frames with the SIFT sets made on the device (SrFrame.sift on each conditioned scan, then the depth gate); cand_idx indexes the
    previous scan's raw set.  parse="device": the two texts are parsed on the device too.  compensation=(form, cutoff): as in vodometry_frames."""
    own, f1, f2, d1, d2 = _two_frames_for(dat_prev, dat_cur, device, frames, parse, compensation)
    try:
        kept = []
        for f, path, d in ((f1, dat_prev, d1), (f2, dat_cur, d2)):
            _load_pair_member(f, path, d, mode, parse)
            f.sift(want_arrays=False)
            kept.append(f.gate(GATE_DEPTH)["keep_idx"])
        out = filt.map_management_policy_frames_seeded(step, f1, f2, seed, seq, thresh, **policy)
    finally:
        if own:
            f1.close(); f2.close()
    out["kept_prev"], out["kept_cur"] = kept
    out["cand_idx"] = kept[0][out["match"][0].astype(np.int64) - 1] if out["K"] else np.zeros(0, np.int32)
    return out
