"""Sparse fp64 restatement of map management's congruence  P <- A P A' + D  (test infrastructure, CPU only).

delete_a_feature.m:47-51, add_a_feature_covariance_inverse_depth.m:29-90 (+ hinv_my_version.m:26-53, add_features_inverse_depth.m:41)
and inversedepth_2_cartesian.m:36-72 written as ONE row map: new row a is either a copy of old row src[a] or a short list of
(old column, coefficient) pairs.  oracle/np_twin.map_convert multiplies dense n x n matrices once per converted landmark, which takes
minutes at n = 2000..3000; here `apply` gathers rows and columns and touches only the few computed ones, so it serves as the reference
of tests/test_gpu_map_blocks.py at two, three and four column blocks.  The formulas are taken from the .m files above (paths under the
reference's matlab_code/), not from 3pre_amd/csrc/pre3_map.hip; the leaf helpers (q2r, undistortion, the distortion Jacobian,
dRq_times_a_by_dq) are the numpy twin's.  tests/test_map_congruence_ref.py checks this module against the twin and the C oracle.

The second half (SIZES, conversion_case, management_case ...) defines the inputs of the GPU cases, so that the CPU checks of the input
conditions and the GPU tests build the very same arrays.

THE GATE FOR COMPUTED ENTRIES.  Errors are measured entry by entry in units of bound[a, b] = (|A| |P| |A|' + |D|)[a, b]; u is the unit
roundoff of the context's element type.  The device forms an entry as two nested fma sums in the element type with at most 6 non-zero
terms each: rounding the coefficients to the element type, the inner and the outer sum cost at most 14 u, the intermediate is rounded
once and D is added in double and rounded once more (2 u): 16 u.  fp32 contexts: the coefficients are computed in fp64 and rounded once,
so the gate is 32 u (the derived 16 u and a factor 2 for the second-order terms).  fp64 contexts: the coefficients themselves differ
between two evaluations (sin / cos / sqrt, the cancellation in dtheta_dgw * dgw_dqwr), which has no derivation; it is measured on the
CPU as the largest disagreement between the C oracle and `apply` over the GPU cases (two independent fp64 evaluations) and the gate is
max(32 u, 8 x that): F64_BASIS_U below, recorded from tests/test_map_congruence_ref.py::test_fp64_gate_basis, which prints the figure
and fails if it ever measures more than what is recorded here.
"""
import importlib

import numpy as np

from oracle import np_twin as tw

INVDEPTH, CARTESIAN = 0, 1
U = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
# largest |C oracle - apply| / bound over the fp64 GPU cases, in units of u = 2^-53 (measured on the CPU, rounded up to two digits)
F64_BASIS_U = 5.6
GATE_U = {"f32": 32.0, "f64": max(32.0, 8.0 * F64_BASIS_U)}


def gate(dtype):
    """Largest admissible |device - apply| / bound of a computed entry."""
    return GATE_U[dtype] * U[dtype]


def offsets(types):
    dims = np.where(np.asarray(types) == INVDEPTH, 6, 3)
    off = 13 + np.concatenate([[0], np.cumsum(dims)[:-1]]).astype(int) if len(dims) else np.zeros(0, int)
    return off, int(13 + dims.sum())


def linearity(types, x, P):
    """inversedepth_2_cartesian.m:41-56 per landmark (-1 for a Cartesian one), the point p and J of :63-65."""
    off, _ = offsets(types)
    N = len(types)
    lin, p_all, J_all = -np.ones(N), np.zeros((N, 3)), np.zeros((N, 3, 6))
    for i in range(N):
        if types[i] != INVDEPTH:
            continue
        o = off[i]
        std_rho = np.sqrt(P[o + 5, o + 5])
        rho, theta, phi = x[o + 5], x[o + 3], x[o + 4]
        std_d = std_rho / rho ** 2
        mi = np.array([np.cos(phi) * np.sin(theta), -np.sin(phi), np.cos(phi) * np.cos(theta)])          # m.m:38-40
        x_c1, x_c2 = x[o:o + 3], x[0:3]
        p = x_c1 + mi / rho                                                                              # inversedepth2cartesian.m
        d_c2p = np.linalg.norm(p - x_c2)
        cos_alpha = ((p - x_c1) @ (p - x_c2)) / (np.linalg.norm(p - x_c1) * d_c2p)
        lin[i] = 4 * std_d * cos_alpha / d_c2p
        dm_dtheta = np.array([np.cos(phi) * np.cos(theta), 0.0, -np.cos(phi) * np.sin(theta)])
        dm_dphi = np.array([-np.sin(phi) * np.sin(theta), -np.cos(phi), -np.sin(phi) * np.cos(theta)])
        J_all[i] = np.hstack([np.eye(3), (dm_dtheta / rho)[:, None], (dm_dphi / rho)[:, None], (-mi / rho ** 2)[:, None]])
        p_all[i] = p
    return lin, p_all, J_all


def new_feature(xv, cam, uvd, std_pxl, rho0):
    """hinv_my_version.m:26-53 and add_a_feature_covariance_inverse_depth.m:29-80: y (6), dy_dxv's quaternion rows (2 x 4), D (6 x 6)."""
    f, Cx, Cy = cam[0], cam[1], cam[2]
    R = tw.q2r(xv[3:7])
    uu, vu = tw.undistort(np.asarray(uvd, float), cam)
    hc = np.array([-(Cx - uu) / f, -(Cy - vu) / f, 1.0])
    Xw, Yw, Zw = R @ hc
    y = np.array([xv[0], xv[1], xv[2], np.arctan2(Xw, Zw), np.arctan2(-Yw, np.sqrt(Xw * Xw + Zw * Zw)), rho0])
    dtheta_dgw = np.array([Zw / (Xw ** 2 + Zw ** 2), 0.0, -Xw / (Xw ** 2 + Zw ** 2)])
    s2, sxz = Xw ** 2 + Yw ** 2 + Zw ** 2, np.sqrt(Xw ** 2 + Zw ** 2)
    dphi_dgw = np.array([(Xw * Yw) / (s2 * sxz), -sxz / s2, (Zw * Yw) / (s2 * sxz)])
    dgw_dqwr = tw.dRq_times_a_by_dq(xv[3:7], hc)
    dq = np.vstack([dtheta_dgw @ dgw_dqwr, dphi_dgw @ dgw_dqwr])
    dgc_dhu = np.array([[1 / f, 0.0], [0.0, 1 / f], [0.0, 0.0]])
    dhu_dhd = np.linalg.inv(tw.jacob_distor(cam, np.asarray(uvd, float)))            # jacob_undistor_fm_my_version.m:38
    dy_dhd = np.zeros((6, 3))
    dy_dhd[3:5, :2] = np.vstack([dtheta_dgw, dphi_dgw]) @ R @ dgc_dhu @ dhu_dhd
    dy_dhd[5, 2] = 1.0
    std_rho = rho0 ** 2 * 0.01                                                      # add_features_inverse_depth.m:41
    Padd = np.diag([std_pxl ** 2, std_pxl ** 2, std_rho ** 2])
    return y, dq, dy_dhd @ Padd @ dy_dhd.T


class RowMap:
    """The row map of one map-management call on the map (types, x, P): deletion of the landmarks del_idx, conversion of every surviving
    inverse-depth landmark whose linearity index is below `threshold` (None: no conversion), then the new features uvd (k x 2), rho.

      src[a]          old row new row a copies, or -1: a computed row
      cols, coef      (n_new, 6): the (old column, coefficient) pairs of every row (a copy: (src[a], 1) and zeros)
      x_new, types_new, lm_src (old index of each new landmark, -1: a new one)
      D               list of (offset, 6 x 6) additive blocks, one per new feature
      lin, conv, rel_dist   linearity index per old landmark, the flag set (a deleted landmark reads 0), |lin - threshold| / threshold
    """

    def __init__(self, types, x, P, del_idx=(), threshold=None, uvd=None, rho=None, cam=None, std_pxl=1.0):
        types = np.asarray(types, np.int32)
        x = np.asarray(x, float)
        N = len(types)
        off, n = offsets(types)
        assert x.shape == (n,) and P.shape == (n, n)
        dele = np.zeros(N, bool)
        dele[list(del_idx)] = True
        self.n_old, self.lin = n, None
        self.conv = np.zeros(N, np.int32)
        self.rel_dist = np.full(N, np.inf)
        if threshold is not None:
            self.lin, p_all, J_all = linearity(types, x, P)
            inv = types == INVDEPTH
            self.conv = (inv & ~dele & (self.lin < threshold)).astype(np.int32)
            self.rel_dist[inv] = np.abs(self.lin[inv] - threshold) / threshold
        src, cols, coef, x_new, types_new, lm_src = list(range(13)), [[i] + [0] * 5 for i in range(13)], [[1.0] + [0.0] * 5 for _ in range(13)], list(x[:13]), [], []
        for i in range(N):
            if dele[i]:
                continue
            o, d = off[i], 6 if types[i] == INVDEPTH else 3
            if self.conv[i]:
                for r in range(3):
                    src.append(-1); cols.append(list(range(o, o + 6))); coef.append(list(J_all[i][r])); x_new.append(p_all[i][r])
                types_new.append(CARTESIAN)
            else:
                for r in range(d):
                    src.append(o + r); cols.append([o + r] + [0] * 5); coef.append([1.0] + [0.0] * 5); x_new.append(x[o + r])
                types_new.append(int(types[i]))
            lm_src.append(i)
        self.D = []
        k = 0 if uvd is None else len(np.asarray(uvd).reshape(-1, 2))
        if k:
            uvd = np.asarray(uvd, float).reshape(-1, 2)
            rho = np.broadcast_to(np.asarray(rho, float), (k,))
            for f in range(k):
                y, dq, Dblk = new_feature(x[:13], cam, uvd[f], std_pxl, rho[f])
                self.D.append((len(src), Dblk))
                for r in range(3):                      # dy_drw = [eye(3); 0]: the camera position's rows, copied (D's rows 0..2 are zero)
                    src.append(r); cols.append([r] + [0] * 5); coef.append([1.0] + [0.0] * 5)
                for r in range(2):
                    src.append(-1); cols.append([3, 4, 5, 6, 0, 0]); coef.append(list(dq[r]) + [0.0, 0.0])
                src.append(-1); cols.append([0] * 6); coef.append([0.0] * 6)          # rho: independent of the state, only D
                x_new += list(y)
                types_new.append(INVDEPTH); lm_src.append(-1)
        self.src = np.array(src, int)
        self.cols, self.coef = np.array(cols, int), np.array(coef, float)
        self.x_new = np.array(x_new, float)
        self.types_new = np.array(types_new, np.int32)
        self.lm_src = np.array(lm_src, int)
        self.n_new = len(src)
        self.computed_rows = np.nonzero(self.src < 0)[0]
        # (a new feature's rows 0..2 are copies of rows 0..2, but its OWN 6 x 6 block still takes D: D's rows / columns 0..2 are exactly
        # zero, so those entries stay bit-exact copies as well)

    @property
    def computed(self):
        c = self.src < 0
        return c[:, None] | c[None, :]

    @property
    def both_copied(self):
        return ~self.computed

    def _congruence(self, P, coef):
        s0 = np.where(self.src >= 0, self.src, 0)
        T = P[s0, :]                                                         # n_new x n_old
        for a in self.computed_rows:
            T[a] = coef[a] @ P[self.cols[a], :]
        out = T[:, s0]
        for b in self.computed_rows:
            out[:, b] = T[:, self.cols[b]] @ coef[b]
        return out

    def apply(self, P):
        """(A P A' + D, bound): both n_new x n_new float64; bound = |A| |P| |A|' + |D| on the computed entries, NaN on the copies."""
        P = np.asarray(P, float)
        out = self._congruence(P, self.coef)
        bound = self._congruence(np.abs(P), np.abs(self.coef))
        for o, Dblk in self.D:
            out[o:o + 6, o:o + 6] += Dblk
            bound[o:o + 6, o:o + 6] += np.abs(Dblk)
        bound[self.both_copied] = np.nan
        return out, bound

    def copied_from(self, P):
        """P[src[a], src[b]] where both are copies (what the result must equal bit for bit), NaN elsewhere."""
        s0 = np.where(self.src >= 0, self.src, 0)
        ref = np.asarray(P, float)[np.ix_(s0, s0)]
        ref[self.computed] = np.nan
        return ref


def worst(P_dev, P_ref, bound, mask):
    """Largest |P_dev - P_ref| / bound over `mask` (an entry with a zero bound must agree exactly) and its index."""
    err = np.abs(P_dev - P_ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    q = np.where(mask, q, 0.0)
    k = np.unravel_index(np.argmax(q), q.shape)
    return float(q[k]), (int(k[0]), int(k[1]))


# ---- the GPU cases' inputs (tests/test_gpu_map_blocks.py, tests/map_blocks_worker.py; their conditions: tests/test_map_congruence_ref.py)
SIZES = {"A": (170, 176), "B": (340, 346), "C": (500, 530)}      # N, max_landmarks: n = 1033 / 2053 / 3013, ld = 1152 / 2176 / 3200, gx = 2 / 3 / 4
THRESHOLD = 0.1
STD_PXL = 1.0
RUN8 = list(range(40, 48))      # eight consecutive landmarks: their converted 3-row blocks start at every residue modulo 8, so two of them
#                                 share a group of 8 rows and one crosses a group boundary, whatever converts in front of them


def straddlers(size):
    """All-inverse-depth landmarks whose six columns straddle a 1024-column boundary: 168 (1021..1026), 339 (2047..2052)."""
    return [168] if size == "A" else [168, 339]


def base_map(size, seed=None):
    synth = importlib.import_module("3pre_amd.synth")
    N = SIZES[size][0]
    x0, P0, _ = synth.make_map(N, {"A": 7101, "B": 7102, "C": 7103}[size] if seed is None else seed)
    return N, x0, P0, np.array(synth.CAM, float)


def make_convertible(P, lms):
    """As tests/test_gpu_map.py does: row and column off + 5 of the chosen (all-inverse-depth map) landmarks scaled by 1e-3."""
    P = P.copy()
    for i in lms:
        o = 13 + 6 * i + 5
        P[o, :] *= 1e-3
        P[:, o] *= 1e-3
    return P


def as_stored(P, dtype):
    """What a context of that element type holds after set_x_p_k_k."""
    return P.astype(np.float32).astype(np.float64) if dtype == "f32" else P


def conversion_named(size):
    N = SIZES[size][0]
    return sorted(set([0, N - 1] + straddlers(size) + RUN8))


def conversion_case(size):
    """Test 3: (N, x0, P0 with the named landmarks made convertible, cam, named)."""
    N, x0, P0, cam = base_map(size)
    named = conversion_named(size)
    return N, x0, make_convertible(P0, named), cam, named


def new_features(k, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(5, 170, k), rng.uniform(5, 140, k)], 1), rng.uniform(0.1, 1.0, k)


def management_case(size):
    """Test 4: one call that deletes (a straddler of column 1024 among them), converts and adds.  Returns
    (N, x0, P0, cam, del_idx, named conversions, uvd, rho)."""
    N, x0, P0, cam = base_map(size)
    dele = sorted(set([3, 100, 168, N - 2]))
    named = sorted(set([0, N - 1] + [s for s in straddlers(size) if s not in dele] + RUN8))
    uvd, rho = new_features(SIZES[size][1] - N + len(dele), 900 + N)          # up to the capacity exactly
    return N, x0, make_convertible(P0, named), cam, dele, named, uvd, rho


def group_properties(rm):
    """(two converted landmarks within one group of 8 new rows, one converted landmark whose 3 new rows cross a group boundary)."""
    starts = [int(a) for a in rm.computed_rows if rm.cols[a][1] == rm.cols[a][0] + 1 and (a == 0 or rm.src[a - 1] >= 0 or rm.cols[a - 1][0] != rm.cols[a][0])]
    starts = [a for a in starts if rm.cols[a][0] >= 13]
    same = any(s // 8 == (s + 2) // 8 == t // 8 == (t + 2) // 8 for s, t in zip(starts, starts[1:]))
    cross = any(s // 8 != (s + 2) // 8 for s in starts)
    return same, cross
