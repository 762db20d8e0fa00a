"""GPU: map management's one-pass congruence (k_map_one, 3pre_amd/csrc/pre3_map.hip) beyond one 1024-column block, entry by entry.

Sizes (ld = round_up(13 + 6 max_landmarks, 128), a workgroup writes 8 rows x 1024 columns, gx = ceil(ld / 1024) column blocks):
  A  N = 170, n = 1033, ld = 1152, gx = 2: landmark 168 occupies columns 1021..1026 and straddles column 1024
  B  N = 340, n = 2053, ld = 2176, gx = 3: the per-row path has all four k in block 1 and a partial block 2; landmark 339 straddles 2048
  C  N = 500, n = 3013, ld = 3200, gx = 4: the headline shape (fp32 only)
The reference is tests/map_congruence_ref.py (checked on the CPU by tests/test_map_congruence_ref.py, which also asserts the input
conditions of every case here), always started from x, P = f._get(0) read back from the device immediately before the call: an entry
whose row and column are copies must equal its source BIT FOR BIT, a computed entry must lie within the gate in units of
bound = |A| |P| |A|' + |D| (derivation: map_congruence_ref's docstring):
  fp32: 32 u, u = 2^-24 (derived 16 u, factor 2 for second-order terms).  Largest observed on an MI355X: 3.78 u (map_management at C).
  fp64: max(32 u, 8 x basis), u = 2^-53; basis = the largest disagreement between the C oracle and the reference over these cases,
        measured on the CPU (test_map_congruence_ref.py::test_fp64_gate_basis): 5.52 u at the conversion of size B, recorded as 5.6 u,
        so the gate is 44.8 u.  Largest observed on an MI355X: 5.00 u (conversion and map_management at A), addition 3.79 u.
        (With fma contraction in k_map_new_features the addition of 6 features was at 218.51 u at B and 35.83 u at A: test_addition's docstring.)
The two-pass form (PRE3_MAP_ONE_PASS=0, read once per process) runs in a child process: tests/map_blocks_worker.py.
"""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import map_blocks_worker as wk
import map_congruence_ref as mc

pytestmark = pytest.mark.gpu
synth = importlib.import_module("3pre_amd.synth")

AB = [("A", "f64"), ("A", "f32"), ("B", "f64"), ("B", "f32")]
OBSERVED = {"f32": 0.0, "f64": 0.0}            # largest computed-entry error of this run, in units of bound * u (printed by the last test)


def _filter(pre3, size, dtype, x, P):
    return wk.make_filter(pre3, size, dtype, x, P)


def _check_against(f, rm, P_old, dtype, what, late):
    """x, P, the landmark table of the context after a call against the row map rm applied to the read-back P_old.  A computed entry outside the
    gate goes to the list `late`, which the test asserts empty at its end (so that one run shows every figure); everything else fails at once."""
    x, P = f._get(0)
    assert f.n == rm.n_new and f.N == len(rm.types_new) and np.array_equal(f.lm_type, rm.types_new), what
    assert np.abs(x - rm.x_new).max() < 1e-13, what
    cpx = rm.src >= 0
    assert np.array_equal(x[cpx], rm.x_new[cpx]), what
    ref, bound = rm.apply(P_old)
    cp = rm.both_copied
    bad = np.argwhere(cp & (P != rm.copied_from(P_old)))
    assert bad.size == 0, "%s: %d copied entries differ from their sources, first at (row, column) %s" % (what, len(bad), bad[:4].tolist())
    w, at = mc.worst(P, ref, bound, rm.computed)
    print("%s %s: largest computed-entry error %.2f u of bound at %s (gate %.0f u)" % (what, dtype, w / mc.U[dtype], at, mc.GATE_U[dtype]))
    OBSERVED[dtype] = max(OBSERVED[dtype], w / mc.U[dtype])
    if not w <= mc.gate(dtype):
        late.append("%s %s: entry %s is %.2f u of its bound from the reference (gate %.1f u)" % (what, dtype, at, w / mc.U[dtype], mc.GATE_U[dtype]))
    ws, at = mc.worst(P, P.T, bound, rm.computed)
    if not ws <= mc.gate(dtype):
        late.append("%s %s: P is not symmetric at %s (%.2f u of bound, gate %.1f u)" % (what, dtype, at, ws / mc.U[dtype], mc.GATE_U[dtype]))
    return x, P


@pytest.mark.parametrize("mixed", [False, True], ids=["inverse_depth", "mixed"])
@pytest.mark.parametrize("size,dtype", AB)
def test_deletion_is_an_exact_selection(pre3, size, dtype, mixed):
    N, x0, P0, cam = mc.base_map(size)
    if mixed:
        P0 = wk.mixed_input(size, P0)
    f = _filter(pre3, size, dtype, x0, P0)
    try:
        if mixed:                                                              # the mixed map is made on the device
            conv = f.inversedepth_2_cartesian(wk.MIXED_THRESHOLD)
            assert 0 < conv.sum() < N and (f.lm_type == 1).sum() == conv.sum()
        types = f.lm_type.copy()
        x_old, P_old = f._get(0)
        off = mc.offsets(types)[0]
        for dele in wk.deletion_lists(size, types):
            keep = np.r_[np.arange(13), [off[i] + c for i in range(N) if i not in set(dele) for c in range(6 if types[i] == 0 else 3)]].astype(int)
            f.delete_features(dele)
            x, P = f._get(0)
            what = "%s %s delete %s" % (size, dtype, dele if len(dele) < 4 else "%d landmarks" % len(dele))
            assert f.N == N - len(dele) and f.n == len(keep), what
            assert np.array_equal(f.lm_type, np.delete(types, dele)), what
            assert np.array_equal(x, x_old[keep]), what
            bad = np.argwhere(P != P_old[np.ix_(keep, keep)])
            assert bad.size == 0, "%s: %d entries differ, first at (row, column) %s" % (what, len(bad), bad[:4].tolist())
            wk.install(f, types, x_old, P_old)
    finally:
        f.close()


@pytest.mark.parametrize("size,dtype", AB)
def test_addition(pre3, size, dtype):
    """What this test found: with k_map_new_features compiled with fma contraction, `B add 6` in fp64 was 218.51 u of bound at entry (389, 2087)
    against the gate of 44.8 u (A: 35.83 u at (308, 1067)), everything else below 4 u.  Column 2087 is row phi of new feature 5.  The synthetic
    map starts at q = (1, 0, 0, 0), where d(phi)/dq0 is exactly zero: that coefficient is the residue of three cancelling O(1) products, and the
    contracted sum left another residue (2.7e-16 away, at both sizes) than the reference's plain products and sums.  bound weighs the coefficient
    with its own magnitude, so the row where |P[3, c]| is largest against |P[4..6, c]| (c = 389 at B, 308 at A: exactly the arg max of
    |P[3, c]| / bound) read one ulp of the cancelled terms as 218 u.  Compiled on the host, the kernel's text without contraction gives the
    reference's coefficients bit for bit; the kernel now carries `#pragma clang fp contract(off)`, and the figure is 3.79 u."""
    N, x0, P0, cam = mc.base_map(size)
    cap = mc.SIZES[size][1]
    types = np.zeros(N, np.int32)
    f = _filter(pre3, size, dtype, x0, P0)
    late = []
    try:
        x_old, P_old = f._get(0)
        for k in sorted({1, 6, cap - N}):
            uvd, rho = mc.new_features(k, 300 + k)
            f.add_features_inverse_depth(uvd, mc.STD_PXL, rho)
            rm = mc.RowMap(types, x_old, P_old, uvd=uvd, rho=rho, cam=cam, std_pxl=mc.STD_PXL)
            x, P = _check_against(f, rm, P_old, dtype, "%s add %d" % (size, k), late)
            assert np.array_equal(P[:f.n - 6 * k, :f.n - 6 * k], P_old)       # the old block is copied, not recomputed
            f.delete_features(range(N, N + k))                                 # the round trip restores the state bit for bit
            x, P = f._get(0)
            assert np.array_equal(x, x_old) and np.array_equal(P, P_old)
        with pytest.raises(pre3.Pre3Error):                                    # beyond the capacity: an error, nothing changes
            f.add_features_inverse_depth(*((np.tile(mc.new_features(1, 1)[0], (cap - N + 1, 1)), mc.STD_PXL, 0.5)))
        assert f.N == N
        # shrink n by more than one 128-tile, then add: the new rows read the region behind the shrunken state only if it was left stale
        dele = list(range(20, N, 6))[:25] + ([] if size == "A" else [339])
        f.delete_features(dele)
        x1, P1 = f._get(0)
        t1 = f.lm_type.copy()
        assert len(x_old) - len(x1) > 128
        uvd, rho = mc.new_features(6, 77)
        f.add_features_inverse_depth(uvd, mc.STD_PXL, rho)
        rm = mc.RowMap(t1, x1, P1, uvd=uvd, rho=rho, cam=cam, std_pxl=mc.STD_PXL)
        _check_against(f, rm, P1, dtype, "%s delete %d then add 6" % (size, len(dele)), late)
    finally:
        f.close()
    assert not late, "\n".join(late)


@pytest.mark.parametrize("size,dtype", AB)
def test_conversion(pre3, size, dtype):
    N, x0, P0, cam, named = mc.conversion_case(size)
    types = np.zeros(N, np.int32)
    f = _filter(pre3, size, dtype, x0, P0)
    late = []
    try:
        x_old, P_old = f._get(0)
        rm = mc.RowMap(types, x_old, P_old, threshold=mc.THRESHOLD)
        assert rm.rel_dist.min() > 1e-6 and rm.conv[named].all() and 0 < rm.conv.sum() < N      # (the conditions of the CPU test, on the read-back P)
        assert mc.group_properties(rm) == (True, True)
        conv = f.inversedepth_2_cartesian(mc.THRESHOLD)
        assert np.array_equal(conv, rm.conv)
        x, P = _check_against(f, rm, P_old, dtype, "%s convert %d" % (size, conv.sum()), late)
        again = f.inversedepth_2_cartesian(mc.THRESHOLD)                       # nothing is left below the threshold: no bit changes
        x2, P2 = f._get(0)
        assert again.sum() == 0 and np.array_equal(x2, x) and np.array_equal(P2, P) and np.array_equal(f.lm_type, rm.types_new)
    finally:
        f.close()
    assert not late, "\n".join(late)


def _management(pre3, size, dtype, riders=False):
    """The one call of test 4 on a fresh context: returns (f, rm, P_old, x, P, extras, late); the caller closes f and asserts `late` empty."""
    N, x0, P0, cam, dele, named, uvd, rho = mc.management_case(size)
    types = np.zeros(N, np.int32)
    f = _filter(pre3, size, dtype, x0, P0)
    try:
        extras = None
        if riders:
            rng = np.random.default_rng(N)
            desc = rng.integers(0, 256, (N, 128)).astype(np.float64)
            book = rng.integers(0, 50, (N, 4)).astype(np.int32)
            f.set_descriptors(desc)
            f.set_book(book)
            f.predict_camera_measurements(which=0)
            assert f.landmark_fields()["has_h"].any()
            extras = (desc, book)
        x_old, P_old = f._get(0)
        rm = mc.RowMap(types, x_old, P_old, del_idx=dele, threshold=mc.THRESHOLD, uvd=uvd, rho=rho, cam=cam, std_pxl=mc.STD_PXL)
        assert rm.rel_dist.min() > 1e-6 and rm.conv[named].all() and rm.conv[dele].sum() == 0
        conv = f.map_management(dele, uvd, mc.STD_PXL, rho, linearity_index_threshold=mc.THRESHOLD)
        assert np.array_equal(conv, rm.conv)
        late = []
        x, P = _check_against(f, rm, P_old, dtype, "%s map_management" % size, late)
        return f, rm, P_old, x, P, extras, late
    except BaseException:
        f.close()
        raise


@pytest.mark.parametrize("size,dtype", [("A", "f32"), ("B", "f64"), ("C", "f32")])
def test_map_management_in_one_call(pre3, size, dtype):
    f, rm, P_old, x, P, _, late = _management(pre3, size, dtype)
    f.close()
    # nothing converts: bit-identical to delete_features then add_features_inverse_depth on a second context (one fp32 context at a time)
    N, x0, P0, cam, dele, named, uvd, rho = mc.management_case(size)
    res = []
    for one_call in (True, False):
        f = _filter(pre3, size, dtype, x0, P0)
        try:
            if one_call:
                assert f.map_management(dele, uvd, mc.STD_PXL, rho).sum() == 0
            else:
                f.delete_features(dele)
                f.add_features_inverse_depth(uvd, mc.STD_PXL, rho)
            res.append(f._get(0) + (f.lm_type.copy(),))
        finally:
            f.close()
    assert all(np.array_equal(a, b) for a, b in zip(*res))
    assert not late, "\n".join(late)


@pytest.mark.parametrize("size", ["A", "C"])
def test_riders_of_the_one_call(pre3, size):
    f, rm, P_old, x, P, (desc, book), late = _management(pre3, size, "f32", riders=True)
    try:
        old = rm.lm_src >= 0
        want_desc = np.where(old[:, None], desc[np.where(old, rm.lm_src, 0)], 0.0)
        want_book = np.where(old[:, None], book[np.where(old, rm.lm_src, 0)], np.array([0, 0, 0, 0], np.int32))     # {0, 0, s, s}, s = 0: no policy call yet
        assert (~old).sum() > 0 and old.sum() < len(desc)
        assert np.array_equal(f.get_descriptors().T, want_desc)
        assert np.array_equal(f.book(), want_book)
        assert not f.landmark_fields()["has_h"].any()
    finally:
        f.close()
    assert not late, "\n".join(late)


def test_step_on_the_relaid_map(pre3, orc):
    """One full step after test 4's call (size A, fp64) against the oracle's step on the reference's state: the tolerances of
    test_gpu_map.py::test_step_after_map_change_matches_oracle."""
    size = "A"
    N, x0, P0, cam, dele, named, uvd, rho = mc.management_case(size)
    f, rm, P_old, x, P, _, late = _management(pre3, size, "f64")
    try:
        seq = synth.make_sequence(N, 1, 8, seed=7101)
        assert np.array_equal(seq["x0"], x0)
        s = seq["steps"][0]
        new_index = {int(old): k for k, old in enumerate(rm.lm_src) if old >= 0}
        sel = [j for j, i in enumerate(s["meas_idx"]) if int(i) in new_index]
        meas = np.array([new_index[int(s["meas_idx"][j])] for j in sel], np.int32)
        z = s["z"][sel]
        hyp = np.stack([np.random.default_rng(9 + k).permutation(len(meas))[:3] for k in range(8)]).astype(np.int32)
        st = f.step(s["u"], meas, z, hyp, threshold=1.0)
        to, off, n = orc.landmark_table(rm.types_new)
        P_ref = rm.apply(P_old)[0]
        ref = orc.step(to, off, cam, rm.x_new, P_ref, s["u"], meas, z, hyp, 1.0)
        li, hi = f.get_flags()
        assert np.array_equal(li, ref["li"]) and np.array_equal(hi, ref["hi"]) and st["n_li"] == int(ref["li"].sum())
        assert np.abs(f.get_x_k_k() - ref["x_kk"]).max() < 1e-10
        assert np.abs(f.get_p_k_k() - ref["P_kk"]).max() < 1e-10 * np.abs(P_ref).max()
    finally:
        f.close()
    assert not late, "\n".join(late)


def _worker(env_value):
    env = dict(os.environ)
    env.pop("PRE3_MAP_ONE_PASS", None)
    if env_value is not None:
        env["PRE3_MAP_ONE_PASS"] = env_value
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "map_blocks_worker.py")
    r = subprocess.run([sys.executable, worker], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("DIGEST ")]
    assert len(lines) > 10, r.stdout
    return lines


def test_two_pass_form_is_bit_identical():
    """docs/DESIGN_rounds1-4.md: the one-pass congruence reproduces the two-pass form (k_map_rows, k_map_cols, k_map_add_noise, k_map_finish)
    bit for bit; here at sizes A and B in fp32, over the call sequences of the deletion, conversion and one-call tests."""
    one, two = _worker(None), _worker("0")
    assert [ln.split()[1] for ln in one] == [ln.split()[1] for ln in two]
    diff = [(a, b) for a, b in zip(one, two) if a != b]
    assert not diff, "the two forms differ at: %s" % [a.split()[1] for a, b in diff]


def test_report_largest_observed_error():
    """Not a check of its own (the tests above assert the gates): prints this run's largest figure per element type, for the record."""
    for dtype in ("f32", "f64"):
        print("largest computed-entry error observed, %s: %.2f u of bound (gate %.1f u)" % (dtype, OBSERVED[dtype], mc.GATE_U[dtype]))
