"""K9 -- the symmetric rank-r down-date P <- P - W'W the project is graded on -- on its own, entry by entry, in all seven of its forms.

Every other parity check of K9 goes through a whole update or step and holds P to 3e-4 max|P| against the fp64 twin; a form that drops a
plane product, skips a k-stage or mis-mirrors a block passes that wherever max|P| is set elsewhere in the matrix.  Here the test hook
EkfFilter.test_downdate hands a W of the test's own to launch_downdate and nothing else runs.  Per case (tests/k9_ref.py):

  * P is finite and bitwise symmetric;
  * exact class (integer W and P0, everything below 2^24): P equals P0 - launches W'W bit for bit, in either dtype;
  * accuracy class: |P - exact|_ij / (u (|P0|_ij + launches (|W|'|W|)_ij)) is inside the gate of tests/golden/k9_tolerance.json on its
    maximum and on its RMS over every entry -- FACTOR x the plain restatement's own figures, u = 2^-24 or 2^-53 by the context's dtype.

Shapes: n on either side of a 64- and a 128-column edge, ld tight and loose, r on either side of every change of the bf16 form's stage
count (nst = 4 .. 12), one and three launches on one context (plane reuse, the persistent form's ticket counter).  r = 129 needs a row
capacity of 192, which the contexts of 8 .. 20 landmarks do not have (the hook refuses it): it runs on (41, 41) and (20, 60).

Measured on an MI355X (256 CUs), worst case over all cases of a form, max / RMS in u, next to plain's: see profiles/k9_alone_accuracy.txt.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import k9_ref as R
import k9_worker as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESULTS = []                # (form, result) of every case that ran, for the report


@pytest.fixture(autouse=True)
def _test_hooks_on(monkeypatch):
    """the hook is inert unless the environment enables it (3pre_amd/csrc/pre3_test_hooks.h)"""
    monkeypatch.setenv("PRE3_TEST_HOOKS", "1")


@pytest.fixture(scope="module", autouse=True)
def _report():
    """K9_ALONE_REPORT=<file>: the measured figures of every accuracy case, next to plain's (profiles/k9_alone_accuracy.txt is one)"""
    yield
    path = os.environ.get("K9_ALONE_REPORT")
    if path and RESULTS:
        with open(path, "w") as fh:
            fh.write("# K9 alone: normalised error |P - exact|_ij / (u (|P0|_ij + launches (|W|'|W|)_ij)), u = 2^-24 (f32) / 2^-53 (f64), max and RMS over all entries\n")
            fh.write("# %-42s %5s %4s %3s %4s   %9s %9s   %9s %9s   %9s %9s\n" % ("form", "n", "r", "L", "type", "dev max", "dev rms", "plain max", "plain rms", "gate max", "gate rms"))
            g = K.gates()
            for form, res in RESULTS:
                c = res["case"]
                if c["cls"] == "acc" and res["fig"]:
                    q = g[R.key_of(c)]
                    fh.write("  %-42s %5d %4d %3d %4s   %9.3f %9.3f   %9.3f %9.3f   %9.3f %9.3f\n" % (form, c["n"], c["r"], c["launches"], c["dtype"], res["fig"]["max"], res["fig"]["rms"],
                                                                                               q["plain_max"], q["plain_rms"], q["gate_max"], q["gate_rms"]))
            n_exact = sum(1 for _, r in RESULTS if r["case"]["cls"] == "exact")
            fh.write("# exact class: %d cases, %d bit-equal to P0 - launches W'W\n" % (n_exact, sum(1 for _, r in RESULTS if r["case"]["cls"] == "exact" and not r["bad"])))


def _num_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _check(form, results, n_min):
    for res in results:
        print(form, K.describe(res))
        RESULTS.append((form, res))
    assert len(results) >= n_min, "only %d cases ran" % len(results)
    assert {r["case"]["cls"] for r in results} == {"exact", "acc"}
    bad = [K.describe(r) for r in results if r["bad"]]
    assert not bad, "%d of %d cases:\n" % (len(bad), len(results)) + "\n".join(bad)


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "N%d_cap%d" % s)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_the_default_forms(pre3, dtype, shape):
    """fp32: k_split_w + k_downdate_b3 on 128 x 128 tiles; fp64: k_downdate_1t<double,32,8> (at most 2 x #CUs tiles of 64 x 64)"""
    assert dtype == "f32" or R.tiles64(shape[1]) <= 2 * _num_cus()
    assert dtype == "f64" or R.tiles128(shape[1], _num_cus())[1] == 0
    _check("k_downdate_b3<128>" if dtype == "f32" else "k_downdate_1t<double,32,8>", K.run_group(pre3, "default", dtype, (shape,)), 20)


def test_the_left_over_tiles_of_the_bf16_form(pre3):
    """ld = 2944: 276 tiles of 128 x 128 on 256 CUs -> one round of 256 and 20 split into 64 x 64 tiles (b3_tile<64>), diagonal ones first"""
    cus = _num_cus()
    n_big, n_small = R.tiles128(R.SMALL_TILES[1], cus)
    if n_small == 0:
        pytest.skip("%d CUs: the 128 x 128 tiles of ld = %d fill whole rounds, no 64 x 64 left-overs" % (cus, R.ld_of(R.SMALL_TILES[1])))
    assert n_big > 0 and n_big % cus == 0
    _check("k_downdate_b3<128> + b3_tile<64>", K.run_group(pre3, "small_tiles", "f32"), 5)


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "N%d_cap%d" % s)
def test_the_f32_mfma_one_tile_form(pre3, shape):
    """PRE3_OPT_K9_BF16X3 off: k_downdate_1t<float,32>"""
    assert R.tiles64(shape[1]) <= 5 * _num_cus()
    _check("k_downdate_1t<float,32>", K.run_group(pre3, "f32_1t", "f32", (shape,)), 8)


def test_the_fp64_one_tile_form_with_16_row_stages(pre3):
    """ld = 2176: 595 tiles of 64 x 64, above 2 x #CUs and up to 5 x #CUs -> k_downdate_1t<double,16>"""
    cus, t = _num_cus(), R.tiles64(R.ONE_TILE_16[1])
    if not 2 * cus < t <= 5 * cus:
        pytest.skip("%d CUs: %d tiles do not select k_downdate_1t<double,16>" % (cus, t))
    _check("k_downdate_1t<double,16>", K.run_group(pre3, "f64_1t16", "f64"), 5)


@pytest.mark.parametrize("group,form", [("persist", "2"), ("forced_1t", "1")])
def test_the_forced_forms(group, form):
    """PRE3_K9_FORM is read once per process: a child per value.  2: the persistent k_downdate<float,32> / <double,32> (ticket counter, one and three
    launches on one context); 1: the one-tile forms forced"""
    env = dict(os.environ, PRE3_K9_FORM=form, PRE3_TEST_HOOKS="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "k9_worker.py"), group], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("K9JSON ")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0][7:])
    for dt, name in (("f32", "<float,32>"), ("f64", "<double,32>")):
        _check(("k_downdate" if form == "2" else "k_downdate_1t (forced)") + name, [x for x in res if x["case"]["dtype"] == dt], 10 if form == "1" else 20)


def test_the_hook_refuses_what_it_must(pre3, monkeypatch):
    N = 20
    P0, W = R.exact_case(R.state_size(N), 2, 1, 1)
    f = pre3.EkfFilter(K.CAM, np.zeros(N, np.int32), dtype="f32", max_hyp=4)
    f.set_x_p_k_k(R.x0_of(N), P0)
    rcap = R.rcap_of(N)
    nan = W.copy(); nan[1, 7] = np.nan
    inf = W.copy(); inf[0, 0] = np.inf
    for Wbad, launches in ((np.ones((rcap + 1, f.n)), 1), (nan, 1), (inf, 1), (W, 0), (1e300 * np.ones((1, f.n)), 1)):
        with pytest.raises(pre3.Pre3Error) as e:
            f.test_downdate(Wbad, launches)
        assert e.value.code == -1                                             # PRE3_E_ARG
        assert np.array_equal(f.get_p_k_k(), P0)
    with pytest.raises(ValueError):
        f.test_downdate(np.ones((2, f.n - 1)))
    monkeypatch.delenv("PRE3_TEST_HOOKS", raising=False)
    with pytest.raises(pre3.Pre3Error) as e:
        f.test_downdate(W)
    assert e.value.code == -4                                                 # PRE3_E_STATE: the hooks are off
    assert np.array_equal(f.get_p_k_k(), P0)
    monkeypatch.setenv("PRE3_TEST_HOOKS", "1")
    f.test_downdate(np.repeat(W[:1], rcap, axis=0), 1)                           # the largest r the context admits
    f.set_x_p_k_k(R.x0_of(N), P0)
    f.test_downdate(W, 1)
    assert np.array_equal(f.get_p_k_k(), R.exact(P0, W, 1))
    f.close()
