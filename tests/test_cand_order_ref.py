"""CPU: the candidates' weighted order.  The restatement tests/cand_order_ref.py against the line-by-line transliteration of
Weighted_Smpl_wo_replacement.m (weights, first-pick marginal) and against the exact Plackett-Luce probabilities of all 24 orders of four candidates;
permutation and tie rules; pre3_philox.h's key function compiled for the host against the restatement; the two symbols declared and exported."""
import ctypes as C
import importlib
import itertools
import math
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import cand_order_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY_RTOL = 1e-12             # fp64 log1p * exp against numpy's: a few ulp; the project's bound for fp64 device geometry (section 17)
FOUR = np.array([[88.0, 72.0], [110.0, 72.0], [88.0, 95.0], [60.0, 50.0]])
N_SEQ = 24000


@pytest.mark.parametrize("box", [(176, 144), (175, 141)])
def test_weights_are_the_normalised_mvnpdf_weights(box):
    if box == (175, 141):
        # 175 / 2 = 87.5 -> 88 and 141 / 2 = 70.5 -> 71 (half away from zero; Python's round() gives 88 and 70), 141 / 6 = 23.5 -> 24
        assert cr.box_params(box) == ((88.0, 71.0), (29.0, 24.0)) and round(141 / 2) == 70
    else:
        assert cr.box_params(box) == ((88.0, 72.0), (29.0, 24.0))
    assert cr.matlab_round(-2.5) == -3 and cr.matlab_round(2.5) == 3 and cr.matlab_round(0.49) == 0
    rng = np.random.default_rng(3)
    uv = np.stack([rng.uniform(0, box[0], 700), rng.uniform(0, box[1], 700)], 1)
    a, b = cr.weights(uv, box), cr.matlab_weights(uv, box)
    assert np.abs(a / b - 1).max() < 1e-15, np.abs(a / b - 1).max()


def test_four_candidates_have_the_plackett_luce_distribution():
    w = cr.weights(FOUR)
    perms = list(itertools.permutations(range(4)))
    p = np.array([cr.pl_probability(w, pm) for pm in perms])
    assert abs(p.sum() - 1) < 1e-12
    assert N_SEQ * p.min() >= 100, N_SEQ * p.min()              # a condition on the inputs: the rarest order is expected often enough
    seen = {pm: 0 for pm in perms}
    first = np.zeros(4)
    for seq in range(N_SEQ):
        o = tuple(int(v) for v in cr.order(FOUR, 20261017, seq))
        seen[o] += 1
        first[o[0]] += 1
    for pm, pr in zip(perms, p):
        sd = math.sqrt(N_SEQ * pr * (1 - pr))
        assert abs(seen[pm] - N_SEQ * pr) < 5 * sd, (pm, seen[pm], N_SEQ * pr, sd)
    # the first pick's marginal against the transliteration's on an independent tape: each within 5 sd of w, and of each other (the difference of two
    # independent counts has twice the variance)
    rng = np.random.default_rng(99)
    first_m = np.zeros(4)
    for _ in range(N_SEQ):
        first_m[cr.weighted_sample(FOUR, iter(rng.random(4)))[0]] += 1
    sd = np.sqrt(N_SEQ * w * (1 - w))
    assert (np.abs(first - N_SEQ * w) < 5 * sd).all() and (np.abs(first_m - N_SEQ * w) < 5 * sd).all(), (first, first_m, N_SEQ * w)
    assert (np.abs(first - first_m) < 5 * math.sqrt(2) * sd).all(), (first, first_m)


def test_the_transliteration_walks_all_candidates_once():
    rng = np.random.default_rng(5)
    uv = np.stack([rng.uniform(0, 176, 65), rng.uniform(0, 144, 65)], 1)
    o = cr.weighted_sample(uv, iter(rng.random(65)))
    assert sorted(o.tolist()) == list(range(65))
    # inverse CDF: u = 0 takes the first candidate with weight left, u near 1 the last
    assert cr.weighted_sample(FOUR, iter([0.0] * 4)).tolist() == [0, 1, 2, 3]
    assert cr.weighted_sample(FOUR, iter([0.999999] * 4)).tolist() == [3, 2, 1, 0]


@pytest.mark.parametrize("K", [1, 2, 64, 65, 700])
def test_the_order_is_a_permutation(K):
    rng = np.random.default_rng(K)
    uv = np.stack([rng.uniform(0, 176, K), rng.uniform(0, 144, K)], 1)
    k = cr.keys(uv, 7, K)
    assert np.isfinite(k).all() and (k >= 0).all()
    o = cr.order_of_keys(k)
    assert sorted(o.tolist()) == list(range(K)) and (np.diff(k[o]) >= 0).all()
    if K >= 64:
        assert not np.array_equal(o, cr.order(uv, 7, K + 1))


def test_equal_keys_break_by_index_and_extreme_keys_are_legal():
    uv = np.array([[50.0, 60.0], [88.0, 72.0], [50.0, 60.0], [88.0, 72.0], [50.0, 60.0]])
    o = cr.order(uv, 0, 0, uniform=lambda i: 0.5)               # duplicates with one uniform: equal keys
    assert o.tolist() == [1, 3, 0, 2, 4]
    # U = 0 -> key 0 (also where exp(q) overflows: never NaN); a pixel absurdly far away -> +inf; both sort by value, then by index
    far = np.array([[1e6, 72.0], [88.0, 72.0], [1e6, 72.0], [88.0, 72.0]])
    k = cr.keys(far, 0, 0, uniform=lambda i: 0.0 if i >= 2 else 0.5)
    assert k[0] == np.inf and k[2] == 0.0 and k[3] == 0.0 and not np.isnan(k).any()
    assert cr.order_of_keys(k).tolist() == [2, 3, 1, 0]


HOST_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "pre3_philox.h"
// stdin: int32 K, W, H | uint64 seed, seq | 2K doubles; stdout: K doubles
int main()
{
    int32_t hdr[3]; uint64_t ss[2];
    if (fread(hdr, 4, 3, stdin) != 3 || fread(ss, 8, 2, stdin) != 2) return 2;
    const int K = hdr[0];
    double *uv = (double *)malloc(sizeof(double) * 2 * K), *k = (double *)malloc(sizeof(double) * K);
    if (fread(uv, 8, 2 * (size_t)K, stdin) != 2 * (size_t)K) return 3;
    const pre3::CandBox b = pre3::cand_box(hdr[1], hdr[2]);
    for (int i = 0; i < K; ++i) k[i] = pre3::cand_key(ss[0], ss[1], i, uv[2 * i], uv[2 * i + 1], b);
    return fwrite(k, 8, K, stdout) == (size_t)K ? 0 : 4;
}
"""


def test_the_headers_key_function_built_for_the_host(tmp_path):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src, exe = tmp_path / "cand_key_host.cpp", tmp_path / "cand_key_host"
    src.write_text(HOST_PROGRAM)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "3pre_amd", "csrc"),
                           str(src), "-o", str(exe), "-lm"])
    for box, seed, seq in (((176, 144), 0x9E3779B97F4A7C15, 41), ((175, 141), 3, 1 << 40)):
        K = 700
        rng = np.random.default_rng(11)
        uv = np.stack([rng.uniform(-20, box[0] + 20, K), rng.uniform(-20, box[1] + 20, K)], 1)
        uv[5] = [1e6, 0.0]                                        # +inf
        inp = struct.pack("<3i2Q", K, box[0], box[1], seed, seq) + np.ascontiguousarray(uv).tobytes()
        out = subprocess.run([str(exe)], input=inp, stdout=subprocess.PIPE, check=True).stdout
        k = np.frombuffer(out, np.float64)
        ref = cr.keys(uv, seed, seq, box)
        assert k.shape == (K,) and k[5] == np.inf == ref[5] and not np.isnan(k).any()
        fin = np.isfinite(ref)
        assert np.abs(k[fin] / ref[fin] - 1).max() < KEY_RTOL, np.abs(k[fin] / ref[fin] - 1).max()
        assert cr.min_relative_gap(ref[fin]) >= 1e3 * KEY_RTOL      # a condition on the inputs: no rounding can swap two neighbours
        assert np.array_equal(cr.order_of_keys(k), cr.order_of_keys(ref))


def test_the_symbols_are_declared_and_exported(pre3):
    txt = open(os.path.join(ROOT, "include", "pre3.h")).read()
    declared = set(re.findall(r"PRE3_API\s+[\w\s\*]+?\b(pre3_\w+)\s*\(", txt))
    lib = C.CDLL(pre3.LIB_PATH)
    for name in ("pre3_candidate_order", "pre3_map_policy_seeded"):
        assert name in declared, "include/pre3.h does not declare %s" % name
        assert hasattr(lib, name), "libpre3.so does not export %s" % name
    assert hasattr(pre3.EkfFilter, "map_management_policy_seeded") and hasattr(importlib.import_module("3pre_amd.synth"), "candidate_order")
