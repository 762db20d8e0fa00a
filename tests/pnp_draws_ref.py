"""The EPnP RANSAC's seeded draw table restated in Python integers (DESIGN.md sections 18 and 35), in tests/draws_ref.py's style and over its Philox
block: six distinct of n for hypothesis h -- ranks in [0, n), [0, n-1), ..., [0, n-5), each later one shifted past the earlier picks in ascending
order (three_distinct's rule continued).  Ranks 0..3 are words 0..3 of block [h, 0, seq, 0], ranks 4 and 5 words 0 and 1 of block [h, 1, seq, 0];
key = [seed, stream 6].  tests/test_gpu_pnp.py compares k_pnp_draw's table with this, integer for integer."""
import numpy as np

from draws_ref import bounded, draw_block

STREAM_PNP = 6


def six_distinct(n, words):
    picks, out = [], []
    for j in range(6):
        r = bounded(words[j], n - j)
        for p in sorted(picks):
            if r >= p:
                r += 1
        picks.append(r)
        out.append(r)
    return out


def draw_pnp(seed, seq, n, n_hyp):
    """(n_hyp, 6) int32"""
    out = np.zeros((n_hyp, 6), np.int32)
    for h in range(n_hyp):
        b0, b1 = draw_block(seed, STREAM_PNP, h, 0, seq), draw_block(seed, STREAM_PNP, h, 1, seq)
        out[h] = six_distinct(n, b0 + b1[:2])
    return out
