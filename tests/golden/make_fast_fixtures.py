"""Generator of tests/golden/fast_lab_crop.npz.  Run where the reference tree exists:

    python tests/golden/make_fast_fixtures.py <reference>/matlab_code

It parses mex_files/Fast_Cr_Ver1/fast_corner_detect_9.m at run time into a walker (if / elseif / else / continue / end over `>` `<` `||` conditions
on one ring pixel each) -- nothing of the tree is written anywhere -- and records what the tree computes on a 144 x 176 crop of
fast-matlab-src/lab.pgm, on which the tree and the published segment test (tests/fast_ref.py) agree pixel for pixel at thresholds 10, 20 and 30.
It fails when the crop loses that property.  The four exhaustive counts (all 3^16 ternary ring states) are recorded too.
"""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import fast_ref as fr  # noqa: E402

CROP_R0, CROP_C0, CROP_ROWS, CROP_COLS = 83, 498, 144, 176      # rows 84..227, columns 499..674, 1-based
RING_K = {d: k for k, d in enumerate(fr.RING)}


def read_pgm(path):
    raw = open(path, "rb").read()
    tok, pos = [], 0
    while len(tok) < 4:
        m = re.compile(rb"\s*(#[^\n]*\n|\S+)").match(raw, pos)
        pos = m.end()
        if not m.group(1).startswith(b"#"):
            tok.append(m.group(1))
    assert tok[0] == b"P5" and int(tok[3]) == 255
    w, h = int(tok[1]), int(tok[2])
    return np.frombuffer(raw, np.uint8, w * h, pos + 1).reshape(h, w).copy()


# ---- the tree, parsed ----------------------------------------------------------------------------------------------------------------------------
COND = re.compile(r"im\(y\+?(-?\d+),x\+?(-?\d+)\)\s*(>|<)\s*(cb|c_b)")


def parse_cond(text):
    """[(ring pixel, wanted ternary state)]: OR of `pixel > cb` (1: brighter) / `pixel < c_b` (2: darker)"""
    out = []
    for part in text.split("||"):
        m = COND.fullmatch(part.strip())
        assert m, text
        dy, dx, op, ref = int(m.group(1)), int(m.group(2)), m.group(3), m.group(4)
        assert (op, ref) in ((">", "cb"), ("<", "c_b")), text
        out.append((RING_K[(dx, dy)], 1 if op == ">" else 2))
    return out


def parse_tree(path):
    lines = [ln.split("%")[0].strip() for ln in open(path, errors="replace").read().splitlines()]
    start = next(i for i, ln in enumerate(lines) if ln.startswith("c_b=")) + 1
    stop = next(i for i, ln in enumerate(lines) if ln.startswith("nc = nc + 1"))
    body = [ln for ln in lines[start:stop] if ln]
    pos = [0]
    questions = [0]

    def block():
        stmts = []
        while pos[0] < len(body):
            ln = body[pos[0]]
            if ln == "continue;":
                pos[0] += 1
                stmts.append("continue")
            elif ln.startswith("if "):
                branches, other = [], None
                cond = parse_cond(ln[3:])
                pos[0] += 1
                while True:
                    questions[0] += 1
                    branches.append((cond, block()))
                    ln2 = body[pos[0]]
                    pos[0] += 1
                    if ln2.startswith("elseif "):
                        cond = parse_cond(ln2[7:])
                    elif ln2 == "else":
                        other = block()
                        assert body[pos[0]] == "end"
                        pos[0] += 1
                        break
                    else:
                        assert ln2 == "end", ln2
                        break
                stmts.append(("if", branches, other))
            else:
                assert ln in ("end", "else") or ln.startswith("elseif "), ln
                return stmts
        return stmts

    tree = block()
    assert pos[0] == len(body)
    return tree, questions[0]


def walk(stmts, states, idx):
    """the indices of idx that fall through stmts (reach the end without `continue`); states is (16, n) int8 in {0, 1, 2}"""
    for st in stmts:
        if idx.size == 0:
            return idx
        if st == "continue":
            return idx[:0]
        _, branches, other = st
        out, rest = [], idx
        for cond, blk in branches:
            hit = np.zeros(rest.size, bool)
            for k, want in cond:
                hit |= states[k, rest] == want
            out.append(walk(blk, states, rest[hit]))
            rest = rest[~hit]
        out.append(walk(other, states, rest) if other is not None else rest)
        idx = np.concatenate(out)
    return idx


def tree_corner_map(tree, im, threshold):
    ring, c = fr.ring_stack(im)
    states = np.where(ring > c + threshold, 1, np.where(ring < c - threshold, 2, 0)).astype(np.int8).reshape(16, -1)
    hit = np.zeros(states.shape[1], bool)
    hit[walk(tree, states, np.arange(states.shape[1]))] = True
    out = np.zeros(np.asarray(im).shape, bool)
    out[3:-3, 3:-3] = hit.reshape(c.shape)
    return out


def exhaustive(tree):
    """over all 3^16 ring states: (tree, segment test, tree only, segment test only)"""
    n_tree = n_seg = only_tree = only_seg = 0
    chunk = 3 ** 12
    low = np.arange(chunk)
    low_digits = np.stack([(low // 3 ** k) % 3 for k in range(12)]).astype(np.int8)
    w = (np.uint32(1) << np.arange(16, dtype=np.uint32))[:, None]
    for hi in range(81):
        states = np.concatenate([low_digits, np.repeat(np.array([(hi // 3 ** k) % 3 for k in range(4)], np.int8)[:, None], chunk, axis=1)])
        t = np.zeros(chunk, bool)
        t[walk(tree, states, low)] = True
        s = fr.has_run9(((states == 1) * w).sum(axis=0)) | fr.has_run9(((states == 2) * w).sum(axis=0))
        n_tree += int(t.sum()); n_seg += int(s.sum()); only_tree += int((t & ~s).sum()); only_seg += int((s & ~t).sum())
    return n_tree, n_seg, only_tree, only_seg


def nonmax_literal(im, barrier, corners):
    """fast_nonmax.m:61-100 as written, a loop over the corner list"""
    a = np.asarray(im).astype(np.int64)
    scores = np.zeros(a.shape, np.int64)
    for x, y in corners.tolist():
        ring = np.array([a[y - 1 + dy, x - 1 + dx] for dx, dy in fr.RING])
        p1 = ring - (a[y - 1, x - 1] + barrier)
        n1 = a[y - 1, x - 1] - barrier - ring
        scores[y - 1, x - 1] = max(int((p1 * (p1 > 0)).sum()), int((n1 * (n1 > 0)).sum()))
    keep = []
    for x, y in corners.tolist():
        p = scores[y - 1, x - 1]
        if sum(p >= scores[y - 1 + dy, x - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy) == 8:
            keep.append((x, y))
    k = np.array(keep, np.int32).reshape(-1, 2)
    return k, scores[k[:, 1] - 1, k[:, 0] - 1].astype(np.int32)


def adjacent_pairs(c):
    s = {tuple(p) for p in c.tolist()}
    return sum(1 for (x, y) in s for dx, dy in ((1, -1), (1, 0), (1, 1), (0, 1)) if (x + dx, y + dy) in s)


def main(ref_root):
    tree, questions = parse_tree(os.path.join(ref_root, "mex_files", "Fast_Cr_Ver1", "fast_corner_detect_9.m"))
    lab = read_pgm(os.path.join(ref_root, "fast-matlab-src", "lab.pgm"))
    assert lab.shape == (288, 768), lab.shape
    crop = lab[CROP_R0:CROP_R0 + CROP_ROWS, CROP_C0:CROP_C0 + CROP_COLS].copy()
    out = dict(image=crop, tree_questions=np.int64(questions))
    for t, want in ((10, 297), (20, 72), (30, 25)):
        tm = tree_corner_map(tree, crop, t)
        assert np.array_equal(tm, fr.corner_map(crop, t)), "the tree and the segment test differ on the crop at threshold %d" % t
        out["corners_%d" % t] = fr._list(tm)
        assert len(out["corners_%d" % t]) == want, (t, len(out["corners_%d" % t]))
    t5, s5 = tree_corner_map(tree, crop, 5), fr.corner_map(crop, 5)
    print("threshold 5: tree %d, segment test %d, pixels that differ %d (not part of the equality claim)" % (t5.sum(), s5.sum(), (t5 != s5).sum()))
    mx, sc = nonmax_literal(crop, 20, out["corners_10"])
    mx2, sc2 = fr.fast_nonmax(crop, 10, 20)
    assert np.array_equal(mx, mx2) and np.array_equal(sc, sc2)
    assert len(mx) == 96 and int((sc == 0).sum()) == 16 and adjacent_pairs(mx) == 7, (len(mx), int((sc == 0).sum()), adjacent_pairs(mx))
    out["maxima_10_20"], out["maxima_scores_10_20"] = mx, sc
    centres = fr.all_centres(CROP_ROWS, CROP_COLS)
    first = np.zeros((len(centres), 2), np.int32)
    for i, (cr, cc) in enumerate(centres):
        r0, c0 = cr - 31, cc - 21
        box = crop[r0:r0 + 61, c0:c0 + 41]
        tm = tree_corner_map(tree, box, 10)
        m, _ = nonmax_literal(box, 20, fr._list(tm))
        seg = fr.box_first_maximum(crop, (cr, cc))
        if len(m):
            first[i] = (m[0, 0] + c0, m[0, 1] + r0)
        assert (tuple(first[i]) if len(m) else None) == seg, "box %d: the tree's first maximum is not the segment test's" % i
    assert len(centres) == 3948 and int((first[:, 0] > 0).sum()) == 3422, (len(centres), int((first[:, 0] > 0).sum()))
    out["box_centres"], out["box_first"] = np.array(centres, np.int32), first
    ex = exhaustive(tree)
    print("3^16 ring states: tree %d, segment test %d, tree only %d, segment test only %d; %d question nodes" % (ex + (questions,)))
    assert ex == (785268, 46658, 747510, 8900), ex
    out["exhaustive"] = np.array(ex, np.int64)
    # what the issue measured on the whole of lab.pgm, for DESIGN.md
    for t in (5, 10, 20, 30):
        a, b = tree_corner_map(tree, lab, t), fr.corner_map(lab, t)
        print("lab.pgm threshold %d: pixels that disagree %d, corners tree %d / segment test %d" % (t, (a != b).sum(), a.sum(), b.sum()))
    path = os.path.join(HERE, "fast_lab_crop.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main(sys.argv[1])
