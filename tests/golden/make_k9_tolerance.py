"""Writes tests/golden/k9_tolerance.json: the gates of tests/test_gpu_k9_alone.py, measured on the CPU with the plain restatement alone
(tests/k9_ref.py: plain) -- never with the device, and never with the emulation of the bf16 form.

Per committed accuracy input (k9_ref.accuracy_keys(): state size n, rows r, launches, dtype) the file records the maximum and the RMS of
norm_err(plain(...)): the error of the same sums formed in the context's dtype one row of W at a time, in units of
u (|P0|_ij + launches (|W|'|W|)_ij), u = 2^-24 (f32) or 2^-53 (f64), over every entry.  The device's gate is FACTOR x each of the two figures,
and no gate exceeds the worst-case bound r + 8 (gamma_r of an r-term dot product in that dtype, the dropped plane products of the bf16 form,
the final subtraction).

FACTOR = 6, not the 4 the plan proposed.  The reason is the rounding count at the smallest r, not a measurement of the device.  plain rounds once
per row of W and entry (the product; its sum starts from zero) and once in the subtraction.  The bf16 form rounds its f32 accumulator once per
plane product and 16-row stage -- five times at r <= 16 (six products, the first lands in a zero accumulator) -- drops b'c + c'b + c'c
(2 * 2^-9 * 2^-17 |w||w| = 0.25 u) and rounds the same subtraction.  With s = |P - W'W| / |W|'|W| (about 0.5 for these inputs) the ratio of the
two worst cases is (5 + 0.25 + s) / (1 + s) = 3.8 at r = 1: a factor of 4 is the worst-case ratio itself and leaves nothing for comparing two
measured maxima over n^2 entries (plain reaches 0.40 of its 0.6 worst case at r = 1, a sum of six errors need not stop at the same fraction).
6 = 4 x 1.5 keeps that headroom and still puts every mutant at r <= 64 beyond twice the gate (asserted in tests/test_k9_ref.py).  From r = 16 on
the ratio falls below 1 (six roundings per 16 rows against 16), so the small r decide the factor; it is not a property of the inputs and one
factor serves every case and both dtypes.

The generator also redoes the figures of the plan's table: the emulation of the bf16 form and its three mutants (a dropped (0,2) product, a
dropped (1,1), both third-plane products dropped) against the gate, for the f32 inputs -- printed, and asserted in tests/test_k9_ref.py.

    python tests/golden/make_k9_tolerance.py          (rewrites the file; tests/test_k9_ref.py checks that it is reproduced)"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import k9_ref as R  # noqa: E402

FACTOR = 6


def cap_of(r):
    return float(r + 8)


def measure(keys=None):
    cases = {}
    for key, (n, r, launches, dtype) in sorted((keys or R.accuracy_keys()).items()):
        P0, W = R.accuracy_case(n, r, launches, dtype)
        mx, rms = R.norm_err(R.plain(P0, W, launches, dtype), P0, W, launches, R.U32 if dtype == "f32" else R.U64)
        cases[key] = dict(n=n, r=r, launches=launches, dtype=dtype, plain_max=mx, plain_rms=rms,
                          gate_max=min(FACTOR * mx, cap_of(r)), gate_rms=min(FACTOR * rms, cap_of(r)))
    return dict(factor=FACTOR, cases=cases)


def emulation_table(out, keys=None):
    """{key: {'emulation': (max, rms), mutant name: (max, rms) ...}} for the f32 inputs"""
    tab = {}
    for key, (n, r, launches, dtype) in sorted((keys or R.accuracy_keys()).items()):
        if dtype != "f32":
            continue
        P0, W = R.accuracy_case(n, r, launches, dtype)
        row = {"emulation": R.norm_err(R.emulate_b3(P0, W, launches), P0, W, launches, R.U32)}
        for name, pairs in R.MUTANTS.items():
            row[name] = R.norm_err(R.emulate_b3(P0, W, launches, pairs), P0, W, launches, R.U32)
        tab[key] = row
    return tab


if __name__ == "__main__":
    out = measure()
    with open(os.path.join(HERE, "k9_tolerance.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("%-22s %14s %14s %14s   mutants (max / RMS, smallest over the three)" % ("case", "plain", "gate", "emulation"))
    for key, row in emulation_table(out).items():
        g = out["cases"][key]
        mm = min(v[0] for k, v in row.items() if k != "emulation"), min(v[1] for k, v in row.items() if k != "emulation")
        print("%-22s %6.2f / %5.2f %6.2f / %5.2f %6.2f / %5.2f   %8.1f / %6.2f" % (key, g["plain_max"], g["plain_rms"], g["gate_max"], g["gate_rms"],
                                                                                row["emulation"][0], row["emulation"][1], mm[0], mm[1]))
