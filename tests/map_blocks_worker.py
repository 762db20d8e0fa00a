"""Worker of tests/test_gpu_map_blocks.py::test_two_pass_form_is_bit_identical, and the home of the helpers both share.

Run as a program it goes through the call sequences of the deletion, conversion and one-call tests at sizes A and B in fp32, in the form of the
congruence the environment selects (PRE3_MAP_ONE_PASS is read once per process: unset or 1 = k_map_one, 0 = k_map_rows + k_map_cols), and prints
one `DIGEST <label> <sha256 of x and P>` line per resulting state.  The test compares the lines of two runs."""
import hashlib
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import map_congruence_ref as mc  # noqa: E402


def make_filter(pre3, size, dtype, x, P):
    synth = importlib.import_module("3pre_amd.synth")
    N, cap = mc.SIZES[size]
    f = pre3.EkfFilter(np.array(synth.CAM, float), np.zeros(N, np.int32), dtype=dtype, max_hyp=8, max_landmarks=cap)
    f.set_x_p_k_k(x, P)
    return f


def install(f, types, x, P):
    """Put a map and its state back (P holds values the element type represents exactly: the bits return as they were)."""
    _lib = importlib.import_module("3pre_amd._lib")
    types = np.ascontiguousarray(types, np.int32)
    _lib.check(_lib.lib.pre3_set_map(f._ctx, len(types), _lib.dptr(types)))
    f._refresh_map()
    f.set_x_p_k_k(x, P)


def mixed_input(size, P0):
    """P0 with some landmarks made convertible (threshold MIXED_THRESHOLD converts exactly those).  Size B: every third one and the straddler of
    column 1024.  Size A: two only -- every conversion takes 3 of the 1033 columns, and a third one would leave the state inside one block."""
    N = mc.SIZES[size][0]
    return mc.make_convertible(P0, [1, 100] if size == "A" else list(range(1, N, 3)) + mc.straddlers(size)[:1])


MIXED_THRESHOLD = 1e-3


def deletion_lists(size, types):
    N = len(types)
    rng = np.random.default_rng(N)
    lists = [[0], [N - 1], [57, 58]] + [[s] for s in mc.straddlers(size)]
    if (types == 1).any():
        # a Cartesian landmark in front of column 1024: everything behind it moves up by 3 (odd alignment of the vector load's source)
        off = mc.offsets(types)[0]
        cart = [i for i in range(N) if types[i] == 1 and off[i] < 1024]
        assert len(cart) >= 2 and mc.offsets(types)[1] >= 1024 + 3          # (sources behind column 1024 exist)
        lists.append([cart[-1]])
        lists.append([cart[0], cart[-1]] if len(cart) == 2 else [cart[0], cart[len(cart) // 2]])
    lists.append(sorted(rng.choice(N, N // 3, replace=False).tolist()))      # short source runs: vector and one-by-one accesses in every block
    lists.append(list(range(N)))                                               # everything: pose only
    return lists


def main():
    pre3 = importlib.import_module("3pre_amd")

    def digest(label, f):
        x, P = f._get(0)
        print("DIGEST %s %s" % (label, hashlib.sha256(x.tobytes() + P.tobytes() + f.lm_type.tobytes()).hexdigest()), flush=True)

    for size in ("A", "B"):
        N, x0, P0, cam = mc.base_map(size)
        for mixed in (False, True):
            f = make_filter(pre3, size, "f32", x0, mixed_input(size, P0) if mixed else P0)
            if mixed:
                f.inversedepth_2_cartesian(MIXED_THRESHOLD)
                digest("%s-mixed-map" % size, f)
            types = f.lm_type.copy()
            x_old, P_old = f._get(0)
            for k, dele in enumerate(deletion_lists(size, types)):
                f.delete_features(dele)
                digest("%s-%s-delete-%d" % (size, "mixed" if mixed else "id", k), f)
                install(f, types, x_old, P_old)
            f.close()
        N, x0, P0, cam, named = mc.conversion_case(size)
        f = make_filter(pre3, size, "f32", x0, P0)
        f.inversedepth_2_cartesian(mc.THRESHOLD)
        digest("%s-convert" % size, f)
        f.close()
        N, x0, P0, cam, dele, named, uvd, rho = mc.management_case(size)
        for thr in (mc.THRESHOLD, None):
            f = make_filter(pre3, size, "f32", x0, P0)
            f.map_management(dele, uvd, mc.STD_PXL, rho, linearity_index_threshold=thr)
            digest("%s-management-%s" % (size, "convert" if thr else "plain"), f)
            f.close()


if __name__ == "__main__":
    main()
