"""CPU: the ownership types of 3pre_amd/csrc/pre3_own.h -- the grown block, the fixed list, the all-or-nothing group and the
staging ring -- built for the host with -fsanitize=address,undefined (tests/own_host_main.cpp, a stand-alone program with its own main; nothing loaded
into Python is instrumented).  The program defines the header's five seam functions over malloc, counts live blocks, logs every call and fails the
k-th allocation on request; each case checks itself and ends with nothing live, and LeakSanitizer's report at exit is the leak check.

What the cases show is listed at each of them in the program: a reserve within the size touches nothing; a growing one frees first, asks for exactly
the capacity and zeroes once with the stream it was given; a failed one leaves an empty block the next call fills; a moved-from block is empty; a group
of five whose k-th allocation fails (k = 1..5) leaves nothing live, its guard false and every pointer null, and completes on the retry; the ring hands
out slots 0, 1, 0, 1, waits only for released slots and with mailbox slot base + k, grows behind two waits, and survives a failing wait or allocation."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["reserve_within", "reserve_grows", "failed_grow", "move", "group", "ring_alternation", "ring_growth", "ring_failure"]


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("own_host") / "own_host"
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "3pre_amd", "csrc"), os.path.join(ROOT, "tests", "own_host_main.cpp"), "-o", str(exe)])
    return str(exe)


@pytest.mark.parametrize("case", CASES)
def test_own_host(host_exe, case):
    r = subprocess.run([host_exe, case], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    out = r.stdout.decode() + r.stderr.decode()
    assert r.returncode == 0, out
    assert out.strip().split("\n")[-1] == case + " ok", out


def test_the_program_has_no_other_case(host_exe):
    assert subprocess.run([host_exe, "nothing"], stdout=subprocess.PIPE).returncode == 2
