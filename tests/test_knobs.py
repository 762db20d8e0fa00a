"""CPU: the table of PRE3_* environment switches (3pre_amd/csrc/pre3_knobs.h).  A stand-alone program built with the host compiler prints every
line of the table and what its accessor returns; the parsing rules are checked on it (unset: the default; set: atoi; the three kinds of their own).
Then the table is tied to its two ends: every accessor is called from some .hip file (no dead switch), and every PRE3_* name the tests -- and
bench.py -- put into an environment is a line of the table (a variant test with a misspelt or retired name compares the default with itself)."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "3pre_amd", "csrc")
INT_KINDS = ("once", "call", "create")
# PRE3_* tokens in tests/ that are not environment switches of the library: option / error enumerators of the ABI, the Python mirror's and the
# bench's own variables, the tests' own, and the constants of the frame and SIFT headers
NOT_SWITCHES = re.compile(r"PRE3_(OPT_.*|E_.*|API|LIB|BENCH_.*|TEST_BACKEND|EXPECT_GPU|SR_.*|SIFT_.*)$")

PROGRAM = r"""
#include <stdio.h>
#include "pre3_knobs.h"
static void show(int v) { printf("%d", v); }
static void show(const char *s) { printf("%s", s ? s : "(null)"); }
int main()
{
#define ROW(acc, env, def, kind, meaning) printf("%s\t%s\t%s\t", #acc, env, #kind); show(def); printf("\t"); show(pre3::knob::acc()); printf("\n");
    PRE3_KNOBS(ROW)
    return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler"
    d = tmp_path_factory.mktemp("knobs")
    src, out = d / "knobs.cpp", d / "knobs"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(out)])
    return str(out)


def table(exe, **env):
    """rows (accessor, environment name, kind, default, value) with only `env` of the PRE3_* family set"""
    e = {k: v for k, v in os.environ.items() if not k.startswith("PRE3_")}
    e.update(env)
    out = subprocess.run([exe], env=e, stdout=subprocess.PIPE, check=True, text=True).stdout
    rows = [tuple(line.split("\t")) for line in out.splitlines()]
    assert rows and all(len(r) == 5 for r in rows), out
    return rows


@pytest.fixture(scope="module")
def rows(exe):
    return table(exe)


def test_names_are_unique(rows):
    for col in (0, 1):
        names = [r[col] for r in rows]
        assert len(set(names)) == len(names), sorted(n for n in set(names) if names.count(n) > 1)
    assert all(re.fullmatch(r"PRE3_[A-Z0-9_]+", r[1]) for r in rows)
    assert {r[2] for r in rows} <= set(INT_KINDS) | {"present", "is1", "text"}


def test_clean_environment_gives_the_defaults(rows):
    assert [(r[1], r[4]) for r in rows] == [(r[1], r[3]) for r in rows]


def test_integer_switches_are_atoi_of_the_text(exe, rows):
    ints = [r[1] for r in rows if r[2] in INT_KINDS]
    assert len(ints) >= 42
    for text, want in (("7", "7"), ("", "0")):
        got = table(exe, **{name: text for name in ints})
        assert [(r[1], r[4]) for r in got if r[2] in INT_KINDS] == [(name, want) for name in ints]
        assert [r[4] for r in got if r[2] not in INT_KINDS] == [r[3] for r in got if r[2] not in INT_KINDS]


def test_kinds_of_their_own(exe):
    def value(name, **env):
        return {r[1]: r[4] for r in table(exe, **env)}[name]
    assert value("PRE3_STEP_TRACE") == "0" and value("PRE3_STEP_TRACE", PRE3_STEP_TRACE="0") == "1" and value("PRE3_STEP_TRACE", PRE3_STEP_TRACE="") == "1"
    assert value("PRE3_TEST_HOOKS") == "0" and value("PRE3_TEST_HOOKS", PRE3_TEST_HOOKS="1") == "1" and value("PRE3_TEST_HOOKS", PRE3_TEST_HOOKS="2") == "0"
    assert value("PRE3_RCCL_LIB") == "(null)" and value("PRE3_RCCL_LIB", PRE3_RCCL_LIB="/x/librccl.so") == "/x/librccl.so"


def test_every_accessor_is_called_and_nothing_else_reads_the_environment(rows):
    text = "".join(open(p).read() for p in sorted(glob.glob(os.path.join(CSRC, "*.hip"))))
    dead = [r[0] for r in rows if not re.search(r"\bknob::%s\(\)" % r[0], text)]
    assert dead == [], "switches that nothing reads: %s" % dead
    assert set(re.findall(r"\bknob::(\w+)\(\)", text)) <= {r[0] for r in rows}
    readers = [os.path.basename(p) for p in sorted(glob.glob(os.path.join(CSRC, "*"))) if os.path.isfile(p) and p.endswith((".hip", ".h")) and "getenv" in open(p).read()]
    assert readers == ["pre3_knobs.h"]


def test_names_the_tests_and_the_bench_set_are_table_entries(rows):
    known = {r[1] for r in rows}
    used = {}
    for p in sorted(glob.glob(os.path.join(ROOT, "tests", "*.py"))):
        if os.path.samefile(p, __file__):
            continue
        for name in re.findall(r"PRE3_[A-Z0-9_]+", open(p).read()):
            if not NOT_SWITCHES.match(name):
                used.setdefault(name, os.path.basename(p))
    # the suites that exercise the switches are among the files read (a moved file must not empty this test)
    assert len(used) >= 26 and {"PRE3_HI_FUSED", "PRE3_PEND_HI", "PRE3_MATCH_FLOAT_FORM", "PRE3_IC_FUSED", "PRE3_MAP_ONE_PASS", "PRE3_TEST_HOOKS"} <= set(used)
    unknown = {n: f for n, f in used.items() if n not in known}
    assert unknown == {}, "set by a test, read by nothing: %s" % unknown
    assert '"PRE3_CHOL_FORM"' in open(os.path.join(ROOT, "bench.py")).read() and "PRE3_CHOL_FORM" in known
