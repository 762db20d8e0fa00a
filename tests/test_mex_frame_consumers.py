"""CPU: the MEX source of the frame consumers -- pre3_mex('plane_frame' / 'heading_frame' / 'set_scan_frame') in
mex/ekf_ctx_gateway.c.  As tests/test_mex_syntax.py: the gateway goes through the compiler's front end against the declarations-only mex.h and the real
include/pre3.h, so a wrong argument count or type against the new C entry points fails here; and each command is there and calls its entry point."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "mex", "ekf_ctx_gateway.c")
COMMANDS = {"plane_frame": "pre3_plane_fit_frame_seeded", "heading_frame": "pre3_heading_from_frame_seeded", "set_scan_frame": "pre3_set_scan_frame"}


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_the_gateway_with_the_frame_commands_passes_the_compiler_front_end():
    r = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror=implicit-function-declaration", "-Werror=incompatible-pointer-types",
                        "-Werror=int-conversion", "-I", os.path.join(ROOT, "tests", "mex_api_decl"), "-I", os.path.join(ROOT, "include"), SRC],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]


@pytest.mark.parametrize("cmd", sorted(COMMANDS))
def test_each_command_is_dispatched_to_its_entry_point(cmd):
    txt = open(SRC).read()
    m = re.search(r'strcmp\(cmd, "%s"\)\) \{(.*?)\n    \}' % cmd, txt, re.S)
    assert m, "pre3_mex('%s') is not dispatched" % cmd
    assert COMMANDS[cmd] + "(" in m.group(1) and "g_sr" in m.group(1)
    assert "pre3_mex('%s'" % cmd in txt[:txt.index("#include")]            # and listed in the table of the file's header comment
