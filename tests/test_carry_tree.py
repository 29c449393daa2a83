"""Pass 1 of the packed sweep builds its strip carries a and b as trees of three-input binary16 maxima in the local classes
compiled for the default scores (smoothxg_amd/csrc/poa_fields.h: p16_carry_leaf_bottom; smoothxg_amd/csrc/poa_dp16_row.inc.h).
tests/csrc/carry_tree_check.cpp restates one strip on the host -- the running form a = pk_max(a + |e|, h) exactly as it was,
and the tree form on packed fields with an integer-only binary16 maximum, clamp leaf and opening included -- and compares both
halves over random and adversarial strips (all fields at the bottom bound, all at the top bound, the winning column at every k,
ties, the clamp leaf winning) at every strip width 4 .. 13; it asserts that every operand of a node is a pattern in
0 .. 0x7BFF and that no half of a leaf subtraction borrows, and holds the constexpr bound against every width of the class
list.  Run as a stand-alone program, plain and under the host's address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "sanitized"])
def test_carry_trees_equal_the_running_form(tmp_path, flags):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "carry_tree_check")
    subprocess.check_call([cxx] + flags + ["-std=c++17", "-Wall", "-o", exe, os.path.join(HERE, "csrc", "carry_tree_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    n, bad = map(int, out.stdout.split())
    # 10 widths x more than 6 000 strips, eight checks each
    assert n > 400000 and bad == 0, out.stderr
