"""Pass 2 of the packed sweep keeps no in-strip state of the long gap piece in the classes compiled for the default scores, and
the local ones carry the clamp at the bias in E (smoothxg_amd/csrc/poa_fields.h: p16_strip_q_dominated;
smoothxg_amd/csrc/poa_dp16_row.inc.h).  tests/csrc/strip_gap_check.cpp restates one row on the host -- the recurrence itself,
the strip form with the per-column Q update, the strip form without it -- and compares the three over random and adversarial
rows (steps, spikes, flat runs at 0, a cliff, global rows at the clamp) at every strip width 4 .. 13, local and global, with
the words that cross a wave's edge; it also holds the constexpr condition against every width of the class list.  Run as a
stand-alone program, plain and under the host's address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "sanitized"])
def test_short_pass2_equals_the_recurrence(tmp_path, flags):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "strip_gap_check")
    subprocess.check_call([cxx] + flags + ["-std=c++17", "-Wall", "-o", exe, os.path.join(HERE, "csrc", "strip_gap_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    n, bad = map(int, out.stdout.split())
    # 10 widths x 2 modes x 2 500 rows and more, at least two checks each
    assert n > 100000 and bad == 0, out.stderr
