"""The stored-row code of the packed sweep's 2-byte classes (smoothxg_amd/csrc/poa_rowcode.h): every representable
(step, H - oF, H - oO) of each score set the tests run on the 2-byte cells decodes back to the cell's H and outgoing gap
candidates, in the biased (local) and the plain (global) arithmetic, convex and not, at the edges of the sweep's ranges."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

# (m, n, g, e, q, c) in the engine's sign convention: smoothxg's default, the affine and linear sets of the parity tests,
# and pggb's asm10 set (16 bits: the widest that takes the 2-byte cells)
SCORES = [(1, -4, -6, -2, -26, -1), (1, -4, -8, -2, -8, -2), (1, -4, -6, -2, -8, -2), (1, -4, -6, -2, -6, -2),
          (2, -3, -5, -5, -9, -1), (2, -3, -5, -5, -5, -5), (1, -10, -2, -2, -2, -2), (1, -9, -16, -2, -41, -1)]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("rowcode") / "rowcode_check")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "csrc", "rowcode_check.cpp")])
    return exe


@pytest.mark.parametrize("scores", SCORES)
def test_row_code_round_trips_every_cell(checker, scores):
    out = subprocess.run([checker] + [str(v) for v in scores], capture_output=True, text=True, check=True)
    n, bad = map(int, out.stdout.split())
    assert n > 0, "score set takes no 2-byte cells"
    assert bad == 0, out.stderr
