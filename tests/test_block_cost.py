"""A block's cost in swept columns and the deal of a launch's blocks over the CUs, checked without a GPU
(tests/csrc/block_cost_check.cpp on smoothxg_amd/csrc/poa_cost.h, plain C++): the width priced for every alignment is the one the
block kernel picks, at the boundary of the second width and on either side of it; the per-alignment prefix sums end at the total;
a class without a second width, a banded block and a 32-bit block reproduce their columns; with slots that do not divide by the
CUs the light CUs are dealt the largest costs and the crowded ones the rest in snake order.  The program runs twice: as built for
the engine, and once more with AddressSanitizer and UBSan, as a program of its own."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "block_cost_check.cpp")


def build_and_run(tmp_path_factory, name, flags):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp(name) / "block_cost_check")
    subprocess.check_call([cxx, "-std=c++17", "-Wall"] + flags + ["-o", exe, SRC])
    return subprocess.run([exe], capture_output=True, text=True)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return build_and_run(tmp_path_factory, "block_cost", ["-O1"])


@pytest.fixture(scope="module")
def check_sanitized(tmp_path_factory):
    return build_and_run(tmp_path_factory, "block_cost_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_cost_and_deal(check):
    assert check.returncode == 0, check.stderr
    rows = [tuple(map(int, line.split())) for line in check.stdout.splitlines()]
    # the eight dual-width classes, each with W2's columns up to the boundary and W's beyond it
    assert sorted((t, w, w2) for t, w, w2, *_ in rows) == [(t, w, w - 1) for t in (256, 512) for w in range(9, 13)]
    for t, w, w2, cap, below, at, above in rows:
        assert cap + 1 == t * 2 * w2
        assert (below, at, above) == (t * 2 * w2, t * 2 * w2, t * 2 * w)


def test_cost_and_deal_under_sanitizers(check_sanitized, check):
    assert check_sanitized.returncode == 0, check_sanitized.stderr
    assert check_sanitized.stdout == check.stdout
