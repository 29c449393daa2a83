"""The deal of a batch over the members of a device group, checked without a GPU (tests/csrc/deal_check.cpp on
smoothxg_amd/csrc/poa_deal.h, plain C++): over batches with no blocks, fewer blocks than members, blocks without sequences,
blocks that cost nothing and one huge block, and for groups of 1 to 16 members, every block is dealt exactly once, every member's
list is ascending, two runs give the same parts, and no member costs more than total / n plus the costliest block.  The program
runs twice: as built for the engine, and once more with AddressSanitizer and UBSan, as a program of its own."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "deal_check.cpp")


def build_and_run(tmp_path_factory, name, flags):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp(name) / "deal_check")
    subprocess.check_call([cxx, "-std=c++17", "-Wall"] + flags + ["-o", exe, SRC])
    return subprocess.run([exe], capture_output=True, text=True)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return build_and_run(tmp_path_factory, "deal", ["-O1"])


@pytest.fixture(scope="module")
def check_sanitized(tmp_path_factory):
    return build_and_run(tmp_path_factory, "deal_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_deal(check):
    assert check.returncode == 0, check.stderr
    rows = {f[0]: list(map(int, f[1:])) for f in (line.split() for line in check.stdout.splitlines())}
    for name in ("empty", "fewer-blocks-than-members", "blocks-without-sequences", "zero-cost-blocks", "huge-block-middle", "headline-shape"):
        assert name in rows
    assert rows["empty"] == [0, 0, 0, 0, 0, 0]
    # columns: blocks, then the largest member's share of the total cost in 1/1000 for 1, 2, 3, 8 and 16 members
    assert all(r[1] == 1000 for r in rows.values() if r[0] and r[1])          # (one member carries everything)
    # 1000 equal blocks: 8 members carry 125 each; 3 and 16 members are out by at most one block
    assert rows["headline-shape"][0] == 1000
    assert rows["headline-shape"][1:] == [1000, 500, 334, 125, 63]
    # a block that outweighs the rest of the batch stays whole: its member carries nearly everything at any n > 1
    assert all(s > 900 for s in rows["huge-block-middle"][2:])


def test_deal_under_sanitizers(check_sanitized, check):
    assert check_sanitized.returncode == 0, check_sanitized.stderr
    assert check_sanitized.stdout == check.stdout
