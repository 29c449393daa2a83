"""The owners of the engine host's device resources, checked without a GPU (tests/csrc/devres_check.cpp on
smoothxg_amd/csrc/poa_devres.h, plain C++ with counting stand-ins for hipMalloc / hipFree, events and streams): a scope exit, an
early return, a growing and a non-growing ensure, a refused allocation with and without a successful retry, moves, a cleared vector
of owners, a double release, and the guard of a result.  Every case ends with nothing alive; a free of something not alive aborts
the program.  It runs twice: plain, and once more with AddressSanitizer and UBSan, as a program of its own."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "devres_check.cpp")

CASES = ["scope-exit", "early-return", "ensure-grows", "ensure-smaller", "first-malloc-fails", "both-mallocs-fail", "move-construct",
         "move-assign", "vector-of-unique-ptr", "release-twice", "guard-frees", "guard-dismissed"]


def build_and_run(tmp_path_factory, name, flags):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp(name) / "devres_check")
    subprocess.check_call([cxx, "-std=c++17", "-Wall"] + flags + ["-o", exe, SRC])
    return subprocess.run([exe], capture_output=True, text=True)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return build_and_run(tmp_path_factory, "devres", ["-O1"])


@pytest.fixture(scope="module")
def check_sanitized(tmp_path_factory):
    return build_and_run(tmp_path_factory, "devres_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_owners_free_what_they_hold(check):
    assert check.returncode == 0, check.stderr
    lines = [line.split() for line in check.stdout.splitlines()]
    assert [f[0] for f in lines] == CASES
    # columns: hipMalloc calls, hipFree calls, a figure of the case
    rows = {f[0]: list(map(int, f[1:])) for f in lines}
    assert rows["scope-exit"][:2] == [1, 1]
    assert rows["early-return"][:2] == [6, 6]
    assert rows["ensure-grows"] == [2, 2, 5000 + 5000 // 8 + 256]
    assert rows["ensure-smaller"][:2] == [1, 1]
    assert rows["first-malloc-fails"] == [2, 1, 3000]
    assert rows["both-mallocs-fail"][:2] == [4, 2]
    assert rows["move-construct"][:2] == [1, 1] and rows["move-assign"][:2] == [2, 2]
    assert rows["vector-of-unique-ptr"][:2] == [7, 7]
    assert rows["release-twice"][:2] == [1, 1]
    assert rows["guard-frees"][2] == 1 and rows["guard-dismissed"][2] == 0


def test_owners_under_sanitizers(check_sanitized, check):
    assert check_sanitized.returncode == 0, check_sanitized.stderr
    assert check_sanitized.stdout == check.stdout
