"""The arithmetic of the range gather, checked without a GPU (tests/csrc/letters_check.cpp on smoothxg_amd/csrc/poa_letters.h,
plain C++): the kernel's per-granule function, walked chunk by chunk and lane by lane over heap buffers of exactly the sizes the
engine allocates, cuts every range out byte for byte -- all source and destination alignments, lengths around the chunk, the ends
of the store, empty, repeated and overlapping ranges --, touches nothing beside a range, finds its ranges as a linear scan does,
and codes all 256 byte values as identity_table's switch.  The program runs twice: as built for the engine, and once more with
AddressSanitizer and UBSan, as a program of its own."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "letters_check.cpp")
HEADER = os.path.join(HERE, "..", "smoothxg_amd", "csrc", "poa_letters.h")


def build_and_run(tmp_path_factory, name, flags):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp(name) / "letters_check")
    subprocess.check_call([cxx, "-std=c++17", "-Wall"] + flags + ["-o", exe, SRC])
    return subprocess.run([exe], capture_output=True, text=True)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return build_and_run(tmp_path_factory, "letters", ["-O2"])


@pytest.fixture(scope="module")
def check_sanitized(tmp_path_factory):
    return build_and_run(tmp_path_factory, "letters_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def digest(run):
    assert run.returncode == 0, run.stderr[-2000:]
    m = re.fullmatch(r"letters (\d+) (\d+) (\d+)\n", run.stdout)
    assert m, run.stdout
    return tuple(int(x) for x in m.groups())


def test_gather_arithmetic(check):
    chunk, cases, granules = digest(check)
    assert chunk % 16 == 0 and chunk > 0
    assert cases >= 16 * 16 * 49 + 16 * 6   # the grid of the docstring, and the edge cases per destination alignment
    assert granules > cases


def test_gather_arithmetic_sanitized(check, check_sanitized):
    assert digest(check_sanitized) == digest(check)


def test_header_is_hip_free():
    text = open(HEADER).read()
    assert "hip_runtime" not in text and "threadIdx" not in text and "blockIdx" not in text
