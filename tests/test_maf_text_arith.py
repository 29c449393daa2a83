"""The arithmetic of the MAF text gather, checked without a GPU (tests/csrc/maf_text_check.cpp on smoothxg_amd/csrc/poa_maf_text.h,
plain C++): the kernel's per-granule function, walked chunk by chunk and lane by lane over heap buffers of exactly the sizes the
engine needs, lays every segment list out byte for byte -- the three kinds, all source and destination alignments, lengths around
the chunk, up to 16 segments in one granule, empty segments, the empty list --, writes nothing outside the destination and reads
nothing outside a segment's source, finds its segments as a linear scan does, complements all 256 byte values as
revcomp_gapped's table, and counts a row's letters as a byte loop.  The program runs twice: as built for the engine, and once
more with AddressSanitizer and UBSan, as a program of its own."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "maf_text_check.cpp")
HEADER = os.path.join(HERE, "..", "smoothxg_amd", "csrc", "poa_maf_text.h")


def build_and_run(tmp_path_factory, name, flags):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp(name) / "maf_text_check")
    subprocess.check_call([cxx, "-std=c++17", "-Wall"] + flags + ["-o", exe, SRC])
    return subprocess.run([exe], capture_output=True, text=True)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return build_and_run(tmp_path_factory, "maf_text", ["-O2"])


@pytest.fixture(scope="module")
def check_sanitized(tmp_path_factory):
    return build_and_run(tmp_path_factory, "maf_text_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def digest(run):
    assert run.returncode == 0, run.stderr[-2000:]
    m = re.fullmatch(r"maf_text (\d+) (\d+) (\d+)\n", run.stdout)
    assert m, run.stdout
    return tuple(int(x) for x in m.groups())


def test_text_arithmetic(check):
    chunk, cases, granules = digest(check)
    assert chunk % 16 == 0 and chunk > 0
    assert cases >= 3 * 16 * 16 * 53 + 4 * 16 + 12 + 2   # the grid of the docstring, the runs, the random lists, the empty lists
    assert granules > cases


def test_text_arithmetic_sanitized(check, check_sanitized):
    assert digest(check_sanitized) == digest(check)


def test_header_is_hip_free():
    text = open(HEADER).read()
    assert "hip_runtime" not in text and "threadIdx" not in text and "blockIdx" not in text and "amdgcn" not in text
