"""The column tiles of the 32-bit sweep, checked without a GPU (tests/csrc/tile_check.cpp on smoothxg_amd/csrc/poa_tiles.h, plain
C++): for every 32-bit geometry the host can choose and every length up to SXG_POA_MAX_SEQ_LEN_TILED the tiles partition the
columns 0 .. L, virtual lanes and (tile, lane) pairs map onto each other one to one, one tile is today's sweep (its padded width,
its lanes), the two boundary buffers alternate, and a tiled launch is priced rows x padded width.  The program runs twice: as
built for the engine, and once more with AddressSanitizer and UBSan, as a program of its own."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "csrc", "tile_check.cpp")


def build_and_run(tmp_path_factory, name, flags):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp(name) / "tile_check")
    subprocess.check_call([cxx, "-std=c++17", "-Wall"] + flags + ["-o", exe, SRC])
    return subprocess.run([exe], capture_output=True, text=True)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return build_and_run(tmp_path_factory, "tiles", ["-O2"])


@pytest.fixture(scope="module")
def check_sanitized(tmp_path_factory):
    return build_and_run(tmp_path_factory, "tiles_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_tiles(check):
    assert check.returncode == 0, check.stderr
    rows = {(t, w): (tc, nt, lpad) for t, w, tc, nt, lpad in (map(int, line.split()) for line in check.stdout.splitlines())}
    # the widest geometry: four tiles of 12 288 columns at the limit; the geometries the GPU tests force with SXG_POA_TILE_COLS
    assert rows[(1024, 12)] == (12288, 4, 49152)
    assert rows[(64, 8)] == (512, 96, 49152)
    assert rows[(512, 12)] == (6144, 8, 49152)
    for (t, w), (tc, nt, lpad) in rows.items():
        assert tc == t * w and lpad == nt * tc and (nt - 1) * tc <= 49151 < lpad


def test_tiles_under_sanitizers(check_sanitized, check):
    assert check_sanitized.returncode == 0, check_sanitized.stderr
    assert check_sanitized.stdout == check.stdout


def test_limit_of_the_header_and_of_the_python_mirror():
    from smoothxg_amd import poa
    src = open(os.path.join(ROOT, "include", "sxg_poa.h")).read()
    assert int(re.search(r"#define SXG_POA_MAX_SEQ_LEN_TILED (\d+)", src).group(1)) == poa.MAX_SEQ_LEN_TILED == 4 * 12288 - 1
