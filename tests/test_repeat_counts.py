"""The arithmetic of the tandem-repeat scan, checked without a GPU (tests/csrc/repeat_check.cpp on smoothxg_amd/csrc/poa_repeat.h,
plain C++): the counting kernel's per-lane function, walked lane by lane and work item by work item over heap buffers of exactly
n bytes, gives the counts of the naive double loop for an exhaustive small grid and for long sequences at the reference's
parameters; the statistics function and the host's decision give the bits of the host scan's sums.  The program runs twice: as
built for the engine, and once more with AddressSanitizer and UBSan, as a program of its own.  Here its printed digest of the long
cases is compared with counts numpy makes from the same letters, and the decided lengths with the oracle's repeat_length."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import smooth_oracle as SO

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "repeat_check.cpp")
MASK = (1 << 64) - 1


def build_and_run(tmp_path_factory, name, flags):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp(name) / "repeat_check")
    subprocess.check_call([cxx, "-std=c++17", "-Wall"] + flags + ["-o", exe, SRC])
    return subprocess.run([exe], capture_output=True, text=True)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return build_and_run(tmp_path_factory, "repeat", ["-O2"])


@pytest.fixture(scope="module")
def check_sanitized(tmp_path_factory):
    return build_and_run(tmp_path_factory, "repeat_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def make_seq(n, period, sub_pct, seed):
    """make_seq of repeat_check.cpp: the same 64-bit LCG, the same draws."""
    alphabet = b"ACGTaN"
    state = seed

    def lcg():
        nonlocal state
        state = (state * 6364136223846793005 + 1442695040888963407) & MASK
        return state >> 33
    unit = bytes(alphabet[lcg() % 6] for _ in range(period))
    out = bytearray(n)
    for i in range(n):
        roll, other = lcg() % 100, lcg() % 6
        out[i] = alphabet[other] if roll < sub_pct else unit[i % period]
    return bytes(out)


def numpy_counts(seq, min_copy, max_copy, stride):
    s = np.frombuffer(seq, np.uint8)
    n = len(s)
    hi = min(max_copy, n - min_copy)
    return np.array([int((s[0:n - L:stride] == s[L:n:stride]).sum()) for L in range(min_copy, hi + 1)], np.int32)


def fnv64(counts):
    h = 1469598103934665603
    for b in counts.astype("<i4").tobytes():
        h = ((h ^ b) * 1099511628211) & MASK
    return h


def test_counts_and_statistics(check):
    assert check.returncode == 0, check.stderr
    lines = check.stdout.splitlines()
    grid = lines[0].split()
    assert grid[0] == "grid" and int(grid[1]) == 201 * 3 * 3 * 5 and int(grid[2]) >= 64 * int(grid[1])
    longs = [line.split() for line in lines[1:]]
    assert [int(f[1]) for f in longs] == [2000, 2001, 21000, 21049, 45000]
    lengths = []
    for k, f in enumerate(longs):
        n, period, n_lags, best, length, digest = int(f[1]), int(f[2]), int(f[3]), int(f[4]), int(f[5]), int(f[6], 16)
        seq = make_seq(n, period, 5, 77 + k)
        counts = numpy_counts(seq, 1000, 20000, 50)
        assert len(counts) == n_lags == min(20000, n - 1000) - 1000 + 1
        assert fnv64(counts) == digest, f
        assert length == SO.repeat_length(seq.decode(), 1000, 20000, 5, 50), f
        assert length in (0, 1000 + best)
        lengths.append(length)
    assert lengths[:2] == [0, 0]   # (2000, 2001: one and two lags, no z of 5)
    assert all(length > 0 and length % int(f[2]) == 0 for length, f in zip(lengths[2:], longs[2:]))   # (a whole number of copies)


def test_counts_under_sanitizers(check_sanitized, check):
    assert check_sanitized.returncode == 0, check_sanitized.stderr
    assert check_sanitized.stdout == check.stdout
