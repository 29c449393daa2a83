"""The second strip width of the packed block classes, checked without a GPU (tests/csrc/width2_check.cpp, host code only): for
every built class that has one, the slot layout's plane, pool and row 0 and the launch's LDS hold a sweep at either width, the
width an alignment runs at is the narrowest that covers its sequence, and only the packed 2-byte block classes of four and eight
waves, W = 9 .. 12, have a second width (W - 1, itself a built class of the same row)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.path.exists(hipcc), "no hipcc"
    exe = str(tmp_path_factory.mktemp("width2") / "width2_check")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-O1", "-std=c++17", "-o", exe, os.path.join(HERE, "csrc", "width2_check.cpp")])
    return subprocess.run([exe], capture_output=True, text=True)


def test_layout_and_choice_cover_both_widths(check):
    assert check.returncode == 0, check.stderr
    rows = [tuple(map(int, line.split())) for line in check.stdout.splitlines()]
    assert sorted((t, w, w2, cb) for t, w, w2, cb, *_ in rows) == [(t, w, w - 1, 2) for t in (256, 512) for w in range(9, 13)]
    for t, w, w2, cb, bs1, bs2, plane, pool, lds, lds_rows in rows:
        # ~1 100 columns around the hint at either width, and a plane row that holds the wider of the two bands
        assert bs1 * w >= 1100 and bs2 * w2 >= 1100 and bs1 % 4 == 0 and bs2 % 4 == 0
        assert lds <= 160 * 1024 // (16 // (t // 64))   # (the share of a CU's LDS when four waves per SIMD are resident)
