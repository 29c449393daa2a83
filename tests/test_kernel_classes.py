"""The host-side choice of a kernel class (smoothxg_amd/csrc/poa_classes.h), checked without a GPU for every sequence length
0 .. 26 623, row modes 0-2, local and global alignment, 2- and 4-byte plane cells, full and narrowed plane, with and without the
spread step's halving, block and align-only kernels: the chosen geometry always has a built class (convex and affine, and the
default-score class where the host asks for it), a class compiled for a thread count runs at it, a class compiled for a plane
that keeps every strip gets one, the columns cover the sequence -- and the choice is the one the engine made before the classes
were listed in one place (tests/golden/geometry_choice.json: break points `first maxlen, W, NW, TMAX` per mode, W = -1 where no
geometry fits or the spread step does not apply)."""
import json
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_LEN = 26623


@pytest.fixture(scope="module")
def choices(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("classes") / "class_check")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "csrc", "class_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    table = {}
    for line in out.stdout.splitlines():
        kind, rm, sw, cb, full, spread, maxlen, w, nw, tmax = map(int, line.split())
        table.setdefault((kind, rm, sw, cb, full, spread), []).append((maxlen, w, nw, tmax))
    return out, table


def test_every_chosen_geometry_has_a_class_it_can_run(choices):
    out, table = choices
    assert out.returncode == 0, out.stderr
    # block kernels: 3 row modes x local/global x 2 cell formats x 2 planes x 2 (spread); align-only: 3 row modes x local/global
    assert len(table) == 48 + 6
    for rows in table.values():
        assert [r[0] for r in rows] == list(range(MAX_LEN + 1))


def test_choice_equals_the_recorded_one(choices):
    _, table = choices
    with open(os.path.join(HERE, "golden", "geometry_choice.json")) as f:
        golden = json.load(f)
    assert golden["max_len"] == MAX_LEN and golden["columns"] == ["first_maxlen", "W", "NW", "TMAX"]
    assert len(golden["modes"]) == len(table)
    compared = 0
    for mode in golden["modes"]:
        key = (1 if mode["kind"] == "align" else 0, mode["rm"], mode["sw"], mode["cb"], mode["full_plane"], mode["spread"])
        breaks = mode["rows"]
        assert breaks[0][0] == 0 and all(a[0] < b[0] for a, b in zip(breaks, breaks[1:]))
        expected = []
        for i, (first, w, nw, tmax) in enumerate(breaks):
            last = breaks[i + 1][0] if i + 1 < len(breaks) else MAX_LEN + 1
            expected.extend((maxlen, w, nw, tmax) for maxlen in range(first, last))
        got = table[key]
        assert len(got) == len(expected) == MAX_LEN + 1
        wrong = [(g, e) for g, e in zip(got, expected) if g != e]
        assert not wrong, "mode %s: %d of %d differ, first (got, recorded) %s" % (key, len(wrong), len(got), wrong[0])
        compared += len(got)
    assert compared == 54 * (MAX_LEN + 1)
