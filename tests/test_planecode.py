"""The traceback plane of the packed sweep's 2-byte classes holds stored-row codes (smoothxg_amd/csrc/poa_rowcode.h, round 11):
strips of 4, 11 and 13 cells built from every representable (step, H - oF, H - oO) of a score set, encoded with the sweep's
p16_row_encode and laid out as a plane row keeps them (the H left of the strip, then the codes, as halfwords), decode back to
every column's H and outgoing gap candidates with the strip decoder the traceback calls -- biased (local) and plain (global)
arithmetic, convex and not, a strip with a left neighbour and "strip 0", whose left word is its own first H."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

# (m, n, g, e, q, c) in the engine's sign convention
SCORES = {
    "default": (1, -4, -6, -2, -26, -1),
    "affine": (1, -4, -6, -2, -6, -2),
    "asm15": (1, -7, -11, -2, -33, -1),
    "asm10": (1, -9, -16, -2, -41, -1),   # 16 bits: the widest code
}


def _compile(tmp_path_factory, flags):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("planecode") / "planecode_check")
    subprocess.check_call([cxx, "-std=c++17"] + flags + ["-o", exe, os.path.join(HERE, "csrc", "planecode_check.cpp")])
    return exe


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _compile(tmp_path_factory, ["-O2"])


@pytest.mark.parametrize("name", list(SCORES))
def test_plane_strips_of_row_codes_decode_to_every_cell(checker, name):
    out = subprocess.run([checker] + [str(v) for v in SCORES[name]], capture_output=True, text=True, check=True)
    n, bad = map(int, out.stdout.split())
    assert n > 0, "score set takes no 2-byte cells"
    assert bad == 0, out.stderr


def test_strip_decoder_is_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path_factory):
    """The same program as a stand-alone host binary built with -fsanitize=address,undefined, on the widest code."""
    exe = _compile(tmp_path_factory, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    out = subprocess.run([exe] + [str(v) for v in SCORES["asm10"]], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    n, bad = map(int, out.stdout.split())
    assert n > 0 and bad == 0, out.stderr
