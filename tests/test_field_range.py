"""The biased fields of the packed sweep's local rows as binary16 patterns (smoothxg_amd/csrc/poa_fields.h): the header's bound
holds for the default scores at every packed strip width, the patterns 0 .. 0x7BFF are strictly increasing in binary16 value
(decoded with integers only) and 0x7C00 is the first that is not finite -- what makes one three-input binary16 maximum equal two
packed integer maxima."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_local_fields_stay_in_the_ordered_binary16_patterns(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "field_range_check")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(HERE, "csrc", "field_range_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, check=True)
    n, bad = map(int, out.stdout.split())
    assert n > 0x7BFF and bad == 0, out.stderr
