"""CPU: the integer arithmetic of decree Q (smoothxg_amd/csrc/poa_identity_key.h, the HIP-free header the kernels include),
checked by tests/csrc/identity_key_check.cpp built for the host with the undefined-behaviour and address sanitizers."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_keys_order_pairs_as_their_fractions_and_ranks_are_the_hosts(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "identity_key_check")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(HERE, "csrc", "identity_key_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    n, bad = map(int, out.stdout.split())
    assert n > 1000000 and bad == 0, out.stderr
