"""The table of the result arrays and the reassembly of a batch's result from its parts, checked without a GPU
(tests/csrc/results_check.cpp on smoothxg_amd/csrc/poa_results.h, plain C++): a random whole result is cut into the results of
parts -- contiguous slices for 1, 2, 3 and 16 parts, interleaved ascending lists as the sharded deal leaves them, a part without
blocks, fewer blocks than parts, blocks without sequences, no blocks at all, every optional group of arrays absent in turn --,
reassembled and compared byte for byte; the full-MSA formatter is run on two small hand-made blocks.  The program runs twice: as
built for the engine, and once more with AddressSanitizer and UBSan, as a program of its own."""
import os
import shutil
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "results_check.cpp")
sys.path.insert(0, HERE)

CASES = ["slices-1", "slices-2", "slices-3", "slices-16", "interleaved-2", "interleaved-3", "interleaved-5", "interleaved-8",
         "empty-part-in-the-middle", "empty-part-first", "empty-parts-without-arrays", "fewer-blocks-than-parts", "fewer-blocks-than-parts-interleaved",
         "blocks-without-sequences", "blocks-without-sequences-interleaved", "only-empty-blocks", "sequences-without-letters",
         "no-blocks", "no-blocks-one-part"] + \
        ["without-%s-%s" % (g, d) for g in ("consensus", "msa", "block-graphs", "paths", "raw-graphs", "block-cycles") for d in ("slices", "interleaved")]


def build_and_run(tmp_path_factory, name, flags):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp(name) / "results_check")
    subprocess.check_call([cxx, "-std=c++17", "-Wall"] + flags + ["-o", exe, SRC])
    return subprocess.run([exe], capture_output=True, text=True)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return build_and_run(tmp_path_factory, "results", ["-O1"])


@pytest.fixture(scope="module")
def check_sanitized(tmp_path_factory):
    return build_and_run(tmp_path_factory, "results_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_reassembly(check):
    assert check.returncode == 0, check.stderr
    lines = [line.split() for line in check.stdout.splitlines()]
    rows = {f[0]: list(map(int, f[1:])) for f in lines if f[0] != "msa"}
    for name in CASES:
        assert name in rows, name
    # columns: blocks, sequences, parts, runs of consecutive blocks, arrays compared, bytes compared
    assert rows["slices-3"][2:4] == [3, 3] and rows["slices-16"][2:4] == [16, 16]      # a contiguous slice is one run
    assert rows["interleaved-5"][3] > 5 and rows["interleaved-8"][3] > 8                 # interleaved parts are several
    assert rows["empty-part-in-the-middle"][2:4] == [3, 2]
    assert rows["no-blocks"][:2] == [0, 0] and rows["no-blocks"][3] == 0
    assert all(r[5] > 0 for r in rows.values())
    # sxg_poa_batch_out has 30 arrays; an optional group that is absent from the parts is absent from the result
    assert all(rows[name][4] == 30 for name in CASES if not name.startswith("without-"))
    assert rows["empty-parts-without-arrays"][2] == 6 and rows["empty-parts-without-arrays-or-block-graphs"][4] == 18
    for group, n in (("consensus", 4), ("msa", 3), ("block-graphs", 12), ("paths", 1), ("raw-graphs", 7), ("block-cycles", 1)):
        assert rows["without-%s-slices" % group][4] == rows["without-%s-interleaved" % group][4] == 30 - n, group


def test_full_msa_rows(check):
    """The formatter's rows are the ones written down in the program (exit status 0) and survive msa_ref's trim of no letters:
    equally long rows per block, no all-gap column in front of or behind them."""
    from msa_ref import trim_rows
    assert check.returncode == 0, check.stderr
    msa = {line.split()[1]: line.split()[2:] for line in check.stdout.splitlines() if line.startswith("msa ")}
    assert msa["consensus=1"] == ["ACGT", "A-GT", "A-GT", "ACT", "AGT", "A-T", "ACT"]
    assert msa["consensus=0"] == ["ACGT", "A-GT", "ACT", "AGT", "A-T"]
    for rows in (msa["consensus=1"][:3], msa["consensus=1"][3:], msa["consensus=0"][:2], msa["consensus=0"][2:]):
        assert trim_rows(rows, 0) == rows


def test_reassembly_under_sanitizers(check_sanitized, check):
    assert check_sanitized.returncode == 0, check_sanitized.stderr
    assert check_sanitized.stdout == check.stdout
