"""CPU: the arithmetic of the trimmed MSA (smoothxg_amd/csrc/poa_msa_cols.h, the HIP-free header the kernels of poa_msa.hip.h
include), checked by tests/csrc/msa_cols_check.cpp built for the host with the undefined-behaviour and address sanitizers; and
the Python restatement of the trimmed MSA the other tests compare with (tests/msa_ref.py), pinned to the oracle's MAF rows."""
import os
import shutil
import subprocess
import sys

import pytest

from oracle import smooth_oracle as SO

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import msa_ref  # noqa: E402

DRB1 = os.path.join(HERE, "golden", "DRB1-3123.seqwish.gfa")


def test_columns_trim_spans_and_the_16_byte_split_equal_a_naive_restatement(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "msa_cols_check")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(HERE, "csrc", "msa_cols_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    n, bad = map(int, out.stdout.split())
    assert n > 500000 and bad == 0, out.stderr


@pytest.mark.parametrize("cons", [0, 1])
def test_trimmed_msa_restatement_gives_the_oracles_maf_row_texts(cons):
    """DRB1 blocks 0, 4 and 8 (path windows of 700): msa_ref.trim_rows of the full MSA == the text of every MAF row of
    oracle/smooth_oracle.py::maf_rows, one row per dedup'd sequence before the rows are repeated for duplicates."""
    g = SO.Graph(open(DRB1).read())
    blocks = SO.blockset_by_path_windows(g, 700)
    seen_pad = False
    for k in (0, 4, 8):
        c = SO.collect(g, blocks[k])
        assert c.seqs
        msa, clen = SO.poa_msa(c, bool(cons))
        rows = SO.maf_rows(g, blocks[k], c, msa, ("Consensus_%d" % k) if cons else "", clen)
        want, at = [], 0
        for rank in range(len(msa)):
            is_cons = bool(cons) and rank == len(msa) - 1
            want.append(rows[at][5])
            at += 1 if is_cons else len(c.dup_rank[rank])
        assert at == len(rows)
        got = msa_ref.trim_rows(msa, c.poa_padding)
        assert got == want
        assert len({len(r) for r in got}) == 1
        for r, s in zip(got, c.seqs):
            assert len(r.replace("-", "")) == len(s) - 2 * c.poa_padding
        seen_pad |= c.poa_padding > 0
    assert seen_pad


def test_trim_rows_edge_cases():
    assert msa_ref.trim_rows([], 3) == []
    assert msa_ref.trim_rows(["AC-GT", "A-CGT"], 0) == ["AC-GT", "A-CGT"]
    assert msa_ref.trim_rows(["AC-GT", "-TCA-"], 1) == ["C-G", "-C-"]          # rows start at different columns
    assert msa_ref.trim_rows(["ACGT", "A--T"], 1) == ["CG", "--"]               # exactly 2 * trim letters: an all-gap row
    assert msa_ref.trim_rows(["ACGT", "A-GT"], 2) == ["", ""]                   # nothing remains
    assert msa_ref.trim_rows(["ACGTA", "AC---"], 2) == ["G", "-"]               # a row with fewer than 2 * trim letters
    assert msa_ref.trim_rows(["A-C-G", "ATCTG"], 1) == ["-C-", "TCT"]           # interior all-gap columns of a row stay
