"""CPU: the MAF iteration over MAF rows built by the provider (sxg_smooth_maf_gfa_device_rows, Smoother.smooth_maf_gfa(...,
device_rows=True)): with merge_blocks off it asks the provider for the TRIMMED MSA (want_msa = 2) and compact block graphs,
takes every block's grooming orientation from the collected ranges and laces the flat way -- and must give the GFA, the MAF and
the flip count of the legacy call and of oracle/smooth_oracle.py.  The provider here is the oracle-backed one of
test_smooth_host.py, answering want_msa == 2 with tests/msa_ref.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import smooth_oracle as SO
from smoothxg_amd import smooth as S

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import msa_ref  # noqa: E402
from test_smooth_host import DRB1, OracleProvider, haplotype_gfa, inversion_gfa, synthetic_gfa  # noqa: E402

HEADER = "##maf version=1"


class TrimmedRowsProvider(OracleProvider):
    """OracleProvider that honours SXG_MSA_TRIMMED: the full rows it formatted, trimmed by msa_ref with the block's bg_trim."""

    def __init__(self):
        super().__init__()
        self.asked = []   # (want_msa, want_block_graph, trims given) of every call

    def _run(self, ctx, pin, pout):
        rc = super()._run(ctx, pin, pout)
        i, o = pin.contents, pout.contents
        self.asked.append((i.want_msa, i.want_block_graph, bool(i.bg_trim)))
        if rc or i.want_msa != 2:
            return rc
        arrs = self.keep[-1]
        nb = i.n_blocks
        blk = np.ctypeslib.as_array(i.blk_off, (nb + 1,))
        raw = bytes(arrs["msa"])
        off, cols, txt = [0], [], b""
        for b in range(nb):
            nrow = int(blk[b + 1] - blk[b]) + (1 if i.want_consensus else 0) if blk[b + 1] > blk[b] else 0
            w = int(arrs["msa_cols"][b]) if nrow else 0
            a = int(arrs["msa_off"][b])
            rows = msa_ref.trim_rows([raw[a + r * w:a + (r + 1) * w].decode() for r in range(nrow)], int(i.bg_trim[b]) if i.bg_trim else 0)
            cols.append(len(rows[0]) if rows else 0)
            txt += "".join(rows).encode()
            off.append(len(txt))
        new = dict(msa_off=np.asarray(off, np.int64), msa_cols=np.asarray(cols or [0], np.int32), msa=np.frombuffer(txt + b"\0", np.uint8).copy())
        self.keep.append(new)
        o.msa_off = new["msa_off"].ctypes.data_as(C.POINTER(C.c_int64))
        o.msa_cols = new["msa_cols"].ctypes.data_as(C.POINTER(C.c_int32))
        o.msa = new["msa"].ctypes.data
        return 0


@pytest.fixture(scope="module")
def prov():
    return TrimmedRowsProvider()


def last_path_first(text):
    """The generator's GFA with its last P line moved in front of the others: the mostly-reversed path becomes the
    lowest-ranked one, and the blocks it runs through groom-flip."""
    lines = text.rstrip("\n").split("\n")
    ps = [k for k, l in enumerate(lines) if l.startswith("P\t")]
    last = lines.pop(ps[-1])
    lines.insert(ps[0], last)
    return "\n".join(lines) + "\n"


def groomed_blocks(g, blocks, fraction=0.001):
    """Blocks whose lowest-ranked non-empty range was collected in reverse (what groom_flip answers on the block graph)."""
    n = 0
    for blk in blocks:
        c = SO.collect(g, blk, fraction)
        if not c.seqs:
            continue
        rev = {}
        for rank, dups in enumerate(c.dup_rank):
            for x, r in enumerate(dups):
                if len(c.seqs[rank]) > 2 * c.poa_padding:
                    rev[r] = c.dup_is_revs[rank][x]
        order = sorted(rev, key=lambda r: (blk[r][0], r))
        n += bool(order and rev[order[0]])
    return n


def run_case(prov, text, sm, blocks, pkw, okw):
    g = SO.Graph(text)
    p = S.default_params(**pkw)
    prov.asked.clear()
    new = sm.smooth_maf_gfa(p, prov.provider(), merge_blocks=False, header=HEADER, device_rows=True)
    assert prov.asked and all(a == (2, 3, True) for a in prov.asked), prov.asked
    prov.asked.clear()
    old = sm.smooth_maf_gfa(p, prov.provider(), merge_blocks=False, header=HEADER)
    assert prov.asked and all(a[0] == 1 and a[1] == 0 for a in prov.asked), prov.asked
    assert new[1] == old[1], "MAF"
    assert new[2] == old[2] == 0, "flips"
    assert new[0] == old[0], "GFA"
    want = SO.smooth(g, blocks, merge=dict(merge_blocks=False, header=HEADER), **okw)
    assert new[1] == want[1] and new[2] == len(want[2]) and new[0] == want[0]
    return g, new


@pytest.mark.parametrize("seed", [0, 1])
def test_groomed_blocks_of_a_reversed_lowest_path(prov, seed):
    """(a) the reversed path ranked lowest: nearly every block groom-flips, and the flag comes from the collected ranges."""
    text = last_path_first(synthetic_gfa(seed))
    sm = S.Smoother(text, 90)
    blocks = SO.blockset_by_path_windows(SO.Graph(text), 90)
    g, new = run_case(prov, text, sm, blocks, dict(add_consensus=1), dict(add_consensus=True))
    assert groomed_blocks(g, blocks) >= len(blocks) - 1 >= 7
    assert groomed_blocks(SO.Graph(synthetic_gfa(seed)), SO.blockset_by_path_windows(SO.Graph(synthetic_gfa(seed)), 90)) == 0
    sm.close()


def test_block_collected_in_reverse_is_groomed_back(prov):
    """(b) a long inversion: the middle block is collected in reverse."""
    text = inversion_gfa(3, length=2400, lo=800, hi=1600)
    sm = S.Smoother(text, 800)
    blocks = SO.blockset_by_path_windows(SO.Graph(text), 800)
    g, new = run_case(prov, text, sm, blocks, dict(add_consensus=1), dict(add_consensus=True))
    assert 1 <= groomed_blocks(g, blocks) < len(blocks)
    sm.close()


@pytest.mark.parametrize("frac", [None, 0.0])
def test_haplotypes_with_and_without_padding(prov, frac):
    """(c) padded blocks (rows trimmed, edge columns cut) and unpadded ones (trimmed == full)."""
    text = haplotype_gfa(0, n_paths=6, length=1500)
    sm = S.Smoother(text, 300)
    blocks = SO.blockset_by_path_windows(SO.Graph(text), 300)
    pkw = {} if frac is None else dict(poa_padding_fraction=frac)
    okw = {} if frac is None else dict(fraction=frac)
    g, new = run_case(prov, text, sm, blocks, pkw, okw)
    pads = [SO.collect(g, blk, 0.001 if frac is None else frac).poa_padding for blk in blocks]
    assert (max(pads) > 0) == (frac is None)
    sm.close()


_DRB1 = {}


def drb1_discovered(prov):
    """(d) the reference's own input with the block discovery of its test (-j 5k -e 5k -l 700 -r 12), consensus on: the new
    call's outputs, computed once for the two tests below."""
    if not _DRB1:
        text = open(DRB1).read()
        g = SO.Graph(text)
        _DRB1["g"] = g
        _DRB1["blocks"] = SO.break_blocks(g, SO.smoothable_blocks(g, 700 * 12, 700, 5000, 5000), 1400)
        sm = S.Smoother(text, discover=dict(target_poa_length=700, n_haps=12, max_path_jump=5000, max_edge_jump=5000))
        p = S.default_params(add_consensus=1)
        prov.asked.clear()
        _DRB1["new"] = sm.smooth_maf_gfa(p, prov.provider(), merge_blocks=False, header=HEADER, device_rows=True)
        assert prov.asked and all(a == (2, 3, True) for a in prov.asked)
        _DRB1["old"] = sm.smooth_maf_gfa(p, prov.provider(), merge_blocks=False, header=HEADER)
        sm.close()
    return _DRB1


def test_drb1_discovered_blocks_equal_the_legacy_call(prov):
    """(d) against the legacy call.  8 of the 2161 discovered blocks (375, 433, 441, 783, 789, 882, 1080, 1372) have a
    consensus of 618..621 nodes under a padding of 311: their consensus row holds fewer than 2 * 311 letters and is all gaps
    in both calls."""
    d = drb1_discovered(prov)
    new, old = d["new"], d["old"]
    assert new[1] == old[1], "MAF"
    assert new[2] == old[2] == 0, "flips"
    assert new[0] == old[0], "GFA"


def oracle_maf_rows_total(g, ranges, c, msa, consensus_name, consensus_len, _orig=SO.maf_rows):
    """SO.maf_rows where it is defined.  It blanks `padding` letters from either end of every row as src/smooth.cpp:791-812
    does and, like the reference, walks off a row that holds fewer than 2 * padding letters (IndexError): the consensus of a
    local alignment can be that short.  For such a consensus row the rule of SXG_MSA_TRIMMED is stated here instead -- the row
    is all gaps, its size 0 --, and the sequence rows still come from SO.maf_rows itself."""
    pad = c.poa_padding
    if msa and consensus_name and pad > 0 and sum(ch != "-" for ch in msa[-1]) < 2 * pad:
        rows = _orig(g, ranges, c, msa[:-1], "", 0)
        return rows + [(consensus_name, 0, 0, False, 0, "-" * (len(rows[0][5]) if rows else 0))]
    return _orig(g, ranges, c, msa, consensus_name, consensus_len)


def test_drb1_discovered_blocks_equal_the_oracle(prov, monkeypatch):
    """(d) against oracle/smooth_oracle.py, all 2161 blocks.  SO.maf_rows cannot format the consensus rows of blocks 375, 433,
    441, 783, 789, 882, 1080 and 1372 (618..621 letters, padding 311: see oracle_maf_rows_total); SO.smooth runs with that
    one function completed for such rows, everything else -- every other row of those blocks included -- is the oracle's."""
    d = drb1_discovered(prov)
    short = []
    def counting(g, ranges, c, msa, name, clen):
        if name and c.poa_padding and sum(ch != "-" for ch in msa[-1]) < 2 * c.poa_padding:
            short.append(name)
        return oracle_maf_rows_total(g, ranges, c, msa, name, clen)
    monkeypatch.setattr(SO, "maf_rows", counting)
    want = SO.smooth(d["g"], d["blocks"], add_consensus=True, merge=dict(merge_blocks=False, header=HEADER))
    assert short == ["Consensus_%d" % k for k in (375, 433, 441, 783, 789, 882, 1080, 1372)]
    new = d["new"]
    assert new[1] == want[1] and new[2] == len(want[2]) and new[0] == want[0]


def test_abpoa_path_with_consensus(prov):
    """(e) -A: banded blocks, the consensus path restricted to visited nodes -- the consensus ROW is not."""
    text = haplotype_gfa(4, 5, 1200)
    sm = S.Smoother(text, 400)
    blocks = SO.blockset_by_path_windows(SO.Graph(text), 400)
    run_case(prov, text, sm, blocks, dict(add_consensus=1, use_abpoa=1), dict(add_consensus=True, abpoa=True))
    sm.close()


def test_two_chunks_give_the_same_bytes(prov, monkeypatch):
    """(f) the chunk pipeline: blocks validated as their chunk comes back, rows built per chunk."""
    text = last_path_first(synthetic_gfa(1))
    sm = S.Smoother(text, 90)
    blocks = SO.blockset_by_path_windows(SO.Graph(text), 90)
    assert len(blocks) >= 4
    p = S.default_params(add_consensus=1)
    one = sm.smooth_maf_gfa(p, prov.provider(), header=HEADER, device_rows=True)
    monkeypatch.setenv("SXG_SMOOTH_CHUNK_BLOCKS", str(len(blocks) // 2))
    prov.asked.clear()
    two = sm.smooth_maf_gfa(p, prov.provider(), header=HEADER, device_rows=True)
    assert len(prov.asked) == 2
    assert two == one
    sm.close()


def test_a_provider_that_returns_the_full_msa_is_refused():
    """The unmodified OracleProvider ignores the value of want_msa and returns untrimmed rows: with padding > 0 the letters
    of a row do not number its length minus twice the padding, and the call fails naming the contract."""
    text = haplotype_gfa(0, n_paths=6, length=1500)
    sm = S.Smoother(text, 300)
    plain = OracleProvider()
    with pytest.raises(S.SmoothError, match="SXG_MSA_TRIMMED"):
        sm.smooth_maf_gfa(S.default_params(), plain.provider(), header=HEADER, device_rows=True)
    assert sm.smooth_maf_gfa(S.default_params(), plain.provider(), header=HEADER)[1].startswith(HEADER)   # the legacy call still works
    sm.close()


def test_with_merging_it_is_the_legacy_call(prov, monkeypatch):
    """merge_blocks on (and SXG_SMOOTH_LEGACY=1 with it off): the provider is asked for the full MSA and no block graphs, and
    the results are the legacy call's."""
    text = synthetic_gfa(6, n_paths=6, n_nodes=80)
    sm = S.Smoother(text, 90)
    p = S.default_params(add_consensus=1)
    prov.asked.clear()
    new = sm.smooth_maf_gfa(p, prov.provider(), merge_blocks=True, jaccard=0.0, header=HEADER, device_rows=True)
    assert all(a[0] == 1 and a[1] == 0 for a in prov.asked)
    assert new == sm.smooth_maf_gfa(p, prov.provider(), merge_blocks=True, jaccard=0.0, header=HEADER)
    assert " merged=true" in new[1]
    monkeypatch.setenv("SXG_SMOOTH_LEGACY", "1")
    prov.asked.clear()
    leg = sm.smooth_maf_gfa(p, prov.provider(), header=HEADER, device_rows=True)
    assert all(a[0] == 1 and a[1] == 0 for a in prov.asked)
    monkeypatch.delenv("SXG_SMOOTH_LEGACY")
    assert leg == sm.smooth_maf_gfa(p, prov.provider(), header=HEADER, device_rows=True)
    sm.close()
