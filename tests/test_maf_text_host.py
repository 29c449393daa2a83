"""Host library only: sxg_smooth_maf_gfa_device_text -- the MAF text laid out by a text provider from literals the library formats
and the trimmed rows a POA provider keeps -- against sxg_smooth_maf_gfa_device_rows with the same provider, byte for byte.  The
POA provider is the oracle-backed one of tests/test_maf_device_rows_host.py, which here keeps its trimmed rows to itself
(SXG_MSA_TRIMMED_RESIDENT: msa comes back NULL); the texter is python_maf_texter over numpy."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import smooth_oracle as SO
from smoothxg_amd import poa as P
from smoothxg_amd import smooth as S

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_maf_device_rows_host import HEADER, TrimmedRowsProvider, groomed_blocks, last_path_first  # noqa: E402
from test_smooth_host import DRB1, inversion_gfa, synthetic_gfa  # noqa: E402

COMP = np.full(256, ord("N"), np.uint8)   # revcomp_gapped's table
for a, b in ("AT", "TA", "CG", "GC", "--"):
    COMP[ord(a)] = ord(b)


class ResidentRowsProvider(TrimmedRowsProvider):
    """TrimmedRowsProvider that honours SXG_MSA_TRIMMED_RESIDENT too: msa_off and msa_cols go out, the rows stay here -- until the
    next call, as on the engine -- for the two functions of a MAF text provider."""

    def __init__(self):
        super().__init__()
        self.rows = None          # the resident rows of the last call that asked for them: a list of uint8 arrays, global row order
        self.letters_calls = self.text_calls = 0
        self.off_by_one = None    # (row index): the letters provider lies about that row
        self.text_fails = False
        self.text_bytes = 0

    def _run(self, ctx, pin, pout):
        i, o = pin.contents, pout.contents
        self.rows = None
        if i.want_msa != P.MSA_TRIMMED_RESIDENT:
            return super()._run(ctx, pin, pout)
        i.want_msa = P.MSA_TRIMMED
        try:
            rc = super()._run(ctx, pin, pout)
        finally:
            i.want_msa = P.MSA_TRIMMED_RESIDENT
        self.asked[-1] = (P.MSA_TRIMMED_RESIDENT,) + self.asked[-1][1:]
        if rc:
            return rc
        nb = i.n_blocks
        blk = np.ctypeslib.as_array(i.blk_off, (nb + 1,))
        new = self.keep[-1]
        self.rows = []
        for b in range(nb):
            nrow = int(blk[b + 1] - blk[b]) + (1 if i.want_consensus else 0) if blk[b + 1] > blk[b] else 0
            w, a = int(new["msa_cols"][b]), int(new["msa_off"][b])
            self.rows += [new["msa"][a + r * w:a + (r + 1) * w].copy() for r in range(nrow)]
        o.msa = None
        return 0

    # the text provider
    def letters(self):
        self.letters_calls += 1
        if self.rows is None:
            return None
        out = [int((r != ord("-")).sum()) for r in self.rows]
        if self.off_by_one is not None and self.off_by_one < len(out):
            out[self.off_by_one] += 1
        return out

    def text(self, segs, literal):
        self.text_calls += 1
        if self.rows is None or self.text_fails:
            return None
        parts = []
        for src, ln, kind in segs.tolist():
            if kind == P.MAF_LITERAL:
                assert 0 <= src and src + ln <= len(literal)
                parts.append(literal[src:src + ln])
            else:
                assert kind in (P.MAF_ROW, P.MAF_ROW_REVCOMP) and len(self.rows[src]) == ln
                parts.append(self.rows[src] if kind == P.MAF_ROW else COMP[self.rows[src][::-1]])
        out = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
        self.text_bytes += len(out)
        return out

    def texter(self):
        return S.python_maf_texter(self.letters, self.text)


@pytest.fixture()
def prov():
    return ResidentRowsProvider()


def both(prov, sm, p, **kw):
    """(device_text, device_rows) results of the same call; the provider was asked for resident rows in the first, and the
    texter was called once per provider call"""
    prov.asked.clear()
    prov.letters_calls = prov.text_calls = 0
    new = sm.smooth_maf_gfa(p, prov.provider(), header=HEADER, device_text=prov.texter(), **kw)
    n_calls = len(prov.asked)
    assert n_calls and all(a == (P.MSA_TRIMMED_RESIDENT, 3, True) for a in prov.asked), prov.asked
    assert prov.text_calls == n_calls and prov.letters_calls <= n_calls
    prov.asked.clear()
    old = sm.smooth_maf_gfa(p, prov.provider(), header=HEADER, device_rows=True, **kw)
    assert all(a[0] == P.MSA_TRIMMED for a in prov.asked)
    return new, old, n_calls


INPUTS = {
    "synthetic": lambda: (last_path_first(synthetic_gfa(0)), 90),
    "inversion": lambda: (inversion_gfa(3, length=2400, lo=800, hi=1600), 800),
}


@pytest.mark.parametrize("cons", [0, 1])
@pytest.mark.parametrize("name", sorted(INPUTS))
def test_text_equals_rows(prov, name, cons):
    text, w = INPUTS[name]()
    sm = S.Smoother(text, w)
    new, old, _ = both(prov, sm, S.default_params(add_consensus=cons))
    assert new[1] == old[1], "MAF"
    assert new[0] == old[0] and new[2] == old[2] == 0
    assert new[1].startswith(HEADER + "\n") and len(new[1].encode()) == prov.text_bytes
    g = SO.Graph(text)
    assert groomed_blocks(g, SO.blockset_by_path_windows(g, w)) >= 1      # kind 2 was in it
    if cons:
        assert "Consensus_0" in new[1]
    sm.close()


def test_without_a_header(prov):
    text, w = INPUTS["synthetic"]()
    sm = S.Smoother(text, w)
    p = S.default_params(add_consensus=1)
    new = sm.smooth_maf_gfa(p, prov.provider(), device_text=prov.texter())
    old = sm.smooth_maf_gfa(p, prov.provider(), device_rows=True)
    assert new == old and new[1].startswith("a blocks=0 ")
    sm.close()


def test_three_chunks_give_the_same_bytes(prov, monkeypatch):
    text, w = INPUTS["synthetic"]()
    sm = S.Smoother(text, w)
    p = S.default_params(add_consensus=1)
    one, old, n1 = both(prov, sm, p)
    assert n1 == 1 and one == old
    monkeypatch.setenv("SXG_SMOOTH_CHUNK_BLOCKS", str(max(1, sm.n_blocks // 3)))
    many, old, n = both(prov, sm, p)
    assert n >= 3
    assert many == one == old
    sm.close()


def test_with_the_range_identity_provider_under_a(prov):
    text, w = INPUTS["inversion"]()
    sm = S.Smoother(text, w)
    p = S.default_params(add_consensus=1, adaptive_poa_params=1)
    calls = []

    def ident(blk_off, seq_off, bases, k, min_len, pct):
        calls.append(len(blk_off) - 1)
        n = len(blk_off) - 1
        used = [int(sum(seq_off[s + 1] - seq_off[s] >= min_len for s in range(blk_off[b], blk_off[b + 1]))) for b in range(n)]
        return used, [90] * n, [100] * n, [0] * n
    rid = S.python_range_identifier(ident)
    new, old, _ = both(prov, sm, p, identity=rid)
    assert calls and new == old
    sm.close()


def test_drb1_with_short_consensus_rows(prov):
    """DRB1 at -l 700, consensus on: 2161 blocks, 8 of them with a consensus row of fewer than 2 * padding letters (all gaps,
    size 0), most of one sequence."""
    sm = S.Smoother(open(DRB1).read(), discover=dict(target_poa_length=700, n_haps=12, max_path_jump=5000, max_edge_jump=5000))
    new, old, _ = both(prov, sm, S.default_params(add_consensus=1))
    assert new[1] == old[1] and new[0] == old[0] and new[2] == old[2] == 0
    assert new[1].count("\na ") >= 2000
    sm.close()


def test_fallbacks_never_call_the_texter(prov, monkeypatch):
    text = synthetic_gfa(6, n_paths=6, n_nodes=80)
    sm = S.Smoother(text, 90)
    p = S.default_params(add_consensus=1)
    prov.asked.clear()
    new = sm.smooth_maf_gfa(p, prov.provider(), merge_blocks=True, jaccard=0.0, header=HEADER, device_text=prov.texter())
    assert all(a[0] == 1 and a[1] == 0 for a in prov.asked) and prov.text_calls == prov.letters_calls == 0
    assert new == sm.smooth_maf_gfa(p, prov.provider(), merge_blocks=True, jaccard=0.0, header=HEADER)
    assert " merged=true" in new[1]
    monkeypatch.setenv("SXG_SMOOTH_LEGACY", "1")
    prov.asked.clear()
    leg = sm.smooth_maf_gfa(p, prov.provider(), header=HEADER, device_text=prov.texter())
    assert all(a[0] == 1 and a[1] == 0 for a in prov.asked) and prov.text_calls == prov.letters_calls == 0
    assert leg == sm.smooth_maf_gfa(p, prov.provider(), header=HEADER)
    sm.close()


def test_a_wrong_letter_count_names_the_block(prov):
    text, w = INPUTS["synthetic"]()
    sm = S.Smoother(text, w)
    g = SO.Graph(text)
    blocks = SO.blockset_by_path_windows(g, w)
    rows_before = sum(len(SO.collect(g, blk, 0.001).seqs) + 1 for blk in blocks[:3])
    prov.off_by_one = rows_before        # the first row of block 3
    with pytest.raises(S.SmoothError, match=r"contract of SXG_MSA_TRIMMED for block 3:"):
        sm.smooth_maf_gfa(S.default_params(add_consensus=1), prov.provider(), header=HEADER, device_text=prov.texter())
    assert prov.text_calls == 0
    sm.close()


def test_a_texter_that_fails_fails_the_call(prov):
    text, w = INPUTS["synthetic"]()
    sm = S.Smoother(text, w)
    prov.text_fails = True
    with pytest.raises(S.SmoothError, match="MAF text provider failed"):
        sm.smooth_maf_gfa(S.default_params(add_consensus=1), prov.provider(), header=HEADER, device_text=prov.texter())
    sm.close()


def test_the_existing_entry_points_write_what_they_wrote(prov):
    """The formatting functions were split for the text path: the legacy call, the device-rows call and the oracle stack agree on
    the same input as before (merged groups included), and a single block's MAF is the oracle's."""
    text = last_path_first(synthetic_gfa(1))
    sm = S.Smoother(text, 90)
    g = SO.Graph(text)
    blocks = SO.blockset_by_path_windows(g, 90)
    p = S.default_params(add_consensus=1)
    want = SO.smooth(g, blocks, add_consensus=True, merge=dict(merge_blocks=False, header=HEADER))
    for kw in (dict(), dict(device_rows=True)):
        got = sm.smooth_maf_gfa(p, prov.provider(), header=HEADER, **kw)
        assert got[1] == want[1] and got[0] == want[0] and got[2] == len(want[2])
    want = SO.smooth(g, blocks, add_consensus=True, merge=dict(merge_blocks=True, jaccard=0.0, header=HEADER))
    got = sm.smooth_maf_gfa(p, prov.provider(), merge_blocks=True, jaccard=0.0, header=HEADER)
    assert got[1] == want[1] and got[0] == want[0] and got[2] == len(want[2])
    sm.close()
