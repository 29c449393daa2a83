"""GPU: the trimmed MSA built on the device (want_msa = SXG_MSA_TRIMMED: msa_cols_kernel + msa_rows_kernel of poa_msa.hip.h)
against tests/msa_ref.py on top of the oracle, row for row, over hand-sized blocks in ONE batch -- and the MAF iteration that
uses it (Smoother.smooth_maf_gfa(..., device_rows=True)) against the legacy call on the same engine and the oracle stack."""
import os
import sys

import numpy as np
import pytest

from oracle import oracle_py as O
from oracle import smooth_oracle as SO
import smoothxg_amd as S
from smoothxg_amd import poa as P
from smoothxg_amd import smooth as SM

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import msa_ref  # noqa: E402
from helpers import random_block  # noqa: E402
from test_maf_device_rows_host import HEADER, last_path_first, oracle_maf_rows_total  # noqa: E402
from test_smooth_host import DRB1, inversion_gfa, synthetic_gfa  # noqa: E402

pytestmark = pytest.mark.gpu

SCORES = (1, -4, -6, -2, -26, -1)
SPOA = 0x10                      # SXG_ORDER_SPOA, what the host library asks for


def edit(rng, s, subs=(), ins=(), dels=()):
    """s with substitutions at `subs`, a random letter inserted in front of `ins`, the letters at `dels` removed."""
    out = []
    for k, b in enumerate(s.tolist()):
        if k in ins:
            out.append(int(rng.integers(0, 4)))
        if k in dels:
            continue
        out.append((b + 1) % 4 if k in subs else b)
    return np.asarray(out, np.uint8)


def make_batch(tile):
    """[(name, sequences, trim, mode, banded)]; the names say what a block is there for."""
    rng = np.random.default_rng(1405)
    B = []
    B.append(("one sequence of 40", [rng.integers(0, 4, 40, dtype=np.uint8)], 0, SPOA, 0))
    a = rng.integers(0, 4, 120, dtype=np.uint8)
    B.append(("two sequences, substitutions, an insertion and a deletion, trim 7",
              [a, edit(rng, a, subs=(30, 31, 77), ins=(50,), dels=(90, 91))], 7, SPOA, 0))
    B.append(("six sequences of about 300, trim 7", random_block(rng, 6, 300, div=0.08), 7, SPOA, 0))
    B.append(("six sequences of about 300, trim 0", random_block(rng, 6, 300, div=0.08), 0, SPOA, 0))
    B.append(("three sequences of about 700, trim 311", random_block(rng, 3, 700, div=0.05), 311, SPOA, 0))
    a = rng.integers(0, 4, 200, dtype=np.uint8)
    B.append(("indels inside the trimmed flanks: rows start at different columns",
              [edit(rng, a, ins=(2, 3, 4)), a, edit(rng, a, dels=(1, 2, 195)), edit(rng, a, ins=(197,), subs=(100,))], 10, SPOA, 0))
    a = rng.integers(0, 4, 90, dtype=np.uint8)
    n = a.copy()
    n[40] = 4
    B.append(("a block with an N", [a, n, edit(rng, n, subs=(10,))], 7, SPOA, 0))
    for w in (1, 15, 16, 17, 255, 257, tile + 1):
        a = rng.integers(0, 4, w + 10, dtype=np.uint8)
        B.append(("width %d" % w, [a, a.copy()], 5, SPOA, 0))
    B.append(("global alignment", random_block(rng, 3, 150, div=0.06), 7, SPOA | 1, 0))
    B.append(("incremental order, local", random_block(rng, 4, 130, div=0.06), 3, 0, 0))
    B.append(("adaptive band", random_block(rng, 3, 200, div=0.05), 7, 0, 2))
    B.append(("empty block", [], 0, SPOA, 0))
    B.append(("one sequence of 27000: too long", [rng.integers(0, 4, 27000, dtype=np.uint8)], 7, SPOA, 0))
    a = rng.integers(0, 4, 14, dtype=np.uint8)
    B.append(("every sequence exactly 2 * trim long", [a, edit(rng, a, subs=(5,))], 7, SPOA, 0))
    # runs of one work item that outgrow the window: the rows kernel's loop over windows
    a = rng.integers(0, 4, 600, dtype=np.uint8)
    sv = np.concatenate([a[:300], rng.integers(0, 4, tile + 900, dtype=np.uint8), a[300:]])
    B.append(("an insertion longer than the window in one sequence", [sv, edit(rng, a, subs=(40, 500)), edit(rng, a, subs=(310,), dels=(100,)), a.copy()],
              7, SPOA | 1, 0))
    a = rng.integers(0, 4, tile + 200, dtype=np.uint8)
    B.append(("a row with fewer than 2 * trim letters in a block wider than the window", [a, edit(rng, a, subs=(100, 2000)), a[1000:1020].copy()],
              11, SPOA, 0))
    B.append(("a last block behind the odd ones", random_block(rng, 2, 61, div=0.05), 2, SPOA, 0))
    return B


def flat(batch):
    seqs = [s for _, ss, _, _, _ in batch for s in ss]
    bases = np.concatenate(seqs) if seqs else np.zeros(0, np.uint8)
    seq_off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    blk_off = np.concatenate([[0], np.cumsum([len(ss) for _, ss, _, _, _ in batch])]).astype(np.int32)
    params = [S.Params(*SCORES, mode, banded) for _, _, _, mode, banded in batch]
    trims = np.asarray([t for _, _, t, _, _ in batch], np.int32)
    return bases, seq_off, blk_off, params, trims


@pytest.fixture(scope="module")
def geom(engine):
    """(CHUNK, TILE) of the rows kernel as the library was built: kept letters of a row per work item, bytes of its window."""
    return engine.msa_geometry()


@pytest.fixture(scope="module")
def batch(geom):
    return make_batch(geom[1])


def item_runs(text, chunk):
    """The runs of columns the work items of one trimmed row own: [(first column, end column, letter columns inside it)]."""
    at = [k for k, ch in enumerate(text) if ch != "-"]
    starts = [0] + [at[k] for k in range(chunk, len(at), chunk)]
    ends = starts[1:] + [len(text)]
    return [(a, z, [k for k in at if a <= k < z]) for a, z in zip(starts, ends)]


@pytest.fixture(scope="module")
def graphs(batch):
    """The oracle's POA graph of every block that has one (computed once, shared, never changed)."""
    out = []
    for name, seqs, trim, mode, banded in batch:
        ok = seqs and max(len(s) for s in seqs) <= P.MAX_SEQ_LEN
        out.append(O.block_run(seqs, None, O.mkparams(*SCORES, mode=mode, banded=banded))[0] if ok else None)
    return out


@pytest.fixture(scope="module")
def runs(engine, batch):
    """The batch through upload / execute / download: trimmed rows with and without consensus, no MSA, the full MSA."""
    bases, seq_off, blk_off, params, trims = flat(batch)
    r = {}
    for key, cons, msa in (("trim+cons", True, P.MSA_TRIMMED), ("trim", False, P.MSA_TRIMMED), ("none+cons", True, 0), ("full+cons", True, P.MSA_FULL)):
        r[key] = engine.run_flat(bases, seq_off, blk_off, None, params, want_consensus=cons, want_msa=msa, check=False, block_graph=3, bg_trim=trims)
    r["trim+cons, with paths"] = engine.run_flat(bases, seq_off, blk_off, None, params, want_consensus=True, want_msa=P.MSA_TRIMMED, check=False,
                                                 block_graph=1, bg_trim=trims)
    return r


@pytest.mark.parametrize("key", ["trim+cons", "trim", "trim+cons, with paths"])
def test_rows_equal_the_restatement(batch, graphs, runs, geom, key):
    cons = "cons" in key
    chunk, tile = geom
    seen_widths, starts_differ = set(), False
    split_run = gap_run = False     # a run longer than the window with letters in its first window and behind it; one without letters
    for b, (name, seqs, trim, mode, banded) in enumerate(batch):
        res = runs[key][b]
        if graphs[b] is None:
            assert res.status == (P.ST_TOO_LONG if seqs else 0), name
            assert not res.msa, name          # owns no bytes: its neighbours' rows are compared below
            continue
        assert res.status == 0, name
        want = msa_ref.trim_rows(graphs[b].msa(cons), trim)
        assert res.msa == want, name
        assert len(res.msa) == len(seqs) + (1 if cons else 0)
        seen_widths.add(len(want[0]))
        starts_differ |= len({len(r) - len(r.lstrip("-")) for r in want[:len(seqs)]}) > 1
        for r in want:
            for a, z, at in item_runs(r, chunk):
                if z - a > tile + 16:         # (a window starts up to 15 bytes in front of the run)
                    split_run |= bool(at) and at[0] - a < tile - 16 and at[-1] - a >= tile
                    gap_run |= not at
    assert {0, 1, 15, 16, 17, 255, 257, tile + 1} <= seen_widths
    assert starts_differ
    assert split_run and gap_run, "no work item's run outgrew the rows kernel's window"


def test_nothing_per_base_is_downloaded_and_the_block_graphs_are_the_same(batch, runs):
    for b, (name, seqs, trim, mode, banded) in enumerate(batch):
        a, z = runs["trim+cons"][b], runs["none+cons"][b]
        assert a.paths is None and a.node_code is None and a.node_rank is None and a.edge_tail is None and a.consensus is None, name
        assert (a.scores == z.scores).all() and a.status == z.status
        assert a.bg.node_seq == z.bg.node_seq and a.bg.edges == z.bg.edges, name
        assert len(a.bg.paths) == len(z.bg.paths) and all((x == y).all() for x, y in zip(a.bg.paths, z.bg.paths)), name
        assert (a.bg.consensus == z.bg.consensus).all(), name
        assert (a.bg.node_indeg == z.bg.node_indeg).all(), name
        w = runs["trim+cons, with paths"][b]      # want_block_graph = 1: everything is there, as without an MSA
        assert w.paths is not None and w.node_code is not None and w.msa == a.msa, name


def test_the_full_msa_is_what_it_was(batch, graphs, runs):
    for b, (name, seqs, trim, mode, banded) in enumerate(batch):
        if graphs[b] is not None:
            assert runs["full+cons"][b].msa == graphs[b].msa(True), name
            assert runs["full+cons"][b].paths is not None     # (the full MSA is formatted from the per-base paths)


def test_sharded_entry_refuses_the_trimmed_msa(engine, batch):
    bases, seq_off, blk_off, params, trims = flat(batch[:3])
    for ranks in (0, 2):
        with pytest.raises(P.PoaError, match="SXG_MSA_TRIMMED"):
            engine.run_flat_sharded(bases, seq_off, blk_off, None, params, want_msa=P.MSA_TRIMMED, simulate_ranks=ranks, block_graph=3, bg_trim=trims)
    assert engine.run_flat_sharded(bases, seq_off, blk_off, None, params, want_msa=P.MSA_FULL)[1].msa is not None


# ---- end to end: the MAF iteration over device rows
def iteration_case(engine, text, sm, blocks, pkw, okw):
    g = SO.Graph(text)
    p = SM.default_params(**pkw)
    new = sm.smooth_maf_gfa(p, SM.gpu_provider(engine), header=HEADER, device_rows=True)
    old = sm.smooth_maf_gfa(p, SM.gpu_provider(engine), header=HEADER)
    assert new[1] == old[1] and new[2] == old[2] == 0 and new[0] == old[0]
    out = SO.Graph(new[0])
    for q, nm in enumerate(g.pname):          # every input path is spelt by the output
        assert out.path_sequence(out.pname.index(nm)) == g.path_sequence(q)
    if okw is not None:
        want = SO.smooth(g, blocks, merge=dict(merge_blocks=False, header=HEADER), **okw)
        assert new[1] == want[1] and new[2] == len(want[2]) and new[0] == want[0]
    return new


@pytest.mark.parametrize("seed", [0, 1])
def test_iteration_with_groomed_blocks(engine, seed):
    text = last_path_first(synthetic_gfa(seed))
    sm = SM.Smoother(text, 90)
    iteration_case(engine, text, sm, SO.blockset_by_path_windows(SO.Graph(text), 90), dict(add_consensus=1), dict(add_consensus=True))
    sm.close()


def test_iteration_with_a_block_collected_in_reverse(engine):
    text = inversion_gfa(3, length=2400, lo=800, hi=1600)
    sm = SM.Smoother(text, 800)
    iteration_case(engine, text, sm, SO.blockset_by_path_windows(SO.Graph(text), 800), dict(add_consensus=1), dict(add_consensus=True))
    sm.close()


@pytest.mark.parametrize("cons", [0, 1])
def test_iteration_on_drb1_windows_of_900(engine, cons):
    text = open(DRB1).read()
    sm = SM.Smoother(text, 900)
    iteration_case(engine, text, sm, SO.blockset_by_path_windows(SO.Graph(text), 900), dict(add_consensus=cons), dict(add_consensus=bool(cons)))
    sm.close()


def drb1_discovered():
    text = open(DRB1).read()
    g = SO.Graph(text)
    blocks = SO.break_blocks(g, SO.smoothable_blocks(g, 700 * 12, 700, 5000, 5000), 1400)
    return text, g, blocks, SM.Smoother(text, discover=dict(target_poa_length=700, n_haps=12, max_path_jump=5000, max_edge_jump=5000))


def test_iteration_on_drb1_discovered_blocks_equals_the_legacy_call(engine):
    """2161 blocks, most of one sequence; 8 have a consensus row of fewer than 2 * 311 letters, which is all gaps."""
    text, g, blocks, sm = drb1_discovered()
    new = iteration_case(engine, text, sm, blocks, dict(add_consensus=1), None)
    assert new[1].count("\na ") + new[1].startswith("a ") >= 2000
    sm.close()


def test_iteration_on_drb1_discovered_blocks_equals_the_oracle(engine, monkeypatch):
    """All 2161 blocks against the oracle stack; SO.maf_rows completed for the 8 consensus rows it cannot format (fewer than
    2 * 311 letters; oracle_maf_rows_total of tests/test_maf_device_rows_host.py)."""
    monkeypatch.setattr(SO, "maf_rows", oracle_maf_rows_total)
    text, g, blocks, sm = drb1_discovered()
    want = SO.smooth(g, blocks, add_consensus=True, merge=dict(merge_blocks=False, header=HEADER))
    new = sm.smooth_maf_gfa(SM.default_params(add_consensus=1), SM.gpu_provider(engine), header=HEADER, device_rows=True)
    assert new[1] == want[1] and new[2] == len(want[2]) and new[0] == want[0]
    sm.close()
