"""CPU: sxg_blockset_split_mash (the splitting half of break_blocks with its mash-based branch, src/breaks.cpp:335-586; decrees
M1-M5 of DESIGN.md section 9) with a ctypes-callback mash split provider backed by tests/split_mash_ref.py, against the
restatement in plain Python on synthetic graphs."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_mash_ref as M  # noqa: E402
import split_ref as R  # noqa: E402
import split_synth as Y  # noqa: E402
from smoothxg_amd import poa as P  # noqa: E402
from smoothxg_amd import smooth as S  # noqa: E402
from test_split_host import RefSplitter, all_ranges, family_block  # noqa: E402


class RefMashSplitter:
    """sxg_poa_split_mash_batch-shaped callback backed by split_mash_ref.greedy_mash; remembers what it was given."""

    def __init__(self, spoil=None):
        self.keep, self.calls, self.spoil, self.seen = [], 0, spoil, []
        self.run = S.SPLIT_MASH_FN(self._run)
        self.free = S.SPLIT_FREE_FN(lambda pout: None)

    def splitter(self):
        return C.cast(self.run, C.c_void_p), C.cast(self.free, C.c_void_p), None

    def _run(self, ctx, pin, pmash, pout, pnmash):
        self.calls += 1
        i, m, o = pin.contents, pmash.contents, pout.contents
        nb = i.n_blocks
        blk = np.ctypeslib.as_array(i.blk_off, (nb + 1,)).copy()
        ns = int(blk[-1])
        so = np.ctypeslib.as_array(i.seq_off, (ns + 1,)).copy()
        bases = np.ctypeslib.as_array(i.bases, (int(so[-1]),)).copy()
        grp, ngs, nps = [], [], []
        for b in range(nb):
            seqs = [bases[so[s]:so[s + 1]] for s in range(blk[b], blk[b + 1])]
            self.seen.append((len(seqs), m.kmer_size, m.min_len[b], m.est_identity[b]))
            g, ng, npairs, _ = M.greedy_mash(seqs, i.identity[b], i.length_ratio_min[b], m.kmer_size, m.min_len[b], m.est_identity[b])
            grp += g
            ngs.append(ng)
            nps.append(npairs)
        arrs = dict(group=np.asarray(grp, np.int32), n_groups=np.asarray(ngs, np.int32), n_pairs=np.asarray(nps, np.int64),
                    status=np.zeros(nb, np.int32))
        if self.spoil == "group":
            arrs["group"][-1] = arrs["n_groups"][-1]
        if self.spoil == "status":
            arrs["status"][0] = P.ST_TOO_LONG
        self.keep.append(arrs)
        o.n_blocks, o.n_seqs = nb, ns
        o.group = arrs["group"].ctypes.data_as(C.POINTER(C.c_int32))
        o.n_groups = arrs["n_groups"].ctypes.data_as(C.POINTER(C.c_int32))
        o.n_pairs = arrs["n_pairs"].ctypes.data_as(C.POINTER(C.c_int64))
        o.status = arrs["status"].ctypes.data_as(C.POINTER(C.c_int32))
        return -4 if self.spoil == "status" else 0


def expected(ranges, seqs, t, ratio, depth, min_len, min_depth, e, k):
    out = []
    for rg, sq in zip(ranges, seqs):
        parts, _, _ = M.split_block_mash(sq, t, ratio, depth, min_len, min_depth, e, k)
        out += [[rg[r] for r in part] for part in parts]
    return out


def run_mash(blocks, t, ratio=0.0, depth=1, min_len=200, min_depth=0, e=0.0, k=17, spoil=None):
    text, ranges, seqs = Y.blocks_gfa(blocks)
    sm = S.Smoother(text, blocks=ranges)
    prov = RefMashSplitter(spoil)
    n_split, n_long = sm.split_blocks_mash(prov.splitter(), t, ratio, depth, min_len, min_depth, e, k)
    got = [[r[:3] for r in blk] for blk in all_ranges(sm)]
    return sm, got, expected(ranges, seqs, t, ratio, depth, min_len, min_depth, e, k), n_split, n_long, prov, ranges


def long_block(seed, n_fam, per_fam):
    return family_block(seed, n_fam, per_fam, length=260, within=2, across=50)


def test_min_len_zero_is_the_split_without_the_branch():
    blocks = [family_block(7, 2, 3), family_block(8, 1, 4), long_block(9, 3, 2), family_block(10, 1, 1)]
    sm, got, want, n_split, n_long, prov, ranges = run_mash(blocks, 0.9, min_len=0)
    text, ranges2, _ = Y.blocks_gfa(blocks)
    plain = S.Smoother(text, blocks=ranges2)
    counts = plain.split_blocks(RefSplitter().splitter(), 0.9, 0.0, 1)
    assert [[r[:3] for r in b] for b in all_ranges(plain)] == got == want and counts == (n_split, n_long) and prov.calls == 1
    assert all(s[2] == 0 for s in prov.seen)


def test_depth_switch_one_block_at_the_cut_and_one_below():
    at, below = long_block(20, 2, 3), long_block(21, 2, 3)[:5]            # 6 and 5 dedup'd sequences, cut at 6
    sm, got, want, n_split, n_long, prov, ranges = run_mash([at, below], 0.95, min_len=200, min_depth=6, e=0.99)
    assert got == want and prov.calls == 1
    assert [(s[0], s[2]) for s in prov.seen] == [(6, 200), (5, 0)]        # M2: the host decides per block
    assert all(s[1] == 17 and s[3] == 0.99 for s in prov.seen)
    # the two rules do split these blocks differently: e = 0.99 on sets keeps nobody together, the edit rule at 0.95 does
    assert len(expected([ranges[0]], [at], 0.95, 0.0, 1, 200, 6, 0.99, 17)) == 6
    assert len(expected([ranges[1]], [below], 0.95, 0.0, 1, 200, 6, 0.99, 17)) == 2
    assert sorted(r for b in got for r in b) == sorted(r for b in ranges for r in b)     # the multiset of ranges is preserved


def test_est_identity_defaults_to_the_group_identity_and_depth_zero_means_every_block():
    sm, got, want, n_split, n_long, prov, ranges = run_mash([long_block(22, 2, 3)], 0.95, min_len=200, min_depth=0, e=0.0)
    assert got == want and len(got) == 2 and prov.seen == [(6, 17, 200, 0.95)]
    where = {r: k for k, b in enumerate(got) for r in b}
    assert len(where) == 6


def test_bad_parameters_are_rejected():
    blk = long_block(23, 2, 3)
    text, ranges, _ = Y.blocks_gfa([blk])
    sm = S.Smoother(text, blocks=ranges)
    prov = RefMashSplitter()
    for kw, msg in ((dict(min_len_mash=16), "at least kmer_size"), (dict(kmer_size=33), "kmer_size"), (dict(kmer_size=0), "kmer_size"),
                    (dict(est_identity=1.5), "est_identity")):
        with pytest.raises(S.SmoothError, match=msg):
            sm.split_blocks_mash(prov.splitter(), 0.95, 0.0, 1, **dict(dict(min_len_mash=200, min_depth_mash=0), **kw))
    assert prov.calls == 0 and [r[:3] for r in sm.block_ranges(0)] == ranges[0]


def test_spoiled_provider_is_refused_and_a_failed_block_stays_whole():
    blk = long_block(24, 2, 3)
    text, ranges, _ = Y.blocks_gfa([blk])
    sm = S.Smoother(text, blocks=ranges)
    with pytest.raises(S.SmoothError, match="group id out of range"):
        sm.split_blocks_mash(RefMashSplitter("group").splitter(), 0.95, 0.0, 1, 200, 0)
    assert [r[:3] for r in sm.block_ranges(0)] == ranges[0]
    sm, got, want, n_split, n_long, prov, ranges = run_mash([long_block(25, 2, 3), long_block(26, 2, 3)], 0.95, spoil="status")
    assert (n_split, n_long) == (1, 1) and got[0] == ranges[0] and got[1:] == want[2:]
