"""CPU: sxg_blockset_split (the splitting half of break_blocks, src/breaks.cpp:335-586; decree P3 of DESIGN.md section 9)
with a ctypes-callback split provider backed by tests/split_ref.py, against P3 in plain Python on synthetic graphs."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_ref as R  # noqa: E402
import split_synth as Y  # noqa: E402
from smoothxg_amd import poa as P  # noqa: E402
from smoothxg_amd import smooth as S  # noqa: E402


class RefSplitter:
    """sxg_poa_split_batch-shaped callback backed by split_ref.greedy."""

    def __init__(self, spoil=None):
        self.keep, self.calls, self.spoil = [], 0, spoil
        self.run = S.SPLIT_FN(self._run)
        self.free = S.SPLIT_FREE_FN(lambda pout: None)

    def splitter(self):
        return C.cast(self.run, C.c_void_p), C.cast(self.free, C.c_void_p), None

    def _run(self, ctx, pin, pout):
        self.calls += 1
        i, o = pin.contents, pout.contents
        nb = i.n_blocks
        blk = np.ctypeslib.as_array(i.blk_off, (nb + 1,)).copy()
        ns = int(blk[-1])
        so = np.ctypeslib.as_array(i.seq_off, (ns + 1,)).copy()
        bases = np.ctypeslib.as_array(i.bases, (int(so[-1]),)).copy()
        grp, ngs, nps = [], [], []
        for b in range(nb):
            seqs = [bases[so[s]:so[s + 1]] for s in range(blk[b], blk[b + 1])]
            assert all(len(x) <= len(y) for x, y in zip(seqs, seqs[1:]))      # sorted by length
            g, ng, npairs = R.greedy(seqs, i.identity[b], i.length_ratio_min[b])
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


def family_block(seed, n_fam, per_fam, length=90, within=1, across=25):
    rng = np.random.default_rng(seed)
    fam = Y.families(rng, n_fam, per_fam, length, within, across, indel_every=3)
    order = rng.permutation(len(fam))
    return [fam[k][1] for k in order]


def all_ranges(sm):
    return [sm.block_ranges(k) for k in range(sm.n_blocks)]


def expected(ranges, seqs, t, ratio, depth):
    """P3 in Python on every block: the new blockset as lists of (path, begin, end)."""
    out = []
    for rg, sq in zip(ranges, seqs):
        parts, _ = R.split_block(sq, t, ratio, depth)
        out += [[rg[r] for r in part] for part in parts]
    return out


def run_split(blocks, t, ratio=0.0, depth=1, spoil=None):
    text, ranges, seqs = Y.blocks_gfa(blocks)
    sm = S.Smoother(text, blocks=ranges)
    prov = RefSplitter(spoil)
    n_split, n_long = sm.split_blocks(prov.splitter(), t, ratio, depth)
    got = [[r[:3] for r in blk] for blk in all_ranges(sm)]
    return sm, got, expected(ranges, seqs, t, ratio, depth), n_split, n_long, prov, ranges


def test_duplicates_and_reverse_complement_duplicates():
    blk = family_block(1, 2, 3)
    blk.insert(3, blk[0].copy())            # an exact duplicate
    blk.append(R.revcomp(blk[1]))           # a reverse-complement duplicate
    sm, got, want, n_split, n_long, prov, ranges = run_split([blk], 0.9)
    assert got == want and len(got) == 2 and (n_split, n_long) == (1, 0) and prov.calls == 1
    where = {r: k for k, b in enumerate(got) for r in b}
    assert where[ranges[0][3]] == where[ranges[0][0]]               # a duplicate goes where its first occurrence goes
    assert where[ranges[0][len(blk) - 1]] == where[ranges[0][1]]
    b0 = got[where[ranges[0][0]]]
    assert b0.index(ranges[0][3]) == b0.index(ranges[0][0]) + 1      # ... right behind it: original ranks in original order


def test_min_dedup_depth_zero_changes_nothing():
    blk = family_block(2, 2, 3)
    sm, got, want, n_split, n_long, prov, ranges = run_split([blk], 0.9, depth=0)
    assert got == [ranges[0]] == want and n_split == 0 and prov.calls == 0


def test_depth_below_the_minimum_and_identity_zero():
    blk = family_block(3, 2, 3)
    blk.append(blk[0].copy())               # 7 ranges, 6 after dedup
    assert run_split([blk], 0.9, depth=7)[1] == [run_split([blk], 0.9, depth=7)[6][0]]
    sm, got, want, n_split, _, prov, ranges = run_split([blk], 0.9, depth=6)
    assert got == want and n_split == 1 and len(got) == 2
    sm, got, want, n_split, _, prov, ranges = run_split([blk], 0.0, depth=1)     # the outer guard: identity 0 = off
    assert got == [ranges[0]] and prov.calls == 0


def test_one_group_leaves_the_block_unchanged():
    blk = family_block(4, 1, 6)
    sm, got, want, n_split, _, prov, ranges = run_split([blk], 0.9)
    assert got == [ranges[0]] == want and n_split == 0 and prov.calls == 1


def test_three_groups_in_group_and_range_order():
    blk = family_block(5, 3, 3, length=100)
    sm, got, want, n_split, _, prov, ranges = run_split([blk], 0.9)
    assert got == want and len(got) == 3 and n_split == 1
    srt, ranks = R.dedup_sort(blk)
    grp, ng, _ = R.greedy(srt, 0.9, 0.0)
    assert ng == 3
    for g in range(3):                       # group order = order of creation; members in insertion order
        assert got[g] == [ranges[0][r] for q in range(len(srt)) if grp[q] == g for r in ranks[q]]


def test_length_ratio_min_reaches_the_provider():
    rng = np.random.default_rng(6)
    long_ = rng.integers(0, 4, 100).astype(np.uint8)
    blk = [long_, long_[:60].copy(), Y.mutate(rng, long_, 1)]
    sm, got, want, n_split, _, prov, ranges = run_split([blk], 0.5, ratio=0.9)
    assert got == want and len(got) == 2     # the short one is never compared with the long ones


def test_consecutive_renumbering_across_blocks():
    blocks = [family_block(7, 2, 3), family_block(8, 1, 4), family_block(9, 3, 2, length=100), family_block(10, 1, 1) * 1]
    sm, got, want, n_split, n_long, prov, ranges = run_split(blocks, 0.9)
    assert got == want and n_split == 2 and prov.calls == 1
    assert len(got) == 2 + 1 + 3 + 1
    assert got[2] == ranges[1] and got[6] == ranges[3]
    assert sorted(r for b in got for r in b) == sorted(r for b in ranges for r in b)     # the multiset of ranges is preserved
    assert sorted(r for b in got[:2] for r in b) == sorted(ranges[0])
    assert sorted(r for b in got[3:6] for r in b) == sorted(ranges[2])


def test_provider_with_a_group_id_out_of_range_is_refused():
    blk = family_block(11, 2, 3)
    text, ranges, _ = Y.blocks_gfa([blk])
    sm = S.Smoother(text, blocks=ranges)
    with pytest.raises(S.SmoothError, match="group id out of range"):
        sm.split_blocks(RefSplitter("group").splitter(), 0.9, 0.0, 1)
    assert [r[:3] for r in sm.block_ranges(0)] == ranges[0]          # the blockset is still the old one


def test_failed_block_stays_whole_and_is_counted():
    blocks = [family_block(12, 2, 3), family_block(13, 2, 3)]
    sm, got, want, n_split, n_long, prov, ranges = run_split(blocks, 0.9, spoil="status")
    assert (n_split, n_long) == (1, 1) and got[0] == ranges[0] and got[1:] == want[2:]


def test_split_blockset_smooths_to_a_valid_gfa():
    from test_smooth_host import OracleProvider
    blocks = [family_block(14, 2, 3, length=120), family_block(15, 1, 4, length=80)]
    text, ranges, _ = Y.blocks_gfa(blocks)
    sm = S.Smoother(text, blocks=ranges)
    assert sm.split_blocks(RefSplitter().splitter(), 0.9, 0.0, 1) == (1, 0) and sm.n_blocks == 3
    out = sm.smooth_gfa(S.default_params(), OracleProvider().provider())
    import gfa_invariants as GI
    GI.check_laced(out, text)               # every path spells its input sequence, edges == walked pairs, unchopped
