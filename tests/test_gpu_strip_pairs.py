"""The packed sweep with ADJACENT strips in a lane (poa_dp16.hip.h, round 10), against the oracle bit for bit, on blocks whose
in-row gaps span many strips and cross every kind of boundary the carries and the hand-over treat differently:

  * an odd/even strip boundary, column (2 l + 1) W of a wave: inside a lane -- the high strip takes its lane's own low strip;
  * a lane boundary, column 2 l W: the lane shift of the scan and of the hand-over;
  * column 64 W of a wave: where the low and the high halves used to be stitched together;
  * a wave edge, column 128 W: the mailbox.

A block is six sequences from one random ancestor with 2 % substitutions.  The FIRST carries a 40-base and a 300-base deletion:
the second sequence, aligned to it, opens in-row gaps of those lengths at the deleted columns.  The THIRD carries an insertion
of each size.  Under the convex scores the 300-base gaps are cheaper by the second gap piece (Q / O), the 40-base gaps by the
first (E / F).  One block per wave count of the packed sweep (1, 2, 3, 4 and 8 waves), and for four waves also the longest
sequence that still fits 128 NW W columns and the first that does not.

The one-wave block has 1 535 letters (12 columns per strip), not the ~255 a smallest one-wave class would take: a sequence that
short cannot hold two 300-base gaps with flanks that outweigh them.  Which class really ran is asserted from the engine's
statistics (threads, columns per lane, row mode); packed_geometry below only documents how the lengths were chosen."""
import numpy as np
import pytest

from helpers import assert_block_equal
from smoothxg_amd import Params

SCORES = {
    # name: ((m, n, g, e, q, c), alignment mode)
    "local_default": ((1, -4, -6, -2, -26, -1), 0),      # the default-score classes
    "local_convex_other": ((1, -3, -5, -2, -20, -1), 0),  # the general classes, 2-byte cells
    "global_affine": ((1, -4, -6, -2, -6, -2), 1),
    "global_4byte_cells": ((1, -19, -39, -3, -81, -1), 1),   # deltas that do not fit the 2-byte plane code
}


def packed_geometry(length):
    """(NW, W) of the packed sweep for a block whose longest sequence has `length` letters: poa_classes.h::variant_for_len
    restated (fewest padded columns; of two equal, the wider strip)."""
    best = None
    for W in (13, 12, 11, 10, 9, 8, 7, 6, 5, 4):
        for NW in (1, 2, 3, 4, 8, 12, 16):
            cols = 128 * NW * W
            if cols < length + 1:
                continue
            if W == 13 or (W < 8 and NW > 4) or (W > 8 and NW > 8):   # (13 columns: only the 16-wave local classes, not reached here)
                break
            if best is None or cols < best[0]:
                best = (cols, NW, W)
            break
    return best[1], best[2]


# longest sequence of the block -> the geometry it must run on
LENGTHS = {1535: (1, 12), 2800: (2, 11), 3400: (3, 9), 5100: (4, 10), 128 * 4 * 11 - 1: (4, 11), 128 * 4 * 11: (4, 12), 9000: (8, 9)}


def test_lengths_reach_the_classes_they_are_meant_for():
    for L, geo in LENGTHS.items():
        assert packed_geometry(L) == geo, (L, packed_geometry(L))


# seed of each block: the first for which the oracle's alignments hold all four gaps UNDIVIDED under every score set the block
# runs with (under the affine scores a substitution or a chance match next to a gap's end splits a few columns off it)
SEEDS = {**{L: 0 for L in LENGTHS}, 1535: 2, 5100: 1}


def gap_block(L, seed=None):
    """The six sequences and the gaps' intended query columns, for a block whose longest sequences have exactly L letters.
    The ancestor has L letters; the insertion carrier is its first L - 340 letters with 340 inserted (what it lacks at the
    end is no in-row gap: a local alignment stops short, a global one ends in a run of skipped rows)."""
    NW, W = LENGTHS[L]
    rng = np.random.default_rng([L, SEEDS[L] if seed is None else seed])
    anc = rng.integers(0, 4, L, dtype=np.uint8)

    def mutated():
        s = anc.copy()
        at = rng.random(L) < 0.02
        s[at] = (s[at] + rng.integers(1, 4, int(at.sum()))) % 4
        return s

    def nearest(x, step, phase):   # the column phase + k * step nearest to x
        return phase + step * int(round((x - phase) / step))

    d300 = 64 * W + 128 * W * ((NW - 1) // 2)           # the old half boundary of a middle wave
    d40 = nearest((d300 - 150) // 2, 2 * W, W)           # an odd/even strip boundary in the flank left of it
    i300 = 128 * W * (NW // 2) if NW > 1 else 64 * W     # a wave edge (one wave has none)
    i40 = nearest((i300 + 150 + L) // 2, 2 * W, 0)       # a lane boundary in the flank right of it
    plain = [mutated() for _ in range(5)]
    keep = np.ones(L, bool)
    keep[d300 - 150:d300 + 150] = False
    keep[d40 - 20:d40 + 20] = False
    del_carrier = plain[0][keep]
    # the insertion carrier: its own coordinates are the query columns, so the ancestor is cut where the insertions END UP
    a, b = sorted([(i40 - 20, 40), (i300 - 150, 300)])
    src = plain[1][:L - 340]
    cut1 = a[0]
    cut2 = b[0] - a[1]
    ins_carrier = np.concatenate([src[:cut1], rng.integers(0, 4, a[1], dtype=np.uint8), src[cut1:cut2],
                                  rng.integers(0, 4, b[1], dtype=np.uint8), src[cut2:]])
    assert len(ins_carrier) == L and len(del_carrier) == L - 340
    seqs = [del_carrier, plain[2], ins_carrier, plain[3], plain[4], mutated()]
    return seqs, dict(d300=d300, d40=d40, i300=i300, i40=i40, NW=NW, W=W)


def interior_private_runs(path, shared):
    """Lengths of the runs of consecutive path nodes outside `shared` that have shared nodes on both sides."""
    inside = np.isin(path, shared)
    runs, n, seen = [], 0, False
    for x in inside.tolist():
        if x:
            if seen and n:
                runs.append(n)
            seen, n = True, 0
        else:
            n += 1
    return runs


def assert_gaps_are_in_the_alignment(g, label):
    """From the ORACLE's graph: the second sequence passes >= 300 (and, elsewhere, >= 40) consecutive nodes that the deletion
    carrier's path skips, between nodes the two share; the insertion carrier does the same against the two sequences before
    it.  (2 % substitutions make runs of one or two; an alignment that gave a flank up instead of bridging the gap leaves its
    private nodes at an END of the path, which does not count.)"""
    p0, p1, p2 = g.seq_path(0), g.seq_path(1), g.seq_path(2)
    for who, runs in (("deletion", interior_private_runs(p1, p0)), ("insertion", interior_private_runs(p2, np.concatenate([p0, p1])))):
        big = [r for r in runs if r >= 300]
        mid = [r for r in runs if 40 <= r < 300]
        assert len(big) == 1 and len(mid) >= 1, f"{label}: {who} gaps not in the oracle's alignment: runs {sorted(runs)[-4:]}"


def cases():
    out = []
    for name in SCORES:
        for L in LENGTHS:
            if name == "global_affine" and L > 128 * 4 * 11:
                continue
            if name == "global_4byte_cells" and L > 2800:
                continue
            out.append(pytest.param(name, L, id=f"{name}-{L}"))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,L", cases())
def test_multi_strip_gaps_across_lane_half_and_wave_boundaries(engine, oracle, monkeypatch, name, L):
    monkeypatch.setenv("SXG_POA_NO_SPREAD", "1")   # (a one-block batch would otherwise be spread over twice the waves)
    (m, n, gg, e, q, c), mode = SCORES[name]
    seqs, where = gap_block(L)
    g, sc, cells = oracle.block_run(seqs, None, oracle.mkparams(m, n, gg, e, q, c, mode=mode))
    assert_gaps_are_in_the_alignment(g, f"{name}/{L}")
    res = engine.run_blocks([seqs], Params(m, n, gg, e, q, c, mode, 0))
    st = engine.stats()
    print(f"{name} L={L} geometry {where['NW']} waves x {where['W']} columns, gaps at {where}, scores {sc.tolist()}, "
          f"ran {st['dom_threads']} threads x {st['dom_cols_per_lane']} columns per lane, row mode {st['dom_row_mode']}, retries {st['retries']}")
    assert st["dom_row_mode"] == 2, st                                   # the packed sweep did it ...
    assert (st["dom_threads"], st["dom_cols_per_lane"]) == (64 * where["NW"], 2 * where["W"]), st   # ... on the class meant
    assert_block_equal(res[0], g, sc, cells, label=f"{name}/{L}")
