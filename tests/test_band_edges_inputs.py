"""tests/band_edges.py without a GPU: the inputs of tests/test_gpu_band_edges.py regenerate with the lengths their edges need, and
the ORACLE's graphs say that they reach the states of the banded sweep they are built for -- rows without a band, a full window
that re-centres, stored predecessors from earlier window origins, the strip left of the window, three and more predecessors,
tied end cells.  (The 65 536-row block is asserted where it runs: its oracle pass takes ~10 s.)"""
import numpy as np

import band_edges as B


def test_lengths_and_strip_widths():
    assert [B.strip_width(L) for L in (1, 2266, 2267, 6466, 6467, 26623)] == [6, 6, 8, 8, 11, 11]
    for top, n in ((2266, 3), (2267, 3), (6466, 2), (6467, 2)):
        blk = B.width_change_block(top, n)
        assert [len(s) for s in blk] == [top, top - 40, top][:n]
        assert all((x == y).all() for x, y in zip(blk, B.width_change_block(top, n)))          # (seeded: the same again)
        assert 40 <= (top // 2) / int((blk[0][:top // 2] != blk[1][:top // 2]).sum()) <= 60      # SNPs every ~50 letters
    blk = B.long_first_block()
    assert [len(s) for s in blk] == [6500, 900, 300, 600, 450]
    for k in (5, 127, 128):
        assert [len(s) for s in B.last_strip_block(k)] == [6 * k + 1, 6 * k, 6 * k - 1, 6 * k + 1, 6 * k]
    # k = 127: column L = 762 is alone in strip 127, the last of the window at origin 0; k = 128: strip 128 lies outside it
    assert 762 // 6 == B.WIN - 1 and 768 // 6 == B.WIN
    assert [len(b) for b in B.tiny_blocks()] == [3, 3, 1, 0] and len(B.tiny_blocks()[0][1]) == 1
    assert [len(s) for s in B.epoch_block()] == [18000, 17900, 17800, 17700, 1200]


def test_rows_without_a_band(oracle):
    for at_end in (0, 1):
        blk = B.empty_band_block(at_end)
        assert [len(s) for s in blk] == [2000, 100, 2000]
        facts = B.check_empty_bands(oracle, blk)
        # every row whose backbone coordinate exceeds L + w (plus the rest of its strip) has no band: 2 000 - 415 rows
        assert facts[0]["empty"] == 2000 - (100 + B.half_width(100) + 1)
        if at_end:
            g, sc, _ = oracle.block_run(blk, None, oracle.mkparams(*B.DEFAULT, mode=0, banded=1))
            assert sc[1] < 20 and g.n_nodes > 2080


def test_a_full_window_that_moves(oracle):
    for ins in (300, 420):
        blk = B.moving_window_block(ins)
        facts = B.check_moving_window(oracle, blk)
        print(ins, facts[-1])
        sc = [oracle.block_run(blk, None, oracle.mkparams(*B.DEFAULT, mode=0, banded=b))[1] for b in (0, 1, 2)]
        if ins == 300:
            assert (sc[1] == sc[0]).all() and (sc[2] == sc[0]).all()
        else:
            assert sc[1][1] < sc[0][1] == sc[2][1]


def test_tied_end_cells(oracle):
    for banded in (1, 2):
        B.check_ties(oracle, banded)


def test_the_window_rule_on_a_chain():
    """sweep_facts on a plain chain with its own column as the coordinate: the counts follow from the rule by hand"""
    n = 2266
    off = np.concatenate([[0, 0], np.arange(1, n)]).astype(np.int32)       # (row 1 has no predecessor, row i has row i - 1)
    f = B.sweep_facts((None, off, np.arange(1, n, dtype=np.int32), None, None), np.arange(1, n + 1), n, 6)
    assert (f["empty"], f["np3"], f["stored_moved"], f["left_read"]) == (0, 0, 0, 0)
    # w = 378: the band is whole from x = 378 to x = 1 888 and moves one strip every six rows; a window of 128 strips holds a
    # band of 127 for two moves and one of 128 for one
    assert 120 <= f["recentres"] <= 260
    assert f["cells"] == sum(min(n, (min((x + 378) // 6, n // 6)) * 6 + 5) - (max(x - 378, 0) // 6) * 6 + 1 for x in range(1, n + 1))
