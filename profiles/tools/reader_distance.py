#!/usr/bin/env python3
"""How far ahead the readers of the packed sweep's stored rows lie (CPU only, needs `make -C oracle`): what decides how many
stored rows the on-chip copies keep out of the HBM ring.

    python profiles/tools/reader_distance.py [--blocks 0,1,2] [--seqs 64] [--length 5000] [--global]

Builds each block's graph with the CPU oracle in spoa's node order after 8, 16, ... sequences and reads the row CSR the sweep
walks (Graph.rows(): rows in sweep order, predecessors as 1-based rows, 0 = the virtual start row).  A row is STORED when a
successor other than the next row reads it.  For a stored row r, cnt = the stored rows in [r, last reader of r): the quantity
finish_rows (smoothxg_amd/csrc/poa_graph_dev.h) compares with lds_rows -- the row stays on chip iff cnt <= lds_rows.  Rows
print the cumulative share of stored rows and of stored-row reads (by the stored rows between the row read and its reader)
up to each cnt, and the share of reads whose row stays on chip with lds_rows = cnt."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import oracle_py as O  # noqa: E402
from smoothxg_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", default="0,1,2", help="block ids of the synthetic generator")
    ap.add_argument("--seqs", type=int, default=64)
    ap.add_argument("--length", type=int, default=5000)
    ap.add_argument("--global", dest="glob", action="store_true", help="global alignment (default: local)")
    a = ap.parse_args()
    p = O.mkparams(1, -4, -6, -2, -26, -1, mode=(0 if not a.glob else 1) | 0x10)
    impl = O.IMPL_AVX2 if O.simd_available() else O.IMPL_SCALAR
    rows = stored = regpred = multi = reads = 0
    hist_rows = np.zeros(66, np.int64)    # stored rows by cnt (65 = more)
    hist_reads = np.zeros(66, np.int64)   # stored-row reads by the stored rows between the row read and its reader
    hist_onchip = np.zeros(66, np.int64)  # stored-row reads by the cnt of the row read: on chip iff that cnt <= lds_rows
    for blk in (int(b) for b in a.blocks.split(",")):
        seqs = synth.make_block(blk, a.seqs, a.length)
        for k in sorted(set(list(range(8, a.seqs, 8)) + [a.seqs - 1])):
            g, _, _ = O.block_run(seqs[:k], None, p, impl=impl)
            _, off, pred, _, _ = g.rows()
            n = len(off) - 1
            last = np.full(n + 1, -1)
            nonadj = np.zeros(n + 1, bool)
            for r in range(1, n + 1):
                for x in pred[off[r - 1]:off[r]]:
                    if x != r - 1:
                        nonadj[x] = True
                    last[x] = max(last[x], r)
            nonadj[0] = False
            sseq = np.concatenate([[0], np.cumsum(nonadj)])   # stored rows among rows 0 .. r-1
            cnt = np.zeros(n + 1, np.int64)
            for r in range(1, n + 1):
                if nonadj[r]:
                    cnt[r] = sseq[last[r]] - sseq[r]
                    hist_rows[min(cnt[r], 65)] += 1
            for r in range(1, n + 1):
                ps = pred[off[r - 1]:off[r]]
                rows += 1
                stored += int(nonadj[r])
                regpred += int(len(ps) == 1 and ps[0] == r - 1)
                multi += int(len(ps) >= 2)
                for x in ps:
                    if x != r - 1 and x != 0:
                        reads += 1
                        hist_reads[min(sseq[r] - sseq[x], 65)] += 1
                        hist_onchip[min(cnt[x], 65)] += 1
    print("rows %d: stored %.1f %%, only the register predecessor %.1f %%, two or more predecessors %.1f %%, "
          "stored-row reads per row %.2f" % (rows, 100.0 * stored / rows, 100.0 * regpred / rows, 100.0 * multi / rows, reads / rows))
    print("%-28s" % "cnt (lds_rows) <=" + "".join("%8d" % c for c in (1, 2, 3, 4, 6, 8)))
    for name, h in (("share of stored rows", hist_rows), ("share of stored-row reads", hist_reads),
                    ("reads served on chip", hist_onchip)):
        cs = np.cumsum(h) / max(h.sum(), 1)
        print("%-28s" % name + "".join("%7.1f%%" % (100.0 * cs[c]) for c in (1, 2, 3, 4, 6, 8)))


if __name__ == "__main__":
    main()
