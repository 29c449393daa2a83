#!/usr/bin/env python3
"""What the packed sweep's twin step (round 13) takes out of the stored-row traffic (CPU only, needs `make -C oracle`).

    python profiles/tools/twin_rows.py [--blocks 0,1,2] [--seqs 64] [--length 5000] [--at 8,24,40,63] [--global]

Builds each block's graph with the CPU oracle in spoa's node order after the given numbers of sequences and reads the row CSR
the sweep walks (Graph.rows()).  Prints, under the old rule (a row is stored when a successor other than the next row reads it)
and under the new one (tests/twin_ref.py: the readers the twin step's registers serve need no store), the stored rows and the
stored-row reads per row, and the share of twin steps and join rows; then how often the cases the step has to get right occur."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import oracle_py as O  # noqa: E402
from smoothxg_amd import synth  # noqa: E402
import twin_ref as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", default="0,1,2", help="block ids of the synthetic generator")
    ap.add_argument("--seqs", type=int, default=64)
    ap.add_argument("--length", type=int, default=5000)
    ap.add_argument("--at", default="8,24,40,63", help="graphs after this many sequences")
    ap.add_argument("--global", dest="glob", action="store_true", help="global alignment (default: local)")
    a = ap.parse_args()
    p = O.mkparams(1, -4, -6, -2, -26, -1, mode=(0 if not a.glob else 1) | 0x10)
    impl = O.IMPL_AVX2 if O.simd_available() else O.IMPL_SCALAR
    rows = 0
    tot = {"old": [0, 0], "new": [0, 0]}   # stored rows, stored-row reads
    cen = {}
    for blk in (int(b) for b in a.blocks.split(",")):
        seqs = synth.make_block(blk, a.seqs, a.length)
        for k in sorted(set(min(int(x), a.seqs - 1) for x in a.at.split(","))):
            g, _, _ = O.block_run(seqs[:k], None, p, impl=impl)
            _, off, pred, _, _ = g.rows()
            rows += len(off) - 1
            for name, new in (("old", False), ("new", True)):
                f = T.row_flags(off, pred, new_rule=new)
                tot[name][0] += int(f["stored"].sum())
                tot[name][1] += len(f["unserved"])
            for key, v in T.census(off, pred).items():
                cen[key] = cen.get(key, 0) + v
    print("blocks %s, %d sequences of %d letters, graphs after %s sequences, %s: %d rows" % (a.blocks, a.seqs, a.length, a.at, "global" if a.glob else "local", rows))
    for name in ("old", "new"):
        print("%s rule: stored rows %5.1f %%, stored-row reads per row %.3f" % (name, 100.0 * tot[name][0] / rows, tot[name][1] / rows))
    print("twin steps %.1f %% of the rows (%.1f %% with the previous row as the predecessor), join rows %.1f %%" %
          (100.0 * cen["twin_steps"] / rows, 100.0 * (cen["twin_steps"] - cen["twin_stored_pred"]) / rows, 100.0 * cen["joins"] / rows))
    print("cases:", ", ".join("%s %d" % kv for kv in sorted(cen.items())))


if __name__ == "__main__":
    main()
