#!/usr/bin/env python3
"""Swept against used cells of the packed sweep on the synthetic blocks, per block and per alignment width.  CPU only, seconds.

A sweep visits all T * 2W columns of its geometry in every row, whatever the sequence's length.  The geometry is chosen per
block from the block's longest sequence (variant_for_len; read here from tests/golden/geometry_choice.json, packed sweep, local,
2-byte cells).  With a second strip width W2 = W - 1 (poa_classes.h: the four- and eight-wave packed classes, W = 9..12) every
alignment whose sequence fits T * 2 * W2 columns sweeps those instead.

Rows are not simulated: alignment k of a block (k = 1 .. n - 1; sequence 0 founds the graph) is weighted with
L0 * (1 + 0.0165 k) graph rows, the growth prepare_plan assumes (1.65 % new nodes per sequence).

    python profiles/tools/swept_columns.py                      # blocks 0-239 of the headline, 64 x 5 kbp
    python profiles/tools/swept_columns.py --blocks 40 --length 1000
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from smoothxg_amd import synth  # noqa: E402

W2_TMAX, W2_WIDTHS = (256, 512), range(9, 13)   # classes with a second width (kClasses parts 2 and 3)


def geometry_table():
    with open(os.path.join(ROOT, "tests", "golden", "geometry_choice.json")) as f:
        gold = json.load(f)
    for m in gold["modes"]:
        if (m["kind"], m["rm"], m["sw"], m["cb"], m["full_plane"], m["spread"]) == ("block", 2, 1, 2, 1, 0):
            return m["rows"]
    raise SystemExit("no packed local 2-byte mode in geometry_choice.json")


def geometry(rows, maxlen):
    g = None
    for first, w, nw, tmax in rows:
        if first <= maxlen:
            g = (w, nw, tmax)
    return g


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--blocks", type=int, default=240)
    ap.add_argument("--first", type=int, default=0)
    ap.add_argument("--seqs", type=int, default=64)
    ap.add_argument("--length", type=int, default=5000)
    a = ap.parse_args()
    rows = geometry_table()
    used = swept1 = swept2 = 0.0
    per_w = {}   # W of the block -> [blocks, swept today, swept with W2, alignments, alignments at W2]
    for b in range(a.first, a.first + a.blocks):
        lens = [len(s) for s in synth.make_block(b, a.seqs, a.length)]
        w, nw, tmax = geometry(rows, lens[0])
        if w < 0:
            raise SystemExit(f"block {b}: no geometry for {lens[0]} letters")
        t = 64 * nw
        w2 = w - 1 if tmax in W2_TMAX and w in W2_WIDTHS else 0
        acc = per_w.setdefault(w, [0, 0.0, 0.0, 0, 0])
        acc[0] += 1
        for k in range(1, len(lens)):
            r = lens[0] * (1 + 0.0165 * k)
            narrow = w2 and lens[k] + 1 <= t * 2 * w2
            c1, c2 = t * 2 * w, t * 2 * (w2 if narrow else w)
            used += r * lens[k]; swept1 += r * c1; swept2 += r * c2
            acc[1] += r * c1; acc[2] += r * c2; acc[3] += 1; acc[4] += 1 if narrow else 0
    print(f"blocks {a.first}..{a.first + a.blocks - 1}: {a.seqs} x {a.length}")
    print(f"swept / used cells, one width per block     : {swept1 / used:.3f}")
    print(f"swept / used cells, the narrower of W, W - 1: {swept2 / used:.3f}  ({100 * (swept2 / swept1 - 1):+.1f} % of all swept cells)")
    for w in sorted(per_w):
        n, s1, s2, al, al2 = per_w[w]
        print(f"  W = {w:2d}: {n:4d} blocks, {s1 / n:.3g} -> {s2 / n:.3g} swept cells per block ({100 * (s2 / s1 - 1):+.1f} %), "
              f"{al2} of {al} alignments at W - 1")


if __name__ == "__main__":
    main()
