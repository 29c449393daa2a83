#!/usr/bin/env python3
"""What decree S6' (mode | SXG_IDS_SPOA: new node ids in spoa's AddAlignment order) costs, on bench.py's batches: the time of
PoaEngine.execute() on resident inputs under mode 0x10 (spoa's order, the default) and under 0x30 (the order and the ids).

  python profiles/tools/ids_price.py [--workloads ns,c2x8] [--blocks N] [--runs 3] [--out FILE.json]

After one warm-up of each, the two modes alternate run by run in ONE process, the batch uploaded once per mode change
(the upload is not timed).  Per workload: the execute() seconds of every run, the ratio of the medians, the spread of 0x10
against itself, the engine's own kernel time (stats: kernel_ms) beside the wall time, and -- the flag is a renaming of the
nodes under the re-sort -- whether scores and node / edge counts of every block agree between the two modes.  Prints (and writes to
--out) one JSON object."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (WORKLOADS: the shapes and scores the benchmark runs)
from smoothxg_amd import poa as P  # noqa: E402
from smoothxg_amd import synth  # noqa: E402

MODES = (("0x10", P.ORDER_SPOA), ("0x30", P.ORDER_SPOA | P.IDS_SPOA))


def spread(xs):
    return dict(runs=[round(x, 4) for x in xs], median=round(float(np.median(xs)), 4), min=round(min(xs), 4), max=round(max(xs), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="ns,c2x8")
    ap.add_argument("--blocks", type=int, default=0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = dict(tool="ids_price", runs=a.runs, timed="PoaEngine.execute() on resident inputs", workloads={})
    eng = P.PoaEngine(0)
    for wl in a.workloads.split(","):
        nb, ns, ln, prm, desc = bench.WORKLOADS[wl]
        nb = a.blocks or nb
        bases, seq_off, blk_off = synth.make_batch(nb, ns, ln)
        wall = {name: [] for name, _ in MODES}
        kern = {name: [] for name, _ in MODES}
        shape, ids = {}, {}
        for r in range(a.runs + 1):                       # run 0 warms both modes up and is not recorded
            for name, mode in MODES:
                eng.upload(bases, seq_off, blk_off, None, P.Params(*prm, mode, 0))
                t = time.perf_counter()
                eng.execute()
                dt = time.perf_counter() - t
                st = eng.stats()
                print("[ids_price] %s run %d %s %.3f s" % (wl, r, name, dt), file=sys.stderr, flush=True)
                if r:
                    wall[name].append(dt)
                    kern[name].append(st["kernel_ms"] / 1e3)
                if r == a.runs:
                    res = eng.download()
                    shape[name] = ([int(x) for b in res for x in b.scores], [len(b.node_code) for b in res], [len(b.edge_tail) for b in res],
                                   [np.sort(b.node_rank).tolist() == list(range(len(b.node_rank))) for b in res])
                    ids[name] = [p.tobytes() for b in res for p in b.paths]
        W = dict(description=desc, blocks=nb)
        for name, _ in MODES:
            W[name] = dict(execute_s=spread(wall[name]), kernel_s=spread(kern[name]))
        a10, a30 = W["0x10"]["execute_s"], W["0x30"]["execute_s"]
        W["ratio_of_medians"] = round(a30["median"] / a10["median"], 4)
        W["spread_0x10_rel"] = round((a10["max"] - a10["min"]) / a10["median"], 4)
        W["spread_0x30_rel"] = round((a30["max"] - a30["min"]) / a30["median"], 4)
        W["same_scores_and_counts"] = shape["0x10"] == shape["0x30"]
        W["sequences_whose_node_ids_differ"] = sum(x != y for x, y in zip(ids["0x10"], ids["0x30"]))
        W["sequences"] = len(ids["0x10"])
        out["workloads"][wl] = W
    eng.close()
    text = json.dumps(out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
