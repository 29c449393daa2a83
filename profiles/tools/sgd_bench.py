"""Measurement of the path-guided SGD node order (sxg_poa_path_sgd_order, decree Y): kernel time from HIP events through
sxg_poa_stats, launch count and scratch, one warm-up and --runs timed runs per line, one JSON object per line.

  drb1      tests/golden/DRB1-3123.seqwish.gfa at full settings (100 iterations), LDS path and global path
  synth     a shuffled chain of --nodes nodes walked by --depth paths, global path (LDS path too when it fits)

No ratio against the reference is claimed: it has no such kernel, and its published 23-25 s for DRB1 is its whole run."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from smoothxg_amd import poa as P  # noqa: E402


def schedule(path_off, iter_max):
    maxsteps = int(np.diff(path_off).max())
    eta_max = float(maxsteps) ** 2
    lam = math.log(eta_max / 0.01) / (iter_max - 1) if iter_max > 1 else 0.0
    return np.array([eta_max * math.exp(-lam * t) for t in range(iter_max)]), iter_max // 2, int(path_off[-1])


def drb1():
    seqs, paths = {}, []
    for line in open(os.path.join(ROOT, "tests", "golden", "DRB1-3123.seqwish.gfa")):
        f = line.rstrip("\n").split("\t")
        if f[0] == "S":
            seqs[int(f[1])] = len(f[2])
        elif f[0] == "P":
            paths.append([int(s[:-1]) for s in f[2].split(",")])
    ids = sorted(seqs)
    rank = {i: r for r, i in enumerate(ids)}
    node_len = np.array([seqs[i] for i in ids], np.int32)
    step_node = [np.array([rank[i] for i in p], np.int32) for p in paths]
    return flat(node_len, step_node)


def flat(node_len, step_node):
    path_off = np.zeros(len(step_node) + 1, np.int64)
    path_off[1:] = np.cumsum([len(p) for p in step_node])
    pos = []
    for p in step_node:
        ln = node_len[p].astype(np.int64)
        pos.append(np.cumsum(ln) - ln)
    return node_len, path_off, np.concatenate(step_node), np.concatenate(pos)


def synth(n_nodes, depth, seed=1):
    rng = np.random.default_rng(seed)
    rank_of = rng.permutation(n_nodes)
    node_len = np.zeros(n_nodes, np.int32)
    node_len[rank_of] = rng.integers(1, 21, n_nodes)
    return flat(node_len, [rank_of[rng.random(n_nodes) >= 0.1].astype(np.int32) for _ in range(depth)])


def measure(engine, name, g, iter_max, mode, runs):
    eta, cs, terms = schedule(g[1], iter_max)
    ms, wall = [], []
    for r in range(runs + 1):
        t = time.time()
        engine.path_sgd_order(*g, eta, cs, terms, 9399220, mode=mode, want_x=False)
        wall.append((time.time() - t) * 1e3)
        st = engine.stats()
        ms.append(st["kernel_ms"])
    print(json.dumps(dict(workload=name, mode={1: "lds", 2: "global"}[mode], nodes=len(g[0]), steps=int(g[1][-1]), iter_max=iter_max,
                          terms_per_iter=terms, launches=st["n_slots"], device_bytes=st["device_bytes"],
                          kernel_ms=[round(v, 3) for v in ms[1:]], call_wall_ms=[round(v, 1) for v in wall[1:]], warmup_kernel_ms=round(ms[0], 3))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1000000)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--iter-max", type=int, default=100)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--skip-synth", action="store_true")
    a = ap.parse_args()
    engine = P.PoaEngine(0)
    g = drb1()
    for mode in (1, 2):
        measure(engine, "drb1", g, 100, mode, a.runs)
    if not a.skip_synth:
        g = synth(a.nodes, a.depth)
        if a.nodes <= P.SGD_LDS_NODES:
            measure(engine, "synth", g, a.iter_max, 1, a.runs)
        measure(engine, "synth", g, a.iter_max, 2, a.runs)
    engine.close()


if __name__ == "__main__":
    main()
