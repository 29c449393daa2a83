#!/usr/bin/env python3
"""What the device group (sxg_poa_group, smoothxg_amd.PoaGroup) costs on ONE GPU, on bench.py's batches, asked for what an
iteration asks for: block graphs only (want_block_graph = 3), consensus and the trimmed MSA.

  python profiles/tools/group_phase.py [--workloads ns,c2x8] [--blocks N] [--runs 3] [--out FILE.json]

  engine      sxg_poa_batch_run on PoaEngine(0): the yardstick, measured in the same process;
  group_1     sxg_poa_group_batch_run on PoaGroup([0]): what the group layer costs when there is nothing to reassemble;
  group_2     ... on PoaGroup([0, 0]): two members on one device, each with half the arena cap a handle takes by default.
              It shows that two members coexist -- two host threads, two sets of streams and arenas, a reassembly -- and is NOT
              a speed-up: both members share one GPU;
  group_2dev  ... on PoaGroup([0, 1]), only where sxg_poa_device_count() >= 2: the first real two-device figure.

The variants alternate run by run after one warm-up of each, in ONE process.  For each: wall seconds of the C call (sxg_poa_batch_run /
sxg_poa_group_batch_run: upload, execute, download, reassembly), sxg_poa_group_timing of the last run, and once per
workload the deal's imbalance (the costliest member's share of the total cost times the number of members; the rule of
smoothxg_amd/csrc/poa_deal.h restated here).  The results of every variant are compared with the engine's.  Prints (and writes
to --out) one JSON object."""
import argparse
import ctypes as C
import hashlib
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


def spread(xs):
    return dict(runs=[round(x, 4) for x in xs], median=round(float(np.median(xs)), 4), min=round(min(xs), 4), max=round(max(xs), 4))


def deal_imbalance(seq_off, blk_off, n):
    """poa_deal.h restated: cost of a block = sum over k >= 1 of L_k (L_0 + 0.05 sum_{j<k} L_j), truncated; block b goes to
    member floor(cost before b * n / total).  Returns the costliest member's cost over total / n."""
    cost = []
    for b in range(len(blk_off) - 1):
        ln = np.diff(seq_off[blk_off[b]:blk_off[b + 1] + 1]).astype(np.float64)
        c, prev = 0.0, 0.0
        for k, l in enumerate(ln):
            if k:
                c += l * (ln[0] + 0.05 * prev)
            prev += l
        cost.append(int(c))
    total, before, load = sum(cost), 0, [0] * n
    for c in cost:
        load[min(n - 1, before * n // total) if total else 0] += c
        before += c
    return round(max(load) * n / total, 4) if total else 1.0


def as_bytes(ptr, n, itemsize):
    return C.string_at(ptr, n * itemsize) if ptr and n else b""


def digest(o):
    """One hash over every array of a want_block_graph = 3 + trimmed MSA result but block_cycles (a timing)."""
    nb, ns = o.n_blocks, int(o.n_seqs)
    h = hashlib.blake2b(digest_size=16)
    last = lambda p, n: int(p[n]) if p and n >= 0 else 0
    for ptr, n, sz in ((o.status, nb, 4), (o.score, ns, 4), (o.cells, ns, 8), (o.node_off, nb + 1, 8), (o.edge_off, nb + 1, 8),
                       (o.cons_off, nb + 1, 8), (o.msa_off, nb + 1, 8), (o.msa_cols, nb, 4), (o.msa, last(o.msa_off, nb), 1),
                       (o.bg_node_off, nb + 1, 8), (o.bg_node_len, last(o.bg_node_off, nb), 4), (o.bg_node_outdeg, last(o.bg_node_off, nb), 4),
                       (o.bg_node_indeg, last(o.bg_node_off, nb), 1), (o.bg_seq_off, nb + 1, 8), (o.bg_seq, last(o.bg_seq_off, nb), 1),
                       (o.bg_edge_off, nb + 1, 8), (o.bg_edge_to, last(o.bg_edge_off, nb), 4), (o.bg_step_off, ns + 1, 8),
                       (o.bg_steps, last(o.bg_step_off, ns), 4), (o.bg_cons_off, nb + 1, 8), (o.bg_cons_steps, last(o.bg_cons_off, nb), 4)):
        h.update(as_bytes(ptr, n, sz))
    cycles = np.ctypeslib.as_array(o.block_cycles, shape=(nb,)) if o.block_cycles and nb else np.zeros(0, np.uint64)
    return h.hexdigest(), int((cycles > 0).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="ns,c2x8")
    ap.add_argument("--blocks", type=int, default=0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = P.load_library()
    variants = [("engine", None), ("group_1", [0]), ("group_2", [0, 0])]
    if lib.sxg_poa_device_count() >= 2:
        variants.append(("group_2dev", [0, 1]))
    out = dict(tool="group_phase", runs=a.runs, request="want_block_graph=3, want_consensus=1, want_msa=SXG_MSA_TRIMMED",
               devices=int(lib.sxg_poa_device_count()), budget="default arena cap (a member: 1/k of a handle's, k members on its device)",
               host_threads=int(os.environ.get("OMP_NUM_THREADS") or len(os.sched_getaffinity(0))), workloads={})
    for wl in a.workloads.split(","):
        nb, ns, ln, prm, desc = bench.WORKLOADS[wl]
        nb = a.blocks or nb
        t0 = time.perf_counter()
        bases, seq_off, blk_off = synth.make_batch(nb, ns, ln)
        params = P.Params(*prm, 0x10, 0)
        W = dict(description=desc, blocks=nb, setup_s=round(time.perf_counter() - t0, 2),
                 deal_imbalance={str(n): deal_imbalance(seq_off, blk_off, n) for n in (2, 8)})
        runners = {name: (P.PoaEngine(0) if devs is None else P.PoaGroup(devs)) for name, devs in variants}
        wall = {name: [] for name, _ in variants}
        timing, equal, ref = {}, {}, None
        bi = runners["engine"]._mk_in(bases, seq_off, blk_off, None, params, True, P.MSA_TRIMMED, 3)
        cycles = {}
        for r in range(a.runs + 1):                       # run 0 warms every variant up and is not recorded
            for name, devs in variants:
                o = P.BatchOut()
                call = lib.sxg_poa_batch_run if devs is None else lib.sxg_poa_group_batch_run
                t = time.perf_counter()
                rc = call(runners[name].h, C.byref(bi), C.byref(o))      # (upload, execute, download, reassembly: the C call alone)
                dt = time.perf_counter() - t
                if rc:
                    raise RuntimeError("%s: %s" % (name, lib.sxg_poa_last_error().decode()))
                if r:
                    wall[name].append(dt)
                print("[group_phase] %s run %d %s %.3f s" % (wl, r, name, dt), file=sys.stderr, flush=True)
                d, cycles[name] = digest(o)
                lib.sxg_poa_batch_free(C.byref(o))
                if name == "engine":
                    ref = d
                else:
                    equal[name] = bool(equal.get(name, True) and d == ref)
                    timing[name] = runners[name].timing()
        W["blocks_with_cycles"] = cycles
        for name, _ in variants:
            W[name] = dict(wall_s=spread(wall[name]))
            if name in timing:
                W[name].update(timing_ms={k: ([round(x, 2) for x in v] if isinstance(v, list) else round(v, 2)) for k, v in timing[name].items()},
                               equals_engine=equal[name])
        e = W["engine"]["wall_s"]
        W["engine_spread_s"] = round(e["max"] - e["min"], 4)
        W["group_1_minus_engine_s"] = round(W["group_1"]["wall_s"]["median"] - e["median"], 4)
        W["group_2_minus_group_1_s"] = round(W["group_2"]["wall_s"]["median"] - W["group_1"]["wall_s"]["median"], 4)
        if "group_2dev" in W:
            W["group_2dev_over_engine"] = round(W["group_2dev"]["wall_s"]["median"] / e["median"], 4)
        for x in runners.values():
            x.close()
        out["workloads"][wl] = W
    text = json.dumps(out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
