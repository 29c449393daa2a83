#!/usr/bin/env python3
"""The identity estimate of the adaptive scores (-a) as a phase of its own, on a bench-shaped batch: the host estimator against
the device call (decree Q), and one -a iteration end to end with and without the identity provider.

  python profiles/tools/identity_phase.py [--workload ns|c2x8|tiny] [--blocks N] [--runs 3] [--parts host,device,e2e] [--out FILE.json]

  host    sxg_blockset_identity_thresholds with ident = NULL: the estimator every -a run used before, over the host threads
          (OMP_NUM_THREADS, else the CPUs the process may use);
  device  the same call with gpu_identifier(engine): wall time of the call (batch coding + upload + kernels + thresholds) and
          kernel_ms of sxg_poa_stats (HIP events around the sketch, pairs and select kernels);
  e2e     sxg_smooth_gfa_adaptive with adaptive_poa_params = 1, ident = NULL against ident = the device call.

The parts alternate run by run (host, device, e2e without, e2e with; then again), after one warm-up of each, in ONE process on
one box.  The yardstick is `host`.  The thresholds of both estimators are compared byte for byte, the two GFAs too.  The three
kernels' separate times are not in sxg_poa_stats: take them from a run of their own,
`rocprofv3 --kernel-trace --stats -d DIR -- python profiles/tools/identity_phase.py --parts device --runs 2`
(mash_sketch_kernel / identity_pairs_kernel / identity_select_kernel in the kernel statistics).
Prints (and writes to --out) one JSON object."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from smoothxg_amd import poa as P  # noqa: E402
from smoothxg_amd import smooth as SM  # noqa: E402
from smoothxg_amd import synth  # noqa: E402

SHAPES = {"ns": (1000, 64, 5000), "c2x8": (8000, 16, 1000), "tiny": (8, 6, 300)}   # bench.py's headline and small-block shapes
K = 17


def smoother_of(nb, depth, length):
    """One node per (block, sequence), one path per sequence rank, block b = the b-th step of every path (as bench.py's
    end-to-end measurement builds its graph)."""
    bases, seq_off, blk_off = synth.make_batch(nb, depth, length)
    text = np.frombuffer(b"ACGTN", np.uint8)[bases].tobytes()
    lines = []
    for b in range(nb):
        for k in range(depth):
            s = int(blk_off[b]) + k
            lines.append(b"S\t%d\t%s\n" % (b * depth + k + 1, text[int(seq_off[s]):int(seq_off[s + 1])]))
    for k in range(depth):
        lines.append(b"P\thap%d\t%s\t*\n" % (k, b",".join(b"%d+" % (b * depth + k + 1) for b in range(nb))))
    return SM.Smoother(b"".join(lines), blocks=[[(k, b, b + 1) for k in range(depth)] for b in range(nb)])


def iteration(sm, params, provider, ident):
    out = C.c_void_p()
    t0 = time.perf_counter()
    rc = sm.L.sxg_smooth_gfa_adaptive(sm.g, sm.b, C.byref(params), provider[0], provider[1], provider[2], ident[0], ident[1], C.byref(out))
    dt = time.perf_counter() - t0
    if rc:
        raise RuntimeError("sxg_smooth_gfa_adaptive: " + sm.L.sxg_smooth_last_error().decode())
    text = C.string_at(out)
    sm.L.sxg_smooth_free(out)
    return dt, text


def spread(xs):
    return dict(runs=[round(x, 4) for x in xs], median=round(float(np.median(xs)), 4), min=round(min(xs), 4), max=round(max(xs), 4)) if xs else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="ns", choices=sorted(SHAPES))
    ap.add_argument("--blocks", type=int, default=0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parts", default="host,device,e2e")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nb, depth, length = SHAPES[a.workload]
    nb = a.blocks or nb
    parts = a.parts.split(",")
    t0 = time.perf_counter()
    sm = smoother_of(nb, depth, length)
    engine = P.PoaEngine(0) if "device" in parts or "e2e" in parts else None      # (the host part alone needs no GPU)
    ident, provider = (SM.gpu_identifier(engine), SM.gpu_provider(engine)) if engine else (None, None)
    params = SM.default_params(adaptive_poa_params=1, kmer_size=K, poa_padding_fraction=0.0)
    out = dict(tool="identity_phase", workload=a.workload, blocks=nb, depth=depth, length=length, kmer_size=K, runs=a.runs,
               pairs_per_block=depth * (depth - 1) // 2, host_threads=int(os.environ.get("OMP_NUM_THREADS") or len(os.sched_getaffinity(0))),
               setup_s=round(time.perf_counter() - t0, 2))
    host_s, dev_s, dev_kernel_ms, e2e_host_s, e2e_dev_s = [], [], [], [], []
    thr_h = thr_d = gfa_h = gfa_d = None
    stats = None
    for r in range(a.runs + 1):                                   # run 0 warms every part up and is not recorded
        if "host" in parts:
            t = time.perf_counter()
            thr_h = sm.identity_thresholds(K)
            if r:
                host_s.append(time.perf_counter() - t)
        if "device" in parts:
            t = time.perf_counter()
            thr_d = sm.identity_thresholds(K, ident)
            if r:
                dev_s.append(time.perf_counter() - t)
                stats = engine.stats()
                dev_kernel_ms.append(stats["kernel_ms"])
        if "e2e" in parts:
            dt, gfa_h = iteration(sm, params, provider, (None, None))
            if r:
                e2e_host_s.append(dt)
            dt, gfa_d = iteration(sm, params, provider, ident)
            if r:
                e2e_dev_s.append(dt)
    out["host_estimator_s"] = spread(host_s)
    out["device_call_wall_s"] = spread(dev_s)
    out["device_kernel_ms"] = spread(dev_kernel_ms)
    if stats:
        out["device_stats"] = dict(dp_launches=int(stats["dp_launches"]), n_slots=int(stats["n_slots"]), device_bytes=int(stats["device_bytes"]))
    out["iteration_host_estimator_s"] = spread(e2e_host_s)
    out["iteration_device_estimator_s"] = spread(e2e_dev_s)
    if thr_h is not None and thr_d is not None:
        out["thresholds_equal"] = bool(thr_h[0].tobytes() == thr_d[0].tobytes() and thr_h[1].tobytes() == thr_d[1].tobytes())
        out["tiers"] = sorted({str(SM.adaptive_poa_scores(float(t))) for t, u in zip(thr_h[0], thr_h[1]) if u > 1})
    if gfa_h is not None:
        out["gfa_equal"] = bool(gfa_h == gfa_d)
        out["gfa_bytes"] = len(gfa_h)
    if engine:
        engine.close()
    text = json.dumps(out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
