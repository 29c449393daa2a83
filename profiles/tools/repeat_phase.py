#!/usr/bin/env python3
"""The tandem-repeat scan of the cutting half of break_blocks as a phase of its own, on a bench-shaped graph whose every block is
cut: the host scan against the device call (decree R).

  python profiles/tools/repeat_phase.py [--blocks 1000] [--depth 64] [--length 5000] [--runs 3] [--parts host,device] [--out FILE.json]

  host    sxg_blockset_break_scan with scan = NULL: the code every run used before (repeat_length per range over the host
          threads: OMP_NUM_THREADS, else the CPUs the process may use), then the cut;
  device  the same call with the engine's sxg_poa_repeat_scan_batch as the provider.  The provider is wrapped by a callback that
          forwards the library's pointers untouched and takes the time around the engine call, so the call's wall time splits
          into kernels (kernel_ms of sxg_poa_stats: HIP events around the count and statistics launches of every round), the rest
          of the engine call (upload of the letters, sorting the work items, download) and the host library's own work
          (collecting the range sequences before the call, deciding and cutting after it).

The parts alternate run by run (host, device; then again) after one warm-up of each, in ONE process on one box.  The yardstick is
`host`.  The blocks of both are compared range for range, and the counts (blocks cut, of which at a repeat).  Every block holds
`depth` ranges of about `length` bases (smoothxg_amd.synth, the bench's generator: related haplotypes, no planted repeat) and
max_poa_length is half of `length`, so every block is cut and every range is scanned.  The two kernels' separate times are not in
sxg_poa_stats: take them from a run of their own,
`rocprofv3 --kernel-trace --stats -d DIR -- python profiles/tools/repeat_phase.py --parts device --runs 2`
(repeat_count_kernel / repeat_stats_kernel in the kernel statistics).
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

REPEATS = (1000, 20000, 5.0, 50)   # src/main.cpp:285-286,457-458


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
    lens = np.diff(seq_off)
    return SM.Smoother(b"".join(lines), blocks=[[(k, b, b + 1) for k in range(depth)] for b in range(nb)]), int(lens.min()), int(lens.max()), int(lens.sum())


def break_scan(sm, max_poa, scan, ctx):
    out = C.c_void_p()
    counts = [C.c_int64(), C.c_int64(), C.c_int64()]
    t0 = time.perf_counter()
    rc = sm.L.sxg_blockset_break_scan(sm.g, sm.b, max_poa, REPEATS[0], REPEATS[1], REPEATS[2], REPEATS[3], 1, scan, ctx, C.byref(out), *(C.byref(c) for c in counts))
    dt = time.perf_counter() - t0
    if rc:
        raise RuntimeError("sxg_blockset_break_scan: " + sm.L.sxg_smooth_last_error().decode())
    keep, sm.b = sm.b, out
    try:
        digest = hash(tuple(tuple(sm.block_ranges(k)) for k in range(sm.n_blocks)))
    finally:
        sm.b = keep
        sm.L.sxg_blockset_free(out)
    return dt, digest, tuple(c.value for c in counts)


def spread(xs):
    return dict(runs=[round(x, 4) for x in xs], median=round(float(np.median(xs)), 4), min=round(min(xs), 4), max=round(max(xs), 4)) if xs else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=1000)
    ap.add_argument("--depth", type=int, default=64)
    ap.add_argument("--length", type=int, default=5000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parts", default="host,device")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    parts = a.parts.split(",")
    t0 = time.perf_counter()
    sm, len_min, len_max, letters = smoother_of(a.blocks, a.depth, a.length)
    engine = P.PoaEngine(0) if "device" in parts else None      # (the host part alone needs no GPU)
    call_s = []

    def forward(ctx, inp, n_lags, best, dev, v, status, match):   # the library's pointers go to the engine as they are
        t = time.perf_counter()
        rc = engine.lib.sxg_poa_repeat_scan_batch(engine.h, inp, n_lags, best, dev, v, status, match)
        call_s.append(time.perf_counter() - t)
        return rc
    cb = SM.REPEAT_FN(forward)
    max_poa = a.length // 2
    out = dict(tool="repeat_phase", blocks=a.blocks, depth=a.depth, length=a.length, range_len_min=len_min, range_len_max=len_max, letters=letters,
               max_poa_length=max_poa, repeats=REPEATS, runs=a.runs, host_threads=int(os.environ.get("OMP_NUM_THREADS") or len(os.sched_getaffinity(0))),
               setup_s=round(time.perf_counter() - t0, 2))
    host_s, dev_s, dev_call_s, dev_kernel_ms = [], [], [], []
    host_res = dev_res = stats = None
    for r in range(a.runs + 1):                                   # run 0 warms every part up and is not recorded
        if "host" in parts:
            dt, digest, counts = break_scan(sm, max_poa, None, None)
            host_res = (digest, counts)
            if r:
                host_s.append(dt)
        if "device" in parts:
            del call_s[:]
            dt, digest, counts = break_scan(sm, max_poa, C.cast(cb, C.c_void_p), None)
            dev_res = (digest, counts)
            if len(call_s) != 1:
                raise RuntimeError("the provider was called %d times" % len(call_s))
            if r:
                dev_s.append(dt)
                dev_call_s.append(call_s[0])
                stats = engine.stats()
                dev_kernel_ms.append(stats["kernel_ms"])
    out["host_scan_and_cut_s"] = spread(host_s)
    out["device_scan_and_cut_s"] = spread(dev_s)
    out["device_engine_call_s"] = spread(dev_call_s)
    out["device_kernel_ms"] = spread(dev_kernel_ms)
    if dev_s:
        out["device_call_minus_kernels_s"] = spread([c - k / 1e3 for c, k in zip(dev_call_s, dev_kernel_ms)])   # upload, item sort, download
        out["device_host_library_s"] = spread([w - c for w, c in zip(dev_s, dev_call_s)])                        # collect, decide, cut
    if stats:
        out["device_stats"] = dict(dp_launches=int(stats["dp_launches"]), n_slots=int(stats["n_slots"]), device_bytes=int(stats["device_bytes"]))
    for name, res in (("host", host_res), ("device", dev_res)):
        if res:
            out[name + "_counts"] = dict(n_cut=res[1][0], n_repeat=res[1][1], n_host=res[1][2])
    if host_res and dev_res:
        out["blocks_equal"] = bool(host_res[0] == dev_res[0] and host_res[1][:2] == dev_res[1][:2])
        out["host_over_device"] = round(float(np.median(host_s)) / float(np.median(dev_s)), 2)
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
