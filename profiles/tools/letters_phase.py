#!/usr/bin/env python3
"""The two provider phases in front of the POA call -- the repeat scan of break_blocks and the identity estimate of -a -- fed
RANGES of the resident path letters, against the `bases` providers ON THE SAME BUILD (the code path every run used before).

  python profiles/tools/letters_phase.py --phase scan     [--blocks 1000] [--depth 64] [--length 5000] [--runs 3] [--out FILE.json]
  python profiles/tools/letters_phase.py --phase identity [--workload ns|c2x8|tiny] [--runs 3] [--out FILE.json]
  python profiles/tools/letters_phase.py --phase e2e      [--workload ns|c2x8|tiny] [--runs 3] [--out FILE.json]

  scan      sxg_blockset_break_scan with sxg_poa_repeat_scan_batch against sxg_blockset_break_scan_ranges with
            sxg_poa_repeat_scan_ranges, on repeat_phase.py's graph (every block is cut, every range is scanned);
  identity  sxg_blockset_identity_thresholds with sxg_poa_block_identity_batch against sxg_blockset_identity_thresholds_ranges with
            sxg_poa_block_identity_ranges, on identity_phase.py's graph;
  e2e       one -a iteration (sxg_smooth_gfa_adaptive) with the bases identifier against the range identifier, each preceded by the
            cut with the matching scanner on the same graph: what an iteration pays for both providers, the one upload counted.

Every provider is wrapped by a callback that forwards the library's pointers untouched and takes the time around the engine call.
Reported per path, median (min - max) over --runs: the wall time of the phase, the engine call, kernel_ms of sxg_poa_stats (which
for ranges includes the gather), and for ranges the gather alone (HIP events of its own: sxg_poa_letters_stats) with the bytes it
read + wrote per second beside the box's measured copy bandwidth.  The ranges path is measured twice: WARM, the letters resident,
alternating run by run with the bases path after one warm-up of each; and COLD, after sxg_poa_letters_drop, when the call pays
the one upload (its time: cold engine call - warm engine call).  The building of the graph's path letters in the host library
(sxg_graph_path_letters, once per graph) is timed by itself.  Results are compared: blocks, counts, thresholds, GFA.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from smoothxg_amd import poa as P  # noqa: E402
from smoothxg_amd import smooth as SM  # noqa: E402
import identity_phase as IP  # noqa: E402
import repeat_phase as RP  # noqa: E402

K = IP.K


def spread(xs, nd=4):
    return dict(runs=[round(x, nd) for x in xs], median=round(float(np.median(xs)), nd), min=round(min(xs), nd), max=round(max(xs), nd)) if xs else None


class Timed:
    """A provider around an engine entry point that forwards the pointers and times the call."""

    def __init__(self, engine, fn_type, entry, ranges):
        self.engine, self.calls, self.ranges = engine, [], ranges
        target = getattr(engine.lib, entry)

        def forward(ctx, *args):
            t = time.perf_counter()
            rc = target(engine.h, *args)
            self.calls.append(time.perf_counter() - t)
            return rc
        self.cb = fn_type(forward)
        tup = (C.cast(self.cb, C.c_void_p), None)
        self.provider = SM.RangeProvider(tup) if ranges else tup


def scan_once(sm, max_poa, prov):
    out = C.c_void_p()
    counts = [C.c_int64(), C.c_int64(), C.c_int64()]
    call = sm.L.sxg_blockset_break_scan_ranges if prov.ranges else sm.L.sxg_blockset_break_scan
    del prov.calls[:]
    t0 = time.perf_counter()
    rc = call(sm.g, sm.b, max_poa, *RP.REPEATS, 1, prov.provider[0], None, C.byref(out), *(C.byref(c) for c in counts))
    dt = time.perf_counter() - t0
    if rc:
        raise RuntimeError(sm.L.sxg_smooth_last_error().decode())
    keep, sm.b = sm.b, out
    try:
        digest = hash(tuple(tuple(sm.block_ranges(k)) for k in range(sm.n_blocks)))
    finally:
        sm.b = keep
        sm.L.sxg_blockset_free(out)
    return dt, (digest, tuple(c.value for c in counts))


def identity_once(sm, prov):
    del prov.calls[:]
    t0 = time.perf_counter()
    thr, used = sm.identity_thresholds(K, prov.provider)
    return time.perf_counter() - t0, (thr.tobytes(), used.tobytes())


def measure(engine, once, bases, ranges, runs):
    """-> the report of one phase: bases and warm ranges alternating after a warm-up of each, then cold ranges."""
    rec = {name: dict(wall=[], call=[], kernel_ms=[], gather_ms=[], gathered=[]) for name in ("bases", "ranges_warm", "ranges_cold")}
    res = {}

    def run(name, prov, keep):
        g0 = engine.letters_stats()
        dt, result = once(prov)
        if len(prov.calls) != 1:
            raise RuntimeError("the provider was called %d times" % len(prov.calls))
        res[name] = result
        if keep:
            g1 = engine.letters_stats()
            r = rec[name]
            r["wall"].append(dt); r["call"].append(prov.calls[0]); r["kernel_ms"].append(engine.stats()["kernel_ms"])
            r["gather_ms"].append(g1["gather_ms"] - g0["gather_ms"]); r["gathered"].append(g1["gathered_bytes"] - g0["gathered_bytes"])
    for r in range(runs + 1):                    # run 0 warms both paths up (and uploads the letters) and is not recorded
        run("bases", bases, r > 0)
        run("ranges_warm", ranges, r > 0)
    for r in range(runs):
        engine.drop_letters()
        run("ranges_cold", ranges, True)
    out = {}
    for name, r in rec.items():
        out[name] = dict(phase_s=spread(r["wall"]), engine_call_s=spread(r["call"]), kernel_ms=spread(r["kernel_ms"], 3),
                         host_library_s=spread([w - c for w, c in zip(r["wall"], r["call"])]))
        if name != "bases":
            out[name]["gather_ms"] = spread(r["gather_ms"], 3)
            out[name]["gathered_bytes"] = int(r["gathered"][0])
            out[name]["gather_GBps_read_plus_written"] = spread([2e-6 * b / ms for b, ms in zip(r["gathered"], r["gather_ms"]) if ms > 0], 1)
    out["upload_s_cold_minus_warm_call"] = round(out["ranges_cold"]["engine_call_s"]["median"] - out["ranges_warm"]["engine_call_s"]["median"], 4)
    out["results_equal"] = bool(res["bases"] == res["ranges_warm"] == res["ranges_cold"])
    b, w = out["bases"]["phase_s"], out["ranges_warm"]["phase_s"]
    out["warm_gain_s"] = round(b["median"] - w["median"], 4)
    out["bases_min_max_range_s"] = round(b["max"] - b["min"], 4)
    out["warm_pays"] = bool(b["median"] - w["median"] > b["max"] - b["min"])     # the bar: faster by more than the yardstick's own spread
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phase", required=True, choices=("scan", "identity", "e2e"))
    ap.add_argument("--workload", default="ns", choices=sorted(IP.SHAPES))
    ap.add_argument("--blocks", type=int, default=1000)
    ap.add_argument("--depth", type=int, default=64)
    ap.add_argument("--length", type=int, default=5000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    engine = P.PoaEngine(0)
    out = dict(tool="letters_phase", phase=a.phase, runs=a.runs, host_threads=int(os.environ.get("OMP_NUM_THREADS") or len(os.sched_getaffinity(0))),
               copy_GBps_measured=round(engine.measure_copy(1 << 30, 5), 1), gather_chunk_bytes=engine.letters_geometry())
    scan_b = Timed(engine, SM.REPEAT_FN, "sxg_poa_repeat_scan_batch", False)
    scan_r = Timed(engine, SM.REPEAT_RANGES_FN, "sxg_poa_repeat_scan_ranges", True)
    id_b = Timed(engine, SM.IDENT_FN, "sxg_poa_block_identity_batch", False)
    id_r = Timed(engine, SM.IDENT_RANGES_FN, "sxg_poa_block_identity_ranges", True)
    if a.phase == "scan":
        sm, len_min, len_max, letters = RP.smoother_of(a.blocks, a.depth, a.length)
        out.update(blocks=a.blocks, depth=a.depth, length=a.length, letters=letters, max_poa_length=a.length // 2, repeats=RP.REPEATS)
    else:
        nb, depth, length = IP.SHAPES[a.workload]
        sm = IP.smoother_of(nb, depth, length)
        out.update(workload=a.workload, blocks=nb, depth=depth, length=length, kmer_size=K)
    t0 = time.perf_counter()
    L = sm.path_letters()
    out["path_letters_build_s"] = round(time.perf_counter() - t0, 4)     # once per graph, cached in it
    out["path_letters_bytes"] = int(len(L.letters))
    if a.phase == "scan":
        out.update(measure(engine, lambda prov: scan_once(sm, a.length // 2, prov), scan_b, scan_r, a.runs))
    elif a.phase == "identity":
        out.update(measure(engine, lambda prov: identity_once(sm, prov), id_b, id_r, a.runs))
    else:
        params = SM.default_params(adaptive_poa_params=1, kmer_size=K)
        provider = SM.gpu_provider(engine)
        walls = {"bases": [], "ranges": []}
        gfa = {}
        u0 = engine.letters_stats()
        for r in range(a.runs + 1):
            for name, sc, ident in (("bases", scan_b, id_b), ("ranges", scan_r, id_r)):
                if name == "ranges":
                    engine.drop_letters()                                # every iteration pays its one upload, as on a new graph
                t0 = time.perf_counter()
                scan_once(sm, length // 2, sc)
                gfa[name] = sm.smooth_gfa(params, provider, identity=ident.provider)
                if r:
                    walls[name].append(time.perf_counter() - t0)
        u1 = engine.letters_stats()
        out["cut_plus_iteration_s"] = {k: spread(v) for k, v in walls.items()}
        out["uploads_per_ranges_iteration"] = (u1["uploads"] - u0["uploads"]) / (a.runs + 1)
        out["gfa_equal"] = bool(gfa["bases"] == gfa["ranges"])
    engine.close()
    text = json.dumps(out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
