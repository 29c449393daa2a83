#!/usr/bin/env python3
"""The MAF iteration (-m without block merging) on a bench-shaped batch: the legacy path (full MSA formatted on one host thread
from the per-base paths, block graphs rebuilt on the host, laced-graph lacing) against the device-rows path (trimmed MSA built
on the GPU, compact block graphs, flat lacing).

  python profiles/tools/maf_phase.py [--workload ns|c2x8|tiny] [--blocks N] [--runs 3] [--out FILE.json]

  legacy       sxg_smooth_maf_gfa with merge_blocks = 0: the yardstick;
  device_rows  sxg_smooth_maf_gfa_device_rows with the same parameters.

The two alternate run by run (legacy, device_rows; then again), after one warm-up of each, in ONE process on one box.  For each:
wall time of the call, wall time inside the POA provider (sxg_poa_batch_run), the bytes its result holds on the host
(downloaded), and the laps the library prints with SXG_SMOOTH_TIMING (stderr is read back through a temporary file).  For the
new path also the HIP-event times of the two kernels (sxg_poa_get_msa_stats) and the rows kernel's rate -- bytes of rows it
wrote per second -- beside the copy rate the same box measures (sxg_poa_measure_copy: bytes read + written per second).
Both GFAs and both MAFs are compared byte for byte.  Prints (and writes to --out) one JSON object."""
import argparse
import ctypes as C
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from smoothxg_amd import poa as P  # noqa: E402
from smoothxg_amd import smooth as SM  # noqa: E402
from identity_phase import SHAPES, smoother_of, spread  # noqa: E402


class TimedProvider:
    """sxg_poa_batch_run behind a callback that keeps the time spent in it and the size of what it returned."""

    def __init__(self, engine):
        self.engine, self.calls = engine, []
        self.run = SM.RUN_FN(self._run)

    def provider(self):
        return C.cast(self.run, C.c_void_p), C.cast(self.engine.lib.sxg_poa_batch_free, C.c_void_p), None

    def _run(self, ctx, pin, pout):
        t = time.perf_counter()
        rc = self.engine.lib.sxg_poa_batch_run(self.engine.h, pin, pout)
        dt = time.perf_counter() - t
        i, o = pin.contents, pout.contents
        nb, ns = i.n_blocks, int(o.n_seqs)
        nbases = int(i.seq_off[ns]) if ns else 0
        last = lambda p, n: int(p[n]) if p else 0
        by = 0
        if o.node_code:
            by += last(o.node_off, nb) * 9 + last(o.edge_off, nb) * 12
        if o.cons_nodes:
            by += last(o.cons_off, nb) * 4
        if o.seq_path_nodes:
            by += nbases * 4
        if o.msa_off:
            by += last(o.msa_off, nb)
        if o.bg_node_off:
            by += last(o.bg_node_off, nb) * 9 + last(o.bg_seq_off, nb) + last(o.bg_edge_off, nb) * 4 + last(o.bg_step_off, ns) * 4
            by += last(o.bg_cons_off, nb) * 4 if o.bg_cons_off else 0
        by += ns * 12 + nb * 12
        self.calls.append(dict(s=dt, bytes=by, msa_bytes=last(o.msa_off, nb), want_msa=i.want_msa, want_block_graph=i.want_block_graph))
        return rc


def iteration(sm, params, prov, device_rows):
    mp = SM.MergeParams()
    sm.L.sxg_merge_default_params(C.byref(mp))
    mp.maf_header = b"##maf version=1"
    gfa, maf, nf = C.c_void_p(), C.c_void_p(), C.c_int64()
    call = sm.L.sxg_smooth_maf_gfa_device_rows if device_rows else sm.L.sxg_smooth_maf_gfa_adaptive
    run, fre, ctx = prov.provider()
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            t0 = time.perf_counter()
            rc = call(sm.g, sm.b, C.byref(params), C.byref(mp), run, fre, ctx, None, None, C.byref(gfa), C.byref(maf), C.byref(nf))
            dt = time.perf_counter() - t0
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        err = tmp.read().decode(errors="replace")
    if rc:
        raise RuntimeError("MAF iteration: " + sm.L.sxg_smooth_last_error().decode())
    laps = {}
    for m in re.finditer(r"\[sxg_smooth\] (.*?)\s+([0-9.]+) s", err):
        laps[m.group(1).strip()] = laps.get(m.group(1).strip(), 0.0) + float(m.group(2))
    out = (C.string_at(gfa), C.string_at(maf), nf.value)
    sm.L.sxg_smooth_free(gfa)
    sm.L.sxg_smooth_free(maf)
    return dt, laps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="ns", choices=sorted(SHAPES))
    ap.add_argument("--blocks", type=int, default=0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nb, depth, length = SHAPES[a.workload]
    nb = a.blocks or nb
    os.environ["SXG_SMOOTH_TIMING"] = "1"
    t0 = time.perf_counter()
    sm = smoother_of(nb, depth, length)
    engine = P.PoaEngine(0)
    prov = TimedProvider(engine)
    params = SM.default_params(add_consensus=1)
    out = dict(tool="maf_phase", workload=a.workload, blocks=nb, depth=depth, length=length, runs=a.runs, add_consensus=1, merge_blocks=0,
               host_threads=int(os.environ.get("OMP_NUM_THREADS") or len(os.sched_getaffinity(0))), setup_s=round(time.perf_counter() - t0, 2))
    rec = {False: dict(wall=[], prov=[], bytes=None, laps=[]), True: dict(wall=[], prov=[], bytes=None, laps=[], cols_ms=[], rows_ms=[], msa_bytes=0)}
    res = {}
    for r in range(a.runs + 1):                                   # run 0 warms both parts up and is not recorded
        for dev in (False, True):
            prov.calls.clear()
            dt, laps, res[dev] = iteration(sm, params, prov, dev)
            if not r:
                continue
            R = rec[dev]
            R["wall"].append(dt)
            R["prov"].append(sum(c["s"] for c in prov.calls))
            R["bytes"] = sum(c["bytes"] for c in prov.calls)
            R["asked"] = sorted({(c["want_msa"], c["want_block_graph"]) for c in prov.calls})
            R["laps"].append(laps)
            if dev:
                cm, rm, mb = engine.msa_stats()
                R["cols_ms"].append(cm)
                R["rows_ms"].append(rm)
                R["msa_bytes"] = mb
    for dev, name in ((False, "legacy"), (True, "device_rows")):
        R = rec[dev]
        o = dict(wall_s=spread(R["wall"]), provider_wall_s=spread(R["prov"]), downloaded_bytes=R["bytes"], asked=R.get("asked"),
                 laps_s={k: spread([l.get(k, 0.0) for l in R["laps"]]) for k in (R["laps"][0] if R["laps"] else {})})
        if dev:
            o["msa_cols_kernel_ms"] = spread(R["cols_ms"])
            o["msa_rows_kernel_ms"] = spread(R["rows_ms"])
            o["msa_bytes"] = int(R["msa_bytes"])
            if R["rows_ms"] and min(R["rows_ms"]) > 0:
                o["msa_rows_written_GBps"] = spread([R["msa_bytes"] / (ms * 1e-3) / 1e9 for ms in R["rows_ms"]])
        out[name] = o
    out["copy_GBps_read_plus_written"] = round(engine.measure_copy(1 << 30, 5), 1)
    out["gfa_equal"] = bool(res[False][0] == res[True][0])
    out["maf_equal"] = bool(res[False][1] == res[True][1])
    out["flips"] = [int(res[False][2]), int(res[True][2])]
    out["gfa_bytes"], out["maf_bytes"] = len(res[True][0]), len(res[True][1])
    engine.close()
    text = json.dumps(out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
