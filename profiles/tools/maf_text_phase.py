#!/usr/bin/env python3
"""The MAF iteration (-m without block merging) on a bench-shaped batch: the device-rows path (trimmed rows downloaded, one
std::string per row, the in-order consumer on one host thread) against the device-text path (rows resident, the MAF text laid
out on the GPU and downloaded once).

  python profiles/tools/maf_text_phase.py [--workload ns|c2x8|tiny] [--blocks N] [--runs 3] [--out FILE.json]

  device_rows  sxg_smooth_maf_gfa_device_rows with merge_blocks = 0: the yardstick;
  device_text  sxg_smooth_maf_gfa_device_text with the same parameters, texter = the same engine.

The two alternate run by run (device_rows, device_text; then again), after one warm-up of each, in ONE process on one box, with
consensus on.  For each: wall time of the call, wall time inside the POA provider (sxg_poa_batch_run), the bytes its result holds
on the host (downloaded: for device_text the MAF text is added, since it is downloaded by the text call), and the laps the
library prints with SXG_SMOOTH_TIMING.  For the new path also the wall time of the two texter calls, the HIP-event time of the
text kernel (sxg_poa_maf_text_stats) and its rate -- bytes read + written per second: every byte of the text is read once from
the rows or the literals and written once -- beside the copy rate the same box measures (sxg_poa_measure_copy).
Both GFAs and both MAFs are compared byte for byte.  Prints (and writes to --out) one JSON object."""
import argparse
import ctypes as C
import json
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from smoothxg_amd import poa as P  # noqa: E402
from smoothxg_amd import smooth as SM  # noqa: E402
from identity_phase import SHAPES, smoother_of, spread  # noqa: E402
from maf_phase import TimedProvider  # noqa: E402


class TimedTexter:
    """sxg_poa_msa_row_letters and sxg_poa_maf_text behind callbacks that keep the time spent in them."""

    def __init__(self, engine):
        self.engine, self.letters_s, self.text_s, self.text_bytes = engine, 0.0, 0.0, 0
        self.cl, self.ct = SM.MSA_LETTERS_FN(self._letters), SM.MAF_TEXT_FN(self._text)

    def reset(self):
        self.letters_s, self.text_s, self.text_bytes = 0.0, 0.0, 0

    def provider(self):
        return SM.MafTextProvider(C.cast(self.cl, C.c_void_p), C.cast(self.ct, C.c_void_p), None)

    def _letters(self, ctx, out):
        t = time.perf_counter()
        rc = self.engine.lib.sxg_poa_msa_row_letters(self.engine.h, out)
        self.letters_s += time.perf_counter() - t
        return rc

    def _text(self, ctx, inp, out, out_bytes):
        t = time.perf_counter()
        rc = self.engine.lib.sxg_poa_maf_text(self.engine.h, inp, out, out_bytes)
        self.text_s += time.perf_counter() - t
        self.text_bytes += out_bytes
        return rc


def iteration(sm, params, prov, texter):
    """One call (texter None: sxg_smooth_maf_gfa_device_rows) -> (wall s, SXG_SMOOTH_TIMING laps, (GFA, MAF, flips))"""
    mp = SM.MergeParams()
    sm.L.sxg_merge_default_params(C.byref(mp))
    mp.maf_header = b"##maf version=1"
    gfa, maf, nf = C.c_void_p(), C.c_void_p(), C.c_int64()
    run, fre, ctx = prov.provider()
    tp = texter.provider() if texter is not None else None
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            t0 = time.perf_counter()
            if tp is None:
                rc = sm.L.sxg_smooth_maf_gfa_device_rows(sm.g, sm.b, C.byref(params), C.byref(mp), run, fre, ctx, None, None, C.byref(gfa), C.byref(maf), C.byref(nf))
            else:
                rc = sm.L.sxg_smooth_maf_gfa_device_text(sm.g, sm.b, C.byref(params), C.byref(mp), run, fre, ctx, C.byref(tp), None, C.byref(gfa), C.byref(maf),
                                                         C.byref(nf))
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
    prov, texter = TimedProvider(engine), TimedTexter(engine)
    params = SM.default_params(add_consensus=1)
    out = dict(tool="maf_text_phase", workload=a.workload, blocks=nb, depth=depth, length=length, runs=a.runs, add_consensus=1, merge_blocks=0,
               host_threads=int(os.environ.get("OMP_NUM_THREADS") or len(os.sched_getaffinity(0))), setup_s=round(time.perf_counter() - t0, 2))
    rec = {k: dict(wall=[], prov=[], bytes=None, laps=[], letters=[], text=[], kernel_ms=[], text_bytes=0) for k in ("device_rows", "device_text")}
    res = {}
    for r in range(a.runs + 1):                                   # run 0 warms both parts up and is not recorded
        for name in ("device_rows", "device_text"):
            prov.calls.clear()
            texter.reset()
            ms0 = engine.maf_text_stats()[0]
            dt, laps, res[name] = iteration(sm, params, prov, None if name == "device_rows" else texter)
            if not r:
                continue
            R = rec[name]
            R["wall"].append(dt)
            R["prov"].append(sum(c["s"] for c in prov.calls))
            # (TimedProvider counts msa_off's total as downloaded rows; resident rows are not downloaded, the text is)
            R["bytes"] = sum(c["bytes"] - (c["msa_bytes"] if c["want_msa"] == P.MSA_TRIMMED_RESIDENT else 0) for c in prov.calls) + texter.text_bytes
            R["asked"] = sorted({(c["want_msa"], c["want_block_graph"]) for c in prov.calls})
            R["laps"].append(laps)
            if name == "device_text":
                R["letters"].append(texter.letters_s)
                R["text"].append(texter.text_s)
                R["kernel_ms"].append(engine.maf_text_stats()[0] - ms0)
                R["text_bytes"] = texter.text_bytes
    for name, R in rec.items():
        o = dict(wall_s=spread(R["wall"]), provider_wall_s=spread(R["prov"]), downloaded_bytes=R["bytes"], asked=R.get("asked"),
                 laps_s={k: spread([l.get(k, 0.0) for l in R["laps"]]) for k in (R["laps"][0] if R["laps"] else {})})
        if name == "device_text":
            o["letters_call_s"] = spread(R["letters"])
            o["text_call_s"] = spread(R["text"])
            o["text_kernel_ms"] = spread(R["kernel_ms"])
            o["text_bytes"] = int(R["text_bytes"])
            if R["kernel_ms"] and min(R["kernel_ms"]) > 0:
                o["text_kernel_GBps_read_plus_written"] = spread([2 * R["text_bytes"] / (ms * 1e-3) / 1e9 for ms in R["kernel_ms"]])
        out[name] = o
    out["pays"] = bool(out["device_text"]["wall_s"]["median"] < out["device_rows"]["wall_s"]["min"])
    out["copy_GBps_read_plus_written"] = round(engine.measure_copy(1 << 30, 5), 1)
    out["gfa_equal"] = bool(res["device_rows"][0] == res["device_text"][0])
    out["maf_equal"] = bool(res["device_rows"][1] == res["device_text"][1])
    out["flips"] = [int(res["device_rows"][2]), int(res["device_text"][2])]
    out["gfa_bytes"], out["maf_bytes"] = len(res["device_text"][0]), len(res["device_text"][1])
    engine.close()
    text = json.dumps(out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
