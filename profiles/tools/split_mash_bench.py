#!/usr/bin/env python3
"""The identity split on one deep block and on a batch of shallow ones: the edit-based walk (PoaEngine.split) against the walk
with the mash-based branch (PoaEngine.split_mash) on the same batches, same process, warm-up then --runs runs each.

  python profiles/tools/split_mash_bench.py [--depth 2000] [--length 1000] [--families 8] [--shallow 500] [--runs 3]
                                            [--paths edit,mash] [--out FILE.json]

Prints (and writes to --out) one JSON object: per batch and path the kernel_ms of every run (HIP events around the kernels,
sxg_poa_stats), the wall time of the call, n_groups / n_pairs / n_mash summed over the batch, cells and device bytes.  The share
of the sketch kernel and of the walk kernel in a mash call is not in sxg_poa_stats: take it from one
`rocprofv3 --kernel-trace --stats -- python profiles/tools/split_mash_bench.py --paths mash --runs 1` (mash_sketch_kernel /
split_mash_kernel in the kernel statistics).

The edit-based walk of a deep block is one wavefront running ~depth^2 * (families - 1) / (2 * families) alignments of length^2
cells one after the other: choose --depth so that it ends (the JSON records what was run)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from smoothxg_amd import poa as P  # noqa: E402

T, K, MIN_LEN = 0.95, 17, 200


def substitute(rng, s, n):
    s = s.copy()
    pos = rng.choice(len(s), size=n, replace=False)
    s[pos] = (s[pos] + rng.integers(1, 4, n)) % 4
    return s


def family_block(rng, n_fam, per_fam, length, within, across):
    """n_fam roots `across` substitutions from one ancestor, members `within` substitutions (every third one also 1-3 bases
    shorter) from their root; distinct sequences sorted by (length, letters), as the host half of the split hands them over."""
    anc = rng.integers(0, 4, length).astype(np.uint8)
    seqs = {}
    for f in range(n_fam):
        root = substitute(rng, anc, across) if f else anc
        for m in range(per_fam):
            s = substitute(rng, root, within)
            if m % 3 == 2:
                cut = int(rng.integers(1, length - 4))
                s = np.concatenate([s[:cut], s[cut + int(rng.integers(1, 4)):]])
            seqs[s.tobytes()] = s
    return [seqs[key] for key in sorted(seqs, key=lambda b: (len(b), b))]


def measure(engine, name, blocks, runs):
    call = (lambda: engine.split(blocks, T, 0.0)) if name == "edit" else (lambda: engine.split_mash(blocks, T, 0.0, K, MIN_LEN))
    call()                                                       # warm-up
    kernel_ms, wall_ms, res, st = [], [], None, None
    for _ in range(runs):
        t0 = time.perf_counter()
        res = call()
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        st = engine.stats()
        kernel_ms.append(st["kernel_ms"])
    return dict(kernel_ms=[round(x, 3) for x in kernel_ms], wall_ms=[round(x, 3) for x in wall_ms],
                n_groups=int(sum(r[1] for r in res)), n_pairs=int(sum(r[2] for r in res)),
                n_mash=int(sum(r[3] for r in res)) if name == "mash" else 0,
                cells=int(st["cells"]), device_bytes=int(st["device_bytes"]), n_slots=int(st["n_slots"]),
                groups_digest=int(sum(int(g) * (q + 1) for r in res for q, g in enumerate(r[0])) % 1000000007))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=2000)
    ap.add_argument("--length", type=int, default=1000)
    ap.add_argument("--families", type=int, default=8)
    ap.add_argument("--shallow", type=int, default=500)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--paths", default="edit,mash")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    deep = family_block(rng, a.families, a.depth // a.families, a.length, a.length // 100, a.length * 15 // 100)
    shallow = [family_block(rng, 2, 4, 300, 3, 45) for _ in range(a.shallow)]
    engine = P.PoaEngine(0)
    out = dict(tool="split_mash_bench", identity=T, kmer_size=K, min_len=MIN_LEN, runs=a.runs,
               deep=dict(depth=len(deep), length=a.length, families=a.families), shallow=dict(blocks=len(shallow), depth=8, length=300))
    for name in a.paths.split(","):
        out["deep"][name] = measure(engine, name, [deep], a.runs)
        if shallow:
            out["shallow"][name] = measure(engine, name, shallow, a.runs)
    engine.close()
    text = json.dumps(out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
