"""Builds smoothxg_amd/csrc/libsxgpoa.so for gfx950 with hipcc (in-tree, travels with gpurun)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
SO = os.path.join(CSRC, "libsxgpoa.so")
# sxg_poa.hip: host side of the C ABI; kern_part.hip: the kernel classes, compiled once per part of the class list
# (poa_classes.h, -DSXG_KERN_PART=k -> build/kern_partK.o) so that the parts compile side by side; kern_split.hip: the kernels
# of the identity split (poa_split.hip.h), of its mash-based branch (poa_mash.hip.h) and of the identity estimate of -a
# (poa_identity.hip.h); kern_sgd.hip: the kernels of the
# path-guided SGD node order (poa_sgd.hip.h), without floating-point contraction (decree Y5: one rounding per operation);
# kern_msa.hip: the kernels of the trimmed MSA (poa_msa.hip.h, arithmetic in poa_msa_cols.h); kern_repeat.hip: the kernels of the
# tandem-repeat scan (poa_repeat.hip.h, arithmetic in poa_repeat.h), without contraction as kern_sgd.hip (decree R3);
# kern_letters.hip: the range gather of the resident path letters (poa_letters.hip.h, arithmetic in poa_letters.h);
# kern_maf.hip: the MAF text gather and the letter count of the resident trimmed rows (poa_maf_text.hip.h, arithmetic in poa_maf_text.h)
KERN_PARTS = range(1, 10)
SOURCES = [("sxg_poa.hip", "sxg_poa.o", []), ("kern_split.hip", "kern_split.o", []), ("kern_msa.hip", "kern_msa.o", []),
           ("kern_sgd.hip", "kern_sgd.o", ["-ffp-contract=off"]), ("kern_repeat.hip", "kern_repeat.o", ["-ffp-contract=off"]),
           ("kern_letters.hip", "kern_letters.o", []), ("kern_maf.hip", "kern_maf.o", [])] + [("kern_part.hip", "kern_part%d.o" % k, ["-DSXG_KERN_PART=%d" % k]) for k in KERN_PARTS]
DEPS = ["sxg_poa.hip", "kern_part.hip", "poa_classes.h", "poa_slot_prof.h", "poa_cost.h", "poa_tiles.h", "poa_deal.h", "poa_results.h", "poa_devres.h", "poa_kernels.hip.h", "poa_kern_tables.hip.h", "poa_dp.hip.h", "poa_dp16.hip.h", "poa_dp16_fill.inc.h", "poa_dp16_row.inc.h", "poa_prep_rows.inc.h", "poa_rowcode.h", "poa_fields.h", "poa_band16.hip.h", "poa_graph_dev.h",
                  "poa_bgraph_dev.h", "poa_types.h", "kern_split.hip", "poa_split.hip.h", "poa_mash.hip.h", "poa_identity.hip.h", "poa_identity_key.h", "kern_sgd.hip", "poa_sgd.hip.h", "kern_msa.hip", "poa_msa.hip.h", "poa_msa_cols.h", "kern_repeat.hip", "poa_repeat.hip.h", "poa_repeat.h", "kern_letters.hip", "poa_letters.hip.h", "poa_letters.h", "kern_maf.hip", "poa_maf_text.hip.h", "poa_maf_text.h", os.path.join("..", "..", "include", "sxg_poa.h")]
OBJ_DIR = os.path.join(CSRC, "build")


def needs_build():
    if not os.path.exists(SO):
        return True
    t = os.path.getmtime(SO)
    return any(os.path.getmtime(os.path.join(CSRC, d)) > t for d in DEPS)


def build(force=False, verbose=False):
    """hipcc --offload-arch=gfx950 on every translation unit (in parallel: SXG_BUILD_JOBS, default = CPUs), then one link."""
    if not force and not needs_build():
        return SO
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"] + os.environ.get("SXG_HIPCC_FLAGS", "").split()
    os.makedirs(OBJ_DIR, exist_ok=True)
    jobs = max(1, int(os.environ.get("SXG_BUILD_JOBS", str(os.cpu_count() or 1))))
    objs, running, pending = [], [], list(SOURCES)
    failed = None
    while pending or running:
        while pending and len(running) < jobs and failed is None:
            src, obj, defs = pending.pop(0)
            obj = os.path.join(OBJ_DIR, obj)
            cmd = [hipcc] + flags + defs + ["-c", "-o", obj, os.path.join(CSRC, src)]
            if verbose:
                print(" ".join(cmd), flush=True)
            running.append((subprocess.Popen(cmd), cmd))
            objs.append(obj)
        if failed is not None:
            pending = []
        if not running:   # (fewer jobs than sources and the only running one failed: nothing left to wait for)
            break
        proc, cmd = running.pop(0)
        if proc.wait() != 0 and failed is None:
            failed = cmd
    if failed is not None:
        raise subprocess.CalledProcessError(1, failed)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", SO] + objs + ["-ldl"]   # (RCCL is dlopen-ed on first use)
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return SO


SMOOTH_SO = os.path.join(CSRC, "libsxgsmooth.so")
SMOOTH_DEPS = ["sxg_smooth.cpp", "prep_host.h", "poa_repeat.h", os.path.join("..", "..", "include", "sxg_smooth.h"),
               os.path.join("..", "..", "include", "sxg_poa.h")]


def build_smooth(force=False, verbose=False):
    """Host-side rows (collection, block graphs, lacing, GFA): plain g++, no HIP."""
    if not force and os.path.exists(SMOOTH_SO) and \
            all(os.path.getmtime(os.path.join(CSRC, d)) <= os.path.getmtime(SMOOTH_SO) for d in SMOOTH_DEPS):
        return SMOOTH_SO
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-fopenmp", "-Wall", "-o", SMOOTH_SO,
           os.path.join(CSRC, "sxg_smooth.cpp")]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return SMOOTH_SO


if __name__ == "__main__":
    build(force=True, verbose=True)
    build_smooth(force=True, verbose=True)
