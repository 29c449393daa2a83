"""Independent restatement of `prep` (src/prep.cpp:11-163) as DESIGN.md section 9 decrees it: the deterministic path-guided
SGD node order (decree Y, Y1-Y7) and the host steps around it (flatten, apply the order, chop: decree C).  Test
infrastructure in numpy, shares no code with the product.

  schedule      Y2: (eta[iter_max], cooling_start, terms_per_iter) from the path lengths in steps;
  sgd_order     Y1, Y3-Y7: (order, X) -- one batch at a time, every term of a batch at once (the integer sums of Y6 do not
                depend on the order of their terms, so np.add.at IS the decree);
  parse_gfa / flatten / apply_order / chop / to_gfa   the host half; prep_gfa strings them together around a sorter.

A graph here is (seqs by rank, paths as (name, [(rank, is_reverse)]), edges as (rank, is_reverse, rank, is_reverse))."""
import math

import numpy as np

SHIFT = 20
ONE = float(1 << SHIFT)
U64 = np.uint64
DEFAULT_SEED = 9399220
LDS_NODES = 8192


def mix(x):
    """Y3: splitmix64's finaliser on an array of uint64 (wrapping)."""
    with np.errstate(over="ignore"):
        x = x + U64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> U64(27))) * U64(0x94D049BB133111EB)
        return x ^ (x >> U64(31))


def schedule(path_off, iter_max=100, eps=0.01, cooling=0.5, term_updates=1.0):
    """Y2.  iter_max == 1 has lambda = 0; no path has eta_max = 1."""
    path_off = np.asarray(path_off, np.int64)
    steps = np.diff(path_off)
    maxsteps = int(steps.max()) if len(steps) else 0
    eta_max = float(maxsteps) * float(maxsteps) if maxsteps > 0 else 1.0
    lam = math.log(eta_max / eps) / (iter_max - 1) if iter_max > 1 else 0.0
    eta = np.array([eta_max * math.exp(-lam * t) for t in range(iter_max)], np.float64)
    return eta, int(iter_max * cooling), int(term_updates * float(int(path_off[-1])))


def sgd_order(node_len, path_off, step_node, step_pos, eta, cooling_start, terms_per_iter, seed=DEFAULT_SEED):
    """Decree Y -> (order: old ranks in the new order, int32; X: int64 in units of 2^-20 bp)."""
    node_len = np.asarray(node_len, np.int64)
    path_off = np.asarray(path_off, np.int64)
    step_node = np.asarray(step_node, np.int64)
    step_pos = np.asarray(step_pos, np.int64)
    N, S = len(node_len), int(path_off[-1])
    total = int(node_len.sum())
    if total >= 1 << 40 or S >= 1 << 32 or N >= 1 << 31:
        raise ValueError("SXG_E_INVALID")
    X = np.zeros(N, np.int64)
    if N:
        X[1:] = np.cumsum(node_len)[:-1]
    X <<= SHIFT                                                                      # Y1
    steps = np.diff(path_off)
    maxsteps = int(steps.max()) if len(steps) else 0
    nb = max(1, (maxsteps - 1).bit_length()) if maxsteps > 0 else 1
    B = max(1, N // 8)                                                               # Y6
    if S == 0 or N == 0:
        terms_per_iter = 0
    for it in range(len(eta)):
        for k0 in range(0, terms_per_iter, B):
            k = np.arange(k0, min(k0 + B, terms_per_iter), dtype=U64)
            base = mix(U64(seed) ^ U64(it << 40) ^ k)                                # Y3
            r1 = mix(base)
            r2 = mix(r1)
            r3 = mix(r2)
            a = (r1 % U64(S)).astype(np.int64)                                       # Y4
            p = np.searchsorted(path_off, a, side="right") - 1
            n = steps[p]
            ia = a - path_off[p]
            bits = ((r2 >> U64(1)) % U64(nb)).astype(np.int64)
            j = (np.int64(1) << bits) + ((r2 >> U64(8)).astype(np.int64) & ((np.int64(1) << bits) - 1))
            fwd = ((r2 >> U64(7)) & U64(1)).astype(bool)
            ib = np.where(fwd, ia + j, ia - j)
            other = np.where(fwd, ia - j, ia + j)
            ib = np.where((ib < 0) | (ib >= n), other, ib)
            ib = np.clip(ib, 0, n - 1)
            zipf = ((r2 & U64(1)) != 0) | (it >= cooling_start)
            ib = np.where(zipf, ib, (r3 % n.astype(U64)).astype(np.int64))
            b = path_off[p] + ib
            na, nbd = step_node[a], step_node[b]
            pa = step_pos[a] + np.where(((r3 >> U64(62)) & U64(1)) != 0, node_len[na], 0)
            pb = step_pos[b] + np.where((r3 >> U64(63)) != 0, node_len[nbd], 0)
            d = np.abs(pa - pb)
            keep = (d != 0) & (na != nbd)
            i, jn, d = na[keep], nbd[keep], d[keep].astype(np.float64)
            dx = (X[i] - X[jn]).astype(np.float64) / ONE                             # Y5: every operation rounded once
            mag = np.abs(dx)
            sgn = np.where(dx > 0, 1.0, np.where(dx < 0, -1.0, np.where(i < jn, -1.0, 1.0)))
            mu = np.minimum(eta[it] / d, 1.0)
            delta = mu * (mag - d) / 2.0
            q = np.rint(delta * sgn * ONE).astype(np.int64)                          # half to even
            D = np.zeros(N, np.int64)
            np.subtract.at(D, i, q)
            np.add.at(D, jn, q)
            X += D                                                                   # Y6: the batch read the X of its start
    order = np.lexsort((np.arange(N), X)).astype(np.int32)                           # Y7: by (X, old rank)
    return order, X


# ---------------------------------------------------------------------------------------------------------------------
# the host half

def parse_gfa(text):
    nodes, plines, llines = [], [], []
    for line in text.split("\n"):
        f = line.rstrip("\r").split("\t")
        if f[0] == "S" and len(f) >= 3:
            nodes.append((int(f[1]), "".join(c if c in "ACGT" else "N" for c in f[2].upper())))
        elif f[0] == "P" and len(f) >= 3:
            plines.append((f[1], f[2]))
        elif f[0] == "L" and len(f) >= 5:
            llines.append((int(f[1]), f[2] == "-", int(f[3]), f[4] == "-"))
    nodes.sort(key=lambda t: t[0])
    rank = {nid: r for r, (nid, _) in enumerate(nodes)}
    seqs = [s for _, s in nodes]
    paths = [(name, [(rank[int(st[:-1])], st[-1] == "-") for st in steps.split(",") if st]) for name, steps in plines]
    edges = [(rank[a], ar, rank[b], br) for a, ar, b, br in llines]
    return seqs, paths, edges


def flatten(seqs, paths):
    """Y's inputs: (node_len, path_off, step_node, step_pos)."""
    node_len = np.array([len(s) for s in seqs], np.int32)
    path_off = np.zeros(len(paths) + 1, np.int64)
    step_node, step_pos = [], []
    for p, (_, steps) in enumerate(paths):
        bp = 0
        for r, _ in steps:
            step_node.append(r)
            step_pos.append(bp)
            bp += len(seqs[r])
        path_off[p + 1] = len(step_node)
    return node_len, path_off, np.array(step_node, np.int32), np.array(step_pos, np.int64)


def apply_order(seqs, paths, edges, order):
    """Node of old rank order[k] becomes rank k (id k + 1)."""
    new = np.empty(len(order), np.int64)
    new[np.asarray(order, np.int64)] = np.arange(len(order))
    new = new.tolist()
    return ([seqs[r] for r in order], [(nm, [(new[r], rv) for r, rv in st]) for nm, st in paths],
            [(new[a], ar, new[b], br) for a, ar, b, br in edges])


def chop(seqs, paths, edges, max_node_length):
    """Decree C."""
    first, last, out = [], [], []
    for s in seqs:
        first.append(len(out))
        out += [s[k:k + max_node_length] for k in range(0, len(s), max_node_length)] or [s]
        last.append(len(out) - 1)
    npaths = []
    for nm, st in paths:
        ns = []
        for r, rv in st:
            pieces = range(first[r], last[r] + 1)
            ns += [(q, True) for q in reversed(pieces)] if rv else [(q, False) for q in pieces]
        npaths.append((nm, ns))
    nedges = [(first[a] if ar else last[a], ar, last[b] if br else first[b], br) for a, ar, b, br in edges]
    for r in range(len(seqs)):
        nedges += [(q, False, q + 1, False) for q in range(first[r], last[r])]
    return out, npaths, nedges


def to_gfa(seqs, paths, edges):
    o = ["H\tVN:Z:1.0"]
    o += ["S\t%d\t%s" % (k + 1, s) for k, s in enumerate(seqs)]
    o += ["L\t%d\t%s\t%d\t%s\t0M" % (a + 1, "-" if ar else "+", b + 1, "-" if br else "+") for a, ar, b, br in sorted(set(edges))]
    o += ["P\t%s\t%s\t*" % (nm, ",".join("%d%s" % (r + 1, "-" if rv else "+") for r, rv in st)) for nm, st in paths]
    return "\n".join(o) + "\n"


def prep_gfa(text, sorter=None, max_node_length=100, term_updates=1.0, iter_max=100, eps=0.01, cooling=0.5, seed=DEFAULT_SEED):
    """flatten -> Y2 -> sorter(node_len, path_off, step_node, step_pos, eta, cooling_start, terms_per_iter, seed) -> order
    -> apply -> chop -> GFA text.  sorter None: sgd_order."""
    seqs, paths, edges = parse_gfa(text)
    node_len, path_off, step_node, step_pos = flatten(seqs, paths)
    eta, cooling_start, terms = schedule(path_off, iter_max, eps, cooling, term_updates)
    if sorter is None:
        order = sgd_order(node_len, path_off, step_node, step_pos, eta, cooling_start, terms, seed)[0]
    else:
        order = sorter(node_len, path_off, step_node, step_pos, eta, cooling_start, terms, seed)
    return to_gfa(*chop(*apply_order(seqs, paths, edges, order), max_node_length))


# ---------------------------------------------------------------------------------------------------------------------
# inputs the tests share

def path_sequences(seqs, paths):
    comp = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
    return {nm: "".join("".join(comp[c] for c in reversed(seqs[r])) if rv else seqs[r] for r, rv in st) for nm, st in paths}


def shuffled_linear(n_nodes, n_paths, seed, skip=0.1, max_len=20):
    """A chain of n_nodes nodes whose ranks are shuffled; every path walks the chain and skips a node now and then.
    -> (node_len, path_off, step_node, step_pos)."""
    rng = np.random.default_rng(seed)
    rank_of = rng.permutation(n_nodes)
    node_len = np.zeros(n_nodes, np.int32)
    node_len[rank_of] = rng.integers(1, max_len + 1, n_nodes)
    path_off, step_node, step_pos = [0], [], []
    for _ in range(n_paths):
        walk = rank_of[rng.random(n_nodes) >= skip]
        lens = node_len[walk].astype(np.int64)
        step_node.append(walk)
        step_pos.append(np.cumsum(lens) - lens)
        path_off.append(path_off[-1] + len(walk))
    return node_len, np.array(path_off, np.int64), np.concatenate(step_node).astype(np.int32), np.concatenate(step_pos).astype(np.int64)


def synthetic_gfa(seed=0, n_nodes=60, n_paths=5):
    """A GFA with shuffled ids, nodes of 1, 100, 101 and 250 bases among others, reverse steps, L lines written in either of
    their two forms and some of them twice."""
    rng = np.random.default_rng(seed)
    lens = [1, 100, 101, 250, 7, 33, 200, 2]
    ids = (rng.permutation(n_nodes) + 1).tolist()                 # id of the k-th node of the chain
    seqs = ["".join("ACGT"[c] for c in rng.integers(0, 4, lens[k % len(lens)])) for k in range(n_nodes)]
    flipped = rng.random(n_nodes) < 0.3                             # nodes stored reverse-complemented: walked as id-
    lines = ["H\tVN:Z:1.0"]
    store = lambda k: "".join({"A": "T", "C": "G", "G": "C", "T": "A"}[c] for c in reversed(seqs[k])) if flipped[k] else seqs[k]  # noqa: E731
    lines += ["S\t%d\t%s" % (ids[k], store(k)) for k in range(n_nodes)]
    edges, plines = [], []
    for p in range(n_paths):
        walk = [k for k in range(n_nodes) if rng.random() >= 0.15]
        back = p % 2 == 1                                           # odd paths walk the chain backwards
        st = [(ids[k], bool(flipped[k]) != back) for k in (reversed(walk) if back else walk)]
        plines.append("P\tpath%d\t%s\t*" % (p, ",".join("%d%s" % (i, "-" if r else "+") for i, r in st)))
        for (a, ar), (b, br) in zip(st, st[1:]):
            e = (a, ar, b, br) if rng.random() < 0.5 else (b, not br, a, not ar)
            edges += [e] * (2 if rng.random() < 0.1 else 1)
    lines += ["L\t%d\t%s\t%d\t%s\t0M" % (a, "-" if ar else "+", b, "-" if br else "+") for a, ar, b, br in edges]
    return "\n".join(lines + plines) + "\n"
