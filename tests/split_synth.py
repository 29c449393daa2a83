"""Synthetic inputs of the identity-split tests (test infrastructure): sequence families and a GFA whose blocks hold them."""
import numpy as np


def mutate(rng, s, n_sub=0, indels=()):
    """s with n_sub substitutions and the given indels ((+k: insertion of k random letters, -k: deletion of k))."""
    s = np.array(s, np.uint8)
    if n_sub:
        pos = rng.choice(len(s), size=min(n_sub, len(s)), replace=False)
        s[pos] = (s[pos] + rng.integers(1, 4, len(pos))) % 4
    for k in indels:
        p = int(rng.integers(1, max(2, len(s) - abs(k) - 1)))
        if k > 0:
            s = np.concatenate([s[:p], rng.integers(0, 4, k).astype(np.uint8), s[p:]])
        elif len(s) + k >= 1:
            s = np.concatenate([s[:p], s[p - k:]])
    return s.astype(np.uint8)


def families(rng, n_fam, per_fam, length, within_sub, across_sub, indel_every=0):
    """n_fam families of per_fam sequences: the family roots differ from one ancestor by across_sub substitutions each,
    the members from their root by within_sub (+ an indel of 1-3 bases for every indel_every-th member)."""
    anc = rng.integers(0, 4, length).astype(np.uint8)
    out = []
    for f in range(n_fam):
        root = mutate(rng, anc, across_sub) if f else anc
        for m in range(per_fam):
            ind = ((int(rng.integers(1, 4)) * (1 if m % 2 else -1)),) if indel_every and m % indel_every == indel_every - 1 else ()
            out.append((f, mutate(rng, root, within_sub, ind)))
    return out


def blocks_gfa(blocks, node_bp=40):
    """A GFA with one path per row of `blocks` position: blocks[k] is a list of code arrays, sequence q of every block lies
    on path q (a path only has the blocks that are deep enough), every path on its own chain of nodes.  Returns (GFA
    text, the blockset as lists of (path, step_begin, step_end), the blocks' sequences as given)."""
    n_paths = max(len(b) for b in blocks)
    lines, plines, nid = ["H\tVN:Z:1.0"], [], 1
    ranges = [[] for _ in blocks]
    for q in range(n_paths):
        steps = []
        for k, blk in enumerate(blocks):
            if q >= len(blk):
                continue
            text = "".join("ACGTN"[c] for c in blk[q])
            begin = len(steps)
            for a in range(0, len(text), node_bp):
                lines.append("S\t%d\t%s" % (nid, text[a:a + node_bp]))
                steps.append("%d+" % nid)
                nid += 1
            ranges[k].append((q, begin, len(steps)))
        plines.append("P\tpath%d\t%s\t*" % (q, ",".join(steps)))
    return "\n".join(lines + plines) + "\n", ranges, blocks


def two_family_gfa(seed, per_fam=4, backbone=12, node_bp=20, flank=30):
    """A variation graph between two shared flank nodes: two families, each on its own chain of backbone nodes with a
    two-allele SNP node after every backbone node; a member path picks its alleles at random.  Blocks that block discovery
    finds over it mix the two families."""
    rng = np.random.default_rng(seed)
    rnd = lambda n: "".join("ACGT"[c] for c in rng.integers(0, 4, n))
    lines, links, nid = ["H\tVN:Z:1.0", "S\t1\t" + rnd(flank)], set(), 2
    fam_nodes = []
    for f in range(2):
        chain = []
        for _ in range(backbone):
            lines.append("S\t%d\t%s" % (nid, rnd(node_bp)))
            a = int(rng.integers(0, 4))
            lines.append("S\t%d\t%s" % (nid + 1, "ACGT"[a]))
            lines.append("S\t%d\t%s" % (nid + 2, "ACGT"[(a + 1) % 4]))
            chain.append((nid, nid + 1, nid + 2))
            nid += 3
        fam_nodes.append(chain)
    last = nid
    lines.append("S\t%d\t%s" % (last, rnd(flank)))
    plines = []
    for f in range(2):
        for m in range(per_fam):
            steps = [1]
            for bb, x, y in fam_nodes[f]:
                steps += [bb, x if rng.random() < 0.5 else y]
            steps.append(last)
            links.update(zip(steps, steps[1:]))
            plines.append("P\tfam%d_%d\t%s\t*" % (f, m, ",".join("%d+" % s for s in steps)))
    lines += ["L\t%d\t+\t%d\t+\t0M" % e for e in sorted(links)]
    return "\n".join(lines + plines) + "\n"
