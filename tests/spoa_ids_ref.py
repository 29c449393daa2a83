"""A plain-Python POA graph with either rule for the ids of new nodes (decrees S6 and S6' of DESIGN.md section 2) under
spoa's re-sort (decree S7').  TEST INFRASTRUCTURE: the reference of the opt-in mode SXG_IDS_SPOA, which the oracle
(oracle/poa_oracle.c) cannot produce.  It shares no text with smoothxg_amd/csrc/poa_graph_dev.h: per-node Python lists, one
sequential depth-first walk, aligned-node lists kept as they grow.  Only the DP and its walk come from the oracle
(oracle_py.align_csr over the rank-space rows of decree S2), as in tests/test_oracle.py and tests/csrc/graph_emul.cpp.

Both rules are RECOLLECTED from spoa's Graph::AddAlignment / TopologicalSort (the library is absent): unverified.
"""
import numpy as np

from oracle import oracle_py as O


class Result:
    """What run_block returns: node code / rank / group, edges in creation order, per-sequence paths, scores."""

    def __init__(self, g, scores):
        self.node_code = np.asarray(g.code, np.uint8)
        self.node_rank = np.asarray(g.rank, np.int32)
        self.node_group = np.asarray(g.group, np.int32)
        self.edge_tail = np.asarray([e[0] for e in g.edges], np.int32)
        self.edge_head = np.asarray([e[1] for e in g.edges], np.int32)
        self.edge_weight = np.asarray([e[2] for e in g.edges], np.uint32)
        self.paths = [np.asarray(p, np.int32) for p in g.paths]
        self.scores = np.asarray(scores, np.int32)
        self.spans = list(g.spans)   # per sequence: (first, last) position of its walk, None for an empty walk


class Graph:
    def __init__(self):
        self.code = []       # letter of node v
        self.group = []      # the first node of v's aligned group
        self.aligned = []    # spoa's aligned-node list of v
        self.ins = []        # tails of v's in-edges, insertion order
        self.outs = []       # heads of v's out-edges, insertion order
        self.edges = []      # [tail, head, weight], creation order
        self.edge_of = {}    # (tail, head) -> index into edges
        self.order = []      # node of every rank
        self.rank = []
        self.paths = []
        self.spans = []

    # ---- decree S2: rows = nodes in rank order, predecessors (row number, 1-based) in in-edge insertion order, sink flags
    def rows(self):
        codes = [self.code[v] for v in self.order]
        off, pred = [0], []
        for v in self.order:
            pred.extend(self.rank[t] + 1 for t in self.ins[v])
            off.append(len(pred))
        sink = [0 if self.outs[v] else 1 for v in self.order]
        return codes, off, pred, sink

    def _new_node(self, c, beside):
        v = len(self.code)
        self.code.append(c)
        self.ins.append([])
        self.outs.append([])
        if beside is None:
            self.group.append(v)
            self.aligned.append([])
        else:
            # a node created aligned to x starts with x's list followed by x, and joins the list of every member the group had
            self.group.append(self.group[beside])
            self.aligned.append(self.aligned[beside] + [beside])
            for m in self.aligned[v]:
                self.aligned[m].append(v)
        return v

    # ---- decree S6 / S6': reuse, aligned sibling, new sibling; weight += 2 w along the path
    def add(self, seq, pairs, weight, ids):
        L = len(seq)
        at = [-1] * L                       # the node position i is aligned to
        walk_pos = [p for _, p in pairs if p >= 0]
        for v, p in pairs:
            if v >= 0 and p >= 0:
                at[p] = v
        span = (walk_pos[0], walk_pos[-1]) if walk_pos else None
        self.spans.append(span)
        target = [-1] * L
        fresh = []                          # positions that need a new node
        for i in range(L):
            c = min(int(seq[i]), 4)
            a = at[i]
            if a >= 0:
                for m in [a] + self.aligned[a]:
                    if self.code[m] == c:
                        target[i] = m
            if target[i] < 0:
                fresh.append(i)
        if ids == "spoa" and span is not None:
            first, last = span
            fresh = [i for i in fresh if i < first] + [i for i in fresh if i > last] + [i for i in fresh if first <= i <= last]
        elif ids not in ("spoa", "sequence"):
            raise ValueError(ids)
        for i in fresh:                     # ids in this order
            target[i] = self._new_node(min(int(seq[i]), 4), at[i] if at[i] >= 0 else None)
        for i in range(1, L):
            key = (target[i - 1], target[i])
            e = self.edge_of.get(key)
            if e is None:
                self.edge_of[key] = len(self.edges)
                self.edges.append([key[0], key[1], 2 * weight])
                self.outs[key[0]].append(key[1])
                self.ins[key[1]].append(key[0])
            else:
                self.edges[e][2] += 2 * weight
        self.paths.append(target)

    # ---- decree S7': for every node in id order, depth-first with an explicit stack
    def resort(self):
        n = len(self.code)
        done = [False] * n
        as_aligned = [False] * n            # pushed as somebody's aligned node ("ignored")
        order = []
        for root in range(n):
            if done[root]:
                continue
            stack = [root]
            while stack:
                v = stack[-1]
                if done[v]:
                    stack.pop()
                    continue
                ready = True
                for t in self.ins[v]:
                    if not done[t]:
                        stack.append(t)
                        ready = False
                if not as_aligned[v]:
                    for m in self.aligned[v]:
                        if not done[m]:
                            stack.append(m)
                            as_aligned[m] = True
                            ready = False
                if ready:
                    done[v] = True
                    if not as_aligned[v]:
                        order.append(v)
                        order.extend(self.aligned[v])
                    stack.pop()
        assert len(order) == n and len(set(order)) == n
        self.order = order
        self.rank = [0] * n
        for r, v in enumerate(order):
            self.rank[v] = r


def run_block(seqs, weights, params, ids="spoa"):
    """One block: every sequence aligned (oracle DP, params.mode & 1: local 0 / global 1) to the graph of those before it, added under
    the chosen id rule, the graph re-sorted (S7') after every one.  weights: None = 1 each."""
    g = Graph()
    scores = []
    for s, seq in enumerate(seqs):
        seq = np.asarray(seq, np.uint8)
        pairs, sc = [], 0
        if g.code and len(seq):
            codes, off, pred, sink = g.rows()
            an, ap, sc = O.align_csr(codes, off, pred, sink, seq, params)
            pairs = [(g.order[r] if r >= 0 else -1, int(p)) for r, p in zip(an.tolist(), ap.tolist())]
        scores.append(sc)
        g.add(seq.tolist(), pairs, 1 if weights is None else int(weights[s]), ids)
        g.resort()
    return Result(g, scores)
