"""Plain restatement of the row flags of the packed sweep's twin step (round 13; smoothxg_amd/csrc/poa_graph_dev.h::twin_flags),
on the row CSR the sweep walks: rows 0 .. n-1 in sweep order, off[r] .. off[r+1] the predecessors of row r as 1-based row
numbers (0 = the virtual start row) -- oracle Graph.rows() and RowsView alike.  Shared by tests/test_twin_rows.py,
tests/test_gpu_twin_rows.py and profiles/tools/twin_rows.py.

  ROW_TWIN on row r:   rows r and r + 1 have exactly one predecessor each, the same row; pairs are disjoint and a run of such
                       rows is paired from its start, up to LOOKBACK rows into the run.
  ROW_JOIN on row r+2: row r carries ROW_TWIN and rows r, r + 1 are both predecessors of row r + 2.
  stored:              a row with a reader the registers do not serve.  Served: the next row; the row after that when the next
                       row carries ROW_TWIN (the pair's shared predecessor); the row after that when the row itself carries
                       ROW_TWIN and that reader ROW_JOIN.
The old rule stores every row with a reader other than the next row."""
import numpy as np

ROW_STORE, ROW_SINK, ROW_REGPRED, ROW_TWIN, ROW_JOIN = 1, 2, 4, 8, 16
LOOKBACK = 8


def preds_of(off, pred):
    return [[int(x) for x in pred[off[r]:off[r + 1]]] for r in range(len(off) - 1)]


def pair_flags(preds, lookback=LOOKBACK):
    """(twin, join): boolean arrays over the rows.  Sequential: walks the runs of rows with the same single predecessor."""
    n = len(preds)
    twin, join = np.zeros(n, bool), np.zeros(n, bool)
    r = 0
    while r < n:
        if len(preds[r]) != 1:
            r += 1
            continue
        e = r + 1
        while e < n and preds[e] == preds[r]:
            e += 1
        for pos in range(0, e - r - 1, 2):   # rows r + pos and r + pos + 1
            if pos < lookback:
                twin[r + pos] = True
        r = e
    for r in range(2, n):
        join[r] = twin[r - 2] and (r - 1) in preds[r] and r in preds[r]   # (rows r - 2, r - 1 are the row numbers r - 1, r)
    return twin, join


def served(x, h, twin, join):
    """Does reader h of row x (both 0-based) find the row in the registers?"""
    return h == x + 1 or (h == x + 2 and bool(twin[x + 1])) or (h == x + 2 and bool(twin[x]) and bool(join[h]))


def row_flags(off, pred, new_rule=True, lookback=LOOKBACK):
    """dict: twin, join, stored (bool arrays), last (last reader of every row, 0-based, the row itself without readers),
    reads = [(reader, row read)] of every non-adjacent read, unserved = those the registers do not serve (all of them
    under the old rule)."""
    preds = preds_of(off, pred)
    n = len(preds)
    twin, join = pair_flags(preds, lookback) if new_rule else (np.zeros(n, bool), np.zeros(n, bool))
    stored, last = np.zeros(n, bool), np.arange(n)
    reads, unserved = [], []
    for h in range(n):
        for p in preds[h]:
            if p == 0:
                continue
            x = p - 1
            last[x] = max(last[x], h)
            if h != x + 1:
                reads.append((h, x))
                if not served(x, h, twin, join):
                    stored[x] = True
                    unserved.append((h, x))
    return dict(twin=twin, join=join, stored=stored, last=last, reads=reads, unserved=unserved, preds=preds)


def slots(stored, last, pool_slots, lds_rows):
    """finish_rows: -1 not stored; -2 - copy for a row that stays on the chip (at most lds_rows stored rows in [row, last reader));
    else the ring slot."""
    n = len(stored)
    sseq = np.concatenate([[0], np.cumsum(stored)])
    out = np.full(n, -1, np.int64)
    for r in range(n):
        if stored[r]:
            cnt = sseq[last[r]] - sseq[r]
            out[r] = -2 - sseq[r] % lds_rows if lds_rows > 0 and cnt <= lds_rows else sseq[r] % pool_slots
    return out


def census(off, pred):
    """Counts of the cases the twin step has to get right, for one graph."""
    f = row_flags(off, pred)
    preds, twin, join = f["preds"], f["twin"], f["join"]
    n = len(preds)
    readers = [[] for _ in range(n)]
    for h in range(n):
        for p in preds[h]:
            if p:
                readers[p - 1].append(h)
    c = dict(rows=n, twin_steps=int(twin.sum()), joins=int(join.sum()), twin_stored_pred=0, joins_more_preds=0, next_reads_first_only=0,
             next_reads_neither=0, runs_of_three=0, pair_after_pair=0, twin_rows_far_reader=0)
    for r in np.flatnonzero(twin):
        c["twin_stored_pred"] += preds[r][0] != r
        if r + 2 < n:
            nxt = preds[r + 2]
            c["joins_more_preds"] += bool(join[r + 2]) and len(nxt) > 2
            c["next_reads_first_only"] += (r + 1) in nxt and (r + 2) not in nxt
            c["next_reads_neither"] += (r + 1) not in nxt and (r + 2) not in nxt
            c["runs_of_three"] += nxt == preds[r]
            c["pair_after_pair"] += bool(twin[r + 2])
        for x in (r, r + 1):
            c["twin_rows_far_reader"] += any(h > x + 2 or (h == x + 2 and not served(x, h, twin, join)) for h in readers[x])
    return {k: int(v) for k, v in c.items()}


# ---- the test blocks (tests/test_twin_rows.py, tests/test_gpu_twin_rows.py)
# name -> (ancestor length, sequences, substitution rate, least and greatest deletion of every third sequence or None, seed)
# (SD: S's recipe with deletions of 250 letters -- the one block whose walks leave a plane of 480 columns)
BLOCKS = {"S": (1500, 8, 0.04, (1, 2), 1301), "L": (5200, 6, 0.03, None, 1302), "SD": (1500, 8, 0.04, (250, 250), 1301)}

_blocks = {}


def block(name):
    if name not in _blocks:
        n, k, sub, dels, seed = BLOCKS[name]
        rng = np.random.default_rng(seed)
        anc = rng.integers(0, 4, n, dtype=np.uint8)
        seqs = []
        for i in range(k):
            s = anc.copy()
            m = rng.random(n) < sub
            s[m] = (s[m] + rng.integers(1, 4, int(m.sum()), dtype=np.uint8)) & 3
            if dels and i % 3 == 2:
                pos, d = int(rng.integers(n // 4, 3 * n // 4)), int(rng.integers(dels[0], dels[1] + 1))
                s = np.concatenate([s[:pos], s[pos + d:]])
            seqs.append(s)
        _blocks[name] = seqs
    return _blocks[name]
