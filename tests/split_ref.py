"""Independent restatement of the identity split of break_blocks (src/breaks.cpp:335-586) as DESIGN.md section 9 decrees
it (P1-P4): test infrastructure, shares no code with the product.

  pair_triple   P1: the lexicographically smallest (penalty, cols, nonmatch) over all global alignments, by the three-state
                recurrence, one row at a time in numpy (the in-row state by np.minimum.accumulate);
  pair_identity P2: (penalty, cols, matches) with cols = matches = 0 when penalty >= cap;
  brute_triple  the same optimum by enumerating every alignment (tiny inputs only);
  gotoh_penalty a plain gap-affine distance written separately (scalars, three matrices);
  greedy        P3 on dedup'd, sorted sequences -> (group id per sequence, number of groups, pair sweeps);
  dedup_sort / split_block   the host half of P3: dedup (equal or reverse complement), guards, sort, reassembly.

Sequences are arrays / lists of codes 0..4 (A, C, G, T, N); N is a letter like any other."""
import numpy as np

MISMATCH, GAP_OPEN, GAP_EXT = 7, 11, 1
SH_P, SH_C = 40, 20                      # one integer key per triple: penalty << 40 | cols << 20 | nonmatch
K_MATCH = 1 << SH_C                                           # (0, 1, 0)
K_MISMATCH = (MISMATCH << SH_P) | (1 << SH_C) | 1             # (7, 1, 1)
K_OPEN_NEW = ((GAP_OPEN + GAP_EXT) << SH_P) | (1 << SH_C) | 1  # (12, 1, 1): a gap after a diagonal column (or at the start)
K_OPEN_SWITCH = (GAP_OPEN + GAP_EXT) << SH_P                  # (12, 0, 0): a gap after a gap of the other kind
K_EXT = GAP_EXT << SH_P                                       # (1, 0, 0)
INF = 1 << 61


def _unkey(k):
    k = int(k)
    return k >> SH_P, (k >> SH_C) & ((1 << SH_C) - 1), k & ((1 << SH_C) - 1)


def revcomp(s):
    s = np.asarray(s, np.uint8)
    return np.where(s < 4, 3 - s, s)[::-1].astype(np.uint8)


def pair_triple(a, b):
    """P1.  Rows run over a, columns over b; M / I / D = last column diagonal / consumed a / consumed b."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    n, m = len(a), len(b)
    assert n >= 1 and m >= 1
    j = np.arange(m + 1, dtype=np.int64)
    M = np.full(m + 1, INF, np.int64)
    I = np.full(m + 1, INF, np.int64)
    D = np.full(m + 1, INF, np.int64)
    M[0] = 0
    D[1:] = K_OPEN_NEW + (j[1:] - 1) * K_EXT
    for i in range(1, n + 1):
        best = np.minimum(np.minimum(M, I), D)
        nM = np.full(m + 1, INF, np.int64)
        nM[1:] = best[:-1] + np.where(b == a[i - 1], K_MATCH, K_MISMATCH)
        nI = np.minimum(np.minimum(I + K_EXT, M + K_OPEN_NEW), D + K_OPEN_SWITCH)
        # D[j] = min over k < j of open[k] + (j - 1 - k) * ext: a running minimum of open[k] - k * ext
        opn = np.minimum(nM + K_OPEN_NEW, nI + K_OPEN_SWITCH)
        run = np.minimum.accumulate(opn - j * K_EXT)
        nD = np.full(m + 1, INF, np.int64)
        nD[1:] = run[:-1] + (j[1:] - 1) * K_EXT
        M, I, D = nM, nI, np.minimum(nD, INF)
    return _unkey(min(M[m], I[m], D[m]))


def pair_identity(a, b, cap):
    """P2: (penalty, cols, matches); cols = matches = 0 when the optimal penalty is not below cap."""
    p, c, x = pair_triple(a, b)
    if p >= cap:
        return p, 0, 0
    return p, c, c - x


def brute_triple(a, b):
    """Every alignment of a and b, column by column; the smallest triple."""
    a, b = list(a), list(b)
    best = [None]

    def cost(cols):
        pen = ncol = non = 0
        prev = None
        for op in cols:
            if op == "=":
                ncol += 1
            elif op == "X":
                pen += MISMATCH
                ncol += 1
                non += 1
            else:
                if prev == op:
                    pen += GAP_EXT
                else:
                    pen += GAP_OPEN + GAP_EXT
                    if prev not in ("I", "D"):
                        ncol += 1
                        non += 1
            prev = op
        return pen, ncol, non

    def rec(i, k, cols):
        if i == len(a) and k == len(b):
            t = cost(cols)
            if best[0] is None or t < best[0]:
                best[0] = t
            return
        if i < len(a) and k < len(b):
            rec(i + 1, k + 1, cols + ["=" if a[i] == b[k] else "X"])
        if i < len(a):
            rec(i + 1, k, cols + ["I"])
        if k < len(b):
            rec(i, k + 1, cols + ["D"])

    rec(0, 0, [])
    return best[0]


def gotoh_penalty(a, b):
    """Gap-affine distance (mismatch 7, gap of k: 11 + k), scalar code with three full matrices."""
    n, m = len(a), len(b)
    big = 10 ** 9
    H = [[big] * (m + 1) for _ in range(n + 1)]
    E = [[big] * (m + 1) for _ in range(n + 1)]
    F = [[big] * (m + 1) for _ in range(n + 1)]
    H[0][0] = 0
    for i in range(n + 1):
        for k in range(m + 1):
            if i == 0 and k == 0:
                continue
            if k > 0:
                E[i][k] = min(E[i][k - 1] + GAP_EXT, H[i][k - 1] + GAP_OPEN + GAP_EXT)
            if i > 0:
                F[i][k] = min(F[i - 1][k] + GAP_EXT, H[i - 1][k] + GAP_OPEN + GAP_EXT)
            d = H[i - 1][k - 1] + (0 if a[i - 1] == b[k - 1] else MISMATCH) if i > 0 and k > 0 else big
            H[i][k] = min(d, E[i][k], F[i][k])
    return H[n][m]


def greedy(seqs, t, ratio_min, pair=pair_identity):
    """P3 on dedup'd sequences sorted by (length, letters): -> (group of every sequence, groups, pair sweeps run)."""
    n = len(seqs)
    groups = [[0]]
    n_pairs = 0
    one_minus = 1.0 - t
    thr = (1 << 64) - 1 if one_minus == 0 else int(t / one_minus)
    for i in range(1, n):
        curr_len = len(seqs[i])
        found = -1
        for curr in (np.asarray(seqs[i], np.uint8), revcomp(seqs[i])):
            for g in range(len(groups) - 1, -1, -1):
                for k in reversed(groups[g]):
                    other_len = len(seqs[k])
                    if float(other_len) / float(curr_len) < ratio_min:
                        break
                    if other_len < curr_len and other_len < thr:
                        break
                    n_pairs += 1
                    pen, cols, matches = pair(curr, seqs[k], curr_len)
                    if cols > 0 and float(matches) / float(cols) >= t:
                        found = g
                        break
                if found >= 0:
                    break
            if found >= 0:
                break
        if found >= 0:
            groups[found].append(i)
        else:
            groups.append([i])
    grp = [0] * n
    for g, mem in enumerate(groups):
        for k in mem:
            grp[k] = g
    return grp, len(groups), n_pairs


def dedup_sort(seqs):
    """Dedup by 'equal to a kept sequence or to its reverse complement' (first occurrence kept, in its orientation), then
    the sort by (length, letters): -> (sorted kept sequences, the original ranks of each)."""
    kept, ranks = [], []
    for r, s in enumerate(seqs):
        s = bytes(bytearray(np.asarray(s, np.uint8).tolist()))
        rc = bytes(bytearray(revcomp(np.frombuffer(s, np.uint8)).tolist())) if len(s) else s
        for q, u in enumerate(kept):
            if s == u or rc == u:
                ranks[q].append(r)
                break
        else:
            kept.append(s)
            ranks.append([r])
    # the reference sorts the strings: letters in ASCII order (A < C < G < N < T)
    order = sorted(range(len(kept)), key=lambda q: (len(kept[q]), kept[q].translate(bytes(bytearray(b"ACGTN") + bytearray(251)))))
    return [np.frombuffer(kept[q], np.uint8) for q in order], [ranks[q] for q in order]


def split_block(seqs, t, ratio_min, min_dedup_depth, pair=pair_identity):
    """The whole of P3 for one block given the sequences of its ranges: a list of new blocks, each a list of original
    range ranks (one block with every rank in order when the block stays whole), and the pair sweeps run."""
    whole = [list(range(len(seqs)))]
    if not (t > 0 and len(seqs) > 1):
        return whole, 0
    srt, ranks = dedup_sort(seqs)
    if not (min_dedup_depth != 0 and len(srt) >= min_dedup_depth):
        return whole, 0
    grp, ng, n_pairs = greedy(srt, t, ratio_min, pair)
    if ng == 1:
        return whole, n_pairs
    out = [[] for _ in range(ng)]
    for q in range(len(srt)):          # members join their group in ascending q: insertion order
        out[grp[q]] += ranks[q]
    return out, n_pairs
