"""Independent restatement of the mash-based branch of the identity split (src/breaks.cpp:388-471) as DESIGN.md section 9
decrees it (M1-M5): test infrastructure, shares no code with the product.

  kmer_set      M1: the distinct canonical k-mers of a sequence as a sorted uint64 array (Python ints, np.unique);
  thresholds    M3: (f, jmin) in double;
  greedy_mash   M4 on dedup'd, sorted sequences -> (group id per sequence, number of groups, pair sweeps, set comparisons);
  block_min_len M2: the per-block decision the host library takes;
  split_block_mash  the host half with M2 in it, as split_ref.split_block.

greedy_mash asserts that no comparison lies within MARGIN of jmin: a last-bit difference between two exp implementations
must not decide a test."""
import math

import numpy as np

import split_ref as R

MARGIN = 1e-9


def kmer_set(s, k):
    """M1.  Codes 0..3 pack into 2 bits each, first letter highest; a window with a code > 3 contributes nothing."""
    s = np.asarray(s, np.uint8)
    n = len(s) - k + 1
    if n <= 0:
        return np.zeros(0, np.uint64)
    fw, rc, bad = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, bool)
    for q in range(k):                       # letter q of every window at once
        c = s[q:q + n]
        bad |= c > 3
        c = (c & 3).astype(np.uint64)
        fw |= c << np.uint64(2 * (k - 1 - q))
        rc |= (np.uint64(3) - c) << np.uint64(2 * q)      # the complement of letter q is letter k-1-q of the other strand
    return np.unique(np.minimum(fw, rc)[~bad])


def thresholds(t, e, k):
    """M3: f = v / (2 - v), v = exp(-(1 - t) k); jmin = w / (2 - w), w = exp(-(1 - e) k)."""
    v = math.exp(-(1.0 - t) * k)
    w = math.exp(-(1.0 - e) * k)
    return v / (2.0 - v), w / (2.0 - w)


def greedy_mash(seqs, t, ratio_min, k, min_len, e=None, pair=R.pair_identity, size_break=True):
    """M4 on dedup'd sequences sorted by (length, letters): -> (groups, n_groups, n_pairs, n_mash).  min_len = 0: P3."""
    if min_len == 0:
        return R.greedy(seqs, t, ratio_min, pair) + (0,)
    assert min_len >= k and 0 < t <= 1
    e = t if e is None or e <= 0 else e
    f, jmin = thresholds(t, e, k)
    n = len(seqs)
    sets = [set(kmer_set(s, k).tolist()) if len(s) >= min_len else set() for s in seqs]
    groups = [[0]]
    n_pairs = n_mash = 0
    one_minus = 1.0 - t
    thr = (1 << 64) - 1 if one_minus == 0 else int(t / one_minus)
    for i in range(1, n):
        curr_len = len(seqs[i])
        size_thr = int(float(len(sets[i])) * f)
        found = -1
        for fwd, curr in ((True, np.asarray(seqs[i], np.uint8)), (False, R.revcomp(seqs[i]))):
            for g in range(len(groups) - 1, -1, -1):
                for m in reversed(groups[g]):
                    other_len = len(seqs[m])
                    if float(other_len) / float(curr_len) < ratio_min:
                        break
                    if curr_len >= min_len and other_len >= min_len:
                        if not fwd:
                            continue
                        if size_break and len(sets[m]) < size_thr:
                            break
                        n_mash += 1
                        inter = len(sets[i] & sets[m])
                        uni = len(sets[i]) + len(sets[m]) - inter
                        if uni > 0:
                            j = float(inter) / float(uni)
                            assert abs(j - jmin) > MARGIN, (i, m, j, jmin)
                            if j >= jmin:
                                found = g
                                break
                        continue
                    if other_len < curr_len and other_len < thr:
                        break
                    n_pairs += 1
                    pen, cols, matches = pair(curr, seqs[m], curr_len)
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
        for m in mem:
            grp[m] = g
    return grp, len(groups), n_pairs, n_mash


def block_min_len(n_dedup, min_len_mash, min_depth_mash):
    """M2: the min_len a block of n_dedup sequences is given (0 = P3 only)."""
    return min_len_mash if min_len_mash > 0 and (min_depth_mash == 0 or n_dedup >= min_depth_mash) else 0


def split_block_mash(seqs, t, ratio_min, min_dedup_depth, min_len_mash, min_depth_mash, e, k):
    """split_ref.split_block with M2 and M4: -> (new blocks as lists of original range ranks, n_pairs, n_mash)."""
    whole = [list(range(len(seqs)))]
    if not (t > 0 and len(seqs) > 1):
        return whole, 0, 0
    srt, ranks = R.dedup_sort(seqs)
    if not (min_dedup_depth != 0 and len(srt) >= min_dedup_depth):
        return whole, 0, 0
    grp, ng, n_pairs, n_mash = greedy_mash(srt, t, ratio_min, k, block_min_len(len(srt), min_len_mash, min_depth_mash), e)
    if ng == 1:
        return whole, n_pairs, n_mash
    out = [[] for _ in range(ng)]
    for q in range(len(srt)):
        out[grp[q]] += ranks[q]
    return out, n_pairs, n_mash
