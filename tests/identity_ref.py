"""Independent restatement of decree Q (include/sxg_poa.h): the identity estimate of the adaptive scores
in exact arithmetic -- Python ints and fractions.Fraction, no float anywhere but the rank of the percentile, which the decree
computes in double.  Test infrastructure, shares no code with the product.

  kmer_set      Q1: the distinct canonical k-mers of a coded sequence (codes 0..3, anything else breaks the window);
  key           Q2: uni ? floor(inter * 2^32 / uni) : 0;
  block         Q3 for one block: (n_used, inter, uni) of the pair at the percentile's rank, pairs ordered by J as Fractions;
  identify      a batch in the provider's layout -> (n_used, inter, uni, status), and the python_identifier-shaped `provider`;
  threshold     max(0.7f, f(J)) as float32: what the host library makes of one (inter, uni)."""
import math
from fractions import Fraction

import numpy as np

MAX_SEQ_LEN = 26623   # SXG_POA_MAX_SEQ_LEN
ST_OK, ST_TOO_LONG = 0, 5
E_BLOCK = -4


def kmer_set(codes, k):
    out, fw, rc, run = set(), 0, 0, 0
    mask = (1 << (2 * k)) - 1
    for c in codes:
        c = int(c)
        if c > 3:
            fw = rc = run = 0
            continue
        fw = ((fw << 2) | c) & mask
        rc = (rc >> 2) | ((3 - c) << (2 * (k - 1)))
        run += 1
        if run >= k:
            out.add(min(fw, rc))
    return out


def key(inter, uni):
    return (inter << 32) // uni if uni else 0


def jaccard(inter, uni):
    return Fraction(inter, uni) if inter and uni else Fraction(0)


def rank(n_pairs, percentile=0.30):
    return int(float(n_pairs - 1) * percentile)


def pair_counts(seqs, k):
    sets = [kmer_set(s, k) for s in seqs]
    out = []
    for i in range(len(sets)):
        for j in range(i + 1, len(sets)):
            inter = len(sets[i] & sets[j])
            out.append((inter, len(sets[i]) + len(sets[j]) - inter))
    return out


def block(seqs, k, min_len, percentile=0.30):
    """-> (n_used, inter, uni, status) of one block of coded sequences."""
    used = [s for s in seqs if len(s) >= min_len]
    if any(len(s) > MAX_SEQ_LEN for s in used):
        return len(used), 0, 0, ST_TOO_LONG
    if len(used) <= 1:
        return len(used), 0, 0, ST_OK
    pairs = sorted(pair_counts(used, k), key=lambda p: (jaccard(*p), p))
    # Q2's claim: the integer keys order the pairs exactly as the Fractions do
    assert all((key(*a) < key(*b)) == (jaccard(*a) < jaccard(*b)) for a, b in zip(pairs, pairs[1:]))
    inter, uni = pairs[rank(len(pairs), percentile)]
    return len(used), inter, uni, ST_OK


def identify(blk_off, seq_off, bases, kmer_size, min_len, percentile=0.30):
    """The provider's contract on flat arrays: -> (n_used, inter, uni, status, return code)."""
    res = [block([bases[seq_off[s]:seq_off[s + 1]] for s in range(blk_off[b], blk_off[b + 1])], kmer_size, min_len, percentile)
           for b in range(len(blk_off) - 1)]
    cols = [np.asarray([r[c] for r in res], np.int32) for c in range(4)]
    return cols[0], cols[1], cols[2], cols[3], (E_BLOCK if any(r[3] != ST_OK for r in res) else 0)


def identify_blocks(blocks, kmer_size, min_len=None, percentile=0.30):
    """The same on a list of blocks, each a list of code arrays."""
    return [block(b, kmer_size, 8 * kmer_size if min_len is None else min_len, percentile) for b in blocks]


def identity(inter, uni, k):
    """The pair identity of the host estimator as float32: 1 - mash distance, the distance being 1 at J = 0."""
    if not inter or not uni:
        return np.float32(0.0)
    J = inter / uni
    return np.float32(1.0 - (-math.log(2.0 * J / (1.0 + J)) / k))


def threshold(inter, uni, k):
    return max(np.float32(0.7), identity(inter, uni, k))
