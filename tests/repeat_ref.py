"""Decree R restated in Python for the tests of the tandem-repeat scan: the match counts with numpy (exact integers), the
statistics pass and the host's decision with Python floats (IEEE double, one rounding per operation, sums in lag order).  What
the oracle decides (oracle.smooth_oracle.repeat_length) is checked against this by the tests that use it."""
import math
import struct

import numpy as np

ST_OK, ST_TOO_LONG, E_BLOCK = 0, 5, -4
MAX_LEN = 1 << 20
TILE_LAGS = 256   # SXG_REPEAT_TILE_LAGS: the lags of one work item of the counting kernel


def n_lags(n, min_copy, max_copy):
    return 0 if n < 2 * min_copy else min(max_copy, n - min_copy) - min_copy + 1


def counts(seq, min_copy, max_copy, stride):
    """R2: match(L) for L = min_copy ... as int32; seq: bytes or a uint8 array."""
    s = np.frombuffer(seq, np.uint8) if isinstance(seq, (bytes, bytearray)) else np.asarray(seq, np.uint8)
    n = len(s)
    return np.array([int((s[0:n - L:stride] == s[L:n:stride]).sum()) for L in range(min_copy, min_copy + n_lags(n, min_copy, max_copy))], np.int32)


def stats(match, n, min_copy, stride):
    """R3: (best, dev, v) of a sequence of n letters with the counts `match` (at least one)."""
    r = [int(m) / float(-(-(n - (min_copy + k)) // stride)) for k, m in enumerate(match)]
    mean = 0.0
    for x in r:
        mean += x
    mean /= float(len(r))
    var = 0.0
    for x in r:
        var += (x - mean) * (x - mean)
    best = max(range(len(r)), key=lambda k: (r[k], -k))   # the first k of the greatest r
    return best, r[best] - mean, var / float(len(r))


def decide(min_copy, best, dev, v, min_z):
    """The host's three operations: the repeat's length, 0.0 when there is none."""
    sd = math.sqrt(v)
    if sd == 0.0:
        return 0.0
    return float(min_copy + best) if dev / sd >= min_z else 0.0


def scan(seq_off, bases, min_copy, max_copy, stride):
    """sxg_poa_repeat_scan_batch's contract on a flat batch: (n_lags, best, dev, v, status, return code)."""
    ns = len(seq_off) - 1
    lags, best, status = np.zeros(ns, np.int32), np.zeros(ns, np.int32), np.zeros(ns, np.int32)
    dev, v = np.zeros(ns, np.float64), np.zeros(ns, np.float64)
    rc = 0
    for s in range(ns):
        seq = bases[seq_off[s]:seq_off[s + 1]]
        if len(seq) < 2 * min_copy:
            continue
        if len(seq) > MAX_LEN:
            status[s], rc = ST_TOO_LONG, E_BLOCK
            continue
        m = counts(seq, min_copy, max_copy, stride)
        lags[s] = len(m)
        best[s], dev[s], v[s] = stats(m, len(seq), min_copy, stride)
    return lags, best, dev, v, status, rc


def bits(x):
    return struct.pack("<d", float(x))
