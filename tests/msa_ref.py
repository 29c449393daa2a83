"""The trimmed MSA (want_msa = SXG_MSA_TRIMMED of include/sxg_poa.h) restated on top of oracle_py's full MSA, for the tests:
every row -- the consensus row included -- loses its first and last `trim` letters (a row with fewer than 2 * trim letters
loses all), then the columns in front of the first column that still holds a letter in any row go, and those behind the
last one; interior columns stay.  Written over letter POSITIONS (numpy), not as the column-by-column walk of
oracle/smooth_oracle.py::maf_rows, which test_msa_cols.py pins it to."""
import numpy as np

from oracle import oracle_py as O


def trim_rows(rows, trim):
    """rows: the full MSA, equally long strings over ACGTN and '-'.  -> the trimmed rows (all "" when nothing remains)."""
    if not rows:
        return []
    width = len(rows[0])
    assert all(len(r) == width for r in rows)
    a = np.frombuffer("".join(rows).encode(), np.uint8).reshape(len(rows), width).copy() if width else np.zeros((len(rows), 0), np.uint8)
    lo, hi = width, 0
    for r in a:
        at = np.flatnonzero(r != ord("-"))
        keep = at[trim:len(at) - trim] if len(at) >= 2 * trim else at[:0]
        gone = np.setdiff1d(at, keep)
        r[gone] = ord("-")
        if len(keep):
            lo, hi = min(lo, int(keep[0])), max(hi, int(keep[-1]) + 1)
    if hi <= lo:
        return [""] * len(rows)
    return [bytes(r[lo:hi]).decode() for r in a]


def block_rows(seqs, weights, params, want_consensus, trim):
    """The trimmed rows of one block: seqs as uint8 code arrays, params an oracle parameter struct (O.mkparams)."""
    g, _, _ = O.block_run([np.asarray(s, np.uint8) for s in seqs], weights, params)
    return trim_rows(g.msa(bool(want_consensus)), int(trim))
