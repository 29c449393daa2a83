"""The in-row carries of the packed sweep with ADJACENT strips in a lane (poa_dp16.hip.h, "carries"), restated in numpy for one
wave of 128 strips and checked against the brute-force max-plus prefix.

Lane l holds the wave-local strips u = 2 l (low half) and 2 l + 1 (high half).  a[u] is what strip u hands on: the gap state
after its last column, from gaps that open inside it.  The state entering strip u is the best of every strip to its left,
each extended across the strips in between, and of what came in through the mailbox (strip u = -1):

    E_in[u] = max( max_{u' < u} a[u'] + (u - 1 - u') W e ,  mailbox + u W e ,  floor )

The kernel computes it with ONE inclusive scan over the lanes per gap piece; this guards the algebra, the GPU test
(test_gpu_strip_pairs.py) guards the code."""
import numpy as np
import pytest

FLOORV = 512           # "minus infinity" of the biased local sweep (P16_FLOOR)
NEG = -(1 << 28)       # what an empty mailbox / the lane before lane 0 contributes


def strip_pair_carries(a, in_x, W, x):
    """Step by step what a wave does.  a: [128] outgoing carries by wave-local strip; in_x: the mailbox's value + W x (as y of
    strip u = -1), NEG if there is none; x: the extension penalty of the gap piece (e or c, <= 0).  Returns E_in[128]."""
    lane = np.arange(64)
    Wx = W * x
    tWx = lane * Wx
    a_lo, a_hi = a[0::2], a[1::2]
    y_lo = a_lo - 2 * tWx
    y_hi = a_hi - 2 * tWx - Wx
    S = np.maximum.accumulate(np.maximum(y_lo, y_hi))             # inclusive scan over the lanes
    X = np.maximum(np.concatenate(([NEG], S[:-1])), in_x)         # wave_shr1, joined with the mailbox
    e_lo = np.maximum(X + 2 * tWx - Wx, FLOORV)
    e_hi = np.maximum(np.maximum(X, y_lo) + 2 * tWx, FLOORV)
    out = np.empty(128, np.int64)
    out[0::2], out[1::2] = e_lo, e_hi
    return out


def brute_force(a, mailbox, W, x):
    out = np.empty(128, np.int64)
    for u in range(128):
        best = FLOORV
        if mailbox is not None:
            best = max(best, mailbox + u * W * x)
        for v in range(u):
            best = max(best, a[v] + (u - 1 - v) * W * x)
        out[u] = best
    return out


# (W, extension penalty): both gap pieces of the default convex scores and of a heavier set, at a narrow and the widest strip
@pytest.mark.parametrize("W", [4, 13])
@pytest.mark.parametrize("x", [-2, -1, -3], ids=["e=-2", "c=-1", "e=-3"])
def test_one_scan_over_lane_maxima_equals_the_max_plus_prefix(W, x):
    rng = np.random.default_rng(1000 * W - x)
    cases = []
    for trial in range(40):
        a = rng.integers(FLOORV, 16000, 128).astype(np.int64)
        if trial % 4 == 1:      # a few tall strips among floors: long-range carries, decided by lanes far to the left
            a[:] = FLOORV
            a[rng.integers(0, 128, 3)] = rng.integers(4000, 16000, 3)
        if trial % 4 == 2:      # every strip at the floor
            a[:] = FLOORV
        mailbox = None if trial % 3 == 0 else int(rng.integers(FLOORV, 16000))
        if trial % 8 == 6:      # ... and the mailbox too
            mailbox = FLOORV
        cases.append((a, mailbox))
    # the carrying strip in each position of a lane pair: only the low, only the high strip of lane 0 / 31 / 63
    for u in (0, 1, 62, 63, 126, 127):
        a = np.full(128, FLOORV, np.int64)
        a[u] = 15000
        cases.append((a, None))
    for a, mailbox in cases:
        in_x = NEG if mailbox is None else mailbox + W * x
        got = strip_pair_carries(a, in_x, W, x)
        want = brute_force(a, mailbox, W, x)
        assert (got == want).all(), (W, x, mailbox, np.flatnonzero(got != want)[:5])


def test_what_leaves_the_wave_is_the_last_strips_own_state():
    """The right neighbour's mailbox receives E after the last column of lane 63's HIGH strip -- still the wave's last strip
    (u = 127); taken as strip -1 of the next wave it continues the same prefix."""
    W, x = 11, -2
    rng = np.random.default_rng(7)
    a = rng.integers(FLOORV, 16000, 256).astype(np.int64)
    first = strip_pair_carries(a[:128], NEG, W, x)
    # what the wave hands on: the better of its last strip's own carry and the state that entered it, extended across it
    handed = max(int(a[127]), int(first[127]) + W * x)
    second = strip_pair_carries(a[128:], handed + W * x, W, x)
    whole = np.empty(256, np.int64)
    for u in range(256):
        best = FLOORV
        for v in range(u):
            best = max(best, a[v] + (u - 1 - v) * W * x)
        whole[u] = best
    assert (np.concatenate([first, second]) == whole).all()
