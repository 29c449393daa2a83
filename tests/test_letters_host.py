"""CPU: the range providers of the host library (sxg_graph_path_letters, sxg_blockset_break_scan_ranges,
sxg_blockset_identity_thresholds_ranges, sxg_smooth_iteration_ranges of include/sxg_smooth.h).  The graph's path letters are the
spelled sequences of its paths; with python_range_scanner around tests/repeat_ref.py and python_range_identifier around
tests/identity_ref.py -- fed RANGES of those letters instead of sequences -- the blocks, the counts, the thresholds and the
smoothed graph are those of the `bases` providers and of the host, bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import identity_ref as IR  # noqa: E402
from oracle import smooth_oracle as SO  # noqa: E402
from smoothxg_amd import smooth as S  # noqa: E402
from test_identity_host import RefIdentifier, smooth_gfa_with  # noqa: E402
from test_identity_ref import A4, B4, POLY_A, POLY_C  # noqa: E402  (4-mer sets that share 1 of 129 k-mers: a pair identity below 0)
from test_repeat_host import CASES, RefScanner, break_ex, break_scan, ranges_of, shared_chain_gfa  # noqa: E402
from test_smooth_host import DRB1, OracleProvider, haplotype_gfa, synthetic_gfa  # noqa: E402


class RangeScanner(RefScanner):
    """RefScanner behind python_range_scanner: the same function, fed the sequences the ranges spell."""

    def __init__(self, decline=None, spoil=None):
        RefScanner.__init__(self, decline, spoil)
        self.provider = S.python_range_scanner(self._run)


class RangeIdentifier(RefIdentifier):
    def __init__(self, too_long=None):
        RefIdentifier.__init__(self, too_long)
        self.provider = S.python_range_identifier(self._run)


# ---------------------------------------------------------------------------------------------------------------------------
# the letters
@pytest.mark.parametrize("text", [lambda: synthetic_gfa(4, n_paths=6, n_nodes=80), lambda: mixed_case_gfa(), lambda: open(DRB1).read()],
                         ids=["synthetic-with-reverse-steps", "mixed-case", "drb1"])
def test_path_letters_are_the_spelled_sequences(text):
    text = text()
    g = SO.Graph(text)
    sm = S.Smoother(text, 200)
    L = sm.path_letters()
    assert L.n_paths == len(g.pname) and L.id != 0
    for p in range(L.n_paths):
        assert L.slice(p, 0, int(L.path_off[p + 1] - L.path_off[p])).tobytes().decode() == g.path_sequence(p), p
    again = sm.path_letters()
    assert again.id == L.id and again.letters.tobytes() == L.letters.tobytes()      # cached: the same letters under the same id
    other = S.Smoother(text, 200)
    assert other.path_letters().id != L.id                                            # another graph object, another id
    sm.close()
    other.close()


def test_synthetic_graph_has_reverse_steps():
    g = SO.Graph(synthetic_gfa(4, n_paths=6, n_nodes=80))
    assert any(h & 1 for steps in g.steps for h in steps)


# ---------------------------------------------------------------------------------------------------------------------------
# the repeat scan
def break_scan_ranges(sm, max_poa, rep, provider):
    out = C.c_void_p()
    counts = [C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)]
    rc = sm.L.sxg_blockset_break_scan_ranges(sm.g, sm.b, max_poa, rep[0], rep[1], rep[2], rep[3], 1, provider[0], provider[1], C.byref(out),
                                             *(C.byref(c) for c in counts))
    if rc:
        raise S.SmoothError(sm.L.sxg_smooth_last_error().decode())
    return ranges_of(sm, out), tuple(c.value for c in counts)


@pytest.fixture(scope="module", params=CASES, ids=[c[0] for c in CASES])
def case(request):
    name, text, blocks_of, max_poa, rep = request.param
    text = text()
    sm = S.Smoother(text, blocks=blocks_of(SO.Graph(text)))
    yield sm, max_poa, rep
    sm.close()


def test_break_scan_ranges_gives_the_blocks_and_counts_of_the_bases_provider_and_the_host(case):
    sm, max_poa, rep = case
    bases = RefScanner()
    want, counts = break_scan(sm, max_poa, rep, bases.provider)
    ref = RangeScanner()
    got, got_counts = break_scan_ranges(sm, max_poa, rep, ref.provider)
    assert got == want == break_ex(sm, max_poa, rep) and got_counts == counts and counts[2] == 0 and counts[0] >= 1
    assert ref.calls == 1 and ref.seen == bases.seen                       # one call, the same sequences' count and parameters


def test_a_declined_range_is_scanned_on_the_host(case):
    sm, max_poa, rep = case
    want, counts = break_scan(sm, max_poa, rep, RefScanner(decline=0).provider)
    ref = RangeScanner(decline=0)
    got, got_counts = break_scan_ranges(sm, max_poa, rep, ref.provider)
    assert got == want == break_ex(sm, max_poa, rep) and got_counts == counts and counts[2] == 1 and ref.calls == 1


def test_a_range_scanner_that_answers_out_of_range_is_refused(case):
    sm, max_poa, rep = case

    def wrong_lags(lags, best, rc):
        lags[0] += 1
        return rc

    def failing(lags, best, rc):
        return -3

    for spoil, msg in ((wrong_lags, "out of range"), (failing, "repeat scan provider failed")):
        with pytest.raises(S.SmoothError, match=msg):
            break_scan_ranges(sm, max_poa, rep, RangeScanner(spoil=spoil).provider)


def test_discovery_takes_a_range_scanner():
    text = shared_chain_gfa(5)
    conf = dict(target_poa_length=4000, n_haps=3, max_poa_length=2000)
    a = S.Smoother(text, discover=conf)
    ref = RangeScanner()
    b = S.Smoother(text, discover=dict(conf, scanner=ref.provider))
    assert [b.block_ranges(k) for k in range(b.n_blocks)] == [a.block_ranges(k) for k in range(a.n_blocks)]
    assert ref.calls == 1 and b.break_counts == (2, 2, 0)
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------------------
# the identity estimate
def mixed_case_gfa():
    """Five near-identical haplotypes and two unrelated paths, every path on its own chain of nodes; stretches in lower case, a run
    of N, and a path that walks another's nodes backwards."""
    rng = np.random.default_rng(41)
    anc = rng.integers(0, 4, 900)
    lines, plines, nid, chains = ["H\tVN:Z:1.0"], [], 1, []
    for p in range(7):
        hap = anc.copy() if p < 5 else rng.integers(0, 4, 900)
        mut = rng.random(900) < 0.01 * (p + 1)
        hap[mut] = (hap[mut] + rng.integers(1, 4, int(mut.sum()))) % 4
        text = "".join("ACGT"[c] for c in hap)
        if p in (1, 3):
            text = text[:200] + text[200:520].lower() + text[520:]
        if p in (2, 3):
            text = text[:640] + "N" * 7 + text[647:]
        steps = []
        for a in range(0, 900, 60):
            lines.append("S\t%d\t%s" % (nid, text[a:a + 60]))
            steps.append(nid)
            nid += 1
        chains.append(steps)
        plines.append("P\tp%d\t%s\t*" % (p, ",".join("%d+" % s for s in steps)))
    plines.append("P\tback\t%s\t*" % ",".join("%d-" % s for s in reversed(chains[0])))
    for name, text in (("neg_a", A4), ("neg_b", B4), ("poly_a", POLY_A), ("poly_c", POLY_C)):   # paths 8 - 11, one node each
        lines.append("S\t%d\t%s" % (nid, text))
        plines.append("P\t%s\t%d+\t*" % (name, nid))
        nid += 1
    return "\n".join(lines + plines) + "\n"


def identity_blocks():
    whole = lambda p: (p, 0, 15)
    return [[whole(p) for p in range(7)],                         # related and unrelated pairs: identities from ~1 down to 0
            [whole(0), whole(7), whole(1)],                        # a path and its reverse complement
            [whole(2)],                                            # one range: not sent
            [whole(0), whole(1), whole(2), whole(3), whole(4), whole(5), whole(6), whole(7)],   # more ranges than max_depth: not sent
            [(0, 0, 1), (1, 0, 15), (2, 3, 4)],                    # one range of at least min_len
            [(5, 0, 15), (6, 0, 15)],                              # unrelated: J = 0
            [(1, 2, 14), (3, 1, 15), (1, 0, 9), (3, 4, 15)],       # lower case and N, overlapping ranges
            [(8, 0, 1), (9, 0, 1)],                                # k = 4: J = 1 / 129, a pair identity below 0
            [(8, 0, 1), (9, 0, 1), (10, 0, 1), (11, 0, 1)]]        # k = 4: negative and zero pair identities in one block


@pytest.mark.parametrize("k", (4, 7, 15))
def test_thresholds_with_the_range_identifier_are_the_host_estimators(k):
    sm = S.Smoother(mixed_case_gfa(), blocks=identity_blocks())
    host_thr, host_used = sm.identity_thresholds(k, None, max_depth=7)
    bases = RefIdentifier()
    b_thr, b_used = sm.identity_thresholds(k, bases.provider, max_depth=7)
    ref = RangeIdentifier()
    thr, used = sm.identity_thresholds(k, ref.provider, max_depth=7)
    assert thr.dtype == np.float32 and thr.tobytes() == host_thr.tobytes() == b_thr.tobytes()
    assert used.tolist() == host_used.tolist() == b_used.tolist()
    assert ref.calls == 1 and ref.seen == bases.seen == [(7, k, 8 * k, 0.30)]
    assert used[2] == 0 and used[3] == 0 and used[0] == 7 and used[4] == (1 if k == 15 else 3)
    if k == 4:    # pairs whose estimate is negative or zero end at the floor
        assert used[7] == 2 and used[8] == 4 and thr[7] == thr[8] == np.float32(0.7)
        assert IR.identity(1, 129, 4) < 0
    if k == 15:   # unrelated paths share no 15-mer: J = 0
        assert used[5] == 2 and thr[5] == np.float32(0.7)
    sm.close()


def test_thresholds_on_drb1():
    sm = S.Smoother(open(DRB1).read(), 700)
    host_thr, host_used = sm.identity_thresholds(17)
    ref = RangeIdentifier()
    thr, used = sm.identity_thresholds(17, ref.provider)
    assert thr.tobytes() == host_thr.tobytes() and used.tolist() == host_used.tolist() and ref.calls == 1 and (used > 1).sum() >= 2
    failing = RangeIdentifier(too_long=3)                                    # a block the provider fails gets the host value
    thr, used = sm.identity_thresholds(17, failing.provider)
    assert host_used[3] > 1 and thr.tobytes() == host_thr.tobytes() and used.tolist() == host_used.tolist()
    sm.close()


def test_a_range_identifier_with_wrong_counts_is_refused():
    sm = S.Smoother(open(DRB1).read(), 700)

    def bad_used(*a):
        used, inter, uni, status, rc = IR.identify(*a)
        used[0] += 1
        return used, inter, uni, status, rc

    def bad_counts(*a):
        used, inter, uni, status, rc = IR.identify(*a)
        inter[0] = uni[0] + 1
        return used, inter, uni, status, rc

    def failing(*a):
        return IR.identify(*a)[:4] + (-3,)

    for fn, msg in ((bad_used, "out of range"), (bad_counts, "out of range"), (failing, "identity provider failed")):
        with pytest.raises(S.SmoothError, match=msg):
            sm.identity_thresholds(17, S.python_range_identifier(fn))
    sm.close()


def test_adaptive_iterations_with_the_range_identifier_are_byte_equal():
    prov = OracleProvider()
    text = haplotype_gfa(400, sub=0.004)
    sm = S.Smoother(text, 450)
    p = S.default_params(adaptive_poa_params=1, kmer_size=15)
    ref = RangeIdentifier()
    without = sm.smooth_gfa(p, prov.provider())
    assert smooth_gfa_with(sm, p, prov.provider(), ref.provider) == without and ref.calls == 1
    maf = sm.smooth_maf_gfa(p, prov.provider())
    assert sm.smooth_maf_gfa(p, prov.provider(), identity=ref.provider) == maf and ref.calls == 2
    sm.close()
