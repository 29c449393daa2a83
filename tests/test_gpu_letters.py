"""GPU: a graph's path letters resident on the device, and the repeat scan and the identity estimate fed with ranges of them
(sxg_poa_letters_*, sxg_poa_range_gather, sxg_poa_repeat_scan_ranges, sxg_poa_block_identity_ranges).  The
gather must write the numpy slices; the ranges calls must give what the `bases` calls give on the same sequences, array for array
and bit for bit; the letters go up once per graph.  There is no tolerance anywhere."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import identity_ref as IR  # noqa: E402
import repeat_ref as RR  # noqa: E402
import test_gpu_repeat as TR  # noqa: E402  (its case table, re-used)
from smoothxg_amd import poa as P  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def own():
    """An engine of this module's own: the residency tests count its uploads from zero."""
    eng = P.PoaEngine(0)
    yield eng
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------------
# the gather
def chunk_bytes():
    import ctypes
    c = ctypes.c_int32()
    P.load_library().sxg_poa_letters_geometry(ctypes.byref(c))
    return int(c.value)


@functools.lru_cache(maxsize=None)
def store():
    """3 paths of chunk + 37, 1 and 5 000 letters over ACGTNacgtn and a few other bytes."""
    chunk = chunk_bytes()
    rng = np.random.default_rng(2031)
    alphabet = np.frombuffer(b"ACGTNacgtn*-R\x00\xff", np.uint8)
    return P.PathLetters([alphabet[rng.integers(0, len(alphabet), n)] for n in (chunk + 37, 1, 5000)]), chunk


@functools.lru_cache(maxsize=None)
def gather_ranges():
    L, chunk = store()
    r = []
    for sa in range(16):                                  # all 16 source alignments x lengths 0..32 (path 2 starts at chunk + 38,
        for n in range(33):                               # and the destination alignment walks through all 16 by itself)
            r.append((2, 100 + sa, 100 + sa + n))
    r += [(0, 5, 5 + chunk - 1), (0, 3, 3), (0, 9, 9 + chunk), (0, 2, 2 + chunk + 1), (2, 7, 7), (2, 11, 4997)]   # chunk - 1, chunk, chunk + 1 between empty ranges
    r += [(0, 0, chunk + 37), (1, 0, 1), (2, 0, 5000)]    # whole paths; the first and the last letter of the store
    r += [(0, 0, 1), (2, 4999, 5000), (1, 0, 0), (1, 1, 1)]
    r += [(2, 40, 90), (2, 40, 90), (2, 60, 120), (2, 50, 61)]   # the same range twice; overlapping ranges
    # (2 chunk + 3 letters do not fit a path of chunk + 37: test_gather_over_several_chunks)
    return np.asarray(r, np.int64)


def slices(L, ranges):
    parts = [L.slice(int(p), int(b), int(e)) for p, b, e in ranges]
    return np.concatenate(parts) if parts else np.zeros(0, np.uint8)


def test_geometry(engine):
    assert engine.letters_geometry() == store()[1]


def test_gather_writes_the_slices(engine):
    L, chunk = store()
    r = gather_ranges()
    assert len(r) >= 540 and L.n_paths == 3
    want = slices(L, r)
    raw = engine.gather_ranges(L, r)
    assert raw.tobytes() == want.tobytes()
    coded = engine.gather_ranges(L, r, coded=True)
    assert coded.tobytes() == P.LETTERS_CODE[want].tobytes()
    assert engine.gather_ranges(L, r).tobytes() == want.tobytes()           # a second call gives the same bytes
    assert engine.gather_ranges(L, r, coded=True).tobytes() == coded.tobytes()
    assert engine.stats()["dp_launches"] == 1 and engine.letters_resident() == (L.id, 3, chunk + 37 + 1 + 5000)


def test_gather_over_several_chunks(engine):
    """2 chunk + 3 letters out of one path, at every source alignment once, between short ranges: a range that spans chunks and
    chunks that hold many ranges."""
    chunk = store()[1]
    rng = np.random.default_rng(5)
    L = P.PathLetters([np.frombuffer(b"ACGTNacgtn", np.uint8)[rng.integers(0, 10, 3 * chunk)]])
    r = []
    for sa in range(16):
        r += [(0, sa, sa + 2 * chunk + 3), (0, 17 * sa, 17 * sa + sa), (0, chunk + sa, chunk + sa + 1)]
    r = np.asarray(r, np.int64)
    want = slices(L, r)
    assert engine.gather_ranges(L, r).tobytes() == want.tobytes()
    assert engine.gather_ranges(L, r, coded=True).tobytes() == P.LETTERS_CODE[want].tobytes()
    assert len(engine.gather_ranges(L, np.zeros((0, 3), np.int64))) == 0 and engine.stats()["dp_launches"] == 0


# ---------------------------------------------------------------------------------------------------------------------------
# the repeat scan
@functools.lru_cache(maxsize=None)
def repeat_store():
    """The sequences of test_gpu_repeat's case table, laid into one store as paths' letters: parameter set after parameter set in
    ONE path each, 1 - 15 filler letters between the sequences so that the ranges start at every alignment."""
    paths, ranges = [], {}
    for p, (key, seqs) in enumerate(TR.batch().items()):
        parts, at, rr = [], 0, []
        for q, s in enumerate(seqs):
            fill = b"acgtn-NACGTacgt"[:1 + (q * 7 + p) % 15]
            parts.append(fill)
            at += len(fill)
            rr.append((p, at, at + len(s)))
            parts.append(s)
            at += len(s)
        paths.append(b"".join(parts))
        ranges[key] = np.asarray(rr, np.int64)
    return P.PathLetters(paths), ranges


def same(a, b):
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:5], b[:5]))
    assert len(a[5]) == len(b[5]) and all(x.tobytes() == y.tobytes() for x, y in zip(a[5], b[5]))


def test_repeat_scan_ranges_equals_the_bases_call(engine):
    L, ranges = repeat_store()
    for key, seqs in TR.batch().items():
        assert [L.slice(*map(int, r)).tobytes() for r in ranges[key]] == list(seqs)
        want = engine.repeat_scan(seqs, *key, want_match=True)
        launches = engine.stats()["dp_launches"]
        got = engine.repeat_scan_ranges(L, ranges[key], *key, want_match=True)
        same(got, want)
        st = engine.stats()
        assert st["dp_launches"] == launches + 1 and st["kernel_ms"] > 0
    assert {len(r) for r in (got[0], want[0])} == {len(seqs)}


def test_repeat_scan_ranges_in_rounds(engine):
    key = TR.REAL + (50,)
    L, ranges = repeat_store()
    seqs, rows = TR.batch()[key], TR.want()[key]
    ns, n_work = len(seqs), sum(r[0] > 0 for r in rows)
    items = sum(-(-r[0] // RR.TILE_LAGS) for r in rows)
    fixed = sum(len(s) for s in seqs) + 16 * (ns + 1) + 8 * items + 4 * n_work + 20 * ns
    most = max(r[0] for r in rows)
    whole = engine.repeat_scan_ranges(L, ranges[key], *key, want_match=True)
    try:
        engine.set_memory_budget(fixed + 4 * (most + 100))
        bases = engine.repeat_scan(seqs, *key, want_match=True)
        rounds = engine.stats()["dp_launches"]
        two = engine.repeat_scan_ranges(L, ranges[key], *key, want_match=True)
        assert engine.stats()["dp_launches"] == rounds + 1 and rounds >= 4     # the rounds of the bases call, and the gather
        engine.set_memory_budget(fixed + 4 * (most - 1))
        with pytest.raises(P.PoaError, match="memory budget too small"):
            engine.repeat_scan_ranges(L, ranges[key], *key)
    finally:
        engine.set_memory_budget(0)
    same(two, bases)
    same(two, whole)


def test_too_long_range_is_declined_alone(engine):
    rng = np.random.default_rng(9)
    a, b = TR.tandem(rng, 600, 40, 0.05), TR.tandem(rng, 333, 25, 0.03)
    filler = (b"ACGTTGCAAC" * ((P.REPEAT_MAX_LEN + 30) // 10 + 1))
    L = P.PathLetters([a + b"nn", filler, b"n" + b])
    r = np.asarray([(0, 0, 600), (1, 3, 3 + P.REPEAT_MAX_LEN + 1), (2, 1, 334)], np.int64)
    lags, best, dev, v, status, match = engine.repeat_scan_ranges(L, r, 8, 64, 3, want_match=True, check=False)
    assert status.tolist() == [0, P.ST_TOO_LONG, 0] and lags.tolist() == [57, 0, 57] and len(match[1]) == 0
    want = engine.repeat_scan([a, b], 8, 64, 3, want_match=True)
    for s, w in ((0, 0), (2, 1)):
        assert match[s].tobytes() == want[5][w].tobytes() == RR.counts((a, b)[w], 8, 64, 3).astype(np.int32).tobytes()
        assert (best[s], dev[s].tobytes(), v[s].tobytes()) == (want[1][w], want[2][w].tobytes(), want[3][w].tobytes())
    assert engine.letters_stats()["gathered_bytes"] > 0
    with pytest.raises(P.PoaError, match="longer than"):
        engine.repeat_scan_ranges(L, r, 8, 64, 3)


# ---------------------------------------------------------------------------------------------------------------------------
# the identity estimate
@functools.lru_cache(maxsize=None)
def identity_case():
    """Blocks of 2 - 12 ranges of 40 - 400 letters over one store: lower case and N, ranges shorter than min_len, a block with one
    taking-part range, an empty block, overlapping ranges."""
    rng = np.random.default_rng(77)
    up = np.frombuffer(b"ACGT", np.uint8)
    anc = up[rng.integers(0, 4, 400)]

    def mutant(n_mut, lower=False, n_run=0):
        s = anc.copy()
        at = rng.integers(0, 400, n_mut)
        s[at] = up[rng.integers(0, 4, n_mut)]
        if lower:
            s[50:200] = np.frombuffer(bytes(s[50:200]).lower(), np.uint8)
        if n_run:
            s[220:220 + n_run] = ord("N")
        return s
    paths = [mutant(0), mutant(8, lower=True), mutant(20, n_run=9), mutant(40), mutant(3, lower=True, n_run=3), up[rng.integers(0, 4, 400)]]
    L = P.PathLetters(paths)
    full = lambda p, b=0, e=400: (p, b, e)
    blocks = [
        [full(0), full(1)],
        [full(0, 3, 390), full(1, 0, 397), full(2, 5, 400), full(3, 1, 299), full(4, 7, 307), full(5, 9, 209)],
        [full(p, (p * 5) % 16, 400 - p) for p in range(6)] + [full(p, 100 + p, 300 + 3 * p) for p in range(6)],   # 12 ranges
        [full(0, 0, 40), full(1, 10, 60), full(2, 0, 400)],                   # one taking-part range
        [],                                                                    # an empty block
        [full(0, 0, 250), full(0, 100, 350), full(0, 150, 400), full(1, 120, 380)],   # overlapping ranges of one path
        [full(0, 10, 50), full(3, 0, 39)],                                    # none takes part
        [full(2, 200, 400), full(4, 200, 400), full(5, 200, 400)],
    ]
    return L, blocks


@pytest.mark.parametrize("k", (4, 17))
def test_block_identity_ranges_equals_the_bases_call_and_the_restatement(engine, k):
    L, blocks = identity_case()
    min_len = 100
    coded = [[P.LETTERS_CODE[L.slice(*r)] for r in blk] for blk in blocks]
    want = engine.block_identity(coded, k, min_len)
    launches = engine.stats()["dp_launches"]
    got = engine.block_identity_ranges(L, blocks, k, min_len)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want))
    assert engine.stats()["dp_launches"] == launches + 1
    ref = IR.identify_blocks(coded, k, min_len)
    used, inter, uni, status = got
    assert [(int(u), int(s)) for u, s in zip(used, status)] == [(r[0], r[3]) for r in ref]
    assert used.tolist() == [2, 6, 12, 1, 0, 4, 0, 3]
    for b, r in enumerate(ref):
        assert int(inter[b]) * r[2] == r[1] * int(uni[b]) and (int(uni[b]) == 0) == (r[2] == 0), (b, int(inter[b]), int(uni[b]), r)


def test_block_with_a_too_long_range_fails_alone(engine):
    L, blocks = identity_case()
    rng = np.random.default_rng(3)
    long_path = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, IR.MAX_SEQ_LEN + 40)]
    L2 = P.PathLetters([L.slice(p, 0, 400) for p in range(6)] + [long_path])
    blks = [blocks[1], [(6, 20, 20 + IR.MAX_SEQ_LEN + 1), (0, 0, 400)], blocks[7]]
    used, inter, uni, status = engine.block_identity_ranges(L2, blks, 17, 100, check=False)
    assert status.tolist() == [0, P.ST_TOO_LONG, 0] and (int(inter[1]), int(uni[1])) == (0, 0) and used.tolist() == [6, 2, 3]
    want = engine.block_identity_ranges(L, [blocks[1], blocks[7]], 17, 100)
    assert [int(inter[0]), int(uni[0]), int(inter[2]), int(uni[2])] == [int(want[1][0]), int(want[2][0]), int(want[1][1]), int(want[2][1])]
    with pytest.raises(P.PoaError, match="longer than"):
        engine.block_identity_ranges(L2, blks, 17, 100)


# ---------------------------------------------------------------------------------------------------------------------------
# residency
def test_one_upload_per_graph(own):
    L, ranges = repeat_store()
    Li, blocks = identity_case()
    key = TR.SMALL + (3,)
    one = P.PathLetters(path_off=L.path_off, letters=L.letters)                  # "a graph": the same letters under an id of its own
    assert own.letters_resident() == (0, 0, 0) and own.letters_stats()["uploads"] == 0
    a = own.repeat_scan_ranges(one, ranges[key], *key, want_match=True)
    own.block_identity_ranges(one, [[(0, 0, 300), (0, 20, 320)]], 4, 100)
    b = own.repeat_scan_ranges(one, ranges[key], *key, want_match=True)
    same(a, b)
    st = own.letters_stats()
    assert (st["uploads"], st["bytes_uploaded"]) == (1, len(one.letters)) and st["gather_ms"] > 0 and st["gathered_bytes"] > 0
    assert own.letters_resident() == (one.id, one.n_paths, len(one.letters))
    # a second graph replaces the first: one more upload
    own.block_identity_ranges(Li, blocks, 17, 100)
    st = own.letters_stats()
    assert (st["uploads"], st["bytes_uploaded"]) == (2, len(one.letters) + len(Li.letters)) and own.letters_resident()[0] == Li.id
    # by id alone: resident letters need no pointer; other ids do
    own.block_identity_ranges(None, blocks, 17, 100, letters_id=Li.id)
    with pytest.raises(P.PoaError, match="not resident"):
        own.repeat_scan_ranges(None, ranges[key], *key, letters_id=one.id)
    with pytest.raises(P.PoaError, match="not resident"):
        own.gather_ranges(None, [(0, 0, 1)], letters_id=one.id)
    assert own.letters_stats()["uploads"] == 2
    # a range beyond its path: refused, nothing launched
    for bad in ((0, 0, 401), (6, 0, 1), (0, -1, 5), (0, 9, 8), (-1, 0, 0)):
        with pytest.raises(P.PoaError, match="range 1 "):
            own.block_identity_ranges(Li, [[(0, 0, 400), bad]], 17, 100)
        assert own.stats()["dp_launches"] == 0
        with pytest.raises(P.PoaError, match="range 0 "):
            own.repeat_scan_ranges(Li, [bad], 8, 64, 3)
        assert own.stats()["dp_launches"] == 0
    # dropped letters go up again with the next call that passes them
    own.drop_letters()
    assert own.letters_resident() == (0, 0, 0)
    with pytest.raises(P.PoaError, match="not resident"):
        own.block_identity_ranges(None, blocks, 17, 100, letters_id=Li.id)
    own.block_identity_ranges(Li, blocks, 17, 100)
    assert own.letters_stats()["uploads"] == 3 and own.letters_resident()[0] == Li.id
    own.upload_letters(one)
    assert own.letters_stats()["uploads"] == 4 and own.letters_resident()[0] == one.id


def test_a_poa_batch_leaves_the_letters_resident(own):
    Li, blocks = identity_case()
    rng = np.random.default_rng(12)
    anc = rng.integers(0, 4, 300).astype(np.uint8)
    seqs = [anc.copy() for _ in range(5)]
    for s in seqs[1:]:
        s[rng.integers(0, 300, 6)] = rng.integers(0, 4, 6)
    params = P.params_from_cli()
    before = own.run_blocks([seqs], params, want_consensus=True)
    want = own.block_identity_ranges(Li, blocks, 17, 100)
    uploads = own.letters_stats()["uploads"]
    between = own.run_blocks([seqs], params, want_consensus=True)
    assert own.letters_resident()[0] == Li.id
    got = own.block_identity_ranges(None, blocks, 17, 100, letters_id=Li.id)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want)) and own.letters_stats()["uploads"] == uploads
    assert before[0].status == between[0].status == 0 and before[0].consensus.tobytes() == between[0].consensus.tobytes()
    assert np.asarray(before[0].scores).tobytes() == np.asarray(between[0].scores).tobytes()


# ---------------------------------------------------------------------------------------------------------------------------
# end to end, through the host library
def test_discovery_with_the_range_scanner_gives_the_blocks_of_the_bases_scanner_and_the_host(own):
    from smoothxg_amd import smooth as S
    uploads = own.letters_stats()["uploads"]
    for name, text, conf in TR.DISCOVER:
        text = text()
        host, _ = TR.blocks_of(text, conf)
        bases, bases_counts = TR.blocks_of(text, dict(conf, scanner=S.gpu_repeat_scanner(own)))
        got, counts = TR.blocks_of(text, dict(conf, scanner=S.gpu_range_scanner(own)))
        assert got == bases == host and counts == bases_counts and counts[0] >= 1 and counts[2] == 0, name
        assert own.stats()["dp_launches"] == 3                              # ONE provider call: the gather and one round
        uploads += 1
        assert own.letters_stats()["uploads"] == uploads                    # one upload per graph


def test_adaptive_iteration_with_the_range_identifier_is_byte_equal(own):
    from smoothxg_amd import smooth as S
    from test_identity_host import smooth_gfa_with
    from test_smooth_host import DRB1, haplotype_gfa
    for text, target, k in ((haplotype_gfa(400, sub=0.004), 450, 15), (open(DRB1).read(), 700, 17)):
        sm = S.Smoother(text, target)
        p = S.default_params(adaptive_poa_params=1, kmer_size=k)
        want = smooth_gfa_with(sm, p, S.gpu_provider(own), S.gpu_identifier(own))
        uploads = own.letters_stats()["uploads"]
        thr = sm.identity_thresholds(k, S.gpu_range_identifier(own))        # the first provider call of this graph pays the upload
        host = sm.identity_thresholds(k)
        assert thr[0].tobytes() == host[0].tobytes() and thr[1].tolist() == host[1].tolist()
        assert smooth_gfa_with(sm, p, S.gpu_provider(own), S.gpu_range_identifier(own)) == want
        assert own.letters_stats()["uploads"] == uploads + 1 and own.letters_resident()[0] == sm.path_letters().id
        maf = sm.smooth_maf_gfa(p, S.gpu_provider(own), identity=S.gpu_identifier(own), device_rows=True)
        assert sm.smooth_maf_gfa(p, S.gpu_provider(own), identity=S.gpu_range_identifier(own), device_rows=True) == maf
        assert own.letters_stats()["uploads"] == uploads + 1
        sm.close()


def test_range_providers_through_a_group_member(engine):
    from smoothxg_amd import smooth as S
    from test_identity_host import smooth_gfa_with
    from test_smooth_host import haplotype_gfa
    group = P.PoaGroup([0, 0])
    try:
        member = group.member(1)
        name, text, conf = TR.DISCOVER[0]
        text = text()
        assert TR.blocks_of(text, dict(conf, scanner=S.gpu_range_scanner(member)))[0] == TR.blocks_of(text, conf)[0]
        sm = S.Smoother(haplotype_gfa(400, sub=0.004), 450)
        p = S.default_params(adaptive_poa_params=1, kmer_size=15)
        want = smooth_gfa_with(sm, p, S.gpu_provider(engine), S.gpu_identifier(engine))
        assert smooth_gfa_with(sm, p, S.gpu_provider(engine), S.gpu_range_identifier(member)) == want
        assert member.letters_stats()["uploads"] == 2 and group.member(0).letters_stats()["uploads"] == 0   # every handle its own copy
        sm.close()
    finally:
        group.close()
