"""tests/golden/class_matrix*.json without a GPU: (a) the classes its cases run on are the built ones (tests/csrc/class_list.cpp
prints smoothxg_amd/csrc/poa_classes.h's list) -- the exclusion list is empty and stays so: a class added later fails here until
a case runs it; (b) every case's inputs regenerate; (c) every case of up to 2 100 letters, and every banded case of up to 2 300
(the W = 6 cases: a banded oracle run is cheap), is re-run through the scalar oracle, align cases through the numpy graph
builder as well.  The model of the host's choice that maps a case to its class (tests/golden/make_class_matrix.py) is held
equal to the recorded choice of tests/golden/geometry_choice.json, its strip width of the banded sweep to the oracle's
poa_band_strip_width at every length."""
import json
import os
import shutil
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_class_matrix as M  # noqa: E402

# Built classes no case runs: (kind, rm, cb, tmax, W, sw, ds) -> reason.  None: every built class has a case, the banded ones
# (kind "band", class_matrix_banded.json) included.  (The int32-row-word classes run for the wide_match family, whose m = 64
# reaches them from 469 letters on without a knob.  The 16-wave global classes beyond the packed score range need no entry: the
# block classes run as the 768-thread launch of the (12,8) blocks, the align-only class on the longest global query the strict
# rule admits.)
EXCLUDED = {}
# the nine class lines of the banded sweep; each is two kernels, convex and affine
BAND_LINES = [(0, 3, 2, 64, w, 1, 0) for w in (6, 8, 11)] + [(0, 3, 4, 64, w, sw, 0) for w in (6, 8, 11) for sw in (0, 1)]


@pytest.fixture(scope="module")
def fixture_cases():
    return M.load_cases()


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("classes") / "class_list")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "csrc", "class_list.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = [tuple(map(int, line.split())) for line in out.stdout.splitlines()]
    assert len(set(lines)) == len(lines)
    return set(lines)


def covered_classes(cases):
    """The classes the GPU test's runs select: every case's own (the wide_match family's among them: the int32-row-word classes,
    block and align-only), the 4-byte affine classes of gen2_affine's packed block cases
    under SXG_POA_CELL_BYTES=4, the 768-thread launch (SXG_POA_FORCE_P16=8,12) of the (12,8) blocks, and the forced re-runs of
    the longest packed global align query (M.ALIGN_GLOBAL_FORCED), and the 4-byte classes of the banded sweep's local 2-byte
    cases under SXG_POA_BAND_CELL_BYTES=4."""
    got = {}
    for c in cases:
        got.setdefault(M.case_class(c), M.case_id(c))
        if c["kind"] == "band" and M.case_class(c)[2] == 2:
            got.setdefault(M.case_class(c, knob4=True), M.case_id(c) + "+bcb4")
        if c["kind"] == "block" and c["rm"] == 2 and c["family"] == "gen2_affine":
            got.setdefault(M.case_class(c, knob4=True), M.case_id(c) + "+cb4")
        if c["kind"] == "block" and c["rm"] == 2 and (c["W"], c["NW"]) == (12, 8) and c["family"] in M.FORCED_768_FAMILIES:
            got.setdefault(M.case_class(c, force=(8, 12)), M.case_id(c) + "+force8,12")
        if c["kind"] == "align" and "top" in c and (c["W"], c["NW"]) == (8, 8):
            for f in M.ALIGN_GLOBAL_FORCED:
                got.setdefault(M.case_class(c, force=f), M.case_id(c) + "+force%d,%d" % f)
    return got


def covered_band_kernels(cases):
    """(class line, convex) of the banded sweep -> the case or knob re-run that selects that KERNEL: a line of poa_classes.h is
    two kernels, and only the gap model of the scores tells them apart"""
    got = {}
    for c in cases:
        if c["kind"] != "band":
            continue
        cvx = int(M.normalise(tuple(c["params"]))[6])
        got.setdefault((M.case_class(c), cvx), M.case_id(c))
        if M.case_class(c)[2] == 2:
            got.setdefault((M.case_class(c, knob4=True), cvx), M.case_id(c) + "+bcb4")
    return got


def missing_and_stale(built_set, cases):
    got = set(covered_classes(cases))
    return sorted(built_set - got - set(EXCLUDED)), sorted(set(EXCLUDED) & got), sorted(got - built_set), sorted(set(EXCLUDED) - built_set)


def test_cases_cover_every_built_class(built, fixture_cases):
    missing, stale, unbuilt, unknown = missing_and_stale(built, fixture_cases)
    assert not unbuilt, "cases whose class is not built: %s" % unbuilt
    assert not unknown, "exclusions that name no built class: %s" % unknown
    assert not stale, "excluded classes that a case does run: %s" % stale
    assert not missing, "built classes (kind rm cb tmax W sw ds) without a case and without a reason: %s" % missing
    assert EXCLUDED == {}, "no built class goes without a case"
    assert len(built) >= 250                                        # (each line stands for two kernels: convex and affine)
    # the banded sweep: its nine lines are built, and each of their 18 kernels is selected by a case or a knob re-run
    assert set(BAND_LINES) == {k for k in built if k[1] == 3}
    kernels = covered_band_kernels(fixture_cases)
    assert sorted(kernels) == sorted((line, cvx) for line in BAND_LINES for cvx in (0, 1)), sorted(kernels)
    no_band = [c for c in fixture_cases if c["kind"] != "band"]
    assert missing_and_stale(built, no_band)[0] == sorted(BAND_LINES)
    # the check bites: without a family's cases its classes are reported (the 4-byte classes run for cb4_convex and, under the
    # knob, for gen2_affine; the align-only classes for both align families)
    for kind, fams, expect in (("block", ("ds",), (0, 2, 2, 256, 10, 0, 1)), ("block", ("cb4_convex", "gen2_affine"), (0, 2, 4, 512, 11, 1, 0)),
                               ("block", ("cb4_convex",), (0, 2, 4, 1024, 8, 0, 0)), ("align", M.ALIGN_FAMILIES, (1, 0, 4, 256, 16, 1, 0)),
                               ("block", ("wide_match",), (0, 1, 4, 256, 8, 0, 0)), ("align", ("wide_match",), (1, 1, 4, 512, 12, 1, 0)),
                               # the banded sweep: a 2-byte local line (its two families), a 4-byte local line (cb4_convex and the
                               # knob re-runs of the 2-byte cases), a global line (every family that runs it)
                               ("band", ("gen2_convex", "gen2_affine"), (0, 3, 2, 64, 8, 1, 0)),
                               ("band", ("gen2_convex", "gen2_affine", "cb4_convex"), (0, 3, 4, 64, 6, 1, 0)),
                               ("band", ("ds", "affine_e1"), (0, 3, 4, 64, 11, 0, 0))):
        some = [c for c in fixture_cases if not (c["family"] in fams and c["kind"] == kind)]
        assert expect in missing_and_stale(built, some)[0], (kind, fams)
    # ... and kernel by kernel: without gen2_affine's local cases the affine 4-byte local kernels have no run (the knob re-runs
    # of gen2_convex are convex), without ds the convex global ones
    for fams, mode, line, cvx in ((("gen2_affine",), 0, (0, 3, 4, 64, 11, 1, 0), 0), (("ds",), 1, (0, 3, 4, 64, 6, 0, 0), 1)):
        some = [c for c in fixture_cases if not (c["kind"] == "band" and c["family"] in fams and c["mode"] == mode)]
        assert (line, cvx) not in covered_band_kernels(some) and (line, 1 - cvx) in covered_band_kernels(some), (fams, line)


def test_the_model_of_the_strip_width_equals_the_oracles(tmp_path):
    """M.band_strip_width against poa_band_strip_width (oracle/poa_oracle.h, compiled here from the header) for every length the
    banded sweep accepts; the lengths the banded cases stand on are the places where it changes"""
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc")
    assert cc, "no host C compiler"
    exe = str(tmp_path / "band_width_list")
    subprocess.check_call([cc, "-O2", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "csrc", "band_width_list.c")])
    out = subprocess.run([exe, str(M.MAX_SEQ_LEN)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    want = [int(x) for x in out.stdout.split()]
    got = [M.band_strip_width(L) for L in range(1, M.MAX_SEQ_LEN + 1)]
    assert len(want) == M.MAX_SEQ_LEN and got == want, [L + 1 for L in range(M.MAX_SEQ_LEN) if got[L] != want[L]][:10]
    changes = [(L, got[L - 1]) for L in range(2, M.MAX_SEQ_LEN + 1) if got[L - 1] != got[L - 2]]
    assert changes == [(2267, 8), (6467, 11)] and got[0] == 6
    assert M.BAND_LENGTHS[6][1] == 2266 and M.BAND_LENGTHS[8][1] == 6466
    # the capped half-width: 693 from 12 734 letters on, 692 before
    assert M.band_half_width(M.BAND_LENGTHS[11][0]) == 693 and M.band_half_width(M.BAND_LENGTHS[11][0] - 1) == 692


def test_the_model_of_the_choice_equals_the_recorded_one():
    with open(os.path.join(HERE, "golden", "geometry_choice.json")) as f:
        golden = json.load(f)
    compared = 0
    for mode in golden["modes"]:
        if mode["kind"] != "block" or not mode["full_plane"] or mode["spread"]:
            continue
        rows = mode["rows"]
        for i, (first, w, nw, tmax) in enumerate(rows):
            last = (rows[i + 1][0] if i + 1 < len(rows) else golden["max_len"] + 1) - 1
            for maxlen in {first, (first + last) // 2, last}:
                v = M.variant_for_len(maxlen, mode["rm"], bool(mode["sw"]))
                assert (v or (-1, -1)) == (w, nw), (mode["rm"], mode["sw"], maxlen)
                if v:
                    assert M.class_tmax(nw, mode["rm"], mode["cb"] if mode["rm"] == 2 else 4) == tmax, (mode, maxlen)
                compared += 1
    assert compared > 300


def test_every_case_regenerates_and_selects_its_geometry(fixture_cases):
    listed = {M.case_id(c): c for c in M.list_cases()}
    assert sorted(listed) == sorted(M.case_id(c) for c in fixture_cases)
    for c in fixture_cases:
        want = listed[M.case_id(c)]
        assert all(c[k] == want[k] for k in want if k != "seed"), M.case_id(c)
        seqs = M.case_inputs(c)
        assert [len(s) for s in seqs] == c["seq_lens"], M.case_id(c)
        W, NW, rm, sw = c["W"], c["NW"], c["rm"], c["mode"] == 0
        top = len(seqs[2]) if c["kind"] == "align" else max(c["seq_lens"])
        if c["kind"] == "band":
            check_band_case(c, top)
            continue
        cap = M.capacity(W, NW, rm)
        if c["kind"] == "block":
            assert cap - 3 <= top <= cap - 1, M.case_id(c)
            assert M.row_mode(tuple(c["params"]), sw, top, top, no_packed=c.get("no_packed", rm != 2), clamp_ok=True) == rm, M.case_id(c)
        elif c["kind"] == "align":
            assert top > cap * (NW - 1) // NW + 64 and top <= c.get("top", cap - 1), M.case_id(c)
            assert M.row_mode(tuple(c["params"]), sw, top, c["rows"], no_packed=c["no_packed"]) == rm, M.case_id(c)
        assert M.variant_for_len(top, rm, sw, force=(W, NW) if c["force"] else None) == (W, NW), M.case_id(c)
        assert c["force"] == (M.variant_for_len(top, rm, sw) != (W, NW)), M.case_id(c)
        # the splices straddle a wave boundary (one wave: a strip boundary)
        for at in (c["del_at"], c["ins_at"]):
            assert at % W == 0 and (NW == 1 or at % (cap // NW) == 0) and 0 < at < cap, M.case_id(c)
    for ti, prm in enumerate(M.TIERS):
        assert M.cell_bytes(prm) == M.TIER_CELL_BYTES[ti]
        tiers = [c for c in fixture_cases if c["kind"] == "tier" and tuple(c["params"]) == prm]
        assert sorted((c["W"], c["NW"]) for c in tiers) == [(10, 4), (11, 4)]


def check_band_case(c, top):
    """A banded case: the sweep and the strip width the model names for its longest sequence, the length conditions of its
    strip width, the splices, and -- on the oracle's recorded row counts -- no refused sweep."""
    cid, W, scores, sw = M.case_id(c), c["W"], tuple(c["params"]), c["mode"] == 0
    w = M.band_half_width(top)
    assert (c["rm"], c["NW"], c["force"]) == (3, 1, False) and c["banded"] in ((1, 2) if sw else (2,)), cid
    assert M.block_sweep(scores, c["mode"], top, c["banded"]) == (3, W, 1, 2 if sw and M.code_bits(scores) <= 16 else 4, 64, 0), cid
    assert c["top"] - c["lo"] <= top <= c["top"], cid
    lo_len, hi_len = M.BAND_LENGTHS[W]
    full = lo_len <= top <= hi_len
    if sw or W == 6 or (W == 8 and c["family"] == "ds"):
        # the band fills the window: 2 w = 126 strips, so a band in the middle of the sequence spans 127 or 128 of the 128
        assert full and 2 * w == 126 * W, cid
        assert M.band_strip_width(hi_len) == W and (W == 11 or M.band_strip_width(hi_len + 1) != W), cid
        assert W != 11 or M.band_half_width(lo_len - 1) < 693 == w, cid
    else:
        # a global case the strict range rule ends early: on W, as long as the model admits with BAND_ROWS_MARGIN rows per letter
        assert not full and c["top"] == M.band_global_top(scores, W) and M.band_strip_width(top) == W, cid
        assert not M.band_no_rerun(scores, 1, [c["top"] + 1] * 2, [0, int((c["top"] + 1) * M.BAND_ROWS_MARGIN) + 1]) or abs(scores[0]) * (c["top"] + 1) >= 15800, cid
    # no re-run: the host's rule on the longest sequence, the kernel's on the oracle's row count in front of every sequence
    assert len(c["rows_before"]) == 3 and c["rows_before"][:2] == [0, c["seq_lens"][0]] and c["rows_before"][2] >= c["rows_before"][1], cid
    assert M.row_mode(scores, sw, top, top) == 2 and M.band_no_rerun(scores, c["mode"], c["seq_lens"], c["rows_before"]), cid
    assert sw or c["rows_before"][2] <= int(top * M.BAND_ROWS_MARGIN), cid
    # the splices sit on strip boundaries where a static band is whole (neither clipped at column 0 nor at the last strip), and
    # the deletion's 40 columns are more than three strips: with at most one strip of slack in the window, the row behind the
    # deletion reads its stored predecessor from before at least one re-centre of the window
    assert (c["del_at"], c["ins_at"]) == M.band_splices(W, c["top"]) and c["del_at"] % W == 0 and c["ins_at"] % W == 0, cid
    assert c["del_at"] - M.SPLICE // 2 - w > 0 and c["ins_at"] + M.SPLICE + w < min(c["seq_lens"]), cid
    assert M.SPLICE // W >= 3 and 2 * w // W + 2 >= (127 if full else 0), cid


def test_small_cases_reproduce_with_the_scalar_oracle(fixture_cases, oracle):
    small = [c for c in fixture_cases if max(c["seq_lens"]) <= (2300 if c["kind"] == "band" else 2100)]
    assert len(small) >= 100 and {c["kind"] for c in small} == {"block", "align", "band"}
    assert sum(c["kind"] == "band" for c in small) == 8 and all(c["W"] == 6 for c in small if c["kind"] == "band")
    for c in small:
        got = M.expectations(c, impl=oracle.IMPL_SCALAR)
        assert all(c[k] == v for k, v in got.items()), M.case_id(c)
