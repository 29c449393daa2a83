"""tests/golden/class_matrix.json without a GPU: (a) the classes its cases run on are the built ones (tests/csrc/class_list.cpp
prints smoothxg_amd/csrc/poa_classes.h's list) minus an explicit exclusion list -- a class added later fails here until a case
runs it; (b) every case's inputs regenerate; (c) every case of up to 2 100 letters is re-run through the scalar oracle, align
cases through the numpy graph builder as well.  The model of the host's choice that maps a case to its class
(tests/golden/make_class_matrix.py) is held equal to the recorded choice of tests/golden/geometry_choice.json."""
import json
import os
import shutil
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_class_matrix as M  # noqa: E402

# Built classes no case runs: (kind, rm, cb, tmax, W, sw, ds) -> reason.  Banded classes only: every class of the full-matrix
# sweeps has a case.  (The int32-row-word classes run for the wide_match family, whose m = 64 reaches them from 469 letters on
# without a knob.  The 16-wave global classes beyond the packed score range need no entry: the block classes run as the
# 768-thread launch of the (12,8) blocks, the align-only class on the longest global query the strict rule admits.)
BANDED = "banded sweep: the subject of test_gpu_banded.py / test_gpu_adaptive_band.py"
EXCLUDED = {}
for w in (6, 8, 11):
    EXCLUDED[(0, 3, 2, 64, w, 1, 0)] = BANDED
    for sw in (0, 1):
        EXCLUDED[(0, 3, 4, 64, w, sw, 0)] = BANDED


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
    the longest packed global align query (M.ALIGN_GLOBAL_FORCED)."""
    got = {}
    for c in cases:
        got.setdefault(M.case_class(c), M.case_id(c))
        if c["kind"] == "block" and c["rm"] == 2 and c["family"] == "gen2_affine":
            got.setdefault(M.case_class(c, knob4=True), M.case_id(c) + "+cb4")
        if c["kind"] == "block" and c["rm"] == 2 and (c["W"], c["NW"]) == (12, 8) and c["family"] in M.FORCED_768_FAMILIES:
            got.setdefault(M.case_class(c, force=(8, 12)), M.case_id(c) + "+force8,12")
        if c["kind"] == "align" and "top" in c and (c["W"], c["NW"]) == (8, 8):
            for f in M.ALIGN_GLOBAL_FORCED:
                got.setdefault(M.case_class(c, force=f), M.case_id(c) + "+force%d,%d" % f)
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
    assert all(k[1] == 3 for k in EXCLUDED), "only banded classes may go without a case"
    assert len(built) >= 250 and len(EXCLUDED) < len(built) // 5   # (each line stands for two kernels: convex and affine)
    # the check bites: without a family's cases its classes are reported (the 4-byte classes run for cb4_convex and, under the
    # knob, for gen2_affine; the align-only classes for both align families)
    for kind, fams, expect in (("block", ("ds",), (0, 2, 2, 256, 10, 0, 1)), ("block", ("cb4_convex", "gen2_affine"), (0, 2, 4, 512, 11, 1, 0)),
                               ("block", ("cb4_convex",), (0, 2, 4, 1024, 8, 0, 0)), ("align", M.ALIGN_FAMILIES, (1, 0, 4, 256, 16, 1, 0)),
                               ("block", ("wide_match",), (0, 1, 4, 256, 8, 0, 0)), ("align", ("wide_match",), (1, 1, 4, 512, 12, 1, 0))):
        some = [c for c in fixture_cases if not (c["family"] in fams and c["kind"] == kind)]
        assert expect in missing_and_stale(built, some)[0], (kind, fams)


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


def test_small_cases_reproduce_with_the_scalar_oracle(fixture_cases, oracle):
    small = [c for c in fixture_cases if max(c["seq_lens"]) <= 2100]
    assert len(small) >= 100 and {c["kind"] for c in small} == {"block", "align"}
    for c in small:
        got = M.expectations(c, impl=oracle.IMPL_SCALAR)
        assert all(c[k] == v for k, v in got.items()), M.case_id(c)
