"""CPU: the host half of prep (sxg_graph_prep: flatten, the schedule Y2, apply the order, chop by decree C) against its
restatement in tests/prep_ref.py, with a Python callback running the reference sort as the sort provider; the invariants of
a prepped GFA; and the point of the feature: block discovery on the prepped DRB1 graph finds blocks of the size the POA
kernels were built for."""
import functools
import hashlib
import json
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import prep_ref as R  # noqa: E402
from oracle import smooth_oracle as SO  # noqa: E402
from smoothxg_amd import smooth as S  # noqa: E402

DRB1 = os.path.join(HERE, "golden", "DRB1-3123.seqwish.gfa")
GOLD = os.path.join(HERE, "golden", "prep_drb1.json")


@functools.lru_cache(maxsize=None)
def drb1_text():
    return open(DRB1).read()


@functools.lru_cache(maxsize=None)
def drb1_prepped():
    """(prepped GFA from the C++ library with the reference sort as provider, what the provider was handed)."""
    seen = {}

    def sorter(node_len, path_off, step_node, step_pos, eta, cooling_start, terms, seed):
        seen.update(eta=eta, cooling_start=cooling_start, terms=terms, seed=seed, path_off=path_off)
        seen["order"] = R.sgd_order(node_len, path_off, step_node, step_pos, eta, cooling_start, terms, seed)[0]
        return seen["order"]
    return S.prep_gfa(drb1_text(), S.python_sorter(sorter)), seen


def rank_jumps(order, path_off, step_node):
    """(mean rank jump per path step, steps that jump more than 100 ranks) with the nodes in `order`."""
    rank = np.empty(len(order), np.int64)
    rank[np.asarray(order, np.int64)] = np.arange(len(order))
    j = np.concatenate([np.abs(np.diff(rank[step_node[path_off[p]:path_off[p + 1]]])) for p in range(len(path_off) - 1)])
    return float(j.mean()), int((j > 100).sum())


def check_invariants(out_text, in_text, max_node_length):
    seqs, paths, edges = R.parse_gfa(out_text)
    seqs0, paths0, _ = R.parse_gfa(in_text)
    assert R.path_sequences(seqs, paths) == R.path_sequences(seqs0, paths0)          # every path spells its sequence
    assert [nm for nm, _ in paths] == [nm for nm, _ in paths0]
    assert max(len(s) for s in seqs) <= max_node_length
    ids = [int(l.split("\t")[1]) for l in out_text.split("\n") if l.startswith("S\t")]
    assert ids == list(range(1, len(ids) + 1))
    have = set(edges)
    for _, st in paths:
        for (a, ar), (b, br) in zip(st, st[1:]):                                     # the L line or its other form
            assert (a, ar, b, br) in have or (b, not br, a, not ar) in have
    llines = [tuple(l.split("\t")[1:5]) for l in out_text.split("\n") if l.startswith("L\t")]
    keys = [(int(a), ao == "-", int(b), bo == "-") for a, ao, b, bo in llines]
    assert keys == sorted(set(keys))                                                 # sorted, no duplicates


def test_drb1_equals_the_restatement_and_the_schedule_is_y2():
    got, seen = drb1_prepped()
    assert got == R.prep_gfa(drb1_text(), lambda *a: seen["order"])
    eta, cs, terms = seen["eta"], seen["cooling_start"], seen["terms"]
    assert len(eta) == 100 and cs == 50 and terms == 25802 and seen["seed"] == R.DEFAULT_SEED
    maxsteps = int(np.diff(seen["path_off"]).max())
    lam = math.log(maxsteps * maxsteps / 0.01) / 99
    for t in range(100):
        assert math.isclose(eta[t], maxsteps * maxsteps * math.exp(-lam * t), rel_tol=1e-12)
    check_invariants(got, drb1_text(), 100)


def test_synthetic_graph_with_reverse_steps_equals_the_restatement():
    text = R.synthetic_gfa(3)
    seqs, paths, _ = R.parse_gfa(text)
    assert {1, 100, 101, 250} <= {len(s) for s in seqs} and any(rv for _, st in paths for _, rv in st)
    for kw in (dict(), dict(max_node_length=50), dict(max_node_length=1), dict(iter_max=7, term_updates=2.5, cooling=0.25, seed=11)):
        ref_kw = dict(kw)
        got = S.prep_gfa(text, S.python_sorter(R.sgd_order), **kw)
        assert got == R.prep_gfa(text, None, **ref_kw), kw
        check_invariants(got, text, kw.get("max_node_length", 100))


def test_identity_order_without_chopping_gives_back_the_input_graph():
    text = R.synthetic_gfa(4)
    seqs, paths, edges = R.parse_gfa(text)
    got = S.prep_gfa(text, S.python_sorter(lambda node_len, *a: np.arange(len(node_len))), max_node_length=max(len(s) for s in seqs))
    seqs2, paths2, edges2 = R.parse_gfa(got)
    assert seqs2 == seqs and paths2 == paths and sorted(set(edges2)) == sorted(set(edges))
    assert got == R.to_gfa(seqs, paths, edges)


def test_a_bad_provider_and_bad_parameters_are_errors():
    text = R.synthetic_gfa(5, n_nodes=12, n_paths=2)
    with pytest.raises(S.SmoothError):
        S.prep_gfa(text, S.python_sorter(lambda node_len, *a: np.zeros(len(node_len), np.int32)))      # not a permutation
    with pytest.raises(S.SmoothError):
        S.prep_gfa(text, S.python_sorter(lambda *a: 1 / 0))                                              # the provider fails
    with pytest.raises(S.SmoothError):
        S.prep_gfa(text, S.python_sorter(R.sgd_order), eps=0.0)
    with pytest.raises(S.SmoothError):
        S.prep_gfa(text, S.python_sorter(R.sgd_order), term_updates=1e30)                                # 2^63 terms or more
    with pytest.raises(TypeError):
        S.prep_gfa(text, S.python_sorter(R.sgd_order), no_such_knob=1)


def test_graph_without_paths_or_nodes():
    assert S.prep_gfa("H\tVN:Z:1.0\n", S.python_sorter(R.sgd_order)) == "H\tVN:Z:1.0\n"
    text = "S\t7\tACGT\nS\t3\t" + "A" * 150 + "\nL\t7\t+\t3\t-\t0M\n"
    assert S.prep_gfa(text, S.python_sorter(R.sgd_order)) == R.prep_gfa(text) == \
        "H\tVN:Z:1.0\nS\t1\t" + "A" * 100 + "\nS\t2\t" + "A" * 50 + "\nS\t3\tACGT\nL\t1\t+\t2\t+\t0M\nL\t3\t+\t2\t-\t0M\n"


def test_block_discovery_on_prepped_drb1_finds_a_tenth_of_the_blocks():
    """The point of prep.  Unprepped, the reference's ctest flags (-l 700 -j 5k -e 5k -r 12) give 2 161 blocks of about 75 bp
    of path each on DRB1; after the sort and the chop at most a tenth of that.  The count obtained and the digest of the
    prepped GFA are pinned in tests/golden/prep_drb1.json (the GPU test compares the device's result with the same digest)."""
    got, _ = drb1_prepped()
    g = SO.Graph(got)
    blocks = SO.break_blocks(g, SO.smoothable_blocks(g, 700 * 12, 700, 5000, 5000), 1400)
    print("blocks", len(blocks), "ranges", sum(len(b) for b in blocks))
    assert len(blocks) <= 216
    gold = json.load(open(GOLD))
    assert len(blocks) == gold["blocks"] and sum(len(b) for b in blocks) == gold["ranges"]
    assert hashlib.sha256(got.encode()).hexdigest() == gold["prepped_gfa_sha256"]


def test_the_sort_shortens_the_rank_jumps_of_drb1():
    """What README and DESIGN quote: the mean rank jump per path step and the steps that jump more than 100 ranks, in the
    input's node order and in the sorted one (before the chop), pinned in tests/golden/prep_drb1.json."""
    _, seen = drb1_prepped()
    seqs, paths, _ = R.parse_gfa(drb1_text())
    _, path_off, step_node, _ = R.flatten(seqs, paths)
    before, after = rank_jumps(np.arange(len(seqs)), path_off, step_node), rank_jumps(seen["order"], path_off, step_node)
    print("rank jumps before", before, "after", after)
    gold = json.load(open(GOLD))
    assert [round(before[0], 3), before[1]] == gold["rank_jump_input"] and [round(after[0], 3), after[1]] == gold["rank_jump_sorted"]
    assert after[0] < before[0] / 10


def test_host_steps_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """flatten, apply and chop of the C++ library (smoothxg_amd/csrc/prep_host.h, what sxg_graph_prep runs) in a stand-alone
    program (tests/csrc/prep_check.cpp) built with -fsanitize=address,undefined and run as a child process, on the synthetic
    graph with a shuffled order.  The sanitizer runtimes are linked statically and the child inherits the environment as it is."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "prep_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-w",
                           "-o", exe, os.path.join(HERE, "csrc", "prep_check.cpp")])
    text = R.synthetic_gfa(6)
    seqs, _, _ = R.parse_gfa(text)
    order = np.random.default_rng(6).permutation(len(seqs))
    (tmp_path / "in.gfa").write_text(text)
    (tmp_path / "order.txt").write_text(" ".join(str(v) for v in order))
    for maxlen in (100, 1, 1000):
        res = subprocess.run([exe, str(tmp_path / "in.gfa"), str(tmp_path / "order.txt"), str(maxlen)], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-2000:]
        assert res.stdout == R.prep_gfa(text, lambda *a: order, max_node_length=maxlen)
