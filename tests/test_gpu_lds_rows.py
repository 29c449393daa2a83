"""The packed sweep keeps a stored row in one of SXG_POA_LDS_ROWS on-chip copies when its last reader comes soon enough, and
sends every other one through the row ring in HBM.  The full-shape fixture blocks must come out the same -- and equal to the
committed oracle output -- whether no stored row (0), one copy's worth (1) or two copies' worth (2, the four-wave 2-byte
classes' default) stay on chip: the ring and the on-chip copies hold the same row code."""
import json
import os
import sys

import pytest

from smoothxg_amd import Params, synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _digests(r):
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from make_fullshape import digest_block
    return digest_block(r.node_code, r.node_rank, r.node_group, r.edge_tail, r.edge_head, r.edge_weight, r.paths,
                        r.consensus)


@pytest.mark.parametrize("lds_rows", ["0", "1", "2"])
@pytest.mark.parametrize("name", ["ns_sw", "ns_nw", "c2"])
def test_full_shape_blocks_agree_for_every_on_chip_row_count(engine, monkeypatch, name, lds_rows):
    monkeypatch.setenv("SXG_POA_LDS_ROWS", lds_rows)
    with open(os.path.join(HERE, "golden", "fullshape_oracle.json")) as f:
        cases = [c for c in json.load(f)["cases"] if c["name"] == name and c.get("order", "s7") == "spoa"]
    assert cases
    blocks = [synth.make_block(c["block_id"], c["n_seqs"], c["length"]) for c in cases]
    res = engine.run_blocks(blocks, Params(*cases[0]["params"], cases[0]["mode"] | 0x10, 0), want_consensus=True)
    for c, r in zip(cases, res):
        label = "%s block %d, SXG_POA_LDS_ROWS=%s" % (name, c["block_id"], lds_rows)
        assert r.status == 0, label
        assert r.scores.tolist() == c["scores"], label
        assert int(r.cells.sum()) == c["cells"], label
        got = _digests(r)
        for k, v in c["digests"].items():
            assert got[k] == v, label + ": " + k
