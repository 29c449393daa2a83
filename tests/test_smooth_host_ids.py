"""CPU: sxg_smooth_params.poa_spoa_order = 2 reaches the engine as mode | SXG_ORDER_SPOA | SXG_IDS_SPOA (decrees S7' + S6'),
1 as mode | SXG_ORDER_SPOA, and -A drops both -- seen by a callback provider that records the params it is handed and serves
flagged blocks from the plain-Python reference (tests/spoa_ids_ref.py; the oracle cannot produce the mode)."""
import numpy as np

import spoa_ids_ref as R
from helpers import heaviest_bundle_independent
from oracle import oracle_py as O
from oracle import smooth_oracle as SO
from smoothxg_amd import poa as P
from smoothxg_amd import smooth as S
from test_smooth_host import OracleProvider, synthetic_gfa


class _RefGraph:
    """What OracleProvider._run reads of an oracle graph, from a reference result."""

    def __init__(self, r):
        self.r = r

    def nodes(self):
        return self.r.node_code, self.r.node_rank, self.r.node_group

    def seq_path(self, k):
        return self.r.paths[k]

    def consensus(self):
        r = self.r
        return heaviest_bundle_independent(r.node_code, r.node_rank, r.edge_tail, r.edge_head, r.edge_weight)


class RecordingProvider(OracleProvider):
    def __init__(self):
        super().__init__()
        self.modes = []

    def _run(self, ctx, pin, pout):
        i = pin.contents
        self.modes += [int(i.params[b if i.per_block_params else 0].mode) for b in range(i.n_blocks)]
        orig = O.block_run

        def block_run(seqs, w, par):
            if par.mode & P.IDS_SPOA:
                return _RefGraph(R.run_block(seqs, w, par, ids="spoa")), None, None
            return orig(seqs, w, par)

        O.block_run = block_run
        try:
            return super()._run(ctx, pin, pout)
        finally:
            O.block_run = orig


def one_iteration(**kw):
    text = synthetic_gfa(5, n_paths=6, n_nodes=80)
    prov = RecordingProvider()
    sm = S.Smoother(text, 250)
    got = sm.smooth_gfa(S.default_params(add_consensus=1, **kw), prov.provider())
    sm.close()
    assert prov.modes
    return text, got, prov.modes


def test_spoa_order_2_hands_the_engine_both_flags():
    assert P.IDS_SPOA == 0x20 and P.ORDER_SPOA == 0x10
    text, got, modes = one_iteration(poa_spoa_order=2)
    assert set(modes) == {0x30}                      # local mode (the default) | SXG_ORDER_SPOA | SXG_IDS_SPOA
    g, out = SO.Graph(text), SO.Graph(got)
    for q, nm in enumerate(g.pname):                 # (tests/gfa_invariants.py has run on `got` as well: conftest.py)
        assert out.path_sequence(out.pname.index(nm)) == g.path_sequence(q)
    # the other values behave as before: 1 = the order alone (and the default), 0 = neither
    text1, got1, modes1 = one_iteration(poa_spoa_order=1)
    assert set(modes1) == {0x10}
    assert one_iteration()[1:] == (got1, modes1)
    assert set(one_iteration(poa_spoa_order=0)[2]) == {0}
    # global mode keeps the flag (the engine treats it as S6 there)
    assert set(one_iteration(poa_spoa_order=2, local_alignment=0)[2]) == {0x31}
    # same sequences and the same graph up to node names: as many bases either way
    assert sum(len(s) for s in out.seq) == sum(len(s) for s in SO.Graph(got1).seq)


def test_abpoa_path_drops_both_flags():
    for order in (1, 2):
        modes = one_iteration(poa_spoa_order=order, use_abpoa=1)[2]
        assert all(m & 0x30 == 0 for m in modes), modes
