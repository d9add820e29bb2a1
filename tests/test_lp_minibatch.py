"""mkbatches (link_prediction.py:477-530) against the reference's own output, bit for bit (CPU)."""
import os

import numpy as np
import pytest

from tests import util

GOLD = os.path.join(os.path.dirname(__file__), "golden", "lp_minibatch.npz")
CONFIGS = {"full": (0, 40), "nb8": (8, 1000), "nb8_m10": (8, 10), "nb16_m7": (16, 7)}


@pytest.mark.parametrize("tag", list(CONFIGS))
def test_mkbatches_matches_reference(tag):
    from mrgcn_amd.data.batch import FullBatch, MiniBatch
    from mrgcn_amd.tasks import link_prediction as lp
    g = np.load(GOLD)
    _, A = util.load_graph("graph_small")
    gb, mb = CONFIGS[tag]
    batches = lp.mkbatches(A, None, g["facts"], gb, mb, 1)
    assert len(batches) == int(g[f"{tag}.count"])
    for i, (batch, facts) in enumerate(batches):
        assert isinstance(batch, FullBatch if gb <= 0 else MiniBatch)
        nodes = np.asarray(batch.node_index)
        assert nodes.dtype == g[f"{tag}.{i}.nodes"].dtype and np.array_equal(nodes, g[f"{tag}.{i}.nodes"]), i
        assert facts.dtype == g[f"{tag}.{i}.facts"].dtype and np.array_equal(facts, g[f"{tag}.{i}.facts"]), i


def test_mkbatches_structure():
    """Node batches: every fact with a batch node lands in that batch (a fact can sit in two), the remapped facts
    index the batch's node set, and the slice path's A_Batch holds the batch nodes' rows."""
    from mrgcn_amd.tasks import link_prediction as lp
    g = np.load(GOLD)
    _, A = util.load_graph("graph_small")
    facts = g["facts"]
    batches = lp.mkbatches(A, None, facts, 8, 1000, 1)
    seen = np.zeros(len(facts), dtype=np.int64)
    keys = {tuple(f): i for i, f in enumerate(facts)}
    for batch, bf in batches:
        nodes = np.asarray(batch.node_index)
        assert bf[:, [0, 2]].max() < len(nodes)
        glob = np.stack([nodes[bf[:, 0]], bf[:, 1], nodes[bf[:, 2]]], 1)
        for f in glob:
            seen[keys[tuple(f)]] += 1
        assert batch.A.row[0].shape == (len(nodes), A.shape[1])
    assert seen.min() >= 1 and seen.max() <= 2
