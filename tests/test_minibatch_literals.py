"""Multimodal mini-batches on the host: `MiniBatch(A, X, ...)` with token, WKT (CSR), numeric and boolean encoding sets,
then `pad_` / `to_dense_` / `as_tensors_`, against the reference's output (tests/golden/make_minibatch_literal_goldens.py):
every array bit for bit, dtypes included.  The golden pins the reference's quirks: a set without a member among the
batch's outermost neighbours becomes `[np.empty(0)] * 3`, the encodings keep the set's member order while the node-id
column is the sorted intersection, a -1 token turns into the pad symbol."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import util

GOLD = os.path.join(util.GOLDEN, "minibatch_literals.npz")
NAMES = ("wkt", "boolean", "numeric", "string")


def features(g):
    """The golden's feature list (object arrays rebuilt from their flat form)."""
    offs, tok = g["in.string.offsets"], g["in.string.tokens"]
    toks = np.empty(len(offs) - 1, dtype=object)
    for i in range(len(toks)):
        toks[i] = tok[offs[i]:offs[i + 1]].copy()
    nnz, C = g["in.wkt.nnz"], int(g["c_wkt"])
    starts = np.concatenate([[0], np.cumsum(nnz)])
    mats = np.empty(len(nnz), dtype=object)
    for i in range(len(nnz)):
        sl = slice(starts[i], starts[i + 1])
        mats[i] = sp.csr_matrix((g["in.wkt.data"][sl], g["in.wkt.indices"][sl], g["in.wkt.indptr"][i]),
                                shape=(C, int(g["in.wkt.widths"][i])))
    return [g["in.X0"].copy(),
            ["ogc.wktLiteral", [[mats, g["in.wkt.node_idx"].copy(), g["in.wkt.seq_lengths"].copy()]], False],
            ["xsd.boolean", [[g["in.boolean.enc"].copy(), g["in.boolean.node_idx"].copy(),
                              g["in.boolean.seq_lengths"].copy()]], False],
            ["xsd.numeric", [[g["in.numeric.enc"].copy(), g["in.numeric.node_idx"].copy(),
                              g["in.numeric.seq_lengths"].copy()]], False],
            ["xsd.string", [[toks, g["in.string.node_idx"].copy(), g["in.string.seq_lengths"].copy()]], False]]


def assert_same(got, want, what):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    if what.endswith(".node_idx") and want.dtype == np.int32:
        # the node-id column is np.intersect1d(set's ids, neighbour ids): the reference's neighbour lists are int32
        # (batch.py:233-249 keeps A.indices' dtype), this package's are int64 (the fixed-width sets' column has
        # always been int64 here), so the column is int64 where the reference's is int32 — the same ids
        assert got.dtype == np.int64, (what, got.dtype)
        got = got.astype(np.int32)
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    np.testing.assert_array_equal(got, want, err_msg=what)


def check_batch(X, g, b):
    assert_same(X[0], g[f"b{b}.X0"], f"b{b}.X0")
    assert [m[0] for m in X[1:]] == ["ogc.wktLiteral", "xsd.boolean", "xsd.numeric", "xsd.string"]
    for name, (_, sets, _) in zip(NAMES, X[1:]):
        assert len(sets) == 1 and len(sets[0]) == 3
        for part, arr in zip(("enc", "node_idx", "seq_lengths"), sets[0]):
            assert_same(arr, g[f"b{b}.{name}.{part}"], f"b{b}.{name}.{part}")


@pytest.mark.parametrize("b", [0, 1, 2])
def test_host_minibatch_literals_match_reference(b):
    from mrgcn_amd.data.batch import MiniBatch
    g = np.load(GOLD)
    _, A = util.load_graph("graph_small")
    mb = MiniBatch(A, features(g), g[f"b{b}.idx"], int(g["num_layers"]))
    np.testing.assert_array_equal(np.asarray(mb.A.neighbours[-1]), g[f"b{b}.outer"])
    mb.pad_(pad_symbols={"xsd.string": int(g["pad_symbol"])})
    mb.to_dense_()
    mb.as_tensors_()
    check_batch(mb.X, g, b)


def test_golden_pins_the_reference_quirks():
    """What the fixture must cover: the boolean set is absent from batch 0 (placeholder), the token set's node ids are
    not ascending and its members come out in member order (not node order), the WKT members are shorter and longer
    than 5, a -1 token became the pad symbol."""
    g = np.load(GOLD)
    assert g["b0.boolean.enc"].dtype == np.float64 and g["b0.boolean.enc"].shape == (0,)
    s_nodes = g["in.string.node_idx"]
    assert np.any(np.diff(s_nodes) < 0)
    for b in range(3):
        sel = np.isin(s_nodes, g[f"b{b}.outer"])
        assert np.array_equal(g[f"b{b}.string.node_idx"], np.sort(s_nodes[sel]))
        assert np.array_equal(g[f"b{b}.string.seq_lengths"], g["in.string.seq_lengths"][sel])   # member order
    w = g["in.wkt.widths"]
    assert w.min() < 5 < w.max()
    assert -1 in g["in.string.tokens"] and -1 not in g["b1.string.enc"]


def test_pad_width_follows_the_host_rule():
    """The padded width is max(max(seq_length), min(longest member, 999)); a member longer than it raises."""
    from mrgcn_amd.data.batch import pad_token_sequences
    seqs = np.empty(2, dtype=object)
    seqs[0], seqs[1] = np.arange(3), np.array([4, -1])
    out = pad_token_sequences(seqs, pad_symbol=7, min_width=2)
    assert out.shape == (2, 3) and out.tolist() == [[0, 1, 2], [4, 7, 7]]
    seqs[0] = np.arange(1200)
    assert pad_token_sequences(seqs, 0, 1200).shape == (2, 1200)
    with pytest.raises(ValueError):
        pad_token_sequences(seqs, 0, 5)


def test_csr_member_beyond_the_padded_width_raises():
    """A CSR member with entries beyond the padded width: an error (the reference re-declares the member unchecked and
    its densification writes out of bounds)."""
    from mrgcn_amd.data.batch import pad_sparse_members
    mats = np.empty(2, dtype=object)
    mats[0] = sp.csr_matrix(np.ones((2, 4), dtype=np.float32))
    mats[1] = sp.csr_matrix(np.ones((2, 1200), dtype=np.float32))
    with pytest.raises(ValueError):
        pad_sparse_members(mats, 1, 5)
    mats[1] = sp.csr_matrix((np.ones(1, np.float32), np.array([3]), np.array([0, 1, 1])), shape=(2, 1200))
    out = pad_sparse_members(mats, 1, 5)               # wider than 999 but its entries fit: re-declared to 999
    assert out[1].shape == (2, 999) and out[1].toarray()[0, 3] == 1.0


def test_masked_batch_subset_on_the_host_uses_the_same_mksubset():
    """`mksubset` (the host path of MiniBatch(A) and MiniBatch(plan=...)) on the golden's outermost neighbours."""
    from mrgcn_amd.data.batch import Batch, mksubset
    g = np.load(GOLD)
    for b in range(3):
        batch = Batch()
        batch.X = mksubset(features(g), g[f"b{b}.outer"])
        batch.node_index = g[f"b{b}.idx"]
        batch.pad_(pad_symbols={"xsd.string": int(g["pad_symbol"])})
        batch.to_dense_()
        batch.as_tensors_()
        check_batch(batch.X, g, b)


def test_mrgcn_init_stream_matches_the_golden_model():
    """The golden's MRGCN (TCNN + MLPs + Transformer head on the stand-in backbone) is rebuilt from the same seed: same
    state-dict keys and per-tensor checksums (what the GPU test's logits and gradients rest on)."""
    from tests.test_gpu_minibatch_literals import build_model
    g = np.load(GOLD)
    model = build_model(g, torch.device("cpu"))
    sd = {k: v.cpu() for k, v in model.state_dict().items()}
    keys = sorted(sd)
    assert keys == list(g["mrgcn.sd.keys"])
    np.testing.assert_allclose([float(sd[k].double().sum()) for k in keys], g["mrgcn.sd.sum"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose([float(sd[k].double().abs().sum()) for k in keys], g["mrgcn.sd.abs"], rtol=1e-9)
