#!/usr/bin/env python
"""Golden vectors for multimodal mini-batches (variable-length literals), AUTHORING CONTAINER ONLY: imports the
reference and drives, on the 50-node golden graph with two layers,
  mrgcn/data/batch.py:150-164, :272-316   MiniBatch(A, X, batch_idx, num_layers) / mksubset on object arrays
  mrgcn/data/batch.py:25-54, :56-68       pad_(pad_symbols=...) / to_dense_
  mrgcn/data/utils.py:109-152             collate_zero_padding_sparse / collate_padding
  mrgcn/models/mrgcn.py:216-305           MRGCN._forward_mini_batch with a TCNN (wkt), an MLP (numeric), a
                                          Transformer head (string, tiny stand-in backbone) and gates
The feature list holds a token set whose node ids are not ascending (with a -1 token), a WKT CSR set whose members
are shorter and longer than 5, a numeric set and a boolean set that is absent from batch 0.  Object arrays are
stored flat (tokens + offsets, concatenated CSR arrays) so that the fixture loads without pickle.
    python tests/golden/make_minibatch_literal_goldens.py"""
import os
import sys

import numpy as np
import scipy.sparse as sp
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as mg  # noqa: E402
from make_encoder_goldens import TinyLM, checksums  # noqa: E402

PAD = 1          # pad symbol of xsd.string
C_WKT = 6        # rows (features) of a WKT member; columns are points (time_dim = 1)
NUM_LAYERS = 2
GRAD_FULL, GRAD_STRIDE = 16384, 16


def make_features(rng, N, avoid):
    """The feature list X = [X0, [datatype, [[encodings, node_idx, seq_lengths]], gpu], ...] and its flat form."""
    flat = {}
    # xsd.string: token sequences, node ids NOT ascending, one -1 token
    s_nodes = rng.permutation(N)[:22].astype(np.int32)
    s_lens = rng.integers(1, 10, len(s_nodes))
    toks = np.empty(len(s_nodes), dtype=object)
    for i, n in enumerate(s_lens):
        toks[i] = rng.integers(2, 50, int(n)).astype(np.int64)
    toks[3][0] = -1
    flat["string.tokens"] = np.concatenate(list(toks))
    flat["string.offsets"] = np.concatenate([[0], np.cumsum(s_lens)]).astype(np.int64)
    flat["string.node_idx"] = s_nodes
    flat["string.seq_lengths"] = s_lens.astype(np.int32)
    # ogc.wktLiteral: CSR members [C_WKT, width], widths 2..12 (shorter and longer than 5), ascending node ids
    w_nodes = np.sort(rng.choice(N, 16, replace=False)).astype(np.int32)
    widths = rng.integers(2, 13, len(w_nodes))
    widths[[1, 6, 11]] = (3, 2, 4)
    mats = np.empty(len(w_nodes), dtype=object)
    for i, w in enumerate(widths):
        d = rng.standard_normal((C_WKT, int(w))).astype(np.float32)
        d[rng.random(d.shape) < 0.3] = 0.0
        mats[i] = sp.csr_matrix(d)
    flat["wkt.data"] = np.concatenate([m.data for m in mats]).astype(np.float32)
    flat["wkt.indices"] = np.concatenate([m.indices for m in mats]).astype(np.int32)
    flat["wkt.indptr"] = np.stack([m.indptr for m in mats]).astype(np.int32)     # [members, C_WKT + 1]
    flat["wkt.nnz"] = np.asarray([m.nnz for m in mats], dtype=np.int64)
    flat["wkt.widths"] = widths.astype(np.int64)
    flat["wkt.node_idx"] = w_nodes
    flat["wkt.seq_lengths"] = widths.astype(np.int32)
    # xsd.numeric: fixed width
    n_nodes = np.sort(rng.choice(N, 25, replace=False)).astype(np.int32)
    flat["numeric.enc"] = rng.standard_normal((25, 3)).astype(np.float32)
    flat["numeric.node_idx"] = n_nodes
    flat["numeric.seq_lengths"] = np.ones(25, dtype=np.int32)
    # xsd.boolean: three members, none among batch 0's outermost neighbours
    b_nodes = np.sort(rng.choice(np.asarray(avoid), 3, replace=False)).astype(np.int32)
    flat["boolean.enc"] = rng.standard_normal((3, 2)).astype(np.float32)
    flat["boolean.node_idx"] = b_nodes
    flat["boolean.seq_lengths"] = np.ones(3, dtype=np.int32)
    flat["X0"] = np.empty((N, 0), dtype=np.float32)
    return flat


def features_from_flat(flat):
    """The reference's feature list, rebuilt from the flat arrays (the tests do the same)."""
    offs, tok = flat["string.offsets"], flat["string.tokens"]
    toks = np.empty(len(offs) - 1, dtype=object)
    for i in range(len(toks)):
        toks[i] = tok[offs[i]:offs[i + 1]].copy()
    nnz = flat["wkt.nnz"]
    starts = np.concatenate([[0], np.cumsum(nnz)])
    mats = np.empty(len(nnz), dtype=object)
    for i in range(len(nnz)):
        sl = slice(starts[i], starts[i + 1])
        mats[i] = sp.csr_matrix((flat["wkt.data"][sl], flat["wkt.indices"][sl], flat["wkt.indptr"][i]),
                                shape=(C_WKT, int(flat["wkt.widths"][i])))
    return [flat["X0"].copy(),
            ["ogc.wktLiteral", [[mats, flat["wkt.node_idx"].copy(), flat["wkt.seq_lengths"].copy()]], False],
            ["xsd.boolean", [[flat["boolean.enc"].copy(), flat["boolean.node_idx"].copy(),
                              flat["boolean.seq_lengths"].copy()]], False],
            ["xsd.numeric", [[flat["numeric.enc"].copy(), flat["numeric.node_idx"].copy(),
                              flat["numeric.seq_lengths"].copy()]], False],
            ["xsd.string", [[toks, flat["string.node_idx"].copy(), flat["string.seq_lengths"].copy()]], False]]


def embedding_config(lm):
    return [("ogc.wktLiteral", (C_WKT, 5, "S", 0.0), False), ("xsd.boolean", (2, 2, 0.0), False),
            ("xsd.numeric", (3, 3, 0.0), False), ("xsd.string", (lm, 4, 0.0), False)]


def main():
    ref = mg.import_reference()
    import mrgcn.data.batch as rb
    import mrgcn.models.mrgcn as rm
    g = np.load(os.path.join(HERE, "graph_small.npz"))
    N, P = int(g["num_nodes"]), int(g["num_pred"])
    R = 2 * P + 1
    A_csr = mg.reference_adjacency(ref, g["triples"], N, P)
    rng = np.random.default_rng(21)
    batches = [np.sort(rng.choice(N, k, replace=False)).astype(np.int64) for k in (3, 6, 8)]
    outer0 = rb.MiniBatch(A_csr, None, batches[0], NUM_LAYERS).A.neighbours[-1]
    avoid = np.setdiff1d(np.arange(N), outer0)
    assert len(avoid) >= 3, "batch 0 reaches every node: pick another seed"
    flat = make_features(rng, N, avoid)
    out = {"in." + k: v for k, v in flat.items()}
    out["num_layers"] = np.int64(NUM_LAYERS)
    out["pad_symbol"] = np.int64(PAD)
    out["c_wkt"] = np.int64(C_WKT)
    names = ["wkt", "boolean", "numeric", "string"]
    for b, idx in enumerate(batches):
        X = features_from_flat(flat)
        mb = rb.MiniBatch(A_csr, X, idx, NUM_LAYERS)
        mb.pad_(pad_symbols={"xsd.string": PAD})
        mb.to_dense_()
        mb.as_tensors_()
        out[f"b{b}.idx"] = idx
        out[f"b{b}.outer"] = np.asarray(mb.A.neighbours[-1], dtype=np.int64)
        out[f"b{b}.X0"] = mb.X[0].numpy().copy()
        widths = []
        for name, (_, sets, _) in zip(names, mb.X[1:]):
            enc, nidx, seq = sets[0]
            out[f"b{b}.{name}.enc"] = enc.numpy().copy()
            out[f"b{b}.{name}.node_idx"] = nidx.numpy().copy()
            out[f"b{b}.{name}.seq_lengths"] = seq.numpy().copy()
            widths.append(tuple(enc.shape))
        print("batch", b, "outer", len(out[f"b{b}.outer"]), "shapes", widths)
        assert out[f"b{b}.wkt.enc"].ndim == 3 and out[f"b{b}.wkt.enc"].shape[2] >= 4   # the TCNN "S" stack
    assert out["b0.boolean.enc"].size == 0 and out["b2.boolean.enc"].size > 0

    # the reference MRGCN on batch 2 (every set present): logits of the batch nodes and every gradient
    B = 2
    torch.manual_seed(31)
    lm = TinyLM()
    rm.loadFromHub = lambda config: lm      # (the hub config is not fetched: the stand-in is the backbone)
    modules = [(5 + 2 + 3 + 4, 6, "mrgcn", nn.ReLU()), (6, 4, "mrgcn", None)]
    model = ref.mrgcn.MRGCN(modules, embedding_config(["stand-in"]), R, N, num_bases=2, p_dropout=0.0,
                            featureless=False, bias=False)
    out.update(checksums("mrgcn.sd.", model.state_dict()))
    X = features_from_flat(flat)
    mb = rb.MiniBatch(A_csr, X, batches[B], NUM_LAYERS)
    mb.pad_(pad_symbols={"xsd.string": PAD})
    mb.to_dense_()
    mb.as_tensors_()
    logits = model(mb)
    y = torch.from_numpy(rng.integers(0, 4, len(batches[B])))
    loss = nn.CrossEntropyLoss()(logits, y)
    loss.backward()
    out["mrgcn.batch"] = np.int64(B)
    out["mrgcn.y"] = y.numpy()
    out["mrgcn.logits"] = logits.detach().numpy().copy()
    out["mrgcn.loss"] = np.float32(loss.item())
    grads = mg.grads_to_np("mrgcn.grad.", model)
    for k, v in grads.items():
        # the TCNN's wide convolutions (~0.6 M weights) are stored as every GRAD_STRIDE-th element + their sums
        out[k] = v if v.size <= GRAD_FULL else v.reshape(-1)[::GRAD_STRIDE].copy()
        out[k + ".sum"], out[k + ".abs"] = np.float64(v.astype(np.float64).sum()), np.float64(np.abs(v).sum())
    out["mrgcn.grad_keys"] = np.asarray(sorted(k[len("mrgcn.grad."):] for k in grads))
    print("mrgcn", logits.shape, "loss", loss.item(), "grads", len(grads), "gate_map", model.gate_map)
    np.savez_compressed(os.path.join(HERE, "minibatch_literals.npz"), **out)
    print(os.path.getsize(os.path.join(HERE, "minibatch_literals.npz")))


if __name__ == "__main__":
    main()
