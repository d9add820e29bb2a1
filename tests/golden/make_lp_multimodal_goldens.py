#!/usr/bin/env python
"""Golden vectors for mini-batch link prediction with literal features, AUTHORING CONTAINER ONLY: imports the
reference (rdflib stubbed as in make_goldens.py) and drives, on the 50-node golden graph,
  mrgcn/tasks/link_prediction.py:477-530   mkbatches(A, X, facts, 8, 1000, num_layers)
  mrgcn/models/rgcn.py:91-128              RGCN._forward_mini_batch with a FEATURED wide `mrgcn` layer
  mrgcn/layers/graph.py:62-102             (W_F = comp_F . V_F, X . W_F[r] on the all-ones slice, A_idx)
  mrgcn/models/mrgcn.py:216-248            MRGCN(link_prediction=True) with one xsd.numeric MLP set
  mrgcn/tasks/link_prediction.py:239-323   within-batch negatives, score_distmult_bc, BCE, clip_grad_norm_, Adam
Parameters are drawn from a seeded numpy generator (`init_state`, which the tests repeat), so no initial state is
stored; arrays of more than BIG elements are stored as every STRIDE-th element and their float64 sum.
    python tests/golden/make_lp_multimodal_goldens.py"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as mg  # noqa: E402
from make_lp_minibatch_goldens import negatives  # noqa: E402

# tag: (K, F, B, training steps)
MODELS = {"k6f200b2": (6, 200, 2, 3), "k145f200b2": (145, 200, 2, 0), "k37f32b1": (37, 32, 1, 0),
          "k13f32b4": (13, 32, 4, 0)}
KMAX = 145
BIG, STRIDE = 4000, 7


def init_state(sd, seed):
    """Every parameter (the reference's layout) from a seeded generator, in sorted key order."""
    rng = np.random.default_rng(seed)
    return {k: torch.from_numpy(rng.uniform(-0.2, 0.2, tuple(sd[k].shape)).astype(np.float32)) for k in sorted(sd)}


def put(out, key, a):
    a = np.asarray(a)
    if a.size > BIG:
        out[key + ".sum"] = np.float64(a.astype(np.float64).sum())
        a = a.reshape(-1)[::STRIDE].copy()
    out[key] = a


def features(N):
    """The feature matrix of the featured layers (the tests draw the same: numpy's PCG64 stream)."""
    return np.random.default_rng(41).standard_normal((N, KMAX)).astype(np.float32)


def numeric_features(N, rng):
    nodes = np.sort(rng.choice(N, 30, replace=False)).astype(np.int64)
    enc = rng.standard_normal((30, 3)).astype(np.float32)
    return nodes, enc


def feature_list(N, nodes, enc):
    return [np.empty((N, 0), dtype=np.float32),
            ["xsd.numeric", [[enc.copy(), nodes.copy(), np.ones(len(nodes), dtype=np.int32)]], False]]


def lp_loss(rlp, E, Rel, data, neg):
    tr = torch.from_numpy(np.concatenate([data, neg]))
    Y = torch.ones(tr.shape[0])
    Y[data.shape[0]:] = 0
    return nn.BCEWithLogitsLoss()(rlp.score_distmult_bc((tr[:, 0], tr[:, 1], tr[:, 2]), E, Rel), Y)


def main():
    ref = mg.import_reference()
    import mrgcn.tasks.link_prediction as rlp
    g = np.load(os.path.join(HERE, "graph_small.npz"))
    N, P = int(g["num_nodes"]), int(g["num_pred"])
    R = 2 * P + 1
    A_csr = mg.reference_adjacency(ref, g["triples"], N, P)
    facts = np.asarray(g["triples"], dtype=np.int64)
    rng = np.random.default_rng(43)
    Xfull = features(N)
    out = {"facts": facts}
    batches = rlp.mkbatches(A_csr, None, facts, 8, 1000, 1)
    for b, _ in batches:
        b.as_tensors_()
    out["count"] = np.int64(len(batches))
    for i in range(3):
        out[f"b{i}.nodes"] = np.asarray(batches[i][0].node_index, dtype=np.int64)
        out[f"b{i}.outer"] = np.asarray(batches[i][0].A.neighbours[-1], dtype=np.int64)

    def xsub(batch, K, grad=False):
        x = torch.from_numpy(Xfull[np.asarray(batch.A.neighbours[-1]), :K].copy())
        return x.requires_grad_(grad)

    for tag, (K, F, B, steps) in MODELS.items():
        model = ref.rgcn.RGCN([(K, F, "mrgcn", nn.ReLU())], R, N, B, 0.0, False, False, True)
        model.load_state_dict(init_state(model.state_dict(), 5))
        pre = ref.rgcn.RGCN([(K, F, "mrgcn", None)], R, N, B, 0.0, False, False, True)
        pre.load_state_dict(model.state_dict())
        with torch.no_grad():
            for i in range(3):
                E = model(xsub(batches[i][0], K), batches[i][0].A)
                Z = pre(xsub(batches[i][0], K), batches[i][0].A)
                assert torch.equal(E, torch.relu(Z))   # (so only the pre-activations are stored)
                out[f"{tag}.pre{i}"] = Z.numpy().copy()
        rs = np.random.RandomState(17)
        batch, data = batches[1]
        neg = negatives(data, rs)
        out[f"{tag}.neg"] = neg
        x = xsub(batch, K, grad=True)
        loss = lp_loss(rlp, model(x, batch.A), model.relations, data, neg)
        loss.backward()
        out[f"{tag}.loss"] = np.float32(loss.item())
        for k, v in mg.grads_to_np(f"{tag}.grad.", model).items():
            put(out, k, v)
        put(out, f"{tag}.grad.X", x.grad.numpy().copy())
        if steps:
            model.zero_grad()
            opt = torch.optim.Adam(model.parameters(), lr=0.01)
            for s in range(steps):
                batch, data = batches[s]
                neg = negatives(data, rs)
                out[f"{tag}.step{s}.neg"] = neg
                opt.zero_grad()
                loss = lp_loss(rlp, model(xsub(batch, K), batch.A), model.relations, data, neg)
                loss.backward()
                torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
                opt.step()
                out[f"{tag}.step{s}.loss"] = np.float32(loss.item())
            for k, v in mg.state_to_np(f"{tag}.final.", model.state_dict()).items():
                put(out, k, v)
        print(tag, "loss", float(out[f"{tag}.loss"]))

    # two layers: a featureless 32-wide input layer, then a hidden 32 -> 200 layer with 2 bases
    batches2 = rlp.mkbatches(A_csr, None, facts, 8, 1000, 2)
    for b, _ in batches2:
        b.as_tensors_()
    model = ref.rgcn.RGCN([(0, 32, "mrgcn", nn.ReLU()), (32, 200, "mrgcn", nn.ReLU())], R, N, 2, 0.0, True, False,
                          True)
    model.load_state_dict(init_state(model.state_dict(), 6))
    with torch.no_grad():
        for i in range(2):
            out[f"two.E{i}"] = model(None, batches2[i][0].A).numpy().copy()
            out[f"two.b{i}.nodes"] = np.asarray(batches2[i][0].node_index, dtype=np.int64)
    rs = np.random.RandomState(19)
    batch, data = batches2[1]
    neg = negatives(data, rs)
    out["two.neg"] = neg
    loss = lp_loss(rlp, model(None, batch.A), model.relations, data, neg)
    loss.backward()
    out["two.loss"] = np.float32(loss.item())
    for k, v in mg.grads_to_np("two.grad.", model).items():
        put(out, k, v)
    print("two loss", float(out["two.loss"]))

    # MRGCN(link_prediction=True): one xsd.numeric MLP set feeding a 200-wide, 2-basis layer (ML100k+ in miniature)
    nodes, enc = numeric_features(N, rng)
    out["num.nodes"], out["num.enc"] = nodes, enc
    torch.manual_seed(7)
    modules = [(3, 200, "mrgcn", nn.ReLU())]
    model = ref.mrgcn.MRGCN(modules, [("xsd.numeric", (3, 3, 0.0), False)], R, N, num_bases=2, p_dropout=0.0,
                            featureless=False, bias=False, link_prediction=True)
    model.load_state_dict(init_state(model.state_dict(), 8))
    mb = rlp.mkbatches(A_csr, feature_list(N, nodes, enc), facts, 8, 1000, 1)
    for b, _ in mb:
        b.pad_(pad_symbols={})
        b.to_dense_()
        b.as_tensors_()
    out["mrgcn.keys"] = np.asarray(sorted(model.state_dict()))
    with torch.no_grad():
        for i in range(2):
            out[f"mrgcn.E{i}"] = model(mb[i][0]).numpy().copy()
    rs = np.random.RandomState(23)
    batch, data = mb[1]
    neg = negatives(data, rs)
    out["mrgcn.neg"] = neg
    loss = lp_loss(rlp, model(batch), model.rgcn.relations, data, neg)
    loss.backward()
    out["mrgcn.loss"] = np.float32(loss.item())
    for k, v in mg.grads_to_np("mrgcn.grad.", model).items():
        put(out, k, v)
    out["mrgcn.grad_keys"] = np.asarray(sorted(n for n, p in model.named_parameters() if p.grad is not None))
    model.zero_grad()
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    for s in range(3):
        batch, data = mb[s]
        neg = negatives(data, rs)
        out[f"mrgcn.step{s}.neg"] = neg
        opt.zero_grad()
        loss = lp_loss(rlp, model(batch), model.rgcn.relations, data, neg)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
        opt.step()
        out[f"mrgcn.step{s}.loss"] = np.float32(loss.item())
    for k, v in mg.state_to_np("mrgcn.final.", model.state_dict()).items():
        put(out, k, v)
    print("mrgcn loss", float(out["mrgcn.loss"]), "grads", list(out["mrgcn.grad_keys"]))
    path = os.path.join(HERE, "lp_multimodal.npz")
    np.savez_compressed(path, **out)
    print("size", os.path.getsize(path))


if __name__ == "__main__":
    main()
