#!/usr/bin/env python
"""Golden vectors for mini-batch link prediction, AUTHORING CONTAINER ONLY: imports the reference (rdflib stubbed as
in make_goldens.py) and drives, on the 50-node golden graph,
  mrgcn/tasks/link_prediction.py:477-530   mkbatches (node batches, array_split of their facts, union1d, remap)
  mrgcn/data/batch.py:166-231              MiniBatch / A_Batch of every batch
  mrgcn/models/rgcn.py:91-128              RGCN._forward_mini_batch (one featureless mrgcn layer + ReLU)
  mrgcn/tasks/link_prediction.py:239-323   within-batch negatives, score_distmult_bc, BCE, clip_grad_norm_, Adam
and records every configuration's batches (node sets, remapped facts), the embeddings of a few batches, the gradients
of one batch loss and the parameters after three training steps on consecutive batches (negatives stored).
    python tests/golden/make_lp_minibatch_goldens.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as mg  # noqa: E402

# (gcn_batchsize, mrr_batchsize): full batch split by facts, node batches, node batches whose facts split
CONFIGS = {"full": (0, 40), "nb8": (8, 1000), "nb8_m10": (8, 10), "nb16_m7": (16, 7)}
# (F, B, training steps recorded)
MODELS = {"f32b1": (32, 1, 0), "f200b2": (200, 2, 0), "f32b4": (32, 4, 0), "f32b2": (32, 2, 3)}


def negatives(batch_data, rs):
    """link_prediction.py:239-263 with a seeded RandomState in place of the global np.random."""
    n = batch_data.shape[0]
    batch_nodes = np.union1d(batch_data[:, 0], batch_data[:, 2])
    ncorrupt = n // 5
    idx = rs.choice(np.arange(n), ncorrupt, replace=False)
    nh = ncorrupt // 2
    nt = ncorrupt - nh
    c = np.empty((ncorrupt, 3), dtype=int)
    c[:] = batch_data[idx]
    c[:nh, 0] = rs.choice(batch_nodes, nh)
    c[-nt:, 2] = rs.choice(batch_nodes, nt)
    return c.astype(np.int64)


def main():
    ref = mg.import_reference()
    import mrgcn.tasks.link_prediction as rlp
    g = np.load(os.path.join(HERE, "graph_small.npz"))
    N, P = int(g["num_nodes"]), int(g["num_pred"])
    R = 2 * P + 1
    A_csr = mg.reference_adjacency(ref, g["triples"], N, P)
    facts = np.asarray(g["triples"], dtype=np.int64)
    out = {"facts": facts}
    for tag, (gb, mb) in CONFIGS.items():
        batches = rlp.mkbatches(A_csr, None, facts, gb, mb, 1)
        out[f"{tag}.count"] = np.int64(len(batches))
        for i, (batch, data) in enumerate(batches):
            out[f"{tag}.{i}.nodes"] = np.asarray(batch.node_index, dtype=np.int64)
            out[f"{tag}.{i}.facts"] = np.asarray(data, dtype=np.int64)
        print(tag, len(batches), "batches", [len(b.node_index) for b, _ in batches])
    batches = rlp.mkbatches(A_csr, None, facts, 8, 1000, 1)
    for b, _ in batches:
        b.as_tensors_()
    for tag, (F, B, steps) in MODELS.items():
        torch.manual_seed(5)
        model = ref.rgcn.RGCN([(0, F, "mrgcn", torch.nn.ReLU())], R, N, B, 0.0, True, False, True)
        out.update(mg.state_to_np(f"{tag}.init.", model.state_dict()))
        crit = torch.nn.BCEWithLogitsLoss()
        rs = np.random.RandomState(17)
        for i in range(3):
            with torch.no_grad():
                out[f"{tag}.E{i}"] = model(None, batches[i][0].A).numpy().copy()
        # one batch loss and its gradients (batch 1)
        batch, data = batches[1]
        neg = negatives(data, rs)
        out[f"{tag}.neg"] = neg
        tr = torch.from_numpy(np.concatenate([data, neg]))
        E = model(None, batch.A)
        Y = torch.ones(tr.shape[0])
        Y[data.shape[0]:] = 0
        loss = crit(rlp.score_distmult_bc((tr[:, 0], tr[:, 1], tr[:, 2]), E, model.relations), Y)
        loss.backward()
        out[f"{tag}.loss"] = np.float32(loss.item())
        out.update(mg.grads_to_np(f"{tag}.grad.", model))
        if steps:
            model.zero_grad()
            opt = torch.optim.Adam(model.parameters(), lr=0.01)
            for s in range(steps):
                batch, data = batches[s]
                neg = negatives(data, rs)
                out[f"{tag}.step{s}.neg"] = neg
                tr = torch.from_numpy(np.concatenate([data, neg]))
                Y = torch.ones(tr.shape[0])
                Y[data.shape[0]:] = 0
                opt.zero_grad()
                E = model(None, batch.A)
                loss = crit(rlp.score_distmult_bc((tr[:, 0], tr[:, 1], tr[:, 2]), E, model.relations), Y)
                loss.backward()
                torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
                opt.step()
                out[f"{tag}.step{s}.loss"] = np.float32(loss.item())
                out.update(mg.state_to_np(f"{tag}.step{s}.", model.state_dict()))
        print(tag, "loss", float(out[f"{tag}.loss"]))
    # test_model's ranking per batch on the f200b2 initial embeddings (raw and filtered)
    torch.manual_seed(5)
    model = ref.rgcn.RGCN([(0, 200, "mrgcn", torch.nn.ReLU())], R, N, 2, 0.0, True, False, True)
    with torch.no_grad():
        for i in range(3):
            batch, data = batches[i]
            E = model(None, batch.A)
            for flt in (False, True):
                rk = rlp.compute_ranks_fast(torch.from_numpy(data), E, model.relations, 50, flt)
                out[f"ranks{i}.{'flt' if flt else 'raw'}"] = rk.numpy().astype(np.int64)
    np.savez_compressed(os.path.join(HERE, "lp_minibatch.npz"), **out)
    print("size", os.path.getsize(os.path.join(HERE, "lp_minibatch.npz")))


if __name__ == "__main__":
    main()
