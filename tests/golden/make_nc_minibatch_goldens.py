#!/usr/bin/env python
"""Golden vectors for the mini-batch node-classification run loop, AUTHORING CONTAINER ONLY: imports the reference
(rdflib stubbed as in make_goldens.py) and runs, on the 50-node golden graph and on the CPU,
  mrgcn/tasks/node_classification.py:329-351   mkbatches (batchsize 8, and 0 for the FullBatch structure)
  mrgcn/tasks/node_classification.py:112-227   train_model: 8 epochs over the fixed batches, Adam lr 0.01
  mrgcn/tasks/node_classification.py:229-256   eval_model (inside train_model)
  mrgcn/tasks/node_classification.py:258-310   test_model on the state after the last epoch
for a 2-layer R-GCN (hidden 6, 4 classes, 3 bases, bias): featureless (`fl_b3`), with 5 given feature columns
(`ft_b3`), featureless with l2_lambda = 5e-4 (`fl_b3_l2`), and `fl_b3` under EarlyStop(patience=2, tolerance=10.0,
delay=0) (`fl_b3_stop`: nothing improves by 10, so it stops at record 3 and restores the state of epoch 1).

The model handed to the reference's loop is its RGCN behind a three-line module that answers `model(batch)`,
`model.rgcn.num_layers` and `model.devices` the way its MRGCN does without encoders (mrgcn.py:216-248: the batch's given
feature columns, then the R-GCN).  The per-batch lists of an epoch are seen through the `np.mean` the loop calls on them
(:203-204, :253-254), every evaluated logits row through `categorical_accuracy` (:432-437) — whose top-two margin must
exceed 1e-3 over all epochs and splits (asserted; the label seed is the first for which it holds), so accuracies and
labels compare exactly.
    python tests/golden/make_nc_minibatch_goldens.py"""
import os
import sys

import numpy as np
import scipy.sparse as sp
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as mg  # noqa: E402

N_TRAIN, N_VALID, N_TEST, CLASSES, HIDDEN, BATCHSIZE, NEPOCH, XW = 23, 11, 9, 4, 6, 8, 8, 5
MARGIN = 1e-3
# tag -> (featureless, l2_lambda, early stop)
CASES = {"fl_b3": (True, 0.0, False), "ft_b3": (False, 0.0, False), "fl_b3_l2": (True, 5e-4, False),
         "fl_b3_stop": (True, 0.0, True)}


class _Means:
    """numpy as the task module sees it, with `mean` also keeping the list it was given."""

    def __init__(self):
        self.lists = []

    def __getattr__(self, name):
        return getattr(np, name)

    def mean(self, values, *a, **kw):
        self.lists.append([float(v) for v in values])
        return np.mean(values, *a, **kw)


class _Labels(sp.csr_matrix):
    """The loop indexes the label matrix with `batch.node_index` once that is a tensor (:163-167), which the scipy of the
    authoring container no longer takes: the same index as an array."""

    def __getitem__(self, key):
        return super().__getitem__(key.numpy() if torch.is_tensor(key) else key)


def label_matrix(nodes, classes, N):
    return _Labels((np.ones(len(nodes), dtype=np.int8), (nodes, classes)), shape=(N, CLASSES), dtype=np.int8)


def run(seed, ref, A_csr, N, R):
    rnc = ref.nc
    rng = np.random.default_rng(seed)
    nodes = rng.choice(N, N_TRAIN + N_VALID + N_TEST, replace=False).astype(np.int64)
    classes = rng.integers(0, CLASSES, len(nodes)).astype(np.int64)
    cut = np.cumsum([N_TRAIN, N_VALID])
    split = dict(zip(("train", "valid", "test"), zip(np.split(nodes, cut), np.split(classes, cut))))
    Y = {k: label_matrix(n, c, N) for k, (n, c) in split.items()}
    X_full = rng.standard_normal((N, XW)).astype(np.float32)
    out = {"seed": np.int64(seed), "X_full": X_full}
    for k, (n, c) in split.items():
        out[f"{k}.nodes"], out[f"{k}.classes"] = n, c
        batches = rnc.mkbatches(A_csr, None, Y[k], BATCHSIZE, 2)
        out[f"{k}.count"] = np.int64(len(batches))
        for i, b in enumerate(batches):
            pos, tgt = Y[k][b.node_index].nonzero()
            out[f"{k}.{i}.node_index"] = np.asarray(b.node_index, dtype=np.int64)
            out[f"{k}.{i}.pos"], out[f"{k}.{i}.targets"] = pos.astype(np.int64), tgt.astype(np.int64)
    full = rnc.mkbatches(A_csr, None, Y["train"], 0, 2)
    out["full.count"] = np.int64(len(full))
    out["full.kind"] = np.array(type(full[0]).__name__)
    out["full.node_index"] = np.asarray(full[0].node_index, dtype=np.int64)

    margin = [np.inf]
    accuracy = rnc.categorical_accuracy

    def watched_accuracy(Y_hat, Yb):
        idx, _ = Yb.nonzero()
        top = torch.topk(Y_hat.detach()[idx], 2, dim=1).values
        margin[0] = min(margin[0], float((top[:, 0] - top[:, 1]).min()))
        return accuracy(Y_hat, Yb)

    means = _Means()
    rnc.categorical_accuracy, rnc.np = watched_accuracy, means
    try:
        for tag, (featureless, l2, stop) in CASES.items():
            torch.manual_seed(seed + 1)
            modules = [(0 if featureless else XW, HIDDEN, "mrgcn", torch.nn.ReLU()), (HIDDEN, CLASSES, "mrgcn", None)]
            rgcn = ref.rgcn.RGCN(modules, R, N, 3, 0.0, featureless, True, False)

            class Model(torch.nn.Module):
                def __init__(self):
                    super().__init__()
                    self.rgcn, self.devices = rgcn, {"relational": torch.device("cpu")}

                def forward(self, batch):
                    return self.rgcn(None if featureless else batch.X[0].float(), batch.A)

            model = Model()
            out.update(mg.state_to_np(f"{tag}.init.", rgcn.state_dict()))
            # (featureless: the reference's batches still want the zero-width X[0] of its dataset build)
            X = [np.empty((N, 0), dtype=float)] if featureless else [X_full]
            optimizer = torch.optim.Adam(model.parameters(), lr=0.01)
            criterion = torch.nn.CrossEntropyLoss()
            early = ref.tutils.EarlyStop(patience=2, tolerance=10.0, delay=0) if stop else None
            means.lists.clear()
            rows = list(rnc.train_model(A_csr, model, optimizer, criterion, X, Y, 0, NEPOCH, "valid", BATCHSIZE, 0.0, l2,
                                        dict(), early))
            out[f"{tag}.rows"] = np.asarray([r[1:] for r in rows], dtype=np.float64)
            out[f"{tag}.epochs"] = np.asarray([r[0] for r in rows], dtype=np.int64)
            # the four lists of epoch 1, in the order the loop takes their means
            for name, lst in zip(("train_loss", "train_acc", "valid_loss", "valid_acc"), means.lists[:4]):
                out[f"{tag}.epoch1.{name}"] = np.asarray(lst, dtype=np.float64)
            out.update(mg.state_to_np(f"{tag}.final.", rgcn.state_dict()))
            loss, acc, labels, targets = rnc.test_model(A_csr, model, criterion, X, Y, "test", BATCHSIZE, dict())
            out[f"{tag}.test.loss"], out[f"{tag}.test.acc"] = np.float64(loss), np.float64(acc)
            out[f"{tag}.test.labels"] = np.asarray(labels, dtype=np.int64)
            out[f"{tag}.test.targets"] = np.asarray(targets, dtype=np.int64)
            print(f"  {tag}: {len(rows)} rows, last {rows[-1][1:]}, test loss {loss:.4f} acc {acc:.4f}")
    finally:
        rnc.categorical_accuracy, rnc.np = accuracy, np
    return out, margin[0]


def main():
    ref = mg.import_reference()
    g = np.load(os.path.join(HERE, "graph_small.npz"))
    N, P = int(g["num_nodes"]), int(g["num_pred"])
    A_csr = mg.reference_adjacency(ref, g["triples"], N, P)
    for seed in range(100, 200):
        out, margin = run(seed, ref, A_csr, N, 2 * P + 1)
        print("seed", seed, "smallest top-two margin", margin)
        if margin > MARGIN:
            break
    assert margin > MARGIN, margin
    assert len(out["fl_b3_stop.rows"]) == 3, "the early-stop case stops at record 3"
    assert [int(out[f"{k}.count"]) for k in ("train", "valid", "test")] == [3, 2, 2]
    assert len(out["test.1.node_index"]) == 1   # (the one-row batch)
    out["margin"] = np.float64(margin)
    path = os.path.join(HERE, "nc_minibatch.npz")
    np.savez_compressed(path, **out)
    print("size", os.path.getsize(path))


if __name__ == "__main__":
    main()
