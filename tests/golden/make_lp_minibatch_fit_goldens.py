#!/usr/bin/env python
"""Golden vectors for the mini-batch link-prediction run loop, AUTHORING CONTAINER ONLY: imports the reference (rdflib
stubbed as in make_goldens.py) and runs, on the 50-node golden graph and on the CPU,
  mrgcn/tasks/link_prediction.py:477-530   mkbatches of a 90 / 30 train / valid split of the 120 facts
  mrgcn/tasks/link_prediction.py:191-373   train_model with gcn_batchsize > 0: Adam lr 0.01, BCEWithLogitsLoss
  mrgcn/tasks/link_prediction.py:375-422   test_model (inside train_model)
for one featureless mrgcn layer (32 wide, 2 bases, ReLU) behind the three-line module of make_nc_minibatch_goldens.py:
`nb17` (gcn_batchsize 17, test_batchsize 40: 3 + 2 batches, two of them with more facts than nodes) and `nb13`
(13, 20: 6 + 3 batches), 6 epochs with eval_interval 2, and `nb13_stop`: eval_interval 1 under EarlyStop(patience=2,
tolerance=10.0, delay=0) — nothing improves by 10, so it yields 3 rows and restores the state of epoch 1.

The loop is watched from outside: the module's `np` is a proxy whose `random.choice` keeps every draw (the negatives of
every (epoch, batch) are rebuilt from them, :249-264) and whose `mean` keeps every list it is given (:331, :418-419);
`compute_ranks_fast` is wrapped to also compute, for the same embeddings, the best and the worst rank every fact can
take when each candidate within TAU of the true score is counted as below it or as above it.  The metrics of a run
trained elsewhere in float32 differ from these by such near-tie pairs only, so every metric value is stored with the
interval [lo, hi] those ranks span; the widest interval must stay below WIDTH (asserted).
    python tests/golden/make_lp_minibatch_fit_goldens.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as mg  # noqa: E402

TAU = 1e-4      # near tie: |candidate score - true score| <= TAU
WIDTH = 0.02    # the widest metric interval allowed
NEPOCH, F, B = 6, 32, 2
# tag -> (gcn_batchsize, test_batchsize, eval_interval, early stop)
CASES = {"nb17": (17, 40, 2, False), "nb13": (13, 20, 2, False), "nb13_stop": (13, 20, 1, True)}


class _Random:
    def __init__(self):
        self.draws = []

    def __getattr__(self, name):
        return getattr(np.random, name)

    def choice(self, *a, **kw):
        out = np.random.choice(*a, **kw)
        self.draws.append(np.array(out, dtype=np.int64))
        return out


class _Numpy:
    """numpy as the task module sees it: `mean` keeps its lists, `random.choice` its draws."""

    def __init__(self):
        self.lists, self.random = [], _Random()

    def __getattr__(self, name):
        return getattr(np, name)

    def mean(self, values, *a, **kw):
        self.lists.append([float(v) for v in values])
        return np.mean(values, *a, **kw)


def score_matrices(data, E, Rel):
    """[facts, nodes] float32 scores of every candidate tail and head (all facts scored)."""
    s, p, o = (torch.as_tensor(data[:, k]).long() for k in range(3))
    return (E[s] * Rel[p]) @ E.T, (Rel[p] * E[o]) @ E.T


def rank_bounds(data, E, Rel, filtered, filter_lists):
    """(best, worst) int64 [2 n] ranks under TAU, with the loop's own rules otherwise: facts at positions >= nodes
    unscored, the other true answers of a filtered fact left out, exact ties by half of them, rounded half to even."""
    n, N = len(data), E.shape[0]
    lists = filter_lists(np.asarray(data)) if filtered else None
    best, worst = [], []
    for head, sc in enumerate(score_matrices(np.asarray(data), E, Rel)):
        sc = sc.double().numpy().copy()
        sc[N:] = 0.0
        if filtered:
            ptr, idx = lists[2 * head], lists[2 * head + 1]
            for f in range(n):
                sc[f, idx[ptr[f]:ptr[f + 1]]] = -np.inf
        t = sc[np.arange(n), np.asarray(data)[:, 0 if head else 2]][:, None]
        gt, eq = (sc > t).sum(1), (sc == t).sum(1)
        above, below = ((sc > t) & (sc <= t + TAU)).sum(1), ((sc < t) & (sc >= t - TAU)).sum(1)
        half = np.round((eq - 1) / 2).astype(np.int64)
        best.append(gt - above + half + 1)
        worst.append(gt + below + half + 1)
    return np.concatenate(best), np.concatenate(worst)


def metrics_of(ranks):
    return [float(np.mean(1.0 / ranks))] + [float(np.mean(ranks <= k)) for k in (1, 3, 10)]


def main():
    ref = mg.import_reference()
    import mrgcn.tasks.link_prediction as rlp
    sys.path.insert(0, os.path.join(HERE, "..", ".."))
    from mrgcn_amd.tasks.link_prediction import filter_lists   # (numpy only)
    g = np.load(os.path.join(HERE, "graph_small.npz"))
    N, P = int(g["num_nodes"]), int(g["num_pred"])
    R = 2 * P + 1
    A_csr = mg.reference_adjacency(ref, g["triples"], N, P)
    facts = np.asarray(g["triples"], dtype=np.int64)
    perm = np.random.default_rng(3).permutation(len(facts))
    data = {"valid": facts[perm[:30]], "train": facts[perm[30:]]}
    out = {"train": data["train"], "valid": data["valid"], "tau": np.float64(TAU)}
    widest = 0.0
    for tag, (gb, tb, interval, stop) in CASES.items():
        torch.manual_seed(5)
        rgcn = ref.rgcn.RGCN([(0, F, "mrgcn", torch.nn.ReLU())], R, N, B, 0.0, True, False, True)

        class Model(torch.nn.Module):
            def __init__(self):
                super().__init__()
                self.rgcn, self.devices = rgcn, {"relational": torch.device("cpu")}

            def forward(self, batch):
                return self.rgcn(None, batch.A)

        model = Model()
        out.update(mg.state_to_np(f"{tag}.init.", rgcn.state_dict()))
        for split in ("train", "valid"):
            bs = rlp.mkbatches(A_csr, [np.empty((N, 0), dtype=float)], data[split], gb, tb, 1)
            out[f"{tag}.{split}.count"] = np.int64(len(bs))
            for i, (b, d) in enumerate(bs):
                out[f"{tag}.{split}.{i}.nodes"] = np.asarray(b.node_index, dtype=np.int64)
                out[f"{tag}.{split}.{i}.facts"] = np.asarray(d, dtype=np.int64)
            assert min(len(d) for _, d in bs) >= 5, "the reference fails on a batch of fewer than 5 facts"
            print(tag, split, [(len(b.node_index), len(d)) for b, d in bs])
        train_facts = [out[f"{tag}.train.{i}.facts"] for i in range(int(out[f"{tag}.train.count"]))]
        nt, nv = len(train_facts), int(out[f"{tag}.valid.count"])

        watch = _Numpy()
        bounds = []          # per test_model call: per batch {rank type: (best, worst)}
        ranks_fast, test_model = rlp.compute_ranks_fast, rlp.test_model

        def watched_ranks(d, E, Rel, mrr_batchsize, filtered=True):
            rk = ranks_fast(d, E, Rel, mrr_batchsize, filtered)
            best, worst = rank_bounds(d.numpy(), E.detach(), Rel.detach(), filtered, filter_lists)
            assert np.all(best <= rk.numpy()) and np.all(rk.numpy() <= worst)
            if not filtered:
                bounds[-1].append({})
            bounds[-1][-1]["flt" if filtered else "raw"] = (best, worst)
            return rk

        def watched_test(*a, **kw):
            bounds.append([])
            return test_model(*a, **kw)

        rlp.np, rlp.compute_ranks_fast, rlp.test_model = watch, watched_ranks, watched_test
        try:
            np.random.seed(11)
            early = ref.tutils.EarlyStop(patience=2, tolerance=10.0, delay=0) if stop else None
            optimizer = torch.optim.Adam(model.parameters(), lr=0.01)
            rows = []
            for row in rlp.train_model(A_csr, [np.empty((N, 0), dtype=float)], data, model, optimizer,
                                       torch.nn.BCEWithLogitsLoss(), 0, NEPOCH, gb, tb, 100, interval, True, 0, 0,
                                       dict(), early, torch.device("cpu"), 80):
                rows.append(row)
                if row[0] == 1:
                    out.update(mg.state_to_np(f"{tag}.epoch1.", rgcn.state_dict()))
        finally:
            rlp.np, rlp.compute_ranks_fast, rlp.test_model = np, ranks_fast, test_model
        out.update(mg.state_to_np(f"{tag}.final.", rgcn.state_dict()))

        # the rows: epoch | loss | train raw mrr h1 h3 h10, flt ... | valid the same (NaN where the loop yields None)
        def flat(mrr, hits):
            if mrr is None:
                return [np.nan] * 8
            return [mrr["raw"]] + list(hits["raw"]) + [mrr["flt"]] + list(hits["flt"])

        out[f"{tag}.epochs"] = np.asarray([r[0] for r in rows], dtype=np.int64)
        table = np.asarray([[r[1]] + flat(r[2], r[3]) + flat(r[4], r[5]) for r in rows], dtype=np.float64)
        out[f"{tag}.rows"] = table
        # the same table's bounds: test_model calls in order, train then valid per evaluating row
        lo, hi = table.copy(), table.copy()
        calls = iter(bounds)
        for r, row in enumerate(table):
            for c0 in (1, 9):
                if np.isnan(row[c0]):
                    continue
                per_batch = next(calls)
                for j, kind in enumerate(("raw", "flt")):
                    hi_m = np.mean([metrics_of(b[kind][0]) for b in per_batch], axis=0)
                    lo_m = np.mean([metrics_of(b[kind][1]) for b in per_batch], axis=0)
                    lo[r, c0 + 4 * j:c0 + 4 * j + 4], hi[r, c0 + 4 * j:c0 + 4 * j + 4] = lo_m, hi_m
        assert next(calls, None) is None
        ok = ~np.isnan(table)
        # (the loop's per-batch means are float32, these float64)
        assert np.all(lo[ok] <= table[ok] + 1e-6) and np.all(table[ok] <= hi[ok] + 1e-6)
        widest = max(widest, float((hi - lo)[ok].max()))
        out[f"{tag}.rows_lo"], out[f"{tag}.rows_hi"] = lo, hi

        # the negatives of every (epoch, batch) from the three draws of each step (:249-264)
        draws = iter(watch.random.draws)
        epochs_run = len(watch.random.draws) // (3 * nt)
        assert len(watch.random.draws) == 3 * nt * epochs_run
        out[f"{tag}.epochs_run"] = np.int64(epochs_run)
        for e in range(1, epochs_run + 1):
            for i, d in enumerate(train_facts):
                idx, heads, tails = next(draws), next(draws), next(draws)
                neg = d[idx].copy()
                neg[:len(heads), 0] = heads
                neg[len(neg) - len(tails):, 2] = tails
                out[f"{tag}.neg.{e}.{i}"] = neg

        # the lists of the first evaluating epoch, in the order the loop takes their means: the loss list, then per
        # test_model call flt mrr, flt hits x 3, raw mrr, raw hits x 3
        first = int(np.flatnonzero(~np.isnan(table[:, 1]))[0])
        lists = watch.lists[first:]          # (one loss list per epoch in front of it)
        out[f"{tag}.first_eval.epoch"] = np.int64(rows[first][0])
        out[f"{tag}.first_eval.loss"] = np.asarray(lists[0], dtype=np.float64)
        names = [f"{k}.{m}" for k in ("flt", "raw") for m in ("mrr", "h1", "h3", "h10")]
        for s, split in enumerate(("train", "valid")):
            for j, name in enumerate(names):
                out[f"{tag}.first_eval.{split}.{name}"] = np.asarray(lists[1 + 8 * s + j], dtype=np.float64)
        assert len(out[f"{tag}.first_eval.valid.raw.mrr"]) == nv and len(out[f"{tag}.first_eval.loss"]) == nt

        if not stop:   # the final state's batch embeddings and candidate scores (what the last row's ranks came from)
            model.eval()
            with torch.no_grad():
                for i, (b, d) in enumerate(rlp.mkbatches(A_csr, [np.empty((N, 0), dtype=float)], data["train"], gb, tb,
                                                          1)):
                    b.pad_(pad_symbols=dict())
                    b.to_dense_()
                    b.as_tensors_()
                    E = model(b)
                    tail, head = score_matrices(d, E, rgcn.relations)
                    out[f"{tag}.final.E.{i}"] = E.numpy().copy()
                    out[f"{tag}.final.tail.{i}"], out[f"{tag}.final.head.{i}"] = tail.numpy().copy(), head.numpy().copy()
        print(f"  {tag}: {len(rows)} rows, epochs {[r[0] for r in rows]}, last loss {rows[-1][1]:.4f}")
    print("widest metric interval", widest)
    assert widest <= WIDTH, widest
    assert len(out["nb13_stop.rows"]) == 3, "the early-stop case yields 3 rows"
    for k in [k for k in out if k.startswith("nb13_stop.epoch1.")]:
        assert np.array_equal(out[k], out["nb13_stop.final." + k[len("nb13_stop.epoch1."):]]), k
    out["widest"] = np.float64(widest)
    path = os.path.join(HERE, "lp_minibatch_fit.npz")
    np.savez_compressed(path, **out)
    print("size", os.path.getsize(path))


if __name__ == "__main__":
    main()
