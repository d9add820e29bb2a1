#!/usr/bin/env python
"""The L1 / L2 weight penalty of the link-prediction loops at the FB15k-237 shape of tools/lp_minibatch_fit_probe.py
(`synth.make_graph("fb15k")`, 1 011 masked batches, one featureless mrgcn layer of 200 outputs, 2 bases), three rows
each for the median batch's `train_batch_step`, for a replayed full-batch epoch (`train.GraphedStep` around
`train_step`) and for a whole eager training epoch over all batches:
  plain    no penalty, no weight decay (the step as it was)
  kernel   l1 = 1e-5, l2 = 5e-4, weight_decay = 5e-4 with the penalty inside the optimizer's step
           (`ClipAdam.step(dense_penalty="kernel")`: csrc/optim.hip's two penalty launches)
  by_hand  the same numbers in the loop one had to write before: `weight_regularisation` added to the loss, a plain
           `optimizer.step()` — nothing but functions the package had before the penalty arguments existed
The rows of a group are sampled alternately: each sample one call between two synchronisations, medians of `--samples`
samples after `--warmup`, with the 10th / 90th percentiles.  On a tree without the penalty arguments the `kernel` rows
are left out (so the same script measures `plain` and `by_hand` there).  Writes profiles/lp_penalty_probe.json.

    python tools/lp_penalty_probe.py [--out FILE] [--samples 20] [--warmup 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
L1, L2, WD = 1e-5, 5e-4, 5e-4


def _wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def _alternating(fns, samples, warmup):
    """{name: median seconds per call and the p10 / p90}, the callables taking turns sample by sample."""
    ts = {k: [] for k in fns}
    for s in range(warmup + samples):
        for k, fn in fns.items():
            t = _wall(fn)
            if s >= warmup:
                ts[k].append(t)
    return {k: dict(median_s=float(np.median(v)), p10_p90_s=[float(np.percentile(v, 10)), float(np.percentile(v, 90))])
            for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "lp_penalty_probe.json"))
    args = ap.parse_args()
    from mrgcn_amd import synth
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.plan import plan_of
    from mrgcn_amd.tasks import link_prediction as lp
    from mrgcn_amd.train import ClipAdam, GraphedStep, weight_regularisation
    has_kernel = hasattr(lp, "penalty_owners")

    sg = synth.make_graph("fb15k", seed=0)
    N, R = sg.num_nodes, sg.num_relations
    facts = np.asarray(sg.triples, dtype=np.int64)
    A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([sg.rows, sg.cols])), torch.from_numpy(sg.vals),
                                (N, R * N)).cuda()
    plan = plan_of(A, N, R)
    bs = lp.prepare_batches(lp.mkbatches(None, None, facts, 32, 500, 1, plan=plan), "cuda")
    out = {"device": torch.cuda.get_device_name(0), "batches": len(bs), "kernel_rows": has_kernel,
           "penalty": dict(l1_lambda=L1, l2_lambda=L2, weight_decay=WD),
           "method": dict(samples=args.samples, warmup=args.warmup, unit="seconds per call, synchronised")}

    def fresh(wd):
        torch.manual_seed(0)
        model = RGCN([(0, 200, "mrgcn", torch.nn.ReLU())], R, N, 2, 0.0, True, False, True).cuda()
        opt = ClipAdam(list(model.parameters()), lr=0.01, weight_decay=wd, max_norm=1.0, capturable=True)
        return model, opt

    kinds = ("plain", "kernel", "by_hand") if has_kernel else ("plain", "by_hand")
    state = {k: fresh(0.0 if k == "plain" else WD) for k in kinds}

    def batch_step(kind, batch, f):
        model, opt = state[kind]
        if kind == "plain":
            return lp.train_batch_step(model, batch, f, opt)
        if kind == "kernel":
            return lp.train_batch_step(model, batch, f, opt, l1_lambda=L1, l2_lambda=L2)
        triples, labels = batch._mrgcn_lp["sampler"]()
        opt.zero_grad()
        loss = lp.binary_crossentropy(lp.score_distmult_bc(triples, lp._embed(model, batch), model.relations), labels)
        loss = loss + weight_regularisation(model, L1, L2)
        loss.backward()
        opt.step()
        return loss.detach()

    # ---- the median batch's step ---------------------------------------------------------------------------------
    order = np.argsort([len(f) for _, f in bs], kind="stable")
    mb, mf = bs[int(order[len(order) // 2])]
    for model, _ in state.values():
        model.train()
    out["batch_step"] = _alternating({k: (lambda k=k: batch_step(k, mb, mf)) for k in kinds}, args.samples, args.warmup)
    out["batch_step"]["shape"] = dict(nodes=int(len(mb.node_index)), facts=int(len(mf)))
    print("batch_step", json.dumps(out["batch_step"]), flush=True)

    # ---- a whole eager training epoch ----------------------------------------------------------------------------
    # (fit_batches' own training epoch — every batch's step, its loss into its slot, the mean into the loss ring —
    # for `plain` and `kernel`; the hand-written steps over the same batches for `by_hand`)
    def by_hand_epoch():
        for batch, f in bs:
            batch_step("by_hand", batch, f)
    epochs = {"plain": lp.BatchFitEpochs(*state["plain"][:1], bs, [], state["plain"][1], None, 8, False).train_epoch}
    if has_kernel:
        epochs["kernel"] = lp.BatchFitEpochs(state["kernel"][0], bs, [], state["kernel"][1], None, 8, False,
                                             l1_lambda=L1, l2_lambda=L2).train_epoch
    epochs["by_hand"] = by_hand_epoch
    out["epoch"] = _alternating(epochs, args.samples, args.warmup)
    print("epoch", json.dumps(out["epoch"]), flush=True)

    # ---- a replayed full-batch epoch -----------------------------------------------------------------------------
    train_dev = torch.from_numpy(facts).cuda()
    steps = {}
    for kind in kinds:
        model, opt = fresh(0.0 if kind == "plain" else WD)
        model.train()
        sampler = lp.DeviceNegativeSampler(train_dev)
        static = lp.SortedTriples(sampler.facts, N, R)

        def full(model=model, opt=opt, sampler=sampler, static=static, kind=kind):
            if kind == "plain":
                return lp.train_step(model, lambda: model(None, A), sampler, opt, static)
            if kind == "kernel":
                return lp.train_step(model, lambda: model(None, A), sampler, opt, static, l1_lambda=L1, l2_lambda=L2)
            triples, labels = sampler()
            loss = lp.binary_crossentropy(lp.score_distmult_bc(triples, model(None, A), model.relations, static=static),
                                          labels)
            loss = loss + weight_regularisation(model, L1, L2)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            return loss.detach()
        steps[kind] = GraphedStep(full, warmup=3)
    out["full_batch_replayed"] = _alternating(steps, args.samples, args.warmup)
    print("full_batch_replayed", json.dumps(out["full_batch_replayed"]), flush=True)

    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
