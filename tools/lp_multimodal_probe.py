#!/usr/bin/env python
"""Mini-batch link prediction WITH literal features at the FB15k-237 shape of synth.py (14 541 nodes, 475 relations)
and the YAGO3-10+ encoder width: one mrgcn layer of 145 constant feature columns -> 200 outputs, 2 bases, no bias,
ReLU (configs/yago3-10+.toml / ml100k+.toml: gcn_batchsize 32, num_bases 2, hidden_nodes 200), batches of
mkbatches(..., 32, 500, 1, plan=...) (masked batches: csrc/basis_xform.hip + the two-table csrc/masked_wide.hip)
against the reference's MiniBatch slices (A_Batch, one plan per batch; the fused slice transform takes out <= 64,
so this layer runs the literal engine there, graph.py's arithmetic op for op), on the same batches.  Records the batch counts and sizes, the build time, the median step time
(train_batch_step: forward, device-drawn negatives, DistMult, BCE, backward, clip, row-sparse Adam), one training
epoch and one evaluation pass (raw + filtered).  Times are wall clock around work that ends in a synchronise.

    python tools/lp_multimodal_probe.py [--steps 50] [--slice-epoch-batches 40] [--out FILE]
    rocprofv3 --kernel-trace --marker-trace --stats --output-format csv -d DIR -o lp_step -- \
        python tools/lp_multimodal_probe.py --trace-step
        (then tools/lp_step_table.py DIR --out profiles/lp_multimodal_kernels.md)"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _sync_time(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


K = 145   # the YAGO3-10+ encoder concatenation


def run_path(name, bs, model_fn, args):
    from mrgcn_amd.optim import RowSparseAdam
    from mrgcn_amd.tasks import link_prediction as lp
    model = model_fn()
    if name == "slice":
        model.set_engine("literal")
    opt = RowSparseAdam(model.parameters(), lr=0.01)
    res = {}
    # warm-up on a few batches (first-use workspaces, lazily built slice plans of those batches)
    for b, f in bs[:3]:
        lp.train_batch_step(model, b, f, opt)
    steps = []
    for b, f in bs[3:3 + args.steps]:
        dt, _ = _sync_time(lambda: lp.train_batch_step(model, b, f, opt))
        steps.append(dt)
    res["median_step_ms"] = 1e3 * float(np.median(steps))
    res["step_ms_p10_p90"] = [1e3 * float(np.percentile(steps, 10)), 1e3 * float(np.percentile(steps, 90))]
    ep = bs if (name == "masked" or args.slice_epoch_batches <= 0) else bs[:args.slice_epoch_batches]
    dt, loss = _sync_time(lambda: lp.train_epoch(ep, model, opt))
    res["epoch_s"] = dt
    res["epoch_batches"] = len(ep)
    res["epoch_loss"] = loss
    dt, (mrr, hits, _) = _sync_time(lambda: lp.evaluate_batches(ep, model, filtered=True))
    res["eval_s"] = dt
    res["eval_mrr"] = {k: float(v) for k, v in mrr.items()}
    # a second epoch on the same batches (what a run repeats: the slice plans are built by now)
    dt, loss2 = _sync_time(lambda: lp.train_epoch(ep, model, opt))
    res["epoch2_s"] = dt
    res["epoch2_loss"] = loss2
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--slice-epoch-batches", type=int, default=40, help="0: the whole epoch on the slice path too")
    ap.add_argument("--skip-slice", action="store_true")
    ap.add_argument("--trace-step", action="store_true", help="one warm masked step only (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join("profiles", "lp_multimodal_probe.json"))
    args = ap.parse_args()
    from mrgcn_amd import synth
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.optim import RowSparseAdam
    from mrgcn_amd.plan import plan_of
    from mrgcn_amd.tasks import link_prediction as lp
    import scipy.sparse as sp

    sg = synth.make_graph("fb15k", seed=0)
    N, R = sg.num_nodes, sg.num_relations
    facts = np.asarray(sg.triples, dtype=np.int64)
    A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([sg.rows, sg.cols])), torch.from_numpy(sg.vals),
                                (N, R * N)).cuda()
    plan = plan_of(A, N, R)

    def model_fn():
        torch.manual_seed(0)
        return RGCN([(K, 200, "mrgcn", torch.nn.ReLU())], R, N, 2, 0.0, False, False, True).cuda()

    # constant features (the encoders themselves are not measured here), every node's row: the masked layer reads the
    # neighbours' rows through the support; the slice batches get X[neighbours[-1]] (what MiniBatch's subset holds)
    Xd = torch.full((N, K), 0.01, device="cuda")

    def with_x(bs, by_node):
        for b, _ in bs:
            b.X = Xd if by_node else Xd.index_select(0, b.A.neighbours[-1].to("cuda").long())
        return bs

    dt_m, bm = _sync_time(lambda: with_x(lp.prepare_batches(lp.mkbatches(None, None, facts, 32, 500, 1, plan=plan),
                                                             "cuda"), True))
    if args.trace_step:
        model = model_fn()
        opt = RowSparseAdam(model.parameters(), lr=0.01)
        for b, f in bm[:3]:
            lp.train_batch_step(model, b, f, opt)
        torch.cuda.synchronize()
        torch.cuda.nvtx.range_push("lp_step")   # (a roctx range: the kernels of this step are the ones inside it)
        lp.train_batch_step(model, bm[3][0], bm[3][1], opt)
        torch.cuda.synchronize()
        torch.cuda.nvtx.range_pop()
        print("traced one step of batch 3")
        return
    sups = [b.A.row[0] for b, _ in bm]
    out = {"shape": dict(nodes=N, predicates=int(sg.num_pred) if hasattr(sg, "num_pred") else 237, relations=R,
                         facts=int(len(facts)), features=K, bases=2, hidden=200, gcn_batchsize=32, test_batchsize=500),
           "batches": len(bm),
           "per_batch": {k: dict(median=float(np.median(v)), min=int(np.min(v)), max=int(np.max(v)))
                         for k, v in dict(nodes=[len(b.node_index) for b, _ in bm], facts=[len(f) for _, f in bm],
                                          rows=[s.NR for s in sups], live_columns=[s.L for s in sups],
                                          entries=[s.E for s in sups], live_nodes=[s.NL for s in sups]).items()},
           "device": torch.cuda.get_device_name(0)}
    out["masked"] = {"build_s": dt_m}
    out["masked"].update(run_path("masked", bm, model_fn, args))
    print(json.dumps(out["masked"]), flush=True)
    if not args.skip_slice:
        A_csr = sp.csr_matrix((sg.vals, (sg.rows, sg.cols)), shape=(N, R * N))
        dt_s, bsl = _sync_time(lambda: with_x(lp.prepare_batches(lp.mkbatches(A_csr, None, facts, 32, 500, 1), "cuda"),
                                              False))
        out["slice"] = {"build_s": dt_s}
        out["slice"].update(run_path("slice", bsl, model_fn, args))
        print(json.dumps(out["slice"]), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
