#!/usr/bin/env python
"""What edge dropout costs (csrc/edge_dropout.hip, RGCN.set_edge_dropout), at the FB15k-237 shape of synth.py
(`synth.make_graph("fb15k")`: one featureless mrgcn layer of 200 outputs, 2 bases, all 310 116 facts) and on the graph
of the AM shape (`synth.make_graph("am")`, 13.6 M entries; the same encoder with `--am-hidden` outputs, trained on the
first `--am-facts` facts so that the decoder does not bury the encoder).  Per shape, medians of `--samples`
synchronised calls after `--warmup` warm-ups, all in one process on one box:
  draw              one layer's draw alone: the three value arrays of an overlay rewritten (mrgcn_edge_dropout_draw_f32)
  epoch_off_first   a replayed `fit` training epoch (tasks.link_prediction.FitEpochs, graphed) with edge dropout off
  epoch_on          the same epoch with set_edge_dropout(0.4, self_loop=0.2)
  epoch_off_last    the first row's epoch again, last in the run
On a tree without `set_edge_dropout` (the parent commit) only the two `epoch_off` rows are written: the same script
measures the parent's epoch on the same box (profiles/edge_dropout_probe_parent.json).

    python tools/edge_dropout_probe.py [--out FILE] [--shapes fb15k am] [--samples 20] [--warmup 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median(fn, samples, warmup):
    ts = []
    for s in range(warmup + samples):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if s >= warmup:
            ts.append(time.perf_counter() - t)
    return dict(median_s=float(np.median(ts)), p10_p90_s=[float(np.percentile(ts, 10)), float(np.percentile(ts, 90))])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=["fb15k", "am"])
    ap.add_argument("--am-hidden", type=int, default=20)
    ap.add_argument("--am-facts", type=int, default=300000)
    ap.add_argument("--out", default=os.path.join("profiles", "edge_dropout_probe.json"))
    args = ap.parse_args()
    from mrgcn_amd import functional as Fn
    from mrgcn_amd import synth
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.plan import plan_of
    from mrgcn_amd.tasks import link_prediction as lp
    from mrgcn_amd.train import ClipAdam
    has = hasattr(RGCN, "set_edge_dropout")
    out = {"device": torch.cuda.get_device_name(0), "edge_dropout": has,
           "method": dict(samples=args.samples, warmup=args.warmup, unit="seconds per call, synchronised",
                          rates=dict(p=0.4, self_loop=0.2))}
    for shape in args.shapes:
        sg = synth.make_graph(shape, seed=0)
        N, R = sg.num_nodes, sg.num_relations
        hidden = 200 if shape == "fb15k" else args.am_hidden
        facts = np.asarray(sg.triples, dtype=np.int64)
        if shape != "fb15k":
            facts = facts[:args.am_facts]
        A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([sg.rows, sg.cols])), torch.from_numpy(sg.vals),
                                    (N, R * N)).cuda()

        def fresh(on):
            torch.manual_seed(0)
            model = RGCN([(0, hidden, "mrgcn", torch.nn.ReLU())], R, N, 2, 0.0, True, False, True).cuda()
            if on:
                model.set_edge_dropout(0.4, self_loop=0.2, seed=1)
            opt = ClipAdam(list(model.parameters()), lr=0.01, max_norm=1.0, capturable=True)
            sampler = lp.DeviceNegativeSampler(torch.from_numpy(facts).cuda())
            static = lp.SortedTriples(sampler.facts, N, R)
            parts = lp.FactParts(facts[:2000], 100, device="cuda")   # (the capture's one evaluating epoch stays small)
            return lp.FitEpochs(model, lambda: model(None, A), parts, None, opt, sampler=sampler, static=static)

        plan = plan_of(A, N, R, operand_row_bytes=[Fn.operand_row_bytes(hidden)])
        row = {"nodes": N, "relations": R, "entries": int(plan.nnz), "hidden": hidden, "facts": int(len(facts))}
        off = fresh(False)
        row["epoch_off_first"] = _median(off.train_epoch, args.samples, args.warmup)
        if has:
            ov = plan.overlay()
            rates = torch.tensor([0.4] * (R - 1) + [0.2], dtype=torch.float32).cuda()
            st = Fn.node_dropout_state(1, 0, rates.device)
            row["draw"] = _median(lambda: ov.draw(rates, st, 0, advance=True), args.samples, args.warmup)
            row["draw"]["bytes_estimate"] = int(plan.nnz) * 16 * (2 if plan.lean else 3)
            ov.close()
            on = fresh(True)
            row["epoch_on"] = _median(on.train_epoch, args.samples, args.warmup)
            del on
        row["epoch_off_last"] = _median(off.train_epoch, args.samples, args.warmup)
        out[shape] = row
        print(shape, json.dumps(row), flush=True)
        del off, plan, A
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
