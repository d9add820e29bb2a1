"""What validation and early stopping cost per epoch, at the AM-shaped and the MUTAG-shaped synthetic graphs:

  replayed_train_only       train.GraphedTrainStep (the training step alone)
  replayed_eval_no_improve  train.GraphedTrainEvalStep: step, both evaluations, metrics row, early-stop record whose
                            score never improves (the snapshot launch returns at its flag)
  replayed_eval_improving   the same with every record improving: the snapshot of parameters and optimizer state runs
  host_loop_no_improve      the loop without the feature: a GraphedTrainStep replay, an eager eval() forward,
                            float(loss), the torch-op accuracy, the host EarlyStop (no improvement)
  host_loop_improving       ... with copy.deepcopy of model.state_dict() and optimizer.state_dict() every epoch

Every figure is the median wall time (stream synchronised before and after) of `--reps` epochs after warm-up.  Writes
profiles/early_stop_probe.json.

    python tools/early_stop_probe.py [--out profiles/early_stop_probe.json] [--shapes am mutag]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)), reps=reps)


def _setup(name):
    from mrgcn_amd import synth
    from mrgcn_amd.plan import GraphPlan
    g = synth.make_graph(name, seed=0)
    N, R = g.num_nodes, g.num_relations
    A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([g.rows, g.cols])), torch.from_numpy(g.vals),
                                (N, R * N)).cuda()
    d = synth.layer_dims(name)
    Bn = synth.SHAPES[name]["bases"]
    idx, y = synth.make_labels(name, N, seed=0)
    X = torch.randn((N, d[0][0]), device="cuda", generator=torch.Generator("cuda").manual_seed(1))

    def model():
        from mrgcn_amd.models.rgcn import RGCN
        torch.manual_seed(0)
        return RGCN([(d[0][0], d[0][1], "mrgcn", torch.nn.ReLU()), (d[1][0], d[1][1], "mrgcn", None)], R, N, Bn, 0.0,
                    False, True, False).cuda()
    plan = GraphPlan(A, N, R, operand_row_bytes=model().operand_row_bytes())
    del A
    idx, y = torch.from_numpy(idx).cuda(), torch.from_numpy(y).cuda()
    return dict(N=N, R=R, A=plan.as_adjacency_handle(), plan=plan, X=X, model=model,
                train=(idx[0::2].contiguous(), y[0::2].contiguous()),
                valid=(idx[1::2].contiguous(), y[1::2].contiguous()))


def _fresh(s):
    from mrgcn_amd.train import ClipAdam
    m = s["model"]()
    return m, ClipAdam(m.parameters(), lr=0.01, max_norm=1.0, capturable=True), (lambda: m(s["X"], s["A"]))


def _train_only(s, args):
    from mrgcn_amd.train import GraphedTrainStep
    m, opt, fwd = _fresh(s)
    return _timed(GraphedTrainStep(m, fwd, s["train"][0], s["train"][1], opt, warmup=3), args.reps)


def _replayed_eval(s, args, improving):
    from mrgcn_amd.train import EarlyStop, GraphedTrainEvalStep
    m, opt, fwd = _fresh(s)
    # score + tolerance < best: always with a tolerance of -1e30, never with +1e30 (patience: never runs out)
    cfg = EarlyStop(patience=1 << 30, tolerance=-1e30 if improving else 1e30, delay=0)
    step = GraphedTrainEvalStep(m, fwd, s["train"][0], s["train"][1], opt, valid=s["valid"], early_stop=cfg, warmup=3)
    out = _timed(step, args.reps)
    st = step.early_stop.state.read()
    assert st.stop == 0 and (st.best_record == st.records if improving else st.best_record == 1), \
        (st.records, st.best_record)
    out["snapshot_bytes"] = step.early_stop.snapshot_bytes
    return out


def _host_loop(s, args, improving):
    import copy

    from mrgcn_amd.train import (EarlyStop, GraphedTrainStep, categorical_accuracy, categorical_crossentropy)
    m, opt, fwd = _fresh(s)
    step = GraphedTrainStep(m, fwd, s["train"][0], s["train"][1], opt, warmup=3)
    es = EarlyStop(patience=1 << 30, tolerance=-1e30 if improving else 1e30, delay=0)
    vi, vy = s["valid"]

    class _Free:   # (the first record always copies: keep that one out of the no-improvement row)
        def state_dict(self):
            return {}
    es.record(1.0, _Free(), _Free())

    def epoch():
        train_loss = float(step())
        m.eval()
        with torch.no_grad():
            out = fwd()
            val_loss = float(categorical_crossentropy(out, vi, vy))
            val_acc = float(categorical_accuracy(out, vi, vy)[0])
        m.train()
        es.record(val_loss, m, opt)
        return train_loss, val_loss, val_acc
    out = _timed(epoch, args.reps)
    assert bool(es.best_weights) == improving   # ({}: only the free first record copied anything)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "early_stop_probe.json"))
    ap.add_argument("--shapes", nargs="+", default=["am", "mutag"])
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps: medians are taken over at least 20 epochs")
    from mrgcn_amd.host import fit_cpu_pool_to_quota
    fit_cpu_pool_to_quota()
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, timing="wall clock, synchronised", shapes={})
    for name in args.shapes:
        s = _setup(name)
        rows = {}
        for key, fn in (("replayed_train_only", lambda: _train_only(s, args)),
                        ("replayed_eval_no_improve", lambda: _replayed_eval(s, args, False)),
                        ("replayed_eval_improving", lambda: _replayed_eval(s, args, True)),
                        ("host_loop_no_improve", lambda: _host_loop(s, args, False)),
                        ("host_loop_improving", lambda: _host_loop(s, args, True))):
            rows[key] = fn()
            print(name, key, json.dumps(rows[key]), flush=True)
            torch.cuda.empty_cache()
        out["shapes"][name] = dict(N=s["N"], R=s["R"], labelled_train=int(s["train"][0].numel()),
                                   labelled_valid=int(s["valid"][0].numel()), rows=rows)
        del s
        torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
