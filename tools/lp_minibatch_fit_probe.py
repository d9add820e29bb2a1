#!/usr/bin/env python
"""The mini-batch link-prediction run loop at the FB15k-237 shape of tools/lp_minibatch_probe.py (1 011 masked batches
of 383-761 nodes and 500-999 facts, one featureless mrgcn layer of 200 outputs, 2 bases):
  (a) batch_eval (mrgcn_distmult_batch_eval: three launches) at the smallest, the median and the largest batch against
      the two sequences it replaces, none of them with a host read: mrgcn_distmult_ranks twice + mrgcn_rank_metrics
      twice, and rank_both + rank_metrics twice.  The three are timed alternately, `--reps` calls between two device
      events per sample, the median of `--samples` samples after `--warmup` of them.
  (b) one evaluation pass over all batches: eval_batches against evaluate_batches (wall clock ending in a synchronise).
  (c) a training epoch, an evaluating epoch and an improving evaluating epoch of fit_batches' eager epochs
      (BatchFitEpochs) against the host loop built from train_epoch, evaluate_batches twice, the host EarlyStop and
      its deepcopies.

    python tools/lp_minibatch_fit_probe.py [--out FILE] [--valid-batches 100]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def _median(fn, samples, warmup):
    ts = [_wall(fn) for _ in range(warmup + samples)][warmup:]
    return dict(median_s=float(np.median(ts)), p10_p90_s=[float(np.percentile(ts, 10)), float(np.percentile(ts, 90))])


def _events_us(fns, reps, samples, warmup):
    """{name: median microseconds per call}, the callables alternating sample by sample."""
    out = {k: [] for k in fns}
    for s in range(warmup + samples):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            if s >= warmup:
                out[k].append(1e3 * a.elapsed_time(b) / reps)
    return {k: dict(median_us=float(np.median(v)), p10_p90_us=[float(np.percentile(v, 10)), float(np.percentile(v, 90))])
            for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--valid-batches", type=int, default=100, help="how many of the batches stand for the validation set")
    ap.add_argument("--epoch-samples", type=int, default=20, help="samples of (b) and (c)")
    ap.add_argument("--epoch-warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "lp_minibatch_fit_probe.json"))
    args = ap.parse_args()
    import ctypes as C

    from mrgcn_amd import _lib as L
    from mrgcn_amd import synth
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.plan import plan_of
    from mrgcn_amd.tasks import link_prediction as lp
    from mrgcn_amd.train import ClipAdam, DeviceEarlyStop, EarlyStop

    sg = synth.make_graph("fb15k", seed=0)
    N, R = sg.num_nodes, sg.num_relations
    facts = np.asarray(sg.triples, dtype=np.int64)
    A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([sg.rows, sg.cols])), torch.from_numpy(sg.vals),
                                (N, R * N)).cuda()
    plan = plan_of(A, N, R)
    bs = lp.prepare_batches(lp.mkbatches(None, None, facts, 32, 500, 1, plan=plan), "cuda")
    torch.manual_seed(0)
    model = RGCN([(0, 200, "mrgcn", torch.nn.ReLU())], R, N, 2, 0.0, True, False, True).cuda()
    out = {"device": torch.cuda.get_device_name(0), "batches": len(bs),
           "method": dict(samples=args.samples, warmup=args.warmup, reps_per_sample=args.reps,
                          epoch_samples=args.epoch_samples, epoch_warmup=args.epoch_warmup)}
    lib = L.load()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731

    # ---- (a) one batch's evaluation -----------------------------------------------------------------------------
    order = np.argsort([len(f) for _, f in bs], kind="stable")
    out["batch_eval"] = {}
    for name, i in (("smallest", order[0]), ("median", order[len(order) // 2]), ("largest", order[-1])):
        b, f = bs[int(i)]
        with torch.no_grad():
            E = model(None, b.A).detach()
        Rel = model.relations.detach()
        st = b._mrgcn_lp
        tr, nf, Nn, H = st["facts"], len(f), int(E.shape[0]), int(E.shape[1])
        lists = lp._batch_lists(st, f)
        ws = lp.batch_eval_workspace(Nn, H, nf, "cuda")
        slot = torch.empty(8, device="cuda")
        raw, flt = (torch.empty(2 * nf, dtype=torch.int64, device="cuda") for _ in range(2))
        ws_bytes = int(lib.mrgcn_distmult_ranks_workspace(Nn, H, nf))
        ws2 = torch.empty((ws_bytes + 3) // 4, dtype=torch.int32, device="cuda")

        def fused():
            lp.batch_eval(E, Rel, tr, lists, slot, (raw, flt), ws)

        def ranks_twice():
            for ls, r, o in (([None] * 4, raw, slot[:4]), (lists, flt, slot[4:])):
                L.check(lib.mrgcn_distmult_ranks(p(E), E.stride(0), Nn, p(Rel), Rel.stride(0), H, p(tr), nf, p(ls[0]),
                                                 p(ls[1]), p(ls[2]), p(ls[3]), p(ws2), ws_bytes, p(r), stream()))
                lp.rank_metrics(r, out=o)

        def both():
            a, c = lp.rank_both(tr, E, Rel, lists)
            lp.rank_metrics(a, out=slot[:4])
            lp.rank_metrics(c, out=slot[4:])

        res = _events_us({"batch_eval": fused, "ranks_x2_metrics_x2": ranks_twice, "rank_both_metrics_x2": both},
                         args.reps, args.samples, args.warmup)
        res["shape"] = dict(nodes=Nn, facts=nf, hidden=H)
        out["batch_eval"][name] = res
        print(name, json.dumps(res), flush=True)

    # ---- (b) one evaluation pass over all batches ---------------------------------------------------------------
    slots = torch.empty((len(bs), 8), device="cuda")
    out["eval_pass"] = {
        "eval_batches": _median(lambda: lp.eval_batches(model, bs, slots=slots), args.epoch_samples, args.epoch_warmup),
        "rank_batches": _median(lambda: lp.rank_batches(model, bs), args.epoch_samples, args.epoch_warmup),
        "evaluate_batches": _median(lambda: lp.evaluate_batches(bs, model, filtered=True), args.epoch_samples, args.epoch_warmup)}
    print(json.dumps(out["eval_pass"]), flush=True)

    # ---- (c) the epochs ------------------------------------------------------------------------------------------
    nv = min(args.valid_batches, len(bs) // 2)
    tb, vb = bs[nv:], bs[:nv]
    opt = ClipAdam(list(model.parameters()), lr=0.01, max_norm=1.0, capturable=True)
    opt.init_state()
    stopper = DeviceEarlyStop(model, opt, patience=1 << 20, tolerance=-1.0, delay=0)   # (every record improves)
    plain = lp.BatchFitEpochs(model, tb, vb, opt, None, 8, False)
    improving = lp.BatchFitEpochs(model, tb, vb, opt, stopper, 8, False)
    host_stop = EarlyStop(patience=1 << 20, tolerance=-1.0, delay=0)

    def host_train():
        lp.train_epoch(tb, model, opt)

    def host_eval(stop):
        lp.train_epoch(tb, model, opt)
        lp.evaluate_batches(tb, model, filtered=True)
        mrr, _, _ = lp.evaluate_batches(vb, model, filtered=True)
        if stop is not None:
            stop.record(1.0 - mrr["raw"], model, opt)

    out["epochs"] = dict(
        train_batches=len(tb), valid_batches=len(vb),
        device=dict(train=_median(plain.train_epoch, args.epoch_samples, args.epoch_warmup),
                    evaluating=_median(plain.eval_epoch, args.epoch_samples, args.epoch_warmup),
                    evaluating_improving=_median(improving.eval_epoch, args.epoch_samples, args.epoch_warmup)),
        host=dict(train=_median(host_train, args.epoch_samples, args.epoch_warmup),
                  evaluating=_median(lambda: host_eval(None), args.epoch_samples, args.epoch_warmup),
                  evaluating_improving=_median(lambda: host_eval(host_stop), args.epoch_samples, args.epoch_warmup)))
    print(json.dumps(out["epochs"]), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
