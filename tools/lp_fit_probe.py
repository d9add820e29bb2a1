"""What link prediction's evaluation and early stopping cost inside the epoch, at the FB15k-237-shaped synthetic graph
(14 541 nodes, h = 200; 272 115 training facts, 17 535 validation facts):

  (i)   ranks: mrgcn_distmult_ranks raw, the same filtered (the parent's two calls), and rank_both (one pass), of the
        validation facts and of the training facts, the filter lists built once outside the timed region
  (ii)  an evaluating epoch: FitEpochs.eval_epoch replayed (step, eval() forward, evaluate_facts of both fact sets,
        record_row, snapshot) against the host loop around a replayed training step (eval() forward, two rank calls
        per part, .item() per metric, tolist() of every rank, the host EarlyStop with copy.deepcopy of both
        state_dicts on improvement), with a record that never improves and one that always does
  (iii) a non-evaluating epoch: FitEpochs.train_epoch replayed (the step and the loss-ring record) against
        train.GraphedStep of the same step

Every figure is the median wall time (stream synchronised before and after) of `--reps` calls after 5 warm-ups, on one
box.  Writes profiles/lp_fit_probe.json.

    python tools/lp_fit_probe.py [--out profiles/lp_fit_probe.json] [--mrr-batchsize 5000]
"""
import argparse
import ctypes as C
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


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _ranks_old(lib, E, Rel, tr, lists):
    """mrgcn_distmult_ranks on ready device lists (compute_ranks_fast without its host work)."""
    from mrgcn_amd import _lib
    nf, N, H = tr.shape[0], E.shape[0], E.shape[1]
    ranks = torch.empty(2 * nf, dtype=torch.int64, device=E.device)
    ws_bytes = lib.mrgcn_distmult_ranks_workspace(N, H, nf)
    ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.int32, device=E.device)
    ls = lists if lists is not None else [None] * 4
    _lib.check(lib.mrgcn_distmult_ranks(_ptr(E), E.stride(0), N, _ptr(Rel), Rel.stride(0), H, _ptr(tr), nf, _ptr(ls[0]),
                                        _ptr(ls[1]), _ptr(ls[2]), _ptr(ls[3]), _ptr(ws), ws_bytes, _ptr(ranks),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)), "distmult_ranks")
    return ranks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lp_fit_probe.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--mrr-batchsize", type=int, default=5000)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps: medians are taken over at least 20 calls")
    from mrgcn_amd import _lib, synth
    from mrgcn_amd.host import fit_cpu_pool_to_quota
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.plan import plan_of
    from mrgcn_amd.tasks import link_prediction as lp
    from mrgcn_amd.train import ClipAdam, EarlyStop, GraphedStep, _as_device_stopper
    fit_cpu_pool_to_quota()
    lib = _lib.load()
    sh = synth.SHAPES["fb15k"]
    g = synth.make_graph("fb15k", seed=0)
    N, R, H, B = g.num_nodes, g.num_relations, sh["hidden"], sh["bases"]
    perm = np.random.RandomState(0).permutation(len(g.triples))
    train, valid = g.triples[perm[:272115]], g.triples[perm[272115:272115 + 17535]]
    A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([g.rows, g.cols])), torch.from_numpy(g.vals),
                                (N, R * N)).cuda()
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmups=5, timing="wall clock, synchronised",
               shape=dict(N=N, R=R, H=H, train_facts=len(train), valid_facts=len(valid)),
               mrr_batchsize=args.mrr_batchsize)

    def fresh():
        torch.manual_seed(0)
        model = RGCN([(0, H, "mrgcn", torch.nn.ReLU())], R, N, B, 0.0, True, False, True).cuda()
        opt = ClipAdam(model.parameters(), lr=0.01, weight_decay=0.0, max_norm=1.0, capturable=True)
        plan = plan_of(A, N, R, operand_row_bytes=model.operand_row_bytes())
        return model, opt, plan

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)

    # (i) ranks -------------------------------------------------------------------------------------------------------
    model, opt, plan = fresh()
    model.eval()
    with torch.no_grad():
        E, Rel = model(None, A).clone(), model.relations.detach().clone()
    out["ranks"] = {}
    for name, facts in (("valid", valid), ("train", train)):
        tr = torch.from_numpy(np.ascontiguousarray(facts)).cuda()
        lists = [torch.from_numpy(a).cuda() for a in lp.filter_lists(facts)]
        raw0, flt0 = _ranks_old(lib, E, Rel, tr, None), _ranks_old(lib, E, Rel, tr, lists)
        raw1, flt1 = lp.rank_both(tr, E, Rel, lists)
        assert torch.equal(raw0, raw1) and torch.equal(flt0, flt1)
        rows = dict(facts=len(facts), list_entries=int(lists[1].numel() + lists[3].numel()),
                    raw_call=_timed(lambda: _ranks_old(lib, E, Rel, tr, None), args.reps),
                    filtered_call=_timed(lambda: _ranks_old(lib, E, Rel, tr, lists), args.reps),
                    rank_both=_timed(lambda: lp.rank_both(tr, E, Rel, lists), args.reps))
        rows["rank_both_over_filtered_call"] = rows["rank_both"]["median_ms"] / rows["filtered_call"]["median_ms"]
        rows["rank_both_over_two_calls"] = rows["rank_both"]["median_ms"] / (
            rows["raw_call"]["median_ms"] + rows["filtered_call"]["median_ms"])
        out["ranks"][name] = rows
        print("ranks", name, json.dumps(rows), flush=True)
        save()
    del model, opt, plan
    torch.cuda.empty_cache()

    # (iii) a non-evaluating epoch -------------------------------------------------------------------------------------
    train_dev = torch.from_numpy(np.ascontiguousarray(train)).cuda()
    tparts = lp.FactParts(train, args.mrr_batchsize, True, device="cuda")
    vparts = lp.FactParts(valid, args.mrr_batchsize, True, device="cuda")
    out["parts"] = dict(train=tparts.nparts, valid=vparts.nparts)

    def graphed_step():
        model, opt, plan = fresh()
        sampler = lp.DeviceNegativeSampler(train_dev)
        static = lp.SortedTriples(sampler.facts, N, R)
        step = GraphedStep(lambda: lp.train_step(model, lambda: model(None, A), sampler, opt, static), warmup=3)
        # (what the captured launches read stays alive with the step: the sampler's buffers, the stored orders)
        step.keep = (model, opt, plan, sampler, static)
        return step

    def epochs(improving):
        model, opt, plan = fresh()
        cfg = EarlyStop(patience=1 << 30, tolerance=-1e30 if improving else 1e30, delay=0)
        stopper = _as_device_stopper(cfg, model, opt)
        run = lp.FitEpochs(model, lambda: model(None, A), tparts, vparts, opt, stopper, poll=8, graphed=True, warmup=3)
        run.keep = plan
        return run
    out["train_epoch"] = dict(graphed_step=_timed(graphed_step(), args.reps * 5),
                              fit_train_epoch=_timed(epochs(False).train_epoch, args.reps * 5))
    print("train_epoch", json.dumps(out["train_epoch"]), flush=True)
    save()
    torch.cuda.empty_cache()

    # (ii) an evaluating epoch -----------------------------------------------------------------------------------------
    out["eval_epoch"] = {}
    for improving in (False, True):
        run = epochs(improving)
        key = "improving" if improving else "no_improve"
        out["eval_epoch"]["replayed_" + key] = _timed(run.eval_epoch, args.reps)
        st = run.eval_ctr.read()
        assert st.stop == 0 and (st.best_record == st.records if improving else st.best_record == 1)
        out["eval_epoch"]["replayed_" + key]["snapshot_bytes"] = run.stopper.snapshot_bytes
        print("eval_epoch replayed", key, json.dumps(out["eval_epoch"]["replayed_" + key]), flush=True)
        save()
        del run
        torch.cuda.empty_cache()
    part_lists = {}   # every part's facts and its own lists on the device, as evaluate_batches keeps them per batch
    for parts, facts in ((tparts, train), (vparts, valid)):
        per = []
        for p in range(parts.nparts):
            a, b = int(parts.part_ptr_host[p]), int(parts.part_ptr_host[p + 1])
            ls = [torch.from_numpy(x).cuda() for x in lp.filter_lists(facts[a:b])]
            ls = [x if x.numel() else torch.zeros(1, dtype=x.dtype, device="cuda") for x in ls]
            per.append((parts.facts[a:b].contiguous(), ls))
        part_lists[id(parts)] = per

    def test_model(parts, E, Rel):
        mrr, hits, rankings = {"raw": [], "flt": []}, {"raw": [[], [], []], "flt": [[], [], []]}, []
        for tr, ls in part_lists[id(parts)]:
            for kind, l4 in (("raw", None), ("flt", ls)):
                ranks = _ranks_old(lib, E, Rel, tr, l4)
                mrr[kind].append(torch.mean(1.0 / ranks.float()).item())
                for i, k in enumerate((1, 3, 10)):
                    hits[kind][i].append(float(torch.mean((ranks <= k).float())))
                rankings.append(ranks.tolist())
        return {k: np.mean(v) for k, v in mrr.items()}, {k: [np.mean(h) for h in v] for k, v in hits.items()}

    for improving in (False, True):
        step = graphed_step()
        model, opt = step.keep[0], step.keep[1]
        es = EarlyStop(patience=1 << 30, tolerance=-1e30 if improving else 1e30, delay=0)

        class _Free:   # (the first record always copies: keep that one out of the no-improvement row)
            def state_dict(self):
                return {}
        es.record(1.0, _Free(), _Free())

        def epoch():
            loss = float(step())
            model.eval()
            with torch.no_grad():
                E, Rel = model(None, A), model.relations
                tm, th = test_model(tparts, E, Rel)
                vm, vh = test_model(vparts, E, Rel)
            model.train()
            es.record(1.0 - vm["raw"], model, opt)
            return loss, tm, th, vm, vh
        key = "host_loop_" + ("improving" if improving else "no_improve")
        out["eval_epoch"][key] = _timed(epoch, args.reps)
        assert bool(es.best_weights) == improving   # ({}: only the free first record copied anything)
        print("eval_epoch", key, json.dumps(out["eval_epoch"][key]), flush=True)
        save()
        del step, model, opt
        torch.cuda.empty_cache()
    save()


if __name__ == "__main__":
    main()
