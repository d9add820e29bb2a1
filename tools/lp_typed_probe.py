"""What type-constrained link prediction costs next to the untyped paths at the shape `bench.py --workload fb15k` builds
(synthetic graph of the FB15k-237 shape, the bench's split and model), with `TypedCandidates.from_facts` over ALL
triples of the graph:

  rank      `rank_typed` over the validation facts against `rank_both` over the same facts (in parts of 100, as
            the other link-prediction probes cut them), and the number of candidate scores each path computes
  sampler   one call of the typed `NegativeSampler` against the keyed untyped one, at rate 1 and rate 10
  topk      typed `predict_topk` against untyped: 500 queries, k = 10 (the typed call with its host grouping, and with
            a `TypedQueries` built beforehand)
  epoch     the replayed full-batch training epoch of `fit` (`FitEpochs.train_epoch`, one captured hipGraph) with the
            typed sampler against the keyed untyped sampler, rate 1

Every figure is the median of `--reps` synchronised, event-timed calls after `--warm` warm-ups, with their range.
Typed and untyped rows alternate in the same run, and every UNTYPED row is measured again at the end: the difference
between the two is the spread between like rows on this box, and the untyped rows are what a checkout of the parent
commit measures with the same calls.  "ratio" is the typed median over the untyped row's first median.
Writes profiles/lp_typed_probe.json.

    python tools/lp_typed_probe.py [--out profiles/lp_typed_probe.json] [--untyped-only]

`--untyped-only` measures the untyped rows alone, with calls a checkout without the typed paths has too: copied into
the parent commit's tree and run on the same box, it gives the figures the untyped rows are compared with.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn, reps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median_ms=float(np.median(ms)), range_ms=[float(min(ms)), float(max(ms))])


def _setup(seed=0):
    """bench.py's link-prediction workload: the graph, its training and validation-sized splits, the adjacency."""
    from mrgcn_amd import synth
    from mrgcn_amd.plan import plan_of
    sh = synth.SHAPES["fb15k"]
    g = synth.make_graph("fb15k", seed=seed)
    N, R = g.num_nodes, g.num_relations
    perm = np.random.RandomState(seed).permutation(len(g.triples))
    ntrain = int(272115 / 310116 * len(g.triples))
    nvalid = int(17535 / 310116 * len(g.triples))
    tr = np.asarray(g.triples, dtype=np.int64)
    A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([g.rows, g.cols])), torch.from_numpy(g.vals),
                                (N, R * N)).cuda()
    return dict(N=N, R=R, H=sh["hidden"], B=sh["bases"], A=A, all=tr, train=tr[perm[:ntrain]],
                valid=tr[perm[ntrain:ntrain + nvalid]],
                plan_of=lambda model: plan_of(A, N, R, operand_row_bytes=model.operand_row_bytes()))


def _model(s):
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.train import ClipAdam
    torch.manual_seed(0)
    model = RGCN([(0, s["H"], "mrgcn", torch.nn.ReLU())], s["R"], s["N"], s["B"], 0.0, True, False, True).cuda()
    opt = ClipAdam(model.parameters(), lr=0.01, weight_decay=0.0, max_norm=1.0, capturable=True)
    return model, opt


def _epoch(s, types, args):
    """The replayed training epoch of `fit` on a fresh model, keyed negatives at rate 1; `types`: None = untyped."""
    from mrgcn_amd.tasks import link_prediction as lp
    model, opt = _model(s)
    plan = s["plan_of"](model)   # noqa: F841  (kept alive with the run, as the bench does)
    kw = {} if types is None else dict(candidates=types)
    smp = lp.NegativeSampler(s["train"], s["N"], s["R"], rate=1, seed=1, **kw)
    tparts = lp.FactParts(s["train"][:2000], 0, filtered=False, device="cuda")
    run = lp.FitEpochs(model, lambda: model(None, s["A"]), tparts, None, opt, graphed=True, warmup=3, sampler=smp,
                       static=lp.SortedTriples(smp.facts, s["N"], s["R"]))
    row = _timed(run.train_epoch, args.reps, args.warm)
    row["unresolved_last_epoch"] = smp.num_unresolved()
    del run, model, opt, smp
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lp_typed_probe.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--untyped-only", action="store_true")
    args = ap.parse_args()
    from mrgcn_amd.host import fit_cpu_pool_to_quota
    from mrgcn_amd.tasks import link_prediction as lp
    fit_cpu_pool_to_quota()
    s = _setup()
    N, R = s["N"], s["R"]
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warm=args.warm, N=N, R=R, H=s["H"],
               train_facts=int(len(s["train"])), valid_facts=int(len(s["valid"])), rows={})
    rows = out["rows"]
    types = None
    if not args.untyped_only:
        types = lp.TypedCandidates.from_facts(s["all"], N, R, device="cuda")
        lens = types.lengths_host
        out["lists"] = dict(total=int(lens.sum()), longest=int(lens.max()), median=float(np.median(lens)),
                            mean=float(lens.mean()), empty=int((lens == 0).sum()))

    def show(name, row):
        rows[name] = row
        print(name, json.dumps(row), flush=True)

    model, _ = _model(s)
    plan = s["plan_of"](model)   # noqa: F841
    with torch.no_grad():
        E = model(None, s["A"]).detach().clone()
    Rel = lp._relations(model).detach().clone()
    del model

    # ---- ranks: the same facts; rank_both in parts of 100 (a call scores at most num_nodes facts of a part, and the
    # other LP probes cut the same way), rank_typed over all of them at once
    vparts = lp.FactParts(s["valid"], 100, device="cuda")
    nv = len(s["valid"])
    rng = np.random.default_rng(0)
    q_host = np.stack([rng.integers(0, N, 500), rng.integers(0, R, 500)], 1)
    q = torch.from_numpy(q_host).cuda()
    samplers = {("untyped", rate): lp.NegativeSampler(s["train"], N, R, rate=rate, seed=1) for rate in (1, 10)}
    untyped = {
        "rank.untyped": lambda: _timed(lambda: lp.rank_both(vparts, E, Rel), args.reps, args.warm),
        "sampler.untyped.rate1": lambda: _timed(samplers["untyped", 1], args.reps, args.warm),
        "sampler.untyped.rate10": lambda: _timed(samplers["untyped", 10], args.reps, args.warm),
        "topk.untyped": lambda: _timed(lambda: lp.predict_topk(q, E, Rel, 10), args.reps, args.warm),
        "epoch.untyped": lambda: _epoch(s, None, args)}
    if args.untyped_only:
        for un, fu in untyped.items():
            show(un, fu())
        for un, fu in untyped.items():
            show(un + "_again", fu())
        out["spread"] = {un: rows[un + "_again"]["median_ms"] / rows[un]["median_ms"] for un in untyped}
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
        print(json.dumps(out))
        return
    tfacts = lp.TypedFacts(s["valid"], types, device="cuda")
    out["rank_scores"] = dict(untyped=2 * nv * N, typed=tfacts.scores_computed, fact_tiles=tfacts.ntiles,
                              untyped_fact_tiles=(nv + 7) // 8, tile_fill=tfacts.tile_fill, blocks=tfacts.nwork,
                              untyped_blocks=2 * ((nv + 7) // 8) * ((N + 255) // 256))
    raw_u, flt_u = lp.rank_both(vparts, E, Rel)
    raw_t, flt_t = lp.rank_typed(tfacts, E, Rel)
    out["rank_check"] = dict(raw_typed_le_untyped=bool((raw_t <= raw_u).all()),
                             mrr_raw_untyped=float((1.0 / raw_u.double()).mean()),
                             mrr_raw_typed=float((1.0 / raw_t.double()).mean()),
                             mrr_flt_untyped=float((1.0 / flt_u.double()).mean()),
                             mrr_flt_typed=float((1.0 / flt_t.double()).mean()))

    # ---- top-k
    tq = lp.TypedQueries(q, types, side="tail")
    out["topk_scores"] = dict(untyped=500 * N, typed=tq.scores_computed, blocks=tq.nwork,
                              untyped_blocks=((500 + 7) // 8) * ((N + 255) // 256))

    for rate in (1, 10):
        samplers["typed", rate] = lp.NegativeSampler(s["train"], N, R, rate=rate, candidates=types, seed=1)
    typed = {
        "rank.typed": lambda: _timed(lambda: lp.rank_typed(tfacts, E, Rel), args.reps, args.warm),
        "sampler.typed.rate1": lambda: _timed(samplers["typed", 1], args.reps, args.warm),
        "sampler.typed.rate10": lambda: _timed(samplers["typed", 10], args.reps, args.warm),
        "topk.typed": lambda: _timed(lambda: lp.predict_topk(q, E, Rel, 10, candidates=types), args.reps, args.warm),
        "epoch.typed": lambda: _epoch(s, types, args)}
    for (un, fu), (tn, ft) in zip(untyped.items(), typed.items()):
        show(un, fu())
        show(tn, ft())
    show("topk.typed_prepared", _timed(lambda: lp.predict_topk(tq, E, Rel, 10), args.reps, args.warm))
    for rate in (1, 10):
        rows[f"sampler.typed.rate{rate}"]["unresolved"] = samplers["typed", rate].num_unresolved()
        rows[f"sampler.untyped.rate{rate}"]["unresolved"] = samplers["untyped", rate].num_unresolved()
    for un, fu in untyped.items():      # (the same rows at the end: the spread between like rows)
        show(un + "_again", fu())
    show("epoch.typed_again", _epoch(s, types, args))
    pairs = {"rank": ("rank.typed", "rank.untyped"), "sampler.rate1": ("sampler.typed.rate1", "sampler.untyped.rate1"),
             "sampler.rate10": ("sampler.typed.rate10", "sampler.untyped.rate10"),
             "topk": ("topk.typed", "topk.untyped"), "topk_prepared": ("topk.typed_prepared", "topk.untyped"),
             "epoch": ("epoch.typed", "epoch.untyped"), "epoch_again": ("epoch.typed_again", "epoch.untyped_again")}
    out["ratio"] = {n: rows[t]["median_ms"] / rows[u]["median_ms"] for n, (t, u) in pairs.items()}
    out["spread"] = {un: rows[un + "_again"]["median_ms"] / rows[un]["median_ms"] for un in untyped}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
