"""What the grouped decoder costs next to the flat one at the FB15k-237 shape (synthetic graph of that shape, bench.py's
split and model; `NegativeSampler` filtered against all triples of the graph) at 1 and 10 negatives per fact:

  epoch      the replayed full-batch training epoch of `fit` (`FitEpochs.train_epoch`, one captured hipGraph) with
             decoder="triples" and decoder="grouped"; grouped also with pos_weight = rate and with the softmax loss
  forward    scores + loss alone on fixed embeddings (eager calls)
  backward   the backward of that loss alone, on the same embeddings
  batch_step the median mini-batch's `train_batch_step` (batches of mkbatches(32, 500)), both decoders

Every figure is the median of `--reps` synchronised, event-timed calls after `--warm` warm-ups, with their range.  The
triples epoch at rate 10 is measured first and last: the difference is the drift of the box during the run.
Writes profiles/lp_grouped_probe.json.

    python tools/lp_grouped_probe.py [--out profiles/lp_grouped_probe.json]
    python tools/lp_grouped_probe.py --rows triples --out parent.json   # only the flat decoder's rows: also runs on a
                                                                        # tree without the grouped decoder
    python tools/lp_grouped_probe.py --parent parent.json               # quotes that file's rows under "parent"
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
    """bench.py's link-prediction workload: the graph, its training split, the adjacency with its plan."""
    from mrgcn_amd import synth
    from mrgcn_amd.plan import plan_of
    sh = synth.SHAPES["fb15k"]
    g = synth.make_graph("fb15k", seed=seed)
    N, R = g.num_nodes, g.num_relations
    perm = np.random.RandomState(seed).permutation(len(g.triples))
    ntrain = int(272115 / 310116 * len(g.triples))
    train = torch.from_numpy(np.asarray(g.triples[perm[:ntrain]], dtype=np.int64)).cuda()
    A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([g.rows, g.cols])), torch.from_numpy(g.vals),
                                (N, R * N)).cuda()
    return dict(N=N, R=R, H=sh["hidden"], B=sh["bases"], A=A, train=train, known=np.asarray(g.triples, dtype=np.int64),
                plan_of=lambda model: plan_of(A, N, R, operand_row_bytes=model.operand_row_bytes()))


def _model(s):
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.train import ClipAdam
    torch.manual_seed(0)
    model = RGCN([(0, s["H"], "mrgcn", torch.nn.ReLU())], s["R"], s["N"], s["B"], 0.0, True, False, True).cuda()
    opt = ClipAdam(model.parameters(), lr=0.01, weight_decay=0.0, max_norm=1.0, capturable=True)
    return model, opt


def _sampler(s, rate):
    from mrgcn_amd.tasks import link_prediction as lp
    return lp.NegativeSampler(s["train"], s["N"], s["R"], rate=rate, known=s["known"], seed=1)


def _epoch(s, rate, args, **decoder):
    """The replayed training epoch of `fit` on a fresh model (no decoder keyword: the flat decoder, on any tree)."""
    from mrgcn_amd.tasks import link_prediction as lp
    model, opt = _model(s)
    plan = s["plan_of"](model)   # noqa: F841  (kept alive with the run, as the bench does)
    sampler = _sampler(s, rate)
    static = lp.SortedTriples(sampler.facts, s["N"], s["R"])
    # (the evaluating epoch of the capture's warm-up ranks these; the timed training epoch does not read them)
    tparts = lp.FactParts(s["train"][:2000], 0, filtered=False)
    run = lp.FitEpochs(model, lambda: model(None, s["A"]), tparts, None, opt, graphed=True, sampler=sampler,
                       static=static, warmup=3, **decoder)
    row = _timed(run.train_epoch, args.reps, args.warm)
    row["triples_scored"] = int(sampler.buf.shape[0])
    del run, model, opt, static, sampler
    torch.cuda.empty_cache()
    return row


def _decoder_alone(s, rate, args, grouped):
    """Scores + loss, and the backward of that loss, on the embeddings of one forward of a fresh model."""
    from mrgcn_amd.tasks import link_prediction as lp
    model, _ = _model(s)
    plan = s["plan_of"](model)   # noqa: F841
    with torch.no_grad():
        E = model(None, s["A"]).detach().clone()
    E.requires_grad_(True)
    Rel = lp._relations(model).detach().clone().requires_grad_(True)
    sampler = _sampler(s, rate)
    static = lp.SortedTriples(sampler.facts, s["N"], s["R"])
    t, y = sampler()
    if grouped:
        def fwd():
            return lp.group_loss(t, E, Rel, sampler.n, rate, static=static)
    else:
        def fwd():
            return lp.binary_crossentropy(lp.score_distmult_bc(t, E, Rel, static=static), y)
    out = dict(forward=_timed(fwd, args.reps, args.warm))
    loss = fwd()
    out["backward"] = _timed(lambda: torch.autograd.grad(loss, [E, Rel], retain_graph=True), args.reps, args.warm)
    del model, static, sampler, loss
    torch.cuda.empty_cache()
    return out


def _batch_steps(s, args, decoders):
    """The median batch's `train_batch_step` at both rates: keyed negatives over the batch's nodes, each decoder."""
    from mrgcn_amd.tasks import link_prediction as lp
    model, opt = _model(s)
    plan = s["plan_of"](model)
    bs = lp.prepare_batches(lp.mkbatches(None, None, s["known"], 32, 500, 1, plan=plan), "cuda")
    order = np.argsort([len(f) for _, f in bs], kind="stable")
    i = int(order[len(order) // 2])
    mb, mf = bs[i]
    model.train()
    out = dict(batches=len(bs), shape=dict(nodes=int(len(mb.node_index)), facts=int(len(mf))))
    for rate in (1, 10):
        smp = lp.batch_negative_samplers(s["N"], s["R"], rate=rate, known=s["known"], seed=1)(i, mb, mf)
        for name in decoders:
            kw = {} if name == "triples" else dict(decoder="grouped")
            out[f"{name}_rate{rate}"] = _timed(lambda: lp.train_batch_step(model, mb, mf, opt, sampler=smp, **kw),
                                               args.reps, args.warm)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lp_grouped_probe.json"))
    ap.add_argument("--rows", choices=["all", "triples"], default="all")
    ap.add_argument("--parent", default=None, help="a --rows triples result of the parent commit, from the same box")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    args = ap.parse_args()
    from mrgcn_amd.host import fit_cpu_pool_to_quota
    fit_cpu_pool_to_quota()
    s = _setup()
    every = args.rows == "all"
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warm=args.warm, N=s["N"], R=s["R"], H=s["H"],
               train_facts=int(s["train"].shape[0]), known_facts=int(len(s["known"])), epoch={}, decoder_alone={})
    epochs, alone = out["epoch"], out["decoder_alone"]

    def show(name, row):
        print(name, json.dumps(row), flush=True)
    epochs["triples_rate10"] = _epoch(s, 10, args)
    show("epoch triples_rate10", epochs["triples_rate10"])
    epochs["triples_rate1"] = _epoch(s, 1, args)
    show("epoch triples_rate1", epochs["triples_rate1"])
    if every:
        for rate in (1, 10):
            epochs[f"grouped_rate{rate}"] = _epoch(s, rate, args, decoder="grouped")
            show(f"epoch grouped_rate{rate}", epochs[f"grouped_rate{rate}"])
            epochs[f"grouped_rate{rate}_pos_weight"] = _epoch(s, rate, args, decoder="grouped", pos_weight=float(rate))
            epochs[f"grouped_rate{rate}_softmax"] = _epoch(s, rate, args, decoder="grouped", loss="softmax")
            show(f"epoch grouped_rate{rate}_softmax", epochs[f"grouped_rate{rate}_softmax"])
    for rate in (1, 10):
        alone[f"triples_rate{rate}"] = _decoder_alone(s, rate, args, False)
        show(f"alone triples_rate{rate}", alone[f"triples_rate{rate}"])
        if every:
            alone[f"grouped_rate{rate}"] = _decoder_alone(s, rate, args, True)
            show(f"alone grouped_rate{rate}", alone[f"grouped_rate{rate}"])
    out["batch_step"] = _batch_steps(s, args, ("triples", "grouped") if every else ("triples",))
    show("batch_step", out["batch_step"])
    epochs["triples_rate10_again"] = _epoch(s, 10, args)   # (the same row at the end: drift of the box)
    show("epoch triples_rate10_again", epochs["triples_rate10_again"])
    if args.parent:
        with open(args.parent) as f:
            par = json.load(f)
        out["parent"] = dict(epoch=par["epoch"], decoder_alone=par["decoder_alone"], batch_step=par["batch_step"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
