"""What the ComplEx scorer costs next to DistMult at the shape `bench.py --workload fb15k` builds (synthetic graph of the
FB15k-237 shape, the bench's split and model, the default 20 % in-batch negatives):

  forward    flat scores + BCE on fixed embeddings (eager calls)
  backward   the backward of that loss alone, on the same embeddings — DistMult's default route (atomic flushes, the
             negatives through the counting sort), DistMult's deterministic route (under torch's flag) and ComplEx's one
             fixed-order route (stable radix sort of the negatives): the rows DESIGN's choice of ONE ComplEx backward
             rests on
  rank_both  raw and filtered ranks of the validation-sized fact set in parts of 100
  topk       `predict_topk` of 500 queries at k = 10
  epoch      the replayed full-batch training epoch of `fit` (`FitEpochs.train_epoch`, one captured hipGraph)

Every figure is the median of `--reps` synchronised, event-timed calls after `--warm` warm-ups, with their range.
DistMult and ComplEx alternate in the same run, and every DistMult row is measured again at the end: the difference
between the two is the spread between like rows on this box.  "ratio" is ComplEx's median over DistMult's first one.
Writes profiles/lp_complex_probe.json.

    python tools/lp_complex_probe.py [--out profiles/lp_complex_probe.json]
"""
import argparse
import json
import os
import sys
from contextlib import contextmanager

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


@contextmanager
def _deterministic(on):
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(on)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev)


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
    return dict(N=N, R=R, H=sh["hidden"], B=sh["bases"], A=A, train=torch.from_numpy(tr[perm[:ntrain]]).cuda(),
                valid=tr[perm[ntrain:ntrain + nvalid]],
                plan_of=lambda model: plan_of(A, N, R, operand_row_bytes=model.operand_row_bytes()))


def _model(s):
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.train import ClipAdam
    torch.manual_seed(0)
    model = RGCN([(0, s["H"], "mrgcn", torch.nn.ReLU())], s["R"], s["N"], s["B"], 0.0, True, False, True).cuda()
    opt = ClipAdam(model.parameters(), lr=0.01, weight_decay=0.0, max_norm=1.0, capturable=True)
    return model, opt


class _Decoder:
    """Fixed embeddings of one forward, one draw of the default sampler, the facts' stored orders."""

    def __init__(self, s):
        from mrgcn_amd.tasks import link_prediction as lp
        model, _ = _model(s)
        plan = s["plan_of"](model)   # noqa: F841
        with torch.no_grad():
            self.E = model(None, s["A"]).detach().clone().requires_grad_(True)
        self.Rel = lp._relations(model).detach().clone().requires_grad_(True)
        sampler = lp.DeviceNegativeSampler(s["train"])
        self.static = lp.SortedTriples(sampler.facts, s["N"], s["R"])
        self.t, self.y = sampler()
        self.sampler = sampler

    def loss(self, scorer):
        from mrgcn_amd.tasks import link_prediction as lp
        score = lp.score_complex_bc if scorer == "complex" else lp.score_distmult_bc
        return lp.binary_crossentropy(score(self.t, self.E, self.Rel, static=self.static), self.y)

    def forward(self, scorer, args):
        return _timed(lambda: self.loss(scorer), args.reps, args.warm)

    def backward(self, scorer, args, det=False):
        with _deterministic(det):
            loss = self.loss(scorer)
            return _timed(lambda: torch.autograd.grad(loss, [self.E, self.Rel], retain_graph=True), args.reps,
                          args.warm)


def _epoch(s, scorer, args):
    """The replayed training epoch of `fit` on a fresh model."""
    from mrgcn_amd.tasks import link_prediction as lp
    model, opt = _model(s)
    plan = s["plan_of"](model)   # noqa: F841  (kept alive with the run, as the bench does)
    # (the evaluating epoch of the capture's warm-up ranks these; the timed training epoch does not read them)
    tparts = lp.FactParts(s["train"][:2000], 0, filtered=False)
    run = lp.FitEpochs(model, lambda: model(None, s["A"]), tparts, None, opt, graphed=True, warmup=3, scorer=scorer)
    row = _timed(run.train_epoch, args.reps, args.warm)
    del run, model, opt
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lp_complex_probe.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    args = ap.parse_args()
    from mrgcn_amd.host import fit_cpu_pool_to_quota
    from mrgcn_amd.tasks import link_prediction as lp
    fit_cpu_pool_to_quota()
    s = _setup()
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warm=args.warm, N=s["N"], R=s["R"], H=s["H"],
               train_facts=int(s["train"].shape[0]), valid_facts=int(len(s["valid"])), rows={})
    rows = out["rows"]

    def show(name, row):
        rows[name] = row
        print(name, json.dumps(row), flush=True)

    d = _Decoder(s)
    out["triples_scored"] = int(d.t.shape[0])
    vparts = lp.FactParts(s["valid"], 100, device="cuda")
    E, Rel = d.E.detach(), d.Rel.detach()
    rng = np.random.default_rng(0)
    q = torch.from_numpy(np.stack([rng.integers(0, s["N"], 500), rng.integers(0, s["R"], 500)], 1)).cuda()
    measures = dict(
        forward=lambda sc: d.forward(sc, args),
        backward=lambda sc: d.backward(sc, args),
        rank_both=lambda sc: _timed(lambda: lp.rank_both(vparts, E, Rel, scorer=sc), args.reps, args.warm),
        topk=lambda sc: _timed(lambda: lp.predict_topk(q, E, Rel, 10, scorer=sc), args.reps, args.warm),
        epoch=lambda sc: _epoch(s, sc, args))
    for name, fn in measures.items():
        for sc in ("distmult", "complex"):
            show(f"{name}.{sc}", fn(sc))
    show("backward.distmult_deterministic", d.backward("distmult", args, det=True))
    show("backward.complex_deterministic", d.backward("complex", args, det=True))
    for name, fn in measures.items():   # (the same rows at the end: the spread between like rows)
        show(f"{name}.distmult_again", fn("distmult"))
    out["ratio"] = {n: rows[f"{n}.complex"]["median_ms"] / rows[f"{n}.distmult"]["median_ms"] for n in measures}
    out["spread"] = {n: rows[f"{n}.distmult_again"]["median_ms"] / rows[f"{n}.distmult"]["median_ms"] for n in measures}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
