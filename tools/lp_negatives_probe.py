"""What keyed, filtered negatives cost at the FB15k-237 shape (synthetic graph of that shape, bench.py's split and
model): the sampler call alone — `NegativeSampler` at 1 and 10 negatives per fact, filtered against every triple of the
graph and unfiltered, next to `DeviceNegativeSampler`'s call — and the replayed full-batch training epoch of `fit`
(`FitEpochs.train_epoch`, one captured hipGraph) with the default sampler and with the keyed one at both rates.  Every
figure is the median of `--reps` synchronised, event-timed calls after `--warm` warm-ups, with their range.  The
default-sampler epoch is measured first and last: the difference is the drift of the box during the run.
Writes profiles/lp_negatives_probe.json.

    python tools/lp_negatives_probe.py [--out profiles/lp_negatives_probe.json]
    python tools/lp_negatives_probe.py --rows default --out parent.json   # only the default sampler's rows: also runs
                                                                          # on a tree without the keyed sampler
    python tools/lp_negatives_probe.py --parent parent.json               # quotes that file's rows as parent_*
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


def _keyed(s, rate, filtered):
    from mrgcn_amd.tasks import link_prediction as lp
    return lp.NegativeSampler(s["train"], s["N"], s["R"], rate=rate, known=s["known"] if filtered else False, seed=1)


def _epoch(s, sampler, args):
    """The replayed training epoch of `fit` on a fresh model; `sampler` None: the default one."""
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.tasks import link_prediction as lp
    from mrgcn_amd.train import ClipAdam
    torch.manual_seed(0)
    model = RGCN([(0, s["H"], "mrgcn", torch.nn.ReLU())], s["R"], s["N"], s["B"], 0.0, True, False, True).cuda()
    opt = ClipAdam(model.parameters(), lr=0.01, weight_decay=0.0, max_norm=1.0, capturable=True)
    plan = s["plan_of"](model)   # noqa: F841  (kept alive with the run, as the bench does)
    keyed = sampler is not None
    if not keyed:   # what `fit` builds when no sampler is given
        sampler = lp.DeviceNegativeSampler(s["train"])
    static = lp.SortedTriples(sampler.facts, s["N"], s["R"])
    # (the evaluating epoch of the capture's warm-up ranks these; the timed training epoch does not read them)
    tparts = lp.FactParts(s["train"][:2000], 0, filtered=False)
    run = lp.FitEpochs(model, lambda: model(None, s["A"]), tparts, None, opt, graphed=True, sampler=sampler,
                       static=static, warmup=3)
    row = _timed(run.train_epoch, args.reps, args.warm)
    row["triples_scored"] = int(sampler.buf.shape[0])
    if keyed:
        row["unresolved_last_epoch"] = sampler.num_unresolved()
    del run, model, opt
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lp_negatives_probe.json"))
    ap.add_argument("--rows", choices=["all", "default"], default="all")
    ap.add_argument("--parent", default=None, help="a --rows default result of the parent commit, from the same box")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    args = ap.parse_args()
    from mrgcn_amd.host import fit_cpu_pool_to_quota
    from mrgcn_amd.tasks import link_prediction as lp
    fit_cpu_pool_to_quota()
    s = _setup()
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warm=args.warm, N=s["N"], R=s["R"],
               train_facts=int(s["train"].shape[0]), known_facts=int(len(s["known"])), sampler_call={}, epoch={})
    calls, epochs = out["sampler_call"], out["epoch"]
    epochs["default"] = _epoch(s, None, args)
    print("epoch default", json.dumps(epochs["default"]), flush=True)
    calls["default"] = _timed(lp.DeviceNegativeSampler(s["train"]), args.reps, args.warm)
    if args.rows == "all":
        for rate in (1, 10):
            for filtered in (True, False):
                smp = _keyed(s, rate, filtered)
                name = f"keyed_rate{rate}_{'filtered' if filtered else 'unfiltered'}"
                calls[name] = _timed(smp, args.reps, args.warm)
                calls[name]["unresolved_last_call"] = smp.num_unresolved()
                del smp
        print("sampler calls", json.dumps(calls), flush=True)
        for rate in (1, 10):
            epochs[f"keyed_rate{rate}_filtered"] = _epoch(s, _keyed(s, rate, True), args)
            print("epoch rate", rate, json.dumps(epochs[f"keyed_rate{rate}_filtered"]), flush=True)
    epochs["default_again"] = _epoch(s, None, args)   # (the same row at the end: drift of the box)
    if args.parent:
        with open(args.parent) as f:
            par = json.load(f)
        for k in ("default", "default_again"):
            epochs["parent_" + k] = par["epoch"][k]
        calls["parent_default"] = par["sampler_call"]["default"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
