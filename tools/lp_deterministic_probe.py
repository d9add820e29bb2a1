"""Link-prediction training at the FB15k-237 shape with torch.use_deterministic_algorithms off and on (and, on, with
torch.utils.deterministic.fill_uninitialized_memory True / False): the replayed full-batch epoch (bench.py --workload
fb15k's step: DeviceNegativeSampler, SortedTriples, ClipAdam(capturable) in a GraphedStep), the mini-batch step median
and one mini-batch epoch (mkbatches(..., 32, 500, 1, plan=...), RowSparseAdam).  Medians of event-timed repeats after
warm-up.  Writes profiles/lp_deterministic_probe.json.

    python tools/lp_deterministic_probe.py [--out profiles/lp_deterministic_probe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn
import torch.utils.deterministic as tud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _elapsed(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def fullbatch(g, A, N, R):
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.plan import plan_of
    from mrgcn_amd.tasks import link_prediction as lp
    from mrgcn_amd.train import ClipAdam, GraphedStep
    torch.manual_seed(0)
    model = RGCN([(0, 200, "mrgcn", nn.ReLU())], R, N, 2, 0.0, True, False, True).cuda()
    opt = ClipAdam(model.parameters(), lr=0.01, weight_decay=0.0, max_norm=1.0, capturable=True)
    plan = plan_of(A, N, R, operand_row_bytes=model.operand_row_bytes())
    rng = np.random.RandomState(0)
    perm = rng.permutation(len(g.triples))
    train = torch.from_numpy(g.triples[perm[:int(272115 / 310116 * len(g.triples))]]).cuda()
    sampler = lp.DeviceNegativeSampler(train)
    static = lp.SortedTriples(sampler.facts, N, R)

    def step():
        t, Y = sampler()
        emb = model(None, A)
        loss = lp.binary_crossentropy(lp.score_distmult_bc(t, emb, model.relations, static=static), Y)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss.detach()
    graphed = GraphedStep(step, warmup=3)
    _elapsed(graphed, 5)
    ms = _elapsed(graphed, 30)
    del plan
    return float(np.median(ms))


def minibatch(bs, N, R):
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.optim import RowSparseAdam
    from mrgcn_amd.tasks import link_prediction as lp
    torch.manual_seed(0)
    model = RGCN([(0, 200, "mrgcn", nn.ReLU())], R, N, 2, 0.0, True, False, True).cuda()
    opt = RowSparseAdam(model.parameters(), lr=0.01)
    for b, f in bs[:20]:
        lp.train_batch_step(model, b, f, opt)
    torch.cuda.synchronize()
    it = iter(bs * 2)
    steps = _elapsed(lambda: lp.train_batch_step(model, *next(it), opt), 200)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lp.train_epoch(bs, model, opt)
    torch.cuda.synchronize()
    return float(np.median(steps)), time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lp_deterministic_probe.json"))
    args = ap.parse_args()
    from mrgcn_amd import synth
    from mrgcn_amd.plan import plan_of
    from mrgcn_amd.tasks import link_prediction as lp
    g = synth.make_graph("fb15k", seed=0)
    N, R = g.num_nodes, g.num_relations
    A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([g.rows, g.cols])), torch.from_numpy(g.vals),
                                (N, R * N)).cuda()
    plan = plan_of(A, N, R)
    bs = lp.prepare_batches(lp.mkbatches(None, None, np.asarray(g.triples, np.int64), 32, 500, 1, plan=plan), "cuda")
    rows = {}
    for name, det, fill in (("flag_off", False, True), ("flag_on_fill", True, True), ("flag_on_nofill", True, False)):
        torch.use_deterministic_algorithms(det)
        tud.fill_uninitialized_memory = fill
        try:
            fb = fullbatch(g, A, N, R)
            step, epoch = minibatch(bs, N, R)
        finally:
            torch.use_deterministic_algorithms(False)
            tud.fill_uninitialized_memory = True
        rows[name] = dict(fullbatch_replayed_epoch_ms=fb, minibatch_step_median_ms=step, minibatch_epoch_s=epoch)
        print(name, rows[name], flush=True)
    off = rows["flag_off"]
    out = dict(shape="fb15k (synth, scale 1)", batches=len(bs), device=torch.cuda.get_device_name(0), rows=rows,
               ratio_on_nofill={k: rows["flag_on_nofill"][k] / off[k] for k in off},
               ratio_on_fill={k: rows["flag_on_fill"][k] / off[k] for k in off})
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out["ratio_on_nofill"]), json.dumps(out["ratio_on_fill"]))


if __name__ == "__main__":
    main()
