"""What node dropout costs: the replayed epoch (train.GraphedTrainStep) at the AM-shaped and the MUTAG-shaped
synthetic graphs with p_dropout = 0 and with p_dropout = 0.2 drawn and applied on the device, and the eager epoch with
the reference's host draw.  Every figure is the median over `--repeats` blocks of the median of `--reps` event-timed
epochs after warm-up; the spread is the range of the block medians.  Writes profiles/node_dropout_probe.json.

    python tools/node_dropout_probe.py [--out profiles/node_dropout_probe.json]
    python tools/node_dropout_probe.py --rows p0 --out parent.json     # only the p = 0 rows: also runs on a tree
                                                                        # without device dropout (the parent's row)
    python tools/node_dropout_probe.py --parent parent.json            # quotes that file as row (a)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P = 0.2


def _timed(fn, reps, repeats, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    meds = []
    for _ in range(repeats):
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        meds.append(float(np.median(ms)))
    return dict(median_ms=float(np.median(meds)), spread_ms=[min(meds), max(meds)])


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

    def model(p):
        from mrgcn_amd.models.rgcn import RGCN
        torch.manual_seed(0)
        return RGCN([(d[0][0], d[0][1], "mrgcn", torch.nn.ReLU()), (d[1][0], d[1][1], "mrgcn", None)], R, N, Bn, p,
                    False, True, False).cuda()
    plan = GraphPlan(A, N, R, operand_row_bytes=model(0.0).operand_row_bytes())
    del A
    return dict(N=N, R=R, A=plan.as_adjacency_handle(), plan=plan, X=X, idx=torch.from_numpy(idx).cuda(),
                y=torch.from_numpy(y).cuda(), model=model)


def _replayed(s, p, args):
    from mrgcn_amd.train import ClipAdam, GraphedTrainStep
    m = s["model"](p)
    if p > 0:
        m.set_node_dropout("device", seed=1)
    opt = ClipAdam(m.parameters(), lr=0.01, max_norm=1.0, capturable=True)
    step = GraphedTrainStep(m, lambda: m(s["X"], s["A"]), s["idx"], s["y"], opt, warmup=3)
    return _timed(step, args.reps, args.repeats)


def _eager_host(s, args):
    from mrgcn_amd.train import ClipAdam, train_step
    m = s["model"](P)
    opt = ClipAdam(m.parameters(), lr=0.01, max_norm=1.0)
    return _timed(lambda: train_step(m, lambda: m(s["X"], s["A"]), s["idx"], s["y"], opt), max(args.reps // 3, 5),
                  args.repeats, warm=3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "node_dropout_probe.json"))
    ap.add_argument("--rows", choices=["all", "p0"], default="all")
    ap.add_argument("--parent", default=None, help="a --rows p0 result of the parent commit, measured on the same box")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    from mrgcn_amd.host import fit_cpu_pool_to_quota
    fit_cpu_pool_to_quota()
    out = dict(device=torch.cuda.get_device_name(0), p_dropout=P, reps=args.reps, repeats=args.repeats, shapes={})
    for name in ("am", "mutag"):
        s = _setup(name)
        rows = {"replayed_p0": _replayed(s, 0.0, args)}
        if args.rows == "all":
            rows["replayed_device"] = _replayed(s, P, args)
            if name == "am":
                rows["eager_host"] = _eager_host(s, args)
            rows["replayed_p0_again"] = _replayed(s, 0.0, args)   # (the same row at the end: drift of the box)
        out["shapes"][name] = dict(N=s["N"], R=s["R"], rows=rows)
        print(name, json.dumps(rows), flush=True)
        del s
        torch.cuda.empty_cache()
    if args.parent:
        with open(args.parent) as f:
            par = json.load(f)
        for name, sh in par["shapes"].items():
            out["shapes"][name]["rows"]["parent_replayed_p0"] = sh["rows"]["replayed_p0"]
    if args.rows == "all":
        for name, sh in out["shapes"].items():
            r = sh["rows"]
            b, c = r["replayed_p0"]["median_ms"], r["replayed_device"]["median_ms"]
            sh["device_minus_p0_ms"], sh["device_over_p0"] = c - b, c / b
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk != "rows"} for k, v in out["shapes"].items()}))


if __name__ == "__main__":
    main()
