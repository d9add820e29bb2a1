"""What the reference's regularisation settings cost per replayed epoch (node_classification.py:35-37, :172-193:
`weight_decay` handed to Adam, l1_lambda / l2_lambda added to the loss), at the AM-shaped and the MUTAG-shaped
synthetic graphs, for four settings (weight_decay, l1_lambda, l2_lambda):

  zero      (0, 0, 0)            the headline epoch
  wd        (5e-4, 0, 0)
  l2        (0, 0, 5e-4)
  l1_l2_wd  (5e-4, 1e-5, 5e-4)

Every figure is the median wall time (stream synchronised before and after) of `--reps` replays of a
train.GraphedTrainStep after 5 warm-up replays — the method of tools/early_stop_probe.py.  The script uses nothing but
API that predates the regularised row update, so the same file runs in a checkout of the parent commit:

    (parent checkout)  python tools/weight_reg_probe.py --rows-only --zero-repeats 3 --out parent.json
    (this tree)        python tools/weight_reg_probe.py --parent parent.json

`--parent` puts the parent's rows into the result as the baseline, with the ratio of every row to it and the spread of
the parent's repeated (0, 0, 0) runs.  `prepass_ms` is the difference of the `l2` and `wd` medians of one tree: both
visit all N nodes, `l2` adds the penalty-norm pass (and a few scalar ops).  Writes profiles/weight_reg_probe.json.
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

SETTINGS = (("zero", (0.0, 0.0, 0.0)), ("wd", (5e-4, 0.0, 0.0)), ("l2", (0.0, 0.0, 5e-4)),
            ("l1_l2_wd", (5e-4, 1e-5, 5e-4)))


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
    return dict(N=N, R=R, B=Bn, F=d[0][1], A=plan.as_adjacency_handle(), plan=plan, X=X, model=model,
                idx=torch.from_numpy(idx).cuda(), y=torch.from_numpy(y).cuda())


def _row(s, setting, reps):
    import mrgcn_amd
    from mrgcn_amd.train import ClipAdam, GraphedTrainStep
    wd, l1, l2 = setting
    m = s["model"]()
    opt = ClipAdam(m.parameters(), lr=0.01, max_norm=1.0, weight_decay=wd, capturable=True)
    mrgcn_amd.reset_stats()
    step = GraphedTrainStep(m, lambda: m(s["X"], s["A"]), s["idx"], s["y"], opt, warmup=3, l1_lambda=l1, l2_lambda=l2)
    st = mrgcn_amd.stats()
    out = _timed(step, reps)
    out.update(weight_decay=wd, l1_lambda=l1, l2_lambda=l2, final_loss=float(step()),
               route={k: int(v) for k, v in st.items() if k.startswith("adam.") or k.startswith("weight_I.")})
    del step, opt, m
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weight_reg_probe.json"))
    ap.add_argument("--shapes", nargs="+", default=["am", "mutag"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--zero-repeats", type=int, default=1, help="measure the (0, 0, 0) row this many times")
    ap.add_argument("--rows-only", action="store_true", help="the rows of this tree alone (for the parent checkout)")
    ap.add_argument("--parent", help="JSON written by --rows-only in a checkout of the parent commit")
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps: medians are taken over at least 20 epochs")
    from mrgcn_amd.host import fit_cpu_pool_to_quota
    fit_cpu_pool_to_quota()
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, timing="wall clock, synchronised, replayed "
               "GraphedTrainStep, 5 warm-up replays", shapes={})
    for name in args.shapes:
        s = _setup(name)
        rows = {}
        for key, setting in SETTINGS:
            rows[key] = _row(s, setting, args.reps)
            print(name, key, json.dumps(rows[key]), flush=True)
        again = [_row(s, SETTINGS[0][1], args.reps)["median_ms"] for _ in range(max(args.zero_repeats - 1, 0))]
        zeros = [rows["zero"]["median_ms"]] + again
        table_bytes = s["N"] * s["B"] * s["F"] * 4
        out["shapes"][name] = dict(N=s["N"], R=s["R"], B=s["B"], F=s["F"], table_bytes=table_bytes, rows=rows,
                                   zero_medians_ms=zeros, zero_spread_ms=float(max(zeros) - min(zeros)),
                                   prepass_ms=rows["l2"]["median_ms"] - rows["wd"]["median_ms"],
                                   prepass_byte_estimate_ms=table_bytes / 6e12 * 1e3)
        del s
        torch.cuda.empty_cache()
    if args.parent and not args.rows_only:
        with open(args.parent) as f:
            base = json.load(f)
        out["baseline"] = dict(what="the same script in a checkout of the parent commit, same box", **base)
        for name, sh in out["shapes"].items():
            b = base["shapes"].get(name)
            if b is None:
                continue
            sh["ratio_to_parent"] = {k: sh["rows"][k]["median_ms"] / b["rows"][k]["median_ms"] for k in sh["rows"]}
            sh["parent_zero_spread_ms"] = b["zero_spread_ms"]
            sh["zero_difference_ms"] = sh["rows"]["zero"]["median_ms"] - b["rows"]["zero"]["median_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
