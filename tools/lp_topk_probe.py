#!/usr/bin/env python
"""Top-k candidate completion at the FB15k-237 decoder shape (14 541 nodes, 2 * 237 + 1 relation rows, h = 200): 500
tail queries, k in {1, 10, 100}, with and without a `known` list of the 500 facts.  Three things timed in this process
on this device, each the median of event-timed launches after warm-up:
  (a) predict_topk (queries and lists resident on the device; `a_host_ms`: numpy queries and facts, lists built per call),
  (b) the route without it: torch.topk((E[s] * Rel[p]) @ E.T, k) — the [queries, nodes] matrix materialised
      (with `known`: the listed entries set to -inf first),
  (c) compute_ranks_fast on the same 500 facts (both directions: twice (a)'s scoring work; numpy facts, as its API takes).
Writes profiles/lp_topk_probe.json.

    python tools/lp_topk_probe.py [--out profiles/lp_topk_probe.json] [--reps 30]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median_ms(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lp_topk_probe.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--nodes", type=int, default=14541)
    ap.add_argument("--rels", type=int, default=237)
    ap.add_argument("--hidden", type=int, default=200)
    ap.add_argument("--queries", type=int, default=500)
    args = ap.parse_args()
    from mrgcn_amd.tasks import link_prediction as lp
    N, P, H, nq = args.nodes, args.rels, args.hidden, args.queries
    gen = torch.Generator(device="cuda").manual_seed(0)
    E = torch.relu(torch.randn((N, H), device="cuda", generator=gen))
    Rel = torch.randn((2 * P + 1, H), device="cuda", generator=gen)
    rng = np.random.default_rng(0)
    facts = np.stack([rng.integers(0, N, nq), rng.integers(0, P, nq), rng.integers(0, N, nq)], 1).astype(np.int64)
    queries = np.ascontiguousarray(facts[:, :2])
    qd = torch.from_numpy(queries).cuda()
    ptr, idx = (torch.from_numpy(a).cuda() for a in lp.known_lists(queries, facts, "tail"))
    # (b)'s mask: the (query, node) pairs of the lists
    rows = torch.repeat_interleave(torch.arange(nq, device="cuda"), ptr[1:] - ptr[:-1])
    cols = idx.long()

    def torch_route(k, filtered):
        sc = (E[qd[:, 0]] * Rel[qd[:, 1]]) @ E.T
        if filtered:
            sc[rows, cols] = float("-inf")
        return torch.topk(sc, k)

    rows_out = {}
    for filtered in (False, True):
        c = _median_ms(lambda: lp.compute_ranks_fast(facts, E, Rel, filtered=filtered), args.reps)
        for k in (1, 10, 100):
            known_dev = (ptr, idx) if filtered else None
            a = _median_ms(lambda: lp.predict_topk(qd, E, Rel, k, known=known_dev), args.reps)
            ah = _median_ms(lambda: lp.predict_topk(queries, E, Rel, k, known=facts if filtered else None), args.reps)
            b = _median_ms(lambda: torch_route(k, filtered), args.reps)
            # the two routes name the same candidates wherever scores differ by more than rounding
            ia, ib = lp.predict_topk(qd, E, Rel, k, known=known_dev)[0], torch_route(k, filtered)[1]
            rows_out[f"k{k}_{'known' if filtered else 'raw'}"] = dict(
                k=k, known=filtered, a_predict_topk_ms=a[0], a_min_max_ms=a[1:], a_host_inputs_ms=ah[0],
                b_torch_topk_ms=b[0], b_min_max_ms=b[1:], c_compute_ranks_fast_ms=c[0], c_min_max_ms=c[1:],
                a_over_c=a[0] / c[0], same_first_candidate=float((ia[:, 0] == ib[:, 0]).float().mean()))
            print(k, filtered, rows_out[f"k{k}_{'known' if filtered else 'raw'}"], flush=True)
    out = dict(shape=dict(nodes=N, relation_rows=2 * P + 1, hidden=H, queries=nq, side="tail"), reps=args.reps,
               timing="median of device-event timed calls after 5 warm-up calls, one process",
               device=torch.cuda.get_device_name(0), rows=rows_out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
