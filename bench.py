#!/usr/bin/env python
"""Headline benchmark: full-batch R-GCN epoch time (ms) + stacked-CSR SpMM HBM GB/s on the
AM-shaped synthetic graph (BASELINE.json `metric`).

    python bench.py --gpus 1 --steps 20 --warmup 3 [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

One "step" = one epoch = forward (2 R-GCN layers), cross-entropy on the labelled rows,
backward, clip_grad_norm_(1.0), Adam — mrgcn/tasks/node_classification.py:166-193 — with all
inputs resident in HBM.  N > 1 runs N independent replicas of the same epoch (the AM graph
and its optimizer state fit one MI355X several times over; see DESIGN.md "multi-GPU").

A plain run sets up, warms up, times the K steps and prints the line: `value` = `ms_per_step` = the epoch time of
those K steps.  `--full` adds every other measurement of the line (SpMM roofline, seeds 0-2 whose median then becomes
`value`, side workloads, reference loops, yardsticks, CPU baseline, the partitioned probes of N > 1).
`--dump-outputs DIR` writes what the last timed step left its caller (loss, trained parameters) as .npy files.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X spec (MI355X_MICROARCH.md); 6.29 TB/s measured copy
# BASELINE.json configs[4] (synthetic 10 M-node graph) and configs[3] (FB15k-237 link prediction, "node-partitioned
# 1 -> 8"): one graph over the GPUs of the node
PARTITIONED_WORKLOADS = ("synth10m", "fb15k")



def _env_switches():
    """The MRGCN_* environment switches set for this run, and the library's configuration entries that differ from their
    defaults (they select kernels and layouts: DESIGN.md, switches table)."""
    out = {k: v for k, v in sorted(os.environ.items()) if k.startswith("MRGCN_")}
    try:
        from mrgcn_amd import _lib
        out["library_config"] = _lib.config()
    except Exception:  # noqa: BLE001  (informational)
        pass
    return out

def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="am", help="am | mutag | aifb | synth10m | fb15k (link prediction: R-GCN encoder + DistMult decoder, BASELINE config 4)")
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the graph (debug only)")
    ap.add_argument("--value-mode", default="norm_f32", choices=["norm_f32", "ref_int8"])
    ap.add_argument("--engine", default="fused", choices=["fused", "literal"])
    ap.add_argument("--reorder", action="store_true",
                    help="relabel the nodes of the synthetic graph so that those within reach of the labels "
                         "come first (mrgcn_amd.data.reorder): the rest of weight_I then never receives "
                         "gradient and whole chunks of it are skipped by the backward and by Adam.  Off by "
                         "default: the benchmark graph keeps the generator's (random) numbering")
    ap.add_argument("--no-renumbered-extra", dest="renumbered_extra", action="store_false",
                    help="skip the informational second measurement (extra.epoch_ms_nodes_renumbered: the same "
                         "epoch on the graph renumbered by mrgcn_amd.data.reorder); N = 1, graphs up to 40 M "
                         "non-zeros only")
    ap.add_argument("--no-graph", dest="graph", action="store_false",
                    help="launch every kernel of the epoch eagerly instead of replaying the epoch captured into a "
                         "hipGraph (GraphedTrainStep: one launch per epoch instead of ~40; AIFB 0.41 -> 0.26 ms, "
                         "MUTAG 0.97 -> 0.47 ms, AM 12.7 -> 12.5 ms)")
    ap.add_argument("--operand", default="f32", choices=["f32", "bf16"],
                    help="storage type of the fused engine's compact operand (bf16: SURVEY §8d's extra run)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--cpu-scale", type=float, default=1.0 / 16,
                    help="fraction of the workload the CPU baseline runs (a second run takes a quarter of it)")
    ap.add_argument("--no-reference-loop", dest="reference_loop", action="store_false",
                    help="skip the informational eager measurements of the reference's own loop (extra.epoch_ms_eager, "
                         "epoch_ms_reference_loop = mrgcn_amd.optim drop-ins, epoch_ms_reference_loop_torch_optim = "
                         "torch.optim.Adam + torch's clip, epoch_ms_dense_path = train_step(row_sparse=False))")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-literal-spmm", action="store_true")
    ap.add_argument("--partition", dest="partition", action="store_true", default=None,
                    help="N > 1: node-partition ONE graph over the ranks (strong scaling, mrgcn_amd.partition) "
                         "instead of running N replicas.  Default: on for the workloads BASELINE.json names as "
                         "partitioned (synth10m = config 5), off (replicas, weak scaling) for the others")
    ap.add_argument("--no-partition", dest="partition", action="store_false")
    ap.add_argument("--spmm-iters", type=int, default=30)
    ap.add_argument("--probe-child", default="", help=argparse.SUPPRESS)   # (internal: run_probe_child)
    ap.add_argument("--no-seeds", dest="seeds", action="store_false",
                    help="skip extra.seeds_ms_per_step (the same K epochs on the graphs of seeds 0-2; default AM run only)")
    ap.add_argument("--no-side-workloads", dest="side_workloads", action="store_false",
                    help="skip extra.workloads (fb15k, synth10m, aifb, mutag, AM ref_int8, AM bf16 as compact records; "
                         "default AM run only)")
    ap.add_argument("--full", action="store_true",
                    help="everything beside the timed steps as well: roofline, seeds 0-2 (their median becomes `value`), "
                         "side workloads, reference loops, yardsticks, CPU baseline, partitioned probes (the --no-* "
                         "switches above select among them).  Off: the line carries the timed steps only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one left its caller (the loss and the trained "
                         "parameters; a fixed, seeded sample of a large one) as DIR/<name>.npy in float32")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return a


DUMP_SAMPLE = 1 << 20           # elements written of a larger parameter (a fixed, seeded choice of positions)
DUMP_BUDGET = 64 << 20          # bytes written by --dump-outputs at most


def dump_outputs(out_dir, loss, named_params):
    """--dump-outputs: the loss of the last timed step and the parameters it left, as float32 .npy files.  A parameter
    of more than DUMP_SAMPLE elements is written as DUMP_SAMPLE draws of its flattened positions (sorted, duplicates
    dropped) from a generator seeded by its name and size: the same positions in every run and every build."""
    import zlib

    import torch
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"loss": loss.detach().float().reshape(1)}
    for name, p in named_params:
        flat = p.detach().reshape(-1)
        if flat.numel() > DUMP_SAMPLE:
            rng = np.random.default_rng(zlib.crc32(f"{name}:{flat.numel()}".encode()))
            pos = np.unique(rng.integers(0, flat.numel(), DUMP_SAMPLE, dtype=np.int64))
            flat = flat[torch.from_numpy(pos).to(flat.device)]
        arrays["param." + name] = flat.float()
    total = 0
    for name, t in arrays.items():
        a = t.cpu().numpy()
        total += a.nbytes
        if total > DUMP_BUDGET:
            raise RuntimeError(f"--dump-outputs: more than {DUMP_BUDGET >> 20} MB at {name}")
        np.save(os.path.join(out_dir, name + ".npy"), a)


def event_time_ms(fn, iters, stream_ptr):
    """Average duration of `fn` over `iters` launches, measured with HIP events recorded on
    the stream the kernels run on (through the C ABI, not torch.cuda.Event)."""
    import ctypes as C
    from mrgcn_amd import _lib as L
    lib = L.load()
    e0, e1 = C.c_void_p(), C.c_void_p()
    L.check(lib.mrgcn_event_create(C.byref(e0)))
    L.check(lib.mrgcn_event_create(C.byref(e1)))
    for _ in range(3):
        fn()
    L.check(lib.mrgcn_event_record(e0, stream_ptr))
    for _ in range(iters):
        fn()
    L.check(lib.mrgcn_event_record(e1, stream_ptr))
    ms = C.c_float()
    L.check(lib.mrgcn_event_elapsed_ms(e0, e1, C.byref(ms)))
    lib.mrgcn_event_destroy(e0)
    lib.mrgcn_event_destroy(e1)
    return ms.value / iters


def spmm_roofline(plan, F, operand, iters, dev, workload, scale, pmc_ok=True):
    """`roofline` of the stacked-CSR product of a layer of F outputs on the COMPACT view, with the operand as the
    layer keeps it: fp32 rows (packed or padded, functional._ld_for) or bf16 rows (`--operand bf16`: 2-byte elements in
    SURVEY §8d's formula).  HIP events on the launch stream around `iters` back-to-back launches."""
    import torch
    from mrgcn_amd import _lib as L
    from mrgcn_amd.functional import _ld_for, _ld_for_bf16
    stream = torch.cuda.current_stream(dev).cuda_stream
    bf16 = operand == "bf16"
    ld = _ld_for_bf16(F) if bf16 else _ld_for(F)
    M = torch.randn((plan.nop, ld), device=dev)
    if bf16:
        M = M.to(torch.bfloat16)
    if F <= 16 and F % 4:
        # the output as the layer holds it: the first F columns of rows padded to whole 16-byte pieces
        Y = torch.empty((plan.num_rows, (F + 3) // 4 * 4), device=dev)[:, :F]
        t_c = event_time_ms(lambda: plan.spmm(L.VIEW_COMPACT, M, F=F, out=Y, pad_writable=True), iters, stream)
    else:
        Y = torch.empty((plan.num_rows, F), device=dev)
        t_c = event_time_ms(lambda: plan.spmm(L.VIEW_COMPACT, M, F=F, out=Y), iters, stream)
    bytes_alg = plan.spmm_bytes(F, elem_bytes=2 if bf16 else 4)
    ach = bytes_alg / (t_c * 1e-3) / 1e9
    # HBM bytes per launch come from separate rocprofv3 --pmc passes (tools/pmc_passes.sh ->
    # tools/make_spmm_pmc_json.py); the file records the digest of the kernel's sources and is only quoted
    # when that equals this tree's — otherwise traffic is null
    traffic, traffic_note = None, "no counter file for this workload"
    if pmc_ok:
        try:
            from mrgcn_amd.build import source_digest
            fname = {"am": "spmm_pmc_latest.json", "fb15k": "spmm_pmc_fb15k.json"}.get(workload)
            pm = json.load(open(os.path.join(ROOT, "profiles", fname))) if fname else {}
            if (pm.get("workload") == workload and pm.get("F") == F and scale == 1.0
                    and pm.get("operand", "f32") == operand):
                if pm.get("source_digest") == source_digest():
                    traffic, traffic_note = pm["hbm_bytes_per_launch"], f"profiles/{fname} (PMC pass of this tree)"
                else:
                    traffic_note = f"profiles/{fname} predates the current spmm.hip / plan.hip: not quoted"
        except Exception as e:  # noqa: BLE001
            traffic_note = "counter file unreadable: " + str(e)[:80]
    kern = ("mrgcn::k_spmm3<G,VEC> (one launch: rows of several blocks are finished in-kernel)" if F <= 16
            else "mrgcn::k_spmm<G,VEC> (+k_spmm_finalize)")
    return {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
            "traffic": traffic, "traffic_source": traffic_note,
            "kernel": "%s on the compact view, F=%d, ld=%d, %s operand" % (kern, F, ld, operand),
            "algorithmic_bytes": bytes_alg, "avg_ms": t_c}


def spmm_in_epoch(live, dims, operand, dev, epochs=6):
    """The stacked-CSR product as the EPOCH launches it — behind the operand's producer, caches in the state the epoch
    leaves them in — instead of thirty back-to-back launches: HIP events around every COMPACT product of `epochs` eager
    epochs of the headline's model (the same kernels the replayed hipGraph holds; a kernel's duration does not depend on
    how it was launched).  Returns {F: {avg_ms, frac}}; `roofline.in_epoch_frac` is the lower fraction."""
    import ctypes as C
    import torch
    from mrgcn_amd import _lib as L
    from mrgcn_amd.train import ClipAdam, train_step
    lib = L.load()
    plan, model = live["plan"], live["model"]
    A, X, idx, tgt = live["A"], live["X"], live["idx"], live["tgt"]
    stream = torch.cuda.current_stream(dev).cuda_stream
    pairs = []
    orig = plan.spmm

    def timed_spmm(view, D, *a, **k):
        if view != L.VIEW_COMPACT:
            return orig(view, D, *a, **k)
        e0, e1 = C.c_void_p(), C.c_void_p()
        L.check(lib.mrgcn_event_create(C.byref(e0)))
        L.check(lib.mrgcn_event_create(C.byref(e1)))
        L.check(lib.mrgcn_event_record(e0, stream))
        out = orig(view, D, *a, **k)
        L.check(lib.mrgcn_event_record(e1, stream))
        pairs.append((int(k.get("F") or D.shape[1]), e0, e1))
        return out

    opt = ClipAdam(model.parameters(), lr=0.01, weight_decay=0.0, max_norm=1.0)
    plan.spmm = timed_spmm
    try:
        for ep in range(epochs + 2):
            if ep == 2:   # two warm-up epochs (allocator, first-use paths), then the measured ones
                torch.cuda.synchronize(dev)
                for _, e0, e1 in pairs:
                    lib.mrgcn_event_destroy(e0)
                    lib.mrgcn_event_destroy(e1)
                pairs.clear()
            train_step(model, lambda: model(X, A), idx, tgt, opt)
        torch.cuda.synchronize(dev)
    finally:
        del plan.spmm   # (the instance attribute shadowed the method)
    by_f = {}
    for F, e0, e1 in pairs:
        ms = C.c_float()
        L.check(lib.mrgcn_event_elapsed_ms(e0, e1, C.byref(ms)))
        lib.mrgcn_event_destroy(e0)
        lib.mrgcn_event_destroy(e1)
        by_f.setdefault(F, []).append(ms.value)
    out = {}
    for F, v in by_f.items():
        avg = sum(v) / len(v)
        b = plan.spmm_bytes(F, elem_bytes=2 if operand == "bf16" else 4)
        out[str(F)] = {"avg_ms": avg, "launches": len(v), "frac": b / (avg * 1e-3) / 1e9 / HBM_PEAK_GBS}
    return out


def epoch_algorithmic_bytes(plan, dims, B, R, N, operand="f32"):
    """ALGORITHMIC bytes of one epoch of the two-layer node-classification model (every operand counted once, gathered
    rows counted once however often they are re-read; the per-kernel terms of DESIGN.md §3): forward operand
    construction + the two products, the backward over the columns / nodes that carry gradient (their counts come from
    the gradient supports the epoch ran on), clip + Adam on the node blocks with gradient.  None when the epoch did
    not run on supports (the counts are then unknown without a device read-back)."""
    sups = sorted(plan.__dict__.get("_supports", {}).values(), key=lambda q: -q.L)
    if len(dims) != 2 or B <= 0 or len(sups) < 2:
        return None
    s0, s1 = sups[0], sups[-1]            # layer 0 (the larger support), layer 1 (the labelled rows')
    (K0, F0), (_, F1) = dims
    e = 2 if operand == "bf16" else 4
    ncols, nnz = plan.ncols, plan.nnz
    ld0, ld1 = (F0 + 3) // 4 * 4, (F1 + 3) // 4 * 4
    fwd = 0
    if K0 > 0:
        fwd += N * K0 * 4 + R * K0 * F0 * 4 + ncols * (ld0 * 4 + 8)          # layer-0 transform: X once, W, addend out
    fwd += N * B * F0 * 4 + ncols * ((ld0 * 4 if K0 > 0 else 0) + F0 * e + 8) + N * 4   # basis mix: V once, M out
    fwd += plan.spmm_bytes(F0, elem_bytes=e)
    fwd += N * F0 * 4 + R * F0 * F1 * 4 + ncols * (F1 * e + 12)              # layer-1 transform: H once, M out
    fwd += plan.spmm_bytes(F1, elem_bytes=e)
    bwd = 0
    for q, ld, F in ((s1, ld1, F1), (s0, ld0, F0)):
        bwd += q.E * 8 + q.L * (ld * 4 + 4)                                   # dM over the support
    bwd += s1.NL * F0 * 4 + s1.L * ld1 * 4 + R * F0 * F1 * 4 * 2 + N * F0 * 4  # layer 1: dW, dX (every row written)
    bwd += s0.NL * B * F0 * 4 + s0.L * (ld0 * 4 + 2 * B * 4)                   # layer 0: V of the live nodes, D out + in
    if K0 > 0:
        bwd += s0.NL * K0 * 4 + s0.L * ld0 * 4 + R * K0 * F0 * 4               # layer 0: dW (X rows of the live nodes)
    adam = 6 * s0.NL * B * F0 * 4 + s0.L * ld0 * 4                            # p, m, v of the blocks with gradient
    return {"forward": fwd, "backward": bwd, "adam": adam, "total": fwd + bwd + adam,
            "live_cols": [s0.L, s1.L], "live_nodes": [s0.NL, s1.NL], "live_entries": [s0.E, s1.E]}


def nc_workload(args, name, dev, value_mode=None, operand=None, seed=None, scale=None, steps=None, warmup=None,
                keep=False):
    """One node-classification workload on this GPU: synthetic graph of the BASELINE shape, model, ClipAdam, the epoch
    (hipGraph replay unless --no-graph), `warmup` untimed and `steps` timed epochs.  Returns a record; with `keep`
    nothing is timed here and the record carries the live objects (the headline: main() times `step` under the
    contract's barriers and runs its extras on them)."""
    import torch
    from mrgcn_amd import synth
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.plan import plan_of
    from mrgcn_amd.train import ClipAdam, GraphedTrainStep, train_step
    value_mode = value_mode or args.value_mode
    operand = operand or args.operand
    seed = args.seed if seed is None else seed
    scale = args.scale if scale is None else scale
    steps = args.steps if steps is None else steps
    warmup = args.warmup if warmup is None else warmup
    sh = synth.SHAPES[name]
    t0 = time.time()
    g = synth.make_graph(name, seed=seed, scale=scale, value_mode=value_mode)
    N, R, B = g.num_nodes, g.num_relations, sh["bases"]
    dims = synth.layer_dims(name)
    featureless = sh["x_width"] == 0
    idx_np, y_np = synth.make_labels(name, N, seed, scale)
    if args.reorder:
        from mrgcn_amd.data import reorder
        order, inv = reorder.label_reach_order(g.rows, g.cols, N, R, idx_np, hops=len(dims))
        g.rows, g.cols = reorder.relabel_coo(g.rows, g.cols, N, inv)
        idx_np = inv[idx_np]
    torch.manual_seed(seed)
    modules = [(i, o, "mrgcn", torch.nn.ReLU() if li < len(dims) - 1 else None) for li, (i, o) in enumerate(dims)]
    A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([g.rows, g.cols])), torch.from_numpy(g.vals),
                                (N, R * N)).to(dev)
    model = RGCN(modules, R, N, B, 0.0, featureless, False, False).to(dev)
    model.set_engine(args.engine)
    model.set_operand_dtype(operand)
    X = None if featureless else torch.randn((N, sh["x_width"]), device=dev)
    idx = torch.from_numpy(idx_np).to(dev)
    tgt = torch.from_numpy(y_np).to(dev)
    opt = ClipAdam(model.parameters(), lr=0.01, weight_decay=0.0, max_norm=1.0, capturable=args.graph)
    plan = plan_of(A, N, R, operand_row_bytes=model.operand_row_bytes())

    def step():
        return train_step(model, lambda: model(X, A), idx, tgt, opt)
    graph_used = False
    if args.graph:
        try:
            graphed = GraphedTrainStep(model, lambda: model(X, A), idx, tgt, opt, warmup=max(warmup, 1))
            graph_used = True

            def step():  # noqa: F811
                return graphed()
        except Exception as e:  # noqa: BLE001  (measurement harness only: time the eager epoch instead)
            print("bench: hipGraph capture failed (%s); timing eager launches" % str(e)[:200], file=sys.stderr)
            opt = ClipAdam(model.parameters(), lr=0.01, weight_decay=0.0, max_norm=1.0)
    setup_s = time.time() - t0
    ms = final = None
    if not keep:   # (the headline's timed region is main()'s own: warm-ups, barrier, K steps, barrier)
        for _ in range(warmup):
            step()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = step()
        torch.cuda.synchronize(dev)
        ms = (time.perf_counter() - t0) / steps * 1e3
        final = float(loss)
    rec = dict(ms_per_step=ms, final_loss=final, setup_s=setup_s, graph_used=graph_used, N=N, R=R, B=B, dims=dims,
               nnz=plan.nnz, ncols=plan.ncols, featureless=featureless, labelled=int(idx.numel()),
               params=sum(p.numel() for p in model.parameters()), value_mode=value_mode, operand=operand,
               scale=scale, seed=seed, x_width=sh["x_width"])
    if keep:
        rec.update(g=g, A=A, X=X, idx=idx, tgt=tgt, idx_np=idx_np, y_np=y_np, model=model, opt=opt, plan=plan,
                   modules=modules, step=step)
    else:
        rec["_plan"] = plan  # (the caller measures the product on it, then drops it)
    return rec


def side_workloads(args, dev):
    """extra.workloads of the default line: the other BASELINE configs, AM with the reference's int8 boundary cast and
    AM with the bf16 operand, each as a compact record {ms_per_step, spmm_frac, spmm_avg_ms, config}; a workload that
    fails leaves {"error": ...} and the rest still run."""
    import gc

    import torch
    out = {}

    def compact(rec, roof, extra_cfg=None):
        cfg = {"N": rec["N"], "R": rec["R"], "nnz": rec["nnz"], "layers": rec["dims"], "num_bases": rec["B"],
               "value_mode": rec["value_mode"], "operand": rec["operand"], "labelled": rec["labelled"],
               "launch": "hipGraph replay" if rec["graph_used"] else "eager", "steps": rec["steps"]}
        cfg.update(extra_cfg or {})
        return {"ms_per_step": rec["ms_per_step"], "spmm_frac": roof["frac"], "spmm_avg_ms": roof["avg_ms"],
                "spmm_gbps": roof["achieved"], "spmm_algorithmic_bytes": roof["algorithmic_bytes"],
                "spmm_kernel": roof["kernel"], "final_loss": rec["final_loss"], "setup_s": rec["setup_s"], "config": cfg}

    plan_nc = [("aifb", dict(name="aifb"), 40), ("mutag", dict(name="mutag"), 40),
               ("am_ref_int8", dict(name="am", value_mode="ref_int8"), 10),
               ("am_bf16", dict(name="am", operand="bf16"), 10),
               ("synth10m", dict(name="synth10m"), 5)]
    for key, kw, steps in plan_nc:
        try:
            rec = nc_workload(args, kw["name"], dev, value_mode=kw.get("value_mode", "norm_f32"),
                              operand=kw.get("operand", "f32"), scale=1.0, steps=steps, warmup=2)
            rec["steps"] = steps
            plan = rec.pop("_plan")
            roof = spmm_roofline(plan, rec["dims"][0][1], rec["operand"], 10, dev, kw["name"], 1.0, pmc_ok=False)
            ab = epoch_algorithmic_bytes(plan, rec["dims"], rec["B"], rec["R"], rec["N"], rec["operand"])
            out[key] = compact(rec, roof)
            if ab:
                out[key]["epoch_algorithmic_bytes"] = ab["total"]
                out[key]["epoch_frac"] = ab["total"] / (rec["ms_per_step"] * 1e-3) / (HBM_PEAK_GBS * 1e9)
            del rec, plan
        except Exception as e:  # noqa: BLE001  (fail-soft: the headline line must still print)
            out[key] = {"error": (type(e).__name__ + ": " + str(e))[:300]}
        gc.collect()
        torch.cuda.empty_cache()
    try:
        sub = argparse.Namespace(**vars(args))
        sub.workload, sub.steps, sub.warmup, sub.no_cpu_baseline, sub.scale = "fb15k", 20, 3, True, 1.0
        sub.value_mode = "norm_f32"
        line = main_lp(sub, emit=False)
        out["fb15k"] = {"ms_per_step": line["ms_per_step"], "spmm_frac": line["roofline"]["frac"],
                        "spmm_avg_ms": line["roofline"]["avg_ms"], "spmm_gbps": line["roofline"]["achieved"],
                        "spmm_algorithmic_bytes": line["roofline"]["algorithmic_bytes"],
                        "spmm_kernel": line["roofline"]["kernel"], "final_loss": line["extra"]["final_loss"],
                        "rank_500_raw_ms": line["extra"].get("rank_500_raw_ms"),
                        "rank_500_filtered_ms": line["extra"].get("rank_500_filtered_ms"), "config": line["config"]}
    except Exception as e:  # noqa: BLE001
        out["fb15k"] = {"error": (type(e).__name__ + ": " + str(e))[:300]}
    gc.collect()
    torch.cuda.empty_cache()
    for key, compute in (("am_encoders", "f32"), ("am_encoders_bf16", "bf16")):
        try:
            out[key] = am_encoders_record(args, dev, compute=compute)
        except Exception as e:  # noqa: BLE001
            out[key] = {"error": (type(e).__name__ + ": " + str(e))[:300]}
        gc.collect()
        torch.cuda.empty_cache()
    return out


def am_encoders_record(args, dev, steps=10, warm=2, compute="f32"):
    """extra.workloads.am_encoders — BASELINE config 3 "full multimodal": `MRGCN(FullBatch)` on the AM-shaped graph with
    the modality encoders in front of the R-GCN instead of given feature columns (mrgcn/models/mrgcn.py:189-214,
    :250-305): two xsd.numeric MLPs (-> 4 each), an xsd.date MLP (-> 3), an xsd.string head (-> 16) on a stand-in
    language model, a blob.image head (-> 128) on a stand-in CNN backbone (no pretrained weights offline: small frozen
    torch modules), and an ogc.wktLiteral TCNN (-> 5): X is N x 160.  One step = encoders + gates + scatter + the two
    R-GCN layers + CE + backward through everything + clip + Adam, replayed from a hipGraph.  `encoder_share` compares
    it with the same epoch on given feature columns of the same width.  `compute` = "bf16": the bf16 pipeline
    (`MRGCN.set_compute_dtype`): bf16 activations in the R-GCN layers, the encoders' products and the stand-in backbones
    on the bf16 matrix cores, fp32 accumulation / parameters / BatchNorm statistics / optimizer."""
    import scipy.sparse as sp
    import torch
    import torch.nn as nn
    from mrgcn_amd import synth
    from mrgcn_amd.data.batch import FullBatch
    from mrgcn_amd.models.mrgcn import MRGCN
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.train import ClipAdam, GraphedTrainStep, train_step

    class StandInLM(nn.Module):        # token ids [n, L] -> (hidden states [n, L, 64],)   (transformer.py:8-38's input)
        def __init__(self):
            super().__init__()
            self.emb = nn.Embedding(1000, 64)
            self.lin = nn.Linear(64, 64)

        def forward(self, ids):
            return (self.lin(self.emb(ids)),)

    class StandInCNN(nn.Module):       # `features` + `classifier` like torchvision's mobilenet_v2 (imagecnn.py:9-41)
        def __init__(self):
            super().__init__()
            self.features = nn.Sequential(nn.Conv2d(3, 16, 3, stride=2, padding=1), nn.ReLU(),
                                          nn.Conv2d(16, 32, 3, stride=2, padding=1))
            self.classifier = nn.Linear(32, 10)

    t0 = time.time()
    g = synth.make_graph("am", seed=args.seed, scale=1.0, value_mode="norm_f32")
    N, R, B = g.num_nodes, g.num_relations, synth.SHAPES["am"]["bases"]
    rng = np.random.default_rng(args.seed + 3)

    def nodes(k):
        return np.sort(rng.choice(N, k, replace=False))
    n_num1, n_num2, n_date, n_str, n_img, n_wkt = 300_000, 200_000, 150_000, 400_000, 50_000, 20_000
    enc = {
        "xsd.numeric": [[rng.standard_normal((n_num1, 1)).astype(np.float32), nodes(n_num1), np.ones(n_num1, dtype=int)],
                        [rng.standard_normal((n_num2, 1)).astype(np.float32), nodes(n_num2), np.ones(n_num2, dtype=int)]],
        "xsd.date": [[rng.standard_normal((n_date, 3)).astype(np.float32), nodes(n_date), np.ones(n_date, dtype=int)]],
        "xsd.string": [[rng.integers(1, 1000, (n_str, 16)).astype(np.int64), nodes(n_str), np.full(n_str, 16)]],
        "blob.image": [[rng.integers(0, 256, (n_img, 3, 16, 16)).astype(np.uint8), nodes(n_img), np.ones(n_img, dtype=int)]],
        "ogc.wktLiteral": [[(rng.random((n_wkt, 9, 20)) < 0.15).astype(np.float32), nodes(n_wkt), np.full(n_wkt, 20)]],
    }
    torch.manual_seed(args.seed)
    emb_cfg = sorted([("blob.image", (StandInCNN(), {"mean": [0.485, 0.456, 0.406], "std": [0.229, 0.224, 0.225]}, 128, 0.0), False),
                      ("xsd.string", (StandInLM(), 16, 0.0), False),
                      ("ogc.wktLiteral", (9, 5, "S", 0.0), False),
                      ("xsd.date", (3, 3, 0.0), False),
                      ("xsd.numeric", (1, 4, 0.0), False), ("xsd.numeric", (1, 4, 0.0), False)], key=lambda t: t[0])
    W = 128 + 16 + 5 + 3 + 4 + 4
    modules = [(W, 10, "mrgcn", nn.ReLU()), (10, 11, "mrgcn", None)]
    model = MRGCN(modules, emb_cfg, R, N, num_bases=B, p_dropout=0.0, featureless=False, bias=True,
                  gcn_gpu_acceleration=True)
    model.set_compute_dtype(compute)
    A = sp.csr_matrix((g.vals, (g.rows, g.cols)), shape=(N, R * N))
    X = [np.empty((N, 0), dtype=np.float32)] + [[dt, enc[dt], False] for dt in sorted(enc)]
    batch = FullBatch(A, X, np.arange(N), value_mode="norm_f32")
    batch.as_tensors_()
    batch.to(model.devices)
    model.train()
    idx_np, y_np = synth.make_labels("am", N, args.seed, 1.0)
    idx, y = torch.from_numpy(idx_np).to(dev), torch.from_numpy(y_np).to(dev)
    opt = ClipAdam([p for p in model.parameters() if p.requires_grad], lr=0.01, max_norm=1.0, capturable=True)
    setup_s = time.time() - t0

    def timed(fn, k):
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        for _ in range(k):
            out = fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t) / k * 1e3, out
    rec = {"config": {"workload": "AM-shaped synthetic KG, MRGCN(FullBatch) with modality encoders (SURVEY §8d config 3, "
                                  "full multimodal)", "N": N, "R": R, "nnz": g.nnz, "num_bases": B,
                      "layers": [[W, 10], [10, 11]], "compute": compute,
                      "literals": {"xsd.numeric": [n_num1, n_num2], "xsd.date": n_date, "xsd.string (16 tokens)": n_str,
                                   "blob.image (3x16x16)": n_img, "ogc.wktLiteral (9x20)": n_wkt},
                      "backbones": "stand-in torch modules (no pretrained weights offline), frozen; heads / MLPs / TCNN "
                                   "on this package's kernels", "labelled": int(len(idx_np))},
           "setup_s": setup_s}
    fwd = lambda: model(batch)   # noqa: E731
    for _ in range(warm):
        train_step(model, fwd, idx, y, opt)
    # (eager steps one by one, the median: the first few also grow torch's caching allocator — fresh segments cost
    # tens of ms each on first touch — which says nothing about the step)
    eager = [timed(lambda: train_step(model, fwd, idx, y, opt), 1)[0] for _ in range(6)]
    rec["ms_per_step_eager"], rec["ms_per_step_eager_all"] = float(np.median(eager)), [round(t, 2) for t in eager]
    try:
        step = GraphedTrainStep(model, fwd, idx, y, opt, warmup=1)
        step()   # (the first replay uploads the graph)
        rec["ms_per_step"], loss = timed(step, steps)
        rec["launch"] = "hipGraph replay"
    except Exception as e:  # noqa: BLE001  (informational record: the eager figure stands)
        rec["ms_per_step"], loss = timed(lambda: train_step(model, fwd, idx, y, opt), steps)
        rec["launch"] = "eager (capture failed: %s)" % str(e)[:120]
    rec["final_loss"] = float(loss)
    # the same epoch with the encoders' output given as feature columns: what the R-GCN part costs at this width
    torch.manual_seed(args.seed)
    ref = RGCN(modules, R, N, B, 0.0, False, True, False).to(dev)
    ref.set_operand_dtype(compute)
    Xg = torch.randn((N, W), device=dev)
    opt2 = ClipAdam(ref.parameters(), lr=0.01, max_norm=1.0, capturable=True)
    step2 = GraphedTrainStep(ref, lambda: ref(Xg, batch.A), idx, y, opt2, warmup=2)
    step2()
    rec["ms_per_step_given_features"], _ = timed(step2, steps)
    rec["encoder_share"] = max(0.0, 1.0 - rec["ms_per_step_given_features"] / rec["ms_per_step"])
    # what the two frozen stand-in backbones cost by themselves (torch modules: MIOpen / hipBLASLt launches, not this
    # package's kernels — the small-image convolution goes through MIOpen's im2col + GEMM per image group, ~10 k launches
    # a step): forward only, they take no gradient (imagecnn.py:17-19, transformer.py:16-18)
    try:
        cnn = next(c[1][0] for c in emb_cfg if c[0] == "blob.image")
        lm = next(c[1][0] for c in emb_cfg if c[0] == "xsd.string")
        p_dev = next(cnn.parameters()).device
        img = torch.rand((n_img, 3, 16, 16), device=p_dev)
        ids = torch.randint(1, 1000, (n_str, 16), device=next(lm.parameters()).device)
        with torch.no_grad():
            t_cnn, _ = timed(lambda: cnn.features(img), 3)
            t_lm, _ = timed(lambda: lm(ids), 3)
        rec["ms_standin_backbones"] = {"image_cnn_features": t_cnn, "language_model": t_lm}
        rec["ms_per_step_less_backbones"] = rec["ms_per_step"] - t_cnn - t_lm
    except Exception as e:  # noqa: BLE001  (informational)
        rec["ms_standin_backbones"] = {"error": str(e)[:160]}
    return rec


def minibatch_record(args, dev, scale=0.25, batch_nodes=1024, steps=24, warm=6):
    """extra.minibatch of the default line: a two-layer model on the AM/4 graph trained on a
    freshly sampled batch of 1 024 nodes every step, nothing prepared ahead — the batch is a chain of forward supports on
    the full graph's plan (data.batch.A_BatchMasked, csrc/masked.hip), the step is mrgcn_amd.train.train_step.
    ms_per_step covers everything between two steps: sampling the ids on the host, the two support builds (one host
    wait), forward, backward, clip, Adam."""
    import scipy.sparse as sp
    import torch
    from mrgcn_amd import synth
    from mrgcn_amd.data import batch as mb
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.plan import GraphPlan
    from mrgcn_amd.train import ClipAdam, train_step
    g = synth.make_graph("am", seed=args.seed, scale=scale)
    N, R = g.num_nodes, g.num_relations
    A = sp.csr_matrix((g.vals, (g.rows, g.cols)), shape=(N, R * N))
    dims = synth.layer_dims("am")
    mods = [(dims[0][0], dims[0][1], "mrgcn", torch.nn.ReLU()), (dims[1][0], dims[1][1], "mrgcn", None)]
    torch.manual_seed(args.seed)
    model = RGCN(mods, R, N, synth.SHAPES["am"]["bases"], 0.0, False, True, False).to(dev)
    opt = ClipAdam(model.parameters(), lr=0.01, max_norm=1.0)
    X = torch.randn((N, dims[0][0]), device=dev)
    plan = GraphPlan.from_csr(A, N, R, value_mode="ref_int8", device=dev, operand_row_bytes=model.operand_row_bytes())
    rng = np.random.default_rng(args.seed)
    ys = torch.from_numpy(rng.integers(0, dims[-1][1], batch_nodes)).to(dev)
    rows = torch.arange(batch_nodes, device=dev)
    sizes = None
    for k in range(steps):
        if k == warm:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
        am = mb.A_BatchMasked(plan, np.sort(rng.choice(N, batch_nodes, replace=False)), 2)
        loss = train_step(model, lambda: model(X, am), rows, ys, opt)
        sizes = [(s_.NR, s_.NL, s_.E) for s_ in am.supports]
        am.close()
    torch.cuda.synchronize(dev)
    ms = (time.perf_counter() - t0) / (steps - warm) * 1e3
    return {"ms_per_step": ms, "graph": "am x %g (N=%d, R=%d, nnz=%d)" % (scale, N, R, A.nnz), "batch_nodes": batch_nodes,
            "layers": dims, "resampled_every_step": True, "prepared_ahead": False,
            "levels_rows_neighbours_entries": sizes, "final_loss": float(loss),
            "path": "masked pass over the full graph's plan (A_BatchMasked + train_step), in line"}


def cpu_baseline(args, shape_name):
    """The reference's ATen op sequence (oracle/aten_literal.py, pinned against the reference's golden vectors)
    timed on this host's cores on bounded samples of the workload: the thread count is the best of a short sweep
    on a 1/64 sample (the reference leaves torch's default = all cores, which on a many-core host is far slower
    for these small sparse ops); the epoch is then timed at TWO scales (--cpu-scale, default 1/16: 3 warm-ups + 10 timed
    epochs, median and min — BASELINE.md's protocol; and a quarter
    of it) so that the linear extrapolation to the full graph is shown by the pair instead of assumed."""
    import torch  # noqa: F401
    from mrgcn_amd import synth
    from oracle import aten_literal as AL
    sh = synth.SHAPES[shape_name]
    dims = synth.layer_dims(shape_name)
    featureless = sh["x_width"] == 0
    cores = os.cpu_count() or 1

    def sample(sc):
        g = synth.make_graph(shape_name, seed=args.seed, scale=sc, value_mode=args.value_mode)
        rng = np.random.default_rng(args.seed)
        X = None if featureless else rng.standard_normal((g.num_nodes, sh["x_width"])).astype(np.float32)
        idx, y = synth.make_labels(shape_name, g.num_nodes, args.seed, sc)
        return g, X, idx, y

    def timed(smp, steps, threads, warmup=1, per_epoch=False):
        g, X, idx, y = smp
        return AL.time_epochs(dims, g.num_relations, g.num_nodes, sh["bases"], g.rows, g.cols, g.vals, X, idx, y,
                              featureless, warmup=warmup, steps=steps, threads=threads, seed=args.seed,
                              per_epoch=per_epoch)

    big = args.cpu_scale * args.scale
    small = big / 4
    probe = sample(min(big, args.scale / 64))
    t_start = time.time()
    sweep = {}
    quota = cpu_quota()
    for th in sorted({min(c, cores) for c in (8, 16, 32, 64)} | ({max(1, min(int(quota), cores))} if quota else set())):
        sweep[th], _ = timed(probe, 1, th)
        if time.time() - t_start > 30:
            break
    best = min(sweep, key=sweep.get)
    del probe
    s_small = sample(small)
    ms_small, _ = timed(s_small, 3, best, warmup=3)
    n_small = s_small[0].num_nodes
    del s_small
    s_big = sample(big)
    g = s_big[0]
    # BASELINE.md's protocol: 3 warm-up epochs discarded, 10 timed, median and min reported (~3 s each at AM / 16)
    n_warm, n_big = 3, 10
    each, threads = timed(s_big, n_big, best, warmup=n_warm, per_epoch=True)
    ms, ms_min = sorted(each)[len(each) // 2], min(each)
    return {
        "value": ms / big, "unit": "ms/epoch", "cores": threads, "kind": "port",
        "sample": (f"{shape_name} x {big:.4g} (N={g.num_nodes}, R={g.num_relations}, nnz={g.nnz}): median {ms:.1f} / min "
                   f"{ms_min:.1f} ms/epoch over {n_big} timed epochs after {n_warm} warm-ups (BASELINE.md's protocol) with "
                   f"the reference's literal ATen op sequence on {threads} of "
                   f"{cores} host threads" + (f" (container CPU quota: {quota:g})" if quota else "") +
                   f" (best of a sweep on a 1/64 sample: "
                   f"{ {k: round(v, 1) for k, v in sweep.items()} }); value = median / {big:.4g}.  Second scale "
                   f"{shape_name} x {small:.4g} (N={n_small}): {ms_small:.1f} ms/epoch over 3 epochs after 3 warm-ups, i.e. "
                   f"{ms_small / small:.0f} ms/epoch extrapolated — the pair shows how linear the extrapolation is"),
        "measured_ms": ms, "measured_min_ms": ms_min, "timed_epochs": n_big, "warmup_epochs": n_warm,
        "sample_scale": big, "host_cores": cores, "host_cpu_quota": quota,
        "second_scale": {"sample_scale": small, "measured_ms": ms_small, "extrapolated_ms": ms_small / small},
    }


def renumbered_epoch_ms(args, g, idx_np, y_np, dims, modules, R, N, B, featureless, x_width, dev):
    """Informational: the same epoch after renumbering the nodes so that those within reach of the labels
    come first (a relabelling of the dataset; logits permute with the nodes).  The half of weight_I that
    never receives gradient is then contiguous and is skipped by the backward and by Adam."""
    import torch
    from mrgcn_amd.data import reorder
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.train import ClipAdam, GraphedTrainStep, train_step
    order, inv = reorder.label_reach_order(g.rows, g.cols, N, R, idx_np, hops=len(dims))
    rows2, cols2 = reorder.relabel_coo(g.rows, g.cols, N, inv)
    A2 = torch.sparse_coo_tensor(torch.from_numpy(np.stack([rows2, cols2])), torch.from_numpy(g.vals),
                                 (N, R * N)).to(dev)
    torch.manual_seed(args.seed)
    model = RGCN(modules, R, N, B, 0.0, featureless, False, False).to(dev)
    model.set_engine(args.engine)
    model.set_operand_dtype(args.operand)
    X = None if featureless else torch.randn((N, x_width), device=dev)
    idx = torch.from_numpy(inv[idx_np]).to(dev)
    tgt = torch.from_numpy(y_np).to(dev)
    opt = ClipAdam(model.parameters(), lr=0.01, weight_decay=0.0, max_norm=1.0, capturable=args.graph)
    if args.graph:
        step = GraphedTrainStep(model, lambda: model(X, A2), idx, tgt, opt, warmup=max(args.warmup, 2))
    else:
        def step():
            return train_step(model, lambda: model(X, A2), idx, tgt, opt)
    for _ in range(max(args.warmup, 2)):
        step()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / args.steps * 1e3


def reference_loop_ms(args, kind, A, X, idx, tgt, modules, R, N, B, featureless, dev):
    """Informational: the epoch as the reference's own loop drives it (tasks/node_classification.py:35-37, :190-193:
    `optim.Adam`, `CrossEntropyLoss`, `zero_grad / backward / clip_grad_norm_(1.0) / step`, launched eagerly) on a
    fresh model — `kind` = "torch" (torch.optim.Adam + torch's clip: dense node-table gradient), "fast" (the
    drop-ins of mrgcn_amd.optim: row-sparse, what install_as_mrgcn(patch_optimizer=True) gives that loop),
    "train_step" / "train_step_dense" (this package's own step, eager, row-sparse / row_sparse=False).  Logits and
    loss stay on the device (the reference copies the logits to the host first, :166)."""
    import torch
    from mrgcn_amd import optim as fast
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.train import ClipAdam, train_step
    torch.manual_seed(args.seed)
    model = RGCN(modules, R, N, B, 0.0, featureless, False, False).to(dev)
    model.set_engine(args.engine)
    model.set_operand_dtype(args.operand)
    groups = [{"params": [p for p in model.parameters() if p.requires_grad]}]
    if kind.startswith("train_step"):
        opt = ClipAdam(groups, lr=0.01, weight_decay=0.0, max_norm=1.0)

        def step():
            return train_step(model, lambda: model(X, A), idx, tgt, opt, row_sparse=None if kind == "train_step" else False)
    else:
        Adam, clip = ((torch.optim.Adam, torch.nn.utils.clip_grad_norm_) if kind == "torch"
                      else (fast.RowSparseAdam, fast.clip_grad_norm_))
        opt = Adam(groups, lr=0.01, weight_decay=0.0)
        criterion = torch.nn.CrossEntropyLoss()

        def step():
            loss = criterion(model(X, A)[idx], tgt)
            opt.zero_grad()
            loss.backward()
            clip(model.parameters(), 1.0)
            opt.step()
            return loss
    for _ in range(max(args.warmup, 2)):
        step()
    torch.cuda.synchronize(dev)
    n = max(args.steps // 2, 3)
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / n * 1e3


def labelled_batch_epoch_ms(args, plan, X, idx_np, y_np, modules, R, N, B, featureless, dev):
    """Informational: the same training step driven through the MINI-BATCH machinery with ONE batch that holds every
    labelled node (data/batch.py:185-263: `getNeighboursSparse` takes all neighbours, no sampling) and the adjacency's
    values kept for both terms (`A_BatchMasked(full_batch_values=True)`): the full-batch arithmetic on the labelled
    nodes' receptive field only — the parameters after the step equal the full-batch step's (tests/test_minibatch.py).
    Not the headline: the headline epoch computes all N rows, as the reference's full-batch mode does."""
    import torch
    from mrgcn_amd.data import batch as mb
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.train import ClipAdam, GraphedTrainStep, train_step
    torch.manual_seed(args.seed)
    model = RGCN(modules, R, N, B, 0.0, featureless, False, False).to(dev)
    order = np.argsort(idx_np, kind="stable")
    nodes = np.asarray(idx_np)[order]
    ys = torch.from_numpy(np.asarray(y_np)[order]).to(dev)
    rows = torch.arange(len(nodes), device=dev)
    am = mb.A_BatchMasked(plan, nodes, len(modules), full_batch_values=True)
    fwd = lambda: model(X, am)   # noqa: E731
    launch = "hipGraph replay"
    try:
        opt = ClipAdam(model.parameters(), lr=0.01, weight_decay=0.0, max_norm=1.0, capturable=True)
        step = GraphedTrainStep(model, fwd, rows, ys, opt, warmup=max(args.warmup, 2))
        step()
    except Exception as e:  # noqa: BLE001  (informational leg: the eager figure stands)
        launch = "eager (capture failed: %s)" % str(e)[:100]
        opt = ClipAdam(model.parameters(), lr=0.01, weight_decay=0.0, max_norm=1.0)
        step = lambda: train_step(model, fwd, rows, ys, opt)   # noqa: E731
        for _ in range(max(args.warmup, 2)):
            step()
    torch.cuda.synchronize(dev)
    n = max(args.steps // 2, 5)
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    torch.cuda.synchronize(dev)
    ms = (time.perf_counter() - t0) / n * 1e3
    sizes = [(s_.NR, s_.NL, s_.E) for s_ in am.supports]
    am.close()
    return {"ms_per_step": ms, "launch": launch, "batch_nodes": int(len(nodes)),
            "levels_rows_neighbours_entries": sizes,
            "what": "one batch = all labelled nodes (all neighbours, no sampling), adjacency values kept for both terms: "
                    "the step of the headline restricted to the labels' receptive field; same parameters after the step"}


def lp_cpu_baseline(args, sh, train_frac):
    """The reference's op sequence for one full-batch link-prediction epoch on the host (encoder: the literal ATen
    port of graph.py:62-102; decoder, loss, clip and Adam: the torch ops of tasks/link_prediction.py:244-326) on a
    bounded sample of the workload."""
    import torch
    from mrgcn_amd import synth
    from mrgcn_amd.tasks import link_prediction as lp
    from oracle import aten_literal as ref
    sc = min(1.0, max(args.cpu_scale * 4, 1e-3)) * args.scale
    g = synth.make_graph("fb15k", seed=args.seed, scale=sc, value_mode=args.value_mode)
    N, R, H, B = g.num_nodes, g.num_relations, sh["hidden"], sh["bases"]
    tr = g.triples
    rng = np.random.RandomState(args.seed)
    train = tr[rng.permutation(len(tr))[:int(train_frac * len(tr))]]
    cores = os.cpu_count() or 1
    threads = min(cores, 32)
    torch.set_num_threads(threads)
    p = ref.make_params([(0, H)], R, N, B, False, True, seed=args.seed)
    p["relations"] = torch.nn.init.xavier_uniform_(torch.empty((R, H))).requires_grad_(True)
    Ac = ref.coo_tensor(g.rows, g.cols, g.vals, (N, R * N))
    opt = torch.optim.Adam(list(p.values()), lr=0.01)
    crit = torch.nn.BCEWithLogitsLoss()

    def step():
        neg, Y = lp.sample_negatives(train, rng)
        tt = torch.from_numpy(np.concatenate([train, neg])).long()
        emb = torch.relu(ref.layer_forward(p, "layers.layer_0.", None, Ac, R, N, B, True, True))
        score = torch.sum(emb[tt[:, 0]] * p["relations"][tt[:, 1]] * emb[tt[:, 2]], dim=-1)
        loss = crit(score, torch.from_numpy(Y))
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(list(p.values()), 1.0)
        opt.step()

    step()
    t0 = time.perf_counter()
    for _ in range(2):
        step()
    ms = (time.perf_counter() - t0) / 2 * 1e3
    return {"value": ms / sc * args.scale, "unit": "ms/epoch", "cores": threads, "kind": "port",
            "sample": (f"fb15k x {sc:.4g} (N={N}, R={R}, nnz={g.nnz}, {len(train)} training triples + 20 % negatives): "
                       f"{ms:.1f} ms/epoch over 2 epochs after 1 warm-up with the reference's op sequence (literal ATen "
                       f"encoder + torch decoder / BCE / clip / Adam) on {threads} of {cores} host threads; value = "
                       f"measured / {sc:.4g} (linear in the triples; the encoder's (R*N) x out operand grows with N too)"),
            "measured_ms": ms, "sample_scale": sc, "host_cores": cores}


def main_lp(args, emit=True):
    """BASELINE config 4: FB15k-237-shaped link prediction.  One step = one full-batch epoch of
    tasks/link_prediction.py:231-326 — 20 % in-batch negatives (drawn on the device), featureless R-GCN encoder
    (N x 200, 2 bases, ReLU), DistMult scores of positives + negatives, BCE-with-logits, backward,
    clip_grad_norm_(1.0), Adam — with everything resident in HBM.  N > 1: the node-partitioned encoder with
    all-gathered embeddings and triples scored rank::world (mrgcn_amd.partition.partitioned_lp_step)."""
    import torch
    import torch.distributed as dist
    from mrgcn_amd import _lib as L
    from mrgcn_amd import dist as mdist
    from mrgcn_amd import synth
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.plan import plan_of
    from mrgcn_amd.tasks import link_prediction as lp
    from mrgcn_amd.train import ClipAdam

    world, rank, local_rank = mdist.env_world()
    ngpu = max(torch.cuda.device_count(), 1)
    dev = torch.device("cuda", (local_rank % ngpu) if world > 1 else 0)
    torch.cuda.set_device(dev)
    backend = os.environ.get("MRGCN_DIST_BACKEND", "nccl" if ngpu >= world else "gloo")
    mdist.init(backend, dev if backend == "nccl" else None)
    sh = synth.SHAPES["fb15k"]
    t0 = time.time()
    g = synth.make_graph("fb15k", seed=args.seed, scale=args.scale, value_mode=args.value_mode)
    N, R, H, B = g.num_nodes, g.num_relations, sh["hidden"], sh["bases"]
    train_frac = 272115 / 310116   # mkdataset.py:46-49: train / valid / test of FB15k-237
    rng = np.random.RandomState(args.seed)
    perm = rng.permutation(len(g.triples))
    ntrain = int(train_frac * len(g.triples))
    train, test = g.triples[perm[:ntrain]], g.triples[perm[ntrain:ntrain + 500]]
    train_dev = torch.from_numpy(train).to(dev)
    gen = torch.Generator(device=dev).manual_seed(args.seed)   # the same draws on every rank
    modules = [(0, H, "mrgcn", torch.nn.ReLU())]
    if args.partition is None:
        args.partition = True
    partitioned = args.partition and world > 1
    torch.manual_seed(args.seed)
    if not partitioned:
        A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([g.rows, g.cols])), torch.from_numpy(g.vals),
                                    (N, R * N)).to(dev)
        model = RGCN(modules, R, N, B, 0.0, True, False, True).to(dev)
        model.set_engine(args.engine)
        use_graph = bool(args.graph) and world == 1
        opt = ClipAdam(model.parameters(), lr=0.01, weight_decay=0.0, max_norm=1.0, capturable=use_graph)
        plan = plan_of(A, N, R, operand_row_bytes=model.operand_row_bytes())
        if use_graph:
            gen = None   # torch's default generator: its state is registered with a captured graph and advances per replay
        # the training facts are the same every epoch: they sit at the head of one buffer, their orders for the decoder's
        # backward are stored once, and one launch per epoch writes the 20 % corrupted copies behind them
        sampler = lp.DeviceNegativeSampler(train_dev, gen)
        static = lp.SortedTriples(sampler.facts, N, R)

        def step():
            t, Y = sampler()
            emb = model(None, A)
            score = lp.score_distmult_bc(t, emb, model.relations, static=static)
            loss = lp.binary_crossentropy(score, Y)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            return loss.detach()
    else:
        from mrgcn_amd.partition import NodePartition, PartitionedRGCN, partitioned_lp_step
        part = NodePartition(N, world, rank)
        model = PartitionedRGCN(modules, R, N, B, True, False, part, link_prediction=True).to(dev)
        model.sync_replicated()
        plan = model.build_plan(g.rows, g.cols, g.vals, dev)
        opt = ClipAdam(model.parameters(), lr=0.01, weight_decay=0.0, max_norm=1.0)
        opt.set_distributed(None, model.sharded_parameters())

        def step():
            neg, Y = lp.sample_negatives_device(train_dev, gen)
            return partitioned_lp_step(model, None, torch.cat([train_dev, neg]), Y, opt)
    launch = "eager"
    if not partitioned and use_graph:
        from mrgcn_amd.train import GraphedStep
        try:
            graphed = GraphedStep(step, warmup=max(args.warmup, 2))
            launch = "hipGraph replay"

            def step():  # noqa: F811
                return graphed()
        except Exception as e:  # noqa: BLE001  (measurement harness only: time the eager epoch instead)
            print("bench: hipGraph capture of the link-prediction epoch failed (%s); timing eager launches" % str(e)[:300],
                  file=sys.stderr)
            opt = ClipAdam(model.parameters(), lr=0.01, weight_decay=0.0, max_norm=1.0)
    setup_s = time.time() - t0
    for _ in range(args.warmup):
        step()
    mdist.barrier(dev)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    mdist.barrier(dev)
    dt = mdist.max_over_ranks(time.perf_counter() - t0, dev)
    ms_per_step = dt / args.steps * 1e3
    if args.dump_outputs and rank == 0 and emit:
        dump_outputs(args.dump_outputs, loss, model.named_parameters())
    out = None
    if rank == 0:
        roofline = ach = None
        if args.full:
            # the encoder's stacked-CSR product at this shape: rows of 800 bytes, the wide-row kernel (k_spmm<G = 64>)
            roofline = spmm_roofline(plan, H, "f32", args.spmm_iters, dev, "fb15k", args.scale)
            ach = roofline["achieved"]
        extra = {}
        if not partitioned and args.full:
            with torch.no_grad():
                emb = model(None, A)
                rel = model.relations
                torch.cuda.synchronize(dev)
                t1 = time.perf_counter()
                raw = lp.compute_ranks_fast(test, emb, rel, filtered=False)
                torch.cuda.synchronize(dev)
                t2 = time.perf_counter()
                flt = lp.compute_ranks_fast(test, emb, rel, filtered=True)
                torch.cuda.synchronize(dev)
                t3 = time.perf_counter()
            # link_prediction.py:398-404: both corruption directions of every fact against all N nodes
            flop = 2.0 * len(test) * N * H * 3
            extra.update(rank_500_raw_ms=(t2 - t1) * 1e3, rank_500_filtered_ms=(t3 - t2) * 1e3,
                         rank_raw_tflops=flop / (t2 - t1) / 1e12, mrr_raw=lp.mrr_hits(raw)[0],
                         mrr_filtered=lp.mrr_hits(flt)[0])
        cpu = None
        if args.full and not args.no_cpu_baseline and world == 1:
            try:
                cpu = lp_cpu_baseline(args, sh, train_frac)
            except Exception as e:  # noqa: BLE001
                cpu = {"value": None, "unit": "ms/epoch", "cores": os.cpu_count(), "kind": "port",
                       "sample": "failed: " + str(e)[:200]}
        n_params = sum(p.numel() for p in model.parameters())
        out = {
            "metric": "full-batch R-GCN link-prediction epoch time (ms), fb15k-shaped graph",
            "value": ms_per_step, "unit": "ms", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "higher_is_better": False, "scaling": "strong" if partitioned else "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"fb15k-237-shaped synthetic KG, link prediction (SURVEY §8d config 4), scale {args.scale:g}",
                       "N": N, "R": R, "nnz": g.nnz, "ncols_touched": plan.ncols, "layers": [[0, H]], "num_bases": B,
                       "train_triples": int(ntrain), "negatives": "20 % in-batch, drawn on the device each epoch",
                       "decoder": "DistMult + BCE-with-logits", "value_mode": args.value_mode, "engine": args.engine,
                       "launch": launch, "params": n_params,
                       "parallelism": ("node-partitioned x%d" % world if partitioned else "replicas x%d" % world)
                       if world > 1 else "1 GPU"},
            "roofline": roofline, "cpu_baseline": cpu, "spmm_hbm_gbps": ach,
            "extra": dict(extra, final_loss=float(loss), setup_s=setup_s, plan_device_mb=plan.device_bytes / 2**20,
                          env_switches=_env_switches()),
        }
    if not emit:
        return out
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if out is not None:
        print(json.dumps(out), flush=True)


def partitioned_probe(args, name, dev, world, rank, steps=5, warmup=2, emit=None):
    """--gpus N on a replica workload: ONE graph of the shape node-partitioned over the N ranks (mrgcn_amd.partition:
    reduce-scatter of every layer's output rows, all-gather of their gradients, sharded node table) next to the replica
    line, so that the first multi-GPU run of the driver exercises the partitioned engine on real xGMI links:
    epoch time, the share of it spent in the collectives, and — the parity requirement of SURVEY §8e — the largest
    difference between the N-GPU logits and a single-GPU model holding the same parameters."""
    import torch
    import torch.distributed as dist
    from mrgcn_amd import dist as mdist
    from mrgcn_amd import synth
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.partition import NodePartition, PartitionedRGCN, all_gather_rows, partitioned_train_step
    from mrgcn_amd.train import ClipAdam
    sh = synth.SHAPES[name]
    g = synth.make_graph(name, seed=args.seed, scale=args.scale, value_mode=args.value_mode)
    N, R, B = g.num_nodes, g.num_relations, sh["bases"]
    dims = synth.layer_dims(name)
    featureless = sh["x_width"] == 0
    idx_np, y_np = synth.make_labels(name, N, args.seed, args.scale)
    modules = [(i, o, "mrgcn", torch.nn.ReLU() if li < len(dims) - 1 else None) for li, (i, o) in enumerate(dims)]
    part = NodePartition(N, world, rank)
    torch.manual_seed(args.seed)
    pmodel = PartitionedRGCN(modules, R, N, B, featureless, False, part).to(dev)
    gen = torch.Generator(device=dev).manual_seed(args.seed)   # the same X on every rank
    X = None if featureless else torch.randn((N, sh["x_width"]), device=dev, generator=gen)
    out = {"workload": name, "rccl_world": world, "backend": dist.get_backend(), "N": N, "nnz": g.nnz}
    # parity first (single-GPU graphs only: every rank can hold the whole model): rank 0's full-size model gives the
    # state every rank shards, and the logits to compare with
    if g.nnz <= 40_000_000:
        torch.manual_seed(args.seed)
        full = RGCN(modules, R, N, B, 0.0, featureless, False, False).to(dev)
        state = {k: v for k, v in full.state_dict().items()}
        pmodel.load_full_state(state)
        pmodel.build_plan(g.rows, g.cols, g.vals, dev)
        Xl = None if X is None else part.shard_rows(X)
        with torch.no_grad():
            mine = pmodel(Xl)
            allrows = all_gather_rows(mine.contiguous())[:N]
            if rank == 0:
                A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([g.rows, g.cols])), torch.from_numpy(g.vals),
                                            (N, R * N)).to(dev)
                ref = full(X, A)
                out["logits_maxdiff_vs_single"] = float((allrows - ref).abs().max())
                out["logits_absmax"] = float(ref.abs().max())
                del A, ref
        del full, state, allrows, mine
        torch.cuda.empty_cache()
    else:
        pmodel.sync_replicated()
        pmodel.build_plan(g.rows, g.cols, g.vals, dev)
        Xl = None if X is None else part.shard_rows(X)
    del X
    opt = ClipAdam(pmodel.parameters(), lr=0.01, weight_decay=0.0, max_norm=1.0)
    opt.set_distributed(None, pmodel.sharded_parameters())

    def step():
        return partitioned_train_step(pmodel, Xl, idx_np, y_np, opt)
    for _ in range(warmup):
        step()
    mdist.barrier(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    mdist.barrier(dev)
    out["ms_per_step"] = mdist.max_over_ranks(time.perf_counter() - t0, dev) / steps * 1e3
    out["final_loss"] = float(loss)
    # the collectives of one step timed alone, on buffers of the step's sizes: per layer a reduce-scatter of
    # [Np, out] partial rows (forward) and an all-gather of [S, out] gradient rows (backward)
    from mrgcn_amd.partition import reduce_scatter_rows
    bufs = [(torch.randn((part.Np, o), device=dev), torch.randn((part.S, o), device=dev)) for _, o in dims]
    for _ in range(2):
        for full_rows, own in bufs:
            reduce_scatter_rows(full_rows)
            all_gather_rows(own)
    mdist.barrier(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        for full_rows, own in bufs:
            reduce_scatter_rows(full_rows)
            all_gather_rows(own)
    mdist.barrier(dev)
    out["collective_ms"] = mdist.max_over_ranks(time.perf_counter() - t0, dev) / steps * 1e3
    out["collective_bytes_per_step"] = sum(2 * part.Np * o * 4 for _, o in dims)
    # the forward reduce-scatters alone: what a step cannot avoid — its backward all-gathers move the rows with
    # gradient only (partition._live_row_exchange), a few thousand rows at these label counts
    mdist.barrier(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        for full_rows, _own in bufs:
            reduce_scatter_rows(full_rows)
    mdist.barrier(dev)
    out["reduce_scatter_ms"] = mdist.max_over_ranks(time.perf_counter() - t0, dev) / steps * 1e3
    # the other form of SURVEY §8e: row partition + halo exchange of operand rows (mrgcn_amd.partition_halo).  Which of
    # the two moves fewer bytes is a property of the graph and the rank count (choose_partition: the measured halo);
    # both are timed here, fail-soft, so that the first contact with several GPUs prices both.
    try:
        from mrgcn_amd.partition_halo import HaloPartitionedRGCN, choose_partition, halo_train_step
        ch = choose_partition(g.rows, g.cols, N, world, [o for _, o in dims])
        out["partition_choice"] = {"by_received_bytes_per_forward": ch["choice"], "column_bytes": ch["column"],
                                   "halo_bytes": ch["halo"]}
        torch.manual_seed(args.seed)
        hmodel = HaloPartitionedRGCN(modules, R, N, B, featureless, False, part).to(dev)
        hmodel.load_state_dict(pmodel.state_dict())   # the same shards as the column engine holds now
        hmodel.build_plan(g.rows, g.cols, g.vals, dev)
        with torch.no_grad():
            d = float((hmodel(Xl) - pmodel(Xl)).abs().max())
        out["halo_logits_maxdiff_vs_column_engine"] = mdist.max_over_ranks(d, dev)
        hopt = ClipAdam(hmodel.parameters(), lr=0.01, weight_decay=0.0, max_norm=1.0)
        hopt.set_distributed(None, hmodel.sharded_parameters())
        for _ in range(warmup):
            halo_train_step(hmodel, Xl, idx_np, y_np, hopt)
        mdist.barrier(dev)
        t0 = time.perf_counter()
        for _ in range(steps):
            hl = halo_train_step(hmodel, Xl, idx_np, y_np, hopt)
        mdist.barrier(dev)
        out["halo_ms_per_step"] = mdist.max_over_ranks(time.perf_counter() - t0, dev) / steps * 1e3
        out["halo_final_loss"] = float(hl)
        out["halo_columns_this_rank"] = hmodel.plans.halo_columns
        del hmodel, hopt
        torch.cuda.empty_cache()
    except Exception as e:  # noqa: BLE001  (informational: the column engine's record stands)
        out["halo_error"] = (type(e).__name__ + ": " + str(e))[:300]
    if emit is not None:
        emit(out)   # the eager record is safe (printed) before anything below can go wrong
    # the same step captured into a hipGraph, RCCL collectives included (partition.GraphedPartitionedStep): at 8 ranks a
    # rank's share of the graph is launch-latency territory.  Exercised with one rank only so far, hence after the
    # eager record and fail-soft; MRGCN_BENCH_PROBE_GRAPH=0 skips it.
    if dist.get_backend() == "nccl" and os.environ.get("MRGCN_BENCH_PROBE_GRAPH", "1") != "0":
        try:
            from mrgcn_amd.partition import GraphedPartitionedStep
            opt2 = ClipAdam(pmodel.parameters(), lr=0.01, weight_decay=0.0, max_norm=1.0, capturable=True)
            opt2.set_distributed(None, pmodel.sharded_parameters())
            graphed = GraphedPartitionedStep(pmodel, Xl, idx_np, y_np, opt2, warmup=2)
            for _ in range(warmup):
                graphed()
            mdist.barrier(dev)
            t0 = time.perf_counter()
            for _ in range(steps):
                loss = graphed()
            mdist.barrier(dev)
            out["ms_per_step_hipgraph"] = mdist.max_over_ranks(time.perf_counter() - t0, dev) / steps * 1e3
            out["final_loss_hipgraph"] = float(loss)
        except Exception as e:  # noqa: BLE001
            out["hipgraph_error"] = (type(e).__name__ + ": " + str(e))[:200]
    return out


def run_probe_child(args, workload, k, world, rank, local_rank, limit=None):
    """Runs `partitioned_probe` in a CHILD process per rank, with a process group of its own (the parent's rendezvous
    port + 1 + k): whatever happens in there — an RCCL failure, a rank that runs out of memory while the others wait
    in a collective — ends with the child (killed after a time limit at the latest) and leaves the parent, its
    process group and the replica line untouched.  Rank 0 returns the child's record (or the error), the others None."""
    import subprocess
    port = int(os.environ.get("MASTER_PORT", "29500")) + 1 + k
    # (none of the elastic agent's variables: with TORCHELASTIC_USE_AGENT_STORE the child's env:// rendezvous would wait
    # for a store the agent hosts on the PARENT's port — rank 0 of the child group hosts its own on port + 1 + k)
    env = {k_: v for k_, v in os.environ.items() if not k_.startswith("TORCHELASTIC")}
    env.update(MASTER_ADDR=os.environ.get("MASTER_ADDR", "127.0.0.1"), MASTER_PORT=str(port), RANK=str(rank),
               LOCAL_RANK=str(local_rank), WORLD_SIZE=str(world), LOCAL_WORLD_SIZE=str(world), GROUP_RANK="0",
               ROLE_RANK=str(rank))
    cmd = [sys.executable, os.path.abspath(__file__), "--probe-child", workload, "--gpus", str(world),
           "--seed", str(args.seed), "--value-mode", args.value_mode,
           "--scale", str(args.scale if workload == args.workload else 1.0)]
    if limit is None:
        limit = float(os.environ.get("MRGCN_BENCH_PROBE_TIMEOUT", "420" if workload == "synth10m" else "240"))
    def last_record(text):
        for line in reversed((text or "").strip().splitlines()):
            if line.startswith("{"):
                try:
                    return json.loads(line)
                except Exception:  # noqa: BLE001
                    return None
        return None

    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired as e:
        if rank != 0:
            return None
        so = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else e.stdout
        rec = last_record(so)   # (the eager record is printed before the captured attempt: a hang there loses only that)
        if rec is not None:
            rec["note"] = "timed out after %.0f s behind this record" % limit
            return rec
        return {"error": "timed out after %.0f s" % limit, "rccl_world": world}
    if rank != 0:
        return None
    rec = last_record(r.stdout)
    if rec is not None:
        return rec
    return {"error": ("exit %d: " % r.returncode) + (r.stderr.strip().splitlines() or ["no output"])[-1][:300],
            "rccl_world": world}


def probe_child_main(args):
    import torch
    import torch.distributed as dist
    from mrgcn_amd import dist as mdist
    world, rank, local_rank = mdist.env_world()
    ngpu = max(torch.cuda.device_count(), 1)
    dev = torch.device("cuda", local_rank % ngpu)
    torch.cuda.set_device(dev)
    backend = os.environ.get("MRGCN_DIST_BACKEND", "nccl" if ngpu >= world else "gloo")
    mdist.init(backend, dev if backend == "nccl" else None)
    if world == 1 and not dist.is_initialized():   # (a one-rank group: the probe run by hand on a one-GPU box)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29555")
        dist.init_process_group(backend, rank=0, world_size=1)

    def emit(rec_):
        if rank == 0:
            print(json.dumps(rec_), flush=True)
    try:
        rec = partitioned_probe(args, args.probe_child, dev, world, rank, emit=emit)
    except Exception as e:  # noqa: BLE001
        rec = {"error": (type(e).__name__ + ": " + str(e))[:300], "rccl_world": world}
    if rank == 0:
        print(json.dumps(rec), flush=True)
    try:
        if "error" not in rec:
            dist.barrier()
            dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        pass


def cpu_quota():
    from mrgcn_amd.host import cpu_quota as q
    return q()


def main():
    args = parse()
    # The bench boxes give this container a CPU quota (cgroup cpu.max: 16 CPUs of a 256-thread host).  torch's intra-op
    # pool defaults to one thread per host thread: every parallel CPU op then wakes 256 spinning workers, the quota of
    # the 100 ms period is gone in a few ms and the kernel parks the WHOLE process for the rest of it — found as 35-60 ms
    # stalls in every second or third eager step of the encoders workload (one `torch.arange(N)` per forward, since
    # removed).  The pool is sized to the quota (mrgcn_amd.host); `cpu_baseline` runs its own thread sweep.
    from mrgcn_amd.host import fit_cpu_pool_to_quota
    fit_cpu_pool_to_quota()
    if args.probe_child:
        return probe_child_main(args)
    if args.workload == "fb15k":
        return main_lp(args)
    import torch
    import torch.distributed as dist
    from mrgcn_amd import dist as mdist

    world, rank, local_rank = mdist.env_world()
    ngpu = max(torch.cuda.device_count(), 1)
    dev = torch.device("cuda", (local_rank % ngpu) if world > 1 else 0)
    torch.cuda.set_device(dev)
    # one process per GPU over RCCL; with fewer GPUs than ranks (functional tests on a 1-GPU box)
    # the ranks share a device and talk over gloo
    backend = os.environ.get("MRGCN_DIST_BACKEND", "nccl" if ngpu >= world else "gloo")
    mdist.init(backend, dev if backend == "nccl" else None)  # no-op at world 1

    from mrgcn_amd import _lib as L
    from mrgcn_amd import synth
    from mrgcn_amd.train import ClipAdam

    name = args.workload
    sh = synth.SHAPES[name]
    if args.partition is None:
        args.partition = name in PARTITIONED_WORKLOADS
    partitioned = args.partition and world > 1

    def barrier():
        mdist.barrier(dev)

    graph_used = False
    live = {}   # the headline's model, plan and inputs: the extras run on them until a leg needs the memory

    def drop_live():
        import gc
        live.clear()
        gc.collect()
        torch.cuda.empty_cache()

    if not partitioned:
        # the headline: N > 1 runs N replicas of it
        live = nc_workload(args, name, dev, keep=True)
        step = live.pop("step")
        g, idx_np, y_np, modules = live["g"], live["idx_np"], live["y_np"], live["modules"]
        N, R, B, dims, featureless = live["N"], live["R"], live["B"], live["dims"], live["featureless"]
        graph_used, setup_s = live["graph_used"], live["setup_s"]
    else:
        # strong scaling: rank g owns node range g, its weight_I rows / Adam state and its columns of A; only
        # the rank's shard of the model and of the plan is ever built
        from mrgcn_amd.partition import NodePartition, PartitionedRGCN, partitioned_train_step
        t0 = time.time()
        g = synth.make_graph(name, seed=args.seed, scale=args.scale, value_mode=args.value_mode)
        N, R, B = g.num_nodes, g.num_relations, sh["bases"]
        dims = synth.layer_dims(name)
        featureless = sh["x_width"] == 0
        idx_np, y_np = synth.make_labels(name, N, args.seed, args.scale)
        torch.manual_seed(args.seed)
        modules = [(i, o, "mrgcn", torch.nn.ReLU() if li < len(dims) - 1 else None)
                   for li, (i, o) in enumerate(dims)]
        part = NodePartition(N, world, rank)
        pmodel = PartitionedRGCN(modules, R, N, B, featureless, False, part).to(dev)
        pmodel.sync_replicated()
        live["plan"] = pmodel.build_plan(g.rows, g.cols, g.vals, dev)
        Xl = None if featureless else part.shard_rows(torch.randn((N, sh["x_width"]), device=dev))
        popt = ClipAdam(pmodel.parameters(), lr=0.01, weight_decay=0.0, max_norm=1.0)
        popt.set_distributed(None, pmodel.sharded_parameters())
        live["model"] = pmodel

        def step():
            return partitioned_train_step(pmodel, Xl, idx_np, y_np, popt)
        if (os.environ.get("MRGCN_PARTITION_GRAPH") == "1" and args.graph and torch.distributed.get_backend() == "nccl"):
            # opt-in: the partitioned step, collectives included, replayed from a hipGraph (exercised with one rank only)
            from mrgcn_amd.partition import GraphedPartitionedStep
            popt = ClipAdam(pmodel.parameters(), lr=0.01, weight_decay=0.0, max_norm=1.0, capturable=True)
            popt.set_distributed(None, pmodel.sharded_parameters())
            graphed = GraphedPartitionedStep(pmodel, Xl, idx_np, y_np, popt, warmup=max(args.warmup, 1))
            graph_used = True

            def step():  # noqa: F811
                return graphed()
        setup_s = time.time() - t0
    for _ in range(args.warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    barrier()
    dt = mdist.max_over_ranks(time.perf_counter() - t0, dev)  # replicas: the slowest rank's time
    ms_per_step = dt / args.steps * 1e3
    final_loss = float(loss)
    if args.dump_outputs and rank == 0:   # (before --full's legs: some of them train the live model further)
        dump_outputs(args.dump_outputs, loss, live["model"].named_parameters())

    def measure_roofline():
        # ---- roofline of the dominant sparse kernel: the stacked-CSR SpMM of layer 0 ----
        plan_, F_ = live["plan"], dims[0][1]
        rf = spmm_roofline(plan_, F_, args.operand if not partitioned else "f32", args.spmm_iters, dev, name, args.scale)
        if len(dims) > 1 and dims[1][1] != F_ and dims[1][1] <= 16:
            # the epoch launches this product once per layer: both widths are timed and the LOWER fraction is the
            # line's `roofline` (the other one stays beside it)
            other = spmm_roofline(plan_, dims[1][1], args.operand if not partitioned else "f32", args.spmm_iters, dev,
                                  name, args.scale, pmc_ok=False)
            lo, hi = (rf, other) if rf["frac"] <= other["frac"] else (other, rf)
            lo = dict(lo)
            lo["other_width"] = {k: hi[k] for k in ("kernel", "frac", "achieved", "avg_ms", "algorithmic_bytes")}
            if lo["traffic"] is None and hi.get("traffic") is not None:
                lo["traffic_other_width"] = hi["traffic"]
            rf = lo
        return rf
    # (with several ranks the replica's model is dropped before the big partition probe: rank 0 measures first)
    early_roofline = measure_roofline() if (args.full and rank == 0 and world > 1 and "plan" in live) else None
    if world > 1:
        barrier()

    # --gpus N on a replica workload: the node-partitioned engine on the same graph (and on the 10 M-node graph),
    # every rank takes part; a failure (RCCL, memory) leaves its message and the replica line still prints
    part_records = None
    if args.full and world > 1 and not partitioned and os.environ.get("MRGCN_BENCH_PARTITION_PROBE", "1") != "0":
        part_records = {}
        probes = [name] + (["synth10m"] if name == "am" and args.scale == 1.0 else [])
        # the probes share ONE time budget (what a hung first contact with a multi-GPU node may add to the run: the
        # replica line must still leave before whoever launched this gives up); every rank takes the same decision
        # (the slowest rank's clock)
        budget = float(os.environ.get("MRGCN_BENCH_PROBE_BUDGET", "420"))
        t_probe = time.perf_counter()
        for k, wl in enumerate(probes):
            spent = mdist.max_over_ranks(time.perf_counter() - t_probe, dev)
            own = float(os.environ.get("MRGCN_BENCH_PROBE_TIMEOUT", "420" if wl == "synth10m" else "240"))
            limit = min(own, budget - spent)
            if limit < 90.0:
                part_records[wl] = {"skipped": "%.0f s of the probes' %.0f s budget left" % (budget - spent, budget)}
                continue
            if wl != name:   # drop the replica's model first: the big graph wants the memory
                step = None
                drop_live()
            part_records[wl] = run_probe_child(args, wl, k, world, rank, local_rank, limit=limit)
            barrier()

    out = None
    if rank == 0:
        extra = {}
        F = dims[0][1]
        have_model = "plan" in live
        plan, model = live.get("plan"), live.get("model")
        A, X, idx, tgt = live.get("A"), live.get("X"), live.get("idx"), live.get("tgt")
        if early_roofline is not None:
            roofline = early_roofline
        elif have_model and args.full:
            roofline = measure_roofline()
        else:
            roofline = None
        ach = roofline["achieved"] if roofline else None
        stream = torch.cuda.current_stream(dev).cuda_stream
        if have_model and world == 1 and args.full:
            bytes_alg_f32 = plan.spmm_bytes(F)
            dY = torch.randn((plan.num_rows, F), device=dev)
            dM = torch.empty((plan.ncols, (F + 3) // 4 * 4), device=dev)
            t_t = event_time_ms(lambda: plan.spmm(L.VIEW_TRANSPOSED, dY, F=F, out=dM), args.spmm_iters, stream)
            extra["spmm_transposed_ms"] = t_t
            extra["spmm_transposed_gbps"] = bytes_alg_f32 / (t_t * 1e-3) / 1e9
            # what the memory system's line size allows these two views (algorithmic bytes per second if every access
            # ran at the 8 TB/s peak): the TRANSPOSED product gathers one dY row per ENTRY (13.6 M random 40-byte rows of
            # a 67 MB table: a 128-byte line each), the LITERAL product one operand row per touched column out of the
            # reference's (R*N) x F table (17.8 GB: every row its own line).  Index / value streams and the output as
            # in SURVEY 8(d)'s formula.
            line = 128
            t_min_T = (plan.nnz * (8 + line) + (plan.ncols + 1) * 4 + plan.ncols * F * 4) / (HBM_PEAK_GBS * 1e9)
            t_min_L = (plan.nnz * 8 + (plan.num_rows + 1) * 4 + plan.ncols * line + plan.num_rows * F * 4) / (HBM_PEAK_GBS * 1e9)
            extra["spmm_transposed_bound_gbps"] = bytes_alg_f32 / t_min_T / 1e9
            extra["spmm_literal_bound_gbps"] = bytes_alg_f32 / t_min_L / 1e9
            del dY, dM
            ab = epoch_algorithmic_bytes(plan, dims, B, R, N, args.operand)
            if ab:
                extra["epoch_algorithmic_bytes"] = ab["total"]
                extra["epoch_algorithmic_bytes_parts"] = {k: ab[k] for k in ("forward", "backward", "adam")}
                extra["epoch_frac"] = ab["total"] / (ms_per_step * 1e-3) / (HBM_PEAK_GBS * 1e9)
                extra["gradient_support"] = {k: ab[k] for k in ("live_cols", "live_nodes", "live_entries")}
            if roofline is not None and not featureless and len(dims) == 2 and max(d[1] for d in dims) <= 16:
                try:   # the same product timed INSIDE epochs (behind its producer), both widths
                    ie = spmm_in_epoch(live, dims, args.operand, dev)
                    roofline["in_epoch"] = ie
                    roofline["in_epoch_frac"] = min(v["frac"] for v in ie.values()) if ie else None
                except Exception as e:  # noqa: BLE001  (a measurement beside the line's own)
                    roofline["in_epoch_error"] = (type(e).__name__ + ": " + str(e))[:200]
            if args.renumbered_extra and not args.reorder and plan.nnz <= 40_000_000:
                try:
                    extra["epoch_ms_nodes_renumbered"] = renumbered_epoch_ms(
                        args, g, idx_np, y_np, dims, modules, R, N, B, featureless, sh["x_width"], dev)
                except Exception as e:  # noqa: BLE001  (informational leg only)
                    extra["epoch_ms_nodes_renumbered_error"] = str(e)[:200]
            if args.reference_loop and plan.nnz <= 40_000_000:
                for kind, key in (("train_step", "epoch_ms_eager"), ("fast", "epoch_ms_reference_loop"),
                                  ("torch", "epoch_ms_reference_loop_torch_optim"),
                                  ("train_step_dense", "epoch_ms_dense_path")):
                    try:
                        extra[key] = reference_loop_ms(args, kind, A, X, idx, tgt, modules, R, N, B, featureless, dev)
                    except Exception as e:  # noqa: BLE001  (informational leg only)
                        extra[key + "_error"] = str(e)[:200]
                    torch.cuda.empty_cache()
            if args.reference_loop and not featureless and plan.nnz <= 40_000_000 and not plan.lean:
                try:
                    extra["labelled_nodes_as_one_batch"] = labelled_batch_epoch_ms(
                        args, plan, X, idx_np, y_np, modules, R, N, B, featureless, dev)
                except Exception as e:  # noqa: BLE001  (informational leg only)
                    extra["labelled_nodes_as_one_batch"] = {"error": (type(e).__name__ + ": " + str(e))[:200]}
                torch.cuda.empty_cache()
            if not args.no_literal_spmm:
                try:  # the reference's own operand layout: dense (R*N) x F, 17.8 GB at AM scale
                    D = torch.randn((R * plan.num_nodes, F), device=dev)
                    Yl = torch.empty((plan.num_rows, F), device=dev)
                    t_l = event_time_ms(lambda: plan.spmm(L.VIEW_LITERAL, D, out=Yl), args.spmm_iters, stream)
                    extra["spmm_literal_ms"] = t_l
                    extra["spmm_literal_gbps"] = bytes_alg_f32 / (t_l * 1e-3) / 1e9
                    del D, Yl
                except Exception as e:  # noqa: BLE001
                    extra["spmm_literal_error"] = str(e)[:200]
        # the roofline denominator next to what a plain device copy reaches on this
        # box, and the bytes the parameter tail of an epoch has to move
        if args.full:
            src = torch.empty(1 << 28, dtype=torch.float32, device=dev)  # 1 GiB
            dst = torch.empty_like(src)
            t_cp = event_time_ms(lambda: dst.copy_(src), 5, stream)
            extra["device_copy_gbps"] = 2 * src.numel() * 4 / (t_cp * 1e-3) / 1e9  # read + write
            # the same as hand-written kernels of this library, ONE-SHOT grids: a float4 copy and a 3-read / 3-write pass (Adam's
            # shape) — the yardsticks the streaming kernels of the epoch are held against
            lib_ = L.load()
            t_cp = event_time_ms(lambda: L.check(lib_.mrgcn_probe_copy_f32(src.data_ptr(), dst.data_ptr(), src.numel(), stream),
                                                 "mrgcn_probe_copy_f32"), 5, stream)
            extra["device_copy_gbps_hip"] = 2 * src.numel() * 4 / (t_cp * 1e-3) / 1e9
            third = torch.zeros_like(src)
            t_tr = event_time_ms(lambda: L.check(lib_.mrgcn_probe_triad_f32(src.data_ptr(), dst.data_ptr(), third.data_ptr(),
                                                                           src.numel(), stream), "mrgcn_probe_triad_f32"), 5, stream)
            extra["triad_gbps"] = 6 * src.numel() * 4 / (t_tr * 1e-3) / 1e9
            # the same two as persistent grid-stride loops (round 5's yardsticks): the shape of a kernel with per-block state
            t_cp = event_time_ms(lambda: L.check(lib_.mrgcn_probe_copy_persistent_f32(src.data_ptr(), dst.data_ptr(), src.numel(), stream),
                                                 "mrgcn_probe_copy_persistent_f32"), 5, stream)
            extra["device_copy_gbps_hip_persistent"] = 2 * src.numel() * 4 / (t_cp * 1e-3) / 1e9
            t_tr = event_time_ms(lambda: L.check(lib_.mrgcn_probe_triad_persistent_f32(src.data_ptr(), dst.data_ptr(), third.data_ptr(),
                                                                                      src.numel(), stream), "mrgcn_probe_triad_persistent_f32"), 5, stream)
            extra["triad_gbps_persistent"] = 6 * src.numel() * 4 / (t_tr * 1e-3) / 1e9
            del src, dst, third
        if have_model:
            n_params = sum(p.numel() for p in model.parameters())
            extra["param_bytes"] = 4 * n_params * (1 + 1 + 6)  # grad write, clip read, Adam 3 reads + 3 writes
            extra.update(plan_device_mb=plan.device_bytes / 2**20, long_rows=plan.long_rows,
                         long_cols=plan.long_cols, max_row_nnz=plan.max_row_nnz)
            nnz, ncols = plan.nnz, plan.ncols
        else:
            n_params, nnz, ncols = None, g.nnz, None
        if part_records is not None:
            extra["partitioned"] = part_records
        torch.cuda.synchronize(dev)
        # seeds 0-2 (report the median): the headline is the seed of --seed, the others run the same
        # K steps on their own graph / labels / parameters
        if (args.full and world == 1 and name == "am" and args.scale == 1.0 and args.seeds and not partitioned):
            seeds = {str(args.seed): ms_per_step}
            import gc
            step = plan = model = A = X = idx = tgt = None
            drop_live()
            for sd in (0, 1, 2):
                if str(sd) in seeds:
                    continue
                try:
                    r2 = nc_workload(args, name, dev, seed=sd, steps=args.steps, warmup=args.warmup)
                    seeds[str(sd)] = r2["ms_per_step"]
                    del r2
                except Exception as e:  # noqa: BLE001
                    seeds[str(sd)] = None
                    extra["seeds_error"] = str(e)[:200]
                gc.collect()
                torch.cuda.empty_cache()
            vals = sorted(v for v in seeds.values() if v is not None)
            extra["seeds_ms_per_step"] = seeds
            extra["seeds_median_ms"] = vals[len(vals) // 2] if vals else None
        if args.full and world == 1 and name == "am" and args.scale == 1.0 and args.side_workloads and not partitioned:
            step = plan = model = A = X = idx = tgt = None
            drop_live()
            extra["workloads"] = side_workloads(args, dev)
            try:  # (fail-soft like the side workloads)
                extra["minibatch"] = minibatch_record(args, dev)
            except Exception as e:  # noqa: BLE001
                extra["minibatch"] = {"error": (type(e).__name__ + ": " + str(e))[:300]}
            gc.collect()
            torch.cuda.empty_cache()
        cpu = None
        if args.full and not args.no_cpu_baseline and world == 1:
            try:
                cpu = cpu_baseline(args, name)
            except Exception as e:  # noqa: BLE001
                cpu = {"value": None, "unit": "ms/epoch", "cores": os.cpu_count(), "kind": "port",
                       "sample": "failed: " + str(e)[:200]}
        # "seeds 0,1,2; report median" — when the line ran the three seeds (the default AM run), `value` and
        # `ms_per_step` are their median; the timed region of THIS process's seed stays beside it
        extra["ms_per_step_this_seed"] = ms_per_step
        headline_ms = extra.get("seeds_median_ms") or ms_per_step
        out = {
            "metric": "full-batch R-GCN epoch time (ms), AM-shaped graph" if name == "am" else
                      "full-batch R-GCN epoch time (ms), %s-shaped graph" % name,
            "value": headline_ms, "unit": "ms", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": headline_ms, "higher_is_better": False,
            "scaling": "strong" if partitioned else "weak", "vs_baseline": None, "dtype": "f32",
            "data": "synthetic",
            "config": {"workload": f"{name}-shaped synthetic KG (SURVEY §8d), scale {args.scale:g}",
                       "N": N, "R": R, "nnz": nnz, "ncols_touched": ncols,
                       "layers": dims, "num_bases": B, "value_mode": args.value_mode,
                       "engine": args.engine, "operand": args.operand, "weight_I": "node-major (N, B, out); row-sparse gradient + Adam",
                       "node_order": "label reach first" if args.reorder else "generator (random)",
                       "launch": "hipGraph replay" if graph_used else "eager", "labelled": int(len(idx_np)), "params": n_params,
                       "seed": args.seed,
                       "parallelism": ("node-partitioned x%d" % world if partitioned else
                                       "replicas x%d" % world) if world > 1 else "1 GPU"},
            "roofline": roofline,
            "cpu_baseline": cpu,
            "spmm_hbm_gbps": ach,
            "extra": dict(extra, final_loss=final_loss, setup_s=setup_s, env_switches=_env_switches()),
        }
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if out is not None:
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
