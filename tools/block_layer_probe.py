"""What a block-diagonal hidden layer (Schlichtkrull et al. 2018, eq. 4; csrc/block_xform.hip) costs at the shape
`bench.py --workload fb15k` builds (synthetic graph of the FB15k-237 shape: 14 541 nodes, 475 relations), 200 -> 200
with 40 blocks of 5 x 5:

  xform_fwd / spmm_compact / spmm_transposed / xform_dx / xform_dw
             the five passes of the layer, each timed on its own through the C ABI
  layer.fused / layer.literal
             forward + backward of the one layer (loss = sum of Y . G) on the fused engine and on the only route the
             layer had before — the literal engine on the same weights expanded by `block_weight_dense` — with the
             peak device memory of each (torch's allocator, above what was allocated before the call)
  epoch.two_layer / epoch.one_layer / epoch.one_layer_again
             the replayed full-batch training epoch of `fit` with the default decoder: the 2-basis node table followed
             by the block layer, beside the one-layer encoder of the bench, which is measured again at the end (the
             spread between like rows on this box)

Every figure is the median of `--reps` synchronised, event-timed calls after `--warm` warm-ups, with their range.
Writes profiles/block_layer_probe.json.

    python tools/block_layer_probe.py [--out profiles/block_layer_probe.json] [--no-literal]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = F = 200
NB = 40


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
    from mrgcn_amd import synth
    sh = synth.SHAPES["fb15k"]
    g = synth.make_graph("fb15k", seed=seed)
    N, R = g.num_nodes, g.num_relations
    perm = np.random.RandomState(seed).permutation(len(g.triples))
    ntrain = int(272115 / 310116 * len(g.triples))
    tr = np.asarray(g.triples, dtype=np.int64)
    A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([g.rows, g.cols])), torch.from_numpy(g.vals),
                                (N, R * N)).cuda()
    return dict(N=N, R=R, H=sh["hidden"], B=sh["bases"], A=A, train=torch.from_numpy(tr[perm[:ntrain]]).cuda())


def _passes(s, args, show):
    """The five passes through the C ABI on fixed buffers."""
    from mrgcn_amd import _lib as L
    from mrgcn_amd.plan import plan_of
    lib = L.load()
    N, R = s["N"], s["R"]
    plan = plan_of(s["A"], N, R, operand_row_bytes=[4 * F])
    g = torch.Generator(device="cuda").manual_seed(0)
    X = torch.randn((N, K), device="cuda", generator=g)
    W = torch.randn((R, NB, K // NB, F // NB), device="cuda", generator=g) * 0.3
    dY = torch.randn((N, F), device="cuda", generator=g)
    M = torch.empty((plan.nop, F), device="cuda")
    dM = torch.empty((plan.ncols, F), device="cuda")
    dX, dW = torch.empty((N, K), device="cuda"), torch.empty_like(W)
    nws = int(lib.mrgcn_block_transform_bwd_workspace(plan.handle, K, F, NB, 1, 1))
    ws = torch.empty((max(nws, 1),), device="cuda")
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731

    def fwd():
        L.check(lib.mrgcn_block_transform_fwd_f32(plan.handle, p(X), K, K, p(W), NB, F, p(M), F, 1, st()), "fwd")

    def bwd(want_dx, want_dw):
        L.check(lib.mrgcn_block_transform_bwd_f32(plan.handle, p(dM), F, p(X), K, K, p(W), NB, F,
                                                  p(dX) if want_dx else None, K, p(dW) if want_dw else None, p(ws), nws,
                                                  st()), "bwd")

    show("xform_fwd", _timed(fwd, args.reps, args.warm))
    plan.replicate(M)
    show("spmm_compact", _timed(lambda: plan.spmm(L.VIEW_COMPACT, M, F=F), args.reps, args.warm))
    show("spmm_transposed", _timed(lambda: plan.spmm(L.VIEW_TRANSPOSED, dY, F=F, out=dM), args.reps, args.warm))
    show("xform_dx", _timed(lambda: bwd(True, False), args.reps, args.warm))
    show("xform_dw", _timed(lambda: bwd(False, True), args.reps, args.warm))
    return dict(ncols=plan.ncols, nnz=plan.nnz, operand_rows=plan.nop, dw_workspace_bytes=4 * nws,
                weight_bytes=4 * W.numel(), dense_weight_bytes=4 * R * K * F, literal_operand_bytes=4 * R * N * F)


def _layer(s, engine, args):
    """Forward + backward of the one layer on `engine`, with the peak memory above the starting level."""
    from mrgcn_amd.layers.graph import GraphConvolution
    torch.manual_seed(0)
    layer = GraphConvolution(K, F, s["R"], s["N"], bias=False, num_blocks=NB).cuda()
    layer.engine = engine
    g = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn((s["N"], K), device="cuda", generator=g).requires_grad_(True)
    G = torch.randn((s["N"], F), device="cuda", generator=g)

    def step():
        layer.zero_grad(set_to_none=True)
        X.grad = None
        (layer(X, s["A"]) * G).sum().backward()

    step()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    row = _timed(step, args.reps if engine == "fused" else max(args.reps // 4, 3), args.warm if engine == "fused" else 1)
    row["peak_bytes_above_start"] = int(torch.cuda.max_memory_allocated() - base)
    del layer, X, G
    torch.cuda.empty_cache()
    return row


def _epoch(s, two_layers, args):
    """The replayed training epoch of `fit` on a fresh model."""
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.plan import plan_of
    from mrgcn_amd.tasks import link_prediction as lp
    from mrgcn_amd.train import ClipAdam
    torch.manual_seed(0)
    mods = [(0, s["H"], "mrgcn", torch.nn.ReLU())]
    if two_layers:
        mods.append((s["H"], F, "mrgcn", None))
    model = RGCN(mods, s["R"], s["N"], s["B"], 0.0, True, False, True, num_blocks=NB if two_layers else -1).cuda()
    opt = ClipAdam(model.parameters(), lr=0.01, weight_decay=0.0, max_norm=1.0, capturable=True)
    plan = plan_of(s["A"], s["N"], s["R"], operand_row_bytes=model.operand_row_bytes())   # noqa: F841
    tparts = lp.FactParts(s["train"][:2000], 0, filtered=False)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    run = lp.FitEpochs(model, lambda: model(None, s["A"]), tparts, None, opt, graphed=True, warmup=3)
    row = _timed(run.train_epoch, args.reps, args.warm)
    row["peak_bytes_above_start"] = int(torch.cuda.max_memory_allocated() - base)
    del run, model, opt
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_layer_probe.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--no-literal", action="store_true", help="skip the literal route (its operand is 5.5 GB)")
    args = ap.parse_args()
    from mrgcn_amd.host import fit_cpu_pool_to_quota
    fit_cpu_pool_to_quota()
    s = _setup()
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warm=args.warm, N=s["N"], R=s["R"], K=K, F=F, NB=NB,
               train_facts=int(s["train"].shape[0]), rows={})
    rows = out["rows"]

    def show(name, row):
        rows[name] = row
        print(name, json.dumps(row), flush=True)

    out.update(_passes(s, args, show))
    show("layer.fused", _layer(s, "fused", args))
    if not args.no_literal:
        show("layer.literal", _layer(s, "literal", args))
    show("epoch.one_layer", _epoch(s, False, args))
    show("epoch.two_layer", _epoch(s, True, args))
    show("epoch.one_layer_again", _epoch(s, False, args))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
