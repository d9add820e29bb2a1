"""What the 1-vs-all softmax decoder (csrc/lp_all.hip) costs at the FB15k-237 shape (synthetic graph of that shape,
bench.py's split and model: 14 541 nodes, H = 200):

  decoder    `all_loss` forward and backward on fixed embeddings at n = 4 096, 32 768 and all 272 115 training facts
             (m = 2 n queries), the three kernels alone through the C entries with their achieved TFLOP/s (2 m N H per
             product: one in the forward, two in each backward kernel), and `F.cross_entropy(Q @ E.T, target)` on the
             materialised matrix in the same run wherever it fits (where it does not, the row says so)
  epoch      the replayed full-batch training epoch of `fit` (`FitEpochs.train_epoch`, one captured hipGraph) with
             decoder="all" against decoder="grouped" at 10 keyed negatives per fact (BCE and softmax)
  batch_step the median mini-batch's `train_batch_step` (batches of mkbatches(32, 500)): decoder="all" against the flat
             decoder's default

Every figure is the median of `--reps` synchronised, event-timed calls after `--warm` warm-ups, with their range.  Every
leg runs in a child process of its own under its own time limit (`--leg-limit` seconds); a leg that fails or runs out of
time leaves {"failed": ...} in its place.  Writes profiles/lp_all_probe.json.

    python tools/lp_all_probe.py [--out profiles/lp_all_probe.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ["decoder_n4096", "decoder_n32768", "decoder_n272115", "epoch", "batch_step"]


def _timed(fn, reps, warm):
    import torch
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


def _decoder(n, args):
    import torch
    import torch.nn.functional as F
    from mrgcn_amd import _lib
    from mrgcn_amd.tasks import link_prediction as lp
    from tools.lp_grouped_probe import _setup
    s = _setup()
    N, H = s["N"], s["H"]
    g = torch.Generator().manual_seed(0)
    E = (0.1 * torch.randn(N, H, generator=g)).cuda().requires_grad_()
    Rel = (0.1 * torch.randn(s["R"], H, generator=g)).cuda().requires_grad_()
    facts = s["train"][:n].contiguous()
    n = int(facts.shape[0])
    m = 2 * n
    out = dict(facts=n, queries=m, nodes=N, H=H, product_tflop=2.0 * m * N * H / 1e12)
    out["all_loss_forward"] = _timed(lambda: lp.all_loss(facts, E, Rel), args.reps, args.warm)
    loss = lp.all_loss(facts, E, Rel)
    out["all_loss_backward"] = _timed(lambda: torch.autograd.grad(loss, [E, Rel], retain_graph=True), args.reps,
                                      args.warm)
    del loss
    # the kernels alone
    lib = _lib.load()
    with torch.no_grad():
        Q, tg = lp.pair_vectors(facts, E, Rel)
        Q, Ed = Q.contiguous(), E.detach()
    lse, xt = torch.empty(2 * m, device="cuda"), torch.empty(m, device="cuda")
    one = torch.ones(1, device="cuda")
    loss_t = torch.empty((), device="cuda")
    nws = int(lib.mrgcn_lp_all_workspace(m, N, H))
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    dQ, dE = torch.empty_like(Q), torch.empty_like(Ed)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)    # noqa: E731

    def fwd():
        _lib.check(lib.mrgcn_lp_all_fwd_f32(p(Q), H, m, p(Ed), H, N, H, p(tg), p(lse), p(xt), p(loss_t), p(ws), nws,
                                            st()))

    def bwd(a, b):
        _lib.check(lib.mrgcn_lp_all_bwd_f32(p(Q), H, m, p(Ed), H, N, H, p(tg), p(lse), p(one), p(a), H, p(b), H, None, 0,
                                            st()))
    for name, fn, products in (("kernel_forward", fwd, 1), ("kernel_dQ", lambda: bwd(dQ, None), 2),
                               ("kernel_dE", lambda: bwd(None, dE), 2)):
        row = _timed(fn, args.reps, args.warm)
        row["tflops"] = products * out["product_tflop"] / (row["median_ms"] / 1e3)
        out[name] = row
    del dQ, dE, ws
    # the materialised route, where it fits
    try:
        def torch_fwd():
            return F.cross_entropy(Q.detach() @ Ed.t(), tg)
        out["torch_forward"] = _timed(torch_fwd, args.reps, args.warm)
        Qg = Q.detach().requires_grad_()
        Eg = Ed.clone().requires_grad_()

        def torch_both():
            torch.autograd.grad(F.cross_entropy(Qg @ Eg.t(), tg), [Qg, Eg])
        row = _timed(torch_both, args.reps, args.warm)
        out["torch_forward_and_backward"] = row
        out["torch_matrix_gb"] = 4.0 * m * N / 1e9
    except RuntimeError as e:
        if "out of memory" not in str(e).lower():
            raise
        out["torch_does_not_fit"] = dict(matrix_gb=4.0 * m * N / 1e9, error=str(e).splitlines()[0][:200])
    return out


def _epochs(args):
    import torch
    from mrgcn_amd.tasks import link_prediction as lp
    from tools.lp_grouped_probe import _model, _sampler, _setup
    s = _setup()
    out = {}
    for name, kw in (("all", dict(decoder="all", loss="softmax")), ("grouped_rate10", dict(decoder="grouped")),
                     ("grouped_rate10_softmax", dict(decoder="grouped", loss="softmax")),
                     ("all_again", dict(decoder="all", loss="softmax"))):
        model, opt = _model(s)
        plan = s["plan_of"](model)   # noqa: F841  (kept alive with the run, as the bench does)
        sampler = _sampler(s, 10)
        tparts = lp.FactParts(s["train"][:2000], 0, filtered=False)
        run = lp.FitEpochs(model, lambda: model(None, s["A"]), tparts, None, opt, graphed=True, sampler=sampler,
                           warmup=3, **kw)
        out[name] = _timed(run.train_epoch, args.reps, args.warm)
        print("epoch", name, json.dumps(out[name]), flush=True)
        del run, model, opt, sampler
        torch.cuda.empty_cache()
    return out


def _batch_step(args):
    from mrgcn_amd.tasks import link_prediction as lp
    from tools.lp_grouped_probe import _model, _setup
    s = _setup()
    model, opt = _model(s)
    plan = s["plan_of"](model)
    bs = lp.prepare_batches(lp.mkbatches(None, None, s["known"], 32, 500, 1, plan=plan), "cuda")
    order = np.argsort([len(f) for _, f in bs], kind="stable")
    i = int(order[len(order) // 2])
    mb, mf = bs[i]
    model.train()
    out = dict(batches=len(bs), shape=dict(nodes=int(len(mb.node_index)), facts=int(len(mf))))
    out["triples"] = _timed(lambda: lp.train_batch_step(model, mb, mf, opt), args.reps, args.warm)
    out["all"] = _timed(lambda: lp.train_batch_step(model, mb, mf, opt, decoder="all", loss="softmax"), args.reps,
                        args.warm)
    return out


def _leg(name, args):
    import torch
    from mrgcn_amd.host import fit_cpu_pool_to_quota
    fit_cpu_pool_to_quota()
    if name.startswith("decoder_n"):
        row = _decoder(int(name[len("decoder_n"):]), args)
    elif name == "epoch":
        row = _epochs(args)
    else:
        row = _batch_step(args)
    row["device"] = torch.cuda.get_device_name(0)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lp_all_probe.json"))
    ap.add_argument("--leg", default=None, help="run this one leg in this process and print its row")
    ap.add_argument("--legs", nargs="*", default=LEGS)
    ap.add_argument("--leg-limit", type=float, default=300.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    args = ap.parse_args()
    if args.leg:
        print("LEG_ROW " + json.dumps(_leg(args.leg, args)), flush=True)
        return
    out = dict(reps=args.reps, warm=args.warm, legs={})
    for name in args.legs:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--reps", str(args.reps), "--warm",
               str(args.warm)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.leg_limit, cwd=ROOT)
            rows = [ln for ln in r.stdout.splitlines() if ln.startswith("LEG_ROW ")]
            out["legs"][name] = json.loads(rows[-1][len("LEG_ROW "):]) if r.returncode == 0 and rows else \
                dict(failed=f"exit status {r.returncode}", stderr=r.stderr[-2000:])
        except subprocess.TimeoutExpired:
            out["legs"][name] = dict(failed=f"no result within {args.leg_limit} s")
        print(name, json.dumps(out["legs"][name]), flush=True)
        if "failed" in out["legs"][name]:   # (a faulted device is not handed to the next leg)
            break
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
