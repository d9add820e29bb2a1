"""What the KvsAll decoder (csrc/lp_kvsall.hip) costs at the FB15k-237 shape (synthetic graph of that shape, bench.py's
split and model: 14 541 nodes, H = 200; the graph of tools/lp_all_probe.py):

  decoder    on fixed embeddings at n = 32 768 and all 272 115 training facts: the queries (m, nnz, m / 2n — the
             synthetic facts repeat few (s, p) and (p, o), so m / 2n is close to 1), `all_loss` forward and backward
             FIRST, `kvsall_loss` forward and backward, `all_loss` again LAST (the spread of the two `all` rows is the
             run's noise); the kernels alone through the C entries with the per-query ratio of each KvsAll entry to the
             1-vs-all one ((t_kvsall / m) / (t_all / 2n): both run the same score-sized products per query; the
             KvsAll forward entry includes its pass over the answer lists, its backward kernels walk them inside the
             tile loop); torch's materialised route `F.binary_cross_entropy_with_logits(Q @ E.T, Y')` forward +
             backward on the same Q, E, Y' where it fits, and the peak device memory of both
  epoch      the replayed full-batch training epoch of `fit` (`FitEpochs.train_epoch`, one captured hipGraph) with
             decoder="kvsall" (label_smoothing 0 and 0.1) beside the untouched decoders: the flat default, "grouped" at
             10 keyed negatives, "all"
  batch_step the median mini-batch's `train_batch_step` (batches of mkbatches(32, 500)): the flat default, "all", "kvsall"

`--legs epoch_untouched batch_step_untouched` runs the untouched decoders' rows alone and uses nothing this decoder
added: copied into a checkout of the parent commit it gives profiles/lp_kvsall_probe_parent.json, the band (p10 - p90)
this tree's rows of the same decoders are held against.

Every figure is the median of `--reps` synchronised, event-timed calls after `--warm` warm-ups, with p10, p90 and the
range.  Every leg runs in a child process of its own under its own time limit (`--leg-limit` seconds); a leg that fails
or runs out of time leaves {"failed": ...} in its place.  Writes profiles/lp_kvsall_probe.json.

    python tools/lp_kvsall_probe.py [--out profiles/lp_kvsall_probe.json]
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

LEGS = ["decoder_n32768", "decoder_n272115", "epoch", "batch_step"]


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
    return dict(median_ms=float(np.median(ms)), p10_ms=float(np.percentile(ms, 10)),
                p90_ms=float(np.percentile(ms, 90)), range_ms=[float(min(ms)), float(max(ms))])


def _peak_gb(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e9


def _decoder(n, args):
    import torch
    import torch.nn.functional as F
    from mrgcn_amd import _lib
    from mrgcn_amd.tasks import link_prediction as lp
    from tools.lp_grouped_probe import _setup
    s = _setup()
    N, H, eps = s["N"], s["H"], 0.1
    g = torch.Generator().manual_seed(0)
    E = (0.1 * torch.randn(N, H, generator=g)).cuda().requires_grad_()
    Rel = (0.1 * torch.randn(s["R"], H, generator=g)).cuda().requires_grad_()
    facts = s["train"][:n].contiguous()
    n = int(facts.shape[0])
    kq = lp.KvsAllQueries(facts, N, s["R"])
    m = kq.m
    out = dict(facts=n, queries_all=2 * n, queries_kvsall=m, nnz=kq.nnz, m_over_2n=m / (2.0 * n), nodes=N, H=H,
               label_smoothing=eps)

    def both(loss_fn):
        loss = loss_fn()
        torch.autograd.grad(loss, [E, Rel])

    def rows(tag, loss_fn):
        out[tag + "_forward"] = _timed(loss_fn, args.reps, args.warm)
        out[tag + "_forward_and_backward"] = _timed(lambda: both(loss_fn), args.reps, args.warm)
    rows("all_loss_first", lambda: lp.all_loss(facts, E, Rel))
    rows("kvsall_loss", lambda: lp.kvsall_loss(kq, E, Rel, eps))
    rows("all_loss_last", lambda: lp.all_loss(facts, E, Rel))
    out["kvsall_peak_gb"] = _peak_gb(lambda: both(lambda: lp.kvsall_loss(kq, E, Rel, eps)))
    # the kernels alone
    lib = _lib.load()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)    # noqa: E731
    one = torch.ones(1, device="cuda")
    loss_t = torch.empty((), device="cuda")
    Ed = E.detach()
    with torch.no_grad():
        Qa, tg = lp.pair_vectors(facts, E, Rel)
        Qa = Qa.contiguous()
        Qk = torch.cat([lp.pair_vectors(kq.reps[:kq.m_tail], E, Rel, "tail")[0],
                        lp.pair_vectors(kq.reps[kq.m_tail:], E, Rel, "head")[0]], 0).contiguous()
    ma = 2 * n
    lse, xt = torch.empty(2 * ma, device="cuda"), torch.empty(ma, device="cuda")
    wa = torch.empty(int(lib.mrgcn_lp_all_workspace(ma, N, H)), dtype=torch.uint8, device="cuda")
    wk = torch.empty(int(lib.mrgcn_lp_kvsall_workspace(m, N, H)), dtype=torch.uint8, device="cuda")
    dQa, dQk, dE = torch.empty_like(Qa), torch.empty_like(Qk), torch.empty_like(Ed)

    def all_fwd():
        _lib.check(lib.mrgcn_lp_all_fwd_f32(p(Qa), H, ma, p(Ed), H, N, H, p(tg), p(lse), p(xt), p(loss_t), p(wa),
                                            wa.numel(), st()))

    def all_bwd(a, b):
        _lib.check(lib.mrgcn_lp_all_bwd_f32(p(Qa), H, ma, p(Ed), H, N, H, p(tg), p(lse), p(one), p(a), H, p(b), H, None,
                                            0, st()))

    def kv_fwd():
        _lib.check(lib.mrgcn_lp_kvsall_fwd_f32(p(Qk), H, m, p(Ed), H, N, H, p(kq.ptr), p(kq.idx), eps, None, p(loss_t),
                                               p(wk), wk.numel(), st()))

    def kv_bwd(a, b):
        _lib.check(lib.mrgcn_lp_kvsall_bwd_f32(p(Qk), H, m, p(Ed), H, N, H, p(kq.ptr), p(kq.idx), p(kq.cptr),
                                               p(kq.cqry), eps, p(one), p(a), H, p(b), H, None, 0, st()))
    kern = {}
    for name, fn in (("all_forward", all_fwd), ("all_dQ", lambda: all_bwd(dQa, None)),
                     ("all_dE", lambda: all_bwd(None, dE)), ("kvsall_forward", kv_fwd),
                     ("kvsall_dQ", lambda: kv_bwd(dQk, None)), ("kvsall_dE", lambda: kv_bwd(None, dE)),
                     ("all_forward_again", all_fwd), ("all_dQ_again", lambda: all_bwd(dQa, None)),
                     ("all_dE_again", lambda: all_bwd(None, dE))):
        kern[name] = _timed(fn, args.reps, args.warm)
    for k in ("forward", "dQ", "dE"):
        a = [kern["all_" + k]["median_ms"] / ma, kern["all_" + k + "_again"]["median_ms"] / ma]
        kern["per_query_ratio_" + k] = dict(kvsall_over_all=[kern["kvsall_" + k]["median_ms"] / m / x for x in a],
                                            all_again_over_all=a[1] / a[0])
    out["kernels"] = kern
    del dQa, dQk, dE, wa, wk, lse, xt
    # the materialised route, where it fits
    try:
        Y = torch.full((m, N), eps / N, device="cuda")
        Y[kq.rows, kq.idx.long()] = (1.0 - eps) + eps / N
        Qg, Eg = Qk.detach().requires_grad_(), Ed.clone().requires_grad_()

        def torch_both():
            torch.autograd.grad(F.binary_cross_entropy_with_logits(Qg @ Eg.t(), Y), [Qg, Eg])
        out["torch_forward_and_backward"] = _timed(torch_both, args.reps, args.warm)
        out["torch_peak_gb"] = _peak_gb(torch_both) + 4.0 * m * N / 1e9    # (with the target it needs beforehand)
        out["torch_matrix_gb"] = 4.0 * m * N / 1e9
    except RuntimeError as e:
        if "out of memory" not in str(e).lower():
            raise
        out["torch_does_not_fit"] = dict(matrix_gb=4.0 * m * N / 1e9, error=str(e).splitlines()[0][:200])
    return out


EPOCH_UNTOUCHED = (("triples", {}), ("grouped_rate10", dict(decoder="grouped")),
                   ("all", dict(decoder="all", loss="softmax")))
EPOCH_NEW = (("kvsall_eps0", dict(decoder="kvsall")), ("kvsall_eps0.1", dict(decoder="kvsall", label_smoothing=0.1)))


def _epochs(args, rows):
    import torch
    from mrgcn_amd.tasks import link_prediction as lp
    from tools.lp_grouped_probe import _model, _sampler, _setup
    s = _setup()
    out = {}
    for name, kw in rows:
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


def _batch_step(args, new):
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
    if new:
        out["kvsall"] = _timed(lambda: lp.train_batch_step(model, mb, mf, opt, decoder="kvsall", label_smoothing=0.1),
                               args.reps, args.warm)
        out["shape"]["queries"] = int(mb._mrgcn_lp["_kvsall"][1].m)
        out["triples_again"] = _timed(lambda: lp.train_batch_step(model, mb, mf, opt), args.reps, args.warm)
    return out


def _leg(name, args):
    import torch
    from mrgcn_amd.host import fit_cpu_pool_to_quota
    fit_cpu_pool_to_quota()
    if name.startswith("decoder_n"):
        row = _decoder(int(name[len("decoder_n"):]), args)
    elif name == "epoch":
        row = _epochs(args, EPOCH_UNTOUCHED + EPOCH_NEW + (("triples_again", {}),))
    elif name == "epoch_untouched":
        row = _epochs(args, EPOCH_UNTOUCHED + (("triples_again", {}),))
    else:
        row = _batch_step(args, name == "batch_step")
    row["device"] = torch.cuda.get_device_name(0)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lp_kvsall_probe.json"))
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
