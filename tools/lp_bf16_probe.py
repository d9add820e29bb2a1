"""What the bf16 score arithmetic of the all-candidates decoders (csrc/lp_tile.hpp: the bf16 tile; set_score_dtype)
costs beside the f32 arithmetic, in the same run, at the FB15k-237 shape (14 541 nodes, H = 200; the synthetic graph of
tools/lp_grouped_probe.py):

  decoder_n<k>   on fixed embeddings, the 1-vs-all and the KvsAll kernels alone through the C entries — forward, dQ, dE,
                 forward + backward — with "f32" and "bf16", TFLOP/s counting 2 m N H per product (one in the forward,
                 two in each gradient: the scores again and the second product), the bytes of the bf16 tables and the
                 time of the two casts; torch's materialised `F.cross_entropy(Q @ E.T, target)` forward + backward in
                 fp32 and under bf16 autocast where its matrix fits.  k = 272 115 (all facts), 32 768, 4 096
  minibatch      the same rows at the median mini-batch's shape (456 nodes, 569 facts)
  epoch          the replayed full-batch training epoch of `fit` (`FitEpochs.train_epoch`, one captured hipGraph) with
                 decoder="all" and decoder="kvsall" under "f32" and under "bf16"

`--f32-only` runs the f32 rows alone and uses nothing the bf16 arithmetic added: copied into a checkout of the parent
commit it gives profiles/lp_bf16_probe_parent.json, the band (p10 - p90) this tree's f32 rows are held against.

Every figure is the median of `--reps` synchronised, event-timed calls after `--warm` warm-ups, with p10, p90 and the
range.  Every leg runs in a child process of its own under its own time limit (`--leg-limit` seconds); a leg that fails
or runs out of time leaves {"failed": ...} in its place and ends the run.  Writes profiles/lp_bf16_probe.json.

    python tools/lp_bf16_probe.py [--f32-only] [--out profiles/lp_bf16_probe.json]
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

LEGS = ["decoder_n272115", "decoder_n32768", "decoder_n4096", "minibatch", "epoch"]


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


def _tflops(row, products, m, N, H):
    row["tflops"] = products * 2.0 * m * N * H / (row["median_ms"] * 1e-3) / 1e12
    return row


def _kernels(args, N, H, R, facts, f32_only):
    """The C entries alone on fixed embeddings -> rows."""
    import torch
    import torch.nn.functional as F
    from mrgcn_amd import _lib
    from mrgcn_amd.tasks import link_prediction as lp
    lib = _lib.load()
    g = torch.Generator().manual_seed(0)
    E = (0.1 * torch.randn(N, H, generator=g)).cuda()
    Rel = (0.1 * torch.randn(R, H, generator=g)).cuda()
    n, eps = int(facts.shape[0]), 0.1
    kq = lp.KvsAllQueries(facts, N, R)
    with torch.no_grad():
        Qa, tg = lp.pair_vectors(facts, E, Rel)
        Qa = Qa.contiguous()
        Qk = torch.cat([lp.pair_vectors(kq.reps[:kq.m_tail], E, Rel, "tail")[0],
                        lp.pair_vectors(kq.reps[kq.m_tail:], E, Rel, "head")[0]], 0).contiguous()
    ma, mk = 2 * n, kq.m
    out = dict(facts=n, nodes=N, H=H, queries_all=ma, queries_kvsall=mk, nnz=kq.nnz, label_smoothing=eps)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)    # noqa: E731
    one, loss_t = torch.ones(1, device="cuda"), torch.empty((), device="cuda")
    lse, xt = torch.empty(2 * ma, device="cuda"), torch.empty(ma, device="cuda")
    wa = torch.empty(int(lib.mrgcn_lp_all_workspace(ma, N, H)), dtype=torch.uint8, device="cuda")
    wk = torch.empty(int(lib.mrgcn_lp_kvsall_workspace(mk, N, H)), dtype=torch.uint8, device="cuda")
    dQa, dQk, dE = torch.empty_like(Qa), torch.empty_like(Qk), torch.empty_like(E)

    def rows(tag, m, fwd, bwd, dQ):
        r = {}
        r["forward"] = _tflops(_timed(fwd, args.reps, args.warm), 1, m, N, H)
        r["dQ"] = _tflops(_timed(lambda: bwd(dQ, None), args.reps, args.warm), 2, m, N, H)
        r["dE"] = _tflops(_timed(lambda: bwd(None, dE), args.reps, args.warm), 2, m, N, H)
        r["forward_and_backward"] = _tflops(_timed(lambda: (fwd(), bwd(dQ, dE)), args.reps, args.warm), 5, m, N, H)
        out[tag] = r
        print(tag, json.dumps(r), flush=True)

    def f32_rows(suffix):
        rows("all_f32" + suffix, ma,
             lambda: _lib.check(lib.mrgcn_lp_all_fwd_f32(p(Qa), H, ma, p(E), H, N, H, p(tg), p(lse), p(xt), p(loss_t),
                                                         p(wa), wa.numel(), st())),
             lambda a, b: _lib.check(lib.mrgcn_lp_all_bwd_f32(p(Qa), H, ma, p(E), H, N, H, p(tg), p(lse), p(one), p(a),
                                                              H, p(b), H, None, 0, st())), dQa)
        rows("kvsall_f32" + suffix, mk,
             lambda: _lib.check(lib.mrgcn_lp_kvsall_fwd_f32(p(Qk), H, mk, p(E), H, N, H, p(kq.ptr), p(kq.idx), eps, None,
                                                            p(loss_t), p(wk), wk.numel(), st())),
             lambda a, b: _lib.check(lib.mrgcn_lp_kvsall_bwd_f32(p(Qk), H, mk, p(E), H, N, H, p(kq.ptr), p(kq.idx),
                                                                 p(kq.cptr), p(kq.cqry), eps, p(one), p(a), H, p(b), H,
                                                                 None, 0, st())), dQk)
    f32_rows("")
    if not f32_only:
        Qab, Qkb, Eb = lp._bf16_table(Qa), lp._bf16_table(Qk), lp._bf16_table(E)
        Hp = int(Eb.shape[1])
        out["bf16_table_bytes"] = dict(Q_all=Qab.numel() * 2, Q_kvsall=Qkb.numel() * 2, E=Eb.numel() * 2)
        out["bf16_casts_all"] = _timed(lambda: (lp._bf16_table(Qa), lp._bf16_table(E)), args.reps, args.warm)
        rows("all_bf16", ma,
             lambda: _lib.check(lib.mrgcn_lp_all_fwd_bf16(p(Qab), Hp, ma, p(Eb), Hp, N, H, p(tg), p(lse), p(xt),
                                                          p(loss_t), p(wa), wa.numel(), st())),
             lambda a, b: _lib.check(lib.mrgcn_lp_all_bwd_bf16(p(Qab), Hp, ma, p(Eb), Hp, N, H, p(tg), p(lse), p(one),
                                                               p(a), H, p(b), H, None, 0, st())), dQa)
        rows("kvsall_bf16", mk,
             lambda: _lib.check(lib.mrgcn_lp_kvsall_fwd_bf16(p(Qkb), Hp, mk, p(Eb), Hp, N, H, p(kq.ptr), p(kq.idx), eps,
                                                             None, p(loss_t), p(wk), wk.numel(), st())),
             lambda a, b: _lib.check(lib.mrgcn_lp_kvsall_bwd_bf16(p(Qkb), Hp, mk, p(Eb), Hp, N, H, p(kq.ptr), p(kq.idx),
                                                                  p(kq.cptr), p(kq.cqry), eps, p(one), p(a), H, p(b), H,
                                                                  None, 0, st())), dQk)
        f32_rows("_again")      # (the same rows at the end: the drift of the box)
        for dec in ("all", "kvsall"):
            out[dec + "_bf16_over_f32"] = {k: out[dec + "_bf16"][k]["median_ms"] / out[dec + "_f32"][k]["median_ms"]
                                           for k in ("forward", "dQ", "dE", "forward_and_backward")}
        del Qab, Qkb, Eb
    del dQa, dQk, dE, wa, wk, lse, xt
    # torch's materialised 1-vs-all route, where its matrix fits
    out["torch_matrix_gb"] = 4.0 * ma * N / 1e9
    try:
        Qg, Eg = Qa.clone().requires_grad_(), E.clone().requires_grad_()

        def torch_f32():
            torch.autograd.grad(F.cross_entropy(Qg @ Eg.t(), tg), [Qg, Eg])

        def torch_bf16():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = F.cross_entropy(Qg @ Eg.t(), tg)
            torch.autograd.grad(loss, [Qg, Eg])
        out["torch_f32_forward_and_backward"] = _tflops(_timed(torch_f32, args.reps, args.warm), 3, ma, N, H)
        out["torch_bf16_autocast_forward_and_backward"] = _tflops(_timed(torch_bf16, args.reps, args.warm), 3, ma, N, H)
    except RuntimeError as e:
        if "out of memory" not in str(e).lower():
            raise
        out["torch_does_not_fit"] = dict(matrix_gb=4.0 * ma * N / 1e9, error=str(e).splitlines()[0][:200])
    return out


def _decoder(n, args):
    from tools.lp_grouped_probe import _setup
    s = _setup()
    return _kernels(args, s["N"], s["H"], s["R"], s["train"][:n].contiguous(), args.f32_only)


def _minibatch(args):
    """The median mini-batch of mkbatches(32, 500) on this graph: 456 nodes, 569 facts (tools/lp_kvsall_probe.py's
    batch_step leg reports the shape); random facts of that shape."""
    import torch
    from tools.lp_grouped_probe import _setup
    s = _setup()
    g = torch.Generator().manual_seed(1)
    N, n = 456, 569
    facts = torch.stack([torch.randint(0, N, (n,), generator=g), torch.randint(0, s["R"], (n,), generator=g),
                         torch.randint(0, N, (n,), generator=g)], 1).cuda()
    return _kernels(args, N, s["H"], s["R"], facts, args.f32_only)


EPOCHS = (("all", dict(decoder="all", loss="softmax")), ("kvsall", dict(decoder="kvsall", label_smoothing=0.1)))


def _epochs(args):
    import torch
    from mrgcn_amd.tasks import link_prediction as lp
    from tools.lp_grouped_probe import _model, _sampler, _setup
    s = _setup()
    out = {}
    order = [(n, kw, "f32") for n, kw in EPOCHS]
    if not args.f32_only:
        order += [(n, kw, "bf16") for n, kw in EPOCHS] + [(n + "_again", kw, "f32") for n, kw in EPOCHS]
    for name, kw, mm in order:
        model, opt = _model(s)
        plan = s["plan_of"](model)   # noqa: F841  (kept alive with the run, as the bench does)
        sampler = _sampler(s, 10)
        tparts = lp.FactParts(s["train"][:2000], 0, filtered=False)
        prev = None if args.f32_only else lp.set_score_dtype(mm)
        try:
            run = lp.FitEpochs(model, lambda: model(None, s["A"]), tparts, None, opt, graphed=True, sampler=sampler,
                               warmup=3, **kw)
            out[f"{name}_{mm}"] = _timed(run.train_epoch, args.reps, args.warm)
        finally:
            if prev is not None:
                lp.set_score_dtype(prev)
        print("epoch", name, mm, json.dumps(out[f"{name}_{mm}"]), flush=True)
        del run, model, opt, sampler
        torch.cuda.empty_cache()
    if not args.f32_only:
        for n, _ in EPOCHS:
            out[n + "_bf16_over_f32"] = out[n + "_bf16"]["median_ms"] / out[n + "_f32"]["median_ms"]
    return out


def _leg(name, args):
    import torch
    from mrgcn_amd.host import fit_cpu_pool_to_quota
    fit_cpu_pool_to_quota()
    if name.startswith("decoder_n"):
        row = _decoder(int(name[len("decoder_n"):]), args)
    elif name == "minibatch":
        row = _minibatch(args)
    else:
        row = _epochs(args)
    row["device"] = torch.cuda.get_device_name(0)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lp_bf16_probe.json"))
    ap.add_argument("--leg", default=None, help="run this one leg in this process and print its row")
    ap.add_argument("--legs", nargs="*", default=LEGS)
    ap.add_argument("--f32-only", action="store_true", help="the f32 rows alone, with nothing the bf16 arithmetic added")
    ap.add_argument("--leg-limit", type=float, default=400.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    args = ap.parse_args()
    if args.leg:
        print("LEG_ROW " + json.dumps(_leg(args.leg, args)), flush=True)
        return
    out = dict(reps=args.reps, warm=args.warm, f32_only=bool(args.f32_only), legs={})
    for name in args.legs:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--reps", str(args.reps), "--warm",
               str(args.warm)] + (["--f32-only"] if args.f32_only else [])
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
