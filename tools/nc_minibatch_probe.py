"""What the mini-batch node-classification run loop costs per epoch on the device, at the shape of the bench line's
mini-batch leg (the AM/4 synthetic graph, a two-layer model with 155 feature columns, 40 bases, hidden 10, 11
classes).  The AM shape carries 250 labels at this scale — less than one batch of the leg's 1 024 nodes — so the probe
draws a label split of its own: 8 192 training and 2 048 validation nodes, cut by `mkbatches` into batches of 1 024
(8 + 2 batches) and of 64 (128 + 32).  Batches are masked batches on the full graph's plan, built once.

Timed per batch size, the median wall time (stream synchronised before and after) of `--reps` epochs after 5 warm-ups
on one box:

  replayed      GraphedBatchEpoch: the whole epoch as one hipGraph replay
  eager         BatchEpoch: the same launches from the host, no synchronisation
  host_loop     the loop as the reference writes it (node_classification.py:154-225) around this package's existing
                functions and nothing of tasks/node_classification.py: per batch `train_step`, `float(loss)`, the logits
                to the host and torch-op accuracy there; per validation batch an eval() forward, logits to the host,
                CrossEntropyLoss and accuracy there; np.mean of the lists; the host EarlyStop with copy.deepcopy of both
                state_dicts on improvement
  two_launches  the eager (and, replayed through train.GraphedStep, the captured) epoch with the loss launch and the
                evaluation launch it replaces (`categorical_crossentropy` + `evaluate` + the copies into the slot):
                (two_launches - fused) / batches is the per-batch price of the pair over the fused launch

Every epoch runs under a stopper that never improves (tolerance 1e30); `*_improving` rows record an improvement
every epoch (tolerance -1e30: the snapshot copies, the host loop deep-copies).  Writes
profiles/nc_minibatch_probe.json.

    python tools/nc_minibatch_probe.py [--out profiles/nc_minibatch_probe.json] [--reps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_TRAIN, N_VALID = 8192, 2048


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nc_minibatch_probe.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scale", type=float, default=0.25)
    ap.add_argument("--batchsizes", type=int, nargs="+", default=[1024, 64])
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps: medians are taken over at least 20 epochs")
    from mrgcn_amd import synth
    from mrgcn_amd.host import fit_cpu_pool_to_quota
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.plan import GraphPlan
    from mrgcn_amd.tasks import node_classification as nc
    from mrgcn_amd.train import (ClipAdam, EarlyStop, GraphedStep, categorical_crossentropy, evaluate, train_step)
    fit_cpu_pool_to_quota()
    dev = torch.device("cuda", torch.cuda.current_device())
    g = synth.make_graph("am", seed=0, scale=args.scale)
    N, R = g.num_nodes, g.num_relations
    A = sp.csr_matrix((g.vals, (g.rows, g.cols)), shape=(N, R * N))
    dims = synth.layer_dims("am")
    classes, bases = dims[-1][1], synth.SHAPES["am"]["bases"]
    mods = [(dims[0][0], dims[0][1], "mrgcn", torch.nn.ReLU()), (dims[1][0], dims[1][1], "mrgcn", None)]
    rng = np.random.default_rng(0)
    nodes = rng.choice(N, N_TRAIN + N_VALID, replace=False)
    ys = rng.integers(0, classes, len(nodes))
    Y = {k: sp.csr_matrix((np.ones(len(n), dtype=np.int8), (n, y)), shape=(N, classes), dtype=np.int8)
         for k, (n, y) in dict(train=(nodes[:N_TRAIN], ys[:N_TRAIN]), valid=(nodes[N_TRAIN:], ys[N_TRAIN:])).items()}
    X = torch.randn((N, dims[0][0]), device=dev)
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmups=5, timing="wall clock, synchronised",
               graph="am x %g (N=%d, R=%d, nnz=%d)" % (args.scale, N, R, A.nnz), layers=dims, bases=bases,
               labels=dict(train=N_TRAIN, valid=N_VALID), sizes={})

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)

    def fresh():
        torch.manual_seed(0)
        model = RGCN(mods, R, N, bases, 0.0, False, True, False).to(dev)
        opt = ClipAdam(model.parameters(), lr=0.01, max_norm=1.0, capturable=True)
        return model, opt

    model, _ = fresh()
    plan = GraphPlan.from_csr(A, N, R, value_mode="ref_int8", device=dev, operand_row_bytes=model.operand_row_bytes())
    del model

    def stop_cfg(improving):
        return EarlyStop(patience=1 << 30, tolerance=-1e30 if improving else 1e30, delay=0)

    for bs in args.batchsizes:
        t0 = time.perf_counter()
        batches = {k: nc.prepare_batches(nc.mkbatches(None, None, Y[k], bs, 2, plan=plan), Y[k], dev, X_full=X)
                   for k in ("train", "valid")}
        torch.cuda.synchronize()
        tb, vb = batches["train"], batches["valid"]
        nb = len(tb) + len(vb)
        res = dict(batchsize=bs, train_batches=len(tb), valid_batches=len(vb),
                   batches_built_once_s=time.perf_counter() - t0,
                   last_level_rows=[int(b.A.supports[-1].NR) for b in (tb[0], tb[-1])])
        out["sizes"][str(bs)] = res

        # the device epochs -----------------------------------------------------------------------------------------
        for improving in (False, True):
            sfx = "_improving" if improving else ""
            model, opt = fresh()
            run = nc.GraphedBatchEpoch(model, tb, vb, opt, stop_cfg(improving), warmup=3)
            res["replayed" + sfx] = _timed(run, args.reps)
            st = run.counter.read()
            assert st.stop == 0 and (st.best_record == st.records if improving else st.best_record == 1)
            res["replayed" + sfx]["snapshot_bytes"] = run.stopper.snapshot_bytes
            del run
            model, opt = fresh()
            run = nc.BatchEpoch(model, tb, vb, opt, stop_cfg(improving))
            res["eager" + sfx] = _timed(run, args.reps)
            print(bs, "replayed" + sfx, json.dumps(res["replayed" + sfx]), "eager", json.dumps(res["eager" + sfx]),
                  flush=True)
            save()
            del run
            torch.cuda.empty_cache()

        # the epoch with the two launches the fused one replaces ----------------------------------------------------
        def two_launch_epoch(model, opt, ep):
            def fn():
                model.train()
                for i, b in enumerate(tb):
                    st, box = b._mrgcn_nc, []

                    def fwd():
                        o = model(X, b.A)
                        box[:] = evaluate(o.detach(), st["pos"], st["tgt"])
                        return o
                    loss = train_step(model, fwd, st["pos"], st["tgt"], opt)
                    ep.train_slots[i, 0:1].copy_(loss.reshape(1))
                    ep.train_slots[i, 1:2].copy_(box[1].reshape(1))
                model.eval()
                with torch.no_grad():
                    for i, b in enumerate(vb):
                        st = b._mrgcn_nc
                        loss, acc = evaluate(model(X, b.A), st["pos"], st["tgt"])
                        ep.valid_slots[i, 0:1].copy_(loss.reshape(1))
                        ep.valid_slots[i, 1:2].copy_(acc.reshape(1))
                model.train()
                nc._batch_means(ep.train_slots, len(tb), ep.valid_slots, len(vb), ep.row)
                ep.stopper.record_row(ep.row[2:3], ep.row, ep.ring)
                return ep.row
            return fn
        model, opt = fresh()
        ep = nc.BatchEpoch(model, tb, vb, opt, stop_cfg(False))
        res["two_launches_eager"] = _timed(two_launch_epoch(model, opt, ep), args.reps)
        model, opt = fresh()
        ep = nc.BatchEpoch(model, tb, vb, opt, stop_cfg(False))
        step = GraphedStep(two_launch_epoch(model, opt, ep), warmup=3)
        res["two_launches_replayed"] = _timed(step, args.reps)
        res["fused_loss_saves_us_per_batch"] = dict(
            eager=(res["two_launches_eager"]["median_ms"] - res["eager"]["median_ms"]) / nb * 1e3,
            replayed=(res["two_launches_replayed"]["median_ms"] - res["replayed"]["median_ms"]) / nb * 1e3)
        print(bs, "two launches", json.dumps(res["two_launches_eager"]), json.dumps(res["two_launches_replayed"]),
              json.dumps(res["fused_loss_saves_us_per_batch"]), flush=True)
        save()
        del step, ep
        torch.cuda.empty_cache()

        # the loop as the reference writes it -----------------------------------------------------------------------
        criterion = torch.nn.CrossEntropyLoss()
        for improving in (False, True):
            model, opt = fresh()
            es = stop_cfg(improving)

            class _Free:   # (the first record always copies: keep that one out of the no-improvement row)
                def state_dict(self):
                    return {}
            es.record(1.0, _Free(), _Free())

            def epoch():
                model.train()
                loss_lst, acc_lst = [], []
                for b in tb:
                    st, box = b._mrgcn_nc, []

                    def fwd():
                        o = model(X, b.A)
                        box[:] = [o.detach()]
                        return o
                    batch_loss = train_step(model, fwd, st["pos"], st["tgt"], opt)
                    Y_hat = box[0].to("cpu")
                    idx, targets = torch.from_numpy(st["pos_host"]), torch.as_tensor(st["tgt_host"], dtype=torch.long)
                    batch_acc = torch.mean(torch.eq(Y_hat[idx].max(dim=1)[1], targets).float())
                    loss_lst.append(float(batch_loss))
                    acc_lst.append(float(batch_acc))
                train_loss, train_acc = np.mean(loss_lst), np.mean(acc_lst)
                model.eval()
                loss_lst, acc_lst = [], []
                for b in vb:
                    st = b._mrgcn_nc
                    with torch.no_grad():
                        Y_hat = model(X, b.A).to("cpu")
                        idx, targets = torch.from_numpy(st["pos_host"]), torch.as_tensor(st["tgt_host"], dtype=torch.long)
                        batch_loss = criterion(Y_hat[idx], targets)
                        batch_acc = torch.mean(torch.eq(Y_hat[idx].max(dim=1)[1], targets).float())
                    loss_lst.append(float(batch_loss))
                    acc_lst.append(float(batch_acc))
                val_loss, val_acc = np.mean(loss_lst), np.mean(acc_lst)
                es.record(val_loss, model, opt)
                return train_loss, train_acc, val_loss, val_acc
            key = "host_loop" + ("_improving" if improving else "")
            res[key] = _timed(epoch, args.reps)
            assert bool(es.best_weights) == improving   # ({}: only the free first record copied anything)
            print(bs, key, json.dumps(res[key]), flush=True)
            save()
            del model, opt
            torch.cuda.empty_cache()
        res["host_loop_over_replayed"] = res["host_loop"]["median_ms"] / res["replayed"]["median_ms"]
        res["eager_over_replayed"] = res["eager"]["median_ms"] / res["replayed"]["median_ms"]
        res["graph_batches"] = nb
        for k in ("train", "valid"):
            for b in batches[k]:
                b.A.close()
        del batches, tb, vb
        torch.cuda.empty_cache()
        save()
    save()


if __name__ == "__main__":
    main()
