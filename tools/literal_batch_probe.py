#!/usr/bin/env python
"""Literal encodings of one mini-batch at a DMG-like shape: the host path (`mksubset` + `pad_` + `to_dense_` +
`as_tensors_` + `to`) against `DeviceEncodings.subset` (csrc/literals.hip).

Seeded synthetic feature list: 260 000 nodes; two token sets (one with its node ids not ascending), one WKT set of CSR
members [11, width], two numeric sets and a temporal one; a batch of 4 000 outermost neighbours.  Both paths are
timed with device events around a call that ends in a synchronise (median of --reps after --warmup), outputs are
checked equal, and the bytes the device path must move (what it reads of the resident sets plus what it writes) are
given over its call time.  The call time includes the one readback and the launches: it is an upper bound of the
kernel time (`rocprofv3 --kernel-trace --stats` gives the kernels' own).

    python tools/literal_batch_probe.py [--nodes 4000] [--reps 20] [--warmup 3] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_features(rng, N):
    def tokens(nodes, lo, hi):
        enc = np.empty(len(nodes), dtype=object)
        lens = rng.integers(lo, hi, len(nodes))
        for i, n in enumerate(lens):
            enc[i] = rng.integers(0, 30000, int(n)).astype(np.int64)
        return enc, lens.astype(np.int32)

    def csr(nodes, C, lo, hi):
        enc = np.empty(len(nodes), dtype=object)
        widths = rng.integers(lo, hi, len(nodes))
        for i, w in enumerate(widths):
            d = rng.standard_normal((C, int(w))).astype(np.float32)
            d[2:][rng.random((C - 2, int(w))) < 0.7] = 0.0     # geometry one-hots: mostly zero
            enc[i] = sp.csr_matrix(d)
        return enc, widths.astype(np.int32)

    s1_nodes = np.sort(rng.choice(N, 60000, replace=False)).astype(np.int32)
    s2_nodes = rng.permutation(N)[:20000].astype(np.int32)               # node ids not ascending
    w_nodes = np.sort(rng.choice(N, 30000, replace=False)).astype(np.int32)
    s1, s1_len = tokens(s1_nodes, 1, 64)
    s2, s2_len = tokens(s2_nodes, 1, 512)
    wk, wk_len = csr(w_nodes, 11, 2, 200)
    num = [np.sort(rng.choice(N, k, replace=False)).astype(np.int32) for k in (50000, 40000, 25000)]
    return [np.empty((N, 0), dtype=np.float32),
            ["xsd.string", [[s1, s1_nodes, s1_len], [s2, s2_nodes, s2_len]], True],
            ["ogc.wktLiteral", [[wk, w_nodes, wk_len]], True],
            ["xsd.numeric", [[rng.standard_normal((len(num[0]), 1)).astype(np.float32), num[0], np.ones(len(num[0]), np.int32)],
                             [rng.standard_normal((len(num[1]), 1)).astype(np.float32), num[1], np.ones(len(num[1]), np.int32)]],
             True],
            ["xsd.dateTime", [[rng.standard_normal((len(num[2]), 6)).astype(np.float32), num[2],
                               np.ones(len(num[2]), np.int32)]], True]]


def host_path(X, nodes_np, pads, dev):
    from mrgcn_amd.data.batch import Batch, mksubset
    b = Batch()
    b.X = mksubset(X, nodes_np)
    b.node_index = nodes_np
    b.pad_(pad_symbols=pads)
    b.to_dense_()
    b.as_tensors_()
    b.A = None
    devs = {m[0]: dev for m in b.X[1:]}
    devs["relational"] = dev
    b.to(devs)
    return [b.X[0].to(dev)] + b.X[1:]


def moved_bytes(X_dev, de):
    """What subset reads of the resident sets and writes: the node list, the map entries of every set at the batch's
    nodes, the selected members' rows / tokens / CSR entries, the outputs."""
    n = int(X_dev[0].shape[0])
    total = n * 8 + len(de._sets) * n * (4 + 16)          # nodes; per set: map entry, member + position lists
    for (dt, sets, _), (_, recs, _) in zip(X_dev[1:], de.modalities):
        for (enc, nidx, seq), r in zip(sets, recs):
            k = int(nidx.numel())
            if k == 0:                                          # (the placeholder of a set without members here)
                continue
            out = enc.numel() * enc.element_size() + nidx.numel() * 8 + seq.numel() * seq.element_size()
            if r.kind == "dense":
                read = out
            elif r.kind == "tokens":
                read = enc.numel() * 8 + k * 16                 # (at most one token per output element; offsets)
            else:
                read = k * (r.C + 1) * 8 + 8 * enc.numel()     # row pointers; (col, value) probes per element
            total += out + read
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("literal_batch_probe needs a GPU")
    from mrgcn_amd.data.batch import DeviceEncodings
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(11)
    N = 260000
    X = make_features(rng, N)
    pads = {"xsd.string": 1}
    nodes_np = np.sort(rng.choice(N, a.nodes, replace=False)).astype(np.int64)
    nodes = torch.from_numpy(nodes_np).to(dev)
    de = DeviceEncodings(X, dev, pad_symbols=pads)

    def timed(fn):
        ts = []
        for i in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                ts.append(e0.elapsed_time(e1))
        return out, float(np.median(ts)), float(np.min(ts)), float(np.max(ts))

    host, t_host, h_lo, h_hi = timed(lambda: host_path(X, nodes_np, pads, dev))
    devx, t_dev, d_lo, d_hi = timed(lambda: de.subset(nodes))
    for (dt, s_h, _), (_, s_d, _) in zip(host[1:], devx[1:]):
        for j, (a_h, a_d) in enumerate(zip(s_h, s_d)):
            for part, x, y in zip(("enc", "node_idx", "seq"), a_h, a_d):
                assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.cpu(), y.cpu()), (dt, j, part)
    nbytes = moved_bytes(devx, de)
    shapes = {f"{dt}[{j}]": list(s[0].shape) for dt, sets, _ in devx[1:] for j, s in enumerate(sets)}
    res = {"device": torch.cuda.get_device_name(dev), "num_nodes": N, "batch_nodes": a.nodes, "reps": a.reps,
           "shapes": shapes, "host_ms_median": round(t_host, 4), "host_ms_min_max": [round(h_lo, 4), round(h_hi, 4)],
           "device_ms_median": round(t_dev, 4), "device_ms_min_max": [round(d_lo, 4), round(d_hi, 4)],
           "speedup": round(t_host / t_dev, 2), "device_bytes_moved": nbytes,
           "device_GBps_over_call_time": round(nbytes / (t_dev * 1e-3) / 1e9, 2), "outputs_equal": True}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
