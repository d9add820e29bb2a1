"""Link-prediction training under torch.use_deterministic_algorithms(True): the DistMult backward, the BCE loss and the
clip's squared norms take their fixed-order twins (csrc/distmult.hip, csrc/optim.hip), so a step's results depend on
its inputs only — the same bits on every call, in every process.  Against the float64 oracle, bitwise across repeats,
full batch (eager and replayed) and mini-batch (featureless and with features), and the routing counters."""
import hashlib
import os
import subprocess
import sys
from contextlib import contextmanager

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD_MB = os.path.join(os.path.dirname(__file__), "golden", "lp_minibatch.npz")
GOLD_MM = os.path.join(os.path.dirname(__file__), "golden", "lp_multimodal.npz")


@contextmanager
def deterministic(on=True):
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(on)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev)


def _triples(n, N, R, hub=False, seed=0):
    rng = np.random.default_rng(seed)
    t = np.stack([rng.integers(0, N, n), rng.integers(0, R, n), rng.integers(0, N, n)], 1).astype(np.int64)
    if hub:   # one relation in 90 % of the triples, one entity in 5 000 of them (both ends)
        t[rng.random(n) < 0.9, 1] = 3
        k = min(5000, n)
        pos = rng.choice(n, k, replace=False)
        t[pos[: k // 2], 0] = 7
        t[pos[k // 2:], 2] = 7
    return t


def _decoder(tr, E0, R0, y, dE_on, dR_on, ns=None):
    from mrgcn_amd.tasks import link_prediction as lp
    E = torch.from_numpy(E0).cuda().requires_grad_(dE_on)
    Rel = torch.from_numpy(R0).cuda().requires_grad_(dR_on)
    trd = torch.from_numpy(tr).cuda()
    st = lp.SortedTriples(trd[:ns], E0.shape[0], R0.shape[0]) if ns else None
    loss = lp.binary_crossentropy(lp.score_distmult_bc(trd, E, Rel, static=st), torch.from_numpy(y).cuda())
    loss.backward()
    return (loss.detach().clone(), E.grad.clone() if dE_on else None, Rel.grad.clone() if dR_on else None)


def _check_decoder(n, H, hub=False, reps=10):
    from oracle import lp_oracle as lo
    N, R = max(40, n // 8), 20
    rng = np.random.default_rng(n * 1000 + H)
    tr = _triples(n, N, R, hub, seed=n + H)
    if hub:   # negatives that duplicate positives
        tr[n - n // 5:] = tr[: n // 5]
    E0 = rng.uniform(-1, 1, (N, H)).astype(np.float32)
    R0 = rng.uniform(-1, 1, (R, H)).astype(np.float32)
    y = np.ones(n, np.float32)
    y[n - n // 5:] = 0
    dE_ref, dR_ref = lo.distmult_bce_grads(tr, E0, R0, y)
    ns = max(n - n // 5, 1)
    with deterministic():
        for static in (None, ns):
            for dE_on, dR_on in ((True, True), (True, False), (False, True)):
                first = _decoder(tr, E0, R0, y, dE_on, dR_on, static)
                if dE_on:
                    np.testing.assert_allclose(first[1].cpu().numpy(), dE_ref, rtol=1e-3, atol=1e-6)
                if dR_on:
                    np.testing.assert_allclose(first[2].cpu().numpy(), dR_ref, rtol=1e-3, atol=1e-6)
                for _ in range(reps - 1 if (dE_on and dR_on) else 1):
                    again = _decoder(tr, E0, R0, y, dE_on, dR_on, static)
                    for a, b in zip(first, again):
                        assert a is None or torch.equal(a, b)


@pytest.mark.parametrize("H", [32, 50, 200, 256, 300])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 3000, 60000])
def test_decoder_backward_vs_oracle_and_bitwise(n, H):
    _check_decoder(n, H, reps=10 if n >= 3000 or H == 200 else 3)


@pytest.mark.parametrize("n", [3000, 60000])
def test_decoder_backward_hub_heavy(n):
    _check_decoder(n, 200, hub=True)
    _check_decoder(n, 50, hub=True, reps=3)


@pytest.mark.parametrize("n", [1, 100, 8192, 8193, 300000])
def test_bce_vs_oracle_and_bitwise(n):
    from mrgcn_amd.tasks import link_prediction as lp
    from oracle import lp_oracle as lo
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * 3).astype(np.float32)
    y = (rng.random(n) < 0.8).astype(np.float32)
    with deterministic():
        outs = []
        for _ in range(5):
            xd = torch.from_numpy(x).cuda().requires_grad_(True)
            loss = lp.binary_crossentropy(xd, torch.from_numpy(y).cuda())
            loss.backward()
            outs.append((loss.detach().clone(), xd.grad.clone()))
    assert abs(float(outs[0][0]) - float(lo.bce_with_logits(x, y))) < 1e-5 * max(1.0, abs(float(outs[0][0])))
    dx = (1.0 / (1.0 + np.exp(-x.astype(np.float64))) - y) / n
    np.testing.assert_allclose(outs[0][1].cpu().numpy(), dx, rtol=1e-4, atol=1e-9)
    for a, b in outs[1:]:
        assert torch.equal(a, outs[0][0]) and torch.equal(b, outs[0][1])


def _clip_params(seed=0):
    rng = np.random.default_rng(seed)
    shapes = [(7,), (33, 5), (200,), (1, 3)] * 5 + [(300000,), (4097,)]   # > 16 small tensors and large ones
    ps = []
    for s in shapes:
        p = torch.nn.Parameter(torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda())
        p.grad = torch.from_numpy((rng.standard_normal(s) * 0.1).astype(np.float32)).cuda()
        ps.append(p)
    return ps


def test_clip_adam_norm_bitwise_and_vs_float64():
    from mrgcn_amd.train import ClipAdam
    ref = None
    with deterministic():
        for _ in range(4):
            ps = _clip_params()
            want = float(np.sqrt(sum((p.grad.double() ** 2).sum().item() for p in ps)))
            opt = ClipAdam(ps, lr=0.01, max_norm=1.0)
            opt.step()
            norm = opt._scratch[ps[0].device]["norm"].clone()
            out = [norm] + [p.detach().clone() for p in ps]
            assert abs(float(norm) - want) < 1e-5 * want
            if ref is None:
                ref = out
            assert all(torch.equal(a, b) for a, b in zip(ref, out))


def test_clip_grad_norm_bitwise_and_vs_float64():
    from mrgcn_amd.optim import clip_grad_norm_
    ref = None
    with deterministic():
        for _ in range(4):
            ps = _clip_params(1)
            want = float(np.sqrt(sum((p.grad.double() ** 2).sum().item() for p in ps)))
            norm = clip_grad_norm_(ps, 1.0)
            out = [norm.detach().clone()] + [p.grad.clone() for p in ps]
            assert abs(float(norm) - want) < 1e-5 * want
            if ref is None:
                ref = out
            assert all(torch.equal(a, b) for a, b in zip(ref, out))


# ---- full batch ---------------------------------------------------------------------------------------------------
def _fullbatch(scale=0.25, seed=0):
    from mrgcn_amd import synth
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.plan import plan_of
    from mrgcn_amd.tasks import link_prediction as lp
    from mrgcn_amd.train import ClipAdam
    g = synth.make_graph("fb15k", seed=seed, scale=scale)
    N, R = g.num_nodes, g.num_relations
    A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([g.rows, g.cols])), torch.from_numpy(g.vals),
                                (N, R * N)).cuda()
    torch.manual_seed(seed)
    model = RGCN([(0, 200, "mrgcn", nn.ReLU())], R, N, 2, 0.0, True, False, True).cuda()
    opt = ClipAdam(model.parameters(), lr=0.01, weight_decay=0.0, max_norm=1.0, capturable=True)
    plan = plan_of(A, N, R, operand_row_bytes=model.operand_row_bytes())
    sampler = lp.DeviceNegativeSampler(torch.from_numpy(np.asarray(g.triples, np.int64)).cuda())
    static = lp.SortedTriples(sampler.facts, N, R)

    def step():
        t, Y = sampler()
        emb = model(None, A)
        loss = lp.binary_crossentropy(lp.score_distmult_bc(t, emb, model.relations, static=static), Y)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss.detach()
    step.plan = plan   # (kept alive with the step, as the bench does)
    return model, opt, step


def _state(model, opt):
    out = [p.detach().clone() for p in model.parameters()]
    for p in model.parameters():
        st = opt.state.get(p, {})
        out += [st["exp_avg"].clone(), st["exp_avg_sq"].clone()] if st else []
    return out


def _fb_eager(steps=5, seed=0):
    torch.manual_seed(seed)
    model, opt, step = _fullbatch()
    losses = [step().clone() for _ in range(steps)]
    torch.cuda.synchronize()
    return losses, _state(model, opt)


def test_fullbatch_steps_bitwise_eager_replayed_and_flag_off():
    from mrgcn_amd.train import GraphedStep
    with deterministic():
        l1, s1 = _fb_eager()
        l2, s2 = _fb_eager()
        assert all(torch.equal(a, b) for a, b in zip(l1, l2))
        assert len(s1) == len(s2) and all(torch.equal(a, b) for a, b in zip(s1, s2))
        torch.manual_seed(0)
        model, opt, step = _fullbatch()
        graphed = GraphedStep(step, warmup=2)
        lg = [graphed().clone() for _ in range(3)]
        torch.cuda.synchronize()
        sg = _state(model, opt)
        assert all(torch.equal(a, b) for a, b in zip(l1[2:], lg)), (l1, lg)
        assert all(torch.equal(a, b) for a, b in zip(s1, sg))
    # flag off: the same arithmetic in another order.  Losses within 1e-5; Adam's m / sqrt(v) magnifies the last-bit
    # differences of gradients that nearly cancel (|g| ~ eps), so a handful of parameter elements move further
    l0, s0 = _fb_eager()
    np.testing.assert_allclose(torch.stack(l0).cpu().numpy(), torch.stack(l1).cpu().numpy(), rtol=1e-5, atol=1e-5)
    for a, b in zip(s0[:3], s1[:3]):   # the parameters
        d = (a - b).abs()
        assert float((d > 1e-5).float().mean()) < 1e-4 and float(d.max()) < 2e-3, float(d.max())


# ---- mini-batch ---------------------------------------------------------------------------------------------------
def _small_graph(path):
    from mrgcn_amd.data.batch import scipy_sparse_to_pytorch_sparse
    from mrgcn_amd.plan import plan_of
    g = np.load(path)
    _, A = util.load_graph("graph_small")
    N = A.shape[0]
    R = A.shape[1] // N
    return g, A, N, R, plan_of(scipy_sparse_to_pytorch_sparse(A, dtype=torch.int8).cuda(), N, R)


def _minibatch_run(seed=0):
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.optim import RowSparseAdam
    from mrgcn_amd.tasks import link_prediction as lp
    g, A, N, R, plan = _small_graph(GOLD_MB)
    bs = lp.prepare_batches(lp.mkbatches(A, None, g["facts"], 8, 1000, 1, plan=plan), "cuda")
    torch.manual_seed(seed)
    model = RGCN([(0, 200, "mrgcn", nn.ReLU())], R, N, 2, 0.0, True, False, True).cuda()
    opt = RowSparseAdam(model.parameters(), lr=0.01)
    losses = [lp.train_epoch(bs, model, opt) for _ in range(2)]
    mrr, hits, ranks = lp.evaluate_batches(bs, model)
    return losses, [p.detach().clone() for p in model.parameters()], (mrr, hits, ranks)


def test_minibatch_golden_graph_bitwise():
    with deterministic():
        a, b = _minibatch_run(), _minibatch_run()
    assert a[0] == b[0]
    assert all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    assert a[2] == b[2]


def test_minibatch_three_reference_steps_under_flag():
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.optim import RowSparseAdam
    from mrgcn_amd.tasks import link_prediction as lp
    g, A, N, R, plan = _small_graph(GOLD_MB)
    tag = "f32b2"
    m = RGCN([(0, 32, "mrgcn", nn.ReLU())], R, N, 2, 0.0, True, False, True)
    m.load_state_dict({k[len(tag) + 6:]: torch.from_numpy(np.array(g[k])) for k in g.files
                       if k.startswith(tag + ".init.")})
    model = m.cuda()
    bs = lp.prepare_batches(lp.mkbatches(A, None, g["facts"], 8, 1000, 1, plan=plan), "cuda")
    opt = RowSparseAdam(model.parameters(), lr=0.01)
    with deterministic():
        for s in range(3):
            loss = lp.train_batch_step(model, bs[s][0], bs[s][1], opt, negatives=g[f"{tag}.step{s}.neg"])
            assert abs(float(loss) - float(g[f"{tag}.step{s}.loss"])) < 1e-5
            for n, p in model.named_parameters():
                np.testing.assert_allclose(util.ref_layout(p.detach(), n).cpu().numpy(), g[f"{tag}.step{s}.{n}"],
                                           rtol=1e-4, atol=2e-6, err_msg=f"step {s} {n}")


def _fb15k_batches(nbatches):
    from mrgcn_amd import synth
    from mrgcn_amd.plan import plan_of
    from mrgcn_amd.tasks import link_prediction as lp
    sg = synth.make_graph("fb15k", seed=0)
    N, R = sg.num_nodes, sg.num_relations
    A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([sg.rows, sg.cols])), torch.from_numpy(sg.vals),
                                (N, R * N)).cuda()
    plan = plan_of(A, N, R)
    bs = lp.mkbatches(None, None, np.asarray(sg.triples, dtype=np.int64), 32, 500, 1, plan=plan)
    return lp.prepare_batches(bs[:nbatches], "cuda"), N, R


def test_minibatch_fb15k_shape_bitwise():
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.train import ClipAdam
    from mrgcn_amd.tasks import link_prediction as lp
    bs, N, R = _fb15k_batches(300)
    runs = []
    with deterministic():
        for _ in range(2):
            torch.manual_seed(0)
            model = RGCN([(0, 200, "mrgcn", nn.ReLU())], R, N, 2, 0.0, True, False, True).cuda()
            opt = ClipAdam(model.parameters(), lr=0.01, max_norm=1.0)
            losses = torch.stack([lp.train_batch_step(model, b, f, opt) for b, f in bs])
            runs.append([losses] + [p.detach().clone() for p in model.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_minibatch_multimodal_wide_features_bitwise():
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.train import ClipAdam
    from mrgcn_amd.tasks import link_prediction as lp
    g, A, N, R, plan = _small_graph(GOLD_MM)
    X = np.random.default_rng(41).standard_normal((N, 145)).astype(np.float32)
    runs = []
    with deterministic():
        for _ in range(2):
            bs = lp.prepare_batches(lp.mkbatches(A, None, g["facts"], 8, 1000, 1, plan=plan), "cuda")
            torch.manual_seed(0)
            model = RGCN([(6, 200, "mrgcn", nn.ReLU())], R, N, 2, 0.0, False, False, True).cuda()
            opt = ClipAdam(model.parameters(), lr=0.01, max_norm=1.0)
            Xd = torch.from_numpy(np.ascontiguousarray(X[:, :6])).cuda()
            losses = []
            for _ in range(2):
                for b, f in bs:
                    b.X = Xd.index_select(0, b.A.neighbours[-1].to("cuda").long())
                    losses.append(lp.train_batch_step(model, b, f, opt))
            runs.append([torch.stack(losses)] + [p.detach().clone() for p in model.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


# ---- across processes ---------------------------------------------------------------------------------------------
def _child():
    from mrgcn_amd.optim import RowSparseAdam
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.tasks import link_prediction as lp
    torch.use_deterministic_algorithms(True)
    h = hashlib.sha256()
    torch.manual_seed(0)
    model, opt, step = _fullbatch()
    for _ in range(3):
        step()
    for t in _state(model, opt):
        h.update(t.cpu().numpy().tobytes())
    g, A, N, R, plan = _small_graph(GOLD_MB)
    bs = lp.prepare_batches(lp.mkbatches(A, None, g["facts"], 8, 1000, 1, plan=plan), "cuda")
    torch.manual_seed(1)
    model = RGCN([(0, 200, "mrgcn", nn.ReLU())], R, N, 2, 0.0, True, False, True).cuda()
    opt = RowSparseAdam(model.parameters(), lr=0.01)
    for i in range(20):
        b, f = bs[i % len(bs)]
        lp.train_batch_step(model, b, f, opt)
    for p in model.parameters():
        h.update(p.detach().cpu().numpy().tobytes())
    print("HASH", h.hexdigest())


def test_two_processes_same_bits():
    hashes = []
    for _ in range(2):
        out = subprocess.run([sys.executable, "-m", "tests.test_gpu_lp_deterministic", "child"], cwd=ROOT,
                             capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-3000:]
        hashes.append([ln for ln in out.stdout.splitlines() if ln.startswith("HASH ")][-1])
    assert hashes[0] == hashes[1]


# ---- routing ------------------------------------------------------------------------------------------------------
DET_KEYS = ("deterministic.distmult_bwd", "deterministic.bce", "deterministic.sumsq")


def test_routing_counters():
    import mrgcn_amd
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.optim import RowSparseAdam
    from mrgcn_amd.tasks import link_prediction as lp
    g, A, N, R, plan = _small_graph(GOLD_MB)
    bs = lp.prepare_batches(lp.mkbatches(A, None, g["facts"], 8, 1000, 1, plan=plan), "cuda")
    model = RGCN([(0, 200, "mrgcn", nn.ReLU())], R, N, 2, 0.0, True, False, True).cuda()
    opt = RowSparseAdam(model.parameters(), lr=0.01)
    lp.train_batch_step(model, bs[0][0], bs[0][1], opt)
    mrgcn_amd.reset_stats()
    lp.train_batch_step(model, bs[1][0], bs[1][1], opt)
    off = mrgcn_amd.stats()
    assert not any(k.startswith("deterministic.") for k in off), off
    mrgcn_amd.reset_stats()
    with deterministic():
        lp.train_batch_step(model, bs[1][0], bs[1][1], opt)
    on = mrgcn_amd.stats()
    for k in DET_KEYS:
        assert on.get(k, 0) >= 1, (k, on)
    # the rest of the step took the same paths
    assert {k: v for k, v in on.items() if not k.startswith("deterministic.")} == off
    # the full-batch wide featureless backward: its atomic-free units even with MRGCN_WIDE_DET=0
    from mrgcn_amd import functional
    prev = functional._WIDE_DET
    functional._WIDE_DET = False
    try:
        model2, opt2, step = _fullbatch(scale=0.05)
        step()
        mrgcn_amd.reset_stats()
        with deterministic():
            step()
        st = mrgcn_amd.stats()
    finally:
        functional._WIDE_DET = prev
    assert st.get("deterministic.wide_input", 0) == 1 and st.get("backward.wide_input", 0) == 1, st
    for k in DET_KEYS:
        assert st.get(k, 0) >= 1, (k, st)


if __name__ == "__main__" and sys.argv[1:] == ["child"]:
    _child()
