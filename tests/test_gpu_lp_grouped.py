"""The grouped DistMult loss on the device (csrc/distmult_group.hip; mrgcn_amd.tasks.link_prediction.group_loss and the
run loops' decoder="grouped").

Bounds.  Scores: the bits of `score_distmult_bc` on the same triples (same products, lane sum and wave sum).  Loss and
gradients: against the float64 restatement of tests/test_cpu_lp_grouped.py (itself held to torch's float64 autograd
there) with the decoder's bounds of tests/test_gpu_lp.py — loss |d| <= 1e-5 max(1, |loss|), dE / dRel rtol 1e-3, atol
1e-6.  E, Rel ~ 0.5 N(0, 1): scores of standard deviation about 1.8, not saturated.  A reference is computed once per
(triples, loss, weight) and shared."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from tests.test_cpu_lp_grouped import draw64, draw_flag_case, embeddings, grouped_reference
from tests.test_cpu_lp_negatives import FIX300_SAMPLER_SEED, N, R, SEED, fixture300, fixture64
from tests.test_gpu_lp_negatives import _check_rows, _encoder_problem, _golden_problem, deterministic

pytestmark = pytest.mark.gpu
_REF: dict = {}
_SETS: dict = {}


def _np(t):
    return t.detach().cpu().numpy()


def _set(name):
    """(triples [n (1 + rate), 3], n, rate, num_nodes, num_relations) of a named case, drawn once by the host mirror."""
    if name in _SETS:
        return _SETS[name]
    from mrgcn_amd import host
    kind, rate = name.rsplit("_", 1)
    rate = int(rate)
    if kind == "fix64":
        t, n = draw64(rate)
        out = (t, n, rate, N, R)
    elif kind == "few64":        # 20 facts: with rate 70 a group spans two chunks of 64 members
        facts = fixture64()["facts"][:20]
        neg, _ = host.negatives_draw(facts, rate, N, N, R, fixture64()["keys"], SEED, 0)
        out = (np.concatenate([facts, neg]), 20, rate, N, R)
    elif kind == "fix300":       # 2 500 facts: the stored-orders route
        facts = fixture300()
        neg, _ = host.negatives_draw(facts, rate, 300, 300, 5, host.fact_keys(facts, 300, 5), FIX300_SAMPLER_SEED, 0)
        out = (np.concatenate([facts, neg]), len(facts), rate, 300, 5)
    elif kind.startswith("first"):   # the first facts of fixture300: the sizes around the backward's switch of routes
        facts = fixture300()[:int(kind[5:])]
        neg, _ = host.negatives_draw(facts, rate, 300, 300, 5, host.fact_keys(facts, 300, 5), FIX300_SAMPLER_SEED, 0)
        out = (np.concatenate([facts, neg]), len(facts), rate, 300, 5)
    elif kind == "long9000":     # 3 000 facts of one predicate, 400 of one subject: runs that cross waves and blocks
        rng = np.random.default_rng(200)
        facts = np.stack([rng.integers(0, 500, 9000), rng.integers(0, 9, 9000), rng.integers(0, 500, 9000)], 1).astype(np.int64)
        facts[:3000, 1] = 2
        facts[3000:3400, 0] = 7
        neg, _ = host.negatives_draw(facts, rate, 500, 500, 9, False, 77, 0)
        out = (np.concatenate([facts, neg]), 9000, rate, 500, 9)
    else:
        raise KeyError(name)
    _SETS[name] = out
    return out


def _reference(name, H, loss, w):
    key = (name, H, loss, float(w))
    if key not in _REF:
        t, n, rate, nn_, nr = _set(name)
        E, Rel = embeddings(nn_, nr, H)
        _REF[key] = grouped_reference(t, n, rate, E, Rel, loss, w)
    return _REF[key]


def _device_run(name, H, loss, pos_weight, with_static, scale=None, statics=None):
    from mrgcn_amd.tasks import link_prediction as lp
    t, n, rate, nn_, nr = _set(name)
    E, Rel = embeddings(nn_, nr, H)
    Et, Rt = torch.from_numpy(E).cuda().requires_grad_(True), torch.from_numpy(Rel).cuda().requires_grad_(True)
    tt = torch.from_numpy(t).cuda()
    static = lp.SortedTriples(tt[:n], nn_, nr) if with_static else None
    if statics is not None:
        statics.append(static)
    out = lp.group_loss(tt, Et, Rt, n, rate, loss=loss, pos_weight=pos_weight, static=static)
    assert out.dtype == torch.float32 and out.dim() == 0 and out.is_cuda
    (out if scale is None else scale * out).backward()
    return float(out.detach()), _np(Et.grad), _np(Rt.grad)


def _within(got, want, what, scale=1.0):
    loss, dE, dR = got
    rl, rE, rR = want[:3]
    print(f"{what}: loss {loss:.7f} ref {rl:.7f} |d| {abs(loss - rl):.2e}; max |ddE| {np.abs(dE - scale * rE).max():.2e} "
          f"of {np.abs(rE).max() * scale:.2e}; max |ddRel| {np.abs(dR - scale * rR).max():.2e} of {np.abs(rR).max() * scale:.2e}")
    assert abs(loss - rl) <= 1e-5 * max(1.0, abs(rl)), what
    np.testing.assert_allclose(dE, scale * rE, rtol=1e-3, atol=1e-6, err_msg=what)
    np.testing.assert_allclose(dR, scale * rR, rtol=1e-3, atol=1e-6, err_msg=what)


# ---- 1. scores: the bits of the flat decoder -------------------------------------------------------------------------
def _scores_equal(t, n, rate, nn_, nr, H):
    from mrgcn_amd.tasks import link_prediction as lp
    E, Rel = embeddings(nn_, nr, H)
    Et, Rt, tt = torch.from_numpy(E).cuda(), torch.from_numpy(Rel).cuda(), torch.from_numpy(t).cuda()
    got = lp.group_scores(tt, Et, Rt, n, rate)
    want = lp.score_distmult_bc(tt, Et, Rt)
    assert got.shape == want.shape == (n * (1 + rate),)
    assert float(want.std()) > 0.1 or H == 4
    assert torch.equal(got, want), f"{int((got != want).sum())} of {got.numel()} scores differ"


@pytest.mark.parametrize("rate", [1, 3, 10, 22])
def test_scores_are_the_flat_decoders_bits_at_every_rate(rate):
    t, n = draw64(rate)
    _scores_equal(t, n, rate, N, R, 200)


@pytest.mark.parametrize("side", [1, 2], ids=["tail", "head"])
def test_scores_bits_of_one_sided_draws(side):
    t, n = draw64(3, side=side)
    _scores_equal(t, n, 3, N, R, 200)


@pytest.mark.parametrize("H", [256, 64, 4])
def test_scores_bits_at_other_widths(H):
    t, n = draw64(3)
    _scores_equal(t, n, 3, N, R, H)


@pytest.mark.parametrize("name", ["one_fact", "flag_case", "two_chunks"])
def test_scores_bits_of_the_edge_groups(name):
    if name == "one_fact":
        t, n = draw64(3)
        t = np.concatenate([t[:1], t[n:n + 3]])
        _scores_equal(t, 1, 3, N, R, 200)
    elif name == "flag_case":
        t, n, _ = draw_flag_case()
        _scores_equal(t, n, 4, 8, 1, 200)
    else:
        t, n, rate, nn_, nr = _set("few64_70")
        _scores_equal(t, n, rate, nn_, nr, 200)


# ---- 2. loss and gradients against the float64 restatement -----------------------------------------------------------
VARIANTS = ["bce_1", "bce_rate", "softmax"]


def _variant(variant, rate):
    """-> [(loss, pos_weight argument, weight of the reference)]"""
    if variant == "bce_1":
        return [("bce", None, 1.0), ("bce", 1.0, 1.0)]
    if variant == "bce_rate":
        return [("bce", float(rate), float(rate))]
    return [("softmax", None, 1.0)]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ["fix64_3", "fix64_10", "few64_70", "fix300_1", "fix300_3", "long9000_3"])
def test_loss_and_gradients_against_the_restatement(name, variant):
    import mrgcn_amd
    rate = _set(name)[2]
    for with_static in (False, True):
        runs = []
        for loss, pw, w in _variant(variant, rate):
            mrgcn_amd.reset_stats()
            got = _device_run(name, 200, loss, pw, with_static)
            st = mrgcn_amd.stats()
            assert st.get("lp.decoder.grouped", 0) == 1 and st.get("lp.decoder.grouped.fallback", 0) == 0
            _within(got, _reference(name, 200, loss, w), f"{name} {loss} pos_weight {pw} static {with_static}")
            runs.append(got)
        if len(runs) == 2:   # pos_weight 1.0 gives the bits of None (the loss is summed in a fixed order)
            assert runs[0][0] == runs[1][0]


@pytest.mark.parametrize("n,stored_orders", [(1023, False), (1024, True)])
def test_the_backward_takes_the_stored_orders_from_1024_facts(n, stored_orders):
    """The smallest size of the stored-orders route and the largest of the atomic one (with `static`): the route's
    scratch is kept on the SortedTriples, so its presence tells which ran."""
    from mrgcn_amd.tasks import link_prediction as lp
    assert lp._GROUP_SORTED_MIN == 1024
    for loss in ("bce", "softmax"):
        statics = []
        got = _device_run(f"first{n}_3", 200, loss, None, True, statics=statics)
        _within(got, _reference(f"first{n}_3", 200, loss, 1.0), f"{n} facts {loss}")
        assert ("group_bwd" in getattr(statics[0], "_group_ws", {})) == stored_orders


def test_pos_weight_one_gives_the_bits_of_none_and_a_tensor_weight_is_read():
    """The forward's outputs — scores, dloss/dscore, loss — carry no atomics: weight 1.0 and None agree bit for bit."""
    from mrgcn_amd.tasks import link_prediction as lp
    t, n, rate, nn_, nr = _set("fix64_10")
    E, Rel = embeddings(nn_, nr, 200)
    Et, Rt, tt = torch.from_numpy(E).cuda(), torch.from_numpy(Rel).cuda(), torch.from_numpy(t).cuda()
    a = lp.group_loss(tt, Et, Rt, n, rate)
    b = lp.group_loss(tt, Et, Rt, n, rate, pos_weight=1.0)
    c = lp.group_loss(tt, Et, Rt, n, rate, pos_weight=torch.tensor([10.0], device="cuda"))
    d = lp.group_loss(tt, Et, Rt, n, rate, pos_weight=10.0)
    assert torch.equal(a, b) and torch.equal(c, d) and not torch.equal(a, c)


@pytest.mark.parametrize("name,with_static", [("fix64_3", False), ("fix300_3", True)])
def test_an_upstream_gradient_scales_both_gradients(name, with_static):
    for loss in ("bce", "softmax"):
        got = _device_run(name, 200, loss, None, with_static, scale=2.5)
        _within(got, _reference(name, 200, loss, 1.0), f"{name} {loss} 2.5 x", scale=2.5)


# ---- 3. the fallback ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_rows_of_70_features_take_the_fallback(variant):
    import mrgcn_amd
    for with_static in (False, True):
        for loss, pw, w in _variant(variant, 3):
            mrgcn_amd.reset_stats()
            got = _device_run("fix64_3", 70, loss, pw, with_static)
            st = mrgcn_amd.stats()
            assert st.get("lp.decoder.grouped", 0) == 1 and st.get("lp.decoder.grouped.fallback", 0) == 1
            _within(got, _reference("fix64_3", 70, loss, w), f"H 70 {loss} pos_weight {pw} static {with_static}")


def _flag_run(facts, A, num_nodes, num_pred, rate, loss):
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.tasks import link_prediction as lp
    from mrgcn_amd.train import ClipAdam
    torch.manual_seed(11)
    model = RGCN([(0, 16, "mrgcn", nn.ReLU())], 2 * num_pred + 1, num_nodes, 2, 0.0, True, False, True).cuda()
    opt = ClipAdam(model.parameters(), lr=0.05, weight_decay=0.0, max_norm=1.0)
    smp = lp.NegativeSampler(facts, num_nodes, num_pred, rate=rate, seed=SEED)
    model.train()
    losses = [lp.train_step(model, lambda: model(None, A), smp, opt, decoder="grouped", loss=loss).clone()
              for _ in range(3)]
    torch.cuda.synchronize()
    return losses, [p.detach().clone() for p in model.parameters()]


@pytest.mark.parametrize("loss", ["bce", "softmax"])
def test_under_the_flag_the_fallback_runs_and_two_runs_are_bitwise_equal(loss):
    import mrgcn_amd
    facts = fixture64()["facts"]
    A = _encoder_problem(facts, N, R)
    with deterministic():
        mrgcn_amd.reset_stats()
        l1, p1 = _flag_run(facts, A, N, R, 3, loss)
        st = mrgcn_amd.stats()
        assert st.get("lp.decoder.grouped", 0) == 3 and st.get("lp.decoder.grouped.fallback", 0) == 3
        assert st.get("deterministic.distmult_bwd", 0) == 3
        l2, p2 = _flag_run(facts, A, N, R, 3, loss)
    print(loss, "losses", [float(x) for x in l1])
    assert all(np.isfinite(float(x)) for x in l1)
    assert all(torch.equal(a, b) for a, b in zip(l1, l2))
    assert len(p1) == len(p2) and all(torch.equal(a, b) for a, b in zip(p1, p2))


# ---- 4. capture and replay -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["atomics", "stored_orders"])
@pytest.mark.parametrize("loss", ["bce", "softmax"])
def test_group_loss_and_backward_replay_with_a_fresh_draw_each(case, loss):
    from mrgcn_amd.tasks import link_prediction as lp
    if case == "atomics":
        facts, nn_, nr, rate = fixture64()["facts"], N, R, 3
    else:
        facts, nn_, nr, rate = fixture300(), 300, 5, 1
    E, Rel = embeddings(nn_, nr, 200)
    Et, Rt = torch.from_numpy(E).cuda().requires_grad_(True), torch.from_numpy(Rel).cuda().requires_grad_(True)
    smp = lp.NegativeSampler(facts, nn_, nr, rate=rate, seed=SEED)
    static = lp.SortedTriples(smp.facts, nn_, nr)
    out = [torch.zeros((), device="cuda"), torch.zeros_like(Et), torch.zeros_like(Rt)]

    def step():
        t, _ = smp()
        val = lp.group_loss(t, Et, Rt, smp.n, rate, loss=loss, static=static)
        dE, dR = torch.autograd.grad(val, [Et, Rt])
        out[0].copy_(val.detach())
        out[1].copy_(dE)
        out[2].copy_(dR)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()     # (the layout is checked and the scratch allocated here, outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
        step()
    seen = []
    for r in range(3):
        graph.replay()
        torch.cuda.synchronize()
        t = _np(smp.buf)
        seen.append(t.copy())
        want = grouped_reference(t, smp.n, rate, E, Rel, loss, 1.0)
        _within((float(out[0]), _np(out[1]), _np(out[2])), want, f"{case} {loss} replay {r}")
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])


# ---- 5. the loops on the 50-node golden problem ----------------------------------------------------------------------------
def test_train_step_grouped_loss_falls_and_counts():
    import mrgcn_amd
    from mrgcn_amd.tasks import link_prediction as lp
    model, opt, A, _, facts, nn_, nr = _golden_problem()
    smp = lp.NegativeSampler(facts, nn_, nr, rate=3, known=facts, seed=SEED)
    model.train()
    mrgcn_amd.reset_stats()
    losses = [float(lp.train_step(model, lambda: model(None, A), smp, opt, decoder="grouped")) for _ in range(4)]
    print("losses", losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    st = mrgcn_amd.stats()
    assert st.get("lp.decoder.grouped", 0) == 4 and st.get("lp.decoder.grouped.fallback", 0) == 0
    assert isinstance(smp._static, lp.SortedTriples)      # built once, on first use


@pytest.mark.parametrize("kw", [dict(pos_weight=3.0), dict(pos_weight=torch.tensor(3.0)), dict(loss="softmax")],
                         ids=["pos_weight", "pos_weight_tensor", "softmax"])
def test_train_step_grouped_with_a_weight_and_with_the_softmax_loss(kw):
    from mrgcn_amd.tasks import link_prediction as lp
    model, opt, A, _, facts, nn_, nr = _golden_problem()
    smp = lp.NegativeSampler(facts, nn_, nr, rate=3, known=facts, seed=SEED)
    static = lp.SortedTriples(smp.facts, nn_, nr)
    model.train()
    losses = [float(lp.train_step(model, lambda: model(None, A), smp, opt, static=static, decoder="grouped", **kw))
              for _ in range(4)]
    print(kw, "losses", losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_train_step_grouped_with_penalties_through_a_clipping_clipadam():
    from mrgcn_amd.tasks import link_prediction as lp
    model, opt, A, _, facts, nn_, nr = _golden_problem()
    assert opt.max_norm is not None and lp.penalty_owners(model, opt)
    smp = lp.NegativeSampler(facts, nn_, nr, rate=3, known=facts, seed=SEED)
    model.train()
    plain = float(lp.train_step(*_fresh_step_args(), decoder="grouped"))
    losses = [float(lp.train_step(model, lambda: model(None, A), smp, opt, decoder="grouped", l1_lambda=1e-5,
                                  l2_lambda=5e-4)) for _ in range(4)]
    print("losses", losses, "without the penalty", plain)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0] and losses[0] > plain


def _fresh_step_args():
    from mrgcn_amd.tasks import link_prediction as lp
    model, opt, A, _, facts, nn_, nr = _golden_problem()
    smp = lp.NegativeSampler(facts, nn_, nr, rate=3, known=facts, seed=SEED)
    model.train()
    return model, (lambda: model(None, A)), smp, opt


def test_first_step_of_the_grouped_decoder_equals_the_flat_decoders():
    from mrgcn_amd.tasks import link_prediction as lp
    runs = []
    for decoder in ("triples", "grouped"):
        model, fwd, smp, opt = _fresh_step_args()
        before = [p.detach().clone() for p in model.parameters()]
        loss = float(lp.train_step(model, fwd, smp, opt, decoder=decoder))
        runs.append((loss, before, [p.detach().clone() for p in model.parameters()], _np(smp.buf)))
    (lt, bt, at, tt), (lg, bg, ag, tg) = runs
    assert np.array_equal(tt, tg) and all(torch.equal(a, b) for a, b in zip(bt, bg))
    print("first-step loss: triples", lt, "grouped", lg)
    assert abs(lt - lg) <= 1e-5 * max(1.0, abs(lt))
    for b, pt, pg in zip(bt, at, ag):
        dt, dg = _np(pt - b), _np(pg - b)
        print("parameter", tuple(b.shape), "max |change|", np.abs(dt).max(), "max |difference|", np.abs(dt - dg).max())
        np.testing.assert_allclose(dg, dt, rtol=1e-3, atol=1e-6)


def test_fit_graphed_grouped():
    import mrgcn_amd
    from mrgcn_amd.tasks import link_prediction as lp
    model, opt, A, _, facts, nn_, nr = _golden_problem()
    train, valid = facts[:100], facts[100:]
    smp = lp.NegativeSampler(train, nn_, nr, rate=3, known=facts, seed=SEED)
    mrgcn_amd.reset_stats()
    rows = list(lp.fit(model, lambda: model(None, A), train, valid, opt, 6, eval_interval=1, mrr_batchsize=50,
                       graphed=True, sampler=smp, decoder="grouped"))
    _check_rows(rows, 6, True)
    print("losses", [r[1] for r in rows])
    assert rows[-1][1] < rows[0][1]
    # 3 warm-up epochs and two captures call group_loss; the replays do not pass through Python
    assert mrgcn_amd.stats().get("lp.decoder.grouped", 0) == 5
    assert mrgcn_amd.stats().get("lp.decoder.grouped.fallback", 0) == 0


def _batch_problem():
    from mrgcn_amd.data.batch import scipy_sparse_to_pytorch_sparse
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.plan import plan_of
    from mrgcn_amd.tasks import link_prediction as lp
    from mrgcn_amd.train import ClipAdam
    _, _, _, A_csr, facts, nn_, nr = _golden_problem()
    torch.manual_seed(3)
    model = RGCN([(0, 32, "mrgcn", nn.ReLU())], nr, nn_, 2, 0.0, True, False, True).cuda()
    opt = ClipAdam(list(model.parameters()), lr=0.01, max_norm=1.0, capturable=True)
    plan = plan_of(scipy_sparse_to_pytorch_sparse(A_csr, dtype=torch.int8).cuda(), nn_, nr)
    train, valid = facts[:90], facts[90:]
    tb = lp.prepare_batches(lp.mkbatches(A_csr, None, train, 17, 40, 1, plan=plan), "cuda")
    vb = lp.prepare_batches(lp.mkbatches(A_csr, None, valid, 13, 20, 1, plan=plan), "cuda")
    return model, opt, tb, vb, lp.batch_negative_samplers(nn_, nr, rate=3, known=facts, seed=SEED)


def test_train_batch_step_and_train_epoch_grouped():
    import mrgcn_amd
    from mrgcn_amd._lib import MrgcnError
    from mrgcn_amd.tasks import link_prediction as lp
    model, opt, tb, _, make = _batch_problem()
    batch, f = tb[0]
    smp = make(0, batch, f)
    model.train()
    mrgcn_amd.reset_stats()
    losses = [float(lp.train_batch_step(model, batch, f, opt, sampler=smp, decoder="grouped")) for _ in range(4)]
    print("batch losses", losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert mrgcn_amd.stats().get("lp.decoder.grouped", 0) == 4
    smps = [make(i, b, ff) for i, (b, ff) in enumerate(tb)]
    means = [lp.train_epoch(tb, model, opt, samplers=smps, decoder="grouped", loss="softmax") for _ in range(3)]
    print("epoch means", means)
    assert all(np.isfinite(means)) and means[-1] < means[0]
    # a sampler without the layout is refused
    with pytest.raises(MrgcnError, match="NegativeSampler"):
        lp.train_batch_step(model, batch, f, opt, sampler=lp.DeviceNegativeSampler(smp.facts), decoder="grouped")
    with pytest.raises(MrgcnError, match="NegativeSampler"):
        lp.train_step(model, None, lp.DeviceNegativeSampler(smp.facts), opt, decoder="grouped")


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graphed"])
def test_fit_batches_grouped(graphed):
    import mrgcn_amd
    from mrgcn_amd.tasks import link_prediction as lp
    model, opt, tb, vb, make = _batch_problem()
    mrgcn_amd.reset_stats()
    rows = list(lp.fit_batches(model, tb, vb, opt, 4, eval_interval=1, graphed=graphed, samplers=make,
                               decoder="grouped"))
    _check_rows(rows, 4, True)
    print("losses", [r[1] for r in rows])
    assert rows[-1][1] < rows[0][1]
    st = mrgcn_amd.stats()
    captured = st.get("lp.batch_epoch.graphed", 0) > 0
    assert captured == graphed
    # (captured: 3 warm-up epochs and two captures pass through Python, the replays do not)
    assert st.get("lp.decoder.grouped", 0) == (5 if captured else 4) * len(tb)
    assert mrgcn_amd.stats().get("lp.decoder.grouped.fallback", 0) == 0
