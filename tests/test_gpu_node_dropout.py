"""Node dropout on the device (RGCN.set_node_dropout("device")): the draw against its host mirror, a training step
with explicit masks against a float64 composition of the oracle's layers, the fast paths of the backward, the replayed
epoch graph, a mini-batch step without synchronisation, and the host mode left as it was.

Tolerances are those of tests/test_gpu_step_oracle.py for its f32 step (logits rtol/atol 1e-4, loss rtol 2e-5 /
atol 1e-6, gradients `_close_grad`, the parameters and moments after the step `_check_adam`)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import util
from tests.test_gpu_step_oracle import LR, _check_adam, _close_grad

pytestmark = pytest.mark.gpu

P = 0.3


def _np(t):
    return t.detach().cpu().numpy()


# ---- 1. the draw -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.2, 0.5, 1.0])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1_000_003])
def test_device_draw_equals_the_host_twin_bit_for_bit(n, p):
    from mrgcn_amd import functional as Fn
    from mrgcn_amd import host
    seed, pos0 = 0x1234_5678_9ABC_DEF0, (1 << 32) - 2   # (both words of the seed and of the position take part)
    state = Fn.node_dropout_state(seed, pos0, "cuda")
    for step in range(3):   # three consecutive positions, two layers each
        masks = Fn.node_dropout_draw(state, n, p, layers=2, layer0=0, advance=True)
        torch.cuda.synchronize()
        for layer, m in enumerate(masks):
            ref = host.node_dropout_mask(n, p, seed, pos0 + step, layer)
            assert np.array_equal(_np(m).view(np.uint32), ref.view(np.uint32)), (n, p, step, layer)
    assert int(state[1].item()) == pos0 + 3
    # one layer at a time (another grid, another launch order): the same values
    state = Fn.node_dropout_state(seed, pos0, "cuda")
    m1 = Fn.node_dropout_draw(state, n, p, layers=1, layer0=1, advance=False)[0]
    assert np.array_equal(_np(m1), host.node_dropout_mask(n, p, seed, pos0, 1))
    assert int(state[1].item()) == pos0


@pytest.mark.parametrize("rows,F,ld", [(1000, 10, 12), (1000, 11, 11), (1000, 12, 12), (777, 3, 3), (513, 200, 200),
                                       (100, 5, 9)])
def test_row_scale_kernels(rows, F, ld):
    """In place on rows with a leading dimension (pad untouched), and the row-live twin (dead rows unread: NaNs there)."""
    from mrgcn_amd import functional as Fn
    g = torch.Generator("cuda").manual_seed(rows + F)
    buf = torch.randn((rows, ld), device="cuda", generator=g)
    m = (torch.rand(rows, device="cuda", generator=g) > 0.3).float() * 1.4285715
    ref = buf.clone()
    ref[:, :F] *= m[:, None]
    Y = buf.clone()
    Fn.row_scale_(Y[:, :F], m)
    assert torch.equal(Y, ref)
    flags = (torch.rand(rows, device="cuda", generator=g) > 0.5).to(torch.uint8)
    dY = buf[:, :F].contiguous()
    dY[flags == 0] = float("nan")
    out = Fn.row_scale_live(dY, m, flags, zero_dead=True)
    want = torch.where(flags.bool()[:, None], ref[:, :F], torch.zeros((), device="cuda"))
    assert torch.equal(out, want)
    out = Fn.row_scale_live(dY, m, flags, zero_dead=False)
    assert torch.equal(out[flags.bool()], want[flags.bool()])


# ---- 2. a step with explicit masks against the float64 composition --------------------------------------------------
def _case(name, p_dropout=P):
    c = util.load_case(name)
    model, dims = util.build_rgcn_from_case(c, "cuda")
    util.load_state_from_case(model, c)
    model = model.cuda()
    model.p_dropout = p_dropout
    g, A_csr = util.load_graph(util.graph_of_case(name))
    A = util.coo_tensor(A_csr, str(c["value_mode"]), "cuda")
    X = None if bool(c["meta.featureless"]) else torch.from_numpy(c["X"]).cuda()
    idx, tgt = torch.from_numpy(c["labels_idx"]).cuda(), torch.from_numpy(c["labels_y"]).cuda()
    return c, model, dims, A_csr, A, X, idx, tgt


def _masks_with_a_dropped_label_and_hub(c, A_csr, N, seed):
    """Two host-drawn masks (layer 0, layer 1); in both, one labelled node and the node most columns name (the hub)
    are dropped and another labelled node is kept, whatever the draw says."""
    rng = np.random.default_rng(seed)
    keep = np.float32(1.0) / np.float32(1.0 - P)
    hub = int(np.bincount(A_csr.indices % N, minlength=N).argmax())
    masks = []
    for _ in range(2):
        m = np.where(rng.random(N) < P, np.float32(0), keep).astype(np.float32)
        m[int(c["labels_idx"][0])] = 0.0
        m[hub] = 0.0
        m[int(c["labels_idx"][1])] = keep
        masks.append(m)
    return masks


def _oracle_step(c, dims, A_csr, X, masks):
    """Forward, cross-entropy, backward, clip 1.0 and one Adam step in float64 with the node masks between the layers:
    h0 = m0 . relu(pre0), out = m1 . pre1 (rgcn.py:78-84 applies the mask to every layer's output)."""
    from oracle import rgcn_oracle as O
    N, R, B = int(c["meta.num_nodes"]), int(c["meta.R"]), int(c["meta.num_bases"])
    cfgs = O.rgcn_cfgs(dims, R, N, B, bool(c["meta.bias"]), bool(c["meta.featureless"]))
    state = {k[len("init."):]: np.array(c[k]).astype(np.float64) for k in c.files if k.startswith("init.")}
    params = O.split_params(state, 2)
    A64 = A_csr.astype(np.float64)
    m0, m1 = (m.astype(np.float64)[:, None] for m in masks)
    pre0, c0 = O.layer_forward(cfgs[0], params[0], X, A64)
    h0 = m0 * np.maximum(pre0, 0.0)
    pre1, c1 = O.layer_forward(cfgs[1], params[1], h0, A64)
    out = m1 * pre1
    loss, dout = O.cross_entropy(out, c["labels_idx"], c["labels_y"])
    g1, dh0 = O.layer_backward(cfgs[1], params[1], h0, A64, m1 * dout, c1)
    g0, _ = O.layer_backward(cfgs[0], params[0], X, A64, m0 * dh0 * (pre0 > 0), c0)
    grads = {f"layers.layer_{li}.{k}": v for li, g in enumerate((g0, g1)) for k, v in g.items()}
    norm, coef = O.clip_grad_norm(list(grads.values()), 1.0)
    adam = O.Adam(lr=LR)
    after = dict(state)
    adam.step(after, {k: v * coef for k, v in grads.items()})
    return dict(logits=out, loss=loss, grads=grads, norm=norm, coef=coef, before=state, after=after)


@pytest.mark.parametrize("name", ["rgcn_small_ft_b3_bias_norm_f32", "rgcn_small_ft_b3_nobias_norm_f32"])
def test_step_with_explicit_masks_against_the_float64_composition(name):
    import mrgcn_amd
    from mrgcn_amd.train import ClipAdam, train_step
    c, model, dims, A_csr, A, X, idx, tgt = _case(name)
    N = int(c["meta.num_nodes"])
    masks = _masks_with_a_dropped_label_and_hub(c, A_csr, N, seed=3)
    ora = _oracle_step(c, dims, A_csr, None if X is None else c["X"], masks)
    model.set_node_dropout("device")
    model.node_dropout_masks = [torch.from_numpy(m).cuda() for m in masks]
    for row_sparse in (False, None):
        util.load_state_from_case(model, c)
        model.zero_grad(set_to_none=True)
        opt = ClipAdam(list(model.parameters()), lr=LR, max_norm=1.0)
        with torch.no_grad():
            logits = model(X, A)
        assert model.last_node_masks[0] is model.node_dropout_masks[0]
        np.testing.assert_allclose(_np(logits), ora["logits"], rtol=1e-4, atol=1e-4)
        assert not _np(logits)[masks[1] == 0].any()
        mrgcn_amd.reset_stats()
        loss = train_step(model, lambda: model(X, A), idx, tgt, opt, row_sparse=row_sparse)
        assert mrgcn_amd.stats().get("node_dropout.device") == 2
        np.testing.assert_allclose(float(loss), ora["loss"], rtol=2e-5, atol=1e-6)
        np.testing.assert_allclose(opt.last_grad_norm(), ora["norm"], rtol=2e-5)
        sd = model.state_dict()
        for n, p in model.named_parameters():
            if row_sparse is False:
                assert p.grad is not None, n
                _close_grad(_np(util.ref_layout(p.grad, n)), ora["grads"][n], f"{name}: grad {n}")
            st = opt.state[p]
            _check_adam(f"{name}: {n}", ora["before"][n], ora["grads"][n], ora["coef"], _np(sd[n]),
                        _np(util.ref_layout(st["exp_avg"], n)), _np(util.ref_layout(st["exp_avg_sq"], n)))


# ---- 3. the fast paths of the backward are kept ---------------------------------------------------------------------
def test_fast_paths_are_those_of_the_step_without_dropout():
    import mrgcn_amd
    from mrgcn_amd.train import ClipAdam, train_step
    c, model, dims, A_csr, A, X, idx, tgt = _case("rgcn_small_ft_b3_bias_norm_f32")
    model.set_node_dropout("device", seed=5)
    wI = model.layers["layer_0"].weight_I
    seen = {}
    for p in (0.0, P):
        model.p_dropout = p
        util.load_state_from_case(model, c)
        opt = ClipAdam(list(model.parameters()), lr=LR, max_norm=1.0)
        train_step(model, lambda: model(X, A), idx, tgt, opt)   # (first use: plans, supports)
        mrgcn_amd.reset_stats()
        train_step(model, lambda: model(X, A), idx, tgt, opt)
        seen[p] = mrgcn_amd.stats()
        assert wI.grad is None, p
    assert seen[P].pop("node_dropout.device") == 2 and "node_dropout.device" not in seen[0.0]
    assert seen[P] == seen[0.0], (seen[P], seen[0.0])
    assert seen[P].get("backward.support") == 2 and (seen[P].get("weight_I.fused_rows") or seen[P].get("weight_I.rows"))


# ---- 4. the replayed epoch graph ------------------------------------------------------------------------------------
def test_graph_replay_draws_fresh_masks_equal_to_eager_steps():
    """GraphedTrainStep with p_dropout = 0.3 in device mode: one warm-up step, the capture, five replays — five
    different mask pairs, bitwise those of eager steps 2..6 from the same seed, position and parameters (and of the
    host twin).  The step's clip norm and basis-coefficient gradients are summed with float atomics, so the losses are
    compared at the oracle's loss tolerance, as tests/test_gpu_layers.py compares replayed and eager epochs."""
    from mrgcn_amd import host
    from mrgcn_amd.train import ClipAdam, GraphedTrainStep, train_step
    name = "rgcn_small_ft_b3_bias_norm_f32"
    c, model, dims, A_csr, A, X, idx, tgt = _case(name)
    N = int(c["meta.num_nodes"])
    model.set_node_dropout("device", seed=77)
    runs = {}
    for graphed in (False, True):
        util.load_state_from_case(model, c)
        model.zero_grad(set_to_none=True)
        model.node_dropout_position = 0
        opt = ClipAdam(list(model.parameters()), lr=LR, max_norm=1.0, capturable=True)
        fwd = lambda: model(X, A)   # noqa: E731
        losses, masks = [], []
        if graphed:
            step = GraphedTrainStep(model, fwd, idx, tgt, opt, warmup=1)
            assert model.node_dropout_position == 1   # (the capture itself draws nothing)
        else:
            train_step(model, fwd, idx, tgt, opt)
        for _ in range(5):
            loss = step() if graphed else train_step(model, fwd, idx, tgt, opt)
            losses.append(float(loss))
            masks.append([_np(m).copy() for m in model.last_node_masks])
        assert model.node_dropout_position == 6
        runs[graphed] = (losses, masks)
    for k in range(5):
        for layer in range(2):
            a, b = runs[False][1][k][layer], runs[True][1][k][layer]
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (k, layer)
            assert np.array_equal(b, host.node_dropout_mask(N, P, 77, 1 + k, layer)), (k, layer)
        np.testing.assert_allclose(runs[True][0][k], runs[False][0][k], rtol=2e-5, atol=1e-6)
    flat = [np.concatenate(m).tobytes() for m in runs[True][1]]
    assert len(set(flat)) == 5, "replays repeated a mask"


# ---- 5. mini-batches -------------------------------------------------------------------------------------------------
def test_minibatch_step_never_synchronises_in_device_mode_and_does_in_host_mode():
    """A wide_features=True link-prediction batch at the FB15k-237 synthetic shape: `train_batch_step` under
    torch.cuda.set_sync_debug_mode("error") passes with device dropout and raises with the host draw (its
    pageable copy is a synchronising call)."""
    from mrgcn_amd import synth
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.optim import RowSparseAdam
    from mrgcn_amd.plan import plan_of
    from mrgcn_amd.tasks import link_prediction as lp
    import mrgcn_amd
    sg = synth.make_graph("fb15k", seed=0)
    N, R = sg.num_nodes, sg.num_relations
    A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([sg.rows, sg.cols])), torch.from_numpy(sg.vals),
                                (N, R * N)).cuda()
    plan = plan_of(A, N, R)
    facts = np.asarray(sg.triples, dtype=np.int64)[:4000]
    Xd = torch.full((N, 145), 0.05, device="cuda") + torch.linspace(0, 0.1, 145, device="cuda")
    bs = lp.prepare_batches(lp.mkbatches(None, None, facts, 32, 500, 1, plan=plan), "cuda")[:4]
    for b, _ in bs:
        b.X = Xd
    torch.manual_seed(0)
    model = RGCN([(145, 200, "mrgcn", nn.ReLU())], R, N, 2, P, False, False, True).cuda()
    opt = RowSparseAdam(model.parameters(), lr=0.01)
    model.set_node_dropout("device", seed=9)
    lp.train_batch_step(model, bs[0][0], bs[0][1], opt)   # (first use: lazily built workspaces, the device state)
    torch.cuda.synchronize()
    mrgcn_amd.reset_stats()
    torch.cuda.set_sync_debug_mode("error")
    try:
        losses = [lp.train_batch_step(model, b, f, opt) for b, f in bs]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    st = mrgcn_amd.stats()
    assert st.get("node_dropout.device") == len(bs) and st.get("masked.wide_feat") == len(bs), st
    assert np.isfinite([float(x) for x in losses]).all()
    m = model.last_node_masks[0]
    assert m.numel() == int(bs[-1][0].A.row[0].NR) and set(np.unique(_np(m)).tolist()) <= {0.0, float(np.float32(1) / np.float32(1 - P))}
    model.set_node_dropout("host")
    lp.train_batch_step(model, bs[0][0], bs[0][1], opt)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            lp.train_batch_step(model, bs[0][0], bs[0][1], opt)
    finally:
        torch.cuda.set_sync_debug_mode("default")


# ---- 6. the host mode is the literal sequence it was ----------------------------------------------------------------
@pytest.mark.parametrize("train", [True, False])
def test_host_mode_is_the_reference_sequence_to_the_bit(train):
    from torch.nn.functional import dropout
    c, model, dims, A_csr, A, X, idx, tgt = _case("rgcn_small_ft_b3_bias_norm_f32")
    assert model.node_dropout_mode == "host"
    model.train(train)   # (the reference draws the mask in eval() too)
    torch.manual_seed(1234)
    with torch.no_grad():
        got = model(X, A)
    torch.manual_seed(1234)
    with torch.no_grad():
        H = X
        for key, layer in model.layers.items():
            H = layer(H, A)
            ones = dropout(torch.ones(model.num_nodes), p=model.p_dropout).to(H.device)
            H = H * ones.unsqueeze(1)
            if model.activations[key] is not None:
                H = model.activations[key](H)
    assert torch.equal(got, H)
    assert (got == 0).all(1).any() and model.last_node_masks == []


def test_link_prediction_graphed_step_draws_fresh_masks_equal_to_eager_steps():
    """The link-prediction epoch in a GraphedStep (featureless 200-wide encoder with 2 bases and ReLU, DistMult, BCE,
    ClipAdam(capturable)) with p_dropout = 0.3 in device mode, on a fixed triple set so that eager and replayed steps
    score the same triples: three warm-up steps, the capture, five replays — five different masks, bitwise those of
    eager steps 4..8 (and of the host twin); the losses at the oracle's loss tolerance (the DistMult backward and the
    clip norm sum with float atomics)."""
    from mrgcn_amd import host, synth
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.tasks import link_prediction as lp
    from mrgcn_amd.train import ClipAdam, GraphedStep
    g = synth.make_graph("fb15k", seed=0, scale=0.25)
    N, R = g.num_nodes, g.num_relations
    A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([g.rows, g.cols])), torch.from_numpy(g.vals), (N, R * N)).cuda()
    rng = np.random.default_rng(0)
    facts = np.asarray(g.triples, dtype=np.int64)[:20000]
    neg = facts[: len(facts) // 5].copy()
    neg[:, 2] = rng.integers(0, N, len(neg))
    triples = torch.from_numpy(np.concatenate([facts, neg])).cuda()
    Y = torch.cat([torch.ones(len(facts)), torch.zeros(len(neg))]).cuda()
    torch.manual_seed(0)
    model = RGCN([(0, 200, "mrgcn", nn.ReLU())], R, N, 2, P, True, False, True).cuda()
    model.set_node_dropout("device", seed=31)
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    runs = {}
    for graphed in (False, True):
        model.load_state_dict(sd0)
        model.node_dropout_position = 0
        opt = ClipAdam(model.parameters(), lr=LR, max_norm=1.0, capturable=True)

        def step():
            emb = model(None, A)
            loss = lp.binary_crossentropy(lp.score_distmult_bc(triples, emb, model.relations), Y)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            return loss.detach()
        if graphed:
            run = GraphedStep(step, warmup=3)
        else:
            run = step
            for _ in range(3):
                step()
        assert model.node_dropout_position == 3
        losses, masks = [], []
        for _ in range(5):
            losses.append(float(run()))
            masks.append(_np(model.last_node_masks[0]).copy())
        assert model.node_dropout_position == 8
        runs[graphed] = (losses, masks)
        del run, opt
    for k in range(5):
        a, b = runs[False][1][k], runs[True][1][k]
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), k
        assert np.array_equal(b, host.node_dropout_mask(N, P, 31, 3 + k, 0)), k
        np.testing.assert_allclose(runs[True][0][k], runs[False][0][k], rtol=2e-5, atol=1e-6)
    assert len({m.tobytes() for m in runs[True][1]}) == 5, "replays repeated a mask"
