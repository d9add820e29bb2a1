"""Mini-batch link prediction with literal features on the masked pass: wide layers WITH a feature term (the basis form
P = X . V_F, csrc/basis_xform.hip, and the two-table gather, csrc/masked_wide.hip) against the reference's
MiniBatch + RGCN._forward_mini_batch / MRGCN (goldens of make_lp_multimodal_goldens.py) and the slice path."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import util

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "lp_multimodal.npz")
MODELS = {"k6f200b2": (6, 200, 2), "k145f200b2": (145, 200, 2), "k37f32b1": (37, 32, 1), "k13f32b4": (13, 32, 4)}
KMAX, STRIDE = 145, 7


def _graph():
    from mrgcn_amd.data.batch import scipy_sparse_to_pytorch_sparse
    from mrgcn_amd.plan import plan_of
    g = np.load(GOLD)
    _, A = util.load_graph("graph_small")
    N = A.shape[0]
    R = A.shape[1] // N
    plan = plan_of(scipy_sparse_to_pytorch_sparse(A, dtype=torch.int8).cuda(), N, R)
    return g, A, N, R, plan


def _features(N):
    return np.random.default_rng(41).standard_normal((N, KMAX)).astype(np.float32)   # (make_lp_multimodal_goldens)


def _init(model, seed):
    sd = model.state_dict()   # (the reference's layout)
    rng = np.random.default_rng(seed)
    model.load_state_dict({k: torch.from_numpy(rng.uniform(-0.2, 0.2, tuple(sd[k].shape)).astype(np.float32))
                           for k in sorted(sd)})
    return model


def _model(tag, N, R):
    from mrgcn_amd.models.rgcn import RGCN
    K, F, B = MODELS[tag]
    return _init(RGCN([(K, F, "mrgcn", nn.ReLU())], R, N, B, 0.0, False, False, True), 5).cuda()


def _batches(g, A, plan, masked, num_layers=1):
    from mrgcn_amd.tasks import link_prediction as lp
    bs = lp.mkbatches(A, None, g["facts"], 8, 1000, num_layers, plan=plan if masked else None)
    return lp.prepare_batches(bs, "cuda")


def _with_x(batch, X, K, by_node=False):
    """The batch's feature rows: the outermost neighbours' (the reference's X[neighbours[-1]]) or all N rows."""
    Xd = torch.from_numpy(np.ascontiguousarray(X[:, :K])).cuda()
    batch.X = Xd if by_node else Xd.index_select(0, batch.A.neighbours[-1].to("cuda").long())
    return batch


def _slice_model(model, F):
    """The model for the slice path: the fused engine's slice transform takes out <= 64, wider layers with a feature
    term run the literal engine there (graph.py's arithmetic op for op)."""
    if F <= 64:
        return model
    m = copy.deepcopy(model)
    m.set_engine("literal")
    return m


def _stored(g, key, a):
    """The golden's array (every STRIDE-th element and the sum when it was large) and ours in the same form."""
    a = np.asarray(a)
    want = g[key]
    if key + ".sum" in g.files:
        np.testing.assert_allclose(a.astype(np.float64).sum(), float(g[key + ".sum"]), rtol=1e-3,
                                   atol=1e-4 * a.size ** 0.5, err_msg=key)
        a = a.reshape(-1)[::STRIDE]
    return a.reshape(want.shape), want


def _close_relu(ours, pre, rtol=1e-4, atol=1e-5):
    """ours == relu(pre) within the tolerances, and the exact zeros of the ReLU where pre is not within 1e-6 of 0."""
    ref = np.maximum(pre, 0)
    np.testing.assert_allclose(ours, ref, rtol=rtol, atol=atol)
    near = np.abs(pre) <= 1e-6
    assert int(near.sum()) <= max(1, ours.size // 1000), f"{int(near.sum())} of {ours.size} near 0"
    assert np.array_equal((ours == 0)[~near], (ref == 0)[~near])
    return int(near.sum())


def _loss_grads(model, batch, facts, neg, x_grad=True):
    from mrgcn_amd.tasks import link_prediction as lp
    model.zero_grad()
    X = batch.X.detach().clone().requires_grad_(x_grad) if batch.X is not None else None
    E = model(X, batch.A)
    tr = torch.from_numpy(np.concatenate([facts, neg])).cuda()
    y = torch.ones(tr.shape[0], device="cuda")
    y[facts.shape[0]:] = 0
    loss = lp.binary_crossentropy(lp.score_distmult_bc(tr, E, model.relations), y)
    loss.backward()
    grads = {n: util.ref_layout(p.grad, n).clone() for n, p in model.named_parameters() if p.grad is not None}
    if x_grad and X is not None:
        grads["X"] = X.grad.clone()
    return E.detach(), float(loss), grads


@pytest.mark.parametrize("tag", list(MODELS))
def test_masked_embeddings_and_grads_vs_reference(tag):
    import mrgcn_amd
    g, A, N, R, plan = _graph()
    K = MODELS[tag][0]
    X = _features(N)
    model = _model(tag, N, R)
    bs = _batches(g, A, plan, masked=True)
    mrgcn_amd.reset_stats()
    excluded = 0
    for i in range(3):
        b = _with_x(bs[i][0], X, K)
        assert np.array_equal(b.A.neighbours[-1].cpu().numpy(), g[f"b{i}.outer"])
        with torch.no_grad():
            E = model(b.X, b.A).cpu().numpy()
        excluded += _close_relu(E, g[f"{tag}.pre{i}"])
    print(f"{tag}: {excluded} elements within 1e-6 of 0 excluded from the zero-pattern check")
    _, loss, grads = _loss_grads(model, bs[1][0], bs[1][1], g[f"{tag}.neg"])
    assert abs(loss - float(g[f"{tag}.loss"])) < 1e-5
    names = ["layers.layer_0.weight_I", "layers.layer_0.weight_I_comp", "layers.layer_0.weight_F",
             "layers.layer_0.weight_F_comp", "relations", "X"]
    for n in names:
        got, want = _stored(g, f"{tag}.grad.{n}", grads[n].cpu().numpy())
        np.testing.assert_allclose(got, want, rtol=1e-3, atol=1e-6, err_msg=n)
    st = mrgcn_amd.stats()
    assert st.get("masked.wide_feat") == 4 and st.get("weight_I.wide_feat") == 1, st


@pytest.mark.parametrize("opt_kind", ["ClipAdam", "RowSparseAdam"])
def test_three_reference_steps(opt_kind):
    from mrgcn_amd.optim import RowSparseAdam
    from mrgcn_amd.tasks import link_prediction as lp
    from mrgcn_amd.train import ClipAdam
    g, A, N, R, plan = _graph()
    tag = "k6f200b2"
    X = _features(N)
    model = _model(tag, N, R)
    bs = _batches(g, A, plan, True)
    opt = ClipAdam(model.parameters(), lr=0.01, max_norm=1.0) if opt_kind == "ClipAdam" else \
        RowSparseAdam(model.parameters(), lr=0.01)
    for s in range(3):
        b = _with_x(bs[s][0], X, 6)
        loss = lp.train_batch_step(model, b, bs[s][1], opt, negatives=g[f"{tag}.step{s}.neg"])
        assert abs(float(loss) - float(g[f"{tag}.step{s}.loss"])) < 1e-5
    for n, p in model.state_dict().items():
        got, want = _stored(g, f"{tag}.final.{n}", p.detach().cpu().numpy())
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5, err_msg=n)


def test_two_layers_hidden_wide_layer_vs_reference():
    """A featureless 32-wide input layer, then a hidden 32 -> 200 layer with 2 bases (feature table only)."""
    import mrgcn_amd
    from mrgcn_amd.models.rgcn import RGCN
    g, A, N, R, plan = _graph()
    model = _init(RGCN([(0, 32, "mrgcn", nn.ReLU()), (32, 200, "mrgcn", nn.ReLU())], R, N, 2, 0.0, True, False, True),
                  6).cuda()
    bs = _batches(g, A, plan, True, num_layers=2)
    mrgcn_amd.reset_stats()
    for i in range(2):
        assert np.array_equal(bs[i][0].node_index.cpu().numpy(), g[f"two.b{i}.nodes"])
        with torch.no_grad():
            E = model(None, bs[i][0].A).cpu().numpy()
        np.testing.assert_allclose(E, g[f"two.E{i}"], rtol=1e-4, atol=1e-5)
    _, loss, grads = _loss_grads(model, bs[1][0], bs[1][1], g["two.neg"])
    assert abs(loss - float(g["two.loss"])) < 1e-5
    for n in grads:
        got, want = _stored(g, f"two.grad.{n}", grads[n].cpu().numpy())
        np.testing.assert_allclose(got, want, rtol=1e-3, atol=1e-6, err_msg=n)
    st = mrgcn_amd.stats()
    assert st.get("masked.wide_feat") == 3 and "weight_I.wide_feat" not in st, st


@pytest.mark.parametrize("path", ["host", "device"])
def test_mrgcn_link_prediction_vs_reference(path):
    """MRGCN(link_prediction=True): one xsd.numeric MLP set feeding a 200-wide, 2-basis layer, batches from
    mkbatches(A, X, facts, 8, 1000, 1, plan=...) with X a host feature list or a DeviceEncodings."""
    import mrgcn_amd
    from mrgcn_amd.data.batch import DeviceEncodings
    from mrgcn_amd.models.mrgcn import MRGCN
    from mrgcn_amd.train import ClipAdam
    from mrgcn_amd.tasks import link_prediction as lp
    g, A, N, R, plan = _graph()
    nodes, enc = g["num.nodes"], g["num.enc"]
    feats = [np.empty((N, 0), dtype=np.float32),
             ["xsd.numeric", [[enc.copy(), nodes.copy(), np.ones(len(nodes), dtype=np.int32)]], False]]
    X = DeviceEncodings(feats, "cuda") if path == "device" else feats
    torch.manual_seed(7)
    model = MRGCN([(3, 200, "mrgcn", nn.ReLU())], [("xsd.numeric", (3, 3, 0.0), False)], R, N, num_bases=2,
                  p_dropout=0.0, featureless=False, bias=False, link_prediction=True, gcn_gpu_acceleration=True)
    assert sorted(model.state_dict()) == [str(k) for k in g["mrgcn.keys"]]
    _init(model, 8)
    model = model.cuda()
    bs = lp.mkbatches(None, X, g["facts"], 8, 1000, 1, plan=plan)
    for b, _ in bs:
        b.pad_(pad_symbols={})
        b.to_dense_()
        b.as_tensors_()
        b.to(model.devices)
    lp.prepare_batches(bs, "cuda")
    mrgcn_amd.reset_stats()
    with torch.no_grad():
        for i in range(2):
            np.testing.assert_allclose(model(bs[i][0]).cpu().numpy(), g[f"mrgcn.E{i}"], rtol=1e-4, atol=1e-5)
    assert mrgcn_amd.stats().get("masked.wide_feat") == 2
    batch, facts = bs[1]
    model.zero_grad()
    E = model(batch)
    tr = torch.from_numpy(np.concatenate([facts, g["mrgcn.neg"]])).cuda()
    y = torch.ones(tr.shape[0], device="cuda")
    y[facts.shape[0]:] = 0
    loss = lp.binary_crossentropy(lp.score_distmult_bc(tr, E, model.rgcn.relations), y)
    loss.backward()
    assert abs(float(loss) - float(g["mrgcn.loss"])) < 1e-5
    sd = dict(model.named_parameters())
    for k in g["mrgcn.grad_keys"]:
        k = str(k)
        got, want = _stored(g, f"mrgcn.grad.{k}", util.ref_layout(sd[k].grad.detach(), k).cpu().numpy())
        np.testing.assert_allclose(got, want, rtol=1e-3, atol=1e-6, err_msg=k)
    model.zero_grad()
    opt = ClipAdam(model.parameters(), lr=0.01, max_norm=1.0)
    for s in range(3):
        loss = lp.train_batch_step(model, bs[s][0], bs[s][1], opt, negatives=g[f"mrgcn.step{s}.neg"])
        assert abs(float(loss) - float(g[f"mrgcn.step{s}.loss"])) < 1e-5
    for n, p in model.state_dict().items():
        got, want = _stored(g, f"mrgcn.final.{n}", p.detach().cpu().numpy())
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5, err_msg=n)


@pytest.mark.parametrize("tag,by_node", [("k6f200b2", False), ("k145f200b2", True), ("k13f32b4", False)])
def test_slice_path_agrees_with_masked(tag, by_node):
    g, A, N, R, plan = _graph()
    K = MODELS[tag][0]
    X = _features(N)
    model = _model(tag, N, R)
    bm, bsl = _batches(g, A, plan, True), _batches(g, A, plan, False)
    for i in (0, 1, 2):
        neg = g[f"{tag}.neg"] if i == 1 else np.zeros((0, 3), np.int64)
        Em, lm, gm = _loss_grads(model, _with_x(bm[i][0], X, K, by_node), bm[i][1], neg)
        Es, ls, gs = _loss_grads(_slice_model(model, MODELS[tag][1]), _with_x(bsl[i][0], X, K), bsl[i][1], neg)
        np.testing.assert_allclose(Em.cpu().numpy(), Es.cpu().numpy(), rtol=1e-4, atol=1e-5)
        assert abs(lm - ls) < 1e-5
        if by_node:   # the whole matrix's gradient: zeros outside the neighbours
            nb = bm[i][0].A.neighbours[-1].long()
            outside = torch.ones(gm["X"].shape[0], dtype=torch.bool, device="cuda")
            outside[nb] = False
            assert not bool(gm["X"][outside].any())
            gm["X"] = gm["X"][nb]
        for n in gm:
            np.testing.assert_allclose(gm[n].cpu().numpy(), gs[n].cpu().numpy(), rtol=1e-3, atol=1e-6, err_msg=n)


def test_hidden_layer_slice_path_agrees_with_masked():
    from mrgcn_amd.models.rgcn import RGCN
    g, A, N, R, plan = _graph()
    model = _init(RGCN([(0, 32, "mrgcn", nn.ReLU()), (32, 200, "mrgcn", nn.ReLU())], R, N, 2, 0.0, True, False, True),
                  6).cuda()
    bm, bsl = _batches(g, A, plan, True, 2), _batches(g, A, plan, False, 2)
    for i in (0, 1):
        neg = g["two.neg"] if i == 1 else np.zeros((0, 3), np.int64)
        Em, lm, gm = _loss_grads(model, bm[i][0], bm[i][1], neg)
        Es, ls, gs = _loss_grads(_slice_model(model, 200), bsl[i][0], bsl[i][1], neg)
        np.testing.assert_allclose(Em.cpu().numpy(), Es.cpu().numpy(), rtol=1e-4, atol=1e-5)
        for n in gm:
            np.testing.assert_allclose(gm[n].cpu().numpy(), gs[n].cpu().numpy(), rtol=1e-3, atol=1e-6, err_msg=n)


@pytest.mark.parametrize("tag", ["k145f200b2", "k13f32b4"])
def test_backward_bitwise_reproducible(tag):
    g, A, N, R, plan = _graph()
    K = MODELS[tag][0]
    X = _features(N)
    model = _model(tag, N, R)
    bs = _batches(g, A, plan, True)
    for i in (0, 1):
        b = _with_x(bs[i][0], X, K)
        grads = []
        for _ in range(2):
            model.zero_grad()
            x = b.X.detach().clone().requires_grad_(True)
            E = model(x, b.A)
            G = torch.from_numpy(np.random.default_rng(i).standard_normal(tuple(E.shape)).astype(np.float32)).cuda()
            E.backward(G)
            grads.append([p.grad.clone() for n, p in model.named_parameters() if "layer_0" in n] + [x.grad.clone()])
        assert len(grads[0]) == 5
        for a, c in zip(*grads):
            assert torch.equal(a, c)


def test_default_batch_still_refuses_featured_wide_layer():
    from mrgcn_amd import _lib as L
    from mrgcn_amd.data.batch import A_BatchMasked
    from mrgcn_amd.models.rgcn import RGCN
    _, A, N, R, plan = _graph()
    model = RGCN([(6, 200, "mrgcn", nn.ReLU())], R, N, 2, 0.0, False, False, True).cuda()
    ab = A_BatchMasked(plan, np.arange(5), 1)
    X = torch.randn((len(ab.neighbours[-1]), 6), device="cuda")
    with pytest.raises(L.MrgcnError, match="featureless input layer with 1 to 4 bases and 16 < out <= 256") as e:
        model(X, ab)
    assert "wide_features=True" in str(e.value)
    ab2 = A_BatchMasked(plan, np.arange(5), 1, wide_features=True)
    assert model(X, ab2).shape == (5, 200)


@pytest.mark.parametrize("F,B", [(200, 0), (200, 5), (202, 2)])
def test_shapes_outside_the_family_raise_on_opted_in_batches(F, B):
    from mrgcn_amd import _lib as L
    from mrgcn_amd.data.batch import A_BatchMasked
    from mrgcn_amd.models.rgcn import RGCN
    _, A, N, R, plan = _graph()
    model = RGCN([(6, F, "mrgcn", nn.ReLU())], R, N, B, 0.0, False, False, True).cuda()
    ab = A_BatchMasked(plan, np.arange(5), 1, wide_features=True)
    X = torch.randn((len(ab.neighbours[-1]), 6), device="cuda")
    with pytest.raises(L.MrgcnError, match="featureless input layer with 1 to 4 bases and 16 < out <= 256"):
        model(X, ab)


def test_fb15k_shape_epochs_with_features():
    """At the FB15k-237 synthetic shape with 145 feature columns (the YAGO3-10+ width): two train_epoch passes with
    no synchronising call inside a step, the loss falls; a few batches' embeddings against the slice path."""
    from mrgcn_amd import synth
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.optim import RowSparseAdam
    from mrgcn_amd.plan import plan_of
    from mrgcn_amd.tasks import link_prediction as lp
    sg = synth.make_graph("fb15k", seed=0)
    N, R = sg.num_nodes, sg.num_relations
    A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([sg.rows, sg.cols])), torch.from_numpy(sg.vals),
                                (N, R * N)).cuda()
    plan = plan_of(A, N, R)
    facts = np.asarray(sg.triples, dtype=np.int64)
    Xd = torch.full((N, 145), 0.05, device="cuda") + torch.linspace(0, 0.1, 145, device="cuda")
    bs = lp.prepare_batches(lp.mkbatches(None, None, facts, 32, 500, 1, plan=plan), "cuda")
    for b, _ in bs:
        b.X = Xd   # (all N rows: the layer reads the neighbours' rows through the support)
    torch.manual_seed(0)
    model = RGCN([(145, 200, "mrgcn", nn.ReLU())], R, N, 2, 0.0, False, False, True).cuda()
    # a few batches against the slice path (the reference's slices of the same batches)
    import scipy.sparse as sp
    A_csr = sp.csr_matrix((sg.vals.astype(np.float32), (sg.rows, sg.cols)), shape=(N, R * N))
    for i in (0, len(bs) // 2):
        from mrgcn_amd.data.batch import MiniBatch
        ms = MiniBatch(A_csr, None, bs[i][0].node_index.cpu().numpy(), 1, value_mode="norm_f32")   # (the plan's values)
        ms.as_tensors_()
        ms.to({"relational": torch.device("cuda")})
        with torch.no_grad():
            Em = model(Xd, bs[i][0].A)
            Es = _slice_model(model, 200)(Xd.index_select(0, ms.A.neighbours[-1].cuda().long()), ms.A)
        np.testing.assert_allclose(Em.cpu().numpy(), Es.cpu().numpy(), rtol=1e-4, atol=1e-5)
    opt = RowSparseAdam(model.parameters(), lr=0.01)
    lp.train_batch_step(model, bs[0][0], bs[0][1], opt)   # (first use: lazily built workspaces)
    torch.cuda.synchronize()
    losses = []
    for _ in range(2):
        torch.cuda.set_sync_debug_mode("error")
        try:
            steps = [lp.train_batch_step(model, b, f, opt) for b, f in bs]
        finally:
            torch.cuda.set_sync_debug_mode("default")
        losses.append(float(torch.stack(steps).mean()))
    assert np.isfinite(losses).all() and losses[1] < losses[0], losses
    mrr, _, _ = lp.evaluate_batches(bs[:20], model, filtered=True)
    assert 0.0 < mrr["raw"] <= mrr["flt"] <= 1.0
