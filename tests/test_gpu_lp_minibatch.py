"""Mini-batch link prediction on the GPU: the wide featureless input layer as a masked pass (csrc/masked_wide.hip)
against the reference's MiniBatch + RGCN._forward_mini_batch (goldens of make_lp_minibatch_goldens.py), the slice
path, the general mix + product pair; batch training steps and per-batch ranking (link_prediction.py:191-530)."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import util

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "lp_minibatch.npz")
MODELS = {"f32b1": (32, 1), "f200b2": (200, 2), "f32b4": (32, 4), "f32b2": (32, 2)}


def _graph():
    from mrgcn_amd.data.batch import scipy_sparse_to_pytorch_sparse
    from mrgcn_amd.plan import plan_of
    g = np.load(GOLD)
    _, A = util.load_graph("graph_small")
    N = A.shape[0]
    R = A.shape[1] // N
    plan = plan_of(scipy_sparse_to_pytorch_sparse(A, dtype=torch.int8).cuda(), N, R)
    return g, A, N, R, plan


def _model(g, tag, N, R):
    from mrgcn_amd.models.rgcn import RGCN
    F, B = MODELS[tag]
    m = RGCN([(0, F, "mrgcn", nn.ReLU())], R, N, B, 0.0, True, False, True)
    m.load_state_dict({k[len(tag) + 6:]: torch.from_numpy(np.array(g[k])) for k in g.files
                       if k.startswith(tag + ".init.")})
    return m.cuda()


def _batches(g, A, plan, masked):
    from mrgcn_amd.tasks import link_prediction as lp
    bs = lp.mkbatches(A, None, g["facts"], 8, 1000, 1, plan=plan if masked else None)
    return lp.prepare_batches(bs, "cuda")


def _loss_grads(model, batch, facts, neg):
    from mrgcn_amd.tasks import link_prediction as lp
    model.zero_grad()
    E = model(None, batch.A)
    tr = torch.from_numpy(np.concatenate([facts, neg])).cuda()
    y = torch.ones(tr.shape[0], device="cuda")
    y[facts.shape[0]:] = 0
    loss = lp.binary_crossentropy(lp.score_distmult_bc(tr, E, model.relations), y)
    loss.backward()
    return E.detach(), float(loss), {n: util.ref_layout(p.grad, n).clone() for n, p in model.named_parameters()}


def _close_relu(ours, ref, rtol=1e-4, atol=1e-5):
    np.testing.assert_allclose(ours, ref, rtol=rtol, atol=atol)
    assert np.array_equal(ours == 0, ref == 0)   # the ReLU's exact zeros


@pytest.mark.parametrize("tag", ["f32b1", "f200b2", "f32b4"])
def test_masked_embeddings_and_grads_vs_reference(tag):
    g, A, N, R, plan = _graph()
    model = _model(g, tag, N, R)
    bs = _batches(g, A, plan, masked=True)
    for i in range(3):
        with torch.no_grad():
            E = model(None, bs[i][0].A).cpu().numpy()
        _close_relu(E, g[f"{tag}.E{i}"])
    _, loss, grads = _loss_grads(model, bs[1][0], bs[1][1], g[f"{tag}.neg"])
    assert abs(loss - float(g[f"{tag}.loss"])) < 1e-5
    for n in ("layers.layer_0.weight_I", "layers.layer_0.weight_I_comp", "relations"):
        np.testing.assert_allclose(grads[n].cpu().numpy(), g[f"{tag}.grad.{n}"], rtol=1e-3, atol=1e-6, err_msg=n)


@pytest.mark.parametrize("tag", ["f32b1", "f200b2"])
def test_slice_path_agrees_with_masked(tag):
    g, A, N, R, plan = _graph()
    model = _model(g, tag, N, R)
    bm, bsl = _batches(g, A, plan, True), _batches(g, A, plan, False)
    for i in (0, 1, 2):
        Em, lm, gm = _loss_grads(model, bm[i][0], bm[i][1], g[f"{tag}.neg"] if i == 1 else np.zeros((0, 3), np.int64))
        Es, ls, gs = _loss_grads(model, bsl[i][0], bsl[i][1], g[f"{tag}.neg"] if i == 1 else np.zeros((0, 3), np.int64))
        _close_relu(Em.cpu().numpy(), Es.cpu().numpy())
        assert abs(lm - ls) < 1e-5
        for n in gm:
            np.testing.assert_allclose(gm[n].cpu().numpy(), gs[n].cpu().numpy(), rtol=1e-3, atol=1e-6, err_msg=n)


@pytest.mark.parametrize("F,B", [(20, 1), (200, 2), (128, 3), (256, 4)])
def test_wide_forward_matches_mix_and_product(F, B):
    from mrgcn_amd import _lib as L
    from mrgcn_amd.data.batch import A_BatchMasked
    g, A, N, R, plan = _graph()
    lib = L.load()
    rng = np.random.default_rng(F + B)
    V = torch.from_numpy(rng.standard_normal((N, B, F)).astype(np.float32)).cuda()
    comp = torch.from_numpy(rng.standard_normal((R, B)).astype(np.float32)).cuda()
    ab = A_BatchMasked(plan, np.array([1, 4, 9, 16, 25, 36, 49]), 1)
    sup = ab.row[0]
    assert lib.mrgcn_support_wide_supported(sup.handle, B, F) == 1
    s = torch.cuda.current_stream().cuda_stream
    ld = (F + 3) // 4 * 4
    M = torch.empty((max(sup.L, 1), ld), device="cuda")
    Y0 = torch.empty((sup.NR, F), device="cuda")
    L.check(lib.mrgcn_support_mix_fwd_f32(sup.handle, V.data_ptr(), comp.data_ptr(), B, F, M.data_ptr(), ld, s), "mix")
    L.check(lib.mrgcn_support_spmm_fwd_f32(sup.handle, 1, M.data_ptr(), ld, F, Y0.data_ptr(), F, 0, 1, s), "spmm")
    Y1 = torch.empty_like(Y0)
    L.check(lib.mrgcn_support_wide_fwd_f32(sup.handle, V.data_ptr(), comp.data_ptr(), B, F, Y1.data_ptr(), F, 1, s),
            "wide")
    torch.cuda.synchronize()
    _close_relu(Y1.cpu().numpy(), Y0.cpu().numpy(), rtol=1e-5, atol=1e-5)
    assert lib.mrgcn_support_wide_supported(sup.handle, B, 16) == 0
    assert lib.mrgcn_support_wide_supported(sup.handle, 5, F) == 0


def test_backward_bitwise_reproducible():
    """The layer's backward from one output gradient twice: the same bits (no float atomics; dcomp and the norm in a
    fixed order).  (The gradient is given: the DistMult backward above it scatters with atomics.)"""
    g, A, N, R, plan = _graph()
    model = _model(g, "f200b2", N, R)
    bs = _batches(g, A, plan, True)
    for i in (0, 1):
        grads = []
        for _ in range(2):
            model.zero_grad()
            E = model(None, bs[i][0].A)
            G = torch.from_numpy(np.random.default_rng(i).standard_normal(tuple(E.shape)).astype(np.float32)).cuda()
            E.backward(G)
            grads.append([p.grad.clone() for n, p in model.named_parameters() if "weight_I" in n])
        assert len(grads[0]) == 2
        for a, b in zip(*grads):
            assert torch.equal(a, b)


def test_three_reference_steps():
    """clip_grad_norm_(1.0) + Adam on consecutive batches with the reference's negatives, row-sparse weight_I: the
    rows outside a later batch move on as the reference's dense Adam has them."""
    from mrgcn_amd.optim import RowSparseAdam
    from mrgcn_amd.tasks import link_prediction as lp
    g, A, N, R, plan = _graph()
    tag = "f32b2"
    model = _model(g, tag, N, R)
    bs = _batches(g, A, plan, True)
    opt = RowSparseAdam(model.parameters(), lr=0.01)
    for s in range(3):
        loss = lp.train_batch_step(model, bs[s][0], bs[s][1], opt, negatives=g[f"{tag}.step{s}.neg"])
        assert abs(float(loss) - float(g[f"{tag}.step{s}.loss"])) < 1e-5
        for n, p in model.named_parameters():
            np.testing.assert_allclose(util.ref_layout(p.detach(), n).cpu().numpy(), g[f"{tag}.step{s}.{n}"],
                                       rtol=1e-4, atol=2e-6, err_msg=f"step {s} {n}")


def test_evaluate_batches_vs_reference_ranks():
    from mrgcn_amd.tasks import link_prediction as lp
    g, A, N, R, plan = _graph()
    model = _model(g, "f200b2", N, R)
    bs = _batches(g, A, plan, True)[:3]
    Rel = model.relations.detach()
    for i in range(3):   # the ranking kernel on the reference's own embeddings: bit-exact
        E = torch.from_numpy(g[f"f200b2.E{i}"]).cuda()
        for kind in ("raw", "flt"):
            rk = lp.compute_ranks_fast(bs[i][1], E, Rel, 50, kind == "flt").cpu().numpy()
            assert np.array_equal(rk, g[f"ranks{i}.{kind}"]), (i, kind)
    mrr, hits, ranks = lp.evaluate_batches(bs, model, filtered=True)
    for kind in ("raw", "flt"):
        per = []
        off = 0
        for i in range(3):
            n = 2 * len(bs[i][1])
            r = np.asarray(ranks[kind][off:off + n])
            off += n
            with torch.no_grad():
                E = model(None, bs[i][0].A)
            ref = lp.compute_ranks_fast(bs[i][1], E, Rel, 50, kind == "flt").cpu().numpy()
            assert np.array_equal(r, ref)
            per.append(r)
        assert off == len(ranks[kind])
        dev = [torch.from_numpy(r).cuda() for r in per]
        assert mrr[kind] == np.mean([torch.mean(1.0 / r.float()).item() for r in dev])
        for j, k in enumerate((1, 3, 10)):
            assert hits[kind][j] == np.mean([float(torch.mean((r <= k).float())) for r in dev])
    mrr2, _, ranks2 = lp.evaluate_batches(bs, model, filtered=False)
    assert mrr2["raw"] == mrr["raw"] and mrr2["flt"] == -1 and ranks2["raw"] == ranks["raw"]


@pytest.mark.parametrize("F,B,featureless", [(200, 0, True), (18, 5, True), (202, 2, True), (200, 2, False)])
def test_unsupported_shapes_raise(F, B, featureless):
    from mrgcn_amd import _lib as L
    from mrgcn_amd.data.batch import A_BatchMasked
    from mrgcn_amd.models.rgcn import RGCN
    _, A, N, R, plan = _graph()
    model = RGCN([(0 if featureless else 6, F, "mrgcn", nn.ReLU())], R, N, B, 0.0, featureless, False, True).cuda()
    ab = A_BatchMasked(plan, np.arange(5), 1)
    X = None if featureless else torch.randn((len(ab.neighbours[-1]), 6), device="cuda")
    with pytest.raises(L.MrgcnError, match="featureless input layer with 1 to 4 bases and 16 < out <= 256"):
        model(X, ab)


def test_fb15k_shape_epochs():
    """At the FB15k-237 synthetic shape: mkbatches(..., 32, 500, 1, plan=...), two epochs of train_epoch with no
    synchronising call inside a step, the loss falls; a few batches' embeddings against the float64 oracle."""
    import scipy.sparse as sp

    from mrgcn_amd import synth
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.optim import RowSparseAdam
    from mrgcn_amd.plan import plan_of
    from mrgcn_amd.tasks import link_prediction as lp
    from oracle import rgcn_oracle as O
    sg = synth.make_graph("fb15k", seed=0)
    N, R = sg.num_nodes, sg.num_relations
    A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([sg.rows, sg.cols])), torch.from_numpy(sg.vals),
                                (N, R * N)).cuda()
    plan = plan_of(A, N, R)
    facts = np.asarray(sg.triples, dtype=np.int64)
    bs = lp.prepare_batches(lp.mkbatches(None, None, facts, 32, 500, 1, plan=plan), "cuda")
    assert len(bs) > 400
    torch.manual_seed(0)
    model = RGCN([(0, 200, "mrgcn", nn.ReLU())], R, N, 2, 0.0, True, False, True).cuda()
    state0 = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    # the embeddings of three batches against the float64 oracle (reference layout of the parameters)
    cfgs, params = O.rgcn_cfgs([(0, 200)], R, N, 2, False, True), O.split_params(state0, 1)
    A_csr = sp.csr_matrix((sg.vals.astype(np.float64), (sg.rows, sg.cols)), shape=(N, R * N))
    for i in (0, len(bs) // 2, len(bs) - 1):
        with torch.no_grad():
            E = model(None, bs[i][0].A).cpu().numpy()
        ref = O.rgcn_forward_at_rows(cfgs, params, None, A_csr, bs[i][0].node_index.cpu().numpy(), relu_last=True)
        np.testing.assert_allclose(E, ref, rtol=1e-4, atol=1e-5)
    opt = RowSparseAdam(model.parameters(), lr=0.01)
    lp.train_batch_step(model, bs[0][0], bs[0][1], opt)   # (first use: lazily built workspaces)
    torch.cuda.synchronize()
    losses = []
    for _ in range(2):
        torch.cuda.set_sync_debug_mode("error")   # (a synchronising call inside a step raises)
        try:
            steps = [lp.train_batch_step(model, b, f, opt) for b, f in bs]
        finally:
            torch.cuda.set_sync_debug_mode("default")
        losses.append(float(torch.stack(steps).mean()))
    assert np.isfinite(losses).all() and losses[1] < losses[0], losses
    mrr, _, _ = lp.evaluate_batches(bs[:20], model, filtered=True)
    assert 0.0 < mrr["raw"] <= mrr["flt"] <= 1.0
