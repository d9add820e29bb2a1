"""Node dropout on the device, every path it is advertised on against an independent float64 reference with explicit
masks: the featureless wide link-prediction layer in full batch (F > 16: the wide-input backward), masked mini-batches
(the narrow `_MaskedLayer` pair of the `minibatch_small` golden and a `wide_features=True` link-prediction batch),
the literal product of a featureless layer without bases, the bf16 pipeline, and the slice walk's row-scale node.

The float64 composition is the oracle's `layer_forward` / `layer_backward` with the node masks applied to every layer's
output, its `cross_entropy`, `clip_grad_norm` and `Adam`.  A masked batch built with `full_batch_values=True` computes
the full-batch arithmetic on the batch's receptive field, so its reference is the same composition on the whole graph
with the loss over the batch's rows and each layer's compact mask scattered to that layer's rows (ones elsewhere: those
rows reach no batch row).  Tolerances: tests/test_gpu_step_oracle.py's, f32 and bf16."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import util
from tests.test_gpu_node_dropout import P, _case, _masks_with_a_dropped_label_and_hub, _np, _oracle_step
from tests.test_gpu_step_oracle import BF16_TOL, LR, _check_adam, _close_bf16, _close_bf16_values, _close_grad

pytestmark = pytest.mark.gpu

KEEP = np.float32(1.0) / np.float32(1.0 - P)


def _compose(cfgs, state, X, A64, masks, relu, idx, y):
    """One step in float64: layer l's output is masks[l] . act_l(pre_l); CE over rows `idx`; clip 1.0; Adam."""
    from oracle import rgcn_oracle as O
    params = O.split_params(state, len(cfgs))
    H, tape = X, []
    for cfg, p, m, act in zip(cfgs, params, masks, relu):
        pre, cache = O.layer_forward(cfg, p, H, A64)
        tape.append((H, pre, cache))
        H = m.astype(np.float64)[:, None] * (np.maximum(pre, 0.0) if act else pre)
    loss, dH = O.cross_entropy(H, idx, y)
    grads = {}
    for li in reversed(range(len(cfgs))):
        Hin, pre, cache = tape[li]
        dpre = masks[li].astype(np.float64)[:, None] * dH
        if relu[li]:
            dpre = dpre * (pre > 0)
        g, dH = O.layer_backward(cfgs[li], params[li], Hin, A64, dpre, cache)
        grads.update({f"layers.layer_{li}.{k}": v for k, v in g.items()})
    norm, coef = O.clip_grad_norm(list(grads.values()), 1.0)
    return dict(logits=H, loss=loss, grads=grads, norm=norm, coef=coef, before=state)


def _state64(model):
    return {k: _np(v).astype(np.float64) for k, v in model.state_dict().items()}


def _step_and_check(name, model, forward, rows, y, ora, ora_rows):
    """forward -> torch's cross-entropy over `rows` of the output -> backward -> ClipAdam; everything against `ora`."""
    from mrgcn_amd.train import ClipAdam
    opt = ClipAdam(list(model.parameters()), lr=LR, max_norm=1.0)
    out = forward()
    np.testing.assert_allclose(_np(out)[rows], ora["logits"][ora_rows], rtol=1e-4, atol=1e-4)
    loss = torch.nn.functional.cross_entropy(out[torch.from_numpy(rows).cuda()], torch.from_numpy(y).cuda())
    opt.zero_grad(set_to_none=True)
    loss.backward()
    np.testing.assert_allclose(float(loss), ora["loss"], rtol=2e-5, atol=1e-6)
    named = [(n, p) for n, p in model.named_parameters() if n in ora["grads"]]
    assert len(named) == len(ora["grads"])
    for n, p in named:
        assert p.grad is not None, n
        _close_grad(_np(util.ref_layout(p.grad, n)), ora["grads"][n], f"{name}: grad {n}")
    opt.step()
    np.testing.assert_allclose(opt.last_grad_norm(), ora["norm"], rtol=2e-5)
    sd = model.state_dict()
    for n, p in named:
        st = opt.state[p]
        _check_adam(f"{name}: {n}", ora["before"][n], ora["grads"][n], ora["coef"], _np(sd[n]),
                    _np(util.ref_layout(st["exp_avg"], n)), _np(util.ref_layout(st["exp_avg_sq"], n)))


def _small_graph():
    from mrgcn_amd.plan import plan_of
    g, A_csr = util.load_graph("graph_small")
    N, R = int(g["num_nodes"]), 2 * int(g["num_pred"]) + 1
    A = util.coo_tensor(A_csr, "norm_f32", "cuda")
    return A_csr.astype(np.float64), A, N, R, plan_of(A, N, R)


def _mask(rng, n, dropped=(), kept=()):
    m = np.where(rng.random(n) < P, np.float32(0), KEEP).astype(np.float32)
    m[list(dropped)] = 0.0
    m[list(kept)] = KEEP
    return m


# ---- the featureless wide link-prediction shape, full batch --------------------------------------------------------
def test_wide_featureless_layer_with_explicit_mask_against_the_float64_composition():
    """RGCN [(0 -> 200, ReLU)], 2 bases, link prediction: `_RgcnLayer` at F > 16, whose backward is the wide-input
    kernel straight from the (scaled) output gradient.  One labelled node and the hub are dropped."""
    import mrgcn_amd
    from mrgcn_amd.models.rgcn import RGCN
    from oracle import rgcn_oracle as O
    A64, A, N, R, _ = _small_graph()
    torch.manual_seed(5)
    model = RGCN([(0, 200, "mrgcn", nn.ReLU())], R, N, 2, P, True, False, True).cuda()
    rng = np.random.default_rng(5)
    rows = np.sort(rng.choice(N, 20, replace=False))
    y = rng.integers(0, 200, len(rows))
    hub = int(np.bincount(A64.indices % N, minlength=N).argmax())
    m = _mask(rng, N, dropped=(rows[0], hub), kept=(rows[1],))
    cfgs = O.rgcn_cfgs([(0, 200)], R, N, 2, False, True)
    ora = _compose(cfgs, _state64(model), None, A64, [m], [True], rows, y)
    model.set_node_dropout("device")
    model.node_dropout_masks = [torch.from_numpy(m).cuda()]
    mrgcn_amd.reset_stats()
    _step_and_check("wide featureless", model, lambda: model(None, A), rows, y, ora, rows)
    st = mrgcn_amd.stats()
    assert st.get("backward.wide_input") == 1 and st.get("node_dropout.device") == 1, st
    assert model.relations.grad is None


# ---- masked mini-batches ---------------------------------------------------------------------------------------------
def test_masked_batch_of_the_minibatch_golden_against_the_float64_composition():
    """The `minibatch_small` golden's batch (features, 3 bases, bias; 5 -> 6 -> 4) as a masked batch: `_MaskedLayer`
    twice with `row_scale`, ReLU fused.  One batch node is dropped in the top mask, one neighbour in the hidden one."""
    import mrgcn_amd
    from mrgcn_amd.data.batch import A_BatchMasked
    from mrgcn_amd.models.rgcn import RGCN
    from oracle import rgcn_oracle as O
    c = util.load_case("minibatch_small")
    A64, A, N, R, plan = _small_graph()
    batch_idx = np.asarray(c["batch_idx"], dtype=np.int64)
    y = np.asarray(c["ft_b3.y"], dtype=np.int64)
    X = np.asarray(c["ft_b3.X_full"], dtype=np.float32)
    model = RGCN([(5, 6, "mrgcn", nn.ReLU()), (6, 4, "mrgcn", None)], R, N, 3, P, False, True, False)
    model.load_state_dict({k[len("ft_b3.init."):]: torch.from_numpy(np.array(c[k])) for k in c.files
                           if k.startswith("ft_b3.init.")}, strict=True)
    model = model.cuda()
    ab = A_BatchMasked(plan, batch_idx, 2, full_batch_values=True)
    top_rows = np.unique(batch_idx)                 # rows of the top layer's support, rising
    hid_rows = _np(ab.neighbours[0])                # rows of the hidden layer's support: the batch rows' source nodes
    assert int(ab.row[0].NR) == len(top_rows) and int(ab.row[1].NR) == len(hid_rows)
    rng = np.random.default_rng(7)
    m_hid = _mask(rng, len(hid_rows), dropped=(0,), kept=(1,))
    m_top = _mask(rng, len(top_rows), dropped=(2,), kept=(0,))
    full_hid, full_top = np.ones(N, np.float32), np.ones(N, np.float32)
    full_hid[hid_rows], full_top[top_rows] = m_hid, m_top
    cfgs = O.rgcn_cfgs([(5, 6), (6, 4)], R, N, 3, True, False)
    ora = _compose(cfgs, _state64(model), X, A64, [full_hid, full_top], [True, False], batch_idx, y)
    model.set_node_dropout("device")
    model.node_dropout_masks = [torch.from_numpy(m_hid).cuda(), torch.from_numpy(m_top).cuda()]
    Xn = torch.from_numpy(X).cuda().index_select(0, ab.neighbours[-1])
    mrgcn_amd.reset_stats()
    _step_and_check("masked batch", model, lambda: model(Xn, ab), np.arange(len(batch_idx)), y, ora, batch_idx)
    assert mrgcn_amd.stats().get("node_dropout.device") == 2
    assert not _np(model(Xn, ab))[np.isin(batch_idx, top_rows[m_top == 0])].any()


def test_wide_features_batch_against_the_float64_composition():
    """A `wide_features=True` link-prediction batch (the nodes of the `lp_minibatch` golden's first batch): one
    7 -> 200 layer with an input and a feature term, 2 bases, ReLU — `_MaskedWideFeat` with `row_scale`."""
    import mrgcn_amd
    from mrgcn_amd.data.batch import A_BatchMasked
    from mrgcn_amd.models.rgcn import RGCN
    from oracle import rgcn_oracle as O
    A64, A, N, R, plan = _small_graph()
    nodes = np.asarray(util.load_case("lp_minibatch")["full.0.nodes"], dtype=np.int64)
    rng = np.random.default_rng(9)
    X = rng.standard_normal((N, 7)).astype(np.float32)
    y = rng.integers(0, 200, len(nodes))
    torch.manual_seed(9)
    model = RGCN([(7, 200, "mrgcn", nn.ReLU())], R, N, 2, P, False, False, True).cuda()
    ab = A_BatchMasked(plan, nodes, 1, full_batch_values=True, wide_features=True)
    rows = np.unique(nodes)
    m = _mask(rng, len(rows), dropped=(1,), kept=(0,))
    full = np.ones(N, np.float32)
    full[rows] = m
    cfgs = O.rgcn_cfgs([(7, 200)], R, N, 2, False, False)
    ora = _compose(cfgs, _state64(model), X, A64, [full], [True], nodes, y)
    model.set_node_dropout("device")
    model.node_dropout_masks = [torch.from_numpy(m).cuda()]
    Xn = torch.from_numpy(X).cuda().index_select(0, ab.neighbours[-1])
    mrgcn_amd.reset_stats()
    _step_and_check("wide features batch", model, lambda: model(Xn, ab), np.arange(len(nodes)), y, ora, nodes)
    st = mrgcn_amd.stats()
    assert st.get("masked.wide_feat") == 1 and st.get("node_dropout.device") == 1, st


# ---- the literal product of a featureless layer without bases -------------------------------------------------------
@pytest.mark.parametrize("name", ["rgcn_small_fl_b0_bias_norm_f32", "rgcn_small_fl_b0_nobias_norm_f32"])
def test_featureless_layer_without_bases_against_the_float64_composition(name):
    """Layer 0 is `_SpmmLiteral` (weight_I is the operand itself) with `row_scale`; both gradient forms of weight_I."""
    from mrgcn_amd.train import ClipAdam, train_step
    c, model, dims, A_csr, A, X, idx, tgt = _case(name)
    assert X is None and int(c["meta.num_bases"]) <= 0
    N = int(c["meta.num_nodes"])
    masks = _masks_with_a_dropped_label_and_hub(c, A_csr, N, seed=4)
    ora = _oracle_step(c, dims, A_csr, None, masks)
    model.set_node_dropout("device")
    model.node_dropout_masks = [torch.from_numpy(m).cuda() for m in masks]
    for row_sparse in (False, None):
        util.load_state_from_case(model, c)
        model.zero_grad(set_to_none=True)
        opt = ClipAdam(list(model.parameters()), lr=LR, max_norm=1.0)
        with torch.no_grad():
            np.testing.assert_allclose(_np(model(X, A)), ora["logits"], rtol=1e-4, atol=1e-4)
        loss = train_step(model, lambda: model(X, A), idx, tgt, opt, row_sparse=row_sparse)
        np.testing.assert_allclose(float(loss), ora["loss"], rtol=2e-5, atol=1e-6)
        np.testing.assert_allclose(opt.last_grad_norm(), ora["norm"], rtol=2e-5)
        sd = model.state_dict()
        for n, p in model.named_parameters():
            if row_sparse is False:
                _close_grad(_np(p.grad), ora["grads"][n], f"{name}: grad {n}")
            st = opt.state[p]
            _check_adam(f"{name}: {n}", ora["before"][n], ora["grads"][n], ora["coef"], _np(sd[n]),
                        _np(st["exp_avg"]), _np(st["exp_avg_sq"]))


# ---- the bf16 pipeline -----------------------------------------------------------------------------------------------
def test_bf16_operands_with_explicit_masks_against_the_float64_composition():
    """operand_dtype "bf16" (the compact operand stored in bf16, fp32 accumulation and outputs) with device dropout:
    the scale is applied to the fp32 output.  Against the fp32 model's float64 composition at the bf16 run's stated
    tolerance (tests/test_gpu_step_oracle.py: logits and loss 2e-2, gradients `_close_bf16`, the basis coefficients'
    gradients by direction and size)."""
    from mrgcn_amd.train import ClipAdam, train_step
    name = "rgcn_small_ft_b3_bias_norm_f32"
    c, model, dims, A_csr, A, X, idx, tgt = _case(name)
    masks = _masks_with_a_dropped_label_and_hub(c, A_csr, int(c["meta.num_nodes"]), seed=6)
    ora = _oracle_step(c, dims, A_csr, c["X"], masks)
    model.set_node_dropout("device")
    model.node_dropout_masks = [torch.from_numpy(m).cuda() for m in masks]
    model.set_operand_dtype("bf16")
    with torch.no_grad():
        logits = _np(model(X, A))
    _close_bf16_values(logits, ora["logits"], "bf16 logits")
    assert np.abs(logits - ora["logits"]).max() > 1e-6, "bit-equal to the fp32 result: the bf16 path did not run"
    assert not logits[masks[1] == 0].any()
    opt = ClipAdam(list(model.parameters()), lr=LR, max_norm=1.0)
    loss = train_step(model, lambda: model(X, A), idx, tgt, opt, row_sparse=False)
    assert abs(float(loss) - ora["loss"]) <= BF16_TOL * abs(ora["loss"])
    for n, p in model.named_parameters():
        got, ref = _np(util.ref_layout(p.grad, n)).astype(np.float64), ora["grads"][n]
        if n.endswith("_comp"):
            a, b = got.ravel(), ref.ravel()
            cos = float(a @ b) / max(np.linalg.norm(a) * np.linalg.norm(b), 1e-300)
            assert cos > 0.99 and abs(np.linalg.norm(a) / np.linalg.norm(b) - 1) < 5e-2, (n, cos)
        else:
            _close_bf16(got, ref, f"bf16: grad {n}")
    assert abs(opt.last_grad_norm() - ora["norm"]) <= BF16_TOL * ora["norm"]


# ---- the slice walk's row-scale node ----------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,F", [(48, 6), (9, 4), (300, 200), (65, 11)])
def test_row_scale_node_forward_and_backward_equal_the_torch_product(rows, F):
    from mrgcn_amd import functional as Fn
    g = torch.Generator("cuda").manual_seed(rows * F)
    X = torch.randn((rows, F), device="cuda", generator=g)
    m = (torch.rand(rows, device="cuda", generator=g) > P).float() * float(KEEP)
    W = torch.randn((rows, F), device="cuda", generator=g)
    grads = []
    for fn in (lambda x: Fn.row_scale(x, m), lambda x: x * m[:, None]):
        x = X.clone().requires_grad_(True)
        y = fn(torch.relu(x))
        (y * W).sum().backward()
        grads.append((y.detach(), x.grad))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])


def test_slice_walk_in_device_mode_equals_the_masked_reference_and_needs_a_gpu_batch():
    """The slice walk (MiniBatch / A_Batch slices) with device dropout: explicit masks, the output against the same
    walk in host arithmetic (`X * m[:, None]` between the layers); a CPU-resident batch raises a clear error."""
    from mrgcn_amd._lib import MrgcnError
    from mrgcn_amd.data.batch import MiniBatch
    from mrgcn_amd.models.rgcn import RGCN
    c = util.load_case("minibatch_small")
    g, A_csr = util.load_graph("graph_small")
    N, R = int(g["num_nodes"]), 2 * int(g["num_pred"]) + 1
    batch_idx = np.asarray(c["batch_idx"], dtype=np.int64)
    model = RGCN([(5, 6, "mrgcn", nn.ReLU()), (6, 4, "mrgcn", None)], R, N, 3, P, False, True, False)
    model.load_state_dict({k[len("ft_b3.init."):]: torch.from_numpy(np.array(c[k])) for k in c.files
                           if k.startswith("ft_b3.init.")}, strict=True)
    model = model.cuda()
    mb = MiniBatch(A_csr.astype(np.float32), None, batch_idx, 2, value_mode="norm_f32")
    mb.as_tensors_()
    model.set_node_dropout("device", seed=3)
    Xc = torch.from_numpy(np.asarray(c["ft_b3.X_full"], np.float32)).index_select(0, mb.A.neighbours[-1].long())
    with pytest.raises(MrgcnError, match="needs the batch on a GPU"):
        model(Xc, mb.A)
    mb.to({"relational": torch.device("cuda")})
    Xn = Xc.cuda().requires_grad_(True)
    out = model(Xn, mb.A)
    masks = list(model.last_node_masks)
    assert [int(m.numel()) for m in masks] == [int(mb.A.row[1].shape[0]), int(mb.A.row[0].shape[0])]
    assert model.node_dropout_position == 1
    out.square().sum().backward()
    got = (out.detach(), Xn.grad.clone(), {n: p.grad.clone() for n, p in model.named_parameters()})
    # the same walk with the masks multiplied in by torch (p_dropout = 0: the layers alone)
    model.zero_grad(set_to_none=True)
    Xr = Xc.cuda().requires_grad_(True)
    model.p_dropout = 0.0
    from mrgcn_amd.data.batch import getAdjacencyNodeColumnIdx
    H = Xr
    for li, (key, layer) in enumerate(model.layers.items()):
        i = model.num_layers - (li + 1)
        A_idx = getAdjacencyNodeColumnIdx(mb.A.neighbours[i], N, R).cuda()
        H = layer(H, mb.A.row[i], A_idx) * masks[li][:, None]
        if model.activations[key] is not None:
            H = model.activations[key](H)
    H.square().sum().backward()
    torch.testing.assert_close(got[0], H.detach(), rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(got[1], Xr.grad, rtol=1e-5, atol=1e-7)
    for n, p in model.named_parameters():
        torch.testing.assert_close(got[2][n], p.grad, rtol=1e-5, atol=1e-7, msg=n)
