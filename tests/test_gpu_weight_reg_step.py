"""Weight decay and L1 / L2 penalties on the row-sparse node-table step (ClipAdam.step, train_step, the drop-ins of
mrgcn_amd.optim): whole epochs against the literal ATen port of the reference's epoch with the three settings
(node_classification.py:35-37, :172-193), the default route against `row_sparse=False`, hipGraph replay, a
`weight_decay` that changes between steps, and the routes that keep the dense step."""
import functools

import numpy as np
import pytest
import torch

from tests import util
from tests.test_gpu_support import _cases

pytestmark = pytest.mark.gpu

MODELS = {
    "ft3": ([(5, 8), (8, 4)], 3, False),
    "ft40": ([(6, 10), (10, 4)], 40, False),
    "fl4": ([(0, 8), (8, 4)], 4, True),
}
SETTINGS = {
    "wd": (5e-4, 0.0, 0.0),
    "l1l2": (0.0, 1e-4, 1e-3),
    "all": (5e-4, 1e-4, 1e-3),
}
EPOCHS = 3


PARAM_SEED = 13   # of the initial parameters (oracle.aten_literal.make_params); see test_epochs_against_the_reference_epoch


@functools.lru_cache(maxsize=None)
def _oracle(model, setting, seed=PARAM_SEED):
    """the host side, once per (model, setting): the graph, the initial parameters and the reference's epochs"""
    from mrgcn_amd import synth
    from oracle import aten_literal as AL
    dims, B, featureless = MODELS[model]
    wd, l1, l2 = SETTINGS[setting]
    g = synth.make_graph("aifb", seed=5, scale=0.5, value_mode="norm_f32")
    N, R = g.num_nodes, g.num_relations
    rng = np.random.default_rng(5)
    X = None if featureless else rng.standard_normal((N, dims[0][0])).astype(np.float32)
    idx = np.sort(rng.choice(N, 100, replace=False)).astype(np.int64)
    y = rng.integers(0, dims[-1][1], 100).astype(np.int64)
    p = AL.make_params(dims, R, N, B, False, featureless, seed=seed)
    init = {k: v.detach().clone() for k, v in p.items()}
    A_cpu = AL.coo_tensor(g.rows, g.cols, g.vals, (N, R * N))
    ep = AL.Epoch(p, len(dims), R, N, B, featureless, weight_decay=wd, l1_lambda=l1, l2_lambda=l2)
    Xc = None if X is None else torch.from_numpy(X)
    ref = [ep.step(Xc, A_cpu, torch.from_numpy(idx), torch.from_numpy(y)) for _ in range(EPOCHS)]
    ref = [(r[0].detach().numpy().copy(), float(r[1].detach())) for r in ref]
    return dict(g=g, N=N, R=R, X=X, idx=idx, y=y, init=init, ref=ref)


def _epochs(model_name, setting, row_sparse, seed=PARAM_SEED):
    """EPOCHS epochs on the GPU -> (per epoch: logits before it and the loss, next to the reference's), stats, model"""
    import mrgcn_amd
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.train import ClipAdam, train_step
    dims, B, featureless = MODELS[model_name]
    wd, l1, l2 = SETTINGS[setting]
    o = _oracle(model_name, setting, seed)
    g, N, R = o["g"], o["N"], o["R"]
    modules = [(i, oo, "mrgcn", torch.nn.ReLU() if li < len(dims) - 1 else None) for li, (i, oo) in enumerate(dims)]
    model = RGCN(modules, R, N, B, 0.0, featureless, False, False)
    model.load_state_dict(dict(o["init"]))
    model = model.cuda()
    A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([g.rows, g.cols])), torch.from_numpy(g.vals),
                                (N, R * N)).cuda()
    Xg = None if o["X"] is None else torch.from_numpy(o["X"]).cuda()
    opt = ClipAdam(model.parameters(), lr=0.01, max_norm=1.0, weight_decay=wd)
    ig, yg = torch.from_numpy(o["idx"]).cuda(), torch.from_numpy(o["y"]).cuda()
    mrgcn_amd.reset_stats()
    out = []
    for e in range(EPOCHS):
        logits = model(Xg, A).detach().cpu().numpy()
        loss = train_step(model, lambda: model(Xg, A), ig, yg, opt, l1_lambda=l1, l2_lambda=l2, row_sparse=row_sparse)
        out.append((logits, o["ref"][e][0], float(loss), o["ref"][e][1]))
    return out, mrgcn_amd.stats(), model


@pytest.mark.parametrize("row_sparse", [None, False])
@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("model_name", list(MODELS))
def test_epochs_against_the_reference_epoch(model_name, setting, row_sparse):
    """`row_sparse=False` is the route this project had before the regularised row update: it must meet the tolerances
    too, else the inputs are at fault (Adam's first steps are sign-like, so an element whose gradient two summation
    orders put on either side of zero moves by 2 lr).  Seed 11 of the initial parameters is such an input: both routes
    miss the logits of `ft40` under `wd` by the same 1.36 x the tolerance; seeds 12, 13, 14 stay within 0.20, 0.16 and
    0.25 of it over all nine cases on both routes.  PARAM_SEED is 13."""
    out, st, model = _epochs(model_name, setting, row_sparse)
    for e, (logits, ref_logits, loss, ref_loss) in enumerate(out):
        np.testing.assert_allclose(logits, ref_logits, rtol=1e-4, atol=1e-4, err_msg=f"logits before epoch {e}")
        np.testing.assert_allclose(loss, ref_loss, rtol=2e-4, atol=2e-5)
    if row_sparse is None:
        assert st.get("adam.reg") == EPOCHS, st
        assert st.get("weight_I.fused_rows") == EPOCHS and "weight_I.dense" not in st, st
        assert model.layers["layer_0"].weight_I.grad is None
    else:
        assert "adam.reg" not in st, st


def _golden_runs(case_name, row_sparse, steps=4, wd=1e-2, l2=1e-3):
    from mrgcn_amd.train import ClipAdam, train_step
    from tests.test_gpu_layers import _adjacency
    c = util.load_case(case_name)
    model, dims = util.build_rgcn_from_case(c, "cuda")
    util.load_state_from_case(model, c)
    model = model.cuda()
    At = _adjacency(c, case_name)
    X = None if bool(c["meta.featureless"]) else torch.from_numpy(c["X"]).cuda()
    idx = torch.from_numpy(c["labels_idx"]).cuda()
    tgt = torch.from_numpy(c["labels_y"]).cuda()
    opt = ClipAdam(model.parameters(), lr=0.01, max_norm=1.0, weight_decay=wd)
    losses = [float(train_step(model, lambda: model(X, At), idx, tgt, opt, l2_lambda=l2, row_sparse=row_sparse))
              for _ in range(steps)]
    return losses, {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}


@pytest.mark.parametrize("case_name", _cases())
def test_default_route_equals_the_dense_step_on_the_golden_cases(case_name):
    l1, p1 = _golden_runs(case_name, None)
    l0, p0 = _golden_runs(case_name, False)
    np.testing.assert_allclose(l1, l0, rtol=1e-5, atol=1e-6)
    for k in p0:
        diff = np.abs(p1[k] - p0[k])
        share = float((diff > 2e-5).mean())
        print(f"{case_name} {k}: share of elements off by more than 2e-5: {share:.3g} (largest {float(diff.max()):.3g})")
        assert share <= 2e-3, (k, float(diff.max()))


def _small_problem(hidden=8, B=5, seed=3):
    """the graph of tests/test_gpu_reference_loop.py (most of the node table never gets gradient) under a model whose
    node table has `B` x `hidden` blocks"""
    from mrgcn_amd.models.rgcn import RGCN
    from tests.test_gpu_reference_loop import _problem
    A, X, idx, tgt, N, R = _problem(N=3000, seed=seed)

    def make():
        torch.manual_seed(0)
        return RGCN([(6, hidden, "mrgcn", torch.nn.ReLU()), (hidden, 4, "mrgcn", None)], R, N, B, 0.0, False, True,
                    False).cuda()
    return A, X, idx, tgt, make


def test_captured_epoch_replays_the_regularised_step():
    """three eager steps against one warm-up step and two replays of GraphedTrainStep (the lambdas and weight_decay
    are launch arguments, baked in at capture like lr)"""
    import mrgcn_amd
    from mrgcn_amd.train import ClipAdam, GraphedTrainStep, train_step
    A, X, idx, tgt, make = _small_problem()
    kw = dict(l1_lambda=1e-4, l2_lambda=1e-3)
    states, losses = [], []
    for graphed in (False, True):
        model = make()
        opt = ClipAdam(list(model.parameters()), lr=0.01, max_norm=1.0, weight_decay=5e-4, capturable=graphed)
        mrgcn_amd.reset_stats()
        if graphed:
            step = GraphedTrainStep(model, lambda: model(X, A), idx, tgt, opt, warmup=1, **kw)
            for _ in range(2):
                loss = step()
        else:
            for _ in range(3):
                loss = train_step(model, lambda: model(X, A), idx, tgt, opt, **kw)
        torch.cuda.synchronize()
        assert mrgcn_amd.stats().get("adam.reg", 0) >= 2 and model.layers["layer_0"].weight_I.grad is None
        states.append({k: v.clone() for k, v in model.state_dict().items()})
        losses.append(float(loss))
    assert abs(losses[0] - losses[1]) <= 1e-5 * max(1.0, abs(losses[0]))
    for k in states[0]:
        torch.testing.assert_close(states[0][k], states[1][k], rtol=1e-5, atol=1e-6, msg=k)


def test_a_weight_decay_that_changes_between_steps():
    """wd = 0, 0, 0.01, 0: the plain list update, then the regularised one, then the list update again — now with the
    pass over the nodes outside the support, because every node holds moments (stale `ever` flags would show here)"""
    import mrgcn_amd
    from mrgcn_amd.train import ClipAdam, train_step
    A, X, idx, tgt, make = _small_problem()
    res = {}
    for row_sparse in (None, False):
        model = make()
        opt = ClipAdam(list(model.parameters()), lr=0.01, max_norm=1.0)
        order, losses = [], []
        for wd in (0.0, 0.0, 0.01, 0.0):
            opt.param_groups[0]["weight_decay"] = wd
            mrgcn_amd.reset_stats()
            losses.append(float(train_step(model, lambda: model(X, A), idx, tgt, opt, row_sparse=row_sparse)))
            st = mrgcn_amd.stats()
            order.append([k for k in ("adam.list", "adam.reg") if k in st])
        res[row_sparse] = (losses, {k: v.clone() for k, v in model.state_dict().items()}, order)
    assert res[None][2] == [["adam.list"], ["adam.list"], ["adam.reg"], ["adam.list"]], res[None][2]
    assert res[False][2] == [[], [], [], []]
    np.testing.assert_allclose(res[None][0], res[False][0], rtol=1e-5, atol=1e-6)
    for k, v in res[False][1].items():
        torch.testing.assert_close(res[None][1][k], v, rtol=1e-5, atol=1e-6, msg=k)


def test_zero_settings_keep_the_list_update():
    import mrgcn_amd
    from mrgcn_amd.train import ClipAdam, train_step
    A, X, idx, tgt, make = _small_problem()
    model = make()
    opt = ClipAdam(list(model.parameters()), lr=0.01, max_norm=1.0, weight_decay=0.0)
    mrgcn_amd.reset_stats()
    for _ in range(2):
        train_step(model, lambda: model(X, A), idx, tgt, opt, l1_lambda=0.0, l2_lambda=0.0)
    st = mrgcn_amd.stats()
    assert "adam.reg" not in st and st.get("adam.list") == 2, st
    assert opt.reg_loss is None


def test_drop_in_adam_with_weight_decay_stays_row_sparse():
    """the reference's loop (node_classification.py:35-37, :190-193) with `weight_decay` in the config and no penalty
    in the loss: RowSparseAdam + this package's clip_grad_norm_ against torch.optim.Adam + torch's clip"""
    import mrgcn_amd
    from mrgcn_amd import optim as O
    A, X, idx, tgt, make = _small_problem()
    res, logs = [], []
    for Adam, clip in ((torch.optim.Adam, torch.nn.utils.clip_grad_norm_), (O.RowSparseAdam, O.clip_grad_norm_)):
        m = make()
        opt = Adam([{"params": [p for p in m.parameters() if p.requires_grad]}], lr=0.01, weight_decay=0.01)
        crit = torch.nn.CrossEntropyLoss()
        log = []
        mrgcn_amd.reset_stats()
        for _ in range(3):
            loss = crit(m(X, A)[idx], tgt)
            opt.zero_grad()
            loss.backward()
            norm = clip(m.parameters(), 1.0)
            opt.step()
            log.append((float(loss), float(norm)))
        if Adam is O.RowSparseAdam:
            assert m.layers["layer_0"].weight_I.grad is None
            assert mrgcn_amd.stats().get("adam.reg") == 3, mrgcn_amd.stats()
        res.append({k: v.clone() for k, v in m.state_dict().items()})
        logs.append(log)
    np.testing.assert_allclose(np.array(logs[1]), np.array(logs[0]), rtol=1e-5, atol=1e-7)
    for k in res[0]:
        torch.testing.assert_close(res[1][k], res[0][k], rtol=1e-5, atol=1e-7, msg=k)


def test_a_shape_outside_the_kernels_keeps_the_dense_step():
    """a hidden width of 32 with an L2 penalty: known before the backward, which then writes the dense gradient"""
    import mrgcn_amd
    from mrgcn_amd.train import ClipAdam, train_step
    A, X, idx, tgt, make = _small_problem(hidden=32, B=4)
    res = {}
    for row_sparse in (None, False):
        model = make()
        opt = ClipAdam(list(model.parameters()), lr=0.01, max_norm=1.0)
        mrgcn_amd.reset_stats()
        losses = [float(train_step(model, lambda: model(X, A), idx, tgt, opt, l2_lambda=1e-3, row_sparse=row_sparse))
                  for _ in range(3)]
        st = mrgcn_amd.stats()
        assert "adam.reg" not in st and model.layers["layer_0"].weight_I.grad is not None, st
        res[row_sparse] = (losses, {k: v.clone() for k, v in model.state_dict().items()})
    np.testing.assert_allclose(res[None][0], res[False][0], rtol=1e-5, atol=1e-6)
    for k, v in res[False][1].items():
        torch.testing.assert_close(res[None][1][k], v, rtol=1e-5, atol=1e-6, msg=k)
