"""Edge dropout on the device: the draw (csrc/edge_dropout.hip) against its host mirror in all three orders of a value
overlay (plan.hip: mrgcn_plan_create_overlay), the layers that compute on an overlay against the float64 oracle with
the mirrored, dropped adjacency, the model's plumbing, a captured link-prediction step, and the refusals.

One synthetic graph serves every test: N = 560 nodes (a column read by more than 512 rows needs that many), R = 7
(3 predicates, their inverses, the identity), rows of 3, 20, 100, 300 and 1 300 entries — every row class of the
compact view and a split row — and the column (node 7, relation 1) read by 540 rows, a split column.  Built as a
default plan and as a lean plan."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch
import torch.nn as nn

import mrgcn_amd
from mrgcn_amd import _lib as L
from mrgcn_amd import host
from tests import util

pytestmark = pytest.mark.gpu

N, R = 560, 7
RN = R * N
RATES = [0.4] * (R - 1) + [0.2]
SEED = 0x0123_4567_89AB_CDEF


def _graph_coo():
    rng = np.random.default_rng(2018)
    keys = set()
    for i in range(N):                       # the identity block, relation R - 1
        keys.add(i * RN + (R - 1) * N + i)
    for i in range(20, N):                   # the split column: (node 7, relation 1)
        keys.add(i * RN + 1 * N + 7)
    for i in range(5, N):                    # a few random entries per row, some rows of 10 .. 30
        k = int(rng.integers(9, 30)) if i % 9 == 0 else int(rng.integers(1, 6))
        for c in rng.choice((R - 1) * N, k, replace=False):
            keys.add(i * RN + int(c))
    for row, want in ((0, 3), (1, 20), (2, 100), (3, 300), (4, 1300)):
        have = sum(1 for k in keys if k // RN == row)
        for c in rng.choice((R - 1) * N, want - have, replace=False):
            keys.add(row * RN + int(c))
    key = np.array(sorted(keys), dtype=np.int64)
    rows, cols = key // RN, key % RN
    vals = rng.uniform(0.1, 1.0, len(key)).astype(np.float32)
    return rows, cols, vals


_CACHE = {}


def graph():
    """The shared graph and both plans, made once."""
    if not _CACHE:
        from mrgcn_amd.plan import GraphPlan
        rows, cols, vals = _graph_coo()
        A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([rows, cols])), torch.from_numpy(vals), (N, RN)).cuda()
        _CACHE.update(rows=rows, cols=cols, vals=vals, A=A, plan=GraphPlan(A, N, R),
                      lean=GraphPlan(A, N, R, lean=True))
        A._mrgcn_plan = _CACHE["plan"]
        lens = np.bincount(rows, minlength=N)
        assert [int(lens[i]) for i in range(5)] == [3, 20, 100, 300, 1300]
        assert int(((cols == N + 7)).sum()) > 512 and (lens <= 8).any() and ((lens > 8) & (lens <= 32)).any()
    return _CACHE


def _state(seed, position):
    from mrgcn_amd import functional as Fn
    return Fn.node_dropout_state(seed, position, torch.device("cuda", torch.cuda.current_device()))


def _rates(rates=RATES):
    return torch.tensor(rates, dtype=torch.float32).cuda()


def view_coords(plan):
    """(row, literal column) of every entry in the three stored orders, from the plan's own index arrays."""
    ex = plan.export
    rowptr, ptr3, cptr = ex(L.ARR_ROWPTR).astype(np.int64), ex(L.ARR_PTR3).astype(np.int64), ex(L.ARR_CPTR).astype(np.int64)
    ulcol = ex(L.ARR_ULCOL).astype(np.int64)
    csr = (np.repeat(np.arange(plan.num_rows), np.diff(rowptr)), ex(L.ARR_LCOL).astype(np.int64))
    col_of_pos = np.empty(plan.ncols, dtype=np.int64)
    col_of_pos[ex(L.ARR_MPOS).astype(np.int64)] = np.arange(plan.ncols)
    compact = (np.repeat(ex(L.ARR_ROWMAP).astype(np.int64), np.diff(ptr3)), ulcol[col_of_pos[ex(L.ARR_MCOL).astype(np.int64)]])
    csc = (ex(L.ARR_CROW).astype(np.int64), np.repeat(ulcol, np.diff(cptr)))
    return {L.ARR_VAL: csr, L.ARR_MVAL: compact, L.ARR_CVAL: csc}


def mirror(coords, stored, rates, seed, position, layer, rescale=True):
    rows, lcol = coords
    return host.edge_dropout_values(rows, lcol % N, lcol // N, stored, rates, seed, position, layer, rescale)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dropped_csr(plan_parent, seed, position, layer, rates=RATES, dtype=np.float64):
    """The adjacency an overlay holds after the draw, from the mirror: scipy CSR in float64."""
    rows, lcol = view_coords(plan_parent)[L.ARR_VAL]
    v = mirror((rows, lcol), plan_parent.export(L.ARR_VAL), rates, seed, position, layer)
    return sp.csr_matrix((v.astype(dtype), (rows, lcol)), shape=(N, RN))


# ---- 1. the draw against the mirror ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plan", "lean"])
def test_draw_equals_the_mirror_in_all_three_orders(kind):
    g = graph()
    parent = g[kind]
    coords = view_coords(parent)
    before = {a: parent.export(a) for a in coords}
    for a in coords:   # the plan's own three orders hold the same matrix
        r, c = coords[a]
        M = sp.csr_matrix((before[a].astype(np.float64), (r, c)), shape=(N, RN))
        A0 = sp.csr_matrix((g["vals"].astype(np.float64), (g["rows"], g["cols"])), shape=(N, RN))
        assert abs(M - A0).max() == 0
    child = parent.overlay()
    assert child.is_overlay and child.parent is parent and child.nnz == parent.nnz and child.lean == parent.lean
    for a in coords:   # a fresh overlay holds the parent's values, in memory of its own
        assert np.array_equal(bits(child.export(a)), bits(before[a]))
        assert child.array_ptr(a)[0] != parent.array_ptr(a)[0] and child.array_ptr(a)[1] == parent.nnz
    for a in (L.ARR_ROWPTR, L.ARR_LCOL, L.ARR_CPTR, L.ARR_CROW, L.ARR_MCOL, L.ARR_ROWMAP, L.ARR_ULCOL):   # borrowed
        assert child.array_ptr(a) == parent.array_ptr(a)
    if kind == "lean":
        assert child.array_ptr(L.ARR_MVAL)[0] == child.array_ptr(L.ARR_VAL)[0]
    rates = _rates()
    for rescale in (True, False):
        for layer, position in ((0, 5), (3, 5), (0, (9 << 32) | 6)):
            child.draw(rates, _state(SEED, position), layer, rescale=rescale, advance=False)
            got = {a: child.export(a) for a in coords}
            for a in coords:
                want = mirror(coords[a], before[a], RATES, SEED, position, layer, rescale)
                assert np.array_equal(bits(got[a]), bits(want)), (kind, a, layer, position, rescale)
            # the three views agree entry by entry
            order = {a: np.argsort(coords[a][0] * RN + coords[a][1], kind="stable") for a in coords}
            ref = bits(got[L.ARR_VAL][order[L.ARR_VAL]])
            assert np.array_equal(bits(got[L.ARR_MVAL][order[L.ARR_MVAL]]), ref)
            assert np.array_equal(bits(got[L.ARR_CVAL][order[L.ARR_CVAL]]), ref)
            share = float((got[L.ARR_VAL] == 0).mean())
            assert 0.3 < share < 0.45
    for a in coords:   # the parent was never written
        assert np.array_equal(bits(parent.export(a)), bits(before[a]))
    # `advance` moves the position by one, behind the draw
    st = _state(SEED, 41)
    child.draw(rates, st, 0, advance=True)
    assert st.cpu().tolist()[1] == 42
    assert np.array_equal(bits(child.export(L.ARR_VAL)),
                          bits(mirror(coords[L.ARR_VAL], before[L.ARR_VAL], RATES, SEED, 41, 0)))
    # a zero rate for the identity block leaves exactly its entries as they are
    child.draw(_rates([0.4] * (R - 1) + [0.0]), _state(SEED, 1), 0)
    v = child.export(L.ARR_VAL)
    ident = coords[L.ARR_VAL][1] // N == R - 1
    assert np.array_equal(bits(v[ident]), bits(before[L.ARR_VAL][ident])) and (v[~ident] == 0).any()
    child.close()


def test_draw_refuses_what_the_key_cannot_hold():
    parent = graph()["plan"]
    child = parent.overlay()
    with pytest.raises(L.MrgcnError, match="layer"):
        child.draw(_rates(), _state(1, 0), 256)
    with pytest.raises(L.MrgcnError):
        child.draw(_rates()[:3], _state(1, 0), 0)
    lib = L.load()
    assert lib.mrgcn_edge_dropout_draw_f32(parent.handle, _rates().data_ptr(), 1, _state(1, 0).data_ptr(), 0, 0, None) != 0
    with pytest.raises(L.MrgcnError):
        child.overlay()
    child.close()


# ---- 2. p = 0 on an overlay ------------------------------------------------------------------------------------------
def _wide_layer(F=20, B=2, seed=3):
    from mrgcn_amd.layers.graph import GraphConvolution
    torch.manual_seed(seed)
    return GraphConvolution(0, F, R, N, num_bases=B, bias=True, input_layer=True, featureless=True).cuda()


def _wide_run(layer, plan, w):
    layer.zero_grad(set_to_none=True)
    Y = layer._forward_fused(None, plan, relu=True)
    (Y * w).sum().backward()
    return Y.detach().clone(), {k: p.grad.clone() for k, p in layer.named_parameters()}


def test_rate_zero_overlay_equals_the_parent_bit_for_bit():
    from mrgcn_amd import functional as Fn
    g = graph()
    parent = g["plan"]
    child = parent.overlay()
    child.draw(_rates([0.0] * R), _state(SEED, 3), 0)
    layer = _wide_layer()
    with torch.no_grad():
        layer.b.uniform_(-0.1, 0.1)
    w = torch.randn(N, 20, device="cuda")
    assert Fn._WIDE_DET
    mrgcn_amd.reset_stats()
    Y0, g0 = _wide_run(layer, parent, w)
    Y1, g1 = _wide_run(layer, child, w)
    assert mrgcn_amd.stats().get("backward.wide_input") == 2
    assert torch.equal(Y0, Y1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    child.close()


# ---- 3. the wide featureless layer against the float64 oracle --------------------------------------------------------
def test_wide_featureless_layer_on_a_drawn_overlay_vs_oracle():
    from oracle import rgcn_oracle as O
    g = graph()
    parent = g["plan"]
    child = parent.overlay()
    position, lyr = 11, 0
    child.draw(_rates(), _state(SEED, position), lyr)
    A = dropped_csr(parent, SEED, position, lyr)
    F, B = 20, 2
    layer = _wide_layer(F, B)
    with torch.no_grad():
        layer.b.uniform_(-0.1, 0.1)
    w = torch.randn(N, F, device="cuda")
    mrgcn_amd.reset_stats()
    Y, grads = _wide_run(layer, child, w)
    assert mrgcn_amd.stats().get("backward.wide_input") == 1 and not mrgcn_amd.stats().get("backward.support")
    cfg = O.LayerCfg(0, F, R, N, B, bias=True, input_layer=True, featureless=True)
    p = {k: v.detach().cpu().numpy() for k, v in layer.state_dict().items()}
    pre, cache = O.layer_forward(cfg, p, None, A)
    np.testing.assert_allclose(Y.cpu().numpy(), np.maximum(pre, 0), rtol=1e-4, atol=1e-4)
    want, _ = O.layer_backward(cfg, p, None, A, w.cpu().numpy().astype(np.float64) * (pre > 0), cache)
    assert set(want) == {"weight_I", "weight_I_comp", "b"}
    for k, v in want.items():
        got = util.ref_layout(grads[k], k).cpu().numpy()
        np.testing.assert_allclose(got, v, rtol=2e-4, atol=2e-5 * (np.abs(v).max() + 1e-12) + 1e-6, err_msg=k)
    # the parent's matrix gives something else (the comparison above means something)
    pre0, _ = O.layer_forward(cfg, p, None, sp.csr_matrix((g["vals"].astype(np.float64), (g["rows"], g["cols"])), shape=(N, RN)))
    assert np.abs(pre0 - pre).max() > 1e-2
    Y2, grads2 = _wide_run(layer, child, w)   # two runs: the same bits
    assert torch.equal(Y, Y2) and all(torch.equal(grads[k], grads2[k]) for k in grads)
    child.close()


# ---- 4. a block-diagonal hidden layer and a narrow two-layer RGCN under a plain CrossEntropyLoss ----------------------
def _labels(C, n=30, seed=5):
    rng = np.random.default_rng(seed)
    idx = np.sort(rng.choice(N, n, replace=False))
    return torch.from_numpy(idx).cuda(), torch.from_numpy(rng.integers(0, C, n)).cuda()


def test_block_diagonal_layer_on_a_drawn_overlay_vs_float64():
    from mrgcn_amd.layers.graph import GraphConvolution, block_weight_dense
    from tests.test_cpu_block_layer import check_rule
    g = graph()
    parent = g["plan"]
    child = parent.overlay()
    position, lyr = 4, 1
    child.draw(_rates(), _state(SEED, position), lyr)
    dense = dropped_csr(parent, SEED, position, lyr).toarray()
    K, F, NB = 8, 8, 2
    torch.manual_seed(8)
    layer = GraphConvolution(K, F, R, N, num_bases=-1, bias=True, input_layer=False, num_blocks=NB)
    with torch.no_grad():
        layer.b.uniform_(-0.5, 0.5)
    X = np.random.default_rng(8).standard_normal((N, K)).astype(np.float32)
    idx, y = _labels(F)

    def restate(dtype):
        leaves = {k: torch.tensor(v, dtype=dtype, requires_grad=True)
                  for k, v in dict(X=X, W=layer.weight_F.detach().numpy(), b=layer.b.detach().numpy()).items()}
        FW = torch.matmul(leaves["X"].unsqueeze(0), block_weight_dense(leaves["W"])).reshape(R * N, F)
        Yr = torch.tensor(dense, dtype=dtype) @ FW + leaves["b"]
        nn.CrossEntropyLoss()(Yr[idx.cpu()], y.cpu()).backward()
        return Yr.detach().numpy(), {k: v.grad.numpy() for k, v in leaves.items()}

    Y64, g64 = restate(torch.float64)
    Y32, g32 = restate(torch.float32)
    layer = layer.cuda()
    Xd = torch.from_numpy(X).cuda().requires_grad_(True)
    mrgcn_amd.reset_stats()
    Y = layer._forward_fused(Xd, child)
    nn.CrossEntropyLoss()(Y[idx], y).backward()
    st = mrgcn_amd.stats()
    assert st.get("layer.block") == 1 and not st.get("layer.block.fallback") and not st.get("backward.support")
    check_rule("block Y", Y.detach().cpu().numpy(), Y32, Y64)
    check_rule("block dX", Xd.grad.cpu().numpy(), g32["X"], g64["X"])
    check_rule("block dweight_F", layer.weight_F.grad.cpu().numpy(), g32["W"], g64["W"])
    check_rule("block db", layer.b.grad.cpu().numpy(), g32["b"], g64["b"])
    child.close()


def _narrow_model(p_dropout=0.0, lp=False):
    from mrgcn_amd.models.rgcn import RGCN
    torch.manual_seed(12)
    return RGCN([(0, 16, "mrgcn", nn.ReLU()), (16, 4, "mrgcn", None)], R, N, 2, p_dropout, True, True, lp).cuda()


def test_narrow_two_layer_rgcn_under_cross_entropy_vs_oracle():
    from oracle import rgcn_oracle as O
    g = graph()
    model = _narrow_model()
    model.set_edge_dropout(0.4, self_loop=0.2, seed=SEED)
    model.edge_dropout_position = 7
    idx, y = _labels(4)
    mrgcn_amd.reset_stats()
    for _ in range(2):   # (a second step: the looked-up row set of a plain gradient would have a support by now)
        pos = model.edge_dropout_position
        model.zero_grad(set_to_none=True)
        logits = model(None, g["A"])
        nn.CrossEntropyLoss()(logits[idx], y).backward()
    st = mrgcn_amd.stats()
    assert not st.get("backward.support") and st.get("edge_dropout.device") == 4 and st.get("backward.general", 0) >= 2
    assert len(model.last_edge_plans) == 2 and all(o.parent is g["plan"] for o in model.last_edge_plans)
    A0, A1 = (dropped_csr(g["plan"], SEED, pos, l) for l in (0, 1))
    cfgs = O.rgcn_cfgs([(0, 16), (16, 4)], R, N, 2, True, True)
    params = O.split_params({k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}, 2)
    pre0, c0 = O.layer_forward(cfgs[0], params[0], None, A0)
    H = np.maximum(pre0, 0)
    pre1, c1 = O.layer_forward(cfgs[1], params[1], H, A1)
    np.testing.assert_allclose(logits.detach().cpu().numpy(), pre1, rtol=1e-4, atol=1e-4)
    _, dlogits = O.cross_entropy(pre1, idx.cpu().numpy(), y.cpu().numpy())
    g1, dH = O.layer_backward(cfgs[1], params[1], H, A1, dlogits, c1)
    g0, _ = O.layer_backward(cfgs[0], params[0], None, A0, dH * (pre0 > 0), c0)
    for li, grads in ((0, g0), (1, g1)):
        for k, v in grads.items():
            got = util.ref_layout(getattr(model.layers[f"layer_{li}"], k).grad, k).cpu().numpy()
            np.testing.assert_allclose(got, v, rtol=2e-4, atol=2e-5 * (np.abs(v).max() + 1e-12) + 1e-6,
                                       err_msg=f"layer {li} {k}")


# ---- 5. the model -----------------------------------------------------------------------------------------------------
def test_model_draws_edges_and_nodes_from_their_own_states():
    g = graph()
    plan = g["plan"]
    coords = view_coords(plan)
    stored = plan.export(L.ARR_VAL)
    model = _narrow_model(p_dropout=0.2)
    model.set_node_dropout("device", seed=31)
    model.set_edge_dropout(0.4, self_loop=0.2, seed=SEED)
    twin = _narrow_model(p_dropout=0.2)
    twin.set_node_dropout("device", seed=31)
    twin.load_state_dict(model.state_dict())
    assert model.edge_dropout_position == 0
    for step in range(3):
        assert model.edge_dropout_position == step and model.node_dropout_position == step
        model(None, g["A"])
        for l, o in enumerate(model.last_edge_plans):
            want = mirror(coords[L.ARR_VAL], stored, RATES, SEED, step, l)
            assert np.array_equal(bits(o.export(L.ARR_VAL)), bits(want)), (step, l)
            want_m = host.node_dropout_mask(N, 0.2, 31, step, l)
            assert np.array_equal(bits(model.last_node_masks[l].cpu().numpy()), bits(want_m))
    assert model.edge_dropout_position == 3
    overlays = list(model.last_edge_plans)
    model(None, g["A"])
    assert all(a is b for a, b in zip(overlays, model.last_edge_plans))   # made once per (model, plan), reused
    # eval(): the parent plan, nothing drawn, the bits of a model without edge dropout
    model.eval(); twin.eval()
    model.node_dropout_position = 9; twin.node_dropout_position = 9
    mrgcn_amd.reset_stats()
    with torch.no_grad():
        Ye, Yt = model(None, g["A"]), twin(None, g["A"])
    assert torch.equal(Ye, Yt) and model.edge_dropout_position == 4 and not mrgcn_amd.stats().get("edge_dropout.device")
    # all rates zero: nothing changes — no overlay, no draw, the twin's bits in train() mode too
    model.train(); twin.train()
    model.set_edge_dropout(0.0)
    model.node_dropout_position = 9; twin.node_dropout_position = 9
    Y0, Y1 = model(None, g["A"]), twin(None, g["A"])
    assert torch.equal(Y0, Y1) and model.edge_dropout_position == 4 and not mrgcn_amd.stats().get("edge_dropout.device")


# ---- 6. capture -------------------------------------------------------------------------------------------------------
def _lp_run(graphed, steps=4, reseed_at=None):
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.tasks import link_prediction as lp
    from mrgcn_amd.train import ClipAdam, GraphedStep
    g = graph()
    rng = np.random.default_rng(6)
    facts = np.stack([rng.integers(0, N, 400), rng.integers(0, R - 1, 400), rng.integers(0, N, 400)], 1).astype(np.int64)
    torch.manual_seed(0)
    model = RGCN([(0, 20, "mrgcn", nn.ReLU())], R, N, 2, 0.0, True, False, True).cuda()
    model.set_edge_dropout(0.4, self_loop=0.2, seed=SEED)
    opt = ClipAdam(model.parameters(), lr=0.01, weight_decay=0.0, max_norm=1.0, capturable=True)
    sampler = lp.DeviceNegativeSampler(torch.from_numpy(facts).cuda())
    static = lp.SortedTriples(sampler.facts, N, R)
    kept = {}

    def forward():
        kept["emb"] = model(None, g["A"])
        return kept["emb"]

    def step():
        return lp.train_step(model, forward, sampler, opt, static)

    if graphed:   # (the warm-up call is step 0, eager; the capture executes nothing)
        run, out = GraphedStep(step, warmup=1), []
    else:
        run, out = step, [(step().clone(), kept["emb"].detach().clone(), 0, SEED)]
    for k in range(1, steps):
        seed = SEED
        if reseed_at is not None and k >= reseed_at:
            seed = SEED + 1
            model.edge_dropout_seed = seed
        loss = run().clone()
        torch.cuda.synchronize()
        out.append((loss, kept["emb"].detach().clone(), k, seed))
        assert model.edge_dropout_position == k + 1
        want = mirror(view_coords(g["plan"])[L.ARR_VAL], g["plan"].export(L.ARR_VAL), RATES, seed, k, 0)
        assert np.array_equal(bits(model.last_edge_plans[0].export(L.ARR_VAL)), bits(want)), (graphed, k)
    return out


def test_captured_lp_step_draws_fresh_edges_at_every_replay_and_equals_eager():
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        eager = _lp_run(False, reseed_at=3)
        replayed = _lp_run(True, reseed_at=3)
    finally:
        torch.use_deterministic_algorithms(prev)
    assert len(eager) == 4 and len(replayed) == 3
    for (l0, e0, k0, _), (l1, e1, k1, _) in zip(eager[1:], replayed):
        assert k0 == k1 and torch.equal(l0, l1) and torch.equal(e0, e1), k0
    assert not torch.equal(eager[1][1], eager[2][1])


# ---- 7. refusals --------------------------------------------------------------------------------------------------------
def test_what_copies_values_out_of_a_plan_refuses_an_overlay():
    from mrgcn_amd.data.batch import A_BatchMasked
    from mrgcn_amd.plan import GraphSupport
    from mrgcn_amd.train import ClipAdam, categorical_crossentropy, train_step
    g = graph()
    parent = g["plan"]
    Y_before = parent.spmm(L.VIEW_COMPACT, torch.full((parent.nop, 8), 0.5, device="cuda"), F=8)
    T_before = parent.spmm(L.VIEW_TRANSPOSED, torch.ones(N, 8, device="cuda"), F=8)
    child = parent.overlay()
    flags = torch.zeros(N, dtype=torch.uint8, device="cuda")
    flags[:30] = 1
    with pytest.raises(L.MrgcnError, match="edge-dropout"):
        child.support_for(flags)
    with pytest.raises(L.MrgcnError, match="edge-dropout"):
        GraphSupport(child, flags)
    with pytest.raises(L.MrgcnError):
        GraphSupport.chain(child, flags, 2)
    import ctypes as C
    sup = C.c_void_p()
    assert L.load().mrgcn_support_create(C.byref(sup), child.handle, flags.data_ptr(), None) != 0
    # a gradient with unwritten rows on an overlay
    from mrgcn_amd.layers.graph import GraphConvolution
    torch.manual_seed(1)
    layer = GraphConvolution(0, 8, R, N, num_bases=2, bias=False, input_layer=True, featureless=True).cuda()
    child.draw(_rates(), _state(1, 0), 0)
    Y = layer._forward_fused(None, child)
    idx, y = _labels(8)
    loss = categorical_crossentropy(Y, idx, y, sole_consumer=True)
    with pytest.raises(L.MrgcnError, match="edge dropout"):
        loss.backward()
    # the steps whose loss hands down such gradients, mini-batches, the literal engine
    model = _narrow_model()
    model.set_edge_dropout(0.4, self_loop=0.2)
    opt = ClipAdam(model.parameters(), lr=0.01, max_norm=1.0)
    with pytest.raises(L.MrgcnError, match="edge dropout: train.train_step"):
        train_step(model, lambda: model(None, g["A"]), idx, y, opt)
    with pytest.raises(L.MrgcnError, match="edge dropout: masked and slice mini-batches"):
        model(None, A_BatchMasked.__new__(A_BatchMasked))
    model.set_engine("literal")
    with pytest.raises(L.MrgcnError, match="edge dropout runs on the fused engine"):
        model(None, g["A"])
    model.set_engine("fused")
    model.eval()
    model(None, g["A"])   # (eval(): the plan itself)
    # a closed overlay leaves the parent usable
    child.close()
    child.close()
    with pytest.raises(L.MrgcnError):
        child.handle
    # closing a plan closes its overlays first (they borrow its arrays)
    from mrgcn_amd.plan import GraphPlan
    p2 = GraphPlan(g["A"], N, R, lean=True)
    o2 = p2.overlay()
    p2.close()
    with pytest.raises(L.MrgcnError):
        o2.handle
    Y_after = parent.spmm(L.VIEW_COMPACT, torch.full((parent.nop, 8), 0.5, device="cuda"), F=8)
    T_after = parent.spmm(L.VIEW_TRANSPOSED, torch.ones(N, 8, device="cuda"), F=8)
    assert torch.equal(Y_before, Y_after) and torch.equal(T_before, T_after)
