"""Block-diagonal relation weights on the device (csrc/block_xform.hip; functional._BlockLayer;
`GraphConvolution(num_blocks=...)`, `RGCN(num_blocks=...)`).

Bounds: the rule of tests/test_cpu_block_layer.py (`check_rule`): per case the float32 host restatement against the
float64 one, the kernel gets 4 x that maximum error with a floor of one float32 ulp of the compared value; nothing is
excluded.  Where bit equality is asked it is bit equality (`tobytes`).

Graphs.  G1 (37 nodes, 5 relations) and G2 (700 nodes, 3 relations, one relation with 650 compact columns: three units
of the dW walk's 256 columns inside one group, 2.5 units and more) are the ones the CPU file builds.  A compact column is
a (source node, relation) pair, so no node of G1 can own more than 5: the node with more than 64 columns lives in G1W
(37 nodes, 70 relations), which the kernel tests run at the small shapes beside G1."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn

import mrgcn_amd
from mrgcn_amd import _lib, host
from mrgcn_amd.layers.graph import GraphConvolution, block_weight_dense
from tests.test_cpu_block_layer import (SHAPES, case_inputs, check_rule, compact_columns, graph_g1, graph_g1_wide,
                                        graph_g2)
from tests.test_gpu_lp_fit import deterministic

pytestmark = pytest.mark.gpu

GRAPHS = {"g1": graph_g1, "g1w": graph_g1_wide, "g2": graph_g2}
_PLANS: dict = {}
SENTINEL = 7.25


def _np(t):
    return t.detach().cpu().numpy()


def _graph(name):
    """(N, R, A on the device, its plan, node / rel / mpos of the compact columns, dense A in float64)."""
    if name not in _PLANS:
        from mrgcn_amd.plan import plan_of
        N, R, rows, cols, vals = GRAPHS[name]()
        A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([rows, cols])), torch.from_numpy(vals), (N, R * N)).cuda()
        plan = plan_of(A, N, R)
        node, rel = compact_columns(N, cols)
        assert np.array_equal(plan.export(_lib.ARR_UNODE), node) and np.array_equal(plan.export(_lib.ARR_UREL), rel)
        dense = np.zeros((N, R * N))
        np.add.at(dense, (rows, cols), vals.astype(np.float64))
        _PLANS[name] = dict(N=N, R=R, A=A, plan=plan, node=node, rel=rel, mpos=plan.export(_lib.ARR_MPOS), dense=dense)
    return _PLANS[name]


def test_the_graphs_have_what_the_cases_need():
    g1, g1w, g2 = _graph("g1"), _graph("g1w"), _graph("g2")
    assert g1["N"] == 37 and g1["R"] == 5 and 280 <= g1["plan"].nnz <= 330
    for g in (g1, g1w):
        assert not np.any(g["rel"] == 3) and not np.any(g["node"] == 36)
    assert int((g1w["node"] == 0).sum()) > 64
    N, R, rows, cols, _ = graph_g1()
    assert len(np.unique(rows * (R * N) + cols)) < len(rows)           # duplicate (row, column) entries
    assert g2["N"] == 700 and g2["R"] == 3 and int((g2["rel"] == 1).sum()) >= 640   # >= 2.5 units of 256 columns


def _padded(a, pad):
    """`a` [n, w] on the device as a view with ld = w + pad of a sentinel-filled buffer."""
    big = torch.full((a.shape[0], a.shape[1] + pad), SENTINEL, dtype=torch.float32, device="cuda")
    big[:, :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    return big[:, :a.shape[1]]


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- 2a. forward kernel ------------------------------------------------------------------------------------------------
FWD_CASES = [("g1", s) for s in SHAPES] + [("g1w", s) for s in SHAPES[:5]] + [("g2", SHAPES[0])]


@pytest.mark.parametrize("gname,shape", FWD_CASES, ids=[f"{g}-{s[0]}x{s[1]}b{s[2]}" for g, s in FWD_CASES])
def test_forward_equals_the_mirror_bit_for_bit(gname, shape):
    K, F, NB = shape
    g = _graph(gname)
    lib, plan = _lib.load(), g["plan"]
    X, W, _ = case_inputs(g["N"], g["R"], K, F, NB, seed=K * 1000 + F)
    want = host.block_transform32(X, W, g["node"], g["rel"])
    assert lib.mrgcn_block_transform_supported(plan.handle, K, F, NB) == 1
    Xd = _padded(X, 3)                                   # ldX > K
    Wd = torch.from_numpy(W).cuda()
    guard = 64
    for order in (0, 1):
        rows = plan.nop if order else plan.ncols
        pos = g["mpos"] if order else np.arange(plan.ncols)
        for ld in ((F + 3) // 4 * 4, F + 7):
            buf = torch.full((rows * ld + guard,), SENTINEL, dtype=torch.float32, device="cuda")
            _lib.check(lib.mrgcn_block_transform_fwd_f32(plan.handle, _p(Xd), Xd.stride(0), K, _p(Wd), NB, F, _p(buf), ld,
                                                         order, _st()), "fwd")
            torch.cuda.synchronize()
            out = _np(buf[:rows * ld]).reshape(rows, ld)
            got = out[pos]
            assert got[:, :F].tobytes() == want.tobytes(), (order, ld, float(np.abs(got[:, :F] - want).max()))
            assert got[:, F:].tobytes() == np.zeros((plan.ncols, ld - F), np.float32).tobytes(), "pad columns are +0.0"
            assert bool((buf[rows * ld:] == SENTINEL).all()), "the guard region behind the buffer was written"
            other = np.setdiff1d(np.arange(rows), pos)
            assert np.all(out[other] == SENTINEL), "a row that holds no compact column was written"
    # bad leading dimensions are refused
    buf = torch.empty((plan.nop * (F + 4),), device="cuda")
    assert lib.mrgcn_block_transform_fwd_f32(plan.handle, _p(Xd), K - 1, K, _p(Wd), NB, F, _p(buf), F, 0, _st()) != 0
    assert lib.mrgcn_block_transform_fwd_f32(plan.handle, _p(Xd), Xd.stride(0), K, _p(Wd), NB, F, _p(buf), F - 1, 0,
                                             _st()) != 0


# ---- 2b. backward kernel -----------------------------------------------------------------------------------------------
# (64, 64, 4) and (66, 32, 2): slabs of 1 024 and 1 056 floats, either side of the size up to which dX stages the slab
BWD_CASES = ([("g1", s) for s in SHAPES] + [("g1w", s) for s in SHAPES[:5]]
             + [("g2", (8, 8, 2)), ("g2", (200, 200, 40)), ("g1", (64, 64, 4)), ("g1", (66, 32, 2))])
_BWD_REF: dict = {}


def _bwd_reference(gname, shape):
    """Inputs and the float32 / float64 restatements of one case (computed once, never changed)."""
    key = (gname, shape)
    if key not in _BWD_REF:
        K, F, NB = shape
        g = _graph(gname)
        X, W, rng = case_inputs(g["N"], g["R"], K, F, NB, seed=K * 1000 + F + 1)
        dM = rng.standard_normal((len(g["node"]), F)).astype(np.float32)
        r32 = host.block_transform_bwd32(dM, X, W, g["node"], g["rel"], g["N"])
        r64 = host.block_transform_bwd64(dM, X, W, g["node"], g["rel"], g["N"])
        _BWD_REF[key] = (X, W, dM, r32, r64)
    return _BWD_REF[key]


def _run_bwd(plan, Xd, Wd, dMd, K, F, NB, want_dX, want_dW, ws_short=0):
    lib = _lib.load()
    N = plan.num_nodes
    dX = torch.full((N, K + 2), SENTINEL, device="cuda") if want_dX else None
    dW = torch.full(tuple(Wd.shape), SENTINEL, device="cuda") if want_dW else None
    nws = int(lib.mrgcn_block_transform_bwd_workspace(plan.handle, K, F, NB, int(want_dX), int(want_dW)))
    ws = torch.full((max(nws, 1),), float("nan"), device="cuda")
    rc = lib.mrgcn_block_transform_bwd_f32(plan.handle, _p(dMd), dMd.stride(0), _p(Xd), Xd.stride(0), K, _p(Wd), NB, F,
                                           _p(dX), K + 2, _p(dW), _p(ws), nws - ws_short, _st())
    torch.cuda.synchronize()
    return rc, dX, dW, nws


@pytest.mark.parametrize("gname,shape", BWD_CASES, ids=[f"{g}-{s[0]}x{s[1]}b{s[2]}" for g, s in BWD_CASES])
def test_backward_against_float64(gname, shape):
    K, F, NB = shape
    g = _graph(gname)
    plan = g["plan"]
    X, W, dM, (dX32, dW32), (dX64, dW64) = _bwd_reference(gname, shape)
    Xd, dMd, Wd = _padded(X, 3), _padded(dM, 5), torch.from_numpy(W).cuda()
    rc, dX, dW, nws = _run_bwd(plan, Xd, Wd, dMd, K, F, NB, True, True)
    assert rc == 0, _lib.load().mrgcn_last_error()
    assert bool((dX[:, K:] == SENTINEL).all()), "dX wrote past a row's K columns"
    gx, gw = _np(dX[:, :K]), _np(dW)
    check_rule(f"dX {gname} {shape}", gx, dX32, dX64)
    check_rule(f"dW {gname} {shape}", gw, dW32, dW64)
    # exact zeros: the relation without entries, the nodes without a column
    for r in np.setdiff1d(np.arange(g["R"]), g["rel"]):
        assert gw[r].tobytes() == np.zeros_like(gw[r]).tobytes()
    no_col = np.setdiff1d(np.arange(g["N"]), g["node"])
    assert len(no_col) > 0 and gx[no_col].tobytes() == np.zeros_like(gx[no_col]).tobytes()
    if gname != "g2":
        assert 3 in np.setdiff1d(np.arange(g["R"]), g["rel"]) and 36 in no_col
    # each output alone gives the same bits, and so does a second run
    rc, dX1, none, _ = _run_bwd(plan, Xd, Wd, dMd, K, F, NB, True, False)
    assert rc == 0 and none is None and _np(dX1).tobytes() == _np(dX).tobytes()
    rc, none, dW1, _ = _run_bwd(plan, Xd, Wd, dMd, K, F, NB, False, True)
    assert rc == 0 and none is None and _np(dW1).tobytes() == gw.tobytes()
    rc, dX2, dW2, _ = _run_bwd(plan, Xd, Wd, dMd, K, F, NB, True, True)
    assert rc == 0 and _np(dX2).tobytes() == _np(dX).tobytes() and _np(dW2).tobytes() == gw.tobytes()
    # a workspace one float short is refused, not used
    assert nws > 0
    rc, dX3, dW3, _ = _run_bwd(plan, Xd, Wd, dMd, K, F, NB, False, True, ws_short=1)
    assert rc != 0 and bool((dW3 == SENTINEL).all())


# ---- restatements of a layer in torch (CPU, float32 or float64) --------------------------------------------------------
def _layer_ref(dtype, dense, X, W, b, relu, m, wI=None, comp=None):
    """(Y, Z) of Y = m . relu?(Z), Z = A [W_I + stack_r X W_r] + b with the dense A and the dense form of the blocks."""
    A = torch.tensor(dense, dtype=dtype)
    N, F = X.shape[0], b.shape[0]
    R = A.shape[1] // N
    FW = torch.matmul(X.unsqueeze(0), block_weight_dense(W)).reshape(R * N, F)
    if wI is not None:
        B = comp.shape[1]
        FW = FW + (comp @ wI.view(B, N * F)).view(R * N, F)
    Z = A @ FW + b
    Y = torch.relu(Z) if relu else Z
    if m is not None:
        Y = Y * m[:, None]
    return Y, Z


def _ref_grads(dtype, dense, tensors, G, relu, m):
    """Forward and the gradients of sum(Y * G) for the leaves in `tensors` (a dict of numpy arrays)."""
    leaves = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in tensors.items()}
    Y, Z = _layer_ref(dtype, dense, leaves["X"], leaves["W"], leaves["b"], relu,
                      None if m is None else torch.tensor(m, dtype=dtype), leaves.get("wI"), leaves.get("comp"))
    (Y * torch.tensor(G, dtype=dtype)).sum().backward()
    return Y.detach().numpy(), Z.detach().numpy(), {k: v.grad.numpy() for k, v in leaves.items()}


def _layer_case(K, F, NB, relu, masked, input_layer, seed):
    g = _graph("g1")
    N, R = g["N"], g["R"]
    torch.manual_seed(seed)
    layer = GraphConvolution(K, F, R, N, num_bases=2 if input_layer else -1, bias=True, input_layer=input_layer,
                             num_blocks=NB)
    with torch.no_grad():
        layer.b.uniform_(-0.5, 0.5)
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, K)).astype(np.float32)
    G = rng.standard_normal((N, F)).astype(np.float32)
    m = None
    if masked:
        m = np.where(rng.random(N) < 0.3, np.float32(0), np.float32(1) / np.float32(0.7)).astype(np.float32)
    tensors = dict(X=X, W=_np(layer.weight_F), b=_np(layer.b))
    if input_layer:
        tensors.update(wI=_np(layer.state_dict()["weight_I"]), comp=_np(layer.weight_I_comp))
    return g, layer, X, G, m, tensors


def _check_layer(K, F, NB, relu, masked, input_layer, seed):
    g, layer, X, G, m, tensors = _layer_case(K, F, NB, relu, masked, input_layer, seed)
    Y64, Z64, g64 = _ref_grads(torch.float64, g["dense"], tensors, G, relu, m)
    Y32, _, g32 = _ref_grads(torch.float32, g["dense"], tensors, G, relu, m)
    if relu:
        assert float(np.abs(Z64).min()) > 1e-5, f"a pre-activation within 1e-5 of zero ({np.abs(Z64).min():.3e})"
    layer = layer.cuda()
    Xd = torch.from_numpy(X).cuda().requires_grad_(True)
    md = None if m is None else torch.from_numpy(m).cuda()
    mrgcn_amd.reset_stats()
    Y = layer._forward_fused(Xd, g["plan"], relu=relu, row_scale=md)
    assert mrgcn_amd.stats().get("layer.block", 0) == 1 and mrgcn_amd.stats().get("layer.block.fallback", 0) == 0
    (Y * torch.from_numpy(G).cuda()).sum().backward()
    tag = f"layer {(K, F, NB)} relu={relu} input={input_layer}"
    check_rule(tag + " Y", _np(Y), Y32, Y64)
    check_rule(tag + " dX", _np(Xd.grad), g32["X"], g64["X"])
    check_rule(tag + " dweight_F", _np(layer.weight_F.grad), g32["W"], g64["W"])
    check_rule(tag + " db", _np(layer.b.grad), g32["b"], g64["b"])
    if input_layer:
        Bn = 2
        to_nm = lambda a: a.reshape(Bn, g["N"], F).transpose(1, 0, 2)   # noqa: E731  (reference rows -> node-major)
        check_rule(tag + " dweight_I", _np(layer.weight_I.grad), to_nm(g32["wI"]), to_nm(g64["wI"]))
        check_rule(tag + " dweight_I_comp", _np(layer.weight_I_comp.grad), g32["comp"], g64["comp"])


# ---- 2d. the layer -------------------------------------------------------------------------------------------------------
LAYER_SHAPES = [(8, 8, 2), (10, 6, 2), (200, 200, 40)]
RELU_SEEDS = {(8, 8, 2): 20, (10, 6, 2): 20, (200, 200, 40): 20}   # seeds whose pre-activations stay off zero


@pytest.mark.parametrize("K,F,NB", LAYER_SHAPES)
def test_layer_without_relu(K, F, NB):
    _check_layer(K, F, NB, relu=False, masked=False, input_layer=False, seed=K + F)


@pytest.mark.parametrize("K,F,NB", LAYER_SHAPES)
def test_layer_with_relu_and_a_row_scale(K, F, NB):
    _check_layer(K, F, NB, relu=True, masked=True, input_layer=False, seed=RELU_SEEDS[(K, F, NB)])


def test_input_layer_with_bases_and_blocks_sums_both_terms():
    _check_layer(8, 8, 2, relu=False, masked=False, input_layer=True, seed=31)


def test_layer_results_do_not_depend_on_the_deterministic_flag():
    g, layer, X, G, m, _ = _layer_case(200, 200, 40, True, True, False, 20)
    layer = layer.cuda()
    outs = []
    for flag in (False, True, False):
        prev = torch.are_deterministic_algorithms_enabled()
        torch.use_deterministic_algorithms(flag)
        try:
            layer.zero_grad()
            Xd = torch.from_numpy(X).cuda().requires_grad_(True)
            Y = layer._forward_fused(Xd, g["plan"], relu=True, row_scale=torch.from_numpy(m).cuda())
            (Y * torch.from_numpy(G).cuda()).sum().backward()
            outs.append([_np(t).tobytes() for t in (Y, Xd.grad, layer.weight_F.grad, layer.b.grad)])
        finally:
            torch.use_deterministic_algorithms(prev)
    assert outs[0] == outs[1] == outs[2]


# ---- 2c. the limits and the fallback -----------------------------------------------------------------------------------
def test_supported_answers_the_limits():
    lib, plan = _lib.load(), _graph("g1")["plan"]
    ok = lambda K, F, NB: lib.mrgcn_block_transform_supported(plan.handle, K, F, NB)   # noqa: E731
    assert ok(8, 8, 2) == 1 and ok(256, 256, 4) == 1 and ok(200, 200, 40) == 1 and ok(64, 64, 1) == 1
    assert ok(130, 4, 2) == 0            # ki = 65
    assert ok(4, 130, 2) == 0            # fo = 65
    assert ok(260, 8, 4) == 0            # K = 260
    assert ok(8, 260, 4) == 0            # F = 260
    assert ok(9, 8, 2) == 0 and ok(8, 9, 2) == 0 and ok(8, 8, 0) == 0    # NB does not divide, no blocks


@pytest.mark.parametrize("K,F,NB", [(130, 4, 2), (260, 8, 4)])
def test_outside_the_limits_the_layer_falls_back(K, F, NB):
    g = _graph("g1")
    torch.manual_seed(K)
    layer = GraphConvolution(K, F, g["R"], g["N"], bias=True, num_blocks=NB)
    rng = np.random.default_rng(K)
    X = rng.standard_normal((g["N"], K)).astype(np.float32)
    G = rng.standard_normal((g["N"], F)).astype(np.float32)
    tensors = dict(X=X, W=_np(layer.weight_F), b=_np(layer.b))
    Y64, _, g64 = _ref_grads(torch.float64, g["dense"], tensors, G, False, None)
    Y32, _, g32 = _ref_grads(torch.float32, g["dense"], tensors, G, False, None)
    layer = layer.cuda()
    outs = {}
    for engine in ("fused", "literal"):
        layer.engine = engine
        layer.zero_grad()
        Xd = torch.from_numpy(X).cuda().requires_grad_(True)
        mrgcn_amd.reset_stats()
        Y = layer(Xd, g["A"])
        st = mrgcn_amd.stats()
        assert st.get("layer.block", 0) == 0 and st.get("layer.block.fallback", 0) == (1 if engine == "fused" else 0)
        (Y * torch.from_numpy(G).cuda()).sum().backward()
        outs[engine] = (Y, Xd.grad, layer.weight_F.grad.clone())
        check_rule(f"{engine} Y", _np(Y), Y32, Y64)
        check_rule(f"{engine} dX", _np(Xd.grad), g32["X"], g64["X"])
        check_rule(f"{engine} dweight_F", _np(layer.weight_F.grad), g32["W"], g64["W"])
    check_rule("fused fallback against the literal engine", _np(outs["fused"][0]), _np(outs["literal"][0]), Y64)


def test_bf16_operand_with_blocks_is_refused():
    g = _graph("g1")
    layer = GraphConvolution(8, 8, g["R"], g["N"], num_blocks=2).cuda()
    layer.operand_dtype = "bf16"
    with pytest.raises(_lib.MrgcnError):
        layer(torch.zeros((g["N"], 8), device="cuda"), g["A"])


# ---- 2e. the model -------------------------------------------------------------------------------------------------------
CYC_N, CYC_R, CYC_SEED = 40, 3, 17


def _cycle():
    from mrgcn_amd.data.batch import scipy_sparse_to_pytorch_sparse
    from mrgcn_amd.data.graph_structure import adjacency_from_triples
    facts = np.stack([np.arange(CYC_N), np.zeros(CYC_N, np.int64), (np.arange(CYC_N) + 1) % CYC_N], 1).astype(np.int64)
    A_csr = adjacency_from_triples(facts, CYC_N, 1)
    assert A_csr.shape == (CYC_N, CYC_R * CYC_N) and np.all(A_csr.data == 1.0)   # (slices and the full graph agree)
    A = scipy_sparse_to_pytorch_sparse(A_csr, dtype=torch.float32).cuda()
    rng = np.random.default_rng(5)
    neg = facts.copy()
    neg[:20, 0] = rng.integers(0, CYC_N, 20)
    neg[20:, 2] = rng.integers(0, CYC_N, 20)
    triples = np.concatenate([facts, neg])
    labels = np.concatenate([np.ones(CYC_N, np.float32), np.zeros(CYC_N, np.float32)])
    return facts, A_csr, A, triples, labels


def _cycle_model():
    from mrgcn_amd.models.rgcn import RGCN
    torch.manual_seed(CYC_SEED)
    return RGCN([(0, 8, "mrgcn", nn.ReLU()), (8, 8, "mrgcn", None)], CYC_R, CYC_N, 2, 0.0, True, False, True,
                num_blocks=2)


def _model_ref(dtype, dense, sd, triples, labels):
    """The model's loss in torch ops on the CPU: (loss, E, layer 0's pre-activations, the leaves by state-dict key)."""
    leaves = {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    A = torch.tensor(dense, dtype=dtype)
    N, R = CYC_N, CYC_R
    comp, wI = leaves["layers.layer_0.weight_I_comp"], leaves["layers.layer_0.weight_I"]
    Z0 = A @ (comp @ wI.view(2, N * 8)).view(R * N, 8)
    H = torch.relu(Z0)
    FW = torch.matmul(H.unsqueeze(0), block_weight_dense(leaves["layers.layer_1.weight_F"])).reshape(R * N, 8)
    E = A @ FW
    t = torch.from_numpy(triples)
    score = (E[t[:, 0]] * leaves["relations"][t[:, 1]] * E[t[:, 2]]).sum(1)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(score, torch.tensor(labels, dtype=dtype))
    return loss, E, Z0, leaves


def test_model_gradients_slices_and_the_masked_refusal():
    from mrgcn_amd.data import batch as mb
    from mrgcn_amd.plan import plan_of
    from mrgcn_amd.tasks import link_prediction as lp
    facts, A_csr, A, triples, labels = _cycle()
    dense = np.asarray(A_csr.todense(), np.float64)
    model = _cycle_model()
    assert sorted(model.state_dict()) == ["layers.layer_0.weight_I", "layers.layer_0.weight_I_comp",
                                          "layers.layer_1.weight_F", "relations"]
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    loss64, E64, Z0, leaves64 = _model_ref(torch.float64, dense, sd, triples, labels)
    loss32, E32, _, leaves32 = _model_ref(torch.float32, dense, sd, triples, labels)
    assert float(Z0.detach().abs().min()) > 1e-5, f"a pre-activation of layer 0 within 1e-5 of zero ({Z0.abs().min():.3e})"
    loss64.backward()
    loss32.backward()
    model = model.cuda()
    td, yd = torch.from_numpy(triples).cuda(), torch.from_numpy(labels).cuda()
    mrgcn_amd.reset_stats()
    E = model(None, A)
    assert mrgcn_amd.stats().get("layer.block", 0) == 1
    loss = lp.binary_crossentropy(lp.score_distmult_bc(td, E, model.relations), yd)
    loss.backward()
    check_rule("model E", _np(E), E32.detach().numpy(), E64.detach().numpy())
    check_rule("model loss", _np(loss), loss32.detach().numpy(), loss64.detach().numpy())
    for name, p in model.named_parameters():
        assert p.grad is not None, name
        g32, g64 = leaves32[name].grad.numpy(), leaves64[name].grad.numpy()
        if name.endswith("layer_0.weight_I"):   # the parameter is node-major, the state dict the reference's rows
            g32, g64 = (a.reshape(2, CYC_N, 8).transpose(1, 0, 2) for a in (g32, g64))
        check_rule("model d" + name, _np(p.grad), g32, g64)
    # the slice mini-batch forward of the same model: the full-batch rows of the batch nodes
    batch_idx = np.array([3, 17, 18, 39, 0])
    ab = mb.A_Batch(A_csr, batch_idx, 2)
    ab.as_tensors_()
    ab.to(torch.device("cuda"))
    mrgcn_amd.reset_stats()
    with torch.no_grad():
        Eb = model(None, ab)
    assert mrgcn_amd.stats().get("layer.block", 0) == 1 and tuple(Eb.shape) == (len(batch_idx), 8)
    check_rule("slice mini-batch rows", _np(Eb), E32.detach().numpy()[batch_idx], E64.detach().numpy()[batch_idx])
    # a masked batch has no block-diagonal pass yet
    am = mb.A_BatchMasked(plan_of(A, CYC_N, CYC_R), batch_idx, 2)
    with pytest.raises(_lib.MrgcnError):
        model(None, am)
    am.close()


def test_train_step_replayed_equals_eager():
    from mrgcn_amd.tasks import link_prediction as lp
    from mrgcn_amd.train import ClipAdam, GraphedStep
    facts, A_csr, A, triples, labels = _cycle()
    td, yd = torch.from_numpy(triples).cuda(), torch.from_numpy(labels).cuda()
    sampler = lambda: (td, yd)   # noqa: E731
    static = lp.SortedTriples(td[:CYC_N].contiguous(), CYC_N, CYC_R)
    with deterministic():
        runs = []
        for graphed in (False, True):
            model = _cycle_model().cuda()
            opt = ClipAdam(model.parameters(), lr=0.05, weight_decay=0.0, max_norm=1.0, capturable=True)
            step = lambda: lp.train_step(model, lambda: model(None, A), sampler, opt, static)   # noqa: E731
            if graphed:
                gs = GraphedStep(step, warmup=3)      # three real steps, then the captured one
                loss = gs().clone()
            else:
                for _ in range(4):
                    loss = step()
            torch.cuda.synchronize()
            runs.append((_np(loss).tobytes(), {k: _np(v).tobytes() for k, v in model.state_dict().items()}))
    assert runs[0][0] == runs[1][0]
    for k in runs[0][1]:
        assert runs[0][1][k] == runs[1][1][k], k
    assert np.isfinite(np.frombuffer(runs[0][0], np.float32)).all()
