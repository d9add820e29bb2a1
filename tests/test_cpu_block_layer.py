"""Block-diagonal relation weights (Schlichtkrull et al. 2018, eq. 4) without a device: the layer's parameters and
constructor errors, `layers.graph.block_weight_dense`, the host mirrors of csrc/block_xform.hip, the C entries'
declarations.  Also the graphs, shapes and the tolerance rule tests/test_gpu_block_layer.py shares.

Tolerance rule.  Nothing is fixed in advance: per case the float32 host restatement is measured against the float64 one
on the same inputs and the quantity under test gets 4 x that maximum error, with a floor of one float32 ulp of the
compared value.  No element is excluded; every message carries the error, the restatement's error and the allowance."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from mrgcn_amd import _lib, host
from mrgcn_amd.layers.graph import GraphConvolution, block_weight_dense
from tests.test_cpu_host import ROOT, header_functions

NAMES = ("mrgcn_block_transform_supported", "mrgcn_block_transform_fwd_f32", "mrgcn_block_transform_bwd_workspace",
         "mrgcn_block_transform_bwd_f32")
CTYPE = {"int32_t": C.c_int32, "int64_t": C.c_int64, "int": C.c_int}

# (K, F, NB)
SHAPES = [(8, 8, 2), (6, 6, 6), (16, 16, 1), (12, 20, 4), (10, 6, 2), (200, 200, 40), (256, 256, 4)]


# ---- shared with the GPU tests ---------------------------------------------------------------------------------------
def graph_g1():
    """G1: 37 nodes, 5 relations, 316 entries as (N, R, rows, literal columns r N + j, values).  Relation 3 has no
    entry, node 36 is the source of none, some (row, column) pairs are stored twice, and node 0 is a hub: every row
    reads its columns under relations 0 and 4 (74 entries).  A compact column is a (source node, relation) pair, so
    with 5 relations no node can own more than 5 of them: the node that owns more than 64 columns is in `graph_g1_wide`,
    which the kernel tests run beside this graph."""
    N, R = 37, 5
    rng = np.random.default_rng(101)
    rows, cols = [], []
    for _ in range(230):
        r = int(rng.choice([0, 1, 2, 4]))
        j = int(rng.integers(0, 36))           # node 36 is never a source
        rows.append(int(rng.integers(0, N)))
        cols.append(r * N + j)
    for i in range(N):                          # node 0: read by every row under relations 0 and 4
        rows += [i, i]
        cols += [0 * N + 0, 4 * N + 0]
    rows += rows[:12]                           # duplicate (row, column) entries
    cols += cols[:12]
    vals = rng.integers(1, 4, len(rows)).astype(np.float32)
    return N, R, np.asarray(rows, np.int64), np.asarray(cols, np.int64), vals


def graph_g1_wide():
    """G1's node count with 70 relations, node 0 a source under 67 of them: one node that owns more than 64 compact
    columns (the dX walk of one node runs past a wave's width).  Relation 3 stays empty and node 36 without outgoing
    entries; duplicates as in G1."""
    N, R = 37, 70
    rng = np.random.default_rng(102)
    rows, cols = [], []
    for r in range(R):
        if r == 3:
            continue
        if r >= 3:
            rows.append(int(rng.integers(0, N)))
            cols.append(r * N + 0)
        for _ in range(3):
            rows.append(int(rng.integers(0, N)))
            cols.append(r * N + int(rng.integers(0, 36)))
    rows += rows[:9]
    cols += cols[:9]
    vals = rng.integers(1, 4, len(rows)).astype(np.float32)
    return N, R, np.asarray(rows, np.int64), np.asarray(cols, np.int64), vals


def graph_g2():
    """G2: 700 nodes, 3 relations; relation 1 owns 650 compact columns (the dW walk crosses three units of 256 columns
    of one group), relation 0 about 90, relation 2 a handful."""
    N, R = 700, 3
    rng = np.random.default_rng(103)
    rows, cols = [], []
    for j in range(650):
        rows.append(int(rng.integers(0, N)))
        cols.append(1 * N + j)
    for _ in range(100):
        rows.append(int(rng.integers(0, N)))
        cols.append(0 * N + int(rng.integers(0, N)))
    for _ in range(7):
        rows.append(int(rng.integers(0, N)))
        cols.append(2 * N + int(rng.integers(0, N)))
    vals = rng.integers(1, 3, len(rows)).astype(np.float32)
    return N, R, np.asarray(rows, np.int64), np.asarray(cols, np.int64), vals


def compact_columns(N, cols):
    """(node, rel) of the compact columns of a graph: its distinct literal columns in (node, relation) order — the
    plan's compact ids (include/mrgcn_hip.h: MRGCN_ARR_UNODE / _UREL)."""
    u = np.unique(cols)
    node, rel = u % N, u // N
    order = np.lexsort((rel, node))
    return node[order], rel[order]


def case_inputs(N, R, K, F, NB, seed):
    """X [N, K], W (R, NB, ki, fo), dM [.., F] generator: float32 arrays of N(0, 1) scaled like a Glorot layer."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, K)).astype(np.float32)
    W = (rng.standard_normal((R, NB, K // NB, F // NB)) * np.sqrt(2.0 / (K // NB + F // NB))).astype(np.float32)
    return X, W, rng


def ulp32(x):
    """One float32 ulp of |x| (of the smallest normal at and below it)."""
    a = np.maximum(np.abs(np.asarray(x, np.float64)), float(np.finfo(np.float32).tiny)).astype(np.float32)
    return (np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64)


def check_rule(what, got, r32, r64):
    """`got` against the float64 statement `r64` under the rule; returns the share of the allowance used."""
    got, r32, r64 = (np.asarray(a, np.float64) for a in (got, r32, r64))
    assert got.shape == r64.shape == r32.shape, (what, got.shape, r32.shape, r64.shape)
    err32 = float(np.abs(r32 - r64).max()) if r64.size else 0.0
    allow = np.maximum(4.0 * err32, ulp32(r64))
    err = np.abs(got - r64)
    share = float((err / allow).max()) if r64.size else 0.0
    worst = float(err.max()) if r64.size else 0.0
    print(f"{what}: error {worst:.3e}, restatement {err32:.3e}, allowance {float(allow.min()):.3e}, share {share:.3f}")
    assert np.all(err <= allow), (f"{what}: error {worst:.3e}, float32 restatement's error {err32:.3e}, allowance "
                                  f"{float(allow.min()):.3e} (share {share:.3f})")
    return share


# ---- 1a. constructor ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,F,NB", SHAPES)
def test_constructor_shapes(K, F, NB):
    layer = GraphConvolution(K, F, 5, 11, num_bases=2, bias=True, num_blocks=NB)
    assert tuple(layer.weight_F.shape) == (5, NB, K // NB, F // NB)
    assert layer.weight_F_comp is None and layer.weight_I is None and layer.num_blocks == NB
    assert list(layer.state_dict()) == ["weight_F", "b"]
    bound = np.sqrt(6.0 / (K // NB + F // NB))
    w = layer.weight_F.detach().numpy()
    assert np.abs(w).max() <= bound and (w.size < 500 or np.abs(w).max() > 0.8 * bound)
    # an input layer keeps its bases for the node table
    both = GraphConvolution(K, F, 5, 11, num_bases=2, bias=False, input_layer=True, num_blocks=NB)
    assert list(both.state_dict()) == ["weight_I_comp", "weight_I", "weight_F"]
    assert tuple(both.weight_I.shape) == (11, 2, F) and tuple(both.state_dict()["weight_I"].shape) == (22, F)


def test_constructor_errors():
    with pytest.raises(_lib.MrgcnError):
        GraphConvolution(9, 8, 3, 7, num_blocks=2)
    with pytest.raises(_lib.MrgcnError):
        GraphConvolution(8, 9, 3, 7, num_blocks=2)
    with pytest.raises(_lib.MrgcnError):
        GraphConvolution(8, 8, 3, 7, num_bases=2, input_layer=True, featureless=True, num_blocks=2)
    with pytest.raises(_lib.MrgcnError):
        GraphConvolution(8, 8, 3, 7, num_bases=2, input_layer=True, shared_bases_weights=True, num_blocks=2)
    from mrgcn_amd.partition import PartitionedRGCN
    from mrgcn_amd.partition_halo import HaloPartitionedRGCN
    for cls in (PartitionedRGCN, HaloPartitionedRGCN):
        with pytest.raises(_lib.MrgcnError):
            cls([(0, 8, "mrgcn", None), (8, 8, "mrgcn", None)], 3, 7, 2, True, False, None, num_blocks=2)


def test_the_draw_takes_weight_F_position_in_the_stream():
    """Registration order weight_I_comp, (no weight_F_comp), weight_I, weight_F, b: the same draws made by hand."""
    torch.manual_seed(5)
    b = GraphConvolution(8, 12, 3, 7, num_bases=2, bias=True, input_layer=True, num_blocks=4)
    torch.manual_seed(5)
    comp = torch.nn.init.xavier_uniform_(torch.empty(3, 2))
    w_i = torch.nn.init.xavier_uniform_(torch.empty(2 * 7, 12))
    bound = (6.0 / (2 + 3)) ** 0.5
    w_f = torch.nn.init.uniform_(torch.empty(3, 4, 2, 3), -bound, bound)
    assert torch.equal(b.weight_I_comp, comp) and torch.equal(b.state_dict()["weight_I"], w_i)
    assert torch.equal(b.weight_F, w_f) and not b.b.any()


# ---- 1b. the dense form ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,F,NB", SHAPES[:5])
def test_block_weight_dense_is_block_diag_and_differentiable(K, F, NB):
    g = torch.Generator().manual_seed(K + F)
    W = torch.randn((3, NB, K // NB, F // NB), generator=g, dtype=torch.float64, requires_grad=True)
    D = block_weight_dense(W)
    assert tuple(D.shape) == (3, K, F)
    for r in range(3):
        assert torch.equal(D[r], torch.block_diag(*[W[r, b] for b in range(NB)]))
    assert np.array_equal(host.block_weight_dense64(W.detach().numpy()), D.detach().numpy())
    assert torch.autograd.gradcheck(block_weight_dense, (W,))


# ---- 1c. host mirrors --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,F,NB", SHAPES)
def test_host_mirrors(K, F, NB):
    N, R, rows, cols, vals = graph_g1()
    node, rel = compact_columns(N, cols)
    X, W, rng = case_inputs(N, R, K, F, NB, seed=K * 1000 + F)
    o32, o64 = host.block_transform32(X, W, node, rel), host.block_transform64(X, W, node, rel)
    assert o32.dtype == np.float32 and o64.dtype == np.float64 and o32.shape == (len(node), F)
    Xt = torch.tensor(X, dtype=torch.float64, requires_grad=True)
    Wt = torch.tensor(W, dtype=torch.float64, requires_grad=True)
    dense = torch.einsum("ck,ckf->cf", Xt[torch.from_numpy(node)], block_weight_dense(Wt)[torch.from_numpy(rel)])
    # the float64 mirror against float64 torch of the dense form: two float64 statements, a few float64 ulps apart
    assert np.abs(o64 - dense.detach().numpy()).max() <= 1e-13 * max(1.0, np.abs(o64).max())
    check_rule("block_transform32", o32, o32, o64)   # (its own yardstick: asserts only that the rule is usable)
    assert np.abs(o32 - o64).max() <= 1e-5 * max(1.0, np.abs(o64).max())
    dM = rng.standard_normal((len(node), F)).astype(np.float32)
    (dense * torch.from_numpy(dM).double()).sum().backward()
    dX64, dW64 = host.block_transform_bwd64(dM, X, W, node, rel, N)
    assert np.abs(dX64 - Xt.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(dX64).max())
    assert np.abs(dW64 - Wt.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(dW64).max())
    dX32, dW32 = host.block_transform_bwd32(dM, X, W, node, rel, N)
    assert dX32.dtype == np.float32 and dW32.dtype == np.float32
    assert np.abs(dX32 - dX64).max() <= 1e-4 * max(1.0, np.abs(dX64).max())
    assert np.abs(dW32 - dW64).max() <= 1e-4 * max(1.0, np.abs(dW64).max())
    assert not dW64[3].any() and not dX64[36].any()   # the empty relation, the node without a column


# ---- 1d. declarations --------------------------------------------------------------------------------------------------
def _header_signature(name):
    src = open(os.path.join(ROOT, "include", "mrgcn_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in the header"
    args = [C.c_void_p if "*" in a else CTYPE[a.replace("const ", "").split()[0]]
            for a in (x.strip() for x in m.group(2).split(",")) if a != "void"]
    return CTYPE[m.group(1)], args


def test_symbols_are_declared_exported_and_bound():
    declared = set(header_functions())
    lib = _lib.load()
    for n in NAMES:
        assert n in declared, f"{n} is not declared in include/mrgcn_hip.h"
        assert n in _lib.SIGNATURES, f"{n} is not in the ctypes table"
        assert hasattr(lib, n), f"{n} is not exported by the library"
        res, args = _header_signature(n)
        assert _lib.SIGNATURES[n][0] is res, n
        assert list(_lib.SIGNATURES[n][1]) == args, n
    src = open(os.path.join(ROOT, "include", "mrgcn_hip.h")).read()
    assert re.search(r"#define\s+MRGCN_ABI_VERSION\s+5\b", src)
    assert _lib.ABI_VERSION == 5 and lib.mrgcn_abi_version() == 5
    # without a plan nothing is supported, no workspace is asked for and the calls refuse before any launch
    assert lib.mrgcn_block_transform_supported(None, 8, 8, 2) == 0
    assert lib.mrgcn_block_transform_bwd_workspace(None, 8, 8, 2, 1, 1) == 0
    assert lib.mrgcn_block_transform_fwd_f32(None, None, 8, 8, None, 2, 8, None, 8, 0, None) != 0
    assert lib.mrgcn_block_transform_bwd_f32(None, None, 8, None, 8, 8, None, 2, 8, None, 8, None, None, 0, None) != 0


# ---- 1e. state dict, deepcopy ------------------------------------------------------------------------------------------
def test_state_dict_round_trip_and_deepcopy():
    torch.manual_seed(3)
    a = GraphConvolution(12, 20, 4, 9, num_bases=2, bias=True, input_layer=True, num_blocks=4)
    sd = a.state_dict()
    assert tuple(sd["weight_F"].shape) == (4, 4, 3, 5) and torch.equal(sd["weight_F"], a.weight_F)
    torch.manual_seed(4)
    b = GraphConvolution(12, 20, 4, 9, num_bases=2, bias=True, input_layer=True, num_blocks=4)
    assert not torch.equal(a.weight_F, b.weight_F)
    b.load_state_dict(sd)
    for (k, x), (_, y) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(x, y), k
    c = copy.deepcopy(a)
    assert c.num_blocks == 4 and torch.equal(c.weight_F, a.weight_F) and c.weight_F is not a.weight_F
    assert getattr(c.weight_I, "_mrgcn_node_major", False)
    assert torch.equal(c.weight_F_dense(), block_weight_dense(a.weight_F))


# ---- 1f. the default changes nothing -----------------------------------------------------------------------------------
def test_default_leaves_parameters_and_the_rng_stream_alone():
    import inspect
    import torch.nn as nn
    from mrgcn_amd.models.rgcn import RGCN
    kw = {"num_blocks": -1} if "num_blocks" in inspect.signature(GraphConvolution.__init__).parameters else {}
    for args in (dict(num_bases=2, bias=True, input_layer=True), dict(num_bases=-1, bias=False),
                 dict(num_bases=3, bias=True, input_layer=True, featureless=True)):
        torch.manual_seed(7)
        a = GraphConvolution(8, 6, 3, 10, **args)
        after_a = torch.rand(4)
        torch.manual_seed(7)
        b = GraphConvolution(8, 6, 3, 10, **args, **kw)
        after_b = torch.rand(4)
        assert list(a.state_dict()) == list(b.state_dict())
        for (k, x), (_, y) in zip(a.state_dict().items(), b.state_dict().items()):
            assert x.shape == y.shape and torch.equal(x, y), k
        assert torch.equal(after_a, after_b)
    mods = [(0, 8, "mrgcn", nn.ReLU()), (8, 8, "mrgcn", None)]
    torch.manual_seed(9)
    m1 = RGCN(mods, 5, 12, 2, 0.0, True, True, True)
    torch.manual_seed(9)
    m2 = RGCN(mods, 5, 12, 2, 0.0, True, True, True, **kw)
    assert list(m1.state_dict()) == list(m2.state_dict())
    for (k, x), (_, y) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert x.shape == y.shape and torch.equal(x, y), k
    assert tuple(m1.state_dict()["layers.layer_1.weight_F"].shape) == (2, 8, 8)


def test_models_pass_num_blocks_to_layers_with_a_feature_term():
    import torch.nn as nn
    from mrgcn_amd.models.rgcn import RGCN
    mods = [(0, 8, "mrgcn", nn.ReLU()), (8, 8, "mrgcn", None)]
    m = RGCN(mods, 5, 12, 2, 0.0, True, True, True, num_blocks=2)
    assert m.layers["layer_0"].num_blocks == -1 and m.layers["layer_0"].num_bases == 2
    assert m.layers["layer_1"].num_blocks == 2
    assert tuple(m.state_dict()["layers.layer_1.weight_F"].shape) == (5, 2, 4, 4)
    assert "layers.layer_1.weight_F_comp" not in m.state_dict()
