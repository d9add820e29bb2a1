"""The layer-0 dW from a table of per-(row, relation) sums of a constant X (csrc/support.hip: k_pair_sums, k_dw_pairs;
plan.GraphSupport.pair_sums): S[p] = sum of val_e . X[node_e] over the entries of pair p = (row, relation),
dW[r] = sum over r's pairs of S[p]^T . dY[row_p].

Tolerance.  An element that is a sum of n products computed in fp32 — whatever the order, each term passing through at
most n roundings of relative size 2^-24 — lies within n . 2^-24 . sum|terms| of the exact sum (the standard summation
bound, first order).  For S[p][k] the terms are val_e . X[node_e][k] over the pair's entries; for dW[r][k][f] they are
val_e . X[node_e][k] . dY[row_e][f] over the relation's kept entries.  The bound is computed per element from the float64
restatement; the gather kernel (mrgcn_support_rel_transform_bwd_f32) is held to the same bound on the same inputs."""
import numpy as np
import pytest
import torch

from tests.test_gpu_plan_spmm import _plan_from_coo

pytestmark = pytest.mark.gpu

N, R = 300, 6
HUB, U = 7, 2.0 ** -24


def _graph():
    """rows 0..199 are labelled.  Relation 0: every row has entries (200 pairs: two chunks); 1: few scattered entries
    (pairs of one entry); 2: the hub row reads every node (300 entries: five pieces); 3: entries in unlabelled rows
    only (no pair); 4: random; 5: self loops.  Values as in `norm_f32`: 1 / (entries of the (row, relation) pair)."""
    rng = np.random.default_rng(11)
    rr, cc = [], []

    def add(r, rows, nodes):
        rr.append(np.asarray(rows, dtype=np.int64))
        cc.append(r * N + np.asarray(nodes, dtype=np.int64))
    for i in range(N):
        add(0, np.full(3, i), rng.choice(N, 3, replace=False))
    add(1, rng.integers(0, N, 60), rng.integers(0, N, 60))
    add(2, np.full(N, HUB), np.arange(N))
    add(3, rng.integers(200, N, 150), rng.integers(0, N, 150))
    add(4, rng.integers(0, N, 1500), rng.integers(0, N, 1500))
    add(5, np.arange(N), np.arange(N))
    key = np.unique(np.concatenate(rr) * (R * N) + np.concatenate(cc))
    rows, cols = key // (R * N), key % (R * N)
    pair = rows * R + cols // N
    cnt = np.bincount(pair, minlength=N * R)
    vals = (1.0 / cnt[pair]).astype(np.float32)
    perm = rng.permutation(len(key))
    flags = np.zeros(N, dtype=np.uint8)
    flags[:200] = 1
    return rows[perm], cols[perm], vals[perm], flags


@pytest.fixture(scope="module")
def world():
    from mrgcn_amd import _lib as L
    rows, cols, vals, flags = _graph()
    plan = _plan_from_coo(rows, cols, vals, N, N, R)
    sup = plan.support_for(torch.from_numpy(flags).cuda())
    info = sup.pair_structure(155)
    host = {n: sup.export(getattr(L, "SUP_" + n.upper()))
            for n in ("pair_ptr", "pair_row", "rel_pair_ptr", "pair_node", "pair_val", "pair_chunk_ptr")}
    # the float64 side's own pairs: kept entries sorted by (relation, row)
    keep = flags[rows] == 1
    er, ec, ev = rows[keep], cols[keep], vals[keep]
    pkey = (ec // N) * N + er
    order = np.argsort(pkey, kind="stable")
    er, ec, ev, pkey = er[order], ec[order], ev[order], pkey[order]
    upair, first = np.unique(pkey, return_index=True)
    w = dict(plan=plan, sup=sup, info=info, host=host, flags=flags, er=er, en=ec % N, ev=ev.astype(np.float64),
             epair=np.searchsorted(upair, pkey), upair=upair, first=first)
    yield w
    plan.close()


def test_the_support_holds_the_four_cases(world):
    h, info = world["host"], world["info"]
    P = int(info.pairs)
    assert P == len(world["upair"]) and len(h["pair_ptr"]) == P + 1 and h["pair_ptr"][-1] == world["sup"].E
    np.testing.assert_array_equal(h["pair_row"], world["upair"] % N)
    np.testing.assert_array_equal(h["rel_pair_ptr"], np.searchsorted(world["upair"] // N, np.arange(R + 1)))
    lens = np.diff(h["pair_ptr"])
    assert (lens >= 1).all() and (lens == 1).any()                     # a pair with exactly one entry
    assert lens.max() >= 300 and lens.max() > info.piece_entries       # the hub row: pieces
    assert int(info.max_pair_entries) == lens.max()
    per_rel = np.diff(h["rel_pair_ptr"])
    assert (per_rel == 0).any()                                        # a relation with no pair at all
    assert per_rel.max() > info.chunk_pairs                            # a relation whose pairs span several chunks
    chunks = np.diff(h["pair_chunk_ptr"])
    assert chunks.max() >= 2 and (chunks[per_rel == 0] == 0).all() and chunks.sum() == info.chunks
    # entries of a pair keep the transposed view's order: (node, then nothing else — one entry per (row, column))
    for p in np.flatnonzero(lens > 1)[:50]:
        assert (np.diff(h["pair_node"][h["pair_ptr"][p]:h["pair_ptr"][p + 1]]) > 0).all()


def _reference(world, X, dY):
    """float64 S [P, K], dW [R, K, F] and the per-element bounds n . 2^-24 . sum|terms|"""
    P = len(world["upair"])
    X64, dY64 = X.astype(np.float64), dY.astype(np.float64)
    terms = world["ev"][:, None] * X64[world["en"]]
    S, Sabs = np.zeros((P, X.shape[1])), np.zeros((P, X.shape[1]))
    np.add.at(S, world["epair"], terms)
    np.add.at(Sabs, world["epair"], np.abs(terms))
    n_pair = np.bincount(world["epair"], minlength=P)
    prow, prel = world["upair"] % N, world["upair"] // N
    dW, dWabs, n_rel = np.zeros((R,) + (X.shape[1], dY.shape[1])), np.zeros((R,) + (X.shape[1], dY.shape[1])), np.zeros(R)
    for r in range(R):
        m = prel == r
        dW[r] = S[m].T @ dY64[prow[m]]
        dWabs[r] = Sabs[m].T @ np.abs(dY64[prow[m]])
        n_rel[r] = n_pair[m].sum()
    return S, n_pair[:, None] * U * Sabs, dW, n_rel[:, None, None] * U * dWabs


def _run_pairs(sup, X, dY, K, F):
    from mrgcn_amd import _lib as L
    lib, s = L.load(), torch.cuda.current_stream().cuda_stream
    P = int(sup.pair_structure(K).pairs)
    S = torch.full((P, K), 7.0, device="cuda")
    L.check(lib.mrgcn_support_pair_sums_build_f32(sup.handle, X.data_ptr(), X.stride(0), K, S.data_ptr(), s))
    nws = int(lib.mrgcn_support_dw_pairs_workspace(sup.handle, K, F))
    ws = torch.empty(nws, device="cuda")
    dW = torch.full((R, K, F), 7.0, device="cuda")
    L.check(lib.mrgcn_support_dw_pairs_f32(sup.handle, S.data_ptr(), K, dY.data_ptr(), dY.stride(0), F, dW.data_ptr(),
                                           ws.data_ptr(), nws, s))
    return S, dW


def _run_gather(sup, X, dY, K, F):
    from mrgcn_amd import _lib as L
    lib, s = L.load(), torch.cuda.current_stream().cuda_stream
    ld = (F + 3) // 4 * 4
    dM = torch.zeros((sup.L, ld), device="cuda")
    L.check(lib.mrgcn_support_spmm_t_f32(sup.handle, dY.data_ptr(), dY.stride(0), F, dM.data_ptr(), ld, s))
    nws = int(lib.mrgcn_support_rel_transform_bwd_workspace(sup.handle, K, F, 0, 1))
    assert nws > 0
    ws = torch.empty(nws, device="cuda")
    W, dW = torch.zeros((R, K, F), device="cuda"), torch.full((R, K, F), 7.0, device="cuda")
    L.check(lib.mrgcn_support_rel_transform_bwd_f32(sup.handle, dM.data_ptr(), ld, X.data_ptr(), X.stride(0), K,
                                                    W.data_ptr(), F, 0, K, dW.data_ptr(), ws.data_ptr(), nws, 0, s))
    return dW


def _inputs(K, F):
    rng = np.random.default_rng(100 * K + F)
    X = rng.standard_normal((N, K)).astype(np.float32)
    dY = rng.standard_normal((N, F)).astype(np.float32)
    return X, dY


@pytest.mark.parametrize("K", [17, 21, 155])
@pytest.mark.parametrize("F", [3, 10])
def test_table_and_dw_against_float64(world, K, F):
    sup = world["sup"]
    X, dY = _inputs(K, F)
    dYp = dY.copy()
    dYp[world["flags"] == 0] = np.nan   # rows outside the row set are never read
    Xd, dYd = torch.from_numpy(X).cuda(), torch.from_numpy(dYp).cuda()
    S, dW = _run_pairs(sup, Xd, dYd, K, F)
    dWg = _run_gather(sup, Xd, dYd, K, F)
    S64, Sb, dW64, dWb = _reference(world, X, dY)
    eS = np.abs(S.cpu().numpy().astype(np.float64) - S64)
    eW = np.abs(dW.cpu().numpy().astype(np.float64) - dW64)
    eG = np.abs(dWg.cpu().numpy().astype(np.float64) - dW64)
    print(f"K={K} F={F}: max err/bound  S {np.max(eS / np.maximum(Sb, 1e-300)):.3f}  "
          f"dW pairs {np.max(eW / np.maximum(dWb, 1e-300)):.3f}  dW gather {np.max(eG / np.maximum(dWb, 1e-300)):.3f}")
    assert (eS <= Sb).all()
    assert (eW <= dWb).all()
    assert (eG <= dWb).all()
    empty = np.flatnonzero(np.diff(world["host"]["rel_pair_ptr"]) == 0)
    assert len(empty) and (dW.cpu().numpy()[empty] == 0).all()   # exact zeros for a relation without pairs


@pytest.mark.parametrize("K", [17, 21, 155])
@pytest.mark.parametrize("F", [3, 10])
def test_build_and_contraction_leave_the_same_bits_twice(world, K, F):
    X, dY = _inputs(K, F)
    Xd, dYd = torch.from_numpy(X).cuda(), torch.from_numpy(dY).cuda()
    S1, W1 = _run_pairs(world["sup"], Xd, dYd, K, F)
    S2, W2 = _run_pairs(world["sup"], Xd, dYd, K, F)
    assert torch.equal(S1, S2) and torch.equal(W1, W2)


# ---- the cache on the support and the path choice -------------------------------------------------------------------
def _layer_case(K=21, F=10):
    from mrgcn_amd.layers.graph import GraphConvolution
    rows, cols, vals, flags = _graph()
    plan = _plan_from_coo(rows, cols, vals, N, N, R)
    torch.manual_seed(3)
    layer = GraphConvolution(K, F, R, N, num_bases=-1, bias=False, input_layer=False, featureless=False).cuda()
    idx = torch.arange(200, device="cuda")
    tgt = torch.from_numpy(np.random.default_rng(5).integers(0, F, 200)).cuda()
    return plan, layer, idx, tgt


def _layer_dw(plan, layer, X, idx, tgt):
    import mrgcn_amd.functional as Fn
    from mrgcn_amd.train import categorical_crossentropy
    layer.weight_F.grad = None
    Y = Fn.rgcn_layer(plan, layer, X)
    Y.retain_grad()
    categorical_crossentropy(Y, idx, tgt).backward()
    return layer.weight_F.grad.clone(), Y.grad.clone()


def test_cache_rules(monkeypatch):
    import mrgcn_amd
    import mrgcn_amd.functional as Fn
    plan, layer, idx, tgt = _layer_case()
    rows, cols, vals, flags = _graph()
    K = layer.indim
    X = torch.randn((N, K), device="cuda", generator=torch.Generator("cuda").manual_seed(1))

    def check(dW, dY, Xt, w):
        _, _, dW64, dWb = _reference(w, Xt.cpu().numpy(), dY.cpu().numpy())
        assert (np.abs(dW.cpu().numpy().astype(np.float64) - dW64) <= dWb).all()

    keep = flags[rows] == 1
    er, ec, ev = rows[keep], cols[keep], vals[keep]
    pkey = (ec // N) * N + er
    order = np.argsort(pkey, kind="stable")
    upair = np.unique(pkey)
    w = dict(ev=ev[order].astype(np.float64), en=(ec % N)[order], epair=np.searchsorted(upair, pkey[order]), upair=upair)

    # the default cap is the byte size of X: this small dense graph has more pairs than nodes, so the gather kernel runs
    mrgcn_amd.reset_stats()
    dW0, dY0 = _layer_dw(plan, layer, X, idx, tgt)
    assert mrgcn_amd.stats().get("backward.dw_pair_sums") is None and mrgcn_amd.stats().get("backward.support") == 1
    check(dW0, dY0, X, w)
    monkeypatch.setattr(Fn, "_DW_PAIR_SUMS_CAP", 1 << 30)
    mrgcn_amd.reset_stats()
    dW, dY = _layer_dw(plan, layer, X, idx, tgt)
    st = mrgcn_amd.stats()
    assert st.get("backward.dw_pair_sums") == 1 and st.get("dw_pair_sums.build") == 1, st
    check(dW, dY, X, w)
    sup = next(iter(plan.__dict__["_supports"].values()))
    info = sup.pair_sums_info()
    assert info["active"] and info["builds"] == 1 and info["table_bytes"] == info["pairs"] * K * 4
    # a second backward reads the table it has
    dW2, _ = _layer_dw(plan, layer, X, idx, tgt)
    assert mrgcn_amd.stats().get("dw_pair_sums.build") == 1 and torch.equal(dW2, dW)
    # an in-place change of X: rebuilt, and the dW is that of the new X
    X.add_(1)
    dW3, dY3 = _layer_dw(plan, layer, X, idx, tgt)
    assert mrgcn_amd.stats().get("dw_pair_sums.build") == 2 and not torch.equal(dW3, dW)
    check(dW3, dY3, X, w)
    # a fresh tensor: the same
    X2 = X * 0.5
    dW4, dY4 = _layer_dw(plan, layer, X2, idx, tgt)
    assert mrgcn_amd.stats().get("dw_pair_sums.build") == 3
    check(dW4, dY4, X2, w)
    # an input that wants a gradient: the gather kernel
    before = mrgcn_amd.stats().get("backward.dw_pair_sums")
    X2.requires_grad_(True)
    dW5, dY5 = _layer_dw(plan, layer, X2, idx, tgt)
    st = mrgcn_amd.stats()
    assert st.get("backward.dw_pair_sums") == before and st.get("dw_pair_sums.build") == 3 and X2.grad is not None
    check(dW5, dY5, X2.detach(), w)
    plan.close()


@pytest.mark.parametrize("K", [21, 155])
def test_replayed_epoch_sees_an_in_place_change_of_x(K, monkeypatch):
    """GraphedTrainStep re-checks the table's key in front of every replay: X changed in place between two replays gives
    the parameters of eager steps on the changed X (the same kernels in the same order: the tolerance the
    captured-epoch tests use, far inside the summation bound of a step on the stale X + 1)."""
    import mrgcn_amd
    from mrgcn_amd.models.rgcn import RGCN
    import mrgcn_amd.functional as Fn
    from mrgcn_amd.train import ClipAdam, GraphedTrainStep, train_step
    monkeypatch.setattr(Fn, "_DW_PAIR_SUMS_CAP", 1 << 30)   # (more pairs than nodes here: past the default cap)
    rows, cols, vals, flags = _graph()
    A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([rows, cols])), torch.from_numpy(vals), (N, R * N)).cuda()
    idx = torch.arange(200, device="cuda")
    tgt = torch.from_numpy(np.random.default_rng(5).integers(0, 4, 200)).cuda()
    out = []
    for graphed in (False, True):
        torch.manual_seed(0)
        model = RGCN([(K, 10, "mrgcn", torch.nn.ReLU()), (10, 4, "mrgcn", None)], R, N, 5, 0.0, False, True, False).cuda()
        X = torch.randn((N, K), device="cuda", generator=torch.Generator("cuda").manual_seed(2))
        opt = ClipAdam(model.parameters(), lr=0.01, max_norm=1.0, capturable=graphed)
        mrgcn_amd.reset_stats()
        if graphed:
            step = GraphedTrainStep(model, lambda: model(X, A), idx, tgt, opt, warmup=1)
            assert len(step._pair_sums) == 1 and mrgcn_amd.stats().get("dw_pair_sums.build") == 1
            step()
            X.add_(1)
            step()
            assert mrgcn_amd.stats().get("dw_pair_sums.build") == 2
        else:
            for i in range(3):
                if i == 2:
                    X.add_(1)
                train_step(model, lambda: model(X, A), idx, tgt, opt)
            assert mrgcn_amd.stats().get("backward.dw_pair_sums") == 3
        torch.cuda.synchronize()
        out.append({k: v.clone() for k, v in model.state_dict().items()})
    for k in out[0]:
        torch.testing.assert_close(out[0][k], out[1][k], rtol=1e-5, atol=1e-6, msg=k)
