"""Top-k candidate completion on the GPU (csrc/distmult_topk.hip through `predict_topk` / `predict_links`) against a
numpy construction: the oracle's sequential float32 scores, excluded candidates removed, order (score descending, node
id ascending, -0 == +0), rows padded with (-1, -inf).  Indices must be equal, scores equal bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import lp_oracle as lo

pytestmark = pytest.mark.gpu


def _dev(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _scores(E, Rel, queries, side):
    """[nq, N] float32, the association of the kernels: (E[s] Rel[p]) E[c] / (E[c] Rel[p]) E[o], summed in h order."""
    a, p = E[queries[:, 0]], Rel[queries[:, 1]]
    if side == "tail":
        prod = ((a * p).astype(np.float32)[:, None, :] * E[None]).astype(np.float32)
    else:
        prod = ((E[None] * p[:, None, :]).astype(np.float32) * a[:, None, :]).astype(np.float32)
    return lo._seq_sum_f32(prod)


def _expected(E, Rel, queries, side, k, lists=None):
    sc = _scores(E, Rel, queries, side)
    nq, N = sc.shape
    idx = np.full((nq, k), -1, np.int64)
    val = np.full((nq, k), -np.inf, np.float32)
    for i in range(nq):
        keep = np.ones(N, bool)
        if lists is not None:
            keep[lists[1][lists[0][i]:lists[0][i + 1]]] = False
        ids = np.arange(N)[keep]
        s = sc[i][keep] + np.float32(0.0)
        order = np.lexsort((ids, -s))[:k]
        idx[i, :len(order)] = ids[order]
        val[i, :len(order)] = s[order]
    return idx, val


def _assert_same(got, want):
    gi, gs = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert gi.dtype == np.int64 and gs.dtype == np.float32 and gi.shape == want[0].shape == gs.shape
    assert np.array_equal(gi, want[0])
    assert np.array_equal((gs + np.float32(0.0)).view(np.int32), (want[1] + np.float32(0.0)).view(np.int32))


def _table(N, H, P, seed):
    """Embeddings as in test_ranks_against_oracle_bit_exact (ReLU-style zeros, an eighth of the rows zero) with a few
    rows duplicated next to their source and far from it: exact ties inside a candidate tile and across tiles."""
    rng = np.random.default_rng(seed)
    E = np.maximum(rng.standard_normal((N, H)), 0).astype(np.float32)
    E[rng.choice(N, N // 8, replace=False)] = 0
    for src in rng.choice(N, 4, replace=False):
        E[(src + 1) % N] = E[src]
        E[(src + N // 2 + 3) % N] = E[src]
    Rel = rng.standard_normal((2 * P + 1, H)).astype(np.float32)
    return rng, E, Rel


def _padded(E):
    N, H = E.shape
    Epad = torch.zeros((N, H + 3), device="cuda")
    Epad[:, :H] = torch.from_numpy(E).cuda()
    return Epad[:, :H]


def _known_for(rng, queries, N, side, per=5):
    """Facts that complete the queries (a few each, some twice) and some that complete none of them."""
    a, r = np.repeat(queries[:, 0], per), np.repeat(queries[:, 1], per)
    c = rng.integers(0, N, len(a))
    rows = np.stack([a, r, c], 1) if side == "tail" else np.stack([c, r, a], 1)
    other = np.stack([rng.integers(0, N, 20), rng.integers(0, 2, 20), rng.integers(0, N, 20)], 1)
    return np.concatenate([rows, rows[::3], other]).astype(np.int64)


@pytest.mark.parametrize("N,H,nq,k", [(257, 7, 70, 10), (1000, 200, 33, 1), (4099, 64, 1, 256), (64, 5, 9, 64)])
@pytest.mark.parametrize("side", ["tail", "head"])
def test_topk_against_oracle_bit_exact(N, H, nq, k, side):
    from mrgcn_amd.tasks import link_prediction as lp
    P = 4
    rng, E, Rel = _table(N, H, P, N + k)
    queries = np.stack([rng.integers(0, N, nq), rng.integers(0, 2 * P + 1, nq)], 1).astype(np.int64)
    Ed, (Rd,) = _padded(E), _dev(Rel)
    _assert_same(lp.predict_topk(queries, Ed, Rd, k, side=side), _expected(E, Rel, queries, side, k))
    known = _known_for(rng, queries, N, side)
    lists = lp.known_lists(queries, known, side)
    assert lists[0][-1] > 0
    _assert_same(lp.predict_topk(queries, Ed, Rd, k, side=side, known=known),
                 _expected(E, Rel, queries, side, k, lists))


def test_padding_and_exclusion():
    from mrgcn_amd.tasks import link_prediction as lp
    N, H, nq, k = 40, 8, 5, 64
    rng, E, Rel = _table(N, H, 2, 1)
    queries = np.stack([rng.integers(0, N, nq), rng.integers(0, 5, nq)], 1).astype(np.int64)
    Ed, Rd = _dev(E, Rel)
    got = lp.predict_topk(queries, Ed, Rd, k)                         # k > N: 24 padded places per row
    _assert_same(got, _expected(E, Rel, queries, "tail", k))
    assert bool((got[0][:, N:] == -1).all()) and bool(torch.isinf(got[1][:, N:]).all()) and bool((got[0][:, :N] >= 0).all())
    # one query whose known list leaves 3 candidates, k = 10; one whose list holds the candidate that would be first
    q2 = queries[:2].copy()
    first = _expected(E, Rel, q2, "tail", 1)[0][:, 0]
    left = np.array([3, 17, 38])
    gone = np.setdiff1d(np.arange(N), left)
    known = np.concatenate([np.stack([np.full(len(gone), q2[0, 0]), np.full(len(gone), q2[0, 1]), gone], 1),
                            [[q2[1, 0], q2[1, 1], first[1]]]]).astype(np.int64)
    if (q2[0] == q2[1]).all():
        pytest.fail("the two queries must differ")
    lists = lp.known_lists(q2, known, "tail")
    got = lp.predict_topk(q2, Ed, Rd, 10, known=known)
    _assert_same(got, _expected(E, Rel, q2, "tail", 10, lists))
    gi = got[0].cpu().numpy()
    assert sorted(gi[0, :3].tolist()) == left.tolist() and (gi[0, 3:] == -1).all()
    assert first[1] not in gi[1] and (gi[1] >= 0).all()


def test_all_ties_keep_node_order():
    from mrgcn_amd.tasks import link_prediction as lp
    N, H, nq, k = 600, 12, 11, 256
    rng = np.random.default_rng(2)
    Rel = rng.standard_normal((5, H)).astype(np.float32)
    queries = np.stack([rng.integers(0, N, nq), rng.integers(0, 5, nq)], 1).astype(np.int64)
    E0 = np.zeros((N, H), np.float32)
    for side in ("tail", "head"):
        idx, sc = lp.predict_topk(queries, *_dev(E0, Rel), k, side=side)
        assert np.array_equal(idx.cpu().numpy(), np.tile(np.arange(k), (nq, 1)))
        assert bool((sc == 0).all())
    # products that are -0.0: a relation row of negative values against non-negative embeddings with zeros
    E = np.maximum(rng.standard_normal((N, H)), 0).astype(np.float32)
    E[rng.choice(N, N // 2, replace=False)] = 0
    Rel[1] = -np.abs(Rel[1]) - 1
    queries[:, 1] = 1
    queries[::2, 0] = np.flatnonzero((E == 0).all(1))[: len(queries[::2])]   # anchors of zeros: every product is -0.0
    assert np.signbit((E[queries[0, 0]] * Rel[1]).astype(np.float32) * E[5]).any()
    for side in ("tail", "head"):
        _assert_same(lp.predict_topk(queries, *_dev(E, Rel), k, side=side), _expected(E, Rel, queries, side, k))


def test_positions_agree_with_the_rank_kernel():
    from mrgcn_amd.tasks import link_prediction as lp
    N, H, nf = 200, 16, 50
    rng = np.random.default_rng(3)
    E = rng.standard_normal((N, H)).astype(np.float32)
    Rel = rng.standard_normal((7, H)).astype(np.float32)
    facts = np.stack([rng.integers(0, N, nf), rng.integers(0, 3, nf), rng.integers(0, N, nf)], 1).astype(np.int64)
    facts[nf // 2:, :2] = facts[: nf - nf // 2, :2]           # shared (s, p) pairs: the filter has something to remove
    Ed, Rd = _dev(E, Rel)
    queries = {"tail": facts[:, [0, 1]], "head": facts[:, [2, 1]]}
    answer = {"tail": facts[:, 2], "head": facts[:, 0]}
    for side in ("tail", "head"):                              # no two candidates of a query score the same
        sc = _scores(E, Rel, queries[side], side) + np.float32(0.0)
        assert all(len(np.unique(row)) == N for row in sc)
    tp, ti, hp, hi = lp.filter_lists(facts)                    # = known_lists(queries, facts) minus the fact's own answer
    for side in ("tail", "head"):
        own = lp.known_lists(queries[side], facts, side)
        fl = (tp, ti) if side == "tail" else (hp, hi)
        for f in range(nf):
            assert sorted(set(own[1][own[0][f]:own[0][f + 1]].tolist()) - {int(answer[side][f])}) == \
                fl[1][fl[0][f]:fl[0][f + 1]].tolist()
    for filtered in (False, True):
        ranks = lp.compute_ranks_fast(facts, Ed, Rd, filtered=filtered).cpu().numpy()
        for side, off in (("tail", 0), ("head", nf)):
            known = None
            if filtered:
                ptr, idx = (tp, ti) if side == "tail" else (hp, hi)
                known = (torch.from_numpy(ptr).cuda(), torch.from_numpy(idx).cuda())
            idx = lp.predict_topk(queries[side], Ed, Rd, N, side=side, known=known)[0].cpu().numpy()
            pos = np.array([int(np.flatnonzero(idx[f] == answer[side][f])[0]) + 1 for f in range(nf)])
            assert np.array_equal(pos, ranks[off:off + nf]), (filtered, side)


def test_reproducible_and_replayable():
    from mrgcn_amd.tasks import link_prediction as lp
    from mrgcn_amd.train import GraphedStep
    N, H, nq, k = 300, 16, 9, 10
    rng, E, Rel = _table(N, H, 3, 4)
    queries = np.stack([rng.integers(0, N, nq), rng.integers(0, 7, nq)], 1).astype(np.int64)
    known = _known_for(rng, queries, N, "tail")
    lists = lp.known_lists(queries, known, "tail")
    Ed, Rd, qd, ptr, idx = _dev(E, Rel, queries, *lists)
    a = lp.predict_topk(queries, Ed, Rd, k, known=known)
    b = lp.predict_topk(qd, Ed, Rd, k, known=(ptr, idx))
    want = _expected(E, Rel, queries, "tail", k, lists)
    _assert_same(a, want)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    step = GraphedStep(lambda: lp.predict_topk(qd, Ed, Rd, k, known=(ptr, idx)), warmup=1)
    for _ in range(2):
        out = step()
        _assert_same(out, want)
        assert torch.equal(out[0], a[0]) and torch.equal(out[1].view(torch.int32), a[1].view(torch.int32))
    E2 = np.roll(E, 7, axis=0) * np.float32(1.5)
    Ed.copy_(torch.from_numpy(E2).cuda())                      # the captured call reads the embeddings where they lie
    want2 = _expected(E2, Rel, queries, "tail", k, lists)
    assert not np.array_equal(want2[0], want[0])
    for _ in range(2):
        _assert_same(step(), want2)


def test_predict_links_on_a_masked_minibatch():
    from mrgcn_amd.tasks import link_prediction as lp
    from tests import test_gpu_lp_minibatch as mb
    g, A, N, R, plan = mb._graph()
    model = mb._model(g, "f32b2", N, R)
    batch, facts = mb._batches(g, A, plan, masked=True)[1]
    queries = np.unique(facts[:, [0, 1]], axis=0)
    k = min(5, len(batch.node_index))
    model.train()
    got = lp.predict_links(model, batch, queries, k, side="tail", known=facts)
    assert model.training is False
    assert all(p.grad is None for p in model.parameters())
    with torch.no_grad():
        E = lp._embed(model, batch)
    assert not E.requires_grad and E.shape[0] == len(batch.node_index)
    want = lp.predict_topk(queries, E, model.relations, k, side="tail", known=facts)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
    assert int(got[0].max()) < len(batch.node_index)           # batch-local ids
    _assert_same(got, _expected(E.cpu().numpy(), model.relations.detach().cpu().numpy(), queries, "tail", k,
                                lp.known_lists(queries, facts, "tail")))


def test_errors_leave_the_library_usable():
    from mrgcn_amd import _lib
    from mrgcn_amd.tasks import link_prediction as lp
    N, H = 50, 8
    rng, E, Rel = _table(N, H, 2, 6)
    Ed, Rd = _dev(E, Rel)
    queries = np.array([[1, 0], [7, 4]], np.int64)
    with pytest.raises(ValueError, match="256"):
        lp.predict_topk(queries, Ed, Rd, 257)
    with pytest.raises(ValueError, match="relation"):
        lp.predict_topk(np.array([[1, 5]]), Ed, Rd, 3)
    with pytest.raises(ValueError, match="node"):
        lp.predict_topk(np.array([[N, 0]]), Ed, Rd, 3)
    ptr, idx = _dev(*lp.known_lists(queries, np.array([[1, 0, 3]]), "tail"))
    for pair in ((ptr, None), (None, idx)):
        with pytest.raises(_lib.MrgcnError, match="both"):
            lp.predict_topk(queries, Ed, Rd, 3, known=pair)
    # the entry point's own checks (no launch happens): the limit is named, half a pair of lists is refused
    lib = _lib.load()
    (qd,) = _dev(queries)
    out_i, out_s = torch.empty((2, 3), dtype=torch.int64, device="cuda"), torch.empty((2, 3), device="cuda")
    ws = torch.empty(lib.mrgcn_distmult_topk_workspace(N, H, 2, 3), dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    call = lambda k, ep, ei: lib.mrgcn_distmult_topk(  # noqa: E731
        p(Ed), Ed.stride(0), N, p(Rd), Rd.stride(0), H, p(qd), 2, 0, p(ep), p(ei), k, p(ws), ws.numel(), p(out_i),
        p(out_s), None)
    assert call(257, None, None) != 0 and b"256" in lib.mrgcn_last_error()
    assert call(3, ptr, None) != 0 and b"both" in lib.mrgcn_last_error()
    assert call(3, None, None) == 0
    torch.cuda.synchronize()
    want = _expected(E, Rel, queries, "tail", 3)
    _assert_same((out_i, out_s), want)
    _assert_same(lp.predict_topk(queries, Ed, Rd, 3), want)
