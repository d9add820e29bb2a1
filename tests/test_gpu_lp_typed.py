"""Type-constrained link prediction on the device (csrc/lp_negatives.hip: mrgcn_negatives_draw_typed_i64;
csrc/lp_typed.hip: the typed ranks; csrc/distmult_topk.hip: the typed top-k) through `NegativeSampler(candidates=
TypedCandidates)`, `rank_typed` / `evaluate_typed` and `predict_topk(candidates=)`.

Bounds.  Everything here is exact.  The draw is integer arithmetic and equals the numpy mirror
(`host.negatives_draw(typed=...)`) bit for bit.  The candidate scores are the untyped kernels' float32 operations in
the same order (`host.distmult_candidate_scores` / `host.complex_candidate_scores` restate them), so ranks are compared
as integers and top-k scores as bits; the metrics are float64 sums in a fixed order rounded once.

600 nodes, 6 relations, declared lists of length 0, 1, 255, 256, 257 and 600 (a candidate tile is 256 positions),
relations with 1, 8 and 9 facts (a fact tile is 8 facts), widths 6 and 70 (the staged h tile is 64 wide; ComplEx at
70 has K = 35)."""
import numpy as np
import pytest
import torch

from tests.test_gpu_lp_negatives import _golden_problem

pytestmark = pytest.mark.gpu
N, R, SEED = 600, 6, 1509
SIDES = {0: "both", 1: "tail", 2: "head"}
ZERO, NEGZERO, DUP_A, DUP_B = 100, 102, 104, 106      # even nodes below 257: in relation 0's and 1's lists
_FIX: dict = {}


def _np(t):
    return t.detach().cpu().numpy()


def fixture600():
    """Declared lists (slot 2 p: tails, 2 p + 1: heads) and facts inside them:
       relation 0   tails 0 .. 599 (600)              heads 0 .. 256 (257)           9 facts
       relation 1   tails 0, 2, .., 510 (256)         heads 1, 3, .., 509 (255)      8 facts
       relation 2   tails [7] (1)                     heads 40 nodes                 1 fact
       relation 3   no candidates, no facts (0, 0)
       relation 4   300 nodes                         300 nodes                      20 facts
       relation 5   0 .. 599                          0 .. 599                       5 facts, (s, p) and (p, o) repeated"""
    if _FIX:
        return _FIX
    from mrgcn_amd.tasks import link_prediction as lp
    r = np.random.default_rng(600)
    lists = [np.arange(600), np.arange(257), np.arange(0, 512, 2), np.arange(1, 510, 2), np.array([7]),
             np.sort(r.choice(600, 40, replace=False)), np.zeros(0, np.int64), np.zeros(0, np.int64),
             np.sort(r.choice(600, 300, replace=False)), np.sort(r.choice(600, 300, replace=False)),
             np.arange(600), np.arange(600)]
    assert [len(a) for a in lists] == [600, 257, 256, 255, 1, 40, 0, 0, 300, 300, 600, 600]
    ptr = np.zeros(2 * R + 1, np.int64)
    np.cumsum([len(a) for a in lists], out=ptr[1:])
    types = lp.TypedCandidates(ptr, np.concatenate(lists).astype(np.int32), N, R)

    def draw(p, n):
        return np.stack([r.choice(lists[2 * p + 1], n), np.full(n, p), r.choice(lists[2 * p], n)], 1)
    facts = np.concatenate([
        draw(0, 5), [(3, 0, ZERO), (3, 0, DUP_A), (4, 0, 599), (256, 0, 0)],            # 9 facts, tails that tie
        draw(1, 6), [(1, 1, ZERO), (509, 1, DUP_B)],                                    # 8 facts
        [(int(lists[5][0]), 2, 7)],                                                     # 1 fact
        draw(4, 20),
        [(10, 5, 20), (10, 5, 21), (10, 5, 22), (11, 5, 20), (599, 5, 599)]]).astype(np.int64)
    assert np.bincount(facts[:, 1], minlength=R).tolist() == [9, 8, 1, 0, 20, 5]
    facts = facts[r.permutation(len(facts))]
    _FIX.update(types=types, facts=facts, lists=lists)
    return _FIX


def embeddings(H, seed=7):
    """Rows with ties: a zero row and a row of negative zeros (scores +0 / -0 products: equal), two equal rows."""
    r = np.random.default_rng(seed + H)
    E = r.standard_normal((N, H)).astype(np.float32)
    Rel = r.standard_normal((R, H)).astype(np.float32)
    E[ZERO] = 0.0
    E[NEGZERO] = -0.0
    E[DUP_B] = E[DUP_A]
    E[22] = E[21]
    return E, Rel


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


# ---- 1. negatives -----------------------------------------------------------------------------------------------------
def _mirror(smp, position, seed):
    from mrgcn_amd import host
    keys = None if smp.keys is None else _np(smp.keys).astype(np.uint64)
    return host.negatives_draw(_np(smp.facts), smp.rate, smp.num_nodes, smp.num_nodes, smp.num_relations, keys, seed,
                               position, side=smp.side, typed=(smp.typed.ptr_host, smp.typed.idx_host))


def _check(smp, position, seed):
    want, flags = _mirror(smp, position, seed)
    assert np.array_equal(_np(smp.buf[smp.n:]), want)
    assert np.array_equal(_np(smp.unresolved), flags)
    return want, flags


@pytest.mark.parametrize("filtered", [True, False], ids=["filtered", "unfiltered"])
@pytest.mark.parametrize("side", [0, 1, 2], ids=["both", "tail", "head"])
@pytest.mark.parametrize("rate", [1, 3])
def test_typed_draw_equals_the_mirror(rate, side, filtered):
    import mrgcn_amd
    from mrgcn_amd.tasks import link_prediction as lp
    fx = fixture600()
    facts, types = fx["facts"], fx["types"]
    mrgcn_amd.reset_stats()
    smp = lp.NegativeSampler(facts, N, R, rate=rate, known=facts if filtered else False, candidates=types,
                             side=SIDES[side], seed=SEED)
    src = np.repeat(facts, rate, axis=0)
    for position in (0, 1):
        triples, labels = smp()
        assert triples is smp.buf and labels is smp.labels and np.array_equal(_np(triples[:smp.n]), facts)
        want, flags = _check(smp, position, SEED)
        head = want[:, 0] != src[:, 0]
        assert types.contains(2 * want[:, 1] + head, np.where(head, want[:, 0], want[:, 2])).all()
        single = (src[:, 1] == 2) & ~head                   # relation 2's only tail is the fact's own
        assert flags[single].all() and (single.any() or side != 1)
        if not filtered:
            assert np.array_equal(flags.astype(bool), single)
    st = mrgcn_amd.stats()
    assert st.get("lp.negatives.typed", 0) == 2 and st.get("lp.negatives.keyed", 0) == 0


@pytest.mark.parametrize("side", [0, 1, 2], ids=["both", "tail", "head"])
def test_typed_draw_with_full_lists_equals_the_untyped_sampler(side):
    from mrgcn_amd.tasks import link_prediction as lp
    facts = fixture600()["facts"]
    full = lp.TypedCandidates.full(N, R)
    for rate, known in ((1, facts), (3, False)):
        typed = lp.NegativeSampler(facts, N, R, rate=rate, known=known, candidates=full, side=SIDES[side], seed=SEED)
        plain = lp.NegativeSampler(facts, N, R, rate=rate, known=known, side=SIDES[side], seed=SEED)
        for _ in range(2):
            typed()
            plain()
            assert torch.equal(typed.buf, plain.buf) and torch.equal(typed.unresolved, plain.unresolved)


def test_typed_draw_under_capture_replays_consecutive_positions():
    from mrgcn_amd.tasks import link_prediction as lp
    from mrgcn_amd.train import capture_without_gc
    fx = fixture600()
    smp = lp.NegativeSampler(torch.from_numpy(fx["facts"]).cuda(), N, R, rate=3, known=fx["facts"],
                             candidates=fx["types"], seed=SEED)
    a, b = smp(), smp()
    assert a[0] is b[0] is smp.buf and a[1] is b[1] is smp.labels
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with capture_without_gc(), torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
        smp()
    torch.cuda.synchronize()
    p = int(smp.state[1])
    assert p == 2
    draws = []
    for r in range(2):
        graph.replay()
        torch.cuda.synchronize()
        draws.append(_check(smp, p + r, SEED)[0])
        assert int(smp.state[1]) == p + r + 1
    assert not np.array_equal(draws[0], draws[1])


# ---- 2. ranks ---------------------------------------------------------------------------------------------------------
CASES = [("distmult", 6), ("distmult", 70), ("complex", 6), ("complex", 70)]
_MIRROR: dict = {}


def mirror_ranks(scorer, H):
    """host.typed_ranks of the fixture, computed once per (scorer, width)."""
    if (scorer, H) not in _MIRROR:
        from mrgcn_amd import host
        fx = fixture600()
        E, Rel = embeddings(H)
        _MIRROR[scorer, H] = host.typed_ranks(fx["facts"], (fx["types"].ptr_host, fx["types"].idx_host), E, Rel,
                                              scorer=scorer)
    return _MIRROR[scorer, H]


@pytest.mark.parametrize("scorer,H", CASES)
def test_typed_ranks_equal_the_mirror(scorer, H):
    import mrgcn_amd
    from mrgcn_amd.tasks import link_prediction as lp
    fx = fixture600()
    E, Rel = embeddings(H)
    Ed, Rd = _dev(E, Rel)
    tf = lp.TypedFacts(fx["facts"], fx["types"])
    mrgcn_amd.reset_stats()
    raw, flt = lp.rank_typed(tf, Ed, Rd, scorer=scorer)
    assert raw.dtype == flt.dtype == torch.int64 and raw.shape == flt.shape == (2 * len(fx["facts"]),)
    want_raw, want_flt = mirror_ranks(scorer, H)
    assert np.array_equal(_np(raw), want_raw)
    assert np.array_equal(_np(flt), want_flt)
    assert (want_flt < want_raw).any()                      # the filter does something
    again = lp.rank_typed(tf, Ed, Rd, scorer=scorer)        # the same tensors: nothing is allocated again
    assert again[0] is raw and again[1] is flt and np.array_equal(_np(raw), want_raw)
    assert mrgcn_amd.stats().get("lp.rank.typed", 0) == 2
    # unfiltered facts: raw ranks only
    raw_only, none = lp.rank_typed(lp.TypedFacts(fx["facts"], fx["types"], filtered=False), Ed, Rd, scorer=scorer)
    assert none is None and np.array_equal(_np(raw_only), want_raw)
    # `known` beyond the facts: the mirror with the same triples
    from mrgcn_amd import host
    sub = fx["facts"][::2]
    raw_s, flt_s = lp.rank_typed(lp.TypedFacts(sub, fx["types"], known=fx["facts"]), Ed, Rd, scorer=scorer)
    w_raw, w_flt = host.typed_ranks(sub, (fx["types"].ptr_host, fx["types"].idx_host), E, Rel, known=fx["facts"],
                                    scorer=scorer)
    assert np.array_equal(_np(raw_s), w_raw) and np.array_equal(_np(flt_s), w_flt)


@pytest.mark.parametrize("scorer,H", CASES)
def test_typed_ranks_with_full_lists_equal_rank_both_and_bound_the_typed_ones(scorer, H):
    from mrgcn_amd.tasks import link_prediction as lp
    fx = fixture600()
    facts = fx["facts"]
    assert len(facts) <= N                                  # rank_both scores every fact of such a call
    Ed, Rd = _dev(*embeddings(H))
    lists = [torch.from_numpy(a).cuda() for a in lp.filter_lists(facts)]
    raw_u, flt_u = lp.rank_both(facts, Ed, Rd, lists, scorer=scorer)
    raw_f, flt_f = lp.rank_typed(lp.TypedFacts(facts, lp.TypedCandidates.full(N, R)), Ed, Rd, scorer=scorer)
    assert torch.equal(raw_f, raw_u) and torch.equal(flt_f, flt_u)
    raw_t, flt_t = lp.rank_typed(lp.TypedFacts(facts, fx["types"]), Ed, Rd, scorer=scorer)
    assert bool((raw_t <= raw_u).all()) and bool((flt_t <= flt_u).all()) and bool((raw_t < raw_u).any())


def test_typed_ranks_under_capture():
    from mrgcn_amd.tasks import link_prediction as lp
    from mrgcn_amd.train import capture_without_gc
    fx = fixture600()
    Ed, Rd = _dev(*embeddings(70))
    tf = lp.TypedFacts(fx["facts"], fx["types"], mrr_batchsize=10)
    out = torch.zeros(8, device="cuda")
    score = torch.zeros((), device="cuda")
    lp.evaluate_typed(Ed, Rd, tf, out=out, score=score)     # the first call allocates
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with capture_without_gc(), torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
        got, raw, flt = lp.evaluate_typed(Ed, Rd, tf, out=out, score=score, want_ranks=True)
    want_raw, want_flt = mirror_ranks("distmult", 70)
    first = out.clone()
    for _ in range(2):
        raw.zero_()
        flt.zero_()
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_np(raw), want_raw) and np.array_equal(_np(flt), want_flt)
        assert torch.equal(out, first) and got is out


@pytest.mark.parametrize("scorer,H", [("distmult", 70), ("complex", 6)])
def test_evaluate_typed_equals_rank_metrics_of_the_mirror(scorer, H):
    from mrgcn_amd.tasks import link_prediction as lp
    fx = fixture600()
    Ed, Rd = _dev(*embeddings(H))
    want_raw, want_flt = mirror_ranks(scorer, H)
    for batchsize in (None, 10):
        tf = lp.TypedFacts(fx["facts"], fx["types"], mrr_batchsize=batchsize)
        assert tf.nparts == (1 if batchsize is None else len(fx["facts"]) // 10)
        score = torch.zeros((), device="cuda")
        out, raw, flt = lp.evaluate_typed(Ed, Rd, tf, score=score, want_ranks=True, scorer=scorer)
        want = torch.cat([lp.rank_metrics(torch.from_numpy(want_raw).cuda(), tf.part_ptr),
                          lp.rank_metrics(torch.from_numpy(want_flt).cuda(), tf.part_ptr)])
        assert _np(out).tobytes() == _np(want).tobytes()
        assert abs(float(score) - (1.0 - float(out[0]))) < 1e-6       # 1 - mrr, rounded from the float64 sum
        assert 0 < float(out[0]) <= float(out[4]) <= 1
        bare = lp.evaluate_typed(Ed, Rd, lp.TypedFacts(fx["facts"], fx["types"], filtered=False,
                                                       mrr_batchsize=batchsize), scorer=scorer)
        assert _np(bare[4:]).tolist() == [-1.0] * 4 and torch.equal(bare[:4], out[:4])


# ---- 3. top-k ---------------------------------------------------------------------------------------------------------
def _queries():
    """Mixed relations in no order: every list length, an empty list (relation 3), anchors with tied candidates."""
    r = np.random.default_rng(11)
    q = np.stack([r.integers(0, N, 21), np.tile([4, 0, 5, 1, 3, 2, 0], 3)], 1)
    q[1] = (3, 0)
    q[2] = (10, 5)
    return q.astype(np.int64)


def _mirror_topk(q, k, side, scorer, H, types, known=None):
    from mrgcn_amd import host
    from mrgcn_amd.tasks import link_prediction as lp
    E, Rel = embeddings(H)
    fn = host.complex_candidate_scores if scorer == "complex" else host.distmult_candidate_scores
    sc = fn(E, Rel, q[:, 0], q[:, 1], side)
    idx = np.full((len(q), k), -1, np.int64)
    val = np.full((len(q), k), -np.inf, np.float32)
    excl = lp.known_lists(q, known, side) if known is not None else None
    for i, (a, p) in enumerate(q.tolist()):
        cand = types.slot(p, side).astype(np.int64)
        if excl is not None:
            cand = cand[~np.isin(cand, excl[1][excl[0][i]:excl[0][i + 1]])]
        s = sc[i, cand] + np.float32(0.0)                   # (-0 counts as +0)
        top = np.argsort(-s, kind="stable")[:k]             # ties: the list rises, so the lower node id first
        idx[i, :len(top)] = cand[top]
        val[i, :len(top)] = sc[i, cand[top]]
    return idx, val


@pytest.mark.parametrize("side", ["tail", "head"])
@pytest.mark.parametrize("scorer,H", [("distmult", 70), ("complex", 6)])
def test_typed_topk_equals_a_stable_sort_of_the_mirror_scores(scorer, H, side):
    import mrgcn_amd
    from mrgcn_amd.tasks import link_prediction as lp
    fx = fixture600()
    Ed, Rd = _dev(*embeddings(H))
    q = _queries()
    mrgcn_amd.reset_stats()
    for k in (1, 10, 256):                                  # 10 > the list of 1; 256 > the lists of 1, 40 and 255
        idx, val = lp.predict_topk(q, Ed, Rd, k, side=side, scorer=scorer, candidates=fx["types"])
        w_idx, w_val = _mirror_topk(q, k, side, scorer, H, fx["types"])
        assert np.array_equal(_np(idx), w_idx)
        got = _np(val)
        assert np.array_equal(got == -np.inf, w_idx < 0)
        assert np.array_equal(np.where(w_idx >= 0, got, 0) + np.float32(0), np.where(w_idx >= 0, w_val, 0) + np.float32(0))
        assert (w_idx[q[:, 1] == 3] == -1).all()            # an empty list: nothing to propose
    assert mrgcn_amd.stats().get("lp.topk.typed", 0) == 3


@pytest.mark.parametrize("scorer,H", [("distmult", 6), ("complex", 70)])
def test_typed_topk_scores_are_the_untyped_scores_of_the_same_pairs(scorer, H):
    """The untyped call with every node OUTSIDE the query's list excluded has the typed call's candidates: the two
    results are equal, indices and score bits."""
    from mrgcn_amd.tasks import link_prediction as lp
    fx = fixture600()
    Ed, Rd = _dev(*embeddings(H))
    q = _queries()
    for side in ("tail", "head"):
        outside = [np.setdiff1d(np.arange(N), fx["types"].slot(p, side)).astype(np.int32) for p in q[:, 1]]
        ptr = np.zeros(len(q) + 1, np.int64)
        np.cumsum([len(a) for a in outside], out=ptr[1:])
        excl = tuple(_dev(ptr, np.concatenate(outside)))
        qd = torch.from_numpy(q).cuda()
        for k in (10, 256):
            u_idx, u_val = lp.predict_topk(qd, Ed, Rd, k, side=side, known=excl, scorer=scorer)
            t_idx, t_val = lp.predict_topk(qd, Ed, Rd, k, side=side, scorer=scorer, candidates=fx["types"])
            assert torch.equal(t_idx, u_idx)
            assert _np(t_val).tobytes() == _np(u_val).tobytes()


def test_typed_topk_exclusions_full_lists_and_prepared_queries():
    from mrgcn_amd.tasks import link_prediction as lp
    fx = fixture600()
    facts, types = fx["facts"], fx["types"]
    Ed, Rd = _dev(*embeddings(70))
    q = np.concatenate([facts[:, [0, 1]], _queries()])
    for side, q_ in (("tail", q), ("head", np.concatenate([facts[:, [2, 1]], _queries()]))):
        idx, val = lp.predict_topk(q_, Ed, Rd, 10, side=side, known=facts, candidates=types)
        w_idx, _ = _mirror_topk(q_, 10, side, "distmult", 70, types, known=facts)
        assert np.array_equal(_np(idx), w_idx)
        ans = facts[:, 0 if side == "head" else 2]
        assert not (_np(idx)[:len(facts)] == ans[:, None]).any()     # a fact's own completion is known: excluded
        if side == "tail":      # relation 2's only tail is its fact's: nothing is left to propose
            bare, _ = lp.predict_topk(q_, Ed, Rd, 10, side=side, candidates=types)
            row = int(np.flatnonzero(facts[:, 1] == 2)[0])
            assert _np(bare)[row].tolist() == [7] + [-1] * 9 and _np(idx)[row].tolist() == [-1] * 10
        # a TypedQueries built beforehand: the same call without host work, rows in the caller's order
        tq = lp.TypedQueries(torch.from_numpy(q_).cuda(), types, side=side, known=facts)
        idx2, val2 = lp.predict_topk(tq, Ed, Rd, 10, side=side)
        with pytest.raises(ValueError):
            lp.predict_topk(tq, Ed, Rd, 10, side="head" if side == "tail" else "tail")
        assert torch.equal(idx2, idx) and _np(val2).tobytes() == _np(val).tobytes()
        # every list 0 .. N - 1: the untyped result
        full = lp.TypedCandidates.full(N, R)
        for k in (1, 256):
            f_idx, f_val = lp.predict_topk(q_, Ed, Rd, k, side=side, known=facts, candidates=full)
            u_idx, u_val = lp.predict_topk(q_, Ed, Rd, k, side=side, known=facts)
            assert torch.equal(f_idx, u_idx) and _np(f_val).tobytes() == _np(u_val).tobytes()
    # one relation per call gives the rows the mixed call returned for it
    only0 = q[q[:, 1] == 0]
    a, _ = lp.predict_topk(only0, Ed, Rd, 10, candidates=types, known=facts)
    b, _ = lp.predict_topk(q, Ed, Rd, 10, candidates=types, known=facts)
    assert torch.equal(a, b[torch.from_numpy(q[:, 1] == 0).cuda()])


# ---- 4. end to end ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decoder", ["triples", "grouped"])
def test_train_steps_with_a_typed_sampler(decoder):
    import mrgcn_amd
    from mrgcn_amd.tasks import link_prediction as lp
    model, opt, A, _, facts, nn_, nr = _golden_problem()
    types = lp.TypedCandidates.from_facts(facts, nn_, nr)
    smp = lp.NegativeSampler(facts, nn_, nr, rate=3, known=facts, candidates=types, seed=SEED)
    model.train()
    mrgcn_amd.reset_stats()
    losses = [float(lp.train_step(model, lambda: model(None, A), smp, opt, decoder=decoder)) for _ in range(4)]
    print(decoder, "losses", losses, "unresolved", smp.num_unresolved())
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]      # (falls, as the untyped samplers' runs are held to)
    st = mrgcn_amd.stats()
    assert st.get("lp.negatives.typed", 0) == 4 and st.get("lp.negatives.keyed", 0) == 0
    neg = _np(smp.buf[smp.n:])
    src = np.repeat(facts, 3, axis=0)
    head = neg[:, 0] != src[:, 0]
    assert types.contains(2 * neg[:, 1] + head, np.where(head, neg[:, 0], neg[:, 2])).all()
