"""The ComplEx scorer on the device (csrc/complex.hip, lp_score.hpp: lp_stage<kLpComplEx>; tasks/link_prediction.py:
score_complex_bc and the `scorer="complex"` keyword).

Bounds.  Candidate scores (top-k, ranks) are the bits of `mrgcn_amd.host.complex_candidate_scores`, so top-k lists and
ranks are exact.  Flat scores and gradients are held to float64 (`complex_scores64`, the gradient formulas as float64
numpy) by the bounds tests/test_gpu_lp.py holds DistMult to on the same input scale: scores rtol 1e-4 / atol 1e-4, dE
and dRel rtol 1e-3 / atol 1e-6 through the mean BCE — a ComplEx element is the same kind of sum with two products
where DistMult has one.  Steps, losses and replayed rows are bitwise under torch.use_deterministic_algorithms(True).
Embeddings are 0.5 N(0, 1) as in the existing decoder tests."""
import numpy as np
import pytest
import torch

from mrgcn_amd import host
from tests.test_cpu_lp_complex import complex_grads64, tables, triples
from tests.test_gpu_lp_fit import NTRAIN, N_, P_, _fwd, _model, _small, deterministic

pytestmark = pytest.mark.gpu

SHAPES = [(300, 5, 200), (300, 5, 130), (64, 7, 64), (64, 7, 6)]


def _np(t):
    return t.detach().cpu().numpy()


def _dev(E, Rel, pad=0):
    """Device copies; `pad`: rows of E with a stride of H + pad."""
    Ed = torch.zeros((E.shape[0], E.shape[1] + pad), device="cuda")
    Ed[:, :E.shape[1]] = torch.from_numpy(E).cuda()
    return Ed[:, :E.shape[1]], torch.from_numpy(Rel).cuda()


# ---- 1. candidate scores are the mirror's bits (through predict_topk) ------------------------------------------------
def _topk_want(scores, excluded, k):
    """Rows (idx, score) by (score descending, id ascending) over the candidates not excluded, padded with (-1, -inf)."""
    nq, N = scores.shape
    idx = np.full((nq, k), -1, np.int64)
    sc = np.full((nq, k), -np.inf, np.float32)
    for q in range(nq):
        live = np.setdiff1d(np.arange(N), excluded[q])
        s = scores[q, live] + np.float32(0)   # (-0 counts as +0)
        order = np.lexsort((live, -s.astype(np.float64)))[:k]
        idx[q, :len(order)] = live[order]
        sc[q, :len(order)] = s[order]
    return idx, sc


def _topk_case(N, R, H, side, nq=21):
    E, Rel = tables(N, R, H, seed=N + H)
    rng = np.random.default_rng(H)
    q = np.stack([rng.integers(0, N, nq), rng.integers(0, R, nq)], 1).astype(np.int64)
    known = np.stack([np.repeat(q[:, 0], 3), np.repeat(q[:, 1], 3), rng.integers(0, N, 3 * nq)], 1)
    if side == "head":
        known = known[:, ::-1].copy()
    known = known[: 3 * (nq - 4)]   # the last queries exclude nothing
    return E, Rel, q, known


@pytest.mark.parametrize("side", ["tail", "head"])
@pytest.mark.parametrize("N,R,H", SHAPES)
def test_topk_returns_the_mirrors_scores_in_the_mirrors_order(N, R, H, side):
    from mrgcn_amd.tasks import link_prediction as lp
    E, Rel, q, known = _topk_case(N, R, H, side)
    Ed, Rd = _dev(E, Rel, pad=3)
    scores = host.complex_candidate_scores(E, Rel, q[:, 0], q[:, 1], side)
    ptr, lst = lp.known_lists(q, known, side)
    excluded = [lst[ptr[i]:ptr[i + 1]] for i in range(len(q))]
    assert sum(len(e) for e in excluded) > 0 and len(excluded[-1]) == 0
    ks = [min(N, 256)] + ([1, 10] if (N, H) == (300, 200) else []) + ([100] if (N, H) == (64, 64) else [])
    for k in ks:
        idx, sc = lp.predict_topk(q, Ed, Rd, k, side=side, known=known, scorer="complex")
        want_idx, want_sc = _topk_want(scores, excluded, k)
        assert np.array_equal(_np(idx), want_idx), k
        assert _np(sc).tobytes() == want_sc.tobytes(), k
        if k > N:   # fewer than k candidates: the row ends in (-1, -inf)
            assert np.all(_np(idx)[:, N:] == -1) and np.all(np.isneginf(_np(sc)[:, N:]))
            assert np.all(_np(idx)[0, : N - len(excluded[0])] >= 0) and _np(idx)[0, N - len(excluded[0])] == -1
    # the same call without exclusions, against DistMult's: another scoring function altogether
    idx_c, _ = lp.predict_topk(q, Ed, Rd, 5, side=side, scorer="complex")
    idx_d, _ = lp.predict_topk(q, Ed, Rd, 5, side=side)
    assert not torch.equal(idx_c, idx_d)


def test_topk_replays_in_a_captured_graph_with_equal_bits():
    from mrgcn_amd.tasks import link_prediction as lp
    N, R, H = SHAPES[1]
    E, Rel, q, known = _topk_case(N, R, H, "head")
    Ed, Rd = _dev(E, Rel)
    ptr, lst = (torch.from_numpy(a).cuda() for a in lp.known_lists(q, known, "head"))
    qd = torch.from_numpy(q).cuda()
    want = lp.predict_topk(qd, Ed, Rd, 10, side="head", known=(ptr, lst), scorer="complex")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        got = lp.predict_topk(qd, Ed, Rd, 10, side="head", known=(ptr, lst), scorer="complex")
    for _ in range(2):
        got[0].zero_()
        got[1].zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]) and _np(got[1]).tobytes() == _np(want[1]).tobytes()


# ---- 2. ranks are the mirror's, exactly ------------------------------------------------------------------------------
def _rank_of(gt, eq):
    m = eq - 1
    half = m // 2
    if m % 2 and half % 2:
        half += 1
    return gt + half + 1


def _want_ranks(facts, E, Rel, ptr):
    """(raw, flt) [2 nf] by the documented rule from mirror scores: greater + half-even ties + 1, the filter of each
    part's own facts from `filter_lists`, a fact at a position >= N of its part scored as all zeros (all ties)."""
    from mrgcn_amd.tasks import link_prediction as lp
    nf, N = len(facts), E.shape[0]
    sides = (host.complex_candidate_scores(E, Rel, facts[:, 0], facts[:, 1], "tail"),
             host.complex_candidate_scores(E, Rel, facts[:, 2], facts[:, 1], "head"))
    raw, flt = np.zeros(2 * nf, np.int64), np.zeros(2 * nf, np.int64)
    for p in range(len(ptr) - 1):
        a, b = int(ptr[p]), int(ptr[p + 1])
        tp, ti, hp, hi = lp.filter_lists(facts[a:b])
        for f in range(a, b):
            for d, (lp_, li_, ans) in enumerate(((tp, ti, facts[f, 2]), (hp, hi, facts[f, 0]))):
                scored = f - a < N
                sc = sides[d][f] if scored else np.zeros(N, np.float32)
                true = sc[ans]
                keep = np.ones(N, bool)
                keep[li_[lp_[f - a]:lp_[f - a + 1]]] = False
                assert keep[ans]
                raw[d * nf + f] = _rank_of(int((sc > true).sum()), int((sc == true).sum()))
                flt[d * nf + f] = _rank_of(int((sc[keep] > true).sum()), int((sc[keep] == true).sum()))
    return raw, flt


def _rank_facts(N, R, nf, seed):
    t = triples(N, R, nf, seed)
    t[nf // 2:, 0] = t[: nf - nf // 2, 0]   # shared (s, p) pairs for the filter
    t[nf // 2:, 1] = t[: nf - nf // 2, 1]
    return t


@pytest.mark.parametrize("N,R,H,nf,part", [(300, 5, 200, 2500, 0), (300, 5, 130, 701, 100), (64, 7, 64, 150, 0),
                                           (64, 7, 6, 150, 37)])
def test_ranks_are_the_mirrors(N, R, H, nf, part):
    from mrgcn_amd.tasks import link_prediction as lp
    E, Rel = tables(N, R, H, seed=nf)
    facts = _rank_facts(N, R, nf, seed=H)
    Ed, Rd = _dev(E, Rel, pad=3 if H != 130 else 0)
    parts = lp.FactParts(facts, part, device="cuda")
    ptr = parts.part_ptr_host
    assert nf % 8 and all(int(s) % 8 for s in np.diff(ptr)) and (part == 0) == (parts.nparts == 1)
    want_raw, want_flt = _want_ranks(facts, E, Rel, ptr)
    unscored = sum(max(int(s) - N, 0) for s in np.diff(ptr))
    print(f"{(N, R, H, nf)}: {parts.nparts} parts, {unscored} unscored facts, raw and filtered ranks differ in "
          f"{int((want_raw != want_flt).sum())} of {2 * nf}")
    # (the mirror's own figures: 4296, 41, 137 and 6 — a kernel that ignores the lists cannot pass)
    assert int((want_raw != want_flt).sum()) >= 5 and (unscored > 0) == (part == 0)
    for slice_facts in (0, 16):
        raw, flt = lp.rank_both(parts, Ed, Rd, slice_facts=slice_facts, scorer="complex")
        assert np.array_equal(_np(raw), want_raw), slice_facts
        assert np.array_equal(_np(flt), want_flt), slice_facts
    raw_only, none = lp.rank_both(facts, Ed, Rd, part_ptr=parts.part_ptr, scorer="complex")
    assert none is None and np.array_equal(_np(raw_only), want_raw)
    if parts.nparts == 1:
        assert np.array_equal(_np(lp.compute_ranks_fast(facts, Ed, Rd, filtered=False, scorer="complex")), want_raw)
        assert np.array_equal(_np(lp.compute_ranks_fast(facts, Ed, Rd, filtered=True, scorer="complex")), want_flt)
    # DistMult's ranks of the same inputs are another matter (and stay what they were: the existing tests)
    assert not np.array_equal(_np(lp.rank_both(parts, Ed, Rd)[0]), want_raw)


def test_ranks_with_constructed_exact_ties_on_both_sides():
    """Three rows of E copied onto three others: the copies tie exactly with the originals as candidates, on both
    sides.  With ONE truth per fact (the tail form's, say) the head side's own answer would no longer tie with itself
    where the two forms differ in their last bits, and these ranks would be off."""
    from mrgcn_amd.tasks import link_prediction as lp
    N, R, H = 64, 7, 64
    E, Rel = tables(N, R, H, seed=9)
    E[[40, 41, 42]] = E[[3, 4, 5]]
    facts = _rank_facts(N, R, 61, seed=2)
    facts[:20, 2] = np.resize([3, 4, 5, 40], 20)     # true tails with a twin
    facts[20:40, 0] = np.resize([41, 5, 3, 42], 20)  # true heads with a twin
    want_raw, want_flt = _want_ranks(facts, E, Rel, np.array([0, 61]))
    tail = host.complex_candidate_scores(E, Rel, facts[:, 0], facts[:, 1], "tail")[np.arange(61), facts[:, 2]]
    head = host.complex_candidate_scores(E, Rel, facts[:, 2], facts[:, 1], "head")[np.arange(61), facts[:, 0]]
    assert np.mean(tail != head) > 0.5   # (the case bites: one truth per fact cannot serve both sides)
    Ed, Rd = _dev(E, Rel)
    lists = [torch.from_numpy(a).cuda() for a in lp.filter_lists(facts)]
    raw, flt = lp.rank_both(facts, Ed, Rd, lists, scorer="complex")
    assert np.array_equal(_np(raw), want_raw) and np.array_equal(_np(flt), want_flt)


# ---- 3. flat scores and gradients against float64 ---------------------------------------------------------------------
_WORST = {"scores": 0.0, "dE": 0.0, "dRel": 0.0}


def _used(got, want, rtol, atol):
    """The largest share of the bound |got - want| <= atol + rtol |want| in use."""
    return float(np.max(np.abs(got.astype(np.float64) - want) / (atol + rtol * np.abs(want))))


def _flat_check(N, R, H, t, n_static=0, needs=(True, True), pad=0, tag=""):
    from mrgcn_amd.tasks import link_prediction as lp
    E, Rel = tables(N, R, H, seed=7)
    Ed, Rd = _dev(E, Rel, pad)
    Ed = Ed.detach().requires_grad_(needs[0])
    Rd = Rd.detach().requires_grad_(needs[1])
    td = torch.from_numpy(t).cuda()
    static = lp.SortedTriples(td[:n_static].contiguous(), N, R) if n_static else None
    labels = np.zeros(len(t), np.float32)
    labels[: max(n_static, len(t) // 2)] = 1
    scores = lp.score_complex_bc(td, Ed, Rd, static=static)
    lp.binary_crossentropy(scores, torch.from_numpy(labels).cuda()).backward()
    want = host.complex_scores64(t, E, Rel)
    g = (1.0 / (1.0 + np.exp(-want)) - labels) / len(t)
    dE, dR = complex_grads64(t, E, Rel, g)
    used = {"scores": _used(_np(scores), want, 1e-4, 1e-4)}
    if needs[0]:
        used["dE"] = _used(_np(Ed.grad), dE, 1e-3, 1e-6)
    else:
        assert Ed.grad is None
    if needs[1]:
        used["dRel"] = _used(_np(Rd.grad), dR, 1e-3, 1e-6)
    else:
        assert Rd.grad is None
    for k, v in used.items():
        _WORST[k] = max(_WORST[k], v)
    print(f"complex flat {tag or (N, R, H, len(t), n_static)}: share of the bound in use {used}; worst so far {_WORST}")
    assert all(v <= 1.0 for v in used.values()), used


def _long_set():
    """The long-run set of tests/test_gpu_lp_grouped.py: 3 000 facts of one predicate, 400 of one subject."""
    rng = np.random.default_rng(200)
    f = np.stack([rng.integers(0, 500, 9000), rng.integers(0, 9, 9000), rng.integers(0, 500, 9000)], 1).astype(np.int64)
    f[:3000, 1] = 2
    f[3000:3400, 0] = 7
    return f


@pytest.mark.parametrize("N,R,H", SHAPES)
def test_flat_scores_and_gradients_without_static(N, R, H):
    t = triples(N, R, 1500, seed=H)
    t[:40, 2] = t[:40, 0]          # s == o
    t[40:80] = t[80:120]           # repeated triples
    _flat_check(N, R, H, t, pad=0 if H % 4 else 3)
    _flat_check(N, R, H, t[:31])   # less than one wave's span


@pytest.mark.parametrize("n_neg", [0, 50, 5000])
def test_flat_scores_and_gradients_with_static_and_negatives_behind_it(n_neg):
    N, R, H = 300, 5, 200
    t = np.concatenate([triples(N, R, 1100, seed=1), triples(N, R, n_neg, seed=2)])
    t[:30, 2] = t[:30, 0]
    _flat_check(N, R, H, t, n_static=1100)


def test_flat_scores_and_gradients_on_the_long_run_set():
    t = _long_set()
    _flat_check(500, 9, 64, t, tag="long9000")
    _flat_check(500, 9, 64, t, n_static=9000, tag="long9000 static")
    neg, _ = host.negatives_draw(t, 1, 500, 500, 9, False, 77, 0)
    _flat_check(500, 9, 64, np.concatenate([t, neg]), n_static=9000, tag="long9000 static + 9000 negatives")


@pytest.mark.parametrize("needs", [(True, False), (False, True)])
def test_flat_gradient_for_one_input_only(needs):
    _flat_check(64, 7, 64, triples(64, 7, 700, seed=4), needs=needs)
    _flat_check(64, 7, 6, triples(64, 7, 700, seed=4), n_static=500, needs=needs)


# ---- 4. determinism ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_static", [0, 9000])
def test_backward_gives_equal_bits_under_the_flag_and_counts(n_static):
    import mrgcn_amd
    from mrgcn_amd.tasks import link_prediction as lp
    N, R, H = 500, 9, 64
    t = _long_set()
    neg, _ = host.negatives_draw(t, 1, 500, 500, 9, False, 77, 0)
    td = torch.from_numpy(np.concatenate([t, neg])).cuda()
    static = lp.SortedTriples(td[:n_static].contiguous(), N, R) if n_static else None
    E, Rel = tables(N, R, H, seed=7)
    g = torch.from_numpy(np.random.default_rng(1).standard_normal(len(td)).astype(np.float32)).cuda()

    def grads():
        Ed, Rd = (x.detach().requires_grad_() for x in _dev(E, Rel))
        s = lp.score_complex_bc(td, Ed, Rd, static=static)
        s.backward(g)
        return s.detach(), Ed.grad, Rd.grad
    plain = [grads(), grads()]
    assert torch.equal(plain[0][0], plain[1][0])   # the forward is a pure function, flag or not
    mrgcn_amd.reset_stats()
    with deterministic():
        a, b = grads(), grads()
    assert mrgcn_amd.stats().get("deterministic.complex_bwd", 0) == 2
    assert mrgcn_amd.stats().get("deterministic.distmult_bwd", 0) == 0
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert float(a[1].abs().max()) > 0 and float(a[2].abs().max()) > 0


# ---- 5. steps and the loop ---------------------------------------------------------------------------------------------
def _static(s):
    from mrgcn_amd.tasks import link_prediction as lp
    return lp.SortedTriples(s["sampler"].buf[:NTRAIN].contiguous(), N_, 2 * P_ + 1)


def test_train_step_equals_the_step_written_by_hand():
    from mrgcn_amd.tasks import link_prediction as lp
    s = _small()
    with deterministic():
        model, opt = _model()
        static = _static(s)
        got = [lp.train_step(model, _fwd(model), s["sampler"], opt, static, scorer="complex") for _ in range(3)]
        model2, opt2 = _model()
        want = []
        for _ in range(3):
            t, y = s["sampler"]()
            loss = lp.binary_crossentropy(lp.score_complex_bc(t, _fwd(model2)(), model2.relations, static=static), y)
            opt2.zero_grad(set_to_none=True)
            loss.backward()
            opt2.step()     # (a ClipAdam with a max_norm clips inside its step)
            want.append(loss.detach())
        model3, opt3 = _model()
        other = [lp.train_step(model3, _fwd(model3), s["sampler"], opt3, static) for _ in range(3)]
    print("complex losses", [float(x) for x in got], "distmult losses", [float(x) for x in other])
    for a, b in zip(got, want):
        assert _np(a).tobytes() == _np(b).tobytes()
    for (k, a), (_, b) in zip(model.state_dict().items(), model2.state_dict().items()):
        assert torch.equal(a, b), k
    assert float(got[0]) != float(other[0])


NEPOCH, INTERVAL = 6, 2


def _fit(model, opt, graphed, sampler, **kw):
    from mrgcn_amd.tasks import link_prediction as lp
    s = _small()
    return list(lp.fit(model, _fwd(model), s["train"], s["valid"], opt, NEPOCH, eval_interval=INTERVAL,
                       mrr_batchsize=100, filter_ranks=True, poll=3, graphed=graphed, sampler=sampler, warmup=3,
                       scorer="complex", **kw))


def _rows_equal(got, want):
    assert len(got) == len(want) == NEPOCH
    for g, w in zip(got, want):
        assert g[0] == w[0] and np.float32(g[1]).tobytes() == np.float32(w[1]).tobytes(), (g, w)
        for a, b in ((g[2], w[2]), (g[3], w[3]), (g[4], w[4]), (g[5], w[5])):
            assert (a is None) == (b is None)
            if a is not None:
                assert np.float32(a["raw"]).tobytes() == np.float32(b["raw"]).tobytes(), (g[0], a, b)
                assert np.float32(a["flt"]).tobytes() == np.float32(b["flt"]).tobytes(), (g[0], a, b)


def _keyed(s):
    from mrgcn_amd.tasks import link_prediction as lp
    return lp.NegativeSampler(s["train"], N_, 2 * P_ + 1, rate=3, seed=41)


@pytest.mark.parametrize("variant", ["plain", "l2", "keyed3"])
def test_fit_replayed_equals_eager_and_its_rows_equal_evaluate_facts(variant):
    from mrgcn_amd.tasks import link_prediction as lp
    s = _small()
    kw = dict(l2_lambda=1e-3) if variant == "l2" else {}
    mk = (lambda: _keyed(s)) if variant == "keyed3" else (lambda: s["sampler"])
    with deterministic():
        model, opt = _model()
        got = _fit(model, opt, True, mk(), **kw)
        model2, opt2 = _model()
        smp2 = mk()
        for _ in range(3):   # the capture's warm-up epochs are real steps
            model2.train()
            lp.train_step(model2, _fwd(model2), smp2, opt2, scorer="complex", **kw)
        want = _fit(model2, opt2, False, smp2, **kw)
        _rows_equal(got, want)
        for (k, a), (_, b) in zip(model.state_dict().items(), model2.state_dict().items()):
            assert torch.equal(a, b), k
        # the evaluating rows are evaluate_facts(scorer="complex") of the embeddings after that epoch's step
        model3, opt3 = _model()
        smp3 = mk()
        tparts, vparts = lp.FactParts(s["train"], 100, device="cuda"), lp.FactParts(s["valid"], 100, device="cuda")
        for epoch in range(1, 3 + INTERVAL + 1):
            model3.train()
            lp.train_step(model3, _fwd(model3), smp3, opt3, scorer="complex", **kw)
        model3.eval()
        with torch.no_grad():
            E = _fwd(model3)()
            tv = _np(lp.evaluate_facts(E, model3.relations, tparts, scorer="complex"))
            vv = _np(lp.evaluate_facts(E, model3.relations, vparts, scorer="complex"))
            dv = _np(lp.evaluate_facts(E, model3.relations, tparts))
    row = got[INTERVAL - 1]
    print(variant, "epoch", row[0], "loss", row[1], "train", row[2], "valid", row[4])
    for vec, (m, h) in ((tv, (row[2], row[3])), (vv, (row[4], row[5]))):
        flat = np.asarray([m["raw"]] + list(h["raw"]) + [m["flt"]] + list(h["flt"]), np.float32)
        assert flat.tobytes() == vec.tobytes()
    assert tv.tobytes() != dv.tobytes()   # (and not DistMult's evaluation of them)


def test_train_batch_step_on_a_masked_batch_equals_the_step_written_by_hand():
    from mrgcn_amd.tasks import link_prediction as lp
    from tests.test_gpu_lp_minibatch_fit import Problem
    with deterministic():
        a, b = Problem("nb13"), Problem("nb13")
        batch, facts = a.batches["train"][0]
        smp = a.fixed()(0, batch, facts)
        got = lp.train_batch_step(a.model, batch, facts, a.opt, sampler=smp, scorer="complex")
        batch2, facts2 = b.batches["train"][0]
        t, y = b.fixed()(0, batch2, facts2)()
        loss = lp.binary_crossentropy(lp.score_complex_bc(t, lp._embed(b.model, batch2), b.model.relations), y)
        b.opt.zero_grad()
        loss.backward()
        b.opt.step()
    assert _np(got).tobytes() == _np(loss.detach()).tobytes()
    for (k, x), (_, z) in zip(a.model.state_dict().items(), b.model.state_dict().items()):
        assert torch.equal(x, z), k


def test_evaluate_batches_equals_compute_ranks_fast_per_batch():
    from mrgcn_amd.tasks import link_prediction as lp
    s = _small()
    model, _ = _model()
    mrr, hits, rankings = lp.evaluate_batches(s["tb"], model, filtered=True, scorer="complex")
    want = {"raw": [], "flt": []}
    with torch.no_grad():
        for batch, facts in s["tb"]:
            E = lp._embed(model, batch)
            for flt in (False, True):
                want["flt" if flt else "raw"] += lp.compute_ranks_fast(np.asarray(facts), E, model.relations, filtered=flt,
                                                                       scorer="complex").tolist()
    assert rankings["raw"] == want["raw"] and rankings["flt"] == want["flt"] and want["raw"] != want["flt"]
    assert rankings["raw"] != lp.evaluate_batches(s["tb"], model, filtered=True)[2]["raw"]
    assert 0.0 < mrr["raw"] <= mrr["flt"] <= 1.0 and len(hits["raw"]) == 3


# ---- 6. it learns what DistMult cannot ---------------------------------------------------------------------------------
CYCLE_N, CYCLE_W, CYCLE_RATE, CYCLE_STEPS, CYCLE_LR, CYCLE_SEED = 40, 16, 5, 200, 0.05, 7


def _cycle_run(scorer):
    from mrgcn_amd.tasks import link_prediction as lp
    N = CYCLE_N
    facts = np.stack([np.arange(N), np.zeros(N, np.int64), (np.arange(N) + 1) % N], 1).astype(np.int64)
    g = torch.Generator().manual_seed(0)
    E = (0.5 * torch.randn(N, CYCLE_W, generator=g)).cuda().requires_grad_()
    Rel = (0.5 * torch.randn(1, CYCLE_W, generator=g)).cuda().requires_grad_()
    opt = torch.optim.Adam([E, Rel], lr=CYCLE_LR)
    smp = lp.NegativeSampler(facts, N, 1, rate=CYCLE_RATE, seed=CYCLE_SEED)
    score = lp.score_complex_bc if scorer == "complex" else lp.score_distmult_bc
    for _ in range(CYCLE_STEPS):
        t, y = smp()
        loss = lp.binary_crossentropy(score(t, E, Rel), y)
        opt.zero_grad()
        loss.backward()
        opt.step()
    ranks = _np(lp.compute_ranks_fast(facts, E, Rel, filtered=True, scorer=scorer))[:N]   # the tail side
    rev = facts[:, ::-1].copy()
    with torch.no_grad():
        fwd, back = _np(score(facts, E, Rel)), _np(score(rev, E, Rel))
    return float(np.mean(1.0 / ranks)), fwd, back, float(loss.detach())


def test_complex_learns_a_directed_cycle_and_distmult_cannot():
    """A 40-node directed cycle under one relation, free embeddings of width 16, a seeded NegativeSampler at rate 5
    filtered by the facts, Adam(lr 0.05) for 200 steps.  The float64 torch restatement on the CPU (the same data, draws
    and optimizer settings) separates the scorers at this step count: filtered tail MRR 0.7375 for DistMult — the
    reversed neighbour always ties with the true tail — and 1.0 for ComplEx, a gap of 0.2625; the margin asserted is
    half of it.  Measured on an MI355X after the 200 steps: ComplEx 1.0000 (loss 0.00033), DistMult 0.7375 (loss
    0.12635) — the same gap."""
    mrr_c, fwd_c, back_c, loss_c = _cycle_run("complex")
    mrr_d, fwd_d, back_d, loss_d = _cycle_run("distmult")
    print(f"directed cycle after {CYCLE_STEPS} steps: filtered tail MRR complex {mrr_c:.4f} (loss {loss_c:.5f}), "
          f"distmult {mrr_d:.4f} (loss {loss_d:.5f})")
    # asserted always: DistMult cannot tell a direction, ComplEx can
    np.testing.assert_allclose(fwd_d, back_d, rtol=1e-5, atol=1e-6)
    assert np.all(np.abs(fwd_c - back_c) > 1e-3)
    assert np.all(fwd_c > back_c)
    assert mrr_c >= mrr_d + 0.13
