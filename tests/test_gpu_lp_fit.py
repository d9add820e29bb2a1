"""Link prediction's run loop on the device (mrgcn_amd.tasks.link_prediction: rank_both, rank_metrics, record_row,
evaluate_facts, fit; csrc/lp_eval.hip).

Bounds.  Ranks are integers from bit-identical scores: exact.  `rank_metrics` adds in float64 and rounds once, so it is
held to one float32 rounding of the float64 numpy value (that value or its float32 neighbour).  Against the host path
(`evaluate_batches`: float32 `torch.mean` per part, float64 mean over parts) the metrics are held to 1e-6 absolute,
what tests/test_gpu_lp.py holds `mrr_hits` to.  Losses, rows of a replayed run and restored parameters are bitwise.

The end-to-end runs are held at hidden 16 (the issue's width: the narrow encoder backward, whose `dcomp` is summed in
a fixed order under torch.use_deterministic_algorithms(True), `deterministic.dcomp` in stats()) and at hidden 32 (the
wide featureless backward on its atomic-free units)."""
import os
from contextlib import contextmanager

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import lp_oracle as lo
from tests import util

pytestmark = pytest.mark.gpu

SHAPES = [(1000, 9, 200, 333), (257, 3, 7, 700), (4099, 20, 64, 1), (300, 4, 70, 1100)]
_CASES: dict = {}


def _np(t):
    return t.detach().cpu().numpy()


def _case(N, P, H, nf):
    """The inputs of tests/test_gpu_lp.py::test_ranks_against_oracle_bit_exact and the oracle's ranks (computed once)."""
    key = (N, P, H, nf)
    if key not in _CASES:
        rng = np.random.default_rng(N + nf)
        E = np.maximum(rng.standard_normal((N, H)), 0).astype(np.float32)
        E[rng.choice(N, N // 8, replace=False)] = 0
        Rel = rng.standard_normal((2 * P + 1, H)).astype(np.float32)
        facts = np.stack([rng.integers(0, N, nf), rng.integers(0, P, nf), rng.integers(0, N, nf)], 1).astype(np.int64)
        facts[nf // 2:, 0] = facts[: nf - nf // 2, 0]  # shared (s, p) pairs for the filter
        facts[nf // 2:, 1] = facts[: nf - nf // 2, 1]
        want = (lo.compute_ranks(facts, E, Rel, False), lo.compute_ranks(facts, E, Rel, True))
        _CASES[key] = (E, Rel, facts, want)
    E, Rel, facts, want = _CASES[key]
    Epad = torch.zeros((N, H + 3), device="cuda")
    Epad[:, :H] = torch.from_numpy(E).cuda()
    return E, Rel, facts, want, Epad[:, :H], torch.from_numpy(Rel).cuda()


def _lists(facts):
    from mrgcn_amd.tasks import link_prediction as lp
    return [torch.from_numpy(a).cuda() for a in lp.filter_lists(facts)]


# ---- 1. rank_both ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,P,H,nf", SHAPES)
def test_rank_both_against_oracle_bit_exact(N, P, H, nf):
    from mrgcn_amd.tasks import link_prediction as lp
    E, Rel, facts, (want_raw, want_flt), Ed, Rd = _case(N, P, H, nf)
    differ = int((want_raw != want_flt).sum())
    print(f"{(N, P, H, nf)}: raw and filtered ranks differ in {differ} of {2 * nf}")
    if nf > 1:
        assert differ >= 100   # (a kernel that ignores the lists cannot pass)
    assert Ed.stride(0) == H + 3
    facts_d = torch.from_numpy(facts).cuda()
    raw, flt = lp.rank_both(facts_d, Ed, Rd, _lists(facts))
    assert np.array_equal(_np(raw), want_raw)
    assert np.array_equal(_np(flt), want_flt)
    assert torch.equal(raw, lp.compute_ranks_fast(facts, Ed, Rd, filtered=False))
    assert torch.equal(flt, lp.compute_ranks_fast(facts, Ed, Rd, filtered=True))
    raw_only, none = lp.rank_both(facts, Ed, Rd)    # host facts, no lists
    assert none is None and torch.equal(raw_only, raw)


def test_rank_both_parts_equal_the_oracle_on_each_part():
    from mrgcn_amd.tasks import link_prediction as lp
    N, P, H, nf = SHAPES[1]
    E, Rel, facts, _, Ed, Rd = _case(N, P, H, nf)
    parts = lp.FactParts(facts, 100, device="cuda")
    assert parts.nparts == 7 and nf > N   # (one call for all facts would leave those behind position N unscored)
    raw, flt = lp.rank_both(parts, Ed, Rd)
    raw, flt = _np(raw), _np(flt)
    moved = 0
    for p in range(parts.nparts):
        a, b = int(parts.part_ptr_host[p]), int(parts.part_ptr_host[p + 1])
        want = [lo.compute_ranks(facts[a:b], E, Rel, filtered) for filtered in (False, True)]
        for got, w in zip((raw, flt), want):
            assert np.array_equal(np.concatenate([got[a:b], got[nf + a:nf + b]]), w), p
        moved += int((want[0] != want[1]).sum())
    assert moved >= 20   # (the oracle's own: the parts' lists do change ranks, though less than the whole set's 500)


def test_rank_both_in_slices_of_16_facts():
    from mrgcn_amd.tasks import link_prediction as lp
    N, P, H, nf = SHAPES[1]
    _, _, facts, (want_raw, want_flt), Ed, Rd = _case(N, P, H, nf)
    assert lp.rank_both_slice() % 8 == 0 and lp.rank_both_slice() > nf
    for slice_facts in (16, 13):    # 44 launches of two tiles (the last one partial); 13 rounds up to 16
        raw, flt = lp.rank_both(facts, Ed, Rd, _lists(facts), slice_facts=slice_facts)
        assert np.array_equal(_np(raw), want_raw) and np.array_equal(_np(flt), want_flt)


# ---- 2. rank_metrics -------------------------------------------------------------------------------------------------
def _metrics_ref(ranks, nf, ptr):
    per = []
    for p in range(len(ptr) - 1):
        r = np.concatenate([ranks[ptr[p]:ptr[p + 1]], ranks[nf + ptr[p]:nf + ptr[p + 1]]]).astype(np.float64)
        per.append([np.mean(1.0 / r)] + [np.mean(r <= k) for k in (1, 3, 10)])
    return np.mean(np.asarray(per, np.float64), axis=0)


def _one_rounding(got, want64):
    w = np.float32(want64)
    return got == w or got == np.nextafter(w, np.float32(np.inf)) or got == np.nextafter(w, np.float32(-np.inf))


@pytest.mark.parametrize("part", [1, 100, 0])
@pytest.mark.parametrize("nf", [1, 63, 64, 65, 1000, 70001])
def test_rank_metrics_against_float64_numpy(nf, part):
    from mrgcn_amd.tasks import link_prediction as lp
    # (seeds picked on the numpy side so that the condition below holds at every size: two ranks need (1, > 10))
    rng = np.random.default_rng((35233 if nf == 1 else 700021 + nf * 7) + part)
    ranks = rng.integers(1, 41, 2 * nf).astype(np.int64)
    size = part if part else nf
    split = np.array_split(np.arange(nf), max(nf // size, 1))
    ptr = np.concatenate([[0], np.cumsum([len(s) for s in split])]).astype(np.int64)
    want = _metrics_ref(ranks, nf, ptr)
    assert all(0.01 < w < 0.99 for w in want), want
    r_d, p_d = torch.from_numpy(ranks).cuda(), torch.from_numpy(ptr).cuda()
    score = torch.zeros((), device="cuda")
    got = lp.rank_metrics(r_d, p_d, score=score)
    score2 = torch.zeros((), device="cuda")
    again = lp.rank_metrics(r_d, p_d, score=score2)
    g = _np(got)
    print(f"nf={nf} parts={len(ptr) - 1}: got {g.tolist()} want {want.tolist()} score {float(score)!r}")
    for k in range(4):
        assert _one_rounding(g[k], want[k]), (k, g[k], want[k])
    assert _one_rounding(_np(score)[()], 1.0 - want[0])
    assert g.tobytes() == _np(again).tobytes() and _np(score).tobytes() == _np(score2).tobytes()
    if len(ptr) == 2:   # one part: part_ptr may be left out
        assert _np(lp.rank_metrics(r_d)).tobytes() == g.tobytes()


# ---- 3. record_row ---------------------------------------------------------------------------------------------------
TRACES = np.load(os.path.join(util.GOLDEN, "early_stop_traces.npz"))


@pytest.mark.parametrize("name", [str(n) for n in TRACES["names"]])
def test_record_row_replays_the_trace_like_record(name):
    from mrgcn_amd.train import _StopState
    patience, tolerance, delay = TRACES[f"{name}.config"]
    scores = TRACES[f"{name}.scores"]
    a = _StopState("cuda", int(patience), float(tolerance), int(delay))
    b = _StopState("cuda", int(patience), float(tolerance), int(delay))
    width, rows = 17, 4
    ring = torch.full((rows, width), -7.0, device="cuda")
    rng = np.random.default_rng(len(scores))
    stopped = False
    for k, score in enumerate(scores):
        s_d = torch.tensor(float(score), dtype=torch.float32, device="cuda")
        src = torch.from_numpy(rng.standard_normal(width).astype(np.float32)).cuda()
        a.record(s_d)
        b.record_row(s_d, src, ring)
        assert bytes(b.read()) == bytes(a.read()), (name, k)
        assert _np(ring)[k % rows].tobytes() == _np(src).tobytes(), (name, k)
        if b.read().stop:
            stopped = True
            break
    if not stopped:
        return
    frozen, ring0 = bytes(b.read()), _np(ring).copy()
    for j in range(5):   # lower scores after the stop: nothing moves, not even the ring
        b.record_row(torch.tensor(1e-3 / (j + 1), dtype=torch.float32, device="cuda"),
                     torch.zeros(width, device="cuda"), ring)
        assert bytes(b.read()) == frozen, (name, j)
    assert _np(ring).tobytes() == ring0.tobytes()


# ---- 4. / 5. a small model ------------------------------------------------------------------------------------------
N_, P_, NTRAIN, NVALID = 300, 4, 1100, 200


@contextmanager
def deterministic():
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev)


class FixedSampler:
    """The training facts and one fixed draw of corrupted copies: the same buffers every epoch."""

    def __init__(self, facts):
        rng = np.random.default_rng(5)
        n = len(facts)
        neg = facts[rng.choice(n, n // 5, replace=False)].copy()
        neg[: len(neg) // 2, 0] = rng.integers(0, N_, len(neg) // 2)
        neg[len(neg) // 2:, 2] = rng.integers(0, N_, len(neg) - len(neg) // 2)
        self.buf = torch.from_numpy(np.concatenate([facts, neg])).cuda()
        self.labels = torch.ones(len(self.buf), device="cuda")
        self.labels[n:] = 0

    def __call__(self):
        return self.buf, self.labels


_SMALL: dict = {}


def _small():
    """Facts, their host batches (mkbatches in full-batch mode, on the device) and the adjacency tensor they carry."""
    if not _SMALL:
        from mrgcn_amd import synth
        from mrgcn_amd.data.graph_structure import adjacency_from_triples
        from mrgcn_amd.tasks import link_prediction as lp
        tr = synth.make_triples(N_, P_, NTRAIN + NVALID, 3)
        tr = tr[np.random.default_rng(3).permutation(len(tr))]
        train, valid = tr[:NTRAIN], tr[NTRAIN:]
        A_csr = adjacency_from_triples(train, N_, P_)
        tb = lp.prepare_batches(lp.mkbatches(A_csr, None, train, 0, 100, 1), "cuda")
        vb = lp.prepare_batches(lp.mkbatches(A_csr, None, valid, 0, 100, 1), "cuda")
        assert len(tb) == 11 and len(vb) == 2
        _SMALL.update(train=train, valid=valid, tb=tb, vb=vb, A=tb[0][0].A, sampler=FixedSampler(train))
    return _SMALL


def _model(hidden=16, lr=0.05):
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.train import ClipAdam
    torch.manual_seed(11)
    model = RGCN([(0, hidden, "mrgcn", nn.ReLU())], 2 * P_ + 1, N_, 2, 0.0, True, False, True).cuda()
    opt = ClipAdam(model.parameters(), lr=lr, weight_decay=0.0, max_norm=1.0, capturable=True)
    return model, opt


def _host_order(ranks, parts):
    """rank_both's layout (all tail ranks, all head ranks) as evaluate_batches flattens it (part by part)."""
    r, nf, ptr = _np(ranks), parts.n, parts.part_ptr_host
    return np.concatenate([np.concatenate([r[ptr[p]:ptr[p + 1]], r[nf + ptr[p]:nf + ptr[p + 1]]])
                           for p in range(parts.nparts)]).tolist()


def test_evaluate_facts_against_evaluate_batches():
    from mrgcn_amd.tasks import link_prediction as lp
    s = _small()
    model, _ = _model()
    mrr, hits, rankings = lp.evaluate_batches(s["tb"], model, filtered=True)
    parts = lp.FactParts(s["train"], 100, device="cuda")
    assert parts.nparts == 11 and NTRAIN > N_
    model.eval()
    with torch.no_grad():
        E = model(None, s["A"])
        vec, raw, flt = lp.evaluate_facts(E, model.relations, parts, want_ranks=True)
        vec_raw = lp.evaluate_facts(E, model.relations, lp.FactParts(s["train"], 100, filtered=False, device="cuda"))
    assert _host_order(raw, parts) == rankings["raw"]
    assert _host_order(flt, parts) == rankings["flt"]
    assert rankings["raw"] != rankings["flt"]
    got = _np(vec).astype(np.float64)
    want = [mrr["raw"]] + list(hits["raw"]) + [mrr["flt"]] + list(hits["flt"])
    print("evaluate_facts", got.tolist(), "evaluate_batches", want)
    assert np.abs(got - np.asarray(want, np.float64)).max() <= 1e-6
    assert _np(vec_raw)[:4].tobytes() == _np(vec)[:4].tobytes() and _np(vec_raw)[4:].tolist() == [-1.0] * 4


NEPOCH, INTERVAL, POLL, PATIENCE, TOLERANCE = 12, 2, 3, 2, 0.05


def _fwd(model):
    A = _small()["A"]
    return lambda: model(None, A)


def _host_loop(model, opt, patience=PATIENCE):
    """train_model (link_prediction.py:224-373) on the host, from the library's step and its host evaluation."""
    from mrgcn_amd.tasks import link_prediction as lp
    from mrgcn_amd.train import EarlyStop
    s = _small()
    es = EarlyStop(patience=patience, tolerance=TOLERANCE, delay=0)
    rows = []
    for epoch in range(1, NEPOCH + 1):
        if es.stop:
            model.load_state_dict(es.best_weights)
            break
        model.train()
        loss = float(lp.train_step(model, _fwd(model), s["sampler"], opt))
        tm = th = vm = vh = None
        if epoch % INTERVAL == 0 or epoch == NEPOCH:
            tm, th, _ = lp.evaluate_batches(s["tb"], model, True)
            if epoch < NEPOCH:
                vm, vh, _ = lp.evaluate_batches(s["vb"], model, True)
                es.record(1.0 - vm["raw"], model, opt)
        rows.append((epoch, loss, tm, th, vm, vh))
    return rows, es


def _flat(m, h):
    return None if m is None else [m["raw"]] + list(h["raw"]) + [m["flt"]] + list(h["flt"])


def _fit(model, opt, graphed, patience=PATIENCE, warmup=3):
    from mrgcn_amd.tasks import link_prediction as lp
    from mrgcn_amd.train import EarlyStop
    s = _small()
    return list(lp.fit(model, _fwd(model), s["train"], s["valid"], opt, NEPOCH, eval_interval=INTERVAL,
                       mrr_batchsize=100, filter_ranks=True,
                       early_stop=EarlyStop(patience=patience, tolerance=TOLERANCE, delay=0), poll=POLL,
                       graphed=graphed, sampler=s["sampler"], warmup=warmup))


HIDDEN = [16, 32]   # 16: the narrow encoder backward; 32: the wide one


def _max_diff(a, b):
    return max(float((x.double() - y.double()).abs().max()) for x, y in zip(a, b))


@pytest.mark.parametrize("hidden", HIDDEN)
def test_fit_eager_against_the_host_loop(hidden):
    with deterministic():
        model, opt = _model(hidden)
        want, es = _host_loop(model, opt)
        print("host loop:", [(r[0], r[1], None if r[4] is None else r[4]["raw"]) for r in want])
        assert es.stop and len(want) < NEPOCH    # (the stop branch is reached)
        model2, opt2 = _model(hidden)
        got = _fit(model2, opt2, graphed=False)
        sd = model2.state_dict()
        print("hidden", hidden, "losses", [(g[1], w[1]) for g, w in zip(got, want)], "restored against best_weights:",
              "max |difference|", _max_diff([sd[k] for k in es.best_weights], list(es.best_weights.values())))
        assert [r[0] for r in got] == [r[0] for r in want]    # the same stopping epoch
        for g, w in zip(got, want):
            assert np.float32(g[1]).tobytes() == np.float32(w[1]).tobytes(), (g[0], g[1], w[1])
            for (gm, gh), (wm, wh) in (((g[2], g[3]), (w[2], w[3])), ((g[4], g[5]), (w[4], w[5]))):
                assert (gm is None) == (wm is None) and (gh is None) == (wh is None), g[0]
                if gm is not None:
                    assert np.abs(np.asarray(_flat(gm, gh)) - np.asarray(_flat(wm, wh), np.float64)).max() <= 1e-6
        assert set(sd) == set(es.best_weights)
        for k, v in es.best_weights.items():
            assert torch.equal(sd[k], v), k


@pytest.mark.parametrize("hidden", HIDDEN)
def test_fit_replayed_equals_warmup_steps_then_eager(hidden):
    from mrgcn_amd.tasks import link_prediction as lp
    with deterministic():
        s = _small()
        model, opt = _model(hidden)
        got = _fit(model, opt, graphed=True, warmup=3)
        model2, opt2 = _model(hidden)
        for _ in range(3):
            model2.train()
            lp.train_step(model2, _fwd(model2), s["sampler"], opt2)
        want = _fit(model2, opt2, graphed=False)
        print("hidden", hidden, "rows", len(got), len(want), "losses", [(g[1], w[1]) for g, w in zip(got, want)],
              "parameters: max |difference|", _max_diff(model.state_dict().values(), model2.state_dict().values()))
        assert len(want) < NEPOCH
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g[0] == w[0] and np.float32(g[1]).tobytes() == np.float32(w[1]).tobytes(), (g, w)
            for a, b in ((g[2], w[2]), (g[3], w[3]), (g[4], w[4]), (g[5], w[5])):
                assert (a is None) == (b is None)
                if a is not None:
                    assert np.float32(a["raw"]).tobytes() == np.float32(b["raw"]).tobytes(), (g[0], a, b)
                    assert np.float32(a["flt"]).tobytes() == np.float32(b["flt"]).tobytes(), (g[0], a, b)
        for (k, a), (_, b) in zip(model.state_dict().items(), model2.state_dict().items()):
            assert torch.equal(a, b), k


def test_fit_that_never_stops_keeps_the_schedule():
    from mrgcn_amd.tasks import link_prediction as lp
    with deterministic():
        model, opt = _model()
        rows = _fit(model, opt, graphed=True, patience=1000)
    sched = lp.eval_schedule(NEPOCH, INTERVAL, True)
    assert len(rows) == NEPOCH
    for (e, loss, tm, th, vm, vh), (se, eval_train, eval_valid, _) in zip(rows, sched):
        assert e == se and np.isfinite(loss)
        assert (tm is not None) == (th is not None) == eval_train, e
        assert (vm is not None) == (vh is not None) == eval_valid, e
        if tm is not None:
            assert 0.0 < tm["raw"] <= tm["flt"] <= 1.0 and len(th["raw"]) == len(th["flt"]) == 3
    assert rows[-1][2] is not None and rows[-1][4] is None
    assert len({r[1] for r in rows}) == NEPOCH    # every epoch its own loss: the ring rows were not mixed up


def test_fit_without_a_filter_reports_minus_one():
    from mrgcn_amd.tasks import link_prediction as lp
    s = _small()
    model, opt = _model()
    rows = list(lp.fit(model, _fwd(model), s["train"], None, opt, 3, eval_interval=2, filter_ranks=False,
                       graphed=False, sampler=s["sampler"]))
    assert [r[2] is not None for r in rows] == [False, True, True] and all(r[4] is None for r in rows)
    assert rows[1][2]["flt"] == -1.0 and rows[1][3]["flt"] == [-1.0] * 3 and 0.0 < rows[1][2]["raw"] <= 1.0


def test_ordered_dcomp_is_the_kernels_dcomp():
    """Under the flag the narrow layer's dcomp is summed again in a fixed order: the same sum as the kernel's atomic one
    (rtol 1e-3, atol 1e-6: what tests/test_gpu_lp_deterministic.py holds the reordered decoder gradients to), on the
    plain transposed product and on the live-column one, and the same bits on every call."""
    from mrgcn_amd import reset_stats, stats
    from mrgcn_amd.tasks import link_prediction as lp
    s = _small()
    model, _ = _model()

    def grads():
        out = []
        for _ in range(3):   # (the live-column backward takes over after the first steps' gauge)
            model.zero_grad(set_to_none=True)
            t, y = s["sampler"]()
            lp.binary_crossentropy(lp.score_distmult_bc(t, model(None, s["A"]), model.relations), y).backward()
            out.append(model.layers["layer_0"].weight_I_comp.grad.clone())
        return out
    plain = grads()
    reset_stats()
    with deterministic():
        first, again = grads(), grads()
    assert stats().get("deterministic.dcomp", 0) == 6
    for a, b, c in zip(plain, first, again):
        assert float(a.abs().max()) > 0
        np.testing.assert_allclose(_np(b), _np(a), rtol=1e-3, atol=1e-6)
        assert torch.equal(b, c)


def test_graphed_step_keeps_what_its_function_closes_over():
    """A GraphedStep is often all the caller keeps; the sampler's buffers and stored orders its launches name must not
    be freed under it."""
    import gc
    import weakref

    from mrgcn_amd.tasks import link_prediction as lp
    from mrgcn_amd.train import GraphedStep
    s = _small()
    model, opt = _model(32)

    def build():
        sampler = FixedSampler(s["train"])
        static = lp.SortedTriples(sampler.buf[:NTRAIN], N_, 2 * P_ + 1)
        return GraphedStep(lambda: lp.train_step(model, _fwd(model), sampler, opt, static), warmup=2), \
            weakref.ref(sampler), weakref.ref(static)
    step, w_sampler, w_static = build()
    gc.collect()
    assert w_sampler() is not None and w_static() is not None
    assert np.isfinite(float(step()))
