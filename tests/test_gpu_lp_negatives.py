"""Keyed, filtered negatives on the device (csrc/lp_negatives.hip; mrgcn_amd.tasks.link_prediction.NegativeSampler,
batch_negative_samplers).

Bounds.  The draw is integer arithmetic: the kernel's triples and flags equal the numpy mirror
(`mrgcn_amd.host.negatives_draw`, whose own properties tests/test_cpu_lp_negatives.py holds) bit for bit, at every
position.  Training runs are held to what they promise: finite values, a falling loss, and — under
torch.use_deterministic_algorithms(True) — bitwise equal parameters and losses of two identical runs."""
from contextlib import contextmanager

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import util
from tests.test_cpu_lp_negatives import FIX300_SAMPLER_SEED, N, R, SEED, fixture300, fixture64, flag_case

pytestmark = pytest.mark.gpu
SIDES = {0: "both", 1: "tail", 2: "head"}


def _np(t):
    return t.detach().cpu().numpy()


@contextmanager
def deterministic():
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev)


def _position(smp):
    return int(smp.state[1])


def _mirror(smp, position, seed):
    """The mirror's draw for a sampler's own arguments."""
    from mrgcn_amd import host
    keys = None if smp.keys is None else _np(smp.keys).astype(np.uint64)
    return host.negatives_draw(_np(smp.facts), smp.rate, smp.n_cand, smp.num_nodes, smp.num_relations, keys, seed,
                               position, side=smp.side, cand=None if smp.candidates is None else _np(smp.candidates),
                               to_global=None if smp.to_global is None else _np(smp.to_global))


def _check(smp, position, seed):
    want, flags = _mirror(smp, position, seed)
    assert np.array_equal(_np(smp.buf[smp.n:]), want)
    assert np.array_equal(_np(smp.unresolved), flags)
    return want, flags


# ---- 1. the kernel equals the mirror bit for bit ----------------------------------------------------------------------
@pytest.mark.parametrize("filtered", [True, False], ids=["filtered", "unfiltered"])
@pytest.mark.parametrize("side", [0, 1, 2], ids=["both", "tail", "head"])
@pytest.mark.parametrize("rate", [1, 3, 10])
def test_draw_equals_the_mirror(rate, side, filtered):
    from mrgcn_amd.tasks import link_prediction as lp
    fx = fixture64()
    for nfacts in (257, 1):     # 257: two blocks at rate 1, the last one partial; 1: a single thread's worth per rate
        smp = lp.NegativeSampler(fx["facts"][:nfacts], N, R, rate=rate, known=fx["known"] if filtered else False,
                                 side=SIDES[side], seed=SEED)
        triples, labels = smp()
        assert triples is smp.buf and labels is smp.labels
        assert np.array_equal(_np(triples[:nfacts]), fx["facts"][:nfacts])
        want, flags = _check(smp, 0, SEED)
        assert int(flags.sum()) == 0 and smp.num_unresolved() == 0
        if filtered:
            keys = _np(smp.keys)
            got = _np(smp.buf[nfacts:])
            assert not np.isin((got[:, 0] * R + got[:, 1]) * N + got[:, 2], keys).any()


def test_draw_with_a_candidate_subset_and_with_global_ids():
    from mrgcn_amd.tasks import link_prediction as lp
    fx = fixture64()
    facts = fx["facts"]
    cand = np.random.default_rng(5).choice(N, 17, replace=False).astype(np.int64)
    smp = lp.NegativeSampler(facts, N, R, rate=3, known=fx["known"], candidates=torch.from_numpy(cand).cuda(), seed=SEED)
    smp()
    want, _ = _check(smp, 0, SEED)
    src = np.repeat(facts, 3, axis=0)
    assert np.isin(np.where(want[:, 0] != src[:, 0], want[:, 0], want[:, 2]), cand).all()
    # local ids under a permutation of the 64 nodes, the known facts in global ids
    perm = np.random.default_rng(6).permutation(N).astype(np.int64)
    inv = np.argsort(perm)
    local = np.stack([inv[facts[:, 0]], facts[:, 1], inv[facts[:, 2]]], 1)
    for known in (fx["known"], None):    # None: the facts' own keys, through to_global
        smp = lp.NegativeSampler(local, N, R, rate=3, known=known, to_global=torch.from_numpy(perm).cuda(), seed=SEED)
        smp()
        want, flags = _check(smp, 0, SEED)
        glob = np.stack([perm[want[:, 0]], want[:, 1], perm[want[:, 2]]], 1)
        keys = _np(smp.keys)
        assert len(keys) == (500 if known is not None else 257)
        assert not np.isin((glob[:, 0] * R + glob[:, 1]) * N + glob[:, 2], keys).any() and int(flags.sum()) == 0


def test_flag_case_equals_the_mirror():
    from mrgcn_amd.tasks import link_prediction as lp
    facts = flag_case()
    smp = lp.NegativeSampler(facts, 8, 1, rate=4, seed=99)     # known = None: the facts themselves
    smp()
    want, flags = _check(smp, 0, 99)
    tail_side = want[:, 0] == np.repeat(facts, 4, axis=0)[:, 0]
    assert np.array_equal(flags.astype(bool), tail_side) and smp.num_unresolved() == int(tail_side.sum()) > 0


# ---- 2. the position advances ----------------------------------------------------------------------------------------
def test_position_advances_and_reseed_puts_it_back():
    from mrgcn_amd.tasks import link_prediction as lp
    fx = fixture64()
    smp = lp.NegativeSampler(fx["facts"], N, R, rate=3, known=fx["known"], seed=SEED)
    assert _np(smp.state).tolist() == [SEED, 0]
    draws = []
    for position in range(3):
        smp()
        draws.append(_check(smp, position, SEED)[0])
        assert _position(smp) == position + 1
    assert not np.array_equal(draws[0], draws[1]) and not np.array_equal(draws[1], draws[2])
    state = smp.state
    smp.reseed(SEED, position=0)
    assert smp.state is state and _np(state).tolist() == [SEED, 0]
    smp()
    assert np.array_equal(_np(smp.buf[smp.n:]), draws[0])
    smp.reseed(SEED + 1, position=5)
    smp()
    _check(smp, 5, SEED + 1)
    torch.manual_seed(77)       # seed=None: torch's initial seed, as set_node_dropout takes it
    auto = lp.NegativeSampler(fx["facts"], N, R, seed=None)
    assert _np(auto.state).tolist() == [77, 0]


# ---- 3. the sampler contract -----------------------------------------------------------------------------------------
def test_sampler_contract_and_graph_replay():
    from mrgcn_amd.tasks import link_prediction as lp
    fx = fixture64()
    n, rate = 257, 3
    smp = lp.NegativeSampler(torch.from_numpy(fx["facts"]).cuda(), N, R, rate=rate, known=fx["known"], seed=SEED)
    a = smp()
    b = smp()
    assert a[0] is b[0] is smp.buf and a[1] is b[1] is smp.labels
    assert smp.buf.shape == (n * (1 + rate), 3) and smp.facts.data_ptr() == smp.buf.data_ptr()
    assert _np(smp.labels).tolist() == [1.0] * n + [0.0] * (n * rate)
    assert smp.unresolved.shape == (n * rate,) and smp.unresolved.dtype == torch.uint8
    static = lp.SortedTriples(smp.facts, N, R)
    assert static.covers(a[0])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
        smp()
    torch.cuda.synchronize()
    p = _position(smp)
    assert p == 2       # (a capture runs nothing)
    for r in range(3):
        graph.replay()
        torch.cuda.synchronize()
        _check(smp, p + r, SEED)
        assert _position(smp) == p + r + 1


# ---- 4. training through every loop ----------------------------------------------------------------------------------
def _golden_problem():
    """The 50-node golden graph, the one-layer featureless encoder of rgcn_small_lp_b2 on it, the graph's 120 triples
    as facts."""
    from mrgcn_amd.train import ClipAdam
    name = "rgcn_small_lp_b2"
    c = util.load_case(name)
    g, A_csr = util.load_graph(util.graph_of_case(name))
    model, _ = util.build_rgcn_from_case(c, "cuda")
    util.load_state_from_case(model, c)
    model = model.cuda()
    A = util.coo_tensor(A_csr, str(c["value_mode"]), "cuda")
    facts = np.asarray(g["triples"], dtype=np.int64)
    opt = ClipAdam(model.parameters(), lr=0.05, weight_decay=0.0, max_norm=1.0, capturable=True)
    return model, opt, A, A_csr, facts, int(c["meta.num_nodes"]), int(c["meta.R"])


def test_train_step_eager_loss_falls():
    from mrgcn_amd.tasks import link_prediction as lp
    model, opt, A, _, facts, nn_, nr = _golden_problem()
    smp = lp.NegativeSampler(facts, nn_, nr, rate=3, known=facts, seed=SEED)
    static = lp.SortedTriples(smp.facts, nn_, nr)
    model.train()
    losses = [float(lp.train_step(model, lambda: model(None, A), smp, opt, static=static)) for _ in range(4)]
    print("losses", losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert smp.num_unresolved() == 0 and _position(smp) == 4


def _check_rows(rows, nepoch, has_valid):
    assert [r[0] for r in rows] == list(range(1, nepoch + 1))
    for epoch, loss, tm, th, vm, vh in rows:
        assert isinstance(loss, float) and np.isfinite(loss)
        assert tm is not None and set(tm) == {"raw", "flt"} and set(th) == {"raw", "flt"}
        vals = [tm["raw"], tm["flt"]] + list(th["raw"]) + list(th["flt"])
        assert len(th["raw"]) == len(th["flt"]) == 3
        if has_valid and epoch < nepoch:
            assert vm is not None
            vals += [vm["raw"], vm["flt"]] + list(vh["raw"]) + list(vh["flt"])
        else:
            assert vm is None and vh is None
        assert all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in vals), vals


def test_fit_graphed_with_the_keyed_sampler():
    import mrgcn_amd
    from mrgcn_amd.tasks import link_prediction as lp
    model, opt, A, _, facts, nn_, nr = _golden_problem()
    train, valid = facts[:100], facts[100:]
    smp = lp.NegativeSampler(train, nn_, nr, rate=3, known=facts, seed=SEED)
    mrgcn_amd.reset_stats()
    rows = list(lp.fit(model, lambda: model(None, A), train, valid, opt, 6, eval_interval=1, mrr_batchsize=50,
                       graphed=True, sampler=smp, static=lp.SortedTriples(smp.facts, nn_, nr)))
    _check_rows(rows, 6, True)
    # ---- 6. the counter
    assert mrgcn_amd.stats().get("lp.negatives.keyed", 0) >= 1
    # 3 warm-up epochs, two captures (nothing runs), 6 replayed epochs: the last draw is the mirror's at position 8
    torch.cuda.synchronize()
    assert _position(smp) == 9
    _check(smp, 8, SEED)
    assert smp.num_unresolved() == 0


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graphed"])
def test_fit_batches_with_batch_negative_samplers(graphed):
    from mrgcn_amd.data.batch import scipy_sparse_to_pytorch_sparse
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.plan import plan_of
    from mrgcn_amd.tasks import link_prediction as lp
    from mrgcn_amd.train import ClipAdam
    _, _, _, A_csr, facts, nn_, nr = _golden_problem()
    torch.manual_seed(3)
    model = RGCN([(0, 32, "mrgcn", nn.ReLU())], nr, nn_, 2, 0.0, True, False, True).cuda()
    opt = ClipAdam(list(model.parameters()), lr=0.01, max_norm=1.0, capturable=True)
    plan = plan_of(scipy_sparse_to_pytorch_sparse(A_csr, dtype=torch.int8).cuda(), nn_, nr)
    train, valid = facts[:90], facts[90:]
    tb = lp.prepare_batches(lp.mkbatches(A_csr, None, train, 17, 40, 1, plan=plan), "cuda")
    vb = lp.prepare_batches(lp.mkbatches(A_csr, None, valid, 13, 20, 1, plan=plan), "cuda")
    assert len(tb) > 1
    inner = lp.batch_negative_samplers(nn_, nr, rate=3, known=facts, seed=SEED)
    made = []

    def samplers(i, batch, f):
        made.append(inner(i, batch, f))
        return made[-1]
    rows = list(lp.fit_batches(model, tb, vb, opt, 3, eval_interval=1, graphed=graphed, samplers=samplers))
    _check_rows(rows, 3, True)
    torch.cuda.synchronize()
    assert len(made) == len(tb)
    keys = np.sort((facts[:, 0] * nr + facts[:, 1]) * nn_ + facts[:, 2])
    for i, (smp, (batch, f)) in enumerate(zip(made, tb)):
        node_index = _np(batch.node_index)
        assert np.array_equal(_np(smp.facts), np.asarray(f)) and np.array_equal(_np(smp.to_global), node_index)
        assert smp.n_cand == len(node_index) and np.array_equal(_np(smp.keys), keys)
        want, flags = _check(smp, _position(smp) - 1, SEED + i)
        neg = _np(smp.buf[smp.n:])
        assert neg[:, [0, 2]].min() >= 0 and neg[:, [0, 2]].max() < len(node_index)      # batch-local ids only
        assert int(flags.sum()) == 0
        glob = (node_index[neg[:, 0]] * nr + neg[:, 1]) * nn_ + node_index[neg[:, 2]]
        assert not np.isin(glob, keys).any()                                               # no known global fact


# ---- 5. reproducibility under the flag -------------------------------------------------------------------------------
def _encoder_problem(facts, num_nodes, num_pred):
    from mrgcn_amd.data.graph_structure import adjacency_from_triples
    from mrgcn_amd.tasks import link_prediction as lp
    A_csr = adjacency_from_triples(facts, num_nodes, num_pred)
    return lp.prepare_batches(lp.mkbatches(A_csr, None, facts, 0, len(facts), 1), "cuda")[0][0].A


def _run(facts, A, num_nodes, num_pred, rate, sampler_seed):
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.tasks import link_prediction as lp
    from mrgcn_amd.train import ClipAdam
    torch.manual_seed(11)
    nr = 2 * num_pred + 1
    model = RGCN([(0, 16, "mrgcn", nn.ReLU())], nr, num_nodes, 2, 0.0, True, False, True).cuda()
    opt = ClipAdam(model.parameters(), lr=0.05, weight_decay=0.0, max_norm=1.0)
    smp = lp.NegativeSampler(facts, num_nodes, num_pred, rate=rate, seed=sampler_seed)   # (the facts' p < num_pred)
    model.train()
    losses = [lp.train_step(model, lambda: model(None, A), smp, opt).clone() for _ in range(3)]
    torch.cuda.synchronize()
    assert smp.num_unresolved() == 0
    return losses, [p.detach().clone() for p in model.parameters()]


@pytest.mark.parametrize("case", ["one_block", "stable_order"])
def test_two_identical_runs_are_bitwise_equal_under_the_flag(case):
    import mrgcn_amd
    from mrgcn_amd.tasks.link_prediction import _DET_SMALL_N
    if case == "one_block":     # n (1 + rate) = 1 028 triples: the deterministic backward sorts them in one block
        facts, nn_, npred, rate, seed = fixture64()["facts"], N, R, 3, SEED
        assert len(facts) * (1 + rate) < _DET_SMALL_N
    else:                       # 5 000 triples: the stable radix sort in front of the owner passes
        facts, nn_, npred, rate, seed = fixture300(), 300, 5, 1, FIX300_SAMPLER_SEED
        assert len(facts) * (1 + rate) > _DET_SMALL_N
    A = _encoder_problem(facts, nn_, npred)
    with deterministic():
        mrgcn_amd.reset_stats()
        l1, p1 = _run(facts, A, nn_, npred, rate, seed)
        assert mrgcn_amd.stats().get("deterministic.distmult_bwd", 0) == 3
        l2, p2 = _run(facts, A, nn_, npred, rate, seed)
    print(case, "losses", [float(x) for x in l1])
    assert all(np.isfinite(float(x)) for x in l1)
    assert all(torch.equal(a, b) for a, b in zip(l1, l2))
    assert len(p1) == len(p2) and all(torch.equal(a, b) for a, b in zip(p1, p2))
