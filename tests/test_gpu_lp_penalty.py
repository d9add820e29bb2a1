"""The L1 / L2 weight penalty of the link-prediction steps and run loops (tasks.link_prediction: train_step,
train_batch_step, fit, fit_batches with l1_lambda / l2_lambda; ClipAdam.step(dense_penalty="kernel")) against the
reference's train_model on the 50-node golden graph (goldens of make_lp_penalty_goldens.py: the `nb17` batching of
tests/test_gpu_lp_minibatch_fit.py under Adam(lr 0.01, weight_decay 5e-4), l1 1e-4, l2 1e-3, 4 epochs, the reference's
negatives replayed), against the same steps with the penalty written into the loss by hand, and against themselves
(replayed, repeated).  Bounds are those of tests/test_gpu_lp_minibatch_fit.py: `LOSS` on every loss, every metric inside
the interval its near ties allow, `check_parameters` on the parameters.

Should the golden run ever miss a bound here while the fallback route (penalty in the loss, torch ops) misses it
equally, the inputs are at fault — a near tie that float32 resolves the other way — and the remedy is another
PARAM_SEED in the golden script, as tests/test_gpu_weight_reg_step.py documents for its own goldens, never a wider
bound."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import test_gpu_lp_minibatch_fit as mb
from tests import util
from tests.test_gpu_lp_minibatch_fit import LOSS, _bitwise, _check_rows, _flat, _np

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "lp_penalty.npz")
NEPOCH, INTERVAL = 4, 2
_G = np.load(GOLD)
LR, WD, L1, L2 = (float(x) for x in _G["hyper"])
PEN = dict(l1_lambda=L1, l2_lambda=L2)


def _optimizer(kind, params):
    from mrgcn_amd.optim import Adam, RowSparseAdam
    from mrgcn_amd.train import ClipAdam
    if kind == "clip":        # dense .grad, the clip inside the step
        return ClipAdam(params, lr=LR, weight_decay=WD, max_norm=1.0, capturable=True)
    if kind == "rows":        # the node table's gradient as flagged rows, the clip inside the step
        opt = RowSparseAdam(params, lr=LR, weight_decay=WD, capturable=True)
        opt.max_norm = 1.0
        return opt
    if kind == "fallback":    # no max_norm: clip_grad_norm_ in front of the step, the penalty in the loss
        return Adam(params, lr=LR, weight_decay=WD, capturable=True)
    raise KeyError(kind)


class Problem(mb.Problem):
    """tests/test_gpu_lp_minibatch_fit.py's problem on this file's golden and optimizers."""

    def __init__(self, kind="clip", masked=True):
        from mrgcn_amd.data.batch import scipy_sparse_to_pytorch_sparse
        from mrgcn_amd.models.rgcn import RGCN
        from mrgcn_amd.plan import plan_of
        from mrgcn_amd.tasks import link_prediction as lp
        self.g, self.tag = _G, "nb17"
        self.gb, self.tb, self.interval = 17, 40, INTERVAL
        _, A = util.load_graph("graph_small")
        N = A.shape[0]
        R = A.shape[1] // N
        self.A_csr, self.N, self.R = A, N, R
        self.model = RGCN([(0, 32, "mrgcn", nn.ReLU())], R, N, 2, 0.0, True, False, True)
        self.load("init")
        self.model = self.model.cuda()
        plan = plan_of(scipy_sparse_to_pytorch_sparse(A, dtype=torch.int8).cuda(), N, R) if masked else None
        self.batches = {}
        for split in ("train", "valid"):
            bs = lp.mkbatches(A, None, self.g[split], self.gb, self.tb, 1, plan=plan)
            assert len(bs) == int(self.g[f"nb17.{split}.count"])
            for i, (b, f) in enumerate(bs):   # the reference's batches, in its order
                assert np.array_equal(np.asarray(b.node_index), self.g[f"nb17.{split}.{i}.nodes"])
                assert np.array_equal(f, self.g[f"nb17.{split}.{i}.facts"])
            self.batches[split] = lp.prepare_batches(bs, "cuda")
        self.opt = _optimizer(kind, list(self.model.parameters()))

    def penalty(self):
        from mrgcn_amd.train import weight_regularisation
        with torch.no_grad():
            return weight_regularisation(self.model, L1, L2)

    def bce(self, batch, triples, labels):
        from mrgcn_amd.tasks import link_prediction as lp
        with torch.no_grad():
            E = lp._embed(self.model, batch)
            return lp.binary_crossentropy(lp.score_distmult_bc(triples, E, lp._relations(self.model)), labels)


def _close_parameters(a, b, steps, what):
    """check_parameters' bounds between two models."""
    for (k, x), (_, y) in zip(a.state_dict().items(), b.state_dict().items()):
        diff = np.abs(_np(x).astype(np.float64) - _np(y))
        print(f"{what}: {k} after {steps} steps max |diff| {diff.max():.3e}, share above 2e-5 {(diff > 2e-5).mean():.2e}")
        assert diff.max() <= 0.021 * steps, (what, k)
        assert (diff > 2e-5).mean() < 2e-3, (what, k, float((diff > 2e-5).mean()))


# ---- 1. the golden run -------------------------------------------------------------------------------------------------
def test_fit_batches_against_the_reference():
    import mrgcn_amd
    from mrgcn_amd.tasks import link_prediction as lp
    p = Problem("clip")
    nt = len(p.batches["train"])
    assert lp.penalty_owners(p.model, p.opt) and all("weight" in n for n, q in p.model.named_parameters()
                                                      if any(q is o for o in lp.penalty_owners(p.model, p.opt)))
    # the penalty matters at the start (the golden script asserts 5 % of the first batch's loss on its side)
    assert float(p.penalty()) >= 0.05 * float(p.g["nb17.first_epoch.loss"][0])
    mrgcn_amd.reset_stats()
    rows = list(p.fit(NEPOCH, graphed=False, poll=3, samplers=p.replayed(), **PEN))
    st = mrgcn_amd.stats()
    _check_rows(p, rows)
    p.check_parameters("final", NEPOCH * nt)
    assert st.get("adam.reg_dense") == NEPOCH * nt, st
    # epoch 1, batch by batch
    q = Problem("clip")
    run = lp.BatchFitEpochs(q.model, q.batches["train"], q.batches["valid"], q.opt, None, 4, False,
                            samplers=q.replayed(), **PEN)
    run.train_epoch()
    got, want = _np(run.loss_slots).astype(np.float64), p.g["nb17.first_epoch.loss"]
    print("epoch 1 slot losses", got.tolist(), "golden", want.tolist())
    np.testing.assert_allclose(got, want, **LOSS)


# ---- 2. the optimizer's routes -----------------------------------------------------------------------------------------
class Synth:
    """Two masked batches of an FB15k-like graph (`synth`, the smallest scale with >= 2 batches), 200 wide, 2 bases."""

    def __init__(self, kind):
        from mrgcn_amd import synth
        from mrgcn_amd.models.rgcn import RGCN
        from mrgcn_amd.plan import plan_of
        from mrgcn_amd.tasks import link_prediction as lp
        sg = synth.make_graph("fb15k", seed=0, scale=0.004)
        N, R = sg.num_nodes, sg.num_relations
        facts = np.asarray(sg.triples, dtype=np.int64)
        A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([sg.rows, sg.cols])), torch.from_numpy(sg.vals),
                                    (N, R * N)).cuda()
        bs = lp.mkbatches(None, None, facts, 32, 500, 1, plan=plan_of(A, N, R))
        assert len(bs) >= 2 and N == 64
        self.batches = {"train": lp.prepare_batches(bs, "cuda")[:3]}
        torch.manual_seed(0)
        self.model = RGCN([(0, 200, "mrgcn", nn.ReLU())], R, N, 2, 0.0, True, False, True).cuda()
        self.opt = _optimizer(kind, list(self.model.parameters()))
        rng = np.random.default_rng(9)
        self.neg = []
        for b, f in self.batches["train"]:
            neg = f[rng.choice(len(f), len(f) // 5, replace=False)].copy()
            neg[: len(neg) // 2, 0] = rng.integers(0, len(b.node_index), len(neg) // 2)
            neg[len(neg) // 2:, 2] = rng.integers(0, len(b.node_index), len(neg) - len(neg) // 2)
            self.neg.append(neg)

    penalty, bce = Problem.penalty, Problem.bce

    def fixed(self):
        def make(i, batch, facts):
            triples = torch.from_numpy(np.concatenate([facts, self.neg[i]])).cuda()
            labels = torch.ones(triples.shape[0], device="cuda")
            labels[len(facts):] = 0
            return lambda: (triples, labels)
        return make


@pytest.mark.parametrize("graph", ["golden", "synth"])
def test_three_routes_take_the_same_steps(graph, monkeypatch):
    """Dense `.grad` (ClipAdam), flagged rows (RowSparseAdam, nothing densified) and the fallback (penalty in the loss)
    step the same model to the same parameters, and every route's loss is BCE + the penalty of the pre-step state."""
    import mrgcn_amd
    from mrgcn_amd import optim
    from mrgcn_amd.tasks import link_prediction as lp
    merges = []
    real = optim.merge_row_grad
    monkeypatch.setattr(optim, "merge_row_grad", lambda p, ent: (merges.append(1), real(p, ent))[1])
    make = Problem if graph == "golden" else Synth
    runs = {kind: make(kind) for kind in ("clip", "rows", "fallback")}
    counts = {}
    for kind, r in runs.items():
        mrgcn_amd.reset_stats()
        merges.clear()
        r.losses = []
        tb = r.batches["train"]
        assert len(tb) >= 2
        for step in range(3):
            i = step % len(tb)
            sampler = r.fixed()(i, *tb[i])
            r.model.train()
            want = float(r.bce(tb[i][0], *sampler())) + float(r.penalty())
            loss = float(lp.train_batch_step(r.model, *tb[i], r.opt, sampler=sampler, **PEN))
            print(f"{graph} {kind} step {step}: loss {loss!r}, BCE + penalty of the pre-step state {want!r}")
            np.testing.assert_allclose(loss, want, **LOSS)
            r.losses.append(loss)
        counts[kind] = (mrgcn_amd.stats(), len(merges))
    st, merged = counts["rows"]
    assert merged == 0 and st.get("adam.reg_dense") == 3 and st.get("weight_I.rows") == 3, (st, merged)
    assert st.get("weight_I.dense") is None, st
    assert counts["clip"][0].get("adam.reg_dense") == 3 and not counts["clip"][0].get("weight_I.rows"), counts["clip"]
    assert counts["fallback"][0].get("adam.reg_dense") is None, counts["fallback"]
    for kind in ("rows", "fallback"):
        np.testing.assert_allclose(runs[kind].losses, runs["clip"].losses, **LOSS)
        _close_parameters(runs[kind].model, runs["clip"].model, 3, f"{graph}: {kind} against clip")
    # every node of the flagged table holds moments now
    ent = dict(runs["rows"].model.named_parameters())["layers.layer_0.weight_I"]._mrgcn_rows
    assert bool(ent["ever"].all()) and ent["ever_in"] == "any"
    moved = max(float((a - b).abs().max()) for a, b in zip(runs["clip"].model.state_dict().values(),
                                                           make("clip").model.state_dict().values()))
    assert moved > 1e-3


# ---- 3. full batch -----------------------------------------------------------------------------------------------------
class Full:
    """The golden graph as one full batch: its 90 training facts with epoch 1's negatives of the three batches' golden
    draws replaced by one fixed draw over all nodes."""

    def __init__(self, kind="clip"):
        from mrgcn_amd.tasks import link_prediction as lp
        self.p = p = Problem(kind)
        self.model, self.opt = p.model, p.opt
        train = np.asarray(p.g["train"], dtype=np.int64)
        self.train, self.valid = train, np.asarray(p.g["valid"], dtype=np.int64)
        fb = lp.prepare_batches(lp.mkbatches(p.A_csr, None, train, 0, 100, 1), "cuda")
        self.A = fb[0][0].A
        rng = np.random.default_rng(5)
        neg = train[rng.choice(len(train), len(train) // 5, replace=False)].copy()
        neg[: len(neg) // 2, 0] = rng.integers(0, p.N, len(neg) // 2)
        neg[len(neg) // 2:, 2] = rng.integers(0, p.N, len(neg) - len(neg) // 2)
        self.triples = torch.from_numpy(np.concatenate([train, neg])).cuda()
        self.labels = torch.ones(len(self.triples), device="cuda")
        self.labels[len(train):] = 0

    def sampler(self):
        return self.triples, self.labels

    def fwd(self):
        return self.model(None, self.A)

    def by_hand(self):
        """One epoch with the penalty written into the loss (the reference's form, :306-326)."""
        from mrgcn_amd.tasks import link_prediction as lp
        from mrgcn_amd.train import weight_regularisation
        self.model.train()
        loss = lp.binary_crossentropy(lp.score_distmult_bc(self.triples, self.fwd(), self.model.relations), self.labels)
        loss = loss + weight_regularisation(self.model, L1, L2)
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        self.opt.step()
        return float(loss.detach())

    def fit(self, nepoch, **kw):
        from mrgcn_amd.tasks import link_prediction as lp
        return list(lp.fit(self.model, self.fwd, self.train, self.valid, self.opt, nepoch, eval_interval=1,
                           mrr_batchsize=40, sampler=self.sampler, **kw))

    live_state = mb.Problem.live_state


def test_full_batch_step_and_fit_against_the_penalty_in_the_loss():
    import mrgcn_amd
    from mrgcn_amd.tasks import link_prediction as lp
    a, b = Full(), Full()
    mrgcn_amd.reset_stats()
    for step in range(3):
        a.model.train()
        got, want = float(lp.train_step(a.model, a.fwd, a.sampler, a.opt, **PEN)), b.by_hand()
        print(f"full batch step {step}: loss {got!r}, by hand {want!r}")
        np.testing.assert_allclose(got, want, **LOSS)
    assert mrgcn_amd.stats().get("adam.reg_dense") == 3
    _close_parameters(a.model, b.model, 3, "train_step against the penalty in the loss")
    c, d = Full(), Full()
    rows = c.fit(3, graphed=False, poll=2, **PEN)
    want = [d.by_hand() for _ in range(3)]
    print("fit losses", [r[1] for r in rows], "by hand", want)
    np.testing.assert_allclose([r[1] for r in rows], want, **LOSS)
    _close_parameters(c.model, d.model, 3, "fit against the penalty in the loss")
    assert float(d.p.penalty()) > 0.01   # (a penalty the LOSS bounds would notice)


# ---- 4. captured ---------------------------------------------------------------------------------------------------------
def _rows_bitwise(got, want):
    assert len(got) == len(want)
    a, b = np.asarray([_flat(r) for r in got]), np.asarray([_flat(r) for r in want])
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)
    assert a[ok].tobytes() == b[ok].tobytes(), (a, b)


def test_fit_replayed_equals_warmup_steps_then_eager():
    from mrgcn_amd.tasks import link_prediction as lp
    torch.use_deterministic_algorithms(True)
    try:
        a, b = Full(), Full()
        got = a.fit(4, graphed=True, warmup=3, poll=3, **PEN)
        for _ in range(3):
            b.model.train()
            lp.train_step(b.model, b.fwd, b.sampler, b.opt, **PEN)
        want = b.fit(4, graphed=False, poll=3, **PEN)
    finally:
        torch.use_deterministic_algorithms(False)
    print("replayed", [r[1] for r in got], "eager", [r[1] for r in want])
    _rows_bitwise(got, want)
    assert _bitwise(a.live_state(), b.live_state())


def test_fit_batches_replayed_equals_eager():
    """`warmup=1`: the capture's warm-up epoch is the eager run's epoch 1, replay e its epoch e + 1."""
    import mrgcn_amd
    torch.use_deterministic_algorithms(True)
    try:
        e, gr = Problem("clip"), Problem("clip")
        rows_e = list(e.fit(5, eval_interval=1, graphed=False, poll=3, samplers=e.fixed(), **PEN))
        mrgcn_amd.reset_stats()
        rows_g = list(gr.fit(4, eval_interval=1, graphed=True, warmup=1, poll=3, samplers=gr.fixed(), **PEN))
        st = mrgcn_amd.stats()
    finally:
        torch.use_deterministic_algorithms(False)
    assert st.get("lp.batch_eval_epoch.graphed") == 3 and st.get("lp.batch_epoch.graphed") == 1, st
    assert [r[0] for r in rows_g] == [1, 2, 3, 4]
    _rows_bitwise(rows_g, rows_e[1:])
    assert _bitwise(gr.live_state(), e.live_state())


# ---- 5. deterministic, 6. unchanged paths ------------------------------------------------------------------------------
def _three_batch_steps(kind, **kw):
    from mrgcn_amd.tasks import link_prediction as lp
    p = Problem(kind)
    for i, (b, f) in enumerate(p.batches["train"]):
        lp.train_batch_step(p.model, b, f, p.opt, negatives=p.g[f"nb17.neg.1.{i}"], **kw)
    return p.live_state()


def _three_full_steps(**kw):
    from mrgcn_amd.tasks import link_prediction as lp
    f = Full()
    for _ in range(3):
        f.model.train()
        lp.train_step(f.model, f.fwd, f.sampler, f.opt, **kw)
    return f.live_state()


@pytest.mark.parametrize("kind", ["clip", "rows"])
def test_two_runs_give_the_same_bits_under_the_deterministic_flag(kind):
    torch.use_deterministic_algorithms(True)
    try:
        assert _bitwise(_three_batch_steps(kind, **PEN), _three_batch_steps(kind, **PEN))
        if kind == "clip":
            assert _bitwise(_three_full_steps(**PEN), _three_full_steps(**PEN))
    finally:
        torch.use_deterministic_algorithms(False)


def test_zero_lambdas_change_nothing():
    torch.use_deterministic_algorithms(True)
    try:
        assert _bitwise(_three_batch_steps("clip"), _three_batch_steps("clip", l1_lambda=0.0, l2_lambda=0.0))
        assert _bitwise(_three_full_steps(), _three_full_steps(l1_lambda=0, l2_lambda=0))
        assert not _bitwise(_three_batch_steps("clip"), _three_batch_steps("clip", **PEN))
    finally:
        torch.use_deterministic_algorithms(False)
