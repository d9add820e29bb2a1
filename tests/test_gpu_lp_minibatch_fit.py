"""The mini-batch link-prediction run loop on the device (mrgcn_amd.tasks.link_prediction.fit_batches, eval_batches,
rank_batches) against the reference's train_model / test_model on the 50-node golden graph (goldens of
make_lp_minibatch_fit_goldens.py: 90 training and 30 validation facts, batches of 17 / 40 and 13 / 20), with the
reference's negatives replayed, and against the package's own per-batch functions.  Model and masked batches are set up
as tests/test_gpu_lp_minibatch.py does."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import util

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "lp_minibatch_fit.npz")
CASES = {"nb17": (17, 40, 2), "nb13": (13, 20, 2), "nb13_stop": (13, 20, 1)}
LOSS = dict(rtol=2e-4, atol=2e-5)
NEPOCH = 6


def _np(t):
    return t.detach().cpu().numpy()


class Problem:
    def __init__(self, tag, masked=True):
        from mrgcn_amd.data.batch import scipy_sparse_to_pytorch_sparse
        from mrgcn_amd.models.rgcn import RGCN
        from mrgcn_amd.plan import plan_of
        from mrgcn_amd.tasks import link_prediction as lp
        from mrgcn_amd.train import ClipAdam
        self.g = g = np.load(GOLD)
        self.tag = tag
        self.gb, self.tb, self.interval = CASES[tag]
        _, A = util.load_graph("graph_small")
        N = A.shape[0]
        R = A.shape[1] // N
        self.model = RGCN([(0, 32, "mrgcn", nn.ReLU())], R, N, 2, 0.0, True, False, True)
        self.load("init")
        self.model = self.model.cuda()
        plan = plan_of(scipy_sparse_to_pytorch_sparse(A, dtype=torch.int8).cuda(), N, R) if masked else None
        self.batches = {}
        for split in ("train", "valid"):
            bs = lp.mkbatches(A, None, g[split], self.gb, self.tb, 1, plan=plan)
            assert len(bs) == int(g[f"{tag}.{split}.count"])
            for i, (b, f) in enumerate(bs):   # the reference's batches, in its order
                assert np.array_equal(np.asarray(b.node_index), g[f"{tag}.{split}.{i}.nodes"])
                assert np.array_equal(f, g[f"{tag}.{split}.{i}.facts"])
            self.batches[split] = lp.prepare_batches(bs, "cuda")
        self.opt = ClipAdam(list(self.model.parameters()), lr=0.01, max_norm=1.0, capturable=True)

    def load(self, state):
        pre = f"{self.tag}.{state}."
        dev = next(self.model.parameters()).device
        self.model.load_state_dict({k[len(pre):]: torch.from_numpy(np.array(self.g[k])).to(dev) for k in self.g.files
                                    if k.startswith(pre) and k[len(pre):] in self.model.state_dict()})

    def replayed(self):
        """`samplers` for fit_batches: batch i's triples of every recorded epoch, uploaded beforehand; call e of the
        sampler hands out epoch e + 1's (past the record: the last epoch's again)."""
        g, tag = self.g, self.tag
        epochs = int(g[f"{tag}.epochs_run"])

        def make(i, batch, facts):
            stack = torch.from_numpy(np.stack([np.concatenate([facts, g[f"{tag}.neg.{e}.{i}"]])
                                               for e in range(1, epochs + 1)])).cuda()
            labels = torch.ones(stack.shape[1], device="cuda")
            labels[len(facts):] = 0
            calls = [0]

            def sampler():
                e = min(calls[0], epochs - 1)
                calls[0] += 1
                return stack[e], labels
            return sampler
        return make

    def fixed(self):
        """`samplers` that hand out the first recorded epoch's negatives every time."""
        g, tag = self.g, self.tag

        def make(i, batch, facts):
            triples = torch.from_numpy(np.concatenate([facts, g[f"{tag}.neg.1.{i}"]])).cuda()
            labels = torch.ones(triples.shape[0], device="cuda")
            labels[len(facts):] = 0
            return lambda: (triples, labels)
        return make

    def fit(self, nepoch, **kw):
        from mrgcn_amd.tasks import link_prediction as lp
        kw.setdefault("eval_interval", self.interval)
        return lp.fit_batches(self.model, self.batches["train"], kw.pop("valid", self.batches["valid"]), self.opt, nepoch,
                              **kw)

    def check_parameters(self, state, steps):
        """tests/test_gpu_nc_minibatch.py::Problem.check_parameters' bounds."""
        sd = self.model.state_dict()
        pre = f"{self.tag}.{state}."
        keys = [k for k in self.g.files if k.startswith(pre) and k[len(pre):] in sd]
        worst = {k[len(pre):]: float(np.abs(_np(sd[k[len(pre):]]) - self.g[k]).max()) for k in keys}
        print(f"{self.tag}: parameters after {steps} steps, max |diff| {worst}")
        assert worst and all(v <= 0.021 * steps for v in worst.values()), worst
        for k in keys:
            diff = np.abs(_np(sd[k[len(pre):]]) - self.g[k])
            print(f"  {k}: share of elements off by more than 2e-5: {float((diff > 2e-5).mean())}")
            assert (diff > 2e-5).mean() < 2e-3, (k, float((diff > 2e-5).mean()))
            moved = np.abs(self.g[k] - self.g[f"{self.tag}.init.{k[len(pre):]}"])
            assert moved.max() > 1e-3, k     # (the golden itself left the initial state: the check has teeth)

    def live_state(self):
        out = [p.detach().clone() for p in self.model.parameters()]
        for p in self.model.parameters():
            out += [v.clone() for v in self.opt.state[p].values() if torch.is_tensor(v)]
        for ent in self.opt._dev_step.values():
            out += [ent[0].clone(), ent[1].clone()]
        return out


def _bitwise(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and _np(x).tobytes() == _np(y).tobytes() for x, y in zip(a, b))


def _flat(row):
    """A yielded tuple as the golden's table row: loss | train raw mrr h1 h3 h10, flt ... | valid ... (NaN for None)."""
    def eight(mrr, hits):
        if mrr is None:
            assert hits is None
            return [np.nan] * 8
        return [mrr["raw"]] + list(hits["raw"]) + [mrr["flt"]] + list(hits["flt"])
    return [row[1]] + eight(row[2], row[3]) + eight(row[4], row[5])


def _check_rows(p, rows):
    g, tag = p.g, p.tag
    want, lo, hi = g[f"{tag}.rows"], g[f"{tag}.rows_lo"], g[f"{tag}.rows_hi"]
    assert [r[0] for r in rows] == g[f"{tag}.epochs"].tolist()
    got = np.asarray([_flat(r) for r in rows], dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want))          # the reference's None pattern
    for e, (a, b) in enumerate(zip(got, want), 1):
        print(f"epoch {e}: got {a.tolist()}\n      golden {b.tolist()}")
    np.testing.assert_allclose(got[:, 0], want[:, 0], **LOSS)
    ok = ~np.isnan(want)
    ok[:, 0] = False
    print("metrics against their intervals: worst excess",
          float(np.maximum(lo[ok] - got[ok], got[ok] - hi[ok]).max()), "widest interval", float((hi - lo)[ok].max()))
    assert np.all(got[ok] >= lo[ok] - 1e-6) and np.all(got[ok] <= hi[ok] + 1e-6)
    assert float((hi - lo)[ok].max()) <= 0.02


@pytest.mark.parametrize("tag,poll", [("nb17", 8), ("nb13", 4)])
def test_eager_fit_against_the_reference(tag, poll):
    """The reference's six epochs with its negatives replayed: epochs, None pattern, losses, every metric inside the
    interval its near ties (TAU) allow, the final parameters — and TAU itself: the final state's candidate scores on
    the device differ from the reference's by at most a quarter of it."""
    from mrgcn_amd.tasks import link_prediction as lp
    p = Problem(tag)
    g = p.g
    assert [(e, t, v) for e, t, v, _ in lp.eval_schedule(NEPOCH, p.interval, True)] == \
        [(e, e % 2 == 0, e % 2 == 0 and e < NEPOCH) for e in range(1, NEPOCH + 1)]
    rows = list(p.fit(NEPOCH, graphed=False, poll=poll, samplers=p.replayed()))
    _check_rows(p, rows)
    p.check_parameters("final", NEPOCH * len(p.batches["train"]))
    tau, drift = float(g["tau"]), 0.0
    p.model.eval()
    with torch.no_grad():
        Rel = p.model.relations
        for i, (b, f) in enumerate(p.batches["train"]):
            E = p.model(None, b.A)
            t = torch.from_numpy(f).cuda()
            tail, head = (E[t[:, 0]] * Rel[t[:, 1]]) @ E.T, (Rel[t[:, 1]] * E[t[:, 2]]) @ E.T
            drift = max(drift, float(np.abs(_np(tail) - g[f"{tag}.final.tail.{i}"]).max()),
                        float(np.abs(_np(head) - g[f"{tag}.final.head.{i}"]).max()),
                        float(np.abs(_np(E) - g[f"{tag}.final.E.{i}"]).max()))
    print(f"{tag}: largest score / embedding difference after {NEPOCH} epochs {drift:.3e}, TAU {tau:.1e}")
    assert drift <= tau / 4


def test_early_stop_restores_epoch_1():
    """EarlyStop(2, 10.0, 0) with eval_interval 1: records 2 and 3 spend the patience, the stop is seen at the poll
    after epoch 4 (poll=4: the ring has wrapped by then), three rows are yielded and epoch 1's state is back."""
    from mrgcn_amd.train import EarlyStop
    p = Problem("nb13_stop")
    rows = list(p.fit(NEPOCH, graphed=False, poll=4, samplers=p.replayed(), early_stop=EarlyStop(2, 10.0, 0)))
    assert len(rows) == 3
    _check_rows(p, rows)
    p.check_parameters("epoch1", len(p.batches["train"]))
    p.check_parameters("final", len(p.batches["train"]))


def test_last_row_ranks_and_means_tie_to_existing_code():
    """After a run that reaches nepoch: the last row's training metrics are `eval_batches` of the final state, bit for
    bit; `rank_batches`' rankings are `evaluate_batches`' exactly, its means `evaluate_batches`' float32 means."""
    from mrgcn_amd.tasks import link_prediction as lp
    p = Problem("nb17")
    rows = list(p.fit(3, eval_interval=1, graphed=False, poll=2))
    assert [r[0] for r in rows] == [1, 2, 3] and rows[-1][4] is None and rows[0][4] is not None
    tb = p.batches["train"]
    means = lp.eval_batches(p.model, tb)
    assert p.model.training
    assert lp._unpack(means.cpu()) == (rows[-1][2], rows[-1][3])
    total = 2 * sum(len(f) for _, f in tb)
    raw, flt = (torch.empty(total, dtype=torch.int64, device="cuda") for _ in range(2))
    slots = torch.empty((len(tb), 8), device="cuda")
    assert lp.eval_batches(p.model, tb, slots=slots, ranks=(raw, flt)) is None
    mrr, hits, ranks = lp.rank_batches(p.model, tb)
    mrr0, hits0, ranks0 = lp.evaluate_batches(tb, p.model, filtered=True)
    for kind, buf in (("raw", raw), ("flt", flt)):
        assert ranks[kind] == ranks0[kind] == buf.tolist()
        np.testing.assert_allclose(mrr[kind], mrr0[kind], rtol=1e-6)
        np.testing.assert_allclose(hits[kind], hits0[kind], rtol=1e-6)
    assert lp._unpack(means.cpu()) == (mrr, hits)
    # the slots are the batches' own values: their float64 means, rounded once, are the row
    want = np.asarray([np.float32(np.mean(_np(slots)[:, k].astype(np.float64))) for k in range(8)])
    assert np.array_equal(_np(means), want)
    mrr1, hits1, ranks1 = lp.rank_batches(p.model, tb, filtered=False)
    assert mrr1["raw"] == mrr["raw"] and mrr1["flt"] == -1 and hits1["flt"] == [-1, -1, -1]
    assert ranks1["raw"] == ranks["raw"] and ranks1["flt"] == lp.evaluate_batches(tb, p.model, filtered=False)[2]["flt"]


@pytest.mark.parametrize("deterministic", [True, False])
def test_graphed_against_eager(deterministic):
    """`warmup=1`: the capture's warm-up epoch is the eager run's epoch 1, replay e its epoch e + 1 (every epoch
    evaluates, every batch has fixed negatives).  Under torch's deterministic flag rows, parameters and Adam state are
    equal bit for bit."""
    import mrgcn_amd
    torch.use_deterministic_algorithms(deterministic)
    try:
        e, gr = Problem("nb17"), Problem("nb17")
        rows_e = list(e.fit(5, eval_interval=1, graphed=False, poll=3, samplers=e.fixed()))
        mrgcn_amd.reset_stats()
        rows_g = list(gr.fit(4, eval_interval=1, graphed=True, warmup=1, poll=3, samplers=gr.fixed()))
        st = mrgcn_amd.stats()
    finally:
        torch.use_deterministic_algorithms(False)
    assert st.get("lp.batch_eval_epoch.graphed") == 3 and st.get("lp.batch_epoch.graphed") == 1, st
    assert not [k for k in st if k.startswith("lp.batch") and k.endswith(".eager")], st
    assert [r[0] for r in rows_g] == [1, 2, 3, 4] and [r[0] for r in rows_e] == [1, 2, 3, 4, 5]
    a, b = np.asarray([_flat(r) for r in rows_g]), np.asarray([_flat(r) for r in rows_e[1:]])
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)
    if deterministic:
        assert a[ok].tobytes() == b[ok].tobytes()
        assert _bitwise(gr.live_state(), e.live_state())
    else:
        np.testing.assert_allclose(a[ok], b[ok], rtol=1e-5, atol=1e-6)


def test_eager_routes_past_the_cap_and_for_slice_batches():
    import mrgcn_amd
    p = Problem("nb17")
    mrgcn_amd.reset_stats()
    rows = list(p.fit(3, graphed=True, max_graph_batches=7, poll=2))   # 2 * 3 + 2 = 8 batch passes
    st = mrgcn_amd.stats()
    assert len(rows) == 3 and st.get("lp.batch_epoch.eager") == 2 and st.get("lp.batch_eval_epoch.eager") == 1, st
    assert not [k for k in st if k.startswith("lp.batch") and k.endswith(".graphed")], st
    s = Problem("nb17", masked=False)
    mrgcn_amd.reset_stats()
    rows = list(s.fit(3, graphed=True, poll=2, samplers=s.replayed()))
    st = mrgcn_amd.stats()
    assert len(rows) == 3 and st.get("lp.batch_epoch.eager") == 2 and st.get("lp.batch_eval_epoch.eager") == 1, st
    np.testing.assert_allclose([r[1] for r in rows], s.g["nb17.rows"][:3, 0], **LOSS)


@pytest.mark.parametrize("graphed", [False, True])
def test_epochs_do_not_wait(graphed):
    """A training and an evaluating epoch under torch's sync debug mode, eager and replayed."""
    from mrgcn_amd.tasks import link_prediction as lp
    p = Problem("nb17")
    run = lp.BatchFitEpochs(p.model, p.batches["train"], p.batches["valid"], p.opt, None, 4, graphed, warmup=1)
    if not graphed:
        run.eval_epoch()   # (first use: the optimizer's state, the batches' lists and workspaces)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")   # (a synchronising call inside an epoch raises)
    try:
        run.train_epoch()
        run.eval_epoch()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    st = run.eval_ctr.read()
    assert int(st.records) == (1 if graphed else 2) and int(run.loss_ctr.read().records) == (2 if graphed else 3)
    row = _np(run.eval_ring)[(int(st.records) - 1) % 4]
    assert np.isfinite(row).all() and 0 < row[1] <= row[5] <= 1 and 0 < row[9] <= row[13] <= 1


def test_refusals_and_defaults():
    from mrgcn_amd import _lib as L
    from mrgcn_amd.tasks import link_prediction as lp
    from mrgcn_amd.train import ClipAdam, EarlyStop
    p = Problem("nb17")
    rows = list(p.fit(2, eval_interval=1, graphed=False, valid=None, filter_ranks=False))
    assert all(r[4] is None and r[5] is None for r in rows) and len(rows) == 2
    assert all(r[2]["flt"] == -1 and r[3]["flt"] == [-1, -1, -1] and 0 < r[2]["raw"] <= 1 for r in rows)
    with pytest.raises(L.MrgcnError, match="early stopping"):
        next(p.fit(2, graphed=False, valid=None, early_stop=EarlyStop(2, 0.0, 0)))
    with pytest.raises(L.MrgcnError, match="capturable"):
        next(lp.fit_batches(p.model, p.batches["train"], p.batches["valid"],
                            ClipAdam(list(p.model.parameters()), lr=0.01, max_norm=1.0), 2, graphed=True))


def test_train_batch_step_keeps_its_defaults():
    """Without the new arguments: the step of before.  With `slot` and a `sampler` that hands out the same triples:
    the same loss and parameters, bit for bit under the deterministic flag, and the loss in the slot."""
    from mrgcn_amd.tasks import link_prediction as lp
    torch.use_deterministic_algorithms(True)
    try:
        a, b = Problem("nb17"), Problem("nb17")
        slot = torch.zeros(3, device="cuda")
        for i in range(3):
            neg = a.g[f"nb17.neg.1.{i}"]
            la = lp.train_batch_step(a.model, *a.batches["train"][i], a.opt, negatives=neg)
            lb = lp.train_batch_step(b.model, *b.batches["train"][i], b.opt, slot=slot[i:i + 1],
                                     sampler=b.fixed()(i, *b.batches["train"][i]))
            assert _np(la).tobytes() == _np(lb).tobytes() == _np(slot[i]).tobytes()
            assert 0.1 < float(la) < 1.0   # (a loss, not a placeholder)
        assert _bitwise(a.live_state(), b.live_state())
        with pytest.raises(lp._lib.MrgcnError, match="not both"):
            lp.train_batch_step(b.model, *b.batches["train"][0], b.opt, negatives=neg, sampler=lambda: None)
    finally:
        torch.use_deterministic_algorithms(False)
