"""The mini-batch node-classification run loop on the device (mrgcn_amd/tasks/node_classification.py) against the
reference's own loop on the CPU (tests/golden/nc_minibatch.npz, written by tests/golden/make_nc_minibatch_goldens.py:
the reference's mkbatches, train_model, eval_model and test_model on the 50-node golden graph; train batches of 8, 8
and 7 nodes, validation batches of 8 and 3, test batches of 8 and ONE).  The batches here are masked batches on the
full graph's plan, set up as tests/test_minibatch.py::test_masked_batch_on_the_full_plan_equals_the_goldens does.

Tolerances: losses rtol 2e-4, atol 2e-5 — what tests/test_gpu_layers.py allows step losses against goldens;
accuracies and labels exact (the generator asserts a top-two logit margin above 1e-3 on every evaluated row);
parameters after s optimizer steps `max |diff| <= 0.021 s`, that file's bound after its golden epochs (Adam moves an
element whose gradient is rounding noise by up to lr per step in either direction); two paths of the same run
rtol 1e-5, atol 1e-6, the bound tests/test_minibatch.py uses between paths.

A graphed run's warm-up epoch is a real optimizer step (GraphedBatchEpoch): with `warmup=1` epoch k of the run is
epoch k + 1 of the golden, and the rows are compared from that matching epoch."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import util

pytestmark = pytest.mark.gpu

GOLD = os.path.join(util.GOLDEN, "nc_minibatch.npz")
LOSS = dict(rtol=2e-4, atol=2e-5)
PATHS = dict(rtol=1e-5, atol=1e-6)
CLASSES, HIDDEN, XW, BATCHSIZE, LAYERS = 4, 6, 5, 8, 2
TAGS = ["fl_b3", "ft_b3", "fl_b3_l2"]
L2 = {"fl_b3_l2": 5e-4}
STEPS_PER_EPOCH = 3


def _np(t):
    return t.detach().cpu().numpy()


def _labels(g, split, N):
    nodes, classes = g[f"{split}.nodes"], g[f"{split}.classes"]
    return sp.csr_matrix((np.ones(len(nodes), dtype=np.int8), (nodes, classes)), shape=(N, CLASSES), dtype=np.int8)


class Problem:
    def __init__(self, tag, state="init", splits=("train", "valid")):
        from mrgcn_amd.data.batch import scipy_sparse_to_pytorch_sparse
        from mrgcn_amd.models.rgcn import RGCN
        from mrgcn_amd.plan import plan_of
        from mrgcn_amd.tasks import node_classification as nc
        from mrgcn_amd.train import ClipAdam
        self.g = g = np.load(GOLD)
        self.tag = tag
        _, A = util.load_graph("graph_small")
        N = A.shape[0]
        R = A.shape[1] // N
        fl = tag.startswith("fl")
        modules = [(0 if fl else XW, HIDDEN, "mrgcn", torch.nn.ReLU()), (HIDDEN, CLASSES, "mrgcn", None)]
        self.model = RGCN(modules, R, N, 3, 0.0, fl, True, False)
        self.load(state)
        self.model = self.model.cuda()
        self.plan = plan_of(scipy_sparse_to_pytorch_sparse(A, dtype=torch.int8).cuda(), N, R)  # the reference's cast
        self.X = None if fl else [np.array(g["X_full"])]
        self.Y = {s: _labels(g, s, N) for s in ("train", "valid", "test")}
        self.batches = {s: nc.prepare_batches(nc.mkbatches(None, self.X, self.Y[s], BATCHSIZE, LAYERS, plan=self.plan),
                                              self.Y[s], "cuda") for s in splits}
        for s in splits:   # the reference's batches, in its order
            assert len(self.batches[s]) == int(g[f"{s}.count"])
            for i, b in enumerate(self.batches[s]):
                assert np.array_equal(_np(b.node_index), g[f"{s}.{i}.node_index"])
                assert np.array_equal(_np(b._mrgcn_nc["pos"]), g[f"{s}.{i}.pos"])
                assert np.array_equal(_np(b._mrgcn_nc["tgt"]), g[f"{s}.{i}.targets"])
        self.opt = ClipAdam(list(self.model.parameters()), lr=0.01, max_norm=1.0, capturable=True)
        self.l2 = L2.get(tag, 0.0)

    def load(self, state):
        g, tag = self.g, self.tag
        pre = f"{tag}.{state}."
        self.model.load_state_dict({k[len(pre):]: torch.from_numpy(np.array(g[k])).to(
            next(self.model.parameters()).device) for k in g.files if k.startswith(pre)})

    def fit(self, nepoch, **kw):
        from mrgcn_amd.tasks import node_classification as nc
        return nc.fit(self.model, self.batches["train"], kw.pop("valid", self.batches.get("valid")), self.opt, nepoch,
                      l2_lambda=self.l2, **kw)

    def check_parameters(self, state, steps):
        sd = self.model.state_dict()
        pre = f"{self.tag}.{state}."
        worst = {}
        for k in self.g.files:
            if k.startswith(pre):
                worst[k[len(pre):]] = float(np.abs(_np(sd[k[len(pre):]]) - self.g[k]).max())
        print(f"{self.tag}: parameters after {steps} steps, max |diff| {worst}")
        assert worst and all(v <= 0.021 * steps for v in worst.values()), worst
        # the bound of tests/test_gpu_layers.py for steps past the first (its :107): all but 2 in 1000 elements of
        # every tensor within 2e-5 of the golden (an element whose gradient is rounding noise may take Adam's lr-sized
        # step the other way; nothing else may differ).  An untrained or wrongly stepped model fails it: Adam moves
        # every element with a gradient by about lr = 1e-2 per step.
        for k in self.g.files:
            if k.startswith(pre):
                diff = np.abs(_np(sd[k[len(pre):]]) - self.g[k])
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


def _check_rows(rows, want, first_epoch=1):
    assert [r[0] for r in rows] == list(range(first_epoch, first_epoch + len(rows)))
    got = np.asarray([r[1:] for r in rows], dtype=np.float64)
    for k, (a, b) in enumerate(zip(got, want)):
        print(f"epoch {k + first_epoch}: got {a.tolist()} golden {b.tolist()}")
    np.testing.assert_allclose(got[:, 0], want[:, 0], **LOSS)
    np.testing.assert_allclose(got[:, 2], want[:, 2], **LOSS)
    # accuracies: the golden means are float64 means of float32 ratios, the rows float32 roundings of the same means
    assert np.array_equal(got[:, 1].astype(np.float32), want[:, 1].astype(np.float32))
    assert np.array_equal(got[:, 3].astype(np.float32), want[:, 3].astype(np.float32))


# ---- fit against the golden rows ------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_eager_fit_yields_the_references_rows(tag):
    """Eight epochs, polled every three (the ring wraps): every row, then the parameters.  `fl_b3_l2`: the batch
    losses, and so the epoch's, include the penalty."""
    p = Problem(tag)
    rows = list(p.fit(8, poll=3, graphed=False))
    _check_rows(rows, p.g[f"{tag}.rows"])
    p.check_parameters("final", 8 * STEPS_PER_EPOCH)
    assert p.model.training


@pytest.mark.parametrize("tag", TAGS)
def test_graphed_fit_yields_the_references_rows_from_the_matching_epoch(tag):
    """`warmup=1`: the capture's warm-up epoch is the golden's epoch 1, the seven replays are its epochs 2 to 8."""
    import mrgcn_amd
    p = Problem(tag)
    mrgcn_amd.reset_stats()
    rows = list(p.fit(7, poll=3, graphed=True, warmup=1))
    st = mrgcn_amd.stats()
    assert st.get("nc.batch_epoch.graphed") == 7 and "nc.batch_epoch.eager" not in st, st
    _check_rows(rows, p.g[f"{tag}.rows"][1:])
    p.check_parameters("final", 8 * STEPS_PER_EPOCH)
    assert int(next(iter(p.opt._dev_step.values()))[0].item()) == 8 * STEPS_PER_EPOCH


@pytest.mark.parametrize("tag", TAGS)
def test_train_batch_step_gives_the_references_batch_values_of_epoch_1(tag):
    from mrgcn_amd.tasks import node_classification as nc
    p = Problem(tag)
    g = p.g
    slots = torch.zeros((3, 2), device="cuda")
    p.model.train()
    got = [nc.train_batch_step(p.model, b, p.opt, l2_lambda=p.l2, slot=slots[i])
           for i, b in enumerate(p.batches["train"])]
    losses = np.asarray([float(l) for l, _ in got])
    accs = np.asarray([float(a) for _, a in got], dtype=np.float32)
    print(f"{tag}: batch losses {losses.tolist()} golden {g[f'{tag}.epoch1.train_loss'].tolist()}")
    np.testing.assert_allclose(losses, g[f"{tag}.epoch1.train_loss"], **LOSS)
    assert np.array_equal(accs, g[f"{tag}.epoch1.train_acc"].astype(np.float32))
    # the table holds what the step returned: the loss with its penalty, the accuracy of the same logits
    assert np.array_equal(_np(slots)[:, 0], losses.astype(np.float32)) and np.array_equal(_np(slots)[:, 1], accs)
    vslots = torch.zeros((2, 2), device="cuda")
    assert nc.eval_model(p.model, p.batches["valid"], slots=vslots) is None and p.model.training
    np.testing.assert_allclose(_np(vslots)[:, 0], g[f"{tag}.epoch1.valid_loss"], **LOSS)
    assert np.array_equal(_np(vslots)[:, 1], g[f"{tag}.epoch1.valid_acc"].astype(np.float32))
    loss, acc = nc.eval_model(p.model, p.batches["valid"])
    np.testing.assert_allclose(float(loss), g[f"{tag}.rows"][0][2], **LOSS)
    assert np.float32(float(acc)) == np.float32(g[f"{tag}.rows"][0][3])


@pytest.mark.parametrize("tag", ["fl_b3", "ft_b3"])
def test_graphed_and_eager_rows_of_the_same_run_agree(tag):
    from mrgcn_amd.tasks import node_classification as nc
    eager = Problem(tag)
    nc.BatchEpoch(eager.model, eager.batches["train"], eager.batches["valid"], eager.opt, l2_lambda=eager.l2)()
    rows_e = list(eager.fit(5, poll=2, graphed=False))     # (the graphed run's warm-up epoch, then five)
    graphed = Problem(tag)
    rows_g = list(graphed.fit(5, poll=2, graphed=True, warmup=1))
    assert [r[0] for r in rows_e] == [r[0] for r in rows_g] == [1, 2, 3, 4, 5]
    np.testing.assert_allclose(np.asarray(rows_g)[:, 1:], np.asarray(rows_e)[:, 1:], **PATHS)
    # more batches than the cap: fit runs the eager epoch instead of capturing
    import mrgcn_amd
    mrgcn_amd.reset_stats()
    capped = Problem(tag)
    rows_c = list(capped.fit(6, poll=2, graphed=True, max_graph_batches=4))
    assert mrgcn_amd.stats().get("nc.batch_epoch.eager") == 6 and "nc.batch_epoch.graphed" not in mrgcn_amd.stats()
    np.testing.assert_allclose(np.asarray(rows_c)[1:, 1:], np.asarray(rows_e)[:, 1:], **PATHS)


# ---- early stopping -------------------------------------------------------------------------------------------------
def test_eager_early_stop_yields_the_references_three_rows_and_its_restored_state():
    from mrgcn_amd.train import EarlyStop
    p = Problem("fl_b3")
    rows = list(p.fit(8, poll=1, graphed=False, early_stop=EarlyStop(2, 10.0, 0)))
    _check_rows(rows, p.g["fl_b3_stop.rows"])
    assert len(rows) == 3
    p.tag = "fl_b3_stop"   # (fl_b3_stop.final: the state the reference's loop restored, that of epoch 1)
    p.check_parameters("final", STEPS_PER_EPOCH)
    # ... and not the state of epoch 3, where the run stood when it stopped (the golden's own epochs differ by more)
    sd = p.model.state_dict()
    k = "layers.layer_1.weight_F"
    assert np.abs(_np(sd[k]) - p.g["fl_b3_stop.final." + k]).max() < 1e-4 < np.abs(p.g["fl_b3.final." + k] - p.g["fl_b3_stop.final." + k]).max()


def test_graphed_early_stop_poll1_yields_three_rows_and_restores_epoch_1_bitwise():
    """EarlyStop(patience 2, tolerance 10, delay 0): record 1 sets the best score, nothing improves by 10, records 2
    and 3 spend the patience — whatever the float noise."""
    from mrgcn_amd.train import EarlyStop
    p = Problem("fl_b3")
    rows, clones = [], {}
    for row in p.fit(8, poll=1, graphed=True, warmup=1, early_stop=EarlyStop(2, 10.0, 0)):
        rows.append(row)
        clones[row[0]] = p.live_state()
    assert [r[0] for r in rows] == [1, 2, 3]
    _check_rows(rows, p.g["fl_b3.rows"][1:4])
    live = p.live_state()
    assert _bitwise(live, clones[1])
    assert not _bitwise(live, clones[3]) and not _bitwise(clones[1], clones[2])
    assert int(next(iter(p.opt._dev_step.values()))[0].item()) == 2 * STEPS_PER_EPOCH   # warm-up epoch + epoch 1


def test_graphed_early_stop_poll4_yields_the_same_three_rows_and_replays_after_the_restore(monkeypatch):
    """The poll after epoch 4 finds the stop of record 3: epoch 4 ran and left nothing behind.  Every replay is
    followed by a clone of the live state, so the restored state is compared with what this run held after epoch 1."""
    from mrgcn_amd.tasks import node_classification as nc
    from mrgcn_amd.train import EarlyStop
    p = Problem("fl_b3")
    clones, replay, made = [], nc.GraphedBatchEpoch.__call__, []

    def replay_then_clone(self):
        out = replay(self)
        clones.append(p.live_state())
        made.append(self)
        return out
    monkeypatch.setattr(nc.GraphedBatchEpoch, "__call__", replay_then_clone)
    rows = list(p.fit(8, poll=4, graphed=True, warmup=1, early_stop=EarlyStop(2, 10.0, 0)))
    assert [r[0] for r in rows] == [1, 2, 3]
    _check_rows(rows, p.g["fl_b3.rows"][1:4])
    assert len(clones) == 4       # one epoch ran past the stop
    live = p.live_state()
    assert _bitwise(live, clones[0])
    assert not _bitwise(clones[0], clones[2]) and not _bitwise(clones[2], clones[3]) and not _bitwise(live, clones[3])
    run = made[0]
    assert (run.stopper.records, run.stopper.best_record, run.stopper.poll()) == (3, 1, True)
    # a replay after restore_(): no _state_gen error, the graph still owns the tensors it was captured on
    gen = p.opt._state_gen
    row = replay(run)
    assert p.opt._state_gen == gen and np.isfinite(_np(row)).all()
    assert run.stopper.records == 3          # (latched: the record changed nothing)
    assert not _bitwise(p.live_state(), clones[0])   # (but the step was taken)


# ---- test_model -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_test_model_on_the_golden_final_state(tag):
    from mrgcn_amd.tasks import node_classification as nc
    p = Problem(tag, state="final", splits=("test",))
    g = p.g
    assert [len(b.node_index) for b in p.batches["test"]] == [8, 1]     # (a one-row batch)
    loss, acc, labels, targets = nc.test_model(p.model, p.batches["test"])
    assert isinstance(loss, float) and isinstance(acc, float) and labels.dtype == np.int64 and targets.dtype == np.int64
    print(f"{tag}: test loss {loss!r} golden {float(g[f'{tag}.test.loss'])!r} acc {acc!r}")
    assert np.array_equal(labels, g[f"{tag}.test.labels"]) and np.array_equal(targets, g[f"{tag}.test.targets"])
    np.testing.assert_allclose(loss, float(g[f"{tag}.test.loss"]), **LOSS)
    assert np.float32(acc) == np.float32(g[f"{tag}.test.acc"])
    # a batch whose node_index is unsorted: labels and targets follow ITS order
    from mrgcn_amd.data.batch import MiniBatch
    order = np.concatenate([g["test.0.node_index"], g["test.1.node_index"]])
    label_of = dict(zip(order.tolist(), g[f"{tag}.test.labels"].tolist()))
    target_of = dict(zip(order.tolist(), g[f"{tag}.test.targets"].tolist()))
    shuffled = order[np.random.default_rng(3).permutation(len(order))]
    assert not np.array_equal(shuffled, np.sort(shuffled))
    b = nc.prepare_batches([MiniBatch(None, p.X, shuffled, LAYERS, plan=p.plan)], p.Y["test"], "cuda")
    _, acc2, labels2, targets2 = nc.test_model(p.model, b)
    assert labels2.tolist() == [label_of[n] for n in shuffled.tolist()]
    assert targets2.tolist() == [target_of[n] for n in shuffled.tolist()]
    assert np.float32(acc2) == np.float32((labels2 == targets2).mean(dtype=np.float32))


# ---- no validation batches ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graphed", [False, True])
def test_fit_without_validation_batches_yields_minus_one_and_refuses_early_stopping(graphed):
    from mrgcn_amd import _lib as L
    from mrgcn_amd.train import EarlyStop
    p = Problem("fl_b3", splits=("train",))
    rows = list(p.fit(3, valid=[], poll=2, graphed=graphed, warmup=1))
    assert [r[0] for r in rows] == [1, 2, 3] and all(r[3] == -1 and r[4] == -1 for r in rows)
    first = 1 if graphed else 0
    np.testing.assert_allclose([r[1] for r in rows], p.g["fl_b3.rows"][first:first + 3, 0], **LOSS)
    with pytest.raises(L.MrgcnError):
        next(p.fit(3, valid=[], graphed=graphed, early_stop=EarlyStop(2, 10.0, 0)))
    with pytest.raises(L.MrgcnError):
        next(p.fit(3, valid=None, graphed=graphed, early_stop=EarlyStop(2, 10.0, 0)))


# ---- no host synchronisation, the routes taken ----------------------------------------------------------------------
def test_an_epoch_never_waits_for_the_device_and_both_epochs_take_the_same_optimizer_route():
    import mrgcn_amd
    from mrgcn_amd.tasks import node_classification as nc
    from mrgcn_amd.train import EarlyStop
    routes = {}
    for kind in ("eager", "graphed"):
        p = Problem("fl_b3")
        args = (p.model, p.batches["train"], p.batches["valid"], p.opt, EarlyStop(7, 0.01, 0))
        run = nc.BatchEpoch(*args)
        run()      # (first use: lazily built workspaces, the optimizer's state, the loss's row flags)
        before = 1
        if kind == "graphed":
            mrgcn_amd.reset_stats()
            run = nc.GraphedBatchEpoch(*args, warmup=1)
            built = mrgcn_amd.stats()   # (the warm-up epoch and the capture: two passes over the host code)
            assert all(v % 2 == 0 for k, v in built.items() if k.split(".")[0] in ("adam", "weight_I")), built
            routes["capture"] = {k: v // 2 for k, v in built.items() if k.split(".")[0] in ("adam", "weight_I")}
            before = 0                  # (the capture resets the counter)
        epochs = 1 if kind == "eager" else 3
        torch.cuda.synchronize()
        mrgcn_amd.reset_stats()
        torch.cuda.set_sync_debug_mode("error")   # (a synchronising call inside an epoch raises)
        try:
            for _ in range(epochs):
                run()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        st = mrgcn_amd.stats()
        assert st.get(f"nc.batch_epoch.{kind}") == epochs, st
        if kind == "eager":
            assert st.get("nc.fused_loss") == 3 + 2, st       # one launch per training and per validation batch
            routes["eager"] = {k: v for k, v in st.items() if k.split(".")[0] in ("adam", "weight_I")}
        else:
            assert "nc.fused_loss" not in st, st              # (a replay runs no host code of the epoch)
        assert run.counter.read().records == before + epochs
        assert np.isfinite(_np(run.ring)[:before + epochs]).all()
    print("optimizer routes per epoch:", routes)
    # the node table's update takes the row-sparse route, once per training batch, eager and inside the capture
    for kind in ("eager", "capture"):
        assert routes[kind].get("weight_I.rows") == 3 and routes[kind].get("adam.rows") == 3, routes
        assert "weight_I.dense" not in routes[kind], routes
    assert routes["eager"] == routes["capture"], routes


def test_slice_batches_run_the_eager_epoch_and_are_not_captured():
    """The reference's slices (mkbatches without a plan) go through BatchEpoch; a capture refuses them by name."""
    import mrgcn_amd
    from mrgcn_amd import _lib as L
    from mrgcn_amd.tasks import node_classification as nc
    p = Problem("fl_b3")
    _, A = util.load_graph("graph_small")
    tb = nc.prepare_batches(nc.mkbatches(A, None, p.Y["train"], BATCHSIZE, LAYERS), p.Y["train"], "cuda")
    vb = nc.prepare_batches(nc.mkbatches(A, None, p.Y["valid"], BATCHSIZE, LAYERS), p.Y["valid"], "cuda")
    with pytest.raises(L.MrgcnError, match="masked"):
        nc.GraphedBatchEpoch(p.model, tb, vb, p.opt)
    mrgcn_amd.reset_stats()
    rows = list(nc.fit(p.model, tb, vb, p.opt, 2, poll=2, graphed=True))
    assert mrgcn_amd.stats().get("nc.batch_epoch.eager") == 2
    _check_rows(rows, p.g["fl_b3.rows"][:2])


# ---- the other ways in: an MRGCN, a shared feature matrix, a full batch, the reference's helpers ----------------------
@pytest.mark.parametrize("graphed", [False, True])
def test_an_mrgcn_takes_the_batches_as_model_of_batch(graphed):
    """`model(batch)` (mrgcn.py:182-248) is what the loop calls for an MRGCN: the featureless golden case behind the
    MRGCN class gives the same rows as the bare R-GCN (graphed: from the matching epoch, warm-up 1)."""
    from mrgcn_amd.models.mrgcn import MRGCN
    from mrgcn_amd.tasks import node_classification as nc
    from mrgcn_amd.train import ClipAdam
    p = Problem("fl_b3")
    g = p.g
    modules = [(0, HIDDEN, "mrgcn", torch.nn.ReLU()), (HIDDEN, CLASSES, "mrgcn", None)]
    _, A = util.load_graph("graph_small")
    N = A.shape[0]
    model = MRGCN(modules, [], A.shape[1] // N, N, num_bases=3, p_dropout=0.0, featureless=True, bias=True)
    model.rgcn.load_state_dict({k[11:]: torch.from_numpy(np.array(g[k])) for k in g.files if k.startswith("fl_b3.init.")})
    model.rgcn.cuda()
    assert hasattr(model, "rgcn") and type(p.batches["train"][0]).__name__ == "MiniBatch"
    opt = ClipAdam([q for q in model.parameters() if q.requires_grad], lr=0.01, max_norm=1.0, capturable=True)
    rows = list(nc.fit(model, p.batches["train"], p.batches["valid"], opt, 3, poll=2, graphed=graphed, warmup=1))
    _check_rows(rows, g["fl_b3.rows"][1:4] if graphed else g["fl_b3.rows"][:3])


def test_a_shared_feature_matrix_gives_the_rows_of_per_batch_subsets():
    """`prepare_batches(..., X_full=)`: masked batches built without features, every one reading the whole [N, K]
    matrix on the device — the featured golden case, row for row."""
    from mrgcn_amd.tasks import node_classification as nc
    p = Problem("ft_b3")
    X = torch.from_numpy(np.array(p.g["X_full"])).cuda()
    share = {}
    tb = nc.prepare_batches(nc.mkbatches(None, None, p.Y["train"], BATCHSIZE, LAYERS, plan=p.plan), p.Y["train"], "cuda",
                            X_full=X, share=share)
    vb = nc.prepare_batches(nc.mkbatches(None, None, p.Y["valid"], BATCHSIZE, LAYERS, plan=p.plan), p.Y["valid"], "cuda",
                            X_full=X, share=share)
    assert all(b._mrgcn_nc["X0"] is X for b in tb + vb)
    # equal positions, one tensor — across the two calls too: lengths 8, 8, 7 and 8, 3
    assert tb[0]._mrgcn_nc["pos"] is tb[1]._mrgcn_nc["pos"] is vb[0]._mrgcn_nc["pos"] and len(share) == 3
    rows = list(nc.fit(p.model, tb, vb, p.opt, 3, poll=4, graphed=False))
    _check_rows(rows, p.g["ft_b3.rows"][:3])
    with pytest.raises(Exception, match="X_full"):
        nc.prepare_batches(tb, p.Y["train"], "cuda", X_full=X.cpu())


def test_one_full_batch_trains_like_the_full_batch_loop():
    """batchsize 0: ONE FullBatch over every node (:346-349), its label pair the labelled nodes' global rows.  `fit`
    over it yields the rows of `train.fit` on the same model, forward and labels (rtol 1e-5, atol 1e-6: two paths of
    the same arithmetic, the loss summed in another order), eager and replayed."""
    from mrgcn_amd import train as T
    from mrgcn_amd.data.batch import FullBatch
    from mrgcn_amd.tasks import node_classification as nc
    _, A = util.load_graph("graph_small")
    runs = {}
    for kind in ("full", "eager", "graphed"):
        p = Problem("fl_b3", splits=())
        if kind == "full":
            At = util.coo_tensor(A, "ref_int8", "cuda")
            pair = {s: tuple(torch.from_numpy(a).cuda() for a in nc.batch_targets(np.arange(A.shape[0]), p.Y[s]))
                    for s in ("train", "valid")}
            T.train_step(p.model, lambda: p.model(None, At), pair["train"][0], pair["train"][1], p.opt)   # (the warm-up)
            runs[kind] = list(T.fit(p.model, lambda: p.model(None, At), pair["train"], pair["valid"], p.opt, 3, poll=2,
                                    graphed=False))
            continue
        tb = nc.prepare_batches(nc.mkbatches(A, None, p.Y["train"], 0, LAYERS), p.Y["train"], "cuda")
        vb = nc.prepare_batches(nc.mkbatches(A, None, p.Y["valid"], 0, LAYERS), p.Y["valid"], "cuda")
        assert len(tb) == len(vb) == 1 and isinstance(tb[0], FullBatch) and tb[0].A.is_cuda
        assert np.array_equal(_np(tb[0]._mrgcn_nc["pos"]), np.sort(p.g["train.nodes"]))
        if kind == "eager":
            nc.BatchEpoch(p.model, tb, vb, p.opt)()   # (the warm-up epoch of the other two)
        runs[kind] = list(nc.fit(p.model, tb, vb, p.opt, 3, poll=2, graphed=(kind == "graphed"), warmup=1))
    for kind in ("eager", "graphed"):
        print(kind, runs[kind], runs["full"])
        np.testing.assert_allclose(np.asarray(runs[kind]), np.asarray(runs["full"]), **PATHS)


def test_the_references_loss_and_accuracy_signatures():
    """`categorical_crossentropy(Y_hat, Y, criterion)` / `categorical_accuracy(Y_hat, Y)` with the scipy label matrix
    (:432-444) against float64 numpy; and `train_epoch`: a DeviceEarlyStop's state lives across calls, a host EarlyStop
    (a configuration that would start anew every call) is refused."""
    from mrgcn_amd import _lib as L
    from mrgcn_amd import train as T
    from mrgcn_amd.tasks import node_classification as nc
    p = Problem("fl_b3")
    _, A = util.load_graph("graph_small")
    with torch.no_grad():
        Y_hat = p.model(None, util.coo_tensor(A, "ref_int8", "cuda"))
    Y = p.Y["train"]
    idx, tgt = Y.nonzero()
    z = _np(Y_hat).astype(np.float64)[idx]
    want = float((np.log(np.exp(z - z.max(1, keepdims=True)).sum(1)) + z.max(1) - z[np.arange(len(idx)), tgt]).mean())
    loss = nc.categorical_crossentropy(Y_hat, Y, torch.nn.CrossEntropyLoss())
    np.testing.assert_allclose(float(loss), want, rtol=1e-5, atol=1e-5)
    acc, labels, targets = nc.categorical_accuracy(Y_hat, Y)
    assert np.array_equal(_np(labels), z.argmax(1)) and np.array_equal(_np(targets), tgt)
    assert np.float32(float(acc)) == np.float32((z.argmax(1) == tgt).mean(dtype=np.float32))
    # train_epoch
    with pytest.raises(L.MrgcnError, match="DeviceEarlyStop"):
        nc.train_epoch(p.model, p.batches["train"], p.batches["valid"], p.opt, early_stop=T.EarlyStop(2, 10.0, 0))
    row = nc.train_epoch(p.model, p.batches["train"], p.batches["valid"], p.opt)
    np.testing.assert_allclose(_np(row)[[0, 2]], p.g["fl_b3.rows"][0][[0, 2]], **LOSS)
    stopper = T.DeviceEarlyStop(p.model, p.opt, 2, 10.0, 0)
    for k in (1, 2, 3):
        nc.train_epoch(p.model, p.batches["train"], p.batches["valid"], p.opt, early_stop=stopper)
        assert stopper.records == k
    assert stopper.poll() and stopper.best_record == 1
