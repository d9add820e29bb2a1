"""Validation and early stopping inside the replayed epoch: the evaluation kernel against float64 numpy, the record
kernel against traces of the reference's EarlyStop, the flag-switched snapshot copy, and `fit` end to end.

Loss tolerance: rtol = atol = 1e-5, what tests/test_gpu_layers.py holds the training loss kernel to.  Counts, labels
and copies are exact.  The reference class keeps counting after `stop` (its loop never records again); the device
state is latched there, so the traces are compared up to their first stop record and the state must then stand still.
Scores are non-negative (the reference's `best_score < 0` sentinel makes negative scores another regime)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu

RTOL = ATOL = 1e-5
TRACES = np.load(os.path.join(util.GOLDEN, "early_stop_traces.npz"))
NAMES = [str(n) for n in TRACES["names"]]
SINGLE = 4096   # csrc/early_stop.hip: kEvalSingle (asserted below)


def _np(t):
    return t.detach().cpu().numpy()


# ---- 1. evaluation kernel -------------------------------------------------------------------------------------------
def _eval_ref(z, idx, tgt):
    rows = z.astype(np.float64)[idx]
    mx = rows.max(axis=1, keepdims=True)
    lse = np.log(np.exp(rows - mx).sum(axis=1)) + mx[:, 0]
    loss = (lse - rows[np.arange(len(idx)), tgt]).mean()
    labels = rows.argmax(axis=1)   # (numpy: the first of equal values)
    return loss, labels, int((labels == tgt).sum())


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025, SINGLE, SINGLE + 1])
@pytest.mark.parametrize("C_", [1, 2, 11, 33, 200])
def test_eval_kernel_matches_float64_numpy(C_, n, pad):
    from mrgcn_amd import _lib as L
    from mrgcn_amd.train import evaluate
    assert int(L.load().mrgcn_xent_eval_single_block_rows()) == SINGLE
    rng = np.random.default_rng(1000 * C_ + n + pad)
    N = max(5, n // 2 + 3)     # fewer rows than labels: idx repeats
    buf = ((rng.random((N, C_ + pad), dtype=np.float32) * 2 - 1) * 80).astype(np.float32)
    idx = rng.integers(0, N, n)
    tgt = rng.integers(0, C_, n)
    want_loss, want_labels, want_correct = _eval_ref(buf[:, :C_], idx, tgt)
    assert np.isfinite(want_loss)
    logits = torch.from_numpy(buf).cuda()[:, :C_]
    assert logits.stride(0) == C_ + pad
    i_d, t_d = torch.from_numpy(idx).cuda(), torch.from_numpy(tgt).cuda()
    loss, acc, labels = evaluate(logits, i_d, t_d, want_labels=True)
    loss2, acc2 = evaluate(logits, i_d, t_d)
    torch.cuda.synchronize()
    print(f"C={C_} n={n} pad={pad}: loss {float(loss)!r} want {want_loss!r}")
    assert np.isfinite(float(loss))
    np.testing.assert_allclose(float(loss), want_loss, rtol=RTOL, atol=ATOL)
    assert np.array_equal(_np(labels), want_labels)
    assert float(acc) == float(np.float32(want_correct) / np.float32(n))
    assert _np(loss).tobytes() == _np(loss2).tobytes() and float(acc) == float(acc2)   # the same bits on every call


def test_eval_kernel_ties_go_to_the_lowest_class():
    from mrgcn_amd.train import evaluate
    rng = np.random.default_rng(7)
    z = rng.integers(0, 3, (500, 6)).astype(np.float32)   # small integers: most rows tie at their maximum
    z[0] = 2.0
    idx = np.arange(500)
    tgt = rng.integers(0, 6, 500)
    assert (np.sort(z, axis=1)[:, -1] == np.sort(z, axis=1)[:, -2]).sum() > 100
    want_loss, want_labels, want_correct = _eval_ref(z, idx, tgt)
    loss, acc, labels = evaluate(torch.from_numpy(z).cuda(), torch.from_numpy(idx).cuda(), torch.from_numpy(tgt).cuda(),
                                 want_labels=True)
    assert np.array_equal(_np(labels), want_labels) and _np(labels)[0] == 0
    assert np.array_equal(_np(labels), _np(torch.from_numpy(z).max(dim=1)[1]))
    assert float(acc) == float(np.float32(want_correct) / np.float32(500))
    np.testing.assert_allclose(float(loss), want_loss, rtol=RTOL, atol=ATOL)


# ---- 2. record kernel -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_record_kernel_replays_the_reference_trace(name):
    from mrgcn_amd.train import _StopState
    patience, tolerance, delay = TRACES[f"{name}.config"]
    scores, want = TRACES[f"{name}.scores"], TRACES[f"{name}.records"]
    st = _StopState("cuda", int(patience), float(tolerance), int(delay))
    ring = torch.full((4, 4), -7.0, device="cuda")
    s0 = st.read()
    assert (s0.best_score, s0.records, s0.best_record, s0.stop, s0.improved) == (-1.0, 0, 0, 0, 0)
    stopped_at = None
    best_record = 0
    for k, score in enumerate(scores):
        assert np.isnan(score) or float(np.float32(score)) == score   # (the golden's scores are float32 values)
        s_d = torch.tensor(float(score), dtype=torch.float32, device="cuda")
        st.record(s_d, ring, (s_d, None, s_d, None))
        got = st.read()
        best, pat, stop, updated = want[k]
        best_record = k + 1 if updated else best_record
        assert np.array_equal(np.float64(got.best_score), best, equal_nan=True), (name, k)
        assert (got.patience, got.stop, got.improved) == (int(pat), int(stop), int(updated)), (name, k)
        assert (got.records, got.best_record) == (k + 1, best_record), (name, k)
        row = _np(ring)[k % 4]
        assert np.array_equal(row, np.float32([score, -1, score, -1]), equal_nan=True), (name, k)
        if stop:
            stopped_at = k
            break
    if stopped_at is None:
        return
    frozen, ring0 = bytes(st.read()), _np(ring).copy()
    for j in range(10):   # lower scores after the stop: nothing moves, not even the ring
        st.record(torch.tensor(1e-3 / (j + 1), dtype=torch.float32, device="cuda"), ring,
                  (torch.zeros((), device="cuda"),) * 4)
        assert bytes(st.read()) == frozen, (name, j)
    assert np.array_equal(_np(ring), ring0, equal_nan=True)


# ---- 3. snapshot_if ---------------------------------------------------------------------------------------------------
def _snapshot_case():
    from mrgcn_amd import _lib as L
    sizes = [0, 4 * 1, 4 * 3, 4 * 4, 4 * 5, 4 * ((1 << 20) + 7), 8]   # floats of 0, 1, 3, 4, 5, 2^20 + 7; one int64
    # offsets inside 16 bytes, source and destination: equal ones (16-byte loads) and different ones
    mis = [(4, 4), (12, 4), (4, 8), (8, 8), (3, 7), (4, 12), (8, 8)]
    block = int(L.load().mrgcn_snapshot_block_bytes())
    rng = np.random.default_rng(3)
    src_off, dst_off, so, do = [], [], 0, 0
    for nbytes, (ms, md) in zip(sizes, mis):
        so = (so + 48 + 15) // 16 * 16 + ms     # >= 32 sentinel bytes between entries
        do = (do + 80 + 15) // 16 * 16 + md
        src_off.append(so)
        dst_off.append(do)
        so, do = so + nbytes, do + nbytes
    src = rng.integers(0, 256, so + 64, dtype=np.uint8)
    dst = rng.integers(0, 256, do + 64, dtype=np.uint8)
    s_d, d_d = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    assert s_d.data_ptr() % 16 == 0 and d_d.data_ptr() % 16 == 0
    table = (L.CopyEntry * len(sizes))()
    blocks = 0
    for i, nbytes in enumerate(sizes):
        table[i] = L.CopyEntry(s_d.data_ptr() + src_off[i], d_d.data_ptr() + dst_off[i], nbytes, blocks)
        blocks += (nbytes + block - 1) // block
    t_d = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).cuda()
    return sizes, src_off, dst_off, src, dst, s_d, d_d, t_d, blocks


def test_snapshot_if_copies_only_behind_a_set_flag_and_restores():
    from mrgcn_amd import _lib as L
    lib = L.load()
    sizes, src_off, dst_off, src, dst, s_d, d_d, t_d, blocks = _snapshot_case()
    stream = torch.cuda.current_stream().cuda_stream
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")

    def go(flag_ptr, restore):
        L.check(lib.mrgcn_snapshot_if(flag_ptr, t_d.data_ptr(), len(sizes), blocks, restore, stream), "snapshot_if")
        torch.cuda.synchronize()
    go(flag.data_ptr(), 0)
    assert np.array_equal(_np(d_d), dst) and np.array_equal(_np(s_d), src)   # flag 0: every byte as it was
    flag.fill_(1)
    go(flag.data_ptr(), 0)
    want = dst.copy()
    for nbytes, so, do in zip(sizes, src_off, dst_off):
        want[do:do + nbytes] = src[so:so + nbytes]
    assert np.array_equal(_np(d_d), want)    # the entries bitwise, every byte between them (sentinels) intact
    assert np.array_equal(_np(s_d), src)
    # restore: the sources are overwritten, then brought back from the copies (flag forced: NULL)
    s_d.copy_(torch.from_numpy(np.random.default_rng(4).integers(0, 256, len(src), dtype=np.uint8)))
    scrambled = _np(s_d).copy()
    go(None, 1)
    back = scrambled.copy()
    for nbytes, so, do in zip(sizes, src_off, dst_off):
        back[so:so + nbytes] = src[so:so + nbytes]
    assert np.array_equal(_np(s_d), back) and np.array_equal(_np(d_d), want)
    flag.zero_()
    s_d.copy_(torch.from_numpy(scrambled))
    go(flag.data_ptr(), 1)    # a restore behind a clear flag does nothing either
    assert np.array_equal(_np(s_d), scrambled)


# ---- 4. end to end ----------------------------------------------------------------------------------------------------
CASE = "rgcn_small_fl_b3_bias_norm_f32"


def _problem(name=CASE, p_dropout=0.0, lr=0.01):
    from mrgcn_amd.train import ClipAdam
    c = util.load_case(name)
    model, _ = util.build_rgcn_from_case(c, "cuda")
    util.load_state_from_case(model, c)
    model = model.cuda()
    model.p_dropout = p_dropout
    g, A_csr = util.load_graph(util.graph_of_case(name))
    A = util.coo_tensor(A_csr, str(c["value_mode"]), "cuda")
    X = None if bool(c["meta.featureless"]) else torch.from_numpy(c["X"]).cuda()
    idx, tgt = torch.from_numpy(c["labels_idx"]).cuda(), torch.from_numpy(c["labels_y"]).cuda()
    assert idx.numel() >= 8
    train = (idx[0::2].contiguous(), tgt[0::2].contiguous())
    valid = (idx[1::2].contiguous(), tgt[1::2].contiguous())
    opt = ClipAdam(list(model.parameters()), lr=lr, max_norm=1.0, capturable=True)
    return model, (lambda: model(X, A)), train, valid, opt


def _live_state(model, opt):
    out = [p.detach().clone() for p in model.parameters()]
    for p in model.parameters():
        out += [v.clone() for v in opt.state[p].values() if torch.is_tensor(v)]
    for ent in opt._dev_step.values():
        out += [ent[0].clone(), ent[1].clone()]
    return out


def _bitwise(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and _np(x).tobytes() == _np(y).tobytes() for x, y in zip(a, b))


def test_fit_graphed_poll1_stops_at_record_6_and_restores_record_3_bitwise():
    """tolerance 10, delay 2, patience 3: records 1-2 are swallowed, record 3 sets the best score, nothing can beat it
    by 10, records 4-6 spend the patience — whatever the float noise."""
    from mrgcn_amd.train import EarlyStop, evaluate, fit
    model, fwd, train, valid, opt = _problem()
    rows, clones = [], {}
    for row in fit(model, fwd, train, valid, opt, 20, early_stop=EarlyStop(3, 10.0, 2), poll=1, graphed=True, warmup=1):
        rows.append(row)
        clones[row[0]] = _live_state(model, opt)
    assert [r[0] for r in rows] == [1, 2, 3, 4, 5, 6]
    assert model.training
    live = _live_state(model, opt)
    assert _bitwise(live, clones[3])
    assert not _bitwise(live, clones[6]) and not _bitwise(clones[2], clones[3])
    assert int(next(iter(opt._dev_step.values()))[0].item()) == 1 + 3    # one warm-up step, three epochs
    # every row's validation figures: an eager evaluation of that epoch's parameters
    nparam = len(list(model.parameters()))
    model.eval()
    for epoch, _, _, val_loss, val_acc in rows:
        with torch.no_grad():
            for p, cl in zip(model.parameters(), clones[epoch][:nparam]):
                p.copy_(cl)
            loss, acc = evaluate(fwd(), valid[0], valid[1])
        print(f"epoch {epoch}: val_loss {val_loss!r} eager {float(loss)!r}  val_acc {val_acc!r} eager {float(acc)!r}")
        np.testing.assert_allclose(val_loss, float(loss), rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(val_acc, float(acc), rtol=RTOL, atol=ATOL)
    assert all(np.isfinite(r[1:]).all() and 0 <= r[2] <= 1 and 0 <= r[4] <= 1 for r in rows)


def test_fit_graphed_poll4_yields_the_same_six_rows_and_its_own_record_3(monkeypatch):
    """The poll after epoch 8 finds the stop of record 6: epochs 7 and 8 ran and left nothing behind.  Every replay
    inside fit is followed by a clone of the live state, so the restored state is compared with what this run held
    after epoch 3 (training is not bitwise reproducible between runs)."""
    from mrgcn_amd import train as T
    model, fwd, train, valid, opt = _problem()
    T.train_step(model, fwd, train[0], train[1], opt)
    stopper = T.DeviceEarlyStop(model, opt, 3, 10.0, 2)
    clones, replay = [], T.GraphedTrainEvalStep.__call__

    def replay_then_clone(self):
        out = replay(self)
        clones.append(_live_state(model, opt))
        return out
    monkeypatch.setattr(T.GraphedTrainEvalStep, "__call__", replay_then_clone)
    rows = list(T.fit(model, fwd, train, valid, opt, 20, early_stop=stopper, poll=4, graphed=True, warmup=1))
    assert [r[0] for r in rows] == [1, 2, 3, 4, 5, 6]
    assert (stopper.records, stopper.best_record, stopper.poll()) == (6, 3, True)
    assert stopper.best_score == np.float64(np.float32(rows[2][3]))
    assert len(clones) == 8       # two epochs ran past the stop
    live = _live_state(model, opt)
    assert _bitwise(live, clones[2])
    assert not _bitwise(clones[2], clones[5]) and not _bitwise(clones[5], clones[7]) and not _bitwise(live, clones[7])
    assert _bitwise([t for t in stopper._live], [t for t in stopper._snap])
    assert int(next(iter(opt._dev_step.values()))[0].item()) == 2 + 3   # the eager step, one warm-up step, three epochs


def test_replay_goes_on_after_restore():
    from mrgcn_amd.train import EarlyStop, GraphedTrainEvalStep
    model, fwd, train, valid, opt = _problem()
    step = GraphedTrainEvalStep(model, fwd, train[0], train[1], opt, valid=valid, early_stop=EarlyStop(3, 10.0, 2),
                                warmup=2)
    assert step.early_stop.records == 0     # the warm-up left no trace
    for _ in range(7):
        step()
    assert step.early_stop.poll() and step.early_stop.records == 6
    gen = opt._state_gen
    assert step.early_stop.restore_()
    assert opt._state_gen == gen
    values = step.step()      # no _state_gen error: the graph still owns the tensors it was captured on
    assert np.isfinite(float(values[0])) and np.isfinite(float(values[2]))
    assert step.early_stop.records == 6


def test_fit_eager_stops_at_the_same_record():
    from mrgcn_amd.train import DeviceEarlyStop, fit, train_step
    model, fwd, train, valid, opt = _problem()
    train_step(model, fwd, train[0], train[1], opt)
    stopper = DeviceEarlyStop(model, opt, 3, 10.0, 2)
    clones = []

    def forward_then_clone():   # two forwards an epoch: the even calls see the state the epoch before left
        if len(clones) % 2 == 0:
            clones.append(_live_state(model, opt))
        else:
            clones.append(None)
        return fwd()
    rows = list(fit(model, forward_then_clone, train, valid, opt, 20, early_stop=stopper, poll=4, graphed=False))
    assert [r[0] for r in rows] == [1, 2, 3, 4, 5, 6] and stopper.best_record == 3
    assert len(clones) == 16      # eight epochs: two past the stop
    live = _live_state(model, opt)
    assert _bitwise(live, clones[6])          # in front of epoch 4: what epoch 3 left
    assert not _bitwise(live, clones[8]) and not _bitwise(live, clones[14])
    assert int(next(iter(opt._dev_step.values()))[0].item()) == 1 + 3     # the eager step, three epochs


def test_fit_starts_a_supplied_stopper_at_record_0():
    """Graphed or not: what a DeviceEarlyStop recorded before the run is discarded, the first row is epoch 1."""
    from mrgcn_amd.train import DeviceEarlyStop, fit, train_step
    for graphed in (False, True):
        model, fwd, train, valid, opt = _problem()
        train_step(model, fwd, train[0], train[1], opt)
        stopper = DeviceEarlyStop(model, opt, 3, 10.0, 0)
        for _ in range(2):
            stopper.record(torch.ones((), device="cuda"))
        assert stopper.records == 2
        rows = list(fit(model, fwd, train, valid, opt, 2, early_stop=stopper, poll=2, graphed=graphed, warmup=1))
        assert [r[0] for r in rows] == [1, 2] and (stopper.records, stopper.best_record) == (2, 1)


def _bn_problem(init=True):
    from mrgcn_amd.train import ClipAdam
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.BatchNorm1d(7)).cuda()
    opt = ClipAdam(list(model.parameters()), lr=0.01, capturable=True)
    if init:
        opt.init_state()     # zero moments and the device step counter, as the first step would leave them
    return model, opt


def test_first_step_after_init_state_is_the_first_step_without_it():
    """ClipAdam.init_state() allocates what step() would: the same gradients then give the same parameters, moments,
    step counter and bias corrections, bit for bit (the squared norm behind the clip coefficient summed in block order,
    the deterministic mode; the Adam update is elementwise)."""
    outs = []
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        for seeded in (False, True):
            model, opt = _bn_problem(init=seeded)
            g = torch.Generator("cuda").manual_seed(3)
            for _ in range(2):
                for p in model.parameters():
                    p.grad = torch.randn(p.shape, device="cuda", generator=g)
                opt.step()
            assert int(next(iter(opt._dev_step.values()))[0].item()) == 2
            outs.append(_live_state(model, opt))
    finally:
        torch.use_deterministic_algorithms(was)
    assert _bitwise(outs[0], outs[1])


def test_fit_that_never_stops_keeps_the_last_epoch():
    from mrgcn_amd.train import DeviceEarlyStop, fit, train_step
    model, fwd, train, valid, opt = _problem()
    train_step(model, fwd, train[0], train[1], opt)
    stopper = DeviceEarlyStop(model, opt, 3, 10.0, 0)
    rows = list(fit(model, fwd, train, valid, opt, 3, early_stop=stopper, poll=2, graphed=False))
    assert [r[0] for r in rows] == [1, 2, 3] and not stopper.poll() and stopper.best_record == 1
    assert int(next(iter(opt._dev_step.values()))[0].item()) == 1 + 3     # nothing restored: the third epoch's state
    assert stopper.restore_()
    assert int(next(iter(opt._dev_step.values()))[0].item()) == 1 + 1


def test_snapshot_covers_module_buffers():
    """BatchNorm's running statistics and batch count are part of the reference's best_weights (a state_dict)."""
    from mrgcn_amd.train import DeviceEarlyStop
    model, opt = _bn_problem()
    bn = model[1]
    stopper = DeviceEarlyStop(model, opt, 3, 0.0, 0)
    bn.running_mean.fill_(0.25)
    bn.num_batches_tracked.fill_(4)
    stopper.record(torch.full((), 1.0, device="cuda"))       # the first record: snapshot
    with torch.no_grad():
        bn.running_mean.fill_(9.0)
        bn.running_var.mul_(3.0)
        bn.num_batches_tracked.fill_(11)
        model[0].weight.add_(1.0)
    stopper.record(torch.full((), 2.0, device="cuda"))       # worse: the snapshot stays
    kept = [b.clone() for b in (bn.running_mean, bn.running_var, bn.num_batches_tracked)]
    assert stopper.restore_()
    assert float(bn.running_mean[0]) == 0.25 and int(bn.num_batches_tracked) == 4
    assert float(bn.running_var[0]) == 1.0 and not _bitwise(kept, [bn.running_mean, bn.running_var,
                                                                     bn.num_batches_tracked])


def test_state_dict_round_trip():
    from mrgcn_amd.train import DeviceEarlyStop
    model, opt = _bn_problem()
    stopper = DeviceEarlyStop(model, opt, 3, 0.0, 0)
    stopper.record(torch.full((), 1.0, device="cuda"))
    stopper.record(torch.full((), 2.0, device="cuda"))
    sd = stopper.state_dict()
    assert (sd["records"], sd["best_record"], sd["best_score"], sd["patience"], sd["stop"]) == (2, 1, 1.0, 2, 0)
    first = [p.detach().clone() for p in model.parameters()]
    with torch.no_grad():
        model[0].weight.add_(1.0)
    stopper.record(torch.full((), 0.5, device="cuda"))       # better: the snapshot moves on
    assert (stopper.records, stopper.best_record, stopper.best_score) == (3, 3, 0.5)
    stopper.load_state_dict(sd)
    assert stopper.state_dict(snapshot=False) == {k: v for k, v in sd.items() if k != "snapshot"}
    assert _bitwise(stopper._snap, sd["snapshot"])
    assert stopper.restore_() and _bitwise([p.detach() for p in model.parameters()], first)


def test_evaluate_refuses_host_index_tensors():
    from mrgcn_amd._lib import MrgcnError
    from mrgcn_amd.train import evaluate
    logits = torch.zeros((4, 3), device="cuda")
    idx, tgt = torch.arange(4), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(MrgcnError, match="on the device"):
        evaluate(logits, idx, tgt.cuda())
    with pytest.raises(MrgcnError, match="on the device"):
        evaluate(logits, idx.cuda(), tgt)


def test_fit_without_validation_yields_minus_one():
    from mrgcn_amd.train import fit
    model, fwd, train, valid, opt = _problem()
    rows = list(fit(model, fwd, train, None, opt, 5, poll=2, graphed=True, warmup=1))
    assert [r[0] for r in rows] == [1, 2, 3, 4, 5]
    assert all(r[3] == -1 and r[4] == -1 and np.isfinite(r[1]) for r in rows)


def test_the_validation_pass_runs_in_eval_mode():
    """p_dropout = 0.3 drawn on the device, lr = 0 (the parameters stand still), valid = train: the training and the
    validation loss differ on the same rows.  The model is in eval() mode under no_grad for the validation forward only,
    and in training mode again afterwards.  (Node dropout itself is drawn in eval() mode too — the reference's
    rgcn.py:78-83 calls the functional dropout without a mode, and RGCN restates that — so the validation loss is the
    loss of a forward with that pass's own masks: replayed here with those masks given explicitly.)"""
    from mrgcn_amd.train import evaluate, train_eval_step
    model, fwd, train, _, opt = _problem("rgcn_small_ft_b3_bias_norm_f32", p_dropout=0.3, lr=0.0)
    model.set_node_dropout("device", seed=5)
    model.train()
    modes = []

    def watched():
        modes.append((model.training, torch.is_grad_enabled()))
        return fwd()
    tl, ta, vl, va = train_eval_step(model, watched, train[0], train[1], opt, valid=train)
    assert modes == [(True, True), (False, False)] and model.training
    model.node_dropout_masks = [m.clone() for m in model.last_node_masks]   # the validation forward's masks
    with torch.no_grad():
        want, _ = evaluate(fwd(), train[0], train[1])
    model.node_dropout_masks = None
    print(f"train {float(tl)!r} valid {float(vl)!r} same masks again {float(want)!r}")
    np.testing.assert_allclose(float(vl), float(want), rtol=RTOL, atol=ATOL)
    assert abs(float(tl) - float(vl)) > 100 * (ATOL + RTOL * abs(float(vl)))
    model.eval()
    train_eval_step(model, watched, train[0], train[1], opt, valid=train)
    assert not model.training     # the mode the caller had is the mode it gets back


def test_device_early_stop_needs_the_optimizer_state():
    from mrgcn_amd._lib import MrgcnError
    from mrgcn_amd.train import DeviceEarlyStop
    model, fwd, train, valid, opt = _problem()
    with pytest.raises(MrgcnError, match="first optimizer step"):
        DeviceEarlyStop(model, opt, 3, 0.01)
