"""csrc/nc_batches.hip at the C ABI: the fused loss launch of a mini-batch (mrgcn_xent_train_eval_rows_f32) and the
epoch's means over the batches' slots (mrgcn_batch_means_f32).

The fused launch against what it replaces: its gradient rows are the BYTES mrgcn_softmax_xent_rows_f32 writes (the
backward consumes them unchanged), its correct count and labels are `train.evaluate`'s, its loss is held to float64
numpy at rtol = atol = 1e-5 (the tolerance tests/test_gpu_early_stop.py holds the evaluation kernel to), the slot is
{loss, float32(correct) / float32(n)}, and two calls write the same bytes.  Shapes: every load form of the row and
both sides of their borders (scalar loads below 4 classes, 16-byte pieces for 4..16, the loop above), one lane, one
wave and its neighbours, several rows per thread, the single-block limit and one row more (block parts and the final
launch), rows padded by 0 and by 3 floats, indices that repeat, and one row of equal logits.

The means against a sequential float64 sum in slot order, bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL = ATOL = 1e-5
SINGLE = 4096   # csrc/nc_batches.hip: kNcSingle (asserted below)


def _np(t):
    return t.detach().cpu().numpy()


def _ref(z, idx, tgt):
    rows = z.astype(np.float64)[idx]
    mx = rows.max(axis=1, keepdims=True)
    lse = np.log(np.exp(rows - mx).sum(axis=1)) + mx[:, 0]
    loss = (lse - rows[np.arange(len(idx)), tgt]).mean()
    labels = rows.argmax(axis=1)   # (numpy: the first of equal values)
    return loss, labels, int((labels == tgt).sum())


def _fused(logits, idx, tgt):
    from mrgcn_amd.tasks.node_classification import xent_train_eval
    n, C_ = idx.numel(), logits.shape[1]
    drows = torch.full((n, C_), 7.0, dtype=torch.float32, device="cuda")
    labels = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    slot = torch.full((2,), -7.0, dtype=torch.float32, device="cuda")
    loss, correct = xent_train_eval(logits, idx, tgt, drows=drows, labels=labels, slot=slot)
    return loss, correct, drows, labels, slot


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025, SINGLE, SINGLE + 1])
@pytest.mark.parametrize("C_", [1, 2, 3, 4, 5, 11, 16, 17, 33])
def test_fused_loss_against_the_two_launches_it_replaces(C_, n, pad):
    from mrgcn_amd import _lib as L
    from mrgcn_amd.train import _stream, evaluate
    lib = L.load()
    assert int(lib.mrgcn_xent_train_eval_single_block_rows()) == SINGLE
    rng = np.random.default_rng(1000 * C_ + n + pad)
    N = max(5, n // 2 + 3)     # fewer rows than labels: idx repeats
    buf = ((rng.random((N, C_ + pad), dtype=np.float32) * 2 - 1) * 80).astype(np.float32)
    buf[0, :] = 1.5            # one row of equal logits: the lowest class wins
    idx = rng.integers(0, N, n)
    idx[0] = 0
    tgt = rng.integers(0, C_, n)
    want_loss, want_labels, want_correct = _ref(buf[:, :C_], idx, tgt)
    assert np.isfinite(want_loss) and want_labels[0] == 0
    logits = torch.from_numpy(buf).cuda()[:, :C_]
    assert logits.stride(0) == C_ + pad
    i_d, t_d = torch.from_numpy(idx).cuda(), torch.from_numpy(tgt).cuda()

    loss, correct, drows, labels, slot = _fused(logits, i_d, t_d)
    # the gradient rows of the launch the training step used so far, byte for byte
    old_loss = torch.empty((), dtype=torch.float32, device="cuda")
    old_rows = torch.full((n, C_), 9.0, dtype=torch.float32, device="cuda")
    L.check(lib.mrgcn_softmax_xent_rows_f32(logits.data_ptr(), logits.stride(0), C_, i_d.data_ptr(), t_d.data_ptr(), n,
                                            old_loss.data_ptr(), old_rows.data_ptr(), _stream(logits.device)))
    e_loss, e_acc, e_labels = evaluate(logits, i_d, t_d, want_labels=True)
    torch.cuda.synchronize()
    print(f"C={C_} n={n} pad={pad}: loss {float(loss)!r} float64 {want_loss!r} rows-kernel {float(old_loss)!r} "
          f"eval-kernel {float(e_loss)!r}")
    assert _np(drows).tobytes() == _np(old_rows).tobytes()
    assert np.array_equal(_np(labels), _np(e_labels)) and np.array_equal(_np(labels), want_labels)
    assert int(correct) == want_correct
    assert float(e_acc) == float(np.float32(want_correct) / np.float32(n))
    assert np.isfinite(float(loss))
    np.testing.assert_allclose(float(loss), want_loss, rtol=RTOL, atol=ATOL)
    # the evaluation kernel on the same logits: the same per-row arithmetic, another block shape for the float64 sum
    np.testing.assert_allclose(float(loss), float(e_loss), rtol=RTOL, atol=ATOL)
    # the slot: the loss's own bits, and correct / n as evaluate() divides them
    assert _np(slot)[0:1].tobytes() == _np(loss).tobytes()
    assert _np(slot)[1:2].tobytes() == np.float32(np.float32(want_correct) / np.float32(n)).tobytes()
    assert _np(slot)[1:2].tobytes() == _np(e_acc).tobytes()
    # the same bytes on a second call
    again = _fused(logits, i_d, t_d)
    torch.cuda.synchronize()
    for a, b in zip((loss, correct, drows, labels, slot), again):
        assert _np(a).tobytes() == _np(b).tobytes()


@pytest.mark.parametrize("C_", [3, 8, 20])
def test_nullable_outputs_and_a_target_outside_the_classes(C_):
    """Without gradient rows, labels and slot the launch writes loss and count only (an evaluation batch); a target
    outside [0, C) poisons the loss and reads nothing, the rows of the gradient stay softmax / n, the count skips it."""
    from mrgcn_amd.tasks.node_classification import xent_train_eval
    rng = np.random.default_rng(C_)
    n = 70
    z = rng.standard_normal((n, C_)).astype(np.float32)
    idx, tgt = np.arange(n), rng.integers(0, C_, n)
    want_loss, want_labels, want_correct = _ref(z, idx, tgt)
    zd, i_d, t_d = torch.from_numpy(z).cuda(), torch.from_numpy(idx).cuda(), torch.from_numpy(tgt).cuda()
    loss, correct = xent_train_eval(zd, i_d, t_d)
    full = _fused(zd, i_d, t_d)
    assert _np(loss).tobytes() == _np(full[0]).tobytes() and int(correct) == int(full[1]) == want_correct
    np.testing.assert_allclose(float(loss), want_loss, rtol=RTOL, atol=ATOL)
    bad = tgt.copy()
    bad[5], bad[6] = C_, -1
    loss_b, correct_b, drows_b, labels_b, slot_b = _fused(zd, i_d, torch.from_numpy(bad).cuda())
    assert np.isnan(float(loss_b)) and np.isnan(_np(slot_b)[0])
    assert np.array_equal(_np(labels_b), want_labels)
    assert int(correct_b) == int((want_labels == bad).sum())
    p = np.exp(z.astype(np.float64) - z.astype(np.float64).max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    np.testing.assert_allclose(_np(drows_b)[5:7], p[5:7] / n, rtol=1e-5, atol=1e-8)
    keep = np.ones(n, dtype=bool)
    keep[5:7] = False
    assert _np(drows_b)[keep].tobytes() == _np(full[2])[keep].tobytes()


def test_more_rows_than_one_block_need_the_workspace():
    from mrgcn_amd import _lib as L
    lib = L.load()
    n = SINGLE + 1
    z = torch.zeros((4, 4), device="cuda")
    idx = torch.zeros(n, dtype=torch.int64, device="cuda")
    out = torch.zeros(4, dtype=torch.int64, device="cuda")
    rc = lib.mrgcn_xent_train_eval_rows_f32(z.data_ptr(), 4, 4, idx.data_ptr(), idx.data_ptr(), n, out.data_ptr(), None,
                                            out[2:].data_ptr(), None, None, None, None)
    assert rc != 0 and b"workspace" in lib.mrgcn_last_error()


# ---- the epoch's means ----------------------------------------------------------------------------------------------
def _mirror(slots):
    """A sequential float64 sum in slot order, one division, one rounding."""
    out = []
    for k in (0, 1):
        t = 0.0
        for v in slots[:, k]:
            t += float(v)
        out.append(np.float32(t / len(slots)))
    return out


@pytest.mark.parametrize("n_valid", [0, 1, 5])
@pytest.mark.parametrize("n_train", [1, 2, 7, 64, 65, 300])
def test_batch_means_are_the_sequential_float64_mean_and_feed_the_record(n_train, n_valid):
    from mrgcn_amd import _lib as L
    from mrgcn_amd.tasks.node_classification import _batch_means
    from mrgcn_amd.train import _COUNT_ONLY, _StopState
    rng = np.random.default_rng(100 * n_train + n_valid)
    # (losses of very different sizes: a float32 sum, or another order, lands on other bits)
    tr = (rng.random((n_train, 2)) * 10.0 ** rng.integers(-3, 3, (n_train, 2))).astype(np.float32)
    va = (rng.random((max(n_valid, 1), 2)) * 10.0 ** rng.integers(-3, 3, (max(n_valid, 1), 2))).astype(np.float32)
    tr_d, va_d = torch.from_numpy(tr).cuda(), torch.from_numpy(va).cuda()
    row = torch.full((4,), 3.0, dtype=torch.float32, device="cuda")
    _batch_means(tr_d, n_train, va_d, n_valid, row)
    want = _mirror(tr) + (_mirror(va[:n_valid]) if n_valid else [np.float32(-1), np.float32(-1)])
    got = _np(row)
    assert got.tobytes() == np.asarray(want, dtype=np.float32).tobytes(), (got, want)
    if n_valid == 0:
        assert got[2] == -1 and got[3] == -1
        # (a NULL table is fine when there is nothing to read)
        L.check(L.load().mrgcn_batch_means_f32(tr_d.data_ptr(), n_train, None, 0, row.data_ptr(), None))
        torch.cuda.synchronize()
        assert _np(row).tobytes() == got.tobytes()
    # the row as the record takes it: into row `records % rows` of the ring, the counter one up
    counter = _StopState(torch.device("cuda", torch.cuda.current_device()), 1, 0.0, _COUNT_ONLY)
    ring = torch.zeros((3, 4), dtype=torch.float32, device="cuda")
    score = row[2:3] if n_valid else row[0:1]
    for k in range(4):
        counter.record_row(score, row, ring)
        assert int(counter.read().records) == k + 1
        assert _np(ring)[k % 3].tobytes() == got.tobytes()
    assert _np(ring)[1].tobytes() == got.tobytes() and _np(ring)[2].tobytes() == got.tobytes()


def test_batch_means_score_drives_the_early_stop_state():
    """`row4[2]`, the mean validation loss, is the score: patience 2 and a tolerance nothing beats stop at record 3."""
    from mrgcn_amd.tasks.node_classification import _batch_means
    from mrgcn_amd.train import _StopState
    state = _StopState(torch.device("cuda", torch.cuda.current_device()), 2, 10.0, 0)
    ring = torch.zeros((4, 4), dtype=torch.float32, device="cuda")
    row = torch.zeros(4, dtype=torch.float32, device="cuda")
    tr = torch.tensor([[1.0, 0.5]], device="cuda")
    for k, v in enumerate((2.0, 1.5, 1.25, 1.0)):
        va = torch.tensor([[v, 0.25], [v + 1, 0.75]], device="cuda")
        _batch_means(tr, 1, va, 2, row)
        state.record_row(row[2:3], row, ring)
    st = state.read()
    assert (st.records, st.best_record, st.stop) == (3, 1, 1) and st.best_score == 2.5
    assert _np(ring)[:3, 2].tolist() == [2.5, 2.0, 1.75] and _np(ring)[3].tolist() == [0, 0, 0, 0]
