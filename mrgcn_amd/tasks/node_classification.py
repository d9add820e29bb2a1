"""Mini-batch node classification — the run loop of `mrgcn/tasks/node_classification.py:112-310` (`mkbatches`
:329-351, the loop over `train_batches` :154-204, `eval_model` :229-256, `test_model` :258-310) on batches that are
built ONCE and reused every epoch (:128-143), with nothing read back per batch: a batch's loss, its compact gradient
rows and its accuracy come out of one launch (csrc/nc_batches.hip), the per-batch values wait in a device table, the
epoch's row is their unweighted mean (`np.mean(loss_lst)`, :203-204, :253-254), and the early stop on the validation
loss and the snapshot of the best state are `mrgcn_amd.train`'s device records.  An epoch is then a fixed,
allocation-stable sequence of launches, which `GraphedBatchEpoch` captures into one hipGraph.

Masked batches (`MiniBatch(plan=...)`, csrc/masked.hip) are the path this is built for; the reference's slice batches
run through the eager epoch.  `mk_target_matrices`, `build_dataset`, `build_model` and `run` (configuration, logging,
TSV writers) stay out of scope."""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib as L
from .. import train as T
from ..stats import bump

MAX_GRAPH_BATCHES = 160   # train + validation batches one captured epoch holds: the largest measured

_WS: dict = {}           # (device, stream) -> block partials of the fused loss launch (4 KiB each, as train._EVAL_WS)


def _stream(dev):
    return T._stream(dev)


# ---- the reference's helpers, on its signatures -----------------------------------------------------------------------
def _nonzero_pair(Y, device):
    idx, targets = Y.nonzero()
    return (torch.as_tensor(np.asarray(idx), dtype=torch.int64).to(device),
            torch.as_tensor(np.asarray(targets), dtype=torch.int64).to(device))


def categorical_crossentropy(Y_hat, Y, criterion=None):
    """node_classification.py:439-444 — `Y` the scipy label matrix of the rows of `Y_hat`; `criterion` is accepted
    and unused (the loss is nn.CrossEntropyLoss()'s, computed by `mrgcn_amd.train.categorical_crossentropy`)."""
    idx, targets = _nonzero_pair(Y, Y_hat.device)
    return T.categorical_crossentropy(Y_hat, idx, targets)


def categorical_accuracy(Y_hat, Y):
    """node_classification.py:432-437: (accuracy, labels, targets)."""
    idx, targets = _nonzero_pair(Y, Y_hat.device)
    return T.categorical_accuracy(Y_hat, idx, targets)


def mkbatches(A, X, Y, batchsize, num_layers, plan=None):
    """node_classification.py:329-351: `Y` the scipy label matrix of one split, `num_samples = len(Y.data)`, slices of
    `batchsize` over `Y.nonzero()[0]` in that order; more than one slice gives one `MiniBatch` per slice, otherwise one
    `FullBatch` over `np.arange(Y.shape[0])` (`batchsize <= 0`: one slice).  `plan` (the full graph's GraphPlan on the
    GPU): the mini-batches are masked batches on it, `MiniBatch(None, X, idx, num_layers, plan=plan)`, with `X` a host
    feature list or a `DeviceEncodings` as in `link_prediction.mkbatches`; without it the reference's slices of the
    scipy CSR `A`."""
    from ..data.batch import FullBatch, MiniBatch
    labelled = len(Y.data)
    step = labelled if batchsize <= 0 else int(batchsize)
    starts = range(0, labelled, step)
    if len(starts) <= 1:
        if A is None:
            raise L.MrgcnError("mkbatches: one slice is a FullBatch over the whole adjacency: pass A")
        return [FullBatch(A, X, np.arange(Y.shape[0]))]
    rows = Y.nonzero()[0]
    if plan is not None:
        return [MiniBatch(None, X, rows[at:at + step], num_layers, plan=plan) for at in starts]
    return [MiniBatch(A, X, rows[at:at + step], num_layers) for at in starts]


def batch_targets(node_index, Y):
    """`Y[batch.node_index].nonzero()` (:167, :433, :440) on the host: the rows inside the batch that carry a label and
    their classes, as int64 arrays."""
    if torch.is_tensor(node_index):
        node_index = node_index.cpu().numpy()
    pos, classes = Y[np.asarray(node_index)].nonzero()
    return np.ascontiguousarray(pos, dtype=np.int64), np.ascontiguousarray(classes, dtype=np.int64)


def _device(device):
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def prepare_batches(batches, Y, device="cuda", X_full=None, share=None):
    """Once per split (:128-143): the batches as tensors on `device`, and per batch the pair
    `Y[batch.node_index].nonzero()` — row positions inside the batch and classes, computed on the host by scipy
    exactly as the reference does per epoch — as int64 device tensors.  Batches with equal positions (every batch of a
    full slice: 0 .. batchsize-1) share ONE position tensor: the loss keeps its row flags under that tensor's identity
    (`train._label_flags`, eight entries), so an epoch over any number of batches uses two or three of them.
    `share`: a dict that carries the shared position tensors from one call to the next (the training, validation
    and test splits of one run); None keeps them to this call.
    `X_full` (a bare RGCN with given features on masked batches built with `X=None`): the whole float32 [N, K] feature
    matrix on the device, shared by every batch in place of a per-batch subset — the masked transform picks the rows
    of the outermost neighbours itself."""
    device = _device(device)
    share = {} if share is None else share
    if X_full is not None and not (torch.is_tensor(X_full) and X_full.is_cuda and X_full.dtype == torch.float32
                                   and X_full.dim() == 2 and X_full.is_contiguous()):
        raise L.MrgcnError("prepare_batches: X_full is a contiguous float32 [N, K] tensor on the device")
    for batch in batches:
        pos, classes = batch_targets(batch.node_index, Y)
        if pos.size == 0:
            raise L.MrgcnError("prepare_batches: a batch without a labelled node")
        if not torch.is_tensor(batch.node_index):
            batch.as_tensors_()
            kinds = {"relational": device}
            for ent in (batch.X[1:] if batch.X is not None else ()):
                kinds[ent[0]] = device
            batch.to(kinds)
        X0 = X_full
        if X0 is not None:
            from ..data.batch import A_BatchMasked
            if not isinstance(batch.A, (A_BatchMasked, torch.Tensor)):
                raise L.MrgcnError("prepare_batches: X_full goes with masked or full batches (slices take the subset)")
        elif batch.X is not None and torch.is_tensor(batch.X[0]) and batch.X[0].dim() == 2 and batch.X[0].shape[1] > 0:
            X0 = batch.X[0].to(device, torch.float32).contiguous()   # (a bare RGCN's input: the given feature columns)
        key = (device, pos.tobytes())
        if key not in share:
            share[key] = torch.from_numpy(pos).to(device)
        batch._mrgcn_nc = dict(device=device, pos=share[key], pos_host=pos,
                               tgt=torch.from_numpy(classes).to(device), tgt_host=classes, n=int(pos.size), X0=X0)
    return batches


def _state(batch):
    st = getattr(batch, "_mrgcn_nc", None)
    if st is None:
        raise L.MrgcnError("node_classification: the batch has no device state yet: prepare_batches(batches, Y, device)")
    return st


def _logits(model, batch):
    """`model(batch)` for an MRGCN (mrgcn.py:182-248); a bare RGCN takes the batch's given features and structure."""
    if hasattr(model, "rgcn"):
        return model(batch)
    return model(_state(batch)["X0"], batch.A)


def _is_fixed_structure(batch) -> bool:
    """Masked batches and full batches: no slices to cut, nothing built per forward."""
    from ..data.batch import A_BatchMasked
    return isinstance(batch.A, (A_BatchMasked, torch.Tensor))


# ---- the fused loss of one batch (csrc/nc_batches.hip) ----------------------------------------------------------------
def _workspace(lib, dev, n):
    if n <= int(lib.mrgcn_xent_train_eval_single_block_rows()):
        return 0
    key = (dev, _stream(dev))   # (block partials: one set per stream)
    t = _WS.get(key)
    if t is None:
        t = _WS[key] = torch.empty(int(lib.mrgcn_xent_train_eval_workspace()), dtype=torch.uint8, device=dev)
    return t.data_ptr()


def xent_train_eval(logits, idx, targets, drows=None, labels=None, slot=None):
    """One launch of mrgcn_xent_train_eval_rows_f32 on the rows `logits[idx]`: returns `(loss, correct)` as device
    scalars (float32, int64); `drows` (float32 [n, C], None: no gradient), `labels` (int64 [n]) and `slot` (float32
    [2] <- {loss, correct / n}) are written when given.  No host synchronisation; capturable."""
    if not (logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2):
        raise L.MrgcnError("xent_train_eval: float32 [N, C] logits on the device")
    if not (idx.dtype == torch.int64 and targets.dtype == torch.int64 and idx.numel() == targets.numel()
            and idx.numel() > 0 and idx.device == logits.device and targets.device == logits.device):
        raise L.MrgcnError("xent_train_eval: idx and targets are int64 tensors of one (non-zero) length on the device "
                           "of the logits")
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    idx, targets = idx.contiguous(), targets.contiguous()
    dev, n, Cn = logits.device, int(idx.numel()), int(logits.shape[1])
    for t, shape, dt, what in ((drows, (n, Cn), torch.float32, "drows"), (labels, (n,), torch.int64, "labels"),
                               (slot, (2,), torch.float32, "slot")):
        if t is not None and not (t.is_cuda and t.device == dev and t.dtype == dt and tuple(t.shape) == shape
                                  and t.is_contiguous()):
            raise L.MrgcnError(f"xent_train_eval: {what} is a contiguous {dt} {shape} tensor on the logits' device")
    lib = L.load()
    loss = torch.empty((), dtype=torch.float32, device=dev)
    correct = torch.empty((), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.mrgcn_xent_train_eval_rows_f32(
            logits.data_ptr(), logits.stride(0), Cn, idx.data_ptr(), targets.data_ptr(), n, loss.data_ptr(),
            drows.data_ptr() if drows is not None else 0, correct.data_ptr(),
            labels.data_ptr() if labels is not None else 0, slot.data_ptr() if slot is not None else 0,
            _workspace(lib, dev, n), _stream(dev)), "mrgcn_xent_train_eval_rows_f32")
    bump("nc.fused_loss")
    return loss, correct


class _FusedXent(torch.autograd.Function):
    """`train._SoftmaxXent` with the forward launch replaced by the fused one: the same compact gradient rows (bit for
    bit), so the backward is `_SoftmaxXent`'s, unchanged; `slot` receives {loss, accuracy} of the same logits."""

    @staticmethod
    def forward(ctx, logits, idx, targets, flags, sparse, slot):
        ctx.flags, ctx.sparse = flags, bool(sparse and flags is not None)
        if logits.stride(1) != 1:
            logits = logits.contiguous()
        N, Cn = logits.shape
        drows = torch.empty((idx.numel(), Cn), dtype=torch.float32, device=logits.device)
        loss, _ = xent_train_eval(logits, idx, targets, drows=drows, slot=slot)
        ctx.save_for_backward(drows, idx)
        ctx.shape = (N, Cn)
        return loss

    @staticmethod
    def backward(ctx, g):
        return T._SoftmaxXent.backward(ctx, g) + (None,)


def fused_crossentropy(Y_hat, idx, targets, slot, sole_consumer: bool = False):
    """`train.categorical_crossentropy` whose launch also writes {loss, accuracy} of the rows into `slot`."""
    flags, sparse = T._loss_route(Y_hat, idx, targets, sole_consumer)
    return _FusedXent.apply(Y_hat, idx.contiguous(), targets.contiguous(), flags, sparse, slot)


def _check_slot(slot, dev):
    if slot is None:
        return torch.empty(2, dtype=torch.float32, device=dev)
    if not (torch.is_tensor(slot) and slot.is_cuda and slot.dtype == torch.float32 and tuple(slot.shape) == (2,)
            and slot.is_contiguous()):
        raise L.MrgcnError("slot: one contiguous float32 [2] row of the epoch's batch table on the device")
    return slot


def train_batch_step(model, batch, optimizer, l1_lambda=0, l2_lambda=0, slot=None):
    """One batch of :158-201 — `train.train_step` on `lambda: model(batch)` with the batch's stored labels: forward,
    loss, backward, clip, Adam, with row-sparse `weight_I` handling, weight decay, L1 / L2 and device node dropout
    being whatever `train_step` does.  The loss is the fused launch, so the accuracy of the same logits (the forward
    in front of the update, as the reference reports it) costs no second pass.  No host readback: returns
    `(loss, acc)` as device scalars, the loss being what `train_step` returns (penalty included); with `slot` (a
    float32 [2] row of the epoch's batch table) both values are also there."""
    st = _state(batch)
    slot = _check_slot(slot, st["device"])
    loss = T.train_step(model, lambda: _logits(model, batch), st["pos"], st["tgt"], optimizer, l1_lambda, l2_lambda,
                        loss_fn=lambda logits, idx, targets: fused_crossentropy(logits, idx, targets, slot,
                                                                                sole_consumer=True))
    if l1_lambda > 0 or l2_lambda > 0:   # (:172-188: the batch's loss is the penalised one)
        slot[0:1].copy_(loss.reshape(1))
    return loss, slot[1]


def _batch_means(train_slots, n_train, valid_slots, n_valid, row4):
    dev = row4.device
    with torch.cuda.device(dev):
        L.check(L.load().mrgcn_batch_means_f32(train_slots.data_ptr(), int(n_train),
                                               valid_slots.data_ptr() if n_valid else 0, int(n_valid),
                                               row4.data_ptr(), _stream(dev)), "mrgcn_batch_means_f32")


def _slot_table(n, dev):
    return torch.zeros((max(int(n), 1), 2), dtype=torch.float32, device=dev)


def _eval_pass(model, batches, slots, labels=None):
    """Every batch's forward under `eval()` and `no_grad` and its loss launch (no gradient rows); `labels`: one int64
    buffer the batches' arg-maxes go to, each at its batch's offset."""
    if not (slots.is_cuda and slots.dtype == torch.float32 and slots.dim() == 2 and slots.shape[1] == 2
            and slots.is_contiguous() and slots.shape[0] >= len(batches)):
        raise L.MrgcnError("slots: a contiguous float32 [batches, 2] table on the device")
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            at = 0
            for i, batch in enumerate(batches):
                st = _state(batch)
                xent_train_eval(_logits(model, batch), st["pos"], st["tgt"], slot=slots[i],
                                labels=labels[at:at + st["n"]] if labels is not None else None)
                at += st["n"]
    finally:
        model.train(was_training)


def eval_model(model, batches, slots=None):
    """:229-256 under `model.eval()` and `no_grad` (the model's mode is put back on exit): per batch the loss and
    accuracy of `model(batch)` on the batch's labels, by the fused launch without gradient rows — `train.evaluate`'s
    values, written straight into the batch's slot.  Returns `(loss, acc)`, the unweighted means over the batches
    (:253-254), as device scalars; with `slots` (the caller's float32 [batches, 2] table, e.g. `BatchEpoch`'s) the
    per-batch values are left there and the means are the caller's business: returns None."""
    if not batches:
        raise L.MrgcnError("eval_model: no batches")
    if slots is not None:
        _eval_pass(model, batches, slots)
        return None
    dev = _state(batches[0])["device"]
    slots, row = _slot_table(len(batches), dev), torch.empty(4, dtype=torch.float32, device=dev)
    _eval_pass(model, batches, slots)
    _batch_means(slots, len(batches), None, 0, row)
    return row[0], row[1]


def test_model(model, batches):
    """:258-310 on prepared batches: the pass of `eval_model` with every batch's labels kept.  Returns
    `(loss, acc, labels, targets)` as the reference does — two floats (means over batches) and two int64 arrays, the
    batches' vectors in batch order; each batch's launch writes its labels at its offset in one device buffer, and
    everything is read back once, at the end."""
    if not batches:
        raise L.MrgcnError("test_model: no batches")
    dev = _state(batches[0])["device"]
    total = sum(_state(b)["n"] for b in batches)
    slots, row = _slot_table(len(batches), dev), torch.empty(4, dtype=torch.float32, device=dev)
    labels = torch.empty(total, dtype=torch.int64, device=dev)
    _eval_pass(model, batches, slots, labels)
    _batch_means(slots, len(batches), None, 0, row)
    # (one wait for both small copies)
    row_h = torch.empty(4, dtype=torch.float32).pin_memory()
    labels_h = torch.empty(total, dtype=torch.int64).pin_memory()
    row_h.copy_(row, non_blocking=True)
    labels_h.copy_(labels, non_blocking=True)
    torch.cuda.current_stream(dev).synchronize()
    targets = np.concatenate([_state(b)["tgt_host"] for b in batches])
    return float(row_h[0]), float(row_h[1]), labels_h.numpy().copy(), targets


test_model.__test__ = False   # (the reference's name; not a pytest case)


# ---- the epoch ----------------------------------------------------------------------------------------------------
class BatchEpoch:
    """One epoch of :154-225 as a callable, with its device tables: every training batch in order
    (`train_batch_step`, slot i), every validation batch (`eval_model`), the epoch's row
    `(train_loss, train_acc, val_loss, val_acc)` — unweighted means over BATCHES, not over samples
    (mrgcn_batch_means_f32; -1, -1 without validation batches) —, the early-stop record on `val_loss`
    (`record_row`: the row goes to row `records % poll` of `ring`) and the snapshot of the best state behind the
    record's flag.  No host synchronisation anywhere.  `early_stop`: None, a DeviceEarlyStop, or a host EarlyStop as its
    configuration; without one a counting record keeps the row counter."""

    def __init__(self, model, train_batches, valid_batches, optimizer, early_stop=None, ring=None, poll=8,
                 l1_lambda=0, l2_lambda=0):
        valid_batches = list(valid_batches or [])
        train_batches = list(train_batches)
        if not train_batches:
            raise L.MrgcnError("BatchEpoch: no training batches")
        if early_stop is not None and not valid_batches:
            raise L.MrgcnError("node_classification: early stopping scores the validation loss: pass valid_batches")
        dev = _state(train_batches[0])["device"]
        for b in train_batches + valid_batches:
            if _state(b)["device"] != dev:
                raise L.MrgcnError("BatchEpoch: the batches live on one device")
        self.model, self.optimizer = model, optimizer
        self.train_batches, self.valid_batches = train_batches, valid_batches
        self.l1_lambda, self.l2_lambda = l1_lambda, l2_lambda
        self.stopper = T._as_device_stopper(early_stop, model, optimizer)
        self.counter = self.stopper.state if self.stopper is not None else T._StopState(dev, 1, 0.0, T._COUNT_ONLY)
        self.ring = ring if ring is not None else torch.zeros((max(int(poll), 1), 4), dtype=torch.float32, device=dev)
        self.train_slots = _slot_table(len(train_batches), dev)
        self.valid_slots = _slot_table(len(valid_batches), dev)
        self.row = torch.zeros(4, dtype=torch.float32, device=dev)

    def reset(self):
        self.counter.reset()
        self.ring.zero_()

    def _run(self):
        self.model.train()   # (:154)
        for i, batch in enumerate(self.train_batches):
            train_batch_step(self.model, batch, self.optimizer, self.l1_lambda, self.l2_lambda,
                             slot=self.train_slots[i])
        nv = len(self.valid_batches)
        if nv:
            eval_model(self.model, self.valid_batches, slots=self.valid_slots)
        _batch_means(self.train_slots, len(self.train_batches), self.valid_slots, nv, self.row)
        score = self.row[2:3] if nv else self.row[0:1]
        (self.stopper if self.stopper is not None else self.counter).record_row(score, self.row, self.ring)
        return self.row

    def __call__(self):
        bump("nc.batch_epoch.eager")
        return self._run()


def train_epoch(model, train_batches, valid_batches, optimizer, early_stop=None, ring=None, l1_lambda=0, l2_lambda=0):
    """One eager epoch on tables of its own (`BatchEpoch(...)()`): returns the device row
    `(train_loss, train_acc, val_loss, val_acc)`.  `early_stop`: None or a DeviceEarlyStop, whose state then lives
    across calls; a host EarlyStop is only a configuration and would start anew every call, so it is refused here —
    a loop over epochs builds one `BatchEpoch` (or calls `fit`)."""
    if early_stop is not None and not isinstance(early_stop, T.DeviceEarlyStop):
        raise L.MrgcnError("train_epoch: pass a DeviceEarlyStop (its state persists between calls), or build one "
                           "BatchEpoch for the run: a host EarlyStop here would be reset every epoch")
    return BatchEpoch(model, train_batches, valid_batches, optimizer, early_stop, ring, l1_lambda=l1_lambda,
                      l2_lambda=l2_lambda)()


class GraphedBatchEpoch(BatchEpoch, T._CapturedStep):
    """`BatchEpoch` captured into ONE hipGraph and replayed through `train.Captured`: `warmup` real
    epochs on the capture stream (plans, per-stream scratch and the loss's row flags exist afterwards), then the
    counter and the ring reset, so that the first replay is record 1.  Needs `ClipAdam(capturable=True)`; the batches
    are masked batches (`mkbatches(..., plan=...)`) or full batches — slice batches cut their slices per forward: run
    them through `BatchEpoch`."""

    def __init__(self, model, train_batches, valid_batches, optimizer, early_stop=None, ring=None, poll=8,
                 l1_lambda=0, l2_lambda=0, warmup: int = 3):
        if not getattr(optimizer, "capturable", False):
            raise L.MrgcnError("GraphedBatchEpoch needs ClipAdam(..., capturable=True)")
        super().__init__(model, train_batches, valid_batches, optimizer, early_stop, ring, poll, l1_lambda, l2_lambda)
        for b in self.train_batches + self.valid_batches:
            if not _is_fixed_structure(b):
                raise L.MrgcnError("GraphedBatchEpoch: slice batches are not captured; build the batches on the full "
                                   "graph's plan (mkbatches(..., plan=plan): the masked path) or use BatchEpoch")
        self._capture(self._run, warmup, optimizer, self.reset)

    def __call__(self):
        T._CapturedStep.__call__(self)
        bump("nc.batch_epoch.graphed")
        return self.row


def fit(model, train_batches, valid_batches, optimizer, nepoch, early_stop=None, poll=8, graphed=True, l1_lambda=0,
        l2_lambda=0, max_graph_batches=None, warmup: int = 3):
    """The reference's mini-batch `train_model` loop (:146-227) as a generator over
    `(epoch, train_loss, train_acc, val_loss, val_acc)` — floats, epochs from 1 — with `train.fit`'s contract: the
    host looks in every `poll` epochs only, the rows wait in a device ring of `poll` rows, the stop is latched on the
    device, the rows up to and including the stopping record are yielded, the best state is restored in place
    (`restore_()`) on a stop, a run that never stops keeps the LAST epoch's state, and both validation values are -1
    when `valid_batches` is empty (early stopping then raises).  The batches are prepared ones
    (`prepare_batches(mkbatches(...), Y, device)`).

    `graphed=True` replays one captured epoch (`GraphedBatchEpoch`; its `warmup` epochs are real optimizer steps
    taken before epoch 1) as long as the epoch has at most `max_graph_batches` batches (training plus validation;
    default `MAX_GRAPH_BATCHES`) of a fixed structure; a longer epoch, or slice batches, run the eager `BatchEpoch`,
    which is just as free of synchronisation."""
    train_batches, valid_batches = list(train_batches), list(valid_batches or [])
    poll = max(int(poll), 1)
    if early_stop is not None and not valid_batches:
        raise L.MrgcnError("fit: early stopping scores the validation loss: pass valid_batches")
    cap = MAX_GRAPH_BATCHES if max_graph_batches is None else int(max_graph_batches)
    both = train_batches + valid_batches
    args = (model, train_batches, valid_batches, optimizer, early_stop, None, poll, l1_lambda, l2_lambda)
    if graphed and len(both) <= cap and all(_is_fixed_structure(b) for b in both):
        run = GraphedBatchEpoch(*args, warmup=warmup)
    else:
        run = BatchEpoch(*args)
        run.reset()
    yield from T._poll_records(run, run.counter, run.ring, nepoch, poll, run.stopper)
