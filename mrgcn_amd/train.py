"""Full-batch epoch driver: the MI355X counterpart of the train step of
mrgcn/tasks/node_classification.py:154-193 —

    Y_hat = model(batch); loss = CE(Y_hat[idx], targets)
    zero_grad; backward; clip_grad_norm_(params, 1.0); Adam.step

with the loss here and the global gradient norm, the clip and Adam in mrgcn_amd.optim (`ClipAdam`) running as HIP
kernels (csrc/optim.hip).  The clip coefficient never leaves the device, so one epoch has no host synchronisation."""
from __future__ import annotations

import ctypes as C

from contextlib import contextmanager

import torch

from . import _lib as L
from . import functional as Fn
from .functional import _ROW_SPARSE_ENV as _ROW_SPARSE_DEFAULT  # MRGCN_ROW_SPARSE=0: no row-sparse weight_I gradient
from .functional import clear_row_grads, dense_from_rows, pop_row_grad, row_sparse_weight_grad  # noqa: F401
from .optim import _MULTI, _MULTI_MAX_NUMEL, ClipAdam, _stream, _to_reference_layout, merge_row_grad  # noqa: F401  (once here)
from .stats import bump


_LABEL_FLAGS: dict = {}


def _label_flags(idx: torch.Tensor, num_rows: int):
    """(flags, unique): uint8 [num_rows] with a 1 at every labelled row, kept under the identity of `idx` — the same
    tensor object, unchanged, gives the same flags tensor every epoch, which is what keys the gradient support of
    the label set (plan.GraphPlan.support_for).  None while a stream capture is under way and the flags do not
    exist yet (their check for repeated rows synchronises)."""
    key = (idx.data_ptr(), idx._version, int(idx.numel()), int(num_rows), idx.device)
    ent = _LABEL_FLAGS.get(key)
    if ent is None:
        if torch.cuda.is_current_stream_capturing():
            return None
        flags = torch.zeros((num_rows,), dtype=torch.uint8, device=idx.device)
        flags[idx] = 1
        unique = int(flags.sum(dtype=torch.int64)) == int(idx.numel())
        while len(_LABEL_FLAGS) >= 8:
            _LABEL_FLAGS.pop(next(iter(_LABEL_FLAGS)))
        ent = _LABEL_FLAGS[key] = (flags, unique, idx)  # (holds `idx`: its address cannot be handed to another tensor)
    return ent[0], ent[1]


class _SoftmaxXent(torch.autograd.Function):
    """nn.CrossEntropyLoss()(Y_hat[idx], targets) (node_classification.py:439-444).  The forward keeps the
    gradient of the labelled rows only (n x C); the backward forms the N x C gradient from it, scaled by the
    upstream gradient in the same pass, and notes which rows hold anything (functional._set_grad_meta: the last
    layer's backward then does not scan 73 MB of zeros for them).  `flags` (from _label_flags): the labelled rows
    as a persistent flags tensor — the note then names a structural row set; `sparse`: the rows outside it are not
    written at all (only for a consumer that reads the flagged rows: functional.rgcn_layer marks such outputs)."""

    @staticmethod
    def forward(ctx, logits, idx, targets, flags=None, sparse=False):
        ctx.flags, ctx.sparse = flags, bool(sparse and flags is not None)
        if logits.stride(1) != 1:        # (rows may be strided: a layer output in a buffer with padded rows)
            logits = logits.contiguous()
        N, C = logits.shape
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        drows = torch.empty((idx.numel(), C), dtype=torch.float32, device=logits.device)
        with torch.cuda.device(logits.device):
            L.check(L.load().mrgcn_softmax_xent_rows_f32(
                logits.data_ptr(), logits.stride(0), C, idx.data_ptr(), targets.data_ptr(), idx.numel(),
                loss.data_ptr(), drows.data_ptr(), _stream(logits.device)), "mrgcn_softmax_xent_rows_f32")
        ctx.save_for_backward(drows, idx)
        ctx.shape = (N, C)
        return loss

    @staticmethod
    def backward(ctx, g):
        from .functional import _set_grad_meta
        drows, idx = ctx.saved_tensors
        N, C = ctx.shape
        dev = drows.device
        g = g.to(torch.float32).contiguous()
        dlogits = torch.empty((N, C), dtype=torch.float32, device=dev)
        if ctx.sparse:  # the labelled rows only: no zero fill of the other N - n
            with torch.cuda.device(dev):
                L.check(L.load().mrgcn_softmax_xent_bwd_rows_f32(
                    drows.data_ptr(), idx.data_ptr(), idx.numel(), C, g.data_ptr(), dlogits.data_ptr(), C,
                    _stream(dev)), "mrgcn_softmax_xent_bwd_rows_f32")
            _set_grad_meta(dlogits, ctx.flags, False, structural=True, sparse_rows=True)
            return dlogits, None, None, None, None
        flags = ctx.flags if ctx.flags is not None else torch.empty((N,), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            L.check(L.load().mrgcn_softmax_xent_bwd_f32(
                drows.data_ptr(), idx.data_ptr(), idx.numel(), C, g.data_ptr(), dlogits.data_ptr(), C, N,
                0 if ctx.flags is not None else flags.data_ptr(), _stream(dev)), "mrgcn_softmax_xent_bwd_f32")
        _set_grad_meta(dlogits, flags, False, structural=ctx.flags is not None)
        return dlogits, None, None, None, None


def categorical_crossentropy(Y_hat: torch.Tensor, idx: torch.Tensor, targets: torch.Tensor, sole_consumer: bool = False):
    """`idx`, `targets`: int64 device tensors (the `Y.nonzero()` pair of the reference).  `sole_consumer`: nothing
    but this loss reads `Y_hat` (train_step): when `Y_hat` comes straight out of a layer whose backward goes by the
    row flags, the gradient's unlabelled rows are then not even zero-filled."""
    flags, sparse = _loss_route(Y_hat, idx, targets, sole_consumer)
    return _SoftmaxXent.apply(Y_hat, idx.contiguous(), targets.contiguous(), flags, sparse)


def _loss_route(Y_hat, idx, targets, sole_consumer):
    """(flags, sparse) of `_SoftmaxXent` for these logits and labels, and the counter of the route taken."""
    assert idx.dtype == torch.int64 and targets.dtype == torch.int64
    from .functional import _SUPPORT
    flags = sparse = None
    if _SUPPORT and Y_hat.is_cuda and idx.is_contiguous():
        ent = _label_flags(idx, Y_hat.shape[0])
        if ent is not None:
            flags = ent[0]
            sparse = bool(sole_consumer and ent[1] and getattr(Y_hat, "_mrgcn_sparse_grad_ok", False)
                          and Y_hat.grad_fn is not None and type(Y_hat.grad_fn).__name__ == "_RgcnLayerBackward")
    bump("loss.sparse_rows" if sparse else "loss.flagged" if flags is not None else "loss.plain")
    return flags, sparse


def categorical_accuracy(Y_hat, idx, targets):
    """node_classification.py:432-437"""
    labels = Y_hat[idx].argmax(dim=1)
    return (labels == targets).float().mean(), labels, targets


def weight_regularisation(model, l1_lambda: float = 0.0, l2_lambda: float = 0.0, skip=()):
    """l1 * sum|p| + l2 * sum p^2 over the parameters whose NAME contains 'weight'
    (node_classification.py:172-188).  Zero in every shipped config; plain tensor ops.  `skip`: parameters left out
    (their penalty is somebody else's: `ClipAdam.step(l1_lambda=, l2_lambda=, reg_params=)`)."""
    reg = None
    skipped = {id(p) for p in skip}
    for name, p in model.named_parameters():
        if "weight" not in name or id(p) in skipped:
            continue
        term = None
        if l1_lambda > 0:
            term = l1_lambda * p.abs().sum()
        if l2_lambda > 0:
            t2 = l2_lambda * (p * p).sum()
            term = t2 if term is None else term + t2
        if term is not None:
            reg = term if reg is None else reg + term
    return reg


_ONES: dict = {}


def _ones_like_loss(loss):
    """The seed gradient of `loss.backward()`: one cached scalar per (device, dtype) instead of a fill per epoch."""
    key = (loss.device, loss.dtype)
    t = _ONES.get(key)
    if t is None:
        t = _ONES[key] = torch.ones((), dtype=loss.dtype, device=loss.device)
    return t


def train_step(model, forward_fn, idx, targets, optimizer, l1_lambda: float = 0.0, l2_lambda: float = 0.0,
               row_sparse=None, loss_fn=None):
    """One full-batch epoch.  `forward_fn()` returns the logits (e.g. `lambda: model(batch)`).
    Returns the loss as a device scalar (no host sync).  `row_sparse`: None = skip the rows of a node-major
    weight_I's gradient / Adam update that carry no gradient whenever that is exact (ClipAdam — `weight_I.grad`
    stays None for such a step, the gradient travels on the parameter; under weight decay or an L1 / L2 penalty the
    update visits every node but still rebuilds the loss's gradient from the support, and the returned loss includes
    the penalty the optimizer computed: DESIGN section 14); False = always the dense gradient in `.grad` and the dense
    Adam kernel.  `loss_fn(logits, idx, targets)`: another loss of the same contract in place of
    `categorical_crossentropy(..., sole_consumer=True)` (tasks.node_classification: the batch's loss with its accuracy
    out of the same launch)."""
    if isinstance(model, torch.nn.Module):
        from .models.rgcn import refuse_edge_dropout
        refuse_edge_dropout(model, "train.train_step (its loss hands down row-sparse gradients, whose backward runs on "
                                   "gradient supports)")
    params = [p for g in optimizer.param_groups for p in g["params"]]
    clear_row_grads(params)
    logits = forward_fn()
    if loss_fn is None:
        loss = categorical_crossentropy(logits, idx, targets, sole_consumer=True)
    else:
        loss = loss_fn(logits, idx, targets)
    reg = l1_lambda > 0 or l2_lambda > 0
    # weight_I's gradient may stay unwritten where no node has any when the optimizer is the one that
    # knows how to read it.  Under weight decay or a penalty every node block moves, which the regularised row update
    # does from the same row-sparse form (csrc/adam_reg.hip) — when every input-term weight of the model is a
    # node-major table of a shape it takes; otherwise the backward writes dense gradients as it always did.
    sparse_ok = row_sparse is not False and _ROW_SPARSE_DEFAULT and isinstance(optimizer, ClipAdam)
    tables = ()
    if sparse_ok and (reg or any(float(g["weight_decay"]) != 0.0 for g in optimizer.param_groups)):
        tables = _reg_tables(model, params)
        sparse_ok = tables is not None and optimizer._dist is None
        tables = tables if (sparse_ok and reg) else ()
    if reg:
        term = weight_regularisation(model, l1_lambda, l2_lambda, skip=tables)
        if term is not None:
            loss = loss + term
    optimizer.zero_grad(set_to_none=True)
    prev = row_sparse_weight_grad(sparse_ok)
    try:
        loss.backward(gradient=_ones_like_loss(loss))
    finally:
        row_sparse_weight_grad(prev)
    if tables:
        optimizer.step(l1_lambda=l1_lambda, l2_lambda=l2_lambda, reg_params=tables)
        return loss.detach() if optimizer.reg_loss is None else loss.detach() + optimizer.reg_loss
    optimizer.step()
    return loss.detach()


def _reg_tables(model, params):
    """The node tables of `model` that the regularised row update can step (node-major `weight_I` of a basis layer,
    shapes of include/mrgcn_hip.h: mrgcn_support_reg_norm_workspace), or None when some input-term weight is known
    not to be one of them (no bases, a wide layer) or is not among `params` — known before the backward runs, which
    then writes dense gradients."""
    stepped = {id(p) for p in params}
    tables = []
    for name, p in model.named_parameters():
        if name.rsplit(".", 1)[-1] != "weight_I" or not p.requires_grad:
            continue
        if not getattr(p, "_mrgcn_node_major", False) or p.dim() != 3 or id(p) not in stepped:
            return None
        _, B, F = p.shape
        if not (0 < B <= 64 and 0 < F <= 16 and F % 2 == 0 and (B * F) % 4 == 0 and B * F <= 512):
            return None
        tables.append(p)
    return tables or None


@contextmanager
def capture_without_gc():
    """Around a stream capture: collect dead cycles first, then keep the cyclic collector off until the capture ends.
    torch no longer collects in front of a capture, and a collection that starts in the middle of one — in whichever
    thread allocates the object that crosses the threshold, the autograd worker included — runs the destructors of
    whatever dead cycle holds device objects (an earlier run's captured graphs and their pools) while the capture is
    open."""
    import gc
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


class Captured:
    """The capture discipline of every graphed step and run loop, once.  `warmup()` runs on a side stream
    (the real steps that build plans, per-stream scratch and lazily filled caches, then whatever counter and ring
    resets the caller wants in front of record 1); then each zero-argument callable of `fns` is captured into a
    hipGraph of its own on that same stream — a single chain per graph, no parallel branches, `thread_local` (calls
    other threads make meanwhile, e.g. a process group's watchdog, do not invalidate the capture), the cyclic
    collector held off (`capture_without_gc`).  Capturing executes nothing on the device.

    `graphs`, `outs` (what each `fn` returned under capture) and `pair_sums` (per graph, the pair-sum tables of a
    constant layer input that the graph reads) are lists in the order of `fns`.  `replay(i)` compares `optimizer`'s
    `_state_gen` with the captured one (`load_state_dict` replaces the moment tensors and the device step counter a
    graph was captured on) and raises `MrgcnError` under the name `who`, refreshes graph i's pair-sum tables (a replay
    cannot see an in-place change of X: integer compares on the host, a rebuild in place on a mismatch), replays and
    returns `outs[i]`."""

    def __init__(self, fns, warmup, optimizer=None, who=""):
        # the captured launches name the addresses of whatever the callables close over (a sampler's buffers, stored
        # orders): they live as long as the graphs do, also when the caller keeps nothing but this object
        self._fns, self._who = tuple(fns), who
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            warmup()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graphs, self.outs, self.pair_sums = [], [], []
        for fn in self._fns:
            g = torch.cuda.CUDAGraph()
            Fn.take_captured_pair_sums()
            # (on the stream the warm-up ran on: whatever keeps scratch per stream has met it already)
            with capture_without_gc(), torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                self.outs.append(fn())
            self.pair_sums.append(Fn.take_captured_pair_sums())
            self.graphs.append(g)
        self._optimizer, self._state_gen = optimizer, (optimizer._state_gen if optimizer is not None else None)

    def replay(self, i=0):
        if self._optimizer is not None and self._optimizer._state_gen != self._state_gen:
            if len(self.graphs) == 1:
                raise L.MrgcnError(f"{self._who}: the optimizer's state was loaded after the capture; build a new "
                                   f"{self._who} (the captured graph still updates the old moment buffers)")
            raise L.MrgcnError(f"{self._who}: the optimizer's state was loaded after the capture (the captured graphs "
                               "still update the old moment buffers)")
        for sup in self.pair_sums[i]:
            sup.pair_sums_refresh()
        self.graphs[i].replay()
        return self.outs[i]


class _CapturedStep:
    """One step captured once (`Captured`) after `warmup` real calls of it (at least one) and replayed by calling the
    object."""

    def _capture(self, step, warmup, optimizer=None, then=None):
        """-> what `step()` returned under capture; `then()` closes the warm-up (counter and ring resets)."""
        self.warmup_steps = max(warmup, 1)

        def warm():
            for _ in range(self.warmup_steps):
                step()
            if then is not None:
                then()
        self._captured = Captured([step], warm, optimizer, type(self).__name__)
        self.graph = self._captured.graphs[0]
        return self._captured.outs[0]

    def __call__(self):
        return self._captured.replay()


class GraphedStep(_CapturedStep):
    """Any allocation-stable, synchronisation-free step `fn()` (returning a device scalar) captured into a hipGraph and
    replayed — e.g. one full-batch link-prediction epoch: negatives drawn on the device from torch's default generator
    (whose state torch advances per replay), encoder, DistMult scores, BCE, backward, `ClipAdam(capturable=True)`.
    `warmup` real calls run first, on the stream the capture then uses (`Captured`)."""

    def __init__(self, fn, warmup: int = 3):
        self.out = self._capture(fn, warmup)


class GraphedTrainStep(_CapturedStep):
    """One full-batch epoch captured into a hipGraph (torch.cuda.CUDAGraph) and replayed: the ~40
    kernel launches of a step become one graph launch, which is what bounds the small shapes
    (AIFB / MUTAG epochs are launch-latency territory).  Everything in the step is stream-ordered
    and allocation-free at the C ABI, the optimizer keeps its step counter on the device
    (`ClipAdam(capturable=True)`), so the captured sequence is exactly the eager one.

        step = GraphedTrainStep(model, lambda: model(X, A), idx, targets, optimizer)
        loss = step()          # device scalar, no host sync

    The graph plans must exist before capture (the warm-up steps build them); shapes are static.  Capturing executes
    nothing on the device: `warmup` optimizer steps have been taken when the constructor returns (the optimizer's
    device counter says the same; ClipAdam.state_dict() reads it back)."""

    def __init__(self, model, forward_fn, idx, targets, optimizer, warmup: int = 3,
                 l1_lambda: float = 0.0, l2_lambda: float = 0.0, row_sparse=None):
        if not getattr(optimizer, "capturable", False):
            raise L.MrgcnError("GraphedTrainStep needs ClipAdam(..., capturable=True)")

        def step():
            return train_step(model, forward_fn, idx, targets, optimizer, l1_lambda, l2_lambda, row_sparse)
        self.loss = self._capture(step, warmup, optimizer)
        self._pair_sums = self._captured.pair_sums[0]


# ---- validation and early stopping inside the epoch (csrc/early_stop.hip) -------------------------------------------
class EarlyStop:
    """The reference's `tasks/utils.py::EarlyStop` on the host: same constructor, attributes and `record(score,
    weights, optim)` — the first `delay` records are swallowed, the next sets `best_score` (kept at -1 until then)
    and spends no patience, every later one spends one and, when `score + tolerance < best_score`, sets the best
    score, deep-copies both `state_dict()`s and gives the patience back; `stop` is set when no patience is left
    after that.  Scores are losses (>= 0): `best_score < 0` is the "none yet" sentinel, as in the reference.

    `fit` and `GraphedTrainEvalStep` also take an instance as the configuration of a `DeviceEarlyStop`."""

    def __init__(self, patience=7, tolerance=0.01, delay=10):
        self.full_patience = self.patience = patience
        self.tolerance, self.delay = tolerance, delay
        self.stop = False
        self.best_score = -1
        self.best_weights = self.best_optim = None

    def record(self, score, weights, optim):
        import copy
        if self.delay > 0:   # still inside the grace period
            self.delay -= 1
            return
        first = self.best_score < 0
        if not first:
            self.patience -= 1
        if first or score + self.tolerance < self.best_score:
            self.best_score = score
            self.best_weights = copy.deepcopy(weights.state_dict())
            self.best_optim = copy.deepcopy(optim.state_dict())
            if not first:
                self.patience, self.stop = self.full_patience, False
        if not first and self.patience <= 0:
            self.stop = True


_COUNT_ONLY = (1 << 31) - 1   # a delay that swallows every record: the state then only counts them


class _StopState:
    """The device struct of include/mrgcn_hip.h: mrgcn_early_stop_state, the launch that records into it and the one
    small copy that reads it back."""

    def __init__(self, device, patience, tolerance, delay):
        self.patience_default, self.tolerance, self.delay0 = int(patience), float(tolerance), int(delay)
        self.buf = torch.zeros(C.sizeof(L.EarlyStopState), dtype=torch.uint8, device=device)
        self.reset()

    def write(self, st):
        self.buf.copy_(torch.frombuffer(bytearray(bytes(st)), dtype=torch.uint8))

    def reset(self):
        self.write(L.EarlyStopState(-1.0, 0, 0, self.delay0, self.patience_default, 0, 0))

    def read(self):
        """One device-to-host copy of the 40 bytes (synchronises with the stream's work so far)."""
        return L.EarlyStopState.from_buffer_copy(self.buf.cpu().numpy().tobytes())

    @property
    def improved_ptr(self) -> int:
        return self.buf.data_ptr() + L.EarlyStopState.improved.offset

    def record(self, score, metrics=None, values=None):
        if not (score.is_cuda and score.dtype == torch.float32 and score.numel() == 1):
            raise L.MrgcnError("early stop: the score is one float32 on the device")
        row = None
        if metrics is not None:
            if not (metrics.is_cuda and metrics.dtype == torch.float32 and metrics.dim() == 2
                    and metrics.shape[1] == 4 and metrics.is_contiguous() and metrics.shape[0] > 0):
                raise L.MrgcnError("metrics: a contiguous float32 [rows, 4] tensor on the device")
            values = tuple(values or ()) + (None,) * (4 - len(values or ()))
            for v in values:
                if v is not None and not (v.is_cuda and v.dtype == torch.float32 and v.numel() == 1):
                    raise L.MrgcnError("metrics: every value is one float32 on the device")
            row = L.MetricsRow((C.c_void_p * 4)(*[v.data_ptr() if v is not None else None for v in values]),
                               metrics.data_ptr(), int(metrics.shape[0]))
        dev = self.buf.device
        with torch.cuda.device(dev):
            L.check(L.load().mrgcn_early_stop_record(self.buf.data_ptr(), score.data_ptr(), self.tolerance,
                                                     self.patience_default, C.byref(row) if row is not None else None,
                                                     _stream(dev)), "mrgcn_early_stop_record")


    def record_row(self, score, row, ring):
        """`record` with a metrics row of any width (mrgcn_early_stop_record_row): the contiguous float32 device
        vector `row` goes to row `records % rows` of the float32 `[rows, len(row)]` device `ring`."""
        if not (score.is_cuda and score.dtype == torch.float32 and score.numel() == 1):
            raise L.MrgcnError("early stop: the score is one float32 on the device")
        if not (row.is_cuda and row.dtype == torch.float32 and row.dim() == 1 and row.is_contiguous() and row.numel() > 0
                and ring.is_cuda and ring.dtype == torch.float32 and ring.dim() == 2 and ring.is_contiguous()
                and ring.shape[0] > 0 and ring.shape[1] == row.numel()):
            raise L.MrgcnError("record_row: a contiguous float32 [width] row and a contiguous float32 [rows, width] "
                               "ring on the device")
        dev = self.buf.device
        with torch.cuda.device(dev):
            L.check(L.load().mrgcn_early_stop_record_row(self.buf.data_ptr(), score.data_ptr(), self.tolerance,
                                                         self.patience_default, row.data_ptr(), int(row.numel()),
                                                         ring.data_ptr(), int(ring.shape[0]), _stream(dev)),
                    "mrgcn_early_stop_record_row")


class DeviceEarlyStop:
    """`EarlyStop` with its state, its decision and its copy of the best weights on the device, so that a replayed epoch
    graph records into it without the host:

        stopper = DeviceEarlyStop(model, optimizer, patience=7, tolerance=0.01)   # after the first optimizer step
        stopper.record(val_loss)       # device float32 scalar; capturable: the record launch, then the snapshot
        if stopper.poll(): stopper.restore_()

    `record` runs `mrgcn_early_stop_record` and then `mrgcn_snapshot_if` on the `improved` flag the record just wrote:
    when this record set the best score, every parameter, every persistent module buffer (BatchNorm's running
    statistics), every tensor of the optimizer's state (both Adam moments) and ClipAdam's device step counter and
    bias corrections are copied into buffers allocated here, once.  (Buffers are named by address: a module that
    replaces a buffer tensor instead of updating it in place needs a new DeviceEarlyStop.)  Once `stop`
    is set the record launch changes nothing, `improved` stays 0, and records taken before the host polls cannot touch
    the snapshot.  `restore_()` copies the snapshot back IN PLACE (no `load_state_dict`, no `_state_gen` bump: a
    captured graph over these tensors stays valid).  The score is any device scalar — a link-prediction loop may pass
    its own.  Scores are >= 0 (`best_score < 0` means "none yet", as in the reference).

    The optimizer's state must exist (it is what gets snapshotted): before the first step the constructor raises.
    A ClipAdam must be `capturable` (its step count then lives on the device and is part of the snapshot)."""

    def __init__(self, model, optimizer, patience=7, tolerance=0.01, delay=10):
        params, seen = [], set()
        for p in list(model.parameters()) + [p for g in optimizer.param_groups for p in g["params"]]:
            if id(p) not in seen:
                seen.add(id(p))
                params.append(p)
        if not params or not all(p.is_cuda for p in params):
            raise L.MrgcnError("DeviceEarlyStop: the parameters live on the GPU")
        live = []
        has_state = False
        for p in params:
            live.append(p.data)
            for k, v in (optimizer.state.get(p) or {}).items():
                if torch.is_tensor(v):
                    live.append(v)
                    has_state = True
                elif k == "step" and not getattr(optimizer, "capturable", False):
                    raise L.MrgcnError("DeviceEarlyStop: the optimizer counts its steps on the host; use "
                                       "ClipAdam(..., capturable=True)")
        if not has_state:
            raise L.MrgcnError("DeviceEarlyStop: the optimizer has no state yet (its moments are what gets "
                               "snapshotted): take the first optimizer step before building it")
        for ent in getattr(optimizer, "_dev_step", {}).values():
            live += [ent[0], ent[1]]
        # the buffers a state_dict() carries (BatchNorm's running statistics and batch count in the encoders): an
        # eval() forward after the restore then sees the best record's statistics, as with the reference's best_weights
        self._buffers = [b for m in model.modules() for k, b in m._buffers.items()
                         if b is not None and k not in m._non_persistent_buffers_set]
        seen_buf = set()
        for b in self._buffers:
            if id(b) not in seen_buf:
                seen_buf.add(id(b))
                live.append(b)
        for t in live:
            if not t.is_contiguous() or not t.is_cuda:
                raise L.MrgcnError("DeviceEarlyStop: parameters and optimizer state are contiguous device tensors")
        device = params[0].device
        self.state = _StopState(device, patience, tolerance, delay)
        self._params, self._live = params, live
        self._snap = [torch.empty_like(t) for t in live]
        block = int(L.load().mrgcn_snapshot_block_bytes())
        table = (L.CopyEntry * len(live))()
        blocks = 0
        for i, (s, d) in enumerate(zip(live, self._snap)):
            nbytes = s.numel() * s.element_size()
            table[i] = L.CopyEntry(s.data_ptr(), d.data_ptr(), nbytes, blocks)
            blocks += (nbytes + block - 1) // block
        self._table = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(device)
        self._n, self._blocks = len(live), int(blocks)
        self.snapshot_bytes = sum(s.numel() * s.element_size() for s in live)
        self._optimizer, self._state_gen = optimizer, getattr(optimizer, "_state_gen", None)

    def _check_gen(self):
        if getattr(self._optimizer, "_state_gen", None) != self._state_gen:
            raise L.MrgcnError("DeviceEarlyStop: the optimizer's state was loaded after this object was built (its "
                               "table still names the old moment buffers); build a new one")

    def _copy(self, flag_ptr, restore):
        dev = self._table.device
        with torch.cuda.device(dev):
            L.check(L.load().mrgcn_snapshot_if(flag_ptr, self._table.data_ptr(), self._n, self._blocks,
                                               1 if restore else 0, _stream(dev)), "mrgcn_snapshot_if")

    def record(self, score_dev, metrics=None, values=None):
        """The record, then the snapshot behind its `improved` flag.  `metrics`, `values`: a float32 [rows, 4] ring and
        up to four device scalars written to row `records % rows` by the same launch (see train_eval_step)."""
        self._check_gen()
        self.state.record(score_dev, metrics, values)
        self._copy(self.state.improved_ptr, False)

    def record_row(self, score_dev, row, ring):
        """`record` with a metrics row of any width (`_StopState.record_row`), then the same snapshot."""
        self._check_gen()
        self.state.record_row(score_dev, row, ring)
        self._copy(self.state.improved_ptr, False)

    def reset(self):
        self.state.reset()

    def poll(self) -> bool:
        """One 40-byte device-to-host copy; True once the run should stop."""
        self._last = self.state.read()
        return bool(self._last.stop)

    def restore_(self) -> bool:
        """The snapshot back into the live parameters, moments and step counter, in place.  False (and nothing
        copied) while no record has set a best score."""
        self._check_gen()
        if self.state.read().best_record == 0:
            return False
        self._copy(None, True)
        torch.autograd.graph.increment_version(self._params)
        return True

    stop = property(lambda self: self.poll())
    best_score = property(lambda self: float(self.state.read().best_score))
    best_record = property(lambda self: int(self.state.read().best_record))
    records = property(lambda self: int(self.state.read().records))
    patience = property(lambda self: int(self.state.read().patience))

    def state_dict(self, snapshot: bool = True):
        st = self.state.read()
        sd = {f: getattr(st, f) for f, _ in L.EarlyStopState._fields_}
        sd.update(patience_default=self.state.patience_default, tolerance=self.state.tolerance)
        if snapshot:
            sd["snapshot"] = [t.clone() for t in self._snap]
        return sd

    def load_state_dict(self, sd):
        if "snapshot" in sd:
            if len(sd["snapshot"]) != len(self._snap):
                raise L.MrgcnError("DeviceEarlyStop: the snapshot belongs to another model / optimizer")
            for d, s in zip(self._snap, sd["snapshot"]):
                d.copy_(s)
        self.state.patience_default, self.state.tolerance = int(sd["patience_default"]), float(sd["tolerance"])
        self.state.write(L.EarlyStopState(*[sd[f] for f, _ in L.EarlyStopState._fields_]))


_EVAL_WS: dict = {}
_EVAL_N: dict = {}


def evaluate(logits, idx, targets, want_labels: bool = False):
    """`(loss, acc)` of the rows `logits[idx]` against `targets` as device scalars — the reference's
    `categorical_crossentropy` and `categorical_accuracy` of an evaluation pass (node_classification.py:432-444) in one
    launch that writes no gradient — and with `want_labels` the arg-max of every row as a third value (`test_model`'s
    `labels`).  `acc = correct / n` in float32; of equal logits the lowest class wins; the sums run in a fixed
    order, so equal inputs give equal bits.  No host synchronisation; capturable."""
    if not (logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2):
        raise L.MrgcnError("evaluate: float32 [N, C] logits on the device")
    if not (idx.dtype == torch.int64 and targets.dtype == torch.int64 and idx.numel() == targets.numel()
            and idx.numel() > 0 and idx.device == logits.device and targets.device == logits.device):
        raise L.MrgcnError("evaluate: idx and targets are int64 tensors of one (non-zero) length on the device of "
                           "the logits")
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    idx, targets = idx.contiguous(), targets.contiguous()
    dev, n = logits.device, int(idx.numel())
    lib = L.load()
    loss = torch.empty((), dtype=torch.float32, device=dev)
    correct = torch.empty((), dtype=torch.int64, device=dev)
    labels = torch.empty((n,), dtype=torch.int64, device=dev) if want_labels else None
    ws = 0
    if n > int(lib.mrgcn_xent_eval_single_block_rows()):
        key = (dev, _stream(dev))   # (block partials: one set per stream that evaluates)
        t = _EVAL_WS.get(key)
        if t is None:
            t = _EVAL_WS[key] = torch.empty(int(lib.mrgcn_xent_eval_workspace()), dtype=torch.uint8, device=dev)
        ws = t.data_ptr()
    with torch.cuda.device(dev):
        L.check(lib.mrgcn_xent_eval_rows_f32(logits.data_ptr(), logits.stride(0), logits.shape[1], idx.data_ptr(),
                                             targets.data_ptr(), n, loss.data_ptr(), correct.data_ptr(),
                                             labels.data_ptr() if want_labels else 0, ws, _stream(dev)),
                "mrgcn_xent_eval_rows_f32")
    # (a tensor divisor: torch divides by a Python scalar as a multiplication by its reciprocal, an ulp off correct / n)
    div = _EVAL_N.get((dev, n))   # (kept for good: a captured graph may read it)
    if div is None:
        div = _EVAL_N[(dev, n)] = torch.full((), float(n), dtype=torch.float32, device=dev)
    acc = correct.to(torch.float32).div_(div)
    return (loss, acc, labels) if want_labels else (loss, acc)


def train_eval_step(model, forward_fn, idx, targets, optimizer, l1_lambda: float = 0.0, l2_lambda: float = 0.0,
                    row_sparse=None, valid=None, early_stop=None, metrics=None, counter=None):
    """One epoch of the reference's `train_model` (node_classification.py:146-225) without the host: `train_step`;
    loss and accuracy of the training pass's own logits (the forward in front of the update, as the reference reports
    them); with `valid=(idx, targets)` one more `forward_fn()` under `model.eval()` and `no_grad` and its loss and
    accuracy on the validation rows; `(train_loss, train_acc, val_loss, val_acc)` into row `records % rows` of the
    float32 `[rows, 4]` device ring `metrics` (-1 where there is no validation), the row counter living in the
    early-stop state on the device; `early_stop.record(val_loss)`.  Returns the four device scalars (None for the
    missing ones).  The model's train / eval mode is put back on exit.

    `counter`: the record counter of a run without `early_stop` (fit and GraphedTrainEvalStep bring one)."""
    if early_stop is not None and valid is None:
        raise L.MrgcnError("train_eval_step: early stopping scores the validation loss: pass valid=(idx, targets)")
    box = []

    def fwd():
        out = forward_fn()
        # (at once: the logits may sit in a buffer the backward is free to reuse)
        box[:] = evaluate(out.detach(), idx, targets)
        return out
    train_loss = train_step(model, fwd, idx, targets, optimizer, l1_lambda, l2_lambda, row_sparse)
    train_acc = box[1]
    val_loss = val_acc = None
    if valid is not None:
        was_training = model.training
        model.eval()
        try:
            with torch.no_grad():
                val_loss, val_acc = evaluate(forward_fn(), valid[0], valid[1])
        finally:
            model.train(was_training)
    values = (train_loss, train_acc, val_loss, val_acc)
    if early_stop is not None:
        early_stop.record(val_loss, metrics, values)
    elif metrics is not None:
        if counter is None:
            raise L.MrgcnError("train_eval_step: `metrics` without `early_stop` needs the record counter that fit / "
                               "GraphedTrainEvalStep provide")
        counter.record(train_loss, metrics, values)
    return values


def _as_device_stopper(early_stop, model, optimizer):
    """A host `EarlyStop` stands for its configuration: the DeviceEarlyStop of that patience, tolerance and delay."""
    if early_stop is None or isinstance(early_stop, DeviceEarlyStop):
        return early_stop
    if not isinstance(optimizer, ClipAdam):
        raise L.MrgcnError("only ClipAdam's state can be allocated ahead of its first step: take one step, then "
                           "build the DeviceEarlyStop yourself")
    optimizer.init_state()
    return DeviceEarlyStop(model, optimizer, early_stop.full_patience, early_stop.tolerance, early_stop.delay)


class GraphedTrainEvalStep(_CapturedStep):
    """`train_eval_step` captured into one hipGraph and replayed: the training step, the evaluation of both label
    sets, the metrics row, the early-stop record and the conditional snapshot of the best state, on the one capture
    stream (a single chain, no parallel branches), with no host synchronisation.

        ring = torch.zeros((8, 4), device="cuda")
        step = GraphedTrainEvalStep(model, lambda: model(X, A), idx, y, optimizer, valid=(vidx, vy),
                                    early_stop=EarlyStop(7, 0.01), metrics=ring)
        step(); ...; step.early_stop.poll()

    Captured and replayed through `Captured`.  `warmup` optimizer steps have been taken when the constructor returns
    (capturing executes nothing), but they leave no trace in the bookkeeping: the early-stop state and the ring are
    reset after the warm-up, just before the capture, so the first replay is record 1.  `early_stop`: a
    DeviceEarlyStop, or a host EarlyStop as its configuration."""

    def __init__(self, model, forward_fn, idx, targets, optimizer, valid=None, early_stop=None, metrics=None,
                 warmup: int = 3, l1_lambda: float = 0.0, l2_lambda: float = 0.0, row_sparse=None):
        if not getattr(optimizer, "capturable", False):
            raise L.MrgcnError("GraphedTrainEvalStep needs ClipAdam(..., capturable=True)")
        self.early_stop = early_stop = _as_device_stopper(early_stop, model, optimizer)
        self.metrics = metrics if metrics is not None else torch.zeros((8, 4), dtype=torch.float32, device=idx.device)
        self.counter = early_stop.state if early_stop is not None else _StopState(idx.device, 1, 0.0, _COUNT_ONLY)
        kw = dict(l1_lambda=l1_lambda, l2_lambda=l2_lambda, row_sparse=row_sparse, valid=valid, early_stop=early_stop,
                  metrics=self.metrics, counter=self.counter)

        def step():
            return train_eval_step(model, forward_fn, idx, targets, optimizer, **kw)

        def reset():
            self.counter.reset()
            self.metrics.zero_()
        self.values = self._capture(step, warmup, optimizer, reset)
        self.loss = self.values[0]

    step = _CapturedStep.__call__


def fit(model, forward_fn, train, valid, optimizer, nepoch, early_stop=None, poll=8, graphed=True,
        l1_lambda: float = 0.0, l2_lambda: float = 0.0, row_sparse=None, warmup: int = 3):
    """The reference's full-batch `train_model` loop (node_classification.py:112-230) as a generator over
    `(epoch, train_loss, train_acc, val_loss, val_acc)` — floats, epochs from 1 — with the host looking in every
    `poll` epochs only: the epochs in between run back to back (one graph replay each with `graphed=True`), their
    rows wait in a device ring of `poll` rows and are yielded at the poll.  `train`, `valid`: `(idx, targets)` pairs;
    `valid=None` trains without validation (the reference's `test_split == "test"`) and yields -1 for both validation
    values.  `early_stop`: None, a DeviceEarlyStop, or a host EarlyStop as its configuration.  A run starts at record 0:
    whatever a DeviceEarlyStop recorded before is discarded (its state is reset, graphed or not), and the first yielded
    epoch is 1.

    When a poll finds `stop` set, the rows up to and including the record that set it are yielded, the best state is
    restored in place (`restore_()`) and the generator ends.  Up to `poll - 1` epochs have then run past the stop:
    their optimizer steps happened, but the latched state ignored their records, their metrics rows were not written,
    no snapshot was taken, and the restore overwrites every tensor they changed — so they are invisible afterwards
    (other than in the dropout position and the time they took).

    A run that reaches `nepoch` without a stop is left with the LAST epoch's parameters and optimizer state, as the
    reference's loop leaves them: nothing is restored.  The best state stays in the stopper (`best_record`; pass a
    DeviceEarlyStop of your own and call its `restore_()` to get it).

    With `graphed=True` the `warmup` epochs of the capture are real optimizer steps taken before epoch 1 (see
    GraphedTrainEvalStep)."""
    idx, targets = train
    poll = max(int(poll), 1)
    ring = torch.zeros((poll, 4), dtype=torch.float32, device=idx.device)
    stopper = _as_device_stopper(early_stop, model, optimizer)
    if stopper is not None and valid is None:
        raise L.MrgcnError("fit: early stopping scores the validation loss: pass valid=(idx, targets)")
    if graphed:
        run = GraphedTrainEvalStep(model, forward_fn, idx, targets, optimizer, valid=valid, early_stop=stopper,
                                   metrics=ring, warmup=warmup, l1_lambda=l1_lambda, l2_lambda=l2_lambda,
                                   row_sparse=row_sparse)
        counter = run.counter
    else:
        counter = stopper.state if stopper is not None else _StopState(idx.device, 1, 0.0, _COUNT_ONLY)
        counter.reset()

        def run():
            return train_eval_step(model, forward_fn, idx, targets, optimizer, l1_lambda, l2_lambda, row_sparse,
                                   valid=valid, early_stop=stopper, metrics=ring, counter=counter)
    yield from _poll_records(run, counter, ring, nepoch, poll, stopper)


def _poll_records(run, counter, ring, nepoch, poll, stopper):
    """The host side of this `fit` and of `node_classification.fit`: `run()` for `nepoch` epochs in windows of `poll`,
    one look at the device per window (`counter.read()`, the ring of `poll` rows), the rows of the records made since
    the last look as `(epoch, train_loss, train_acc, val_loss, val_acc)`, `stopper.restore_()` after a latched stop."""
    done = 0
    epoch = 0
    while epoch < nepoch:
        for _ in range(min(poll, nepoch - epoch)):
            run()
            epoch += 1
        st = counter.read()
        rows = ring.cpu()
        for r in range(done, int(st.records)):
            row = rows[r % poll]
            yield (r + 1, float(row[0]), float(row[1]), float(row[2]), float(row[3]))
        done = int(st.records)
        if st.stop:
            stopper.restore_()
            return
