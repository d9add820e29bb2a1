"""DistMult link-prediction decoder on the R-GCN encoder's output — the numeric core of
`mrgcn/tasks/link_prediction.py` (scores :645-665, loss :550-554, negative sampling :247-263,
ranks :593-643, metrics :373-420), same function names and argument meaning, computed by the
HIP kernels of `csrc/distmult.hip` through the C ABI.  The reference's mini-batch flow (mkbatches
:477-530, train_model's batch loop :226-331, test_model :375-422) is mirrored further down, its
full-batch run loop with evaluation and early stopping on the device (`fit`, csrc/lp_eval.hip) and its mini-batch
run loop (`fit_batches`, csrc/lp_batches.hip) at the end of this file; logging and TSV writers are out of scope
(SURVEY §8)."""
from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple

import numpy as np
import torch

from .. import _lib
from ..stats import bump


_SORTED_BWD_MIN = 4096  # below this the scatter kernel's atomics do not collide enough to matter
_DET_SMALL_N = 4096     # mrgcn_distmult_score_bwd_det_f32 sorts up to this many triples itself (one block)
_DET_WS: dict = {}      # (device, what) -> scratch of the deterministic entries, kept (fully written before it is read)


def _det_scratch(device, what: str, nbytes: int) -> torch.Tensor:
    key = (str(device), what)
    t = _DET_WS.get(key)
    if t is None or t.numel() < nbytes:
        t = _DET_WS[key] = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
    return t


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _or_dummy(t: torch.Tensor) -> torch.Tensor:
    """A filter or exclusion list as the entries take it: an empty one as one zero (an empty tensor has no address;
    the list is empty either way)."""
    return t if t.numel() else torch.zeros(1, dtype=t.dtype, device=t.device)


def _f32_rows(t: torch.Tensor, what: str) -> torch.Tensor:
    if not t.is_cuda:
        raise _lib.MrgcnError(f"{what} must live on the GPU (mrgcn_amd has no CPU decoder)")
    if t.dtype != torch.float32 or t.dim() != 2:
        raise TypeError(f"{what} must be a 2-D float32 tensor")
    return t if t.stride(1) == 1 else t.contiguous()


def _triples(data, device) -> torch.Tensor:
    """(s, p, o) 1-D index tensors, or an [n, 3] array -> contiguous int64 [n, 3] on `device`."""
    if isinstance(data, (tuple, list)):
        si, pi, oi = (torch.as_tensor(x) for x in data)
        if not (si.dim() == pi.dim() == oi.dim() == 1 and len(si) == len(pi) == len(oi)):
            raise NotImplementedError("score_distmult_bc: only equally long 1-D index tensors (the "
                                      "train_model call); ranking goes through compute_ranks_fast")
        t = torch.stack([si.long(), pi.long(), oi.long()], 1)
    else:
        t = torch.as_tensor(data).long()
        if t.dim() != 2 or t.shape[1] != 3:
            raise ValueError("facts must be [n, 3]")
    return t.to(device).contiguous()


class SortedTriples:
    """The orders of a FIXED triple set by subject / predicate / object (what the sorted decoder backward walks), built
    once: a full-batch run scores the same training facts every epoch (tasks/link_prediction.py:231-263 — only the 20 %
    corrupted copies are drawn anew), so three per-epoch sorts of 326 k keys (0.16 ms of a 1.7 ms epoch at the
    FB15k-237 shape) shrink to nothing.  Pass it to `score_distmult_bc(..., static=...)` when the first
    `len(static)` rows of the scored triples ARE these facts, in this order (checked by identity / version)."""

    def __init__(self, triples: torch.Tensor, num_nodes: int, num_relations: int):
        t = triples.contiguous()
        if not t.is_cuda or t.dtype != torch.int64 or t.dim() != 2 or t.shape[1] != 3:
            raise TypeError("SortedTriples: int64 [n, 3] triples on the GPU")
        self.triples, self.version, self.n = t, t._version, int(t.shape[0])
        # built once, so the sorts may be anything: stable argsorts with a secondary key — inside a run of equal
        # predicate the facts follow their subject (the subject's embedding row repeats for consecutive facts instead of
        # being gathered anew), inside a run of equal subject / object the other end rises
        s_, p_, o_ = t[:, 0], t[:, 1], t[:, 2]
        nn_ = int(num_nodes)
        self.order = [torch.argsort(s_ * nn_ + o_, stable=True), torch.argsort(p_ * nn_ + s_, stable=True),
                      torch.argsort(o_ * nn_ + s_, stable=True)]
        self._tail = None
        self._tail_det = None

    def tail_orders_stable(self, nt: int, num_nodes: int, num_relations: int):
        """The same buffers for the stable radix sort (mrgcn_distmult_orders: what the deterministic backward needs)."""
        if self._tail_det is None or self._tail_det[0] != nt:
            dev = self.triples.device
            ws = torch.empty(int(_lib.load().mrgcn_distmult_orders_workspace(nt)), dtype=torch.uint8, device=dev)
            self._tail_det = (nt, [torch.empty(nt, dtype=torch.int64, device=dev) for _ in range(3)] + [ws])
        return self._tail_det[1]

    def tail_orders(self, nt: int, num_nodes: int, num_relations: int):
        """Buffers for the orders of the `nt` triples behind the fixed facts (+ the counting sort's workspace), kept."""
        if self._tail is None or self._tail[0] != (nt, num_nodes, num_relations):
            dev = self.triples.device
            ws = torch.empty(int(_lib.load().mrgcn_distmult_orders_counting_workspace(num_nodes, num_relations)),
                             dtype=torch.uint8, device=dev)
            self._tail = ((nt, num_nodes, num_relations),
                          [torch.empty(nt, dtype=torch.int64, device=dev) for _ in range(3)] + [ws])
        return self._tail[1]

    def __len__(self):
        return self.n

    def covers(self, triples: torch.Tensor) -> bool:
        """May the stored orders serve `triples`?  The facts are unchanged since the orders were built and `triples`
        starts with them (compared once, outside stream captures; afterwards the caller's contract)."""
        if self.triples._version != self.version or triples.shape[0] < self.n:
            return False
        if not getattr(self, "_checked", False) and not torch.cuda.is_current_stream_capturing():
            if not torch.equal(triples[: self.n], self.triples):
                return False
            self._checked = True
        return True


# ---- the two scorers: DistMult, and ComplEx beside it (Trouillon et al. 2016; csrc/complex.hip) --------------------
SCORERS = ("distmult", "complex")


class _Entries:
    """One scorer's entries of the library — mrgcn_{scorer}_{score_f32, ranks_both, topk, typed_ranks, typed_topk} —
    looked up by suffix on first use and kept: `entries(suffix)` -> (the entry, its `_workspace` twin or None, the
    label an error of the entry carries).  `complex`: is the scorer ComplEx?"""

    def __init__(self, scorer):
        self.scorer, self.complex, self._kept = scorer, scorer == "complex", {}

    def __call__(self, suffix):
        e = self._kept.get(suffix)
        if e is None:
            lib, name = _lib.load(), f"mrgcn_{self.scorer}_{suffix}"
            e = self._kept[suffix] = (getattr(lib, name), getattr(lib, name + "_workspace", None),
                                      f"{self.scorer}_{suffix}".replace("_f32", ""))
        return e


_ENTRIES = {s: _Entries(s) for s in SCORERS}


def _complex_width(H: int, who: str):
    if int(H) % 2:
        raise _lib.MrgcnError(f"{who}: scorer='complex' reads a row as H / 2 complex numbers: the width {int(H)} is odd")


def _scorer(scorer, who: str, H=None) -> _Entries:
    """The `scorer` keyword, checked before any kernel is touched (with `H`: ComplEx's even width too) -> its
    `_Entries`."""
    if scorer not in SCORERS:
        raise _lib.MrgcnError(f"{who}: scorer is 'distmult' or 'complex', not {scorer!r}")
    if H is not None and scorer == "complex":
        _complex_width(H, who)
    return _ENTRIES[scorer]


def _no_complex(scorer, who: str):
    """The entries whose ComplEx form is not built yet (csrc/lp_batches.hip's fused batch evaluation and run loop)."""
    if _scorer(scorer, who).complex:
        raise _lib.MrgcnError(f"{who}: scorer='complex' is not available in the mini-batch run loop and its fused "
                              "batch evaluation (csrc/lp_batches.hip scores DistMult only); use train_epoch / "
                              "evaluate_batches, or the full-batch `fit`")


# ---- the flat score backward: a plan of segments (pure), and one walk that runs it ----------------------------------
_COUNTING_MIN = 1024          # triples behind the stored facts from which a counting sort and the sorted passes pay
_COUNTING_MAX_IDS = 1 << 22   # mrgcn_distmult_orders_counting's tables: nodes and relations up to this many


def _bwd_plan(scorer, n, stored, num_nodes, num_relations, deterministic, sorted_bwd=True):
    """The segments of the backward of `n` scored triples, without a tensor or the library: a tuple of (start, count,
    orders, kernel), empty segments left out.  `stored`: how many triples at the front are the facts of a covering
    `SortedTriples` (None: there is none).  `orders` — "stored": the facts' stored orders; "counting": a counting sort
    into the SortedTriples' kept buffers; "radix": the stable radix sort, into kept buffers behind a stored segment,
    else into fresh ones; "self": none passed, the deterministic kernel sorts inside one block; None: the scatter
    kernel takes none.  `kernel` — "sorted" (runs of equal targets summed in registers along the orders), "scatter"
    (one float atomic per triple and feature), "det" (every row summed in a fixed order by one owner) or "complex"
    (ComplEx's one route: stable orders, one owner per row, with or without torch's deterministic flag).
    `sorted_bwd=False` (MRGCN_LP_SORTED_BWD=0) takes DistMult off the stored and sorted routes; ComplEx has no
    other.  DESIGN §8 has the table."""
    cx = scorer == "complex"
    use = stored is not None and (sorted_bwd or cx)
    ns = stored if use else 0
    m = n - ns
    if cx:
        head, tail = "complex", ("radix", "complex")
    elif deterministic:
        head, tail = "det", ("self" if m <= _DET_SMALL_N else "radix", "det")
    elif use:
        # the fixed facts through their stored orders, the freshly drawn ones behind them through a counting sort (four
        # launches) and the sorted passes once there are enough to collide in the scatter kernel's atomics (54 k
        # corrupted facts on 237 relation rows: 310 us at the FB15k-237 shape): no radix sort in the epoch
        counting = m >= _COUNTING_MIN and num_nodes <= _COUNTING_MAX_IDS and num_relations <= _COUNTING_MAX_IDS
        head, tail = "sorted", (("counting", "sorted") if counting else (None, "scatter"))
    else:
        head, tail = None, (("radix", "sorted") if n >= _SORTED_BWD_MIN and sorted_bwd else (None, "scatter"))
    return tuple(seg for seg in ((0, ns, "stored", head), (ns, m) + tail) if seg[1] > 0)


def _grad_buffers(E, Rel, want_E: bool, want_R: bool):
    """(dE, dR) zeroed, None where not wanted; both out of ONE buffer when both are (one fill launch per step instead
    of two), dR keeping the buffer's 16-byte alignment."""
    if want_E and want_R:
        off = (E.numel() + 3) // 4 * 4
        buf = torch.zeros(off + Rel.numel(), dtype=torch.float32, device=E.device)
        return buf[:E.numel()].view(E.shape), buf[off:].view(Rel.shape)
    return (torch.zeros_like(E, memory_format=torch.contiguous_format) if want_E else None,
            torch.zeros_like(Rel, memory_format=torch.contiguous_format) if want_R else None)


def _run_bwd_plan(plan, E, Rel, triples, g, dE, dR, static):
    """Runs the segments of `_bwd_plan` on rows [start, start + count) of `triples` and `g`, adding into dE / dR."""
    lib = _lib.load()
    N, R, H, dev = E.shape[0], Rel.shape[0], E.shape[1], E.device
    emb = (_ptr(E), E.stride(0), _ptr(Rel), Rel.stride(0), H)
    out = (_ptr(dE), dE.stride(0) if dE is not None else 0, _ptr(dR), dR.stride(0) if dR is not None else 0)
    for a, c, orders, kernel in plan:
        tr, gs = (triples, g) if c == triples.shape[0] else (triples[a:a + c], g[a:a + c])
        if orders == "stored":
            o = static.order
        elif orders == "counting":
            o = static.tail_orders(c, N, R)
            _lib.check(lib.mrgcn_distmult_orders_counting(_ptr(tr), c, N, R, _ptr(o[0]), _ptr(o[1]), _ptr(o[2]),
                                                          _ptr(o[3]), o[3].numel(), _stream()), "distmult_orders_counting")
        elif orders == "radix":
            if a:
                o = static.tail_orders_stable(c, N, R)
            else:
                o = [torch.empty(c, dtype=torch.int64, device=dev) for _ in range(3)]
                o.append(torch.empty(int(lib.mrgcn_distmult_orders_workspace(c)), dtype=torch.uint8, device=dev))
            _lib.check(lib.mrgcn_distmult_orders(_ptr(tr), c, N, R, _ptr(o[0]), _ptr(o[1]), _ptr(o[2]), _ptr(o[3]),
                                                 o[3].numel(), _stream()), "distmult_orders")
        else:
            o = (None, None, None)
        seg = emb + (_ptr(tr), c, _ptr(gs), _ptr(o[0]), _ptr(o[1]), _ptr(o[2])) + out
        if kernel == "scatter":
            _lib.check(lib.mrgcn_distmult_score_bwd_f32(*emb, _ptr(tr), c, _ptr(gs), *out, _stream()),
                       "distmult_score_bwd")
        elif kernel == "sorted":
            _lib.check(lib.mrgcn_distmult_score_bwd_sorted_f32(*seg, _stream()), "distmult_score_bwd_sorted")
        elif kernel == "det":
            ws = _det_scratch(dev, "distmult_bwd", int(lib.mrgcn_distmult_bwd_det_workspace(c, H)))
            _lib.check(lib.mrgcn_distmult_score_bwd_det_f32(*seg, _ptr(ws), ws.numel(), _stream()),
                       "distmult_score_bwd_det")
        else:
            ws = _det_scratch(dev, "complex_bwd", int(lib.mrgcn_complex_bwd_workspace(c, H)))
            _lib.check(lib.mrgcn_complex_score_bwd_f32(*seg, _ptr(ws), ws.numel(), _stream()), "complex_score_bwd")


class _Score(torch.autograd.Function):
    """The flat scores of either scorer; the backward is `_bwd_plan`'s, run by `_run_bwd_plan`."""

    @staticmethod
    def forward(ctx, E, Rel, triples, static, scorer):
        ctx.static, ctx.scorer = static, scorer
        score, _, what = _ENTRIES[scorer]("score_f32")
        n = triples.shape[0]
        scores = torch.empty(n, dtype=torch.float32, device=E.device)
        _lib.check(score(_ptr(E), E.stride(0), _ptr(Rel), Rel.stride(0), E.shape[1], _ptr(triples), n, _ptr(scores),
                         _stream()), what)
        ctx.save_for_backward(E, Rel, triples)
        return scores

    @staticmethod
    def backward(ctx, g):
        E, Rel, triples = ctx.saved_tensors
        want_E, want_R = ctx.needs_input_grad[:2]
        if not (want_E or want_R):
            return None, None, None, None, None
        g = g.contiguous().float()
        dE, dR = _grad_buffers(E, Rel, want_E, want_R)
        det = torch.are_deterministic_algorithms_enabled()
        if det:
            bump(f"deterministic.{ctx.scorer}_bwd")
        st = ctx.static
        stored = len(st) if st is not None and st.covers(triples) else None
        plan = _bwd_plan(ctx.scorer, triples.shape[0], stored, E.shape[0], Rel.shape[0], det,
                         os.environ.get("MRGCN_LP_SORTED_BWD", "1") != "0")
        _run_bwd_plan(plan, E, Rel, triples, g, dE, dR, st)
        return dE, dR, None, None, None


def score_distmult_bc(data, node_embeddings, edge_embeddings, static: "SortedTriples | None" = None):
    """link_prediction.py:645-665 for the 1-D (s, p, o) index tensors train_model passes (or an int64 [n, 3] tensor).
    `static`: the stored orders of the facts the triples START with (SortedTriples): the backward then sorts nothing."""
    E = _f32_rows(node_embeddings, "node_embeddings")
    Rel = _f32_rows(edge_embeddings, "edge_embeddings")
    return _Score.apply(E, Rel, _triples(data, E.device), static, "distmult")


def score_complex_bc(data, node_embeddings, edge_embeddings, static: "SortedTriples | None" = None):
    """`score_distmult_bc`'s twin for ComplEx (Trouillon et al. 2016): Re sum_k e_s[k] r[k] conj(e_o[k]) over the
    H / 2 complex numbers of a row (real parts first), with autograd.  Same triples, same `static` (the stored orders
    of the facts the triples START with; the triples behind them — freshly drawn negatives — are sorted anew by the
    stable radix sort).  An odd width raises `MrgcnError`."""
    H = int(node_embeddings.shape[-1])
    _scorer("complex", "score_complex_bc", H)
    E = _f32_rows(node_embeddings, "node_embeddings")
    Rel = _f32_rows(edge_embeddings, "edge_embeddings")
    if Rel.shape[1] != H:
        raise ValueError("score_complex_bc: node and edge embeddings differ in width")
    return _Score.apply(E, Rel, _triples(data, E.device), static, "complex")


class _BceLogits(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y):
        lib = _lib.load()
        x = x.contiguous()
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x)
        if torch.are_deterministic_algorithms_enabled():
            # the loss summed in block order and written (no float atomic on it)
            bump("deterministic.bce")
            ws = _det_scratch(x.device, "bce", int(lib.mrgcn_bce_logits_det_workspace(x.numel())))
            _lib.check(lib.mrgcn_bce_logits_det_f32(_ptr(x), _ptr(y), x.numel(), _ptr(loss), _ptr(dx), _ptr(ws),
                                                    ws.numel(), _stream()), "bce_logits_det")
        else:
            _lib.check(lib.mrgcn_bce_logits_f32(_ptr(x), _ptr(y), x.numel(), _ptr(loss), _ptr(dx), _stream()),
                       "bce_logits")
        ctx.save_for_backward(dx)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dx,) = ctx.saved_tensors
        return dx * g, None


def binary_crossentropy(Y_hat, Y, criterion=None):
    """link_prediction.py:550-554 with criterion = nn.BCEWithLogitsLoss() (:57); `criterion` is
    accepted for signature parity and must be that loss (or None)."""
    if criterion is not None and not isinstance(criterion, torch.nn.BCEWithLogitsLoss):
        raise NotImplementedError("only nn.BCEWithLogitsLoss is implemented on the device")
    if not Y_hat.is_cuda:
        raise _lib.MrgcnError("binary_crossentropy: scores must live on the GPU")
    return _BceLogits.apply(Y_hat.float(), Y.to(Y_hat.device).float().contiguous())


# ---- the grouped decoder: a fact and its keyed negatives scored and differentiated as one group ---------------------
GROUP_LOSSES = {"bce": 0, "softmax": 1}   # include/mrgcn_hip.h: MRGCN_GROUP_LOSS_*
_GROUP_SORTED_MIN = 1024   # facts from which the backward sums stored rows along the stored orders (below: row atomics)


def check_groups(triples, num_facts, rate):
    """The layout contract of the grouped decoder, as torch ops (CPU or GPU tensors; synchronises): `triples` is int64
    [num_facts * (1 + rate), 3], rows [0, num_facts) the facts, row num_facts + i * rate + j negative j of fact i, which
    has fact i's predicate and at least one of its two ends.  Raises `MrgcnError` naming the first offending row."""
    n, rate = int(num_facts), int(rate)
    t = torch.as_tensor(triples)
    if n < 1 or rate < 1:
        raise _lib.MrgcnError("check_groups: num_facts >= 1 and rate >= 1")
    if t.dim() != 2 or t.shape[1] != 3 or t.dtype != torch.int64:
        raise _lib.MrgcnError("check_groups: triples are int64 [num_facts * (1 + rate), 3]")
    if t.shape[0] != n * (1 + rate):
        raise _lib.MrgcnError(f"check_groups: {t.shape[0]} rows for {n} facts at rate {rate}: "
                              f"{n * (1 + rate)} expected")
    facts = t[:n].repeat_interleave(rate, dim=0)
    neg = t[n:]
    bad_p = neg[:, 1] != facts[:, 1]
    bad_e = (neg[:, 0] != facts[:, 0]) & (neg[:, 2] != facts[:, 2])
    bad = bad_p | bad_e
    if bool(bad.any()):
        k = int(torch.nonzero(bad)[0])
        what = "another predicate than" if bool(bad_p[k]) else "neither end of"
        raise _lib.MrgcnError(f"check_groups: row {n + k} (negative {k % rate} of fact {k // rate}) has {what} its fact: "
                              f"{tuple(int(v) for v in neg[k])} against {tuple(int(v) for v in t[k // rate])}")


def _check_group_ids(t, E, Rel, who):
    """The ids of the triples address rows of the embeddings (the kernels do not look; synchronises)."""
    lo, hi = t.min(0).values.tolist(), t.max(0).values.tolist()
    if min(lo) < 0 or max(hi[0], hi[2]) >= E.shape[0] or hi[1] >= Rel.shape[0]:
        raise _lib.MrgcnError(f"{who}: an id of the triples is outside the embeddings")


def _group_ws(owner, device, what: str, nbytes: int) -> torch.Tensor:
    """Scratch of the grouped decoder, allocated once and kept: on the facts' `SortedTriples` when there is one
    (`owner`), else with the deterministic entries' scratch (fully written before it is read)."""
    if owner is None:
        return _det_scratch(device, what, nbytes)
    ws = owner.__dict__.setdefault("_group_ws", {})
    t = ws.get(what)
    if t is None or t.numel() < nbytes:
        t = ws[what] = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
    return t


class _GroupLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, E, Rel, triples, n, rate, kind, weight, static):
        lib = _lib.load()
        total = triples.shape[0]
        scores = torch.empty(total, dtype=torch.float32, device=E.device)
        g = torch.empty(total, dtype=torch.float32, device=E.device)
        loss = torch.empty((), dtype=torch.float32, device=E.device)
        ws = _group_ws(static, E.device, "group_fwd", int(lib.mrgcn_distmult_group_fwd_workspace()))
        _lib.check(lib.mrgcn_distmult_group_fwd_f32(
            _ptr(E), E.stride(0), _ptr(Rel), Rel.stride(0), E.shape[1], _ptr(triples), n, rate, kind, weight,
            _ptr(scores), _ptr(g), _ptr(loss), _ptr(ws), ws.numel(), _stream()), "distmult_group_fwd")
        ctx.save_for_backward(E, Rel, triples, g)
        ctx.group = (n, rate, static)
        ctx.mark_non_differentiable(scores)
        return loss, scores

    @staticmethod
    def backward(ctx, gl, _gs):
        E, Rel, triples, g = ctx.saved_tensors
        n, rate, st = ctx.group
        lib = _lib.load()
        gl = gl.contiguous().float()
        # (both gradients out of ONE zeroed buffer, as the flat decoder's backward)
        off = (E.numel() + 3) // 4 * 4
        buf = torch.zeros(off + Rel.numel(), dtype=torch.float32, device=E.device)
        dE, dR = buf[:E.numel()].view(E.shape), buf[off:].view(Rel.shape)
        if st is not None and n >= _GROUP_SORTED_MIN and st.covers(triples):
            ws = _group_ws(st, E.device, "group_bwd", int(lib.mrgcn_distmult_group_bwd_workspace(n, rate, E.shape[1])))
            orders, wsp, wsn = [_ptr(o) for o in st.order], _ptr(ws), ws.numel()
        else:
            orders, wsp, wsn = [None] * 3, None, 0
        _lib.check(lib.mrgcn_distmult_group_bwd_f32(
            _ptr(E), E.stride(0), _ptr(Rel), Rel.stride(0), E.shape[1], _ptr(triples), n, rate, _ptr(g), _ptr(gl),
            E.shape[0], orders[0], orders[1], orders[2], _ptr(dE), dE.stride(0), _ptr(dR), dR.stride(0), wsp, wsn,
            _stream()), "distmult_group_bwd")
        return (dE if ctx.needs_input_grad[0] else None, dR if ctx.needs_input_grad[1] else None,
                None, None, None, None, None, None)


def _group_args(loss, pos_weight, who):
    """(loss kind, positive weight as a host float) of the grouped decoder's keywords; a one-element tensor is read
    here, once, outside the step."""
    if loss not in GROUP_LOSSES:
        raise _lib.MrgcnError(f"{who}: loss is one of {sorted(GROUP_LOSSES)}, not {loss!r}")
    if pos_weight is None:
        return GROUP_LOSSES[loss], 1.0
    if loss == "softmax":
        raise _lib.MrgcnError(f"{who}: pos_weight belongs to loss='bce' (the softmax loss has no labels to weigh)")
    if torch.is_tensor(pos_weight):
        if pos_weight.numel() != 1:
            raise _lib.MrgcnError(f"{who}: pos_weight is one number")
        if pos_weight.is_cuda and torch.cuda.is_current_stream_capturing():
            raise _lib.MrgcnError(f"{who}: a pos_weight tensor is read on the host: pass it outside a stream capture")
        pos_weight = float(pos_weight)
    w = float(pos_weight)
    if not (w > 0.0 and np.isfinite(w)):
        raise _lib.MrgcnError(f"{who}: pos_weight is a positive finite number")
    return GROUP_LOSSES[loss], w


def group_loss(triples, node_embeddings, edge_embeddings, num_facts, rate, loss="bce", pos_weight=None, static=None):
    """The DistMult loss (link_prediction.py:645-665, :550-554) of facts and their keyed negatives, scored and
    differentiated group by group (csrc/distmult_group.hip): a float32 device scalar carrying autograd to both embedding
    tensors; never synchronises, so a hipGraph captures it.  `triples`: int64 [num_facts * (1 + rate), 3] in
    `NegativeSampler`'s layout — rows [0, n) the facts, row n + i * rate + j negative j of fact i, with fact i's
    predicate and at least one of its ends (`check_groups`, run once per triples tensor outside stream captures).  A
    negative counts as head-corrupted when its column 0 differs from the fact's subject and as tail-corrupted
    otherwise: one equal to its fact is a tail negative with the fact's own object.

    `loss="bce"`: `BCEWithLogitsLoss(pos_weight=w)`, mean over all n (1 + rate) scores; `pos_weight` a host float or a
    one-element tensor (read once, here), None = 1.  `loss="softmax"`: the mean over facts of -log softmax of the fact's
    score among its 1 + rate scores — `cross_entropy` of the [n, 1 + rate] score matrix with target 0; takes no
    `pos_weight`.  `static`: the `SortedTriples` of the facts: from 1 024 facts on the backward then sums along the
    stored orders instead of by row atomics, and keeps its scratch there.

    Shapes the group kernels do not take — H % 4 != 0, H > 256, rows not 16-byte aligned, ids past 2^31 — and
    `torch.use_deterministic_algorithms(True)` go through `score_distmult_bc(..., static=...)` and torch's loss on its
    scores (`stats()["lp.decoder.grouped.fallback"]`): under the flag the fixed-order backward runs."""
    import torch.nn.functional as F
    kind, w = _group_args(loss, pos_weight, "group_loss")
    E = _f32_rows(node_embeddings, "node_embeddings")
    Rel = _f32_rows(edge_embeddings, "edge_embeddings")
    n, rate = int(num_facts), int(rate)
    t = triples if torch.is_tensor(triples) and triples.is_cuda and triples.dtype == torch.int64 \
        and triples.is_contiguous() else _triples(triples, E.device)
    if getattr(t, "_mrgcn_groups", None) != (n, rate):
        if torch.cuda.is_current_stream_capturing():
            if t.dim() != 2 or t.shape[0] != n * (1 + rate) or n < 1 or rate < 1:
                raise _lib.MrgcnError("group_loss: triples are [num_facts * (1 + rate), 3]")
        else:
            check_groups(t, n, rate)
            _check_group_ids(t, E, Rel, "group_loss")
            try:
                t._mrgcn_groups = (n, rate)
            except AttributeError:
                pass
    bump("lp.decoder.grouped")
    lib = _lib.load()
    if torch.are_deterministic_algorithms_enabled() or not lib.mrgcn_distmult_group_supported(
            _ptr(E), E.stride(0), _ptr(Rel), Rel.stride(0), E.shape[1], E.shape[0], Rel.shape[0], n, rate):
        bump("lp.decoder.grouped.fallback")
        scores = score_distmult_bc(t, E, Rel, static=static)
        if kind == GROUP_LOSSES["softmax"]:
            x = torch.cat([scores[:n, None], scores[n:].view(n, rate)], 1)
            return F.cross_entropy(x, torch.zeros(n, dtype=torch.int64, device=E.device))
        y = torch.zeros_like(scores)
        y[:n] = 1
        pw = None if pos_weight is None else torch.full((), w, dtype=torch.float32, device=E.device)
        return F.binary_cross_entropy_with_logits(scores, y, pos_weight=pw)
    return _GroupLoss.apply(E, Rel, t, n, rate, kind, w, static)[0]


def group_scores(triples, node_embeddings, edge_embeddings, num_facts, rate):
    """The scores the group kernels write for `triples` (float32 [num_facts * (1 + rate)], no autograd): bit for bit
    `score_distmult_bc`'s.  Raises where the group kernels do not take the shape."""
    E = _f32_rows(node_embeddings, "node_embeddings")
    Rel = _f32_rows(edge_embeddings, "edge_embeddings")
    n, rate = int(num_facts), int(rate)
    t = _triples(triples, E.device)
    check_groups(t, n, rate)
    _check_group_ids(t, E, Rel, "group_scores")
    if not _lib.load().mrgcn_distmult_group_supported(_ptr(E), E.stride(0), _ptr(Rel), Rel.stride(0), E.shape[1],
                                                      E.shape[0], Rel.shape[0], n, rate):
        raise _lib.MrgcnError("group_scores: the group kernels do not take this shape")
    with torch.no_grad():
        return _GroupLoss.apply(E.detach(), Rel.detach(), t, n, rate, 0, 1.0, None)[1]


# ---- the 1-vs-all softmax decoder (csrc/lp_all.hip) ----------------------------------------------------------------
# Every fact scored against ALL candidates on both sides under a softmax cross-entropy — the objective DistMult and
# ComplEx are normally trained with (Kadlec et al. 2017; Lacroix et al. 2018; Ruffinelli et al. 2020) — without the
# [queries, nodes] score matrix ever being stored.
ALL_SIDES = ("both", "tail", "head")


def _all_side(side, who):
    if side not in ALL_SIDES:
        raise _lib.MrgcnError(f"{who}: side is one of {ALL_SIDES}, not {side!r}")
    return side


def pair_vectors(facts, E, Rel, side="both", scorer="distmult"):
    """(Q [m, H], target [m]) of the facts (an int64 [n, 3] tensor on E's device), as torch ops under autograd
    (index_select and elementwise work, O(m H)): Q[i] is the vector whose plain dot product with a candidate's row is
    the score of fact i with that candidate as its missing end, target[i] the fact's own end.  DistMult: tail
    q = E[s] * Rel[p], target o; head q = Rel[p] * E[o], target s.  ComplEx: csrc/lp_score.hpp's pair vectors, real
    parts first — tail (xr rr - xi ri | xi rr + xr ri), head (rr xr + ri xi | rr xi - ri xr).  `side="both"`: the tail
    queries, then the head queries (m = 2 n).  `host.pair_vectors64` is the float64 mirror."""
    cx = _scorer(scorer, "pair_vectors").complex
    _all_side(side, "pair_vectors")
    H = int(E.shape[1])
    if cx:
        _complex_width(H, "pair_vectors")
    K = H // 2
    s, p, o = facts[:, 0], facts[:, 1], facts[:, 2]
    r = Rel.index_select(0, p)
    q, tg = [], []
    if side in ("both", "tail"):
        x = E.index_select(0, s)
        if cx:
            xr, xi, rr, ri = x[:, :K], x[:, K:], r[:, :K], r[:, K:]
            q.append(torch.cat([xr * rr - xi * ri, xi * rr + xr * ri], 1))
        else:
            q.append(x * r)
        tg.append(o)
    if side in ("both", "head"):
        x = E.index_select(0, o)
        if cx:
            xr, xi, rr, ri = x[:, :K], x[:, K:], r[:, :K], r[:, K:]
            q.append(torch.cat([rr * xr + ri * xi, rr * xi - ri * xr], 1))
        else:
            q.append(r * x)
        tg.append(s)
    if len(q) == 1:
        return q[0], tg[0].contiguous()
    return torch.cat(q, 0), torch.cat(tg, 0)


# Arithmetic of the score product of the two all-candidates decoders (`decoder="all"`, `decoder="kvsall"`): "f32"
# (v_mfma_f32_16x16x4_f32, exact fp32 — the default) or "bf16" (Q and E rounded to bf16 tables once per forward,
# v_mfma_f32_16x16x32_bf16 with fp32 sums, the gradient tile rounded to bf16 as the second product's operand; lse,
# softplus, the merges, the loss and both gradients stay fp32 / float64).  Process-wide, as `dense.set_matmul_dtype`;
# every entry point takes `mm=` for one call, and a backward runs what its forward ran.
SCORE_DTYPES = ("f32", "bf16")
_SCORE_DTYPE = "f32"


def set_score_dtype(dtype: str) -> str:
    """Returns the previous setting."""
    global _SCORE_DTYPE
    if dtype not in SCORE_DTYPES:
        raise _lib.MrgcnError(f"set_score_dtype: the score arithmetic is one of {SCORE_DTYPES}, not {dtype!r}")
    prev, _SCORE_DTYPE = _SCORE_DTYPE, dtype
    return prev


def score_dtype() -> str:
    return _SCORE_DTYPE


def _mm(mm, who) -> str:
    if mm is None:
        return _SCORE_DTYPE
    if mm not in SCORE_DTYPES:
        raise _lib.MrgcnError(f"{who}: mm is one of {SCORE_DTYPES} or None (the setting), not {mm!r}")
    return mm


def _bf16_table(X: torch.Tensor) -> torch.Tensor:
    """The float32 rows of X as a bf16 table [n, Hp], Hp = 32 ceil(H / 32), zeros past H (raw 16-bit rows; one cast
    kernel, stream ordered)."""
    n, H = int(X.shape[0]), int(X.shape[1])
    Hp = (H + 31) // 32 * 32
    T = torch.empty((n, Hp), dtype=torch.int16, device=X.device)
    _lib.check(_lib.load().mrgcn_cast_rows_bf16(_ptr(X), X.stride(0), n, H, _ptr(T), Hp, _stream()),
               "mrgcn_cast_rows_bf16")
    return T


def _bf16_through(X: torch.Tensor) -> torch.Tensor:
    """X rounded to bf16 with the rounding passed straight through by autograd (the materialised fallback's operands)."""
    return X + (X.bfloat16().float() - X).detach()


def _all_supported(lib, Q, E) -> bool:
    return bool(Q.shape[0] >= 1 and E.shape[0] >= 1 and lib.mrgcn_lp_all_supported(
        _ptr(Q), Q.stride(0), Q.shape[0], _ptr(E), E.stride(0), E.shape[0], E.shape[1]))


def _bf16_supported(Q, E) -> bool:
    """The bf16 kernels' shapes (mrgcn_lp_all_supported_bf16 on the tables `_bf16_table` makes: their strides and
    alignment always qualify, so the rule is the width's)."""
    H = int(E.shape[1])
    return bool(Q.shape[0] >= 1 and E.shape[0] >= 1 and H % 4 == 0 and 4 <= H <= 256)


def _all_fwd(lib, Q, E, target):
    m, N, H = Q.shape[0], E.shape[0], E.shape[1]
    out = torch.empty(3 * m + 1, dtype=torch.float32, device=E.device)
    lse, xt, loss = out[:2 * m], out[2 * m:3 * m], out[3 * m:].view(())   # (lse: the float32 values, then their remainders)
    ws = _det_scratch(E.device, "lp_all", int(lib.mrgcn_lp_all_workspace(m, N, H)))
    _lib.check(lib.mrgcn_lp_all_fwd_f32(_ptr(Q), Q.stride(0), m, _ptr(E), E.stride(0), N, H, _ptr(target), _ptr(lse),
                                        _ptr(xt), _ptr(loss), _ptr(ws), ws.numel(), _stream()), "lp_all_fwd")
    return lse, xt, loss


def _all_fwd_bf16(lib, Q, E, target):
    """-> (lse, xt, loss, Qb, Eb): the bf16 tables are made here, once, and handed on to the backward."""
    m, N, H = Q.shape[0], E.shape[0], E.shape[1]
    Qb, Eb = _bf16_table(Q), _bf16_table(E)
    if not lib.mrgcn_lp_all_supported_bf16(_ptr(Qb), Qb.stride(0), m, _ptr(Eb), Eb.stride(0), N, H):
        raise _lib.MrgcnError("the bf16 1-vs-all kernels do not take this shape")
    out = torch.empty(3 * m + 1, dtype=torch.float32, device=E.device)
    lse, xt, loss = out[:2 * m], out[2 * m:3 * m], out[3 * m:].view(())
    ws = _det_scratch(E.device, "lp_all", int(lib.mrgcn_lp_all_workspace(m, N, H)))
    _lib.check(lib.mrgcn_lp_all_fwd_bf16(_ptr(Qb), Qb.stride(0), m, _ptr(Eb), Eb.stride(0), N, H, _ptr(target),
                                         _ptr(lse), _ptr(xt), _ptr(loss), _ptr(ws), ws.numel(), _stream()),
               "lp_all_fwd_bf16")
    return lse, xt, loss, Qb, Eb


class _AllLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Q, E, target):
        lse, _, loss = _all_fwd(_lib.load(), Q, E, target)
        ctx.save_for_backward(Q, E, target, lse)
        return loss

    @staticmethod
    def backward(ctx, gl):
        Q, E, target, lse = ctx.saved_tensors
        gl = gl.contiguous().float()
        dQ = torch.empty(Q.shape, dtype=torch.float32, device=Q.device) if ctx.needs_input_grad[0] else None
        dE = torch.empty(E.shape, dtype=torch.float32, device=E.device) if ctx.needs_input_grad[1] else None
        _lib.check(_lib.load().mrgcn_lp_all_bwd_f32(
            _ptr(Q), Q.stride(0), Q.shape[0], _ptr(E), E.stride(0), E.shape[0], E.shape[1], _ptr(target), _ptr(lse),
            _ptr(gl), _ptr(dQ), Q.shape[1], _ptr(dE), E.shape[1], None, 0, _stream()), "lp_all_bwd")
        return dQ, dE, None


class _AllLossBf16(torch.autograd.Function):
    """`_AllLoss` on the bf16 kernels: the forward's tables are saved, the backward reads them (no second cast)."""
    @staticmethod
    def forward(ctx, Q, E, target):
        lse, _, loss, Qb, Eb = _all_fwd_bf16(_lib.load(), Q, E, target)
        ctx.save_for_backward(Qb, Eb, target, lse)
        ctx.width = int(E.shape[1])
        return loss

    @staticmethod
    def backward(ctx, gl):
        Qb, Eb, target, lse = ctx.saved_tensors
        m, N, H = Qb.shape[0], Eb.shape[0], ctx.width
        gl = gl.contiguous().float()
        dQ = torch.empty((m, H), dtype=torch.float32, device=Qb.device) if ctx.needs_input_grad[0] else None
        dE = torch.empty((N, H), dtype=torch.float32, device=Eb.device) if ctx.needs_input_grad[1] else None
        _lib.check(_lib.load().mrgcn_lp_all_bwd_bf16(
            _ptr(Qb), Qb.stride(0), m, _ptr(Eb), Eb.stride(0), N, H, _ptr(target), _ptr(lse), _ptr(gl), _ptr(dQ), H,
            _ptr(dE), H, None, 0, _stream()), "lp_all_bwd_bf16")
        return dQ, dE, None


def all_pairs_loss(Q, E, target, mm=None):
    """The mean softmax cross-entropy of the scores Q E^T against `target` (float32 [m, H] and [N, H] on the device,
    int64 [m]) as a float32 device scalar carrying autograd to Q and E — `F.cross_entropy(Q @ E.T, target)` without the
    [m, N] matrix (csrc/lp_all.hip); never synchronises.  Shapes the kernels do not take — H % 4 != 0, H > 256, rows
    not 16-byte aligned — materialise the matrix (`stats()["lp.decoder.all.fallback"]`).  `mm`: the score arithmetic,
    "f32" or "bf16" (None: `score_dtype()`); under "bf16" the fallback materialises the scores of the operands rounded
    to bf16, the rounding passed straight through."""
    import torch.nn.functional as F
    mm = _mm(mm, "all_pairs_loss")
    Q, E = _f32_rows(Q, "Q"), _f32_rows(E, "E")
    if Q.shape[1] != E.shape[1] or target.shape[0] != Q.shape[0]:
        raise _lib.MrgcnError("all_pairs_loss: Q [m, H], E [N, H], target [m]")
    target = target.contiguous()
    if mm == "bf16":
        if not _bf16_supported(Q, E):
            bump("lp.decoder.all.fallback")
            return F.cross_entropy(_bf16_through(Q) @ _bf16_through(E).t(), target)
        return _AllLossBf16.apply(Q, E, target)
    if not _all_supported(_lib.load(), Q, E):
        bump("lp.decoder.all.fallback")
        return F.cross_entropy(Q @ E.t(), target)
    return _AllLoss.apply(Q, E, target)


def all_lse(Q, E, target, mm=None):
    """(lse [m], xt [m]) as the forward kernel writes them — lse[q] = log sum_c exp(Q[q] . E[c]),
    xt[q] = Q[q] . E[target[q]] — without autograd, for tests and tools.  Raises where the kernels do not take the
    shape.  `mm`: as `all_pairs_loss`."""
    mm = _mm(mm, "all_lse")
    Q, E = _f32_rows(Q, "Q"), _f32_rows(E, "E")
    lib = _lib.load()
    if Q.shape[1] != E.shape[1] or target.shape[0] != Q.shape[0] or \
            not (_bf16_supported(Q, E) if mm == "bf16" else _all_supported(lib, Q, E)):
        raise _lib.MrgcnError("all_lse: the 1-vs-all kernels do not take this shape")
    with torch.no_grad():
        fwd = _all_fwd_bf16 if mm == "bf16" else _all_fwd
        lse, xt = fwd(lib, Q.detach(), E.detach(), target.contiguous())[:2]
    return lse[:Q.shape[0]], xt


def all_loss(facts, node_embeddings, edge_embeddings, side="both", scorer="distmult", mm=None):
    """The mean 1-vs-all softmax cross-entropy of the facts: every fact scored against ALL rows of `node_embeddings` as
    its missing tail and — `side="both"` — as its missing head (`side`: "both", "tail" or "head"), the fact's own end
    the target.  A float32 device scalar carrying autograd to both embedding tensors; never synchronises, so a hipGraph
    captures it.  `facts`: an int64 [n, 3] array or device tensor, n >= 1; its ids are checked once per tensor, outside
    stream captures.  `scorer`: "distmult" or "complex" (`pair_vectors` builds the query vectors; the kernels of
    csrc/lp_all.hip do not know the scorer).  Known answers other than the fact's own stay in the denominator (no
    filtering), there is no label smoothing.  Shapes the kernels do not take go through
    `F.cross_entropy(Q @ E.T, target)` (`stats()["lp.decoder.all.fallback"]`).  `mm`: the score arithmetic, "f32" or
    "bf16" (None: `score_dtype()`, which is how the steps and run loops choose it); a bf16 call also counts in
    `stats()["lp.decoder.all.bf16"]`."""
    _scorer(scorer, "all_loss")
    _all_side(side, "all_loss")
    mm = _mm(mm, "all_loss")
    E = _f32_rows(node_embeddings, "node_embeddings")
    Rel = _f32_rows(edge_embeddings, "edge_embeddings")
    t = facts if torch.is_tensor(facts) and facts.is_cuda and facts.dtype == torch.int64 and facts.dim() == 2 \
        and facts.is_contiguous() else _triples(facts, E.device)
    if t.shape[0] < 1:
        raise _lib.MrgcnError("all_loss: facts are [n, 3] with n >= 1")
    shape = (int(E.shape[0]), int(Rel.shape[0]))
    if getattr(t, "_mrgcn_all", None) != shape and not torch.cuda.is_current_stream_capturing():
        _check_group_ids(t, E, Rel, "all_loss")
        try:
            t._mrgcn_all = shape
        except AttributeError:
            pass
    bump("lp.decoder.all")
    if mm == "bf16":
        bump("lp.decoder.all.bf16")
    Q, target = pair_vectors(t, E, Rel, side, scorer)
    return all_pairs_loss(Q, E, target, mm=mm)


def _all_facts(sampler, fallback, who, decoder="all"):
    """The facts of the 1-vs-all and KvsAll decoders: `sampler.facts` (both device samplers have it; the sampler is NOT
    called, no negatives are drawn), else `fallback`."""
    if sampler is None:
        return fallback
    facts = getattr(sampler, "facts", None)
    if facts is None:
        raise _lib.MrgcnError(f"{who}: decoder={decoder!r} reads the facts from `sampler.facts` (DeviceNegativeSampler "
                              f"and NegativeSampler have it), which {type(sampler).__name__} lacks")
    return facts


# ---- the KvsAll decoder (csrc/lp_kvsall.hip) ------------------------------------------------------------------------
# Dettmers et al. 2018's "1-N scoring": every DISTINCT (s, p, ?) and (?, p, o) query of the facts scored once against
# all nodes under a binary cross-entropy whose target marks ALL known answers of the query, with label smoothing
# (Szegedy et al. 2016) — what Ruffinelli et al. 2020 found, with 1-vs-all, to train DistMult and ComplEx best.  The
# 1-vs-all softmax keeps a query's other true answers in its denominator; here they are positives.
def _smoothing(label_smoothing, who) -> float:
    eps = float(label_smoothing)
    if not 0.0 <= eps < 1.0:
        raise _lib.MrgcnError(f"{who}: label_smoothing is in [0, 1), not {label_smoothing!r}")
    return eps


class KvsAllQueries:
    """The queries of the KvsAll objective over a fixed fact set, built once on the host (`host.kvsall_queries`: the
    order of queries and answers is defined there) and kept on `device` (None: the facts' device for a tensor, else the
    current GPU; "cpu" works without one): `reps` int64 [m, 3] — one fact per query, tail queries first —, `ptr` int64
    [m + 1] / `idx` int32 [nnz] the answers of every query, `cptr` int64 [num_nodes + 1] / `cqry` int32 [nnz] the
    queries of every node, `rows` int64 [nnz] the query of every (query, answer) pair; `m`, `m_tail`, `nnz` as host
    ints.  Reads the facts on the host: not inside a stream capture."""

    def __init__(self, facts, num_nodes, num_relations, side="both", device=None):
        from .. import host
        _all_side(side, "KvsAllQueries")
        if torch.is_tensor(facts):
            if facts.is_cuda and torch.cuda.is_current_stream_capturing():
                raise _lib.MrgcnError("KvsAllQueries: the kvsall queries are built on the host, outside a stream capture")
            if device is None:
                device = facts.device
            facts = facts.detach().cpu().numpy()
        t = np.asarray(facts)
        if t.ndim != 2 or t.shape[1] != 3 or t.shape[0] < 1 or t.dtype.kind not in "iu":
            raise _lib.MrgcnError("KvsAllQueries: the kvsall facts are integer [n, 3] with n >= 1")
        try:
            reps, m_tail, ptr, idx, cptr, cqry = host.kvsall_queries(t, num_nodes, num_relations, side)
        except ValueError as e:
            raise _lib.MrgcnError(f"KvsAllQueries: {e}") from None
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.side, self.num_nodes, self.num_relations = side, int(num_nodes), int(num_relations)
        self.m, self.m_tail, self.nnz = int(len(reps)), int(m_tail), int(len(idx))
        rows = np.repeat(np.arange(self.m, dtype=np.int64), np.diff(ptr))
        self.reps, self.ptr, self.idx, self.cptr, self.cqry, self.rows = (
            torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in (reps, ptr, idx, cptr, cqry, rows))
        self.device = self.reps.device


def _kvsall_supported(lib, Q, E) -> bool:
    return bool(Q.shape[0] >= 1 and E.shape[0] >= 1 and lib.mrgcn_lp_kvsall_supported(
        _ptr(Q), Q.stride(0), Q.shape[0], _ptr(E), E.stride(0), E.shape[0], E.shape[1]))


class _KvsAllLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Q, E, kq, eps):
        lib = _lib.load()
        m, N, H = Q.shape[0], E.shape[0], E.shape[1]
        loss = torch.empty((), dtype=torch.float32, device=E.device)
        ws = _det_scratch(E.device, "lp_kvsall", int(lib.mrgcn_lp_kvsall_workspace(m, N, H)))
        _lib.check(lib.mrgcn_lp_kvsall_fwd_f32(_ptr(Q), Q.stride(0), m, _ptr(E), E.stride(0), N, H, _ptr(kq.ptr),
                                               _ptr(kq.idx), eps, None, _ptr(loss), _ptr(ws), ws.numel(), _stream()),
                   "lp_kvsall_fwd")
        ctx.save_for_backward(Q, E)
        ctx.kvsall = (kq, eps)
        return loss

    @staticmethod
    def backward(ctx, gl):
        Q, E = ctx.saved_tensors
        kq, eps = ctx.kvsall
        gl = gl.contiguous().float()
        dQ = torch.empty(Q.shape, dtype=torch.float32, device=Q.device) if ctx.needs_input_grad[0] else None
        dE = torch.empty(E.shape, dtype=torch.float32, device=E.device) if ctx.needs_input_grad[1] else None
        _lib.check(_lib.load().mrgcn_lp_kvsall_bwd_f32(
            _ptr(Q), Q.stride(0), Q.shape[0], _ptr(E), E.stride(0), E.shape[0], E.shape[1], _ptr(kq.ptr), _ptr(kq.idx),
            _ptr(kq.cptr), _ptr(kq.cqry), eps, _ptr(gl), _ptr(dQ), Q.shape[1], _ptr(dE), E.shape[1], None, 0,
            _stream()), "lp_kvsall_bwd")
        return dQ, dE, None, None


class _KvsAllLossBf16(torch.autograd.Function):
    """`_KvsAllLoss` on the bf16 kernels: the forward's tables are saved, the backward reads them (no second cast)."""
    @staticmethod
    def forward(ctx, Q, E, kq, eps):
        lib = _lib.load()
        m, N, H = Q.shape[0], E.shape[0], E.shape[1]
        Qb, Eb = _bf16_table(Q), _bf16_table(E)
        if not lib.mrgcn_lp_kvsall_supported_bf16(_ptr(Qb), Qb.stride(0), m, _ptr(Eb), Eb.stride(0), N, H):
            raise _lib.MrgcnError("the bf16 kvsall kernels do not take this shape")
        loss = torch.empty((), dtype=torch.float32, device=E.device)
        ws = _det_scratch(E.device, "lp_kvsall", int(lib.mrgcn_lp_kvsall_workspace(m, N, H)))
        _lib.check(lib.mrgcn_lp_kvsall_fwd_bf16(_ptr(Qb), Qb.stride(0), m, _ptr(Eb), Eb.stride(0), N, H, _ptr(kq.ptr),
                                                _ptr(kq.idx), eps, None, _ptr(loss), _ptr(ws), ws.numel(), _stream()),
                   "lp_kvsall_fwd_bf16")
        ctx.save_for_backward(Qb, Eb)
        ctx.kvsall = (kq, eps, int(H))
        return loss

    @staticmethod
    def backward(ctx, gl):
        Qb, Eb = ctx.saved_tensors
        kq, eps, H = ctx.kvsall
        m, N = Qb.shape[0], Eb.shape[0]
        gl = gl.contiguous().float()
        dQ = torch.empty((m, H), dtype=torch.float32, device=Qb.device) if ctx.needs_input_grad[0] else None
        dE = torch.empty((N, H), dtype=torch.float32, device=Eb.device) if ctx.needs_input_grad[1] else None
        _lib.check(_lib.load().mrgcn_lp_kvsall_bwd_bf16(
            _ptr(Qb), Qb.stride(0), m, _ptr(Eb), Eb.stride(0), N, H, _ptr(kq.ptr), _ptr(kq.idx), _ptr(kq.cptr),
            _ptr(kq.cqry), eps, _ptr(gl), _ptr(dQ), H, _ptr(dE), H, None, 0, _stream()), "lp_kvsall_bwd_bf16")
        return dQ, dE, None, None


def kvsall_pairs_loss(Q, E, queries, label_smoothing=0.0, mm=None):
    """The mean binary cross-entropy of the scores Q E^T (float32 [m, H] and [N, H] on the device) against the
    label-smoothed multi-hot target of `queries` (a `KvsAllQueries` with m queries over N nodes, on the same device):
    `F.binary_cross_entropy_with_logits(Q @ E.T, (1 - eps) Y + eps / N)` as a float32 device scalar carrying autograd
    to Q and E, without the [m, N] matrices (csrc/lp_kvsall.hip); never synchronises.  Shapes the kernels do not take —
    H % 4 != 0, H > 256, rows not 16-byte aligned — materialise both (`stats()["lp.decoder.kvsall.fallback"]`).  `mm`:
    the score arithmetic, as `all_pairs_loss`."""
    import torch.nn.functional as F
    eps = _smoothing(label_smoothing, "kvsall_pairs_loss")
    mm = _mm(mm, "kvsall_pairs_loss")
    Q, E = _f32_rows(Q, "Q"), _f32_rows(E, "E")
    if not isinstance(queries, KvsAllQueries):
        raise _lib.MrgcnError("kvsall_pairs_loss: queries is a KvsAllQueries")
    if Q.shape[1] != E.shape[1] or Q.shape[0] != queries.m or E.shape[0] != queries.num_nodes \
            or queries.device != E.device:
        raise _lib.MrgcnError("kvsall_pairs_loss: Q [m, H], E [N, H] and the kvsall queries' m, num_nodes and device")
    if mm == "bf16" and _bf16_supported(Q, E):
        return _KvsAllLossBf16.apply(Q, E, queries, eps)
    if mm == "bf16" or not _kvsall_supported(_lib.load(), Q, E):
        bump("lp.decoder.kvsall.fallback")
        if mm == "bf16":
            Q, E = _bf16_through(Q), _bf16_through(E)
        N = E.shape[0]
        Y = torch.full((queries.m, N), eps / N, dtype=torch.float32, device=E.device)
        Y[queries.rows, queries.idx.long()] = (1.0 - eps) + eps / N
        # (the m N terms added in float64 and rounded once, as the kernels' loss is)
        terms = F.binary_cross_entropy_with_logits(Q @ E.t(), Y, reduction="none")
        return (terms.sum(dtype=torch.float64) / (float(queries.m) * float(N))).float()
    return _KvsAllLoss.apply(Q, E, queries, eps)


def kvsall_loss(queries, node_embeddings, edge_embeddings, label_smoothing=0.0, scorer="distmult", mm=None):
    """The KvsAll loss of a fact set's `KvsAllQueries`: every distinct (s, p, ?) query — and (?, p, o) query, by the
    queries' side — scored against ALL rows of `node_embeddings`, all known answers of the query positives, the target
    smoothed to (1 - label_smoothing) Y + label_smoothing / N, the binary cross-entropy averaged over all m N scores
    (`kvsall_pairs_loss`).  A float32 device scalar carrying autograd to both embedding tensors; never synchronises, so
    a hipGraph captures it.  `scorer`: "distmult" or "complex" — the query vectors are `pair_vectors` of the queries'
    representative facts, the tail queries' then the head queries'; the kernels do not know the scorer.  `mm`: the score
    arithmetic, "f32" or "bf16" (None: `score_dtype()`); a bf16 call also counts in
    `stats()["lp.decoder.kvsall.bf16"]`."""
    _scorer(scorer, "kvsall_loss")
    eps = _smoothing(label_smoothing, "kvsall_loss")
    mm = _mm(mm, "kvsall_loss")
    if not isinstance(queries, KvsAllQueries):
        raise _lib.MrgcnError("kvsall_loss: queries is a KvsAllQueries (the kvsall decoder scores distinct queries, not "
                              "facts)")
    E = _f32_rows(node_embeddings, "node_embeddings")
    Rel = _f32_rows(edge_embeddings, "edge_embeddings")
    if queries.num_nodes != E.shape[0] or queries.num_relations > Rel.shape[0]:
        raise _lib.MrgcnError("kvsall_loss: the kvsall queries were built for other num_nodes / num_relations")
    bump("lp.decoder.kvsall")
    if mm == "bf16":
        bump("lp.decoder.kvsall.bf16")
    mt, q = queries.m_tail, []
    if mt:
        q.append(pair_vectors(queries.reps[:mt], E, Rel, "tail", scorer)[0])
    if mt < queries.m:
        q.append(pair_vectors(queries.reps[mt:], E, Rel, "head", scorer)[0])
    return kvsall_pairs_loss(q[0] if len(q) == 1 else torch.cat(q, 0), E, queries, eps, mm=mm)


def _kvsall_queries_of(holder, facts, num_nodes, num_relations, device):
    """The `KvsAllQueries` of the loops' facts, built on first use outside a stream capture and kept on `holder` — the
    sampler of a full-batch loop (beside `_static`), a batch's device state in the mini-batch loops."""
    get = holder.get if isinstance(holder, dict) else lambda k: getattr(holder, k, None)
    kept = get("_kvsall")
    if kept is not None and kept[0] is facts and (kept[1].num_nodes, kept[1].num_relations) == (num_nodes, num_relations):
        return kept[1]
    if torch.cuda.is_current_stream_capturing():
        raise _lib.MrgcnError("decoder='kvsall': the facts' queries are built on first use, outside a stream capture")
    kept = (facts, KvsAllQueries(facts, num_nodes, num_relations, "both", device=device))
    if isinstance(holder, dict):
        holder["_kvsall"] = kept
    else:
        holder._kvsall = kept
    return kept[1]


def _decoder_args(decoder, loss, pos_weight, samplers, who, scorer="distmult", label_smoothing=0.0):
    """The run loops' `decoder` / `loss` / `pos_weight` / `scorer` / `label_smoothing` keywords, checked before any
    kernel is touched -> the `_Decoder` they resolve to.  A `_Decoder` as `decoder` (a loop handing its record to the
    epochs it builds) is taken as it is; the samplers are checked either way."""
    if isinstance(decoder, _Decoder):
        return decoder.checked(samplers, who)
    cx = _scorer(scorer, who).complex
    eps = _smoothing(label_smoothing, who)
    if decoder == "kvsall":
        if loss == "softmax":
            raise _lib.MrgcnError(f"{who}: decoder='kvsall' is the multi-hot binary cross-entropy: it takes loss='bce' "
                                  "(a KL / softmax form of kvsall is not built)")
        if loss != "bce":
            raise _lib.MrgcnError(f"{who}: decoder='kvsall' takes loss='bce', not {loss!r}")
        if pos_weight is not None:
            raise _lib.MrgcnError(f"{who}: pos_weight is not built for decoder='kvsall'")
        return _Decoder("kvsall", "bce", None, scorer, eps).checked(samplers, who)
    if eps != 0.0:
        raise _lib.MrgcnError(f"{who}: label_smoothing belongs to decoder='kvsall', not to decoder={decoder!r}")
    if decoder not in ("triples", "grouped", "all"):
        raise _lib.MrgcnError(f"{who}: decoder is 'triples', 'grouped' or 'all', not {decoder!r}")
    if decoder == "all":
        if loss == "bce":
            raise _lib.MrgcnError(f"{who}: decoder='all' is the 1-vs-all softmax cross-entropy: pass loss='softmax' "
                                  "(a 1-vs-all BCE is not built)")
        if loss != "softmax":
            raise _lib.MrgcnError(f"{who}: decoder='all' takes loss='softmax', not {loss!r}")
        if pos_weight is not None:
            raise _lib.MrgcnError(f"{who}: pos_weight belongs to loss='bce' (the 1-vs-all softmax has no labels to "
                                  "weigh)")
        return _Decoder("all", "softmax", None, scorer, 0.0).checked(samplers, who)
    if cx and decoder == "grouped":
        raise _lib.MrgcnError(f"{who}: decoder='grouped' scores DistMult only: scorer='complex' takes the flat "
                              "decoder (decoder='triples')")
    if decoder == "triples":
        if loss != "bce" or pos_weight is not None:
            raise _lib.MrgcnError(f"{who}: loss={loss!r} / pos_weight need decoder='grouped' (the flat decoder has the "
                                  "plain BCE only)")
        return _Decoder("triples", "bce", None, scorer, 0.0).checked(samplers, who)
    _, w = _group_args(loss, pos_weight, who)
    return _Decoder("grouped", loss, None if pos_weight is None else w, scorer, 0.0).checked(samplers, who)


def _sampler_static(sampler, num_nodes, num_relations):
    """The `SortedTriples` of a `NegativeSampler`'s facts, built once per sampler (outside stream captures) and kept."""
    st = getattr(sampler, "_static", None)
    if st is None:
        if torch.cuda.is_current_stream_capturing():
            raise _lib.MrgcnError("decoder='grouped': the facts' orders are built on first use, outside a stream capture")
        st = sampler._static = SortedTriples(sampler.facts, num_nodes, num_relations)
    return st


class _Decoder(NamedTuple):
    """The steps' and run loops' decoder keywords, resolved once by `_decoder_args`: `kind` ("triples", "grouped",
    "all", "kvsall"), `loss` ("bce" / "softmax"), `pos_weight` (a host float or None), `scorer`, `label_smoothing`."""
    kind: str
    loss: str
    pos_weight: "float | None"
    scorer: str
    label_smoothing: float

    def checked(self, samplers, who):
        """-> self, after what the decoder asks of the samplers it is given (None: a batch's own facts and draws)."""
        for smp in samplers:
            if self.kind in ("all", "kvsall"):
                _all_facts(smp, None, who, self.kind)
            elif self.kind == "grouped" and not isinstance(smp, NegativeSampler):
                raise _lib.MrgcnError(f"{who}: decoder='grouped' takes NegativeSampler's layout (rate negatives behind "
                                      f"every fact): pass NegativeSampler(s), not {type(smp).__name__}")
        return self

    def scored(self, sampler, who, st=None, negatives=None):
        """What a step scores -> (triples, labels).  The `all` and `kvsall` decoders read the facts — `sampler.facts`,
        else those of the batch's device state `st` — and do not call the sampler: no negatives are drawn, labels are
        None.  The others call `sampler`, else the batch's own sampler, else append the caller's `negatives`."""
        if self.kind in ("all", "kvsall"):
            if negatives is not None:
                raise _lib.MrgcnError(f"{who}: decoder={self.kind!r} scores every node of the batch: it takes no "
                                      "negatives")
            if sampler is None and st is None:
                raise _lib.MrgcnError(f"{who}: decoder={self.kind!r} reads the facts from `sampler.facts`: pass a "
                                      "sampler")
            return _all_facts(sampler, None if st is None else st["facts"], who, self.kind), None
        if sampler is not None or st is None:
            return sampler()
        if negatives is None:
            return st["sampler"]()
        facts = st["facts"]
        neg = torch.as_tensor(np.asarray(negatives), dtype=torch.int64).to(facts.device)
        triples = torch.cat([facts, neg.reshape(-1, 3)])
        labels = torch.ones(triples.shape[0], dtype=torch.float32, device=facts.device)
        labels[facts.shape[0]:] = 0
        return triples, labels

    def loss_of(self, triples, labels, E, Rel, static, sampler, holder=None):
        """The decoder line of every step and run loop: the flat BCE of `score_distmult_bc` (`scorer="complex"`: of
        `score_complex_bc`), or the grouped loss over `sampler`'s groups (`static` None: the sampler's own stored
        orders), or — `all`, `triples` then the facts alone — the 1-vs-all softmax cross-entropy on both sides
        (`all_loss`), or — `kvsall`, `triples` again the facts — the KvsAll loss of their distinct queries
        (`kvsall_loss`; the queries are kept on `holder`, None: on the sampler)."""
        if self.kind == "all":
            return all_loss(triples, E, Rel, side="both", scorer=self.scorer)
        if self.kind == "kvsall":
            kq = _kvsall_queries_of(sampler if holder is None else holder, triples, int(E.shape[0]), int(Rel.shape[0]),
                                    E.device)
            return kvsall_loss(kq, E, Rel, self.label_smoothing, self.scorer)
        if self.kind != "grouped":
            score = score_complex_bc if self.scorer == "complex" else score_distmult_bc
            return binary_crossentropy(score(triples, E, Rel, static=static), labels)
        if static is None:
            static = _sampler_static(sampler, int(E.shape[0]), int(Rel.shape[0]))
        return group_loss(triples, E, Rel, sampler.n, sampler.rate, loss=self.loss, pos_weight=self.pos_weight,
                          static=static)


def sample_negatives(batch_data: np.ndarray, rng=np.random):
    """train_model's within-batch corruption (link_prediction.py:239-263): 20 % of the positives
    are copied, half get a random in-batch head, half a random in-batch tail.  Returns
    (corrupted [ncorrupt, 3], labels float32 [n + ncorrupt]).  `rng`: np.random or a RandomState
    (the reference uses the global np.random)."""
    n = batch_data.shape[0]
    batch_nodes = np.union1d(batch_data[:, 0], batch_data[:, 2])
    ncorrupt = n // 5
    neg_idx = rng.choice(np.arange(n), ncorrupt, replace=False)
    nhead = ncorrupt // 2
    ntail = ncorrupt - nhead
    corrupted = np.empty((ncorrupt, 3), dtype=int)
    corrupted[:] = batch_data[neg_idx]
    corrupted[:nhead, 0] = rng.choice(batch_nodes, nhead)
    if ntail:
        corrupted[-ntail:, 2] = rng.choice(batch_nodes, ntail)
    Y = np.ones(n + ncorrupt, dtype=np.float32)
    if ncorrupt:
        Y[-ncorrupt:] = 0
    return corrupted, Y


def sample_negatives_device(batch_data: torch.Tensor, generator=None):
    """The same corruption scheme drawn on the device (a torch generator instead of np.random, so
    not the reference's random stream): `batch_data` int64 [n, 3] on the GPU -> (corrupted
    [n // 5, 3], labels float32 [n + n // 5]), no host round trip."""
    n = batch_data.shape[0]
    dev = batch_data.device
    # the nodes of the batch: a sort-based unique (half of this function's device time) — kept for the tensor it was
    # computed from while that tensor is unchanged (a full-batch run passes the same training facts every epoch)
    cached = getattr(batch_data, "_mrgcn_nodes", None)
    if cached is not None and cached[0] == batch_data._version:
        nodes = cached[1]
    else:
        nodes = torch.unique(torch.cat([batch_data[:, 0], batch_data[:, 2]]))
        try:
            batch_data._mrgcn_nodes = (batch_data._version, nodes)
        except AttributeError:
            pass
    ncorrupt = n // 5
    # ncorrupt distinct facts: a keyed bijection of [0, n) evaluated at 0..ncorrupt-1 (one launch; a randperm sorts n keys)
    seed = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, device=dev, generator=generator)
    neg_idx = torch.empty(ncorrupt, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mrgcn_random_subset_i64(n, ncorrupt, _ptr(seed), _ptr(neg_idx), _stream()), "random_subset")
    nhead = ncorrupt // 2
    ntail = ncorrupt - nhead
    corrupted = batch_data[neg_idx].clone()
    pick = lambda k: nodes[torch.randint(0, nodes.numel(), (k,), device=dev, generator=generator)]  # noqa: E731
    corrupted[:nhead, 0] = pick(nhead)
    if ntail:
        corrupted[ncorrupt - ntail:, 2] = pick(ntail)
    Y = torch.ones(n + ncorrupt, dtype=torch.float32, device=dev)
    Y[n:] = 0
    return corrupted, Y


class DeviceNegativeSampler:
    """`sample_negatives_device` for a FIXED fact set, without its per-epoch torch traffic: the facts sit at the head of
    one [n + n // 5, 3] buffer, a single launch (mrgcn_corrupt_triples_i64) writes the corrupted copies behind them, the
    labels are built once.  `triples, labels = sampler()` — the same tensors every call (their contents change): what a
    captured epoch wants.  The draws come from a 64-bit seed taken from torch's generator per call."""

    def __init__(self, facts: torch.Tensor, generator=None):
        n = int(facts.shape[0])
        dev = facts.device
        self.n, self.ncorrupt = n, n // 5
        self.nhead = self.ncorrupt // 2
        self.generator = generator
        self.buf = torch.empty((n + self.ncorrupt, 3), dtype=torch.int64, device=dev)
        self.buf[:n] = facts
        self.facts = self.buf[:n]
        self.nodes = torch.unique(torch.cat([facts[:, 0], facts[:, 2]]))
        self.labels = torch.ones(n + self.ncorrupt, dtype=torch.float32, device=dev)
        self.labels[n:] = 0

    def __call__(self):
        dev = self.buf.device
        seed = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, device=dev, generator=self.generator)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().mrgcn_corrupt_triples_i64(
                _ptr(self.buf), self.n, _ptr(self.nodes), int(self.nodes.numel()), _ptr(seed), self.ncorrupt, self.nhead,
                C.c_void_p(self.buf.data_ptr() + 24 * self.n), _stream()), "corrupt_triples")
        return self.buf, self.labels


def _fact_keys_device(triples: torch.Tensor, num_nodes: int, num_relations: int, to_global=None) -> torch.Tensor:
    """`host.fact_keys` with torch ops on the triples' device (built once per sampler: no kernel of its own)."""
    s_, p_, o_ = triples[:, 0], triples[:, 1], triples[:, 2]
    if to_global is not None:
        s_, o_ = to_global[s_], to_global[o_]
    return torch.sort((s_ * int(num_relations) + p_) * int(num_nodes) + o_).values.contiguous()


class TypedCandidates:
    """Type constraints for link prediction (Krompass, Baier, Tresp: "Type-Constrained Representation Learning in
    Knowledge Graphs", ISWC 2015): per relation the nodes that may stand at its tail (its range) and at its head (its
    domain), as a CSR over 2 * num_relations slots — slot 2 p the TAIL candidates of relation p, slot 2 p + 1 its HEAD
    candidates.  `ptr` (int64 [2 R + 1]) and `idx` (int32, every list ascending and duplicate free) are device tensors;
    `ptr_host` / `idx_host` are their numpy copies, which every host-side check reads.  `TypedCandidates(ptr, idx,
    num_nodes, num_relations)` takes DECLARED lists and validates them on the host (ValueError: `ptr` not monotone, an
    id outside [0, num_nodes), a list not sorted or with duplicates); `from_facts` builds the OBSERVED sets;
    `full` makes every list 0 .. N - 1 (the typed kernels then compute what the untyped ones do).  Accepted by
    `NegativeSampler(candidates=)`, `TypedFacts` / `rank_typed` / `evaluate_typed` and `predict_topk(candidates=)`."""

    def __init__(self, ptr, idx, num_nodes, num_relations, device=None):
        from ..host import check_typed_candidates
        as_np = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)   # noqa: E731
        self.ptr_host, self.idx_host = check_typed_candidates(as_np(ptr), as_np(idx), num_nodes, num_relations)
        self.num_nodes, self.num_relations = int(num_nodes), int(num_relations)
        if device is None:
            device = ptr.device if torch.is_tensor(ptr) and ptr.is_cuda else (
                "cuda" if torch.cuda.is_available() else "cpu")
        self.ptr = torch.from_numpy(self.ptr_host).to(device)
        self.idx = _dev_or_dummy(self.idx_host, device)
        self.lengths_host = np.diff(self.ptr_host)
        self._keys = None

    @classmethod
    def from_facts(cls, known, num_nodes, num_relations, device=None):
        """range(p) = {o : (., p, o) in known} in slot 2 p, domain(p) = {s : (s, p, .) in known} in slot 2 p + 1
        (`mrgcn_amd.host.typed_candidates`)."""
        from ..host import typed_candidates
        kn = known.detach().cpu().numpy() if torch.is_tensor(known) else np.asarray(known)
        return cls(*typed_candidates(kn, num_nodes, num_relations), num_nodes, num_relations, device=device)

    @classmethod
    def full(cls, num_nodes, num_relations, device=None):
        N, R = int(num_nodes), int(num_relations)
        return cls(np.arange(2 * R + 1, dtype=np.int64) * N, np.tile(np.arange(N, dtype=np.int32), 2 * R), N, R,
                   device=device)

    def to(self, device):
        """The same lists on `device` (the host copies are shared)."""
        d = torch.device(device)
        if d.type == self.ptr.device.type and (d.index is None or d.index == self.ptr.device.index):
            return self
        return TypedCandidates(self.ptr_host, self.idx_host, self.num_nodes, self.num_relations, device=device)

    def slot(self, relation: int, side="tail"):
        """The numpy list of `relation`'s tail ("tail") or head ("head") candidates."""
        s = 2 * int(relation) + _side(side)
        return self.idx_host[self.ptr_host[s]:self.ptr_host[s + 1]]

    def contains(self, slots, nodes):
        """Per (slot, node) pair: is the node in the slot's list?  (host arrays)"""
        if self._keys is None:   # the lists as one rising key array
            self._keys = (np.repeat(np.arange(2 * self.num_relations, dtype=np.int64), self.lengths_host)
                          * self.num_nodes + self.idx_host)
        k = np.asarray(slots, dtype=np.int64) * self.num_nodes + np.asarray(nodes, dtype=np.int64)
        if len(self._keys) == 0:
            return np.zeros(k.shape, bool)
        return self._keys[np.minimum(np.searchsorted(self._keys, k), len(self._keys) - 1)] == k


def _relation_tiles(rel, what: str):
    """Groups items by relation for the typed kernels: `order` (int64: the items' indices relation by relation, stable),
    `tile_ptr` (int64 [ntiles + 1]) over that sequence — tiles of at most 8 (csrc/lp_score.hpp: kLpFB) items of ONE
    relation — and `tile_rel` (int32 [ntiles])."""
    rel = np.asarray(rel, dtype=np.int64)
    order = np.argsort(rel, kind="stable")
    rs = rel[order]
    starts = np.flatnonzero(np.r_[True, rs[1:] != rs[:-1]]) if len(rs) else np.zeros(0, np.int64)
    ends = np.r_[starts[1:], len(rs)] if len(rs) else np.zeros(0, np.int64)
    per_run = (ends - starts + 7) // 8                                   # tiles of each relation's run
    run_of_tile = np.repeat(np.arange(len(starts)), per_run)
    first = np.cumsum(per_run) - per_run                                 # a run's first tile
    begin = starts[run_of_tile] + 8 * (np.arange(len(run_of_tile)) - first[run_of_tile])
    tile_ptr = np.r_[begin, len(rs)].astype(np.int64)
    tile_rel = rs[begin].astype(np.int32) if len(begin) else np.zeros(0, np.int32)
    assert np.all(np.diff(tile_ptr) >= 1) and np.all(np.diff(tile_ptr) <= 8), what
    return order.astype(np.int64), tile_ptr, tile_rel


def _dev_or_dummy(a: np.ndarray, device) -> torch.Tensor:
    """A host array on the device, under `_or_dummy`'s rule."""
    return _or_dummy(torch.from_numpy(np.ascontiguousarray(a)).to(device))


class NegativeSampler:
    """`rate` negatives per fact, corrupted against `candidates` (None: every node 0 .. num_nodes - 1) and refused when
    they are known facts — what the reference's sampler (link_prediction.py:247-264: 20 % of the facts, nodes of the
    batch, never checked; `DeviceNegativeSampler`) does not offer.  `DeviceNegativeSampler`'s contract: the facts sit at
    the head of one [n * (1 + rate), 3] buffer (`.facts`, `.buf`), `.labels` (n ones, n * rate zeros) is built once,
    `triples, labels = sampler()` is two launches (mrgcn_negatives_draw_i64: the draw and the move of its position) and
    returns the same tensors every call, nothing synchronised — capturable; negative j of fact i is row n + i * rate + j.

    `known`: None — the facts themselves —, an [m, 3] array or tensor of GLOBAL triples (train + valid + test,
    typically) or False (unfiltered: only the fact's own end is refused); their sorted keys are built here, once.
    `to_global` (an id tensor): the facts and candidates hold local ids, position i standing for node to_global[i] of
    the graph the keys speak of.  `side`: "both" (a random bit per negative), "tail" or "head".  `seed` (None:
    `torch.initial_seed()`) and the position live in `.state`, two int64 on the device; `reseed` rewrites them in place,
    also under a captured graph.  `.unresolved` flags the negatives whose MRGCN_NEG_MAX_ATTEMPTS draws were all refused
    (the last draw stands: it may be a known fact with label 0); `num_unresolved()` reads the count back.

    `candidates` may be a `TypedCandidates`: the type-constrained draw (mrgcn_negatives_draw_typed_i64) — the new tail
    of a fact of relation p comes from the relation's tail candidates, the new head from its head candidates; the same
    Philox counter, side bit and refusals, so with `TypedCandidates.full` the buffer equals the untyped sampler's bit
    for bit.  A fact whose relation has an EMPTY list on a side the sampler may draw raises ValueError here (host,
    once); a list whose only node is the end it replaces is refused at every attempt and flagged in `.unresolved`.
    Typed lists hold global ids: together with `to_global` they raise `MrgcnError`.  Everything else — the tensors, the
    two launches, the capture, `train_step`, `fit`, both flat and grouped decoders — is unchanged;
    `stats()["lp.negatives.typed"]` counts these calls."""

    def __init__(self, facts, num_nodes, num_relations, rate=1, known=None, candidates=None, to_global=None,
                 side="both", seed=None):
        from .. import functional as Fn
        from ..host import NEG_SIDES
        facts = torch.as_tensor(np.asarray(facts) if not torch.is_tensor(facts) else facts).long()
        if facts.dim() != 2 or facts.shape[1] != 3:
            raise ValueError("NegativeSampler: facts must be [n, 3]")
        if isinstance(candidates, TypedCandidates):   # (host checks first: they answer without a device)
            if to_global is not None:
                raise _lib.MrgcnError("NegativeSampler: typed candidates hold global ids; batch-local ids "
                                      "(to_global) are not supported with them")
            if side not in NEG_SIDES:
                raise ValueError(f"NegativeSampler: side is one of {sorted(NEG_SIDES)}, not {side!r}")
            if candidates.num_nodes != int(num_nodes) or candidates.num_relations != int(num_relations):
                raise ValueError("NegativeSampler: the typed candidates were built for another num_nodes / "
                                 "num_relations")
            rel = facts[:, 1].cpu().numpy()
            if len(rel) and (rel.min() < 0 or rel.max() >= candidates.num_relations):
                raise ValueError(f"NegativeSampler: relation ids must lie in [0, {candidates.num_relations})")
            for sd, name in ((0, "tail"), (1, "head")):
                if NEG_SIDES[side] in (0, 1 + sd):
                    empty = candidates.lengths_host[2 * rel + sd] == 0
                    if empty.any():
                        raise ValueError(f"NegativeSampler: relation {int(rel[empty][0])} has no {name} candidates, "
                                         f"but the sampler may draw that side")
        if not facts.is_cuda:
            facts = facts.cuda()
        dev = facts.device
        if side not in NEG_SIDES:
            raise ValueError(f"NegativeSampler: side is one of {sorted(NEG_SIDES)}, not {side!r}")
        n, rate = int(facts.shape[0]), int(rate)
        N, R = int(num_nodes), int(num_relations)
        if rate < 1 or N < 1 or R < 1 or N * R * N >= 1 << 63:
            raise ValueError("NegativeSampler: rate >= 1 and num_nodes * num_relations * num_nodes < 2^63")
        self.n, self.rate, self.num_nodes, self.num_relations, self.side = n, rate, N, R, NEG_SIDES[side]
        self.buf = torch.empty((n * (1 + rate), 3), dtype=torch.int64, device=dev)
        self.buf[:n] = facts
        self.facts = self.buf[:n]
        self.labels = torch.ones(n * (1 + rate), dtype=torch.float32, device=dev)
        self.labels[n:] = 0
        self.unresolved = torch.zeros(n * rate, dtype=torch.uint8, device=dev)
        self.to_global = None if to_global is None else torch.as_tensor(to_global).long().to(dev).contiguous()
        self.typed = None
        if isinstance(candidates, TypedCandidates):
            self.typed = candidates.to(dev)
            self.candidates, self.n_cand = None, N
        elif candidates is None:
            self.candidates, self.n_cand = None, (N if self.to_global is None else int(self.to_global.numel()))
        else:
            self.candidates = torch.as_tensor(candidates).long().to(dev).contiguous()
            self.n_cand = int(self.candidates.numel())
        if self.n_cand < 1:
            raise ValueError("NegativeSampler: no candidates")
        if known is False:
            self.keys = None
        elif known is None:
            self.keys = _fact_keys_device(self.facts, N, R, self.to_global)
        else:
            self.keys = _fact_keys_device(_triples(known.cpu().numpy() if torch.is_tensor(known) else known, dev), N, R)
        if self.keys is not None and self.keys.numel() == 0:
            self.keys = None
        self.state = Fn.node_dropout_state(torch.initial_seed() if seed is None else seed, 0, dev)

    def reseed(self, seed, position=0):
        """Rewrites {seed, position} in place (a copy into `.state`: the captured launches read the same memory)."""
        from .. import functional as Fn
        self.state.copy_(Fn.node_dropout_state(seed, position, self.state.device))

    def num_unresolved(self) -> int:
        return int(self.unresolved.sum())

    def __call__(self):
        if self.typed is not None:
            with torch.cuda.device(self.buf.device):
                _lib.check(_lib.load().mrgcn_negatives_draw_typed_i64(
                    _ptr(self.buf), self.n, self.rate, _ptr(self.typed.ptr), _ptr(self.typed.idx), _ptr(self.keys),
                    int(self.keys.numel()) if self.keys is not None else 0, self.num_nodes, self.num_relations,
                    self.side, _ptr(self.state), C.c_void_p(self.buf.data_ptr() + 24 * self.n), _ptr(self.unresolved),
                    _stream()), "negatives_draw_typed")
            bump("lp.negatives.typed")
            return self.buf, self.labels
        with torch.cuda.device(self.buf.device):
            _lib.check(_lib.load().mrgcn_negatives_draw_i64(
                _ptr(self.buf), self.n, self.rate, _ptr(self.candidates), self.n_cand, _ptr(self.to_global),
                _ptr(self.keys), int(self.keys.numel()) if self.keys is not None else 0, self.num_nodes,
                self.num_relations, self.side, _ptr(self.state), C.c_void_p(self.buf.data_ptr() + 24 * self.n),
                _ptr(self.unresolved), _stream()), "negatives_draw")
        bump("lp.negatives.keyed")
        return self.buf, self.labels


def batch_negative_samplers(num_nodes, num_relations, rate=1, known=None, side="both", seed=None):
    """The `samplers` factory of `fit_batches` / `BatchFitEpochs` for keyed negatives: `samplers(i, batch, facts)` is a
    `NegativeSampler` over training batch i's facts whose candidates are the batch's local ids
    0 .. len(batch.node_index) - 1 (the nodes the batch has embeddings for) and whose filter is the GLOBAL one — local
    ids go through `batch.node_index`; a batch's facts keep their global relation ids (`mkbatches`).  `known`: None —
    each batch's own facts —, global triples, or False, as `NegativeSampler`'s.  Sampler i draws under `seed + i`
    (None: `torch.initial_seed()`)."""
    base = torch.initial_seed() if seed is None else int(seed)
    shared: dict = {}   # device -> the sorted keys of `known`, built once for all batches

    def samplers(i, batch, facts):
        st = getattr(batch, "_mrgcn_lp", None)
        dev = st["device"] if st is not None else torch.device("cuda", torch.cuda.current_device())
        f = st["facts"] if st is not None else torch.as_tensor(np.asarray(facts), dtype=torch.int64).to(dev)
        node_index = torch.as_tensor(np.asarray(batch.node_index) if not torch.is_tensor(batch.node_index)
                                     else batch.node_index).long().to(dev)
        own = known if known is None or known is False else False
        smp = NegativeSampler(f, num_nodes, num_relations, rate=rate, known=own, to_global=node_index, side=side,
                              seed=base + i)
        if known is not None and known is not False:
            if dev not in shared:
                shared[dev] = _fact_keys_device(
                    _triples(known.cpu().numpy() if torch.is_tensor(known) else known, dev), num_nodes, num_relations)
            smp.keys = shared[dev] if shared[dev].numel() else None
        return smp
    return samplers


def filter_lists(data: np.ndarray):
    """The filter of compute_ranks_fast(filtered=True) (truedicts :568-591 + filter_scores_
    :667-689) as CSR lists: per fact, the sorted nodes that are other true objects of (s, p)
    [tail corruption] / other true subjects of (p, o) [head corruption] among `data`."""
    data = np.asarray(data, dtype=np.int64)
    nf = len(data)

    def build(key_a, key_b, ans):
        # group facts by (key_a, key_b); members of a group = unique answers
        order = np.lexsort((ans, key_b, key_a))
        ka, kb, an = key_a[order], key_b[order], ans[order]
        new_grp = np.ones(nf, bool)
        new_grp[1:] = (ka[1:] != ka[:-1]) | (kb[1:] != kb[:-1])
        uniq = new_grp.copy()
        uniq[1:] |= an[1:] != an[:-1]
        gid_sorted = np.cumsum(new_grp) - 1                # group id per sorted fact
        ngrp = int(gid_sorted[-1]) + 1 if nf else 0
        gptr = np.zeros(ngrp + 1, np.int64)
        np.add.at(gptr, gid_sorted[uniq] + 1, 1)
        gptr = np.cumsum(gptr)
        members = an[uniq]                                  # sorted within each group
        gid = np.empty(nf, np.int64)
        gid[order] = gid_sorted
        cnt = gptr[gid + 1] - gptr[gid] - 1                 # minus the fact's own answer
        ptr = np.zeros(nf + 1, np.int64)
        np.cumsum(cnt, out=ptr[1:])
        idx = np.empty(int(ptr[-1]), np.int32)
        # expand: for fact f, members of its group except ans[f]
        rep = np.repeat(np.arange(nf), cnt + 1)
        off = np.arange(len(rep)) - np.repeat(np.cumsum(cnt + 1) - (cnt + 1), cnt + 1)
        cand = members[gptr[gid[rep]] + off]
        keep = cand != ans[rep]
        idx[:] = cand[keep]
        return ptr, idx

    if nf == 0:
        z = np.zeros(1, np.int64)
        return z, np.zeros(0, np.int32), z.copy(), np.zeros(0, np.int32)
    tp, ti = build(data[:, 0], data[:, 1], data[:, 2])
    hp, hi = build(data[:, 1], data[:, 2], data[:, 0])
    return tp, ti, hp, hi


def _rank_inputs(scorer, who, node_embeddings, edge_embeddings):
    """What every rank and top-k entry starts with: the scorer keyword and ComplEx's even width checked first, then
    the detached float32 tables of equal width -> (E, Rel, N, H, the scorer's `_Entries`)."""
    entries = _scorer(scorer, who, node_embeddings.shape[-1])
    E = _f32_rows(node_embeddings.detach(), "node_embeddings")
    Rel = _f32_rows(edge_embeddings.detach(), "edge_embeddings")
    N, H = int(E.shape[0]), int(E.shape[1])
    if Rel.shape[1] != H:
        raise ValueError(f"{who}: node and edge embeddings differ in width")
    return E, Rel, N, H, entries


def _check_lists(lists, nf, who):
    ls = list(lists)
    if len(ls) != 4 or not all(torch.is_tensor(a) and a.is_cuda for a in ls):
        raise _lib.MrgcnError(f"{who}: lists are the four device tensors of filter_lists")
    if not (ls[0].dtype == ls[2].dtype == torch.int64 and ls[1].dtype == ls[3].dtype == torch.int32
            and ls[0].numel() == ls[2].numel() == nf + 1):
        raise _lib.MrgcnError(f"{who}: lists are (int64 [n + 1], int32, int64 [n + 1], int32)")
    return [_or_dummy(a.contiguous()) for a in ls]


def _device_filter_lists(facts, device):
    """`filter_lists(facts)` as the four device tensors the rank entries take."""
    return [_or_dummy(torch.from_numpy(a).to(device)) for a in filter_lists(np.asarray(facts))]


def _rank_one_side(E, Rel, tr, lists=None):
    """mrgcn_distmult_ranks: the int64 [2 * nf] ranks of the device triples `tr` (tail corruption, then head
    corruption) in one rank type — filtered by `lists` (`_device_filter_lists`), raw without."""
    nf, N, H, dev = int(tr.shape[0]), E.shape[0], E.shape[1], E.device
    ranks = torch.empty(2 * nf, dtype=torch.int64, device=dev)
    if nf == 0:
        return ranks
    lib = _lib.load()
    ls = lists if lists is not None else [None] * 4
    ws_bytes = lib.mrgcn_distmult_ranks_workspace(N, H, nf)
    ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.int32, device=dev)
    _lib.check(lib.mrgcn_distmult_ranks(_ptr(E), E.stride(0), N, _ptr(Rel), Rel.stride(0), H, _ptr(tr), nf,
                                        _ptr(ls[0]), _ptr(ls[1]), _ptr(ls[2]), _ptr(ls[3]), _ptr(ws), ws_bytes,
                                        _ptr(ranks), _stream()), "distmult_ranks")
    return ranks


def compute_ranks_fast(data, node_embeddings, edge_embeddings, batch_size=100, filtered=False, scorer="distmult"):
    """link_prediction.py:593-643.  Returns the int64 [2 * num_facts] ranks (tail corruption
    then head corruption) on the embeddings' device.  `batch_size` (the reference's
    mrr_batchsize, a memory knob for its [facts, nodes] score matrix) is accepted and unused:
    scores are never materialised here.  `scorer="complex"`: ComplEx scores (`rank_both` over one part; an odd width
    raises `MrgcnError`)."""
    E, Rel, _, _, entries = _rank_inputs(scorer, "compute_ranks_fast", node_embeddings, edge_embeddings)
    facts_np = data.cpu().numpy() if torch.is_tensor(data) else np.asarray(data)
    if not entries.complex:   # (`_triples` checks the shape, of an empty array too)
        tr = _triples(facts_np, E.device)
        return _rank_one_side(E, Rel, tr, _device_filter_lists(facts_np, E.device) if filtered and len(tr) else None)
    if len(facts_np) == 0:
        return torch.empty(0, dtype=torch.int64, device=E.device)
    lists = _device_filter_lists(facts_np, E.device) if filtered else None
    raw, flt = rank_both(facts_np, E, Rel, lists=lists, scorer=scorer)
    return flt if filtered else raw


def mrr_hits(ranks, K=(1, 3, 10)):
    """One batch's metrics as test_model computes them (link_prediction.py:403-407)."""
    r = ranks.float()
    return torch.mean(1.0 / r).item(), [float(torch.mean((ranks <= k).float())) for k in K]


# ---- mini-batch link prediction (link_prediction.py:191-530 with gcn_batchsize > 0) -----------------------------
def mkbatches(A, X, data, gcn_batchsize, mrr_batchsize, num_layers, plan=None):
    """link_prediction.py:477-530: batches of the nodes that occur in `data` (`gcn_batchsize` of them each, in rising
    id order), each batch's facts (those with a batch node as head or tail: a fact can sit in two batches) cut by
    `np.array_split` into parts of about `mrr_batchsize` facts, every part with the sorted nodes of its facts
    (`union1d`) and its facts remapped to positions among them.  Returns [(batch, facts)], as the reference does.
    `plan` (the full graph's GraphPlan on the GPU): the batches are masked batches on it (`MiniBatch(plan=...,
    wide_features=True)`, no row slices: wide encoder layers with literal features run on it too); otherwise the reference's `MiniBatch` slices of the scipy CSR `A`.  gcn_batchsize <= 0: one FullBatch per
    part, facts keep their global ids (:536-545)."""
    from ..data.batch import FullBatch, MiniBatch
    data = np.asarray(data)
    sample_nodes = np.union1d(data[:, 0], data[:, 2])
    num_nodes = len(sample_nodes)
    if gcn_batchsize <= 0:
        gcn_batchsize = num_nodes
    if mrr_batchsize <= 0:
        mrr_batchsize = data.shape[0]
    batch_slices = [slice(begin, min(begin + gcn_batchsize, num_nodes)) for begin in range(0, num_nodes, gcn_batchsize)]
    batches = []
    if len(batch_slices) > 1:
        for slce in batch_slices:
            batch_node_idx = sample_nodes[slce]
            data_mask = np.isin(data[:, 0], batch_node_idx) | np.isin(data[:, 2], batch_node_idx)
            batch_data = data[data_mask]
            num_samples = batch_data.shape[0]
            for subset in np.array_split(np.arange(num_samples), max(num_samples // mrr_batchsize, 1)):
                data_subset = np.copy(batch_data[subset])
                subset_node_idx = np.union1d(data_subset[:, 0], data_subset[:, 2])
                # (the reference's {node: position} map: subset_node_idx is sorted and holds every head and tail)
                data_subset[:, 0] = np.searchsorted(subset_node_idx, data_subset[:, 0])
                data_subset[:, 2] = np.searchsorted(subset_node_idx, data_subset[:, 2])
                if plan is not None:
                    batch = MiniBatch(None, X, subset_node_idx, num_layers, plan=plan, wide_features=True)
                else:
                    batch = MiniBatch(A, X, subset_node_idx, num_layers)
                batches.append((batch, data_subset))
    else:
        num_samples = data.shape[0]
        for subset in np.array_split(np.arange(num_samples), max(num_samples // mrr_batchsize, 1)):
            data_subset = np.copy(data[subset])
            subset_node_idx = np.union1d(data_subset[:, 0], data_subset[:, 2])
            batches.append((FullBatch(A, X, subset_node_idx), data_subset))
    return batches


def _embed(model, batch):
    """The batch nodes' embeddings: `model(batch)` for an MRGCN (mrgcn.py:216-248), the R-GCN's mini-batch forward
    on the batch structure for a bare RGCN (featureless: no X)."""
    if hasattr(model, "rgcn"):
        return model(batch)
    return model(batch.X, batch.A)


def _relations(model):
    return model.rgcn.relations if hasattr(model, "rgcn") else model.relations


def _batch_state(batch, facts, device):
    """What a batch keeps on the device across epochs (built once, outside the steps): the facts, the negative
    sampler over the batch's nodes (the remapped facts' nodes are exactly 0 .. len(node_index) - 1)."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    st = getattr(batch, "_mrgcn_lp", None)
    if st is None or st["device"] != device:
        if not torch.is_tensor(batch.node_index):   # (train_model :207-214: as tensors, on the device)
            batch.as_tensors_()
            batch.to({"relational": device})
        f = torch.as_tensor(np.asarray(facts), dtype=torch.int64).to(device).contiguous()
        st = dict(device=device, facts=f, sampler=DeviceNegativeSampler(f), lists=None, eval_ws=None)
        batch._mrgcn_lp = st
    return st


def penalty_owners(model, optimizer, on_device=True):
    """The parameters whose L1 / L2 penalty (link_prediction.py:306-322) the optimizer's own step takes over
    (`ClipAdam.step(l1_lambda=, l2_lambda=, reg_params=, dense_penalty="kernel")`): those whose NAME contains `weight`
    (a bare RGCN's `layers.0.weight_I`, or the same under an `rgcn.` prefix), that the optimizer steps, that require a
    gradient and that are float32, contiguous and — `on_device` — on the GPU; none unless the optimizer is a `ClipAdam`
    that clips inside its own step (`max_norm` set) and is not distributed.  Everything else keeps its penalty in the
    loss."""
    from ..optim import ClipAdam
    if not (isinstance(optimizer, ClipAdam) and optimizer.max_norm is not None and optimizer._dist is None):
        return []
    stepped = {id(p) for g in optimizer.param_groups for p in g["params"]}
    return [p for name, p in model.named_parameters()
            if "weight" in name and id(p) in stepped and p.requires_grad and p.dtype == torch.float32
            and p.is_contiguous() and (p.is_cuda or not on_device)]


def _penalised_backward_and_step(model, optimizer, loss, clip, l1_lambda, l2_lambda):
    """backward, clip and step of a loss that carries the loop's weight penalty (:306-326) -> BCE + penalty as a device
    scalar, the penalty taken from the parameters before the step.  The optimizer owns the penalty of
    `penalty_owners`; the others' stays in the loss (`weight_regularisation`), so every route steps the same thing."""
    from ..optim import clip_grad_norm_
    from ..train import ClipAdam, weight_regularisation
    owned = penalty_owners(model, optimizer)
    term = weight_regularisation(model, l1_lambda, l2_lambda, skip=owned)
    if term is not None:
        loss = loss + term
    loss.backward()
    if not (isinstance(optimizer, ClipAdam) and optimizer.max_norm is not None):
        clip_grad_norm_(model.parameters(), clip)
    if not owned:
        optimizer.step()
        return loss.detach()
    optimizer.step(l1_lambda=l1_lambda, l2_lambda=l2_lambda, reg_params=owned, dense_penalty="kernel")
    return loss.detach() if optimizer.reg_loss is None else loss.detach() + optimizer.reg_loss


def _backward_and_step(model, optimizer, loss, clip, l1_lambda, l2_lambda):
    """The tail of every step: backward, the gradient clipped at `clip` (inside the step of a `ClipAdam` that has a
    `max_norm`, by `clip_grad_norm_` otherwise), the optimizer step -> the loss (with its penalty) as a device scalar."""
    from ..optim import clip_grad_norm_
    from ..train import ClipAdam
    if l1_lambda > 0 or l2_lambda > 0:
        return _penalised_backward_and_step(model, optimizer, loss, clip, l1_lambda, l2_lambda)
    loss.backward()
    if not (isinstance(optimizer, ClipAdam) and optimizer.max_norm is not None):
        clip_grad_norm_(model.parameters(), clip)
    optimizer.step()
    return loss.detach()


def train_batch_step(model, batch, facts, optimizer, negatives=None, clip=1.0, slot=None, sampler=None,
                     l1_lambda=0.0, l2_lambda=0.0, decoder="triples", loss="bce", pos_weight=None, scorer="distmult",
                     label_smoothing=0.0):
    """One batch of train_model (link_prediction.py:226-331): 20 % of the batch's facts corrupted inside the batch
    (half the heads, half the tails replaced by batch nodes, :239-263) — drawn on the device, or `negatives` (an
    [n // 5, 3] array of batch-local triples, e.g. the reference's draws) —, DistMult scores of facts + negatives, BCE,
    clip_grad_norm_(clip) and the optimizer step.  No host readback: returns the loss as a device scalar.  A
    `mrgcn_amd.train.ClipAdam` with a max_norm clips inside its own step; any other optimizer gets
    `mrgcn_amd.optim.clip_grad_norm_` first (torch's, unless a row-sparse weight_I gradient is among the parameters:
    `mrgcn_amd.optim.RowSparseAdam` then steps only the node blocks of the batch and the ones that ever had
    gradient).  `slot` (a float32 [1] piece of the epoch's loss table on the device): the loss also goes there.
    `sampler`: any callable with `train_step`'s sampler contract — `triples, labels = sampler()`, the batch's facts
    followed by their corrupted copies and the 1 / 0 labels on the device, without synchronising — in place of the
    batch's own `DeviceNegativeSampler`.  `l1_lambda` / `l2_lambda` (:306-322): l1 sum|p| + l2 sum p^2 over the
    parameters named `weight*` joins the loss, is clipped with it and is part of the returned loss; a `ClipAdam` with
    a max_norm takes the penalty of the weights it steps into its own step (`penalty_owners`), without an autograd
    graph over them.  `decoder="grouped"` (with a `NegativeSampler` as `sampler`): the grouped loss (`group_loss`) in
    place of the flat scores and BCE — `loss` "bce" (with `pos_weight`) or "softmax"; everything else unchanged.
    `scorer="complex"`: ComplEx scores (`score_complex_bc`) under the flat BCE; not with the grouped decoder.
    `decoder="all"` with `loss="softmax"`: the 1-vs-all softmax cross-entropy (`all_loss`) of the batch's facts —
    `sampler.facts` when there is a sampler, which is not called — against the batch's own nodes, on both sides.
    `decoder="kvsall"` (with `loss="bce"`, the default) and `label_smoothing`: the KvsAll loss (`kvsall_loss`) of the
    distinct queries of those same facts, in batch-local ids, against the batch's own nodes; the `KvsAllQueries` are
    built on the first step, outside a stream capture, and kept with the batch's device state."""
    dec = _decoder_args(decoder, loss, pos_weight, [sampler], "train_batch_step", scorer, label_smoothing)
    return _train_batch_step(model, batch, facts, optimizer, negatives, clip, slot, sampler, l1_lambda, l2_lambda, dec)


def _train_batch_step(model, batch, facts, optimizer, negatives, clip, slot, sampler, l1_lambda, l2_lambda, dec):
    """`train_batch_step` behind its keyword checks, on the resolved `_Decoder`."""
    who = "train_batch_step"
    E = _embed(model, batch)
    st = _batch_state(batch, facts, E.device)
    if slot is not None and not (torch.is_tensor(slot) and slot.is_cuda and slot.dtype == torch.float32
                                 and slot.numel() == 1):
        raise _lib.MrgcnError(f"{who}: slot is one float32 on the device")
    if negatives is not None and sampler is not None:
        raise _lib.MrgcnError(f"{who}: negatives or a sampler, not both")
    triples, labels = dec.scored(sampler, who, st, negatives)
    optimizer.zero_grad()
    loss = dec.loss_of(triples, labels, E, _relations(model), None, sampler, st)
    loss = _backward_and_step(model, optimizer, loss, clip, l1_lambda, l2_lambda)
    if slot is not None:
        slot.view(1).copy_(loss.view(1))
    return loss


def prepare_batches(batches, device):
    """Moves the batches of `mkbatches` to `device` once (train_model :207-228) and builds their device state."""
    for batch, facts in batches:
        _batch_state(batch, facts, device)
    return batches


def train_epoch(batches, model, optimizer, clip=1.0, l1_lambda=0.0, l2_lambda=0.0, samplers=None, decoder="triples",
                loss="bce", pos_weight=None, scorer="distmult", label_smoothing=0.0):
    """One epoch of train_model (:226-331): every batch once, in the fixed order of `mkbatches`; the mean of the batch
    losses (:326-331), read back once after the last step.  `l1_lambda` / `l2_lambda`: see `train_batch_step`.
    `samplers`: one sampler per batch (None: each batch's own `DeviceNegativeSampler`); `decoder` / `loss` /
    `pos_weight` / `scorer` / `label_smoothing`: see `train_batch_step` — the grouped decoder needs
    `NegativeSampler`s."""
    batches = list(batches)
    smps = list(samplers) if samplers is not None else [None] * len(batches)
    if len(smps) != len(batches):
        raise _lib.MrgcnError("train_epoch: one sampler per batch")
    dec = _decoder_args(decoder, loss, pos_weight, smps, "train_epoch", scorer, label_smoothing)
    model.train()
    losses = [_train_batch_step(model, batch, facts, optimizer, None, clip, None, smp, l1_lambda, l2_lambda, dec)
              for (batch, facts), smp in zip(batches, smps)]
    return float(np.mean([float(x) for x in torch.stack(losses).cpu().numpy()])) if losses else float("nan")


def evaluate_batches(batches, model, filtered=True, scorer="distmult"):
    """test_model (link_prediction.py:375-422): every batch's facts ranked against that batch's embeddings only
    (mrgcn_distmult_ranks), raw and — `filtered` — filtered by the true facts of that batch (truedicts(batch facts),
    computed once per batch and kept).  Returns (mrr, hits_at_k, rankings) as test_model does: {"raw", "flt"} means
    over the batches of the batches' MRR and hits@{1, 3, 10} (-1 for "flt" when not `filtered`), and the ranks of all
    batches flattened.  `scorer="complex"`: ComplEx scores (`rank_both` per batch)."""
    _scorer(scorer, "evaluate_batches")
    model.eval()
    K = [1, 3, 10]
    hits_at_k = {"flt": [[] for _ in K], "raw": [[] for _ in K]}
    mrr = {"flt": [], "raw": []}
    rankings = {"flt": [], "raw": []}
    with torch.no_grad():
        for batch, facts in batches:
            E, Rel, _, _, entries = _rank_inputs(scorer, "evaluate_batches", _embed(model, batch), _relations(model))
            st = _batch_state(batch, facts, E.device)
            tr = st["facts"]
            for flt in (False, True):
                rank_type = "flt" if flt else "raw"
                if flt and not filtered:
                    mrr[rank_type].append(-1)
                    for i, _ in enumerate(K):
                        hits_at_k[rank_type][i].append(-1)
                    rankings[rank_type].append(-1)
                    continue
                lists = _batch_lists(st, facts) if flt else None
                if entries.complex and tr.shape[0]:
                    ranks = rank_both(tr, E, Rel, lists=lists, scorer=scorer)[1 if flt else 0]
                else:
                    ranks = _rank_one_side(E, Rel, tr, lists)
                mrr[rank_type].append(torch.mean(1.0 / ranks.float()).item())
                for i, k in enumerate(K):
                    hits_at_k[rank_type][i].append(float(torch.mean((ranks <= k).float())))
                rankings[rank_type].append(ranks.tolist())
    for rank_type in ("flt", "raw"):
        mrr[rank_type] = np.mean(mrr[rank_type])
        hits_at_k[rank_type] = [np.mean(k) for k in hits_at_k[rank_type]]
        rankings[rank_type] = [r for r_list in rankings[rank_type]
                               for r in (r_list if isinstance(r_list, list) else [r_list])]
    return mrr, hits_at_k, rankings


# ---- top-k candidate completion (the question a trained model answers: which nodes complete (s, p, ?) / (?, p, o)) ---
TOPK_MAX = 256  # include/mrgcn_hip.h: mrgcn_distmult_topk takes 1 <= k <= 256
_SIDES = {"tail": 0, "head": 1}


def _side(side) -> int:
    if side not in _SIDES:
        raise ValueError(f"side must be 'tail' or 'head', not {side!r}")
    return _SIDES[side]


def known_lists(queries, known, side="tail"):
    """Per query (anchor, relation) the sorted, duplicate-free int32 nodes c for which the completed triple is a row of
    `known` ([m, 3] facts): (anchor, relation, c) for side="tail", (c, relation, anchor) for side="head".  Returns the
    CSR pair (ptr int64 [nq + 1], idx int32) `predict_topk` excludes.  Unlike `filter_lists` nothing is taken out as
    "the fact's own answer": a query has no answer, what is known is excluded."""
    head = _side(side)
    q = np.asarray(queries, dtype=np.int64).reshape(-1, 2)
    kn = np.asarray(known, dtype=np.int64).reshape(-1, 3)
    nq = len(q)
    ptr = np.zeros(nq + 1, np.int64)
    if nq == 0 or len(kn) == 0:
        return ptr, np.zeros(0, np.int32)
    ka, kr, kc = (kn[:, 2], kn[:, 1], kn[:, 0]) if head else (kn[:, 0], kn[:, 1], kn[:, 2])
    # the distinct (anchor, relation, completion) rows, sorted; groups of equal (anchor, relation)
    order = np.lexsort((kc, kr, ka))
    ka, kr, kc = ka[order], kr[order], kc[order]
    uniq = np.ones(len(ka), bool)
    uniq[1:] = (ka[1:] != ka[:-1]) | (kr[1:] != kr[:-1]) | (kc[1:] != kc[:-1])
    ka, kr, kc = ka[uniq], kr[uniq], kc[uniq]
    first = np.ones(len(ka), bool)
    first[1:] = (ka[1:] != ka[:-1]) | (kr[1:] != kr[:-1])
    gstart = np.flatnonzero(first)                       # group -> first member
    gend = np.append(gstart[1:], len(ka))
    # every query's group: the (anchor, relation) pairs of groups and queries ranked together
    ga, gr = ka[gstart], kr[gstart]
    both_a, both_r = np.concatenate([ga, q[:, 0]]), np.concatenate([gr, q[:, 1]])
    _, inv = np.unique(np.stack([both_a, both_r], 1), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    ng = len(ga)
    group_of_rank = np.full(int(inv.max()) + 1, -1, np.int64)
    group_of_rank[inv[:ng]] = np.arange(ng)
    gq = group_of_rank[inv[ng:]]                         # -1: nothing known for the query
    has = gq >= 0
    cnt = np.where(has, gend[np.maximum(gq, 0)] - gstart[np.maximum(gq, 0)], 0)
    np.cumsum(cnt, out=ptr[1:])
    off = np.arange(int(ptr[-1])) - np.repeat(ptr[:-1], cnt)
    idx = kc[np.repeat(gstart[np.maximum(gq, 0)], cnt) + off].astype(np.int32)
    return ptr, idx


def _check_ids(queries, num_nodes: int, num_relations: int):
    """Raises for a query whose node is outside [0, num_nodes) or whose relation is outside [0, num_relations)."""
    if len(queries) == 0:
        return
    if torch.is_tensor(queries):   # (on the device: one readback for the four bounds)
        lo_n, lo_r, hi_n, hi_r = torch.cat([queries.min(0).values, queries.max(0).values]).tolist()
    else:
        (lo_n, lo_r), (hi_n, hi_r) = (int(v) for v in queries.min(0)), (int(v) for v in queries.max(0))
    if lo_n < 0 or hi_n >= num_nodes:
        raise ValueError(f"predict_topk: query node ids must lie in [0, {num_nodes}): found {lo_n} .. {hi_n}")
    if lo_r < 0 or hi_r >= num_relations:
        raise ValueError(f"predict_topk: relation ids must lie in [0, {num_relations}) (the rows of edge_embeddings): "
                         f"found {lo_r} .. {hi_r}")


class TypedQueries:
    """The queries of a type-constrained `predict_topk`, grouped by relation on the host: `queries` [nq, 2] rows (anchor
    node, relation) — a device tensor is read back once, as `known_lists` needs them on the host anyway —, `types` a
    `TypedCandidates`, `side` "tail" / "head", `known` as `predict_topk`'s (None, an [m, 3] array of facts, or a ready
    (ptr, idx) pair of device tensors indexed by the caller's query order).  Holds the device tensors of the call:
    `q`, `order` / `tile_ptr` / `tile_rel` (tiles of at most 8 queries of ONE relation), `work` (one row {tile,
    candidate tile} per block), `q_tiles` (candidate tiles per query), the exclusion lists, and `max_slot`, the
    longest candidate list among the queries' — what the workspace is sized by.  Build it beforehand and pass it as
    `queries` to capture the call in a graph."""

    def __init__(self, queries, types: TypedCandidates, side="tail", known=None, device=None):
        if not isinstance(types, TypedCandidates):
            raise TypeError("TypedQueries: types must be a TypedCandidates")
        self.side, self.head = side, _side(side)
        if device is None:
            device = queries.device if torch.is_tensor(queries) and queries.is_cuda else types.ptr.device
        q_host = (queries.detach().cpu().numpy() if torch.is_tensor(queries) else np.asarray(queries)).astype(
            np.int64).reshape(-1, 2)
        _check_ids(q_host, types.num_nodes, types.num_relations)
        self.types = types.to(device)
        self.nq = nq = len(q_host)
        order, tile_ptr, tile_rel = _relation_tiles(q_host[:, 1], "TypedQueries")
        lens = types.lengths_host[2 * q_host[:, 1] + self.head] if nq else np.zeros(0, np.int64)
        self.max_slot = int(lens.max()) if nq else 0
        q_tiles = (lens + 255) // 256
        ctiles = q_tiles[order[tile_ptr[:-1]]] if len(tile_rel) else np.zeros(0, np.int64)
        work = np.stack([np.repeat(np.arange(len(tile_rel), dtype=np.int64), ctiles),
                         np.arange(int(ctiles.sum())) - np.repeat(np.cumsum(ctiles) - ctiles, ctiles)], 1)
        if len(work) >= 1 << 31:
            raise ValueError("TypedQueries: too many (query tile, candidate tile) pairs for one grid")
        self.ntiles, self.nwork = len(tile_rel), len(work)
        self.scores_computed = int(lens.sum())
        self.q_host = q_host
        self.q = torch.from_numpy(np.ascontiguousarray(q_host)).to(device)
        self.order = _dev_or_dummy(order, device)
        self.tile_ptr = torch.from_numpy(tile_ptr).to(device)
        self.tile_rel = _dev_or_dummy(tile_rel, device)
        self.work = _dev_or_dummy(work.astype(np.int32), device)
        self.q_tiles = _dev_or_dummy(q_tiles.astype(np.int32), device)
        self.excl = None
        if known is not None:
            if isinstance(known, (tuple, list)) and len(known) == 2 and all(torch.is_tensor(a) for a in known):
                ptr, idx = known
                if not (ptr.dtype == torch.int64 and idx.dtype == torch.int32 and ptr.numel() == nq + 1):
                    raise ValueError("predict_topk: known=(ptr, idx) must be tensors, int64 [nq + 1] and int32")
                ptr, idx = ptr.to(device).contiguous(), idx.to(device).contiguous()
            elif isinstance(known, (tuple, list)) and len(known) == 2 and any(
                    a is None or torch.is_tensor(a) for a in known):
                raise _lib.MrgcnError("predict_topk: exclusion lists need both tensors of the (ptr, idx) pair")
            else:
                kn = known.cpu().numpy() if torch.is_tensor(known) else np.asarray(known)
                ptr, idx = (torch.from_numpy(a).to(device) for a in known_lists(q_host, kn, side))
            self.excl = (ptr, _or_dummy(idx))


def _predict_topk_typed(tq: TypedQueries, E, Rel, k: int, entries: _Entries):
    dev, N, H = E.device, int(E.shape[0]), int(E.shape[1])
    types = tq.types
    if N != types.num_nodes or int(Rel.shape[0]) < types.num_relations or tq.q.device != dev:
        raise _lib.MrgcnError("predict_topk: the embeddings do not match the typed queries (nodes, relations or device)")
    nq = tq.nq
    out_idx = torch.empty((nq, k), dtype=torch.int64, device=dev)
    out_score = torch.empty((nq, k), dtype=torch.float32, device=dev)
    if nq == 0:
        return out_idx, out_score
    topk, workspace, what = entries("typed_topk")
    ws_bytes = int(workspace(N, H, nq, k, tq.max_slot))
    if ws_bytes < 0:
        raise _lib.MrgcnError("predict_topk: sizes outside mrgcn_distmult_typed_topk's limits")
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    ptr, idx = tq.excl if tq.excl is not None else (None, None)
    with torch.cuda.device(dev):
        _lib.check(topk(
            _ptr(E), E.stride(0), N, _ptr(Rel), Rel.stride(0), H, _ptr(tq.q), nq, tq.head, _ptr(tq.order),
            _ptr(tq.tile_ptr), _ptr(tq.tile_rel), tq.ntiles, _ptr(tq.work), tq.nwork, _ptr(tq.q_tiles),
            _ptr(types.ptr), _ptr(types.idx), tq.max_slot, _ptr(ptr), _ptr(idx), k, _ptr(ws), ws_bytes,
            _ptr(out_idx), _ptr(out_score), _stream()), what)
    bump("lp.topk.typed")
    return out_idx, out_score


def predict_topk(queries, node_embeddings, edge_embeddings, k, side="tail", known=None, scorer="distmult",
                 candidates=None):
    """The k best completions of every query: `queries` [nq, 2] rows (anchor node, relation) — numpy or a tensor —,
    side="tail" ranks the nodes c of (anchor, relation, c), side="head" those of (c, relation, anchor).  Returns
    (idx int64 [nq, k], scores float32 [nq, k]) on the embeddings' device: score descending, equal scores (-0 == +0) by
    ascending node id, rows with fewer than k candidates end in (-1, -inf).  The scores are those of
    `compute_ranks_fast`, bit for bit (sequential float32 sums), so a fact of rank r sits at position r of its row
    when no score ties; the [nq, nodes] score matrix is never stored (mrgcn_distmult_topk).  `known`: None, an [m, 3]
    array of facts whose completions are excluded (`known_lists` builds the lists), or a ready (ptr, idx) pair of
    device tensors (int64 [nq + 1], int32) — with it and `queries` as a device tensor a call builds nothing on the host
    and can be captured in a graph (ids are then checked outside captures only).  1 <= k <= 256.  Embeddings must be
    finite; results with NaN are undefined.  `scorer="complex"`: ComplEx scores — those of the ComplEx ranks, bit for
    bit, and of `mrgcn_amd.host.complex_candidate_scores` (mrgcn_complex_topk); an odd width raises `MrgcnError`.
    `candidates` (a `TypedCandidates`): the k best nodes OF THE QUERY RELATION'S LIST on the asked side (its tail
    candidates for side="tail", its head candidates for side="head") instead of all nodes — the same order, ties,
    exclusions and (-1, -inf) tails, scores bit-equal to the untyped call's for the same (query, node) pairs
    (mrgcn_distmult_typed_topk).  The queries are grouped by relation on the host at call time (a device tensor is read
    back once) and the rows come back in the caller's order; a `TypedQueries` built beforehand and passed as `queries`
    makes the call host-free and capturable.  It carries its own side, lists and exclusions: `side` must then name the
    side it was built for, `known` must be left out and `candidates`, when given, must hold the lists it was built
    with — anything else raises ValueError instead of answering another question than the one asked."""
    if isinstance(queries, TypedQueries):
        if side != queries.side:
            raise ValueError(f"predict_topk: the TypedQueries were built for side={queries.side!r}, not {side!r}; "
                             f"pass side={queries.side!r}")
        if known is not None:
            raise ValueError("predict_topk: a TypedQueries carries its own exclusions (TypedQueries(known=...)); "
                             "leave `known` out")
        if candidates is not None and not (
                isinstance(candidates, TypedCandidates) and candidates.num_nodes == queries.types.num_nodes
                and np.array_equal(candidates.ptr_host, queries.types.ptr_host)
                and np.array_equal(candidates.idx_host, queries.types.idx_host)):
            raise ValueError("predict_topk: the TypedQueries were built with other candidate lists")
    head = _side(side)
    _scorer(scorer, "predict_topk")   # (the keywords before `k`, `k` before the embeddings are looked at)
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= TOPK_MAX:
        raise ValueError(f"predict_topk: k must be an integer in [1, {TOPK_MAX}], not {k!r}")
    k = int(k)
    E, Rel, N, H, entries = _rank_inputs(scorer, "predict_topk", node_embeddings, edge_embeddings)
    dev = E.device
    if N == 0:
        raise ValueError("predict_topk: no nodes")
    if candidates is not None or isinstance(queries, TypedQueries):
        if not isinstance(queries, TypedQueries):
            if not isinstance(candidates, TypedCandidates):
                raise TypeError("predict_topk: candidates must be a TypedCandidates")
            queries = TypedQueries(queries, candidates, side=side, known=known, device=dev)
        return _predict_topk_typed(queries, E, Rel, k, entries)
    on_device = torch.is_tensor(queries) and queries.is_cuda
    q_host = None
    if on_device:
        q = queries.to(dev, torch.int64).reshape(-1, 2).contiguous()
        if not torch.cuda.is_current_stream_capturing():
            _check_ids(q, N, int(Rel.shape[0]))
    else:
        q_host = (queries.numpy() if torch.is_tensor(queries) else np.asarray(queries)).astype(np.int64).reshape(-1, 2)
        _check_ids(q_host, N, int(Rel.shape[0]))
        q = torch.from_numpy(np.ascontiguousarray(q_host)).to(dev)
    nq = int(q.shape[0])
    ptr = idx = None
    if known is not None:
        if isinstance(known, (tuple, list)) and len(known) == 2 and all(torch.is_tensor(a) for a in known):
            ptr, idx = known
            if not (ptr.is_cuda and idx.is_cuda and ptr.dtype == torch.int64 and idx.dtype == torch.int32
                    and ptr.numel() == nq + 1):
                raise ValueError("predict_topk: known=(ptr, idx) must be device tensors, int64 [nq + 1] and int32")
            ptr, idx = ptr.contiguous(), idx.contiguous()
        elif isinstance(known, (tuple, list)) and len(known) == 2 and any(a is None or torch.is_tensor(a) for a in known):
            raise _lib.MrgcnError("predict_topk: exclusion lists need both tensors of the (ptr, idx) pair")
        else:
            if q_host is None:
                q_host = q.cpu().numpy()
            kn = known.cpu().numpy() if torch.is_tensor(known) else np.asarray(known)
            ptr, idx = (torch.from_numpy(a).to(dev) for a in known_lists(q_host, kn, side))
        idx = _or_dummy(idx)
    out_idx = torch.empty((nq, k), dtype=torch.int64, device=dev)
    out_score = torch.empty((nq, k), dtype=torch.float32, device=dev)
    if nq == 0:
        return out_idx, out_score
    topk, workspace, what = entries("topk")
    ws_bytes = int(workspace(N, H, nq, k))
    if ws_bytes < 0:
        raise _lib.MrgcnError("predict_topk: sizes outside mrgcn_distmult_topk's limits")
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(topk(_ptr(E), E.stride(0), N, _ptr(Rel), Rel.stride(0), H, _ptr(q), nq, head, _ptr(ptr), _ptr(idx),
                        k, _ptr(ws), ws_bytes, _ptr(out_idx), _ptr(out_score), _stream()), what)
    return out_idx, out_score


def predict_links(model, batch, queries, k, side="tail", known=None, scorer="distmult", candidates=None):
    """`predict_topk` on a model's own embeddings: `model.eval()`, then — without gradients — the batch's node
    embeddings (`_embed`: an MRGCN's forward, or a bare RGCN on the batch structure) against the model's relation
    embeddings.  `batch`: a FullBatch or a masked / sliced MiniBatch.  With a mini-batch the node ids of `queries`,
    `known` and the result are the BATCH-LOCAL ones (positions in `batch.node_index`, as in the facts `mkbatches`
    returns); map results back with `batch.node_index[idx]`.  The model is left in eval mode.  `scorer`: see
    `predict_topk`.  `candidates` (a `TypedCandidates` over the ids of the embeddings, so full-batch): see
    `predict_topk`."""
    _side(side)
    _scorer(scorer, "predict_links")
    model.eval()
    with torch.no_grad():
        E = _embed(model, batch)
        return predict_topk(queries, E, _relations(model), k, side=side, known=known, scorer=scorer,
                            candidates=candidates)


# ---- the reference's full-batch run loop on the device (link_prediction.py:191-422; csrc/lp_eval.hip) ---------------
EVAL_ROW = 17   # loss | train raw mrr, h@1, h@3, h@10, flt mrr, h@1, h@3, h@10 | the same eight of the validation facts


class FactParts:
    """The facts of an evaluation cut as `mkbatches` cuts them in full-batch mode (:536-545:
    `np.array_split(arange(n), max(n // mrr_batchsize, 1))`), with the filter lists of EACH PART'S OWN facts
    (test_model filters a part by `truedicts(batch_data)`, :568-591) concatenated into one CSR set with running
    offsets, and `part_ptr` [nparts + 1] over the facts.  Built once on the host; `facts` (int64 [n, 3]), `part_ptr`
    (int64) and `lists` (tail_ptr int64 [n + 1], tail_idx int32, head_ptr, head_idx; None when not `filtered`) are
    tensors on `device` — default: the device of `facts` when it is a tensor, else the current GPU, else the host."""

    def __init__(self, facts, mrr_batchsize, filtered=True, device=None):
        if device is None:
            device = facts.device if torch.is_tensor(facts) else ("cuda" if torch.cuda.is_available() else "cpu")
        data = (facts.detach().cpu().numpy() if torch.is_tensor(facts) else np.asarray(facts)).astype(np.int64)
        if data.ndim != 2 or data.shape[1] != 3 or len(data) == 0:
            raise ValueError("FactParts: facts must be a non-empty [n, 3] array")
        n = len(data)
        if mrr_batchsize <= 0:
            mrr_batchsize = n
        subsets = np.array_split(np.arange(n), max(n // int(mrr_batchsize), 1))
        self.sizes = [len(s) for s in subsets]
        ptr = np.zeros(len(subsets) + 1, np.int64)
        np.cumsum(self.sizes, out=ptr[1:])
        self.n, self.nparts, self.filtered = n, len(subsets), bool(filtered)
        self.part_ptr_host = ptr
        self.facts = torch.from_numpy(np.ascontiguousarray(data)).to(device)
        self.part_ptr = torch.from_numpy(ptr).to(device)
        self.lists = None
        if filtered:
            tps, tis, hps, his = [np.zeros(1, np.int64)], [], [np.zeros(1, np.int64)], []
            toff = hoff = 0
            for p in range(self.nparts):
                tp, ti, hp, hi = filter_lists(data[ptr[p]:ptr[p + 1]])
                tps.append(tp[1:] + toff)
                hps.append(hp[1:] + hoff)
                tis.append(ti)
                his.append(hi)
                toff += len(ti)
                hoff += len(hi)
            cat = [np.concatenate(tps), np.concatenate(tis).astype(np.int32), np.concatenate(hps),
                   np.concatenate(his).astype(np.int32)]
            self.lists = tuple(torch.from_numpy(a).to(device) for a in cat)


def rank_both_slice() -> int:
    """How many facts one launch of `rank_both`'s scoring grid takes by default (any number of facts is cut into such
    slices inside the call)."""
    return int(_lib.load().mrgcn_distmult_ranks_both_slice())


def rank_both(facts, node_embeddings, edge_embeddings, lists=None, part_ptr=None, slice_facts=0, scorer="distmult"):
    """Raw and filtered ranks of `facts` from ONE pass over the candidate scores (mrgcn_distmult_ranks_both): `(raw,
    flt)`, each what `compute_ranks_fast` returns without / with the filter, bit for bit; `flt` is None without lists.
    `facts`: an [n, 3] array, or a `FactParts` (its lists and parts are then taken).  `lists`: the four device tensors
    of `filter_lists` (concatenated per part for several parts).  `part_ptr` (device int64 [nparts + 1]): the call
    stands for one `compute_ranks_fast` per part — the reference leaves facts at positions >= the number of nodes of a
    call unscored, and the position is then the one inside the part.  `slice_facts`: facts per launch of the scoring
    grid (0: `rank_both_slice()`).  With device tensors nothing is copied from or to the host, nothing synchronises and
    a graph captures the call.  `scorer="complex"`: ComplEx scores (mrgcn_complex_ranks_both: the same contract, the
    fact's own score kept per side, because the two sides round differently); an odd width raises `MrgcnError`."""
    E, Rel, N, H, entries = _rank_inputs(scorer, "rank_both", node_embeddings, edge_embeddings)
    if isinstance(facts, FactParts):
        lists = facts.lists if lists is None else lists
        part_ptr = facts.part_ptr if part_ptr is None else part_ptr
        facts = facts.facts
    dev = E.device
    if torch.is_tensor(facts) and facts.is_cuda and facts.dtype == torch.int64 and facts.is_contiguous():
        tr = facts
        if tr.dim() != 2 or tr.shape[1] != 3:
            raise ValueError("facts must be [n, 3]")
    else:
        tr = _triples(facts, dev)
    nf = int(tr.shape[0])
    raw = torch.empty(2 * nf, dtype=torch.int64, device=dev)
    flt = torch.empty(2 * nf, dtype=torch.int64, device=dev) if lists is not None else None
    if nf == 0:
        return raw, flt
    ls = _check_lists(lists, nf, "rank_both") if lists is not None else [None] * 4
    nparts = 0
    if part_ptr is not None:
        if not (part_ptr.is_cuda and part_ptr.dtype == torch.int64 and part_ptr.dim() == 1 and part_ptr.numel() >= 2):
            raise _lib.MrgcnError("rank_both: part_ptr is a device int64 [nparts + 1] tensor")
        part_ptr, nparts = part_ptr.contiguous(), int(part_ptr.numel()) - 1
    ranks_both, workspace, what = entries("ranks_both")
    ws_bytes = int(workspace(N, H, nf))
    ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(ranks_both(_ptr(E), E.stride(0), N, _ptr(Rel), Rel.stride(0), H, _ptr(tr), nf, _ptr(ls[0]),
                              _ptr(ls[1]), _ptr(ls[2]), _ptr(ls[3]), _ptr(part_ptr), nparts, int(slice_facts),
                              _ptr(ws), ws_bytes, _ptr(raw), _ptr(flt), _stream()), what)
    return raw, flt


def rank_metrics(ranks, part_ptr=None, out=None, score=None):
    """test_model's metrics (:403-419) of an int64 `[2 * nf]` rank vector (tail ranks, then head ranks) on the device:
    float32 `[mrr, hits@1, hits@3, hits@10]`, the mean over the parts of `part_ptr` (device int64 [nparts + 1]; None:
    one part) of each part's means — part p owns ranks [p0, p1) and nf + [p0, p1) —, added in float64 in a fixed order
    and rounded once (mrgcn_rank_metrics): equal ranks give equal bits.  `out`: a contiguous float32 [4] device tensor
    to write; `score`: a float32 device scalar that receives `1 - mrr`, the score train_model records (:363).  No
    synchronisation; capturable — so `part_ptr` is not read here: the caller guarantees `0 = part_ptr[0] < ... <
    part_ptr[-1] = nf` (a `FactParts` does by construction, and `evaluate_facts` compares its host copy with the
    ranks); the kernel clamps bounds outside `[0, nf]`, so a wrong one gives wrong means, never a stray read."""
    if not (ranks.is_cuda and ranks.dtype == torch.int64 and ranks.dim() == 1 and ranks.numel() >= 2
            and ranks.numel() % 2 == 0 and ranks.is_contiguous()):
        raise _lib.MrgcnError("rank_metrics: a contiguous, non-empty int64 [2 * nf] rank vector on the device")
    dev, nf = ranks.device, int(ranks.numel()) // 2
    nparts = 1
    if part_ptr is not None:
        if not (part_ptr.is_cuda and part_ptr.dtype == torch.int64 and part_ptr.dim() == 1 and part_ptr.numel() >= 2
                and part_ptr.is_contiguous()):
            raise _lib.MrgcnError("rank_metrics: part_ptr is a contiguous device int64 [nparts + 1] tensor")
        nparts = int(part_ptr.numel()) - 1
    if out is None:
        out = torch.empty(4, dtype=torch.float32, device=dev)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.numel() == 4 and out.is_contiguous()):
        raise _lib.MrgcnError("rank_metrics: out is a contiguous float32 [4] tensor on the device")
    if score is not None and not (score.is_cuda and score.dtype == torch.float32 and score.numel() == 1):
        raise _lib.MrgcnError("rank_metrics: score is one float32 on the device")
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mrgcn_rank_metrics(_ptr(ranks), nf, _ptr(part_ptr), nparts, _ptr(out), _ptr(score),
                                                  _stream()), "rank_metrics")
    return out


def evaluate_facts(node_embeddings, edge_embeddings, parts: FactParts, want_ranks=False, out=None, score=None,
                   slice_facts=0, scorer="distmult"):
    """test_model (:375-422) of the parts of a `FactParts` against ONE set of embeddings (full-batch mode: every part
    sees the whole graph's), without the host: `rank_both` and one `rank_metrics` per rank type.  Returns the float32
    `[8]` device vector raw mrr, hits@1, hits@3, hits@10, then the same filtered (-1 each when the parts carry no
    lists, as test_model reports them) — `out`, when given — and with `want_ranks` also `(raw, flt)`, the ranks of all
    parts as `rank_both` lays them out.  `score` (a float32 device scalar) receives `1 - raw mrr`.  No
    synchronisation; capturable.  `scorer`: see `rank_both`."""
    _scorer(scorer, "evaluate_facts")
    ptr = parts.part_ptr_host
    if not (ptr[0] == 0 and ptr[-1] == parts.n == parts.facts.shape[0] and bool(np.all(np.diff(ptr) > 0))
            and parts.part_ptr.numel() == len(ptr)):
        raise _lib.MrgcnError("evaluate_facts: part_ptr must rise from 0 to the number of facts, no part empty")
    raw, flt = rank_both(parts, node_embeddings, edge_embeddings, slice_facts=slice_facts, scorer=scorer)
    return _metrics_of_ranks(raw, flt, parts.part_ptr, out, score, want_ranks)


def _metrics_of_ranks(raw, flt, part_ptr, out, score, want_ranks):
    """The end of `evaluate_facts` and `evaluate_typed`: one `rank_metrics` per rank type into the float32 [8] `out`
    (None: a new one; -1 in the filtered four without `flt`), `1 - raw mrr` into `score`."""
    if out is None:
        out = torch.empty(8, dtype=torch.float32, device=raw.device)
    rank_metrics(raw, part_ptr, out[:4], score)
    if flt is not None:
        rank_metrics(flt, part_ptr, out[4:])
    else:
        out[4:].fill_(-1.0)
    return (out, raw, flt) if want_ranks else out


# ---- type-constrained ranks (csrc/lp_typed.hip) -----------------------------------------------------------------------
class TypedFacts:
    """The facts of a type-constrained evaluation, grouped for `rank_typed` — built once on the host, like `FactParts`.
    `types`: a `TypedCandidates`.  Every fact's tail must be among its relation's tail candidates and its head among
    the head candidates (ValueError otherwise: the rank rule counts the fact's own answer among the candidates).  The
    facts are ordered by relation and cut into tiles of at most 8 facts of ONE relation (`order`, `tile_ptr`,
    `tile_rel`; `work`: one row {2 tile + side, candidate tile} per block of the scoring grid).  `lists`: the filter
    lists in `filter_lists`' CSR form, indexed by the fact's ORIGINAL position — with `known=None` from the facts
    themselves (truedicts' semantics over the whole fact set), with `known` ([m, 3]) from those triples; None when not
    `filtered`.  `part_ptr` (with `mrr_batchsize`: the parts of `FactParts`, else one part) serves `rank_metrics` only:
    the ranks do not depend on it.  `scores_computed`: candidate scores one `rank_typed` call forms."""

    def __init__(self, facts, types: TypedCandidates, known=None, filtered=True, mrr_batchsize=None, device=None):
        if not isinstance(types, TypedCandidates):
            raise TypeError("TypedFacts: types must be a TypedCandidates")
        if device is None:
            device = facts.device if torch.is_tensor(facts) and facts.is_cuda else types.ptr.device
        data = (facts.detach().cpu().numpy() if torch.is_tensor(facts) else np.asarray(facts)).astype(np.int64)
        if data.ndim != 2 or data.shape[1] != 3 or len(data) == 0:
            raise ValueError("TypedFacts: facts must be a non-empty [n, 3] array")
        n, N, R = len(data), types.num_nodes, types.num_relations
        if data.min() < 0 or data[:, [0, 2]].max() >= N or data[:, 1].max() >= R:
            raise ValueError(f"TypedFacts: node ids must lie in [0, {N}), relation ids in [0, {R})")
        ok_t = types.contains(2 * data[:, 1], data[:, 2])
        ok_h = types.contains(2 * data[:, 1] + 1, data[:, 0])
        if not (ok_t.all() and ok_h.all()):
            f = int(np.flatnonzero(~(ok_t & ok_h))[0])
            raise ValueError(f"TypedFacts: fact {f} {tuple(int(v) for v in data[f])} has its "
                             f"{'tail' if not ok_t[f] else 'head'} outside its relation's candidates")
        self.n, self.filtered, self.types = n, bool(filtered), types.to(device)
        order, tile_ptr, tile_rel = _relation_tiles(data[:, 1], "TypedFacts")
        lens = types.lengths_host
        both = np.repeat(2 * np.arange(len(tile_rel), dtype=np.int64), 2) + np.tile([0, 1], len(tile_rel))
        ctiles = (lens[2 * tile_rel[both >> 1].astype(np.int64) + (both & 1)] + 255) // 256
        work = np.stack([np.repeat(both, ctiles),
                         np.arange(int(ctiles.sum())) - np.repeat(np.cumsum(ctiles) - ctiles, ctiles)], 1)
        if len(work) >= 1 << 31 or len(tile_rel) >= 1 << 30:
            raise ValueError("TypedFacts: too many (fact tile, candidate tile) pairs for one grid")
        self.ntiles, self.nwork = len(tile_rel), len(work)
        self.tile_fill = n / (8.0 * max(len(tile_rel), 1))
        self.scores_computed = int((lens[2 * data[:, 1]] + lens[2 * data[:, 1] + 1]).sum())
        self.order_host, self.tile_ptr_host, self.tile_rel_host = order, tile_ptr, tile_rel
        self.facts = torch.from_numpy(np.ascontiguousarray(data)).to(device)
        self.order = torch.from_numpy(order).to(device)
        self.tile_ptr = torch.from_numpy(tile_ptr).to(device)
        self.tile_rel = _dev_or_dummy(tile_rel, device)
        self.work = _dev_or_dummy(work.astype(np.int32), device)
        if mrr_batchsize is None or mrr_batchsize <= 0:
            mrr_batchsize = n
        sizes = [len(s) for s in np.array_split(np.arange(n), max(n // int(mrr_batchsize), 1))]
        self.part_ptr_host = np.zeros(len(sizes) + 1, np.int64)
        np.cumsum(sizes, out=self.part_ptr_host[1:])
        self.nparts = len(sizes)
        self.part_ptr = torch.from_numpy(self.part_ptr_host).to(device)
        self.lists = None
        if filtered:
            kn = data if known is None else (known.detach().cpu().numpy() if torch.is_tensor(known)
                                             else np.asarray(known)).astype(np.int64).reshape(-1, 3)
            cat = []
            for side, a, ans in (("tail", 0, 2), ("head", 2, 0)):
                ptr, idx = known_lists(data[:, [a, 1]], kn, side)     # what is known per (anchor, relation) ...
                owner = np.repeat(np.arange(n), np.diff(ptr))
                keep = idx != data[owner, ans]                        # ... but the fact's own answer
                kept = np.zeros(n + 1, np.int64)
                np.cumsum(np.bincount(owner[keep], minlength=n), out=kept[1:])
                cat += [kept, idx[keep].astype(np.int32)]
            self.lists = tuple(_dev_or_dummy(a, device) for a in cat)
        self._bufs: dict = {}


def rank_typed(tfacts: TypedFacts, node_embeddings, edge_embeddings, scorer="distmult"):
    """Type-constrained raw and filtered ranks (mrgcn_distmult_typed_ranks / mrgcn_complex_typed_ranks): `(raw, flt)`,
    int64 [2 * nf] device tensors — tail ranks, then head ranks, in the ORIGINAL fact order, so `rank_metrics` applies
    unchanged; `flt` is None when `tfacts` carries no lists.  A fact's tail is ranked among its relation's tail
    candidates and its head among the head candidates: rank = #greater + round_half_even((#ties - 1) / 2) + 1 over
    those candidates, for `flt` without the fact's filter list.  A candidate's score is `compute_ranks_fast`'s, bit for
    bit (the same float32 operations in the same order), so with `TypedCandidates.full` the ranks equal `rank_both`'s.
    EVERY fact is scored: the reference's rule that facts at positions >= num_nodes of a call stay unscored is
    `compute_ranks_fast`'s contract and is NOT carried over.  The workspace and both results are allocated at the first
    call for a shape and kept on `tfacts`: later calls return the same tensors, allocate nothing and do not
    synchronise — capturable.  `scorer="complex"`: ComplEx scores; an odd width raises `MrgcnError`."""
    _scorer(scorer, "rank_typed", node_embeddings.shape[-1])
    if not isinstance(tfacts, TypedFacts):
        raise TypeError("rank_typed: facts must be a TypedFacts (it holds the grouping by relation)")
    E, Rel, N, H, entries = _rank_inputs(scorer, "rank_typed", node_embeddings, edge_embeddings)
    dev, nf, types = E.device, tfacts.n, tfacts.types
    if N != types.num_nodes or int(Rel.shape[0]) < types.num_relations or tfacts.facts.device != dev:
        raise _lib.MrgcnError("rank_typed: the embeddings do not match the typed facts (nodes, relations or device)")
    typed_ranks, workspace, what = entries("typed_ranks")
    key = (N, H, entries.complex)
    if key not in tfacts._bufs:
        ws_bytes = int(workspace(N, H, nf))
        if ws_bytes < 0:
            raise _lib.MrgcnError("rank_typed: sizes outside the typed rank kernels' limits")
        tfacts._bufs[key] = (torch.empty((ws_bytes + 3) // 4, dtype=torch.int32, device=dev), ws_bytes,
                             torch.empty(2 * nf, dtype=torch.int64, device=dev),
                             torch.empty(2 * nf, dtype=torch.int64, device=dev) if tfacts.lists is not None else None)
    ws, ws_bytes, raw, flt = tfacts._bufs[key]
    ls = tfacts.lists if tfacts.lists is not None else [None] * 4
    with torch.cuda.device(dev):
        _lib.check(typed_ranks(
            _ptr(E), E.stride(0), N, _ptr(Rel), Rel.stride(0), H, _ptr(tfacts.facts), nf, _ptr(tfacts.order),
            _ptr(tfacts.tile_ptr), _ptr(tfacts.tile_rel), tfacts.ntiles, _ptr(tfacts.work), tfacts.nwork,
            _ptr(types.ptr), _ptr(types.idx), _ptr(ls[0]), _ptr(ls[1]), _ptr(ls[2]), _ptr(ls[3]), _ptr(ws), ws_bytes,
            _ptr(raw), _ptr(flt), _stream()), what)
    bump("lp.rank.typed")
    return raw, flt


def evaluate_typed(node_embeddings, edge_embeddings, tfacts: TypedFacts, out=None, score=None, want_ranks=False,
                   scorer="distmult"):
    """`evaluate_facts` over type-constrained ranks: `rank_typed` and one `rank_metrics` per rank type over the parts of
    `tfacts`.  Returns the float32 `[8]` device vector raw mrr, hits@1, hits@3, hits@10, then the same filtered (-1
    each without lists) — `out`, when given — and with `want_ranks` also `(raw, flt)`.  `score` (a float32 device
    scalar) receives `1 - raw mrr`.  No synchronisation; capturable (with `out` given, nothing is allocated after the
    first call).  The tuples `fit` yields keep the reference's shape: call this beside it."""
    _scorer(scorer, "evaluate_typed")
    raw, flt = rank_typed(tfacts, node_embeddings, edge_embeddings, scorer=scorer)
    return _metrics_of_ranks(raw, flt, tfacts.part_ptr, out, score, want_ranks)


def eval_schedule(nepoch, eval_interval, has_valid):
    """Which epochs of train_model evaluate what: `[(epoch, eval_train, eval_valid, records)]` for epochs 1 .. nepoch.
    The training facts are evaluated when `epoch % eval_interval == 0 or epoch == nepoch` (:336); the validation
    facts, and the early-stop record with them, only then and only with a validation set and `epoch < nepoch`
    (:350, :362)."""
    out = []
    for epoch in range(1, int(nepoch) + 1):
        eval_train = epoch % eval_interval == 0 or epoch == nepoch
        eval_valid = bool(eval_train and has_valid and epoch < nepoch)
        out.append((epoch, eval_train, eval_valid, eval_valid))
    return out


def train_step(model, forward_fn, sampler, optimizer, static=None, clip=1.0, l1_lambda=0.0, l2_lambda=0.0,
               decoder="triples", loss="bce", pos_weight=None, scorer="distmult", label_smoothing=0.0):
    """One full-batch epoch of train_model (:231-326): `triples, labels = sampler()` (a `DeviceNegativeSampler`, or any
    callable that returns the facts followed by their corrupted copies and the 1 / 0 labels on the device without
    synchronising), `forward_fn()` for the node embeddings (e.g. `lambda: model(None, A)`), DistMult scores, BCE,
    backward, the gradient clipped at `clip` — inside the step of a `ClipAdam` that has a `max_norm`, by
    `clip_grad_norm_` otherwise — and the optimizer step.  `static`: the `SortedTriples` of the facts the triples start
    with.  `l1_lambda` / `l2_lambda`: the loop's weight penalty, as in `train_batch_step`.  Returns the loss (BCE +
    penalty) as a device scalar; no host read, so a graph captures it.  `decoder="grouped"` (`sampler` a
    `NegativeSampler`): `group_loss` over the sampler's groups — `loss` "bce" (with `pos_weight`, a host float) or
    "softmax" — in place of the flat scores and BCE; `static` None then means the sampler's own stored orders, built
    on first use outside a capture.  `scorer="complex"`: ComplEx scores (`score_complex_bc`) under the flat BCE; not
    with the grouped decoder.  `decoder="all"` with `loss="softmax"`: the 1-vs-all softmax cross-entropy (`all_loss`)
    of `sampler.facts` against every row of the embeddings, on both sides, with either scorer; the sampler is not
    called and no negatives are drawn.  `decoder="kvsall"` (with `loss="bce"`, the default) and `label_smoothing`: the
    KvsAll loss (`kvsall_loss`) of the distinct (s, p, ?) and (?, p, o) queries of `sampler.facts`, all known answers
    of a query positives, with either scorer; the sampler is not called, and the `KvsAllQueries` are built on the
    first step, outside a stream capture, and kept on the sampler."""
    dec = _decoder_args(decoder, loss, pos_weight, [sampler], "train_step", scorer, label_smoothing)
    return _train_step(model, forward_fn, sampler, optimizer, static, clip, l1_lambda, l2_lambda, dec)


def _train_step(model, forward_fn, sampler, optimizer, static, clip, l1_lambda, l2_lambda, dec):
    """`train_step` behind its keyword checks, on the resolved `_Decoder`."""
    triples, labels = dec.scored(sampler, "train_step")
    emb = forward_fn()
    loss = dec.loss_of(triples, labels, emb, _relations(model), static, sampler)
    optimizer.zero_grad(set_to_none=True)
    return _backward_and_step(model, optimizer, loss, clip, l1_lambda, l2_lambda)


def _unpack(vec):
    """A metrics vector of evaluate_facts as the reference's pair ({"raw", "flt"} mrr, {"raw", "flt"} hits lists)."""
    v = [float(x) for x in vec]
    return {"raw": v[0], "flt": v[4]}, {"raw": v[1:4], "flt": v[5:8]}


class _Epochs:
    """What `FitEpochs` and `BatchFitEpochs` share: the counters (`loss_ctr` counts every epoch, `eval_ctr` the
    records), the rings of `poll` rows, `row` and `score`, `reset()`, and `train_epoch()` / `eval_epoch()`, which run
    the subclass's `_train_epoch` / `_eval_epoch` — eagerly, or as a replay of the one captured hipGraph each is
    (`train.Captured`, the discipline of DESIGN §13: the `warmup` epochs of the capture are real optimizer steps, the
    last of them an evaluating epoch, after which the counters and rings are reset).  Subclasses also supply
    `last_epoch`."""
    _stats = None   # the stats() keys of a training and an evaluating epoch, counted as `.graphed` or `.eager`

    def _tables(self, dev, stopper, poll):
        from ..train import _COUNT_ONLY, _StopState
        self.loss_ctr = _StopState(dev, 1, 0.0, _COUNT_ONLY)   # counts every epoch
        self.eval_ctr = stopper.state if stopper is not None else _StopState(dev, 1, 0.0, _COUNT_ONLY)
        self.loss_ring = torch.zeros((poll, 4), dtype=torch.float32, device=dev)
        self.eval_ring = torch.zeros((poll, EVAL_ROW), dtype=torch.float32, device=dev)
        self.row = torch.zeros(EVAL_ROW, dtype=torch.float32, device=dev)
        self.score = torch.zeros((), dtype=torch.float32, device=dev)

    def _start(self, graphed, warmup, optimizer, who):
        from ..train import Captured
        self.graphed = bool(graphed)
        if not graphed:
            self.reset()
            return
        nw = self.warmup_steps = max(int(warmup), 1)

        def warm():
            for _ in range(nw - 1):
                self._train_epoch()
            self._eval_epoch()
            self.reset()
        self._captured = Captured((self._train_epoch, self._eval_epoch), warm, optimizer, who)

    def reset(self):
        self.loss_ctr.reset()
        self.eval_ctr.reset()
        self.loss_ring.zero_()
        self.eval_ring.zero_()

    def _epoch(self, i):
        out = self._captured.replay(i) if self.graphed else (self._train_epoch, self._eval_epoch)[i]()
        if self._stats is not None:
            bump(f"{self._stats[i]}.{'graphed' if self.graphed else 'eager'}")
        return out

    def train_epoch(self):
        return self._epoch(0)

    def eval_epoch(self):
        return self._epoch(1)


class FitEpochs(_Epochs):
    """The two epochs `fit` is made of, as callables on one set of device rings (see `fit` for what they do):
    `train_epoch()` — `train_step`, its loss into row `epochs % poll` of `loss_ring` — and `eval_epoch()` — the same,
    then one `eval()` forward, `evaluate_facts` of the training and the validation parts, the `EVAL_ROW` values into row
    `records % poll` of `eval_ring` by the early-stop record, the snapshot behind its flag — and `last_epoch()`:
    a training epoch, then the training metrics into `last`, eagerly.  `graphed=True`: the first two are one captured
    hipGraph each (`_Epochs`)."""

    def __init__(self, model, forward_fn, tparts, vparts, optimizer, stopper=None, poll=8, graphed=True, sampler=None,
                 static=None, warmup=3, l1_lambda=0.0, l2_lambda=0.0, decoder="triples", loss="bce", pos_weight=None,
                 scorer="distmult", label_smoothing=0.0):
        self.dec = dec = _decoder_args(decoder, loss, pos_weight, [sampler], "fit", scorer, label_smoothing)
        if stopper is not None and vparts is None:
            raise _lib.MrgcnError("fit: early stopping scores the validation MRR: pass valid_facts")
        if graphed and not getattr(optimizer, "capturable", False):
            raise _lib.MrgcnError("fit(graphed=True) needs ClipAdam(..., capturable=True)")
        dev = tparts.facts.device
        if sampler is None:
            sampler = DeviceNegativeSampler(tparts.facts)
            if static is None and dec.kind not in ("all", "kvsall"):   # (those have no stored orders to walk)
                was = model.training
                model.eval()
                with torch.no_grad():
                    num_nodes = int(forward_fn().shape[0])
                model.train(was)
                static = SortedTriples(sampler.facts, num_nodes, int(_relations(model).shape[0]))
        self.model, self.forward_fn, self.tparts, self.vparts = model, forward_fn, tparts, vparts
        self.optimizer, self.stopper, self.sampler, self.static, self.poll = optimizer, stopper, sampler, static, poll
        self.l1_lambda, self.l2_lambda = float(l1_lambda), float(l2_lambda)
        self._tables(dev, stopper, poll)
        self.last = torch.zeros(8, dtype=torch.float32, device=dev)
        self._start(graphed, warmup, optimizer, "fit")

    def _train_epoch(self):
        self.model.train()
        loss = _train_step(self.model, self.forward_fn, self.sampler, self.optimizer, self.static, 1.0,
                           self.l1_lambda, self.l2_lambda, self.dec)
        self.loss_ctr.record(loss, self.loss_ring, (loss,))
        return loss

    def _evaluate_train(self, out):
        self.model.eval()
        with torch.no_grad():
            E, Rel = self.forward_fn(), _relations(self.model)
            evaluate_facts(E, Rel, self.tparts, out=out, scorer=self.dec.scorer)
        return E, Rel

    def _eval_epoch(self):
        loss = self._train_epoch()
        self.row[0:1].copy_(loss.reshape(1))
        try:
            E, Rel = self._evaluate_train(self.row[1:9])
            if self.vparts is not None:   # (against the same embeddings)
                evaluate_facts(E, Rel, self.vparts, out=self.row[9:17], score=self.score, scorer=self.dec.scorer)
        finally:
            self.model.train()
        (self.stopper if self.stopper is not None else self.eval_ctr).record_row(self.score, self.row, self.eval_ring)
        return loss

    def last_epoch(self):
        self.train_epoch()
        try:
            self._evaluate_train(self.last)
        finally:
            self.model.train()


def _run_schedule(run, sched, nepoch, poll, stopper):
    """The host side of `fit` and `fit_batches`: the epochs of `sched` in windows of `poll` on `run` (`train_epoch`,
    `eval_epoch`, `last_epoch`; `loss_ring`, `eval_ring`, `last`, `eval_ctr`), one look at the device per window, the
    reference's tuples for the rows up to and including the record that latched a stop, `restore_()` after it."""
    evals_before = 0     # evaluating epochs < nepoch in front of the current window = records at its start
    epoch = 0
    while epoch < nepoch:
        window = sched[epoch:epoch + poll]
        for e, eval_train, _, _ in window:
            if e == nepoch:
                run.last_epoch()
            elif eval_train:
                run.eval_epoch()
            else:
                run.train_epoch()
        epoch += len(window)
        st = run.eval_ctr.read()
        losses, rows, last_host = run.loss_ring.cpu(), run.eval_ring.cpu(), run.last.cpu()
        k = evals_before
        for e, eval_train, eval_valid, _ in window:
            tm = th = vm = vh = None
            if eval_train and e < nepoch:
                if k >= int(st.records):    # the stop was latched in front of this epoch
                    break
                r = rows[k % poll]
                k += 1
                tm, th = _unpack(r[1:9])
                if eval_valid:
                    vm, vh = _unpack(r[9:17])
            elif eval_train:
                tm, th = _unpack(last_host)
            yield (e, float(losses[(e - 1) % poll][0]), tm, th, vm, vh)
            if st.stop and k == int(st.records) and eval_train:
                break
        evals_before = k
        if st.stop:
            stopper.restore_()
            return


def fit(model, forward_fn, train_facts, valid_facts, optimizer, nepoch, eval_interval=1, mrr_batchsize=100,
        filter_ranks=True, early_stop=None, poll=8, graphed=True, sampler=None, warmup=3, static=None,
        l1_lambda=0.0, l2_lambda=0.0, decoder="triples", loss="bce", pos_weight=None, scorer="distmult",
        label_smoothing=0.0):
    """The reference's full-batch link-prediction loop (train_model, link_prediction.py:191-373, with test_model
    :375-422) as a generator over its tuples `(epoch, loss, train_mrr, train_hits_at_k, valid_mrr, valid_hits_at_k)`
    — epochs from 1, `loss` a float, an mrr `{"raw", "flt"}`, hits `{"raw": [h@1, h@3, h@10], "flt": [...]}`, None
    where the reference yields None (`eval_schedule`), "flt" values -1 when `filter_ranks` is off — with the host
    looking in every `poll` epochs only.  `forward_fn()` returns the node embeddings of the whole graph.  Training
    facts are evaluated in parts of `mrr_batchsize` (`FactParts`), `valid_facts` (None: no validation) likewise; the
    early stop scores `1 - valid_mrr["raw"]` (:363).  `early_stop`: None, a DeviceEarlyStop, or a host EarlyStop as
    its configuration.  `sampler`: see `train_step`; None draws the reference's 20 % in-batch negatives on the device
    (`DeviceNegativeSampler`, with the stored orders of the facts for the decoder's backward).  `l1_lambda` /
    `l2_lambda`: the loop's weight penalty (:306-322, `train_batch_step`), part of every step — captured ones too —
    and of the yielded loss.  `decoder="grouped"` (`sampler` a `NegativeSampler`), `loss`, `pos_weight`: the grouped
    loss in every step (`train_step`, `group_loss`); a `pos_weight` tensor is read once, here.  `scorer="complex"`:
    ComplEx in place of DistMult, in the steps' flat BCE (eager and captured) and in both evaluations of an evaluating
    epoch; not with the grouped decoder.  `decoder="all"` with `loss="softmax"`: the 1-vs-all softmax cross-entropy
    (`all_loss`) of the training facts against all nodes in every step, with either scorer; no negatives are drawn.
    `decoder="kvsall"` with `label_smoothing`: the KvsAll loss (`kvsall_loss`) of the training facts' distinct queries
    in every step, with either scorer; the warm-up epochs of a capture build the `KvsAllQueries`.

    An epoch is one of two step functions, chosen on the host from the epoch number (no device read):
    a training epoch — `train_step`, its loss into a device ring — and an evaluating epoch — the same, then ONE
    `forward_fn()` under `model.eval()` and `no_grad`, `evaluate_facts` of the training parts and of the validation
    parts against those same embeddings, the 17 values into row `records % poll` of a device ring by the early-stop
    record (`record_row`), the snapshot of the best state behind the record's flag.  With `graphed=True` each is one
    captured hipGraph, a single chain on the capture stream, and needs `ClipAdam(capturable=True)`; the `warmup`
    epochs of the capture are REAL optimizer steps taken before epoch 1 (the last of them also evaluates; the
    early-stop state and the rings are reset after them).  The last epoch (training metrics only, no record) evaluates
    eagerly.

    Stop semantics are `mrgcn_amd.train.fit`'s.  A run starts at record 0 (a DeviceEarlyStop's earlier state is
    discarded).  When a poll finds `stop` set, the rows up to and including the epoch whose record set it are
    yielded — no loss rows of later epochs —, the best state is restored in place and the generator ends; the up to
    `poll - 1` epochs that ran past the stop took optimizer steps, but the latched state ignored their records, their
    rows were not written, no snapshot was taken and the restore overwrites every tensor they changed.  A run that
    reaches `nepoch` is left with the LAST epoch's parameters and optimizer state; nothing is restored.

    Under `torch.use_deterministic_algorithms(True)` the step takes the deterministic decoder kernels; what is added
    here (ranks: integer counts; metrics: a fixed-order float64 sum; records) has no float atomics."""
    from ..train import _as_device_stopper
    dec = _decoder_args(decoder, loss, pos_weight, [sampler], "fit", scorer, label_smoothing)
    dev = next(model.parameters()).device
    nepoch, poll = int(nepoch), max(int(poll), 1)
    tparts = FactParts(train_facts, mrr_batchsize, filter_ranks, device=dev)
    vparts = FactParts(valid_facts, mrr_batchsize, filter_ranks, device=dev) if valid_facts is not None else None
    stopper = _as_device_stopper(early_stop, model, optimizer)
    run = FitEpochs(model, forward_fn, tparts, vparts, optimizer, stopper, poll, graphed, sampler, static, warmup,
                    l1_lambda, l2_lambda, dec)
    sched = eval_schedule(nepoch, eval_interval, vparts is not None)
    yield from _run_schedule(run, sched, nepoch, poll, stopper)


# ---- the reference's mini-batch run loop on the device (link_prediction.py:224-422; csrc/lp_batches.hip) -----------
def batch_eval_workspace(num_nodes, H, num_facts, device):
    """The workspace one `batch_eval` of that shape needs, as an int64 device tensor (kept by the caller)."""
    nbytes = int(_lib.load().mrgcn_distmult_batch_eval_workspace(int(num_nodes), int(H), int(num_facts)))
    if nbytes < 0:
        raise _lib.MrgcnError("batch_eval: sizes outside mrgcn_distmult_batch_eval's limits (at least one node, one "
                              "fact and one feature)")
    return torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=device)


def batch_eval(node_embeddings, edge_embeddings, facts, lists=None, slot=None, ranks=None, workspace=None,
               scorer="distmult"):
    """test_model's work on ONE batch (:392-414) in one call of three launches (mrgcn_distmult_batch_eval): the
    batch's `facts` (a contiguous int64 [n, 3] device tensor of batch-local ids, n >= 1) ranked against the batch's own
    `node_embeddings`, raw and — with `lists`, the four device tensors of `filter_lists(facts)` — filtered, and the
    float32 `[8]` slot raw mrr, hits@1, hits@3, hits@10, then the same filtered (-1 each without lists).  The ranks
    are `compute_ranks_fast`'s bit for bit (facts at positions >= the number of nodes unscored, as there), each slot
    half is `rank_metrics`' of those ranks.  `slot`: the contiguous float32 [8] row to write (None: a new one);
    `ranks`: a pair of contiguous int64 [2 n] device tensors (raw, flt; either may be None) that receive the ranks;
    `workspace`: `batch_eval_workspace(...)` of this shape (None: allocated here).  Returns the slot.  No
    synchronisation; capturable.  `scorer`: "distmult" only (`scorer="complex"` raises `MrgcnError`)."""
    _no_complex(scorer, "batch_eval")
    E = _f32_rows(node_embeddings.detach(), "node_embeddings")
    Rel = _f32_rows(edge_embeddings.detach(), "edge_embeddings")
    dev = E.device
    if not (torch.is_tensor(facts) and facts.is_cuda and facts.dtype == torch.int64 and facts.dim() == 2
            and facts.shape[1] == 3 and facts.is_contiguous() and facts.shape[0] >= 1):
        raise _lib.MrgcnError("batch_eval: facts is a contiguous, non-empty int64 [n, 3] tensor on the device")
    nf, N, H = int(facts.shape[0]), int(E.shape[0]), int(E.shape[1])
    if Rel.shape[1] != H:
        raise ValueError("batch_eval: node and edge embeddings differ in width")
    if N == 0:
        raise ValueError("batch_eval: no nodes")
    ls = _check_lists(lists, nf, "batch_eval") if lists is not None else [None] * 4
    if slot is None:
        slot = torch.empty(8, dtype=torch.float32, device=dev)
    elif not (torch.is_tensor(slot) and slot.is_cuda and slot.dtype == torch.float32 and tuple(slot.shape) == (8,)
              and slot.is_contiguous()):
        raise _lib.MrgcnError("batch_eval: slot is a contiguous float32 [8] tensor on the device")
    raw, flt = ranks if ranks is not None else (None, None)
    for r in (raw, flt):
        if r is not None and not (torch.is_tensor(r) and r.is_cuda and r.dtype == torch.int64
                                  and tuple(r.shape) == (2 * nf,) and r.is_contiguous()):
            raise _lib.MrgcnError("batch_eval: ranks are contiguous int64 [2 * n] tensors on the device")
    lib = _lib.load()
    if workspace is None:
        workspace = batch_eval_workspace(N, H, nf, dev)
    ws_bytes = int(workspace.numel()) * workspace.element_size()
    if not workspace.is_cuda or ws_bytes < int(lib.mrgcn_distmult_batch_eval_workspace(N, H, nf)):
        raise _lib.MrgcnError("batch_eval: the workspace is too small for this batch (batch_eval_workspace)")
    with torch.cuda.device(dev):
        _lib.check(lib.mrgcn_distmult_batch_eval(_ptr(E), E.stride(0), N, _ptr(Rel), Rel.stride(0), H, _ptr(facts), nf,
                                                 _ptr(ls[0]), _ptr(ls[1]), _ptr(ls[2]), _ptr(ls[3]), _ptr(workspace),
                                                 ws_bytes, _ptr(raw), _ptr(flt), _ptr(slot), _stream()),
                   "distmult_batch_eval")
    return slot


def _lp_batch_means(loss_slots, n_loss, train_slots, n_train, valid_slots, n_valid, row, score=None):
    dev = row.device
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mrgcn_lp_batch_means_f32(
            _ptr(loss_slots) if n_loss else None, int(n_loss), _ptr(train_slots) if n_train else None, int(n_train),
            _ptr(valid_slots) if n_valid else None, int(n_valid), _ptr(row), _ptr(score), _stream()),
            "lp_batch_means")


def _batch_lists(st, facts):
    """The batch's filter lists on the device, built once (shared with `evaluate_batches`)."""
    if st["lists"] is None:
        st["lists"] = _device_filter_lists(facts, st["device"])
    return st["lists"]


def _check_slots(slots, n, who):
    if not (torch.is_tensor(slots) and slots.is_cuda and slots.dtype == torch.float32 and slots.dim() == 2
            and slots.shape[1] == 8 and slots.is_contiguous() and slots.shape[0] >= n):
        raise _lib.MrgcnError(f"{who}: slots is a contiguous float32 [batches, 8] table on the device")


def eval_batches(model, batches, filtered=True, slots=None, ranks=None, scorer="distmult"):
    """test_model (:375-422) over prepared batches without the host: every batch's forward under `eval()` and
    `no_grad` (the model's mode is put back on exit), then `batch_eval` into row i of `slots`.  A batch's filter lists
    are built once and its workspace is allocated once; both stay with the batch.  Returns the float32 `[8]` device
    vector of the unweighted means over the batches (:416-419; -1 for the filtered four when not `filtered`) — or,
    with `slots` (the caller's float32 [batches, 8] table, e.g. `BatchFitEpochs`'), leaves the per-batch values there
    and returns None: the means are the caller's business.  `ranks`: a pair of int64 device buffers of
    `2 * sum(facts)` values (raw, flt; flt may be None when not `filtered`); batch i's ranks land at twice the facts in
    front of it, the order `evaluate_batches` flattens to.  No synchronisation.  `scorer`: "distmult" only
    (`scorer="complex"` raises `MrgcnError`; `evaluate_batches` ranks with ComplEx)."""
    _no_complex(scorer, "eval_batches")
    batches = list(batches)
    if not batches:
        raise _lib.MrgcnError("eval_batches: no batches")
    own = slots is None
    raw_all, flt_all = ranks if ranks is not None else (None, None)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            Rel = _relations(model).detach()
            at = 0
            for i, (batch, facts) in enumerate(batches):
                E = _embed(model, batch).detach()
                st = _batch_state(batch, facts, E.device)
                if i == 0:
                    if own:
                        slots = torch.empty((len(batches), 8), dtype=torch.float32, device=E.device)
                    _check_slots(slots, len(batches), "eval_batches")
                f = st["facts"]
                nf, shape = int(f.shape[0]), (int(E.shape[0]), int(E.shape[1]), int(f.shape[0]))
                ws = st.get("eval_ws")
                if ws is None or ws[0] != shape:
                    ws = st["eval_ws"] = (shape, batch_eval_workspace(*shape, E.device))
                pair = None
                if ranks is not None:
                    pair = (raw_all[at:at + 2 * nf] if raw_all is not None else None,
                            flt_all[at:at + 2 * nf] if flt_all is not None and filtered else None)
                batch_eval(E, Rel, f, _batch_lists(st, facts) if filtered else None, slots[i], pair, ws[1])
                at += 2 * nf
    finally:
        model.train(was_training)
    if not own:
        return None
    row = torch.empty(EVAL_ROW, dtype=torch.float32, device=slots.device)
    _lp_batch_means(None, 0, slots, len(batches), None, 0, row)
    return row[1:9]


def rank_batches(model, batches, filtered=True, scorer="distmult"):
    """`evaluate_batches`' result — `(mrr, hits_at_k, rankings)` as test_model returns them — from `eval_batches`:
    the batches' ranks land in two device buffers, the means come from the batches' slots, and everything is read back
    once, through pinned memory, after the last batch.  The rankings are `evaluate_batches`' exactly; its means are
    float32 means of float32 values where these are float64 sums rounded once.  `scorer`: "distmult" only
    (`scorer="complex"` raises `MrgcnError`)."""
    _no_complex(scorer, "rank_batches")
    batches = list(batches)
    if not batches:
        raise _lib.MrgcnError("rank_batches: no batches")
    dev = next(model.parameters()).device
    total = 2 * sum(int(np.asarray(f).shape[0]) if not torch.is_tensor(f) else int(f.shape[0]) for _, f in batches)
    raw = torch.empty(total, dtype=torch.int64, device=dev)
    flt = torch.empty(total, dtype=torch.int64, device=dev) if filtered else None
    means = eval_batches(model, batches, filtered, ranks=(raw, flt))
    means_h = torch.empty(8, dtype=torch.float32).pin_memory()
    ranks_h = torch.empty((2 if filtered else 1, total), dtype=torch.int64).pin_memory()
    means_h.copy_(means, non_blocking=True)
    ranks_h[0].copy_(raw, non_blocking=True)
    if filtered:
        ranks_h[1].copy_(flt, non_blocking=True)
    torch.cuda.current_stream(dev).synchronize()
    mrr, hits_at_k = _unpack(means_h)
    rankings = {"raw": ranks_h[0].tolist(), "flt": ranks_h[1].tolist() if filtered else [-1] * len(batches)}
    return mrr, hits_at_k, rankings


class BatchFitEpochs(_Epochs):
    """The epochs `fit_batches` is made of, as callables on one set of device tables (see `fit_batches` for what they
    do): `train_epoch()` — every training batch in order (`train_batch_step`, its loss into slot i), the mean of the
    slots into row `epochs % poll` of `loss_ring` —, `eval_epoch()` — the same, then `eval_batches` of the training
    batches and of the validation batches, the `EVAL_ROW` means into row `records % poll` of `eval_ring` by the
    early-stop record, the snapshot behind its flag — and `last_epoch()`: a training epoch, then the training metrics
    into `last`, eagerly.  `graphed=True`: the first two are one captured hipGraph each (`_Epochs`).  The epochs are
    counted in `stats()` (`lp.batch_epoch.*`, `lp.batch_eval_epoch.*`)."""
    _stats = ("lp.batch_epoch", "lp.batch_eval_epoch")

    def __init__(self, model, train_batches, valid_batches, optimizer, stopper=None, poll=8, graphed=True,
                 filter_ranks=True, samplers=None, warmup=3, clip=1.0, l1_lambda=0.0, l2_lambda=0.0,
                 decoder="triples", loss="bce", pos_weight=None, scorer="distmult", label_smoothing=0.0):
        _no_complex(scorer, "BatchFitEpochs")
        dec = _decoder_args(decoder, loss, pos_weight, [None] if samplers is None else [], "fit_batches",
                            label_smoothing=label_smoothing)
        train_batches, valid_batches = list(train_batches), list(valid_batches or [])
        if not train_batches:
            raise _lib.MrgcnError("fit_batches: no training batches")
        if stopper is not None and not valid_batches:
            raise _lib.MrgcnError("fit_batches: early stopping scores the validation MRR: pass valid_batches")
        if graphed and not getattr(optimizer, "capturable", False):
            raise _lib.MrgcnError("fit_batches(graphed=True) needs ClipAdam(..., capturable=True)")
        dev = _batch_state(*train_batches[0], next(model.parameters()).device)["device"]
        for batch, facts in train_batches + valid_batches:
            if _batch_state(batch, facts, dev)["device"] != dev:
                raise _lib.MrgcnError("fit_batches: the batches live on one device")
        self.model, self.optimizer, self.stopper, self.poll = model, optimizer, stopper, poll
        self.train_batches, self.valid_batches = train_batches, valid_batches
        self.filter_ranks, self.clip = bool(filter_ranks), clip
        self.l1_lambda, self.l2_lambda = float(l1_lambda), float(l2_lambda)
        self.samplers = [samplers(i, b, f) if samplers is not None else None for i, (b, f) in enumerate(train_batches)]
        self.dec = dec.checked(self.samplers, "fit_batches")
        nt, nv = len(train_batches), len(valid_batches)
        self._tables(dev, stopper, poll)
        self.loss_slots = torch.zeros(nt, dtype=torch.float32, device=dev)
        self.train_slots = torch.zeros((nt, 8), dtype=torch.float32, device=dev)
        self.valid_slots = torch.zeros((max(nv, 1), 8), dtype=torch.float32, device=dev)
        self._last_row = torch.zeros(EVAL_ROW, dtype=torch.float32, device=dev)
        self.last = self._last_row[1:9]
        self._start(graphed, warmup, optimizer, "fit_batches")

    def _train_epoch(self):
        self.model.train()   # (:232)
        for i, (batch, facts) in enumerate(self.train_batches):
            _train_batch_step(self.model, batch, facts, self.optimizer, None, self.clip, self.loss_slots[i:i + 1],
                              self.samplers[i], self.l1_lambda, self.l2_lambda, self.dec)
        _lp_batch_means(self.loss_slots, len(self.train_batches), None, 0, None, 0, self.row)
        self.loss_ctr.record(self.row[0:1], self.loss_ring, (self.row[0:1],))

    def _eval_epoch(self):
        self._train_epoch()
        try:
            nt, nv = len(self.train_batches), len(self.valid_batches)
            eval_batches(self.model, self.train_batches, self.filter_ranks, slots=self.train_slots)
            if nv:
                eval_batches(self.model, self.valid_batches, self.filter_ranks, slots=self.valid_slots)
            _lp_batch_means(None, 0, self.train_slots, nt, self.valid_slots, nv, self.row, self.score)
        finally:
            self.model.train()
        (self.stopper if self.stopper is not None else self.eval_ctr).record_row(self.score, self.row, self.eval_ring)

    def last_epoch(self):
        self.train_epoch()
        try:
            eval_batches(self.model, self.train_batches, self.filter_ranks, slots=self.train_slots)
            _lp_batch_means(None, 0, self.train_slots, len(self.train_batches), None, 0, self._last_row)
        finally:
            self.model.train()


def fit_batches(model, train_batches, valid_batches, optimizer, nepoch, eval_interval=1, filter_ranks=True,
                early_stop=None, poll=8, graphed=True, max_graph_batches=None, warmup=3, samplers=None,
                l1_lambda=0.0, l2_lambda=0.0, decoder="triples", loss="bce", pos_weight=None, scorer="distmult",
                label_smoothing=0.0):
    """The reference's mini-batch link-prediction loop (train_model with gcn_batchsize > 0, link_prediction.py:224-373,
    with test_model :375-422) as a generator over its tuples `(epoch, loss, train_mrr, train_hits_at_k, valid_mrr,
    valid_hits_at_k)`, with `fit`'s contract row for row: the schedule (`eval_schedule`), the loss ring and the eval
    ring of `poll` rows, the early-stop record on `1 - valid_mrr["raw"]`, the snapshot behind its flag, the latched stop
    and what is yielded around it, `restore_()` on a stop, a run that reaches `nepoch` left with the LAST epoch's state,
    and the eagerly evaluated last epoch.  The batches are prepared ones (`prepare_batches(mkbatches(...), device)`);
    `valid_batches` None or empty: no validation (both validation fields are None; early stopping then raises).

    A training epoch runs every training batch in `mkbatches`' order (`train_batch_step`, the batch's loss into its
    slot), then the mean of the slots (`np.mean(loss_lst)`, :331) into the loss ring.  An evaluating epoch adds
    `eval_batches` of the training batches, then of the validation batches — each batch's own forward under `eval()`,
    its ranks and its eight metric values in three launches (mrgcn_distmult_batch_eval) —, then the unweighted means
    over batches (mrgcn_lp_batch_means_f32, :416-419), then the record.  Nothing synchronises inside an epoch.
    `samplers(i, batch, facts) -> sampler` supplies training batch i's negatives (`train_batch_step`'s `sampler`);
    None draws the reference's 20 % in-batch corruptions on the device.

    `graphed=True` captures the two epochs (`BatchFitEpochs`; needs `ClipAdam(capturable=True)`, and its `warmup`
    epochs are REAL optimizer steps taken before epoch 1) when the evaluating epoch has at most `max_graph_batches`
    batch passes — `2 * len(train_batches) + len(valid_batches)`; default `node_classification.MAX_GRAPH_BATCHES`, the
    largest capture measured — and every batch has a fixed structure (masked or full batches).  Otherwise the eager
    epochs run, which are equally free of synchronisation: FB15k-237's 1 011 batches run eagerly.

    `l1_lambda` / `l2_lambda`: the loop's weight penalty (:306-322) in every batch step, eager or captured, and in
    every recorded loss (`train_batch_step`).  `decoder="grouped"` (with `samplers` that make `NegativeSampler`s,
    e.g. `batch_negative_samplers`), `loss`, `pos_weight`: the grouped loss in every batch step (`group_loss`).
    `decoder="all"` with `loss="softmax"`: the 1-vs-all softmax cross-entropy (`all_loss`) of every batch's facts
    against that batch's own nodes; `samplers` may stay None, and a sampler that is given is not called.
    `decoder="kvsall"` with `label_smoothing`: the KvsAll loss (`kvsall_loss`) of every batch's distinct queries against
    that batch's own nodes, the `KvsAllQueries` built by the warm-up epochs (or the first eager epoch) per batch.

    Out of scope: literal-encoder batches inside a capture, the partitioned engines, and `scorer="complex"` (raises
    `MrgcnError`: the fused batch evaluation scores DistMult only)."""
    from ..train import _as_device_stopper
    from .node_classification import MAX_GRAPH_BATCHES, _is_fixed_structure
    _no_complex(scorer, "fit_batches")
    dec = _decoder_args(decoder, loss, pos_weight, [None] if samplers is None else [], "fit_batches",
                        label_smoothing=label_smoothing)
    train_batches, valid_batches = list(train_batches), list(valid_batches or [])
    nepoch, poll = int(nepoch), max(int(poll), 1)
    if early_stop is not None and not valid_batches:
        raise _lib.MrgcnError("fit_batches: early stopping scores the validation MRR: pass valid_batches")
    if graphed and not getattr(optimizer, "capturable", False):
        raise _lib.MrgcnError("fit_batches(graphed=True) needs ClipAdam(..., capturable=True)")
    cap = MAX_GRAPH_BATCHES if max_graph_batches is None else int(max_graph_batches)
    capture = bool(graphed and 2 * len(train_batches) + len(valid_batches) <= cap
                   and all(_is_fixed_structure(b) for b, _ in train_batches + valid_batches))
    stopper = _as_device_stopper(early_stop, model, optimizer)
    run = BatchFitEpochs(model, train_batches, valid_batches, optimizer, stopper, poll, capture, filter_ranks, samplers,
                         warmup, l1_lambda=l1_lambda, l2_lambda=l2_lambda, decoder=dec)
    sched = eval_schedule(nepoch, eval_interval, bool(valid_batches))
    yield from _run_schedule(run, sched, nepoch, poll, stopper)
