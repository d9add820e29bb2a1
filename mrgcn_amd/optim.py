"""The optimizer half of the reference's own training loop on the fast path.

The reference drives a step as (mrgcn/tasks/node_classification.py:35-37, :190-193; link_prediction.py:325)

    optimizer = optim.Adam(optimizer_params(model, ...), lr=..., weight_decay=...)
    ...
    optimizer.zero_grad(); batch_loss.backward()
    nn.utils.clip_grad_norm_(model.parameters(), 1.0)
    optimizer.step()

With `torch.optim.Adam` / `torch.nn.utils.clip_grad_norm_` that loop works on this package's models as it is
(dense gradients).  The optimizer CHECKPOINT of run.py:232-235 / node_classification.py:73-80 needs one thing more:
the moments of the node-major `weight_I` must travel in the reference's `(B*N, out)` shape.  `install_as_mrgcn()`
therefore always binds `optim.Adam` inside the reference's two task modules to `ReferenceLayoutAdam` (torch's own
Adam with the layout translated in `state_dict()` / `load_state_dict()`), or to `RowSparseAdam` with
`patch_optimizer=True`; an optimizer built elsewhere gets the same through `speak_reference_layout(optimizer)`
(`reference_state_dict` / `load_reference_state_dict` are the one-shot forms).  Beyond the checkpoint, the node table
`weight_I` then costs a dense gradient write, a norm pass, a scaling pass and a dense Adam pass over memory that
mostly holds zeros.  `Adam` and `clip_grad_norm_` here are
drop-ins for the two names with the same call signatures: the backward leaves the gradient of a node-major
`weight_I` in row-sparse form (mrgcn_amd.functional), `clip_grad_norm_` folds its squared norm — a by-product of
the backward — into the total norm and hands the coefficient on, `Adam.step()` touches only the node blocks that
have (or ever had) gradient.  Same arithmetic as the dense loop (tests/test_gpu_reference_loop.py: golden vectors
of the reference's own loop).  `mrgcn_amd.install_as_mrgcn(patch_optimizer=True)` puts them in place of `optim.Adam`
and `nn.utils.clip_grad_norm_` inside the reference's task modules.

`ClipAdam` (clip_grad_norm_ and Adam as HIP kernels, csrc/optim.hip; the clip coefficient never leaves the device) lives
here too and the epoch driver, mrgcn_amd.train, imports it.  Its `step()` reads as the list of its phases.
"""
from __future__ import annotations

import collections
import ctypes as C
import os
import weakref

import torch

from . import _lib as L
from .functional import _stream, clear_row_grads, dense_from_rows, pop_row_grad
from .stats import bump

# MRGCN_MULTI=0: one launch per small tensor and phase (sum of squares, Adam) instead of the two multi-tensor launches
_MULTI = os.environ.get("MRGCN_MULTI", "1") != "0"
_MULTI_MAX_NUMEL = 1 << 20


def _to_reference_layout(t):
    """Moments of a node-major parameter, (N, B, F) -> the reference's (B*N, F)."""
    N, B, F = t.shape
    return t.permute(1, 0, 2).reshape(B * N, F)


def _from_reference_layout(t, shape):
    """The inverse: (B*N, F) -> node-major `shape` = (N, B, F)."""
    N, B, F = shape
    return t.view(B, N, F).permute(1, 0, 2).contiguous()


def _penalty_kernel_takes(p) -> bool:
    """May the penalty kernels step `p`?  float32, contiguous, on the GPU, dense storage."""
    return bool(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and not p.is_sparse
                and (p.grad is None or not p.grad.is_sparse))


def merge_row_grad(p, ent):
    """Adds the gradient a row-sparse entry stands for (scaled by the clip coefficient it may carry) to `p.grad`."""
    g = dense_from_rows(p, ent)
    pre = ent.pop("coef", None)
    if pre is not None:
        g = g * pre
    p.grad = g if p.grad is None else p.grad.add_(g)


class _SumSq:
    """Squared norms of float32 tensors added into a device double: atomically or, with `det`
    (torch.use_deterministic_algorithms(True)), in block order.  Owns the scratch of the deterministic kernels."""

    def __init__(self, device):
        self.device, self._det = device, None

    def det_scratch(self):
        """(block partials: written before they are read; ticket: zero at the start, left zero by every launch)"""
        if self._det is None:
            self._det = (torch.empty(int(L.load().mrgcn_sumsq_det_workspace()) // 8, dtype=torch.float64,
                                     device=self.device), torch.zeros((), dtype=torch.int32, device=self.device))
        return self._det

    def accum(self, ptr, numel, acc, s, det):
        lib = L.load()
        if det:
            dp, dt = (t.data_ptr() for t in self.det_scratch())
            L.check(lib.mrgcn_sumsq_accum_det_f32(ptr, numel, acc.data_ptr(), dp, dt, s), "mrgcn_sumsq_accum_det_f32")
        else:
            L.check(lib.mrgcn_sumsq_accum_f32(ptr, numel, acc.data_ptr(), s), "mrgcn_sumsq_accum_f32")


def _clip_coef(sumsq, max_norm, coef, norm, s):   # coef = min(1, max_norm / (norm + 1e-6)), norm = sqrt(sumsq)
    L.check(L.load().mrgcn_clip_coef_f32(sumsq.data_ptr(), float(max_norm), coef.data_ptr(), norm.data_ptr(), s),
            "mrgcn_clip_coef_f32")


# (`reg`: the regularised update over all nodes — decay, penalty; `owned`: this optimizer adds the penalty's gradient)
_RowGrad = collections.namedtuple("_RowGrad", "group p ent reg owned")
# `small`: indices of the dense gradients the multi-tensor launches take; `multi`: one launch closes the norm
_Launch = collections.namedtuple("_Launch", "hyper small multi det use_clip")


class ClipAdam(torch.optim.Optimizer):
    """clip_grad_norm_(all params, max_norm) followed by torch.optim.Adam, as two passes of
    HIP kernels: (1) sum of squares of every gradient into one device double, (2) Adam with
    the clip coefficient read from device memory.  Same hyper-parameter names / param-group
    layout as torch.optim.Adam so that `optimizer_params` groups (tasks/utils.py:8-45) work.

    `state_dict()` / `load_state_dict()` speak the reference's layout: the moments of a node-major
    `weight_I` (mrgcn_amd.layers.graph) are handed out and accepted as `(B*N, out)` tensors, so an
    optimizer checkpoint (run.py:230-236) is interchangeable with torch.optim.Adam over the reference
    model.  With `capturable=True` the step counter lives on the device (hipGraph replays advance it);
    `state_dict()` reads it back, `load_state_dict()` seeds it."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 max_norm=1.0, capturable=False):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self.max_norm = max_norm
        # capturable: step counter and bias corrections on the device (one per distinct betas), so
        # that a hipGraph-captured step replays correctly (see GraphedTrainStep)
        self.capturable = capturable
        self._dev_step = {}
        self._scratch = {}
        self._dist = None  # (group, ids of parameters sharded across ranks)
        self._state_gen = 0  # bumped by load_state_dict: row flags built for the old moments are re-derived
        self.reg_loss = None  # the weight penalty the last step() owned (step(l1_lambda=, l2_lambda=)), a device scalar

    # -- checkpoints --------------------------------------------------------------------------------
    def _sync_host_steps(self):
        """Device step counters (capturable) -> the per-parameter `step` entries.  Synchronises."""
        if not self._dev_step:
            return
        for group in self.param_groups:
            ent = self._dev_step.get(tuple(float(b) for b in group["betas"]))
            if ent is None:
                continue
            t = int(ent[0].item())
            for p in group["params"]:
                st = self.state.get(p)
                if st:
                    st["step"] = t

    def state_dict(self):
        self._sync_host_steps()
        sd = super().state_dict()
        return _translated(self, sd, _moments_out) or sd

    def load_state_dict(self, state_dict):
        params = [p for g in self.param_groups for p in g["params"]]
        sd = dict(state_dict, state=dict(state_dict["state"]))
        for k, st in sd["state"].items():
            p = params[k]
            if "exp_avg" not in st:
                continue
            if getattr(p, "_mrgcn_node_major", False) and st["exp_avg"].dim() == 2:
                st = dict(st)
                for key in ("exp_avg", "exp_avg_sq"):
                    st[key] = _from_reference_layout(st[key], p.shape)
                sd["state"][k] = st
            elif tuple(st["exp_avg"].shape) != tuple(p.shape):
                # same element count in another layout (a reference-shaped moment for a parameter this optimizer
                # does not know to be node-major) would load silently permuted
                raise L.MrgcnError(f"optimizer state {k}: moments of shape {tuple(st['exp_avg'].shape)} for a "
                                   f"parameter of shape {tuple(p.shape)}")
        super().load_state_dict(sd)
        self._state_gen += 1
        self._dev_step = {}  # re-seeded from the loaded `step` entries at the next step

    def set_distributed(self, group, sharded_params):
        """Node-partitioned training (mrgcn_amd.partition): `sharded_params` hold disjoint shards
        per rank (their squared norms add up across ranks); every other parameter is replicated
        and already carries the all-reduced gradient (counted once)."""
        self._dist = (group, {id(p) for p in sharded_params})

    def _dev_scratch(self, device):
        s = self._scratch.get(device)
        if s is None:
            s = dict(accum=torch.zeros((), dtype=torch.float64, device=device),   # (self-cleaning: zero between steps)
                     sumsq=torch.zeros((), dtype=torch.float64, device=device),
                     sumsq_sharded=torch.zeros((), dtype=torch.float64, device=device),
                     coef=torch.ones((), dtype=torch.float32, device=device),
                     norm=torch.zeros((), dtype=torch.float32, device=device),
                     sums=_SumSq(device))
            s["sums"].det_scratch()   # (allocated now: its ticket also serves the launch that closes the norm)
            self._scratch[device] = s
        return s

    def _index_rows_ok(self, p, ent) -> bool:
        """A compact-rows gradient (kind "index") may skip the rows outside its index set only while those rows hold no
        moments: checked once per optimizer state (a loaded state, dense steps in between), with one host read."""
        owner = (id(self), self._state_gen)
        if ent.get("seeded_for") != owner:
            if p.is_cuda and torch.cuda.is_current_stream_capturing():
                raise L.MrgcnError("ClipAdam: the first step with a compact literal gradient looks at the moments "
                                   "(a host read): run one step before capturing")
            st = self.state.get(p)
            ok = p.dim() == 2 and p.is_contiguous() and p.shape[1] % 4 == 0
            if ok and st and int(st.get("step", 0)) > 0:
                outside = torch.ones(p.shape[0], dtype=torch.bool, device=p.device)
                outside[ent["index"]] = False
                ok = not bool(((st["exp_avg"][outside] != 0).any() | (st["exp_avg_sq"][outside] != 0).any()).item())
            ent["dense_only"] = not ok
            ent["seeded_for"] = owner
        return not ent["dense_only"]

    def _new_state(self, p):
        st = self.state[p]
        if not st:
            st["step"] = 0
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        return st

    def _dev_step_entry(self, key, device):
        """The device step counter and bias corrections of one (beta1, beta2) (capturable)."""
        ent = self._dev_step.get(key)
        if ent is None:
            # seeded with the steps already taken (a loaded checkpoint, eager steps before)
            t0 = max([int(self.state[p].get("step", 0)) for g2 in self.param_groups
                      if tuple(float(b) for b in g2["betas"]) == key for p in g2["params"]
                      if self.state.get(p)] or [0])
            ent = (torch.full((), t0, dtype=torch.int64, device=device),
                   torch.ones(2, dtype=torch.float32, device=device))
            self._dev_step[key] = ent
        return ent

    def init_state(self):
        """What the first `step()` would allocate, without taking it: zero moments for every parameter that requires
        a gradient and, with `capturable`, the device step counters — so that a DeviceEarlyStop built in front of the
        first epoch has every buffer it snapshots.  A parameter that then never receives a gradient keeps its zero
        moments (and an entry in `state_dict()`) where `step()` alone would have left it without state; its value is
        the same either way."""
        for group in self.param_groups:
            for p in group["params"]:
                if p.requires_grad:
                    self._new_state(p)
            if self.capturable and group["params"]:
                self._dev_step_entry(tuple(float(b) for b in group["betas"]), group["params"][0].device)

    def _reg_rows_ok(self, ent) -> bool:
        """Can this row-sparse entry take the regularised row update (mrgcn_support_adam_rows_reg_f32)?  It needs the
        backward to have run on a gradient support and a shape the kernels take."""
        fz = ent.get("fused")
        return (fz is not None and fz.get("sup") is not None and self._dist is None
                and int(L.load().mrgcn_support_reg_norm_workspace(fz["sup"].handle, fz["B"], fz["F"])) >= 0)

    # -- step(): the phases ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None, *, l1_lambda=0.0, l2_lambda=0.0, reg_params=None, dense_penalty="torch"):
        """`l1_lambda` / `l2_lambda`: the reference's weight penalty (node_classification.py:172-188) on the parameters
        the CALLER LEFT OUT of the penalty it put into the loss — `reg_params`, by default the node-major tables that
        carry a row-sparse gradient.  The optimizer owns their penalty whichever route they end up on: r(p) =
        l1 sign(p) + 2 l2 p joins the gradient in front of this step's clip (`max_norm`), the value
        l1 sum|p| + l2 sum p^2 is left in `self.reg_loss` (a float32 device scalar; None when nothing was owned).
        `dense_penalty`: what an owned parameter off the regularised row update gets — "torch": r(p) is added to a
        dense `p.grad` with torch ops (a row-sparse entry is densified first); "kernel": the gradient stays as the
        backward left it (dense, or the flagged rows of a node-kind entry) and two multi-tensor launches do the
        penalty's share of the clip and the update (csrc/optim.hip: mrgcn_penalty_norm_multi_f32,
        mrgcn_adam_step_reg_multi_f32), in a fixed summation order."""
        if dense_penalty not in ("torch", "kernel"):
            raise ValueError(f"dense_penalty must be 'torch' or 'kernel', not {dense_penalty!r}")
        l1, l2 = float(l1_lambda), float(l2_lambda)
        pen = l1 > 0 or l2 > 0
        self.reg_loss = None
        rows, indexed, dense, torch_pen, kernel_pen = self._route(
            pen, {id(p) for p in reg_params} if (pen and reg_params is not None) else None,
            pen and dense_penalty == "kernel")
        self._add_torch_penalties(torch_pen, l1, l2)
        if not dense and not rows and not indexed and not kernel_pen:
            return None
        device = (dense[0][1] if dense else (rows or indexed or kernel_pen)[0][1]).device
        if not all(p.device == device for _, p in dense) or not all(p.device == device for _, p, _ in kernel_pen):
            raise L.MrgcnError("ClipAdam: all parameters must live on one GPU")
        sc, s = self._dev_scratch(device), _stream(device)
        # (contiguous and 16-byte aligned, as the vector kernels read them: a gradient that is a view into a flat
        # bucket at an odd offset is copied)
        grads = [p.grad if (p.grad.is_contiguous() and p.grad.data_ptr() % 16 == 0) else p.grad.contiguous().clone()
                 for _, p in dense]
        how = self._launch_plan(dense, grads, rows, indexed, kernel_pen)
        with torch.cuda.device(device):
            row_sumsq = self._penalty_prepass(rows, l1, l2, device, s)
            if kernel_pen:  # one more squared norm for the clip: sum (g + r(p))^2 over the penalised tensors
                row_sumsq = row_sumsq + [self._penalty_norm(kernel_pen, l1, l2, sc, s)]
            # capturable: one device counter (and its bias corrections) per distinct (beta1, beta2)
            betas = dict.fromkeys(tuple(float(b) for b in g["betas"]) for g in self.param_groups)
            bias = {key: self._dev_step_entry(key, device)[1] for key in betas} if self.capturable else {}
            if how.multi:
                self._norm_in_one_launch(sc, s, how, grads, len(row_sumsq), row_sumsq, indexed, bias)
            else:
                self._norm_per_tensor(sc, s, how, dense, grads, rows, row_sumsq, indexed, bias)
            coef_ptr = sc["coef"].data_ptr() if how.use_clip else 0
            self._step_rows(rows, bias, coef_ptr, l1, l2, s)
            self._step_indexed(indexed, bias, coef_ptr, s)
            self._step_dense(dense, grads, how, bias, coef_ptr, s)
            self._step_penalised(kernel_pen, bias, coef_ptr, l1, l2, s)
        # the kernels wrote through raw pointers: tell autograd (and every cache keyed by a tensor's version — the gate
        # decisions of models.mrgcn) that these parameters changed, as an in-place torch update would
        torch.autograd.graph.increment_version([p for _, p in dense] + [r.p for r in rows] + [p for _, p, _ in indexed]
                                               + [p for _, p, _ in kernel_pen])

    def _route(self, pen, owned, kernel=False):
        """Pops every row-sparse entry and sends each parameter to one update -> (`rows`: _RowGrad, `indexed`:
        (group, p, entry) of compact literal rows, `dense`: (group, p) stepped from `p.grad`, `torch_pen`: those of them
        whose penalty this optimizer owns, `kernel_pen`: (group, p, entry or None) — with `kernel`, the owned
        parameters that would have been `torch_pen`, stepped by the penalty kernels and not part of `dense`).  An
        entry stays row-sparse only while it is the parameter's whole gradient
        (`alone`); `plain` = and nothing but that gradient moves the parameter (no decay, no owned penalty).  Anything
        else is merged into `p.grad`: another term left a dense gradient there (a regulariser), no support, a shape
        outside the kernels — except that a node-kind entry with its own gradient buffer and flags (`g` / `cur`, no
        `fused`) goes to `kernel_pen` as it is."""
        rows, indexed, dense, torch_pen, kernel_pen = [], [], [], [], []
        for g in self.param_groups:
            wd = float(g["weight_decay"])
            for p in g["params"]:
                ent = pop_row_grad(p)
                index = ent is not None and ent.get("kind") == "index"
                mine = (id(p) in owned) if owned is not None else bool(
                    pen and ent is not None and not index and getattr(p, "_mrgcn_node_major", False))
                alone = ent is not None and p.grad is None
                plain = alone and wd == 0.0 and not mine
                if index and plain and self._dist is None and self._index_rows_ok(p, ent):
                    indexed.append((g, p, ent))
                elif not index and plain:
                    rows.append(_RowGrad(g, p, ent, False, False))
                elif not index and alone and self._reg_rows_ok(ent):
                    # every node block moves (decay, penalty): the row update over all N nodes, the loss's gradient
                    # still rebuilt from the support's dM
                    rows.append(_RowGrad(g, p, ent, True, mine))
                elif kernel and mine and _penalty_kernel_takes(p):
                    flagged = (ent is not None and not index and alone and ent.get("fused") is None
                               and ent.get("g") is not None and ent.get("cur") is not None and "coef" not in ent)
                    if ent is not None and not flagged:
                        merge_row_grad(p, ent)
                    kernel_pen.append((g, p, ent if flagged else None))
                else:
                    if ent is not None:
                        merge_row_grad(p, ent)
                    if mine:
                        torch_pen.append(p)
                    if mine or p.grad is not None:
                        dense.append((g, p))
        return rows, indexed, dense, torch_pen, kernel_pen

    def _add_torch_penalties(self, torch_pen, l1, l2):
        """The owned parameters on the dense route: r(p) joins `p.grad` and the value `self.reg_loss` with torch ops."""
        for p in torch_pen:
            r = None
            if l1 > 0:
                r = l1 * torch.sign(p)
                self.reg_loss = l1 * p.abs().sum() + (0 if self.reg_loss is None else self.reg_loss)
            if l2 > 0:
                r = (2.0 * l2) * p if r is None else r.add_(p, alpha=2.0 * l2)
                self.reg_loss = l2 * (p * p).sum() + (0 if self.reg_loss is None else self.reg_loss)
            p.grad = r if p.grad is None else p.grad.add_(r)

    def _launch_plan(self, dense, grads, rows, indexed, kernel_pen=()) -> _Launch:
        # The dense parameters besides the node table are a handful of small tensors: their squared norms, the
        # row-sparse gradients' norms, the clip coefficient and the device step counter take ONE launch
        # (mrgcn_sumsq_clip_multi_f32) and their Adam updates another (mrgcn_adam_step_multi_f32) when every group
        # shares (beta1, beta2, eps) — the reference's groups do (tasks/utils.py:8-45 vary lr / weight_decay only).
        groups = [g for g, _ in dense] + [r.group for r in rows] + [g for g, _, _ in indexed] + \
            [g for g, _, _ in kernel_pen]
        hyper = {(float(g["betas"][0]), float(g["betas"][1]), float(g["eps"])) for g in groups}
        small = [i for i, g in enumerate(grads) if g.numel() <= _MULTI_MAX_NUMEL]
        # (16 tensors per launch: a model with more — an MRGCN with encoders has ~40 — takes a few launches, not 2 x 40)
        multi = (_MULTI and self._dist is None and len(hyper) == 1 and len(small) >= 1
                 and len(rows) + bool(kernel_pen) <= 16)
        # torch.use_deterministic_algorithms(True): every squared norm summed in block order (the _det twins)
        det = torch.are_deterministic_algorithms_enabled()
        if det:
            bump("deterministic.sumsq")
        return _Launch(hyper, small, multi, det, self.max_norm is not None and self.max_norm > 0)

    def _penalty_prepass(self, rows, l1, l2, device, s):
        """-> per row-sparse gradient, the squared norm it brings to the clip (a 0-dim / 1-element double).  For an
        owned penalty that takes one read of the table in front of the clip: sum (g + r)^2 then stands where the entry's
        ||g||^2 would, and l1 sum|p| + l2 sum p^2 joins `self.reg_loss`.  (Weight decay needs none: torch adds wd . p
        inside Adam.step, after the clip.)"""
        lib, out = L.load(), []
        for r in rows:
            if not r.owned:
                out.append(r.ent["sumsq"])
                continue
            fz = r.ent["fused"]
            nbytes = int(lib.mrgcn_support_reg_norm_workspace(fz["sup"].handle, fz["B"], fz["F"]))
            ws = fz["sup"].workspace(("reg_norm", fz["B"], fz["F"]), (nbytes + 3) // 4)
            out3 = r.ent.get("reg_sums")
            if out3 is None or out3.device != device:
                out3 = r.ent["reg_sums"] = torch.empty(3, dtype=torch.float64, device=device)
            L.check(lib.mrgcn_support_reg_norm_f32(
                fz["sup"].handle, fz["dM"].data_ptr(), fz["ld"], fz["comp"].data_ptr(), fz["B"], fz["F"],
                r.p.data_ptr(), l1, l2, out3.data_ptr(), ws.data_ptr(), nbytes, s), "mrgcn_support_reg_norm_f32")
            out.append(out3[:1])
            term = (l1 * out3[1] + l2 * out3[2]).float()
            self.reg_loss = term if self.reg_loss is None else self.reg_loss + term
        if self.reg_loss is not None and self.reg_loss.dtype != torch.float32:
            self.reg_loss = self.reg_loss.float()
        return out

    @staticmethod
    def _penalty_args(items):
        """The tensor list of one penalty launch as ctypes arrays: gradients (NULL: none this step), sizes, row flags."""
        n = len(items)
        gs, fl, rl = [], [], []
        for _, p, ent in items:
            if ent is not None:   # the flagged rows of a node-kind entry: rows off the flags are never read
                gs.append(ent["g"].data_ptr())
                fl.append(ent["cur"].data_ptr())
                rl.append(p.numel() // max(p.shape[0], 1))
            else:
                gs.append(p.grad.data_ptr() if p.grad is not None else None)
                fl.append(None)
                rl.append(0)
        return (n, (C.c_void_p * n)(*[p.data_ptr() for _, p, _ in items]), (C.c_void_p * n)(*gs),
                (C.c_int64 * n)(*[p.numel() for _, p, _ in items]), (C.c_void_p * n)(*fl), (C.c_int32 * n)(*rl))

    @staticmethod
    def _penalty_launches(items):
        """<= 16 tensors a launch; a tensor above _MULTI_MAX_NUMEL takes one of its own."""
        small = [it for it in items if it[1].numel() <= _MULTI_MAX_NUMEL]
        return [[it] for it in items if it[1].numel() > _MULTI_MAX_NUMEL] + \
            [small[c0:c0 + 16] for c0 in range(0, len(small), 16)]

    def _penalty_norm(self, kernel_pen, l1, l2, sc, s):
        """-> the 1-element double sum (g + r(p))^2 over the penalised tensors (mrgcn_penalty_norm_multi_f32: block
        order, the same bits on every run); l1 sum|p| + l2 sum p^2 joins `self.reg_loss`.  No gradient is rewritten."""
        lib = L.load()
        for _, p, ent in kernel_pen:
            if ent is None and p.grad is not None and not (p.grad.is_contiguous() and p.grad.dtype == torch.float32):
                p.grad = p.grad.float().contiguous()
        if "pen3" not in sc:
            dev = kernel_pen[0][1].device
            sc["pen3"] = torch.zeros(3, dtype=torch.float64, device=dev)
            sc["pen_ws"] = torch.empty(int(lib.mrgcn_penalty_norm_workspace()) // 8, dtype=torch.float64, device=dev)
            sc["pen_ticket"] = torch.zeros((), dtype=torch.int32, device=dev)
        out3 = sc["pen3"]
        out3.zero_()   # (a device op inside the step: a captured step zeroes it at every replay)
        for part in self._penalty_launches(kernel_pen):
            n, pp, gp, nn_, fl, rl = self._penalty_args(part)
            L.check(lib.mrgcn_penalty_norm_multi_f32(n, pp, gp, nn_, fl, rl, l1, l2, out3.data_ptr(),
                                                     sc["pen_ws"].data_ptr(), sc["pen_ticket"].data_ptr(), s),
                    "mrgcn_penalty_norm_multi_f32")
        term = (l1 * out3[1] + l2 * out3[2]).float()
        self.reg_loss = term if self.reg_loss is None else self.reg_loss + term
        return out3[:1]

    def _step_penalised(self, kernel_pen, bias, coef_ptr, l1, l2, s):
        """Adam on the penalised tensors, every element: gg = (g + r(p)) . coef + wd . p (mrgcn_adam_step_reg_multi_f32)."""
        if not kernel_pen:
            return
        lib = L.load()
        bump("adam.reg_dense")
        by_hyper = {}
        for group, p, ent in kernel_pen:
            st = self._new_state(p)
            if ent is not None:
                self._seed_row_flags(ent, st)
            st["step"] += 1
            if ent is not None:   # every node holds moments afterwards (as the regularised row update leaves it)
                ent["ever"].fill_(1)
                ent["ever_in"] = "any"
            else:
                rows = getattr(p, "_mrgcn_rows", None)
                if rows is not None and not rows.get("dense_only"):
                    rows["seeded_for"] = None
            b1, b2 = group["betas"]
            key = (float(b1), float(b2), float(group["eps"]), None if self.capturable else int(st["step"]))
            by_hyper.setdefault(key, []).append((group, p, ent))
        for (b1, b2, eps, _), items in by_hyper.items():
            for c0 in range(0, len(items), 16):
                part = items[c0:c0 + 16]
                n, pp, gp, nn_, fl, rl = self._penalty_args(part)
                L.check(lib.mrgcn_adam_step_reg_multi_f32(
                    n, pp, gp, nn_, fl, rl,
                    (C.c_void_p * n)(*[self.state[p]["exp_avg"].data_ptr() for _, p, _ in part]),
                    (C.c_void_p * n)(*[self.state[p]["exp_avg_sq"].data_ptr() for _, p, _ in part]),
                    (C.c_float * n)(*[float(g["lr"]) for g, _, _ in part]),
                    (C.c_float * n)(*[float(g["weight_decay"]) for g, _, _ in part]), l1, l2, b1, b2, eps,
                    int(self.state[part[0][1]]["step"]), bias[(b1, b2)].data_ptr() if self.capturable else 0,
                    coef_ptr, s), "mrgcn_adam_step_reg_multi_f32")

    def _norm_in_one_launch(self, sc, s, how, grads, n_rows, row_sumsq, indexed, bias):
        """Total norm, clip coefficient and the device step counters when one multi-tensor launch can close the norm:
        large and surplus gradients stream into `accum` first, the closing launch adds its own tensors, the row-sparse
        norms and leaves `sumsq`, `coef`, `norm` and the bias corrections."""
        lib, sums, acc = L.load(), sc["sums"], sc["accum"]
        dp, dt = (t.data_ptr() for t in sums.det_scratch())
        small = how.small
        try:
            b1m, b2m, _ = next(iter(how.hyper))
            for i, g in enumerate(grads):
                if i not in small:  # (a large dense gradient: its own streaming pass into the same accumulator)
                    sums.accum(g.data_ptr(), g.numel(), acc, s, how.det)
            for c0 in range(0, len(small) - 16, 16) if len(small) > 16 else ():
                part = small[c0:c0 + 16]
                gp_, gn_ = ((C.c_void_p * len(part))(*[grads[i].data_ptr() for i in part]),
                            (C.c_int64 * len(part))(*[grads[i].numel() for i in part]))
                if how.det:
                    L.check(lib.mrgcn_sumsq_accum_multi_det_f32(len(part), gp_, gn_, acc.data_ptr(), dp, dt, s),
                            "mrgcn_sumsq_accum_multi_det_f32")
                else:
                    L.check(lib.mrgcn_sumsq_accum_multi_f32(len(part), gp_, gn_, acc.data_ptr(), s),
                            "mrgcn_sumsq_accum_multi_f32")
            closing = [grads[i] for i in small[(len(small) - 1) // 16 * 16:]]   # the launch that also closes the norm
            for _, _, ent in indexed:  # (a compact gradient: in the closing launch while it has room for it)
                if len(closing) < 16 and ent["g"].numel() <= 4 * _MULTI_MAX_NUMEL:
                    closing.append(ent["g"])
                else:
                    sums.accum(ent["g"].data_ptr(), ent["g"].numel(), acc, s, how.det)
            gp = (C.c_void_p * len(closing))(*[g.data_ptr() for g in closing])
            gn = (C.c_int64 * len(closing))(*[g.numel() for g in closing])
            ex = (C.c_void_p * max(n_rows, 1))(*[t.data_ptr() for t in row_sumsq])
            dstep = self._dev_step.get((b1m, b2m)) if self.capturable else None
            args = (len(closing), gp, gn, n_rows, ex, acc.data_ptr(), dt,
                    float(self.max_norm) if how.use_clip else 0.0, sc["sumsq"].data_ptr(), sc["coef"].data_ptr(),
                    sc["norm"].data_ptr(), dstep[0].data_ptr() if dstep else 0, b1m, b2m,
                    dstep[1].data_ptr() if dstep else 0)
            if how.det:
                L.check(lib.mrgcn_sumsq_clip_multi_det_f32(*args, dp, s), "mrgcn_sumsq_clip_multi_det_f32")
            else:
                L.check(lib.mrgcn_sumsq_clip_multi_f32(*args, s), "mrgcn_sumsq_clip_multi_f32")
            # groups with other betas (no gradient this step): their counters too
            self._advance_counters({k: v for k, v in bias.items() if k != (b1m, b2m)}, s)
        except BaseException:
            # the scratch words are self-cleaning only when the closing launch ran: a failure in between must not
            # leak a partial sum into every later norm
            acc.zero_()
            sums.det_scratch()[1].zero_()
            raise

    def _norm_per_tensor(self, sc, s, how, dense, grads, rows, row_sumsq, indexed, bias):
        """The same with one accumulate call per gradient: groups that differ in (beta1, beta2, eps), MRGCN_MULTI=0, a
        distributed group, where the sharded parameters' squared norms add up across ranks."""
        sums, sumsq, sharded_sum = sc["sums"], sc["sumsq"], sc["sumsq_sharded"]
        sumsq.zero_()
        sharded_sum.zero_()
        sharded = self._dist[1] if self._dist else ()
        for (_, p), g in zip(dense, grads):
            sums.accum(g.data_ptr(), g.numel(), sharded_sum if id(p) in sharded else sumsq, s, how.det)
        for r, sq in zip(rows, row_sumsq):  # ||g||^2 came for free with the gradient
            (sharded_sum if id(r.p) in sharded else sumsq).add_(sq.reshape(()))
        for sq in row_sumsq[len(rows):]:    # (the penalised tensors' sum (g + r(p))^2: never sharded)
            sumsq.add_(sq.reshape(()))
        for _, _, ent in indexed:
            sums.accum(ent["g"].data_ptr(), ent["g"].numel(), sumsq, s, how.det)
        if self._dist:
            from .partition import all_reduce_sum_
            all_reduce_sum_(sharded_sum, self._dist[0])
        sumsq += sharded_sum
        if how.use_clip:
            _clip_coef(sumsq, self.max_norm, sc["coef"], sc["norm"], s)
        self._advance_counters(bias, s)

    def _advance_counters(self, bias, s):
        for key, bc_t in bias.items():
            L.check(L.load().mrgcn_adam_bias_f32(self._dev_step[key][0].data_ptr(), key[0], key[1], bc_t.data_ptr(), s),
                    "mrgcn_adam_bias_f32")

    def _seed_row_flags(self, ent, st):
        """`ever` flags that have not seen this optimizer's moments yet (a loaded or dense-built state, a fresh gradient
        entry): every node that holds a non-zero moment counts as `ever`."""
        owner = (id(self), self._state_gen)
        if ent.get("seeded_for") == owner:
            return
        ent["ever"].zero_()
        ent["ever_in"] = None      # which row set the flags lie inside: None = none set yet
        if st["step"] > 0:   # (a parameter that never took a step has zero moments)
            nz = (st["exp_avg"] != 0).flatten(1).any(1) | (st["exp_avg_sq"] != 0).flatten(1).any(1)
            ent["ever"] |= nz.to(torch.uint8)
            ent["ever_in"] = "any"  # (moments from steps this entry has not seen)
        ent["seeded_for"] = owner

    def _step_rows(self, rows, bias, step_coef_ptr, l1, l2, s):
        """Adam on the row-sparse gradients of node-major tables: regularised over all nodes, on the gradient support,
        rebuilt from dM by the plan's flags, or from the gradient buffer."""
        lib = L.load()
        for group, p, ent, reg, owned in rows:
            st = self._new_state(p)
            self._seed_row_flags(ent, st)
            st["step"] += 1
            b1, b2 = group["betas"]
            fz = ent.get("fused")
            # the coefficient of a clip that ran between backward and step (mrgcn_amd.optim.clip_grad_norm_)
            pre = ent.pop("coef", None)
            if fz is not None and fz.get("comp_version") is not None and fz["comp"]._version != fz["comp_version"]:
                raise L.MrgcnError("row-sparse weight_I gradient: weight_I_comp was modified between backward and "
                                   "the node table's update (the fused update re-reads it)")
            # what the four kernels share
            pmv = (p.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr())
            hyp = (float(group["lr"]), float(b1), float(b2), float(group["eps"]))
            tail = (int(st["step"]), bias[(float(b1), float(b2))].data_ptr() if self.capturable else 0,
                    pre.data_ptr() if pre is not None else step_coef_ptr)
            ever = ent["ever"].data_ptr()
            src = (fz["dM"].data_ptr(), fz["ld"]) if fz is not None else None
            if reg:
                # all N nodes, gg = (g + r(p)) . coef + wd . p; r only where this optimizer owns the penalty.
                # Every node holds moments afterwards: a later plain step must look outside its support.
                ent["ever_in"] = "any"
                bump("adam.reg")
                L.check(lib.mrgcn_support_adam_rows_reg_f32(
                    fz["sup"].handle, *src, fz["comp"].data_ptr(), fz["B"], fz["F"], *pmv, ever, *hyp,
                    float(group["weight_decay"]), l1 if owned else 0.0, l2 if owned else 0.0, *tail, s),
                    "mrgcn_support_adam_rows_reg_f32")
            elif fz is not None and fz.get("sup") is not None:  # the same on the gradient support of the label set
                # every step since the flags were zeroed ran on THIS support: no node outside it holds moments and
                # the pass that looks for such nodes is not launched
                inside = ent.get("ever_in", "any")
                outside = 0 if (inside is None or inside is fz["sup"]) else 1
                ent["ever_in"] = fz["sup"] if not outside else "any"
                bump("adam.list")
                L.check(lib.mrgcn_support_adam_rows_fused_f32(
                    fz["sup"].handle, *src, fz["comp"].data_ptr(), fz["B"], fz["F"], *pmv, ever, *hyp, *tail,
                    outside, s), "mrgcn_support_adam_rows_fused_f32")
            elif fz is not None:  # no gradient tensor: the blocks are rebuilt from dM inside the Adam pass
                ent["ever_in"] = "any"
                bump("adam.rows_fused")
                L.check(lib.mrgcn_adam_step_rows_fused_f32(
                    fz["plan"].handle, *src, fz["live"].data_ptr(), fz["comp"].data_ptr(), fz["B"], fz["F"], *pmv,
                    ent["cur"].data_ptr(), ever, *hyp, *tail, s), "mrgcn_adam_step_rows_fused_f32")
            else:
                ent["ever_in"] = "any"
                bump("adam.rows")
                L.check(lib.mrgcn_adam_step_rows_f32(
                    pmv[0], ent["g"].data_ptr(), *pmv[1:], p.shape[0], p.numel() // max(p.shape[0], 1),
                    ent["cur"].data_ptr(), ever, *hyp, *tail, s), "mrgcn_adam_step_rows_f32")

    def _step_indexed(self, indexed, bias, step_coef_ptr, s):
        """Adam on the compact rows of a literal operand: the rows of the index set only."""
        for group, p, ent in indexed:
            st = self._new_state(p)
            st["step"] += 1
            b1, b2 = group["betas"]
            bc = bias[(float(b1), float(b2))].data_ptr() if self.capturable else 0
            pre = ent.pop("coef", None)
            g = ent["g"]
            bump("adam.index_rows")
            L.check(L.load().mrgcn_adam_step_index_rows_f32(
                p.data_ptr(), g.data_ptr(), g.stride(0), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                ent["index_ptr"], g.shape[0], p.numel() // max(p.shape[0], 1), float(group["lr"]), float(b1),
                float(b2), float(group["eps"]), int(st["step"]), bc,
                pre.data_ptr() if pre is not None else step_coef_ptr, s), "mrgcn_adam_step_index_rows_f32")

    def _step_dense(self, dense, grads, how, bias, coef_ptr, s):
        """Adam from `p.grad`: the small tensors 16 to a launch when they share hyper-parameters and step count, others
        one launch each."""
        lib, small = L.load(), how.small
        for _, p in dense:
            self._new_state(p)["step"] += 1
            rows = getattr(p, "_mrgcn_rows", None)
            if rows is not None and not rows.get("dense_only"):
                rows["seeded_for"] = None  # a dense step may put moments where the row flags never looked
        # (host-side bias corrections are per step count: the one launch needs the tensors to share it)
        adam_multi = how.multi and (self.capturable or len({int(self.state[dense[i][1]]["step"]) for i in small}) == 1)
        if adam_multi:
            b1m, b2m, epsm = next(iter(how.hyper))
            for c0 in range(0, len(small), 16):
                sel = [(dense[i][0], dense[i][1], grads[i]) for i in small[c0:c0 + 16]]
                n = len(sel)
                arr = lambda ptrs: (C.c_void_p * n)(*ptrs)  # noqa: E731
                L.check(lib.mrgcn_adam_step_multi_f32(
                    n, arr([p.data_ptr() for _, p, _ in sel]), arr([g.data_ptr() for _, _, g in sel]),
                    arr([self.state[p]["exp_avg"].data_ptr() for _, p, _ in sel]),
                    arr([self.state[p]["exp_avg_sq"].data_ptr() for _, p, _ in sel]),
                    (C.c_int64 * n)(*[p.numel() for _, p, _ in sel]),
                    (C.c_float * n)(*[float(g["lr"]) for g, _, _ in sel]),
                    (C.c_float * n)(*[float(g["weight_decay"]) for g, _, _ in sel]), b1m, b2m, epsm,
                    int(self.state[sel[0][1]]["step"]), bias[(b1m, b2m)].data_ptr() if self.capturable else 0,
                    coef_ptr, s), "mrgcn_adam_step_multi_f32")
        for i, ((group, p), g) in enumerate(zip(dense, grads)):
            if adam_multi and i in small:
                continue
            st = self.state[p]
            b1, b2 = group["betas"]
            args = (p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel(),
                    float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]))
            if self.capturable:
                L.check(lib.mrgcn_adam_step_dev_f32(*args, bias[(float(b1), float(b2))].data_ptr(), coef_ptr, s),
                        "mrgcn_adam_step_dev_f32")
            else:
                L.check(lib.mrgcn_adam_step_f32(*args, int(st["step"]), coef_ptr, s), "mrgcn_adam_step_f32")

    def last_grad_norm(self) -> float:
        """Total gradient norm of the last step (synchronises)."""
        return float(self._scratch[next(iter(self._scratch))]["norm"].item())


class Adam(ClipAdam):
    """`torch.optim.Adam(params, lr, betas, eps, weight_decay)` on HIP kernels; no clipping of its own (the
    reference clips with `nn.utils.clip_grad_norm_` between backward and step).  `state_dict()` /
    `load_state_dict()` speak the reference's layout (ClipAdam).

    `row_sparse` (default False: every gradient dense, `.grad` of every parameter as torch leaves it — any clip,
    scaler or inspection code sees all of it).  True: the optimizer announces itself on the node-major `weight_I`
    parameters it owns and a plain `loss.backward()` then leaves their gradient in ROW-SPARSE form (`weight_I.grad`
    stays None; flags, `dM` and the squared norm travel on the parameter) — with `weight_decay` as well: torch adds
    wd . p inside `Adam.step`, after the clip, so the norm below is unchanged and the decay happens in the row update
    (an L1 / L2 term the caller's loop writes into the loss still arrives as a dense `.grad`).  Only this module's `clip_grad_norm_`
    knows that form — torch's would skip the node table, i.e. leave its norm out of the total and step it unclipped —
    so the two go together: `RowSparseAdam` + `clip_grad_norm_`, which is what `install_as_mrgcn(patch_optimizer=True)`
    binds inside the reference's task modules."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, *,
                 foreach=None, maximize=False, capturable=False, differentiable=False, fused=None,
                 row_sparse=False):
        if amsgrad or maximize or differentiable:
            raise L.MrgcnError("mrgcn_amd.optim.Adam: amsgrad / maximize / differentiable are not implemented")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_norm=None,
                         capturable=capturable)
        if row_sparse:
            me = weakref.ref(self)
            for g in self.param_groups:
                # (a decayed group too: every node block then moves, which the regularised row update does from the
                # same row-sparse form when the backward ran on a gradient support — ClipAdam.step; otherwise the
                # entry is densified there, as before)
                for p in g["params"]:
                    if getattr(p, "_mrgcn_node_major", False):
                        p._mrgcn_row_consumer = me

    def zero_grad(self, set_to_none: bool = True):
        clear_row_grads([p for g in self.param_groups for p in g["params"]])
        super().zero_grad(set_to_none=set_to_none)


class RowSparseAdam(Adam):
    """`Adam(row_sparse=True)` under the constructor signature of `torch.optim.Adam`: what the reference's loop gets
    for `optim.Adam` next to this module's `clip_grad_norm_` (mrgcn_amd.patch_task_optimizer)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, **kw):
        kw.setdefault("row_sparse", True)
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, **kw)


_CLIP_SUMS: dict = {}  # device -> the _SumSq of clip_grad_norm_


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """`torch.nn.utils.clip_grad_norm_` that also sees gradients in row-sparse form.  The total norm, the
    coefficient `max_norm / (norm + 1e-6)` (clamped to 1) and the scaling stay on the device; the returned norm
    is a 0-dim device tensor like torch's.  Anything this path does not cover (other norm types, no row-sparse
    gradient among the parameters, gradients on the CPU / another GPU / of another dtype) goes to torch's
    implementation, row-sparse entries densified first."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    params = list(parameters)
    rows = [(p, getattr(p, "_mrgcn_rows", None)) for p in params]
    rows = [(p, e) for p, e in rows if e is not None and e["fresh"]]

    def torch_clip():   # densify, then torch
        for p, e in rows:
            e["fresh"] = False
            merge_row_grad(p, e)
        return torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=norm_type,
                                              error_if_nonfinite=error_if_nonfinite, foreach=foreach)
    if not rows or float(norm_type) != 2.0:
        return torch_clip()
    for p, e in rows:
        if p.grad is not None:  # a second, dense term on the same parameter: one dense gradient
            e["fresh"] = False
            merge_row_grad(p, e)
    rows = [(p, e) for p, e in rows if e["fresh"]]
    dev = (rows[0][0] if rows else params[0]).device
    dense = [p.grad for p in params if p.grad is not None]
    if dev.type != "cuda" or any(g.device != dev or g.dtype != torch.float32 or g.is_sparse for g in dense) \
            or any(p.device != dev for p, _ in rows):
        # gradients on another device (the reference spreads modules over model.devices) or of another type: the
        # kernels below would read them as float32 pointers of `dev`
        return torch_clip()
    sumsq = torch.zeros((), dtype=torch.float64, device=dev)
    coef = torch.ones((), dtype=torch.float32, device=dev)
    norm = torch.zeros((), dtype=torch.float32, device=dev)
    s = _stream(dev)
    det = torch.are_deterministic_algorithms_enabled()
    if det:  # torch.use_deterministic_algorithms(True): the squared norms summed in block order
        bump("deterministic.sumsq")
    sums = _CLIP_SUMS.get(str(dev))
    if sums is None:
        sums = _CLIP_SUMS[str(dev)] = _SumSq(dev)
    with torch.cuda.device(dev):
        for g in [g if g.is_contiguous() else g.contiguous() for g in dense]:
            sums.accum(g.data_ptr(), g.numel(), sumsq, s, det)
        for _, e in rows:
            if e.get("kind") == "index":   # compact rows of a literal operand: the norm of the compact gradient
                sums.accum(e["g"].data_ptr(), e["g"].numel(), sumsq, s, det)
            else:
                sumsq.add_(e["sumsq"])
        _clip_coef(sumsq, max_norm, coef, norm, s)
    if error_if_nonfinite and not bool(torch.isfinite(norm)):
        raise RuntimeError("The total norm for gradients from `parameters` is non-finite, so it cannot be clipped")
    for g in dense:
        g.mul_(coef)
    for _, e in rows:
        e["coef"] = coef  # applied inside the row-sparse Adam pass
    return norm


# ---- torch.optim.Adam over this package's models: checkpoint layout ---------------------------------------------
def _moments_out(st, p):
    return {key: (_to_reference_layout(v) if torch.is_tensor(v) and v.dim() == 3 else v) for key, v in st.items()}


def _moments_in(st, p):
    ref = (p.shape[0] * p.shape[1], p.shape[2])
    return {key: (_from_reference_layout(v, p.shape) if torch.is_tensor(v) and v.dim() == 2 and tuple(v.shape) == ref
                  else v) for key, v in st.items()}


def _translated(optimizer, state_dict, fn):
    """`state_dict` with `fn` applied to the state of every node-major parameter; None when there is none."""
    params = [p for g in optimizer.param_groups for p in g["params"]]
    idx = {i for i, p in enumerate(params) if getattr(p, "_mrgcn_node_major", False)}
    if not idx:
        return None
    return dict(state_dict, state={k: (fn(st, params[k]) if k in idx else st) for k, st in state_dict["state"].items()})


def _ref_layout_post_hook(optimizer, state_dict):
    """state_dict post-hook: moments of node-major parameters leave in the reference's `(B*N, out)` shape."""
    return _translated(optimizer, state_dict, _moments_out)


def _ref_layout_load_pre_hook(optimizer, state_dict):
    """load_state_dict pre-hook: reference-shaped moments of node-major parameters are transposed on the way in."""
    return _translated(optimizer, state_dict, _moments_in)


def speak_reference_layout(optimizer):
    """Makes ANY torch optimizer whose state tensors have the parameter's shape (Adam, AdamW, SGD with momentum, ...)
    save and load its checkpoint in the reference's layout: `optimizer.state_dict()` hands the moments of a node-major
    `weight_I` out as `(B*N, out)` (what `torch.save(optimizer.state_dict())` of run.py:232-235 holds for the reference
    model) and `optimizer.load_state_dict()` accepts them in that shape (node_classification.py:73-80) — instance
    hooks, nothing global.  Idempotent; returns the optimizer.  `ClipAdam` and its subclasses speak it natively."""
    if isinstance(optimizer, ClipAdam) or optimizer.__dict__.get("_mrgcn_reference_layout"):
        return optimizer
    optimizer.register_state_dict_post_hook(_ref_layout_post_hook)
    optimizer.register_load_state_dict_pre_hook(_ref_layout_load_pre_hook)
    optimizer.__dict__["_mrgcn_reference_layout"] = True
    return optimizer


class ReferenceLayoutAdam(torch.optim.Adam):
    """`torch.optim.Adam` itself — torch's arithmetic, dense gradients, every keyword — whose checkpoints are in the
    reference's layout (`speak_reference_layout`).  What `install_as_mrgcn()` binds for `optim.Adam` inside the
    reference's task modules by default, so that `optimizer.load_state_dict(checkpoint['optimizer_state_dict'])`
    (node_classification.py:73-80) takes a checkpoint written by the reference and `optimizer.state_dict()`
    (run.py:230-236) writes one the reference can load."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        speak_reference_layout(self)

    def __setstate__(self, state):   # (unpickling / deepcopy drop instance hooks)
        super().__setstate__(state)
        # load_state_dict ends in __setstate__ too, with the hook dicts intact: register again only when they are gone
        if not self.__dict__.get("_optimizer_state_dict_post_hooks"):
            self.__dict__.pop("_mrgcn_reference_layout", None)
        speak_reference_layout(self)


def reference_state_dict(optimizer) -> dict:
    """`optimizer.state_dict()` with the moments of node-major `weight_I` parameters in the reference's `(B*N, out)`
    layout — what `torch.save(optimizer.state_dict())` of run.py:232-235 holds for the reference model.  For
    any optimizer whose state tensors have the parameter's shape (torch.optim.Adam, AdamW, ...)."""
    sd = optimizer.state_dict()
    if isinstance(optimizer, ClipAdam) or optimizer.__dict__.get("_mrgcn_reference_layout"):
        return sd  # already speaks the reference's layout
    return _translated(optimizer, sd, _moments_out) or dict(sd)


def load_reference_state_dict(optimizer, state_dict) -> None:
    """The inverse: loads an optimizer checkpoint written for the reference model (or by `reference_state_dict`)."""
    if not (isinstance(optimizer, ClipAdam) or optimizer.__dict__.get("_mrgcn_reference_layout")):
        state_dict = _translated(optimizer, state_dict, _moments_in) or state_dict
    optimizer.load_state_dict(state_dict)
