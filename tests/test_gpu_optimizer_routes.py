"""Every route of `ClipAdam.step` through the public surface only (`ClipAdam`, `mrgcn_amd.optim.Adam`, `.step()`,
`.state`, `last_grad_norm()`, `state_dict()`, `mrgcn_amd.stats()`): gradients set by hand, three steps with a fresh
seeded N(0, s^2) gradient each, against `torch.nn.utils.clip_grad_norm_` + `torch.optim.Adam` on float64 copies of
the same parameters and gradients on the GPU.

The routes: one group (one closing norm launch, one multi-tensor Adam launch), 1 / 16 / 17 / 32 / 33 small tensors
(the 16-tensor chunks of both launches), groups that differ in betas or eps (the per-tensor norm without a
distributed group), a dense gradient above the multi-tensor size limit next to small ones and alone, a parameter
whose first gradient comes at step 2 (norm in one launch, Adam per tensor; with `capturable` the device counter),
a gradient at an unaligned address (copied), no clip at all, all of it again under
`torch.use_deterministic_algorithms(True)`, and a compact-rows node table next to 16 small tensors (the closing
launch has no room left for the compact gradient).

BOUNDS: errors are in units of each array's largest magnitude (as in tests/test_gpu_weight_reg_kernels.py), the
worst over the tensors of a case and over the cases; each bound is TWICE what the commit before the optimizer
moved into mrgcn_amd.optim measured on an MI355X:

    p 1.245e-07  exp_avg 5.555e-07  exp_avg_sq 1.310e-05  norm 6.478e-08

over three repetitions of the matrix, the same figures with the flag on and off (the worst elements are Adam's, not
the norm's; exp_avg_sq carries the float32 rounding of 1 - beta2 = 0.001, 1.3e-5 of it).

`late_capturable` has a bound of its own for p: with `capturable` ONE device counter per (beta1, beta2) gives every
parameter of the group the bias corrections of the group's step, so a parameter whose first gradient comes at
step 2 is stepped with the corrections of step 2 where torch (one counter per parameter) uses those of step 1 —
measured 1.356e-03 of the largest |p| in both modes; its moments meet the common bounds."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STEPS = 3
BIG = (1 << 20) + 4   # above the multi-tensor launches' size limit (1 << 20 elements)

# twice the measured worst errors (module docstring): p, exp_avg, exp_avg_sq, norm
BOUNDS = (2 * 1.245e-07, 2 * 5.555e-07, 2 * 1.310e-05, 2 * 6.478e-08)
BOUND_LATE_CAPTURABLE_P = 2 * 1.356e-03


def _group(sizes, **kw):
    return dict(sizes=tuple(sizes), **kw)


def _small(n):
    return tuple(1 + (5 * i) % 13 for i in range(n))


# name -> dict(groups, s = the gradient's sigma, and what differs from ClipAdam(max_norm=1.0))
CASES = {
    # 5174 elements: s = 1 gives a norm near 72 (clip active), 1e-3 one near 0.07 (idle)
    "single_clipped": dict(groups=[_group((1, 3, 7, 64, 1000, 4099))], s=1.0),
    "single_idle": dict(groups=[_group((1, 3, 7, 64, 1000, 4099))], s=1e-3),
    **{f"chunks_{n}": dict(groups=[_group(_small(n))], s=1.0 if n % 2 else 1e-2) for n in (1, 16, 17, 32, 33)},
    "betas": dict(groups=[_group((5, 64, 333)), _group((3, 1000), betas=(0.8, 0.99))], s=1.0),
    "eps": dict(groups=[_group((5, 64, 333)), _group((3, 1000), eps=1e-6, lr=3e-3, weight_decay=1e-2)], s=1e-3),
    "large_with_small": dict(groups=[_group((7, BIG, 64, 1000))], s=1e-2),
    "large_alone": dict(groups=[_group((BIG,))], s=1e-4),
    "late": dict(groups=[_group((64, 333, 7))], s=1.0, late=1),
    "late_capturable": dict(groups=[_group((64, 333, 7))], s=1.0, late=1, capturable=True),
    "unaligned": dict(groups=[_group((1000, 64))], s=1.0, unaligned=0),
    "no_clip": dict(groups=[_group((1, 3, 7, 64, 1000, 4099), weight_decay=1e-3)], s=1.0, no_clip=True),
}
MAX_NORM = 1.0


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """Initial parameters and the gradient of every step (float32, on the GPU; None: no gradient that step)."""
    case = CASES[name]
    gen = torch.Generator().manual_seed(sorted(CASES).index(name) + 1)
    sizes = [n for g in case["groups"] for n in g["sizes"]]
    params = [torch.randn(n, generator=gen).cuda() for n in sizes]
    grads = []
    for step in range(STEPS):
        row = [(case["s"] * torch.randn(n + 1, generator=gen)).cuda() for n in sizes]
        grads.append([None if (case.get("late") == i and step == 0) else
                      # (a view one float into its buffer: not 16-byte aligned)
                      g[1:] if case.get("unaligned") == i else g[:-1].clone() for i, g in enumerate(row)])
    return params, grads


def _param_groups(case, params):
    out, at = [], 0
    for g in case["groups"]:
        kw = {k: v for k, v in g.items() if k != "sizes"}
        out.append(dict(params=params[at:at + len(g["sizes"])], **kw))
        at += len(g["sizes"])
    return out


@functools.lru_cache(maxsize=None)
def _reference(name):
    """clip_grad_norm_ + torch.optim.Adam in float64 -> (p, exp_avg, exp_avg_sq, step) per parameter, norm per step."""
    case = CASES[name]
    p0, grads = _inputs(name)
    params = [torch.nn.Parameter(p.double()) for p in p0]
    opt = torch.optim.Adam(_param_groups(case, params), lr=1e-2)
    norms = []
    for row in grads:
        for p, g in zip(params, row):
            p.grad = None if g is None else g.double().clone()
        if not case.get("no_clip"):
            norms.append(float(torch.nn.utils.clip_grad_norm_(params, MAX_NORM)))
        opt.step()
    st = [opt.state[p] for p in params]
    return ([p.detach() for p in params], [s["exp_avg"] for s in st], [s["exp_avg_sq"] for s in st],
            [int(s["step"]) for s in st], norms)


def _run(name):
    """The same steps on this package's optimizer -> the same tuple in float32, and stats()."""
    import mrgcn_amd
    from mrgcn_amd.optim import Adam
    from mrgcn_amd.train import ClipAdam
    case = CASES[name]
    p0, grads = _inputs(name)
    params = [torch.nn.Parameter(p.clone()) for p in p0]
    groups = _param_groups(case, params)
    if case.get("no_clip"):
        opt = Adam(groups, lr=1e-2)
        assert opt.max_norm is None
    else:
        opt = ClipAdam(groups, lr=1e-2, max_norm=MAX_NORM, capturable=bool(case.get("capturable")))
    mrgcn_amd.reset_stats()
    norms = []
    for row in grads:
        for p, g in zip(params, row):
            p.grad = g    # (step() reads it: the unaligned view stays a view)
        opt.step()
        if not case.get("no_clip"):
            norms.append(opt.last_grad_norm())
    st = [opt.state[p] for p in params]
    sd = opt.state_dict()["state"]    # (keyed by the parameter's position, in the order the states were made)
    steps = [sd[k]["step"] for k in range(len(params))]
    return ([p.detach().clone() for p in params], [s["exp_avg"].clone() for s in st],
            [s["exp_avg_sq"].clone() for s in st], steps, norms), mrgcn_amd.stats()


def _scaled_err(a, ref):
    return float((a.double() - ref).abs().max() / ref.abs().max())


def _errors(name, det):
    """(p, exp_avg, exp_avg_sq, norm) errors against float64, worst over the case's tensors; under `det` the run is
    made twice and must repeat itself bit for bit."""
    ref = _reference(name)
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(det)
    try:
        got, st = _run(name)
        if det:
            again, _ = _run(name)
            for a, b in zip(got[:3], again[:3]):
                assert all(torch.equal(x, y) for x, y in zip(a, b)), f"{name}: two deterministic runs differ"
            assert got[4] == again[4], (got[4], again[4])
    finally:
        torch.use_deterministic_algorithms(prev)
    assert st.get("deterministic.sumsq", 0) == (STEPS if det else 0), st
    if not CASES[name].get("capturable"):   # (the device counter is the group's: state_dict() reports it for all)
        assert got[3] == ref[3], (got[3], ref[3])
    err = [max(_scaled_err(a, r) for a, r in zip(got[k], ref[k])) for k in range(3)]
    err.append(max([abs(a - r) / r for a, r in zip(got[4], ref[4])], default=0.0))
    assert len(got[4]) == len(ref[4])
    return err


@pytest.mark.parametrize("det", [False, True], ids=["plain", "deterministic"])
@pytest.mark.parametrize("name", list(CASES))
def test_step_against_float64_clip_and_adam(name, det):
    err = _errors(name, det)
    bound = list(BOUNDS)
    if name == "late_capturable":
        bound[0] = BOUND_LATE_CAPTURABLE_P
    print(f"{name} det={det}: p {err[0]:.3g} exp_avg {err[1]:.3g} exp_avg_sq {err[2]:.3g} norm {err[3]:.3g}")
    for k, e, b in zip(("p", "exp_avg", "exp_avg_sq", "norm"), err, bound):
        assert np.isfinite(e) and e <= b, (k, e, b)


# ---- a compact-rows node table next to a full closing launch ----------------------------------------------------
def _train_compact_with_extras(row_sparse, steps=4, N=2000, R=3):
    import mrgcn_amd
    from mrgcn_amd.models.rgcn import RGCN
    from mrgcn_amd.train import ClipAdam, train_step
    from tests.test_gpu_layers import _sparse_label_problem
    rows, cols, vals, idx, y = _sparse_label_problem(N, R, labelled=40)
    A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([rows, cols])), torch.from_numpy(vals), (N, R * N)).cuda()
    torch.manual_seed(0)
    # a featureless layer without bases: weight_I is the literal (R*N) x 16 operand, its gradient compact rows
    model = RGCN([(N, 16, "mrgcn", torch.nn.ReLU()), (16, 4, "mrgcn", None)], R, N, 0, 0.0, True, True, False).cuda()
    extras = [torch.nn.Parameter(torch.randn(4 + i, device="cuda")) for i in range(16)]
    wI = model.layers["layer_0"].weight_I
    # the node table and exactly 16 small dense gradients: the launch that closes the norm is full
    opt = ClipAdam([wI] + extras, lr=0.01, max_norm=1.0)
    ig, yg = torch.from_numpy(idx).cuda(), torch.from_numpy(y).cuda()

    def forward():   # (every extra enters the logits as a per-class offset)
        return model(None, A) + sum((i + 1) * e[:4] for i, e in enumerate(extras))
    mrgcn_amd.reset_stats()
    losses = []
    for _ in range(steps):
        losses.append(float(train_step(model, forward, ig, yg, opt, row_sparse=row_sparse)))
        for p in model.parameters():   # (the parameters this optimizer does not step: nothing accumulates)
            if p is not wI:
                p.grad = None
    tensors = [wI.detach().clone()] + [e.detach().clone() for e in extras]
    for p in [wI] + extras:
        tensors += [opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()]
    return tensors, losses + [opt.last_grad_norm()], mrgcn_amd.stats(), wI


def test_compact_rows_next_to_a_full_closing_launch():
    """16 small dense gradients fill the closing launch of the norm, so the compact gradient of the literal operand
    takes an accumulate call of its own: same parameters, moments, losses and norm as with `row_sparse=False`, at the
    tolerance tests/test_gpu_layers.py compares the two routes at."""
    dense, ld, st_d, _ = _train_compact_with_extras(False)
    assert "adam.index_rows" not in st_d, st_d
    sparse, ls, st, wI = _train_compact_with_extras(None)
    assert st.get("weight_I.index_rows") == 4 and st.get("adam.index_rows") == 4, st
    assert wI.grad is None and wI._mrgcn_rows["kind"] == "index"
    np.testing.assert_allclose(ls, ld, rtol=1e-6, atol=1e-7)
    for a, b in zip(sparse, dense):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-7)
