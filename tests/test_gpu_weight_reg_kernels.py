"""The two kernels of the regularised node-table step (csrc/adam_reg.hip) through the C ABI against float64 numpy:
the penalty-norm pass (sum (g + r(p))^2, sum |p|, sum p^2) and the row Adam over all N nodes with
gg = (g + r(p)) scale + wd p.  Nothing read from dM's padding, nothing written behind the arrays or the reported
workspace, unsupported shapes refused without a write."""
import functools
import itertools

import numpy as np
import pytest
import torch

from tests.test_gpu_mix_bwd_stream import _keep_live_nodes, _with_column_counts
from tests.test_gpu_plan_spmm import _plan_from_coo, _random_graph

pytestmark = pytest.mark.gpu

GUARD = 1024            # elements behind every array and behind the reported workspace size
PATTERN = 0x5A5A5A5A
ERR_UNSUPPORTED = 3

GRAPHS = {
    # name: (seed, N, R, nnz, hubs, labelled, exact live nodes or None, forced column counts or None)
    "hubs13": (5, 2500, 13, 30000, 2, 300, None, (1, 4, 5, 8, 13)),
    "nl1": (7, 300, 7, 2500, 0, 12, 1, None),                          # nearly every node is outside the support
    "n2501": (5, 2501, 13, 30000, 2, 300, None, (1, 4, 5, 8, 13)),     # a block tail and a nodes-per-wave tail
}
# (40, 10): 100 pieces, the second half-wave partly filled; (16, 16): exactly 64; (32, 16): 128, the limit
SHAPES = [(40, 10), (16, 16), (32, 16), (10, 16), (5, 4)]
LR, B1, B2, EPS = (np.float32(x) for x in (0.01, 0.9, 0.999, 1e-8))
STEP = 3
SCALE = np.float32(0.37)
SETTINGS = [(5e-4, 0.0, 0.0), (0.0, 1e-4, 1e-3), (1e-2, 1e-4, 1e-3), (0.0, 1e-3, 0.0)]   # (wd, l1, l2)


@functools.lru_cache(maxsize=None)
def _problem(name):
    from mrgcn_amd import _lib as L
    seed, N, R, nnz, hubs, labelled, keep, counts = GRAPHS[name]
    rng = np.random.default_rng(seed)
    rows, cols, vals = _random_graph(rng, N, N, R, nnz, hub_rows=hubs, hub_len=min(1500, N), hub_cols=hubs)
    flags = np.zeros(N, dtype=np.uint8)
    flags[rng.choice(N, labelled, replace=False)] = 1
    if keep is not None:
        rows, cols, vals = _keep_live_nodes(rows, cols, vals, flags, N, keep)
    if counts is not None:
        rows, cols, vals = _with_column_counts(rng, rows, cols, vals, flags, N, R, counts)
    plan = _plan_from_coo(rows, cols, vals, N, N, R)
    sup = plan.support_for(torch.from_numpy(flags).cuda())
    nlptr = sup.export(L.SUP_NLPTR).astype(np.int64)
    lrel = sup.export(L.SUP_LREL).astype(np.int64)
    ncols = np.diff(nlptr)
    assert len(nlptr) == N + 1 and sup.L == len(lrel)
    if keep is not None:
        assert sup.NL == keep
    if counts is not None:
        assert set(counts) <= set(ncols.tolist())
    return dict(plan=plan, sup=sup, N=N, R=R, lrel=lrel, ncols=ncols, node_of=np.repeat(np.arange(N), ncols))


def _guarded(a, dtype=torch.float32):
    """`a` on the device with GUARD pattern words behind it -> (whole tensor, view of the array)"""
    n = a.size
    t = torch.full((n + GUARD,), PATTERN, dtype=torch.int32, device="cuda").view(dtype)
    t[:n] = torch.from_numpy(a.reshape(-1)).cuda()
    return t, n


@functools.lru_cache(maxsize=None)
def _inputs(name, B, F):
    """host inputs and the float64 gradient, made once per (graph, shape)"""
    q = _problem(name)
    N, R, Lc = q["N"], q["R"], len(q["lrel"])
    rng = np.random.default_rng(1000 * B + F)
    ld = (F + 3) // 4 * 4 + 4
    p = rng.standard_normal((N, B, F)).astype(np.float32)
    z = rng.random((N, B, F))
    p[z < 0.025] = 0.0           # about 5 % exact zeros, of both signs
    p[z > 0.975] = -0.0
    m = (0.1 * rng.standard_normal((N, B, F))).astype(np.float32)
    v = rng.uniform(1e-2, 1.0, (N, B, F)).astype(np.float32)
    band = slice(N // 3, N // 3 + 40)   # nodes that never held moments
    m[band] = 0.0
    v[band] = 0.0
    dead = np.nonzero(q["ncols"] == 0)[0]
    still = dead[:: max(len(dead) // 7, 1)][:7]   # nodes outside the support with p = m = v = 0: nothing may move
    p[still] = 0.0
    m[still] = 0.0
    v[still] = 0.0
    comp = rng.standard_normal((R, B)).astype(np.float32)
    dM = rng.standard_normal((Lc, F)).astype(np.float32)
    dMp = np.full((Lc, ld), np.nan, dtype=np.float32)
    dMp[:, :F] = dM
    g = np.zeros((N, B, F))
    np.add.at(g, q["node_of"], comp.astype(np.float64)[q["lrel"]][:, :, None] * dM.astype(np.float64)[:, None, :])
    # Where m = v = 0 the update is lr' . 0.1 gg / (0.58 |gg| + eps): a step of fixed size whose direction turns over
    # within |gg| ~ 1e-7 of zero, where no fp32 chain (the existing kernel's included) says anything about a float64 one.
    # g alone never comes that close to zero, but g + r(p) + wd p does when the three terms cancel (first seen at
    # p = -1.29, g = 0.0156, wd = 1e-2, l1 = 1e-4, l2 = 1e-3: gg = 1.5e-7).  On the band's nodes p therefore takes the sign
    # of g, so that penalty and decay add to the gradient instead of cancelling it; nodes that hold moments
    # (v >= 1e-2) are well conditioned whatever the signs.
    sg = np.sign(g[band]).astype(np.float32)
    p[band] = np.where(sg != 0, np.abs(p[band]) * sg, p[band])
    return dict(p=p, m=m, v=v, still=still, comp=torch.from_numpy(comp).cuda(), dM=torch.from_numpy(dMp).cuda(), ld=ld,
                g=g)


def _penalty_grad(p64, l1, l2):
    l1, l2 = float(np.float32(l1)), float(np.float32(l2))
    return l1 * np.sign(p64) + 2.0 * l2 * p64


def _adam_ref(x, wd, l1, l2, scale):
    """the float64 restatement: gg = (g + r(p)) scale + wd p, then Adam's update at step STEP"""
    p, m, v = (x[k].astype(np.float64) for k in ("p", "m", "v"))
    lr, b1, b2, eps = (float(t) for t in (LR, B1, B2, EPS))
    sc = 1.0 if scale is None else float(scale)
    gg = (x["g"] + _penalty_grad(p, l1, l2)) * sc + float(np.float32(wd)) * p
    m1 = b1 * m + (1.0 - b1) * gg
    v1 = b2 * v + (1.0 - b2) * gg * gg
    bc1, bc2s = 1.0 - b1 ** STEP, np.sqrt(1.0 - b2 ** STEP)
    return p - (lr / bc1) * (m1 / (np.sqrt(v1) / bc2s + eps)), m1, v1


def _run_adam(name, B, F, entry, wd=0.0, l1=0.0, l2=0.0, scale=None, dev_step=False):
    """one call of `entry` ("reg": the new kernel; "fused": the existing one with every node flagged and
    ever_outside = 1) -> (p, m, v, row_ever) as numpy"""
    from mrgcn_amd import _lib as L
    lib = L.load()
    q, x = _problem(name), _inputs(name, B, F)
    sup = q["sup"]
    bufs = [_guarded(x[k]) for k in ("p", "m", "v")]
    ever = torch.full((q["N"] + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    ever[: q["N"]] = 1 if entry == "fused" else 0
    sc = torch.full((), float(scale), device="cuda") if scale is not None else None
    bc = None
    if dev_step:
        bc = torch.tensor([1.0 - float(B1) ** STEP, np.sqrt(1.0 - float(B2) ** STEP)], dtype=torch.float32,
                          device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    head = (sup.handle, x["dM"].data_ptr(), x["ld"], x["comp"].data_ptr(), B, F, bufs[0][0].data_ptr(),
            bufs[1][0].data_ptr(), bufs[2][0].data_ptr(), ever.data_ptr(), float(LR), float(B1), float(B2), float(EPS))
    tail = (0 if dev_step else STEP, bc.data_ptr() if dev_step else 0, sc.data_ptr() if sc is not None else 0)
    if entry == "reg":
        L.check(lib.mrgcn_support_adam_rows_reg_f32(*head, float(wd), float(l1), float(l2), *tail, s),
                "mrgcn_support_adam_rows_reg_f32")
    else:
        L.check(lib.mrgcn_support_adam_rows_fused_f32(*head, *tail, 1, s), "mrgcn_support_adam_rows_fused_f32")
    torch.cuda.synchronize()
    out = []
    for t, n in bufs:
        assert bool((t[n:].view(torch.int32) == PATTERN).all()), "written behind p / m / v"
        out.append(t[:n].cpu().numpy().reshape(q["N"], B, F))
    assert bool((ever[q["N"]:] == 0x5A).all()), "written behind row_ever"
    return out[0], out[1], out[2], ever[: q["N"]].cpu().numpy()


def _scaled_err(got, ref):
    """largest error of an array in units of its largest value"""
    return float(np.abs(got.astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


def _check_norm(name, B, F):
    from mrgcn_amd import _lib as L
    lib = L.load()
    q, x = _problem(name), _inputs(name, B, F)
    sup = q["sup"]
    nbytes = int(lib.mrgcn_support_reg_norm_workspace(sup.handle, B, F))
    assert nbytes > 0 and nbytes % 8 == 0
    p_t, n = _guarded(x["p"])
    p64 = x["p"].astype(np.float64)
    for l1, l2 in ((1e-4, 1e-3), (1e-3, 0.0), (0.0, 5e-4)):
        outs = []
        for _ in range(2):
            ws = torch.full((nbytes // 4 + GUARD,), PATTERN, dtype=torch.int32, device="cuda")
            out3 = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
            L.check(lib.mrgcn_support_reg_norm_f32(sup.handle, x["dM"].data_ptr(), x["ld"], x["comp"].data_ptr(), B, F,
                                                   p_t.data_ptr(), float(l1), float(l2), out3.data_ptr(),
                                                   ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream),
                    "mrgcn_support_reg_norm_f32")
            torch.cuda.synchronize()
            assert bool((ws[nbytes // 4:] == PATTERN).all()), "written behind the reported workspace size"
            outs.append(out3.cpu().numpy())
        t = x["g"] + _penalty_grad(p64, l1, l2)
        ref = np.array([(t * t).sum(), np.abs(p64).sum(), (p64 * p64).sum()])
        rel = np.abs(outs[0] - ref) / ref
        print(f"{name} B={B} F={F} l1={l1} l2={l2}: rel err of sum (g+r)^2 {rel[0]:.3g}, sum|p| {rel[1]:.3g}, "
              f"sum p^2 {rel[2]:.3g}")
        assert np.isfinite(outs[0]).all()
        assert rel[0] <= 1e-5 and rel[1] <= 1e-9 and rel[2] <= 1e-9, rel
        assert np.array_equal(outs[0].view(np.int64), outs[1].view(np.int64)), "two calls differ"
    assert bool((p_t[n:].view(torch.int32) == PATTERN).all())


def _check_adam(name, B, F):
    """Bound of the non-zero settings: twice the largest error of the EXISTING entry point
    (mrgcn_support_adam_rows_fused_f32, lambdas zero) against the same float64 restatement on the same inputs and the
    same scale / step form — the new chain is the old one plus three operations per element.  Errors are in units of
    each array's largest value.  Measured on an MI355X, largest over the graphs, shapes and forms: the existing entry
    point p 5.6e-8, m 1.4e-7, v 6.2e-8 (so bounds of up to 1.1e-7, 2.8e-7, 1.2e-7, each case against its own); the new
    kernel p 5.7e-8, m 1.9e-7, v 8.2e-8; the largest ratio new / existing within one case 1.98 (p), 1.93 (m), 1.46 (v).
    The norm pass on the same inputs: sum (g + r)^2 off by 2.0e-8 relative at most, sum |p| by 2.4e-16, sum p^2 by
    5.8e-16."""
    x = _inputs(name, B, F)
    for scale, dev_step in itertools.product((None, SCALE), (False, True)):
        old = _run_adam(name, B, F, "fused", scale=scale, dev_step=dev_step)
        zero = _run_adam(name, B, F, "reg", scale=scale, dev_step=dev_step)
        for a, b, k in zip(old[:3], zero[:3], "pmv"):
            assert np.isfinite(b).all() and bool((a == b).all()), f"{k}: all-zero settings differ from the sibling kernel"
        assert bool((zero[3] == 1).all())
        ref0 = _adam_ref(x, 0.0, 0.0, 0.0, scale)
        base = [_scaled_err(a, r) for a, r in zip(old[:3], ref0)]
        for wd, l1, l2 in SETTINGS:
            got = _run_adam(name, B, F, "reg", wd, l1, l2, scale=scale, dev_step=dev_step)
            ref = _adam_ref(x, wd, l1, l2, scale)
            err = [_scaled_err(a, r) for a, r in zip(got[:3], ref)]
            w = np.unravel_index(np.abs(got[0] - ref[0]).argmax(), ref[0].shape)   # the element p is furthest off at
            print(f"{name} B={B} F={F} scale={scale} dev_step={dev_step} wd={wd} l1={l1} l2={l2}: "
                  f"existing p/m/v {base[0]:.3g} {base[1]:.3g} {base[2]:.3g}, new {err[0]:.3g} {err[1]:.3g} {err[2]:.3g}"
                  f" (worst p at {w}: p {x['p'][w]!r} m {x['m'][w]!r} v {x['v'][w]!r} g {x['g'][w]!r} -> "
                  f"{got[0][w]!r} / {ref[0][w]!r})")
            for k, e, b in zip("pmv", err, base):
                assert np.isfinite(e) and e <= 2.0 * b, (k, e, 2.0 * b)
            for a in got[:3]:   # outside the support with p = m = v = 0: exactly zero afterwards
                assert bool((a[x["still"]] == 0).all())
            assert bool((got[3] == 1).all()), "row_ever"


@pytest.mark.parametrize("B,F", SHAPES)
@pytest.mark.parametrize("name", list(GRAPHS))
def test_penalty_norm_pass(name, B, F):
    _check_norm(name, B, F)


@pytest.mark.parametrize("B,F", SHAPES)
@pytest.mark.parametrize("name", list(GRAPHS))
def test_regularised_row_adam(name, B, F):
    _check_adam(name, B, F)


@pytest.mark.parametrize("B,F", [(64, 16), (3, 10), (40, 11)])
def test_unsupported_shapes_are_refused_without_a_write(B, F):
    from mrgcn_amd import _lib as L
    lib = L.load()
    q = _problem("hubs13")
    sup, N = q["sup"], q["N"]
    assert lib.mrgcn_support_reg_norm_workspace(sup.handle, B, F) < 0
    n = N * B * F
    ld = (F + 3) // 4 * 4 + 4
    bufs = [torch.full((n,), PATTERN, dtype=torch.int32, device="cuda") for _ in range(3)]
    ever = torch.full((N,), 0x5A, dtype=torch.uint8, device="cuda")
    ws = torch.full((1 << 16,), PATTERN, dtype=torch.int32, device="cuda")
    out3 = torch.full((3,), PATTERN, dtype=torch.int32, device="cuda").repeat(2)
    dM = torch.zeros((sup.L, ld), device="cuda")
    comp = torch.zeros((q["R"], B), device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    rc = lib.mrgcn_support_reg_norm_f32(sup.handle, dM.data_ptr(), ld, comp.data_ptr(), B, F, bufs[0].data_ptr(), 1e-4,
                                        1e-3, out3.data_ptr(), ws.data_ptr(), ws.numel() * 4, s)
    assert rc == ERR_UNSUPPORTED
    rc = lib.mrgcn_support_adam_rows_reg_f32(sup.handle, dM.data_ptr(), ld, comp.data_ptr(), B, F, bufs[0].data_ptr(),
                                             bufs[1].data_ptr(), bufs[2].data_ptr(), ever.data_ptr(), 0.01, 0.9, 0.999,
                                             1e-8, 5e-4, 1e-4, 1e-3, 1, 0, 0, s)
    assert rc == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    for t in bufs + [ws, out3]:
        assert bool((t == PATTERN).all())
    assert bool((ever == 0x5A).all())
