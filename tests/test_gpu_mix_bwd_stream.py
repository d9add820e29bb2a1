"""The norm-only mix backward on a gradient support as a one-shot grid (csrc/support.hip: k_mix_bwd_stream,
`sup_mix_stream=1`) against float64 numpy and against the resident kernel (k_mix_bwd_sup, `sup_mix_stream=0`):
dcomp and D bit for bit, ||dV||^2 to rounding (its parts are grouped differently), nothing read outside the support,
nothing written behind the reported workspace; then whole epochs under either value of the switch."""
import functools

import numpy as np
import pytest
import torch

from tests.test_gpu_plan_spmm import _plan_from_coo, _random_graph
from tests.test_gpu_support import _cases, _epoch_runs

pytestmark = pytest.mark.gpu

GUARD = 1024            # floats behind the reported workspace size
PATTERN = 0x5A5A5A5A


def _keep_live_nodes(rows, cols, vals, flags, N, keep):
    """drops, among the entries of flagged rows, those of all but the first `keep` source nodes they touch: the
    support then has exactly `keep` live nodes"""
    live = flags[rows] != 0
    nodes = np.unique(cols[live] % N)
    assert len(nodes) >= keep
    ok = ~live | np.isin(cols % N, nodes[:keep])
    return rows[ok], cols[ok], vals[ok]


def _with_column_counts(rng, rows, cols, vals, flags, N, R, counts):
    """gives one node per entry of `counts` exactly that many live columns (relations 0 .. count - 1, read by one
    flagged row)"""
    row = int(np.nonzero(flags)[0][0])
    nodes = rng.choice(N, len(counts), replace=False)
    ok = ~np.isin(cols % N, nodes)
    rows, cols, vals = rows[ok], cols[ok], vals[ok]
    add_c = np.concatenate([np.arange(c) * N + j for c, j in zip(counts, nodes)]).astype(cols.dtype)
    add_r = np.full(len(add_c), row, dtype=rows.dtype)
    add_v = rng.standard_normal(len(add_c)).astype(np.float32)
    return np.concatenate([rows, add_r]), np.concatenate([cols, add_c]), np.concatenate([vals, add_v])


GRAPHS = {
    # name: (seed, N, R, nnz, hubs, labelled, exact live nodes or None, forced column counts or None)
    "hubs13": (5, 2500, 13, 30000, 2, 300, None, (1, 4, 5, 8, 13)),
    "rel3": (6, 900, 3, 4000, 1, 200, None, None),
    "nl1": (7, 300, 7, 2500, 0, 12, 1, None),
    "nl3": (8, 300, 7, 2500, 0, 12, 3, None),
    "nl256": (9, 1500, 11, 20000, 0, 60, 256, None),   # a multiple of four waves x two entries
    "nl257": (9, 1500, 11, 20000, 0, 60, 257, None),   # one more: a wave and a block tail
}


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
    lnode = sup.export(L.SUP_LNODE).astype(np.int64)
    nlptr = sup.export(L.SUP_NLPTR).astype(np.int64)
    lrel = sup.export(L.SUP_LREL).astype(np.int64)
    ncols = np.diff(nlptr)
    assert sup.NL == len(lnode) and sup.L == len(lrel) and np.array_equal(np.nonzero(ncols)[0], lnode)
    if keep is not None:
        assert sup.NL == keep
    if counts is not None:
        assert set(counts) <= set(ncols.tolist())
    if R == 3:
        assert ncols.max() <= 3
    return dict(plan=plan, sup=sup, N=N, R=R, lnode=lnode, nlptr=nlptr, lrel=lrel,
                node_of=np.repeat(np.arange(N), ncols))


@functools.lru_cache(maxsize=None)
def _inputs(name, B, F):
    """inputs (NaN wherever the pass must not read) and the float64 reference, made once per (graph, shape)"""
    p = _problem(name)
    N, R, Lc = p["N"], p["R"], len(p["lrel"])
    rng = np.random.default_rng(1000 * B + F)
    ld = (F + 3) // 4 * 4 + 4
    V = rng.standard_normal((N, B, F)).astype(np.float32)
    comp = rng.standard_normal((R, B)).astype(np.float32)
    dM = rng.standard_normal((Lc, F)).astype(np.float32)
    Vp = V.copy()
    dead = np.ones(N, dtype=bool)
    dead[p["lnode"]] = False
    Vp[dead] = np.nan
    dMp = np.full((Lc, ld), np.nan, dtype=np.float32)
    dMp[:, :F] = dM
    terms = dM.astype(np.float64)[:, None, :] * V.astype(np.float64)[p["node_of"]]          # [L, B, F]
    dcomp, bound = np.zeros((R, B)), np.zeros((R, B))
    for r in range(R):
        t = terms[p["lrel"] == r]
        dcomp[r] = t.sum(axis=(0, 2))
        bound[r] = 4.0 * (t.shape[0] * F) * 2.0 ** -24 * np.abs(t).sum(axis=(0, 2))
    dV = np.zeros((N, B, F))
    np.add.at(dV, p["node_of"], comp.astype(np.float64)[p["lrel"]][:, :, None] * dM.astype(np.float64)[:, None, :])
    return dict(V=torch.from_numpy(Vp).cuda(), comp=torch.from_numpy(comp).cuda(), dM=torch.from_numpy(dMp).cuda(),
                ld=ld, dcomp=dcomp, bound=bound, sumsq=float((dV * dV).sum()))


def _run(name, B, F, stream):
    """one call of the norm-only pass under `sup_mix_stream` = stream -> (dcomp, D, ||dV||^2) as numpy"""
    from mrgcn_amd import _lib as L
    lib = L.load()
    p, x = _problem(name), _inputs(name, B, F)
    sup = p["sup"]
    n = int(lib.mrgcn_support_mix_bwd_workspace(sup.handle, B))
    ws = torch.full((n + GUARD,), PATTERN, dtype=torch.int32, device="cuda")
    dcomp = torch.full((p["R"], B), float("nan"), device="cuda")
    sq = torch.full((), float("nan"), dtype=torch.float64, device="cuda")
    old = L.set_config(sup_mix_stream=stream)
    try:
        L.check(lib.mrgcn_support_mix_bwd_f32(sup.handle, x["dM"].data_ptr(), x["ld"], x["V"].data_ptr(),
                                              x["comp"].data_ptr(), B, F, 0, 0, dcomp.data_ptr(), sq.data_ptr(),
                                              ws.data_ptr(), n, torch.cuda.current_stream().cuda_stream),
                "mrgcn_support_mix_bwd_f32")
        torch.cuda.synchronize()
    finally:
        L.set_config(**old)
    assert bool((ws[n:] == PATTERN).all()), "written behind the reported workspace size"
    D = ws[: sup.L * B].view(torch.float32).cpu().numpy().copy()
    return dcomp.cpu().numpy(), D, float(sq)


def _check(name, B, F):
    x = _inputs(name, B, F)
    new1 = _run(name, B, F, 1)
    new2 = _run(name, B, F, 1)
    old = _run(name, B, F, 0)
    for tag, (dcomp, D, sq) in (("one-shot", new1), ("resident", old)):
        assert np.isfinite(dcomp).all() and np.isfinite(D).all() and np.isfinite(sq), tag
        err = np.abs(dcomp - x["dcomp"])
        print(f"{name} B={B} F={F} {tag}: max dcomp err / bound {float((err / np.maximum(x['bound'], 1e-300)).max()):.3g}, "
              f"sumsq rel err {abs(sq - x['sumsq']) / max(x['sumsq'], 1e-300):.3g}")
        assert (err <= x["bound"]).all(), (tag, float((err - x["bound"]).max()))
        assert abs(sq - x["sumsq"]) <= 1e-5 * x["sumsq"], (tag, sq, x["sumsq"])
    # the forms against each other: the same fmaf chains
    assert np.array_equal(new1[0].view(np.int32), old[0].view(np.int32)), "dcomp differs between the forms"
    assert np.array_equal(new1[1].view(np.int32), old[1].view(np.int32)), "D differs between the forms"
    assert abs(new1[2] - old[2]) <= 1e-6 * abs(old[2])
    # two calls of the new form: the same bits
    assert np.array_equal(new1[0].view(np.int32), new2[0].view(np.int32)) and new1[2] == new2[2]
    assert np.array_equal(new1[1].view(np.int32), new2[1].view(np.int32))


# (40, 10): two pieces per lane, the second half partly filled; (30, 16): 120 pieces; (10, 16): fewer pieces than
# lanes; (64, 16): four pieces per lane, the limit; (8, 4), (5, 4): a handful of pieces; (3, 10): B F no multiple of 4
# and (40, 11): odd F — both keep the resident kernel under either value; (16, 6): a padded feature count
@pytest.mark.parametrize("B,F", [(40, 10), (30, 16), (10, 16), (64, 16), (8, 4), (5, 4), (3, 10), (40, 11), (16, 6)])
def test_shapes_on_nodes_of_1_to_13_live_columns(B, F):
    _check("hubs13", B, F)


@pytest.mark.parametrize("B,F", [(40, 10), (8, 4)])
def test_never_more_than_three_live_columns(B, F):
    _check("rel3", B, F)


@pytest.mark.parametrize("name", ["nl1", "nl3", "nl256", "nl257"])
@pytest.mark.parametrize("B,F", [(40, 10), (10, 16)])
def test_wave_and_block_tails(name, B, F):
    _check(name, B, F)


def _epochs_under(case_name, stream):
    from mrgcn_amd import _lib as L
    old = L.set_config(sup_mix_stream=stream)
    try:
        return _epoch_runs(case_name, True, steps=3)
    finally:
        L.set_config(**old)


@pytest.mark.parametrize("case_name", _cases())
def test_epochs_under_either_form(case_name):
    l1, p1 = _epochs_under(case_name, 1)
    l0, p0 = _epochs_under(case_name, 0)
    np.testing.assert_allclose(l1, l0, rtol=1e-5, atol=1e-6)
    for k in p0:
        diff = np.abs(p1[k] - p0[k])
        assert (diff > 2e-5).mean() <= 2e-3, (k, float(diff.max()))


def test_captured_epoch_replays_the_one_shot_form():
    """GraphedTrainStep under `sup_mix_stream=1`: one warm-up step and two replays against three eager steps"""
    from mrgcn_amd import _lib as L
    from mrgcn_amd.train import ClipAdam, GraphedTrainStep, train_step
    from tests import util
    from tests.test_gpu_layers import _adjacency
    name = "rgcn_smoke_ft_b5_norm_f32"
    c = util.load_case(name)
    A = _adjacency(c, name)
    X = torch.from_numpy(c["X"]).cuda()
    idx = torch.from_numpy(c["labels_idx"]).cuda()
    tgt = torch.from_numpy(c["labels_y"]).cuda()
    old = L.set_config(sup_mix_stream=1)
    try:
        states, losses = [], []
        for graphed in (False, True):
            model, _ = util.build_rgcn_from_case(c, "cuda")
            util.load_state_from_case(model, c)
            model = model.cuda()
            opt = ClipAdam(list(model.parameters()), lr=0.01, max_norm=1.0, capturable=graphed)
            if graphed:
                step = GraphedTrainStep(model, lambda: model(X, A), idx, tgt, opt, warmup=1)
                for _ in range(2):
                    loss = step()
            else:
                for _ in range(3):
                    loss = train_step(model, lambda: model(X, A), idx, tgt, opt)
            torch.cuda.synchronize()
            states.append({k: v.clone() for k, v in model.state_dict().items()})
            losses.append(float(loss))
    finally:
        L.set_config(**old)
    assert abs(losses[0] - losses[1]) <= 1e-5 * max(1.0, abs(losses[0]))
    for k in states[0]:
        torch.testing.assert_close(states[0][k], states[1][k], rtol=1e-5, atol=1e-6, msg=k)
