"""The grouped DistMult loss (csrc/distmult_group.hip; mrgcn_amd.tasks.link_prediction.group_loss, check_groups)
without a GPU: the entry points are declared, bound and exported; the float64 numpy restatement of the grouped maths —
what tests/test_gpu_lp_grouped.py holds the kernels to — equals torch's float64 CPU autograd over the flat triples; the
layout contract and the run loops' keyword checks answer before any kernel is touched.  Every seed is fixed."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests.test_cpu_host import ROOT, header_functions
from tests.test_cpu_lp_negatives import N, R, SEED, fixture64, flag_case

NAMES = ("mrgcn_distmult_group_supported", "mrgcn_distmult_group_fwd_workspace", "mrgcn_distmult_group_fwd_f32",
         "mrgcn_distmult_group_bwd_workspace", "mrgcn_distmult_group_bwd_f32")


# ---- the restatement -------------------------------------------------------------------------------------------------
def grouped_reference(triples, n, rate, E, Rel, loss="bce", w=1.0):
    """The grouped maths in float64, group by group: (loss, dE, dRel, scores).  A negative is head-corrupted when its
    column 0 differs from the fact's subject, tail-corrupted otherwise; scores[0:n] the facts', scores[n + i rate + j]
    negative j's of fact i."""
    t = np.asarray(triples, dtype=np.int64)
    E, Rel = np.asarray(E, dtype=np.float64), np.asarray(Rel, dtype=np.float64)
    assert t.shape == (n * (1 + rate), 3)
    dE, dR = np.zeros_like(E), np.zeros_like(Rel)
    scores = np.zeros(len(t))
    total, count = 0.0, (n * (1 + rate) if loss == "bce" else n)
    for i in range(n):
        si, pi, oi = t[i]
        s, p, o = E[si], Rel[pi], E[oi]
        neg = t[n + i * rate: n + (i + 1) * rate]
        head = neg[:, 0] != si
        c_id = np.where(head, neg[:, 0], neg[:, 2])
        c = E[c_id]
        x = np.empty(1 + rate)
        x[0] = ((s * p) * o).sum()
        x[1:] = np.where(head, ((c * p) * o).sum(1), ((s * p) * c).sum(1))
        scores[i], scores[n + i * rate: n + (i + 1) * rate] = x[0], x[1:]
        if loss == "bce":
            y = np.zeros(1 + rate)
            y[0] = 1.0
            k = 1.0 + (w - 1.0) * y
            total += ((1.0 - y) * x + k * (np.log1p(np.exp(-np.abs(x))) + np.maximum(-x, 0.0))).sum()
            g = (k / (1.0 + np.exp(-x)) - w * y) / count
        else:
            m = x.max()
            lse = m + np.log(np.exp(x - m).sum())
            total += lse - x[0]
            g = np.exp(x - lse)
            g[0] -= 1.0
            g /= count
        gj = g[1:, None]
        A = g[0] * o + (gj * c)[~head].sum(0)
        Hd = (gj * c)[head].sum(0)
        dE[si] += p * A
        dE[oi] += p * (g[0] * s + Hd)
        dR[pi] += s * A + o * Hd
        np.add.at(dE, c_id, gj * np.where(head[:, None], p * o, s * p))
    return total / count, dE, dR, scores


def flat_autograd(triples, n, rate, E, Rel, loss="bce", w=None):
    """torch's float64 CPU autograd over the flat triples: BCEWithLogitsLoss(pos_weight=) / cross_entropy."""
    t = torch.as_tensor(np.asarray(triples, dtype=np.int64))
    Et = torch.tensor(np.asarray(E, dtype=np.float64), requires_grad=True)
    Rt = torch.tensor(np.asarray(Rel, dtype=np.float64), requires_grad=True)
    x = (Et[t[:, 0]] * Rt[t[:, 1]] * Et[t[:, 2]]).sum(1)
    if loss == "bce":
        y = torch.zeros_like(x)
        y[:n] = 1
        pw = None if w is None else torch.tensor(float(w), dtype=torch.float64)
        out = torch.nn.BCEWithLogitsLoss(pos_weight=pw)(x, y)
    else:
        mat = torch.cat([x[:n, None], x[n:].view(n, rate)], 1)
        out = torch.nn.functional.cross_entropy(mat, torch.zeros(n, dtype=torch.int64))
    out.backward()
    return float(out.detach()), Et.grad.numpy(), Rt.grad.numpy(), x.detach().numpy()


def embeddings(num_nodes, num_relations, H, seed=0):
    """E, Rel ~ 0.5 N(0, 1): scores of standard deviation about 1.8, not saturated."""
    rng = np.random.default_rng(1000 + seed)
    return ((0.5 * rng.standard_normal((num_nodes, H))).astype(np.float32),
            (0.5 * rng.standard_normal((num_relations, H))).astype(np.float32))


def draw64(rate, side=0, position=0):
    from mrgcn_amd import host
    fx = fixture64()
    neg, _ = host.negatives_draw(fx["facts"], rate, N, N, R, fx["keys"], SEED, position, side=side)
    return np.concatenate([fx["facts"], neg]), len(fx["facts"])


def draw_flag_case():
    """8 nodes, 1 relation, rate 4, seed 99: no tail corruption can be accepted, so some negatives equal their fact."""
    from mrgcn_amd import host
    facts = flag_case()
    neg, unresolved = host.negatives_draw(facts, 4, 8, 8, 1, host.fact_keys(facts, 8, 1), 99, 0)
    return np.concatenate([facts, neg]), len(facts), unresolved


# ---- 1. declaration and binding --------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported_and_the_abi_version_stays():
    from mrgcn_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        assert name in header_functions(), f"{name} is not declared in include/mrgcn_hip.h"
        assert name in _lib.SIGNATURES, f"{name} is not in the ctypes table"
        assert hasattr(lib, name)
    res, args = _lib.SIGNATURES["mrgcn_distmult_group_fwd_f32"]
    assert res is C.c_int and len(args) == 16 and args.count(C.c_float) == 1
    res, args = _lib.SIGNATURES["mrgcn_distmult_group_bwd_f32"]
    assert res is C.c_int and len(args) == 21
    src = open(os.path.join(ROOT, "include", "mrgcn_hip.h")).read()
    assert re.search(r"#define\s+MRGCN_ABI_VERSION\s+5\b", src) and lib.mrgcn_abi_version() == 5 == _lib.ABI_VERSION
    assert re.search(r"#define\s+MRGCN_GROUP_LOSS_BCE\s+0\b", src) and re.search(r"#define\s+MRGCN_GROUP_LOSS_SOFTMAX\s+1\b", src)
    from mrgcn_amd.tasks import link_prediction as lp
    assert lp.GROUP_LOSSES == {"bce": 0, "softmax": 1}
    text = open(os.path.join(ROOT, "mrgcn_amd", "csrc", "distmult_group.hip")).read()
    assert "link_prediction.py:645-665" in text and ":550-554" in text
    # the size answers need no device
    assert lib.mrgcn_distmult_group_fwd_workspace() > 0
    assert lib.mrgcn_distmult_group_bwd_workspace(0, 1, 8) == -1 and lib.mrgcn_distmult_group_bwd_workspace(5, 0, 8) == -1
    assert lib.mrgcn_distmult_group_bwd_workspace(2500, 3, 200) >= 3 * 2500 * 200 * 4 + 4 * 7500 * 4
    assert lib.mrgcn_distmult_group_bwd_workspace(1 << 28, 8, 200) == -1      # n rate >= 2^31


# ---- 2. the restatement equals torch's float64 autograd over the flat triples -------------------------------------------
def _compare(t, n, rate, E, Rel):
    for loss, w in (("bce", None), ("bce", 1.0), ("bce", float(rate)), ("softmax", None)):
        got = grouped_reference(t, n, rate, E, Rel, loss, 1.0 if w is None else w)
        want = flat_autograd(t, n, rate, E, Rel, loss, w)
        for a, b, what in zip(got, want, ("loss", "dE", "dRel", "scores")):
            err = float(np.max(np.abs(np.asarray(a) - np.asarray(b))))
            print(f"rate {rate} {loss} w {w} {what}: max |diff| {err:.3e}")
            assert err <= 1e-12, (loss, w, what, err)


@pytest.mark.parametrize("rate", [1, 3, 10, 22])
def test_restatement_equals_flat_autograd_on_fixture64(rate):
    t, n = draw64(rate)
    E, Rel = embeddings(N, R, 12, rate)
    _compare(t, n, rate, E, Rel)


def test_restatement_equals_flat_autograd_on_the_flag_case():
    t, n, unresolved = draw_flag_case()
    same = int((t[n:] == np.repeat(t[:n], 4, axis=0)).all(1).sum())
    print("negatives equal to their fact:", same, "of", len(t) - n, "unresolved", int(unresolved.sum()))
    assert same >= 1 and len(t) - n == 32
    E, Rel = embeddings(8, 1, 8, 7)
    _compare(t, n, 4, E, Rel)


# ---- 3. the layout contract and the keyword checks -------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [1, 3, 10, 22])
def test_check_groups_accepts_the_draws(rate):
    from mrgcn_amd.tasks import link_prediction as lp
    t, n = draw64(rate)
    lp.check_groups(torch.from_numpy(t), n, rate)
    tf, nf, _ = draw_flag_case()
    lp.check_groups(torch.from_numpy(tf), nf, 4)


def test_check_groups_names_the_first_offending_row():
    from mrgcn_amd._lib import MrgcnError
    from mrgcn_amd.tasks import link_prediction as lp
    t, n = draw64(3)
    bad = t.copy()
    row = n + 3 * 5 + 1                       # negative 1 of fact 5
    bad[row, 1] = (bad[row, 1] + 1) % R
    bad[row + 4, 1] = (bad[row + 4, 1] + 1) % R
    with pytest.raises(MrgcnError, match=rf"row {row} \(negative 1 of fact 5\).*predicate"):
        lp.check_groups(torch.from_numpy(bad), n, 3)
    bad = t.copy()
    row = n + 3 * 100 + 2
    bad[row, 0], bad[row, 2] = (t[100, 0] + 1) % N, (t[100, 2] + 1) % N
    with pytest.raises(MrgcnError, match=rf"row {row} \(negative 2 of fact 100\).*neither end"):
        lp.check_groups(torch.from_numpy(bad), n, 3)
    with pytest.raises(MrgcnError, match="rows"):
        lp.check_groups(torch.from_numpy(t[:-1]), n, 3)
    with pytest.raises(MrgcnError, match="rows"):
        lp.check_groups(torch.from_numpy(t), n, 2)
    with pytest.raises(MrgcnError):
        lp.check_groups(torch.from_numpy(t).int(), n, 3)
    # a negative whose new end equals the fact's other end is a group member like any other
    ok = t.copy()
    ok[n, 0], ok[n, 2] = t[0, 0], t[0, 0]
    lp.check_groups(torch.from_numpy(ok), n, 3)


def test_keyword_errors_come_before_any_kernel():
    """None stands for every model, batch and optimizer: the checks answer before anything is touched."""
    from mrgcn_amd._lib import MrgcnError
    from mrgcn_amd.tasks import link_prediction as lp

    def not_a_sampler():
        raise AssertionError("the sampler was called")
    smp = not_a_sampler

    def train_step(**kw):
        return lp.train_step(None, None, smp, None, **kw)

    def train_batch_step(**kw):
        return lp.train_batch_step(None, None, None, None, sampler=smp, **kw)

    def train_epoch(**kw):
        return lp.train_epoch([(None, None)], None, None, samplers=[smp], **kw)

    def fit_epochs(**kw):
        return lp.FitEpochs(None, None, None, None, None, sampler=smp, **kw)

    def fit(**kw):
        return next(lp.fit(None, None, None, None, None, 1, sampler=smp, **kw))

    def batch_fit_epochs(**kw):
        return lp.BatchFitEpochs(None, [], None, None, **kw)

    def fit_batches(**kw):
        return next(lp.fit_batches(None, [], None, None, 1, **kw))
    calls = {f.__name__: f for f in (train_step, train_batch_step, train_epoch, fit_epochs, fit, batch_fit_epochs,
                                     fit_batches)}
    for who, call in calls.items():
        with pytest.raises(MrgcnError, match="decoder"):
            call(decoder="flat")
        with pytest.raises(MrgcnError, match="grouped"):
            call(loss="softmax")                          # the flat decoder has the plain BCE only
        with pytest.raises(MrgcnError, match="grouped"):
            call(pos_weight=3.0)
        with pytest.raises(MrgcnError, match="loss"):
            call(decoder="grouped", loss="hinge")
        with pytest.raises(MrgcnError, match="pos_weight"):
            call(decoder="grouped", loss="softmax", pos_weight=2.0)
        with pytest.raises(MrgcnError, match="pos_weight"):
            call(decoder="grouped", pos_weight=-1.0)
        with pytest.raises(MrgcnError, match="NegativeSampler"):
            call(decoder="grouped")                       # not a NegativeSampler (the batch loops: no samplers)
    with pytest.raises(MrgcnError, match="loss"):
        lp.group_loss(None, None, None, 1, 1, loss="hinge")
    with pytest.raises(MrgcnError, match="pos_weight"):
        lp.group_loss(None, None, None, 1, 1, loss="softmax", pos_weight=torch.tensor([2.0]))
