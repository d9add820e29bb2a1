"""The ComplEx scorer without a GPU: the numpy mirror of the candidate scores (mrgcn_amd.host.complex_candidate_scores:
the float32 operations the rank and top-k kernels perform) against the independent complex128 formulation, the
antisymmetry DistMult lacks, the gradient formulas of csrc/complex.hip against torch's float64 complex autograd, the
new symbols at the C ABI, and the argument checks that raise before a kernel is touched."""
import ctypes as C

import numpy as np
import pytest
import torch

from mrgcn_amd import _lib, host
from mrgcn_amd.tasks import link_prediction as lp
from tests.test_cpu_host import header_functions

SHAPES = [(300, 5, 200), (300, 5, 130), (64, 7, 64), (64, 7, 6), (500, 9, 64)]
NAMES = ("mrgcn_complex_score_f32", "mrgcn_complex_bwd_workspace", "mrgcn_complex_score_bwd_f32",
         "mrgcn_complex_ranks_both_workspace", "mrgcn_complex_ranks_both", "mrgcn_complex_topk_workspace",
         "mrgcn_complex_topk")


def tables(N, R, H, seed=0, dtype=np.float32):
    rng = np.random.default_rng(seed)
    return (0.5 * rng.standard_normal((N, H))).astype(dtype), (0.5 * rng.standard_normal((R, H))).astype(dtype)


def triples(N, R, n, seed=1):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, N, n), rng.integers(0, R, n), rng.integers(0, N, n)], 1).astype(np.int64)


def complex_grads64(t, E, Rel, g):
    """dE, dRel of sum_i g[i] score(t[i]) by the formulas of include/mrgcn_hip.h, numpy float64."""
    E, Rel, g = np.asarray(E, np.float64), np.asarray(Rel, np.float64), np.asarray(g, np.float64)[:, None]
    K = E.shape[1] // 2
    s, r, o = E[t[:, 0]], Rel[t[:, 1]], E[t[:, 2]]
    sr, si, rr, ri, or_, oi = s[:, :K], s[:, K:], r[:, :K], r[:, K:], o[:, :K], o[:, K:]
    dE, dR = np.zeros_like(E), np.zeros_like(Rel)
    np.add.at(dE, t[:, 0], g * np.concatenate([rr * or_ + ri * oi, rr * oi - ri * or_], 1))
    np.add.at(dE, t[:, 2], g * np.concatenate([sr * rr - si * ri, si * rr + sr * ri], 1))
    np.add.at(dR, t[:, 1], g * np.concatenate([sr * or_ + si * oi, sr * oi - si * or_], 1))
    return dE, dR


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("side", ["tail", "head"])
def test_mirror_matches_complex128(shape, side):
    N, R, H = shape
    E, Rel = tables(N, R, H)
    t = triples(N, R, 40)
    anchors = t[:, 0] if side == "tail" else t[:, 2]
    got = host.complex_candidate_scores(E, Rel, anchors, t[:, 1], side)
    assert got.dtype == np.float32 and got.shape == (40, N)
    cand = np.tile(np.arange(N), 40)
    full = np.stack([np.repeat(t[:, 0], N), np.repeat(t[:, 1], N), np.repeat(t[:, 2], N)], 1)
    full[:, 2 if side == "tail" else 0] = cand
    want = host.complex_scores64(full, E, Rel).reshape(40, N)
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4)


def test_the_two_sides_round_differently():
    """Why the rank kernels keep the fact's own score per side: the tail-form and the head-form score of the same
    triple differ in their last bits for most facts."""
    N, R, H = 300, 5, 200
    E, Rel = tables(N, R, H)
    t = triples(N, R, 400)
    tail = host.complex_candidate_scores(E, Rel, t[:, 0], t[:, 1], "tail")[np.arange(400), t[:, 2]]
    head = host.complex_candidate_scores(E, Rel, t[:, 2], t[:, 1], "head")[np.arange(400), t[:, 0]]
    assert np.mean(tail != head) > 0.5
    np.testing.assert_allclose(tail, head, rtol=1e-4, atol=1e-4)


def test_complex_is_antisymmetric_where_distmult_is_not():
    N, R, H = 64, 7, 64
    E, Rel = tables(N, R, H)
    t = triples(N, R, 200)
    t = t[t[:, 0] != t[:, 2]]
    fwd = host.complex_candidate_scores(E, Rel, t[:, 0], t[:, 1], "tail")[np.arange(len(t)), t[:, 2]]
    rev = host.complex_candidate_scores(E, Rel, t[:, 2], t[:, 1], "tail")[np.arange(len(t)), t[:, 0]]
    assert np.all(np.abs(fwd - rev) > 1e-3 * np.maximum(np.abs(fwd), np.abs(rev)))
    E64, R64 = E.astype(np.float64), Rel.astype(np.float64)
    dm_fwd = (E64[t[:, 0]] * R64[t[:, 1]] * E64[t[:, 2]]).sum(1)
    dm_rev = (E64[t[:, 2]] * R64[t[:, 1]] * E64[t[:, 0]]).sum(1)
    np.testing.assert_allclose(dm_fwd, dm_rev, rtol=1e-14, atol=0)


@pytest.mark.parametrize("shape", [(64, 7, 64), (64, 7, 6)])
def test_gradient_formulas_match_complex_autograd(shape):
    N, R, H = shape
    K = H // 2
    E, Rel = tables(N, R, H, dtype=np.float64)
    t = triples(N, R, 300)
    t[:20, 2] = t[:20, 0]            # s == o: both contributions into one row
    t[20:40] = t[40:60]              # repeated triples
    g = np.random.default_rng(3).standard_normal(len(t))
    Et, Rt = torch.from_numpy(E).requires_grad_(), torch.from_numpy(Rel).requires_grad_()
    Ec, Rc = torch.complex(Et[:, :K], Et[:, K:]), torch.complex(Rt[:, :K], Rt[:, K:])
    tt = torch.from_numpy(t)
    sc = (Ec[tt[:, 0]] * Rc[tt[:, 1]] * Ec[tt[:, 2]].conj()).sum(1).real
    np.testing.assert_allclose(sc.detach().numpy(), host.complex_scores64(t, E, Rel), rtol=1e-13, atol=1e-13)
    (sc * torch.from_numpy(g)).sum().backward()
    dE, dR = complex_grads64(t, E, Rel, g)
    np.testing.assert_allclose(dE, Et.grad.numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(dR, Rt.grad.numpy(), rtol=1e-12, atol=1e-13)


def test_symbols_are_in_header_ctypes_table_and_library():
    declared = set(header_functions())
    lib = _lib.load()
    for n in NAMES:
        assert n in declared, f"{n} is not declared in include/mrgcn_hip.h"
        assert n in _lib.SIGNATURES, f"{n} is not in the ctypes table"
        assert hasattr(lib, n), f"{n} is not exported by the library"
    for n in NAMES:
        twin = {"mrgcn_complex_bwd_workspace": "mrgcn_distmult_bwd_det_workspace",
                "mrgcn_complex_score_bwd_f32": "mrgcn_distmult_score_bwd_det_f32"}.get(n, n.replace("complex", "distmult"))
        assert _lib.SIGNATURES[n] == _lib.SIGNATURES[twin], f"{n} and {twin} differ in signature"
    assert _lib.SIGNATURES["mrgcn_complex_bwd_workspace"][0] is C.c_int64
    # the workspace queries need no device: an odd width has no ComplEx reading
    assert lib.mrgcn_complex_bwd_workspace(100, 7) == -1 and lib.mrgcn_complex_bwd_workspace(100, 8) > 0
    assert lib.mrgcn_complex_topk_workspace(64, 7, 10, 5) == -1
    assert lib.mrgcn_complex_topk_workspace(64, 8, 10, 5) == lib.mrgcn_distmult_topk_workspace(64, 8, 10, 5)
    assert (lib.mrgcn_complex_ranks_both_workspace(64, 8, 10)
            == lib.mrgcn_distmult_ranks_both_workspace(64, 8, 10) + 4 * 10)   # the second truth per fact


def test_entries_refuse_an_odd_width_before_any_launch():
    lib = _lib.load()
    one = C.c_void_p(16)   # never dereferenced: the width is checked first
    assert lib.mrgcn_complex_score_f32(one, 7, one, 7, 7, one, 1, one, None) != 0
    assert lib.mrgcn_complex_score_bwd_f32(one, 7, one, 7, 7, one, 1, one, one, one, one, one, 7, one, 7, one, 1 << 20,
                                           None) != 0
    assert lib.mrgcn_complex_ranks_both(one, 7, 4, one, 7, 7, one, 1, None, None, None, None, None, 0, 0, one, 1 << 20,
                                        one, None, None) != 0
    assert lib.mrgcn_complex_topk(one, 7, 4, one, 7, 7, one, 1, 0, None, None, 1, one, 1 << 20, one, one, None) != 0


# ---- argument checks of the public interface that need no device -----------------------------------------------------
def test_odd_width_raises():
    E, Rel = torch.zeros(4, 7), torch.zeros(2, 7)
    t = np.array([[0, 0, 1]])
    for call in (lambda: lp.score_complex_bc(t, E, Rel),
                 lambda: lp.compute_ranks_fast(t, E, Rel, scorer="complex"),
                 lambda: lp.rank_both(t, E, Rel, scorer="complex"),
                 lambda: lp.predict_topk(np.array([[0, 0]]), E, Rel, 1, scorer="complex")):
        with pytest.raises(_lib.MrgcnError, match="odd"):
            call()


def test_unknown_scorer_raises_naming_the_two():
    E, Rel = torch.zeros(4, 8), torch.zeros(2, 8)
    t = np.array([[0, 0, 1]])
    calls = [lambda: lp.compute_ranks_fast(t, E, Rel, scorer="transe"),
             lambda: lp.rank_both(t, E, Rel, scorer="transe"),
             lambda: lp.predict_topk(np.array([[0, 0]]), E, Rel, 1, scorer="transe"),
             lambda: lp.predict_links(None, None, np.array([[0, 0]]), 1, scorer="transe"),
             lambda: lp.evaluate_batches([], None, scorer="transe"),
             lambda: lp.train_step(None, None, None, None, scorer="transe"),
             lambda: lp.train_batch_step(None, None, None, None, scorer="transe"),
             lambda: lp.train_epoch([], None, None, scorer="transe"),
             lambda: next(lp.fit(None, None, None, None, None, 1, scorer="transe")),
             lambda: next(lp.fit_batches(None, [], None, None, 1, scorer="transe"))]
    for call in calls:
        with pytest.raises(_lib.MrgcnError, match="'distmult' or 'complex'"):
            call()


def test_grouped_decoder_refuses_complex():
    calls = [lambda: lp.train_step(None, None, None, None, decoder="grouped", scorer="complex"),
             lambda: lp.train_batch_step(None, None, None, None, decoder="grouped", scorer="complex"),
             lambda: lp.train_epoch([], None, None, decoder="grouped", scorer="complex"),
             lambda: next(lp.fit(None, None, None, None, None, 1, decoder="grouped", scorer="complex"))]
    for call in calls:
        with pytest.raises(_lib.MrgcnError, match="grouped.*DistMult only"):
            call()


def test_minibatch_run_loop_refuses_complex():
    E, Rel = torch.zeros(4, 8), torch.zeros(2, 8)
    calls = [lambda: next(lp.fit_batches(None, [], None, None, 1, scorer="complex")),
             lambda: lp.BatchFitEpochs(None, [], None, None, scorer="complex"),
             lambda: lp.batch_eval(E, Rel, None, scorer="complex"),
             lambda: lp.eval_batches(None, [], scorer="complex"),
             lambda: lp.rank_batches(None, [], scorer="complex")]
    for call in calls:
        with pytest.raises(_lib.MrgcnError, match="scorer='complex' is not available in the mini-batch run loop"):
            call()
