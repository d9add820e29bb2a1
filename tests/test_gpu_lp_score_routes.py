"""Which kernels the flat score backward launches, on which rows, for every row of DESIGN §8's route table — and that
each route's gradients are right.  Public API only (`score_distmult_bc`, `score_complex_bc`, `SortedTriples`,
`binary_crossentropy`): the library is watched through a proxy swapped in for `_lib.load`, which records every backward
and order entry as (name, number of triples, byte offset of its triples from the scored tensor's start).

Shapes: 50 nodes, 7 relations, widths 8 (16-byte rows) and 6 (the element-wise kernels; even, so ComplEx reads it too);
the triple counts sit on both sides of every threshold (4096 for the sorted and the self-sorting deterministic kernel,
1024 behind 100 stored facts for the counting sort).  Gradients are held to the float64 oracle at rtol 1e-3 /
atol 1e-6 through the mean BCE, the bound tests/test_gpu_lp.py and tests/test_gpu_lp_deterministic.py hold them to;
routes without float atomics (every deterministic and every ComplEx one) repeat bit for bit."""
import contextlib

import numpy as np
import pytest
import torch

from mrgcn_amd import host
from oracle import lp_oracle as lo
from tests.test_cpu_lp_complex import complex_grads64, tables, triples
from tests.test_gpu_lp_fit import deterministic

pytestmark = pytest.mark.gpu

N, R, NS = 50, 7, 100
KERNELS = {"sorted": "mrgcn_distmult_score_bwd_sorted_f32", "scatter": "mrgcn_distmult_score_bwd_f32",
           "det": "mrgcn_distmult_score_bwd_det_f32", "complex": "mrgcn_complex_score_bwd_f32"}
SORTS = {"counting": "mrgcn_distmult_orders_counting", "radix": "mrgcn_distmult_orders"}


class Recorder:
    """Delegates to the real library; the backward and order entries (not their workspace queries) are recorded."""

    def __init__(self, lib):
        self._lib, self.calls, self.base = lib, [], 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not ("score_bwd" in name or "distmult_orders" in name) or name.endswith("_workspace"):
            return fn
        at = 0 if "distmult_orders" in name else 5          # (triples, n) lead the order entries, follow H in the others

        def recorded(*args):
            self.calls.append((name, int(args[at + 1]), int(args[at].value) - self.base))
            return fn(*args)
        return recorded


def launches(plan):
    """The entries a plan of (start, count, orders, kernel) segments calls, as the recorder writes them."""
    out = []
    for start, count, orders, kernel in plan:
        if orders in SORTS:
            out.append((SORTS[orders], count, 24 * start))
        out.append((KERNELS[kernel], count, 24 * start))
    return out


_REF: dict = {}


def reference(scorer, H, n):
    """(E, Rel, triples, labels, dE, dR) of a case, the float64 gradients computed once."""
    key = (scorer, H, n)
    if key not in _REF:
        E, Rel = tables(N, R, H, seed=H)
        t = triples(N, R, n, seed=n)
        labels = (np.arange(n) < max(NS, n // 2)).astype(np.float32)
        if scorer == "distmult":
            dE, dR = lo.distmult_bce_grads(t, E, Rel, labels)
        else:
            x = host.complex_scores64(t, E, Rel)
            dE, dR = complex_grads64(t, E, Rel, (1.0 / (1.0 + np.exp(-x)) - labels) / n)
        _REF[key] = (E, Rel, t, labels, dE, dR)
    return _REF[key]


def run_case(monkeypatch, scorer, H, n, plan, static=None, det=False, exact=False):
    from mrgcn_amd.tasks import link_prediction as lp
    E, Rel, t, labels, dE, dR = reference(scorer, H, n)
    td, yd = torch.from_numpy(t).cuda(), torch.from_numpy(labels).cuda()
    st = None
    if static == "covering":
        st = lp.SortedTriples(td[:NS].clone(), N, R)
    elif static == "other":
        st = lp.SortedTriples(torch.from_numpy(triples(N, R, NS, seed=n + 1)).cuda(), N, R)
    score = lp.score_distmult_bc if scorer == "distmult" else lp.score_complex_bc
    rec = Recorder(lp._lib.load())
    monkeypatch.setattr(lp._lib, "load", lambda: rec)
    rec.base = td.data_ptr()
    want = launches(plan)

    def grads(need_E, need_R):
        Ed, Rd = torch.from_numpy(E).cuda().requires_grad_(need_E), torch.from_numpy(Rel).cuda().requires_grad_(need_R)
        del rec.calls[:]
        lp.binary_crossentropy(score(td, Ed, Rd, static=st), yd).backward()
        assert rec.calls == want, (rec.calls, want)
        return (Ed.grad.cpu().numpy() if need_E else None), (Rd.grad.cpu().numpy() if need_R else None)

    with deterministic() if det else contextlib.nullcontext():
        both = grads(True, True)
        only_E, only_R = grads(True, False)[0], grads(False, True)[1]
        again = grads(True, True) if exact else None
    for got in (both[0], only_E):
        np.testing.assert_allclose(got, dE, rtol=1e-3, atol=1e-6)
    for got in (both[1], only_R):
        np.testing.assert_allclose(got, dR, rtol=1e-3, atol=1e-6)
    if exact:
        assert again[0].tobytes() == both[0].tobytes() and again[1].tobytes() == both[1].tobytes()


WIDTHS = pytest.mark.parametrize("H", [8, 6])


@WIDTHS
@pytest.mark.parametrize("n, plan", [
    (65, [(0, 65, None, "scatter")]),
    (4095, [(0, 4095, None, "scatter")]),
    (4096, [(0, 4096, "radix", "sorted")]),
])
def test_distmult_without_stored_orders(monkeypatch, H, n, plan):
    run_case(monkeypatch, "distmult", H, n, plan)


@WIDTHS
@pytest.mark.parametrize("n, tail", [
    (100, []),
    (125, [(100, 25, None, "scatter")]),
    (1123, [(100, 1023, None, "scatter")]),
    (1124, [(100, 1024, "counting", "sorted")]),
])
def test_distmult_behind_stored_facts(monkeypatch, H, n, tail):
    run_case(monkeypatch, "distmult", H, n, [(0, NS, "stored", "sorted")] + tail, static="covering")


@WIDTHS
def test_distmult_stored_facts_with_the_sorted_backward_switched_off(monkeypatch, H):
    monkeypatch.setenv("MRGCN_LP_SORTED_BWD", "0")
    run_case(monkeypatch, "distmult", H, 1124, [(0, 1124, None, "scatter")], static="covering")


@WIDTHS
def test_stored_orders_that_do_not_cover_the_scored_triples_are_not_walked(monkeypatch, H):
    run_case(monkeypatch, "distmult", H, 125, [(0, 125, None, "scatter")], static="other")


@WIDTHS
@pytest.mark.parametrize("n, plan", [
    (65, [(0, 65, "self", "det")]),
    (4096, [(0, 4096, "self", "det")]),
    (4097, [(0, 4097, "radix", "det")]),
])
def test_deterministic_distmult_without_stored_orders(monkeypatch, H, n, plan):
    run_case(monkeypatch, "distmult", H, n, plan, det=True, exact=True)


@WIDTHS
@pytest.mark.parametrize("n, tail", [
    (125, [(100, 25, "self", "det")]),
    (NS + 4097, [(100, 4097, "radix", "det")]),
])
def test_deterministic_distmult_behind_stored_facts(monkeypatch, H, n, tail):
    run_case(monkeypatch, "distmult", H, n, [(0, NS, "stored", "det")] + tail, static="covering", det=True, exact=True)


@WIDTHS
@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("n, static, plan", [
    (65, None, [(0, 65, "radix", "complex")]),
    (125, "covering", [(0, NS, "stored", "complex"), (100, 25, "radix", "complex")]),
])
def test_complex_has_one_route(monkeypatch, H, det, n, static, plan):
    run_case(monkeypatch, "complex", H, n, plan, static=static, det=det, exact=True)
