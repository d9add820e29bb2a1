"""The 1-vs-all softmax decoder without a device: the C entries' declarations and argument checks, the keyword checks
of `decoder="all"`, and the float64 mirrors (`host.pair_vectors64`, `host.all_loss64`, `host.all_lse32`) against torch
in float64 and against the scorers' own formulations."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from mrgcn_amd import _lib, host
from mrgcn_amd.tasks import link_prediction as lp
from tests.test_cpu_host import ROOT, header_functions

NAMES = ("mrgcn_lp_all_supported", "mrgcn_lp_all_chunk", "mrgcn_lp_all_workspace", "mrgcn_lp_all_fwd_f32",
         "mrgcn_lp_all_bwd_f32")
CTYPE = {"int32_t": C.c_int32, "int64_t": C.c_int64, "int": C.c_int}


def _header_signature(name):
    """(result, argument list) of `name` as include/mrgcn_hip.h declares it, in ctypes."""
    import os
    src = open(os.path.join(ROOT, "include", "mrgcn_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in the header"
    args = []
    for a in (x.strip() for x in m.group(2).split(",")):
        if a == "void":
            continue
        args.append(C.c_void_p if "*" in a else CTYPE[a.replace("const ", "").split()[0]])
    return CTYPE[m.group(1)], args


def test_symbols_are_declared_exported_and_bound_with_the_headers_arguments():
    declared = set(header_functions())
    lib = _lib.load()
    for n in NAMES:
        assert n in declared, f"{n} is not declared in include/mrgcn_hip.h"
        assert n in _lib.SIGNATURES, f"{n} is not in the ctypes table"
        assert hasattr(lib, n), f"{n} is not exported by the library"
        res, args = _header_signature(n)
        assert _lib.SIGNATURES[n][0] is res, n
        assert list(_lib.SIGNATURES[n][1]) == args, n
    assert lib.mrgcn_abi_version() == 5
    c = lib.mrgcn_lp_all_chunk()
    assert c >= 64 and c % 64 == 0


def test_workspace_sizes_and_bad_arguments():
    lib = _lib.load()
    c = lib.mrgcn_lp_all_chunk()
    assert lib.mrgcn_lp_all_workspace(0, 5, 8) == -1 and lib.mrgcn_lp_all_workspace(5, 0, 8) == -1
    assert lib.mrgcn_lp_all_workspace(1 << 31, 5, 8) == -1 and lib.mrgcn_lp_all_workspace(5, 1 << 31, 8) == -1
    # few queries: one (max, sum) pair per query and chunk; many: one chunk
    assert lib.mrgcn_lp_all_workspace(70, 2 * c + 1, 8) >= 3 * 70 * 8
    assert lib.mrgcn_lp_all_workspace(70, 2 * c + 1, 8) > lib.mrgcn_lp_all_workspace(70, c, 8)
    assert lib.mrgcn_lp_all_workspace(1 << 20, 2 * c + 1, 8) < 3 * (1 << 20) * 8
    a = np.zeros((8, 8), np.float32)
    ok = lib.mrgcn_lp_all_supported
    base = a.ctypes.data // 16 * 16 + 16
    assert ok(base, 8, 4, base, 8, 4, 8) == 1
    assert ok(base, 8, 4, base, 8, 4, 6) == 0        # H % 4
    assert ok(base, 260, 4, base, 260, 4, 260) == 0  # H > 256
    assert ok(base, 8, 4, base, 10, 4, 8) == 0       # a stride that is no multiple of 4
    assert ok(base + 4, 8, 4, base, 8, 4, 8) == 0    # a base that is not 16-byte aligned
    assert ok(base, 8, 0, base, 8, 4, 8) == 0 and ok(base, 8, 4, base, 8, 1 << 31, 8) == 0
    assert ok(None, 8, 4, base, 8, 4, 8) == 0
    # NULL and bad sizes return non-zero before anything is launched
    assert lib.mrgcn_lp_all_fwd_f32(None, 8, 4, None, 8, 4, 8, None, None, None, None, None, 0, None) != 0
    assert b"NULL" in lib.mrgcn_last_error()
    assert lib.mrgcn_lp_all_fwd_f32(base, 8, 4, base, 8, 4, 6, base, base, base, base, base, 1 << 20, None) != 0
    assert b"shape" in lib.mrgcn_last_error()
    assert lib.mrgcn_lp_all_fwd_f32(base, 8, 4, base, 8, 4, 8, base, base, base, base, base, 16, None) != 0
    assert b"workspace" in lib.mrgcn_last_error()
    assert lib.mrgcn_lp_all_bwd_f32(base, 8, 4, base, 8, 4, 8, base, None, base, base, 8, base, 8, None, 0, None) != 0
    assert lib.mrgcn_lp_all_bwd_f32(base, 8, 4, base, 8, 4, 8, base, base, base, base, 4, base, 8, None, 0, None) != 0
    assert b"lddQ" in lib.mrgcn_last_error()


def test_keyword_checks_need_no_device():
    from mrgcn_amd._lib import MrgcnError

    class Smp:
        facts = None

    def train_step(**kw):
        return lp.train_step(None, None, Smp(), None, **kw)

    def train_batch_step(**kw):
        return lp.train_batch_step(None, None, None, None, **kw)

    def train_epoch(**kw):
        return lp.train_epoch([], None, None, **kw)

    def fit_epochs(**kw):
        return lp.FitEpochs(None, None, None, None, None, sampler=Smp(), **kw)

    def fit(**kw):
        return next(lp.fit(None, None, None, None, None, 1, sampler=Smp(), **kw))

    def batch_fit_epochs(**kw):
        return lp.BatchFitEpochs(None, [], None, None, **kw)

    def fit_batches(**kw):
        return next(lp.fit_batches(None, [], None, None, 1, **kw))
    calls = {f.__name__: f for f in (train_step, train_batch_step, train_epoch, fit_epochs, fit, batch_fit_epochs,
                                     fit_batches)}
    for who, call in calls.items():
        with pytest.raises(MrgcnError, match="loss='softmax'"):
            call(decoder="all")                                   # the default loss is the BCE
        with pytest.raises(MrgcnError, match="1-vs-all BCE is not built"):
            call(decoder="all", loss="bce")
        with pytest.raises(MrgcnError, match="loss"):
            call(decoder="all", loss="hinge")
        with pytest.raises(MrgcnError, match="pos_weight"):
            call(decoder="all", loss="softmax", pos_weight=2.0)
        with pytest.raises(MrgcnError, match="decoder"):
            call(decoder="every")
    with pytest.raises(MrgcnError, match="facts"):
        lp.train_step(None, None, lambda: None, None, decoder="all", loss="softmax")   # a sampler without `.facts`
    # ComplEx stays out of the mini-batch run loop, with the 1-vs-all decoder too
    with pytest.raises(MrgcnError, match="scorer='complex' is not available in the mini-batch run loop"):
        next(lp.fit_batches(None, [], None, None, 1, decoder="all", loss="softmax", scorer="complex"))
    E, Rel = torch.zeros(5, 7), torch.zeros(2, 7)
    facts = torch.zeros((3, 3), dtype=torch.int64)
    with pytest.raises(MrgcnError, match="odd"):
        lp.pair_vectors(facts, E, Rel, "both", "complex")
    with pytest.raises(MrgcnError, match="side"):
        lp.pair_vectors(facts, E, Rel, "left", "distmult")
    with pytest.raises(MrgcnError, match="side"):
        lp.all_loss(facts, E, Rel, side="left")
    with pytest.raises(MrgcnError, match="'distmult' or 'complex'"):
        lp.all_loss(facts, E, Rel, scorer="transe")
    with pytest.raises(MrgcnError, match="GPU"):
        lp.all_loss(facts, E, Rel)                                # no CPU decoder
    with pytest.raises(ValueError, match="side"):
        host.pair_vectors64(facts.numpy(), E.numpy(), Rel.numpy(), "left")


def _problem(H, seed=3, N=41, R=5, n=60):
    rng = np.random.default_rng(seed)
    E, Rel = rng.standard_normal((N, H)), rng.standard_normal((R, H))
    facts = np.stack([rng.integers(0, N, n), rng.integers(0, R, n), rng.integers(0, N, n)], 1).astype(np.int64)
    return E, Rel, facts


@pytest.mark.parametrize("scorer", ["distmult", "complex"])
@pytest.mark.parametrize("side", ["both", "tail", "head"])
def test_pair_vectors_dotted_with_a_candidate_are_the_corrupted_triples_scores(side, scorer):
    E, Rel, facts = _problem(12)
    N, n = E.shape[0], len(facts)
    Q, tg = host.pair_vectors64(facts, E, Rel, side, scorer)
    x = Q @ E.T
    corrupt = []
    if side in ("both", "tail"):
        corrupt.append((2, facts[:, 2]))
    if side in ("both", "head"):
        corrupt.append((0, facts[:, 0]))
    assert Q.shape == (n * len(corrupt), 12) and np.array_equal(tg, np.concatenate([c[1] for c in corrupt]))
    for k, (col, _) in enumerate(corrupt):
        for c in range(N):
            t = facts.copy()
            t[:, col] = c
            want = host.complex_scores64(t, E, Rel) if scorer == "complex" \
                else np.sum(E[t[:, 0]] * Rel[t[:, 1]] * E[t[:, 2]], axis=1)
            np.testing.assert_allclose(x[k * n:(k + 1) * n, c], want, rtol=1e-12, atol=1e-12)
    # the torch form under autograd is the same function
    Qt, tgt = lp.pair_vectors(torch.from_numpy(facts), torch.from_numpy(E), torch.from_numpy(Rel), side, scorer)
    np.testing.assert_allclose(Qt.numpy(), Q, rtol=1e-14, atol=1e-14)
    assert np.array_equal(tgt.numpy(), tg)


@pytest.mark.parametrize("scorer", ["distmult", "complex"])
def test_mirror_equals_torch_cross_entropy_in_float64_with_its_gradients(scorer):
    import torch.nn.functional as F
    E, Rel, facts = _problem(8, seed=4)
    Q, tg = host.pair_vectors64(facts, E, Rel, "both", scorer)
    Qt, Et = torch.from_numpy(Q).requires_grad_(), torch.from_numpy(E).requires_grad_()
    want = F.cross_entropy(Qt @ Et.t(), torch.from_numpy(tg))
    (want * -1.75).backward()
    loss, lse, dQ, dE = host.all_loss64(Q, E, tg, upstream=-1.75)
    assert abs(loss - float(want.detach())) <= 1e-13 * abs(float(want.detach()))
    np.testing.assert_allclose(lse, torch.logsumexp(Qt @ Et.t(), 1).detach().numpy(), rtol=1e-13)
    np.testing.assert_allclose(dQ, Qt.grad.numpy(), rtol=1e-11, atol=1e-14)
    np.testing.assert_allclose(dE, Et.grad.numpy(), rtol=1e-11, atol=1e-14)


def test_mirror_survives_scores_of_plus_minus_200_and_one_candidate():
    rng = np.random.default_rng(5)
    Q, E = rng.standard_normal((9, 4)), rng.standard_normal((30, 4))
    s = np.sqrt(200.0 / np.abs(Q @ E.T).max())
    loss, lse, dQ, dE = host.all_loss64(s * Q, s * E, np.arange(9))
    assert np.isfinite(loss) and np.all(np.isfinite(lse)) and np.all(np.isfinite(dQ)) and np.all(np.isfinite(dE))
    lse32, xt32 = host.all_lse32(s * Q, s * E, np.arange(9))
    assert lse32.dtype == np.float32 and xt32.dtype == np.float32
    np.testing.assert_allclose(lse32, lse, rtol=1e-5)
    loss, lse, dQ, dE = host.all_loss64(Q[:1], E[:1], np.zeros(1, np.int64))
    assert loss == 0.0 and not dQ.any() and not dE.any()
