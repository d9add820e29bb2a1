"""The KvsAll decoder without a device: the C entries' declarations and argument checks, the keyword checks of
`decoder="kvsall"` / `label_smoothing`, the query lists of `host.kvsall_queries` against a brute-force dictionary, and
the float64 mirror (`host.kvsall_loss64`) against torch's `binary_cross_entropy_with_logits` in float64."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from mrgcn_amd import _lib, host
from mrgcn_amd.tasks import link_prediction as lp
from tests.test_cpu_host import ROOT, header_functions

NAMES = ("mrgcn_lp_kvsall_supported", "mrgcn_lp_kvsall_workspace", "mrgcn_lp_kvsall_fwd_f32",
         "mrgcn_lp_kvsall_bwd_f32")
CTYPE = {"int32_t": C.c_int32, "int64_t": C.c_int64, "int": C.c_int, "float": C.c_float, "double": C.c_double}


def _header_signature(name):
    """(result, argument list) of `name` as include/mrgcn_hip.h declares it, in ctypes."""
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


def test_workspace_sizes_and_bad_arguments():
    lib = _lib.load()
    c = lib.mrgcn_lp_all_chunk()
    ws = lib.mrgcn_lp_kvsall_workspace
    assert ws(0, 5, 8) == -1 and ws(5, 0, 8) == -1 and ws(1 << 31, 5, 8) == -1 and ws(5, 1 << 31, 8) == -1
    # few queries: a (sum softplus, sum x) pair per query and chunk, a float per query, a double per 256 queries
    assert ws(70, 2 * c + 1, 8) >= 3 * 70 * 8 + 70 * 4 + 8
    assert ws(70, 2 * c + 1, 8) > ws(70, c, 8)
    assert ws(1 << 20, 2 * c + 1, 8) < 3 * (1 << 20) * 8     # many queries: one chunk
    a = np.zeros((8, 8), np.float32)
    base = a.ctypes.data // 16 * 16 + 16
    ok = lib.mrgcn_lp_kvsall_supported
    assert ok(base, 8, 4, base, 8, 4, 8) == 1
    assert ok(base, 8, 4, base, 8, 4, 6) == 0        # H % 4
    assert ok(base, 260, 4, base, 260, 4, 260) == 0  # H > 256
    assert ok(base, 8, 4, base, 10, 4, 8) == 0       # a stride that is no multiple of 4
    assert ok(base + 4, 8, 4, base, 8, 4, 8) == 0    # a base that is not 16-byte aligned
    assert ok(base, 8, 0, base, 8, 4, 8) == 0 and ok(base, 8, 4, base, 8, 1 << 31, 8) == 0
    assert ok(None, 8, 4, base, 8, 4, 8) == 0
    big = 1 << 20

    def fwd(Q=base, ldQ=8, H=8, ptr=base, idx=base, eps=0.0, loss=base, w=base, nw=big):
        return lib.mrgcn_lp_kvsall_fwd_f32(Q, ldQ, 4, base, 8, 4, H, ptr, idx, eps, None, loss, w, nw, None)

    def bwd(Q=base, ldQ=8, H=8, ptr=base, idx=base, cptr=base, cqry=base, eps=0.0, gl=base, dQ=base, lddQ=8, dE=base,
            lddE=8):
        return lib.mrgcn_lp_kvsall_bwd_f32(Q, ldQ, 4, base, 8, 4, H, ptr, idx, cptr, cqry, eps, gl, dQ, lddQ, dE, lddE,
                                           None, 0, None)
    # every one of these returns non-zero before anything is launched (there is no device here)
    for bad in (dict(Q=None), dict(ptr=None), dict(idx=None), dict(loss=None)):
        assert fwd(**bad) != 0 and b"NULL" in lib.mrgcn_last_error(), bad
    for bad in (dict(H=6), dict(H=260, ldQ=260), dict(ldQ=10), dict(Q=base + 4)):
        assert fwd(**bad) != 0 and b"shape" in lib.mrgcn_last_error(), bad
        assert bwd(**bad) != 0 and b"shape" in lib.mrgcn_last_error(), bad
    for eps in (1.0, -0.1, 1.5, float("nan")):
        assert fwd(eps=eps) != 0 and b"label_smoothing" in lib.mrgcn_last_error(), eps
        assert bwd(eps=eps) != 0 and b"label_smoothing" in lib.mrgcn_last_error(), eps
    for bad in (dict(w=None), dict(nw=16), dict(w=base + 4)):
        assert fwd(**bad) != 0 and b"workspace" in lib.mrgcn_last_error(), bad
    for bad in (dict(Q=None), dict(gl=None), dict(ptr=None), dict(idx=None), dict(cptr=None), dict(cqry=None)):
        assert bwd(**bad) != 0 and b"NULL" in lib.mrgcn_last_error(), bad
    for bad in (dict(lddQ=4), dict(lddE=4)):
        assert bwd(**bad) != 0 and b"lddQ" in lib.mrgcn_last_error(), bad


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
        with pytest.raises(MrgcnError, match="kvsall.*loss='bce'"):
            call(decoder="kvsall", loss="softmax")
        with pytest.raises(MrgcnError, match="kvsall.*loss='bce'"):
            call(decoder="kvsall", loss="hinge")
        with pytest.raises(MrgcnError, match="pos_weight.*kvsall"):
            call(decoder="kvsall", pos_weight=2.0)
        for eps in (1.0, -0.1):
            with pytest.raises(MrgcnError, match=r"label_smoothing is in \[0, 1\)"):
                call(decoder="kvsall", label_smoothing=eps)
        with pytest.raises(MrgcnError, match="label_smoothing belongs to decoder='kvsall'"):
            call(decoder="triples", label_smoothing=0.1)
        with pytest.raises(MrgcnError, match="label_smoothing belongs to decoder='kvsall'"):
            call(decoder="all", loss="softmax", label_smoothing=0.1)
        # what was refused before still is, in the same words
        with pytest.raises(MrgcnError, match="1-vs-all BCE is not built"):
            call(decoder="all", loss="bce")
        with pytest.raises(MrgcnError, match="decoder"):
            call(decoder="every")
    with pytest.raises(MrgcnError, match="decoder='kvsall' reads the facts"):
        lp.train_step(None, None, lambda: None, None, decoder="kvsall")   # a sampler without `.facts`
    with pytest.raises(MrgcnError, match="scorer='complex' is not available in the mini-batch run loop"):
        next(lp.fit_batches(None, [], None, None, 1, decoder="kvsall", scorer="complex"))
    E, Rel = torch.zeros(5, 8), torch.zeros(2, 8)
    kq = lp.KvsAllQueries(np.zeros((3, 3), np.int64), 5, 2, device="cpu")
    with pytest.raises(MrgcnError, match="label_smoothing"):
        lp.kvsall_loss(kq, E, Rel, label_smoothing=1.0)
    with pytest.raises(MrgcnError, match="'distmult' or 'complex'"):
        lp.kvsall_loss(kq, E, Rel, scorer="transe")
    with pytest.raises(MrgcnError, match="kvsall"):
        lp.kvsall_loss(np.zeros((3, 3), np.int64), E, Rel)        # facts, not queries
    with pytest.raises(MrgcnError, match="GPU"):
        lp.kvsall_loss(kq, E, Rel)                                # no CPU decoder
    with pytest.raises(MrgcnError, match="side"):
        lp.KvsAllQueries(np.zeros((3, 3), np.int64), 5, 2, side="left", device="cpu")


# node 6 is never an answer (nor anything else); (0, 0, ?) has the tails 1, 2, 3; (?, 1, 5) has the heads 2, 3, 4; the
# fact (0, 0, 2) stands twice
N_, R_ = 7, 2
FACTS = np.array([[0, 0, 2], [3, 1, 5], [0, 0, 1], [4, 1, 5], [0, 0, 2], [0, 0, 3], [2, 1, 5], [5, 0, 0], [1, 1, 0],
                  [5, 1, 0]], np.int64)


def _brute(side):
    """The queries as a dictionary walk: (key, representative's (s, p) or (p, o), sorted answers) per query, in order."""
    facts = sorted(set(map(tuple, FACTS.tolist())))
    out = []
    if side in ("both", "tail"):
        d = {}
        for s, p, o in facts:
            d.setdefault(s * R_ + p, ((s, p), set()))[1].add(o)
        out += [("tail", d[k][0], sorted(d[k][1])) for k in sorted(d)]
    if side in ("both", "head"):
        d = {}
        for s, p, o in facts:
            d.setdefault(p * N_ + o, ((p, o), set()))[1].add(s)
        out += [("head", d[k][0], sorted(d[k][1])) for k in sorted(d)]
    return out


@pytest.mark.parametrize("side", ["both", "tail", "head"])
def test_queries_against_a_brute_force_dictionary(side):
    reps, m_tail, ptr, idx, cptr, cqry = host.kvsall_queries(FACTS, N_, R_, side)
    want = _brute(side)
    m = len(want)
    assert reps.shape == (m, 3) and ptr.shape == (m + 1,) and ptr.dtype == np.int64 and idx.dtype == np.int32
    assert cptr.shape == (N_ + 1,) and cptr.dtype == np.int64 and cqry.dtype == np.int32
    assert m_tail == sum(1 for w in want if w[0] == "tail") == {"both": 7, "tail": 7, "head": 0}[side]
    assert ptr[0] == 0 and ptr[-1] == len(idx) == len(cqry) == cptr[-1]
    known = set(map(tuple, FACTS.tolist()))
    for q, (kind, key, ans) in enumerate(want):
        got = idx[ptr[q]:ptr[q + 1]].tolist()
        assert got == ans, (q, kind, key, got, ans)                  # ascending, a duplicate fact once
        assert tuple(reps[q]) in known
        assert (reps[q, 0], reps[q, 1]) == key if kind == "tail" else (reps[q, 1], reps[q, 2]) == key
        assert reps[q, 2 if kind == "tail" else 0] in ans
    if side != "head":
        assert idx[ptr[0]:ptr[1]].tolist() == [1, 2, 3]              # (0, 0, ?)
    if side != "tail":
        q = [w[1] for w in want].index((1, 5))
        assert idx[ptr[q]:ptr[q + 1]].tolist() == [2, 3, 4]          # (?, 1, 5)
    # the transposed lists are exactly the transpose, queries ascending per node; node 6 has none
    pairs = {(q, int(c)) for q in range(m) for c in idx[ptr[q]:ptr[q + 1]]}
    assert len(pairs) == len(idx)
    tr = set()
    for c in range(N_):
        qs = cqry[cptr[c]:cptr[c + 1]].tolist()
        assert qs == sorted(set(qs)), (c, qs)
        tr |= {(q, c) for q in qs}
    assert tr == pairs
    assert cptr[6] == cptr[7]
    assert m < (2 if side == "both" else 1) * len(known)


def test_queries_object_on_the_cpu_holds_the_mirrors_arrays_and_checks_ids():
    from mrgcn_amd._lib import MrgcnError
    for facts in (FACTS, torch.from_numpy(FACTS)):
        kq = lp.KvsAllQueries(facts, N_, R_, device="cpu")
        want = host.kvsall_queries(FACTS, N_, R_, "both")
        assert (kq.m, kq.m_tail, kq.nnz) == (len(want[0]), want[1], len(want[3]))
        for got, w in zip((kq.reps, kq.ptr, kq.idx, kq.cptr, kq.cqry), (want[0], want[2], want[3], want[4], want[5])):
            assert got.device.type == "cpu" and got.numpy().dtype == w.dtype and np.array_equal(got.numpy(), w)
        assert np.array_equal(kq.rows.numpy(), np.repeat(np.arange(kq.m), np.diff(want[2])))
    for bad in ([[7, 0, 0]], [[0, 0, 7]], [[0, 2, 0]], [[-1, 0, 0]]):
        with pytest.raises(MrgcnError, match="outside num_nodes"):
            lp.KvsAllQueries(np.array(bad, np.int64), N_, R_, device="cpu")
        with pytest.raises(ValueError, match="outside num_nodes"):
            host.kvsall_queries(np.array(bad, np.int64), N_, R_)
    with pytest.raises(MrgcnError, match=r"\[n, 3\]"):
        lp.KvsAllQueries(np.zeros((0, 3), np.int64), N_, R_, device="cpu")


def _torch64(Q, E, ptr, idx, eps, upstream):
    import torch.nn.functional as F
    m, N = Q.shape[0], E.shape[0]
    Y = torch.zeros((m, N), dtype=torch.float64)
    Y[np.repeat(np.arange(m), np.diff(ptr)), idx.astype(np.int64)] = 1
    Qt, Et = torch.from_numpy(Q).requires_grad_(), torch.from_numpy(E).requires_grad_()
    x = Qt @ Et.t()
    loss = F.binary_cross_entropy_with_logits(x, (1 - eps) * Y + eps / N, reduction="mean")
    (loss * upstream).backward()
    per_query = F.binary_cross_entropy_with_logits(x, (1 - eps) * Y + eps / N, reduction="none").sum(1)
    return float(loss.detach()), per_query.detach().numpy(), Qt.grad.numpy(), Et.grad.numpy()


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_mirror_equals_torch_bce_with_logits_in_float64_with_its_gradients(eps):
    rng = np.random.default_rng(11)
    E, Rel = rng.standard_normal((N_, 8)), rng.standard_normal((R_, 8))
    reps, m_tail, ptr, idx, _, _ = host.kvsall_queries(FACTS, N_, R_)
    Q = np.concatenate([host.pair_vectors64(reps[:m_tail], E, Rel, "tail")[0],
                        host.pair_vectors64(reps[m_tail:], E, Rel, "head")[0]])
    want = _torch64(Q, E, ptr, idx, eps, -1.75)
    got = host.kvsall_loss64(Q, E, ptr, idx, eps, upstream=-1.75)
    assert abs(got[0] - want[0]) <= 1e-12 * abs(want[0])
    for g, w in zip(got[1:], want[1:]):
        np.testing.assert_allclose(g, w, rtol=1e-12, atol=1e-12 * np.abs(w).max())
    loss32, pq32 = host.kvsall_loss32(Q, E, ptr, idx, eps)
    assert loss32.dtype == np.float32 and pq32.dtype == np.float32
    np.testing.assert_allclose(pq32, got[1], rtol=1e-5)
    assert abs(float(loss32) - got[0]) <= 1e-5 * abs(got[0])


def test_mirror_survives_scores_of_plus_minus_200_and_one_candidate():
    rng = np.random.default_rng(5)
    Q, E = rng.standard_normal((9, 4)), rng.standard_normal((30, 4))
    s = np.sqrt(200.0 / np.abs(Q @ E.T).max())
    x = (s * Q) @ (s * E).T
    ptr = np.arange(10, dtype=np.int64)
    idx = x.argmin(axis=1).astype(np.int32)          # every query's positive is its most negative score
    assert x.max() > 199 or x.min() < -199
    for eps in (0.0, 0.1):
        loss, pq, dQ, dE = host.kvsall_loss64(s * Q, s * E, ptr, idx, eps)
        assert np.isfinite(loss) and all(np.all(np.isfinite(a)) for a in (pq, dQ, dE))
        want = _torch64(s * Q, s * E, ptr, idx, eps, 1.0)
        assert abs(loss - want[0]) <= 1e-12 * abs(want[0])
        np.testing.assert_allclose(dQ, want[2], rtol=1e-12, atol=1e-12 * np.abs(want[2]).max())
        loss32, pq32 = host.kvsall_loss32(s * Q, s * E, ptr, idx, eps)
        assert np.isfinite(loss32) and np.all(np.isfinite(pq32))
    # N = 1: the smoothed target of the lone candidate is (1 - eps) y + eps
    for ptr1, idx1 in ((np.array([0, 1]), np.array([0], np.int32)), (np.array([0, 0]), np.zeros(0, np.int32))):
        for eps in (0.0, 0.1):
            got = host.kvsall_loss64(Q[:1], E[:1], ptr1, idx1, eps)
            want = _torch64(Q[:1], E[:1], ptr1, idx1, eps, 1.0)
            assert np.isfinite(got[0]) and abs(got[0] - want[0]) <= 1e-12 * abs(want[0])
            np.testing.assert_allclose(got[3], want[3], rtol=1e-12, atol=1e-15)
