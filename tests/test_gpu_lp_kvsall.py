"""The KvsAll decoder on the device (csrc/lp_kvsall.hip; mrgcn_amd.tasks.link_prediction: KvsAllQueries,
kvsall_pairs_loss, kvsall_loss, decoder="kvsall").

Bounds: the rule of tests/test_gpu_lp_all.py.  Nothing is fixed in advance: for every case the float32 restatement of
the same arithmetic — `host.kvsall_loss32` (a float32 matmul, a float32 softplus, float32 sums) for the loss and the
per-query sums, float32 torch autograd of the materialised `F.binary_cross_entropy_with_logits(Q @ E.T, Y')` on the CPU
for the gradients — is measured against the float64 mirror (`host.kvsall_loss64`) on the same inputs, and the kernel
gets 4 x that maximum error: it differs from the restatement in summation order and in the last ulp of expf / log1pf.
The floor is one float32 ulp of the compared value.  No element is excluded; every assertion message carries the
measured error and the allowance.

Answer lists.  Every case's lists come from a seeded generator and hold, where the shape has room for them (m >= 4,
N >= 4): an empty list (query 1), a list of all N candidates (query 2), answers at c = 0 and c = N - 1 (query 0), a
candidate that is an answer of every query with a non-empty list, a candidate that is an answer of none but the
all-N query, and non-empty lists for the last query and the last candidate (the ends of the partly filled tiles).
The (1, 2, 4) shape has one query: its list is both candidates."""
import ctypes as C

import numpy as np
import pytest
import torch

from mrgcn_amd import host
from tests.test_gpu_lp_fit import N_, P_, _fwd, _model, _small, deterministic

pytestmark = pytest.mark.gpu
EPS = [0.0, 0.1]


def _np(t):
    return t.detach().cpu().numpy()


def _chunk():
    from mrgcn_amd import _lib
    return int(_lib.load().mrgcn_lp_all_chunk())


# ---- answer lists -----------------------------------------------------------------------------------------------------
def answer_lists(m, N, seed):
    """-> list of m sorted answer lists (see the module docstring)."""
    rng = np.random.default_rng(seed)
    if m < 4 or N < 4:
        return [list(range(N)) for _ in range(m)]
    every, none = N // 2, N // 2 + 1
    lists = []
    for q in range(m):
        s = set(rng.choice(N, size=int(rng.integers(1, 6)), replace=False).tolist()) | {every}
        s.discard(none)
        lists.append(s)
    lists[0] |= {0, N - 1}
    lists[1] = set()
    lists[2] = set(range(N))
    lists[m - 1] |= {N - 1}
    lists = [sorted(s) for s in lists]
    assert lists[1] == [] and lists[2] == list(range(N)) and lists[0][0] == 0 and lists[0][-1] == N - 1
    assert all(every in s for q, s in enumerate(lists) if q != 1)
    assert all(none not in s for q, s in enumerate(lists) if q != 2)
    assert lists[m - 1] and lists[m - 1][-1] == N - 1
    return lists


def csr(lists, N):
    """(ptr, idx, cptr, cqry) of the lists, as `host.kvsall_queries` lays them out."""
    ptr = np.concatenate([[0], np.cumsum([len(s) for s in lists])]).astype(np.int64)
    idx = np.asarray([c for s in lists for c in s], np.int32)
    rows = np.repeat(np.arange(len(lists), dtype=np.int64), np.diff(ptr))
    order = np.argsort(idx, kind="stable")
    cptr = np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=N))]).astype(np.int64)
    return ptr, idx, cptr, rows[order].astype(np.int32)


# ---- the kernels through the C ABI -----------------------------------------------------------------------------------
def _device_rows(a, pad):
    """`a` as a strided view (ld = H + pad) into a larger table filled with a sentinel."""
    big = torch.full((a.shape[0], a.shape[1] + pad), 7.0, dtype=torch.float32, device="cuda")
    big[:, :a.shape[1]] = torch.from_numpy(a).cuda()
    return big, big[:, :a.shape[1]]


def _dev(a):
    """A device copy of a host array; one spare element, so that an empty array still has an address."""
    t = torch.zeros(len(a) + 1, dtype=torch.from_numpy(a).dtype, device="cuda")
    t[:len(a)] = torch.from_numpy(a).cuda()
    return t


def run_abi(Q, E, lists, eps, gl=1.0, pad=0, want=(True, True), cand=True):
    """forward + backward through the C entries -> dict of device results (dQ / dE None when not asked for)."""
    from mrgcn_amd import _lib
    lib = _lib.load()
    m, H = Q.shape
    N = E.shape[0]
    Qb, Qd = _device_rows(Q, pad)
    Eb, Ed = _device_rows(E, pad)
    ptr, idx, cptr, cqry = (_dev(a) for a in csr(lists, N))
    assert lib.mrgcn_lp_kvsall_supported(Qd.data_ptr(), Qd.stride(0), m, Ed.data_ptr(), Ed.stride(0), N, H) == 1
    pq, loss = torch.empty(m, device="cuda"), torch.empty((), device="cuda")
    nws = int(lib.mrgcn_lp_kvsall_workspace(m, N, H))
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    gld = torch.full((1,), gl, dtype=torch.float32, device="cuda")
    dQb = torch.full((m, H + pad), 7.0, device="cuda") if want[0] else None
    dEb = torch.full((N, H + pad), 7.0, device="cuda") if want[1] else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
    _lib.check(lib.mrgcn_lp_kvsall_fwd_f32(p(Qd), Qd.stride(0), m, p(Ed), Ed.stride(0), N, H, p(ptr), p(idx), eps, p(pq),
                                           p(loss), p(ws), nws, st), "fwd")
    _lib.check(lib.mrgcn_lp_kvsall_bwd_f32(p(Qd), Qd.stride(0), m, p(Ed), Ed.stride(0), N, H, p(ptr), p(idx),
                                           p(cptr) if cand else None, p(cqry) if cand else None, eps, p(gld), p(dQb),
                                           H + pad, p(dEb), H + pad, None, 0, st), "bwd")
    torch.cuda.synchronize()
    for b, src in ((dQb, Qb), (dEb, Eb)):
        if b is not None and pad:
            assert bool((b[:, H:] == 7.0).all()), "the backward wrote past a row's H columns"
        assert bool((src[:, H:] == 7.0).all())
    return dict(loss=loss, per_query=pq, dQ=None if dQb is None else dQb[:, :H], dE=None if dEb is None else dEb[:, :H])


_REF: dict = {}


def reference(key, Q, E, lists, eps, gl):
    """float64 values and what the float32 restatement misses them by (computed once per case, never changed)."""
    if key not in _REF:
        import torch.nn.functional as F
        m, N = Q.shape[0], E.shape[0]
        ptr, idx, _, _ = csr(lists, N)
        loss64, pq64, dQ64, dE64 = host.kvsall_loss64(Q, E, ptr, idx, eps, gl)
        loss32, pq32 = host.kvsall_loss32(Q, E, ptr, idx, eps)
        Y = torch.zeros((m, N), dtype=torch.float32)
        Y[np.repeat(np.arange(m), np.diff(ptr)), idx.astype(np.int64)] = 1
        Ys = (1.0 - eps) * Y + eps / N
        Qt, Et = torch.from_numpy(Q).requires_grad_(), torch.from_numpy(E).requires_grad_()
        (F.binary_cross_entropy_with_logits(Qt @ Et.t(), Ys) * np.float32(gl)).backward()
        _REF[key] = dict(
            want=dict(loss=np.float64(loss64), per_query=pq64, dQ=dQ64, dE=dE64),
            err=dict(loss=abs(float(loss32) - loss64), per_query=np.abs(pq32 - pq64).max(),
                     dQ=np.abs(Qt.grad.numpy() - dQ64).max(), dE=np.abs(Et.grad.numpy() - dE64).max()))
    return _REF[key]


def within(name, got, ref, what):
    want, err32 = np.asarray(ref["want"][what]), float(ref["err"][what])
    got = np.asarray(_np(got), np.float64)
    assert np.all(np.isfinite(got)), f"{name} {what}: not finite"
    allow = np.maximum(4.0 * err32, np.spacing(np.abs(want).astype(np.float32)).astype(np.float64))
    err = np.abs(got - want)
    msg = (f"{name} {what}: kernel max error {err.max():.3e}, float32 restatement {err32:.3e}, "
           f"allowance {np.max(allow):.3e} (4 x restatement, floor 1 ulp), ratio {err.max() / max(err32, 1e-300):.2f}")
    print(msg)
    assert np.all(err <= allow), msg


def check_case(name, Q, E, lists, eps, gl=1.0, pad=0, want=(True, True), cand=True):
    ref = reference((name, eps, gl), Q, E, lists, eps, gl)
    out = run_abi(Q, E, lists, eps, gl, pad, want, cand)
    for what in ("loss", "per_query") + (("dQ",) if want[0] else ()) + (("dE",) if want[1] else ()):
        within(f"{name} eps={eps}", out[what], ref, what)
    return out


def tables(m, N, H, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    Q = (scale * rng.standard_normal((m, H))).astype(np.float32)
    E = (scale * rng.standard_normal((N, H))).astype(np.float32)
    return Q, E, answer_lists(m, N, seed)


def shapes():
    return [(1, 2, 4), (63, 65, 12), (65, 63, 20), (130, 300, 200), (257, 64, 256), (70, 2 * _chunk() + 1, 8)]


SHAPE_IDS = ["1x2x4", "63x65x12", "65x63x20", "130x300x200", "257x64x256", "70x(2C+1)x8"]


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("i", range(6), ids=SHAPE_IDS)
def test_loss_per_query_and_gradients_at_every_shape(i, eps):
    from mrgcn_amd import _lib
    m, N, H = shapes()[i]
    if i == 5:
        assert _lib.load().mrgcn_lp_kvsall_workspace(m, N, H) >= 3 * m * 8    # three chunks, the last of one candidate
    Q, E, lists = tables(m, N, H, 100 + i, scale=0.5)
    check_case(f"shape{(m, N, H)}", Q, E, lists, eps)


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("i", [1, 2, 3], ids=[SHAPE_IDS[k] for k in (1, 2, 3)])
def test_strided_views_into_larger_tables(i, eps):
    m, N, H = shapes()[i]
    Q, E, lists = tables(m, N, H, 100 + i, scale=0.5)
    a = check_case(f"shape{(m, N, H)}", Q, E, lists, eps, pad=4)
    b = run_abi(Q, E, lists, eps, pad=0)
    for k in ("loss", "per_query", "dQ", "dE"):
        assert _np(a[k]).tobytes() == _np(b[k]).tobytes(), k


@pytest.mark.parametrize("eps", EPS)
def test_rows_scaled_to_plus_minus_200_with_positives_among_the_lowest_scores(eps):
    m, N, H = 65, 300, 20
    Q, E, lists = tables(m, N, H, 41)
    x = Q.astype(np.float64) @ E.astype(np.float64).T
    Q *= np.float32(np.sqrt(200.0 / np.abs(x).max()))
    E *= np.float32(np.sqrt(200.0 / np.abs(x).max()))
    x = Q.astype(np.float64) @ E.astype(np.float64).T
    assert x.max() > 150 and x.min() < -150
    low = x.argmin(axis=1)
    lists = [sorted(set(s) | {int(low[q])}) if s else s for q, s in enumerate(lists)]   # (query 1 stays empty)
    assert min(x[q, c] for q, s in enumerate(lists) for c in s) < -190
    assert sum(1 for q, s in enumerate(lists) for c in s if x[q, c] < -30) > m // 2
    check_case("scaled200", Q, E, lists, eps)


def test_an_upstream_scalar_and_one_gradient_only():
    m, N, H = 65, 63, 20
    Q, E, lists = tables(m, N, H, 102, scale=0.5)
    both = check_case("upstream", Q, E, lists, 0.1, gl=-2.5)
    only_q = check_case("upstream", Q, E, lists, 0.1, gl=-2.5, want=(True, False), cand=False)   # cand_* NULL
    only_e = check_case("upstream", Q, E, lists, 0.1, gl=-2.5, want=(False, True))
    assert only_q["dE"] is None and only_e["dQ"] is None
    assert torch.equal(only_q["dQ"], both["dQ"]) and torch.equal(only_e["dE"], both["dE"])


def _queries_from_lists(lists, N):
    """A `KvsAllQueries` whose tail queries have exactly the non-empty `lists`: query q is (0, q, ?)."""
    from mrgcn_amd.tasks import link_prediction as lp
    lists = [s for s in lists if s]
    facts = np.asarray([(0, q, c) for q, s in enumerate(lists) for c in s], np.int64)
    kq = lp.KvsAllQueries(facts, N, len(lists), side="tail", device="cuda")
    assert kq.m == kq.m_tail == len(lists) and kq.nnz == len(facts)
    return kq, lists


def _pairs_problem(m, N, H, seed, eps, gl):
    from mrgcn_amd.tasks import link_prediction as lp
    Q, E, lists = tables(m, N, H, seed, scale=0.5)
    keep = [q for q, s in enumerate(lists) if s]
    kq, lists = _queries_from_lists(lists, N)
    Q = np.ascontiguousarray(Q[keep])
    Qd = torch.from_numpy(Q).cuda().requires_grad_()
    Ed = torch.from_numpy(E).cuda().requires_grad_()

    def step():
        loss = lp.kvsall_pairs_loss(Qd, Ed, kq, eps)
        dQ, dE = torch.autograd.grad(loss * gl, [Qd, Ed])
        return loss.detach(), dQ, dE
    return Q, E, lists, step


def test_equal_bits_on_every_run_with_and_without_the_flag():
    import mrgcn_amd
    Q, E, lists, step = _pairs_problem(130, 300, 200, 103, 0.1, 0.75)
    before = mrgcn_amd.stats().get("lp.decoder.kvsall.fallback", 0)
    a, b, c = step(), step(), step()
    with deterministic():
        d = step()
    assert mrgcn_amd.stats().get("lp.decoder.kvsall.fallback", 0) == before
    for x, y, z, w in zip(a, b, c, d):
        assert torch.equal(x, y) and torch.equal(x, z) and torch.equal(x, w)
    ref = reference(("bits", 0.1, 0.75), Q, E, lists, 0.1, 0.75)
    for got, what in zip(a, ("loss", "dQ", "dE")):
        within("kvsall_pairs_loss", got, ref, what)


def test_a_captured_call_replays_with_equal_bits():
    Q, E, lists, step = _pairs_problem(70, 2 * _chunk() + 1, 8, 104, 0.1, 1.5)
    want = [t.clone() for t in step()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
        got = step()
    for _ in range(2):
        for t in got:
            t.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b)
    ref = reference(("captured", 0.1, 1.5), Q, E, lists, 0.1, 1.5)
    for a, what in zip(got, ("loss", "dQ", "dE")):
        within("captured", a, ref, what)


@pytest.mark.parametrize("eps", EPS)
def test_rows_of_six_floats_take_the_fallback(eps):
    import mrgcn_amd
    Q, E, lists, step = _pairs_problem(63, 65, 6, 105, eps, 1.0)
    before = mrgcn_amd.stats().get("lp.decoder.kvsall.fallback", 0)
    got = step()
    assert mrgcn_amd.stats().get("lp.decoder.kvsall.fallback", 0) == before + 1
    ref = reference(("fallback", eps, 1.0), Q, E, lists, eps, 1.0)
    for a, what in zip(got, ("loss", "dQ", "dE")):
        within("fallback", a, ref, what)


# ---- through the public interface -------------------------------------------------------------------------------------
def _emb(N, R, H, seed, n=150, ends=30):
    """Embeddings and facts whose ends come from the first `ends` nodes only: equal (s, p) and (p, o) are frequent and
    the other nodes are never an answer."""
    rng = np.random.default_rng(seed)
    E = (0.5 * rng.standard_normal((N, H))).astype(np.float32)
    Rel = (0.5 * rng.standard_normal((R, H))).astype(np.float32)
    facts = np.stack([rng.integers(0, ends, n), rng.integers(0, R, n), rng.integers(0, ends, n)], 1).astype(np.int64)
    return E, Rel, facts


def _torch_route(reps, m_tail, ptr, idx, E, Rel, eps, scorer, dt):
    """The materialised loss and its gradients to E and Rel in torch on the CPU, in `dt`."""
    import torch.nn.functional as F
    from mrgcn_amd.tasks import link_prediction as lp
    Et = torch.from_numpy(E).to(dt).requires_grad_()
    Rt = torch.from_numpy(Rel).to(dt).requires_grad_()
    r = torch.from_numpy(reps)
    q = [lp.pair_vectors(r[:m_tail], Et, Rt, "tail", scorer)[0]] if m_tail else []
    if m_tail < len(reps):
        q.append(lp.pair_vectors(r[m_tail:], Et, Rt, "head", scorer)[0])
    Q = torch.cat(q, 0)
    m, N = len(reps), E.shape[0]
    Y = torch.zeros((m, N), dtype=dt)
    Y[np.repeat(np.arange(m), np.diff(ptr)), idx.astype(np.int64)] = 1
    loss = F.binary_cross_entropy_with_logits(Q @ Et.t(), (1.0 - eps) * Y + eps / N)
    loss.backward()
    return loss.detach().numpy(), Et.grad.numpy(), Rt.grad.numpy()


def _kvsall_want(facts, E, Rel, side, scorer, eps):
    """float64 loss and gradients of E and Rel along the mirror chain (`host.kvsall_queries` -> `host.pair_vectors64`
    -> `host.kvsall_loss64`, the gradients by float64 torch autograd of the same chain) and what float32 torch on the
    CPU misses them by."""
    reps, m_tail, ptr, idx, _, _ = host.kvsall_queries(facts, E.shape[0], Rel.shape[0], side)
    out = {dt: _torch_route(reps, m_tail, ptr, idx, E, Rel, eps, scorer, dt) for dt in (torch.float64, torch.float32)}
    Q64 = np.concatenate([host.pair_vectors64(reps[:m_tail], E, Rel, "tail", scorer)[0] if m_tail else
                          np.zeros((0, E.shape[1])),
                          host.pair_vectors64(reps[m_tail:], E, Rel, "head", scorer)[0] if m_tail < len(reps) else
                          np.zeros((0, E.shape[1]))])
    loss64 = host.kvsall_loss64(Q64, E, ptr, idx, eps)[0]
    assert abs(loss64 - float(out[torch.float64][0])) <= 1e-12 * max(1.0, abs(loss64))
    names = ("loss", "dE", "dRel")
    return len(reps), dict(want=dict(zip(names, out[torch.float64])),
                           err={k: np.abs(np.asarray(a, np.float64) - b).max()
                                for k, a, b in zip(names, out[torch.float32], out[torch.float64])})


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("side", ["both", "tail", "head"])
@pytest.mark.parametrize("scorer", ["distmult", "complex"])
def test_kvsall_loss_against_the_mirror_chain(scorer, side, eps):
    import mrgcn_amd
    from mrgcn_amd.tasks import link_prediction as lp
    E, Rel, facts = _emb(97, 5, 24, 17)
    m, ref = _kvsall_want(facts, E, Rel, side, scorer, eps)
    assert m < (2 if side == "both" else 1) * len(facts)       # equal (s, p) and (p, o) were merged
    kq = lp.KvsAllQueries(facts, 97, 5, side=side, device="cuda")
    assert kq.m == m
    Ed, Rd = torch.from_numpy(E).cuda().requires_grad_(), torch.from_numpy(Rel).cuda().requires_grad_()
    before = dict(mrgcn_amd.stats())
    loss = lp.kvsall_loss(kq, Ed, Rd, label_smoothing=eps, scorer=scorer)
    loss.backward()
    after = mrgcn_amd.stats()
    assert after.get("lp.decoder.kvsall", 0) == before.get("lp.decoder.kvsall", 0) + 1
    assert after.get("lp.decoder.kvsall.fallback", 0) == before.get("lp.decoder.kvsall.fallback", 0)
    name = f"kvsall_loss-{scorer}-{side}-eps{eps}"
    within(name, loss, ref, "loss")
    within(name, Ed.grad, ref, "dE")
    within(name, Rd.grad, ref, "dRel")


def test_one_answer_per_query_is_the_one_hot_problem():
    """eps = 0 and facts in which every (s, p) and every (p, o) occurs once: the loss is the binary cross-entropy of
    the materialised one-hot problem of `pair_vectors` (the order of the queries does not enter a mean)."""
    import torch.nn.functional as F
    from mrgcn_amd.tasks import link_prediction as lp
    N, R, H, n = 97, 5, 24, 60
    rng = np.random.default_rng(19)
    E = (0.5 * rng.standard_normal((N, H))).astype(np.float32)
    Rel = (0.5 * rng.standard_normal((R, H))).astype(np.float32)
    facts = np.stack([rng.permutation(N)[:n], rng.integers(0, R, n), rng.permutation(N)[:n]], 1).astype(np.int64)
    out = {}
    for dt in (torch.float64, torch.float32):
        Et, Rt = torch.from_numpy(E).to(dt).requires_grad_(), torch.from_numpy(Rel).to(dt).requires_grad_()
        Q, tg = lp.pair_vectors(torch.from_numpy(facts), Et, Rt, "both", "distmult")
        loss = F.binary_cross_entropy_with_logits(Q @ Et.t(), F.one_hot(tg, N).to(dt))
        loss.backward()
        out[dt] = (loss.detach().numpy(), Et.grad.numpy(), Rt.grad.numpy())
    names = ("loss", "dE", "dRel")
    ref = dict(want=dict(zip(names, out[torch.float64])),
               err={k: np.abs(np.asarray(a, np.float64) - b).max()
                    for k, a, b in zip(names, out[torch.float32], out[torch.float64])})
    kq = lp.KvsAllQueries(facts, N, R, device="cuda")
    assert kq.m == 2 * n == kq.nnz
    Ed, Rd = torch.from_numpy(E).cuda().requires_grad_(), torch.from_numpy(Rel).cuda().requires_grad_()
    loss = lp.kvsall_loss(kq, Ed, Rd)
    loss.backward()
    within("one-hot", loss, ref, "loss")
    within("one-hot", Ed.grad, ref, "dE")
    within("one-hot", Rd.grad, ref, "dRel")


EPS_STEP = 0.1


def _hand_loss(E, Rel, facts, eps, scorer="distmult"):
    """torch's materialised loss over the distinct queries of `facts` (a device tensor), in float32 on the device."""
    import torch.nn.functional as F
    from mrgcn_amd.tasks import link_prediction as lp
    N, R = int(E.shape[0]), int(Rel.shape[0])
    reps, m_tail, ptr, idx, _, _ = host.kvsall_queries(_np(facts), N, R)
    r = torch.from_numpy(reps).cuda()
    Q = torch.cat([lp.pair_vectors(r[:m_tail], E, Rel, "tail", scorer)[0],
                   lp.pair_vectors(r[m_tail:], E, Rel, "head", scorer)[0]], 0)
    Y = torch.zeros((len(reps), N), device="cuda")
    rows = torch.from_numpy(np.repeat(np.arange(len(reps)), np.diff(ptr))).cuda()
    Y[rows, torch.from_numpy(idx.astype(np.int64)).cuda()] = 1
    return F.binary_cross_entropy_with_logits(Q @ E.t(), (1.0 - eps) * Y + eps / N)


def _hand_step(model, opt, E, facts, eps):
    loss = _hand_loss(E, model.relations, facts, eps)
    opt.zero_grad(set_to_none=True)
    loss.backward()
    opt.step()     # (a ClipAdam with a max_norm clips inside its step)
    return loss.detach()


def _oracle_step(sd0, facts, lr, eps):
    """One step of the tiny model with the KvsAll loss in float64 (oracle.rgcn_oracle's encoder, clip and Adam around
    `host.kvsall_loss64` and the DistMult pair vectors' own gradients) -> (loss, {name: parameter after the step})."""
    import scipy.sparse as sp
    from mrgcn_amd.data.graph_structure import adjacency_from_triples
    from oracle import rgcn_oracle as O
    A = sp.csr_matrix(adjacency_from_triples(_small()["train"], N_, P_))
    A.data = A.data.astype(np.int8).astype(np.float64)      # the reference's boundary cast (what the device tensor holds)
    st = {k: _np(v) for k, v in sd0.items()}
    Rel = st.pop("relations").astype(np.float64)
    cfgs = O.rgcn_cfgs([(0, Rel.shape[1])], 2 * P_ + 1, N_, 2, False, True)
    reps, mt, ptr, idx, _, _ = host.kvsall_queries(facts, N_, Rel.shape[0])

    def loss_fn(rows, Hm):
        assert np.array_equal(rows, np.arange(N_))
        Q = np.concatenate([host.pair_vectors64(reps[:mt], Hm, Rel, "tail")[0],
                            host.pair_vectors64(reps[mt:], Hm, Rel, "head")[0]])
        loss, _, dQ, dE = host.kvsall_loss64(Q, Hm, ptr, idx, eps)
        dR = np.zeros_like(Rel)
        for dq, f, end in ((dQ[:mt], reps[:mt], reps[:mt, 0]), (dQ[mt:], reps[mt:], reps[mt:, 2])):
            np.add.at(dE, end, dq * Rel[f[:, 1]])                # q = E[end] * Rel[p] on either side
            np.add.at(dR, f[:, 1], dq * Hm[end])
        return loss, dE, {"relations": dR}

    ora = O.rgcn_train_step_at_rows(cfgs, O.split_params(st, 1), None, A, np.arange(N_), None,
                                    sample_nodes=np.arange(N_), t=1, lr=lr, relu_last=True, loss_fn=loss_fn,
                                    extra_params={"relations": Rel})
    return ora["loss"], {"relations": ora["new_extra"]["relations"][0],
                         "layers.layer_0.weight_I_comp": ora["new"][0]["weight_I_comp"][0],
                         "layers.layer_0.weight_I": ora["new"][0]["weight_I"][0]}


def _update_within(name, before, got, hand, truth=None):
    """The measure of tests/test_gpu_lp_all.py on the parameter UPDATE (new - old) of one step: the kernel route's
    update against the float64 step's (`truth`), allowed 4 x what the hand-written float32 step (torch's materialised
    loss) misses that by, over the parameter, with a floor of one float32 ulp of the parameter the update is added to.
    Without `truth` (the masked batch, whose encoder has no float64 form here) the restatement's own error is taken
    from the number format: 4 float32 ulps of the hand-written update, the same floor."""
    for k in before:
        b, g, h = (_np(x[k]).astype(np.float64) for x in (before, got, hand))
        floor = np.spacing(np.abs(_np(hand[k])).astype(np.float32)).astype(np.float64)
        if truth is None:
            want, allow = h - b, np.maximum(4.0 * np.spacing(np.abs(h - b).astype(np.float32)), floor)
            err32 = float("nan")
        else:
            t = np.asarray(truth[k], np.float64)
            if t.shape != b.shape:      # the state dict keeps weight_I in the reference's (B N, out) layout
                nb = t.shape[1]
                b, g, h = (x.reshape(nb, -1, x.shape[-1]).transpose(1, 0, 2) for x in (b, g, h))
                floor = floor.reshape(nb, -1, floor.shape[-1]).transpose(1, 0, 2)
            want = t - b
            err32 = float(np.abs((h - b) - want).max())
            allow = np.maximum(4.0 * err32, floor)
        err = np.abs((g - b) - want)
        msg = (f"{name} {k}: kernel route's update off by {err.max():.3e}, float32 restatement {err32:.3e}, "
               f"allowance {allow.max():.3e}, update size {np.abs(want).max():.3e}")
        print(msg)
        assert np.all(err <= allow), msg


def test_train_step_equals_the_step_written_by_hand():
    import mrgcn_amd
    from mrgcn_amd.tasks import link_prediction as lp
    s = _small()
    smp = lp.NegativeSampler(s["train"], N_, 2 * P_ + 1, rate=2, seed=5)
    smp()
    buf = smp.buf.clone()
    with deterministic():
        model, opt = _model()
        before = {k: v.clone() for k, v in model.state_dict().items()}
        drawn = mrgcn_amd.stats().get("lp.negatives.keyed", 0)
        got = lp.train_step(model, _fwd(model), smp, opt, decoder="kvsall", label_smoothing=EPS_STEP)
        assert mrgcn_amd.stats().get("lp.negatives.keyed", 0) == drawn     # the sampler was not called
        assert torch.equal(smp.buf, buf)
        kq = smp._kvsall[1]
        assert isinstance(kq, lp.KvsAllQueries) and kq.m < 2 * len(s["train"])
        model2, opt2 = _model()
        want = _hand_step(model2, opt2, _fwd(model2)(), smp.facts, EPS_STEP)
    loss64, truth = _oracle_step(before, s["train"], 0.05, EPS_STEP)
    err32 = abs(float(want) - loss64)
    allow = max(4 * err32, float(np.spacing(np.float32(abs(loss64)))))
    msg = (f"train_step decoder=kvsall loss {float(got)!r}, by hand {float(want)!r}, float64 {loss64!r}: kernel route "
           f"off by {abs(float(got) - loss64):.3e}, float32 restatement {err32:.3e}, allowance {allow:.3e}")
    print(msg)
    assert abs(float(got) - loss64) <= allow, msg
    _update_within("train_step", before, model.state_dict(), model2.state_dict(), truth)


NEPOCH, INTERVAL = 6, 2


def _fit(model, opt, graphed, sampler, scorer):
    from mrgcn_amd.tasks import link_prediction as lp
    s = _small()
    return list(lp.fit(model, _fwd(model), s["train"], s["valid"], opt, NEPOCH, eval_interval=INTERVAL,
                       mrr_batchsize=100, filter_ranks=True, poll=3, graphed=graphed, sampler=sampler, warmup=3,
                       decoder="kvsall", label_smoothing=EPS_STEP, scorer=scorer))


def _rows_equal(got, want, n):
    assert len(got) == len(want) == n
    for g, w in zip(got, want):
        assert g[0] == w[0] and np.float32(g[1]).tobytes() == np.float32(w[1]).tobytes(), (g, w)
        for a, b in ((g[2], w[2]), (g[3], w[3]), (g[4], w[4]), (g[5], w[5])):
            assert (a is None) == (b is None)
            if a is not None:
                assert np.float32(a["raw"]).tobytes() == np.float32(b["raw"]).tobytes(), (g[0], a, b)
                assert np.float32(a["flt"]).tobytes() == np.float32(b["flt"]).tobytes(), (g[0], a, b)


@pytest.mark.parametrize("scorer", ["distmult", "complex"])
def test_fit_replayed_equals_eager(scorer):
    from mrgcn_amd.tasks import link_prediction as lp
    s = _small()
    facts = torch.from_numpy(s["train"]).cuda()
    with deterministic():
        model, opt = _model()
        got = _fit(model, opt, True, lp.DeviceNegativeSampler(facts), scorer)
        model2, opt2 = _model()
        smp2 = lp.DeviceNegativeSampler(facts)
        for _ in range(3):   # the capture's warm-up epochs are real steps
            model2.train()
            lp.train_step(model2, _fwd(model2), smp2, opt2, decoder="kvsall", label_smoothing=EPS_STEP, scorer=scorer)
        want = _fit(model2, opt2, False, smp2, scorer)
    print(scorer, "losses", [r[1] for r in got])
    _rows_equal(got, want, NEPOCH)
    assert got[-1][1] < got[0][1]
    for (k, a), (_, b) in zip(model.state_dict().items(), model2.state_dict().items()):
        assert torch.equal(a, b), k


def test_train_batch_step_on_a_masked_batch_equals_the_step_written_by_hand():
    from mrgcn_amd.tasks import link_prediction as lp
    from tests.test_gpu_lp_minibatch_fit import Problem
    with deterministic():
        a, b = Problem("nb13"), Problem("nb13")
        batch, facts = a.batches["train"][0]
        before = {k: v.clone() for k, v in a.model.state_dict().items()}
        got = lp.train_batch_step(a.model, batch, facts, a.opt, decoder="kvsall", label_smoothing=EPS_STEP)
        batch2, facts2 = b.batches["train"][0]
        E = lp._embed(b.model, batch2)
        f2 = lp._batch_state(batch2, facts2, E.device)["facts"]
        assert int(f2[:, [0, 2]].max()) < E.shape[0]
        kq = batch._mrgcn_lp["_kvsall"][1]
        assert kq.num_nodes == E.shape[0]        # batch-local ids, the batch's own nodes the candidates
        want = _hand_step(b.model, b.opt, E, f2, EPS_STEP)
    print("train_batch_step decoder=kvsall loss", float(got), "by hand", float(want), "nodes", E.shape[0], "facts",
          len(f2), "queries", kq.m)
    assert abs(float(got) - float(want)) <= 4 * np.spacing(np.float32(abs(float(want))))
    _update_within("train_batch_step", before, a.model.state_dict(), b.model.state_dict())


def test_fit_batches_captured_equals_eager():
    from mrgcn_amd.tasks import link_prediction as lp
    from tests.test_gpu_lp_minibatch_fit import Problem
    rows = {}
    with deterministic():
        for graphed in (True, False):
            p = Problem("nb13")
            tb = p.batches["train"][:3]
            if not graphed:   # the capture's warm-up epochs are real steps
                for _ in range(3):
                    lp.train_epoch(tb, p.model, p.opt, decoder="kvsall", label_smoothing=EPS_STEP)
            rows[graphed] = list(lp.fit_batches(p.model, tb, p.batches["valid"][:1], p.opt, 2, eval_interval=1,
                                                poll=2, graphed=graphed, warmup=3, decoder="kvsall",
                                                label_smoothing=EPS_STEP))
    print("fit_batches decoder=kvsall losses", [r[1] for r in rows[True]])
    _rows_equal(rows[True], rows[False], 2)


def test_a_capture_without_cached_queries_raises():
    """The step raises before it launches anything: the forward here hands out embeddings computed beforehand, so the
    capture that is ended by the error is empty."""
    from mrgcn_amd._lib import MrgcnError
    from mrgcn_amd.tasks import link_prediction as lp
    s = _small()
    model, opt = _model()
    with torch.no_grad():
        E = _fwd(model)().clone()
    smp = lp.DeviceNegativeSampler(torch.from_numpy(s["train"]).cuda())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert getattr(smp, "_kvsall", None) is None
    g = torch.cuda.CUDAGraph()
    with pytest.raises(MrgcnError, match="kvsall.*outside a stream capture"):
        with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
            lp.train_step(model, lambda: E, smp, opt, decoder="kvsall")
    torch.cuda.synchronize()
    assert getattr(smp, "_kvsall", None) is None
    # the same step outside a capture builds the queries and keeps them on the sampler
    lp.train_step(model, lambda: E.requires_grad_(), smp, opt, decoder="kvsall")
    assert isinstance(smp._kvsall[1], lp.KvsAllQueries)


def test_a_default_train_step_touches_no_kvsall_counter():
    import mrgcn_amd
    from mrgcn_amd.tasks import link_prediction as lp
    s = _small()
    model, opt = _model()
    smp = lp.DeviceNegativeSampler(torch.from_numpy(s["train"]).cuda())
    before = {k: v for k, v in mrgcn_amd.stats().items() if k.startswith("lp.decoder.kvsall")}
    lp.train_step(model, _fwd(model), smp, opt)
    torch.cuda.synchronize()
    after = {k: v for k, v in mrgcn_amd.stats().items() if k.startswith("lp.decoder.kvsall")}
    assert after == before
    assert getattr(smp, "_kvsall", None) is None
