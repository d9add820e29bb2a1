"""The bf16 matrix-core arithmetic of the all-candidates decoders on the device (csrc/lp_tile.hpp: the bf16 tile;
mrgcn_lp_all_*_bf16, mrgcn_lp_kvsall_*_bf16; tasks.link_prediction: set_score_dtype, mm="bf16").

Forward rule (lse, xt, the loss; KvsAll's per-query sums and loss) — the rule of tests/test_gpu_lp_all.py, unchanged:
the value is the float64 mirror on the operands ROUNDED to bf16, the allowance 4 x what the float32 restatement
(`host.all_lse32`, `host.kvsall_loss32` on the rounded operands) misses it by, floor one float32 ulp.  The products
of two bf16 values are exact in float32, so the kernel differs from the restatement in summation order only.

Backward rule — per element |got - want| <= B + max(4 err32, 1 ulp) (tests/test_cpu_lp_bf16.py states and tries it):
`want` and B = 2^-8 |G| |other operand| from the mirror (`host.all_loss_bf16_64`, `host.kvsall_loss_bf16_64`), err32
what float32 torch autograd of the materialised loss on the rounded operands, on the CPU, misses `want` by.  No element
is excluded; every assertion message carries the measured error and the allowance."""
import ctypes as C

import numpy as np
import pytest
import torch

from mrgcn_amd import host
from tests.test_cpu_lp_bf16 import assert_bf16_rule, autograd32_all, autograd32_kvsall
from tests.test_gpu_lp_all import _chunk, _emb, _np, _rows_equal, ordered_tables
from tests.test_gpu_lp_fit import N_, P_, _fwd, _model, _small, deterministic
from tests.test_gpu_lp_kvsall import _dev, answer_lists, csr

pytestmark = pytest.mark.gpu
EPS = [0.0, 0.1]
SENTINEL = 0x40E0      # bf16 7.0


def shapes():
    return [(1, 2, 4), (63, 65, 12), (65, 63, 36), (130, 300, 200), (257, 64, 256), (70, 2 * _chunk() + 1, 8)]


SHAPE_IDS = ["1x2x4", "63x65x12", "65x63x36", "130x300x200", "257x64x256", "70x(2C+1)x8"]


def tables(m, N, H, seed, scale=0.5):
    rng = np.random.default_rng(seed)
    Q = (scale * rng.standard_normal((m, H))).astype(np.float32)
    E = (scale * rng.standard_normal((N, H))).astype(np.float32)
    return Q, E, rng.integers(0, N, m).astype(np.int64)


# ---- the kernels through the C ABI -----------------------------------------------------------------------------------
def bf16_rows(a, extra):
    """`a` [n, H] as a bf16 table on the device: rows of ld = Hp + extra 16-bit elements, round_bf16(a) in [0, H), zeros
    in [H, Hp), a sentinel past Hp -> (the whole table, ld)."""
    n, H = a.shape
    Hp = (H + 31) // 32 * 32
    big = np.full((n, Hp + extra), SENTINEL, np.uint16)
    big[:, :Hp] = 0
    big[:, :H] = (host.round_bf16(a).view(np.uint32) >> 16).astype(np.uint16)
    return torch.from_numpy(big.view(np.int16)).cuda(), Hp + extra


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _outputs(m, N, H, opad, want):
    dQb = torch.full((m, H + opad), 7.0, device="cuda") if want[0] else None
    dEb = torch.full((N, H + opad), 7.0, device="cuda") if want[1] else None
    return dQb, dEb


def _finish(Qt, Et, extra, dQb, dEb, H, opad):
    torch.cuda.synchronize()
    Hp = (H + 31) // 32 * 32
    for t in (Qt, Et):     # the inputs are read only
        assert bool((t[:, Hp:].view(torch.int16) == np.int16(SENTINEL)).all())
    for b in (dQb, dEb):
        if b is not None and opad:
            assert bool((b[:, H:] == 7.0).all()), "the backward wrote past a row's H columns"
    return (None if dQb is None else dQb[:, :H]), (None if dEb is None else dEb[:, :H])


def run_all(Q, E, tg, gl=1.0, extra=0, opad=0, want=(True, True)):
    from mrgcn_amd import _lib
    lib = _lib.load()
    (m, H), N = Q.shape, E.shape[0]
    (Qt, ldQ), (Et, ldE) = bf16_rows(Q, extra), bf16_rows(E, extra)
    tgd = torch.from_numpy(np.asarray(tg, np.int64)).cuda()
    assert lib.mrgcn_lp_all_supported_bf16(_p(Qt), ldQ, m, _p(Et), ldE, N, H) == 1
    lse, xt, loss = torch.empty(2 * m, device="cuda"), torch.empty(m, device="cuda"), torch.empty((), device="cuda")
    nws = int(lib.mrgcn_lp_all_workspace(m, N, H))
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    gld = torch.full((1,), gl, dtype=torch.float32, device="cuda")
    dQb, dEb = _outputs(m, N, H, opad, want)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.mrgcn_lp_all_fwd_bf16(_p(Qt), ldQ, m, _p(Et), ldE, N, H, _p(tgd), _p(lse), _p(xt), _p(loss), _p(ws),
                                         nws, st), "fwd")
    _lib.check(lib.mrgcn_lp_all_bwd_bf16(_p(Qt), ldQ, m, _p(Et), ldE, N, H, _p(tgd), _p(lse), _p(gld), _p(dQb),
                                         H + opad, _p(dEb), H + opad, None, 0, st), "bwd")
    dQ, dE = _finish(Qt, Et, extra, dQb, dEb, H, opad)
    return dict(loss=loss, lse=lse[:m], xt=xt, dQ=dQ, dE=dE)


def run_kv(Q, E, lists, eps, gl=1.0, extra=0, opad=0, want=(True, True), cand=True):
    from mrgcn_amd import _lib
    lib = _lib.load()
    (m, H), N = Q.shape, E.shape[0]
    (Qt, ldQ), (Et, ldE) = bf16_rows(Q, extra), bf16_rows(E, extra)
    ptr, idx, cptr, cqry = (_dev(a) for a in csr(lists, N))
    assert lib.mrgcn_lp_kvsall_supported_bf16(_p(Qt), ldQ, m, _p(Et), ldE, N, H) == 1
    pq, loss = torch.empty(m, device="cuda"), torch.empty((), device="cuda")
    nws = int(lib.mrgcn_lp_kvsall_workspace(m, N, H))
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    gld = torch.full((1,), gl, dtype=torch.float32, device="cuda")
    dQb, dEb = _outputs(m, N, H, opad, want)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.mrgcn_lp_kvsall_fwd_bf16(_p(Qt), ldQ, m, _p(Et), ldE, N, H, _p(ptr), _p(idx), eps, _p(pq), _p(loss),
                                            _p(ws), nws, st), "fwd")
    _lib.check(lib.mrgcn_lp_kvsall_bwd_bf16(_p(Qt), ldQ, m, _p(Et), ldE, N, H, _p(ptr), _p(idx),
                                            _p(cptr) if cand else None, _p(cqry) if cand else None, eps, _p(gld),
                                            _p(dQb), H + opad, _p(dEb), H + opad, None, 0, st), "bwd")
    dQ, dE = _finish(Qt, Et, extra, dQb, dEb, H, opad)
    return dict(loss=loss, per_query=pq, dQ=dQ, dE=dE)


_REF: dict = {}


def ref_all(key, Q, E, tg, gl):
    """The mirror's values and bounds and what the float32 restatements miss them by (once per case, never changed)."""
    if key not in _REF:
        loss, lse, xt, dQ, dE, BQ, BE = host.all_loss_bf16_64(Q, E, tg, gl)
        Qr, Er = host.round_bf16(Q), host.round_bf16(E)
        lse32, xt32 = host.all_lse32(Qr, Er, tg)
        gq, ge = autograd32_all(Q, E, tg, gl)
        _REF[key] = dict(
            want=dict(loss=np.float64(loss), lse=lse, xt=xt, dQ=dQ, dE=dE), B=dict(dQ=BQ, dE=BE),
            err=dict(loss=abs(float(np.mean(lse32 - xt32, dtype=np.float32)) - loss), lse=np.abs(lse32 - lse).max(),
                     xt=np.abs(xt32 - xt).max(), dQ=np.abs(gq - dQ).max(), dE=np.abs(ge - dE).max()))
    return _REF[key]


def ref_kv(key, Q, E, lists, eps, gl):
    if key not in _REF:
        ptr, idx, _, _ = csr(lists, E.shape[0])
        loss, pq, dQ, dE, BQ, BE = host.kvsall_loss_bf16_64(Q, E, ptr, idx, eps, gl)
        loss32, pq32 = host.kvsall_loss32(host.round_bf16(Q), host.round_bf16(E), ptr, idx, eps)
        gq, ge = autograd32_kvsall(Q, E, ptr, idx, eps, gl)
        _REF[key] = dict(
            want=dict(loss=np.float64(loss), per_query=pq, dQ=dQ, dE=dE), B=dict(dQ=BQ, dE=BE),
            err=dict(loss=abs(float(loss32) - loss), per_query=np.abs(pq32 - pq).max(), dQ=np.abs(gq - dQ).max(),
                     dE=np.abs(ge - dE).max()))
    return _REF[key]


def within(name, got, ref, what):
    """A forward value under the forward rule, a gradient under the backward rule."""
    want, err32 = np.asarray(ref["want"][what]), float(ref["err"][what])
    got = np.asarray(_np(got), np.float64)
    if what in ref["B"]:
        return assert_bf16_rule(f"{name} {what}", got, want, ref["B"][what], err32)
    assert np.all(np.isfinite(got)), f"{name} {what}: not finite"
    allow = np.maximum(4.0 * err32, np.spacing(np.abs(want).astype(np.float32)).astype(np.float64))
    err = np.abs(got - want)
    msg = (f"{name} {what}: kernel max error {err.max():.3e}, float32 restatement {err32:.3e}, allowance "
           f"{np.max(allow):.3e} (4 x restatement, floor 1 ulp), kernel / restatement {err.max() / max(err32, 1e-300):.2f}")
    print(msg)
    assert np.all(err <= allow), msg


def check_all(name, Q, E, tg, gl=1.0, extra=0, opad=0, want=(True, True)):
    ref = ref_all((name, gl), Q, E, tg, gl)
    out = run_all(Q, E, tg, gl, extra, opad, want)
    for what in ("loss", "lse", "xt") + (("dQ",) if want[0] else ()) + (("dE",) if want[1] else ()):
        within(name, out[what], ref, what)
    return out


def check_kv(name, Q, E, lists, eps, gl=1.0, extra=0, opad=0, want=(True, True), cand=True):
    ref = ref_kv((name, eps, gl), Q, E, lists, eps, gl)
    out = run_kv(Q, E, lists, eps, gl, extra, opad, want, cand)
    for what in ("loss", "per_query") + (("dQ",) if want[0] else ()) + (("dE",) if want[1] else ()):
        within(f"{name} eps={eps}", out[what], ref, what)
    return out


@pytest.mark.parametrize("i", range(6), ids=SHAPE_IDS)
def test_all_loss_lse_and_gradients_at_every_shape(i):
    m, N, H = shapes()[i]
    Q, E, tg = tables(m, N, H, 100 + i)
    if i == 5:       # three chunks: targets at the chunk edges, the last chunk of one candidate
        c = _chunk()
        tg[:] = N - 1
        tg[::3], tg[1::3] = c - 1, c
    check_all(f"all{(m, N, H)}", Q, E, tg)


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("i", range(6), ids=SHAPE_IDS)
def test_kvsall_loss_per_query_and_gradients_at_every_shape(i, eps):
    """(the lists of tests/test_gpu_lp_kvsall.py: query 1 empty, query 2 all N candidates — whole tiles listed)"""
    m, N, H = shapes()[i]
    Q, E, _ = tables(m, N, H, 100 + i)
    lists = answer_lists(m, N, 100 + i)
    if m >= 4 and N >= 4:
        assert lists[1] == [] and lists[2] == list(range(N))
    check_kv(f"kvsall{(m, N, H)}", Q, E, lists, eps)


@pytest.mark.parametrize("targets", ["last", "first", "repeated"])
@pytest.mark.parametrize("i", [1, 2], ids=[SHAPE_IDS[k] for k in (1, 2)])
def test_targets_at_the_edges(i, targets):
    m, N, H = shapes()[i]
    Q, E, tg = tables(m, N, H, 200 + i)
    tg = {"last": np.full(m, N - 1), "first": np.zeros(m), "repeated": np.arange(m) % 3 + N // 2}[targets].astype(np.int64)
    check_all(f"targets-{targets}{(m, N, H)}", Q, E, tg)


@pytest.mark.parametrize("rising", [True, False], ids=["rising", "falling"])
@pytest.mark.parametrize("i", [2, 3, 5], ids=[SHAPE_IDS[k] for k in (2, 3, 5)])
def test_scores_of_plus_minus_200_with_the_max_moving_at_every_tile(i, rising):
    m, N, H = shapes()[i]
    Q, E, tg = ordered_tables(m, N, H, rising, 300 + i)
    x = host.round_bf16(Q).astype(np.float64) @ host.round_bf16(E).astype(np.float64).T
    assert x.max() > 150 and x.min() < -150                      # the rounded operands still span it
    d = np.diff(x[:, ::64], axis=1)                              # ... and the maximum still moves at every tile
    assert np.all(d > 0) if rising else np.all(d < 0)
    check_all(f"ordered-{'rising' if rising else 'falling'}{(m, N, H)}", Q, E, tg)


def test_an_upstream_scalar_and_one_gradient_only():
    m, N, H = 65, 63, 36
    Q, E, tg = tables(m, N, H, 102)
    both = check_all("upstream", Q, E, tg, gl=-2.5)
    only_q = check_all("upstream", Q, E, tg, gl=-2.5, want=(True, False))
    only_e = check_all("upstream", Q, E, tg, gl=-2.5, want=(False, True))
    assert only_q["dE"] is None and only_e["dQ"] is None
    assert torch.equal(only_q["dQ"], both["dQ"]) and torch.equal(only_e["dE"], both["dE"])
    lists = answer_lists(m, N, 102)
    kb = check_kv("upstream", Q, E, lists, 0.1, gl=-2.5)
    kq = check_kv("upstream", Q, E, lists, 0.1, gl=-2.5, want=(True, False), cand=False)      # cand_* NULL
    ke = check_kv("upstream", Q, E, lists, 0.1, gl=-2.5, want=(False, True))
    assert torch.equal(kq["dQ"], kb["dQ"]) and torch.equal(ke["dE"], kb["dE"])


@pytest.mark.parametrize("i", [1, 2, 3], ids=[SHAPE_IDS[k] for k in (1, 2, 3)])
def test_strided_inputs_and_padded_outputs(i):
    """Input rows of Hp and of Hp + 32 elements (a sentinel past Hp), output rows of H and of H + 4 floats (a sentinel
    that must survive): the same bits either way."""
    m, N, H = shapes()[i]
    Q, E, tg = tables(m, N, H, 100 + i)
    a = check_all(f"all{(m, N, H)}", Q, E, tg, extra=32, opad=4)
    b = run_all(Q, E, tg)
    for k in ("loss", "lse", "xt", "dQ", "dE"):
        assert _np(a[k]).tobytes() == _np(b[k]).tobytes(), k
    lists = answer_lists(m, N, 100 + i)
    a = check_kv(f"kvsall{(m, N, H)}", Q, E, lists, 0.1, extra=32, opad=4)
    b = run_kv(Q, E, lists, 0.1)
    for k in ("loss", "per_query", "dQ", "dE"):
        assert _np(a[k]).tobytes() == _np(b[k]).tobytes(), k


def test_equal_bits_on_every_run_with_and_without_the_flag():
    m, N, H = 130, 300, 200
    Q, E, tg = tables(m, N, H, 103)
    lists = answer_lists(m, N, 103)
    a, b = run_all(Q, E, tg, gl=0.75), run_all(Q, E, tg, gl=0.75)
    ka, kb = run_kv(Q, E, lists, 0.1, gl=0.75), run_kv(Q, E, lists, 0.1, gl=0.75)
    with deterministic():
        c, kc = run_all(Q, E, tg, gl=0.75), run_kv(Q, E, lists, 0.1, gl=0.75)
    for k in ("loss", "lse", "xt", "dQ", "dE"):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    for k in ("loss", "per_query", "dQ", "dE"):
        assert torch.equal(ka[k], kb[k]) and torch.equal(ka[k], kc[k]), k


def _replays_with_equal_bits(step):
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
    return got


def test_a_captured_call_replays_with_equal_bits():
    from mrgcn_amd.tasks import link_prediction as lp
    m, N, H = 70, 2 * _chunk() + 1, 8
    Q, E, tg = tables(m, N, H, 104)
    Qd, Ed = torch.from_numpy(Q).cuda().requires_grad_(), torch.from_numpy(E).cuda().requires_grad_()
    tgd = torch.from_numpy(tg).cuda()

    def step():
        loss = lp.all_pairs_loss(Qd, Ed, tgd, mm="bf16")
        dQ, dE = torch.autograd.grad(loss * 1.5, [Qd, Ed])
        return loss.detach(), dQ, dE
    got = _replays_with_equal_bits(step)
    ref = ref_all(("captured", 1.5), Q, E, tg, 1.5)
    for a, what in zip(got, ("loss", "dQ", "dE")):
        within("captured all", a, ref, what)
    # the public route is the C entries on the tables the cast kernel makes
    out = run_all(Q, E, tg, gl=1.5)
    assert torch.equal(got[0], out["loss"]) and torch.equal(got[1], out["dQ"]) and torch.equal(got[2], out["dE"])
    lse, xt = lp.all_lse(Qd, Ed, tgd, mm="bf16")
    assert torch.equal(lse, out["lse"]) and torch.equal(xt, out["xt"])

    lists = [s for s in answer_lists(m, N, 104) if s]
    facts = np.asarray([(0, q, c) for q, s in enumerate(lists) for c in s], np.int64)
    kq = lp.KvsAllQueries(facts, N, len(lists), side="tail", device="cuda")
    Qk = np.ascontiguousarray(Q[:len(lists)])
    Qkd = torch.from_numpy(Qk).cuda().requires_grad_()

    def kstep():
        loss = lp.kvsall_pairs_loss(Qkd, Ed, kq, 0.1, mm="bf16")
        dQ, dE = torch.autograd.grad(loss * 1.5, [Qkd, Ed])
        return loss.detach(), dQ, dE
    got = _replays_with_equal_bits(kstep)
    ref = ref_kv(("captured", 0.1, 1.5), Qk, E, lists, 0.1, 1.5)
    for a, what in zip(got, ("loss", "dQ", "dE")):
        within("captured kvsall", a, ref, what)


# ---- through the public interface -------------------------------------------------------------------------------------
def _grads(loss, *ts):
    for t in ts:
        t.grad = None
    loss.backward()
    return [loss.detach().clone()] + [t.grad.clone() for t in ts]


@pytest.mark.parametrize("side", ["both", "tail", "head"])
@pytest.mark.parametrize("scorer", ["distmult", "complex"])
def test_all_loss_and_kvsall_loss_are_the_pair_losses_of_the_pair_vectors(scorer, side):
    import mrgcn_amd
    from mrgcn_amd.tasks import link_prediction as lp
    E, Rel, facts = _emb(97, 5, 24, 17)
    Ed, Rd = torch.from_numpy(E).cuda().requires_grad_(), torch.from_numpy(Rel).cuda().requires_grad_()
    fd = torch.from_numpy(facts).cuda()
    kq = lp.KvsAllQueries(facts, 97, 5, side=side, device="cuda")
    with deterministic():
        before = dict(mrgcn_amd.stats())
        got = _grads(lp.all_loss(fd, Ed, Rd, side=side, scorer=scorer, mm="bf16"), Ed, Rd)
        after = dict(mrgcn_amd.stats())
        for k, d in (("lp.decoder.all", 1), ("lp.decoder.all.bf16", 1), ("lp.decoder.all.fallback", 0),
                     ("lp.decoder.kvsall.bf16", 0)):
            assert after.get(k, 0) == before.get(k, 0) + d, k
        Q, tg = lp.pair_vectors(fd, Ed, Rd, side, scorer)
        want = _grads(lp.all_pairs_loss(Q, Ed, tg, mm="bf16"), Ed, Rd)
        f32 = _grads(lp.all_loss(fd, Ed, Rd, side=side, scorer=scorer), Ed, Rd)
        assert mrgcn_amd.stats().get("lp.decoder.all.bf16", 0) == after.get("lp.decoder.all.bf16", 0)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        assert not torch.equal(got[1], f32[1])           # ... and not the f32 arithmetic
        before = dict(mrgcn_amd.stats())
        got = _grads(lp.kvsall_loss(kq, Ed, Rd, 0.1, scorer=scorer, mm="bf16"), Ed, Rd)
        after = dict(mrgcn_amd.stats())
        for k, d in (("lp.decoder.kvsall", 1), ("lp.decoder.kvsall.bf16", 1), ("lp.decoder.kvsall.fallback", 0)):
            assert after.get(k, 0) == before.get(k, 0) + d, k
        mt = kq.m_tail
        q = ([lp.pair_vectors(kq.reps[:mt], Ed, Rd, "tail", scorer)[0]] if mt else []) + \
            ([lp.pair_vectors(kq.reps[mt:], Ed, Rd, "head", scorer)[0]] if mt < kq.m else [])
        want = _grads(lp.kvsall_pairs_loss(torch.cat(q, 0), Ed, kq, 0.1, mm="bf16"), Ed, Rd)
        for a, b in zip(got, want):
            assert torch.equal(a, b)


def test_rows_of_six_floats_take_the_fallback_on_rounded_operands():
    import torch.nn.functional as F
    import mrgcn_amd
    from mrgcn_amd.tasks import link_prediction as lp
    E, Rel, facts = _emb(97, 5, 6, 18)
    Ed, Rd = torch.from_numpy(E).cuda().requires_grad_(), torch.from_numpy(Rel).cuda().requires_grad_()
    fd = torch.from_numpy(facts).cuda()
    with deterministic():
        before = dict(mrgcn_amd.stats())
        got = _grads(lp.all_loss(fd, Ed, Rd, mm="bf16"), Ed, Rd)
        after = dict(mrgcn_amd.stats())
        assert after.get("lp.decoder.all.fallback", 0) == before.get("lp.decoder.all.fallback", 0) + 1
        assert after.get("lp.decoder.all.bf16", 0) == before.get("lp.decoder.all.bf16", 0) + 1
        Q, tg = lp.pair_vectors(fd, Ed, Rd)
        st = lambda X: X + (X.bfloat16().float() - X).detach()    # noqa: E731
        want = _grads(F.cross_entropy(st(Q) @ st(Ed).t(), tg), Ed, Rd)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        kq = lp.KvsAllQueries(facts, 97, 5, device="cuda")
        before = mrgcn_amd.stats().get("lp.decoder.kvsall.fallback", 0)
        got = _grads(lp.kvsall_loss(kq, Ed, Rd, 0.1, mm="bf16"), Ed, Rd)
        assert mrgcn_amd.stats().get("lp.decoder.kvsall.fallback", 0) == before + 1
        # the f32 fallback (H % 4 != 0) on operands rounded by hand is the same materialised expression
        mt = kq.m_tail
        Q = torch.cat([lp.pair_vectors(kq.reps[:mt], Ed, Rd, "tail")[0], lp.pair_vectors(kq.reps[mt:], Ed, Rd, "head")[0]])
        want = _grads(lp.kvsall_pairs_loss(st(Q), st(Ed), kq, 0.1, mm="f32"), Ed, Rd)
        for a, b in zip(got, want):
            assert torch.equal(a, b)


def _hand_step(model, opt, E, facts, kind):
    from mrgcn_amd.tasks import link_prediction as lp
    Rel = model.relations
    if kind == "all":
        Q, tg = lp.pair_vectors(facts, E, Rel, "both")
        loss = lp.all_pairs_loss(Q, E, tg, mm="bf16")
    else:
        kq = lp.KvsAllQueries(facts, int(E.shape[0]), int(Rel.shape[0]), "both")
        Q = torch.cat([lp.pair_vectors(kq.reps[:kq.m_tail], E, Rel, "tail")[0],
                       lp.pair_vectors(kq.reps[kq.m_tail:], E, Rel, "head")[0]], 0)
        loss = lp.kvsall_pairs_loss(Q, E, kq, 0.1, mm="bf16")
    opt.zero_grad(set_to_none=True)
    loss.backward()
    opt.step()     # (a ClipAdam with a max_norm clips inside its step)
    return loss.detach()


KW = {"all": dict(decoder="all", loss="softmax"), "kvsall": dict(decoder="kvsall", label_smoothing=0.1)}


@pytest.mark.parametrize("kind", ["all", "kvsall"])
def test_train_step_under_the_setting_equals_the_step_written_by_hand(kind):
    import mrgcn_amd
    from mrgcn_amd.tasks import link_prediction as lp
    s = _small()
    smp = lp.NegativeSampler(s["train"], N_, 2 * P_ + 1, rate=2, seed=5)
    prev = lp.set_score_dtype("bf16")
    try:
        with deterministic():
            model, opt = _model()
            before = mrgcn_amd.stats().get(f"lp.decoder.{kind}.bf16", 0)
            got = lp.train_step(model, _fwd(model), smp, opt, **KW[kind])
            assert mrgcn_amd.stats().get(f"lp.decoder.{kind}.bf16", 0) == before + 1
            lp.set_score_dtype("f32")                      # the hand-written step asks per call
            model2, opt2 = _model()
            want = _hand_step(model2, opt2, _fwd(model2)(), smp.facts, kind)
            model3, opt3 = _model()
            f32 = lp.train_step(model3, _fwd(model3), smp, opt3, **KW[kind])
    finally:
        lp.set_score_dtype(prev)
    assert lp.score_dtype() == "f32"
    print(f"train_step {kind}: bf16 loss {float(got)!r}, by hand {float(want)!r}, f32 arithmetic {float(f32)!r}")
    assert torch.equal(got, want)
    for (k, a), (_, b) in zip(model.state_dict().items(), model2.state_dict().items()):
        assert torch.equal(a, b), k
    assert not all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), model3.state_dict().values()))


NEPOCH, INTERVAL = 6, 2


def _fit(model, opt, graphed, sampler, kind):
    from mrgcn_amd.tasks import link_prediction as lp
    s = _small()
    return list(lp.fit(model, _fwd(model), s["train"], s["valid"], opt, NEPOCH, eval_interval=INTERVAL,
                       mrr_batchsize=100, filter_ranks=True, poll=3, graphed=graphed, sampler=sampler, warmup=3,
                       **KW[kind]))


@pytest.mark.parametrize("kind", ["all", "kvsall"])
def test_fit_replayed_equals_eager_under_bf16(kind):
    import mrgcn_amd
    from mrgcn_amd.tasks import link_prediction as lp
    s = _small()
    facts = torch.from_numpy(s["train"]).cuda()
    prev = lp.set_score_dtype("bf16")
    try:
        with deterministic():
            before = mrgcn_amd.stats().get(f"lp.decoder.{kind}.bf16", 0)
            model, opt = _model()
            got = _fit(model, opt, True, lp.DeviceNegativeSampler(facts), kind)
            assert mrgcn_amd.stats().get(f"lp.decoder.{kind}.bf16", 0) > before
            model2, opt2 = _model()
            smp2 = lp.DeviceNegativeSampler(facts)
            for _ in range(3):   # the capture's warm-up epochs are real steps
                model2.train()
                lp.train_step(model2, _fwd(model2), smp2, opt2, **KW[kind])
            want = _fit(model2, opt2, False, smp2, kind)
    finally:
        lp.set_score_dtype(prev)
    print(kind, "bf16 losses", [r[1] for r in got])
    _rows_equal(got, want, NEPOCH)
    assert got[-1][1] < got[0][1]
    for (k, a), (_, b) in zip(model.state_dict().items(), model2.state_dict().items()):
        assert torch.equal(a, b), k


def test_a_graph_captured_under_bf16_keeps_its_arithmetic():
    from mrgcn_amd.tasks import link_prediction as lp
    E, Rel, facts = _emb(97, 5, 24, 21)
    Ed, Rd = torch.from_numpy(E).cuda().requires_grad_(), torch.from_numpy(Rel).cuda().requires_grad_()
    fd = torch.from_numpy(facts).cuda()

    def step():
        loss = lp.all_loss(fd, Ed, Rd)          # no mm: the setting decides
        dE, dR = torch.autograd.grad(loss, [Ed, Rd])
        return loss.detach(), dE, dR
    with deterministic():                       # (pair_vectors' own backward adds rows: fixed order under the flag)
        f32 = [t.clone() for t in step()]
        prev = lp.set_score_dtype("bf16")
        try:
            bf16 = [t.clone() for t in step()]
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                got = step()
        finally:
            lp.set_score_dtype(prev)
        assert lp.score_dtype() == "f32"
        assert not torch.equal(f32[1], bf16[1])
        for t in got:
            t.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(got, bf16):
            assert torch.equal(a, b)
        for a, b in zip(step(), f32):           # ... while an eager call is back on the f32 kernels
            assert torch.equal(a, b)


def test_fit_batches_captured_equals_eager_under_bf16():
    from mrgcn_amd.tasks import link_prediction as lp
    from tests.test_gpu_lp_minibatch_fit import Problem
    rows = {}
    prev = lp.set_score_dtype("bf16")
    try:
        with deterministic():
            for graphed in (True, False):
                p = Problem("nb13")
                tb = p.batches["train"][:3]
                if not graphed:   # the capture's warm-up epochs are real steps
                    for _ in range(3):
                        lp.train_epoch(tb, p.model, p.opt, decoder="all", loss="softmax")
                rows[graphed] = list(lp.fit_batches(p.model, tb, p.batches["valid"][:1], p.opt, 2, eval_interval=1,
                                                    poll=2, graphed=graphed, warmup=3, decoder="all", loss="softmax"))
    finally:
        lp.set_score_dtype(prev)
    print("fit_batches decoder=all bf16 losses", [r[1] for r in rows[True]])
    _rows_equal(rows[True], rows[False], 2)


def test_complex_learns_the_directed_cycle_under_the_bf16_1_vs_all_loss():
    """tests/test_gpu_lp_complex.py's 40-node directed cycle with its 200 Adam steps, `all_loss(mm="bf16")`: a filtered
    tail MRR of exactly 1.0."""
    from mrgcn_amd.tasks import link_prediction as lp
    from tests.test_gpu_lp_complex import CYCLE_LR, CYCLE_N, CYCLE_STEPS, CYCLE_W
    N = CYCLE_N
    facts = np.stack([np.arange(N), np.zeros(N, np.int64), (np.arange(N) + 1) % N], 1).astype(np.int64)
    g = torch.Generator().manual_seed(0)
    E = (0.5 * torch.randn(N, CYCLE_W, generator=g)).cuda().requires_grad_()
    Rel = (0.5 * torch.randn(1, CYCLE_W, generator=g)).cuda().requires_grad_()
    opt = torch.optim.Adam([E, Rel], lr=CYCLE_LR)
    fd = torch.from_numpy(facts).cuda()
    for _ in range(CYCLE_STEPS):
        loss = lp.all_loss(fd, E, Rel, scorer="complex", mm="bf16")
        opt.zero_grad()
        loss.backward()
        opt.step()
    ranks = _np(lp.compute_ranks_fast(facts, E, Rel, filtered=True, scorer="complex"))[:N]
    mrr = float(np.mean(1.0 / ranks))
    print(f"directed cycle, decoder=all bf16, after {CYCLE_STEPS} steps: filtered tail MRR {mrr:.4f} "
          f"(loss {float(loss.detach()):.5f})")
    assert mrr == 1.0
