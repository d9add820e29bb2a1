"""The 1-vs-all softmax decoder on the device (csrc/lp_all.hip; mrgcn_amd.tasks.link_prediction: pair_vectors, all_loss,
all_lse, decoder="all").

Bounds.  Nothing is fixed in advance: for every case the float32 restatement of the same arithmetic — `host.all_lse32`
(a float32 matmul plus a float32 logsumexp) for lse / xt / the loss, float32 torch autograd of the materialised
`F.cross_entropy(Q @ E.T, target)` on the CPU for the gradients — is measured against the float64 mirror
(`host.all_loss64`) on the same inputs, and the kernel gets 4 x that maximum error: it differs from the restatement in
summation order only (the MFMA chain is a k-ordered float32 fma chain, 0.75-1.5e-7 sum|a b|, the class of a float32
matmul).  The floor is one float32 ulp of the compared value.  No element is excluded; every assertion message carries
the measured error and the allowance."""
import ctypes as C

import numpy as np
import pytest
import torch

from mrgcn_amd import host
from tests.test_gpu_lp_fit import N_, P_, _fwd, _model, _small, deterministic

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


def _chunk():
    from mrgcn_amd import _lib
    return int(_lib.load().mrgcn_lp_all_chunk())


# ---- the kernels through the C ABI -----------------------------------------------------------------------------------
def _device_rows(a, pad):
    """`a` as a strided view (ld = H + pad) into a larger table filled with a sentinel."""
    big = torch.full((a.shape[0], a.shape[1] + pad), 7.0, dtype=torch.float32, device="cuda")
    big[:, :a.shape[1]] = torch.from_numpy(a).cuda()
    return big, big[:, :a.shape[1]]


def run_abi(Q, E, tg, gl=1.0, pad=0, want=(True, True)):
    """forward + backward through the C entries -> dict of device results (dQ / dE None when not asked for)."""
    from mrgcn_amd import _lib
    lib = _lib.load()
    m, H = Q.shape
    N = E.shape[0]
    Qb, Qd = _device_rows(Q, pad)
    Eb, Ed = _device_rows(E, pad)
    tgd = torch.from_numpy(np.asarray(tg, np.int64)).cuda()
    assert lib.mrgcn_lp_all_supported(Qd.data_ptr(), Qd.stride(0), m, Ed.data_ptr(), Ed.stride(0), N, H) == 1
    lse, xt = torch.empty(2 * m, device="cuda"), torch.empty(m, device="cuda")   # (lse: values, then remainders)
    loss = torch.empty((), device="cuda")
    nws = int(lib.mrgcn_lp_all_workspace(m, N, H))
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    gld = torch.full((1,), gl, dtype=torch.float32, device="cuda")
    dQb = torch.full((m, H + pad), 7.0, device="cuda") if want[0] else None
    dEb = torch.full((N, H + pad), 7.0, device="cuda") if want[1] else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
    _lib.check(lib.mrgcn_lp_all_fwd_f32(p(Qd), Qd.stride(0), m, p(Ed), Ed.stride(0), N, H, p(tgd), p(lse), p(xt),
                                        p(loss), p(ws), nws, st), "fwd")
    _lib.check(lib.mrgcn_lp_all_bwd_f32(p(Qd), Qd.stride(0), m, p(Ed), Ed.stride(0), N, H, p(tgd), p(lse), p(gld),
                                        p(dQb), H + pad, p(dEb), H + pad, None, 0, st), "bwd")
    torch.cuda.synchronize()
    for b in (dQb, dEb):
        if b is not None and pad:
            assert bool((b[:, H:] == 7.0).all()), "the backward wrote past a row's H columns"
    return dict(loss=loss, lse=lse[:m], xt=xt, dQ=None if dQb is None else dQb[:, :H], dE=None if dEb is None else dEb[:, :H])


_REF: dict = {}


def reference(key, Q, E, tg, gl):
    """float64 values and what the float32 restatement misses them by (computed once per case, never changed)."""
    if key not in _REF:
        import torch.nn.functional as F
        loss64, lse64, dQ64, dE64 = host.all_loss64(Q, E, tg, gl)
        xt64 = np.einsum("qh,qh->q", Q.astype(np.float64), E.astype(np.float64)[tg])
        lse32, xt32 = host.all_lse32(Q, E, tg)
        loss32 = np.mean(lse32 - xt32, dtype=np.float32)
        Qt, Et = torch.from_numpy(Q).requires_grad_(), torch.from_numpy(E).requires_grad_()
        (F.cross_entropy(Qt @ Et.t(), torch.from_numpy(np.asarray(tg, np.int64))) * np.float32(gl)).backward()
        _REF[key] = dict(
            want=dict(loss=np.float64(loss64), lse=lse64, xt=xt64, dQ=dQ64, dE=dE64),
            err=dict(loss=abs(float(loss32) - loss64), lse=np.abs(lse32 - lse64).max(), xt=np.abs(xt32 - xt64).max(),
                     dQ=np.abs(Qt.grad.numpy() - dQ64).max(), dE=np.abs(Et.grad.numpy() - dE64).max()))
    return _REF[key]


def within(name, got, ref, what):
    want, err32 = np.asarray(ref["want"][what]), float(ref["err"][what])
    got = np.asarray(_np(got), np.float64)
    assert np.all(np.isfinite(got)), f"{name} {what}: not finite"
    allow = np.maximum(4.0 * err32, np.spacing(np.abs(want).astype(np.float32)).astype(np.float64))
    err = np.abs(got - want)
    msg = (f"{name} {what}: kernel max error {err.max():.3e}, float32 restatement {err32:.3e}, "
           f"allowance {np.max(allow):.3e} (4 x restatement, floor 1 ulp)")
    print(msg)
    assert np.all(err <= allow), msg


def check_case(name, Q, E, tg, gl=1.0, pad=0, want=(True, True)):
    ref = reference(name, Q, E, tg, gl)
    out = run_abi(Q, E, tg, gl, pad, want)
    for what in ("loss", "lse", "xt") + (("dQ",) if want[0] else ()) + (("dE",) if want[1] else ()):
        within(name, out[what], ref, what)
    return out


def tables(m, N, H, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    Q = (scale * rng.standard_normal((m, H))).astype(np.float32)
    E = (scale * rng.standard_normal((N, H))).astype(np.float32)
    return Q, E, rng.integers(0, N, m).astype(np.int64)


def shapes():
    return [(1, 2, 4), (63, 65, 12), (65, 63, 20), (130, 300, 200), (257, 64, 256), (70, 2 * _chunk() + 1, 8)]


SHAPE_IDS = ["1x2x4", "63x65x12", "65x63x20", "130x300x200", "257x64x256", "70x(2C+1)x8"]


@pytest.mark.parametrize("i", range(6), ids=SHAPE_IDS)
def test_loss_lse_and_gradients_at_every_shape(i):
    m, N, H = shapes()[i]
    Q, E, tg = tables(m, N, H, 100 + i, scale=0.5)
    check_case(f"shape{(m, N, H)}", Q, E, tg, gl=1.0)


def test_one_candidate_gives_exactly_zero():
    Q, E, tg = tables(1, 1, 4, 7)
    out = run_abi(Q, E, tg)
    assert float(out["loss"]) == 0.0
    assert _np(out["lse"]).tobytes() == _np(out["xt"]).tobytes()
    assert not _np(out["dQ"]).any() and not _np(out["dE"]).any()


def test_three_chunks_the_last_one_of_one_candidate():
    from mrgcn_amd import _lib
    c = _chunk()
    m, N, H = 70, 2 * c + 1, 8
    assert _lib.load().mrgcn_lp_all_workspace(m, N, H) >= 3 * m * 8
    Q, E, _ = tables(m, N, H, 31, scale=0.7)
    tg = np.full(m, N - 1, np.int64)      # every target is the lone candidate of the last chunk
    tg[::3] = c - 1                        # ... or the last one of the first chunk
    tg[1::3] = c                           # ... or the first one of the second
    check_case("chunks", Q, E, tg)


@pytest.mark.parametrize("i", [1, 2, 3], ids=[SHAPE_IDS[k] for k in (1, 2, 3)])
def test_strided_views_into_larger_tables(i):
    m, N, H = shapes()[i]
    Q, E, tg = tables(m, N, H, 100 + i, scale=0.5)
    a = check_case(f"shape{(m, N, H)}", Q, E, tg, pad=4)
    b = run_abi(Q, E, tg, pad=0)
    for k in ("loss", "lse", "xt", "dQ", "dE"):
        assert _np(a[k]).tobytes() == _np(b[k]).tobytes(), k


@pytest.mark.parametrize("targets", ["last", "first", "repeated"])
@pytest.mark.parametrize("i", [1, 2], ids=[SHAPE_IDS[k] for k in (1, 2)])
def test_targets_at_the_edges(i, targets):
    m, N, H = shapes()[i]
    Q, E, tg = tables(m, N, H, 200 + i, scale=0.5)
    tg = {"last": np.full(m, N - 1), "first": np.zeros(m), "repeated": np.arange(m) % 3 + N // 2}[targets].astype(np.int64)
    check_case(f"targets-{targets}{(m, N, H)}", Q, E, tg)


def ordered_tables(m, N, H, rising, seed):
    """Scores that span +-200 with the candidates ordered by rising (falling) score for EVERY query: along a fixed
    direction u, E[c] = a_c u with a_c rising through [-1, 1] and Q[q] = b_q u with 0.5 <= b_q <= 1, |u|^2 = 200."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal(H)
    u *= np.sqrt(200.0) / np.linalg.norm(u)
    a = np.linspace(-1.0, 1.0, N) if N > 1 else np.ones(1)
    if not rising:
        a = a[::-1]
    b = 0.5 + 0.5 * rng.random(m)
    Q, E = (b[:, None] * u[None, :]).astype(np.float32), (a[:, None] * u[None, :]).astype(np.float32)
    x = Q.astype(np.float64) @ E.astype(np.float64).T
    assert x.max() > 150 and x.min() < -150
    d = np.diff(x, axis=1)
    assert np.all(d > 0) if rising else np.all(d < 0)
    return Q, E, rng.integers(0, N, m).astype(np.int64)


@pytest.mark.parametrize("rising", [True, False], ids=["rising", "falling"])
@pytest.mark.parametrize("i", [2, 3, 5], ids=[SHAPE_IDS[k] for k in (2, 3, 5)])
def test_scores_of_plus_minus_200_with_the_max_moving_at_every_tile(i, rising):
    m, N, H = shapes()[i]
    Q, E, tg = ordered_tables(m, N, H, rising, 300 + i)
    check_case(f"ordered-{'rising' if rising else 'falling'}{(m, N, H)}", Q, E, tg)


def test_rows_scaled_to_plus_minus_200():
    m, N, H = 65, 300, 20
    Q, E, tg = tables(m, N, H, 41)
    x = Q.astype(np.float64) @ E.astype(np.float64).T
    Q *= np.float32(np.sqrt(200.0 / np.abs(x).max()))
    E *= np.float32(np.sqrt(200.0 / np.abs(x).max()))
    assert np.abs(Q.astype(np.float64) @ E.astype(np.float64).T).max() > 190
    check_case("scaled200", Q, E, tg)


def test_an_upstream_scalar_and_one_gradient_only():
    m, N, H = 65, 63, 20
    Q, E, tg = tables(m, N, H, 102, scale=0.5)
    both = check_case("upstream", Q, E, tg, gl=-2.5)
    only_q = check_case("upstream", Q, E, tg, gl=-2.5, want=(True, False))
    only_e = check_case("upstream", Q, E, tg, gl=-2.5, want=(False, True))
    assert only_q["dE"] is None and only_e["dQ"] is None
    assert torch.equal(only_q["dQ"], both["dQ"]) and torch.equal(only_e["dE"], both["dE"])


def test_equal_bits_on_every_run_with_and_without_the_flag():
    m, N, H = 130, 300, 200
    Q, E, tg = tables(m, N, H, 103, scale=0.5)
    a, b = run_abi(Q, E, tg, gl=0.75), run_abi(Q, E, tg, gl=0.75)
    with deterministic():
        c = run_abi(Q, E, tg, gl=0.75)
    for k in ("loss", "lse", "xt", "dQ", "dE"):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k


def test_a_captured_call_replays_with_equal_bits():
    from mrgcn_amd.tasks import link_prediction as lp
    m, N, H = 70, 2 * _chunk() + 1, 8
    Q, E, tg = tables(m, N, H, 104, scale=0.5)
    Qd = torch.from_numpy(Q).cuda().requires_grad_()
    Ed = torch.from_numpy(E).cuda().requires_grad_()
    tgd = torch.from_numpy(tg).cuda()

    def step():
        loss = lp.all_pairs_loss(Qd, Ed, tgd)
        dQ, dE = torch.autograd.grad(loss * 1.5, [Qd, Ed])
        return loss.detach(), dQ, dE
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
    ref = reference("captured", Q, E, tg, 1.5)
    within("captured", got[0], ref, "loss")
    within("captured", got[1], ref, "dQ")
    within("captured", got[2], ref, "dE")


def test_all_lse_is_the_forward():
    from mrgcn_amd.tasks import link_prediction as lp
    Q, E, tg = tables(63, 65, 12, 105, scale=0.5)
    lse, xt = lp.all_lse(torch.from_numpy(Q).cuda(), torch.from_numpy(E).cuda(), torch.from_numpy(tg).cuda())
    out = run_abi(Q, E, tg)
    assert torch.equal(lse, out["lse"]) and torch.equal(xt, out["xt"])


# ---- through the public interface -------------------------------------------------------------------------------------
def _emb(N, R, H, seed):
    rng = np.random.default_rng(seed)
    E = (0.5 * rng.standard_normal((N, H))).astype(np.float32)
    Rel = (0.5 * rng.standard_normal((R, H))).astype(np.float32)
    facts = np.stack([rng.integers(0, N, 150), rng.integers(0, R, 150), rng.integers(0, N, 150)], 1).astype(np.int64)
    return E, Rel, facts


def _all_loss_want(facts, E, Rel, side, scorer):
    """float64 loss and gradients of E and Rel (float64 torch autograd through the mirror's formulas) and what float32
    torch on the CPU misses them by."""
    import torch.nn.functional as F
    out = {}
    for dt in (torch.float64, torch.float32):
        Et = torch.from_numpy(E).to(dt).requires_grad_()
        Rt = torch.from_numpy(Rel).to(dt).requires_grad_()
        from mrgcn_amd.tasks import link_prediction as lp
        Q, tg = lp.pair_vectors(torch.from_numpy(facts), Et, Rt, side, scorer)
        loss = F.cross_entropy(Q @ Et.t(), tg)
        loss.backward()
        out[dt] = (loss.detach().numpy(), Et.grad.numpy(), Rt.grad.numpy())
    Q64, tg64 = host.pair_vectors64(facts, E, Rel, side, scorer)
    loss64 = host.all_loss64(Q64, E, tg64)[0]
    assert abs(loss64 - float(out[torch.float64][0])) <= 1e-12 * max(1.0, abs(loss64))
    names = ("loss", "dE", "dRel")
    return dict(want=dict(zip(names, out[torch.float64])),
                err={k: np.abs(np.asarray(a, np.float64) - b).max()
                     for k, a, b in zip(names, out[torch.float32], out[torch.float64])})


@pytest.mark.parametrize("side", ["both", "tail", "head"])
@pytest.mark.parametrize("scorer", ["distmult", "complex"])
def test_all_loss_against_the_mirror(scorer, side):
    import mrgcn_amd
    from mrgcn_amd.tasks import link_prediction as lp
    E, Rel, facts = _emb(97, 5, 24, 17)
    ref = _all_loss_want(facts, E, Rel, side, scorer)
    Ed, Rd = torch.from_numpy(E).cuda().requires_grad_(), torch.from_numpy(Rel).cuda().requires_grad_()
    before = dict(mrgcn_amd.stats())
    loss = lp.all_loss(facts, Ed, Rd, side=side, scorer=scorer)
    loss.backward()
    after = mrgcn_amd.stats()
    assert after.get("lp.decoder.all", 0) == before.get("lp.decoder.all", 0) + 1
    assert after.get("lp.decoder.all.fallback", 0) == before.get("lp.decoder.all.fallback", 0)
    name = f"all_loss-{scorer}-{side}"
    within(name, loss, ref, "loss")
    within(name, Ed.grad, ref, "dE")
    within(name, Rd.grad, ref, "dRel")


def test_rows_of_six_floats_take_the_fallback():
    import mrgcn_amd
    from mrgcn_amd.tasks import link_prediction as lp
    E, Rel, facts = _emb(97, 5, 6, 18)
    ref = _all_loss_want(facts, E, Rel, "both", "distmult")
    Ed, Rd = torch.from_numpy(E).cuda().requires_grad_(), torch.from_numpy(Rel).cuda().requires_grad_()
    before = mrgcn_amd.stats().get("lp.decoder.all.fallback", 0)
    loss = lp.all_loss(facts, Ed, Rd)
    loss.backward()
    assert mrgcn_amd.stats().get("lp.decoder.all.fallback", 0) == before + 1
    within("fallback", loss, ref, "loss")
    within("fallback", Ed.grad, ref, "dE")
    within("fallback", Rd.grad, ref, "dRel")


def _hand_step(model, opt, E, facts, scorer="distmult"):
    import torch.nn.functional as F
    from mrgcn_amd.tasks import link_prediction as lp
    Q, tg = lp.pair_vectors(facts, E, model.relations, "both", scorer)
    loss = F.cross_entropy(Q @ E.t(), tg)
    opt.zero_grad(set_to_none=True)
    loss.backward()
    opt.step()     # (a ClipAdam with a max_norm clips inside its step)
    return loss.detach()


def _oracle_step(sd0, facts, lr):
    """One step of the tiny model with the 1-vs-all loss in float64 (oracle.rgcn_oracle's encoder, clip and Adam around
    `host.all_loss64` and the DistMult pair vectors' own gradients) -> (loss, {name: parameter after the step})."""
    import scipy.sparse as sp
    from mrgcn_amd.data.graph_structure import adjacency_from_triples
    from oracle import rgcn_oracle as O
    A = sp.csr_matrix(adjacency_from_triples(_small()["train"], N_, P_))
    A.data = A.data.astype(np.int8).astype(np.float64)      # the reference's boundary cast (what the device tensor holds)
    st = {k: _np(v) for k, v in sd0.items()}
    Rel = st.pop("relations").astype(np.float64)
    cfgs = O.rgcn_cfgs([(0, Rel.shape[1])], 2 * P_ + 1, N_, 2, False, True)
    n = len(facts)

    def loss_fn(rows, Hm):
        assert np.array_equal(rows, np.arange(N_))
        Q, tg = host.pair_vectors64(facts, Hm, Rel, "both", "distmult")
        loss, _, dQ, dE = host.all_loss64(Q, Hm, tg)
        dR = np.zeros_like(Rel)
        for dq, end in ((dQ[:n], facts[:, 0]), (dQ[n:], facts[:, 2])):    # q = E[end] * Rel[p] on either side
            np.add.at(dE, end, dq * Rel[facts[:, 1]])
            np.add.at(dR, facts[:, 1], dq * Hm[end])
        return loss, dE, {"relations": dR}

    ora = O.rgcn_train_step_at_rows(cfgs, O.split_params(st, 1), None, A, np.arange(N_), None,
                                    sample_nodes=np.arange(N_), t=1, lr=lr, relu_last=True, loss_fn=loss_fn,
                                    extra_params={"relations": Rel})
    return ora["loss"], {"relations": ora["new_extra"]["relations"][0],
                         "layers.layer_0.weight_I_comp": ora["new"][0]["weight_I_comp"][0],
                         "layers.layer_0.weight_I": ora["new"][0]["weight_I"][0]}


def _update_within(name, before, got, hand, truth=None):
    """The tolerance rule on the parameter UPDATE (new - old) of one step: the kernel route's update against the
    float64 step's (`truth`), allowed 4 x what the hand-written float32 step (the materialised
    `F.cross_entropy(Q @ E.T, target)`) misses that by, over the parameter, with a floor of one float32 ulp of the
    parameter the update is added to.  (Adam's first update is -lr g / (|g| + eps): where a gradient entry is of the
    size of eps the last bits of g move the update by far more than an ulp, in the float32 restatement as in the
    kernel route — which is why the rule measures the restatement.)  Without `truth` (the masked batch, whose encoder
    has no float64 form here) the restatement's own error is taken from the number format: 4 float32 ulps of the
    hand-written update, the same floor."""
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
        got = lp.train_step(model, _fwd(model), smp, opt, decoder="all", loss="softmax")
        assert mrgcn_amd.stats().get("lp.negatives.keyed", 0) == drawn     # the sampler was not called
        assert torch.equal(smp.buf, buf)
        model2, opt2 = _model()
        want = _hand_step(model2, opt2, _fwd(model2)(), smp.facts)
    loss64, truth = _oracle_step(before, s["train"], 0.05)
    err32 = abs(float(want) - loss64)
    allow = max(4 * err32, float(np.spacing(np.float32(abs(loss64)))))
    msg = (f"train_step decoder=all loss {float(got)!r}, by hand {float(want)!r}, float64 {loss64!r}: kernel route off by "
           f"{abs(float(got) - loss64):.3e}, float32 restatement {err32:.3e}, allowance {allow:.3e}")
    print(msg)
    assert abs(float(got) - loss64) <= allow, msg
    _update_within("train_step", before, model.state_dict(), model2.state_dict(), truth)


NEPOCH, INTERVAL = 6, 2


def _fit(model, opt, graphed, sampler, scorer):
    from mrgcn_amd.tasks import link_prediction as lp
    s = _small()
    return list(lp.fit(model, _fwd(model), s["train"], s["valid"], opt, NEPOCH, eval_interval=INTERVAL,
                       mrr_batchsize=100, filter_ranks=True, poll=3, graphed=graphed, sampler=sampler, warmup=3,
                       decoder="all", loss="softmax", scorer=scorer))


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
            lp.train_step(model2, _fwd(model2), smp2, opt2, decoder="all", loss="softmax", scorer=scorer)
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
        got = lp.train_batch_step(a.model, batch, facts, a.opt, decoder="all", loss="softmax")
        batch2, facts2 = b.batches["train"][0]
        E = lp._embed(b.model, batch2)
        f2 = lp._batch_state(batch2, facts2, E.device)["facts"]
        assert int(f2[:, [0, 2]].max()) < E.shape[0]
        want = _hand_step(b.model, b.opt, E, f2)
    print("train_batch_step decoder=all loss", float(got), "by hand", float(want), "nodes", E.shape[0], "facts", len(f2))
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
                    lp.train_epoch(tb, p.model, p.opt, decoder="all", loss="softmax")
            rows[graphed] = list(lp.fit_batches(p.model, tb, p.batches["valid"][:1], p.opt, 2, eval_interval=1,
                                                poll=2, graphed=graphed, warmup=3, decoder="all", loss="softmax"))
    print("fit_batches decoder=all losses", [r[1] for r in rows[True]])
    _rows_equal(rows[True], rows[False], 2)


def test_complex_learns_the_directed_cycle_under_the_1_vs_all_loss():
    """tests/test_gpu_lp_complex.py's 40-node directed cycle (free embeddings of width 16, Adam(lr 0.05), its 200
    steps): ComplEx trained with the 1-vs-all loss reaches a filtered tail MRR of 1.0."""
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
        loss = lp.all_loss(fd, E, Rel, scorer="complex")
        opt.zero_grad()
        loss.backward()
        opt.step()
    ranks = _np(lp.compute_ranks_fast(facts, E, Rel, filtered=True, scorer="complex"))[:N]
    mrr = float(np.mean(1.0 / ranks))
    print(f"directed cycle, decoder=all, after {CYCLE_STEPS} steps: filtered tail MRR {mrr:.4f} (loss {float(loss.detach()):.5f})")
    assert mrr == 1.0
