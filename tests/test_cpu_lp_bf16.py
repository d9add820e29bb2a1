"""The bf16 score arithmetic of the all-candidates decoders without a device: `host.round_bf16` against torch's bf16
bit for bit, the new C entries' declarations and bindings, the `set_score_dtype` setting, and the gradient bound of the
float64 mirrors (`host.all_loss_bf16_64`, `host.kvsall_loss_bf16_64`) tried on a torch CPU emulation of the kernels'
arithmetic — rounded operands, a float32 product, G rounded to bf16, the straight-through backward.

The backward rule (tests/test_gpu_lp_bf16.py applies the same function to the kernels): per element
    |got - want| <= B + max(4 err32, 1 ulp)
with `want` the float64 gradient on the rounded operands (G not rounded), B = 2^-8 |G| |other operand| what rounding G
to bf16 can move the element by (2^-8: bf16's unit roundoff, 8 significand bits), err32 what float32 torch autograd of
the materialised loss on the rounded operands misses `want` by (its maximum), the floor one float32 ulp of `want`."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from mrgcn_amd import _lib, host
from mrgcn_amd.tasks import link_prediction as lp
from tests.test_cpu_host import ROOT, header_functions

NAMES = ("mrgcn_lp_all_supported_bf16", "mrgcn_lp_all_fwd_bf16", "mrgcn_lp_all_bwd_bf16",
         "mrgcn_lp_kvsall_supported_bf16", "mrgcn_lp_kvsall_fwd_bf16", "mrgcn_lp_kvsall_bwd_bf16")
CTYPE = {"int32_t": C.c_int32, "int64_t": C.c_int64, "int": C.c_int, "double": C.c_double}
SHAPES = [(63, 65, 12), (65, 63, 36), (130, 300, 200), (257, 64, 256)]
EPS = 0.1


# ---- round_bf16 -------------------------------------------------------------------------------------------------------
def _f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def test_round_bf16_equals_torchs_bf16_bit_for_bit():
    rng = np.random.default_rng(0)
    hi = rng.integers(0x0080, 0x7f7f, 64).astype(np.uint32) << 16     # finite bf16 values of either parity
    cases = {
        "normals": rng.standard_normal(4096).astype(np.float32) * np.float32(3.0),
        "ties to an even and to an odd neighbour": _f32(np.concatenate([hi | 0x8000, (hi | 0x8000) ^ 0x80000000])),
        "just off a tie": _f32(np.concatenate([hi | 0x7fff, hi | 0x8001])),
        "zeros": np.asarray([0.0, -0.0], np.float32),
        "denormals": _f32([1, 0x7fff, 0x8000, 0x18000, 0x28000, 0x7fffff, 0x80000001, 0x807fffff]),
        "the largest finite float32": np.asarray([np.finfo(np.float32).max, -np.finfo(np.float32).max], np.float32),
    }
    parities = (hi >> 16) & 1
    assert parities.min() == 0 and parities.max() == 1
    for name, a in cases.items():
        assert not np.isnan(a).any()
        got = host.round_bf16(a)
        want = torch.from_numpy(a.copy()).bfloat16().float().numpy()
        assert got.dtype == np.float32 and got.shape == a.shape
        assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist(), name
        assert not (got.view(np.uint32) & 0xffff).any(), name
    assert np.isinf(host.round_bf16(cases["the largest finite float32"])).all()
    two_d = rng.standard_normal((5, 7)).astype(np.float32)
    assert host.round_bf16(two_d).shape == (5, 7)
    assert np.array_equal(two_d, two_d.copy()) and host.round_bf16(two_d) is not two_d      # the input is not written


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def _header_signature(name):
    src = open(os.path.join(ROOT, "include", "mrgcn_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in the header"
    args = [C.c_void_p if "*" in a else CTYPE[a.replace("const ", "").split()[0]]
            for a in (x.strip() for x in m.group(2).split(","))]
    return CTYPE[m.group(1)], args


def test_new_entries_are_declared_exported_and_bound_with_the_headers_arguments():
    declared = set(header_functions())
    lib = _lib.load()
    for n in NAMES:
        assert n in declared, f"{n} is not declared in include/mrgcn_hip.h"
        assert n in _lib.SIGNATURES, f"{n} is not in the ctypes table"
        assert hasattr(lib, n), f"{n} is not exported by the library"
        res, args = _header_signature(n)
        assert _lib.SIGNATURES[n][0] is res, n
        assert list(_lib.SIGNATURES[n][1]) == args, n
        f32 = n.replace("supported_bf16", "supported").replace("_bf16", "_f32")     # the same contract as the f32 entry
        assert list(_lib.SIGNATURES[n][1]) == list(_lib.SIGNATURES[f32][1]), (n, f32)


def test_supported_rule_and_bad_arguments():
    lib = _lib.load()
    a = np.zeros((16, 64), np.uint16)
    base = a.ctypes.data // 16 * 16 + 16
    for ok in (lib.mrgcn_lp_all_supported_bf16, lib.mrgcn_lp_kvsall_supported_bf16):
        assert ok(base, 32, 4, base, 32, 4, 8) == 1
        assert ok(base, 64, 4, base, 32, 4, 32) == 1
        assert ok(base, 32, 4, base, 32, 4, 6) == 0        # H % 4
        assert ok(base, 288, 4, base, 288, 4, 260) == 0    # H > 256
        assert ok(base, 32, 4, base, 32, 4, 36) == 0       # ld < Hp = 64
        assert ok(base, 40, 4, base, 32, 4, 8) == 0        # a stride that is no multiple of 32
        assert ok(base + 8, 32, 4, base, 32, 4, 8) == 0    # a base that is not 16-byte aligned
        assert ok(base, 32, 0, base, 32, 4, 8) == 0 and ok(base, 32, 4, base, 32, 1 << 31, 8) == 0
        assert ok(None, 32, 4, base, 32, 4, 8) == 0
    assert lib.mrgcn_lp_all_fwd_bf16(None, 32, 4, None, 32, 4, 8, None, None, None, None, None, 0, None) != 0
    assert b"NULL" in lib.mrgcn_last_error()
    assert lib.mrgcn_lp_all_fwd_bf16(base, 40, 4, base, 32, 4, 8, base, base, base, base, base, 1 << 20, None) != 0
    assert b"shape" in lib.mrgcn_last_error()
    assert lib.mrgcn_lp_all_fwd_bf16(base, 32, 4, base, 32, 4, 8, base, base, base, base, base, 16, None) != 0
    assert b"workspace" in lib.mrgcn_last_error()
    assert lib.mrgcn_lp_all_bwd_bf16(base, 32, 4, base, 32, 4, 8, base, base, base, base, 4, base, 8, None, 0, None) != 0
    assert b"lddQ" in lib.mrgcn_last_error()
    assert lib.mrgcn_lp_kvsall_fwd_bf16(base, 32, 4, base, 32, 4, 8, base, base, 1.0, None, base, base, 1 << 20,
                                        None) != 0
    assert b"label_smoothing" in lib.mrgcn_last_error()
    assert lib.mrgcn_lp_kvsall_bwd_bf16(base, 32, 4, base, 32, 4, 8, base, base, None, None, 0.0, base, None, 8, base, 8,
                                        None, 0, None) != 0
    assert b"NULL" in lib.mrgcn_last_error()


# ---- the setting ------------------------------------------------------------------------------------------------------
def test_set_score_dtype_returns_the_previous_value_and_rejects_anything_else():
    from mrgcn_amd._lib import MrgcnError
    assert lp.score_dtype() == "f32"
    try:
        assert lp.set_score_dtype("bf16") == "f32" and lp.score_dtype() == "bf16"
        assert lp.set_score_dtype("bf16") == "bf16"
        assert lp.set_score_dtype("f32") == "bf16" and lp.score_dtype() == "f32"
        for bad in ("fp16", "BF16", None, 16):
            with pytest.raises(MrgcnError, match="'f32', 'bf16'"):
                lp.set_score_dtype(bad)
            assert lp.score_dtype() == "f32"
    finally:
        lp.set_score_dtype("f32")
    E, Rel = torch.zeros(5, 8), torch.zeros(2, 8)
    facts = torch.zeros((3, 3), dtype=torch.int64)
    with pytest.raises(MrgcnError, match="mm is one of"):
        lp.all_loss(facts, E, Rel, mm="fp8")
    with pytest.raises(MrgcnError, match="mm is one of"):
        lp.all_pairs_loss(E, E, facts[:, 0], mm="fp8")
    with pytest.raises(MrgcnError, match="GPU"):
        lp.all_loss(facts, E, Rel, mm="bf16")                                # no CPU decoder in either arithmetic
    assert lp._Decoder._fields == ("kind", "loss", "pos_weight", "scorer", "label_smoothing")


# ---- the bound, tried on a CPU emulation of the kernels' arithmetic ---------------------------------------------------
def bf16_rule(name, got, want, B, err32):
    """-> (max error, max allowance, max error / allowance) under the backward rule; asserts nothing."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    allow = np.asarray(B, np.float64) + np.maximum(4.0 * float(err32),
                                                   np.spacing(np.abs(want).astype(np.float32)).astype(np.float64))
    err = np.abs(got - want)
    return float(err.max()), float(allow.max()), float((err / allow).max())


def assert_bf16_rule(name, got, want, B, err32):
    assert np.all(np.isfinite(np.asarray(got, np.float64))), f"{name}: not finite"
    err, allow, ratio = bf16_rule(name, got, want, B, err32)
    msg = (f"{name}: max error {err:.3e}, allowance up to {allow:.3e} (B + max(4 x {float(err32):.3e}, 1 ulp)), "
           f"max error / allowance {ratio:.3f}")
    print(msg)
    assert ratio <= 1.0, msg
    return ratio


def tables(m, N, H, seed):
    g = torch.Generator().manual_seed(seed)
    Q, E = 0.5 * torch.randn(m, H, generator=g), 0.5 * torch.randn(N, H, generator=g)
    return Q.numpy(), E.numpy(), torch.randint(0, N, (m,), generator=g).numpy().astype(np.int64)


def answer_lists(m, N, seed):
    rng = np.random.default_rng(seed)
    lists = [sorted(rng.choice(N, size=int(rng.integers(0, 6)), replace=False).tolist()) for _ in range(m)]
    lists[min(2, m - 1)] = list(range(N))
    ptr = np.concatenate([[0], np.cumsum([len(s) for s in lists])]).astype(np.int64)
    return ptr, np.asarray([c for s in lists for c in s], np.int32)


def _bf(t):
    return t.bfloat16().float()


def emulate_all(Q, E, tg, gl, drop_last=False):
    """The kernels' 1-vs-all arithmetic in torch on the CPU -> (dQ, dE) as float32 arrays."""
    Qr, Er = _bf(torch.from_numpy(Q)), _bf(torch.from_numpy(E))
    tgt = torch.from_numpy(tg)
    x = Qr @ Er.t()
    G = torch.exp(x - torch.logsumexp(x, 1, keepdim=True))
    G[torch.arange(len(tg)), tgt] -= 1.0
    Gr = _bf(G * (np.float32(gl) / np.float32(len(tg))))
    dQ = Gr[:, :-1] @ Er[:-1] if drop_last else Gr @ Er
    return dQ.numpy(), (Gr.t() @ Qr).numpy()


def emulate_kvsall(Q, E, ptr, idx, eps, gl, drop_last=False):
    Qr, Er = _bf(torch.from_numpy(Q)), _bf(torch.from_numpy(E))
    m, N = Q.shape[0], E.shape[0]
    Y = torch.zeros((m, N))
    Y[np.repeat(np.arange(m), np.diff(ptr)), idx.astype(np.int64)] = 1
    x = Qr @ Er.t()
    Gr = _bf((torch.sigmoid(x) - ((1.0 - eps) * Y + eps / N)) * (np.float32(gl) / np.float32(m * N)))
    dQ = Gr[:, :-1] @ Er[:-1] if drop_last else Gr @ Er
    return dQ.numpy(), (Gr.t() @ Qr).numpy()


def autograd32_all(Q, E, tg, gl):
    """float32 torch autograd of the materialised loss on the ROUNDED operands -> (dQ, dE)."""
    import torch.nn.functional as F
    Qt = torch.from_numpy(host.round_bf16(Q)).requires_grad_()
    Et = torch.from_numpy(host.round_bf16(E)).requires_grad_()
    (F.cross_entropy(Qt @ Et.t(), torch.from_numpy(tg)) * np.float32(gl)).backward()
    return Qt.grad.numpy(), Et.grad.numpy()


def autograd32_kvsall(Q, E, ptr, idx, eps, gl):
    import torch.nn.functional as F
    m, N = Q.shape[0], E.shape[0]
    Y = torch.zeros((m, N))
    Y[np.repeat(np.arange(m), np.diff(ptr)), idx.astype(np.int64)] = 1
    Qt = torch.from_numpy(host.round_bf16(Q)).requires_grad_()
    Et = torch.from_numpy(host.round_bf16(E)).requires_grad_()
    (F.binary_cross_entropy_with_logits(Qt @ Et.t(), (1.0 - eps) * Y + eps / N) * np.float32(gl)).backward()
    return Qt.grad.numpy(), Et.grad.numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_the_all_bound_holds_for_the_emulation_and_rejects_a_dropped_candidate(shape):
    m, N, H = shape
    Q, E, tg = tables(m, N, H, 500 + H)
    loss, lse, xt, dQ, dE, BQ, BE = host.all_loss_bf16_64(Q, E, tg, 1.0)
    assert dQ.shape == BQ.shape == (m, H) and dE.shape == BE.shape == (N, H) and lse.shape == xt.shape == (m,)
    assert (BQ >= 0).all() and (BE >= 0).all()
    # the mirror is all_loss64 on the rounded operands
    l2, lse2, dQ2, dE2 = host.all_loss64(host.round_bf16(Q), host.round_bf16(E), tg, 1.0)
    assert loss == l2 and np.array_equal(lse, lse2) and np.array_equal(dQ, dQ2) and np.array_equal(dE, dE2)
    gq, ge = autograd32_all(Q, E, tg, 1.0)
    eq, ee = np.abs(gq - dQ).max(), np.abs(ge - dE).max()
    emq, eme = emulate_all(Q, E, tg, 1.0)
    assert_bf16_rule(f"all {shape} dQ", emq, dQ, BQ, eq)
    assert_bf16_rule(f"all {shape} dE", eme, dE, BE, ee)
    bad, _ = emulate_all(Q, E, tg, 1.0, drop_last=True)
    ratio = bf16_rule("dropped", bad, dQ, BQ, eq)[2]
    print(f"all {shape}: dQ without the last candidate is {ratio:.1f} x the allowance")
    assert ratio > 1.0


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_the_kvsall_bound_holds_for_the_emulation_and_rejects_a_dropped_candidate(shape):
    m, N, H = shape
    Q, E, _ = tables(m, N, H, 600 + H)
    ptr, idx = answer_lists(m, N, 600 + H)
    loss, pq, dQ, dE, BQ, BE = host.kvsall_loss_bf16_64(Q, E, ptr, idx, EPS, 1.0)
    assert dQ.shape == BQ.shape == (m, H) and dE.shape == BE.shape == (N, H) and pq.shape == (m,)
    l2, pq2, dQ2, dE2 = host.kvsall_loss64(host.round_bf16(Q), host.round_bf16(E), ptr, idx, EPS, 1.0)
    assert loss == l2 and np.array_equal(pq, pq2) and np.array_equal(dQ, dQ2) and np.array_equal(dE, dE2)
    gq, ge = autograd32_kvsall(Q, E, ptr, idx, EPS, 1.0)
    eq, ee = np.abs(gq - dQ).max(), np.abs(ge - dE).max()
    emq, eme = emulate_kvsall(Q, E, ptr, idx, EPS, 1.0)
    assert_bf16_rule(f"kvsall {shape} dQ", emq, dQ, BQ, eq)
    assert_bf16_rule(f"kvsall {shape} dE", eme, dE, BE, ee)
    bad, _ = emulate_kvsall(Q, E, ptr, idx, EPS, 1.0, drop_last=True)
    ratio = bf16_rule("dropped", bad, dQ, BQ, eq)[2]
    print(f"kvsall {shape}: dQ without the last candidate is {ratio:.1f} x the allowance")
    assert ratio > 1.0
