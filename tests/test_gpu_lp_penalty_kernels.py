"""The two penalty entry points of csrc/optim.hip through the C ABI: mrgcn_penalty_norm_multi_f32 (sum (g + r(p))^2,
sum |p|, sum p^2 with r(p) = l1 sgn(p) + 2 l2 p, in a fixed order) and mrgcn_adam_step_reg_multi_f32 (Adam on
(g + r(p)) scale + wd p) against float64 restatements, against themselves run again and replayed from a graph, and
against mrgcn_adam_step_multi_f32 bit for bit where the penalty is off.  Shapes: every size at which the kernels take
another path — below one 16-byte piece, odd tails, more than one block, a misaligned base (scalar path), flagged rows of
whole pieces (64) and not (66), more tensors than a launch takes, a tensor above the multi-tensor limit, no gradient."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
L1, L2 = 1e-3, 5e-3
B1, B2, EPS, STEP = 0.9, 0.999, 1e-8, 5


def _lib():
    from mrgcn_amd import _lib as L
    return L, L.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class T:
    """One tensor of a list: parameter, gradient (None: none this step), row flags (None: every row counts)."""

    def __init__(self, n, gen, rows=None, flags=None, misaligned=False, grad=True):
        def draw(lo=0.0):
            buf = torch.empty(n + 8, device="cuda")
            v = buf[1:1 + n] if misaligned else buf[:n]
            x = torch.randn(n, device="cuda", generator=gen)
            v.copy_(torch.where(x >= 0, x + lo, x - lo))
            return v
        self.n, self.rows, self.row_len = n, rows, (n // rows if rows else 0)
        self.p = draw()
        if n >= 3:   # both zeros among the parameters
            self.p[0], self.p[n // 2] = 0.0, -0.0
        self.g = draw(1e-3) if grad else None       # |g| >= 1e-3
        self.m = draw() * 0.1
        self.v = draw().abs_() * 0.01 + 1e-4        # v >= 1e-4
        self.flags = None
        if rows:
            f = torch.zeros(rows, dtype=torch.uint8, device="cuda")
            if flags == "all":
                f[:] = 1
            elif flags == "third":
                f[::3] = 1
            self.flags = f
            # the rows off the flags hold garbage that must never count
            self.g.view(rows, -1)[f == 0] = float("nan")
        assert (self.p.data_ptr() % 16 == 4) == bool(misaligned)

    def g_effective(self):
        """float64 gradient the kernels must see: zeros without a gradient and in the rows off the flags."""
        if self.g is None:
            return np.zeros(self.n)
        g = self.g.double().cpu().numpy().copy()
        if self.flags is not None:
            g.reshape(self.rows, -1)[self.flags.cpu().numpy() == 0] = 0.0
        return g

    def state(self):
        return [self.p.clone(), self.m.clone(), self.v.clone()]


def _tensors(gen, which):
    if which == "mixed":
        ts = [T(n, gen) for n in (1, 3, 255, 1029, 70001)]
        ts += [T(1029, gen, misaligned=True), T(515, gen, grad=False)]
        ts += [T(37 * w, gen, rows=37, flags=f) for w in (64, 66) for f in ("none", "all", "third")]
        return ts
    if which == "seventeen":
        return [T(n, gen) for n in (1, 3, 255, 1029, 70001, 7, 64, 4096, 4097, 33, 2, 1023, 1024, 1025, 5, 8191, 12)]
    if which == "large":
        from mrgcn_amd.optim import _MULTI_MAX_NUMEL
        return [T(_MULTI_MAX_NUMEL + 5, gen)]
    raise KeyError(which)


def _arrays(ts):
    n = len(ts)
    return (n, (C.c_void_p * n)(*[t.p.data_ptr() for t in ts]),
            (C.c_void_p * n)(*[t.g.data_ptr() if t.g is not None else None for t in ts]),
            (C.c_int64 * n)(*[t.n for t in ts]),
            (C.c_void_p * n)(*[t.flags.data_ptr() if t.flags is not None else None for t in ts]),
            (C.c_int32 * n)(*[t.row_len for t in ts]))


class Norm:
    def __init__(self):
        L, lib = _lib()
        self.out3 = torch.zeros(3, dtype=torch.float64, device="cuda")
        self.ws = torch.empty(int(lib.mrgcn_penalty_norm_workspace()) // 8, dtype=torch.float64, device="cuda")
        self.ticket = torch.zeros((), dtype=torch.int32, device="cuda")

    def __call__(self, ts, l1=L1, l2=L2):
        """The call sequence of a list: 16 tensors a launch, all into one out3."""
        L, lib = _lib()
        self.out3.zero_()
        for c0 in range(0, len(ts), 16):
            L.check(lib.mrgcn_penalty_norm_multi_f32(*_arrays(ts[c0:c0 + 16]), l1, l2, self.out3.data_ptr(),
                                                     self.ws.data_ptr(), self.ticket.data_ptr(), _stream()), "norm")
        return self.out3


def _want_sums(ts, l1, l2):
    a = b = c = 0.0
    for t in ts:
        p = t.p.double().cpu().numpy()
        x = t.g_effective() + l1 * np.sign(p) + 2.0 * l2 * p
        a, b, c = a + float((x * x).sum()), b + float(np.abs(p).sum()), c + float((p * p).sum())
    return np.asarray([a, b, c])


@pytest.mark.parametrize("which", ["mixed", "seventeen", "large"])
def test_sums_against_float64_same_bits_every_call_and_in_a_replay(which):
    gen = torch.Generator(device="cuda").manual_seed(3)
    ts = _tensors(gen, which)
    norm = Norm()
    want = _want_sums(ts, L1, L2)
    got = [norm(ts).cpu().numpy().copy() for _ in range(3)]
    print(which, "sums", got[0].tolist(), "float64", want.tolist(), "relative", (np.abs(got[0] - want) / want).tolist())
    assert int(norm.ticket) == 0
    # the tolerance of test_clip_adam_norm_bitwise_and_vs_float64: 1e-5 of the norm; the two penalty sums likewise
    assert abs(np.sqrt(got[0][0]) - np.sqrt(want[0])) < 1e-5 * np.sqrt(want[0])
    assert np.all(np.abs(got[0][1:] - want[1:]) < 1e-5 * want[1:])
    assert got[0].tobytes() == got[1].tobytes() == got[2].tobytes()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        norm(ts)
    norm.out3.fill_(-1.0)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert norm.out3.cpu().numpy().tobytes() == got[0].tobytes()
    # without a penalty the first sum is the gradient's own squared norm
    zero = norm(ts, 0.0, 0.0).cpu().numpy()
    plain = sum(float((t.g_effective() ** 2).sum()) for t in ts)
    assert abs(np.sqrt(zero[0]) - np.sqrt(plain)) < 1e-5 * np.sqrt(plain)


def _adam_reg(ts, l1, l2, lrs, wds, coef, bc=None):
    L, lib = _lib()
    for c0 in range(0, len(ts), 16):
        part = ts[c0:c0 + 16]
        n = len(part)
        L.check(lib.mrgcn_adam_step_reg_multi_f32(
            *_arrays(part), (C.c_void_p * n)(*[t.m.data_ptr() for t in part]),
            (C.c_void_p * n)(*[t.v.data_ptr() for t in part]), (C.c_float * n)(*lrs[c0:c0 + 16]),
            (C.c_float * n)(*wds[c0:c0 + 16]), l1, l2, B1, B2, EPS, STEP, bc.data_ptr() if bc is not None else None,
            coef.data_ptr(), _stream()), "adam_reg")


def _hyper(ts):
    return [0.01 * (1 + i % 3) for i in range(len(ts))], [0.0 if i % 2 else 5e-4 for i in range(len(ts))]


@pytest.mark.parametrize("which", ["mixed", "seventeen", "large"])
def test_adam_against_float64(which):
    gen = torch.Generator(device="cuda").manual_seed(4)
    ts = _tensors(gen, which)
    lrs, wds = _hyper(ts)
    coef = torch.tensor(0.37, device="cuda")
    f32 = lambda x: float(np.float32(x))  # noqa: E731  (the constants as the kernel holds them)
    b1, b2, eps, sc = f32(B1), f32(B2), f32(EPS), f32(0.37)
    # (the bias corrections come from the float32 betas, in double, as the host side of the entry point computes them:
    # 1 - 0.999f^5 differs from 1 - 0.999^5 by 1.3e-5 of itself)
    bc1, bc2s = f32(1.0 - b1 ** STEP), f32(np.sqrt(1.0 - b2 ** STEP))
    want = []
    for t, lr, wd in zip(ts, lrs, wds):
        p, m, v = (x.double().cpu().numpy() for x in (t.p, t.m, t.v))
        gg = (t.g_effective() + f32(L1) * np.sign(p) + f32(2 * np.float32(L2)) * p) * sc + f32(wd) * p
        m = b1 * m + (1 - b1) * gg
        v = b2 * v + (1 - b2) * gg * gg
        want.append((p - f32(lr) / bc1 * (m / (np.sqrt(v) / bc2s + eps)), m, v))
    _adam_reg(ts, L1, L2, lrs, wds, coef)
    worst = 0.0
    for t, w in zip(ts, want):
        for name, a, b in zip("pmv", (t.p, t.m, t.v), w):
            a = a.double().cpu().numpy()
            assert np.isfinite(a).all(), (t.n, name)
            worst = max(worst, float((np.abs(a - b) / (1e-7 + 1e-5 * np.abs(b))).max()))
            np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-7, err_msg=f"{name} of a tensor of {t.n}")
    print(which, "worst error in units of the tolerance", worst)


def _adam_multi(ts, grads, lrs, wds, coef, bc=None):
    L, lib = _lib()
    for c0 in range(0, len(ts), 16):
        part, gs = ts[c0:c0 + 16], grads[c0:c0 + 16]
        n = len(part)
        arr = lambda ptrs: (C.c_void_p * n)(*ptrs)  # noqa: E731
        L.check(lib.mrgcn_adam_step_multi_f32(
            n, arr([t.p.data_ptr() for t in part]), arr([g.data_ptr() for g in gs]),
            arr([t.m.data_ptr() for t in part]), arr([t.v.data_ptr() for t in part]),
            (C.c_int64 * n)(*[t.n for t in part]), (C.c_float * n)(*lrs[c0:c0 + 16]),
            (C.c_float * n)(*wds[c0:c0 + 16]), B1, B2, EPS, STEP, bc.data_ptr() if bc is not None else None,
            coef.data_ptr(), _stream()), "adam_multi")


@pytest.mark.parametrize("which,device_bias", [("mixed", False), ("seventeen", True), ("large", False)])
def test_adam_without_penalty_is_the_multi_tensor_adam_bit_for_bit(which, device_bias):
    """l1 = l2 = 0: no flags -> mrgcn_adam_step_multi_f32's bits; flags -> its bits on the gradient with the rows off
    the flags zeroed (and on zeros without a gradient)."""
    coef = torch.tensor(0.37, device="cuda")
    bc = torch.tensor([1.0 - B1 ** STEP, float(np.sqrt(1.0 - B2 ** STEP))], device="cuda") if device_bias else None
    a = _tensors(torch.Generator(device="cuda").manual_seed(5), which)
    b = _tensors(torch.Generator(device="cuda").manual_seed(5), which)
    assert all(torch.equal(x.p, y.p) and torch.equal(x.v, y.v) for x, y in zip(a, b))
    lrs, wds = _hyper(a)
    before = [t.p.clone() for t in a]
    _adam_reg(a, 0.0, 0.0, lrs, wds, coef, bc)
    grads = [torch.from_numpy(t.g_effective()).float().cuda() for t in b]
    _adam_multi(b, grads, lrs, wds, coef, bc)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        for name, u, w in zip("pmv", x.state(), y.state()):
            assert u.cpu().numpy().tobytes() == w.cpu().numpy().tobytes(), (x.n, x.row_len, name)
    assert all(not torch.equal(x.p, p0) for x, p0 in zip(a, before))   # (a step was taken)


def test_refusals():
    L, lib = _lib()
    gen = torch.Generator(device="cuda").manual_seed(6)
    norm = Norm()
    big = [T(70001, gen)]
    with pytest.raises(L.MrgcnError):   # negative lambdas
        norm(big, -1.0, 0.0)
    t = T(37 * 64, gen, rows=37, flags="all")
    t.row_len = 60   # does not divide the size
    with pytest.raises(L.MrgcnError):
        norm([t])
    assert int(norm.ticket) == 0
