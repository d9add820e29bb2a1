"""The forward relation transform (mrgcn_rel_transform_fwd_f32 / _bf16, mrgcn_support_rel_transform_fwd_f32) and the
wide segment sums of its input gradient, every kernel form against a float64 restatement written here:

    ref[c] = X64[node_c, :K] @ W64[rel_c]        node_c, rel_c from ULCOL; row c (operand_order = 0) or MPOS[c]

Tolerance (derived, not tuned): any summation order of K products rounded to f32 obeys
    |got - ref| <= 2 K 2^-24 sum_k |x_k| |w_k|   per element (the sum taken in float64; the factor 2 covers fused and
pairwise orders alike), plus 2^-8 |ref| for the one round-to-nearest-even of a bf16 store.  A dropped, doubled or
misplaced term is of order 1.

Which parameter values reach which instantiation (csrc/rgcn_fused.hip: rel_transform_fwd_impl, csrc/xform_mfma.hip:
xform_cols_lds / xform_mfma_fwd_one); `_form` below restates the dispatch and names the form in every failure:

  k_xform_cols_lds<KT>      switches at their defaults, K, F, ldOut <= 16 (tests 2, 4, 5)
      KT = 4   K in {1, 2, 3} (the K < 4 branch), 4          KT = 12  K in {9, 12}
      KT = 8   K in {5, 8}                                     KT = 16  K in {13, 15, 16}
      table copy by 16 bytes: F in {4, 12, 16} with W aligned; element-wise: every other F, and W one float
      into a larger buffer;  16-byte row stores: 4q + 4 <= ldOut; element-wise: ldOut = F in {1, 3, 10, 11}, bf16
  k_xform_mfma_fwd<NT, false, KS>   xform_cols_lds = 0 (tests 1, 4, 5), or K > 16 / F > 16; always in the support
                                    form (test 6: NT = 1, and 2 for F = 16 with ldT 20; both sides of every KS boundary)
      NT = min(4, ceil(ldOut / 16)), ldOut in {roundup4(F), roundup4(F) + 4}:
          1: F in {1, 10}, F = 16 with ldOut 16;   2: F = 16 with ldOut 20, F = 17, F = 32 with ldOut 32;
          3: F = 32 with ldOut 36, F = 33, F = 48 with ldOut 48;
          4: F = 48 with ldOut 52, F in {49, 64} (F = 64 with ldOut 68: the zero tail past the tiles)
      NT = 1, KS by ceil(K / 16):  1: K <= 16 (K in {1, 2, 3}: the tiny branch);  2: 17..32;  3: 33, 48;  4: 49, 64;
                                   6: 65, 96;  8: 97, 128;  10: 129, 160;  12: 161, 192;  16: 193, 255, 256
      NT > 1, KS:  1: K in {3, 5, 16} (and the K <= 16 of F = 16, ldOut 20);  4: 17, 64 (17..64);  16: 65, 256 (65..256)
      the shifted last piece: every K % 4 != 0 with K >= 4;  partial tiles, sweeps and chunks: the fixture's
      relations of 1, 15, 16, 17, 63, 64, 65, 127, 1023, 1024, 1025 and 2100 columns
  k_xform_fwd               K in {257, 300}, and any shape with xform_mfma = xform_cols_lds = 0 (tests 3, 4); F > 64 is
                            refused by the entry point and served in slices of W's columns (F = 64: the kernel's limit)
  segment sums (test 7), through mrgcn_support_rel_transform_bwd_f32 (NLPTR, every node) and
  mrgcn_support_rel_transform_bwd_compact_f32 (LNPTR, live nodes):
      k_segment_sum<false>  K in {17, 64};  k_segment_sum_wide<2> {65, 128};  <3> {129, 192};  <4> {193, 256}
"""
import contextlib

import numpy as np
import pytest
import torch

from tests import util
from tests.test_gpu_plan_spmm import _plan_from_coo

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # unit roundoff of f32
SENTINEL = -7.25        # exact in f32 and bf16; no product of standard normals lands on it
GUARD = 96              # elements behind the output that must keep the sentinel (besides one extra row)

N, R = 3000, 14
HUB_REL, HUB_NODE, HUB_ROWS = 6, 1234, 400
# distinct touched columns per relation: an empty relation, single and partial 16-column tiles, the 4-wave x 16 sweep
# boundary, one / one-plus-one / three chunks of kRelChunk = 1024, and a relation of a few hundred with the hub node
COUNTS = (17, 1024, 0, 1, 2100, 15, 300, 16, 63, 1025, 64, 65, 127, 1023)


def _roundup4(x):
    return (x + 3) // 4 * 4


class _Graph:
    pass


def _index_graph(g, rows, cols, vals, n_rows, n_nodes, n_rel):
    g.plan = _plan_from_coo(rows, cols, vals, n_rows, n_nodes, n_rel)
    g.ref = util.numpy_plan(rows, cols, vals, n_rows, n_nodes, n_rel)
    g.ncols = g.ref["ncols"]
    ul = g.ref["ulcol"].astype(np.int64)
    g.rel, g.node = ul // n_nodes, ul % n_nodes
    g.mpos = g.ref["mpos"].astype(np.int64)
    relptr, rperm = g.ref["relptr"], g.ref["rperm"]
    g.place = np.empty(g.ncols, dtype=np.int64)     # position of a column inside its relation's walk
    for r in range(n_rel):
        g.place[rperm[relptr[r]:relptr[r + 1]]] = np.arange(relptr[r + 1] - relptr[r])
    g.cases = {}


@pytest.fixture(scope="module")
def graph():
    from mrgcn_amd import _lib as L
    rng = np.random.default_rng(20240607)
    nodes, rels = [], []
    for r, n in enumerate(COUNTS):
        pick = rng.choice(N, n, replace=False)
        if r == HUB_REL and HUB_NODE not in pick:
            pick[0] = HUB_NODE
        nodes.append(pick)
        rels.append(np.full(n, r))
    nodes, rels = np.concatenate(nodes), np.concatenate(rels)
    per_col = rng.integers(1, 4, len(nodes))                      # one to three reading rows per column ...
    per_col[(rels == HUB_REL) & (nodes == HUB_NODE)] = HUB_ROWS   # ... and the hub: the source in many rows
    cols = np.repeat(rels * N + nodes, per_col)
    rows = rng.integers(0, N, len(cols))
    hub = cols == HUB_REL * N + HUB_NODE
    rows[hub] = rng.choice(N, HUB_ROWS, replace=False)
    key = np.unique(rows.astype(np.int64) * (R * N) + cols)
    key = key[rng.permutation(len(key))]
    rows, cols = key // (R * N), key % (R * N)
    vals = rng.standard_normal(len(rows)).astype(np.float32)
    g = _Graph()
    _index_graph(g, rows, cols, vals, N, N, R)
    # the fixture cannot drift: the counts as the library's own relation-major order has them
    relptr = g.plan.export(L.ARR_RELPTR)
    assert tuple(np.diff(relptr)) == COUNTS
    np.testing.assert_array_equal(g.plan.export(L.ARR_ULCOL), g.ref["ulcol"])
    np.testing.assert_array_equal(g.plan.export(L.ARR_MPOS), g.ref["mpos"])
    assert g.plan.nop == g.ncols == sum(COUNTS)
    assert not np.array_equal(g.mpos, np.arange(g.ncols))          # the two orders differ
    assert int(np.diff(g.ref["cptr"]).max()) == HUB_ROWS
    yield g
    g.plan.close()


class _Case:
    """X, W and the float64 reference of one (K, F) on a graph: computed once, shared, never written again."""

    def __init__(self, g, K, F, n_in=None, in_row=None, rel=None):
        rng = np.random.default_rng([K, F, 5])
        n_in = g.plan.num_nodes if n_in is None else n_in
        in_row = g.node if in_row is None else in_row
        rel = g.rel if rel is None else rel
        self.K, self.F, self.in_row = K, F, in_row
        self.X = rng.standard_normal((n_in, K)).astype(np.float32)
        self.W = rng.standard_normal((g.plan.num_relations, K, F)).astype(np.float32)
        X64, W64 = self.X.astype(np.float64), self.W.astype(np.float64)
        self.ref = np.zeros((len(rel), F))
        mag = np.zeros((len(rel), F))
        for r in range(g.plan.num_relations):
            sel = np.nonzero(rel == r)[0]
            if len(sel):
                self.ref[sel] = X64[in_row[sel]] @ W64[r]
                mag[sel] = np.abs(X64[in_row[sel]]) @ np.abs(W64[r])
        self.bound = 2.0 * K * U * mag
        self.ref.setflags(write=False)
        self.bound.setflags(write=False)
        self._dev = {}

    def x(self, ldX, X=None, key="x"):
        """rows of ldX floats on the device; what lies past K is NaN and must never reach a result"""
        if (key, ldX) not in self._dev:
            X = self.X if X is None else X
            t = torch.full((X.shape[0], ldX), float("nan"), device="cuda")
            t[:, :self.K] = torch.from_numpy(X).cuda()
            self._dev[(key, ldX)] = t
        return self._dev[(key, ldX)]

    def w(self, unaligned=False):
        """W on a 16-byte boundary, or as a view that starts one float into a larger buffer"""
        if ("w", unaligned) not in self._dev:
            flat = torch.from_numpy(self.W.reshape(-1)).cuda()
            if unaligned:
                buf = torch.zeros(flat.numel() + 4, device="cuda")
                view = buf[1:1 + flat.numel()]
                view.copy_(flat)
                flat = view
            assert flat.data_ptr() % 16 == (4 if unaligned else 0)
            self._dev[("w", unaligned)] = flat
        return self._dev[("w", unaligned)]


def _case(g, K, F):
    if (K, F) not in g.cases:
        if len(g.cases) >= 24:      # (bounded: a reference of the widest shapes is a few MB)
            g.cases.pop(next(iter(g.cases)))
        g.cases[(K, F)] = _Case(g, K, F)
    return g.cases[(K, F)]


@contextlib.contextmanager
def _switches(**kw):
    from mrgcn_amd import _lib as L
    old = L.set_config(**kw)        # mrgcn_config_set; the previous values come back
    try:
        yield
    finally:
        L.set_config(**old)


def _form(K, F, ldOut, n_rel=R, narrow=True):
    """the kernel form the dispatch takes for this shape under the switches as they stand (`narrow` = False: the
    support entry point, which never takes the narrow kernel)"""
    import ctypes
    from mrgcn_amd import _lib as L
    cfg = {}
    for k in ("xform_cols_lds", "xform_mfma"):
        v = ctypes.c_int64()
        L.check(L.load().mrgcn_config_get(k.encode(), ctypes.byref(v)))
        cfg[k] = int(v.value)
    if narrow and cfg["xform_cols_lds"] and K <= 16 and F <= 16 and ldOut <= 16 and n_rel * K * _roundup4(F) * 4 <= 150 * 1024:
        return f"k_xform_cols_lds<KT={4 if K <= 4 else 8 if K <= 8 else 12 if K <= 12 else 16}>"
    if cfg["xform_mfma"] and K <= 256 and F <= 64:
        nt = min(4, max((ldOut + 15) // 16, (F + 15) // 16))
        steps = (K + 15) // 16
        ks = next(k for k in ((1, 2, 3, 4, 6, 8, 10, 12, 16) if nt == 1 else (1, 4, 16)) if steps <= k)
        return f"k_xform_mfma_fwd<NT={nt}, KS={ks}>"
    return "k_xform_fwd"


def _verify(g, case, out, tail, F, ldOut, pos, label, bf16=False, rel=None, place=None):
    """out: [rows, ldOut] float64 copy of the output, tail: what lies behind it.  Column c at row pos[c]."""
    rel = g.rel if rel is None else rel
    body = out[pos, :F]
    lim = case.bound + (2.0 ** -8 * np.abs(case.ref) if bf16 else 0.0)
    err = np.abs(body - case.ref)
    bad = ~(err <= lim)             # (a NaN or an untouched sentinel is bad)
    if bad.any():
        cs = np.unique(np.nonzero(bad)[0])
        c, f = (int(v) for v in np.argwhere(bad)[0])
        where = "" if place is None else f", place {int(place[c])} of its relation's walk"
        pytest.fail(f"{label}: {int(bad.sum())} elements in {len(cs)} columns outside the bound, relations "
                    f"{sorted(set(int(r) for r in rel[cs]))}, features {sorted(set(int(v) for v in np.nonzero(bad)[1]))[:20]}; "
                    f"first: column {c} (relation {int(rel[c])}{where}), feature {f}: got {body[c, f]!r}, "
                    f"want {case.ref[c, f]!r}, |err| {err[c, f]:.3e} > bound {lim[c, f]:.3e}")
    pad = out[:, F:]
    assert (pad == 0).all(), (f"{label}: the padded row is not written whole: columns "
                              f"{sorted(set(int(v) + F for v in np.nonzero(pad != 0)[1]))} of [F, ldOut) are not zero")
    assert (tail == SENTINEL).all(), f"{label}: wrote behind the last row ({int((tail != SENTINEL).sum())} elements)"


def _run(g, case, K, F, ldX, ldOut, order, bf16=False, unaligned=False, what=""):
    from mrgcn_amd import _lib as L
    lib = L.load()
    X, W = case.x(ldX), case.w(unaligned)
    rows = g.ncols
    buf = torch.full(((rows + 1) * ldOut + GUARD,), SENTINEL, dtype=torch.bfloat16 if bf16 else torch.float32,
                     device="cuda")
    fn = lib.mrgcn_rel_transform_fwd_bf16 if bf16 else lib.mrgcn_rel_transform_fwd_f32
    label = (f"{what}{_form(K, F, ldOut)}{' bf16 out' if bf16 else ''} K={K} F={F} ldX={ldX} ldOut={ldOut} "
             f"operand_order={order}{' W unaligned' if unaligned else ''}")
    L.check(fn(g.plan.handle, X.data_ptr(), ldX, K, W.data_ptr(), F, buf.data_ptr(), ldOut, order,
               torch.cuda.current_stream().cuda_stream), label)
    host = buf.float().cpu().numpy().astype(np.float64)
    _verify(g, case, host[:rows * ldOut].reshape(rows, ldOut), host[rows * ldOut:], F, ldOut,
            g.mpos if order else np.arange(rows), label, bf16=bf16, place=g.place)


# ---- 1. matrix-core forward, every instantiation -------------------------------------------------------------------
MFMA_K = [1, 2, 3, 4, 5, 6, 7, 15, 16, 17, 18, 19, 32, 33, 48, 49, 64, 65, 96, 97, 128, 129, 160, 161, 192, 193, 255,
          256]
MFMA_SHAPES = ([(K, F) for K in MFMA_K for F in (1, 10, 16)] +
               [(K, F) for F in (17, 32, 33, 48, 49, 64) for K in (3, 5, 16, 17, 64, 65, 256)])


@pytest.mark.parametrize("K,F", MFMA_SHAPES)
def test_matrix_core_forward_every_instantiation(graph, K, F):
    case = _case(graph, K, F)
    with _switches(xform_cols_lds=0):
        for ldOut in (_roundup4(F), _roundup4(F) + 4):
            assert _form(K, F, ldOut).startswith("k_xform_mfma_fwd")
            for ldX in (K, K + 3):
                for order in (0, 1):
                    _run(graph, case, K, F, ldX, ldOut, order)


# ---- 2. the narrow kernel (switches at their defaults) -------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 3, 4, 10, 11, 12, 16])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 8, 9, 12, 13, 15, 16])
def test_narrow_forward_in_output_order(graph, K, F):
    case = _case(graph, K, F)
    for ldOut in sorted({F, _roundup4(F), 16}):     # ldOut = F not a multiple of 4: the element-wise row store
        assert _form(K, F, ldOut).startswith("k_xform_cols_lds")
        for unaligned in (False, True):             # the view forces the element-wise staging of the table
            for ldX in (K, K + 3):
                for order in (0, 1):
                    _run(graph, case, K, F, ldX, ldOut, order, unaligned=unaligned)


# ---- 3. the LDS-FMA fallback ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,F", [(257, 10), (300, 10)])
def test_fallback_beyond_the_matrix_core_limits(graph, K, F):
    case = _case(graph, K, F)
    for ldOut in (_roundup4(F), _roundup4(F) + 4):
        assert _form(K, F, ldOut) == "k_xform_fwd"
        for ldX in (K, K + 3):
            for order in (0, 1):
                _run(graph, case, K, F, ldX, ldOut, order)


@pytest.mark.parametrize("K,F", [(20, 65), (20, 80)])
def test_wider_than_64_features_is_refused_and_served_in_slices(graph, K, F):
    """F > 64 is outside every kernel (the fallback's accumulators are sized for 64): the entry point says so and
    writes nothing; the transform is then taken in slices of W's columns, 64 (the fallback's limit) and the rest, each
    into an output of its own — the same reference and bound."""
    from mrgcn_amd import _lib as L
    lib = L.load()
    g, case = graph, _case(graph, K, F)
    s = torch.cuda.current_stream().cuda_stream
    X = case.x(K)
    out = torch.full((g.ncols, F), SENTINEL, device="cuda")
    rc = lib.mrgcn_rel_transform_fwd_f32(g.plan.handle, X.data_ptr(), K, K, case.w().data_ptr(), F, out.data_ptr(), F,
                                         0, s)
    assert rc != L.OK and "F <= 64" in lib.mrgcn_last_error().decode()
    assert bool((out == SENTINEL).all())
    with _switches(xform_mfma=0, xform_cols_lds=0):
        for order in (0, 1):
            parts = []
            for f0, f1 in ((0, 64), (64, F)):
                Fs, ld = f1 - f0, _roundup4(f1 - f0)
                assert _form(K, Fs, ld) == "k_xform_fwd"
                Ws = torch.from_numpy(np.ascontiguousarray(case.W[:, :, f0:f1])).cuda()
                buf = torch.full(((g.ncols + 1) * ld + GUARD,), SENTINEL, device="cuda")
                L.check(lib.mrgcn_rel_transform_fwd_f32(g.plan.handle, X.data_ptr(), K, K, Ws.data_ptr(), Fs,
                                                        buf.data_ptr(), ld, order, s))
                host = buf.cpu().numpy().astype(np.float64)
                assert (host[g.ncols * ld:] == SENTINEL).all()
                part = host[:g.ncols * ld].reshape(g.ncols, ld)
                assert (part[:, Fs:] == 0).all()
                parts.append(part[:, :Fs])
            whole = np.concatenate(parts, axis=1)
            _verify(g, case, whole, np.full(1, SENTINEL), F, F, g.mpos if order else np.arange(g.ncols),
                    f"k_xform_fwd in slices 64 + {F - 64} K={K} F={F} operand_order={order}", place=g.place)


def test_a_row_stride_past_int32_is_refused(graph):
    """the kernels take the row's length as a 32-bit count: a longer row is an error, nothing is launched"""
    from mrgcn_amd import _lib as L
    lib = L.load()
    case = _case(graph, 10, 10)
    out = torch.full((16,), SENTINEL, device="cuda")
    for sw in ({}, dict(xform_mfma=0)):
        with _switches(**sw):
            rc = lib.mrgcn_rel_transform_fwd_f32(graph.plan.handle, case.x(10).data_ptr(), 10, 10, case.w().data_ptr(),
                                                 10, out.data_ptr(), 2 ** 31, 0, torch.cuda.current_stream().cuda_stream)
            assert rc != L.OK
    assert bool((out == SENTINEL).all())


@pytest.mark.parametrize("K,F", [(10, 10), (155, 10), (33, 40)])
def test_fallback_on_shapes_the_other_kernels_would_take(graph, K, F):
    case = _case(graph, K, F)
    with _switches(xform_mfma=0, xform_cols_lds=0):
        for ldOut in (_roundup4(F), _roundup4(F) + 4):
            assert _form(K, F, ldOut) == "k_xform_fwd"
            for ldX in (K, K + 3):
                for order in (0, 1):
                    _run(graph, case, K, F, ldX, ldOut, order)


# ---- 4. one shape, three kernels: each against float64, not against each other ------------------------------------
@pytest.mark.parametrize("K,F,ldOut", [(10, 10, 12), (16, 16, 16), (3, 5, 8), (7, 11, 12)])
def test_one_shape_through_all_three_kernels(graph, K, F, ldOut):
    case = _case(graph, K, F)
    for kind, sw in (("k_xform_cols_lds", {}), ("k_xform_mfma_fwd", dict(xform_cols_lds=0)),
                     ("k_xform_fwd", dict(xform_cols_lds=0, xform_mfma=0))):
        with _switches(**sw):
            assert _form(K, F, ldOut).startswith(kind)
            for ldX in (K, K + 3):
                for order in (0, 1):
                    _run(graph, case, K, F, ldX, ldOut, order)


# ---- 5. the bf16-output twin on both sides of every KS / NT / KT boundary ------------------------------------------
BF16_MFMA = ([(K, 10) for K in (3, 4, 16, 17, 32, 33, 48, 49, 64, 65, 96, 97, 128, 129, 160, 161, 192, 193, 256)] +
             [(K, F) for F in (17, 33, 49) for K in (16, 17, 64, 65)] +
             [(17, F) for F in (16, 32, 48, 64)])


@pytest.mark.parametrize("K,F", BF16_MFMA)
def test_bf16_output_matrix_core(graph, K, F):
    case = _case(graph, K, F)
    with _switches(xform_cols_lds=0):
        for ldOut in (_roundup4(F), _roundup4(F) + 4):
            assert _form(K, F, ldOut).startswith("k_xform_mfma_fwd")
            for ldX, order in ((K, 0), (K + 3, 1)):
                _run(graph, case, K, F, ldX, ldOut, order, bf16=True)


@pytest.mark.parametrize("F", [4, 10, 11])
@pytest.mark.parametrize("K", [3, 4, 5, 8, 9, 12, 13, 16])
def test_bf16_output_narrow(graph, K, F):
    case = _case(graph, K, F)
    for ldOut in sorted({F, _roundup4(F), 16}):
        assert _form(K, F, ldOut).startswith("k_xform_cols_lds")
        for ldX, order, unaligned in ((K, 0, False), (K + 3, 1, True)):
            _run(graph, case, K, F, ldX, ldOut, order, bf16=True, unaligned=unaligned)


# ---- 6. the support form: the same product over the live columns, by live number -----------------------------------
@pytest.fixture(scope="module")
def support(graph):
    from mrgcn_amd import _lib as L
    from mrgcn_amd.plan import GraphSupport
    rng = np.random.default_rng(31)
    flags = (rng.random(N) < 0.3).astype(np.uint8)
    sup = GraphSupport(graph.plan, torch.from_numpy(flags).cuda(), forward=True)
    s = _Graph()
    s.sup, s.plan = sup, graph.plan
    s.lrel = sup.export(L.SUP_LREL).astype(np.int64)
    s.ordn = sup.export(L.SUP_LNODE_ORD).astype(np.int64)
    s.lnode = sup.export(L.SUP_LNODE).astype(np.int64)
    lcol = sup.export(L.SUP_LCOL).astype(np.int64)
    # the exported arrays say what the header says: live column k is compact column LCOL[k]
    np.testing.assert_array_equal(s.lrel, graph.rel[lcol])
    np.testing.assert_array_equal(s.lnode[s.ordn], graph.node[lcol])
    live_rows = np.isin(graph.ref["rowidx"], np.nonzero(flags)[0])
    np.testing.assert_array_equal(lcol, np.unique(graph.ref["ccol"][live_rows]))
    per_rel = np.bincount(s.lrel, minlength=R)
    assert per_rel.max() > 512 and per_rel[2] == 0     # more than one chunk of a support's order; an empty relation
    yield s
    sup.close()


@pytest.mark.parametrize("F", [10, 16])
@pytest.mark.parametrize("K", [4, 5, 16, 17, 32, 33, 48, 49, 64, 65, 96, 97, 128, 129, 160, 161, 192, 193, 256])
def test_support_forward_by_live_number(support, K, F):
    from mrgcn_amd import _lib as L
    lib = L.load()
    q, sup = support, support.sup
    assert lib.mrgcn_support_rel_transform_supported(sup.handle, K, F, 0)
    case = _Case(q, K, F, n_in=sup.NL, in_row=q.ordn, rel=q.lrel)
    Xfull = np.full((N, K), np.nan, dtype=np.float32)   # rows of nodes outside the support are never read
    Xfull[q.lnode] = case.X
    W = case.w()
    s = torch.cuda.current_stream().cuda_stream
    for ldT in (_roundup4(F), _roundup4(F) + 4):
        for by_node in (0, 1):
            for ldX in (K, K + 3):
                X = case.x(ldX, Xfull, "xfull") if by_node else case.x(ldX)
                buf = torch.full(((sup.L + 1) * ldT + GUARD,), SENTINEL, device="cuda")
                label = (f"support {_form(K, F, ldT, narrow=False)} K={K} F={F} ldX={ldX} ldT={ldT} x_by_node={by_node}")
                L.check(lib.mrgcn_support_rel_transform_fwd_f32(sup.handle, X.data_ptr(), ldX, by_node, K, W.data_ptr(),
                                                                F, buf.data_ptr(), ldT, s), label)
                host = buf.cpu().numpy().astype(np.float64)
                _verify(q, case, host[:sup.L * ldT].reshape(sup.L, ldT), host[sup.L * ldT:], F, ldT,
                        np.arange(sup.L), label, rel=q.lrel)


# ---- 7. wide segment sums of the input gradient --------------------------------------------------------------------
# segment_sum_arrays is reached, for K > 16, by the dX halves of mrgcn_support_rel_transform_bwd_f32 (node pointers
# NLPTR: every node of the graph) and mrgcn_support_rel_transform_bwd_compact_f32 (LNPTR: the live nodes).  A node owns
# at most R columns, so the nodes of more than 64 columns need a graph of their own with more than 64 relations.
N2, R2 = 160, 72
NODE_COLS = (72, 0, 1, 3, 4, 5, 65, 2, 8, 7)    # columns of the first nodes; the rest: 0..8 at random


@pytest.fixture(scope="module")
def wide_nodes():
    from mrgcn_amd import _lib as L
    from mrgcn_amd.plan import GraphSupport
    rng = np.random.default_rng(77)
    cnt = np.concatenate([NODE_COLS, rng.integers(0, 9, N2 - len(NODE_COLS))])
    cols = np.concatenate([rng.choice(R2, c, replace=False) * N2 + j for j, c in enumerate(cnt)]).astype(np.int64)
    rows = rng.integers(0, N2, len(cols))
    rows[:NODE_COLS[0]] = rng.integers(0, N2 // 2, NODE_COLS[0])  # (the widest node stays live under the half flags)
    vals = rng.standard_normal(len(cols)).astype(np.float32)
    g = _Graph()
    _index_graph(g, rows, cols, vals, N2, N2, R2)
    np.testing.assert_array_equal(np.diff(g.ref["nptr"]), cnt)
    np.testing.assert_array_equal(g.plan.export(L.ARR_NPTR), g.ref["nptr"])
    sups = {}
    for name, flags, fwd in (("every", np.ones(N2, np.uint8), False),
                             ("half", (np.arange(N2) < N2 // 2).astype(np.uint8), True)):
        sup = GraphSupport(g.plan, torch.from_numpy(flags).cuda(), forward=fwd)
        lcol = sup.export(L.SUP_LCOL).astype(np.int64)
        sups[name] = (sup, lcol)
    assert np.array_equal(sups["every"][1], np.arange(g.ncols))
    per_node = np.bincount(g.node[sups["half"][1]], minlength=N2)
    assert per_node.max() > 64 and {1, 3, 4, 5} <= set(per_node.tolist())
    g.sups = sups
    yield g
    for sup, _ in sups.values():
        sup.close()
    g.plan.close()


@pytest.mark.parametrize("K", [17, 64, 65, 128, 129, 192, 193, 256])
@pytest.mark.parametrize("form", ["every", "half"])
def test_wide_segment_sums_of_the_input_gradient(wide_nodes, form, K):
    """dX[j, 0:K] = sum over node j's n live columns c of Z[c] = dM[c, 0:F] . W[r_c]^T.  Bound, with u = 2^-24 and
    S_c = sum_f |dM| |W| (float64): each Z[c] is off by at most 2 F u S_c (the forward's bound for its F products), so
    |Z[c]| <= (1 + 2 F u) S_c; adding n such rows in any order costs at most gamma_(n-1) = (n-1) u / (1 - (n-1) u)
    times the sum of their magnitudes.  Together: sum_c 2 F u S_c + gamma_(n-1) (1 + 2 F u) sum_c S_c per element.  A
    node without columns: exactly zero."""
    from mrgcn_amd import _lib as L
    lib = L.load()
    g = wide_nodes
    sup, lcol = g.sups[form]
    F, ldM = 10, 12
    rng = np.random.default_rng([K, 9])
    rel, node = g.rel[lcol], g.node[lcol]
    dM = np.full((sup.L, ldM), np.nan, dtype=np.float32)     # what lies past F is never read
    dM[:, :F] = rng.standard_normal((sup.L, F))
    W = rng.standard_normal((R2, K, F)).astype(np.float32)
    dM64, W64 = dM[:, :F].astype(np.float64), W.astype(np.float64)
    Z, S = np.zeros((sup.L, K)), np.zeros((sup.L, K))
    for r in range(R2):
        sel = np.nonzero(rel == r)[0]
        Z[sel] = dM64[sel] @ W64[r].T
        S[sel] = np.abs(dM64[sel]) @ np.abs(W64[r]).T
    if form == "every":     # one row per node of the graph
        out_rows, seg = N2, node
    else:                   # one row per live node, by rank
        lnode = sup.export(L.SUP_LNODE).astype(np.int64)
        out_rows, seg = sup.NL, np.searchsorted(lnode, node)
        np.testing.assert_array_equal(seg, sup.export(L.SUP_LNODE_ORD))
    want = np.zeros((out_rows, K))
    np.add.at(want, seg, Z)
    mags = np.zeros((out_rows, K))
    np.add.at(mags, seg, S)
    n_seg = np.bincount(seg, minlength=out_rows).astype(np.float64)[:, None]
    gamma = np.maximum(n_seg - 1.0, 0.0) * U / (1.0 - np.maximum(n_seg - 1.0, 0.0) * U)
    bound = 2.0 * F * U * mags + gamma * (1.0 + 2.0 * F * U) * mags
    s = torch.cuda.current_stream().cuda_stream
    dMg, Wg = torch.from_numpy(dM).cuda(), torch.from_numpy(W).cuda()
    Xg = torch.full((N2, K), float("nan"), device="cuda")     # dX never reads X
    kernel = ("k_segment_sum<false>" if K <= 64 else f"k_segment_sum_wide<{(K + 63) // 64}>")
    for lddX in (K, K + 5):
        nws = int(lib.mrgcn_support_rel_transform_bwd_workspace(sup.handle, K, F, 1, 0))
        assert nws > 0
        ws = torch.full((nws,), float("nan"), device="cuda")
        buf = torch.full(((out_rows + 1) * lddX + GUARD,), SENTINEL, device="cuda")
        label = f"{kernel} ({form} node) K={K} F={F} lddX={lddX}"
        if form == "every":
            L.check(lib.mrgcn_support_rel_transform_bwd_f32(sup.handle, dMg.data_ptr(), ldM, Xg.data_ptr(), K, K,
                                                            Wg.data_ptr(), F, buf.data_ptr(), lddX, 0, ws.data_ptr(),
                                                            nws, 0, s), label)
        else:
            L.check(lib.mrgcn_support_rel_transform_bwd_compact_f32(sup.handle, dMg.data_ptr(), ldM, Xg.data_ptr(), K,
                                                                    1, K, Wg.data_ptr(), F, buf.data_ptr(), lddX, 0,
                                                                    ws.data_ptr(), nws, 0, s), label)
        host = buf.cpu().numpy().astype(np.float64)
        got = host[:out_rows * lddX].reshape(out_rows, lddX)
        err = np.abs(got[:, :K] - want)
        bad = ~(err <= bound)
        if bad.any():
            j, i = (int(v) for v in np.argwhere(bad)[0])
            pytest.fail(f"{label}: {int(bad.sum())} elements outside the bound in rows of "
                        f"{sorted(set(int(v) for v in np.bincount(seg, minlength=out_rows)[np.nonzero(bad)[0]]))} "
                        f"columns; first: row {j}, element {i}: got {got[j, i]!r}, want {want[j, i]!r}, "
                        f"|err| {err[j, i]:.3e} > bound {bound[j, i]:.3e}")
        assert (got[:, K:] == SENTINEL).all(), f"{label}: wrote past K in a row of dX"
        assert (host[out_rows * lddX:] == SENTINEL).all(), f"{label}: wrote behind the last row"
