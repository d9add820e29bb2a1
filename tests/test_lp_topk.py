"""Top-k candidate completion, the host side: the exclusion lists of `known_lists` against a brute-force set
construction, the workspace formula of mrgcn_distmult_topk through the C ABI, and the argument checks of `predict_topk`
that must fire before anything is loaded on the GPU side."""
import numpy as np
import pytest

from mrgcn_amd import _lib
from mrgcn_amd.tasks import link_prediction as lp


def _brute(queries, known, side):
    out = []
    for a, r in queries:
        if side == "tail":
            out.append(sorted({int(o) for s, p, o in known if s == a and p == r}))
        else:
            out.append(sorted({int(s) for s, p, o in known if o == a and p == r}))
    return out


def _data():
    rng = np.random.default_rng(5)
    m = 120
    known = np.stack([rng.integers(0, 9, m), rng.integers(0, 4, m), rng.integers(0, 9, m)], 1).astype(np.int64)
    known = np.concatenate([known, known[:40], known[10:20]])              # duplicate facts
    queries = np.stack([rng.integers(0, 9, 40), rng.integers(0, 4, 40)], 1).astype(np.int64)
    queries[30:36] = queries[:6]                                           # the same (anchor, relation) asked twice
    queries[36:] = [[11, 0], [3, 7], [12, 9], [0, 5]]                      # nothing known about these
    return queries, known


@pytest.mark.parametrize("side", ["tail", "head"])
def test_known_lists_equal_brute_force(side):
    queries, known = _data()
    ptr, idx = lp.known_lists(queries, known, side)
    want = _brute(queries, known, side)
    assert ptr.dtype == np.int64 and idx.dtype == np.int32
    assert ptr.shape == (len(queries) + 1,) and ptr[0] == 0 and ptr[-1] == len(idx)
    assert np.all(np.diff(ptr) >= 0)
    got = [idx[ptr[i]:ptr[i + 1]].tolist() for i in range(len(queries))]
    assert got == want
    assert any(len(w) == 0 for w in want) and any(len(w) > 1 for w in want)
    for g in got:                                                          # sorted and duplicate-free
        assert all(a < b for a, b in zip(g, g[1:]))
    assert got[30:36] == got[:6]


@pytest.mark.parametrize("side", ["tail", "head"])
def test_known_lists_empty_inputs(side):
    queries, known = _data()
    ptr, idx = lp.known_lists(np.zeros((0, 2), np.int64), known, side)
    assert ptr.tolist() == [0] and ptr.dtype == np.int64 and idx.shape == (0,) and idx.dtype == np.int32
    ptr, idx = lp.known_lists(queries, np.zeros((0, 3), np.int64), side)
    assert ptr.tolist() == [0] * (len(queries) + 1) and idx.shape == (0,) and idx.dtype == np.int32


def test_known_lists_rejects_a_side_it_does_not_know():
    with pytest.raises(ValueError, match="side"):
        lp.known_lists(np.zeros((1, 2), np.int64), np.zeros((1, 3), np.int64), "both")


def test_topk_workspace_through_the_abi():
    ws = _lib.load().mrgcn_distmult_topk_workspace
    for bad in ((0, 8, 4, 10), (-1, 8, 4, 10), (100, 0, 4, 10), (100, 8, -1, 10), (100, 8, 4, 0), (100, 8, 4, 257),
                (1 << 31, 8, 4, 10)):
        assert ws(*bad) == -1, bad
    for N, H, nq, k in ((100, 8, 4, 10), (14541, 200, 500, 10), (4099, 64, 1, 256), (257, 7, 0, 1)):
        tiles = -(-N // 256)
        got = ws(N, H, nq, k)
        assert got >= 4 * H * N
        assert got == (4 * H * N + 7) // 8 * 8 + 8 * nq * k * tiles     # the transpose + the tile lists, nothing else


def test_predict_topk_checks_arguments_before_touching_the_gpu(monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    q = np.zeros((2, 2), np.int64)
    for kw, what in ((dict(side="both", k=3), "side"), (dict(k=0), "k must"), (dict(k=257), "256")):
        with pytest.raises((ValueError, _lib.MrgcnError), match=what):
            lp.predict_topk(q, None, None, **kw)      # (no embeddings either: nothing may look at them yet)
    with pytest.raises((ValueError, _lib.MrgcnError), match="side"):
        lp.predict_links(None, None, q, 3, side="both")
