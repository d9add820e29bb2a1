"""csrc/lp_batches.hip on its own: mrgcn_distmult_batch_eval (one batch's raw and filtered ranks and its eight metric
values in one call) bit for bit against mrgcn_distmult_ranks and mrgcn_rank_metrics on random embeddings — shapes around
the candidate tile (256), the fact tile (8) and the h tile (64), more facts than nodes (the reference leaves the facts at
positions >= the number of nodes unscored), ties and masked ties —, and mrgcn_lp_batch_means_f32 against numpy's float64
means."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
R = 5

# (nodes, facts, H): every N of {1, 7, 255, 256, 257, 600}, every nf of {1, 8, 9, N - 1, N, N + 1, 2 N}, every H of
# {1, 63, 64, 65, 200}; the last is the largest batch of the FB15k-237 shape
SHAPES = [(1, 1, 1), (1, 2, 64), (7, 8, 63), (7, 9, 65), (7, 6, 200), (7, 14, 1), (255, 255, 64), (255, 254, 1),
          (256, 257, 65), (256, 512, 63), (257, 256, 200), (257, 1, 64), (600, 1200, 200), (600, 8, 63), (600, 601, 1),
          (761, 999, 200)]


def _problem(N, nf, H, seed=0, table="random"):
    rng = np.random.default_rng(seed + 1000 * N + nf + H)
    if table == "random":
        E = rng.standard_normal((N, H)).astype(np.float32)
    elif table == "duplicates":   # four distinct rows: ties between candidates, and between candidates and the truth
        E = rng.standard_normal((4, H)).astype(np.float32)[np.arange(N) % 4]
    else:
        E = np.zeros((N, H), np.float32)
    Rel = rng.standard_normal((R, H)).astype(np.float32)
    facts = np.stack([rng.integers(0, N, nf), rng.integers(0, R, nf), rng.integers(0, N, nf)], 1).astype(np.int64)
    return torch.from_numpy(E).cuda(), torch.from_numpy(Rel).cuda(), facts


def _lists(facts):
    from mrgcn_amd.tasks import link_prediction as lp
    # (an empty tensor has no address: one unread element stands for an empty index array, as in evaluate_batches)
    return [torch.from_numpy(a if len(a) else np.zeros(1, a.dtype)).cuda() for a in lp.filter_lists(facts)]


def _check(E, Rel, facts, with_lists=True):
    """batch_eval against compute_ranks_fast (mrgcn_distmult_ranks) and rank_metrics; returns (raw, flt, slot)."""
    from mrgcn_amd.tasks import link_prediction as lp
    nf = len(facts)
    f = torch.from_numpy(facts).cuda()
    raw = torch.full((2 * nf,), -7, dtype=torch.int64, device="cuda")
    flt = torch.full((2 * nf,), -7, dtype=torch.int64, device="cuda")
    slot = lp.batch_eval(E, Rel, f, _lists(facts) if with_lists else None, ranks=(raw, flt))
    ref_raw = lp.compute_ranks_fast(facts, E, Rel, 50, False)
    assert torch.equal(raw, ref_raw)
    assert torch.equal(slot[:4], lp.rank_metrics(ref_raw))
    if with_lists:
        ref_flt = lp.compute_ranks_fast(facts, E, Rel, 50, True)
        assert torch.equal(flt, ref_flt)
        assert torch.equal(slot[4:], lp.rank_metrics(ref_flt))
    else:
        assert bool((flt == -7).all())   # untouched
        assert slot[4:].tolist() == [-1.0] * 4
    return raw, flt, slot


@pytest.mark.parametrize("N,nf,H", SHAPES)
def test_batch_eval_bitwise(N, nf, H):
    from mrgcn_amd.tasks import link_prediction as lp
    E, Rel, facts = _problem(N, nf, H)
    raw, flt, slot = _check(E, Rel, facts)
    _check(E, Rel, facts, with_lists=False)
    # the slot without the rank buffers (the ranks then live in the workspace), and a second call: equal bits
    f = torch.from_numpy(facts).cuda()
    ws = lp.batch_eval_workspace(N, H, nf, "cuda")
    again = lp.batch_eval(E, Rel, f, _lists(facts), workspace=ws)
    assert torch.equal(again.view(torch.int32), slot.view(torch.int32))
    raw2 = torch.empty_like(raw)
    once_more = lp.batch_eval(E, Rel, f, _lists(facts), ranks=(raw2, None), workspace=ws)
    assert torch.equal(raw2, raw) and torch.equal(once_more.view(torch.int32), slot.view(torch.int32))


def test_strided_tables():
    """E and Rel as column slices of wider tables (ldE, ldR > H)."""
    E, Rel, facts = _problem(70, 90, 65)
    Ew, Rw = torch.randn((70, 80), device="cuda"), torch.randn((R, 72), device="cuda")
    Ew[:, :65], Rw[:, 3:68] = E, Rel
    a = _check(E, Rel, facts)
    b = _check(Ew[:, :65], Rw[:, 3:68], facts)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_empty_lists():
    """No fact shares (s, p) or (p, o) with another: both lists are empty and the filtered ranks are the raw ones."""
    from mrgcn_amd.tasks import link_prediction as lp
    E, Rel, _ = _problem(7, 7, 64)
    facts = np.stack([np.arange(7), np.arange(7) % R, np.arange(7)[::-1]], 1).astype(np.int64)
    assert all(len(a) == 0 for a in lp.filter_lists(facts)[1::2])
    raw, flt, slot = _check(E, Rel, facts)
    assert torch.equal(raw, flt) and torch.equal(slot[:4], slot[4:])


@pytest.mark.parametrize("table", ["duplicates", "zeros"])
def test_ties_masked_ties_and_unscored_facts(table):
    """Duplicated embedding rows and an all-zero table, twice as many facts as nodes.  N = 22: a fact at a position
    >= N is unscored, all 22 candidates tie with its truth 0, and its raw rank is round_half_even(21 / 2) + 1 = 11 —
    rounding half up gives 12, dropping the quirk gives the ranks of real scores."""
    N, nf, H = 22, 44, 8
    E, Rel, facts = _problem(N, nf, H, table=table)
    facts[:5] = np.stack([np.zeros(5), np.zeros(5), np.arange(1, 6)], 1)   # five answers of one (s, p): four masked each
    raw, flt, _ = _check(E, Rel, facts)
    raw, flt = raw.cpu().numpy(), flt.cpu().numpy()
    assert (N - 1) % 2 == 1 and ((N - 1) // 2) % 2 == 0   # x.5 with x even: half-even rounds down
    expect = (N - 1) // 2 + 1
    unscored = np.r_[N:nf, nf + N:2 * nf]
    assert np.all(raw[unscored] == expect)                 # a rank that came from the half-even rule
    if table == "zeros":
        assert np.all(raw == expect)
    assert np.any(raw != flt)                              # masked ties exist
    assert np.all(flt <= raw)


def test_bad_arguments_do_not_launch():
    from mrgcn_amd import _lib as L
    from mrgcn_amd.tasks import link_prediction as lp
    lib = L.load()
    assert lib.mrgcn_distmult_batch_eval_workspace(0, 8, 4) == -1
    assert lib.mrgcn_distmult_batch_eval_workspace(5, 0, 4) == -1
    assert lib.mrgcn_distmult_batch_eval_workspace(5, 8, 0) == -1
    assert lib.mrgcn_distmult_batch_eval_workspace(5, 8, 4) >= 4 * (5 * 8 + 4)
    E, Rel, facts = _problem(9, 12, 16)
    f = torch.from_numpy(facts).cuda()
    ls = _lists(facts)
    ws = lp.batch_eval_workspace(9, 16, 12, "cuda")
    slot = torch.full((8,), 3.0, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731

    def call(nf=12, lists=ls, ws_bytes=ws.numel() * 8, slot_=slot, H=16):
        return lib.mrgcn_distmult_batch_eval(p(E), E.stride(0), 9, p(Rel), Rel.stride(0), H, p(f), nf, p(lists[0]),
                                             p(lists[1]), p(lists[2]), p(lists[3]), p(ws), ws_bytes, None, None,
                                             p(slot_), s)

    assert call(nf=0) != L.OK
    assert call(lists=[ls[0], ls[1], None, None]) != L.OK
    assert call(lists=[ls[0], None, ls[2], None]) != L.OK
    assert call(ws_bytes=64) != L.OK
    assert call(slot_=None) != L.OK
    assert call(H=0) != L.OK
    torch.cuda.synchronize()
    assert slot.tolist() == [3.0] * 8
    assert call() == L.OK
    torch.cuda.synchronize()
    assert 0 < slot[0].item() <= 1
    # the wrapper's own checks
    with pytest.raises(L.MrgcnError, match="facts"):
        lp.batch_eval(E, Rel, f[:0], None)
    with pytest.raises(L.MrgcnError, match="lists"):
        lp.batch_eval(E, Rel, f, ls[:2])
    with pytest.raises(L.MrgcnError, match="slot"):
        lp.batch_eval(E, Rel, f, ls, slot=torch.zeros(4, device="cuda"))
    with pytest.raises(L.MrgcnError, match="ranks"):
        lp.batch_eval(E, Rel, f, ls, ranks=(torch.zeros(5, dtype=torch.int64, device="cuda"), None))
    with pytest.raises(L.MrgcnError, match="workspace"):
        lp.batch_eval(E, Rel, f, ls, workspace=torch.zeros(2, dtype=torch.int64, device="cuda"))


def _means(loss, train, valid, want_score=True):
    from mrgcn_amd.tasks import link_prediction as lp
    row = torch.full((lp.EVAL_ROW,), 9.0, device="cuda")
    score = torch.full((), 9.0, device="cuda") if want_score else None
    d = lambda a: torch.from_numpy(a).cuda() if a is not None else None   # noqa: E731
    lp._lp_batch_means(d(loss), 0 if loss is None else len(loss), d(train), 0 if train is None else len(train),
                       d(valid), 0 if valid is None else len(valid), row, score)
    return row.cpu().numpy(), (float(score) if want_score else None)


def _mean32(a):
    """numpy's float64 sum in slot order, divided, rounded once."""
    t = np.float64(0)
    for v in a:
        t += np.float64(v)
    return np.float32(t / np.float64(len(a)))


def test_batch_means():
    rng = np.random.default_rng(4)
    for nl, nt, nv in [(1, 1, 1), (3, 3, 2), (1011, 1011, 97), (6, 6, 3)]:
        loss = rng.random(nl).astype(np.float32)
        train, valid = rng.random((nt, 8)).astype(np.float32), rng.random((nv, 8)).astype(np.float32)
        train[:, 4:] = -1.0   # (filter_ranks off: the filtered four of every batch are -1)
        row, score = _means(loss, train, valid)
        assert row[0] == _mean32(loss)
        for k in range(8):
            assert row[1 + k] == _mean32(train[:, k]) and row[9 + k] == _mean32(valid[:, k]), (nl, k)
        assert np.all(row[5:9] == -1.0)
        t = np.float64(0)
        for v in valid[:, 0]:
            t += np.float64(v)
        assert score == np.float32(1.0 - t / nv)
    # float64 sums, not float32 ones: 2^24 + 1 + 1 is 2^24 + 2 only in float64
    loss = np.array([16777216.0, 1.0, 1.0, 0.0], np.float32)
    assert _means(loss, None, None)[0][0] == np.float32((16777216.0 + 2.0) / 4.0)
    # zero counts leave their columns (and the score) unwritten
    row, score = _means(rng.random(4).astype(np.float32), None, None)
    assert np.all(row[1:] == 9.0) and score == 9.0
    row, score = _means(None, rng.random((2, 8)).astype(np.float32), None)
    assert row[0] == 9.0 and np.all(row[9:] == 9.0) and np.all(row[1:9] != 9.0) and score == 9.0
    row, _ = _means(None, None, rng.random((2, 8)).astype(np.float32), want_score=False)
    assert np.all(row[:9] == 9.0) and np.all(row[9:] != 9.0)
