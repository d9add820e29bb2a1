"""Type-constrained link prediction without a GPU (Krompass, Baier, Tresp, ISWC 2015; csrc/lp_typed.hip,
mrgcn_amd.tasks.link_prediction.TypedCandidates / TypedFacts, mrgcn_amd.host.typed_candidates / typed_ranks /
negatives_draw(typed=...)): the candidate lists against a brute-force set construction, the validation errors, the
numpy mirrors the device kernels are pinned to in tests/test_gpu_lp_typed.py, and the exports.  Every seed is fixed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.test_cpu_host import ROOT, header_functions

N, R, SEED = 40, 5, 2015
NEW = ["mrgcn_negatives_draw_typed_i64", "mrgcn_distmult_typed_ranks_workspace", "mrgcn_distmult_typed_ranks",
       "mrgcn_complex_typed_ranks_workspace", "mrgcn_complex_typed_ranks", "mrgcn_distmult_typed_topk_workspace",
       "mrgcn_distmult_typed_topk", "mrgcn_complex_typed_topk_workspace", "mrgcn_complex_typed_topk"]
_FIX: dict = {}


def fixture40():
    """40 nodes, 5 relations.  Relation 0: heads 0 .. 14, tails 10 .. 29 (nodes 10 .. 14 are domain AND range);
    relation 1: heads 0 .. 5, the SINGLE tail 7; relation 2: no facts (two empty lists); relation 3: heads 30 .. 39,
    tails 0 .. 9; relation 4: the literal-like one — heads 0 .. 19, tails 35 .. 39."""
    if not _FIX:
        r = np.random.default_rng(40)
        f0 = np.stack([r.integers(0, 15, 60), np.zeros(60, np.int64), r.integers(10, 30, 60)], 1)
        f0 = np.concatenate([f0, [(s, 0, 10 + s) for s in range(15)], [(0, 0, o) for o in range(10, 30)]])
        f1 = np.array([(s, 1, 7) for s in range(6)])
        f3 = np.stack([r.integers(30, 40, 25), np.full(25, 3), r.integers(0, 10, 25)], 1)
        f3 = np.concatenate([f3, [(30 + i, 3, i) for i in range(10)]])
        f4 = np.concatenate([[(s, 4, 35 + s % 5) for s in range(20)]])
        facts = np.unique(np.concatenate([f0, f1, f3, f4]).astype(np.int64), axis=0)
        _FIX["facts"] = facts[r.permutation(len(facts))]
    return _FIX["facts"]


def brute_lists(facts, n_rel):
    out = []
    for p in range(n_rel):
        out.append(sorted({int(o) for s, q, o in facts if q == p}))
        out.append(sorted({int(s) for s, q, o in facts if q == p}))
    return out


# ---- 1. the lists -----------------------------------------------------------------------------------------------------
def test_from_facts_equals_a_brute_force_set_construction():
    from mrgcn_amd import host
    from mrgcn_amd.tasks import link_prediction as lp
    facts = fixture40()
    types = lp.TypedCandidates.from_facts(facts, N, R, device="cpu")
    want = brute_lists(facts.tolist(), R)
    assert types.ptr_host.dtype == np.int64 and types.idx_host.dtype == np.int32
    assert types.ptr.dtype.is_floating_point is False and str(types.idx.dtype) == "torch.int32"
    assert types.ptr_host.shape == (2 * R + 1,) and types.ptr_host[0] == 0
    got = [types.idx_host[types.ptr_host[s]:types.ptr_host[s + 1]].tolist() for s in range(2 * R)]
    assert got == want
    assert got[4] == [] and got[5] == []                         # relation 2: no facts, two empty lists
    assert got[2] == [7] and got[3] == [0, 1, 2, 3, 4, 5]        # relation 1: a single tail
    assert set(range(10, 15)) <= set(got[0]) & set(got[1])       # nodes that are domain and range of relation 0
    assert types.slot(1, "tail").tolist() == [7] and types.slot(1, "head").tolist() == got[3]
    ptr, idx = host.typed_candidates(facts, N, R)
    assert np.array_equal(ptr, types.ptr_host) and np.array_equal(idx, types.idx_host)
    assert types.contains([2, 2, 4, 0], [7, 8, 0, 29]).tolist() == [True, False, False, True]
    full = lp.TypedCandidates.full(N, R, device="cpu")
    assert np.array_equal(full.ptr_host, np.arange(2 * R + 1) * N)
    assert all(np.array_equal(full.slot(p, sd), np.arange(N)) for p in range(R) for sd in ("tail", "head"))
    # declared lists pass through unchanged
    again = lp.TypedCandidates(types.ptr_host, types.idx_host, N, R, device="cpu")
    assert np.array_equal(again.idx_host, types.idx_host)


# ---- 2. validation ---------------------------------------------------------------------------------------------------
def _declared():
    ptr = np.array([0, 3, 5, 5, 6], dtype=np.int64)              # 2 relations: [1 4 9] [0 2] [] [3]
    idx = np.array([1, 4, 9, 0, 2, 3], dtype=np.int32)
    return ptr, idx


@pytest.mark.parametrize("case", ["unsorted", "duplicate", "id_out_of_range", "negative_id", "ptr_not_monotone",
                                  "ptr_wrong_length", "ptr_wrong_end"])
def test_declared_lists_are_validated(case):
    from mrgcn_amd.tasks import link_prediction as lp
    ptr, idx = _declared()
    assert lp.TypedCandidates(ptr, idx, 10, 2, device="cpu").slot(0).tolist() == [1, 4, 9]
    if case == "unsorted":
        idx[:3] = [4, 1, 9]
    elif case == "duplicate":
        idx[:3] = [1, 1, 9]
    elif case == "id_out_of_range":
        idx[2] = 10
    elif case == "negative_id":
        idx[0] = -1
    elif case == "ptr_not_monotone":
        ptr[:] = [0, 5, 3, 5, 6]
    elif case == "ptr_wrong_length":
        ptr = ptr[:-1]
    else:
        ptr[-1] = 5
    with pytest.raises(ValueError):
        lp.TypedCandidates(ptr, idx, 10, 2, device="cpu")


def test_a_list_boundary_is_not_taken_for_an_unsorted_pair():
    from mrgcn_amd.tasks import link_prediction as lp
    # [9] [0 2]: 9 -> 0 falls across a boundary and is fine
    lp.TypedCandidates(np.array([0, 1, 3]), np.array([9, 0, 2]), 10, 1, device="cpu")


def test_typed_facts_need_their_own_answer_among_the_candidates():
    from mrgcn_amd.tasks import link_prediction as lp
    facts = fixture40()
    types = lp.TypedCandidates.from_facts(facts, N, R, device="cpu")
    tf = lp.TypedFacts(facts, types, device="cpu")
    assert tf.n == len(facts) and tf.lists is not None and len(tf.lists) == 4
    with pytest.raises(ValueError, match="tail"):
        lp.TypedFacts(np.array([[0, 1, 8]]), types, device="cpu")       # 8 is not a tail of relation 1
    with pytest.raises(ValueError, match="head"):
        lp.TypedFacts(np.array([[9, 1, 7]]), types, device="cpu")       # 9 is not a head of relation 1
    with pytest.raises(ValueError):
        lp.TypedFacts(np.array([[0, 2, 1]]), types, device="cpu")       # relation 2 has no candidates at all
    with pytest.raises(ValueError):
        lp.TypedFacts(np.array([[0, 5, 1]]), types, device="cpu")       # no such relation


def test_typed_facts_grouping_and_filter_lists():
    from mrgcn_amd.tasks import link_prediction as lp
    facts = fixture40()
    types = lp.TypedCandidates.from_facts(facts, N, R, device="cpu")
    tf = lp.TypedFacts(facts, types, mrr_batchsize=30, device="cpu")
    order, tptr, trel = tf.order_host, tf.tile_ptr_host, tf.tile_rel_host
    assert sorted(order.tolist()) == list(range(len(facts))) and tptr[0] == 0 and tptr[-1] == len(facts)
    for t in range(len(trel)):
        members = facts[order[tptr[t]:tptr[t + 1]], 1]
        assert 1 <= len(members) <= 8 and np.all(members == trel[t])
    counts = np.bincount(facts[:, 1], minlength=R)
    assert len(trel) == int(((counts + 7) // 8).sum())
    # the lists are filter_lists' (the facts' own truedicts) ...
    want = lp.filter_lists(facts)
    for got, w in zip(tf.lists, want):
        assert np.array_equal(got.numpy()[:len(w)], w)
    # ... and with `known` what is known beyond the facts is filtered too
    half = lp.TypedFacts(facts[::2], types, known=facts, device="cpu")
    w_all = lp.filter_lists(facts)
    tp = half.lists[0].numpy()
    for i, f in enumerate(range(0, len(facts), 2)):
        assert np.array_equal(half.lists[1].numpy()[tp[i]:tp[i + 1]], w_all[1][w_all[0][f]:w_all[0][f + 1]])
    assert tf.part_ptr_host.tolist() == lp.FactParts(facts, 30, filtered=False, device="cpu").part_ptr_host.tolist()
    assert tf.scores_computed == int(sum(len(types.slot(p, "tail")) + len(types.slot(p, "head")) for p in facts[:, 1]))


def test_the_sampler_refuses_empty_lists_and_local_ids():
    from mrgcn_amd import _lib
    from mrgcn_amd.tasks import link_prediction as lp
    facts = fixture40()
    types = lp.TypedCandidates.from_facts(facts, N, R, device="cpu")
    declared = lp.TypedCandidates(np.array([0, 2, 2]), np.array([1, 2]), 4, 1, device="cpu")   # tails [1 2], heads []
    one = np.array([[0, 0, 1]])
    with pytest.raises(ValueError, match="no head candidates"):
        lp.NegativeSampler(one, 4, 1, candidates=declared)
    with pytest.raises(ValueError, match="no head candidates"):
        lp.NegativeSampler(one, 4, 1, candidates=declared, side="head")
    with pytest.raises(ValueError, match="no tail candidates"):
        lp.NegativeSampler(np.array([[0, 2, 1]]), N, R, candidates=types, side="tail")
    with pytest.raises(_lib.MrgcnError, match="to_global"):
        lp.NegativeSampler(facts, N, R, candidates=types, to_global=np.arange(N))
    with pytest.raises(ValueError):
        lp.NegativeSampler(facts, N + 1, R, candidates=types)


# ---- 3. the negatives mirror -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [0, 1, 2], ids=["both", "tail", "head"])
@pytest.mark.parametrize("rate", [1, 3])
def test_mirror_with_full_lists_equals_the_untyped_mirror(rate, side):
    from mrgcn_amd import host
    from mrgcn_amd.tasks import link_prediction as lp
    facts = fixture40()
    full = lp.TypedCandidates.full(N, R, device="cpu")
    for keys in (host.fact_keys(facts, N, R), False):
        for position in (0, 1):
            want = host.negatives_draw(facts, rate, N, N, R, keys, SEED, position, side=side)
            got = host.negatives_draw(facts, rate, N, N, R, keys, SEED, position, side=side,
                                      typed=(full.ptr_host, full.idx_host))
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_mirror_negatives_stay_inside_their_lists_and_flag_the_single_tail():
    from mrgcn_amd import host
    from mrgcn_amd.tasks import link_prediction as lp
    facts = fixture40()
    types = lp.TypedCandidates.from_facts(facts, N, R, device="cpu")
    rate = 4
    src = np.repeat(facts, rate, axis=0)
    for position in (0, 1):
        out, flags = host.negatives_draw(facts, rate, N, N, R, False, SEED, position,
                                         typed=(types.ptr_host, types.idx_host))
        assert out.shape == (len(facts) * rate, 3) and np.array_equal(out[:, 1], src[:, 1])
        head = out[:, 0] != src[:, 0]
        tail = ~head                       # (a refused tail draw keeps the fact: it counts as a tail negative)
        assert np.array_equal(out[head, 2], src[head, 2]) and np.array_equal(out[tail, 0], src[tail, 0])
        assert head.any() and (tail & (src[:, 1] != 1)).any()
        new_end = np.where(head, out[:, 0], out[:, 2])
        assert types.contains(2 * out[:, 1] + head, new_end).all()
        # relation 1 has the single tail 7: its tail negatives cannot be resolved, every other negative is
        want_flags = (src[:, 1] == 1) & tail
        assert np.array_equal(flags.astype(bool), want_flags) and want_flags.any()
        assert np.all(out[want_flags, 2] == 7)
        changed = (out != src).any(axis=1)
        assert np.array_equal(changed, ~want_flags)
    # with the facts' keys as the filter no resolved negative is a known fact
    keys = host.fact_keys(facts, N, R)
    out, flags = host.negatives_draw(facts, rate, N, N, R, keys, SEED, 0, typed=(types.ptr_host, types.idx_host))
    k = (out[:, 0] * R + out[:, 1]) * N + out[:, 2]
    assert not np.isin(k[flags == 0].astype(np.uint64), keys).any()
    with pytest.raises(ValueError):
        host.negatives_draw(facts, 1, N, N, R, False, SEED, 0, typed=(types.ptr_host, types.idx_host),
                            cand=np.arange(N))


# ---- 4. the rank mirror ----------------------------------------------------------------------------------------------
def _embeddings(H, seed=3):
    r = np.random.default_rng(seed)
    E = r.standard_normal((N, H)).astype(np.float32)
    Rel = r.standard_normal((R, H)).astype(np.float32)
    E[21] = E[22] = E[23] = E[20]          # four equal rows among relation 0's tails: ties of 2, 3 and 4
    E[11] = E[10]                          # two equal rows among relation 0's heads (and tails)
    return E, Rel


def _half_even(m):
    return int(round(m / 2.0))             # Python rounds halves to the even neighbour


@pytest.mark.parametrize("scorer,H", [("distmult", 6), ("complex", 6), ("distmult", 7)])
def test_typed_ranks_equal_a_direct_count_over_the_slot(scorer, H):
    from mrgcn_amd import host
    from mrgcn_amd.tasks import link_prediction as lp
    facts = fixture40()
    extra = np.array([(0, 0, o) for o in (20, 21, 22, 23)] + [(10, 0, 20), (11, 0, 21)], dtype=np.int64)
    facts = np.unique(np.concatenate([facts, extra]), axis=0)
    types = lp.TypedCandidates.from_facts(facts, N, R, device="cpu")
    E, Rel = _embeddings(H)
    raw, flt = host.typed_ranks(facts, (types.ptr_host, types.idx_host), E, Rel, scorer=scorer)
    scores = host.complex_candidate_scores if scorer == "complex" else host.distmult_candidate_scores
    known = {tuple(f) for f in facts.tolist()}
    nf = len(facts)
    tie_sizes = set()
    for head, side in ((0, "tail"), (1, "head")):
        sc = scores(E, Rel, facts[:, 2] if head else facts[:, 0], facts[:, 1], side)
        for f, (s, p, o) in enumerate(facts.tolist()):
            ans = s if head else o
            cand = types.slot(p, side).tolist()
            assert ans in cand
            gt = sum(1 for c in cand if sc[f, c] > sc[f, ans])
            eq = sum(1 for c in cand if sc[f, c] == sc[f, ans])
            assert raw[head * nf + f] == gt + _half_even(eq - 1) + 1
            tie_sizes.add(eq)
            keep = [c for c in cand if c == ans or ((c, p, o) if head else (s, p, c)) not in known]
            gt = sum(1 for c in keep if sc[f, c] > sc[f, ans])
            eq = sum(1 for c in keep if sc[f, c] == sc[f, ans])
            assert flt[head * nf + f] == gt + _half_even(eq - 1) + 1
            assert 1 <= flt[head * nf + f] <= raw[head * nf + f] <= len(cand)
    assert {2, 4} <= tie_sizes             # x.5 rounded down to 0 and up to 2: the half-even rule is exercised
    assert host.rank_of([3, 3, 3, 3, 3], [1, 2, 3, 4, 5]).tolist() == [4, 4, 5, 6, 6]
    # typed ranks never exceed the ranks among all nodes
    full = lp.TypedCandidates.full(N, R, device="cpu")
    raw_all, flt_all = host.typed_ranks(facts, (full.ptr_host, full.idx_host), E, Rel, scorer=scorer)
    assert np.all(raw <= raw_all) and np.all(flt <= flt_all) and np.any(raw < raw_all)
    # `known` beyond the facts filters more
    raw_h, flt_h = host.typed_ranks(facts[::2], (types.ptr_host, types.idx_host), E, Rel, known=facts, scorer=scorer)
    assert np.array_equal(raw_h[:len(facts[::2])], raw[:nf][::2]) and np.array_equal(flt_h[:len(facts[::2])], flt[:nf][::2])
    with pytest.raises(ValueError):
        host.typed_ranks(np.array([[0, 1, 8]]), (types.ptr_host, types.idx_host), E, Rel, scorer=scorer)


def test_distmult_candidate_scores_are_the_sequential_float32_sums():
    from mrgcn_amd import host
    E, Rel = _embeddings(7)
    facts = fixture40()[:9]
    for side, a in (("tail", 0), ("head", 2)):
        got = host.distmult_candidate_scores(E, Rel, facts[:, a], facts[:, 1], side)
        assert got.dtype == np.float32 and got.shape == (9, N)
        for i, (s, p, o) in enumerate(facts.tolist()):
            for c in (0, 7, 39):
                acc = np.float32(0)
                for h in range(7):
                    if side == "tail":
                        acc = np.float32(acc + np.float32(np.float32(E[s, h] * Rel[p, h]) * E[c, h]))
                    else:
                        acc = np.float32(acc + np.float32(np.float32(E[c, h] * Rel[p, h]) * E[o, h]))
                assert got[i, c] == acc


# ---- 5. exports --------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported_and_the_abi_version_stays():
    from mrgcn_amd import _lib
    declared = header_functions()
    lib = _lib.load()
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/mrgcn_hip.h"
        assert name in _lib.SIGNATURES, f"{name} is not in the ctypes table"
        assert hasattr(lib, name)
    src = open(os.path.join(ROOT, "include", "mrgcn_hip.h")).read()
    assert re.search(r"#define\s+MRGCN_ABI_VERSION\s+5\b", src) and lib.mrgcn_abi_version() == 5 == _lib.ABI_VERSION
    assert os.path.exists(os.path.join(ROOT, "mrgcn_amd", "csrc", "lp_typed.hip"))
    res, args = _lib.SIGNATURES["mrgcn_negatives_draw_typed_i64"]
    assert res is C.c_int and len(args) == 14


def test_workspaces_and_argument_checks_answer_before_any_launch():
    from mrgcn_amd import _lib
    lib = _lib.load()
    assert lib.mrgcn_distmult_typed_ranks_workspace(10, 3, 7) == 4 * (30 + 7) + 4 * 8 * 7
    assert lib.mrgcn_complex_typed_ranks_workspace(10, 4, 7) == 4 * (40 + 14) + 4 * 8 * 7
    assert lib.mrgcn_complex_typed_ranks_workspace(10, 3, 7) == -1
    assert lib.mrgcn_distmult_typed_ranks_workspace(0, 3, 7) == -1
    # the tile lists are sized by the longest slot, not by the number of nodes
    et = lib.mrgcn_distmult_topk_workspace(100000, 8, 10, 5) - 8 * 10 * 5 * ((100000 + 255) // 256)
    assert lib.mrgcn_distmult_typed_topk_workspace(100000, 8, 10, 5, 300) == et + 8 * 10 * 5 * 2
    assert lib.mrgcn_distmult_typed_topk_workspace(100000, 8, 10, 5, 0) == et + 8 * 10 * 5 * 1
    assert lib.mrgcn_distmult_typed_topk_workspace(100, 8, 10, 5, 101) == -1
    assert lib.mrgcn_complex_typed_topk_workspace(100, 7, 10, 5, 50) == -1
    assert lib.mrgcn_distmult_typed_topk_workspace(100, 8, 10, 257, 50) == -1
    buf = (C.c_int64 * 16)()
    a = C.addressof(buf)
    # no lists / a bad side / a bad rate: refused before the first launch
    assert lib.mrgcn_negatives_draw_typed_i64(a, 4, 1, None, None, None, 0, 8, 1, 0, a, a, None, None) == 1
    assert lib.mrgcn_negatives_draw_typed_i64(a, 4, 1, a, a, None, 0, 8, 1, 3, a, a, None, None) == 1
    assert lib.mrgcn_negatives_draw_typed_i64(a, 4, 0, a, a, None, 0, 8, 1, 0, a, a, None, None) == 1
    assert lib.mrgcn_last_error().decode().startswith("invalid argument")
    assert lib.mrgcn_distmult_typed_ranks(a, 4, 4, a, 4, 4, a, 1, None, a, a, 1, a, 1, a, a, None, None, None, None, a,
                                          1 << 20, a, None, None) == 1      # no order
    assert lib.mrgcn_complex_typed_ranks(a, 3, 4, a, 3, 3, a, 1, a, a, a, 1, a, 1, a, a, None, None, None, None, a,
                                         1 << 20, a, None, None) == 1       # an odd width
    assert lib.mrgcn_distmult_typed_topk(a, 4, 4, a, 4, 4, a, 1, 0, a, a, a, 1, a, 1, a, a, a, 4, None, None, 0, a,
                                         1 << 20, a, a, None) == 1          # k = 0


def test_typed_queries_group_by_relation_and_size_by_the_longest_list():
    from mrgcn_amd.tasks import link_prediction as lp
    facts = fixture40()
    types = lp.TypedCandidates.from_facts(facts, N, R, device="cpu")
    q = np.array([(0, 4), (1, 0), (2, 1), (3, 0), (4, 2), (5, 4)])
    tq = lp.TypedQueries(q, types, side="tail", known=facts, device="cpu")
    assert tq.nq == 6 and tq.max_slot == len(types.slot(0, "tail")) and tq.ntiles == 4
    assert tq.q_tiles.tolist() == [1, 1, 1, 1, 0, 1]            # relation 2 has no tails: no candidate tile
    assert tq.order.tolist() == [1, 3, 2, 4, 0, 5] and tq.nwork == 3
    assert tq.excl[0].numel() == 7
    with pytest.raises(ValueError):
        lp.TypedQueries(np.array([(0, 5)]), types, device="cpu")
    with pytest.raises(ValueError):
        lp.TypedQueries(q, types, side="both", device="cpu")


def test_prepared_queries_refuse_arguments_that_contradict_them():
    """These checks answer before the embeddings are looked at (no GPU needed)."""
    import torch

    from mrgcn_amd.tasks import link_prediction as lp
    facts = fixture40()
    types = lp.TypedCandidates.from_facts(facts, N, R, device="cpu")
    tq = lp.TypedQueries(np.array([(0, 4), (1, 0)]), types, side="head", known=facts, device="cpu")
    E, Rel = torch.zeros(N, 4), torch.zeros(R, 4)
    with pytest.raises(ValueError, match="side='head'"):
        lp.predict_topk(tq, E, Rel, 3)                                   # the default side is the tail
    with pytest.raises(ValueError, match="side='head'"):
        lp.predict_topk(tq, E, Rel, 3, side="tail")
    with pytest.raises(ValueError, match="known"):
        lp.predict_topk(tq, E, Rel, 3, side="head", known=facts)
    with pytest.raises(ValueError, match="other candidate lists"):
        lp.predict_topk(tq, E, Rel, 3, side="head", candidates=lp.TypedCandidates.full(N, R, device="cpu"))
    from mrgcn_amd import _lib
    with pytest.raises(_lib.MrgcnError):                                 # consistent arguments get as far as the device check
        lp.predict_topk(tq, E, Rel, 3, side="head", candidates=types)
