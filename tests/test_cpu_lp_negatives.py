"""Keyed, filtered negatives (csrc/lp_negatives.hip, mrgcn_amd.host.negatives_draw) without a GPU: the entry point is
declared, bound and exported, its argument checks answer before any launch, and the numpy mirror — what the device draw
is pinned to bit for bit in tests/test_gpu_lp_negatives.py — has the properties the sampler promises.  Every seed is
fixed, so every figure below is deterministic."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.test_cpu_host import ROOT, header_functions

NAME = "mrgcn_negatives_draw_i64"
N, R, SEED = 64, 3, 1234
_FIX: dict = {}


def fixture64():
    """All 12 288 triples of 64 nodes x 3 relations in (s, p, o) nested order, 500 of them known, the first 257 of
    those the facts."""
    if not _FIX:
        from mrgcn_amd import host
        rng = np.random.default_rng(0)
        every = np.array([(s, p, o) for s in range(N) for p in range(R) for o in range(N)], dtype=np.int64)
        known = every[rng.choice(len(every), 500, replace=False)]
        _FIX.update(known=known, facts=known[:257], keys=host.fact_keys(known, N, R))
    return _FIX


def fixture300(seed=1):
    """2 500 distinct facts on 300 nodes x 5 relations (the stable-order case of the GPU file's reproducibility test)."""
    r = np.random.default_rng(seed)
    tr = np.unique(np.stack([r.integers(0, 300, 2600), r.integers(0, 5, 2600), r.integers(0, 300, 2600)], 1), axis=0)
    return tr[r.permutation(len(tr))][:2500].astype(np.int64)


FIX300_SAMPLER_SEED = 4321


def flag_case():
    """8 nodes, one relation, facts = known = (0, 0, o) for every o: no tail corruption can be accepted."""
    return np.array([(0, 0, o) for o in range(8)], dtype=np.int64)


def _keys_of(t, n=N, r=R):
    t = np.asarray(t).astype(np.uint64)
    return (t[:, 0] * np.uint64(r) + t[:, 1]) * np.uint64(n) + t[:, 2]


# ---- 1. declaration and binding ---------------------------------------------------------------------------------------
def test_symbol_is_declared_bound_and_exported_and_the_abi_version_stays():
    from mrgcn_amd import _lib, host
    assert NAME in header_functions(), f"{NAME} is not declared in include/mrgcn_hip.h"
    assert NAME in _lib.SIGNATURES, f"{NAME} is not in the ctypes table"
    res, args = _lib.SIGNATURES[NAME]
    assert res is C.c_int and len(args) == 15 and args.count(C.c_int32) == 2 and args.count(C.c_int64) == 5
    lib = _lib.load()
    assert hasattr(lib, NAME)
    src = open(os.path.join(ROOT, "include", "mrgcn_hip.h")).read()
    m = re.search(r"#define\s+MRGCN_NEG_MAX_ATTEMPTS\s+(\d+)", src)
    assert m and int(m.group(1)) == host.NEG_MAX_ATTEMPTS == 8
    assert re.search(r"#define\s+MRGCN_ABI_VERSION\s+5\b", src) and lib.mrgcn_abi_version() == 5 == _lib.ABI_VERSION
    # the kernel file cites the reference's sampler and shares the Philox body with node dropout
    csrc = os.path.join(ROOT, "mrgcn_amd", "csrc")
    assert "link_prediction.py:247-264" in open(os.path.join(csrc, "lp_negatives.hip")).read()
    for f in ("lp_negatives.hip", "node_dropout.hip"):
        text = open(os.path.join(csrc, f)).read()
        assert '#include "philox.hpp"' in text and "kPhiloxM0 =" not in text, f


# ---- 2. mirror properties --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [1, 3, 10])
def test_mirror_negatives_keep_the_fact_change_one_end_and_avoid_known_facts(rate):
    from mrgcn_amd import host
    fx = fixture64()
    facts, keys = fx["facts"], fx["keys"]
    outs = []
    for position in (0, 1, 2):
        out, unresolved = host.negatives_draw(facts, rate, N, N, R, keys, SEED, position)
        assert out.shape == (257 * rate, 3) and out.dtype == np.int64 and unresolved.shape == (257 * rate,)
        src = np.repeat(facts, rate, axis=0)
        assert np.array_equal(out[:, 1], src[:, 1])
        head, tail = out[:, 0] != src[:, 0], out[:, 2] != src[:, 2]
        assert np.all(head ^ tail)                      # exactly one end differs
        assert head.any() and tail.any()                # side = both: a bit per negative
        assert not np.isin(_keys_of(out), keys).any()   # no negative is a known fact
        assert int(unresolved.sum()) == 0
        assert 0 <= out.min() and out[:, [0, 2]].max() < N
        unfiltered, un2 = host.negatives_draw(facts, rate, N, N, R, False, SEED, position)
        hits = int(np.isin(_keys_of(unfiltered), keys).sum())
        print(f"rate {rate} position {position}: {hits} unfiltered negatives are known facts")
        assert hits > 0 and int(un2.sum()) == 0         # the filter does something
        again, _ = host.negatives_draw(facts, rate, N, N, R, keys, SEED, position)
        assert np.array_equal(out, again)
        outs.append(out)
    assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[1], outs[2])
    other_seed, _ = host.negatives_draw(facts, rate, N, N, R, keys, SEED + 1, 0)
    assert not np.array_equal(outs[0], other_seed)


def test_mirror_sides_candidates_and_global_ids():
    from mrgcn_amd import host
    fx = fixture64()
    facts, keys = fx["facts"], fx["keys"]
    src = np.repeat(facts, 3, axis=0)
    tails, _ = host.negatives_draw(facts, 3, N, N, R, keys, SEED, 0, side=1)
    heads, _ = host.negatives_draw(facts, 3, N, N, R, keys, SEED, 0, side="head")
    assert np.array_equal(tails[:, :2], src[:, :2]) and np.all(tails[:, 2] != src[:, 2])
    assert np.array_equal(heads[:, 1:], src[:, 1:]) and np.all(heads[:, 0] != src[:, 0])
    cand = np.random.default_rng(5).choice(N, 17, replace=False).astype(np.int64)
    out, _ = host.negatives_draw(facts, 3, 17, N, R, keys, SEED, 0, cand=cand)
    changed = np.where(out[:, 0] != src[:, 0], out[:, 0], out[:, 2])
    assert np.isin(changed, cand).all() and len(np.unique(changed)) == 17
    # local ids under a permutation: the same draws, the filter applied to the global triples
    perm = np.random.default_rng(6).permutation(N).astype(np.int64)
    inv = np.argsort(perm)
    local = np.stack([inv[facts[:, 0]], facts[:, 1], inv[facts[:, 2]]], 1)
    out, unresolved = host.negatives_draw(local, 3, N, N, R, keys, SEED, 0, to_global=perm)
    glob = np.stack([perm[out[:, 0]], out[:, 1], perm[out[:, 2]]], 1)
    assert not np.isin(_keys_of(glob), keys).any() and int(unresolved.sum()) == 0
    # the stream is apart from node dropout's under the same seed
    a = host.philox4x32_10((0, 0, 0, 0), (SEED & 0xFFFFFFFF, SEED >> 32))
    b = host.philox4x32_10((0, 0, 0, 0), (SEED & 0xFFFFFFFF, (SEED >> 32) ^ host.NEG_KEY_TAG))
    assert [int(w[0]) for w in a] != [int(w[0]) for w in b]


def test_fact_keys_are_sorted_uint64_and_large_candidate_counts_multiply_exactly():
    from mrgcn_amd import host
    fx = fixture64()
    keys = fx["keys"]
    assert keys.dtype == np.uint64 and np.all(np.diff(keys.astype(np.int64)) > 0) and len(keys) == 500
    assert np.array_equal(keys, np.sort(_keys_of(fx["known"])))
    h = np.array([0, 1, 0xFFFFFFFFFFFFFFFF, 0x8000000000000001, 0x123456789ABCDEF0], dtype=np.uint64)
    for n in (1, 63, 64, (1 << 32) - 1, 1 << 32, (1 << 40) + 12345, (1 << 63) - 1):
        assert host._mul_hi64(h, n).tolist() == [(int(v) * n) >> 64 for v in h], n


def test_second_fixture_resolves_every_negative():
    """The facts of the GPU file's stable-order reproducibility run (2 500 facts, 300 nodes, 5 relations, rate 1,
    sampler seed 4321): no negative is left unresolved at the positions that run takes."""
    from mrgcn_amd import host
    tr = fixture300()
    assert tr.shape == (2500, 3) and len(np.unique(tr, axis=0)) == 2500
    keys = host.fact_keys(tr, 300, 5)
    for position in range(4):
        out, unresolved = host.negatives_draw(tr, 1, 300, 300, 5, keys, FIX300_SAMPLER_SEED, position)
        assert int(unresolved.sum()) == 0
        assert not np.isin(_keys_of(out, 300, 5), keys).any()


# ---- 3. uniformity ---------------------------------------------------------------------------------------------------
def test_mirror_picks_are_uniform_over_the_other_nodes():
    from mrgcn_amd import host
    facts = np.tile(np.array([[0, 0, 1]], dtype=np.int64), (6400, 1))
    out, unresolved = host.negatives_draw(facts, 10, 64, 64, 1, False, 7, 0, side=1)
    assert np.all(out[:, 0] == 0) and np.all(out[:, 1] == 0) and int(unresolved.sum()) == 0
    counts = np.bincount(out[:, 2], minlength=64)
    assert counts[1] == 0 and counts.sum() == 64000
    others = np.delete(counts, 1)
    print("counts of the 63 other nodes: min", others.min(), "max", others.max())
    # 64 000 draws over 63 nodes: mean 1016, standard deviation 31.6
    assert np.all(np.abs(others - 1016) <= 6 * 31.6)


# ---- 4. the flag path ------------------------------------------------------------------------------------------------
def test_mirror_flags_exactly_the_negatives_it_could_not_resolve():
    from mrgcn_amd import host
    facts = flag_case()
    out, unresolved = host.negatives_draw(facts, 4, 8, 8, 1, host.fact_keys(facts, 8, 1), 99, 0, side=0)
    src = np.repeat(facts, 4, axis=0)
    tail_side = out[:, 0] == src[:, 0]
    print("flagged", int(unresolved.sum()), "of", len(out), "tail-side", int(tail_side.sum()))
    assert np.array_equal(unresolved.astype(bool), tail_side)
    assert 0 < int(tail_side.sum()) < len(out)
    assert np.all(out[~tail_side, 0] != 0) and np.array_equal(out[~tail_side, 2], src[~tail_side, 2])


# ---- 5. argument checks ----------------------------------------------------------------------------------------------
def _call(lib, n=4, rate=1, n_cand=8, num_nodes=8, num_relations=1, side=0):
    """The entry with valid-looking host addresses it never gets to use: every case below fails its argument check,
    which answers before the first launch."""
    facts = (C.c_int64 * 12)()
    state = (C.c_int64 * 2)()
    out = (C.c_int64 * 12)()
    return lib.mrgcn_negatives_draw_i64(C.addressof(facts), n, rate, None, n_cand, None, None, 0, num_nodes,
                                        num_relations, side, C.addressof(state), C.addressof(out), None, None)


@pytest.mark.parametrize("bad", [dict(rate=0), dict(n_cand=0), dict(num_nodes=1 << 31, num_relations=2),
                                 dict(num_nodes=3037000500, num_relations=1), dict(n=1 << 55, rate=2),
                                 dict(n=1 << 56, rate=1), dict(side=3), dict(n=-1)],
                         ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_argument_checks_answer_before_any_launch(bad):
    from mrgcn_amd import _lib
    lib = _lib.load()
    assert _call(lib, **bad) == 1    # MRGCN_ERR_INVALID
    assert lib.mrgcn_last_error().decode().startswith("invalid argument")


def test_null_pointers_are_refused():
    from mrgcn_amd import _lib
    lib = _lib.load()
    buf = (C.c_int64 * 12)()
    a = C.addressof(buf)
    for facts, state, out in ((None, a, a), (a, None, a), (a, a, None)):
        assert lib.mrgcn_negatives_draw_i64(facts, 4, 1, None, 8, None, None, 0, 8, 1, 0, state, out, None, None) == 1
