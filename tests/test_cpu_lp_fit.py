"""Host side of the link-prediction run loop (mrgcn_amd.tasks.link_prediction.fit): the new C ABI entries are
declared everywhere, `eval_schedule` restates the reference's three conditions, `FactParts` cuts the facts as
`mkbatches` does in full-batch mode and filters every part by its own facts.  No GPU."""
import os
import re

import numpy as np
import pytest

from oracle import lp_oracle as lo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mrgcn_distmult_ranks_both_workspace", "mrgcn_distmult_ranks_both", "mrgcn_rank_metrics",
       "mrgcn_early_stop_record_row"]


def test_new_entries_are_declared_and_bound_and_the_abi_version_stays():
    from mrgcn_amd import _lib
    src = open(os.path.join(ROOT, "include", "mrgcn_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mrgcn_[a-z0-9_]+)\s*\(", src))
    for name in NEW + ["mrgcn_distmult_ranks_both_slice"]:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
    assert _lib.ABI_VERSION == 5
    assert re.search(r"#define\s+MRGCN_ABI_VERSION\s+5\b", open(os.path.join(ROOT, "include", "mrgcn_hip.h")).read())
    lib = _lib.load()
    assert lib.mrgcn_abi_version() == 5
    for name in NEW:
        assert hasattr(lib, name), name
    # the workspace: Et [H, N] + truth [nf] floats, scored [nf] + counts [8 nf] int32; the slice is whole tiles of 8
    assert lib.mrgcn_distmult_ranks_both_workspace(10, 3, 7) == 4 * (30 + 7) + 4 * 9 * 7
    assert lib.mrgcn_distmult_ranks_both_workspace(10, 0, 7) == -1
    assert 0 < lib.mrgcn_distmult_ranks_both_slice() <= 524280 and lib.mrgcn_distmult_ranks_both_slice() % 8 == 0


@pytest.mark.parametrize("has_valid", [False, True])
@pytest.mark.parametrize("eval_interval", [1, 2, 5, 7])
@pytest.mark.parametrize("nepoch", [1, 5, 12])
def test_eval_schedule_is_the_reference_loop(nepoch, eval_interval, has_valid):
    from mrgcn_amd.tasks import link_prediction as lp
    want = []
    for epoch in range(1, nepoch + 1):
        train = valid = record = False
        if epoch % eval_interval == 0 or epoch == nepoch:          # link_prediction.py:336
            train = True
            if has_valid and epoch < nepoch:                        # :350
                valid = True
                record = True                                       # :362 (with an early_stop)
        want.append((epoch, train, valid, record))
    assert lp.eval_schedule(nepoch, eval_interval, has_valid) == want
    assert want[-1][1] and not want[-1][2]


@pytest.mark.parametrize("n,bs", [(700, 100), (333, 100), (99, 100), (1100, 100), (250, 7), (5, 1), (64, 0)])
def test_fact_parts_cut_and_filter_like_mkbatches(n, bs):
    from mrgcn_amd.tasks import link_prediction as lp
    rng = np.random.default_rng(n + bs)
    facts = np.stack([rng.integers(0, 40, n), rng.integers(0, 3, n), rng.integers(0, 40, n)], 1).astype(np.int64)
    facts[n // 2:, 0] = facts[: n - n // 2, 0]   # shared (s, p) pairs: non-empty lists
    facts[n // 2:, 1] = facts[: n - n // 2, 1]
    parts = lp.FactParts(facts, bs, device="cpu")
    split = np.array_split(np.arange(n), max(n // (bs if bs > 0 else n), 1))
    assert parts.sizes == [len(s) for s in split] and parts.nparts == len(split) and parts.n == n
    ptr = parts.part_ptr.numpy()
    assert np.array_equal(ptr, np.concatenate([[0], np.cumsum(parts.sizes)]))
    assert np.array_equal(parts.facts.numpy(), facts)
    tp, ti, hp, hi = (a.numpy() for a in parts.lists)
    assert tp.dtype == hp.dtype == np.int64 and ti.dtype == hi.dtype == np.int32
    assert len(tp) == len(hp) == n + 1 and tp[0] == hp[0] == 0 and tp[-1] == len(ti) and hp[-1] == len(hi)
    nonempty = 0
    for p in range(parts.nparts):
        a, b = ptr[p], ptr[p + 1]
        otp, oti, ohp, ohi = lo.filter_lists(facts[a:b])
        assert np.array_equal(tp[a:b + 1] - tp[a], otp) and np.array_equal(ti[tp[a]:tp[b]], oti), p
        assert np.array_equal(hp[a:b + 1] - hp[a], ohp) and np.array_equal(hi[hp[a]:hp[b]], ohi), p
        nonempty += len(oti)
    assert nonempty > 0 or n < 10
    assert lp.FactParts(facts, bs, filtered=False, device="cpu").lists is None
