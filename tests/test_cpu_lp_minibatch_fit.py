"""The arithmetic of the mini-batch link-prediction rows, without a GPU: the golden's per-batch lists
(make_lp_minibatch_fit_goldens.py) give its rows by UNWEIGHTED means over batches (link_prediction.py:331, :416-419) —
not by fact-weighted ones, which the golden tells apart —, `eval_schedule` gives its None pattern, and the entry points
of csrc/lp_batches.hip are declared in the header and the ctypes table."""
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "lp_minibatch_fit.npz")
NAMES = [f"{k}.{m}" for k in ("raw", "flt") for m in ("mrr", "h1", "h3", "h10")]   # the order of a row's eight


@pytest.mark.parametrize("tag", ["nb17", "nb13", "nb13_stop"])
def test_rows_are_unweighted_means_over_batches(tag):
    g = np.load(GOLD)
    epoch = int(g[f"{tag}.first_eval.epoch"])
    row = g[f"{tag}.rows"][g[f"{tag}.epochs"].tolist().index(epoch)]
    losses = g[f"{tag}.first_eval.loss"]
    assert len(losses) == int(g[f"{tag}.train.count"])
    assert row[0] == np.mean(losses)
    differs = False
    for s, split in enumerate(("train", "valid")):
        n = int(g[f"{tag}.{split}.count"])
        weights = np.asarray([len(g[f"{tag}.{split}.{i}.facts"]) for i in range(n)], dtype=np.float64)
        assert len(set(weights.tolist())) > 1       # batches of different sizes: the two means can differ
        for k, name in enumerate(NAMES):
            per_batch = g[f"{tag}.first_eval.{split}.{name}"]
            assert len(per_batch) == n
            assert row[1 + 8 * s + k] == np.mean(per_batch), (split, name)
            differs |= abs(np.average(per_batch, weights=weights) - np.mean(per_batch)) > 1e-4
    assert differs   # (a fact-weighted mean would not reproduce the rows)


def test_intervals_hold_the_rows():
    g = np.load(GOLD)
    for tag in ("nb17", "nb13", "nb13_stop"):
        rows, lo, hi = g[f"{tag}.rows"], g[f"{tag}.rows_lo"], g[f"{tag}.rows_hi"]
        ok = ~np.isnan(rows)
        assert np.all(lo[ok] <= rows[ok] + 1e-6) and np.all(rows[ok] <= hi[ok] + 1e-6)
        assert float((hi - lo)[ok].max()) <= 0.02 and float(g["tau"]) >= 1e-4


@pytest.mark.parametrize("tag,interval", [("nb17", 2), ("nb13", 2), ("nb13_stop", 1)])
def test_eval_schedule_is_the_goldens_none_pattern(tag, interval):
    from mrgcn_amd.tasks.link_prediction import eval_schedule
    g = np.load(GOLD)
    rows, epochs = g[f"{tag}.rows"], g[f"{tag}.epochs"].tolist()
    sched = {e: (t, v) for e, t, v, _ in eval_schedule(6, interval, True)}
    for e, row in zip(epochs, rows):
        assert (not np.isnan(row[1]), not np.isnan(row[9])) == sched[e], e
    if tag == "nb13_stop":
        assert epochs == [1, 2, 3]   # stopped at record 3
        pre = "nb13_stop.epoch1."
        for k in [k for k in g.files if k.startswith(pre)]:
            assert np.array_equal(g[k], g["nb13_stop.final." + k[len(pre):]])   # and restored epoch 1's state


def test_entry_points_are_declared():
    from mrgcn_amd import _lib
    with open(os.path.join(ROOT, "include", "mrgcn_hip.h")) as f:
        header = f.read()
    for name in ("mrgcn_distmult_batch_eval_workspace", "mrgcn_distmult_batch_eval", "mrgcn_lp_batch_means_f32"):
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["mrgcn_distmult_batch_eval"][1]) == 18
    assert len(_lib.SIGNATURES["mrgcn_lp_batch_means_f32"][1]) == 9
