"""Writes tests/golden/early_stop_traces.npz from the reference's own `mrgcn.tasks.utils.EarlyStop` (DEVELOPMENT
MACHINE ONLY: imports the reference tree).

    python tests/golden/make_early_stop_goldens.py

Per trace `t<k>`: `scores` (float64), `patience`, `tolerance`, `delay`, and per record a row of `records`:
(best_score, patience, stop, updated) as float64 — `updated` = the record called `state_dict()` on both of its
arguments (it set the best score).  `best_score` is -1 while none is set.  Scores are non-negative, as losses are: the
reference's `best_score < 0` sentinel makes negative scores another regime, which is left alone.

Every score is rounded to float32 first and handed to the reference as that value widened to a Python float: the
device kernel takes a float32 score and compares in double, so both sides see the same doubles.  The reference class
keeps counting after `stop` (its loop never records again once it is set); the rows behind the first stop record that
only, the device state is latched there."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_goldens import REF, _stub_rdflib  # noqa: E402

_stub_rdflib()
sys.path.insert(0, REF)
from mrgcn.tasks.utils import EarlyStop  # noqa: E402


class _Counted:
    def __init__(self):
        self.calls = 0

    def state_dict(self):
        self.calls += 1
        return {}


f32 = np.float32
TRACES = [
    # best set at record 3, stop at record 6: nothing beats a tolerance of 10
    ("flat_tol10", [5, 5, 5, 4, 4, 4, 4, 4, 4, 4], 3, 10.0, 2),
    # updates at records 1, 2, 4, 5; stop at record 8
    ("improving", [1.0, .9, .895, .88, .5, .6, .7, .8], 3, 0.01, 0),
    ("patience1", [2.0, 1.0, 0.5, 0.5, 0.1], 1, 0.01, 0),
    ("default_delay", [3.0 - 0.1 * i for i in range(12)] + [2.5] * 10, 7, 0.01, 10),
    # record 4 improves while patience is 1: patience is given back, no stop
    ("improve_at_patience1", [1.0, 1.0, 1.0, 0.5, 0.5, 0.5, 0.5], 3, 0.01, 0),
    # 0.75 + 0.25 == 1.0 exactly: strict <, not an improvement; 0.5 is one
    ("exactly_best_minus_tol", [1.0, 0.75, 0.5, 0.25, 0.25, 0.25], 2, 0.25, 0),
    # float32 losses widened to double (0.1f + 0.01 against 0.11f, ...)
    ("float32_widened", [float(f32(x)) for x in (0.7, 0.11, 0.1, 0.1 - 0.0100001, 0.3, 0.05, 0.2, 0.2, 0.2)], 3,
     0.01, 1),
    ("nan_score", [1.0, 0.5, float("nan"), 0.2, 0.3, 0.3, 0.3], 3, 0.01, 0),
    ("nan_first", [float("nan"), 0.5, 0.4, 0.3], 3, 0.01, 0),
]


def main():
    out = {"names": np.array([t[0] for t in TRACES])}
    for name, scores, patience, tolerance, delay in TRACES:
        es = EarlyStop(patience, tolerance, delay)
        rows = []
        scores = [float(f32(s)) for s in scores]
        for s in scores:
            w, o = _Counted(), _Counted()
            es.record(float(s), w, o)
            assert w.calls == o.calls and w.calls in (0, 1)
            rows.append((float(es.best_score), float(es.patience), float(bool(es.stop)), float(w.calls)))
        out[f"{name}.scores"] = np.asarray(scores, dtype=np.float64)
        out[f"{name}.config"] = np.asarray([patience, tolerance, delay], dtype=np.float64)
        out[f"{name}.records"] = np.asarray(rows, dtype=np.float64)
    np.savez(os.path.join(HERE, "early_stop_traces.npz"), **out)
    for name, *_ in TRACES:
        print(name, out[f"{name}.records"].tolist())


if __name__ == "__main__":
    main()
