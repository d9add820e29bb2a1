"""Host side of early stopping: `mrgcn_amd.train.EarlyStop` against traces of the reference's own class
(tests/golden/make_early_stop_goldens.py), its place under `mrgcn.tasks.utils` after `install_as_mrgcn()`, and the
parameter groups of `mrgcn_amd.tasks.utils.optimizer_params`."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.util import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACES = np.load(os.path.join(GOLDEN, "early_stop_traces.npz"))
NAMES = [str(n) for n in TRACES["names"]]


class _Counted:
    def __init__(self):
        self.calls = 0

    def state_dict(self):
        self.calls += 1
        return {"calls": self.calls}


def test_the_golden_holds_the_traces_the_feature_was_specified_with():
    assert len(NAMES) >= 8
    r = TRACES["flat_tol10.records"]   # best at record 3, stop at record 6
    assert r[2, 3] == 1 and r[:, 3].sum() == 1 and np.flatnonzero(r[:, 2])[0] == 5
    r = TRACES["improving.records"]    # updates at records 1, 2, 4, 5; stop at record 8
    assert list(np.flatnonzero(r[:, 3]) + 1) == [1, 2, 4, 5] and np.flatnonzero(r[:, 2])[0] == 7
    r = TRACES["improve_at_patience1.records"]   # record 4 lands at patience 1 and does not stop
    assert r[2, 1] == 1 and r[3, 3] == 1 and r[3, 2] == 0
    r = TRACES["exactly_best_minus_tol.records"]   # strict <
    assert r[1, 3] == 0 and r[2, 3] == 1


@pytest.mark.parametrize("name", NAMES)
def test_host_early_stop_replays_the_reference_trace_field_for_field(name):
    from mrgcn_amd.train import EarlyStop
    patience, tolerance, delay = TRACES[f"{name}.config"]
    es = EarlyStop(int(patience), float(tolerance), int(delay))
    assert es.stop is False and es.best_score == -1 and es.best_weights is None and es.best_optim is None
    for k, (score, want) in enumerate(zip(TRACES[f"{name}.scores"], TRACES[f"{name}.records"])):
        w, o = _Counted(), _Counted()
        es.record(float(score), w, o)
        best, pat, stop, updated = want
        assert (w.calls, o.calls) == (int(updated), int(updated)), (name, k)
        assert np.array_equal(np.float64(es.best_score), best, equal_nan=True), (name, k)
        assert es.patience == int(pat) and es.stop is bool(stop), (name, k)
        if updated:
            assert es.best_weights == {"calls": 1} and es.best_optim == {"calls": 1}


def test_defaults_are_the_reference_constructor():
    from mrgcn_amd.train import EarlyStop
    es = EarlyStop()
    assert (es.patience, es.tolerance, es.delay) == (7, 0.01, 10)


def test_early_stop_is_reachable_as_mrgcn_tasks_utils(tmp_path):
    """`install_as_mrgcn()` answers for the leaf `mrgcn.tasks.utils` wherever a `mrgcn.tasks` package exists (here a
    bare stand-in for the reference installation; its own `utils` must lose against the alias)."""
    pkg = tmp_path / "mrgcn" / "tasks"
    pkg.mkdir(parents=True)
    (tmp_path / "mrgcn" / "__init__.py").write_text("")
    (pkg / "__init__.py").write_text("")
    (pkg / "utils.py").write_text("raise ImportError('the installation\\'s own module was imported')\n")
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import mrgcn_amd; mrgcn_amd.install_as_mrgcn();"
            "import mrgcn.tasks.utils; from mrgcn.tasks.utils import EarlyStop, optimizer_params;"
            "import mrgcn_amd.train as t; assert mrgcn.tasks.utils.EarlyStop is t.EarlyStop;"
            "assert mrgcn.tasks.utils.__name__ == 'mrgcn_amd.tasks.utils'; print('ok')" % (ROOT, str(tmp_path)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_optimizer_params_groups():
    """tasks/utils.py:8-45: default group, the gates' group, one group per encoder datatype, frozen parameters out."""
    from mrgcn_amd.tasks.utils import optimizer_params

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.gate_weights = torch.nn.Parameter(torch.zeros(3))
            self.rgcn = torch.nn.Linear(2, 2)
            self.module_dict = torch.nn.ModuleDict({"xsd_string_0": torch.nn.Linear(2, 2),
                                                    "xsd_string_1": torch.nn.Linear(2, 2, bias=False),
                                                    "ogc_wktLiteral_0": torch.nn.Linear(2, 2)})
            self.rgcn.bias.requires_grad_(False)
    m = M()
    cfg = {"gate_weights": {"lr": 0.5}, "xsd.string": {"lr": 0.25}, "ogc.wktLiteral": {"weight_decay": 0.125}}
    groups = optimizer_params(m, cfg, False)
    assert [len(g["params"]) for g in groups] == [1, 1, 3, 2]
    assert groups[0]["params"][0] is m.rgcn.weight and set(groups[0]) == {"params"}
    assert groups[1]["params"][0] is m.gate_weights and groups[1]["lr"] == 0.5
    assert groups[2]["lr"] == 0.25 and groups[3]["weight_decay"] == 0.125
    groups = optimizer_params(m, {"xsd.string": {}, "ogc.wktLiteral": {}}, True)   # featureless: gates are ordinary
    assert [len(g["params"]) for g in groups] == [2, 3, 2]
