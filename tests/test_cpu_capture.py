"""The capture helper (`train.Captured`) and what was folded around it, without a device: the capture calls occur in
`train.py`'s helper only, every graphed class refuses an optimizer that is not capturable before it touches CUDA, the
poll loop of the two node-classification `fit`s on fakes, and the record `_decoder_args` resolves the link-prediction
keywords to."""
import ast
import os
from collections import namedtuple

import pytest
import torch

from mrgcn_amd import partition, train
from mrgcn_amd._lib import MrgcnError
from mrgcn_amd.tasks import link_prediction as lp
from mrgcn_amd.tasks import node_classification as nc
from tests.test_cpu_host import ROOT


def _dotted(node):
    parts = []
    while isinstance(node, ast.Attribute):
        parts.append(node.attr)
        node = node.value
    return ".".join(reversed(parts + [node.id])) if isinstance(node, ast.Name) else None


def test_stream_captures_occur_in_the_helper_only():
    """An eighth hand-kept copy of the capture discipline fails here: `torch.cuda.graph(...)` and
    `torch.cuda.CUDAGraph()` are called once each, inside `train.Captured`."""
    sites = []
    pkg = os.path.join(ROOT, "mrgcn_amd")
    for folder, _, files in os.walk(pkg):
        for f in sorted(files):
            if not f.endswith(".py"):
                continue
            path = os.path.join(folder, f)
            tree = ast.parse(open(path).read(), path)
            owner = {}
            for top in ast.walk(tree):
                if isinstance(top, ast.ClassDef):
                    for sub in ast.walk(top):
                        owner[id(sub)] = top.name
            for node in ast.walk(tree):
                if isinstance(node, ast.Call) and _dotted(node.func) in ("torch.cuda.graph", "torch.cuda.CUDAGraph"):
                    sites.append((os.path.relpath(path, pkg), owner.get(id(node)), _dotted(node.func)))
    assert sorted(sites) == [("train.py", "Captured", "torch.cuda.CUDAGraph"),
                             ("train.py", "Captured", "torch.cuda.graph")], sites
    # (no other spelling of the two names either: an alias or a `from torch.cuda import graph` would hide a site)
    for folder, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py") and f != "train.py":
                src = open(os.path.join(folder, f)).read()
                assert "CUDAGraph(" not in src and "cuda.graph(" not in src and "import graph" not in src, f


def test_capturability_is_checked_before_the_device_is_touched(monkeypatch):
    """Six of the seven graphed classes take an optimizer (`GraphedStep` takes a bare callable and has nothing to
    refuse): each raises its own exception type, naming `capturable`, while CUDA is still untouched."""
    def touched(*a, **k):
        raise AssertionError("the device was touched before the capturability check")
    for name in ("Stream", "current_stream", "synchronize", "CUDAGraph", "graph"):
        monkeypatch.setattr(torch.cuda, name, touched)

    class Smp:
        facts = None
    opt = object()
    builds = [
        (MrgcnError, lambda: train.GraphedTrainStep(None, None, None, None, opt)),
        (MrgcnError, lambda: train.GraphedTrainEvalStep(None, None, None, None, opt)),
        (MrgcnError, lambda: nc.GraphedBatchEpoch(None, None, None, opt)),
        (MrgcnError, lambda: lp.FitEpochs(None, None, None, None, opt, sampler=Smp())),
        (MrgcnError, lambda: lp.BatchFitEpochs(None, [(None, None)], None, opt, samplers=lambda i, b, f: Smp())),
        (RuntimeError, lambda: partition.GraphedPartitionedStep(None, None, None, None, opt)),
    ]
    for exc, build in builds:
        with pytest.raises(exc, match="capturable") as e:
            build()
        assert type(e.value) is exc
    assert not torch.cuda.is_initialized()


Read = namedtuple("Read", "records stop")


class _FakeRun:
    """Epoch e (from 1) writes the row (e, 10 e, 100 e, 1000 e) at `records % poll` unless the stop is latched, which
    the record `stop_at` does — a DeviceEarlyStop's and a metrics ring's behaviour on the host."""

    def __init__(self, poll, stop_at=None):
        self.ring = torch.zeros((poll, 4))
        self.calls = self.records = self.restores = 0
        self.stop, self.stop_at = False, stop_at

    def __call__(self):
        self.calls += 1
        if self.stop:
            return
        e = self.calls
        self.ring[self.records % self.ring.shape[0]] = torch.tensor([e, 10.0 * e, 100.0 * e, 1000.0 * e])
        self.records += 1
        self.stop = self.records == self.stop_at

    def read(self):
        return Read(self.records, self.stop)

    def restore_(self):
        self.restores += 1


def test_poll_records_yields_up_to_the_stop_and_restores_once():
    run = _FakeRun(3, stop_at=5)
    rows = list(train._poll_records(run, run, run.ring, 7, 3, run))
    assert rows == [(e, float(e), 10.0 * e, 100.0 * e, 1000.0 * e) for e in range(1, 6)]
    assert run.calls == 6 and run.restores == 1


def test_poll_records_without_a_stop_yields_every_epoch_and_restores_nothing():
    run = _FakeRun(3)
    rows = list(train._poll_records(run, run, run.ring, 7, 3, run))
    assert rows == [(e, float(e), 10.0 * e, 100.0 * e, 1000.0 * e) for e in range(1, 8)]
    assert run.calls == 7 and run.restores == 0


def test_both_node_classification_fits_end_in_the_poll_generator():
    for fit in (train.fit, nc.fit):
        last = ast.parse(_source(fit)).body[0].body[-1]
        assert isinstance(last, ast.Expr) and isinstance(last.value, ast.YieldFrom)
        assert _dotted(last.value.value.func).rsplit(".", 1)[-1] == "_poll_records"


def _source(fn):
    import inspect
    import textwrap
    return textwrap.dedent(inspect.getsource(fn))


def test_decoder_args_returns_an_immutable_record():
    rec = lp._decoder_args("triples", "bce", None, [], "t", "complex")
    assert rec == ("triples", "bce", None, "complex", 0.0) and type(rec) is lp._Decoder
    rec = lp._decoder_args("grouped", "softmax", None, [], "t")
    assert (rec.kind, rec.loss, rec.pos_weight, rec.scorer, rec.label_smoothing) == \
        ("grouped", "softmax", None, "distmult", 0.0)
    rec = lp._decoder_args("grouped", "bce", torch.tensor(2), [], "t")
    assert rec.pos_weight == 2.0 and type(rec.pos_weight) is float
    rec = lp._decoder_args("all", "softmax", None, [], "t")
    assert (rec.kind, rec.loss, rec.pos_weight, rec.label_smoothing) == ("all", "softmax", None, 0.0)
    rec = lp._decoder_args("kvsall", "bce", None, [], "t", "complex", 0.1)
    assert (rec.kind, rec.loss, rec.pos_weight, rec.scorer) == ("kvsall", "bce", None, "complex")
    assert rec.label_smoothing == 0.1 and type(rec.label_smoothing) is float
    with pytest.raises(AttributeError):
        rec.loss = "softmax"
    with pytest.raises(AttributeError):
        rec.extra = 1
    # a resolved record passes through as it is, and its samplers are still checked
    assert lp._decoder_args(rec, "hinge", 3.0, [], "t") is rec
    with pytest.raises(MrgcnError, match="facts"):
        lp._decoder_args(rec, "bce", None, [lambda: None], "t")
