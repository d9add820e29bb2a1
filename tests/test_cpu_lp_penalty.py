"""The L1 / L2 weight penalty of the link-prediction loops without a GPU: the two penalty entry points and their
workspace query at the C ABI (csrc/optim.hip) are declared in the header, listed in the ctypes table with matching
argument counts and exported by the built library; the owner selection of tasks.link_prediction picks exactly the
`weight`-named parameters and owns nothing off the device; `eval_schedule` is what it was.  No compute call is made."""
import ctypes as C
import inspect
import os
import re

import torch

from tests.test_cpu_host import ROOT, header_functions

NAMES = ("mrgcn_penalty_norm_workspace", "mrgcn_penalty_norm_multi_f32", "mrgcn_adam_step_reg_multi_f32")


def _declared_argument_count(name):
    src = open(os.path.join(ROOT, "include", "mrgcn_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    args = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", src).group(1).strip()
    return 0 if args in ("", "void") else len(args.split(","))


def test_the_symbols_are_in_header_ctypes_table_and_library():
    from mrgcn_amd import _lib
    declared = set(header_functions())
    lib = _lib.load()
    for n in NAMES:
        assert n in declared, f"{n} is not declared in include/mrgcn_hip.h"
        assert n in _lib.SIGNATURES, f"{n} is not in the ctypes table"
        assert hasattr(lib, n), f"{n} is not exported by the library"
        assert len(_lib.SIGNATURES[n][1]) == _declared_argument_count(n), n
    assert _lib.SIGNATURES["mrgcn_penalty_norm_workspace"][0] is C.c_int64
    # l1, l2 travel as floats in both; the Adam entry adds beta1, beta2, eps
    assert _lib.SIGNATURES["mrgcn_penalty_norm_multi_f32"][1].count(C.c_float) == 2
    assert len(_lib.SIGNATURES["mrgcn_penalty_norm_multi_f32"][1]) == 12
    assert _lib.SIGNATURES["mrgcn_adam_step_reg_multi_f32"][1].count(C.c_float) == 5
    assert len(_lib.SIGNATURES["mrgcn_adam_step_reg_multi_f32"][1]) == 19
    # three double partials per block, a whole number of them
    ws = int(lib.mrgcn_penalty_norm_workspace())
    assert ws > 0 and ws % 24 == 0


class _Net(torch.nn.Module):
    """Parameter names as a bare RGCN's and as an MRGCN's (`rgcn.` prefix), one frozen weight, one float64 weight."""

    def __init__(self):
        super().__init__()
        self.weight_I = torch.nn.Parameter(torch.randn(5, 2, 4))
        self.weight_I_comp = torch.nn.Parameter(torch.randn(3, 2))
        self.relations = torch.nn.Parameter(torch.randn(3, 4))
        self.b = torch.nn.Parameter(torch.zeros(4))
        self.rgcn = torch.nn.Module()
        self.rgcn.weight_F = torch.nn.Parameter(torch.randn(4, 4))
        self.rgcn.bias = torch.nn.Parameter(torch.zeros(4))
        self.frozen_weight = torch.nn.Parameter(torch.randn(2), requires_grad=False)
        self.wide_weight = torch.nn.Parameter(torch.randn(2, dtype=torch.float64))
        self.unstepped_weight = torch.nn.Parameter(torch.randn(2))


def test_owner_selection():
    from mrgcn_amd.optim import RowSparseAdam
    from mrgcn_amd.tasks import link_prediction as lp
    from mrgcn_amd.train import ClipAdam
    net = _Net()
    stepped = [p for n, p in net.named_parameters() if n != "unstepped_weight"]
    clip = ClipAdam(stepped, lr=0.01, max_norm=1.0)
    # CPU parameters: the optimizer owns nothing (the penalty kernels are device code)
    assert lp.penalty_owners(net, clip) == []
    # the rule without the device condition: `weight` in the name, stepped, requires grad, float32
    got = {id(p) for p in lp.penalty_owners(net, clip, on_device=False)}
    want = {n for n, p in net.named_parameters() if id(p) in got}
    assert want == {"weight_I", "weight_I_comp", "rgcn.weight_F"}, want
    # nothing for an optimizer that does not clip inside its step, a distributed one, or another class
    assert lp.penalty_owners(net, ClipAdam(stepped, lr=0.01, max_norm=None), on_device=False) == []
    assert lp.penalty_owners(net, RowSparseAdam(stepped, lr=0.01), on_device=False) == []
    assert lp.penalty_owners(net, torch.optim.Adam(stepped, lr=0.01), on_device=False) == []
    rs = RowSparseAdam(stepped, lr=0.01)
    rs.max_norm = 1.0   # (a row-sparse optimizer that clips in its step owns them too)
    assert {id(p) for p in lp.penalty_owners(net, rs, on_device=False)} == got
    clip.set_distributed(object(), [])
    assert lp.penalty_owners(net, clip, on_device=False) == []


def test_the_entry_points_take_the_penalty_arguments():
    from mrgcn_amd.optim import ClipAdam
    from mrgcn_amd.tasks import link_prediction as lp
    for fn in (lp.train_step, lp.train_batch_step, lp.train_epoch, lp.fit, lp.fit_batches, lp.FitEpochs.__init__,
               lp.BatchFitEpochs.__init__):
        sig = inspect.signature(fn).parameters
        assert sig["l1_lambda"].default == 0 and sig["l2_lambda"].default == 0, fn
    assert inspect.signature(ClipAdam.step).parameters["dense_penalty"].default == "torch"
    assert "Out of scope: the loop's l1_lambda" not in lp.fit_batches.__doc__


def test_eval_schedule_is_unchanged():
    from mrgcn_amd.tasks import link_prediction as lp
    assert lp.eval_schedule(4, 2, True) == [(1, False, False, False), (2, True, True, True), (3, False, False, False),
                                            (4, True, False, False)]
    assert lp.eval_schedule(3, 1, False) == [(1, True, False, False), (2, True, False, False), (3, True, False, False)]
    assert lp.eval_schedule(5, 3, True) == [(1, False, False, False), (2, False, False, False), (3, True, True, True),
                                            (4, False, False, False), (5, True, False, False)]
