"""Edge dropout without a GPU: the host mirror of the device draw (mrgcn_amd.host.edge_dropout_values), the model's
setter and its refusals, state_dict keys, and the C ABI's declarations."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests.test_cpu_host import header_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, N = 7, 1000
SEED, POS = 0x1234_5678_9ABC_DEF0, (3 << 32) | 17
NEW = ("mrgcn_plan_create_overlay", "mrgcn_plan_is_overlay", "mrgcn_edge_dropout_draw_f32")


def _coords(n=20000, seed=0):
    rng = np.random.default_rng(seed)
    rows, nodes, rels = rng.integers(0, N, n), rng.integers(0, N, n), rng.integers(0, R, n)
    vals = rng.uniform(0.1, 1.0, n).astype(np.float32)
    return rows, nodes, rels, vals


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


# ---- the mirror --------------------------------------------------------------------------------------------------------
def test_equal_inputs_give_equal_output_whatever_the_order():
    from mrgcn_amd import host
    rows, nodes, rels, vals = _coords()
    rates = [0.4] * (R - 1) + [0.2]
    a = host.edge_dropout_values(rows, nodes, rels, vals, rates, SEED, POS, 1)
    b = host.edge_dropout_values(rows, nodes, rels, vals, rates, SEED, POS, 1)
    assert a.dtype == np.float32 and np.array_equal(_bits(a), _bits(b))
    perm = np.random.default_rng(1).permutation(len(rows))   # a value depends on its coordinates, not on its place
    c = host.edge_dropout_values(rows[perm], nodes[perm], rels[perm], vals[perm], rates, SEED, POS, 1)
    assert np.array_equal(_bits(c), _bits(a[perm]))


def test_the_draw_is_the_philox_word_below_the_threshold_and_one_fp32_multiply():
    from mrgcn_amd import host
    rows, nodes, rels, vals = _coords(500)
    rates = np.array([0.1, 0.25, 0.4, 0.5, 0.7, 0.9, 0.2], np.float32)
    out = host.edge_dropout_values(rows, nodes, rels, vals, rates, SEED, POS, 5)
    for e in range(0, 500, 7):
        w = host.philox4x32_10((int(rows[e]), int(nodes[e]), int(rels[e]) | (5 << 24), POS & 0xFFFFFFFF),
                               (SEED & 0xFFFFFFFF, (SEED >> 32) ^ (POS >> 32) ^ host.EDGE_KEY_TAG))
        p = rates[rels[e]]
        if int(w[0][0]) < int(float(p) * 4294967296.0):
            assert out[e] == 0.0
        else:
            assert out[e] == np.float32(vals[e] * (np.float32(1) / np.float32(np.float32(1) - p)))
    assert host.EDGE_KEY_TAG != host.NEG_KEY_TAG


def test_rate_zero_is_the_identity_on_the_bits():
    from mrgcn_amd import host
    rows, nodes, rels, vals = _coords()
    vals[:4] = [-0.0, np.float32(1e-42), np.inf, -3.5]
    out = host.edge_dropout_values(rows, nodes, rels, vals, [0.0] * R, SEED, POS, 0)
    assert np.array_equal(_bits(out), _bits(vals))


def test_a_zero_for_the_last_relation_leaves_exactly_its_entries_untouched():
    from mrgcn_amd import host
    rows, nodes, rels, vals = _coords()
    out = host.edge_dropout_values(rows, nodes, rels, vals, [0.4] * (R - 1) + [0.0], SEED, POS, 0)
    last = rels == R - 1
    assert np.array_equal(_bits(out[last]), _bits(vals[last]))
    assert np.all(_bits(out[~last]) != _bits(vals[~last]))   # dropped (0.0) or rescaled (a / 0.6 != a for a > 0)


@pytest.mark.parametrize("what", ["layer", "position", "seed"])
def test_another_layer_position_or_seed_gives_another_mask(what):
    from mrgcn_amd import host
    rows, nodes, rels, vals = _coords()
    base = dict(seed=SEED, position=POS, layer=0)
    other = dict(base)
    other[what] = {"layer": 1, "position": POS + 1, "seed": SEED ^ 1}[what]
    a = host.edge_dropout_values(rows, nodes, rels, vals, [0.4] * R, **base) == 0
    b = host.edge_dropout_values(rows, nodes, rels, vals, [0.4] * R, **other) == 0
    # independent masks at p = 0.4 disagree on 2 p (1 - p) = 48 % of the entries
    assert 0.40 < float((a != b).mean()) < 0.56
    hi = dict(base, position=POS + (1 << 32))   # the position's high word reaches the key
    c = host.edge_dropout_values(rows, nodes, rels, vals, [0.4] * R, **hi) == 0
    assert 0.40 < float((a != c).mean()) < 0.56


def test_without_rescaling_kept_entries_hold_the_stored_values():
    from mrgcn_amd import host
    rows, nodes, rels, vals = _coords()
    out = host.edge_dropout_values(rows, nodes, rels, vals, [0.4] * R, SEED, POS, 0, rescale=False)
    scaled = host.edge_dropout_values(rows, nodes, rels, vals, [0.4] * R, SEED, POS, 0)
    kept = out != 0
    assert np.array_equal(_bits(out[kept]), _bits(vals[kept])) and np.array_equal(kept, scaled != 0)
    keep = np.float32(1) / np.float32(1 - np.float32(0.4))
    assert np.array_equal(_bits(scaled[kept]), _bits((vals[kept] * keep).astype(np.float32)))


def test_the_dropped_share_lies_within_five_sigma_of_p():
    from mrgcn_amd import host
    n, p = 20000, 0.4
    rows, nodes, rels, vals = _coords(n, seed=3)
    out = host.edge_dropout_values(rows, nodes, rels, vals, [p] * R, SEED, POS, 0)
    sigma = np.sqrt(p * (1 - p) / n)
    assert abs(float((out == 0).mean()) - p) <= 5 * sigma


def test_the_mirror_refuses_what_the_device_refuses():
    from mrgcn_amd import host
    rows, nodes, rels, vals = _coords(10)
    with pytest.raises(ValueError):
        host.edge_dropout_values(rows, nodes, rels, vals, [0.4] * R, SEED, POS, 256)
    with pytest.raises(ValueError):
        host.edge_dropout_values(rows, nodes, rels, vals, [0.4] * (R - 1) + [1.0], SEED, POS, 0)
    with pytest.raises(ValueError):
        host.edge_dropout_values(rows, nodes, rels, vals, [0.4] * (R - 1), SEED, POS, 0)   # a relation without a rate


# ---- the model's interface ---------------------------------------------------------------------------------------------
def _model(lp=False):
    from mrgcn_amd.models.rgcn import RGCN
    torch.manual_seed(0)
    return RGCN([(0, 16, "mrgcn", nn.ReLU()), (16, 4, "mrgcn", None)], R, 50, 2, 0.0, True, True, lp)


def test_setter_rates_and_validation():
    from mrgcn_amd._lib import MrgcnError
    m = _model()
    assert m.set_edge_dropout(0.4, self_loop=0.2) is m
    assert m._edge_rates == [0.4] * (R - 1) + [0.2] and m._edge_dropout_active()
    m.set_edge_dropout(0.3)
    assert m._edge_rates == [0.3] * R
    m.set_edge_dropout(rates=[0.1, 0.0, 0.2, 0.0, 0.3, 0.0, 0.5], rescale=False)
    assert m._edge_rates[4] == 0.3 and m._edge_rescale is False
    m.eval()
    assert not m._edge_dropout_active()
    m.train()
    m.set_edge_dropout(0.0)
    assert m._edge_rates is None and not m._edge_dropout_active()
    for bad in (dict(p=1.0), dict(p=-0.1), dict(p=0.4, self_loop=1.5), dict(rates=[0.4] * (R - 1)),
                dict(rates=[0.4] * (R - 1) + [1.0]), dict(rates=[float("nan")] * R)):
        with pytest.raises(ValueError):
            m.set_edge_dropout(**bad)
    m.set_engine("literal")
    with pytest.raises(MrgcnError, match="fused engine"):
        m.set_edge_dropout(0.4)
    m.set_edge_dropout(0.0)   # (turning it off is fine on any engine)


def test_state_of_its_own_and_state_dict_keys_unchanged():
    m = _model(lp=True)
    keys = list(m.state_dict().keys())
    m.set_edge_dropout(0.4, self_loop=0.2, seed=99)
    assert list(m.state_dict().keys()) == keys
    assert not any("edge" in k for k, _ in list(m.named_parameters()) + list(m.named_buffers()))
    assert m.edge_dropout_seed == 99 and m.edge_dropout_position == 0
    m.edge_dropout_position = 12
    m.edge_dropout_seed = (1 << 64) - 1
    assert m.edge_dropout_position == 12 and m.edge_dropout_seed == (1 << 64) - 1
    assert m.node_dropout_position == 0   # (node dropout's state is another one)
    import copy
    m2 = copy.deepcopy(m)
    assert m2.edge_dropout_position == 12 and m2._edge_rates == m._edge_rates and m2._edge_plans == {}


def test_mrgcn_delegates_and_partitioned_engines_refuse():
    from mrgcn_amd._lib import MrgcnError
    from mrgcn_amd.models.mrgcn import MRGCN
    from mrgcn_amd.partition import PartitionedRGCN
    from mrgcn_amd.partition_halo import HaloPartitionedRGCN
    assert MRGCN.set_edge_dropout is not None and isinstance(MRGCN.edge_dropout_position, property)
    for cls in (PartitionedRGCN, HaloPartitionedRGCN):
        obj = cls.__new__(cls)
        with pytest.raises(MrgcnError, match="edge dropout"):
            cls.set_edge_dropout(obj, 0.4)
        with pytest.raises(MrgcnError, match="edge dropout"):
            cls.set_edge_dropout(obj, 0.0, self_loop=0.2)
        assert cls.set_edge_dropout(obj, 0.0) is obj


def test_refusal_helper_names_the_step():
    from mrgcn_amd._lib import MrgcnError
    from mrgcn_amd.models.rgcn import refuse_edge_dropout
    m = _model()
    refuse_edge_dropout(m, "x")
    m.set_edge_dropout(0.4)
    with pytest.raises(MrgcnError, match="edge dropout: the step"):
        refuse_edge_dropout(nn.Sequential(m), "the step")
    m.eval()
    refuse_edge_dropout(m, "x")   # (an eval() forward draws nothing)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_declarations_agree():
    from mrgcn_amd import _lib
    declared = header_functions()
    lib = _lib.load()
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/mrgcn_hip.h"
        assert name in _lib.SIGNATURES, f"{name} is not in the ctypes table"
        assert hasattr(lib, name)
    src = open(os.path.join(ROOT, "include", "mrgcn_hip.h")).read()
    assert re.search(r"#define\s+MRGCN_ABI_VERSION\s+5\b", src) and lib.mrgcn_abi_version() == 5 == _lib.ABI_VERSION
    assert os.path.exists(os.path.join(ROOT, "mrgcn_amd", "csrc", "edge_dropout.hip"))
    # argument counts as the header states them
    flat = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW:
        args = re.search(name + r"\s*\(([^)]*)\)", flat).group(1)
        assert len([a for a in args.split(",") if a.strip() and a.strip() != "void"]) == len(_lib.SIGNATURES[name][1]), name
        assert _lib.SIGNATURES[name][0] is C.c_int
    # argument checks answer before any launch (no device needed)
    assert lib.mrgcn_plan_is_overlay(None) == 0
    child = C.c_void_p()
    assert lib.mrgcn_plan_create_overlay(None, C.byref(child), None) != 0
    assert lib.mrgcn_edge_dropout_draw_f32(None, None, 1, None, 0, 0, None) != 0
    tag = re.search(r"kEdgeTag\s*=\s*(0x[0-9A-Fa-f]+)", open(os.path.join(ROOT, "mrgcn_amd", "csrc", "edge_dropout.hip")).read())
    from mrgcn_amd import host
    assert int(tag.group(1), 16) == host.EDGE_KEY_TAG
