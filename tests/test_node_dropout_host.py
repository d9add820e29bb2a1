"""Node dropout on the device, the parts a CPU can check: the host mirror of the draw (mrgcn_amd.host) against the
published Philox4x32-10 known-answer vectors, the mask's values and statistics, and the public interface
(`RGCN.set_node_dropout`) — default mode, state_dict keys, unsupported engines."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from mrgcn_amd import host

# Random123's kat_vectors for philox4x32 with 10 rounds: (counter, key) -> output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,expected", KAT)
def test_host_twin_is_philox4x32_10(counter, key, expected):
    out = host.philox4x32_10(counter, key)
    assert tuple(int(w[0]) for w in out) == expected


def test_host_twin_takes_counter_arrays():
    ctr = np.array([0, 0xffffffff, 0x243f6a88], dtype=np.uint64)
    out = host.philox4x32_10((ctr, 0, 0, 0), (0, 0))
    assert int(out[0][0]) == 0x6627e8d5 and out[0].shape == (3,)
    single = host.philox4x32_10((0x243f6a88, 0, 0, 0), (0, 0))
    assert [int(w[2]) for w in out] == [int(w[0]) for w in single]


@pytest.mark.parametrize("p", [0.0, 0.2, 0.3, 0.5, 0.9, 0.999, 1.0])
def test_mask_values_are_what_torch_dropout_yields(p):
    m = host.node_dropout_mask(4099, p, seed=5, position=2, layer=1)
    assert m.dtype == np.float32 and m.shape == (4099,)
    ref = torch.nn.functional.dropout(torch.ones(20000), p).numpy()   # (its values, not its draw)
    keep = ref.max() if p < 1.0 else np.float32(0.0)
    assert set(np.unique(m).tolist()) <= {0.0, float(keep)}
    if p == 0.0:
        assert (m == 1.0).all()
    if p == 1.0:
        assert (m == 0.0).all()
    if 0.0 < p < 1.0:
        assert host.node_dropout_keep_value(p) == keep and (m == keep).any() and (m == 0).any()


def test_keep_count_within_six_sigma():
    n, p = 1 << 20, 0.3
    m = host.node_dropout_mask(n, p, seed=20240229, position=0, layer=0)
    sigma = np.sqrt(n * p * (1 - p))
    assert abs(int((m > 0).sum()) - n * (1 - p)) <= 6 * sigma


def test_masks_differ_by_layer_and_step_and_repeat_by_key():
    a = host.node_dropout_mask(5000, 0.5, seed=1, position=0, layer=0)
    assert np.array_equal(a, host.node_dropout_mask(5000, 0.5, seed=1, position=0, layer=0))
    for other in (dict(seed=1, position=0, layer=1), dict(seed=1, position=1, layer=0), dict(seed=2, position=0, layer=0),
                  dict(seed=1, position=1 << 32, layer=0), dict(seed=1 + (1 << 32), position=0, layer=0)):
        assert not np.array_equal(a, host.node_dropout_mask(5000, 0.5, **other)), other
    # a prefix of a longer mask: a node's value does not depend on n
    assert np.array_equal(a[:63], host.node_dropout_mask(63, 0.5, seed=1, position=0, layer=0))


def _rgcn(p=0.3):
    from mrgcn_amd.models.rgcn import RGCN
    return RGCN([(8, 4, "mrgcn", nn.ReLU()), (4, 3, "mrgcn", None)], 5, 20, 2, p, False, True, False)


def test_default_mode_is_host_and_state_dict_keys_do_not_change():
    m = _rgcn()
    assert m.node_dropout_mode == "host"
    keys = list(m.state_dict())
    m.set_node_dropout("device", seed=11)
    assert m.node_dropout_mode == "device" and m.node_dropout_seed == 11 and m.node_dropout_position == 0
    assert list(m.state_dict()) == keys
    m.node_dropout_position = 7
    assert m.node_dropout_position == 7 and list(m.state_dict()) == keys
    m.set_node_dropout("host")
    assert list(m.state_dict()) == keys and m.node_dropout_seed == 11
    with pytest.raises(ValueError):
        m.set_node_dropout("gpu")


def test_mrgcn_forwards_set_node_dropout():
    from mrgcn_amd.models.mrgcn import MRGCN
    assert callable(getattr(MRGCN, "set_node_dropout"))


def test_device_mode_on_an_unsupported_engine_raises():
    from mrgcn_amd._lib import MrgcnError
    from mrgcn_amd.partition import PartitionedRGCN
    from mrgcn_amd.partition_halo import HaloPartitionedRGCN
    m = _rgcn()
    m.set_engine("literal")
    with pytest.raises(MrgcnError, match="fused engine"):
        m.set_node_dropout("device")
    assert m.node_dropout_mode == "host"
    for cls in (PartitionedRGCN, HaloPartitionedRGCN):
        with pytest.raises(MrgcnError, match="partitioned"):
            cls.set_node_dropout(object.__new__(cls), "device")
