"""Mini-batch node classification without a GPU (mrgcn_amd/tasks/node_classification.py, csrc/nc_batches.hip):
`mkbatches` on the reference's slices against the batches the reference cut (tests/golden/nc_minibatch.npz, written by
tests/golden/make_nc_minibatch_goldens.py), the per-batch label pairs, the C ABI symbols in header, ctypes table and
library, and the arithmetic of the epoch's means.  No compute call is made."""
import ctypes as C
import os

import numpy as np
import scipy.sparse as sp

from tests import util
from tests.test_cpu_host import header_functions

GOLD = os.path.join(os.path.dirname(__file__), "golden", "nc_minibatch.npz")
NAMES = ("mrgcn_xent_train_eval_rows_f32", "mrgcn_batch_means_f32", "mrgcn_xent_train_eval_workspace",
         "mrgcn_xent_train_eval_single_block_rows")
SPLITS = ("train", "valid", "test")
CLASSES = 4


def label_matrix(g, split, N):
    nodes, classes = g[f"{split}.nodes"], g[f"{split}.classes"]
    return sp.csr_matrix((np.ones(len(nodes), dtype=np.int8), (nodes, classes)), shape=(N, CLASSES), dtype=np.int8)


def sequential_mean(values):
    """csrc/nc_batches.hip: k_nc_batch_means — a float64 sum in slot order, one division."""
    t = 0.0
    for v in values:
        t += float(v)
    return t / len(values)


def test_mkbatches_without_a_plan_cuts_the_references_batches():
    from mrgcn_amd.data.batch import FullBatch, MiniBatch
    from mrgcn_amd.tasks.node_classification import batch_targets, mkbatches
    g = np.load(GOLD)
    _, A = util.load_graph("graph_small")
    N = A.shape[0]
    for split in SPLITS:
        Y = label_matrix(g, split, N)
        batches = mkbatches(A, None, Y, 8, 2)
        assert len(batches) == int(g[f"{split}.count"])
        for i, b in enumerate(batches):
            assert isinstance(b, MiniBatch)
            want = g[f"{split}.{i}.node_index"]
            assert np.array_equal(b.node_index, want)
            pos, classes = batch_targets(b.node_index, Y)
            assert pos.dtype == np.int64 and classes.dtype == np.int64
            assert np.array_equal(pos, g[f"{split}.{i}.pos"]) and np.array_equal(classes, g[f"{split}.{i}.targets"])
    assert [len(b.node_index) for b in mkbatches(A, None, label_matrix(g, "test", N), 8, 2)] == [8, 1]
    # batchsize 0 (and anything that leaves one slice): ONE FullBatch over every node
    Y = label_matrix(g, "train", N)
    for bs in (0, -3, 23, 1000):
        full = mkbatches(A, None, Y, bs, 2)
        assert len(full) == int(g["full.count"]) == 1 and isinstance(full[0], FullBatch)
        assert str(g["full.kind"]) == "FullBatch" and np.array_equal(full[0].node_index, g["full.node_index"])
        assert full[0].A is A


def test_the_symbols_are_in_header_ctypes_table_and_library():
    from mrgcn_amd import _lib
    declared = set(header_functions())
    lib = _lib.load()
    for n in NAMES:
        assert n in declared, f"{n} is not declared in include/mrgcn_hip.h"
        assert n in _lib.SIGNATURES, f"{n} is not in the ctypes table"
        assert hasattr(lib, n), f"{n} is not exported by the library"
    assert _lib.ABI_VERSION == 5 and lib.mrgcn_abi_version() == 5
    res, args = _lib.SIGNATURES["mrgcn_xent_train_eval_rows_f32"]
    assert res is C.c_int and len(args) == 13 and args[1] is C.c_int64 and args[2] is C.c_int32 and args[5] is C.c_int64
    res, args = _lib.SIGNATURES["mrgcn_batch_means_f32"]
    assert res is C.c_int and len(args) == 6 and args[1] is C.c_int64 and args[3] is C.c_int64
    assert lib.mrgcn_xent_train_eval_single_block_rows() >= 64
    assert lib.mrgcn_xent_train_eval_workspace() > 0 and lib.mrgcn_xent_train_eval_workspace() % 16 == 0


def test_the_entry_points_refuse_bad_arguments_without_a_launch():
    from mrgcn_amd import _lib
    lib = _lib.load()
    one = 16   # (any non-NULL address: the argument checks come first)
    assert lib.mrgcn_xent_train_eval_rows_f32(None, 4, 4, one, one, 1, one, None, one, None, None, None, None) != 0
    assert lib.mrgcn_xent_train_eval_rows_f32(one, 3, 4, one, one, 1, one, None, one, None, None, None, None) != 0
    assert lib.mrgcn_xent_train_eval_rows_f32(one, 4, 4, one, one, 0, one, None, one, None, None, None, None) != 0
    big = lib.mrgcn_xent_train_eval_single_block_rows() + 1   # (more rows than one block takes: a workspace)
    assert lib.mrgcn_xent_train_eval_rows_f32(one, 4, 4, one, one, big, one, None, one, None, None, None, None) != 0
    assert lib.mrgcn_batch_means_f32(one, 0, None, 0, one, None) != 0
    assert lib.mrgcn_batch_means_f32(one, 1, None, 2, one, None) != 0
    assert lib.mrgcn_batch_means_f32(None, 1, None, 0, one, None) != 0


def test_the_sequential_float64_mean_is_numpys_mean_on_the_golden_rows():
    g = np.load(GOLD)
    for tag in ("fl_b3", "ft_b3", "fl_b3_l2", "fl_b3_stop"):
        row = g[f"{tag}.rows"][0]
        for k, name in enumerate(("train_loss", "train_acc", "valid_loss", "valid_acc")):
            values = g[f"{tag}.epoch1.{name}"]
            assert len(values) == (3 if k < 2 else 2)
            m = sequential_mean(values)
            assert abs(m - np.mean(values)) <= 1e-12 * abs(np.mean(values))
            assert abs(m - row[k]) <= 1e-12 * abs(row[k])   # (the row the reference's loop yielded)
    # the means are over batches, not over samples: batches of 8, 8 and 7 rows
    acc = g["fl_b3.epoch1.train_acc"]
    weighted = (8 * acc[0] + 8 * acc[1] + 7 * acc[2]) / 23
    assert abs(weighted - g["fl_b3.rows"][0][1]) > 1e-4
