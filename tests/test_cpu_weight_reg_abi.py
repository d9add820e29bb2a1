"""The regularised node-table step at the C ABI (csrc/adam_reg.hip), without a GPU: the three entry points are declared
in the header, listed in the ctypes table and exported by the built library; the workspace query refuses a NULL
support.  No compute call is made."""
import ctypes as C

from tests.test_cpu_host import header_functions

NAMES = ("mrgcn_support_reg_norm_workspace", "mrgcn_support_reg_norm_f32", "mrgcn_support_adam_rows_reg_f32")


def test_the_three_symbols_are_in_header_ctypes_table_and_library():
    from mrgcn_amd import _lib
    declared = set(header_functions())
    lib = _lib.load()
    for n in NAMES:
        assert n in declared, f"{n} is not declared in include/mrgcn_hip.h"
        assert n in _lib.SIGNATURES, f"{n} is not in the ctypes table"
        assert hasattr(lib, n), f"{n} is not exported by the library"
    assert _lib.SIGNATURES["mrgcn_support_reg_norm_workspace"][0] is C.c_int64
    # weight_decay, l1, l2 travel as floats between eps and the step count
    sig = _lib.SIGNATURES["mrgcn_support_adam_rows_reg_f32"][1]
    assert sig.count(C.c_float) == 7 and len(sig) == 21
    assert len(_lib.SIGNATURES["mrgcn_support_reg_norm_f32"][1]) == 13


def test_workspace_query_refuses_a_null_support():
    from mrgcn_amd import _lib
    lib = _lib.load()
    for B, F in ((40, 10), (16, 16), (64, 16)):
        assert lib.mrgcn_support_reg_norm_workspace(None, B, F) < 0
