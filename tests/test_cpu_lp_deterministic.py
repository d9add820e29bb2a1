"""The C entries of the deterministic link-prediction step (torch.use_deterministic_algorithms(True)): declared in
include/mrgcn_hip.h, exported by the library, bound in the ctypes table with the header's argument lists.  No GPU."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    "mrgcn_distmult_bwd_det_workspace": 2,
    "mrgcn_distmult_score_bwd_det_f32": 18,
    "mrgcn_bce_logits_det_workspace": 1,
    "mrgcn_bce_logits_det_f32": 8,
    "mrgcn_sumsq_det_workspace": 0,
    "mrgcn_sumsq_accum_det_f32": 6,
    "mrgcn_sumsq_accum_multi_det_f32": 7,
    "mrgcn_sumsq_clip_multi_det_f32": 17,
}


def _declarations():
    src = open(os.path.join(ROOT, "include", "mrgcn_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(int64_t|int)\s+(mrgcn_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        args = [a.strip() for a in m.group(3).split(",") if a.strip() and a.strip() != "void"]
        out[m.group(2)] = (m.group(1), args)
    return out


def test_header_declares_the_deterministic_entries():
    decl = _declarations()
    for name, nargs in NEW.items():
        assert name in decl, name
        assert len(decl[name][1]) == nargs, (name, decl[name])
        assert decl[name][0] == ("int64_t" if name.endswith("_workspace") else "int"), name


def test_ctypes_table_matches_the_header():
    import ctypes as C

    from mrgcn_amd import _lib
    decl = _declarations()
    for name, nargs in NEW.items():
        res, args = _lib.SIGNATURES[name]
        assert len(args) == nargs, name
        assert res in ((C.c_int64,) if name.endswith("_workspace") else (C.c_int,)), name
        for a, t in zip(decl[name][1], args):
            if "*" in a:
                assert t is C.c_void_p, (name, a)
            elif a.startswith("int64_t"):
                assert t is C.c_int64, (name, a)
            elif a.startswith("int32_t"):
                assert t is C.c_int32, (name, a)
            elif a.startswith("float"):
                assert t is C.c_float, (name, a)


def test_library_exports_the_deterministic_entries():
    from mrgcn_amd import _lib
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.mrgcn_abi_version() == 5
    # host-only size queries
    assert lib.mrgcn_distmult_bwd_det_workspace(100, 200) > 0
    assert lib.mrgcn_distmult_bwd_det_workspace(100000, 200) >= 2 * (100000 // 32) * 200 * 4
    assert lib.mrgcn_bce_logits_det_workspace(10 ** 6) >= 256 * 4
    assert lib.mrgcn_sumsq_det_workspace() >= 1024 * 8
