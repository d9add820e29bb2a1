"""The flat score backward's plan (`link_prediction._bwd_plan`) against DESIGN §8's table, at both sides of every
threshold, and where the scorer-specific entries of the library may be read in `link_prediction.py`: the lookup, the
plan's walk and the single-side rank helper.  No device."""
import ast
import os
import re

import pytest

from mrgcn_amd import _lib
from mrgcn_amd._lib import MrgcnError
from mrgcn_amd.tasks import link_prediction as lp
from tests.test_cpu_host import ROOT

N, R = 50, 7
BIG = 2 ** 22


def plan(scorer, n, stored=None, det=False, sorted_bwd=True, nodes=N, rels=R):
    return lp._bwd_plan(scorer, n, stored, nodes, rels, det, sorted_bwd)


def test_the_thresholds_are_the_named_constants():
    assert (lp._COUNTING_MIN, lp._SORTED_BWD_MIN, lp._DET_SMALL_N) == (1024, 4096, 4096)


# ---- DistMult, torch's deterministic flag off ------------------------------------------------------------------------
@pytest.mark.parametrize("n, want", [
    (0, ()),
    (1, ((0, 1, None, "scatter"),)),
    (4095, ((0, 4095, None, "scatter"),)),
    (4096, ((0, 4096, "radix", "sorted"),)),
])
def test_distmult_without_stored_orders(n, want):
    assert plan("distmult", n) == want
    # the node and relation counts bear on the counting sort only
    assert plan("distmult", n, nodes=BIG + 1, rels=BIG + 1) == want


@pytest.mark.parametrize("m, tail", [
    (0, None), (25, (None, "scatter")), (1023, (None, "scatter")), (1024, ("counting", "sorted")),
    (4096, ("counting", "sorted")), (4097, ("counting", "sorted")),
])
def test_distmult_behind_stored_facts(m, tail):
    want = ((0, 100, "stored", "sorted"),) + (((100, m) + tail,) if m else ())
    assert plan("distmult", 100 + m, 100) == want


@pytest.mark.parametrize("nodes, rels, tail", [
    (BIG, R, ("counting", "sorted")), (BIG + 1, R, (None, "scatter")),
    (N, BIG, ("counting", "sorted")), (N, BIG + 1, (None, "scatter")),
    (BIG, BIG, ("counting", "sorted")),
])
def test_the_counting_sort_ends_where_its_tables_do(nodes, rels, tail):
    for m in (1024, 4097):
        assert plan("distmult", 100 + m, 100, nodes=nodes, rels=rels) == \
            ((0, 100, "stored", "sorted"), (100, m) + tail)
    assert plan("distmult", 100 + 1023, 100, nodes=nodes, rels=rels)[1] == (100, 1023, None, "scatter")


def test_distmult_with_the_sorted_backward_switched_off_scatters_everything():
    for stored in (None, 0, 100):
        for n in (100, 125, 1124, 4095, 4096, 100 + 4097):
            assert plan("distmult", n, stored, sorted_bwd=False) == ((0, n, None, "scatter"),)
    assert plan("distmult", 0, None, sorted_bwd=False) == ()


def test_distmult_behind_an_empty_stored_set_keeps_the_tail_rule():
    assert plan("distmult", 0, 0) == ()
    assert plan("distmult", 25, 0) == ((0, 25, None, "scatter"),)
    assert plan("distmult", 1023, 0) == ((0, 1023, None, "scatter"),)
    assert plan("distmult", 1024, 0) == ((0, 1024, "counting", "sorted"),)
    assert plan("distmult", 4096, 0) == ((0, 4096, "counting", "sorted"),)      # (not the radix sort of stored=None)
    assert plan("distmult", 4096, 0, nodes=BIG + 1) == ((0, 4096, None, "scatter"),)


# ---- DistMult, torch's deterministic flag on -------------------------------------------------------------------------
@pytest.mark.parametrize("n, want", [
    (0, ()),
    (1, ((0, 1, "self", "det"),)),
    (4095, ((0, 4095, "self", "det"),)),
    (4096, ((0, 4096, "self", "det"),)),
    (4097, ((0, 4097, "radix", "det"),)),
])
def test_deterministic_distmult_without_stored_orders(n, want):
    for stored in (None, 0):
        assert plan("distmult", n, stored, det=True) == want
    assert plan("distmult", n, 100 if n >= 100 else None, det=True, sorted_bwd=False) == want
    assert plan("distmult", n, det=True, nodes=BIG + 1, rels=BIG + 1) == want


@pytest.mark.parametrize("m, orders", [(0, None), (25, "self"), (1023, "self"), (1024, "self"), (4096, "self"),
                                       (4097, "radix")])
def test_deterministic_distmult_behind_stored_facts(m, orders):
    want = ((0, 100, "stored", "det"),) + (((100, m, orders, "det"),) if m else ())
    assert plan("distmult", 100 + m, 100, det=True) == want
    assert plan("distmult", 100 + m, 100, det=True, nodes=BIG + 1, rels=BIG + 1) == want


# ---- ComplEx: one route, whatever the flag and the switch -----------------------------------------------------------
@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("sorted_bwd", [True, False])
def test_complex_has_one_route(det, sorted_bwd):
    kw = dict(det=det, sorted_bwd=sorted_bwd)
    assert plan("complex", 0, **kw) == ()
    for n in (1, 4095, 4096, 4097):
        for stored in (None, 0):
            assert plan("complex", n, stored, **kw) == ((0, n, "radix", "complex"),)
    for m in (0, 25, 1023, 1024, 4096, 4097):
        want = ((0, 100, "stored", "complex"),) + (((100, m, "radix", "complex"),) if m else ())
        assert plan("complex", 100 + m, 100, **kw) == want
        assert plan("complex", 100 + m, 100, nodes=BIG + 1, rels=BIG + 1, **kw) == want


def test_segments_tile_the_triples_and_none_is_empty():
    for scorer in lp.SCORERS:
        for det in (False, True):
            for stored in (None, 0, 100):
                for n in (0, 1, 100, 125, 1124, 4096, 4197):
                    if stored is not None and n < stored:
                        continue
                    at = 0
                    for start, count, _, _ in plan(scorer, n, stored, det=det):
                        assert start == at and count > 0
                        at += count
                    assert at == n


# ---- the scorer's entries: one lookup ---------------------------------------------------------------------------------
def test_the_lookup_resolves_every_entry_its_workspace_and_its_label():
    lib = _lib.load()
    for scorer in lp.SCORERS:
        entries = lp._scorer(scorer, "t")
        assert entries is lp._scorer(scorer, "t", 8) and entries.complex == (scorer == "complex")
        for suffix in ("ranks_both", "topk", "typed_ranks", "typed_topk"):
            fn, ws, what = entries(suffix)
            assert fn is getattr(lib, f"mrgcn_{scorer}_{suffix}")
            assert ws is getattr(lib, f"mrgcn_{scorer}_{suffix}_workspace")
            assert what == f"{scorer}_{suffix}"
            assert entries(suffix) is entries(suffix)                 # looked up once, kept
        fn, ws, what = entries("score_f32")
        assert fn is getattr(lib, f"mrgcn_{scorer}_score_f32") and ws is None and what == f"{scorer}_score"
    with pytest.raises(MrgcnError, match="'distmult' or 'complex'"):
        lp._scorer("transe", "t")
    with pytest.raises(MrgcnError, match="odd"):
        lp._scorer("complex", "t", 7)
    lp._scorer("distmult", "t", 7)


SCORER_ENTRY = re.compile(r"^mrgcn_(complex_\w+|distmult_(score_|ranks_both|topk|typed_)\w*)$")


def test_scorer_entries_are_read_in_the_lookup_the_walk_and_the_rank_helper_only():
    """A call site that picks `lib.mrgcn_complex_X if ... else lib.mrgcn_distmult_X` again fails here: the entries that
    exist per scorer are reached through `_Entries` (by name, so no attribute read at all), the backward kernels are
    read in the plan's walk, once each, and `mrgcn_distmult_ranks` in the single-side helper."""
    path = os.path.join(ROOT, "mrgcn_amd", "tasks", "link_prediction.py")
    tree = ast.parse(open(path).read(), path)
    owner = {}
    for top in tree.body:
        if isinstance(top, (ast.FunctionDef, ast.ClassDef)):
            for sub in ast.walk(top):
                owner[id(sub)] = top.name
    # (`mrgcn_distmult_ranks_both_slice` has no ComplEx twin: a constant of the library, read in `rank_both_slice`)
    reads = [(node.attr, owner.get(id(node))) for node in ast.walk(tree)
             if isinstance(node, ast.Attribute) and SCORER_ENTRY.match(node.attr)
             and node.attr != "mrgcn_distmult_ranks_both_slice"]
    assert sorted(reads) == [("mrgcn_complex_bwd_workspace", "_run_bwd_plan"),
                             ("mrgcn_complex_score_bwd_f32", "_run_bwd_plan"),
                             ("mrgcn_distmult_score_bwd_det_f32", "_run_bwd_plan"),
                             ("mrgcn_distmult_score_bwd_f32", "_run_bwd_plan"),
                             ("mrgcn_distmult_score_bwd_sorted_f32", "_run_bwd_plan")], reads
    single = [(node.attr, owner.get(id(node))) for node in ast.walk(tree)
              if isinstance(node, ast.Attribute) and node.attr in ("mrgcn_distmult_ranks",
                                                                   "mrgcn_distmult_ranks_workspace")]
    assert sorted(single) == [("mrgcn_distmult_ranks", "_rank_one_side"),
                              ("mrgcn_distmult_ranks_workspace", "_rank_one_side")], single
    # entries looked up by name — `getattr` on the library object, which this file calls `lib` or `_lib.load()` —: in
    # `_Entries` alone
    def is_library(node):
        return (isinstance(node, ast.Name) and node.id == "lib") or (
            isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "load")
    by_name = [owner.get(id(node)) for node in ast.walk(tree)
               if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "getattr"
               and node.args and is_library(node.args[0])]
    assert by_name and set(by_name) == {"_Entries"}, by_name
    # one autograd function for the flat scores, and one environment switch on its backward
    src = open(path).read()
    assert "_DistMultScore" not in src and "_ComplexScore" not in src and "MRGCN_LP_COUNTING" not in src
    assert src.count('"MRGCN_LP_SORTED_BWD"') == 1
