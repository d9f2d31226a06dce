"""The commit path's host side under the churn of trie_churn.py, on a
host-only engine: after every commit tm_debug_check_trie (nodes, edge tables,
Bloom masks, summaries and dictionary against the logical trie) and
tm_debug_check_filters hold and the node count is the oracle's (O1 kept in
step), across layout {0, 1, 2} x hot_edges {0, 3} x summaries {1, 0}.

The cap on the generator (layout 0 and 1): tm_debug_commit_stats, which on a
host-only engine reports the decisions a device with two image epochs would
take, must report a scatter for the node table, and for every other trie
table the round changed, in every small round that does not follow a
whole-table copy, and a whole-table copy in every large round -- so the GPU
test that runs the same rounds provably takes the scatter path."""
import ctypes

import pytest

from emqx_amd import Engine
from oracle import O1
from trie_churn import check_decisions, hot_options, packed, schedule


@pytest.fixture(scope="module")
def run():
    """the base filters, the rounds and the oracle's node count after the base and after each round
    (computed once, never changed)"""
    base, rounds = schedule()
    o1 = O1()
    o1.insert_many(*packed(base))
    counts = [o1.node_count]
    for _, _, ops, _ in rounds:
        for op, f in ops:
            getattr(o1, op)(f)
        counts.append(o1.node_count)
    o1.close()
    return base, rounds, counts


def check(eng, want_nodes):
    eng.debug_check_trie()
    f = eng.lib.tm_debug_check_filters
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p]
    assert f(eng.h) == 0
    assert eng.node_count == want_nodes


@pytest.mark.parametrize("summaries", [1, 0])
@pytest.mark.parametrize("hot_edges", [0, 3])
@pytest.mark.parametrize("layout", [0, 1, 2])
def test_trie_image_holds_under_churn(run, layout, hot_edges, summaries):
    base, rounds, counts = run
    assert len(rounds) >= 40 and max(len(ops) for _, kind, ops, _ in rounds if kind == "small") <= 120
    eng = Engine(device=-1)
    for k, v in (("layout", layout), ("summaries", summaries)) + hot_options(hot_edges):
        eng.set_option(k, v)
    eng.insert_many(*packed(base))
    check(eng, counts[0])       # before the first commit: no relayout yet, supersets only
    eng.commit()
    check(eng, counts[0])
    prev = eng.debug_commit_stats()
    assert all(prev[t][0] == 3 for t in ("nodes", "edges", "dict"))
    kinds = set()
    for r, kind, ops, _ in rounds:
        for op, f in ops:
            getattr(eng, op)(f)
        if kind == "relayout":
            eng.set_option("relayout", 1)
        eng.commit()
        check(eng, counts[r + 1])
        stats = eng.debug_commit_stats()
        if layout != 2:
            check_decisions(r, kind, stats, prev, hot_edges != 0)
            if kind == "small":
                kinds.add(stats["nodes"][0])
        prev = stats
    assert layout == 2 or kinds == {2, 3}     # two-log scatters, and the copies that follow a large round
    eng.close()
