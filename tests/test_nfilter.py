"""Per-node filters inside the node's own cache line (option "nfilter",
image.h), host side on a host-only engine: through the first commit, inserts
and deletes without a relayout, a deleted filtered node whose id is reused, a
forced relayout and the option switched off and on, tm_debug_check_filters
holds -- every literal child of a filtered node passes its filter, every
reference carries its target's class, a filtered node's id is a multiple of 4
and none of its extension slots is live, free-listed or referenced -- and the
node count stays the oracle's (extension slots are not nodes).  The filter is
also worth its bits: at the 64-children node, fewer than half of the absent
words the in-node Bloom lets through pass the filter too (384 bits for 64
children at 2 bits per word: (1 - e^(-2*64/12/32))^2, about 8 %; any layout
of 384 bits per node stays below one half)."""
import ctypes

import numpy as np

from emqx_amd import Engine
from nfilter_trie import COUNTS, ROOT_FILL, churn_adds, churn_dels, filters, packed
from oracle import O1


def check(eng, o1):
    f = eng.lib.tm_debug_check_filters
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p]
    assert f(eng.h) == 0
    assert eng.node_count == o1.node_count


def filter_pass(eng, node, word):
    """(literal children, filtered, passes the Bloom, passes Bloom and filter)"""
    f = eng.lib.tm_debug_filter_pass
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint32,
                  ctypes.POINTER(ctypes.c_uint32)]
    out = (ctypes.c_uint32 * 4)()
    assert f(eng.h, node, len(node), word, len(word), out) == 0, (node, word)
    return tuple(out)


def both(eng, o1, op, fs):
    for f in fs:
        getattr(eng, op)(f)
        getattr(o1, op)(f)


def test_filters_hold_through_churn_reuse_relayout_and_option():
    eng, o1 = Engine(device=-1), O1()
    fb, fo = packed(filters())
    eng.insert_many(fb, fo)
    o1.insert_many(fb, fo)
    eng.commit()
    check(eng, o1)
    # which nodes took a filter: the least children count is 16
    for c in COUNTS:
        for node in (b"p%d/+" % c, b"t/%dn" % c):
            n, filtered, _, _ = filter_pass(eng, node, b"w1")
            assert n == c and filtered == (1 if c >= 16 else 0), (node, n, filtered)
    assert filter_pass(eng, b"", b"w1")[:2] == (len(COUNTS) + 2 + ROOT_FILL, 1)    # the root: p<c>, t, r<i>, $sys
    assert filter_pass(eng, b"$sys", b"w1")[1] == 1
    # new children under filtered and unfiltered nodes, no relayout
    both(eng, o1, "insert", churn_adds())
    check(eng, o1)
    eng.commit()
    check(eng, o1)
    for k in range(50):   # a new child passes its parent's filter at once
        assert filter_pass(eng, b"p64/+", b"n%d" % k)[2:] == (1, 1)
    both(eng, o1, "delete", churn_dels())
    check(eng, o1)
    eng.commit()
    check(eng, o1)
    # a whole filtered node goes (p200/+ and its parent), then 1,000 new nodes reuse the free ids: never an
    # extension slot
    both(eng, o1, "delete", [b"p200/+/w%d" % i for i in range(200)] + [b"p200/+/#", b"p200/+/w3/#", b"p200/lit/x",
                                                                      b"p200/#"])
    check(eng, o1)
    both(eng, o1, "insert", [b"new/%d" % i for i in range(500)] + [b"new/%d/deep" % i for i in range(500)])
    check(eng, o1)
    eng.commit()
    check(eng, o1)
    assert filter_pass(eng, b"new", b"w1")[:2] == (500, 0)      # created since the relayout: no filter yet
    eng.set_option("relayout", 1)
    eng.commit()
    check(eng, o1)
    assert filter_pass(eng, b"new", b"w1")[:2] == (500, 1)
    for on in (0, 1, 0):
        eng.set_option("nfilter", on)
        eng.commit()
        check(eng, o1)
        assert filter_pass(eng, b"new", b"w1")[1] == on
        both(eng, o1, "insert", [b"new/x%d_%d" % (on, i) for i in range(20)])
        check(eng, o1)
    eng.close()


def test_filter_halves_the_blooms_false_positives():
    eng = Engine(device=-1)
    fb, fo = packed(filters())
    eng.insert_many(fb, fo)
    eng.commit()
    absent = [b"w%d" % i for i in range(64, 1500)] + [b"r%d" % i for i in range(564)]
    assert len(absent) == 2000
    res = np.array([filter_pass(eng, b"p64/+", w) for w in absent])
    assert (res[:, 0] == 64).all() and (res[:, 1] == 1).all()
    bloom, both_ = int(res[:, 2].sum()), int(res[:, 3].sum())
    print("64 children, 2000 absent words: %d pass the Bloom, %d pass Bloom and filter" % (bloom, both_))
    assert bloom > 0 and both_ * 2 < bloom
    for i in range(64):   # and no child is ever rejected
        assert filter_pass(eng, b"p64/+", b"w%d" % i)[2:] == (1, 1)
    eng.close()
