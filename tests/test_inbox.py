"""The inbox plan without a GPU: the two entry points in the header, the
library and the ctypes table; their status codes on a host-only engine; and
the reference model (tests/inbox_ref.py) on a hand-worked case."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from inbox_ref import DROP, NO_MEMBER, NO_WORD, PICK, ROUTE_TOPIC, expected_plan, grouped, sends_of_planes  # noqa: E402
from emqx_amd import Engine  # noqa: E402
from emqx_amd import _lib as L  # noqa: E402

NAMES = ("tm_inbox_plan", "tm_inbox_plan_device")


def test_inbox_symbols_in_header_library_and_signatures():
    with open(os.path.join(ROOT, "include", "topicmatch.h")) as f:
        hdr = f.read()
    sigs = {name for name, _res, _args in L.SIGNATURES}
    e = Engine(device=-1)
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in sigs, name
        assert hasattr(e.lib, name), name
    assert "ONE DEVIATION" in hdr and "TM_INBOX_PICK" in hdr
    assert Engine.INBOX_PICK == PICK and Engine.NO_WORD == NO_WORD and Engine.DELIVER_DROP == DROP
    e.close()


def _planes():
    """one publish: one pair, one delivery slot with a pick"""
    u32 = lambda *x: np.array(x, dtype=np.uint32)   # noqa: E731
    u64 = lambda *x: np.array(x, dtype=np.uint64)   # noqa: E731
    return dict(sub_off=u64(0, 1), sub_to=u32(3), sub_id=u32(9), sub_word=u32(1), sub_total=u64(1),
                count=u32(1), off=u64(0, 1), to=u32(4), pick=u32(9), pick_word=u32(2), total=u64(1),
                hdr=np.zeros(4, dtype=np.uint64), inbox=np.zeros((4, 4), dtype=np.uint32),
                ent_pub=np.zeros(4, dtype=np.uint32), ent_to=np.zeros(4, dtype=np.uint32),
                ent_word=np.zeros(4, dtype=np.uint32))


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _host(e, a, n=1, sub_cap=1, out_cap=1, inbox_cap=4, ent_cap=4, h=True, **nulls):
    g = lambda k: None if k in nulls else _p(a[k])   # noqa: E731
    return e.lib.tm_inbox_plan(e.h if h else None, n, g("sub_off"), g("sub_to"), g("sub_id"), g("sub_word"), sub_cap,
                               1, g("count"), g("off"), g("to"), g("pick"), g("pick_word"), out_cap, 1, g("hdr"),
                               g("inbox"), inbox_cap, g("ent_pub"), g("ent_to"), g("ent_word"), ent_cap)


def _dev(e, a, n=1, sub_cap=1, out_cap=1, inbox_cap=4, ent_cap=4, h=True, **nulls):
    # host arrays stand in for device memory: a call that is refused reads none of them
    g = lambda k: None if k in nulls else _p(a[k])   # noqa: E731
    return e.lib.tm_inbox_plan_device(e.h if h else None, n, g("sub_off"), g("sub_to"), g("sub_id"), g("sub_word"),
                                      sub_cap, g("sub_total"), g("count"), g("off"), g("to"), g("pick"),
                                      g("pick_word"), out_cap, g("total"), g("hdr"), g("inbox"), inbox_cap,
                                      g("ent_pub"), g("ent_to"), g("ent_word"), ent_cap, None)


def test_inbox_plan_host_only_engine_is_edevice():
    e = Engine(device=-1)                                  # no tm_set_local_node: the plan reads no image
    a = _planes()
    assert _host(e, a) == L.TM_EDEVICE and _dev(e, a) == L.TM_EDEVICE
    assert b"host-only" in e.lib.tm_last_error(e.h)
    with pytest.raises(L.TopicMatchError) as ex:
        e.inbox_plan(a["sub_off"], a["sub_to"], a["sub_id"], a["sub_word"], a["count"], a["off"], a["to"], a["pick"],
                     a["pick_word"])
    assert ex.value.code == L.TM_EDEVICE
    with pytest.raises(L.TopicMatchError) as ex:
        d = lambda k: a[k].ctypes.data   # noqa: E731
        e.inbox_plan_device(1, d("sub_off"), d("sub_to"), d("sub_id"), d("sub_word"), 1, d("sub_total"), d("count"),
                            d("off"), d("to"), d("pick"), d("pick_word"), 1, d("total"), d("hdr"), d("inbox"), 4,
                            d("ent_pub"), d("ent_to"), d("ent_word"), 4)
    assert ex.value.code == L.TM_EDEVICE
    assert list(a["hdr"]) == [0, 0, 0, 0]
    e.close()


def test_inbox_plan_null_arguments():
    e = Engine(device=-1)
    a = _planes()
    ok = L.TM_EDEVICE                                      # what a call that passes the checks returns here
    for call in (_host, _dev):
        assert call(e, a) == ok
        assert call(e, a, hdr=1) == L.TM_EINVAL
        assert call(e, a, sub_off=1) == L.TM_EINVAL
        # a null plane with its capacity
        assert call(e, a, sub_to=1) == L.TM_EINVAL and call(e, a, sub_id=1) == L.TM_EINVAL
        assert call(e, a, sub_cap=0, sub_to=1, sub_id=1, sub_word=1) == ok
        assert call(e, a, sub_word=1) == ok                # the pair-word plane may be null
        assert call(e, a, to=1) == L.TM_EINVAL
        assert call(e, a, out_cap=0, to=1) == ok
        # a null result array with its capacity; ent_word may be null
        assert call(e, a, inbox=1) == L.TM_EINVAL
        assert call(e, a, ent_pub=1) == L.TM_EINVAL and call(e, a, ent_to=1) == L.TM_EINVAL
        assert call(e, a, ent_word=1) == ok
        assert call(e, a, inbox_cap=0, ent_cap=0, inbox=1, ent_pub=1, ent_to=1, ent_word=1) == ok
        # a pick-word plane without a pick plane; no pick plane: nothing of the deliveries is needed
        assert call(e, a, pick=1) == L.TM_EINVAL
        assert call(e, a, pick=1, pick_word=1) == ok
        assert call(e, a, pick=1, pick_word=1, count=1, off=1, to=1, total=1) == ok
        # with a pick plane: off and count
        assert call(e, a, off=1) == L.TM_EINVAL
        assert call(e, a, count=1) == L.TM_EINVAL
        assert call(e, a, n=0, count=1) == ok              # n == 0: count may be null
        assert call(e, a, pick_word=1) == ok               # the pick-word plane may be null
        assert call(e, a, h=False) == L.TM_EINVAL
    assert _dev(e, a, sub_total=1) == L.TM_EINVAL
    assert _dev(e, a, total=1) == L.TM_EINVAL
    assert _dev(e, a, total=1, pick=1, pick_word=1) == ok
    e.close()


def test_inbox_plan_capacities_out_of_range():
    e = Engine(device=-1)
    a = _planes()
    top = 2 ** 32 - 2
    for call in (_host, _dev):
        assert call(e, a, sub_cap=top) == L.TM_ERANGE
        assert b"inbox" in e.lib.tm_last_error(e.h)
        assert call(e, a, out_cap=top) == L.TM_ERANGE
        assert call(e, a, sub_cap=2 ** 40) == L.TM_ERANGE
        assert call(e, a, sub_cap=top - 1, out_cap=top - 1) == L.TM_EDEVICE
        assert call(e, a, out_cap=top, pick=1, pick_word=1) == L.TM_EDEVICE     # no pick plane: out_cap unread
        assert call(e, a, n=2 ** 31) == L.TM_ERANGE        # bit 31 of ent_pub is the kind
    e.close()


def test_model_hand_worked_case():
    """two publishes.  Publish 0: pairs (To 5, sub 7, word 1), (To 5, sub 3,
    dropped), (To 6, sub 7, word 2); slots: a pick of member 7 (word 4) on To
    8, a $share delivery without a pick, and a hole that holds a pick value.
    Publish 1: pair (its own topic, sub 3, word 0); slots: a pick of member 2
    with TM_NO_WORD, a pick of member 7 dropped by no-local."""
    sub_off = [0, 3, 4]
    sub_to = [5, 5, 6, ROUTE_TOPIC]
    sub_id = [7, 3, 7, 3]
    sub_word = [1, DROP, 2, 0]
    counts = [2, 2]
    offs = [0, 3, 5]                                       # publish 0: span 3, count 2 -> slot 2 is a hole
    to = [8, 9, 8, 10, 11]
    pick = [7, NO_MEMBER, 7, 2, 7]
    pick_word = [4, NO_WORD, 4, NO_WORD, DROP]
    sends = sends_of_planes(sub_off, sub_to, sub_id, sub_word, counts, offs, to, pick, pick_word)
    assert sends == [(7, 0, 0, 0, 5, 1), (7, 0, 0, 2, 6, 2), (3, 1, 0, 3, ROUTE_TOPIC, 0),
                     (7, 0, 1, 0, 8, 4), (2, 1, 1, 3, 10, NO_WORD)]
    hdr, inbox, ent_pub, ent_to, ent_word = expected_plan(sends)
    assert hdr == [5, 3, 3, 2]
    assert inbox == [(2, 0, 1, 1), (3, 1, 1, 0), (7, 2, 3, 1)]
    assert ent_pub == [1 | PICK, 1, 0, 0, 0 | PICK]        # subscriber 7: its two pairs of publish 0, then the pick
    assert ent_to == [10, ROUTE_TOPIC, 5, 6, 8]
    assert ent_word == [NO_WORD, 0, 1, 2, 4]
    assert grouped(sends) == {2: [(1, 10, NO_WORD, True)], 3: [(1, ROUTE_TOPIC, 0, False)],
                              7: [(0, 5, 1, False), (0, 6, 2, False), (0, 8, 4, True)]}
    # without word planes every pair and every pick is a send, and no word is reported
    bare = sends_of_planes(sub_off, sub_to, sub_id, None, counts, offs, to, pick, None)
    assert [s[:4] for s in bare] == [(7, 0, 0, 0), (3, 0, 0, 1), (7, 0, 0, 2), (3, 1, 0, 3),
                                     (7, 0, 1, 0), (2, 1, 1, 3), (7, 1, 1, 4)]
    assert all(s[5] is None for s in bare) and expected_plan(bare)[4] == [0] * 7
    # the capacity bounds: pairs at or past min(sub_total, sub_cap), slots at or past min(total, out_cap)
    cut = sends_of_planes(sub_off, sub_to, sub_id, sub_word, counts, offs, to, pick, pick_word, sub_total=4,
                          sub_cap=3, total=5, out_cap=3)
    assert [s[:4] for s in cut] == [(7, 0, 0, 0), (7, 0, 0, 2), (7, 0, 1, 0)]
    assert sends_of_planes(sub_off, sub_to, sub_id, sub_word) == sends[:3]      # no pick plane: no pick sends
    assert expected_plan([]) == ([0, 0, 0, 0], [], [], [], [])
