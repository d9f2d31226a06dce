"""The host shared-subscription table (engine.cpp: the emqx_shared_subscription
bag, src/emqx_shared_sub.erl:75-87, 251-252, 316-321) and its in-place share
image, on a host-only engine, against tests/shared_ref.py: random churn with
tm_debug_check_shares after every commit (duplicate adds, deletes of absent
records, member_down across groups, `remaining` and the count, table regrowth,
set-index and xid recycling, filters deleted and re-inserted behind the
table's back), the group / node target split, filter-id reuse, the reserved
member id, TM_ENOSPC of tm_share_members, and the reference suite's two
properties (test/emqx_shared_sub_SUITE.erl:217-221) on the oracle itself."""
import ctypes
import random

import numpy as np
import pytest

from shared_ref import NO_MEMBER, SharedSub as RefShared, route_shared
from emqx_amd import Engine
from emqx_amd import _lib as L
from emqx_amd.emqx_broker import Broker
from emqx_amd.emqx_router import Router
from emqx_amd.emqx_shared_sub import SharedSub
from emqx_amd.engine import pack
from oracle import pytrie

GROUPS = [b"g1", b"g2", b"g3", b"", b"n1"]
TOPICS = [b"a/b", b"a/+", b"#", b"a/#", b"", b"a/b\x00", b"$SYS/x", b"+/+", b"x" * 70, b"a/b/c"]


def _fid(e, filt):
    """the id of trie filter filt, or None"""
    info = L.TmNodeInfo()
    rc = e.lib.tm_lookup(e.h, filt, len(filt), ctypes.byref(info))
    return None if rc == L.TM_ENOENT or info.filter_id == L.TM_NO_FILTER else info.filter_id


def _same(e, ref):
    assert e.share_count == ref.size()
    for g in GROUPS:
        for t in TOPICS:
            assert e.share_members(g, t) == ref.subscribers(g, t), (g, t)


def test_share_table_churn_vs_oracle():
    rng = random.Random(5)
    e, ref = Engine(device=-1), RefShared()
    e.set_option("route_gc", 8)                               # pool and arena compactions happen in this test
    for step in range(4000):
        g, t, m = rng.choice(GROUPS), rng.choice(TOPICS), rng.randrange(24)
        x = rng.random()
        if x < 0.55:
            before = ref.subscribers(g, t)
            e.share_add(g, t, m)
            ref.subscribe(g, t, m)
            if m in before:                                   # a duplicate add keeps the first position
                assert e.share_members(g, t) == before
        elif x < 0.85:                                        # often an absent record
            assert e.share_del(g, t, m) == ref.unsubscribe(g, t, m)
        elif x < 0.93:
            assert e.share_member_down(m) == ref.cleanup_down(m)
        elif x < 0.97:                                        # the trie changes behind the table's back
            f = rng.choice([tp for tp in TOPICS if b"+" in tp or b"#" in tp])
            if _fid(e, f) is None:
                e.insert(f)
            else:
                e.delete(f)
        else:
            e.commit()
            e.debug_check_shares()
        if step % 400 == 399:
            e.commit()
            e.debug_check_shares()
            _same(e, ref)
    for m in range(24):
        assert e.share_member_down(m) == ref.cleanup_down(m)
    e.commit()
    e.debug_check_shares()
    assert e.share_count == 0 == ref.size()
    e.close()


def test_share_batch_calls_and_growth():
    """the bulk forms in order, sets past one pool segment and tables past
    their first 16 slots, then every second record deleted in bulk"""
    e, ref = Engine(device=-1), RefShared()
    recs = [(b"g%d" % (i % 7), b"t/%d" % (i % 41) if i % 3 else b"t/+/%d" % (i % 5), i % 300) for i in range(3000)]
    gb, go = pack([r[0] for r in recs])
    tb, to = pack([r[1] for r in recs])
    e.share_add_many(gb, go, tb, to, [r[2] for r in recs])
    for g, t, m in recs:
        ref.subscribe(g, t, m)
    e.commit()
    e.debug_check_shares()
    assert e.share_count == ref.size()
    gone = recs[::2]
    gb, go = pack([r[0] for r in gone])
    tb, to = pack([r[1] for r in gone])
    e.share_del_many(gb, go, tb, to, [r[2] for r in gone])
    for g, t, m in gone:
        ref.unsubscribe(g, t, m)
    e.commit()
    e.debug_check_shares()
    assert e.share_count == ref.size()
    for g, t, _ in recs[:200]:
        assert e.share_members(g, t) == ref.subscribers(g, t)
    with pytest.raises(L.TopicMatchError):
        e.share_add_many(gb[:2], go[:2], tb[:3], to[:2], [0xFFFFFFFF])
    e.close()


def test_group_and_node_with_equal_bytes_stay_apart():
    """the group b"n1" is the TM_TARGET_GROUP target, the node n1 another: the
    members of the group never show under the node's deliveries, and a group
    may have members before it has a route"""
    e = Engine(device=-1)
    r = Router(e, node="n1")
    b = Broker(e, r)
    e.share_add(b"n1", b"a/b", 7)                        # no route, no dest yet
    assert e.share_members(b"n1", b"a/b") == [7]
    r.add_route(b"a/b", "n1")                            # the node atom n1
    r.add_route(b"a/b", ("n1", "n2"))                    # the group <<"n1">>
    tid_node = e.dest_target(b"\x02n1", Engine.TARGET_NODE, b"n1")
    tid_group = e.dest_target(b"\x01\x02n1\x00\x02n2", Engine.TARGET_GROUP, b"n1")
    assert tid_node != tid_group
    assert e.target_bytes(tid_node) == (Engine.TARGET_NODE, b"n1")
    assert e.target_bytes(tid_group) == (Engine.TARGET_GROUP, b"n1")
    e.commit()
    e.debug_check_shares()
    assert b.shared.subscribers("n1", b"a/b") == [7]
    e.close()


def test_filter_id_reuse_does_not_inherit_members():
    """a set keyed by filter id follows the id's lifetime: after the filter is
    deleted the set has no To key, and the id reused for another filter finds
    no set (tm_debug_check_shares compares every link with the trie)"""
    e = Engine(device=-1)
    e.insert(b"a/+")
    fid = _fid(e, b"a/+")
    e.share_add(b"g", b"a/+", 1)
    e.share_add(b"g", b"a/+", 2)
    e.commit()
    e.debug_check_shares()
    e.delete(b"a/+")
    e.debug_check_shares()
    for _ in range(3):
        e.commit()
    e.insert(b"b/#")
    assert _fid(e, b"b/#") == fid                                  # the id is reused (tests/test_id_reuse.py)
    e.commit()
    e.debug_check_shares()                               # b/#'s id names no set; a/+'s set is unkeyed
    assert e.share_members(b"g", b"a/+") == [1, 2] and e.share_members(b"g", b"b/#") == []
    e.share_add(b"g", b"b/#", 9)
    e.insert(b"a/+")                                     # a/+ is back under a new id: linked again
    e.commit()
    e.debug_check_shares()
    assert e.share_members(b"g", b"b/#") == [9]
    e.close()


def test_reserved_member_id_is_einval():
    e = Engine(device=-1)
    for call in (lambda: e.share_add(b"g", b"t", 0xFFFFFFFF), lambda: e.share_del(b"g", b"t", 0xFFFFFFFF),
                 lambda: e.share_member_down(0xFFFFFFFF)):
        with pytest.raises(L.TopicMatchError) as ei:
            call()
        assert ei.value.code == L.TM_EINVAL
    assert e.share_count == 0
    e.close()


def test_share_members_enospc():
    e = Engine(device=-1)
    for m in (5, 3, 9):
        e.share_add(b"g", b"t", m)
    out = np.zeros(2, dtype=np.uint32)
    n = ctypes.c_uint32()
    rc = e.lib.tm_share_members(e.h, b"g", 1, b"t", 1, ctypes.c_void_p(out.ctypes.data), 2, ctypes.byref(n))
    assert rc == L.TM_ENOSPC and n.value == 3 and list(out) == [5, 3]
    with pytest.raises(L.TopicMatchError) as ei:
        e.share_members(b"g", b"t", cap=2)
    assert ei.value.code == L.TM_ENOSPC
    assert e.share_members(b"g", b"t") == [5, 3, 9] == e.share_members(b"g", b"t", cap=3)
    e.close()


def test_publish_calls_need_a_device_and_a_known_strategy():
    e = Engine(device=-1)
    e.set_local_node(b"n1")
    buf, off = pack([b"a"])
    with pytest.raises(L.TopicMatchError) as ei:
        e.match_publish_batch(buf, off, Engine.SHARE_ROUND_ROBIN)
    assert ei.value.code == L.TM_EDEVICE
    for strategy, keys in ((0, None), (3, None), (Engine.SHARE_KEYED, None)):
        with pytest.raises(L.TopicMatchError) as ei:
            e.match_publish_batch(buf, off, strategy, keys)
        assert ei.value.code == L.TM_EINVAL
    e.close()


def test_broker_subscribe_feeds_the_member_table():
    """handle_cast #subscribe / #unsubscribe call emqx_shared_sub (:394, :353)"""
    e = Engine(device=-1)
    b = Broker(e, Router(e, node="n1"))
    assert isinstance(b.shared, SharedSub) and b.shared.strategy == "round_robin"
    b.subscribe(b"a/b", 1, "g")
    b.subscribe(b"a/b", 2, "g")
    b.subscribe(b"a/b", 3)                               # undefined group: not a member
    assert b.shared.subscribers("g", b"a/b") == [1, 2]
    b.unsubscribe(b"a/b", 1, "g")
    assert b.shared.subscribers("g", b"a/b") == [2]
    b.shared.cleanup_down(2)
    assert b.shared.subscribers("g", b"a/b") == [] and e.share_count == 0
    e.debug_check_shares()
    e.close()


def test_suite_properties_on_the_oracle():
    """test/emqx_shared_sub_SUITE.erl:217-221 with two members of group1 on
    foo/bar and two publishes: round robin gives different members, an equal
    key (hash of one ClientId) the same one; plus the stated cursor rules"""
    o = pytrie.RouteTable()
    o.add_route(b"foo/bar", ("group1", "n1"))
    for strategy, same in (("round_robin", False), ("keyed", True)):
        sh = RefShared()
        sh.subscribe(b"group1", b"foo/bar", 1)
        sh.subscribe(b"group1", b"foo/bar", 2)
        a = route_shared(o, sh, strategy, 12345, b"foo/bar")
        b = route_shared(o, sh, strategy, 12345, b"foo/bar")
        assert len(a) == len(b) == 1 and a[0] in (1, 2) and b[0] in (1, 2)
        assert (a == b) is same
    sh = RefShared()
    assert route_shared(o, sh, "round_robin", 0, b"foo/bar") == [NO_MEMBER]
    sh.subscribe(b"group1", b"foo/bar", 1)
    assert [sh.do_pick("round_robin", 0, b"group1", b"foo/bar") for _ in range(3)] == [1, 1, 1]
    assert sh.pd == {}                                   # one member: the cursor is not touched
    sh.subscribe(b"group1", b"foo/bar", 2)
    sh.subscribe(b"group1", b"foo/bar", 3)
    assert [sh.do_pick("round_robin", 0, b"group1", b"foo/bar") for _ in range(4)] == [1, 2, 3, 1]
    sh.pd[("shared_sub_round_robin", b"group1", b"foo/bar")] = 2
    sh.unsubscribe(b"group1", b"foo/bar", 3)             # N = 2 >= Count = 2: (2 + 1) rem 2 = 1
    assert sh.do_pick("round_robin", 0, b"group1", b"foo/bar") == 2
    sh.cleanup_down(1)
    sh.cleanup_down(2)
    assert sh.pd == {}                                   # the emptied set forgot its cursor
    sh.subscribe(b"group1", b"foo/bar", 4)
    sh.subscribe(b"group1", b"foo/bar", 5)
    assert sh.do_pick("round_robin", 0, b"group1", b"foo/bar") == 4
