"""The host subscriber table (engine.cpp: the emqx_subscriber duplicate_bag,
src/emqx_broker.erl:398-415, 245-247) and its in-place device image, on a
host-only engine: the reference suite's known answers (tests/golden/
kat_broker.json), insert_subscriber/3's quirks, delete_object's `remaining`,
and random churn against tests/dispatch_ref.py with tm_debug_check_subs after
every burst (compaction, table regrowth, filters deleted and re-inserted
behind the table's back)."""
import json
import os
import random

import pytest

from dispatch_ref import SubscriberBag, route_dispatch
from emqx_amd import Engine
from emqx_amd import _lib as L
from emqx_amd.emqx_broker import Broker
from emqx_amd.emqx_router import Router
from emqx_amd.engine import pack
from oracle import pytrie

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kat_cases():
    with open(os.path.join(ROOT, "tests", "golden", "kat_broker.json")) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("case", kat_cases(), ids=lambda c: c["name"])
def test_broker_suite_known_answers(case):
    """subscribe / unsubscribe of the reference's own suite: the bag it
    asserts, and (through the oracle's route/2 + dispatch/2 over the same
    ops) the dispatch it waits for"""
    e = Engine(device=-1)
    b = Broker(e, Router(e, node="n1"))
    o, bag = pytrie.RouteTable(), SubscriberBag()
    for op in case["ops"]:
        t, sub = op[1].encode(), op[2]
        if op[0] == "subscribe":
            assert b.subscribe(t, sub) == "ok"
            bag.insert_subscriber(None, t, sub)
            o.add_route(t, "n1")
        else:
            assert b.unsubscribe(t, sub) == "ok"
            if bag.delete_object(None, t, sub) == 0:
                o.del_route(t, "n1")
        e.debug_check_subs()
    for t, want in case["subscribers"].items():
        assert b.subscribers(t.encode()) == want
        assert bag.subscribers(t.encode()) == want
    if case["publish"] is not None:
        counts, pairs = route_dispatch(o, bag, b"n1", case["publish"].encode())
        assert [[to.decode(), s] for to, s in pairs] == case["dispatched"]
        assert counts == [1]
        assert e.get_routes(case["dispatched"][0][0].encode()) != []
    else:
        assert e.sub_count == 0 and e.route_count == 0
    e.close()


def test_insert_subscriber_quirks_and_remaining():
    e = Engine(device=-1)
    t = b"a/+"
    e.sub_add(t, 7)
    e.sub_add(t, 7)                       # a plain entry suppresses a plain add
    e.sub_add(t, 7, b"g1")                # ... and a shared add of the same sub, whatever the group
    assert e.subscribers(t) == [(7, Engine.NO_GROUP)]
    e.sub_add(t, 8, b"g1")
    e.sub_add(t, 8, b"g1")                # a repeated shared add duplicates the entry
    e.sub_add(t, 8, b"g2")
    e.sub_add(t, 8)                       # no plain 8 yet: appended
    e.sub_add(t, 8, b"g1")                # now suppressed by the plain 8
    g1, g2 = e.subscribers(t)[1][1], e.subscribers(t)[3][1]
    assert e.sub_group_bytes(g1) == b"g1" and e.sub_group_bytes(g2) == b"g2"
    assert e.subscribers(t) == [(7, Engine.NO_GROUP), (8, g1), (8, g1), (8, g2), (8, Engine.NO_GROUP)]
    assert e.sub_count == 5
    e.debug_check_subs()
    assert e.sub_del(t, 8, b"nogroup") == 5      # an absent object (unknown group): no-op
    assert e.sub_del(t, 9) == 5                  # an absent subscriber
    assert e.sub_del(t, 8, b"g1") == 3           # every duplicate goes, only entries of that group
    assert e.subscribers(t) == [(7, Engine.NO_GROUP), (8, g2), (8, Engine.NO_GROUP)]
    assert e.sub_del(t, 8, b"g1") == 3           # repeated: no-op
    assert e.sub_del(t, 8) == 2
    assert e.sub_del(t, 7) == 1
    e.debug_check_subs()
    assert e.sub_del(t, 8, b"g2") == 0
    assert e.subscribers(t) == [] and e.sub_count == 0
    assert e.sub_del(t, 8, b"g2") == 0           # the bag is gone
    assert e.sub_del(b"never", 1) == 0
    e.debug_check_subs()
    # the empty group is a group, not undefined
    e.sub_add(b"x", 1, b"")
    assert e.subscribers(b"x")[0][1] != Engine.NO_GROUP
    with pytest.raises(L.TopicMatchError) as ex:
        e.sub_add(b"x", 0xFFFFFFFF)
    assert ex.value.code == L.TM_EINVAL
    # none of it touched the trie or the routes
    assert e.filter_count == 0 and e.route_count == 0
    e.close()


def test_dispatch_calls_need_local_node_and_a_device():
    e = Engine(device=-1)
    buf, off = pack([b"a"])
    with pytest.raises(L.TopicMatchError) as ex:
        e.match_dispatch_batch(buf, off)
    assert ex.value.code == L.TM_EDEVICE      # host-only: no quiet CPU fall-back
    with pytest.raises(L.TopicMatchError) as ex:
        e.dispatch_batch(buf, off)
    assert ex.value.code == L.TM_EDEVICE
    e.close()


def test_sub_batches_match_single_calls():
    e1, e2 = Engine(device=-1), Engine(device=-1)
    rng = random.Random(3)
    topics = [b"t/%d" % rng.randrange(20) for _ in range(500)]
    subs = [rng.randrange(30) for _ in range(500)]
    groups = [rng.choice([None, b"g1", b"g2", b""]) for _ in range(500)]
    tb, to = pack(topics)
    gb, go = pack([g or b"" for g in groups])
    sh = [0 if g is None else 1 for g in groups]
    e1.sub_add_many(tb, to, subs, gb, go, sh)
    for t, s, g in zip(topics, subs, groups):
        e2.sub_add(t, s, g)
    e1.debug_check_subs()
    assert e1.sub_count == e2.sub_count > 0

    def named(e, t):
        return [(s, None if g == Engine.NO_GROUP else e.sub_group_bytes(g)) for s, g in e.subscribers(t)]
    for t in set(topics):
        assert named(e1, t) == named(e2, t)
    e1.sub_del_many(tb[: int(to[250])].copy(), to[:251], subs[:250], gb, go[:251], sh[:250])
    for t, s, g in list(zip(topics, subs, groups))[:250]:
        e2.sub_del(t, s, g)
    e1.debug_check_subs()
    for t in set(topics):
        assert named(e1, t) == named(e2, t)
    # plain-only form: no group arrays at all
    e1.sub_add_many(tb, to, subs)
    e1.debug_check_subs()
    e1.close()
    e2.close()


@pytest.mark.parametrize("seed", [1, 2])
def test_subscriber_image_mirrors_bags_under_churn(seed):
    """5,000 random add / del ops over 60 topics against dispatch_ref; route_gc
    tiny, so pool and arena compactions, exact-table regrowth and filters
    deleted / re-inserted behind the table's back all occur"""
    rng = random.Random(seed)
    e = Engine(device=-1)
    e.set_option("route_gc", 8)
    bag = SubscriberBag()
    words = [b"a", b"b", b"", b"+", b"#", b"$SYS", b"c", b"d"]
    pool = set()
    while len(pool) < 60:
        ws = [rng.choice(words) for _ in range(rng.randint(1, 5))]
        if b"#" not in ws[:-1]:
            pool.add(b"/".join(ws))
    pool = sorted(pool)
    wild = [t for t in pool if b"+" in t.split(b"/") or t.endswith(b"#")]
    groups = [None, None, None, None, b"g1", b"g2", b"g3"]
    in_trie = set()
    for burst in range(25):
        for _ in range(200):
            t, s, g = rng.choice(pool), rng.randrange(80), rng.choice(groups)
            if rng.random() < 0.04:
                s = 1000 + rng.randrange(400)          # long bags on a few topics: the membership index
                t = pool[burst % 3]
                g = None
            if rng.random() < 0.55:
                e.sub_add(t, s, g)
                bag.insert_subscriber(g, t, s)
            else:
                assert e.sub_del(t, s, g) == bag.delete_object(g, t, s)
        # trie filters come and go independently of the bag, in either order of arrival
        for t in rng.sample(wild, 4):
            if t in in_trie:
                e.delete(t)
                in_trie.discard(t)
            else:
                e.insert(t)
                in_trie.add(t)
            e.debug_check_subs()
        if burst % 6 == 5:                              # a burst that empties most bags: garbage past half
            for t in pool[::2]:
                for x in bag.subscribers(t):
                    s, g = (x[2], x[1]) if isinstance(x, tuple) else (x, None)
                    assert e.sub_del(t, s, g) == bag.delete_object(g, t, s)
        e.debug_check_subs()
        assert e.sub_count == bag.size()
        for t in pool:
            got = [(s, None if g == Engine.NO_GROUP else e.sub_group_bytes(g)) for s, g in e.subscribers(t)]
            want = [(x[2], x[1]) if isinstance(x, tuple) else (x, None) for x in bag.subscribers(t)]
            assert got == want, (burst, t)
    e.close()
