"""publish/1's local dispatch on the GPU (walk + route expansion + aggre +
dispatch.hip) against tests/dispatch_ref.py (route/2 + dispatch/2 over
oracle/pytrie.py RouteTable.match_deliveries): per delivery the dispatch Count
(or NOT_LOCAL), per topic the ordered (To, subscriber) pairs, compared element
for element."""
import json
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dispatch_ref import SubscriberBag, route_dispatch  # noqa: E402
from emqx_amd import Engine  # noqa: E402
from emqx_amd import _lib as L  # noqa: E402
from emqx_amd.emqx_broker import Broker  # noqa: E402
from emqx_amd.emqx_router import Router  # noqa: E402
from emqx_amd.engine import pack  # noqa: E402
from oracle import pytrie  # noqa: E402
from trie_churn import read_back  # noqa: E402

pytestmark = pytest.mark.gpu

DESTS = ["n1", "n2", ("g1", "n1"), ("g1", "n2"), ("g2", "n2"), "n3", ("a", "n3"), "g1"]
GROUPS = ["g1", "g2", "g3"]


def _pool(rng, k):
    words = [b"a", b"b", b"", b"+", b"#", b"$SYS", b"c", b"d"]
    pool = set()
    while len(pool) < k:
        ws = [rng.choice(words) for _ in range(rng.randint(1, 5))]
        if b"#" in ws[:-1]:
            continue
        pool.add(b"/".join(ws))
    return sorted(pool)


def _topics(rng, k):
    words = [b"a", b"b", b"", b"$SYS", b"c", b"d", b"x"]
    return [b"/".join(rng.choice(words) for _ in range(rng.randint(1, 6))) for _ in range(k)]


def _check(b, o, bag, topics, tag=None):
    """publish_many(topics) against the oracle; returns the per-topic pair totals"""
    got = b.publish_many(topics)
    totals = []
    for tp, pub in zip(topics, got):
        counts, pairs = route_dispatch(o, bag, b"n1", tp)
        assert [(d.to, d.target) for d in pub.deliveries] == o.match_deliveries(tp), (tag, tp)
        assert [d.count for d in pub.deliveries] == counts, (tag, tp)
        assert pub.pairs == pairs, (tag, tp)
        totals.append(len(pairs))
    return totals


def test_dispatch_random_ops_vs_oracle(gpu_device):
    rng = random.Random(77)
    for rep in range(4):
        e = Engine(device=gpu_device)
        if rep % 2:
            e.set_option("layout", 2)
        r, o, bag = Router(e, node="n1"), pytrie.RouteTable(), SubscriberBag()
        b = Broker(e, r)
        pool = _pool(rng, 60)
        for step in range(600):
            t = rng.choice(pool)
            if rng.random() < 0.5:
                d = rng.choice(DESTS)
                if rng.random() < 0.7:
                    r.add_route(t, d)
                    o.add_route(t, d)
                else:
                    r.del_route(t, d)
                    o.del_route(t, d)
            else:
                s = rng.randrange(40)
                g = rng.choice(GROUPS) if rng.random() < 1 / 3 else None
                if rng.random() < 0.7:
                    e.sub_add(t, s, g.encode() if g else None)
                    bag.insert_subscriber(g, t, s)
                else:
                    assert e.sub_del(t, s, g.encode() if g else None) == bag.delete_object(g, t, s)
            if step % 150 == 149:
                totals = _check(b, o, bag, _topics(rng, 300) + pool, (rep, step))
                assert sum(totals) > 0
        e.close()


def test_dispatch_bag_sizes_across_emit_partitions(gpu_device):
    """bags of 0 / 1 / 63 / 64 / 65 / 257 / 5,000 plain subscribers on '#',
    'a/#', 'a/+', '+/b' and the exact topic 'a/b': one pair, a wave's 64-slot
    window and its neighbours, several windows, several 1024-pair chunks of
    one bag; with a shared-only bag (Count > 0, no pair), a route without a
    bag (Count 0), a remote-node and a group delivery (NOT_LOCAL, no pair)"""
    sizes = [0, 1, 63, 64, 65, 257, 5000]
    where = [b"#", b"a/#", b"a/+", b"+/b", b"a/b"]
    topics = [b"a/b", b"a/c", b"x/b", b"a", b"$SYS/b", b"q"]
    seen = set()
    rng = random.Random(9)
    for shift in (0, 3, 5):
        e = Engine(device=gpu_device)
        r, o, bag = Router(e, node="n1"), pytrie.RouteTable(), SubscriberBag()
        b = Broker(e, r)
        ids = list(range(20000))
        rng.shuffle(ids)
        tl, sl = [], []
        for i, f in enumerate(where):
            r.add_route(f, "n1")
            o.add_route(f, "n1")
            for _ in range(sizes[(i + shift) % len(sizes)]):
                s = ids.pop()
                tl.append(f)
                sl.append(s)
                bag.insert_subscriber(None, f, s)
        tb, to = pack(tl)
        e.sub_add_many(tb, to, sl)
        for f, d in [(b"q", "n1"), (b"$SYS/+", "n1"), (b"a/+", "n2"), (b"#", ("g1", "n1"))]:
            r.add_route(f, d)
            o.add_route(f, d)
        for s in (1, 2, 2):                              # a bag of shared entries only, one duplicated
            e.sub_add(b"q", 30000 + s, b"g1")
            bag.insert_subscriber("g1", b"q", 30000 + s)
        totals = _check(b, o, bag, topics, shift)
        seen.update(totals)
        pub = dict(zip(topics, b.publish_many(topics)))
        q = {d.to: d.count for d in pub[b"q"].deliveries if d.target == (0, b"n1")}
        assert q[b"q"] == 3 and not [p for p in pub[b"q"].pairs if p[0] == b"q"]
        assert [d.count for d in pub[b"$SYS/b"].deliveries] == [0] and pub[b"$SYS/b"].pairs == []
        assert None in [d.count for d in pub[b"a/b"].deliveries if d.target == (0, b"n2")]
        assert None in [d.count for d in pub[b"q"].deliveries if d.target == (1, b"g1")]
        e.close()
    assert 0 in seen and any(0 < x <= 64 for x in seen) and any(x > 5000 for x in seen), sorted(seen)


def test_dispatch_over_aggre_holes(gpu_device):
    """a topic whose aggre usort removed duplicates (out_count < span): the
    pairs come from the deliveries kept, the hole dispatches nothing"""
    e = Engine(device=gpu_device)
    r, o, bag = Router(e, node="n1"), pytrie.RouteTable(), SubscriberBag()
    b = Broker(e, r)
    for t in [b"a/+", b"a/#", b"#", b"a/b"]:
        r.add_route(t, "n1")
        o.add_route(t, "n1")
    for d in [("g", "n2"), ("g", "n1")]:
        r.add_route(b"a/#", d)
        o.add_route(b"a/#", d)
    k = 0
    for t, m in [(b"a/+", 3), (b"a/#", 70), (b"#", 2), (b"a/b", 5)]:
        for _ in range(m):
            e.sub_add(t, k)
            bag.insert_subscriber(None, t, k)
            k += 1
    topics = [b"a/b", b"$SYS/x", b"", b"a"]
    tb, to = pack(topics)
    counts, offs, to_, tg, nd, scount, soff, sto, sid = e.match_dispatch_batch(tb, to)
    assert int(counts[0]) < int(offs[1]) - int(offs[0])          # the hole
    assert int(counts[0]) == 5 and int(offs[1]) == 6
    assert int(scount[0]) == 80 and list(soff) == [0, 80, 80, 82, 154]
    _check(b, o, bag, topics)
    e.close()


def test_dispatch_device_api_caps_and_empty(gpu_device):
    import torch
    e = Engine(device=gpu_device)
    dev = torch.device("cuda", gpu_device)
    r, o, bag = Router(e, node="n1"), pytrie.RouteTable(), SubscriberBag()
    tb0, to0 = pack([b"a/b"])
    with pytest.raises(L.TopicMatchError) as ex:                  # before tm_set_local_node
        e.match_dispatch_batch(tb0, to0)
    assert ex.value.code == L.TM_EINVAL
    with pytest.raises(L.TopicMatchError) as ex:
        e.dispatch_batch(tb0, to0)
    assert ex.value.code == L.TM_EINVAL
    b = Broker(e, r)
    k = 0
    for t, m in [(b"a/+", 300), (b"#", 40), (b"a/b", 7)]:
        r.add_route(t, "n1")
        o.add_route(t, "n1")
        for _ in range(m):
            e.sub_add(t, k)
            bag.insert_subscriber(None, t, k)
            k += 1
    topics = [b"a/b", b"x", b"$SYS/x", b"a/c"]
    tb, to = pack(topics)
    n = len(topics)
    want_pairs = sum((route_dispatch(o, bag, b"n1", tp)[1] for tp in topics), [])
    assert len(want_pairs) == 347 + 40 + 340
    # host call: each capacity reports its own need, then an exact retry
    with pytest.raises(L.TopicMatchError) as ex:
        e.match_dispatch_batch(tb, to, out_cap=64, sub_cap=100)
    assert ex.value.code == L.TM_ENOSPC and ex.value.sub_needed == len(want_pairs) and ex.value.needed == 6
    with pytest.raises(L.TopicMatchError) as ex:
        e.match_dispatch_batch(tb, to, out_cap=2, sub_cap=1 << 12)
    assert ex.value.code == L.TM_ENOSPC and ex.value.needed == 6 and ex.value.sub_needed == len(want_pairs)
    res = e.match_dispatch_batch(tb, to, out_cap=6, sub_cap=len(want_pairs))
    assert len(res[7]) == len(want_pairs) and int(res[6][-1]) == len(want_pairs)
    names = {Engine.TOPIC_ROUTE: None}

    def pairs_of(sto, sid, soff, scount):
        out = []
        for t in range(n):
            for j in range(int(soff[t]), int(soff[t]) + int(scount[t])):
                s = int(sto[j])
                if s not in names:
                    names[s] = e.filter_bytes(s)
                out.append((topics[t] if s == Engine.TOPIC_ROUTE else names[s], int(sid[j])))
        return out
    assert pairs_of(res[7], res[8], res[6], res[5]) == want_pairs

    def dev_call(d_b, d_o, m, nbytes, out_cap, sub_cap):
        t = dict(c=torch.zeros(max(m, 1), dtype=torch.int32, device=dev),
                 o=torch.full((m + 1,), -1, dtype=torch.int64, device=dev),
                 to=torch.zeros(max(out_cap, 1), dtype=torch.int32, device=dev),
                 tg=torch.zeros(max(out_cap, 1), dtype=torch.int32, device=dev),
                 nd=torch.zeros(max(out_cap, 1), dtype=torch.int32, device=dev),
                 tot=torch.full((1,), -1, dtype=torch.int64, device=dev),
                 sc=torch.zeros(max(m, 1), dtype=torch.int32, device=dev),
                 so=torch.full((m + 1,), -1, dtype=torch.int64, device=dev),
                 sto=torch.full((sub_cap + 8,), -7, dtype=torch.int32, device=dev),
                 sid=torch.full((sub_cap + 8,), -7, dtype=torch.int32, device=dev),
                 stot=torch.full((1,), -1, dtype=torch.int64, device=dev))
        torch.cuda.synchronize()
        e.match_dispatch_batch_device(d_b, d_o, m, nbytes, t["c"], t["o"], t["to"], t["tg"], t["nd"], out_cap,
                                      t["tot"], t["sc"], t["so"], t["sto"], t["sid"], sub_cap, t["stot"])
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in t.items()}
    d_b = torch.from_numpy(tb.copy()).to(dev)
    d_o = torch.from_numpy(to.view(np.int64).copy()).to(dev)
    # n = 0
    z = dev_call(d_b, d_o, 0, 0, 16, 16)
    assert int(z["o"][0]) == 0 and int(z["tot"][0]) == 0 and int(z["so"][0]) == 0 and int(z["stot"][0]) == 0
    # enough room
    full = dev_call(d_b, d_o, n, int(to[-1]), 64, 1024)
    assert int(full["tot"][0]) == 6 and int(full["stot"][0]) == len(want_pairs)
    assert pairs_of(full["sto"].view(np.uint32), full["sid"].view(np.uint32), full["so"], full["sc"]) == want_pairs
    assert list(full["nd"][:6].view(np.uint32)) == list(res[4])
    assert list(full["sid"][len(want_pairs):]) == [-7] * (1024 + 8 - len(want_pairs))
    # sub_cap short: the pairs past it are dropped, nothing is written past it, the totals are right
    cut = dev_call(d_b, d_o, n, int(to[-1]), 64, 100)
    assert int(cut["stot"][0]) == len(want_pairs) and list(cut["so"]) == list(full["so"])
    assert list(cut["sc"]) == list(full["sc"])
    assert list(cut["sid"][:100]) == list(full["sid"][:100]) and list(cut["sto"][:100]) == list(full["sto"][:100])
    assert list(cut["sid"][100:]) == [-7] * 8 and list(cut["sto"][100:]) == [-7] * 8
    e.close()


def test_dispatch_batch_by_to_bytes(gpu_device):
    """tm_dispatch_batch: dispatch/2 as forward/3 calls it, To given by its bytes"""
    e = Engine(device=gpu_device)
    r, bag = Router(e, node="n1"), SubscriberBag()
    b = Broker(e, r)
    k = 0
    for t, m, g in [(b"a/+", 130, None), (b"a/b", 3, None), (b"a/b", 2, "g1"), (b"s/#", 4, "g2")]:
        for _ in range(m):
            b.subscribe(t, k, g)
            bag.insert_subscriber(g, t, k)
            k += 1
    tos = [b"a/+", b"a/b", b"nobody/home", b"s/#", b"a/+", b""]
    got = b.dispatch_many(tos)
    for to, (count, subs) in zip(tos, got):
        want = bag.subscribers(to)
        assert count == len(want)
        assert subs == [x for x in want if not isinstance(x, tuple)]
    assert got[0][0] == 130 and got[1] == (5, [130, 131, 132]) and got[2] == (0, []) and got[3] == (4, [])
    nd, soff, sid = e.dispatch_batch(*pack(tos))
    with pytest.raises(L.TopicMatchError) as ex:
        e.dispatch_batch(*pack(tos), cap=10)
    assert ex.value.code == L.TM_ENOSPC
    assert int(soff[-1]) == 263
    e.close()


def test_broker_suite_publishes_on_device(gpu_device):
    """the reference suite's publishes (tests/golden/kat_broker.json): each
    subscriber receives {dispatch, To, Msg} for exactly the To it names"""
    with open(os.path.join(ROOT, "tests", "golden", "kat_broker.json")) as f:
        cases = json.load(f)["cases"]
    e = Engine(device=gpu_device)
    b = Broker(e, Router(e, node="n1"))
    for case in cases:
        for op in case["ops"]:
            (b.subscribe if op[0] == "subscribe" else b.unsubscribe)(op[1].encode(), op[2])
        for t, want in case["subscribers"].items():
            assert b.subscribers(t.encode()) == want
        if case["publish"] is not None:
            pub = b.publish(case["publish"].encode())
            assert [[to.decode(), s] for to, s in pub.pairs] == case["dispatched"]
            assert [d.count for d in pub.deliveries] == [1]
        for op in case["ops"]:                                   # leave nothing behind for the next case
            b.unsubscribe(op[1].encode(), op[2])
        assert e.sub_count == 0 and e.route_count == 0
    e.close()


def test_released_filter_id_carries_no_bag(gpu_device):
    """fs_meta is cleared when a filter id is released (the hazard of
    tests/test_id_reuse.py): another filter that takes the id must not
    dispatch to the old filter's subscribers, and the bag joins its filter
    again when the filter comes back (either order of arrival)"""
    e = Engine(device=gpu_device)
    r = Router(e, node="n1")
    b = Broker(e, r)
    for s in (1, 2, 3):
        b.subscribe(b"a/+", s)
    assert b.publish(b"a/x").pairs == [(b"a/+", 1), (b"a/+", 2), (b"a/+", 3)]
    e.delete(b"a/+")                      # the filter leaves the trie behind the broker's back
    assert b.publish(b"a/x") == ([], [])
    for _ in range(3):                    # both image epochs drop the id: it becomes reusable
        e.commit()
    for k in range(4):                    # new filters, one of which takes the released id
        r.add_route(b"b%d/+" % k, "n1")
    got = b.publish_many([b"b%d/x" % k for k in range(4)] + [b"a/x"])
    for k in range(4):
        assert [(d.to, d.count) for d in got[k].deliveries] == [(b"b%d/+" % k, 0)] and got[k].pairs == []
    assert got[4] == ([], [])
    e.insert(b"a/+")                      # the filter is back: its bag is linked again
    assert b.publish(b"a/x").pairs == [(b"a/+", 1), (b"a/+", 2), (b"a/+", 3)]
    assert b.dispatch_many([b"a/+"]) == [(3, [1, 2, 3])]
    e.debug_check_subs()
    e.close()


@pytest.mark.parametrize("double_buffer", [1, 0])
def test_subscriber_image_churn_on_device_vs_oracle(gpu_device, double_buffer):
    """the in-place subscriber image on the device under churn: compactions
    (route_gc tiny), exact-table regrowth, a filter deleted and re-inserted
    behind the broker's back; every burst's publishes equal the oracle's,
    with two image epochs and with one"""
    rng, mini = random.Random(53 + double_buffer), random.Random(153)
    copies, scatters = {}, {}
    e = Engine(device=gpu_device)
    e.set_option("route_gc", 64)
    e.set_option("double_buffer", double_buffer)
    r, o, bag = Router(e, node="n1"), pytrie.RouteTable(), SubscriberBag()
    b = Broker(e, r)
    pool = _pool(rng, 400) + [b"t/%05d" % i for i in range(600)]

    def dest(g):
        return "n1" if g is None else (g, "n1")
    live = []
    for burst in range(12):
        for _ in range(700):
            if rng.random() < 0.6 or not live:
                t = rng.choice(pool) if rng.random() < 0.9 else pool[burst]     # a few long bags
                s = rng.randrange(5000)
                g = rng.choice(GROUPS) if rng.random() < 0.25 else None
                b.subscribe(t, s, g)
                bag.insert_subscriber(g, t, s)
                o.add_route(t, dest(g))
                live.append((t, s, g))
            else:
                t, s, g = live.pop(rng.randrange(len(live)))
                b.unsubscribe(t, s, g)
                if bag.delete_object(g, t, s) == 0:
                    o.del_route(t, dest(g))
        if burst % 3 == 2:   # a wildcard filter deleted and re-inserted behind the broker's back
            w = [t for t in o.routes if b"+" in t.split(b"/") or t.endswith(b"#")]
            if w:
                t = rng.choice(sorted(w))
                e.delete(t)
                e.insert(t)
        if burst % 4 == 3:
            e.debug_check_subs()
            e.debug_check_routes()
        # the image read back after the burst's commit (mostly whole-table copies: 700 ops on small
        # tables), then two bursts of ten ops: their commits scatter the changed elements
        read_back(e, copies)
        for _ in range(2):
            for k in range(10):
                if k % 2 == 0:      # a new plain subscriber of a topic that has some
                    t, s = mini.choice(live)[0], 6000 + mini.randrange(1000)
                    b.subscribe(t, s, None)
                    bag.insert_subscriber(None, t, s)
                    o.add_route(t, dest(None))
                    live.append((t, s, None))
                else:
                    t, s, g = live.pop(mini.randrange(len(live)))
                    b.unsubscribe(t, s, g)
                    if bag.delete_object(g, t, s) == 0:
                        o.del_route(t, dest(g))
            read_back(e, scatters)
        topics = _topics(rng, 200) + [t for t in pool[:50] if b"+" not in t and b"#" not in t] + pool[400:420]
        totals = _check(b, o, bag, topics, burst)
        assert sum(totals) > 0
    # the exact table, the subscriber pool and fs_meta each took the scatter path (one log with one
    # image epoch, this and the previous commit's with two) at least once
    for t in ("sx_slots", "sx_pool", "fs_meta"):
        assert scatters[t] & {1, 2} == {2 if double_buffer else 1}, (t, scatters[t], copies[t])
    e.close()
