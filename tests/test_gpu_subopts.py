"""The per-pair delivery word on the GPU (dispatch.hip tm_dispatch_count_pub /
tm_dispatch_emit_opts over the option pool sx_opt) against
tests/subopts_ref.py: handle_dispatch/3 + run_dispatch_steps/3
(src/emqx_session.erl:667-684, 797-819) for every (To, subscriber) pair of
publish/1, with every other output element for element what the call without
options returns."""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import subopts_corpus as C  # noqa: E402
from emqx_amd import Engine  # noqa: E402
from emqx_amd.emqx_broker import Broker, pack_msgs, pack_subopts, unpack_deliver  # noqa: E402
from emqx_amd.emqx_router import Router  # noqa: E402
from emqx_amd.engine import pack  # noqa: E402
from oracle import pytrie  # noqa: E402
from subopts_ref import SubOptionTable, dispatch_opts, route_dispatch_opts  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -7


def _flags(upgrade):
    return Engine.DELIVER_UPGRADE_QOS if upgrade else 0


def _dev_call(e, dev, tb, to, out_cap, sub_cap, deliver=None):
    """the device form (plain, or with deliver=(pub_flags, pub_from | None,
    flags)) -> numpy arrays; the pair arrays carry 8 sentinel words past
    sub_cap"""
    import torch
    n = len(to) - 1
    d_b = torch.from_numpy(np.ascontiguousarray(tb).copy()).to(dev)
    d_o = torch.from_numpy(to.view(np.int64).copy()).to(dev)
    i32 = dict(dtype=torch.int32, device=dev)
    t = dict(c=torch.zeros(max(n, 1), **i32), o=torch.full((n + 1,), -1, dtype=torch.int64, device=dev),
             to=torch.zeros(max(out_cap, 1), **i32), tg=torch.zeros(max(out_cap, 1), **i32),
             nd=torch.zeros(max(out_cap, 1), **i32), tot=torch.full((1,), -1, dtype=torch.int64, device=dev),
             sc=torch.zeros(max(n, 1), **i32), so=torch.full((n + 1,), -1, dtype=torch.int64, device=dev),
             sto=torch.full((sub_cap + 8,), SENTINEL, **i32), sid=torch.full((sub_cap + 8,), SENTINEL, **i32),
             stot=torch.full((1,), -1, dtype=torch.int64, device=dev))
    dv = None
    if deliver is not None:
        pf, fr, fl = deliver
        t["sdv"] = torch.full((sub_cap + 8,), SENTINEL, **i32)
        d_pf = torch.from_numpy(np.asarray(pf, dtype=np.uint32).view(np.int32).copy()).to(dev)
        d_fr = None if fr is None else torch.from_numpy(np.asarray(fr, dtype=np.uint32).view(np.int32).copy()).to(dev)
        dv = (d_pf, d_fr, fl, t["sdv"])
    torch.cuda.synchronize()
    e.match_dispatch_batch_device(d_b, d_o, n, int(to[-1]), t["c"], t["o"], t["to"], t["tg"], t["nd"], out_cap,
                                  t["tot"], t["sc"], t["so"], t["sto"], t["sid"], sub_cap, t["stot"], deliver=dv)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in t.items()}


def _check(b, o, ref, topics, msgs, upgrade, dev=None, tag=None):
    """publish_many(topics, msgs) against the oracle and against the plain
    call; with dev also the device form against the host form's arrays.
    Returns the outcomes the batch showed."""
    e = b.engine
    got = b.publish_many(topics, msgs, upgrade_qos=upgrade)
    plain = b.publish_many(topics)
    seen = set()
    for tp, msg, pub, pl in zip(topics, msgs, got, plain):
        counts, pairs = route_dispatch_opts(o, ref, b"n1", tp, msg, upgrade)
        assert pub.deliveries == pl.deliveries and [d.count for d in pub.deliveries] == counts, (tag, tp)
        assert [p[:2] for p in pub.pairs] == pl.pairs, (tag, tp)
        assert pub.pairs == pairs, (tag, tp, msg)
        for to, s, res in pairs:
            seen |= C.outcomes(ref.get_subopts(to, s), msg, res)
    if dev is not None:
        tb, to = pack(topics)
        pf, fr = pack_msgs(msgs)
        host = e.match_dispatch_batch(tb, to, deliver=(pf, fr, _flags(upgrade)))
        out_cap, sub_cap = len(host[2]) + 3, len(host[7]) + 5
        d1 = _dev_call(e, dev, tb, to, out_cap, sub_cap, (pf, fr, _flags(upgrade)))
        d0 = _dev_call(e, dev, tb, to, out_cap, sub_cap)
        k, sk = len(host[2]), len(host[7])
        assert int(d1["tot"][0]) == k and int(d1["stot"][0]) == sk
        for name in ("c", "o", "to", "tg", "nd", "tot", "sc", "so", "sto", "sid", "stot"):
            assert np.array_equal(d1[name], d0[name]), (tag, name)      # every existing output: the plain call's
        live = np.zeros(k, dtype=bool)                       # a span's slots past its count are holes: undefined
        for t in range(len(topics)):
            live[int(host[1][t]):int(host[1][t]) + int(host[0][t])] = True
        for name, i, m in (("c", 0, len(topics)), ("o", 1, len(topics) + 1), ("to", 2, k), ("tg", 3, k), ("nd", 4, k),
                           ("sc", 5, len(topics)), ("so", 6, len(topics) + 1), ("sto", 7, sk), ("sid", 8, sk),
                           ("sdv", 9, sk)):
            a, h = d1[name][:m].view(host[i].dtype), host[i]
            if name in ("to", "tg", "nd"):
                a, h = a[live], h[live]
            assert np.array_equal(a, h), (tag, name)
        assert list(d1["sdv"][sk:]) == [SENTINEL] * (sub_cap + 8 - sk)
    return seen


@pytest.mark.parametrize("upgrade", [False, True])
def test_opts_random_ops_vs_oracle(gpu_device, upgrade):
    import torch
    dev = torch.device("cuda", gpu_device)
    seen = set()
    for rep, steps in enumerate(C.corpus()):
        e = Engine(device=gpu_device)
        if rep % 2:
            e.set_option("layout", 2)
        r, o, ref = Router(e, node="n1"), pytrie.RouteTable(), SubOptionTable()
        b = Broker(e, r)
        for i, step in enumerate(steps):
            op = step[0]
            if op == "check":
                seen |= _check(b, o, ref, step[1], step[2], upgrade, dev, (rep, i))
                continue
            want = C.apply_ref(step, o, ref)
            if op == "route_add":
                r.add_route(step[1], step[2])
            elif op == "route_del":
                r.del_route(step[1], step[2])
            elif op == "add":
                _, t, s, g, opts = step
                if opts is None:
                    e.sub_add(t, s, g.encode() if g else None)
                else:
                    e.sub_add_opts(t, s, pack_subopts(opts), g.encode() if g else None)
            elif op == "del":
                assert e.sub_del(step[1], step[2], step[3].encode() if step[3] else None) == want
            else:
                assert b.set_subopts(step[1], step[2], step[3]) is want
        e.debug_check_subs()
        e.close()
    assert seen == set(C.OUTCOMES) - {"downgraded" if upgrade else "upgraded"}, sorted(seen)


def _word(i):
    """a distinct option word per subscriber, no-local set"""
    return {"qos": i % 3, "nl": 1, "rap": (i >> 1) & 1, "subid": i + 1}


def test_opts_bag_sizes_across_emit_partitions(gpu_device):
    """bags of 1 / 63 / 64 / 65 / 257 / 5,000 with a distinct word per
    subscriber on '#', 'a/#', 'a/+', '+/b' and 'a/b'; the publisher's own id
    first, last and at positions 63 / 64 / 1,023 / 1,024 of the 5,000 bag (the
    64-slot window and the 1,024-pair chunk edges) with no-local set; a
    shared-only bag, a hole left by aggre's usort and NOT_LOCAL slots between
    the local ones"""
    sizes = [1, 63, 64, 65, 257, 5000]
    where = [b"#", b"a/#", b"a/+", b"+/b", b"a/b"]
    rng = random.Random(9)
    dropped = 0
    for shift in (1, 3, 5):
        e = Engine(device=gpu_device)
        r, o, ref = Router(e, node="n1"), pytrie.RouteTable(), SubOptionTable()
        b = Broker(e, r)
        ids = list(range(20000))
        rng.shuffle(ids)
        tl, sl, wl, big = [], [], [], None
        for i, f in enumerate(where):
            r.add_route(f, "n1")
            o.add_route(f, "n1")
            size = sizes[(i + shift) % len(sizes)]
            bag = [ids.pop() for _ in range(size)]
            if size == 5000:
                big = (f, bag)
            for s in bag:
                tl.append(f)
                sl.append(s)
                wl.append(pack_subopts(_word(s)))
                ref.do_subscribe(None, f, s, _word(s))
        tb, to = pack(tl)
        e.sub_add_opts_many(tb, to, sl, wl)
        for f, d in [(b"q", "n1"), (b"$SYS/+", "n1"), (b"a/+", "n2"), (b"#", ("g1", "n1")), (b"a/#", ("g", "n2")),
                     (b"a/#", ("g", "n1"))]:
            r.add_route(f, d)
            o.add_route(f, d)
        for s in (1, 2, 2):                                  # a bag of shared entries only
            e.sub_add_opts(b"q", 30000 + s, pack_subopts(_word(s)), b"g1")
            ref.do_subscribe("g1", b"q", 30000 + s, _word(s))
        f, bag = big
        hit = {b"#": b"a/b", b"a/#": b"a/b", b"a/+": b"a/c", b"+/b": b"x/b", b"a/b": b"a/b"}[f]
        topics = [b"a/b", b"a/c", b"x/b", b"a", b"$SYS/b", b"q"] + [hit] * 6
        msgs = [(2, 1, 0, None)] * 6 + [(1, 1, 0, bag[p]) for p in (0, 63, 64, 1023, 1024, 4999)]
        counts = e.match_dispatch_batch(*pack([b"a/b"]))[0]
        offs = e.match_dispatch_batch(*pack([b"a/b"]))[1]
        assert int(counts[0]) < int(offs[1])                 # the hole is there
        _check(b, o, ref, topics, msgs, False, None, shift)
        got = b.publish_many(topics, msgs)
        for pub, msg in zip(got[6:], msgs[6:]):
            gone = [p for p in pub.pairs if p[2] is None]
            assert [(p[0], p[1]) for p in gone] == [(f, msg[3])]      # exactly the publisher's own pair
            dropped += len(gone)
        e.debug_check_subs()
        e.close()
    assert dropped == 18


@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_opts_publish_index_per_slot(gpu_device, n):
    """the count pass works on blocks of 256 topics: every pair carries its
    own publish's (qos, retain, from) on both sides of the block edges"""
    e = Engine(device=gpu_device)
    r, o, ref = Router(e, node="n1"), pytrie.RouteTable(), SubOptionTable()
    b = Broker(e, r)
    for t in [b"t/+"] + [b"t/%d" % i for i in range(0, n, 3)]:
        r.add_route(t, "n1")
        o.add_route(t, "n1")
    for s in (1000, 1001, 1002):
        opts = {"qos": 2, "nl": 0, "rap": 1, "subid": s}
        e.sub_add_opts(b"t/+", s, pack_subopts(opts))
        ref.do_subscribe(None, b"t/+", s, opts)
    for i in range(0, n, 3):                                  # the topic's own subscriber is its publisher
        opts = {"qos": 2, "nl": i % 2, "rap": 1}
        e.sub_add_opts(b"t/%d" % i, i, pack_subopts(opts))
        ref.do_subscribe(None, b"t/%d" % i, i, opts)
    topics = [b"t/%d" % i for i in range(n)]
    msgs = [(i % 3, (i >> 2) & 1, 1 if i % 7 == 0 else 0, i if i % 5 else None) for i in range(n)]
    seen = _check(b, o, ref, topics, msgs, False, None, n)
    assert "dropped" in seen
    got = b.publish_many(topics, msgs)
    for i, pub in enumerate(got):
        want = (min(2, i % 3), 1 if i % 7 == 0 else (i >> 2) & 1)
        assert [p[2][:2] for p in pub.pairs if p[0] == b"t/+"] == [want] * 3, i
    e.close()


def test_opts_device_capacities(gpu_device):
    """out_cap and sub_cap below the need: the words below sub_cap are exact,
    nothing is written past it"""
    import torch
    dev = torch.device("cuda", gpu_device)
    e = Engine(device=gpu_device)
    r, o, ref = Router(e, node="n1"), pytrie.RouteTable(), SubOptionTable()
    Broker(e, r)
    k = 0
    for t, m in [(b"a/+", 300), (b"#", 40), (b"a/b", 7)]:
        r.add_route(t, "n1")
        o.add_route(t, "n1")
        for _ in range(m):
            e.sub_add_opts(t, k, pack_subopts(_word(k)))
            ref.do_subscribe(None, t, k, _word(k))
            k += 1
    topics = [b"a/b", b"x", b"$SYS/x", b"a/c"]
    msgs = [(2, 1, 0, 5), (1, 0, 1, 301), (0, 0, 0, None), (2, 1, 1, 299)]
    tb, to = pack(topics)
    pf, fr = pack_msgs(msgs)
    names = {}

    def expect(d, limit):
        """the words of the pairs the call kept, from the oracle's option table"""
        out = []
        for t in range(len(topics)):
            for j in range(int(d["so"][t]), int(d["so"][t]) + int(d["sc"][t])):
                if j >= limit:
                    continue
                fid, s = int(d["sto"].view(np.uint32)[j]), int(d["sid"][j])
                if fid not in names:
                    names[fid] = topics[t] if fid == Engine.TOPIC_ROUTE else e.filter_bytes(fid)
                to_name = topics[t] if fid == Engine.TOPIC_ROUTE else names[fid]
                opts = ref.get_subopts(to_name, s)
                out.append(e.deliver_word(pack_subopts(opts), pf[t], s == fr[t], 0))
        return out
    full = _dev_call(e, dev, tb, to, 64, 1024, (pf, fr, 0))
    need = int(full["stot"][0])
    assert need == 347 + 40 + 340 and list(full["sdv"][:need].view(np.uint32)) == expect(full, need)
    assert Engine.DELIVER_DROP in list(full["sdv"][:need])
    assert list(full["sdv"][need:]) == [SENTINEL] * (1024 + 8 - need)
    for out_cap, sub_cap in ((64, 100), (64, 65), (2, 1024), (2, 100), (64, 0)):
        cut = _dev_call(e, dev, tb, to, out_cap, sub_cap, (pf, fr, 0))
        ref_cut = _dev_call(e, dev, tb, to, out_cap, sub_cap)
        for name in ref_cut:
            assert np.array_equal(cut[name], ref_cut[name]), (out_cap, sub_cap, name)
        kept = min(int(cut["stot"][0]), sub_cap)
        assert list(cut["sdv"][:kept].view(np.uint32)) == expect(cut, kept), (out_cap, sub_cap)
        assert list(cut["sdv"][kept:]) == [SENTINEL] * (sub_cap + 8 - kept), (out_cap, sub_cap)
        if out_cap == 64:
            assert list(cut["sdv"][:kept]) == list(full["sdv"][:kept])
    e.close()


@pytest.mark.parametrize("double_buffer", [1, 0])
def test_opts_across_commits(gpu_device, double_buffer):
    """set_opts, del and re-add, then a segment move, each between two
    batches: the batch before sees the old words, the batch after the new
    ones, in both image epochs; a filter id deleted and reused inherits no
    word"""
    e = Engine(device=gpu_device)
    e.set_option("double_buffer", double_buffer)
    r, o, ref = Router(e, node="n1"), pytrie.RouteTable(), SubOptionTable()
    b = Broker(e, r)
    for t in (b"a/+", b"a/x", b"z"):
        r.add_route(t, "n1")
        o.add_route(t, "n1")

    def sub(t, s, opts):
        e.sub_add_opts(t, s, pack_subopts(opts))
        ref.do_subscribe(None, t, s, opts)

    def words():
        topics, msgs = [b"a/x", b"z"], [(2, 1, 0, 2), (1, 1, 0, None)]
        _check(b, o, ref, topics, msgs, False, None)
        return [p[2] for p in b.publish_many(topics, msgs)[0].pairs]
    for s in (1, 2, 3):
        sub(b"a/+", s, {"qos": 1, "nl": 0, "rap": 0})
    sub(b"z", 9, {"qos": 0})
    w0 = words()
    assert w0 == [(1, 0, None)] * 3
    assert b.set_subopts(b"a/+", 2, {"nl": 1}) and ref.set_subopts(b"a/+", 2, {"nl": 1})
    w1 = words()                                             # this commit wrote one image
    assert w1 == [(1, 0, None), None, (1, 0, None)]
    assert b.set_subopts(b"z", 9, {"qos": 2}) and ref.set_subopts(b"z", 9, {"qos": 2})
    assert words() == w1                                     # the other image got the word from the previous log
    assert e.sub_del(b"a/+", 2) == ref.do_unsubscribe(None, b"a/+", 2) == 2
    assert words() == [(1, 0, None)] * 2
    sub(b"a/+", 2, {"qos": 2, "rap": 1, "subid": 5})         # re-added last, with other options
    assert words() == [(1, 0, None), (1, 0, None), (2, 1, 5)]
    e.sub_add(b"a/+", 4)                                     # a 4th and 5th entry: the segment moves (cap 4 -> 8)
    ref.bag.insert_subscriber(None, b"a/+", 4)
    sub(b"a/+", 5, {"qos": 0, "rap": 1})
    assert e.debug_sub_pool_stats()[3] >= 3
    assert words() == [(1, 0, None), (1, 0, None), (2, 1, 5), (2, 1, None), (0, 1, None)]
    assert words() == [(1, 0, None), (1, 0, None), (2, 1, 5), (2, 1, None), (0, 1, None)]
    e.debug_check_subs()
    # the filter leaves the trie behind the broker's back and its id is reused
    e.delete(b"a/+")
    o.del_route(b"a/+", "n1")
    for _ in range(3):
        e.commit()
    for k in range(4):
        r.add_route(b"b%d/+" % k, "n1")
        o.add_route(b"b%d/+" % k, "n1")
        for s in (1, 2, 3):
            e.sub_add(b"b%d/+" % k, s)                       # no option entries
            ref.bag.insert_subscriber(None, b"b%d/+" % k, s)
    topics = [b"b%d/x" % k for k in range(4)]
    msgs = [(2, 1, 0, 2)] * 4
    _check(b, o, ref, topics, msgs, False, None)
    for pub in b.publish_many(topics, msgs):
        assert [p[2] for p in pub.pairs] == [(2, 1, None)] * 3        # the message as it is
    e.close()


def test_publish_opts_keeps_the_picks(gpu_device):
    """tm_match_publish_batch_opts: the keyed picks of tm_match_publish_batch, plus the words"""
    e = Engine(device=gpu_device)
    b = Broker(e, Router(e, node="n1"))
    for s in range(6):
        b.subscribe(b"s/+", 100 + s, "g1")
        b.subscribe(b"s/1", 200 + s, "g2")
    for s in range(70):
        b.subscribe(b"s/#", s, opts={"qos": s % 3, "nl": s % 2, "rap": 1, "subid": s + 1})
    topics = [b"s/1", b"s/2", b"s/1", b"q"]
    keys = [7, 11, 12, 3]
    msgs = [(2, 1, 0, 1), (1, 0, 0, None), (0, 1, 1, 2), (2, 0, 0, 1)]
    plain = b.publish_shared_many(topics, "hash", keys)
    got = b.publish_shared_many(topics, "hash", keys, msgs=msgs)
    words = b.publish_many(topics, msgs)
    for p, g, w in zip(plain, got, words):
        assert g.picks == p.picks and g.deliveries == p.deliveries
        assert [x[:2] for x in g.pairs] == p.pairs and g.pairs == w.pairs
    assert sum(len(g.picks) for g in got) == 5 and got[0].pairs[1][2] is None
    e.close()


def test_dispatch_many_with_msgs(gpu_device):
    """tm_dispatch_batch_opts, the receiving half of forward/3: entry i is (To
    i, message i), a To listed once per message"""
    e = Engine(device=gpu_device)
    b = Broker(e, Router(e, node="n1"))
    ref = SubOptionTable()
    k = 0
    for t, m, g in [(b"a/+", 130, None), (b"a/b", 3, None), (b"a/b", 2, "g1"), (b"s/#", 4, "g2")]:
        for _ in range(m):
            opts = None if k % 4 == 0 else {"qos": k % 3, "nl": 0, "rap": k % 2, "subid": k + 1}
            b.subscribe(t, k, g, opts)
            if opts is None:
                ref.bag.insert_subscriber(g, t, k)
            else:
                ref.do_subscribe(g, t, k, opts)
            k += 1
    tos = [b"a/+", b"a/b", b"nobody/home", b"s/#", b"a/+", b""]
    msgs = [(2, 1, 0, None), (1, 1, 1, None), (2, 0, 0, None), (0, 0, 0, None), (0, 0, 1, None), (1, 0, 0, None)]
    for upgrade in (False, True):
        got = b.dispatch_many(tos, msgs, upgrade_qos=upgrade)
        assert got == [dispatch_opts(ref, to, m, upgrade) for to, m in zip(tos, msgs)]
        assert [(c, [s for s, _ in subs]) for c, subs in got] == b.dispatch_many(tos)
    assert got[0][1] != got[4][1] and [s for s, _ in got[0][1]] == [s for s, _ in got[4][1]]
    assert unpack_deliver(Engine.DELIVER_DROP) is None
    e.close()
