"""publish/1's $share clause on the GPU (walk + routes + aggre + dispatch.hip +
share.hip) against tests/shared_ref.py (do_pick/5 over oracle/pytrie.py
RouteTable.match_deliveries): per delivery slot the picked member or
NO_MEMBER, compared element for element for both strategies, and every other
output compared with the dispatch call's."""
import contextlib
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import byte_corpus as C  # noqa: E402
from dispatch_ref import SubscriberBag, route_dispatch  # noqa: E402
from shared_ref import NO_MEMBER, SharedSub as RefShared, route_shared  # noqa: E402
from emqx_amd import Engine  # noqa: E402
from emqx_amd import _lib as L  # noqa: E402
from emqx_amd.emqx_broker import Broker  # noqa: E402
from emqx_amd.emqx_router import Router  # noqa: E402
from emqx_amd.engine import pack  # noqa: E402
from oracle import pytrie  # noqa: E402
from trie_churn import read_back  # noqa: E402

pytestmark = pytest.mark.gpu

DESTS = ["n1", "n2", ("g1", "n1"), ("g1", "n2"), ("g2", "n2"), "n3", ("a", "n3"), "g1"]
GROUPS = [b"g1", b"g2", b"a", b"g3"]
KEYS = [0, 1, 2 ** 27 - 1, 2 ** 32 - 1]


class World:
    """an engine with its Router / Broker and the three oracles, fed together"""

    def __init__(self, device):
        self.e = Engine(device=device)
        self.r, self.o = Router(self.e, node="n1"), pytrie.RouteTable()
        self.b = Broker(self.e, self.r)
        self.bag, self.sh = SubscriberBag(), RefShared()

    def route(self, topic, dest, add=True):
        (self.r.add_route if add else self.r.del_route)(topic, dest)
        (self.o.add_route if add else self.o.del_route)(topic, dest)

    def member(self, group, topic, m, add=True):
        if add:
            self.e.share_add(group, topic, m)
            self.sh.subscribe(group, topic, m)
        else:
            assert self.e.share_del(group, topic, m) == self.sh.unsubscribe(group, topic, m)

    def members(self, group, topic, ms):
        if not ms:
            return
        gb, go = pack([group] * len(ms))
        tb, to = pack([topic] * len(ms))
        self.e.share_add_many(gb, go, tb, to, ms)
        for m in ms:
            self.sh.subscribe(group, topic, m)

    def close(self):
        self.e.close()


def _want(w, topics, strategy, keys, stats=None):
    """the oracle's picks per topic: [(To, Group, member | None)] of the $share
    deliveries (round robin advances the oracle's cursors).  stats: counts the
    picks by the set's size class"""
    out = []
    for i, tp in enumerate(topics):
        dels = w.o.match_deliveries(tp)
        picks = route_shared(w.o, w.sh, strategy, None if keys is None else int(keys[i]), tp)
        row = []
        for (to, (kind, x)), m in zip(dels, picks):
            if kind == 1:
                row.append((to, x, m))
                if stats is not None:
                    c = len(w.sh.subscribers(x, to))
                    stats[min(c, 2)] = stats.get(min(c, 2), 0) + 1
        out.append(row)
    return out


def _compare(w, topics, strategy, keys, want, tag=None):
    """publish_shared_many against the oracle's picks and against publish_many"""
    got = w.b.publish_shared_many(topics, strategy, keys)
    plain = w.b.publish_many(topics)
    for tp, pub, pl, wp in zip(topics, got, plain, want):
        assert pub.deliveries == pl.deliveries and pub.pairs == pl.pairs, (tag, tp)
        assert pub.picks == wp, (tag, strategy, tp)


def _both(w, topics, rng, tag=None, floor=None):
    """one check round: the keyed picks (stateless), then round robin.  floor
    = (picks from sets of >= 2 members, `false` picks, picks from sets of one)
    the oracle alone must reach before anything is compared"""
    keys = [rng.choice(KEYS + [rng.randrange(2 ** 32)]) for _ in topics]
    stats = {}
    want_k = _want(w, topics, "keyed", keys, stats)
    if floor is not None:
        assert stats.get(2, 0) >= floor[0] and stats.get(0, 0) >= floor[1] and stats.get(1, 0) >= floor[2], stats
    _compare(w, topics, "keyed", keys, want_k, tag)
    _compare(w, topics, "round_robin", None, _want(w, topics, "round_robin", None), tag)
    return stats


# ---- random operations --------------------------------------------------------------------

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


def _random_ops(w, rng, pool, hot, steps, check):
    for step in range(steps):
        x = rng.random()
        t = rng.choice(hot) if rng.random() < 0.5 else rng.choice(pool)
        if x < 0.35:
            w.route(t, rng.choice(DESTS), rng.random() < 0.75)
        elif x < 0.55:
            s = rng.randrange(40)
            g = rng.choice(["g1", "g2", "g3"]) if rng.random() < 1 / 3 else None
            if rng.random() < 0.7:
                w.e.sub_add(t, s, g.encode() if g else None)
                w.bag.insert_subscriber(g, t, s)
            else:
                assert w.e.sub_del(t, s, g.encode() if g else None) == w.bag.delete_object(g, t, s)
        elif x < 0.97:
            w.member(rng.choice(GROUPS[:3]), t, rng.randrange(12), rng.random() < 0.62)
        else:
            m = rng.randrange(12)
            assert w.e.share_member_down(m) == w.sh.cleanup_down(m)
        if step % 150 == 149:
            check(step)


@pytest.mark.parametrize("layout", [None, 2])
def test_shared_random_ops_vs_oracle(gpu_device, layout):
    rng = random.Random(41)
    w = World(gpu_device)
    if layout:
        w.e.set_option("layout", layout)
    pool = _pool(rng, 60)
    hot = [f for f in pool if f.endswith(b"#") or f.startswith(b"+")][:8] + pool[:6]
    for i, f in enumerate(hot[:8]):                          # so that every round has busy sets from its start
        w.route(f, (("g1", "g2")[i % 2], "n1"))
        w.members((b"g1", b"g2")[i % 2], f, [20 + i, 21 + i, 22 + i])
    rounds = []

    def check(step):
        rounds.append(_both(w, _topics(rng, 300) + pool, rng, (layout, step), floor=(200, 1, 1)))
    _random_ops(w, rng, pool, hot, 600, check)
    assert len(rounds) == 4
    w.close()


# ---- set sizes and keys ---------------------------------------------------------------------

def test_shared_set_sizes_and_keys(gpu_device):
    """sets of 0 / 1 / 2 / 3 / 63 / 64 / 65 / 257 members on '#', 'a/#', 'a/+'
    and the exact topic 'a/b' (a non-wildcard $share), three groups on one
    filter beside a local and a remote delivery, a $SYS topic; keys 0, 1,
    Count - 1, Count, 2^27 - 1, 2^32 - 1"""
    sizes = [0, 1, 2, 3, 63, 64, 65, 257]
    where = [b"#", b"a/#", b"a/+", b"a/b"]
    topics = [b"a/b", b"a/c", b"x/b", b"a", b"$SYS/b", b"q", b"a/b"]
    seen = {}
    for rnd in range(4):
        w = World(gpu_device)
        ids = list(range(3000))
        random.Random(rnd).shuffle(ids)
        counts = set()
        for i, f in enumerate(where):
            n = sizes[(2 * i + rnd) % 8]
            w.route(f, ("g1", "n1"))
            w.members(b"g1", f, [ids.pop() for _ in range(n)])
            counts.add(n)
        for g, n in ((b"g2", 3), (b"g3", 64)):                 # three groups on a/#, beside n1 and n2
            w.route(b"a/#", (g.decode(), "n2"))
            w.members(g, b"a/#", [ids.pop() for _ in range(n)])
            counts.add(n)
        for d in ("n1", "n2"):
            w.route(b"a/#", d)
        w.e.sub_add(b"a/#", 7)
        w.bag.insert_subscriber(None, b"a/#", 7)
        w.route(b"$SYS/#", ("g1", "n1"))
        w.members(b"g1", b"$SYS/#", [ids.pop() for _ in range(5)])
        w.route(b"q", ("g9", "n1"))                              # a group without any member: `false`
        w.members(b"g1", b"x/y", [1, 2])                         # members without a route: never a delivery
        for c in sorted(counts | {5}):
            for key in {0, 1, max(c - 1, 0), c, 2 ** 27 - 1, 2 ** 32 - 1}:
                keys = [key] * len(topics)
                st = {}
                _compare(w, topics, "keyed", keys, _want(w, topics, "keyed", keys, st), (rnd, c, key))
                for k, v in st.items():
                    seen[k] = seen.get(k, 0) + v
        _compare(w, topics, "round_robin", None, _want(w, topics, "round_robin", None), rnd)
        _compare(w, topics, "round_robin", None, _want(w, topics, "round_robin", None), rnd)
        pub = dict(zip(topics, w.b.publish_shared_many(topics, "keyed", [1] * len(topics))))
        ab = pub[b"a/b"]
        assert [g for to, g, _ in ab.picks if to == b"a/#"] == [b"g1", b"g2", b"g3"]
        assert {d.target for d in ab.deliveries if d.to == b"a/#"} >= {(0, b"n1"), (0, b"n2")}
        assert (b"q", b"g9", None) in pub[b"q"].picks
        assert [to for to, _, m in pub[b"$SYS/b"].picks if m is not None] == [b"$SYS/#"]
        w.close()
    assert seen.get(0, 0) > 0 and seen.get(1, 0) > 0 and seen.get(2, 0) > 0, seen


# ---- round robin ------------------------------------------------------------------------------

def _rr_world(device, filler):
    """a hot set of 5 on hot/#, a second of 3 on hot2/+, 120 sets of 2 on exact
    topics; after `filler` dummy sets, so the set indices need three radix
    passes when filler >= 65,536"""
    w = World(device)
    if filler:
        gb, go = pack([b"d"] * filler)
        tb, to = pack([b"d/%d" % i for i in range(filler)])
        w.e.share_add_many(gb, go, tb, to, list(range(filler)))
        for i in range(filler):
            w.sh.subscribe(b"d", b"d/%d" % i, i)
    w.route(b"hot/#", ("g", "n1"))
    w.members(b"g", b"hot/#", [11, 12, 13, 14, 15])
    w.route(b"hot2/+", ("h", "n2"))
    w.members(b"h", b"hot2/+", [21, 22, 23])
    for i in range(120):
        w.route(b"one/%d" % i, ("s", "n1"))
        w.members(b"s", b"one/%d" % i, [1000 + 2 * i, 1001 + 2 * i])
    return w


def _rr_batch(k, every, singles):
    """k publishes of the hot set, one of the second hot set after every
    `every`-th, and `singles` sets seen once spread between them"""
    ts = []
    step = max(1, k // max(singles, 1))
    s = 0
    for j in range(k):
        ts.append(b"hot/%d" % (j % 7))
        if j % every == every - 1:
            ts.append(b"hot2/x")
        if j % step == 0 and s < singles:
            ts.append(b"one/%d" % s)
            s += 1
    return ts


def _picks_raw(e, topics, strategy=Engine.SHARE_ROUND_ROBIN, keys=None):
    buf, off = pack(topics)
    out = e.match_publish_batch(buf, off, strategy, keys)
    counts, offs, pick = out[0], out[1], out[9]
    return [[int(pick[j]) for j in range(int(offs[t]), int(offs[t]) + int(counts[t]))] for t in range(len(topics))]


def test_shared_round_robin_runs_across_wave_block_and_tile_edges(gpu_device):
    """one batch in which a set occurs k times, k = 1, 2, Count - 1, Count,
    Count + 1 and 4,097 (past one 4,096-key sort tile), interleaved with a
    second hot set and sets seen once: equal to the oracle and to the same
    publishes sent one per batch to a second engine"""
    w, w2 = _rr_world(gpu_device, 70000), _rr_world(gpu_device, 70000)
    for k, every, singles in ((1, 1, 3), (2, 1, 5), (4, 2, 9), (5, 2, 9), (6, 3, 9), (4097, 16, 64)):
        ts = _rr_batch(k, every, singles)
        want = _want(w, ts, "round_robin", None)
        got = _picks_raw(w.e, ts)
        flat = [[NO_MEMBER if m == Engine.NO_MEMBER else m for m in row] for row in got]
        assert flat == [[m for _, _, m in row] for row in want], k
        one = []
        for t in ts:                                        # the same publishes, one per batch
            tb, to = pack([t])
            o = w2.e.match_publish_batch(tb, to, Engine.SHARE_ROUND_ROBIN, None, out_cap=8, sub_cap=8)
            one.append([int(x) for x in o[9][: int(o[0][0])]])
        assert one == got, k
    w.close()
    w2.close()


def test_shared_round_robin_cursor_across_batches_and_commits(gpu_device):
    w = World(gpu_device)
    w.route(b"t/#", ("g", "n1"))
    w.route(b"u", ("g", "n1"))
    w.members(b"g", b"u", [71, 72])
    ts = [b"t/1", b"u", b"t/2"]

    def rr(tag):
        _compare(w, ts, "round_robin", None, _want(w, ts, "round_robin", None), tag)
    w.member(b"g", b"t/#", 1)
    rr("one member")                                       # Count = 1: the cursor stays undefined
    rr("one member again")
    w.member(b"g", b"t/#", 2)
    w.member(b"g", b"t/#", 3)
    rr("grown 1 -> 3")                                     # first use: members 1, 2
    assert w.sh.pd[("shared_sub_round_robin", b"g", b"t/#")] == 1
    rr("carried")                                          # 3, 1
    rr("carried")                                          # 2, 3: stored Rem = 2
    assert w.sh.pd[("shared_sub_round_robin", b"g", b"t/#")] == 2
    w.member(b"g", b"t/#", 3, add=False)
    rr("shrunk below the stored value")                    # (2 + 1) rem 2 = 1
    for m in (1, 2):
        w.member(b"g", b"t/#", m, add=False)
    rr("emptied")                                          # `false`
    for _ in range(3):                                     # the index may be recycled meanwhile
        w.e.commit()
    w.members(b"g", b"t/#", [5, 6, 7])
    w.route(b"v/+", ("g", "n1"))
    w.members(b"g", b"v/+", [8, 9])                        # a new set, free to take the old index
    ts.append(b"v/1")
    rr("refilled: reset")
    assert w.sh.pd[("shared_sub_round_robin", b"g", b"t/#")] == 1
    rr("after the reset")
    w.close()


# ---- capacity -----------------------------------------------------------------------------------

def test_shared_host_enospc_leaves_the_cursors(gpu_device):
    w = _rr_world(gpu_device, 0)
    ts = _rr_batch(9, 2, 6)
    total = sum(len(w.o.match_routes(t)) for t in ts)
    buf, off = pack(ts)
    for cap, scap in ((total - 1, 16), (0, 16)):
        with pytest.raises(L.TopicMatchError) as ei:
            w.e.match_publish_batch(buf, off, Engine.SHARE_ROUND_ROBIN, None, out_cap=cap, sub_cap=scap)
        assert ei.value.code == L.TM_ENOSPC and ei.value.needed == total
    _compare(w, ts, "round_robin", None, _want(w, ts, "round_robin", None), "retry")
    w.close()


def _dev(x, dev, dtype=None):
    import torch
    a = np.ascontiguousarray(x)
    return torch.from_numpy(a.view(dtype).copy() if dtype else a.copy()).to(torch.device("cuda", dev))


def _full(n, dev, dtype, fill=-1):
    import torch
    return torch.full((max(n, 1),), fill, dtype=dtype, device=torch.device("cuda", dev))


def _device_publish(e, dev, buf, off, strategy, keys, cap, scap):
    """tm_match_publish_batch_device -> (counts, offsets, to, target, ndisp, pick, total) on the host"""
    import torch
    n = len(off) - 1
    d_b, d_o = _dev(buf, dev), _dev(off, dev, np.int64)
    c, o, tot = _full(n, dev, torch.int32), _full(n + 1, dev, torch.int64), _full(1, dev, torch.int64)
    to, tg, nd, pk = (_full(cap, dev, torch.int32, -7) for _ in range(4))
    sc, so, stot = _full(n, dev, torch.int32), _full(n + 1, dev, torch.int64), _full(1, dev, torch.int64)
    sto, sid = _full(scap, dev, torch.int32), _full(scap, dev, torch.int32)
    d_k = None if keys is None else _dev(np.asarray(keys, dtype=np.uint32), dev, np.int32)
    torch.cuda.synchronize()
    e.match_publish_batch_device(d_b, d_o, n, int(off[-1] - off[0]), c, o, to, tg, nd, cap, tot, sc, so, sto, sid,
                                 scap, stot, strategy, d_k, pk)
    torch.cuda.synchronize()
    u = lambda t: t.cpu().numpy().view(np.uint32)   # noqa: E731
    return u(c), o.cpu().numpy(), u(to), u(tg), u(nd), u(pk), int(tot.item())


def test_shared_device_small_out_cap_drops_slots_without_a_cursor_value(gpu_device):
    """deliveries at or past out_cap are dropped and take no cursor value: the
    later publishes continue where the oracle, fed only the kept slots, stands"""
    w = _rr_world(gpu_device, 0)
    ts = _rr_batch(12, 2, 8)
    total = sum(len(w.o.match_routes(t)) for t in ts)
    cap = total - 7
    buf, off = pack(ts)
    c, o, to, tg, nd, pk, tot = _device_publish(w.e, gpu_device, buf, off, Engine.SHARE_ROUND_ROBIN, None, cap, 64)
    assert tot == total
    kept = 0
    for t, tp in enumerate(ts):                              # the oracle, slot by slot
        for j, (dto, (kind, x)) in enumerate(w.o.match_deliveries(tp)):
            slot = int(o[t]) + j
            if slot >= cap:
                continue
            m = w.sh.do_pick("round_robin", None, x, dto) if kind == 1 else NO_MEMBER
            assert int(pk[slot]) == (Engine.NO_MEMBER if m is NO_MEMBER else m), (tp, slot)
            kept += 1
    assert 0 < kept < sum(len(w.o.match_deliveries(t)) for t in ts)
    _compare(w, ts, "round_robin", None, _want(w, ts, "round_robin", None), "after the cut batch")
    w.close()


# ---- topic bytes ---------------------------------------------------------------------------------

@contextlib.contextmanager
def _deep():
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 3 * C.DEEP_LEVELS + 1000))
    try:
        yield
    finally:
        sys.setrecursionlimit(old)


class _ByteWorld:
    """a $share route on every topic of the stratified subset, members on
    every second one (so of a trailing-NUL sibling pair one side has a set and
    the other must miss); the oracle's picks computed once"""

    def __init__(self, device):
        # publish topics only: a level '+' or '#' would make the topic a trie filter, not an exact-topic set
        self.topics = [t for t in C.stratified() if not pytrie.wildcard(t)]
        assert 1000 < len(self.topics) <= 1500
        nul = set(C.sections()["nul"])
        assert {t for t in nul if not pytrie.wildcard(t)} <= set(self.topics)   # every trailing-NUL sibling
        self.w = w = World(device)
        m = 0
        for i, t in enumerate(self.topics):
            w.route(t, ("g1", "n1"))
            if i % 2 == 0:
                k = 1 + i % 3
                w.members(b"g1", t, list(range(m, m + k)))
                m += k
        rng = random.Random(C.SEED + 9)
        self.keys = [rng.randrange(2 ** 32) for _ in self.topics]
        w.e.commit()
        with _deep():
            self.dels = [w.o.match_deliveries(t) for t in self.topics]
            st = {}
            self.want_keyed = _want(w, self.topics, "keyed", self.keys, st)
        assert st.get(0, 0) > 100 and st.get(1, 0) > 100 and st.get(2, 0) > 100, st
        hit = [t for i, t in enumerate(self.topics) if i % 2 == 0 and t + b"\0" in nul and
               self.topics.index(t + b"\0") % 2 == 1]
        assert hit                                           # w has a set, w + NUL has none


@pytest.fixture(scope="module")
def byte_world(gpu_device):
    bw = _ByteWorld(gpu_device)
    yield bw
    bw.w.close()


@pytest.mark.parametrize("lead", [0, 5])
def test_shared_exact_topic_sets_over_the_byte_corpus(byte_world, gpu_device, lead):
    """exact-topic sets found through the share image's own exact table by the
    bytes at d_topic_off as given, in both envelopes"""
    bw, w = byte_world, byte_world.w
    ts = bw.topics
    with _deep():
        slots = sum(len(w.o.match_routes(t)) for t in ts)
        want_rr = _want(w, ts, "round_robin", None)
    buf, off = C.envelope(ts, lead)
    for strategy, keys, want in ((Engine.SHARE_KEYED, bw.keys, bw.want_keyed),
                                 (Engine.SHARE_ROUND_ROBIN, None, want_rr)):
        c, o, to, tg, nd, pk, tot = _device_publish(w.e, gpu_device, buf, off, strategy, keys, slots + 5, 64)
        assert tot == slots and list(pk[slots:].view(np.int32)) == [-7] * 5
        for t, tp in enumerate(ts):
            a = int(o[t])
            got = [int(pk[a + j]) for j, (_, (kind, _x)) in enumerate(bw.dels[t]) if kind == 1]
            exp = [Engine.NO_MEMBER if m is NO_MEMBER else m for _, _, m in want[t]]
            assert int(c[t]) == len(bw.dels[t]) and got == exp, (strategy, t, tp[:60])


# ---- edges -------------------------------------------------------------------------------------

def test_shared_edges_empty_batch_and_no_share_record(gpu_device):
    w = World(gpu_device)
    for f, d in ((b"a/#", "n1"), (b"a/+", ("g1", "n1")), (b"a/b", ("g2", "n2")), (b"#", "n2")):
        w.route(f, d)
    w.e.sub_add(b"a/#", 3)
    w.bag.insert_subscriber(None, b"a/#", 3)
    buf, off = pack([])
    for strategy, keys in ((Engine.SHARE_KEYED, np.zeros(0, dtype=np.uint32)), (Engine.SHARE_ROUND_ROBIN, None)):
        out = w.e.match_publish_batch(buf, off, strategy, keys)
        assert len(out[0]) == 0 and list(out[1]) == [0] and len(out[9]) == 0
    assert w.e.share_count == 0
    ts = [b"a/b", b"a", b"x", b"a/b/c"]
    buf, off = pack(ts)
    base = w.e.match_dispatch_batch(buf, off)
    for strategy, keys in ((Engine.SHARE_KEYED, [5] * len(ts)), (Engine.SHARE_ROUND_ROBIN, None)):
        out = w.e.match_publish_batch(buf, off, strategy, keys)
        for a, b in zip(base, out[:9]):
            assert np.array_equal(a, b)
        assert len(out[9]) == len(out[2]) > 0 and set(out[9].tolist()) == {Engine.NO_MEMBER}
    _both(w, ts, random.Random(1))
    w.close()


def test_shared_filter_id_reuse_on_the_device(gpu_device):
    """the id of a deleted filter, reused for another, finds no members"""
    w = World(gpu_device)
    w.route(b"a/+", ("g", "n1"))
    w.members(b"g", b"a/+", [1, 2])
    _both(w, [b"a/x"], random.Random(2))
    w.route(b"a/+", ("g", "n1"), add=False)                  # the trie filter goes, the members stay
    for _ in range(3):
        w.e.commit()
    w.route(b"b/#", ("g", "n1"))                             # takes the freed id
    _both(w, [b"a/x", b"b/x"], random.Random(3))
    got = w.b.publish_shared_many([b"b/x"], "round_robin")[0]
    assert got.picks == [(b"b/#", b"g", None)]
    w.route(b"a/+", ("g", "n1"))
    _both(w, [b"a/x", b"b/x"], random.Random(4))
    w.close()


# ---- every mirrored table through both image epochs ---------------------------------------------

def test_one_small_delta_per_commit_reaches_both_image_epochs(gpu_device):
    """double_buffer 1: eight consecutive commits, each after exactly one small
    delta -- a route, a plain subscriber, a share member, a trie filter deleted
    and re-inserted behind the tables (a new filter id: nodes, edges, fr_meta,
    fs_meta and fx all move), twice over.  Each commit writes the image epoch
    that missed the previous commit, from that commit's dirty log and this
    one's (a few elements of tables of dozens: the scatter path), so a host
    table left out of the commit's upload or rotation shows as a stale
    delivery, Count, pair or pick.  After every commit a 64-topic publish
    equals the oracle's."""
    rng = random.Random(9)
    w = World(gpu_device)
    w.e.set_option("double_buffer", 1)
    wild = [b"a/+", b"a/#", b"+/b", b"#", b"c/+/d", b"c/#", b"+/+", b"d/+", b"a/b/#", b"+/c/+", b"e/#", b"e/+"]
    exact = [b"t/%d" % i for i in range(20)] + [b"a/b", b"c/x/d", b"e/f", b"d"]
    for i, f in enumerate(wild + exact):
        w.route(f, "n1")
        w.e.sub_add(f, 100 + i)
        w.bag.insert_subscriber(None, f, 100 + i)
        if i % 2 == 0:
            g = (b"g1", b"g2")[i // 2 % 2]
            w.route(f, (g.decode(), "n1"))
            w.members(g, f, [300 + 3 * i, 301 + 3 * i, 302 + 3 * i][:1 + i % 3])
    topics = (exact + [b"a/c", b"x/b", b"c/y/d", b"c/z", b"q/r", b"d/e", b"a/b/c", b"z/c/z", b"e/g", b"e", b"q"] +
              _topics(rng, 64))[:64]
    assert len(topics) == 64

    seen = {}

    def check(tag):
        read_back(w.e, seen)     # the commit, and the live image read back against the host tables
        for tp, pub in zip(topics, w.b.publish_many(topics)):
            counts, pairs = route_dispatch(w.o, w.bag, b"n1", tp)
            assert [(d.to, d.target) for d in pub.deliveries] == w.o.match_deliveries(tp), (tag, tp)
            assert [d.count for d in pub.deliveries] == counts, (tag, tp)
            assert pub.pairs == pairs, (tag, tp)
        stats = _both(w, topics, rng, tag)
        assert stats.get(2, 0) > 0 and stats.get(1, 0) > 0, stats

    check("built")
    check("second epoch")
    for k in range(2):
        w.route(wild[k], "n2")                                   # one route
        check(("route", k))
        w.e.sub_add(exact[k], 900 + k)                           # one plain subscriber
        w.bag.insert_subscriber(None, exact[k], 900 + k)
        check(("subscriber", k))
        w.member((b"g1", b"g2")[k], wild[2 * k], 500 + k)        # one share member
        check(("member", k))
        w.e.delete(wild[4 + k])                                  # one trie filter, behind the tables
        w.e.insert(wild[4 + k])
        check(("filter", k))
    # Tables of dozens mostly copy whole (a scatter has to stay within a quarter of the table's bytes), so:
    # one large burst -- 150 more topics, half of them wildcard filters, each with a route, a subscriber
    # and a member -- then two bursts of ten ops.  The second small commit's two logs are both small: the
    # set and topic tables, the member pool and fx take the scatter path.
    big = [b"u/%d/+" % i if i % 2 else b"u/%d" % i for i in range(150)]
    for i, f in enumerate(big):
        w.route(f, ("g1", "n1"))
        w.members(b"g1", f, [2000 + i])
        w.e.sub_add(f, 3000 + i)
        w.bag.insert_subscriber(None, f, 3000 + i)
    check("large burst")
    seen.clear()
    for k in range(2):
        w.route(wild[6 + k], "n3")
        w.e.sub_add(exact[5 + k], 950 + k)
        w.bag.insert_subscriber(None, exact[5 + k], 950 + k)
        w.member(b"g1", big[k], 2500 + k)                        # a second member of a set
        w.route(b"v/%d" % k, ("g2", "n1"))                       # a new exact topic with a set
        w.member(b"g2", b"v/%d" % k, 2600 + k)
        w.e.delete(wild[8 + 2 * k])                              # a filter with a set, behind the tables
        w.e.insert(wild[8 + 2 * k])
        check(("small burst", k))
    for t in ("sh_sets", "sh_tx", "sh_pool", "sh_fx", "fs_meta", "fr_meta"):
        assert 2 in seen[t], (t, seen[t])
    w.e.debug_check_routes()
    w.e.debug_check_subs()
    w.e.debug_check_shares()
    w.close()
