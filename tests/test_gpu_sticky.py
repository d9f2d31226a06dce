"""TM_SHARE_STICKY and tm_share_pick_batch on the GPU against tests/sticky_ref.py
(pick/5 of src/emqx_shared_sub.erl:211-249 with is_active_sub/2), list for
list: random table operations, runs across wave / block / sort-tile edges, the
quirks of the clause, the state across commits and contexts, overflow of the
host, device and stream-ordered calls, the batcher's lanes, and the retry
picks of all three strategies."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from sticky_ref import StickySub, route_pick  # noqa: E402
from test_gpu_shared import KEYS, World, _device_publish, _picks_raw, _pool, _random_ops, _topics  # noqa: E402
from test_gpu_publish_stream import Stream, _publish_one, _reference, _same  # noqa: E402
from emqx_amd import Engine  # noqa: E402
from emqx_amd import _lib as L  # noqa: E402
from emqx_amd.emqx_shared_sub import SharedSub  # noqa: E402
from emqx_amd.engine import pack  # noqa: E402

pytestmark = pytest.mark.gpu

STICKY = Engine.SHARE_STICKY
ROOMY = (50_000, 50_000, 50_000, 20_000)


class SWorld(World):
    def __init__(self, device):
        super().__init__(device)
        self.sh = StickySub()

    def down(self, m):
        assert self.e.share_member_down(m) == self.sh.cleanup_down(m)


class Pd:
    """one more publisher process over a world's member table and live set"""

    def __init__(self, w):
        self.sh = StickySub()
        self.sh.tab, self.sh.alive = w.sh.tab, w.sh.alive

    def cleanup_down(self, m):
        """the world's cleanup_down has run: this dictionary's share of it"""
        for k in [k for k, v in self.sh.pd.items() if k[0] == "shared_sub_sticky" and v == m]:
            del self.sh.pd[k]


def _want(w, topics, keys, sh=None):
    """per topic [(To, Group, member | None)] of its $share deliveries"""
    out = []
    for tp, key in zip(topics, keys):
        dels = w.o.match_deliveries(tp)
        picks = route_pick(w.o, sh or w.sh, "sticky", int(key), tp)
        out.append([(to, x, m) for (to, (kind, x)), m in zip(dels, picks) if kind == 1])
    return out


def _check(w, topics, keys, tag=None):
    want = _want(w, topics, keys)
    got = w.b.publish_shared_many(topics, "sticky", keys)
    for tp, pub, wp in zip(topics, got, want):
        assert pub.picks == wp, (tag, tp)
    return want


def _keys(rng, n):
    return [rng.choice(KEYS + [rng.randrange(2 ** 32)]) for _ in range(n)]


# ---- random operations --------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", [None, 2])
def test_sticky_random_ops_vs_oracle(gpu_device, layout):
    rng = random.Random(43)
    w = SWorld(gpu_device)
    if layout:
        w.e.set_option("layout", layout)
    pool = _pool(rng, 40)
    hot = [f for f in pool if f.endswith(b"#") or f.startswith(b"+")][:8] + pool[:6]
    for i, f in enumerate(hot[:8]):
        w.route(f, (("g1", "g2")[i % 2], "n1"))
        w.members((b"g1", b"g2")[i % 2], f, [i % 12, (i + 1) % 12, (i + 5) % 12])
    picked = strangers = 0
    for rnd in range(16):                                     # 400 steps, a batch (and its commit) after every 25
        _random_ops(w, rng, pool, hot, 25, None)
        if rnd % 2:
            w.down(rng.randrange(12))
        topics = _topics(rng, 90) + rng.sample(pool, 20)
        want = _check(w, topics, _keys(rng, len(topics)), (layout, rnd))
        for row in want:
            for to, g, m in row:
                picked += m is not None
                strangers += m is not None and m not in w.sh.subscribers(g, to)
    assert picked >= 2000 and strangers >= 20, (picked, strangers)     # stuck members that had unsubscribed
    w.close()


# ---- runs ---------------------------------------------------------------------------------------------------

def _run_world(device):
    w = SWorld(device)
    w.route(b"hot/#", ("g", "n1"))
    w.members(b"g", b"hot/#", [11, 12, 13, 14, 15])
    w.route(b"hot2/+", ("h", "n2"))
    w.members(b"h", b"hot2/+", [21, 22, 23])
    w.route(b"one/+", ("s", "n1"))
    w.members(b"s", b"one/+", [31, 32])
    return w


def _run_batch(k):
    ts = []
    for j in range(k):
        ts.append(b"hot/%d" % (j % 7))
        if j % 7 == 3:
            ts.append(b"hot2/x")
        if j % 11 == 5:
            ts.append(b"one/1")
    return ts


@pytest.mark.parametrize("k", [300, 4200])
def test_sticky_runs_across_wave_block_and_tile_edges(gpu_device, k):
    """k publishes reach one set whose entry is undefined, between publishes to
    two other sets: in sorted order its run crosses the wave (64), block (256)
    and, for k = 4200, sort-tile (4096) edges and the other runs start inside
    a wave.  Every pick of a run is the keyed pick of the run's first publish."""
    w = _run_world(gpu_device)
    ts = _run_batch(k)
    keys = [(i * 2654435761 + 3) % 2 ** 32 for i in range(len(ts))]
    first = {p: keys[next(i for i, t in enumerate(ts) if t.startswith(p))] for p in (b"hot/", b"hot2/", b"one/")}
    member = {b"hot/": 11 + first[b"hot/"] % 5, b"hot2/": 21 + first[b"hot2/"] % 3, b"one/": 31 + first[b"one/"] % 2}
    want = [[member[t[:t.index(b"/") + 1]]] for t in ts]
    assert _picks_raw(w.e, ts, STICKY, keys) == want
    assert [[m for _, _, m in row] for row in _want(w, ts, keys)] == want
    keys2 = [(x * 7 + 1) % 2 ** 32 for x in keys]             # other keys: the entries are defined, no key is used
    assert member[b"hot/"] != 11 + keys2[0] % 5
    assert _picks_raw(w.e, ts, STICKY, keys2) == want
    w.close()


# ---- the quirks of the clause -------------------------------------------------------------------------------

def test_sticky_quirks(gpu_device):
    w = SWorld(gpu_device)
    for f, g in ((b"a/#", "g"), (b"b", "g"), (b"c/+", "g"), (b"d", "g")):
        w.route(f, (g, "n1"))
    pub = lambda tp, key: [m for _, _, m in _check(w, [tp], [key], tp)[0]]   # noqa: E731
    # (a) the stuck member unsubscribes from a two-member set and is still picked
    w.members(b"g", b"a/#", [1, 2])
    assert pub(b"a/x", 1) == [2]
    w.member(b"g", b"a/#", 2, add=False)
    assert pub(b"a/y", 0) == [2] and w.e.share_members(b"g", b"a/#") == [1]
    # (b) down: the next publish picks again with its own key
    w.members(b"g", b"a/#", [3])                              # [1, 3]
    w.down(2)                                                 # no record left (removed = 0): reported all the same
    assert pub(b"a/z", 1) == [3]
    w.down(3)
    assert pub(b"a/z", 5) == [1]                              # [1] -> 1
    # (c) a one-member set sticks, grows to three, and still returns the first
    w.members(b"g", b"b", [7])
    assert pub(b"b", 9) == [7]
    w.members(b"g", b"b", [8, 9])
    assert pub(b"b", 1) == [7] and pub(b"b", 2) == [7]
    # (d) a set emptied and re-created starts undefined
    w.members(b"g", b"c/+", [4, 5, 6])
    assert pub(b"c/1", 2) == [6]
    for m in (4, 5, 6):
        w.member(b"g", b"c/+", m, add=False)
    assert pub(b"c/1", 0) == [None]
    for _ in range(3):
        w.e.commit()
    w.members(b"g", b"c/+", [4, 5, 6])
    w.members(b"g", b"d", [41, 42])                           # a new set, free to take the old index
    assert pub(b"c/1", 1) == [5] and pub(b"d", 0) == [41]     # 6 is alive, but nothing remembers it
    # a u32 that comes back after its down is a new process
    w.down(5)
    w.members(b"g", b"c/+", [5])                              # [4, 6, 5]
    assert pub(b"c/2", 3) == [4]
    w.close()


def test_sticky_state_survives_growth_and_relayout(gpu_device):
    w = SWorld(gpu_device)
    w.route(b"a/#", ("g", "n1"))
    w.route(b"x", ("g", "n1"))
    w.members(b"g", b"a/#", [1, 2, 3, 4])
    w.members(b"g", b"x", [11, 12, 13])
    ts, keys = [b"a/1", b"x"], [2, 1]
    assert [r[0][2] for r in _check(w, ts, keys)] == [3, 12]
    k = 3000                                                  # past the arrays' first capacity: they grow, contents kept
    gb, go = pack([b"f"] * k)
    tb, to = pack([b"f/%d" % i for i in range(k)])
    w.e.share_add_many(gb, go, tb, to, list(range(100, 100 + k)))
    for i in range(k):
        w.sh.subscribe(b"f", b"f/%d" % i, 100 + i)
    w.e.commit()
    assert [r[0][2] for r in _check(w, ts, [0, 0])] == [3, 12]
    w.e.set_option("layout", 2)                               # every commit from here on lays the image out again
    w.route(b"a/+/c", "n2")
    w.e.commit()
    w.route(b"f/7", ("f", "n1"))
    assert [r[0][2] for r in _check(w, ts + [b"f/7"], [1, 2, 5])] == [3, 12, 107]
    w.close()


# ---- contexts -----------------------------------------------------------------------------------------------

def _stream_picks(w, dev, topics, keys, ctx, caps=(64, 64, 64, 64)):
    s = Stream(w, dev, topics, keys, STICKY, caps, ctx)
    assert s.state == 0
    return [int(x) for x in s.d[:, 3]], s


def test_sticky_contexts_are_independent(gpu_device):
    w = _run_world(gpu_device)
    w.e.commit()
    c1, c2 = w.e.share_cursors(0), w.e.share_cursors(0)
    ts = [b"hot/1", b"one/1"]
    for ctx, key, want in ((c1, 0, [11, 31]), (c2, 1, [12, 32]), (None, 7, [13, 32])):
        assert _stream_picks(w, gpu_device, ts, [key, key], ctx)[0] == want
    for ctx, want in ((None, [13, 32]), (c2, [12, 32]), (c1, [11, 31])):     # other keys: each keeps its own
        got, s = _stream_picks(w, gpu_device, ts, [3, 4], ctx)
        assert got == want and s.h[5] == 0
    assert _picks_raw(w.e, ts, STICKY, [9, 9]) == [[13], [32]]               # the host call reads the built-in array
    w.down(12)                                                               # c2's member on hot/#: only c2 picks again
    w.e.commit()
    for ctx, want in ((c1, [11, 31]), (None, [13, 32]), (c2, [14, 32])):     # [11, 13, 14, 15], key 2 -> 14
        got, s = _stream_picks(w, gpu_device, ts, [2, 2], ctx)
        assert got == want and s.h[5] == (1 if ctx is c2 else 0)
    other = World(gpu_device)
    foreign = other.e.share_cursors(0)
    with pytest.raises(L.TopicMatchError) as ei:                             # a context of another engine
        SharedSub(w.e, "sticky").pick("g", b"hot/#", 1, [], cursors=foreign)
    assert ei.value.code == L.TM_EINVAL
    foreign.close()
    other.close()
    c1.close()
    c2.close()
    w.close()


# ---- capacities ---------------------------------------------------------------------------------------------

def test_sticky_host_enospc_changes_nothing(gpu_device):
    w = _run_world(gpu_device)
    ts = [b"hot/1", b"hot2/x", b"hot/2", b"one/1"]
    buf, off = pack(ts)
    for cap, scap in ((3, 16), (0, 16)):
        with pytest.raises(L.TopicMatchError) as ei:
            w.e.match_publish_batch(buf, off, STICKY, [1, 1, 1, 1], out_cap=cap, sub_cap=scap)
        assert ei.value.code == L.TM_ENOSPC and ei.value.needed == 4
    assert [r[0][2] for r in _check(w, ts, [3, 2, 0, 0])] == [14, 23, 14, 31]   # as a first call: its own keys
    w.close()


def test_sticky_device_small_out_cap_lets_no_dropped_slot_pick(gpu_device):
    w = _run_world(gpu_device)
    w.e.commit()
    ts = [b"one/1", b"hot/1", b"hot2/x", b"hot/2"]
    buf, off = pack(ts)
    c, o, to, tg, nd, pk, tot = _device_publish(w.e, gpu_device, buf, off, STICKY, [0, 1, 2, 3], 2, 16)
    assert tot == 4 and [int(x) for x in pk[:2]] == [31, 12]
    # hot2/+ was reached by a dropped slot only: its entry is still undefined, so this publish draws with its key
    assert _picks_raw(w.e, [b"hot2/x", b"hot/9", b"one/2"], STICKY, [1, 0, 1]) == [[22], [12], [31]]
    w.close()


def test_sticky_stream_overflow_and_rerun(gpu_device):
    """caps.rr one below the slots whose entry is undefined: state 4, d_hdr[5]
    exact, no entry stored; the rerun equals the two-call path bit for bit"""
    w = _run_world(gpu_device)
    for i in range(40):
        w.route(b"t/%d" % i, ("g", "n1"))
        w.members(b"g", b"t/%d" % i, [100 + 3 * i, 101 + 3 * i, 102 + 3 * i][: 1 + i % 3])
    w.e.commit()
    ctx = w.e.share_cursors(0)
    ts = [b"t/%d" % (i % 40) for i in range(70)] + _run_batch(30) + [b"nothing/here"]
    keys = [(i * 40503 + 11) % 2 ** 32 for i in range(len(ts))]
    flagged = len(ts) - 1                                       # every $share slot: nothing is defined yet
    for cursors in (None, ctx):
        s = Stream(w, gpu_device, ts, keys, STICKY, (ROOMY[0], ROOMY[1], ROOMY[2], flagged - 1), cursors)
        assert s.state == 4 and s.h[5] == flagged and s.h[0] == flagged
    ref = _reference(w, gpu_device, ts, keys, STICKY, ROOMY[1], ROOMY[2])       # the built-in array: a first run
    again = Stream(w, gpu_device, ts, keys, STICKY, ROOMY, ctx)                # the context: a first run too
    _same(again, ref)
    assert again.h[5] == flagged
    want = [m for row in _want(w, ts, keys) for _, _, m in row]
    assert [int(x) for x in again.d[:, 3]] == want
    exact = Stream(w, gpu_device, ts, [k ^ 0x5555 for k in keys], STICKY, ROOMY[:3] + (0,), None)   # steady state:
    assert exact.state == 0 and exact.h[5] == 0                                # nothing flagged, caps.rr = 0 is room
    assert [int(x) for x in exact.d[:, 3]] == want
    ctx.close()
    w.close()


# ---- the batcher ----------------------------------------------------------------------------------------------

def _batcher_world(device):
    w = SWorld(device)
    w.route(b"r/+", ("g", "n1"))
    w.route(b"r/#", ("h", "n2"))
    w.route(b"x/t", ("g", "n1"))
    w.members(b"g", b"r/+", [1, 2, 3])
    w.members(b"h", b"r/#", [11, 12])
    w.members(b"g", b"x/t", [21, 22, 23, 24])
    w.e.commit()
    return w


def test_batcher_sticky_one_lane_is_one_publisher(gpu_device):
    from emqx_amd.batcher import Batcher
    w = _batcher_world(gpu_device)
    b = Batcher(w.e, max_topics=64, deadline_us=100, publish=True, sticky=True, lanes_per_replica=1)
    pd = Pd(w)
    rng = random.Random(5)
    seq = [b"r/1", b"r/2", b"x/t", b"r/1/z", b"r/9", b"nothing"]
    for step in range(240):
        if step % 40 == 39:                                    # a process exits; it subscribes again as a new one
            m = rng.choice([1, 2, 3, 11, 12, 21, 22, 23, 24])
            sets = [k for k, v in w.sh.tab.items() if m in v]
            w.down(m)
            pd.cleanup_down(m)
            for g, t in sets:
                w.member(g, t, m)
            w.e.commit()
        tp, key = rng.choice(seq), rng.randrange(2 ** 32)
        d, p = _publish_one(b, tp, key)
        want = [m for _, _, m in _want(w, [tp], [key], pd.sh)[0]]
        got = [pk for (_, tg, _, pk) in d if w.e.target_bytes(tg)[0] == Engine.TARGET_GROUP]
        assert [None if pk == Engine.NO_MEMBER else pk for pk in got] == want, (step, tp)
    st = b.stats()
    assert st["failed_batches"] == 0 and st["topics"] == 240
    b.close()
    w.close()


def test_batcher_sticky_two_lanes_each_consistent(gpu_device):
    """two lanes are two publisher processes: until a member goes down a set
    shows at most two members, one per lane; after the down none of them"""
    from emqx_amd.batcher import Batcher
    w = _batcher_world(gpu_device)
    b = Batcher(w.e, max_topics=4, deadline_us=50, publish=True, sticky=True, lanes_per_replica=2)
    rng = random.Random(6)

    def flood(k):
        seen = {}
        for _ in range(k):
            tp = rng.choice([b"r/1", b"x/t"])
            d, _ = _publish_one(b, tp, rng.randrange(2 ** 32))
            for to, tg, _, pk in d:
                if w.e.target_bytes(tg)[0] == Engine.TARGET_GROUP:
                    seen.setdefault((to, tg), set()).add(pk)
        return seen
    seen = flood(120)
    assert len(seen) == 3 and all(1 <= len(v) <= 2 for v in seen.values()), seen
    gone = set().union(*seen.values())
    for m in gone:
        w.down(m)
    w.e.commit()
    after = flood(120)
    assert all(1 <= len(v) <= 2 and not (v & gone) and Engine.NO_MEMBER not in v for v in after.values()), after
    b.close()
    w.close()


# ---- retry picks ------------------------------------------------------------------------------------------------

SIZES = (1, 2, 63, 64, 65, 300)


def _retry_world(device):
    w = SWorld(device)
    w.base = {}
    for i, k in enumerate(SIZES):
        w.base[k] = 1000 * (i + 1)
        w.members(b"g", b"s/%d" % k, list(range(w.base[k], w.base[k] + k)))
    w.members(b"g2", b"s/2", [5, 6])                          # the same topic under another group
    w.members(b"g", b"w/+/#", [7, 8, 9])                      # a wildcard To is found by its bytes as well
    w.e.commit()
    return w


def _failed_lists(w, k, rng):
    ms = list(range(w.base[k], w.base[k] + k))
    strangers = list(range(50_000, 50_400))                   # 400 non-members: longer than the LDS window
    yield []
    yield [rng.choice(ms)]
    yield [m for m in ms if m != ms[k // 2]]                  # all but one
    yield list(ms)                                            # all
    yield strangers[:3]
    yield strangers + ms[:k // 2]                             # past the window, members at its end
    yield ms[k // 2:] + strangers + ms[:1]
    yield []


@pytest.mark.parametrize("strategy", ["keyed", "round_robin", "sticky"])
def test_pick_batch_vs_oracle(gpu_device, strategy):
    w = _retry_world(gpu_device)
    rng = random.Random(SIZES.index(64) + len(strategy))
    api = SharedSub(w.e, strategy)
    ctx = w.e.share_cursors(0)
    pds = {None: w.sh, ctx: Pd(w).sh}
    assert api.pick_many([]) == []                            # n = 0
    # every set with every kind of failed list, twice over: the same set several times in one call
    reqs = [("g", b"s/%d" % k, rng.randrange(2 ** 32), f) for _ in range(2) for k in SIZES
            for f in _failed_lists(w, k, rng)]
    reqs += [("g", b"w/+/#", 4, [8]), ("g2", b"s/2", 1, []), ("g2", b"s/2", 1, [6]), ("g", b"w/+/#", 5, [])]
    reqs += [("nobody", b"s/2", 1, []), ("g", b"s/3", 1, [1]), ("g2", b"s/64", 0, []), ("g", b"", 0, [])]   # no such set
    rng.shuffle(reqs)
    for cursors in (None, ctx, None):
        sh = pds[cursors]
        want = [sh.pick(strategy, key, g.encode(), t, f) for g, t, key, f in reqs]
        assert api.pick_many(reqs, cursors=cursors) == want
    assert sum(m is None for m in want) >= 14 and sum(m is not None for m in want) >= 40
    ctx.close()
    w.close()


def test_pick_batch_order_semantics_by_hand(gpu_device):
    w = _retry_world(gpu_device)
    b = w.base[64]
    G64 = ("g", b"s/64")
    # sticky: undefined -> member (1 rem 64); the stuck member failed -> of the 63 left, member (2 rem 63); kept
    api = SharedSub(w.e, "sticky")
    assert api.pick_many([G64 + (1, []), G64 + (2, [b + 1]), G64 + (3, [])]) == [b + 1, b + 3, b + 3]
    assert api.pick_many([G64 + (9, [])]) == [b + 3]                        # and across calls
    assert _picks_raw(w.e, [b"s/64"], STICKY, [0]) == [[]]                   # (no route: no delivery)
    w.route(b"s/64", ("g", "n1"))
    assert _picks_raw(w.e, [b"s/64"], STICKY, [0]) == [[b + 3]]              # the publish calls read the same entry
    everyone = list(range(b, b + 64))
    assert api.pick_many([G64 + (0, everyone), G64 + (5, [])]) == [None, b + 5]   # `false` is stored as undefined
    # round robin: Rem 0; [b+2 ..]: (0 + 1) rem 63 = 1 -> the second of the rest; one left: cursor untouched; on
    rr = SharedSub(w.e, "round_robin")
    got = rr.pick_many([G64 + (0, []), G64 + (0, [b]), G64 + (0, everyone[1:]), G64 + (0, []), G64 + (0, everyone)])
    assert got == [b, b + 2, b, b + 2, None]
    # keyed is stateless: member (key rem Count') of the rest
    kd = SharedSub(w.e, "keyed")
    assert kd.pick_many([G64 + (64, []), G64 + (64, [b]), G64 + (1, [b + 1])]) == [b, b + 2, b + 2]
    # a context of its own starts undefined whatever the built-in arrays hold
    with w.e.share_cursors(0) as ctx:
        assert api.pick_many([G64 + (7, [])], cursors=ctx) == [b + 7]
        assert api.pick_many([G64 + (8, [])]) == [b + 5]
    w.close()


@pytest.mark.parametrize("nsets", [1, 256])
@pytest.mark.parametrize("strategy", ["round_robin", "sticky"])
def test_pick_batch_missing_sets_between_requests_on_one_set(gpu_device, strategy, nsets):
    """requests for sets that do not exist lie between the requests on one
    set: the set's requests still count in index order.  With one set the
    set indices need no bit at all, and with 256 sets the last index, 255, has
    the all-ones low byte: the key of "no such set" must sort apart from both."""
    w = SWorld(gpu_device)
    for i in range(nsets - 1):
        w.members(b"g", b"f/%d" % i, [5000 + i])
    w.members(b"g", b"last", [1, 2, 3, 4, 5])                  # set index nsets - 1
    w.e.commit()
    api = SharedSub(w.e, strategy)
    hit, miss, other = ("g", b"last"), ("g", b"none"), ("nobody", b"last")
    reqs = [hit + (1, []), miss + (0, []), hit + (2, [2]), other + (3, [1]), miss + (4, []), hit + (3, []),
            hit + (0, [1, 2, 3, 4, 5]), miss + (9, []), hit + (4, [])]
    if nsets > 1:
        reqs[4:4] = [("g", b"f/0", 7, []), ("g", b"f/%d" % (nsets - 2), 7, [])]
    want = [w.sh.pick(strategy, key, g.encode(), t, f) for g, t, key, f in reqs]
    by_hand = {"sticky": [2, None, 4, None, None, 4, None, None, 5],     # 1 rem 5; [1,3,4,5]: 2 rem 4; kept; false; 4 rem 5
               "round_robin": [1, None, 3, None, None, 3, None, None, 4]}[strategy]   # Rem 0; (0+1) rem 4 of [1,3,4,5]; 2; -; 3
    if nsets > 1:
        by_hand[4:4] = [5000, 5000 + nsets - 2]
    assert want == by_hand
    assert api.pick_many(reqs) == want
    assert api.pick_many(reqs[::-1]) == [w.sh.pick(strategy, key, g.encode(), t, f) for g, t, key, f in reqs[::-1]]
    w.close()
