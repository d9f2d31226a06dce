"""The byte corpus of tests/byte_corpus.py through every device entry that
reads topic bytes, element for element and in order against the CPU oracles
(oracle.O1 for match lists, oracle.pytrie.RouteTable for routes and
deliveries, tests/dispatch_ref.py for the local dispatch).  The four SWAR
byte-code copies each meet every byte value beside a '/', every word-length
class at every alignment, trailing-NUL siblings and the two giants:

    kernels.hip   a  tm_tokenize (wave, per-lane LDS, per-lane global) via match_batch
                  b  the same through tm_match_batch_device with off[0] = 0 and 5
                  c  tm_match_small (tokenize_one over global bytes: the NIF's and the batcher's path)
                  d  the micro-batcher, topics submitted singly
    route.hip     e  the routed mode's owner hash against the host's tm_route_of placement
    routes.hip    f  exact_lookup of the publish topic's own routes, then aggre
    dispatch.hip  g  sub_exact_lookup by the publish topic and by To bytes
The device entries of f and g take the same envelopes as b (off[0] = 0 and 5).

A wrong word id, hash or owner loses the topic's exact filter (every topic's
own text is a filter, a route topic and a subscribed topic), so the
comparison fails for that topic; every failure names the first differing
topic with repr of its bytes.  Forced collisions of the dictionary tag and of
the 64-bit topic hash (the negative branch of every byte-verify) are in
tests/test_gpu_collisions.py."""
import contextlib
import os
import random
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import byte_corpus as C  # noqa: E402
from dispatch_ref import SubscriberBag, route_dispatch  # noqa: E402
from emqx_amd import Engine, pack  # noqa: E402

pytestmark = pytest.mark.gpu

WAVE_WALK_DEFAULT = 32768     # option "wave_walk_max" (topicmatch.h)
DESTS = ["n1", "n2", ("g1", "n1"), ("g1", "n2"), ("g2", "n2"), "n3"]


@contextlib.contextmanager
def _deep():
    """oracle.pytrie recurses once per level: room for the 2,000-level topic"""
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 3 * C.DEEP_LEVELS + 1000))
    try:
        yield
    finally:
        sys.setrecursionlimit(old)


def _show(t):
    return repr(t) if len(t) <= 120 else "%r... (%d bytes)" % (t[:120], len(t))


def _first_diff(tag, ts, got, want):
    """got / want: (counts, offsets, ids) CSR; names the first topic whose list differs"""
    gc, go, gi = got
    wc, wo, wi = want
    for t in range(len(ts)):
        a = gi[int(go[t]):int(go[t]) + int(gc[t])]
        b = wi[int(wo[t]):int(wo[t]) + int(wc[t])]
        if len(a) != len(b) or not np.array_equal(a, b):
            bad = sum(1 for u in range(len(ts)) if int(gc[u]) != int(wc[u]))
            raise AssertionError("%s: topic %d %s: got %s want %s (%d topics differ in count)"
                                 % (tag, t, _show(ts[t]), a[:16].tolist(), b[:16].tolist(), bad))


def _check_csr(tag, ts, got, want):
    _first_diff(tag, ts, got, want)
    assert np.array_equal(got[0], want[0]), tag
    assert np.array_equal(got[1], want[1]), tag            # an exclusive scan, n + 1 entries
    assert np.array_equal(got[2], want[2]), tag


# ---- the filter set, the batches and O1's lists: computed once ---------------------

class _Ref:
    def __init__(self):
        from oracle import O1
        self.fs = C.filters(C.all_topics())
        self.fb, self.fo = pack(self.fs)
        o1 = O1(len(self.fs))
        o1.insert_many(self.fb, self.fo)
        self.batches = [("corpus", C.topics())] + [(name, ts) for name, _, ts in C.wave_batches()]
        self.want = {}
        for name, ts in self.batches:
            tb, to = pack(ts)
            self.want[name] = o1.match_ids(tb, to, threads=16)
        o1.close()
        oc = self.want["corpus"][0]
        assert (oc > 0).mean() >= 0.95                      # (tests/test_byte_corpus.py pins this on the CPU)


@pytest.fixture(scope="module")
def ref():
    return _Ref()


@pytest.fixture(scope="module")
def eng(gpu_device, ref):
    e = Engine(device=gpu_device)
    e.insert_many(ref.fb, ref.fo)
    e.commit()
    yield e
    e.close()


def _options(e, tok_wave, wave_walk_max):
    e.set_option("tok_wave", tok_wave)
    e.set_option("wave_walk_max", WAVE_WALK_DEFAULT if wave_walk_max is None else wave_walk_max)


# ---- a. the tokenizer through the host entry ----------------------------------------

@pytest.mark.parametrize("tok_wave", [1, 0])
@pytest.mark.parametrize("wave_walk_max", [None, 0])        # the wave walk / the per-lane queue walk read the rows
def test_tokenizer_byte_corpus_vs_o1(eng, ref, tok_wave, wave_walk_max):
    _options(eng, tok_wave, wave_walk_max)
    try:
        for name, ts in ref.batches:
            tb, to = pack(ts)
            want = ref.want[name]
            _check_csr("%s owned" % name, ts, eng.match_batch(tb, to), want)                 # library-owned output
            cap = int(want[1][-1]) + 7
            _check_csr("%s out_cap" % name, ts, eng.match_batch(tb, to, out_cap=cap), want)  # the caller's array
    finally:
        _options(eng, 1, None)


# ---- b. the device entry, off[0] = 0 and 5, '/' all around ---------------------------

def _device_csr(e, buf, off, dev):
    import torch
    from emqx_amd.engine import check_total
    d = torch.device("cuda", dev)
    n = len(off) - 1
    nbytes = int(off[-1] - off[0])
    d_b = torch.from_numpy(buf.copy()).to(d)
    d_o = torch.from_numpy(np.ascontiguousarray(off).view(np.int64).copy()).to(d)
    d_c = torch.full((max(n, 1),), -1, dtype=torch.int32, device=d)
    d_oo = torch.full((n + 1,), -1, dtype=torch.int64, device=d)
    d_t = torch.full((1,), -1, dtype=torch.int64, device=d)
    torch.cuda.synchronize(d)
    e.match_batch_device(d_b, d_o, n, nbytes, d_c, d_oo, None, 0, d_t)      # counts, offsets, the total
    torch.cuda.synchronize(d)
    cap = int(d_t.item()) + 3
    d_i = torch.full((cap,), -1, dtype=torch.int32, device=d)
    torch.cuda.synchronize(d)
    e.match_batch_device(d_b, d_o, n, nbytes, d_c, d_oo, d_i, cap, d_t)
    torch.cuda.synchronize(d)
    total = check_total(d_t, cap)
    ids = d_i.cpu().numpy().view(np.uint32)
    assert np.all(ids[total:] == 0xFFFFFFFF)                 # nothing written past the total
    return d_c.cpu().numpy().view(np.uint32)[:n], d_oo.cpu().numpy().view(np.uint64), ids[:total]


@pytest.mark.parametrize("lead", [0, 5])
@pytest.mark.parametrize("tok_wave", [1, 0])
def test_device_entry_in_an_envelope_vs_o1(eng, ref, gpu_device, lead, tok_wave):
    _options(eng, tok_wave, None)
    try:
        for name, ts in ref.batches:
            buf, off = C.envelope(ts, lead)
            _check_csr("%s lead %d" % (name, lead), ts, _device_csr(eng, buf, off, gpu_device), ref.want[name])
    finally:
        _options(eng, 1, None)


# ---- c. the one-launch small path: tokenize_one over global bytes --------------------

@pytest.mark.parametrize("lead", [0, 5])
def test_small_path_in_an_envelope_vs_o1(eng, ref, gpu_device, lead):
    from test_gpu_small import _check, _small
    for name, ts in ref.batches:
        buf, off = C.envelope(ts, lead)
        oc, oo, oi = ref.want[name]
        c, o, ids, total = _small(eng, buf, off, cap=int(oo[-1]) + 64, dev=gpu_device)
        _first_diff("%s lead %d" % (name, lead), ts, (c, o, ids), (oc, oo, oi))
        _check(c, o, ids, total, oc, oo, oi)                # lists tile [0, total), each topic id for id


# ---- the route bag and the subscriber bag over a stratified subset --------------------

class _World:
    """routes on the subset's exact topics (the route source is then the
    publish topic itself) and on its wildcard filters, plain and shared
    subscribers on both, in the engine and in the oracles"""

    def __init__(self, device):
        from emqx_amd.emqx_broker import Broker
        from emqx_amd.emqx_router import Router
        from oracle import pytrie
        rng = random.Random(C.SEED + 50)
        self.topics = C.stratified()
        self.filters = C.filters(self.topics)
        self.e = Engine(device=device)
        self.r, self.o, self.bag = Router(self.e, node="n1"), pytrie.RouteTable(), SubscriberBag()
        self.b = Broker(self.e, self.r)
        sub = 0
        for f in self.filters:
            for d in rng.sample(DESTS, rng.choice([1, 1, 2, 3])):
                self.r.add_route(f, d)
                self.o.add_route(f, d)
            if rng.random() < 0.7:
                for _ in range(rng.choice([1, 1, 2, 5])):
                    g = rng.choice(["g1", "g2"]) if rng.random() < 0.3 else None
                    self.e.sub_add(f, sub, g.encode() if g else None)
                    self.bag.insert_subscriber(g, f, sub)
                    sub += 1
        self.e.commit()
        assert sum(1 for t in self.topics if t in self.o.routes) > len(self.topics) * 0.9
        assert sum(1 for t in self.topics if self.bag.member(t)) > len(self.topics) * 0.6


@pytest.fixture(scope="module")
def world(gpu_device):
    w = _World(gpu_device)
    yield w
    w.e.close()


# ---- d. the micro-batcher --------------------------------------------------------------

def _submit_all(b, topics):
    got = [None] * len(topics)

    def producer(k):
        for t in range(k, len(topics), 4):
            def cb(status, ids, dests, t=t):
                got[t] = (status, ids, dests)
            b.submit(topics[t], cb)
    th = [threading.Thread(target=producer, args=(k,)) for k in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    b.flush()
    st = b.stats()
    b.close()
    assert st["topics"] == len(topics) and st["failed_batches"] == 0
    return got


def test_batcher_match_every_corpus_topic_vs_o1(eng, ref):
    """every corpus topic, the 65,535-byte one included (max_bytes is 64 MiB), singly from 4 threads"""
    from emqx_amd.batcher import Batcher
    ts = C.topics()
    oc, oo, oi = ref.want["corpus"]
    got = _submit_all(Batcher(eng, max_topics=700, deadline_us=300), ts)
    for t, topic in enumerate(ts):
        status, ids, _ = got[t]
        assert status == 0, _show(topic)
        assert ids == oi[int(oo[t]):int(oo[t + 1])].tolist(), "topic %d %s" % (t, _show(topic))


def test_batcher_routes_every_corpus_topic_vs_pytrie(world):
    from emqx_amd.batcher import Batcher
    e, ts = world.e, C.topics()
    got = _submit_all(Batcher(e, max_topics=700, deadline_us=300, routes=True), ts)
    names = {}
    routes = 0
    with _deep():
        for t, topic in enumerate(ts):
            status, src, dst = got[t]
            assert status == 0, _show(topic)
            have = []
            for s, d in zip(src, dst):
                if s != Engine.TOPIC_ROUTE and s not in names:
                    names[s] = e.filter_bytes(s)
                have.append((topic if s == Engine.TOPIC_ROUTE else names[s], world.r._dest(d)))
            assert have == world.o.match_routes(topic), "topic %d %s" % (t, _show(topic))
            routes += len(have)
    assert routes > len(ts)


# ---- e. the routed sharded mode: route.hip's owner against tm_route_of ----------------

@pytest.mark.parametrize("S,depth", [(2, 1), (3, 2)])
def test_routed_every_rank_equals_o1(gpu_device, ref, S, depth):
    from emqx_amd import shard
    ts = C.topics()
    oc, oo, oi = ref.want["corpus"]
    rs = shard.RoutedSet([0] * S, depth=depth, filters_hint=len(ref.fs))
    try:
        rs.insert_many(ref.fb, ref.fo)                     # global ids = the filter's index = O1's ids
        # rank r's batch starts at off[0] = 0 (even r) or 5 (odd r), '/' all around: an owner hashed
        # over one byte outside the topic's first levels sends the topic to a shard without its filters
        got = rs.match_batches([C.envelope(ts[r::S], (0, 5)[r % 2]) for r in range(S)])
    finally:
        rs.close()
    for r in range(S):
        idx = range(r, len(ts), S)
        wc = oc[r::S]
        wo = np.zeros(len(wc) + 1, dtype=np.uint64)
        wo[1:] = np.cumsum(wc, dtype=np.uint64)
        wi = np.concatenate([oi[int(oo[t]):int(oo[t + 1])] for t in idx] + [np.zeros(0, dtype=np.uint32)])
        _check_csr("rank %d of %d, depth %d" % (r, S, depth), ts[r::S], got[r], (wc, wo, wi))


# ---- f. routes and deliveries ----------------------------------------------------------

def test_routes_and_deliveries_vs_pytrie(world):
    ts = world.topics
    routes = world.r.match_routes_many(ts)
    dels = world.r.match_deliveries_many(ts, tagged=True)
    exact = 0
    with _deep():
        for t, topic in enumerate(ts):
            want = world.o.match_routes(topic)
            assert [(x.topic, x.dest) for x in routes[t]] == want, "routes of topic %d %s" % (t, _show(topic))
            assert dels[t] == world.o.match_deliveries(topic), "deliveries of topic %d %s" % (t, _show(topic))
            exact += sum(1 for to, _ in want if to == topic and not _wild(topic))
    assert exact > len(ts)                                  # routes found by the topic's own bytes


def _wild(t):
    lv = t.split(b"/")
    return b"+" in lv or b"#" in lv


def _dev(x, dev, dtype=None):
    import torch
    a = np.ascontiguousarray(x)
    return torch.from_numpy(a.view(dtype).copy() if dtype else a.copy()).to(torch.device("cuda", dev))


def _i32(n, dev, fill=-1):
    import torch
    return torch.full((max(n, 1),), fill, dtype=torch.int32, device=torch.device("cuda", dev))


def _i64(n, dev, fill=-1):
    import torch
    return torch.full((max(n, 1),), fill, dtype=torch.int64, device=torch.device("cuda", dev))


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("lead", [0, 5])
def test_routes_and_deliveries_device_entries_in_an_envelope(world, gpu_device, lead):
    """tm_match_routes_batch_device / tm_match_deliveries_batch_device read the
    publish topic's bytes at d_topic_off as given (routes.hip exact_lookup)"""
    import torch
    e, ts = world.e, world.topics
    n = len(ts)
    with _deep():
        want_r = [world.o.match_routes(t) for t in ts]
        want_d = [world.o.match_deliveries(t) for t in ts]
    cap = sum(len(x) for x in want_r) + 5
    buf, off = C.envelope(ts, lead)
    d_b, d_o = _dev(buf, gpu_device), _dev(off, gpu_device, np.int64)
    nbytes = int(off[-1] - off[0])
    names, tnames = {}, {}

    def name(s, topic):
        if s == Engine.TOPIC_ROUTE:
            return topic
        if s not in names:
            names[s] = e.filter_bytes(s)
        return names[s]
    c, o, tot = _i32(n, gpu_device), _i64(n + 1, gpu_device), _i64(1, gpu_device)
    a, b = _i32(cap, gpu_device), _i32(cap, gpu_device)
    torch.cuda.synchronize()
    e.match_routes_batch_device(d_b, d_o, n, nbytes, c, o, a, b, cap, tot)
    torch.cuda.synchronize()
    assert int(tot.item()) == cap - 5
    ch, oh, ah, bh = _u32(c), o.cpu().numpy(), _u32(a), _u32(b)
    for t, topic in enumerate(ts):
        got = [(name(int(ah[j]), topic), world.r._dest(int(bh[j]))) for j in range(int(oh[t]), int(oh[t + 1]))]
        assert int(ch[t]) == len(got) and got == want_r[t], "routes of topic %d %s" % (t, _show(topic))
    c, o, tot = _i32(n, gpu_device), _i64(n + 1, gpu_device), _i64(1, gpu_device)
    a, b = _i32(cap, gpu_device), _i32(cap, gpu_device)
    torch.cuda.synchronize()
    e.match_deliveries_batch_device(d_b, d_o, n, nbytes, c, o, a, b, cap, tot)
    torch.cuda.synchronize()
    assert int(tot.item()) == cap - 5
    ch, oh, ah, bh = _u32(c), o.cpu().numpy(), _u32(a), _u32(b)
    for t, topic in enumerate(ts):
        got = []
        for j in range(int(oh[t]), int(oh[t]) + int(ch[t])):
            g = int(bh[j])
            if g not in tnames:
                tnames[g] = e.target_bytes(g)
            got.append((name(int(ah[j]), topic), tnames[g]))
        assert got == want_d[t], "deliveries of topic %d %s" % (t, _show(topic))


# ---- g. the local dispatch ---------------------------------------------------------------

def test_publish_dispatch_vs_reference(world):
    ts = world.topics
    got = world.b.publish_many(ts)
    pairs = local = 0
    with _deep():
        for topic, pub in zip(ts, got):
            counts, want = route_dispatch(world.o, world.bag, b"n1", topic)
            assert [(d.to, d.target) for d in pub.deliveries] == world.o.match_deliveries(topic), _show(topic)
            assert [d.count for d in pub.deliveries] == counts, _show(topic)      # Counts and NOT_LOCAL (None)
            assert pub.pairs == want, _show(topic)                                # ordered (To, subscriber) pairs
            pairs += len(want)
            local += sum(1 for c in counts if c is not None)
    assert pairs > len(ts) and local > len(ts)


@pytest.mark.parametrize("lead", [0, 5])
def test_dispatch_device_entry_in_an_envelope(world, gpu_device, lead):
    """tm_match_dispatch_batch_device: dispatch.hip looks the publish topic's
    own bag up by the bytes at d_topic_off as given"""
    import torch
    e, ts = world.e, world.topics
    n = len(ts)
    with _deep():
        want = [route_dispatch(world.o, world.bag, b"n1", t) for t in ts]
        slots = sum(len(world.o.match_routes(t)) for t in ts)      # deliveries sit at their route offsets
    pairs = sum(len(p) for _, p in want)
    cap, scap = slots + 5, pairs + 5
    buf, off = C.envelope(ts, lead)
    d_b, d_o = _dev(buf, gpu_device), _dev(off, gpu_device, np.int64)
    c, o, tot = _i32(n, gpu_device), _i64(n + 1, gpu_device), _i64(1, gpu_device)
    to, tg, nd = _i32(cap, gpu_device), _i32(cap, gpu_device), _i32(cap, gpu_device)
    sc, so, stot = _i32(n, gpu_device), _i64(n + 1, gpu_device), _i64(1, gpu_device)
    sto, sid = _i32(scap, gpu_device, -7), _i32(scap, gpu_device, -7)
    torch.cuda.synchronize()
    e.match_dispatch_batch_device(d_b, d_o, n, int(off[-1] - off[0]), c, o, to, tg, nd, cap, tot, sc, so, sto, sid,
                                  scap, stot)
    torch.cuda.synchronize()
    assert int(tot.item()) == slots and int(stot.item()) == pairs
    ch, oh, toh, ndh = _u32(c), o.cpu().numpy(), _u32(to), _u32(nd)
    sch, soh, stoh, sidh = _u32(sc), so.cpu().numpy(), _u32(sto), _u32(sid)
    assert list(sidh[pairs:].view(np.int32)) == [-7] * 5         # nothing past the pairs
    names = {}

    def name(s, topic):
        if s == Engine.TOPIC_ROUTE:
            return topic
        if s not in names:
            names[s] = e.filter_bytes(s)
        return names[s]
    for t, topic in enumerate(ts):
        counts, wp = want[t]
        a = int(oh[t])
        got_c = [None if int(ndh[j]) == Engine.NOT_LOCAL else int(ndh[j]) for j in range(a, a + int(ch[t]))]
        assert got_c == counts, "Counts of topic %d %s" % (t, _show(topic))
        p = int(soh[t])
        got_p = [(name(int(stoh[j]), topic), int(sidh[j])) for j in range(p, p + int(sch[t]))]
        assert got_p == wp, "pairs of topic %d %s" % (t, _show(topic))


def test_dispatch_by_to_bytes_vs_bag(world):
    """Tos present in the table, absent from it, and differing from a present
    one only by a trailing NUL (heads and arena are zero padded: only the
    length tells them apart)"""
    present = [f for f in world.filters if world.bag.member(f)]
    absent = [f for f in world.filters if not world.bag.member(f)]
    nul = [f + b"\0" for f in present[::3]] + [f[:-1] for f in present if f.endswith(b"\0")] + \
        [f[:-1] + b"\0" for f in present[::5] if f]
    tos = present + absent + nul + [b"nobody/home", b"", b"\0"]
    assert any(not world.bag.member(t) for t in nul) and len(present) > 1000 and len(absent) > 100
    got = world.b.dispatch_many(tos)
    hit = 0
    for to, (count, subs) in zip(tos, got):
        want = world.bag.subscribers(to)
        assert count == len(want), _show(to)
        assert subs == [x for x in want if not isinstance(x, tuple)], _show(to)
        hit += bool(want)
    assert hit >= len(present)
    # subscribers/1 by bytes on the host agrees on the same keys
    for to in nul[:200] + present[:200]:
        assert world.b.subscribers(to) == [x if not isinstance(x, tuple) else ("share", x[1].encode(), x[2])
                                           for x in world.bag.subscribers(to)], _show(to)
