"""tm_publish_stream_device and tm_share_cursors on the GPU.

The oracles are tests/shared_ref.py, tests/dispatch_ref.py and oracle/pytrie.py;
tm_match_publish_batch_device + tm_publish_pack_device are a second check.  One
small world per module: a few hundred filters with local, remote-node and group
routes, plain subscribers, member sets of 0, 1, 2, 3 and 64 members on filters
and on exact topics.

Every stream call runs with 64 guard elements of a fill pattern after each
output and after the workspace (which is itself pre-filled with the pattern, so
stale workspace is what every pass finds), and they must come back unchanged.

The built-in cursor array, the context CTX of the module and the oracle
dictionary PD move in lock step: whatever advances one is run on the others.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import byte_corpus as C  # noqa: E402
from publish_util import GUARD, World  # noqa: E402
from shared_ref import SharedSub as RefShared, route_shared  # noqa: E402
from emqx_amd import Engine  # noqa: E402
from emqx_amd.engine import pack  # noqa: E402
from oracle import pytrie  # noqa: E402

pytestmark = pytest.mark.gpu

G = 64                      # guard elements
KEYED, RR = Engine.SHARE_KEYED, Engine.SHARE_ROUND_ROBIN
SIZES = (0, 1, 2, 3, 64)
ROOMY = (200_000, 200_000, 200_000, 100_000)


class Pd:
    """one publisher process's dictionary over the world's one member table"""

    def __init__(self, w):
        self.sh = RefShared()
        self.sh.tab = w.sh.tab


def _build(device):
    w = World(device)
    wild = [b"a/+", b"a/#", b"+/b", b"c/+/d", b"c/#", b"+/+", b"d/+", b"a/b/#", b"+/c/+", b"e/#", b"e/+", b"s/#"]
    exact = [b"t/%d" % i for i in range(40)] + [b"a/b", b"c/x/d", b"e/f", b"d"]
    m = 1000
    for i, f in enumerate(wild + exact):
        w.route(f, ("n1", "n2", "n1")[i % 3])
        if i % 3 != 1:
            w.sub(f, 100 + i)
        if i % 4 == 0:
            w.sub(f, 300 + i)
        if i % 2 == 0:
            g = ("g1", "g2")[i // 2 % 2]
            w.route(f, (g, "n1"))
            k = SIZES[i // 2 % 5]
            if k:
                w.members(g.encode(), f, list(range(m, m + k)))
                m += k
    for f in (b"a/#", b"t/3", b"+/+"):                     # {g, n1} and {g, n2}: aggre leaves a hole
        w.route(f, ("g3", "n1"))
        w.route(f, ("g3", "n2"))
    w.members(b"g3", b"a/#", [71, 72, 73])
    for i in range(240):                                   # filler: a few hundred filters
        f = b"f/%d/+" % i
        w.route(f, "n1" if i % 2 else "n2")
        if i % 7 == 0:
            w.sub(f, 4000 + i)
        if i % 5 == 0:
            w.route(f, ("g2", "n2"))
            k = SIZES[i // 5 % 5]
            if k:
                w.members(b"g2", f, list(range(m, m + k)))
                m += k
    w.route(b"hot/#", ("gh", "n1"))
    w.members(b"gh", b"hot/#", [9001, 9002, 9003])
    w.route(b"hot2/+", ("gh", "n2"))
    w.members(b"gh", b"hot2/+", [9101, 9102])
    w.route(b"one/+", ("g1", "n1"))
    w.members(b"g1", b"one/+", [9201])
    w.route(b"xt/hot", ("gh", "n1"))                       # an exact-topic set of 64
    w.members(b"gh", b"xt/hot", list(range(9300, 9364)))
    w.e.commit()
    w.pool = exact + [b"a/c", b"x/b", b"c/y/d", b"c/z", b"d/e", b"a/b/c", b"z/c/z", b"e/g", b"nothing/at/all/here",
                      b"s/1", b"t/3", b"hot/1", b"hot2/x", b"one/1", b"xt/hot"] + [b"f/%d/x" % i for i in range(0, 240, 3)]
    w.ctx = w.e.share_cursors(0)
    w.pd = Pd(w)
    return w


@pytest.fixture(scope="module")
def world(gpu_device):
    w = _build(gpu_device)
    yield w
    w.ctx.close()
    w.close()


def _batch(w, n, salt=0):
    ts = [w.pool[(7 * i + salt) % len(w.pool)] for i in range(n)]
    return ts, [(i * 2654435761 + 17) % 2 ** 32 for i in range(n)]


def _filled(count, dev, width=4):
    import torch
    a = np.full(max(count, 1) * (width // 4), GUARD, dtype=np.uint32)
    return torch.from_numpy(a.view(np.int32).copy()).to(torch.device("cuda", dev))


class Stream:
    """one tm_publish_stream_device call over torch buffers, guards included"""

    def __init__(self, w, dev, topics, keys, strategy, caps, cursors, envelope=None, stream=None, sync=True):
        import torch
        self.w, self.n, self.caps = w, len(topics), tuple(int(c) for c in caps)
        n = self.n
        buf, off = envelope if envelope is not None else pack(topics)
        tdev = torch.device("cuda", dev)
        self.d_b = torch.from_numpy((buf if len(buf) else np.zeros(1, np.uint8)).copy()).to(tdev)
        self.d_o = torch.from_numpy(np.ascontiguousarray(off).view(np.int64).copy()).to(tdev)
        self.d_k = None if keys is None else torch.from_numpy(
            np.asarray(keys if n else [0], dtype=np.uint32).view(np.int32).copy()).to(tdev)
        self.nbytes = int(off[-1] - off[0])
        self.ws_bytes = w.e.publish_stream_workspace_bytes(n, self.nbytes, self.caps)
        assert self.ws_bytes > 0 and self.ws_bytes % 4 == 0
        self.ws = _filled(self.ws_bytes // 4 + G, dev)
        self.hdr = _filled(8 + G, dev, 8)
        self.doff, self.soff = _filled(n + 1 + G, dev, 8), _filled(n + 1 + G, dev, 8)
        self.deliv, self.pairs = _filled(self.caps[1] + G, dev, 16), _filled(self.caps[2] + G, dev, 8)
        torch.cuda.synchronize()
        self.call = lambda: w.e.publish_stream_device(                                   # noqa: E731
            self.d_b, self.d_o, n, self.nbytes, strategy, self.d_k, cursors, self.caps, self.ws, self.ws_bytes,
            self.hdr, self.doff, self.soff, self.deliv, self.pairs, stream=stream)
        if sync:
            self.call()
            torch.cuda.synchronize()
            self.read()

    def read(self):
        u32 = lambda t: t.cpu().numpy().view(np.uint32)      # noqa: E731
        u64 = lambda t: t.cpu().numpy().view(np.uint64)      # noqa: E731
        n, (_, cr, cp, _) = self.n, self.caps
        hdr, doff, soff = u64(self.hdr), u64(self.doff), u64(self.soff)
        deliv, pairs, ws = u32(self.deliv).reshape(-1, 4), u32(self.pairs).reshape(-1, 2), u32(self.ws)
        g64 = np.uint64(GUARD << 32 | GUARD)
        assert (hdr[8:] == g64).all() and (doff[n + 1:] == g64).all() and (soff[n + 1:] == g64).all()
        assert (deliv[cr:] == GUARD).all() and (pairs[cp:] == GUARD).all()
        assert (ws[self.ws_bytes // 4:] == GUARD).all() and len(ws) == self.ws_bytes // 4 + G
        self.h = [int(x) for x in hdr[:8]]
        self.state = self.h[6]
        assert self.h[7] == 0
        self.o, self.so = doff[:n + 1], soff[:n + 1]
        if self.state == 0:
            D, P = self.h[2], self.h[3]
            assert (deliv[D:cr] == GUARD).all() and (pairs[P:cp] == GUARD).all()    # nothing past D / P either
            self.d, self.p = deliv[:D], pairs[:P]
        return self


def _reference(w, dev, topics, keys, strategy, cap, scap):
    """tm_match_publish_batch_device + tm_publish_pack_device: (hdr[4], doff, sub_off, deliv[:D], pairs[:P])"""
    import torch
    n = len(topics)
    buf, off = pack(topics)
    tdev = torch.device("cuda", dev)
    d_b = torch.from_numpy((buf if len(buf) else np.zeros(1, np.uint8)).copy()).to(tdev)
    d_o = torch.from_numpy(off.view(np.int64).copy()).to(tdev)
    d_k = None if keys is None else torch.from_numpy(np.asarray(keys if n else [0], np.uint32).view(np.int32).copy()).to(tdev)
    i32 = lambda k: torch.full((max(k, 1),), -7, dtype=torch.int32, device=tdev)     # noqa: E731
    i64 = lambda k: torch.full((max(k, 1),), -7, dtype=torch.int64, device=tdev)     # noqa: E731
    c, o, tot, sc, so, stot = i32(n), i64(n + 1), i64(1), i32(n), i64(n + 1), i64(1)
    to, tg, nd, pk, sto, sid = i32(cap), i32(cap), i32(cap), i32(cap), i32(scap), i32(scap)
    hdr, doff, deliv, pairs = i64(4), i64(n + 1), i32(4 * cap), i32(2 * scap)
    torch.cuda.synchronize()
    w.e.match_publish_batch_device(d_b, d_o, n, int(off[-1] - off[0]), c, o, to, tg, nd, cap, tot, sc, so, sto, sid,
                                   scap, stot, strategy, d_k, pk)
    w.e.publish_pack(n, c, o, to, tg, nd, pk, cap, tot, so, sto, sid, scap, stot, hdr, doff, deliv, cap, pairs, scap)
    torch.cuda.synchronize()
    h = [int(x) for x in hdr.cpu().numpy().view(np.uint64)]
    return (h, doff.cpu().numpy().view(np.uint64)[:n + 1], so.cpu().numpy().view(np.uint64)[:n + 1],
            deliv.cpu().numpy().view(np.uint32).reshape(-1, 4)[:h[2]], pairs.cpu().numpy().view(np.uint32).reshape(-1, 2)[:h[3]])


def _oracle(w, topics, keys, strategy, pd):
    """per topic (deliveries in the terms of World.got, pairs), and the four stage totals"""
    from dispatch_ref import route_dispatch
    from publish_util import NODE
    rows, ids, routes, npairs, ranked = [], 0, 0, 0, 0
    for i, t in enumerate(topics):
        ids += len(w.o.trie.match(t))
        routes += len(w.o.match_routes(t))
        dels = w.o.match_deliveries(t)
        counts, pairs = route_dispatch(w.o, w.bag, NODE, t)
        picks = route_shared(w.o, pd.sh, "keyed" if strategy == KEYED else "round_robin",
                             None if keys is None else int(keys[i]), t)
        ranked += sum(1 for to, (kind, x) in dels if kind == 1 and len(w.sh.tab.get((x, to), ())) >= 2)
        npairs += len(pairs)
        rows.append(([(to, tg, c, m) for (to, tg), c, m in zip(dels, counts, picks)], pairs))
    return rows, (ids, routes, npairs, ranked)


def _check_oracle(w, topics, s, rows):
    for t, tp in enumerate(topics):
        d = [tuple(int(x) for x in r) for r in s.d[int(s.o[t]):int(s.o[t + 1])]]
        p = [tuple(int(x) for x in r) for r in s.p[int(s.so[t]):int(s.so[t + 1])]]
        assert w.got(tp, d, p) == rows[t], (t, tp)


def _same(s, ref):
    h, doff, soff, deliv, pairs = ref
    assert s.state == 0 and s.h[:4] == h
    assert np.array_equal(s.o, doff) and np.array_equal(s.so, soff)
    assert np.array_equal(s.d, deliv) and np.array_equal(s.p, pairs)


def _paired_rr(w, dev, topics, caps=ROOMY):
    """round robin on the built-in array (the existing call), on CTX (the new
    call) and on PD (the oracle), which stay in lock step; returns the call"""
    ref = _reference(w, dev, topics, None, RR, caps[1], caps[2])
    s = Stream(w, dev, topics, None, RR, caps, w.ctx)
    rows, totals = _oracle(w, topics, None, RR, w.pd)
    _same(s, ref)
    _check_oracle(w, topics, s, rows)
    assert (s.h[4], s.h[0], s.h[1], s.h[5]) == totals
    return s


# ---- 1. equality, keyed and round robin ---------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 256, 257, 600])
def test_stream_equals_publish_and_pack(world, gpu_device, n):
    w = world
    ts, keys = _batch(w, n, salt=n)
    s = Stream(w, gpu_device, ts, keys, KEYED, ROOMY, None)
    _same(s, _reference(w, gpu_device, ts, keys, KEYED, ROOMY[1], ROOMY[2]))
    rows, totals = _oracle(w, ts, keys, KEYED, w.pd)
    _check_oracle(w, ts, s, rows)
    assert (s.h[4], s.h[0], s.h[1], s.h[5]) == totals[:3] + (0,)
    if n == 0:
        assert s.h == [0] * 8 and list(s.o) == [0] and list(s.so) == [0]
    r = _paired_rr(w, gpu_device, ts)
    if n >= 63:
        assert r.h[5] > 0 and r.h[0] > r.h[2] > 0 and r.h[1] > 0      # ranked slots, holes, pairs: all there


# ---- 2. round-robin runs across the wave, block and sort-tile edges -----------------------------------------

@pytest.mark.parametrize("k", [1, 63, 64, 65, 257, 4200])
def test_round_robin_run_lengths(world, gpu_device, k):
    """one hot set hit k times in a batch, interleaved with other sets, sets of one and the 64-member exact set"""
    w = world
    others = [b"hot2/x", b"one/1", b"xt/hot", b"a/b", b"f/0/x", b"t/4"]
    ts = []
    for i in range(k):
        ts.append(b"hot/%d" % (i % 5))
        if i % 3 == 0:
            ts.append(others[(i // 3) % len(others)])
    rows, totals = _oracle(w, ts, None, RR, Pd(w))
    m = totals[3]
    assert m >= k
    for rr_cap in (m + 1000, m):
        with w.e.share_cursors(0) as ctx:                               # a fresh publisher: the same picks again
            s = Stream(w, gpu_device, ts, None, RR, (totals[0] + 5, totals[1] + 5, totals[2] + 5, rr_cap), ctx)
            assert s.state == 0 and s.h[5] == m
            _check_oracle(w, ts, s, rows)
    hot = [d[3] for r, _ in rows for d in r if d[0] == b"hot/#"]
    assert hot == [9001 + i % 3 for i in range(k)]


def test_round_robin_nothing_to_rank(world, gpu_device):
    """m = 0 with caps.rr = 0: sets of one, empty sets, node deliveries only"""
    w = world
    ts = [b"one/1", b"x/y", b"nothing/at/all/here", b"one/2", b"f/1/x"] * 30
    rows, totals = _oracle(w, ts, None, RR, Pd(w))
    assert totals[3] == 0
    with w.e.share_cursors(0) as ctx:
        s = Stream(w, gpu_device, ts, None, RR, (totals[0], totals[1], totals[2], 0), ctx)
    assert s.state == 0 and s.h[5] == 0
    _check_oracle(w, ts, s, rows)
    assert any(d[3] == 9201 for r, _ in rows for d in r)


# ---- 3. cursor persistence and independence -----------------------------------------------------------------

def test_cursors_persist_and_contexts_are_independent(world, gpu_device):
    w = world
    b1, b2, b3 = (_batch(w, 90, salt=s)[0] + [b"hot/1", b"xt/hot"] * 4 for s in (1, 2, 3))
    _paired_rr(w, gpu_device, b1)
    _paired_rr(w, gpu_device, b2)
    w.e.commit()                                                         # nothing changed: the cursors stay
    w.sub(b"t/1", 77001)                                                 # and a commit that rewrites an image
    w.e.commit()
    _paired_rr(w, gpu_device, b3)
    # a second publisher on the same sets starts at Rem 0 ...
    with w.e.share_cursors(0) as other:
        pd2 = Pd(w)
        for b in (b1, b3):
            s = Stream(w, gpu_device, b, None, RR, ROOMY, other)
            _check_oracle(w, b, s, _oracle(w, b, None, RR, pd2)[0])
        assert pd2.sh.pd != w.pd.sh.pd
        # ... and has not disturbed the first
        _paired_rr(w, gpu_device, b2)
    # NULL = the built-in array, continued by the existing call; CTX and PD catch up with the same batches
    s = Stream(w, gpu_device, b1, None, RR, ROOMY, None)
    ref = _reference(w, gpu_device, b2, None, RR, ROOMY[1], ROOMY[2])
    s1 = Stream(w, gpu_device, b1, None, RR, ROOMY, w.ctx)
    s2 = Stream(w, gpu_device, b2, None, RR, ROOMY, w.ctx)
    assert np.array_equal(s.d, s1.d)
    _same(s2, ref)
    _check_oracle(w, b1, s1, _oracle(w, b1, None, RR, w.pd)[0])
    _check_oracle(w, b2, s2, _oracle(w, b2, None, RR, w.pd)[0])


def test_reused_set_index_is_undefined_in_every_context(gpu_device):
    w = World(gpu_device)
    w.route(b"r/+", ("g", "n1"))
    w.route(b"q/+", ("g", "n1"))
    w.members(b"g", b"r/+", [1, 2, 3])
    w.members(b"g", b"q/+", [11, 12, 13])
    w.e.commit()
    ctxs = [w.e.share_cursors(0) for _ in range(2)]
    pds = [Pd(w) for _ in ctxs]

    def publish(ts, which):
        for i in which:
            s = Stream(w, gpu_device, ts, None, RR, (64, 64, 64, 64), ctxs[i])
            _check_oracle(w, ts, s, _oracle(w, ts, None, RR, pds[i])[0])
            yield [int(x) for x in s.d[:, 3]]

    assert list(publish([b"r/1", b"q/1", b"r/2"], (0, 1))) == [[1, 11, 2]] * 2
    assert list(publish([b"r/1"], (0,))) == [[3]]
    for m in (1, 2, 3):                                                  # the set goes: its index is freed ...
        w.e.share_del(b"g", b"r/+", m)
        w.sh.unsubscribe(b"g", b"r/+", m)
    w.e.commit()
    w.e.commit()                                                         # ... by both epochs
    w.route(b"z/+", ("g", "n1"))
    w.members(b"g", b"z/+", [21, 22, 23])                                # a new set takes it
    w.e.commit()
    third = w.e.share_cursors(0)                                         # opened after sets exist: all undefined
    ctxs.append(third)
    pds.append(Pd(w))
    assert list(publish([b"z/1", b"q/1", b"r/1"], (0, 1, 2))) == [[21, 12, 0xFFFFFFFF]] * 2 + [[21, 11, 0xFFFFFFFF]]
    for c in ctxs:
        c.close()
    w.close()


def test_engine_closed_before_its_context(gpu_device):
    w = World(gpu_device)
    w.route(b"r/+", ("g", "n1"))
    w.members(b"g", b"r/+", [1, 2])
    w.e.commit()
    ctx = w.e.share_cursors(0)
    s = Stream(w, gpu_device, [b"r/1"], None, RR, (8, 8, 8, 8), ctx)
    assert [int(x) for x in s.d[:, 3]] == [1]
    with pytest.raises(Exception):
        w.e.share_cursors(1)                                             # no such replica
    w.close()
    ctx.close()                                                          # detached: only the host struct goes


# ---- 4. overflow of each stage ------------------------------------------------------------------------------

@pytest.mark.parametrize("stage", [1, 2, 3, 4])
def test_stage_overflow_leaves_totals_guards_and_cursors(world, gpu_device, stage):
    w = world
    ts = _batch(w, 257, salt=stage)[0] + [b"hot/1", b"hot2/x", b"xt/hot", b"hot/2"] * 8
    scratch = Pd(w)
    scratch.sh.pd = dict(w.pd.sh.pd)
    rows, totals = _oracle(w, ts, None, RR, scratch)                     # what a first call from here must pick
    assert min(totals) > 64
    with w.e.share_cursors(0) as probe:                                  # a publisher at Rem 0 for the exact-fit run
        fit = Stream(w, gpu_device, ts, None, RR, totals, probe)
        assert fit.state == 0 and (fit.h[4], fit.h[0], fit.h[1], fit.h[5]) == totals
        _check_oracle(w, ts, fit, _oracle(w, ts, None, RR, Pd(w))[0])
    caps = list(totals)
    caps[stage - 1] -= 1
    s = Stream(w, gpu_device, ts, None, RR, caps, w.ctx)                 # one short: guards checked in read()
    assert s.state == stage
    got = (s.h[4], s.h[0], s.h[1], s.h[5])
    assert got[:stage] == totals[:stage] and got[stage:] == (0,) * (4 - stage)
    assert s.h[3] == s.h[1]
    # no cursor changed: the rerun with room picks what a first call would have
    again = Stream(w, gpu_device, ts, None, RR, ROOMY, w.ctx)
    assert again.state == 0
    _check_oracle(w, ts, again, rows)
    w.pd.sh.pd = scratch.sh.pd
    _reference(w, gpu_device, ts, None, RR, ROOMY[1], ROOMY[2])          # the built-in array keeps step


# ---- 5. no host wait ----------------------------------------------------------------------------------------

def test_call_returns_while_the_stream_is_busy(world, gpu_device):
    """a 1 s device spin queued ahead on the stream: the call must come back
    while it runs (any read-back inside the call would wait for it)"""
    import torch
    from inflight_commit import raw_stream
    w = world
    ts, keys = _batch(w, 300, salt=5)
    st = raw_stream(torch, gpu_device)
    warm = Stream(w, gpu_device, ts, keys, KEYED, ROOMY, None, stream=st)       # slots and streams warmed up
    with torch.cuda.stream(st):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(st)
        torch.cuda._sleep(20_000_000)
        ev1.record(st)
    ev1.synchronize()
    per_s = 20_000_000 / (ev0.elapsed_time(ev1) / 1e3)
    for strategy, k, ctx in ((KEYED, keys, None), (RR, None, w.e.share_cursors(0))):
        s = Stream(w, gpu_device, ts, k, strategy, ROOMY, ctx, stream=st, sync=False)
        done = torch.cuda.Event()
        with torch.cuda.stream(st):
            torch.cuda._sleep(int(per_s * 1.0))
        s.call()
        done.record(st)
        returned_early = not done.query()
        st.synchronize()
        assert returned_early, "tm_publish_stream_device waited for the stream"
        s.read()
        assert s.state == 0
        if strategy == KEYED:
            assert np.array_equal(s.d, warm.d) and np.array_equal(s.p, warm.p) and s.h == warm.h
        else:
            _check_oracle(w, ts, s, _oracle(w, ts, None, RR, Pd(w))[0])
            ctx.close()


# ---- 9. the byte corpus through the new call ----------------------------------------------------------------

def test_exact_topic_sets_over_the_byte_corpus(gpu_device):
    topics = [t for t in C.stratified() if not pytrie.wildcard(t)]
    w = World(gpu_device)
    m = 0
    for i, t in enumerate(topics):
        w.route(t, ("g1", "n1"))
        if i % 2 == 0:
            k = 1 + i % 3
            w.members(b"g1", t, list(range(m, m + k)))
            m += k
    w.e.commit()
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 3 * C.DEEP_LEVELS + 1000))
    try:
        rows, totals = _oracle(w, topics, None, RR, Pd(w))
    finally:
        sys.setrecursionlimit(old)
    assert totals[3] > 100
    with w.e.share_cursors(0) as ctx:
        s = Stream(w, gpu_device, topics, None, RR, [x + 3 for x in totals], ctx, envelope=C.envelope(topics, 5))
    assert s.state == 0 and (s.h[4], s.h[0], s.h[1], s.h[5]) == totals
    for t, tp in enumerate(topics):
        got = [int(r[3]) for r in s.d[int(s.o[t]):int(s.o[t + 1])]]
        want = [Engine.NO_MEMBER if d[3] is None else d[3] for d in rows[t][0]]
        assert got == want, (t, tp[:60])
    w.close()


# ---- 6-8. the batcher ---------------------------------------------------------------------------------------

def _publish_one(b, topic, key=0):
    """submit one topic and wait for its reply, as a publisher process does"""
    got = []
    b.submit_publish(topic, key, lambda status, d, p: got.append((status, d, p)))
    b.flush()
    assert len(got) == 1 and got[0][0] == 0, got
    return got[0][1], got[0][2]


def test_batcher_one_lane_is_one_publisher(gpu_device):
    from emqx_amd.batcher import Batcher
    w = World(gpu_device)
    w.route(b"r/+", ("g", "n1"))
    w.route(b"r/#", ("h", "n2"))
    w.route(b"r/1", "n1")
    w.sub(b"r/1", 5)
    w.members(b"g", b"r/+", [1, 2, 3])
    w.members(b"h", b"r/#", [11, 12])
    w.route(b"x/t", ("g", "n1"))                                          # an exact-topic set
    w.members(b"g", b"x/t", [21, 22, 23, 24])
    w.e.commit()
    b = Batcher(w.e, max_topics=64, deadline_us=100, publish=True, round_robin=True, lanes_per_replica=1)
    pd = Pd(w)
    seq = [b"r/1", b"r/2", b"x/t", b"r/1", b"r/1/z", b"x/t", b"r/9", b"r/1", b"x/t"]

    def run(topics):
        for tp in topics:
            d, p = _publish_one(b, tp)
            want = _oracle(w, [tp], None, RR, pd)[0][0]
            assert w.got(tp, d, p) == want, tp
    run(seq)
    assert pd.sh.pd[("shared_sub_round_robin", b"g", b"r/+")] == 1        # five publishes on three members
    w.e.share_del(b"g", b"r/+", 3)                                        # the set shrinks: N >= Count is possible
    w.sh.unsubscribe(b"g", b"r/+", 3)
    w.e.share_del(b"g", b"x/t", 21)
    w.sh.unsubscribe(b"g", b"x/t", 21)
    w.e.commit()
    run(seq)
    st = b.stats()
    assert st["failed_batches"] == 0 and st["topics"] == 2 * len(seq)
    b.close()
    w.close()


def test_batcher_rerun_advances_each_cursor_once(gpu_device):
    """a first batch far past the lane's first capacities: one topic of 12
    levels matched by all 4,096 literal-or-'+' filters of its levels, each with
    a group route and three members"""
    from emqx_amd.batcher import Batcher
    w = World(gpu_device)
    lv = [b"v%d" % i for i in range(12)]
    topic = b"/".join(lv)
    fs = [b"/".join(b"+" if m >> i & 1 else lv[i] for i in range(12)) for m in range(4096)]
    gb, go = pack([b"g"] * (3 * len(fs)))
    tb, to = pack([f for f in fs for _ in range(3)])
    for f in fs:
        w.r.add_route(f, ("g", "n1"))
    w.e.share_add_many(gb, go, tb, to, [3 * i + k for i in range(len(fs)) for k in range(3)])
    w.e.commit()
    b = Batcher(w.e, max_topics=16, deadline_us=100, publish=True, round_robin=True, lanes_per_replica=1)
    index = {f: i for i, f in enumerate(fs)}
    for rnd in (0, 1):
        d, p = _publish_one(b, topic)
        assert len(d) == 4096 and p == []
        seen = set()
        for to_id, tg, nd, pk in d:
            f = topic if to_id == Engine.TOPIC_ROUTE else w.e.filter_bytes(to_id)   # the all-literal one is the topic
            seen.add(f)
            assert nd == Engine.NOT_LOCAL and pk == 3 * index[f] + rnd, (rnd, f)
        assert len(seen) == 4096
        if rnd == 0:
            assert b.stats()["reruns"] >= 1                                # it cannot have fitted the first time
    b.close()
    w.close()


def test_batcher_four_lanes_flood(world, gpu_device):
    import threading
    from emqx_amd.batcher import Batcher
    w = world
    lanes = 4
    sets = {b"hot/1": (b"gh", b"hot/#"), b"hot2/x": (b"gh", b"hot2/+"), b"xt/hot": (b"gh", b"xt/hot"),
            b"t/2": (b"g2", b"t/2"), b"c/z": (b"g1", b"c/#")}
    size = {tp: len(w.sh.tab[gt]) for tp, gt in sets.items()}
    assert sorted(size.values()) == [2, 2, 2, 3, 64]
    tps = list(sets)
    topics = [tps[i % len(tps)] for i in range(20000)]
    keys = [(i * 2654435761 + 17) % 2 ** 32 for i in range(len(topics))]

    def flood(b):
        got = [None] * len(topics)

        def producer(k):
            for t in range(k, len(topics), 8):
                def cb(status, d, p, t=t):
                    got[t] = (status, d, p) if got[t] is None else "twice"
                b.submit_publish(topics[t], keys[t], cb)
        ths = [threading.Thread(target=producer, args=(k,)) for k in range(8)]
        for x in ths:
            x.start()
        for x in ths:
            x.join()
        b.flush()
        st = b.stats()
        b.close()
        assert st["topics"] == len(topics) and st["failed_batches"] == 0
        return got

    got = flood(Batcher(w.e, max_topics=700, deadline_us=200, publish=True, round_robin=True, lanes_per_replica=lanes))
    hits = {tp: {} for tp in tps}
    for t, tp in enumerate(topics):
        status, d, p = got[t]
        assert status == 0
        grp, to = sets[tp]
        mine = [r for r in w.got(tp, d, p)[0] if r[0] == to and r[1] == (1, grp)]
        assert len(mine) == 1 and mine[0][3] in w.sh.tab[(grp, to)], (t, tp)
        hits[tp][mine[0][3]] = hits[tp].get(mine[0][3], 0) + 1
    for tp, (grp, to) in sets.items():
        per = [hits[tp].get(m, 0) for m in w.sh.tab[(grp, to)]]
        # each lane's own cursor leaves its members at most 1 apart, and the lanes' counts add
        assert sum(per) == topics.count(tp) and max(per) - min(per) <= lanes, (tp, per)
    # the keyed batcher, with and without the flag that once chose its device path, returns ticket for ticket what
    # the batch API (tm_match_publish_batch_device) gives that topic with that key
    from publish_util import slices
    bb, bo = pack(topics)
    out = slices(w.e.match_publish_batch(bb, bo, Engine.SHARE_KEYED, np.asarray(keys, dtype=np.uint32)), len(topics))
    for b in (Batcher(w.e, max_topics=700, deadline_us=200, publish=True, lanes_per_replica=lanes),
              Batcher(w.e, max_topics=700, deadline_us=200, publish=True, stream=True, lanes_per_replica=lanes)):
        got = flood(b)
        for t in range(len(topics)):
            assert got[t] == (0, out[t][0], out[t][1]), t
