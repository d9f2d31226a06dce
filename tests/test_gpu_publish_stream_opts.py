"""tm_publish_stream_opts_device and tm_publish_pack_opts_device on the GPU:
the stream-ordered publish call and the pack with the delivery words of the
local pairs and of the $share picks, against tests/pickword_ref.py and
tests/subopts_ref.py, and bit for bit against the plain calls for everything
the plain calls write.  The world is tests/pickword_world.py's.  Every output
carries guard words past its capacity, which must come back unchanged."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pickword_world import (GUARD, STRATEGIES, DevPublish, build_world, deliver_of, dev, publishes, u32)  # noqa: E402
from sticky_ref import StickySub  # noqa: E402
from emqx_amd import Engine  # noqa: E402
from emqx_amd import _lib as L  # noqa: E402
from emqx_amd.engine import pack  # noqa: E402

pytestmark = pytest.mark.gpu

G = 64
ROOMY = (20_000, 20_000, 20_000, 10_000)
NO_WORD = Engine.NO_WORD


def _filled(count, device, width=4):
    return dev(np.full(max(count, 1) * (width // 4), GUARD, dtype=np.uint32), device, np.int32)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


class Call:
    """one stream call over torch buffers, plain or with options (deliver
    given), the workspace pre-filled with the guard pattern"""

    def __init__(self, w, device, pubs, strategy, caps, cursors, deliver=None, run=True):
        import torch
        self.e, self.n, self.caps, self.opts = w.e, len(pubs), tuple(int(c) for c in caps), deliver is not None
        n = self.n
        buf, off = pack([t for t, _k, _m in pubs])
        self.d_b, self.d_o = dev(buf, device), dev(off, device, np.int64)
        self.d_k = dev(np.asarray([k for _t, k, _m in pubs] if n else [0], dtype=np.uint32), device, np.int32)
        self.nbytes = int(off[-1] - off[0])
        size = w.e.publish_stream_opts_workspace_bytes if self.opts else w.e.publish_stream_workspace_bytes
        self.ws_bytes = size(n, self.nbytes, self.caps)
        assert self.ws_bytes > 0 and self.ws_bytes % 4 == 0
        self.ws = _filled(self.ws_bytes // 4 + G, device)
        self.hdr = _filled(8 + G, device, 8)
        self.doff, self.soff = _filled(n + 1 + G, device, 8), _filled(n + 1 + G, device, 8)
        self.deliv, self.pairs = _filled(self.caps[1] + G, device, 16), _filled(self.caps[2] + G, device, 8)
        self.pkw, self.prw = _filled(self.caps[1] + G, device), _filled(self.caps[2] + G, device)
        if self.opts:
            pf, fr, fl = deliver
            self.dv = (dev(pf if n else np.zeros(1, np.uint32), device, np.int32),
                       dev(fr if n else np.zeros(1, np.uint32), device, np.int32), fl, self.prw)
        torch.cuda.synchronize()
        self.strategy, self.cursors = strategy, cursors
        if run:
            self.run()

    def run(self):
        import torch
        a = (self.d_b, self.d_o, self.n, self.nbytes, self.strategy, self.d_k, self.cursors, self.caps, self.ws,
             self.ws_bytes, self.hdr, self.doff, self.soff, self.deliv, self.pairs)
        if self.opts:
            self.e.publish_stream_opts_device(*a, self.dv, self.pkw)
        else:
            self.e.publish_stream_device(*a)
        torch.cuda.synchronize()
        n, (_, cr, cp, _) = self.n, self.caps
        hdr, doff, soff = _u64(self.hdr), _u64(self.doff), _u64(self.soff)
        deliv, pairs = u32(self.deliv).reshape(-1, 4), u32(self.pairs).reshape(-1, 2)
        g64 = np.uint64(GUARD << 32 | GUARD)
        assert (hdr[8:] == g64).all() and (doff[n + 1:] == g64).all() and (soff[n + 1:] == g64).all()
        assert (deliv[cr:] == GUARD).all() and (pairs[cp:] == GUARD).all()
        assert (u32(self.ws)[self.ws_bytes // 4:] == GUARD).all()
        self.pick_words, self.pair_words = u32(self.pkw), u32(self.prw)
        assert (self.pick_words[cr:] == GUARD).all() and (self.pair_words[cp:] == GUARD).all()
        self.h = [int(x) for x in hdr[:8]]
        self.state = self.h[6]
        self.o, self.so = doff[:n + 1].copy(), soff[:n + 1].copy()
        if self.state == 0:
            D, P = self.h[2], self.h[3]
            assert (deliv[D:] == GUARD).all() and (pairs[P:] == GUARD).all()
            assert (self.pick_words[D:] == GUARD).all() and (self.pair_words[P:] == GUARD).all()
            self.d, self.p = deliv[:D].copy(), pairs[:P].copy()
            self.pick_words, self.pair_words = self.pick_words[:D].copy(), self.pair_words[:P].copy()
        return self


def _same(a, b):
    assert a.h == b.h
    assert (a.o == b.o).all() and (a.so == b.so).all()
    assert a.d.tobytes() == b.d.tobytes() and a.p.tobytes() == b.p.tobytes()


def _fresh_pd(w):
    """a new publisher process over the world's member table"""
    sh = StickySub()
    sh.tab, sh.alive = w.sh.tab, w.sh.alive
    return sh


def _model(w, sh, strategy, pubs, upgrade):
    keep, w.sh = w.sh, sh
    try:
        return w.want(strategy, pubs, upgrade)
    finally:
        w.sh = keep


def _check_words(w, c, want, pubs, upgrade, tag):
    """the dense pick words and picks against the model, the pair words against subopts_ref"""
    for t, rows in enumerate(want):
        a, b = int(c.o[t]), int(c.o[t + 1])
        assert b - a == len(rows), (tag, t)
        for k, (m, word) in enumerate(rows):
            assert int(c.d[a + k][3]) == m and int(c.pick_words[a + k]) == word, (tag, t, k)
    for t, rows in enumerate(w.want_pairs(pubs, upgrade)):
        a, b = int(c.so[t]), int(c.so[t + 1])
        assert [(w.to_bytes(int(x[0]), pubs[t][0]), int(x[1])) for x in c.p[a:b]] == [(to, s) for to, s, _ in rows]
        assert [int(x) for x in c.pair_words[a:b]] == [wd for _to, _s, wd in rows], (tag, t)


@pytest.fixture(scope="module")
def world(gpu_device):
    w = build_world(gpu_device)
    w.e.commit()
    yield w
    w.close()


@pytest.mark.parametrize("upgrade", [False, True])
@pytest.mark.parametrize("strategy", ["keyed", "round_robin", "sticky"])
def test_stream_opts_state_0(world, gpu_device, strategy, upgrade):
    w, s = world, STRATEGIES[strategy]
    pubs = publishes(w)
    dv = deliver_of(pubs, upgrade)
    ca, cb = w.e.share_cursors(0), w.e.share_cursors(0)
    plain = Call(w, gpu_device, pubs, s, ROOMY, ca)
    opts = Call(w, gpu_device, pubs, s, ROOMY, cb, deliver=dv)
    assert plain.state == 0 == opts.state
    _same(plain, opts)
    pd = _fresh_pd(w)
    _check_words(w, opts, _model(w, pd, strategy, pubs, upgrade), pubs, upgrade, strategy)
    assert (opts.pick_words != NO_WORD).sum() == 48 and (opts.pair_words == Engine.DELIVER_DROP).sum() >= 1
    # the pair words are those of tm_match_publish_batch_opts_device
    import torch
    sdv = dev(np.full(4096, GUARD, dtype=np.uint32), gpu_device, np.int32)
    ref = _batch_opts(w, gpu_device, pubs, dv, sdv)
    torch.cuda.synchronize()
    assert (u32(sdv)[:opts.h[3]] == opts.pair_words).all() and ref == opts.h[3]
    # the state both calls left is the same: a second plain call on either context gives the same records
    pubs2 = pubs[::-1]
    p2, o2 = Call(w, gpu_device, pubs2, s, ROOMY, ca), Call(w, gpu_device, pubs2, s, ROOMY, cb)
    _same(p2, o2)
    want2 = _model(w, pd, strategy, pubs2, upgrade)
    for t, rows in enumerate(want2):
        assert [int(x[3]) for x in o2.d[int(o2.o[t]):int(o2.o[t + 1])]] == [m for m, _ in rows]
    ca.close()
    cb.close()


def _batch_opts(w, device, pubs, dv, sdv):
    """tm_match_publish_batch_opts_device (keyed: the pair words do not depend
    on the picks) writing the pair words into sdv -> the pair total"""
    import torch
    n = len(pubs)
    buf, off = pack([t for t, _k, _m in pubs])
    i32 = lambda k, fill=0: torch.full((max(k, 1),), fill, dtype=torch.int32, device=torch.device("cuda", device))  # noqa: E731,E501
    i64 = lambda k: torch.full((k,), -1, dtype=torch.int64, device=torch.device("cuda", device))   # noqa: E731
    stot = i64(1)
    pf, fr, fl = dv
    w.e.match_publish_batch_device(dev(buf, device), dev(off, device, np.int64), n, int(off[-1]), i32(n), i64(n + 1),
                                   i32(4096), i32(4096), i32(4096), 4096, i64(1), i32(n), i64(n + 1), i32(4096),
                                   i32(4096), 4096, stot, Engine.SHARE_KEYED,
                                   dev(np.asarray([k for _t, k, _m in pubs], np.uint32), device, np.int32), i32(4096),
                                   deliver=(dev(pf, device, np.int32), dev(fr, device, np.int32), fl, sdv))
    torch.cuda.synchronize()
    return int(stot.item())


@pytest.mark.parametrize("strategy", ["keyed", "round_robin", "sticky"])
def test_stream_opts_overflow(world, gpu_device, strategy):
    """each capacity one below its exact total in turn: the documented state,
    nothing in the word planes, no cursor or sticky entry moved -- the rerun
    sized from the header returns what a first full-capacity run returns"""
    w, s = world, STRATEGIES[strategy]
    pubs = publishes(w)
    dv = deliver_of(pubs, False)
    c0 = w.e.share_cursors(0)
    full = Call(w, gpu_device, pubs, s, ROOMY, c0, deliver=dv)
    assert full.state == 0
    exact = (full.h[4], full.h[0], full.h[1], full.h[5])     # ids, routes, pairs, ranked slots
    stages = 3 if strategy == "keyed" else 4                 # keyed picks rank nothing: caps.rr is ignored
    assert all(x > 0 for x in exact[:stages]), exact
    for stage in range(stages):
        caps = list(exact)
        caps[stage] -= 1
        ctx = w.e.share_cursors(0)
        short = Call(w, gpu_device, pubs, s, caps, ctx, deliver=dv)
        assert short.state == stage + 1, (stage, short.h)
        assert short.h[(4, 0, 1, 5)[stage]] == exact[stage]
        # (the guards past caps.routes / caps.pairs words were checked by the call itself)
        assert (short.pick_words == GUARD).all()
        assert stage == 3 or (short.pair_words == GUARD).all()   # state 4 is found after the emit ran
        rerun = Call(w, gpu_device, pubs, s, exact, ctx, deliver=dv)
        assert rerun.state == 0
        _same(full, rerun)
        assert (rerun.pick_words == full.pick_words).all() and (rerun.pair_words == full.pair_words).all()
        ctx.close()
    c0.close()


def test_stream_opts_empty_batch_and_arguments(world, gpu_device):
    w = world
    c = Call(w, gpu_device, [], Engine.SHARE_KEYED, (8, 8, 8, 8), None, deliver=(np.zeros(0, np.uint32),
                                                                                 np.zeros(0, np.uint32), 0))
    assert c.h == [0] * 8 and int(c.o[0]) == 0 == int(c.so[0])
    assert (c.pick_words == GUARD).all() and (c.pair_words == GUARD).all()
    pubs = publishes(w)[:4]
    dv = deliver_of(pubs, False)
    ok = Call(w, gpu_device, pubs, Engine.SHARE_KEYED, ROOMY, None, deliver=dv, run=False)
    a = (ok.d_b, ok.d_o, ok.n, ok.nbytes, ok.strategy, ok.d_k, None, ok.caps, ok.ws, ok.ws_bytes, ok.hdr, ok.doff,
         ok.soff, ok.deliv, ok.pairs)
    for bad_dv, pkw in ((None, ok.pkw), ((None, ok.dv[1], 0, ok.prw), ok.pkw), ((ok.dv[0], None, 0, None), ok.pkw),
                        ((ok.dv[0], None, 2, ok.prw), ok.pkw), (ok.dv, None)):
        with pytest.raises(L.TopicMatchError):
            w.e.publish_stream_opts_device(*a, bad_dv, pkw)
    # the plain call's workspace is too small for the call with options, and its size is what it was
    keyed_caps = ROOMY[:3] + (0,)                             # a keyed call ignores caps.rr
    plain_bytes = w.e.publish_stream_workspace_bytes(ok.n, ok.nbytes, keyed_caps)
    assert plain_bytes < w.e.publish_stream_opts_workspace_bytes(ok.n, ok.nbytes, keyed_caps) <= ok.ws_bytes
    with pytest.raises(L.TopicMatchError):
        w.e.publish_stream_opts_device(*a[:9], plain_bytes, *a[10:], ok.dv, ok.pkw)
    ok.run()
    assert ok.state == 0


def test_pack_with_words(world, gpu_device):
    import torch
    w = world
    pubs = publishes(w)
    dv = deliver_of(pubs, True)
    want = w.want("keyed", pubs, True)
    d = DevPublish(w.e, gpu_device, pubs, Engine.SHARE_KEYED, 1024, 1024)
    slot_words = d.words(dv)
    sdv = dev(np.full(1024 + 8, GUARD, dtype=np.uint32), gpu_device, np.int32)
    P = _batch_opts(w, gpu_device, pubs, dv, sdv)
    total, D = int(d.tot.item()), int(u32(d.c).sum())
    assert int(d.stot.item()) == P

    def run(deliv_cap, pair_cap):
        hdr, doff = _filled(4 + G, gpu_device, 8), _filled(d.n + 1 + G, gpu_device, 8)
        deliv, pairs = _filled(deliv_cap + G, gpu_device, 16), _filled(pair_cap + G, gpu_device, 8)
        pkw, prw = _filled(deliv_cap + G, gpu_device), _filled(pair_cap + G, gpu_device)
        torch.cuda.synchronize()
        w.e.publish_pack_opts(d.n, d.c, d.o, d.to, d.tg, d.nd, d.pk, d.cap, d.tot, d.so, d.sto, d.sid, d.scap, d.stot,
                              hdr, doff, deliv, deliv_cap, pairs, pair_cap, sdv, slot_words, prw, pkw)
        torch.cuda.synchronize()
        return ([int(x) for x in _u64(hdr)[:4]], _u64(doff)[:d.n + 1], u32(deliv).reshape(-1, 4), u32(pairs).reshape(-1, 2),
                u32(pkw), u32(prw))

    hdr, doff, deliv, pairs, pkw, prw = run(D + 5, P + 5)
    assert hdr == [total, P, D, P]
    # the dense pick words are the slot plane with the holes removed, the pair words the input plane
    sw, o, c = u32(slot_words), u32(d.o).view(np.uint64), u32(d.c)
    dense = np.concatenate([sw[int(o[t]):int(o[t]) + int(c[t])] for t in range(d.n)])
    assert (pkw[:D] == dense).all() and (pkw[D:] == GUARD).all()
    assert (prw[:P] == u32(sdv)[:P]).all() and (prw[P:] == GUARD).all()
    for t, rows in enumerate(want):
        assert [int(x) for x in pkw[int(doff[t]):int(doff[t + 1])]] == [wd for _m, wd in rows]
        assert [int(x[3]) for x in deliv[int(doff[t]):int(doff[t + 1])]] == [m for m, _ in rows]
    # capacities below the need: nothing at or past them, the header exact
    hdr, doff2, deliv, pairs, pkw, prw = run(D - 7, P - 3)
    assert hdr == [total, P, D, P] and (doff2 == doff).all()
    assert (pkw[D - 7:] == GUARD).all() and (prw[P - 3:] == GUARD).all()
    assert (deliv[D - 7:] == GUARD).all() and (pairs[P - 3:] == GUARD).all()


# ---- the micro-batcher with TM_BATCHER_OPTS ------------------------------------------------------------------

def _submit_all(b, pubs, threads=2):
    """single-topic options submits from `threads` threads -> per publish
    (status, deliveries, pick_words, pairs, pair_words)"""
    import threading
    got = [None] * len(pubs)

    def work(lo):
        for i in range(lo, len(pubs), threads):
            topic, key, msg = pubs[i]
            pf, fr = (msg[0] | (4 if msg[1] else 0) | (8 if msg[2] else 0),
                      Engine.NO_SUBSCRIBER if msg[3] is None else msg[3])
            b.submit_publish_opts(topic, key, pf, fr, lambda *a, i=i: got.__setitem__(i, a))
    ts = [threading.Thread(target=work, args=(k,)) for k in range(threads)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    b.flush()
    return got


def _check_callbacks(w, pubs, got, strategy, upgrade):
    """every callback against the model for its publish's message: the
    records and the pairs with their words; a keyed pick is the model's, a
    round-robin or sticky pick (which depends on the lane and the order the
    submits were gathered in) is a member of its set, and its word is the
    model's for that member"""
    from pickword_ref import outcome_word, pick_outcome
    want_pairs = w.want_pairs(pubs, upgrade)
    picks = 0
    for i, (topic, key, msg) in enumerate(pubs):
        status, deliv, pick_words, pairs, pair_words = got[i]
        assert status == 0, (i, status)
        dels = w.o.match_deliveries(topic)
        assert len(deliv) == len(dels) == len(pick_words), (i, topic)
        for (to_id, tg, nd, pk), word, (to, (kind, x)) in zip(deliv, pick_words, dels):
            assert w.to_bytes(to_id, topic) == to and w.e.target_bytes(tg)[1] == x
            if kind != 1:
                assert pk == Engine.NO_MEMBER and word == NO_WORD
                continue
            members = w.sh.subscribers(x, to)
            assert pk in members, (i, topic)
            if strategy == "keyed":
                assert pk == members[key % len(members)]
            assert word == outcome_word(pick_outcome(w.so, w.sh, x, to, pk, msg, upgrade)), (i, topic, pk)
            picks += 1
        assert [(w.to_bytes(t, topic), s) for t, s in pairs] == [(to, s) for to, s, _ in want_pairs[i]]
        assert pair_words == [wd for _to, _s, wd in want_pairs[i]], (i, topic)
    return picks


@pytest.mark.parametrize("strategy,upgrade", [("keyed", False), ("round_robin", True), ("sticky", False)])
def test_batcher_opts(world, strategy, upgrade):
    from emqx_amd.batcher import Batcher
    w = world
    base = publishes(w)
    pubs = [base[(7 * i) % len(base)] for i in range(200)]
    b = Batcher(w.e, max_topics=48, deadline_us=100, publish=True, opts=True, upgrade_qos=upgrade,
                round_robin=strategy == "round_robin", sticky=strategy == "sticky")
    got = _submit_all(b, pubs)
    st = b.stats()
    assert st["failed_batches"] == 0 and st["topics"] == 200 and st["batches"] >= 2
    assert _check_callbacks(w, pubs, got, strategy, upgrade) >= 100
    # the plain submits are refused, nothing queued
    with pytest.raises(L.TopicMatchError):
        b.submit_publish(b"a", 1, lambda *a: None)
    with pytest.raises(L.TopicMatchError):
        b.submit(b"a", lambda *a: None)
    b.flush()
    assert b.stats()["topics"] == 200
    b.close()


def test_batcher_opts_first_batch_is_rerun(gpu_device):
    """tiny first capacities (a one-topic batch: 1,044 pairs), then one topic
    with a 1,500-subscriber bag: the stream call reports state 3, the batch
    runs again at the capacity the header names, and the words are right"""
    from emqx_amd.batcher import Batcher
    import random
    w = build_world(gpu_device)
    rng = random.Random(3)
    w.route(b"bag/of/many", "n1")
    for s in range(1500):
        w.plain(b"bag/of/many", 50000 + s, None if s % 5 == 4 else
                {"qos": rng.randrange(3), "nl": s % 2, "rap": rng.randrange(2), "subid": 1 + s % 9})
    w.e.commit()
    pubs = [(b"bag/of/many", 5, (2, 1, 0, 50001))]
    b = Batcher(w.e, max_topics=4, deadline_us=100, publish=True, opts=True, lanes_per_replica=1)
    got = _submit_all(b, pubs, threads=1)
    st = b.stats()
    assert st["reruns"] > 0 and st["failed_batches"] == 0 and st["batches"] == 1
    _check_callbacks(w, pubs, got, "keyed", False)
    assert len(got[0][3]) == 1500 and got[0][4].count(Engine.DELIVER_DROP) == 1
    # and the batches after it, which find the capacities grown
    more = publishes(w)[:40] + pubs
    got = _submit_all(b, more)
    assert _check_callbacks(w, more, got, "keyed", False) >= 20
    b.close()
    w.close()


def test_batcher_opts_batch_past_the_read_back_threshold(world):
    """one batch of more than 32768 topics: the header comes back first, then
    exactly D records, P pairs and their two word planes"""
    from emqx_amd.batcher import Batcher
    w = world
    base = publishes(w)
    kinds = [base[0], base[5], base[-1], base[-4], (b"nothing/at/all", 1, (1, 0, 0, None))]
    pubs = [kinds[i % len(kinds)] for i in range(33_000)]
    b = Batcher(w.e, max_topics=40_000, deadline_us=5_000_000, publish=True, opts=True, lanes_per_replica=1)
    got = _submit_all(b, pubs)
    st = b.stats()
    b.close()
    assert st["batches"] == 1 and st["max_batch"] == 33_000 and st["failed_batches"] == 0
    _check_callbacks(w, pubs[:len(kinds)], got[:len(kinds)], "keyed", False)
    for i, g in enumerate(got):                               # every publish of a kind got that kind's answer
        assert g == got[i % len(kinds)], i
