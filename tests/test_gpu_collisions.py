"""The forced hash collisions of tests/collision_corpus.py through every device
path that turns topic bytes into an identity: hash, probe, then verify the
bytes.  Every other GPU test only ever runs the "bytes equal" side of the
verify; here every stored key has a partner with the same dictionary tag and
home slot (or the same 64-bit hash and length), so a lookup that accepted
the first slot with a matching tag or hash returns the partner's id.

    kernels.hip     dict_end       tm_tokenize per lane (tok_wave 0) and tm_match_small
                    wave_dict_end  tm_tokenize's wave path (tok_wave 1)
    device_bytes.h  exact_find     routes.hip, dispatch.hip and share.hip

Everything is compared element for element and in order with the CPU oracles
(oracle.O1; oracle.pytrie.RouteTable, tests/dispatch_ref.py and
tests/shared_ref.py); a failure names the first differing topic by repr and
its collision class, which is the branch that should have rejected it."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import byte_corpus as C  # noqa: E402
import collision_corpus as K  # noqa: E402
from dispatch_ref import route_dispatch  # noqa: E402
from emqx_amd import Engine, pack  # noqa: E402

pytestmark = pytest.mark.gpu


def _fail(tag, i, rows, got, want):
    cls, absent, t = rows[i]
    raise AssertionError("%s: topic %d %r (class %s%s): got %s want %s"
                         % (tag, i, t, cls, ", absent" if absent else "", got, want))


def _check_csr(tag, rows, got, want):
    """got / want: (counts, offsets, ids); names the first topic whose list differs"""
    gc, go, gi = got
    wc, wo, wi = want
    for i in range(len(rows)):
        a = gi[int(go[i]):int(go[i]) + int(gc[i])]
        b = wi[int(wo[i]):int(wo[i]) + int(wc[i])]
        if len(a) != len(b) or not np.array_equal(a, b):
            _fail(tag, i, rows, a.tolist(), b.tolist())
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), tag


# ---- the dictionary: filters, batches and O1's lists, computed once --------------------------

class _Ref:
    def __init__(self, reverse):
        from oracle import O1
        self.fs = K.filters(reverse)
        self.fb, self.fo = pack(self.fs)
        wild = {i for i, f in enumerate(self.fs) if f in K.WILD}
        o1 = O1(len(self.fs))
        o1.insert_many(self.fb, self.fo)
        self.batches, self.want = K.batches(), {}
        for name, rows in self.batches:
            tb, to = pack([t for _, _, t in rows])
            oc, oo, oi = self.want[name] = o1.match_ids(tb, to, threads=4)
            for i, (cls, absent, t) in enumerate(rows):
                ids = set(oi[int(oo[i]):int(oo[i + 1])].tolist())
                assert ids and (ids <= wild if absent else ids - wild), (cls, t)   # (pinned on the CPU too)
        o1.close()


@pytest.fixture(scope="module")
def ref():
    return _Ref(False)


def _engine(device, r):
    e = Engine(device=device)
    e.insert_many(r.fb, r.fo)
    e.commit()
    return e


@pytest.fixture(scope="module")
def eng(gpu_device, ref):
    e = _engine(gpu_device, ref)
    yield e
    e.close()


def _host_entry(e, r, tok_wave):
    from test_gpu_bytes import _options
    _options(e, tok_wave, None)
    try:
        for name, rows in r.batches:
            tb, to = pack([t for _, _, t in rows])
            want = r.want[name]
            _check_csr("%s owned, tok_wave %d" % (name, tok_wave), rows, e.match_batch(tb, to), want)
            cap = int(want[1][-1]) + 7
            _check_csr("%s out_cap, tok_wave %d" % (name, tok_wave), rows, e.match_batch(tb, to, out_cap=cap), want)
    finally:
        _options(e, 1, None)


@pytest.mark.parametrize("tok_wave", [1, 0])                 # wave_dict_end / dict_end
def test_tokenizer_rejects_colliding_words(eng, ref, tok_wave):
    _host_entry(eng, ref, tok_wave)


@pytest.mark.parametrize("tok_wave", [1, 0])
def test_tokenizer_with_the_partners_inserted_in_reverse(gpu_device, tok_wave):
    """the partners of every group interned in the opposite order: the wanted
    word now sits in the second slot of the run where it sat in the first"""
    r = _Ref(True)
    e = _engine(gpu_device, r)
    try:
        _host_entry(e, r, tok_wave)
    finally:
        e.close()


@pytest.mark.parametrize("lead", [0, 5])
@pytest.mark.parametrize("tok_wave", [1, 0])
def test_device_entry_in_an_envelope(eng, ref, gpu_device, lead, tok_wave):
    from test_gpu_bytes import _device_csr, _options
    _options(eng, tok_wave, None)
    try:
        for name, rows in ref.batches:
            buf, off = C.envelope([t for _, _, t in rows], lead)
            _check_csr("%s lead %d, tok_wave %d" % (name, lead, tok_wave), rows,
                       _device_csr(eng, buf, off, gpu_device), ref.want[name])
    finally:
        _options(eng, 1, None)


@pytest.mark.parametrize("lead", [0, 5])
def test_small_path_in_an_envelope(eng, ref, gpu_device, lead):
    """tm_match_small: tokenize_one over global bytes (dict_end)"""
    from test_gpu_small import _check, _small
    for name, rows in ref.batches:
        buf, off = C.envelope([t for _, _, t in rows], lead)
        oc, oo, oi = ref.want[name]
        c, o, ids, total = _small(eng, buf, off, cap=int(oo[-1]) + 64, dev=gpu_device)
        for i in range(len(rows)):
            a, b = ids[int(o[i]):int(o[i]) + int(c[i])], oi[int(oo[i]):int(oo[i + 1])]
            if not np.array_equal(a, b):
                _fail("small %s lead %d" % (name, lead), i, rows, a.tolist(), b.tolist())
        _check(c, o, ids, total, oc, oo, oi)


# ---- the exact-topic tables ----------------------------------------------------------------------

def _dev(x, dev, dtype=None):
    import torch
    a = np.ascontiguousarray(x)
    return torch.from_numpy(a.view(dtype).copy() if dtype else a.copy()).to(torch.device("cuda", dev))


def _full(n, dev, dtype, fill=-1):
    import torch
    return torch.full((max(n, 1),), fill, dtype=dtype, device=torch.device("cuda", dev))


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _rows_equal(tag, rows, counts, offs, cols, wcounts, woffs, wcols):
    """two outputs in (counts, offsets, parallel columns) form, topic by topic"""
    for i in range(len(rows)):
        a, b = int(offs[i]), int(woffs[i])
        got = [c[a:a + int(counts[i])].tolist() for c in cols]
        want = [c[b:b + int(wcounts[i])].tolist() for c in wcols]
        if got != want:
            _fail(tag, i, rows, got, want)


OUTSIDE = b"outside/the/corpus"


class _Exact:
    """routes, plain and $share subscribers and share members on every stored
    topic of the given exact groups, numbered so that a wrong slot shows; the
    absent topic of each group is published with them and owns nothing.
    fillers: that many more stored topics, never published: upload_table
    (engine.cpp) scatters a commit's dirty slots only while they are under
    about 2/9 of a table of 32 B slots and copies the whole table otherwise,
    so the delete of ~20 run heads (a few shifted slots each) reaches an
    image as a delta only in a table of about a thousand slots"""

    def __init__(self, device, groups, root_wildcard, fillers=0):
        from test_gpu_shared import World
        self.w = w = World(device)
        w.e.set_option("double_buffer", 1)
        self.groups = groups
        self.num = {}
        self.epoch = None
        self.touched = False
        self.rows = [(g.cls, t == g.absent, t) for g in groups for t in K.strings(g)]   # partners side by side
        self.topics = [t for _, _, t in self.rows]
        self.keys = [(2654435761 * (i + 1)) % 2 ** 32 for i in range(len(self.topics))]
        if root_wildcard:                                    # something every topic matches besides its own key
            w.route(b"#", "n1")
            w.route(b"#", ("g1", "n1"))
            w.e.sub_add(b"#", 7)
            w.bag.insert_subscriber(None, b"#", 7)
            w.members(b"g1", b"#", [8, 9])
        for g in groups:
            for t in g.members:
                self.add(t)
        for i in range(fillers):
            self.add(b"fill/%d" % i)

    def touch(self):
        """one small delta on a topic no corpus topic matches or equals (a
        plain subscriber added, the next time deleted): no answer changes, but
        the next commit is a real one -- a commit with nothing to publish
        returns early, without writing or flipping an image"""
        w = self.w
        if self.touched:
            assert w.e.sub_del(OUTSIDE, 999999) == w.bag.delete_object(None, OUTSIDE, 999999)
        else:
            w.e.sub_add(OUTSIDE, 999999)
            w.bag.insert_subscriber(None, OUTSIDE, 999999)
        self.touched = not self.touched

    def add(self, t):
        w, i = self.w, self.num.setdefault(t, len(self.num))
        for d in ("n1", "n2", ("g1", "n1"), ("g%d" % (2 + i % 2), "n2")):
            w.route(t, d)
        for s, g in ((10 * i + 1, None), (10 * i + 2, "g1"), (10 * i + 3, None)):
            w.e.sub_add(t, s, g.encode() if g else None)
            w.bag.insert_subscriber(g, t, s)
        w.members(b"g1", t, [100 * i + 1, 100 * i + 2, 100 * i + 3][:1 + i % 3])
        w.members(b"g%d" % (2 + i % 2), t, [100 * i + 50])

    def drop(self, t):
        w, i = self.w, self.num[t]
        for d in ("n1", "n2", ("g1", "n1"), ("g%d" % (2 + i % 2), "n2")):
            w.route(t, d, add=False)
        for s, g in ((10 * i + 1, None), (10 * i + 2, "g1"), (10 * i + 3, None)):
            assert w.e.sub_del(t, s, g.encode() if g else None) == w.bag.delete_object(g, t, s)
        for m in [100 * i + 1, 100 * i + 2, 100 * i + 3][:1 + i % 3]:
            w.member(b"g1", t, m, add=False)
        w.member(b"g%d" % (2 + i % 2), t, 100 * i + 50, add=False)

    def check(self, tag, device):
        from shared_ref import NO_MEMBER
        from test_gpu_shared import _device_publish, _want
        w, e, rows, ts = self.w, self.w.e, self.rows, self.topics
        self.touch()
        ep = e.commit()
        # written and flipped: the image that missed the previous commit is the live one now
        assert self.epoch is None or ep == self.epoch + 1, (tag, ep, self.epoch)
        self.epoch = ep
        e.debug_check_routes()
        e.debug_check_subs()
        e.debug_check_shares()
        stored = {t for g in self.groups for t in g.members if w.o.get_routes(t)}
        # the oracles, and what the absent topics must not get: anything of a literal topic's own
        want_r = [w.o.match_routes(t) for t in ts]
        want_d = [w.o.match_deliveries(t) for t in ts]
        for (cls, absent, t), r in zip(rows, want_r):
            own = [x for x in r if x[0] == t]
            assert (len(own) == 4) == (t in stored) and (own == [] or t in stored), (tag, cls, t)
        # match_routes_batch, match_deliveries_batch
        got_r = w.r.match_routes_many(ts)
        got_d = w.r.match_deliveries_many(ts, tagged=True)
        for i, t in enumerate(ts):
            if [(x.topic, x.dest) for x in got_r[i]] != want_r[i]:
                _fail("%s: routes" % tag, i, rows, got_r[i], want_r[i])
            if got_d[i] != want_d[i]:
                _fail("%s: deliveries" % tag, i, rows, got_d[i], want_d[i])
        # match_dispatch_batch
        pubs = w.b.publish_many(ts)
        for i, (t, pub) in enumerate(zip(ts, pubs)):
            counts, pairs = route_dispatch(w.o, w.bag, b"n1", t)
            got = ([(d.to, d.target) for d in pub.deliveries], [d.count for d in pub.deliveries], pub.pairs)
            if got != (want_d[i], counts, pairs):
                _fail("%s: dispatch" % tag, i, rows, got, (want_d[i], counts, pairs))
        # dispatch_batch by To bytes
        for i, (t, (count, subs)) in enumerate(zip(ts, w.b.dispatch_many(ts))):
            bag = w.bag.subscribers(t)
            want = (len(bag), [x for x in bag if not isinstance(x, tuple)])
            if (count, subs) != want:
                _fail("%s: dispatch by To" % tag, i, rows, (count, subs), want)
            assert bool(bag) == (t in stored)
        # match_publish_batch, keyed
        want_p = _want(w, ts, "keyed", self.keys)
        shared = w.b.publish_shared_many(ts, "keyed", self.keys)
        for i, (pub, pl) in enumerate(zip(shared, pubs)):
            if pub.picks != want_p[i] or pub.deliveries != pl.deliveries or pub.pairs != pl.pairs:
                _fail("%s: publish" % tag, i, rows, pub.picks, want_p[i])
        assert sum(1 for row in want_p for _, _, m in row if m is not NO_MEMBER) >= len(stored)
        # the device entries in the off[0] = 5 envelope, '/' all around: raw output equal to the host entries'
        import torch
        n = len(ts)
        hb, ho = pack(ts)
        buf, off = C.envelope(ts, 5)
        d_b, d_o, nbytes = _dev(buf, device), _dev(off, device, np.int64), int(off[-1] - off[0])
        hc, hoff, hsrc, hdst = e.match_routes_batch(hb, ho)
        cap = len(hsrc) + 5
        c, o, tot = _full(n, device, torch.int32), _full(n + 1, device, torch.int64), _full(1, device, torch.int64)
        a, b = _full(cap, device, torch.int32), _full(cap, device, torch.int32)
        torch.cuda.synchronize()
        e.match_routes_batch_device(d_b, d_o, n, nbytes, c, o, a, b, cap, tot)
        torch.cuda.synchronize()
        assert int(tot.item()) == cap - 5
        _rows_equal("%s: routes, device entry" % tag, rows, _u32(c), o.cpu().numpy(), [_u32(a), _u32(b)],
                    hc, hoff, [hsrc, hdst])
        hd = e.match_dispatch_batch(hb, ho)
        cap, scap = len(hd[2]) + 5, len(hd[7]) + 5
        c, o, tot = _full(n, device, torch.int32), _full(n + 1, device, torch.int64), _full(1, device, torch.int64)
        to, tg, nd = (_full(cap, device, torch.int32) for _ in range(3))
        sc, so, stot = _full(n, device, torch.int32), _full(n + 1, device, torch.int64), _full(1, device, torch.int64)
        sto, sid = _full(scap, device, torch.int32), _full(scap, device, torch.int32)
        torch.cuda.synchronize()
        e.match_dispatch_batch_device(d_b, d_o, n, nbytes, c, o, to, tg, nd, cap, tot, sc, so, sto, sid, scap, stot)
        torch.cuda.synchronize()
        assert int(tot.item()) == cap - 5 and int(stot.item()) == scap - 5
        _rows_equal("%s: dispatch, device entry" % tag, rows, _u32(c), o.cpu().numpy(), [_u32(to), _u32(tg), _u32(nd)],
                    hd[0], hd[1], [hd[2], hd[3], hd[4]])
        _rows_equal("%s: dispatch pairs, device entry" % tag, rows, _u32(sc), so.cpu().numpy(), [_u32(sto), _u32(sid)],
                    hd[5], hd[6], [hd[7], hd[8]])
        hp = e.match_publish_batch(hb, ho, Engine.SHARE_KEYED, self.keys)
        c, o, to, tg, nd, pk, tot = _device_publish(e, device, buf, off, Engine.SHARE_KEYED, self.keys,
                                                    len(hp[2]) + 5, len(hp[7]) + 5)
        assert tot == len(hp[2])
        _rows_equal("%s: publish, device entry" % tag, rows, c, o, [to, tg, nd, pk], hp[0], hp[1],
                    [hp[2], hp[3], hp[4], hp[9]])


@pytest.mark.parametrize("world", ["all", "wrap16"])
def test_exact_tables_reject_equal_hash_topics(gpu_device, world):
    """all: every exact group among 400 filler topics, in tables of 1024 slots.
    wrap16: two E-wrap triples alone, six keys of home 15 in tables of 16
    slots: the run wraps the table's end, on the device as on the host (a
    table that small is always copied whole, see _Exact).

    Every check commits after one small delta outside the corpus, so each
    commit writes the image epoch that missed the previous one and flips to
    it.  Built: both images written in full.  Then the first member of every
    group is deleted (the run shifts back over its partners): one image takes
    the delete as this commit's delta and is checked, then the other takes it
    from the previous commit's dirty log and is checked in the same
    delete-only state.  The re-add goes through both images the same way."""
    if world == "all":
        x = _Exact(gpu_device, K.exact_groups(), True, fillers=400)
    else:
        x = _Exact(gpu_device, K.groups()["E-wrap"][:2], False)
    try:
        x.check("built, first image", gpu_device)
        x.check("built, second image", gpu_device)
        for g in x.groups:
            x.drop(g.members[0])
        x.check("first members deleted, this commit's delta", gpu_device)
        x.check("first members deleted, the previous commit's delta", gpu_device)
        for g in x.groups:
            x.add(g.members[0])
        x.check("re-added, this commit's delta", gpu_device)
        x.check("re-added, the previous commit's delta", gpu_device)
    finally:
        x.w.close()
