"""tm_publish_stream_gated_device on the GPU: the stream-ordered publish call
behind an admission verdict.  A refused publish leaves no trace from the route
stage on: everything the gated call leaves equals what the existing call
leaves for the batch with the refused topics removed.

Two checks per case: the existing ungated call on the compacted batch with a
cursor context of its own (bit for bit, cursors included), and the oracles
(tests/shared_ref.py, tests/dispatch_ref.py, oracle/pytrie.py) applied to the
admitted topics only.  The world is tests/test_gpu_publish_stream.py's, plus
the 512 nine-level filters of every '+' / literal combination of
big/1/2/3/4/5/6/7/8 and '#' tails, so that one topic matches more than one
256-id chunk of tm_route_emit's loop.  Every call runs with 64 guard elements
after each output and after the (pre-filled) workspace."""
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from publish_util import GUARD  # noqa: E402
from test_gpu_publish_stream import Pd, _batch, _build, _check_oracle, _filled, _oracle  # noqa: E402
from emqx_amd import Engine  # noqa: E402
from emqx_amd.engine import pack  # noqa: E402

pytestmark = pytest.mark.gpu

G = 64
KEYED, RR, STICKY = Engine.SHARE_KEYED, Engine.SHARE_ROUND_ROBIN, Engine.SHARE_STICKY
STRATEGY = {"keyed": KEYED, "round_robin": RR, "sticky": STICKY}
ROOMY = (60_000, 60_000, 60_000, 20_000)
BIG = b"big/1/2/3/4/5/6/7/8"
PICK = 0x80000000


@pytest.fixture(scope="module")
def world(gpu_device):
    w = _build(gpu_device)
    lv = BIG.split(b"/")
    n = 0
    for i, mask in enumerate(itertools.product((False, True), repeat=9)):
        f = b"/".join(b"+" if m else x for m, x in zip(mask, lv))
        w.route(f, "n2" if i % 5 == 0 else "n1")
        n += 1
        if i % 16 == 0:
            w.sub(f, 20000 + i)
    for k in (1, 3, 8):                                        # '#' tails
        f = b"/".join(lv[:k]) + b"/#"
        w.route(f, "n1")
        w.sub(f, 21000 + k)
        n += 1
    w.route(b"big/#", ("gb", "n1"))
    w.members(b"gb", b"big/#", [9501, 9502, 9503])
    w.e.commit()
    assert len(w.o.trie.match(BIG)) >= 300 and n >= 512
    yield w
    w.ctx.close()
    w.close()


class Call:
    """one stream call over torch buffers: the existing plain / options call
    (code=None, gated=False) or the gated one, guards included"""

    def __init__(self, w, dev, topics, keys, strategy, caps, cursors, opts=False, code=None, gated=True, flags=None):
        import torch
        self.w, self.n, self.caps, self.opts = w, len(topics), tuple(int(c) for c in caps), opts
        n = self.n
        buf, off = pack(topics)
        tdev = torch.device("cuda", dev)
        up = lambda a, v=None: torch.from_numpy((np.ascontiguousarray(a).view(v) if v else a).copy()).to(tdev)  # noqa: E731,E501
        self.d_b, self.d_o = up(buf if len(buf) else np.zeros(1, np.uint8)), up(off, np.int64)
        self.d_k = None if keys is None else up(np.asarray(keys if n else [0], dtype=np.uint32), np.int32)
        self.nbytes = int(off[-1] - off[0])
        size = w.e.publish_stream_opts_workspace_bytes if opts else w.e.publish_stream_workspace_bytes
        self.ws_bytes = size(n, self.nbytes, self.caps)
        assert self.ws_bytes > 0 and self.ws_bytes % 4 == 0
        self.ws = _filled(self.ws_bytes // 4 + G, dev)
        self.hdr = _filled(8 + G, dev, 8)
        self.doff, self.soff = _filled(n + 1 + G, dev, 8), _filled(n + 1 + G, dev, 8)
        self.deliv, self.pairs = _filled(self.caps[1] + G, dev, 16), _filled(self.caps[2] + G, dev, 8)
        self.pkw, self.prw = _filled(self.caps[1] + G, dev), _filled(self.caps[2] + G, dev)
        self.dv = None
        if opts:
            if flags is None:
                flags = [(i % 3) | (4 if i % 5 == 0 else 0) for i in range(n)]
            pf = np.asarray(list(flags) or [0], dtype=np.uint32)
            fr = np.asarray([100 + i % 7 for i in range(n)] or [0], dtype=np.uint32)
            self.dv = (up(pf, np.int32), up(fr, np.int32), 0, self.prw)
        self.d_code = None if code is None else up(np.asarray(code if n else [0], dtype=np.uint8))
        self.strategy, self.cursors, self.gated = strategy, cursors, gated
        torch.cuda.synchronize()
        self.run()

    def run(self):
        import torch
        a = (self.d_b, self.d_o, self.n, self.nbytes, self.strategy, self.d_k, self.cursors, self.caps, self.ws,
             self.ws_bytes, self.hdr, self.doff, self.soff, self.deliv, self.pairs)
        if self.gated:
            self.w.e.publish_stream_gated_device(*a, self.dv, self.pkw if self.opts else None, self.d_code)
        elif self.opts:
            self.w.e.publish_stream_opts_device(*a, self.dv, self.pkw)
        else:
            self.w.e.publish_stream_device(*a)
        torch.cuda.synchronize()
        u32 = lambda t: t.cpu().numpy().view(np.uint32)      # noqa: E731
        u64 = lambda t: t.cpu().numpy().view(np.uint64)      # noqa: E731
        n, (_, cr, cp, _) = self.n, self.caps
        hdr, doff, soff = u64(self.hdr), u64(self.doff), u64(self.soff)
        deliv, pairs, ws = u32(self.deliv).reshape(-1, 4), u32(self.pairs).reshape(-1, 2), u32(self.ws)
        pkw, prw = u32(self.pkw), u32(self.prw)
        g64 = np.uint64(GUARD << 32 | GUARD)
        assert (hdr[8:] == g64).all() and (doff[n + 1:] == g64).all() and (soff[n + 1:] == g64).all()
        assert (deliv[cr:] == GUARD).all() and (pairs[cp:] == GUARD).all()
        assert (pkw[cr:] == GUARD).all() and (prw[cp:] == GUARD).all()
        assert (ws[self.ws_bytes // 4:] == GUARD).all() and len(ws) == self.ws_bytes // 4 + G
        self.h = [int(x) for x in hdr[:8]]
        self.state = self.h[6]
        assert self.h[7] == 0
        self.o, self.so = doff[:n + 1].copy(), soff[:n + 1].copy()
        if self.state == 0:
            D, P = self.h[2], self.h[3]
            assert (deliv[D:cr] == GUARD).all() and (pairs[P:cp] == GUARD).all()
            self.d, self.p = deliv[:D].copy(), pairs[:P].copy()
            if self.opts:
                assert (pkw[D:] == GUARD).all() and (prw[P:] == GUARD).all()
                self.pick_words, self.pair_words = pkw[:D].copy(), prw[:P].copy()
            else:
                assert (pkw == GUARD).all() and (prw == GUARD).all()
        return self


def _keep(xs, code):
    return [x for x, c in zip(xs, code) if not c]


def _compact(off, code):
    """an offset array with the refused topics' entries deleted"""
    return np.array([off[0]] + [off[t + 1] for t in range(len(code)) if not code[t]], dtype=np.uint64)


def _equal_compacted(g, c, code, ids=None):
    """gated call g over the whole batch == existing call c over the admitted topics"""
    assert g.state == 0 == c.state
    assert g.h[:4] == c.h[:4] and g.h[5] == c.h[5]
    if ids is not None:
        assert g.h[4] == ids                         # stage 1 is ungated: the refused topics' ids count
    for t, r in enumerate(code):
        if r:
            assert g.o[t + 1] == g.o[t] and g.so[t + 1] == g.so[t], t
    assert np.array_equal(_compact(g.o, code), c.o) and np.array_equal(_compact(g.so, code), c.so)
    assert g.d.tobytes() == c.d.tobytes() and g.p.tobytes() == c.p.tobytes()
    if g.opts:
        assert np.array_equal(g.pick_words, c.pick_words) and np.array_equal(g.pair_words, c.pair_words)


def _same(a, b):
    assert a.h == b.h and np.array_equal(a.o, b.o) and np.array_equal(a.so, b.so)
    assert a.d.tobytes() == b.d.tobytes() and a.p.tobytes() == b.p.tobytes()
    if a.opts:
        assert np.array_equal(a.pick_words, b.pick_words) and np.array_equal(a.pair_words, b.pair_words)


def _probe(w, dev, strategy, ca, *others):
    """the contexts hold the same cursors / sticky entries: the same follow-up
    batch, run once on each, gives the same records"""
    ts, keys = _batch(w, 150, salt=5)
    ts += [BIG, b"hot/1", b"hot/2", b"xt/hot"]
    keys += [3, 4, 5, 6]
    first = Call(w, dev, ts, keys, strategy, ROOMY, ca, gated=False)
    for cb in others:
        _same(first, Call(w, dev, ts, keys, strategy, ROOMY, cb, gated=False))


def _mixed(w, n):
    """a batch with the >= 300-match topic refused between admitted neighbours
    and admitted between two refused ones, inside the first block"""
    ts, keys = _batch(w, n, salt=n)
    for i in (9, 11, 13, 40, 41, 42, n - 2):
        if 0 <= i < n:
            ts[i] = BIG
    return ts, keys


MASKS = {
    "all_admitted": (130, lambda n: [0] * n),
    "all_refused": (130, lambda n: [1] * n),
    "alternating": (130, lambda n: [t & 1 for t in range(n)]),                 # BIG at 9, 11, 13, 41 refused; 40, 42 in
    "alternating_odd_in": (130, lambda n: [1 - (t & 1) for t in range(n)]),    # BIG 40, 42 refused around 41 admitted
    "first": (130, lambda n: [1] + [0] * (n - 1)),
    "last": (130, lambda n: [0] * (n - 1) + [5]),
    "block_edge": (513, lambda n: [3 if t in (255, 256) else 0 for t in range(n)]),
    "big_refused": (130, lambda n: [2 if t in (9, 13, 40, 42) else 0 for t in range(n)]),   # 11 and 41 admitted between
}


@pytest.mark.parametrize("strategy", ["keyed", "round_robin", "sticky"])
@pytest.mark.parametrize("opts", [False, True])
@pytest.mark.parametrize("mask", list(MASKS))
def test_masks(world, gpu_device, mask, opts, strategy):
    w, s = world, STRATEGY[strategy]
    n, f = MASKS[mask]
    code = f(n)
    ts, keys = _mixed(w, n)
    ca, cb = w.e.share_cursors(0), w.e.share_cursors(0)
    try:
        flags = [(i % 3) | (4 if i % 5 == 0 else 0) for i in range(n)]
        g = Call(w, gpu_device, ts, keys, s, ROOMY, ca, opts, code, flags=flags)
        c = Call(w, gpu_device, _keep(ts, code), _keep(keys, code), s, ROOMY, cb, opts, gated=False,
                 flags=_keep(flags, code))
        ids = sum(len(w.o.trie.match(t)) for t in ts)
        _equal_compacted(g, c, code, ids)
        if not any(code):
            assert g.o[-1] == g.h[2] > 0
        if all(code):
            assert g.h[:4] == [0, 0, 0, 0] and g.h[5] == 0 and g.h[4] == ids > 0 and not g.o.any() and not g.so.any()
        if strategy != "sticky" and not opts:                  # the oracles, over the admitted topics only
            rows, totals = _oracle(w, _keep(ts, code), _keep(keys, code), s, Pd(w))
            _check_oracle(w, _keep(ts, code), c, rows)
            assert (g.h[0], g.h[1]) == totals[1:3] and g.h[5] == (0 if s == KEYED else totals[3])
        _probe(w, gpu_device, s, ca, cb)
    finally:
        ca.close()
        cb.close()


@pytest.mark.parametrize("strategy", ["keyed", "round_robin", "sticky"])
@pytest.mark.parametrize("opts", [False, True])
def test_null_and_zero_planes_are_the_existing_call(world, gpu_device, opts, strategy):
    w, s = world, STRATEGY[strategy]
    ts, keys = _mixed(w, 300)
    cs = [w.e.share_cursors(0) for _ in range(3)]
    try:
        ref = Call(w, gpu_device, ts, keys, s, ROOMY, cs[0], opts, gated=False)
        null = Call(w, gpu_device, ts, keys, s, ROOMY, cs[1], opts, code=None)
        zero = Call(w, gpu_device, ts, keys, s, ROOMY, cs[2], opts, code=[0] * 300)
        assert ref.state == 0 and ref.h[2] > 0
        _same(null, ref)
        _same(zero, ref)
        _probe(w, gpu_device, s, *cs)
    finally:
        for c in cs:
            c.close()


def _picks(c, t):
    return [int(r[3]) for r in c.d[int(c.o[t]):int(c.o[t + 1])] if int(r[3]) != Engine.NO_MEMBER]


def test_round_robin_counts_the_admitted_only(world, gpu_device):
    """six publishes hit one set of three members, the second and fourth
    refused: the admitted picks are members 0, 1, 2, 0 from a fresh context,
    and the cursor afterwards is that of four ungated publishes"""
    w = world
    ts, code = [b"hot/1"] * 6, [0, 1, 0, 4, 0, 0]
    ca, cb = w.e.share_cursors(0), w.e.share_cursors(0)
    try:
        g = Call(w, gpu_device, ts, None, RR, ROOMY, ca, code=code)
        assert [_picks(g, t) for t in range(6)] == [[9001], [], [9002], [], [9003], [9001]]
        assert g.h[5] == 4
        c = Call(w, gpu_device, ts[:4], None, RR, ROOMY, cb, gated=False)
        _equal_compacted(g, c, code)
        nxt = [Call(w, gpu_device, [b"hot/1"], None, RR, ROOMY, x, gated=False) for x in (ca, cb)]
        assert _picks(nxt[0], 0) == _picks(nxt[1], 0) == [9002]
    finally:
        ca.close()
        cb.close()


def test_sticky_entry_is_drawn_by_the_first_admitted_publish(world, gpu_device):
    w = world
    ca, cb, cc = (w.e.share_cursors(0) for _ in range(3))
    try:
        # a batch whose only publish to the set is refused leaves the entry undefined ...
        g0 = Call(w, gpu_device, [b"hot/1"], [1], STICKY, ROOMY, ca, code=[1])
        assert g0.h[:4] == [0, 0, 0, 0] and g0.h[5] == 0
        # ... so the next batch draws it: refused first (key 1), the first admitted publish's key 2 decides
        g = Call(w, gpu_device, [b"hot/1"] * 3, [1, 2, 0], STICKY, ROOMY, ca, code=[5, 0, 0])
        c = Call(w, gpu_device, [b"hot/1"] * 2, [2, 0], STICKY, ROOMY, cb, gated=False)
        _equal_compacted(g, c, [5, 0, 0])
        assert _picks(g, 0) == [] and _picks(g, 1) == _picks(g, 2) == [9003] and g.h[5] >= 1  # member 2 rem 3
        other = Call(w, gpu_device, [b"hot/1"], [1], STICKY, ROOMY, cc, gated=False)
        assert _picks(other, 0) == [9002]                                                      # what key 1 would have drawn
        after = [Call(w, gpu_device, [b"hot/1"], [7], STICKY, ROOMY, x, gated=False) for x in (ca, cb)]
        assert _picks(after[0], 0) == _picks(after[1], 0) == [9003]
    finally:
        for x in (ca, cb, cc):
            x.close()


@pytest.mark.parametrize("strategy", ["round_robin", "sticky"])
def test_states_follow_the_admitted_totals(world, gpu_device, strategy):
    """capacities that fit the admitted topics but not the whole batch give
    state 0; one below the admitted need gives that stage's state with exact
    admitted totals and no cursor moved; the rerun equals a first run"""
    w, s = world, STRATEGY[strategy]
    ts, keys = _mixed(w, 130)
    code = [1 if t in (9, 13, 40, 42) or t % 3 == 0 else 0 for t in range(130)]
    cs = [w.e.share_cursors(0) for _ in range(3)]
    try:
        whole = Call(w, gpu_device, ts, keys, s, ROOMY, cs[0], gated=False)
        full = Call(w, gpu_device, ts, keys, s, ROOMY, cs[1], code=code)
        need = (full.h[4], full.h[0], full.h[1], full.h[5])
        assert whole.h[0] > need[1] and whole.h[1] > need[2] and whole.h[5] > need[3] > 0
        for stage in (2, 3, 4):
            tight = list(need)                                   # exactly the admitted need: below the whole batch's
            fit = Call(w, gpu_device, ts, keys, s, tight, w.e.share_cursors(0), code=code)
            assert fit.state == 0
            _same(fit, full)
            fit.cursors.close()
            tight[stage - 1] -= 1
            short = Call(w, gpu_device, ts, keys, s, tight, cs[2], code=code)
            assert short.state == stage
            assert short.h[4] == need[0] and short.h[0] == need[1]
            if stage >= 3:
                assert short.h[1] == need[2] and short.h[2] == full.h[2]
            if stage == 4:
                assert short.h[5] == need[3]
        rerun = Call(w, gpu_device, ts, keys, s, need, cs[2], code=code)     # cs[2] has not moved: a first run
        _same(rerun, full)
        _probe(w, gpu_device, s, cs[1], cs[2])
    finally:
        for c in cs:
            c.close()


def test_plans_over_gated_outputs(world, gpu_device):
    """the inbox plan and the forward plan read only the packed outputs: over
    a gated call's they equal the plans over the compacted batch once ent_pub /
    pub are mapped back, and no refused publish appears in either"""
    import torch
    w, dev = world, gpu_device
    ts, keys = _mixed(w, 130)
    code = [1 if t in (9, 13, 40, 42) or t % 4 == 1 else 0 for t in range(130)]
    back = np.array([t for t in range(130) if not code[t]], dtype=np.uint32)
    ca, cb = w.e.share_cursors(0), w.e.share_cursors(0)
    try:
        flags = [1] * 130
        g = Call(w, dev, ts, keys, RR, ROOMY, ca, True, code, flags=flags)
        c = Call(w, dev, _keep(ts, code), _keep(keys, code), RR, ROOMY, cb, True, gated=False, flags=_keep(flags, code))
        _equal_compacted(g, c, code)
        D, P = g.h[2], g.h[3]
        assert D > 0 and P > 0
        u32 = lambda t: t.cpu().numpy().view(np.uint32)      # noqa: E731
        u64 = lambda t: t.cpu().numpy().view(np.uint64)      # noqa: E731

        def plans(x):
            ecap = D + P
            iws = w.e.inbox_plan_stream_workspace_bytes(x.n, D, P, ecap)
            fws = w.e.forward_plan_stream_workspace_bytes(x.n, D, D)
            assert iws > 0 and fws > 0
            ws_i, ws_f = _filled(iws // 4, dev), _filled(fws // 4, dev)
            ih, fh = _filled(8, dev, 8), _filled(8, dev, 8)
            inbox, epub, eto, ewd = _filled(ecap, dev, 16), _filled(ecap, dev), _filled(ecap, dev), _filled(ecap, dev)
            groups, fpub = _filled(D, dev, 16), _filled(D, dev)
            torch.cuda.synchronize()
            w.e.inbox_plan_stream_device(x.n, x.hdr, x.doff, x.soff, x.deliv, x.pkw, D, x.pairs, x.prw, P, 0, ws_i, iws,
                                         ih, inbox, ecap, epub, eto, ewd, ecap)
            w.e.forward_plan_stream_device(x.n, x.hdr, x.doff, x.deliv, D, ws_f, fws, fh, groups, D, fpub, D)
            torch.cuda.synchronize()
            ih, fh = [int(v) for v in u64(ih)], [int(v) for v in u64(fh)]
            assert ih[6] == 0 and fh[6] == 0
            E, S, M, Gn = ih[0], ih[1], fh[0], fh[1]
            return (ih, u32(inbox).reshape(-1, 4)[:S], u32(epub)[:E], u32(eto)[:E], u32(ewd)[:E],
                    fh, u32(groups).reshape(-1, 4)[:Gn], u32(fpub)[:M])
        gi, ginbox, gpub, gto, gwd, gf, ggroups, gfpub = plans(g)
        ci, cinbox, cpub, cto, cwd, cf, cgroups, cfpub = plans(c)
        assert gi == ci and gf == cf and gi[0] > 0 and gf[0] > 0
        assert np.array_equal(ginbox, cinbox) and np.array_equal(gto, cto) and np.array_equal(gwd, cwd)
        assert np.array_equal(gpub, back[cpub & (PICK - 1)] | (cpub & PICK))
        assert np.array_equal(ggroups, cgroups) and np.array_equal(gfpub, back[cfpub])
        refused = {t for t in range(130) if code[t]}
        assert not refused & {int(v) for v in gpub & (PICK - 1)} and not refused & {int(v) for v in gfpub}
    finally:
        ca.close()
        cb.close()
