"""Shared by the pick-word GPU tests: a small world -- an engine fed together
with the route oracle (oracle/pytrie.py RouteTable), the option table
(tests/subopts_ref.py) and the member table (tests/sticky_ref.py) -- whose
member sets sit on both sides of the pick-word kernel's lane-scan / wave-scan
switch and of a wave boundary, its publishes, the model's answer per publish
(tests/pickword_ref.py) and the device-side publish call over torch buffers."""
import random

import numpy as np

from pickword_ref import outcome_word, route_pick_words
from sticky_ref import StickySub
from subopts_corpus import rand_opts
from subopts_ref import SubOptionTable, route_dispatch_opts
from emqx_amd import Engine
from emqx_amd.emqx_broker import Broker, pack_msgs, pack_subopts
from emqx_amd.emqx_router import Router
from emqx_amd.engine import pack
from oracle import pytrie

NODE = b"n1"
GUARD = 0xA5A5A5A5
SIZES = [1, 2, 7, 8, 9, 63, 64, 65, 130]       # 8 | 9: lane scan | wave scan; 64 | 65: one | two wave steps
STRATEGIES = {"keyed": Engine.SHARE_KEYED, "round_robin": Engine.SHARE_ROUND_ROBIN, "sticky": Engine.SHARE_STICKY}
NL_OPTS = {"qos": 1, "nl": 1, "rap": 1, "subid": 17}
# every pub_flags combination: QoS 0-2 x retain x retained
FLAG_COMBOS = [(q, r, rd) for q in range(3) for r in range(2) for rd in range(2)]


class PWorld:
    def __init__(self, device):
        self.e = Engine(device=device)
        self.r, self.o = Router(self.e, node="n1"), pytrie.RouteTable()
        self.b = Broker(self.e, self.r)                   # tm_set_local_node
        self.so, self.sh = SubOptionTable(), StickySub()
        self.sets = []                                    # (group bytes, To bytes, publish topic, [member])
        self.plain_topics = []
        self._names, self._targets = {}, {}

    def route(self, topic, dest):
        self.r.add_route(topic, dest)
        self.o.add_route(topic, dest)

    def plain(self, topic, s, opts=None):
        if opts is None:
            self.e.sub_add(topic, s)
            self.so.bag.insert_subscriber(None, topic, s)
        else:
            self.e.sub_add_opts(topic, s, pack_subopts(opts))
            self.so.do_subscribe(None, topic, s, opts)

    def member(self, group, topic, m, opts=None, share_first=False):
        """a $share subscriber: the member record and (opts given) its
        emqx_suboption entry, in either call order"""
        if share_first:
            self.e.share_add(group, topic, m)
        if opts is None:
            self.e.sub_add(topic, m, group)
            self.so.bag.insert_subscriber(group.decode(), topic, m)
        else:
            self.e.sub_add_opts(topic, m, pack_subopts(opts), group)
            self.so.do_subscribe(group.decode(), topic, m, opts)
        if not share_first:
            self.e.share_add(group, topic, m)
        self.sh.subscribe(group, topic, m)

    def set_opts(self, topic, m, opts):
        assert self.b.set_subopts(topic, m, opts) == self.so.set_subopts(topic, m, opts)

    def unshare(self, group, topic, m):
        assert self.e.share_del(group, topic, m) == self.sh.unsubscribe(group, topic, m)

    def close(self):
        self.e.close()

    # ---- the model's publish, and the engine's slots in the same terms ----
    def to_bytes(self, s, topic):
        if s == Engine.TOPIC_ROUTE:
            return topic
        if s not in self._names:
            self._names[s] = self.e.filter_bytes(s)
        return self._names[s]

    def want(self, strategy, pubs, upgrade=False):
        """per publish [(member | NO_MEMBER id, word)] of its deliveries, in
        aggre's order; the picks advance the model's cursors / sticky entries"""
        out = []
        for topic, key, msg in pubs:
            rows = route_pick_words(self.o, self.sh, self.so, strategy, int(key), topic, msg, upgrade)
            out.append([(Engine.NO_MEMBER if m is None else m, outcome_word(oc)) for m, oc in rows])
        return out

    def want_pairs(self, pubs, upgrade=False):
        """per publish [(To, Sub, word)] of its local pairs"""
        out = []
        for topic, _key, msg in pubs:
            _counts, pairs = route_dispatch_opts(self.o, self.so, NODE, topic, msg, upgrade)
            out.append([(to, s, outcome_word(oc)) for to, s, oc in pairs])
        return out


def build_world(device, seed=11):
    rng = random.Random(seed)
    w = PWorld(device)
    for i, c in enumerate(SIZES):
        # a set on a wildcard To (a filter id keys it) and one on the publish topic itself (TM_ROUTE_TOPIC slots)
        for kind, to, topic, base in (("w", b"w%d/+" % i, b"w%d/z" % i, 1000 * (i + 1)),
                                      ("x", b"x%d/t" % i, b"x%d/t" % i, 100000 + 1000 * (i + 1))):
            g = ("g%s%d" % (kind, i)).encode()
            w.route(to, (g.decode(), "n1"))
            if i % 2:
                w.route(to, (g.decode(), "n2"))           # the same group through another node: aggre leaves a hole
            ms = [base + k for k in range(c)]
            for k, m in enumerate(ms):
                # the last member has no-local set and is the publisher of the publish that picks it;
                # every third member has no option entry; both call orders
                opts = NL_OPTS if k == c - 1 else None if k % 3 == 1 else rand_opts(rng)
                w.member(g, to, m, opts, share_first=bool(k % 2))
            w.sets.append((g, to, topic, ms))
    # plain subscribers with random option words, local and remote routes, a filter every publish topic matches
    for j in range(20):
        t = b"p%d/t" % j
        w.plain_topics.append(t)
        w.route(t, ("n1", "n2", "n3")[j % 3])
        if j % 3 == 0:
            for s in range(1 + j % 5):
                w.plain(t, 500 + 10 * j + s, None if s % 4 == 3 else rand_opts(rng))
    w.route(b"+/t", "n1")
    w.route(b"+/t", "n2")
    for s in range(6):
        w.plain(b"+/t", 700 + s, rand_opts(rng))
    w.plain(b"+/t", 799, NL_OPTS)                             # a no-local subscriber that also publishes
    w.route(b"#", "n3")
    return w


def publishes(w, seed=5):
    """[(topic, key, msg)]: every set picked (keyed) at its first, a middle and
    its last member, the publisher being the member picked; then the plain
    topics.  Every pub_flags combination occurs."""
    rng = random.Random(seed)
    pubs, k = [], 0
    for _g, _to, topic, ms in w.sets:
        c = len(ms)
        for pos in sorted({0, c // 2, c - 1}):
            q, r, rd = FLAG_COMBOS[k % len(FLAG_COMBOS)]
            k += 1
            pubs.append((topic, pos + c * rng.randrange(1000), (q, r, rd, ms[pos])))
    for t in w.plain_topics:
        q, r, rd = FLAG_COMBOS[k % len(FLAG_COMBOS)]
        k += 1
        pubs.append((t, rng.randrange(2 ** 32), (q, r, rd, None if k % 2 else 799 if k % 4 == 0 else 700 + k % 6)))
    return pubs


def deliver_of(pubs, upgrade):
    pf, fr = pack_msgs([m for _t, _k, m in pubs])
    return (np.asarray(pf, dtype=np.uint32), np.asarray(fr, dtype=np.uint32),
            Engine.DELIVER_UPGRADE_QOS if upgrade else 0)


# ---- device calls over torch buffers ---------------------------------------------------

def dev(x, device, dtype=None):
    import torch
    a = np.ascontiguousarray(x)
    return torch.from_numpy(a.view(dtype).copy() if dtype else a.copy()).to(torch.device("cuda", device))


def full(n, device, dtype, fill=-1):
    import torch
    return torch.full((max(n, 1),), fill, dtype=dtype, device=torch.device("cuda", device))


def u32(t):
    return t.cpu().numpy().view(np.uint32)


class DevPublish:
    """tm_match_publish_batch_device into torch buffers that stay on the
    device for the post-pass"""

    def __init__(self, e, device, pubs, strategy, cap, scap, stream=None):
        import torch
        topics = [t for t, _k, _m in pubs]
        self.e, self.device, self.n, self.cap, self.scap = e, device, len(topics), cap, scap
        buf, off = pack(topics)
        n = self.n
        self.off = off
        self.d_b, self.d_o = dev(buf, device), dev(off, device, np.int64)
        self.c, self.o = full(n, device, torch.int32), full(n + 1, device, torch.int64)
        self.tot = full(1, device, torch.int64)
        self.to, self.tg, self.nd, self.pk = (full(cap, device, torch.int32, -7) for _ in range(4))
        self.sc, self.so, self.stot = (full(n, device, torch.int32), full(n + 1, device, torch.int64),
                                       full(1, device, torch.int64))
        self.sto, self.sid = full(scap, device, torch.int32, -9), full(scap, device, torch.int32, -9)
        d_k = dev(np.asarray([k for _t, k, _m in pubs], dtype=np.uint32), device, np.int32)
        torch.cuda.synchronize()
        e.match_publish_batch_device(self.d_b, self.d_o, n, int(off[-1] - off[0]), self.c, self.o, self.to, self.tg,
                                     self.nd, cap, self.tot, self.sc, self.so, self.sto, self.sid, scap, self.stot,
                                     strategy, d_k, self.pk, stream=stream)
        torch.cuda.synchronize()

    def prepare(self, deliver, extra=8):
        """the post-pass's inputs and its word plane (cap + extra words,
        pre-filled with GUARD) on the device"""
        import torch
        pf, fr, self.fl = deliver
        self.d_pf = dev(pf, self.device, np.int32)
        self.d_fr = None if fr is None else dev(fr, self.device, np.int32)
        self.pw = dev(np.full(self.cap + extra, GUARD, dtype=np.uint32), self.device, np.int32)
        torch.cuda.synchronize()

    def launch(self, out_cap=None, stream=None):
        """tm_share_pick_words_device, enqueued only"""
        self.e.share_pick_words_device(self.d_b, self.d_o, self.n, self.c, self.o, self.to, self.tg, self.pk,
                                       self.cap if out_cap is None else out_cap, self.tot,
                                       (self.d_pf, self.d_fr, self.fl), self.pw, stream=stream)

    def words(self, deliver, extra=8, out_cap=None):
        """prepare + launch + wait -> the word plane as a device tensor"""
        import torch
        self.prepare(deliver, extra)
        self.launch(out_cap)
        torch.cuda.synchronize()
        return self.pw


def check_planes(want, counts, offs, pick, words, bound, tag=None):
    """every live slot below `bound` against the model; everything else of the
    word plane keeps GUARD.  Returns (slots with a word, slots without)."""
    words = np.asarray(words)
    live = np.zeros(len(words), dtype=bool)
    worded = bare = 0
    for t, rows in enumerate(want):
        a, c = int(offs[t]), int(counts[t])
        assert c == len(rows), (tag, t)
        for k, (m, word) in enumerate(rows):
            s = a + k
            if s >= bound:
                continue
            live[s] = True
            assert int(pick[s]) == m, (tag, t, k)
            assert int(words[s]) == word, (tag, t, k, hex(int(words[s])), hex(word))
            if word == Engine.NO_WORD:
                bare += 1
            else:
                worded += 1
    assert (words[~live] == GUARD).all(), tag
    return worded, bare
