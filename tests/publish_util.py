"""Shared by the publish-pack and publish-batcher GPU tests: an engine fed
together with the three test oracles (oracle/pytrie.py RouteTable,
tests/dispatch_ref.py, tests/shared_ref.py), the oracles' answer for one
publish in the shape of the packed records, and the device-side publish +
pack calls over torch buffers."""
import numpy as np

from dispatch_ref import SubscriberBag, route_dispatch
from shared_ref import SharedSub as RefShared, route_shared
from emqx_amd import Engine
from emqx_amd.emqx_broker import Broker
from emqx_amd.emqx_router import Router
from emqx_amd.engine import pack
from oracle import pytrie

NODE = b"n1"
GUARD = 0xA5A5A5A5


class World:
    def __init__(self, device, local=True):
        self.e = Engine(device=device)
        self.r, self.o = Router(self.e, node="n1"), pytrie.RouteTable()
        if local:
            Broker(self.e, self.r)                       # tm_set_local_node
        self.bag, self.sh = SubscriberBag(), RefShared()
        self._names, self._targets = {}, {}

    def route(self, topic, dest):
        self.r.add_route(topic, dest)
        self.o.add_route(topic, dest)

    def sub(self, topic, s, group=None):
        self.e.sub_add(topic, s, group)
        self.bag.insert_subscriber(None if group is None else group.decode(), topic, s)

    def subs(self, topic, ss):
        tb, to = pack([topic] * len(ss))
        self.e.sub_add_many(tb, to, np.asarray(ss, dtype=np.uint32))
        for s in ss:
            self.bag.insert_subscriber(None, topic, s)

    def members(self, group, topic, ms):
        gb, go = pack([group] * len(ms))
        tb, to = pack([topic] * len(ms))
        self.e.share_add_many(gb, go, tb, to, ms)
        for m in ms:
            self.sh.subscribe(group, topic, m)

    def close(self):
        self.e.close()

    # ---- the oracles' publish, and the engine's records in the same terms ----
    def want(self, topic, key):
        """([(To, target, Count | None, member | None)], [(To, Sub)]) of one
        publish with TM_SHARE_KEYED key"""
        dels = self.o.match_deliveries(topic)
        counts, pairs = route_dispatch(self.o, self.bag, NODE, topic)
        picks = route_shared(self.o, self.sh, "keyed", int(key), topic)
        return [(to, tg, c, m) for (to, tg), c, m in zip(dels, counts, picks)], pairs

    def _to(self, s, topic):
        if s == Engine.TOPIC_ROUTE:
            return topic
        if s not in self._names:
            self._names[s] = self.e.filter_bytes(s)
        return self._names[s]

    def got(self, topic, deliveries, pairs):
        """packed records (id tuples) in the terms of want()"""
        out = []
        for to, tg, nd, pk in deliveries:
            if tg not in self._targets:
                self._targets[tg] = self.e.target_bytes(tg)
            out.append((self._to(to, topic), self._targets[tg], None if nd == Engine.NOT_LOCAL else nd,
                        None if pk == Engine.NO_MEMBER else pk))
        return out, [(self._to(to, topic), s) for to, s in pairs]


def slices(out, n):
    """Engine.match_publish_batch's tuple -> per topic ([(to, target, ndisp,
    pick)], [(to, sub)]) as the batcher's callbacks give them"""
    counts, offs, to, tg, nd, scount, soff, sto, sid, pick = out
    res = []
    for t in range(n):
        a, c = int(offs[t]), int(counts[t])
        p, q = int(soff[t]), int(soff[t]) + int(scount[t])
        res.append(([(int(to[k]), int(tg[k]), int(nd[k]), int(pick[k])) for k in range(a, a + c)],
                    [(int(sto[k]), int(sid[k])) for k in range(p, q)]))
    return res


# ---- device calls over torch buffers ---------------------------------------------------

def _dev(x, dev, dtype=None):
    import torch
    a = np.ascontiguousarray(x)
    return torch.from_numpy(a.view(dtype).copy() if dtype else a.copy()).to(torch.device("cuda", dev))


def _full(n, dev, dtype, fill=-1):
    import torch
    return torch.full((max(n, 1),), fill, dtype=dtype, device=torch.device("cuda", dev))


class DevicePublish:
    """tm_match_publish_batch_device(TM_SHARE_KEYED) into torch buffers that
    stay on the device for the pack; .host() copies them back"""

    def __init__(self, e, dev, topics, keys, cap, scap):
        import torch
        self.e, self.dev, self.n, self.cap, self.scap = e, dev, len(topics), cap, scap
        buf, off = pack(topics)
        n = self.n
        d_b, d_o = _dev(buf if len(buf) else np.zeros(1, np.uint8), dev), _dev(off, dev, np.int64)
        self.c, self.o = _full(n, dev, torch.int32), _full(n + 1, dev, torch.int64)
        self.tot = _full(1, dev, torch.int64)
        self.to, self.tg, self.nd, self.pk = (_full(cap, dev, torch.int32, -7) for _ in range(4))
        self.sc, self.so, self.stot = _full(n, dev, torch.int32), _full(n + 1, dev, torch.int64), _full(1, dev,
                                                                                                         torch.int64)
        self.sto, self.sid = _full(scap, dev, torch.int32, -9), _full(scap, dev, torch.int32, -9)
        d_k = _dev(np.asarray(keys, dtype=np.uint32) if n else np.zeros(1, np.uint32), dev, np.int32)
        torch.cuda.synchronize()
        e.match_publish_batch_device(d_b, d_o, n, int(off[-1] - off[0]), self.c, self.o, self.to, self.tg, self.nd,
                                     cap, self.tot, self.sc, self.so, self.sto, self.sid, scap, self.stot,
                                     Engine.SHARE_KEYED, d_k, self.pk)
        torch.cuda.synchronize()

    def host(self):
        u = lambda t: t.cpu().numpy().view(np.uint32)   # noqa: E731
        return dict(c=u(self.c)[:self.n], o=self.o.cpu().numpy().view(np.uint64), to=u(self.to), tg=u(self.tg),
                    nd=u(self.nd), pk=u(self.pk), tot=int(self.tot.item()), so=self.so.cpu().numpy().view(np.uint64),
                    sto=u(self.sto), sid=u(self.sid), stot=int(self.stot.item()))

    def pack(self, deliv_cap, pair_cap, pick=True, guard=4):
        """tm_publish_pack_device -> (hdr[4], doff[n+1], deliv (deliv_cap +
        guard, 4) u32, pairs (pair_cap + guard, 2) u32): `guard` records after
        each capacity are pre-filled with GUARD and must come back unchanged"""
        import torch
        dev = self.dev
        hdr, doff = _full(4, dev, torch.int64, -3), _full(self.n + 1, dev, torch.int64, -3)
        deliv = _dev(np.full((deliv_cap + guard) * 4, GUARD, dtype=np.uint32), dev, np.int32)
        pairs = _dev(np.full((pair_cap + guard) * 2, GUARD, dtype=np.uint32), dev, np.int32)
        torch.cuda.synchronize()
        self.e.publish_pack(self.n, self.c, self.o, self.to, self.tg, self.nd, self.pk if pick else None, self.cap,
                            self.tot, self.so, self.sto, self.sid, self.scap, self.stot, hdr, doff, deliv, deliv_cap,
                            pairs, pair_cap)
        torch.cuda.synchronize()
        return (hdr.cpu().numpy().view(np.uint64), doff.cpu().numpy().view(np.uint64)[:self.n + 1],
                deliv.cpu().numpy().view(np.uint32).reshape(-1, 4), pairs.cpu().numpy().view(np.uint32).reshape(-1, 2))
