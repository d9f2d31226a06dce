"""Micro-batcher publish mode on the GPU (TM_BATCHER_PUBLISH): publisher threads
submit single topics with a pick key each; every callback's delivery records
(To, target, Count, pick) and (To, subscriber) pairs must equal that topic's
slice of Engine.match_publish_batch(SHARE_KEYED, keys), whatever batch it rode
in, and a sample is checked against tests/dispatch_ref.py and
tests/shared_ref.py directly.  Keys on the partial-take path, the rerun of a
batch that outgrew the lane's first capacities, a missing local node, and a
deliveries batcher beside a publish batcher on one engine."""
import os
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from publish_util import World, slices  # noqa: E402
from emqx_amd import Engine  # noqa: E402
from emqx_amd import _lib as L  # noqa: E402
from emqx_amd import workload as W  # noqa: E402
from emqx_amd.batcher import Batcher  # noqa: E402
from emqx_amd.engine import pack  # noqa: E402

pytestmark = pytest.mark.gpu


class _C1:
    """workload config 1 with routes to three nodes and two groups, subscriber
    bags and member sets of 1, 2 and 7 members; the batch API's publish of the
    40,000 topics with pub_key = i, computed once"""

    def __init__(self, device):
        fb, fo = W.filters(1)
        tb, to = W.topics(1, n=40000)
        self.topics = W.unpack(tb, to)
        self.w = w = World(device)
        filters = W.unpack(fb, fo)
        for i, f in enumerate(filters):
            w.route(f, "n%d" % (1 + i % 3))
            if i % 3 == 0:                                       # a {Group, Node} route, on a third of them twice
                g = "grp%d" % (i % 4)
                w.route(f, (g, "n1"))
                if i % 9 == 0:
                    w.route(f, (g, "n2"))                        # aggre/1 leaves a hole
                if i % 6 == 0:
                    w.members(g.encode(), f, [50000 + 8 * i + k for k in range((1, 2, 7)[i // 6 % 3])])
            if i % 2 == 0:
                w.sub(f, 2 * i)
            if i % 10 == 0:
                w.sub(f, 2 * i + 1)
                w.sub(f, 900000 + i, b"grp1")                    # a shared entry: counts, no pair
        for j, t in enumerate(self.topics[::5]):
            w.route(t, ("n1", "n3")[j % 2])
            if j % 4 == 0:
                w.sub(t, 700000 + j)
            if j % 8 == 0:
                w.route(t, ("grp2", "n2"))
                w.members(b"grp2", t, [800000 + 8 * j + k for k in range((7, 1, 2)[j // 8 % 3])])
        w.e.commit()
        self.keys = np.arange(len(self.topics), dtype=np.uint32)
        self.out = w.e.match_publish_batch(tb, to, Engine.SHARE_KEYED, self.keys)
        self.want = slices(self.out, len(self.topics))
        for t in range(0, len(self.topics), 7):                  # the batch API itself against the oracles
            assert w.got(self.topics[t], *self.want[t]) == w.want(self.topics[t], t), t
        picks = [d[3] for dl, _ in self.want for d in dl]
        assert sum(1 for x in picks if x != Engine.NO_MEMBER) > 10000
        assert sum(len(p) for _, p in self.want) > 100000


@pytest.fixture(scope="module")
def c1(gpu_device):
    x = _C1(gpu_device)
    yield x
    x.w.close()


def _flood(b, topics, keys, got, threads=4):
    def producer(k):
        for t in range(k, len(topics), threads):
            def cb(status, deliveries, pairs, t=t):
                got[t] = (status, deliveries, pairs) if got[t] is None else "twice"
            b.submit_publish(topics[t], int(keys[t]), cb)
    ts = [threading.Thread(target=producer, args=(k,)) for k in range(threads)]
    for x in ts:
        x.start()
    for x in ts:
        x.join()
    b.flush()


@pytest.mark.parametrize("cbt", [0, 2])
def test_publish_batcher_equals_batch_api(c1, cbt):
    """cbt > 0: callback threads share each batch's callbacks with its lane
    (batches of up to 20K topics: parts of >= 8192)"""
    topics = c1.topics
    b = Batcher(c1.w.e, max_topics=20000 if cbt else 3000, deadline_us=500, publish=True, callback_threads=cbt)
    got = [None] * len(topics)
    _flood(b, topics, c1.keys, got)
    st = b.stats()
    b.close()
    assert st["topics"] == len(topics) and st["failed_batches"] == 0 and st["batches"] >= (2 if cbt else 5)
    for t in range(len(topics)):
        assert got[t] == (0, c1.want[t][0], c1.want[t][1]), t
    assert st["results"] == sum(len(d) for d, _ in c1.want)
    for t in range(0, len(topics), 7):
        assert c1.w.got(topics[t], got[t][1], got[t][2]) == c1.w.want(topics[t], t), t


def test_deliveries_and_publish_batchers_concurrently(c1):
    topics = c1.topics[:12000]
    counts, offs, to, tg = c1.out[0], c1.out[1], c1.out[2], c1.out[3]
    want_d = [([int(x) for x in to[offs[t]:offs[t] + counts[t]]], [int(x) for x in tg[offs[t]:offs[t] + counts[t]]])
              for t in range(len(topics))]
    bd = Batcher(c1.w.e, max_topics=1500, deadline_us=300, deliveries=True)
    bp = Batcher(c1.w.e, max_topics=2000, deadline_us=300, publish=True)
    got_d, got_p = [None] * len(topics), [None] * len(topics)

    def producer(k):
        for t in range(k, len(topics), 4):
            def cb(status, ids, ds, t=t):
                got_d[t] = (status, ids, ds)
            bd.submit(topics[t], cb)
    ts = [threading.Thread(target=producer, args=(k,)) for k in range(4)]
    ts.append(threading.Thread(target=_flood, args=(bp, topics, c1.keys, got_p)))
    for x in ts:
        x.start()
    for x in ts:
        x.join()
    bd.flush()
    bp.flush()
    assert bd.stats()["failed_batches"] == 0 and bp.stats()["failed_batches"] == 0
    bd.close()
    bp.close()
    for t in range(len(topics)):
        assert got_d[t] == (0, want_d[t][0], want_d[t][1]), t
        assert got_p[t] == (0, c1.want[t][0], c1.want[t][1]), t


def test_keys_travel_with_their_topics_through_partial_takes(gpu_device):
    """max_topics 64, one lane, producers far ahead: seals take a stripe's
    oldest topics and advance its head.  Every topic has one 7-member group
    delivery and a key of its own: the pick must be members[key % 7]"""
    w = World(gpu_device)
    members = [310, 311, 312, 313, 314, 315, 316]
    w.route(b"k/+", ("g", "n1"))
    w.members(b"g", b"k/+", members)
    w.e.commit()
    n = 9000
    topics = [b"k/%d" % (i % 50) for i in range(n)]
    keys = [(i * 2654435761 + 3) % 2 ** 32 for i in range(n)]
    assert len(set(keys)) == n
    b = Batcher(w.e, max_topics=64, deadline_us=50, lanes_per_replica=1, publish=True)
    got = [None] * n
    _flood(b, topics, keys, got, threads=3)
    st = b.stats()
    b.close()
    assert st["failed_batches"] == 0 and st["topics"] == n and st["max_batch"] <= 64
    for i in range(n):
        status, deliveries, pairs = got[i]
        assert status == 0 and pairs == [] and len(deliveries) == 1, i
        assert deliveries[0][3] == members[keys[i] % 7], i
    assert w.got(topics[5], got[5][1], got[5][2]) == w.want(topics[5], keys[5])
    w.close()


@pytest.mark.parametrize("kind", ["deliveries", "pairs"])
def test_first_batch_outgrows_the_first_capacities_and_is_rerun(gpu_device, kind):
    """a fresh batcher's first batch: one topic with 2,048 deliveries (2^11
    filters of '+' and literals over an 11-level topic), or one topic with a
    3,000-subscriber bag -- more than a one-topic batch's first capacities
    (1,044 records each)"""
    w = World(gpu_device)
    if kind == "deliveries":
        lv = [b"m%d" % i for i in range(11)]
        topic = b"/".join(lv)

        def f(m):
            return b"/".join(b"+" if m >> i & 1 else lv[i] for i in range(11))
        for m in range(2048):
            w.route(f(m), ("n1", "n2", ("g", "n1"))[m % 3])
        w.members(b"g", f(2), [1, 2, 3])                         # m % 3 == 2: group routes
        w.members(b"g", f(5), [4])
        w.sub(f(0), 78)                                          # m % 3 == 0: local
        w.sub(f(3), 77)
    else:
        topic = b"bag/of/many"
        w.route(topic, "n1")
        w.route(b"bag/#", ("g", "n2"))
        w.members(b"g", b"bag/#", [4, 5])
        w.subs(topic, list(range(40000, 43000)))
    w.e.commit()
    buf, off = pack([topic])
    want = slices(w.e.match_publish_batch(buf, off, Engine.SHARE_KEYED, [9]), 1)[0]
    assert (len(want[0]) == 2048) if kind == "deliveries" else (len(want[1]) == 3000)
    assert w.got(topic, *want) == w.want(topic, 9)
    b = Batcher(w.e, max_topics=1000, deadline_us=100, publish=True)
    got = [None]
    _flood(b, [topic], [9], got, threads=1)
    st = b.stats()
    b.close()
    assert st["batches"] == 1 and st["failed_batches"] == 0
    assert got[0] == (0, want[0], want[1])
    w.close()


def test_local_node_not_set_gives_einval(gpu_device):
    w = World(gpu_device, local=False)
    w.route(b"a/+", "n1")
    w.e.commit()
    b = Batcher(w.e, max_topics=100, deadline_us=100, publish=True)
    got = [None] * 300
    _flood(b, [b"a/%d" % i for i in range(300)], list(range(300)), got, threads=2)
    st = b.stats()
    b.close()
    assert all(g == (L.TM_EINVAL, None, None) for g in got)
    assert st["failed_batches"] == st["batches"] >= 1
    w.close()
