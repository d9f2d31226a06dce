"""The micro-batcher's forward mode on the GPU (TM_BATCHER_FORWARD,
tm_batcher_open_plans): per batch the plan of the batch's remote-node
deliveries, grouped per (node, To), after the inbox plan's callback and before
the per-publish callbacks; against tests/forward_ref.py over the TM_NOT_LOCAL
node records the same batch's per-publish callbacks carried, and against the
same batcher without the flag for everything the per-publish callbacks carry.
One lane wherever cursors are compared."""
import os
import sys
import threading

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from forward_ref import expected_plan, forward_deliveries  # noqa: E402
from pickword_world import NODE, build_world, deliver_of, publishes  # noqa: E402
from emqx_amd import Engine  # noqa: E402
from emqx_amd import _lib as L  # noqa: E402
from emqx_amd.batcher import Batcher  # noqa: E402
from emqx_amd.emqx_router import _enc  # noqa: E402

pytestmark = pytest.mark.gpu


class Sink:
    """what a batcher's callbacks saw, in the order each lane thread made them"""

    def __init__(self):
        self.lock = threading.Lock()
        self.by_thread = {}          # thread id -> [("inbox" | "forward", tickets) | ("pub", index)]
        self.plans = []              # (tickets, hdr, group rows, pub): copies
        self.inboxes = []            # (tickets, hdr, inbox rows, ent_pub, ent_to, ent_word): copies
        self.pubs = {}               # submit index -> the per-publish callback's arguments

    def _note(self, row):
        self.by_thread.setdefault(threading.get_ident(), []).append(row)

    def on_forward(self, status, tickets, hdr, groups, pub):
        assert status == L.TM_OK
        plan = ([int(t) for t in tickets], [int(x) for x in hdr], [tuple(r) for r in groups.tolist()],
                [int(x) for x in pub])                           # the views die with the call
        with self.lock:
            self.plans.append(plan)
            self._note(("forward", plan[0]))

    def on_inbox(self, status, tickets, hdr, inbox, ent_pub, ent_to, ent_word):
        assert status == L.TM_OK
        plan = ([int(t) for t in tickets], [int(x) for x in hdr], inbox.tolist(), ent_pub.tolist(), ent_to.tolist(),
                ent_word.tolist())
        with self.lock:
            self.inboxes.append(plan)
            self._note(("inbox", plan[0]))

    def on_pub(self, i):
        def cb(status, *rest):
            with self.lock:
                self.pubs[i] = (status,) + rest
                self._note(("pub", i))
        return cb


def _submit_all(b, pubs, cb_of, opts, upgrade=False, first=None):
    """every publish through b; first: flush after every `first` submits (one lane: batches of that size)"""
    pf, fr, _fl = deliver_of(pubs, upgrade)
    tickets = []
    for i, (topic, key, _msg) in enumerate(pubs):
        if opts:
            tickets.append(b.submit_publish_opts(topic, int(key), int(pf[i]), int(fr[i]), cb_of(i)))
        else:
            tickets.append(b.submit_publish(topic, int(key), cb_of(i)))
        if first and i % first == first - 1:
            b.flush()
    b.flush()
    return tickets


def _check_order(sink, tickets, inbox):
    """per lane thread: a batch's inbox plan (if any), its forward plan, then
    exactly that batch's publishes, then the next batch"""
    index = {t: i for i, t in enumerate(tickets)}
    batches = 0
    for seq in sink.by_thread.values():
        at = 0
        while at < len(seq):
            if inbox:
                assert seq[at][0] == "inbox" and seq[at + 1][0] == "forward" and seq[at][1] == seq[at + 1][1]
                at += 1
            kind, tk = seq[at]
            assert kind == "forward"
            rows = seq[at + 1:at + 1 + len(tk)]
            assert [r[0] for r in rows] == ["pub"] * len(tk)
            assert sorted(r[1] for r in rows) == sorted(index[t] for t in tk)
            at += 1 + len(tk)
            batches += 1
    assert batches == len(sink.plans) and len(sink.inboxes) == (batches if inbox else 0)
    assert sorted(t for p in sink.plans for t in p[0]) == sorted(tickets)   # every publish in exactly one plan


def _check_plans(w, sink, tickets, pubs):
    """each batch's plan equals expected_plan over the TM_NOT_LOCAL node records
    that the same batch's per-publish callbacks carried, pub mapped through
    tickets; and, over names, forward/3's deliveries of the route oracle"""
    index = {t: i for i, t in enumerate(tickets)}
    remote = {w.e.dest_target(_enc(nm), Engine.TARGET_NODE, nm.encode()): nm.encode() for nm in ("n2", "n3")}
    total = 0
    for tk, hdr, groups, pub in sink.plans:
        triples = []
        for p, t in enumerate(tk):
            status, deliv = sink.pubs[index[t]][:2]
            assert status == L.TM_OK
            for to, target, ndisp, _pick in deliv:
                if ndisp == Engine.NOT_LOCAL and target in remote:
                    triples.append((target, to, p))
        want = expected_plan(triples)
        assert hdr == want[0] and groups == want[1] and pub == want[2]
        assert all(p < len(tk) for p in pub)
        batch = [pubs[index[t]][0] for t in tk]
        named = sorted((remote[tg], w.to_bytes(to, batch[p]), p) for tg, to, first, count in groups
                       for p in pub[first:first + count])
        assert named == sorted((nd, tob, t) for nd, tob, t, _k in forward_deliveries(w.o, NODE, batch))
        total += hdr[0]
    assert total > len(pubs)                                     # every topic matches '#' -> n3, many a second node


def _run(w, pubs, sink, opts, forward, inbox=False, first=None, **kw):
    b = Batcher(w.e, max_topics=64, deadline_us=100_000 if first else 200, publish=True, opts=opts,
                forward=sink.on_forward if forward else None, inbox=sink.on_inbox if inbox else None, **kw)
    tickets = _submit_all(b, pubs, sink.on_pub, opts, kw.get("upgrade_qos", False), first)
    st = b.stats()
    b.close()
    assert st["topics"] == len(pubs) and st["failed_batches"] == 0
    return tickets, st


def _world(gpu_device, k=300):
    w = build_world(gpu_device)
    w.e.commit()
    base = publishes(w)
    return w, [base[i % len(base)] for i in range(k)]


def test_keyed_forward_plan_per_batch(gpu_device):
    """PUBLISH|FORWARD: the stream-ordered call with keyed picks; per-publish
    callbacks equal those of a plain publish batcher"""
    assert hasattr(Engine, "NOT_LOCAL")
    w, pubs = _world(gpu_device)
    sink = Sink()
    tickets, st = _run(w, pubs, sink, opts=False, forward=True)
    assert len(sink.plans) == st["batches"] >= 5
    _check_order(sink, tickets, False)
    _check_plans(w, sink, tickets, pubs)
    plain = Sink()
    _run(w, pubs, plain, opts=False, forward=False)
    assert not plain.plans and all(sink.pubs[i] == plain.pubs[i] for i in range(len(pubs)))
    assert any(len(sink.pubs[i][2]) for i in range(len(pubs)))    # pairs still come with the publishes
    w.close()


def test_round_robin_opts_forward_one_lane(gpu_device):
    """PUBLISH|OPTS|FORWARD|ROUND_ROBIN on one lane: the picks advance once per
    batch, exactly as without the flag (two fresh worlds: the cursors start equal)"""
    seen = []
    for forward in (True, False):
        w, pubs = _world(gpu_device)
        sink = Sink()
        tickets, st = _run(w, pubs, sink, opts=True, forward=forward, round_robin=True, lanes_per_replica=1, first=64)
        if forward:
            assert len(sink.plans) == st["batches"] >= 5
            _check_order(sink, tickets, False)
            _check_plans(w, sink, tickets, pubs)
        seen.append([sink.pubs[i] for i in range(len(pubs))])
        w.close()
    assert seen[0] == seen[1]
    assert any(d[3] != Engine.NO_MEMBER for row in seen[0] for d in row[1])


def test_sticky_inbox_and_forward_one_lane(gpu_device):
    """PUBLISH|OPTS|INBOX|FORWARD|STICKY on one lane: the inbox plan is what an
    inbox batcher without the forward flag delivers, and the order holds"""
    seen = []
    for forward in (True, False):
        w, pubs = _world(gpu_device)
        sink = Sink()
        tickets, st = _run(w, pubs, sink, opts=True, forward=forward, inbox=True, sticky=True, lanes_per_replica=1,
                           first=64)
        if forward:
            assert len(sink.plans) == st["batches"] >= 5
            _check_order(sink, tickets, True)
            _check_plans(w, sink, tickets, pubs)
        index = {t: i for i, t in enumerate(tickets)}
        seen.append(([sink.pubs[i] for i in range(len(pubs))],
                     [([index[t] for t in p[0]],) + p[1:] for p in sink.inboxes]))
        w.close()
    assert seen[0][0] == seen[1][0]                              # picks, words and pair counts
    assert seen[0][1] == seen[1][1] and len(seen[0][1]) >= 5     # the inbox plans, batch for batch
    assert all(row[3] is None for row in seen[0][0])             # the pairs are in the inbox plan


def test_publish_rerun_gives_the_same_plans_and_picks(gpu_device):
    """a first batch far above the lane's initial capacities: the publish call
    reports a state, the whole chain runs again, and plans and picks equal a
    run whose first batch fits (keyed: the picks do not depend on the batching)"""
    w = build_world(gpu_device)
    for i in range(60):                                          # every topic below fans out to 60 more filters
        w.route(b"+/t", "m%02d" % i)
    w.e.commit()
    base = [p for p in publishes(w) if p[0].endswith(b"/t")]
    pubs = [base[i % len(base)] for i in range(64)]
    big = Sink()
    tickets, st = _run(w, pubs, big, opts=False, forward=True, lanes_per_replica=1, first=64)
    assert st["reruns"] > 0 and st["batches"] == 1 and len(big.plans) == 1
    assert big.plans[0][1][0] > 64 * 60                          # M: far above 16 deliveries per topic
    _check_order(big, tickets, False)
    small = Sink()
    b = Batcher(w.e, max_topics=8, deadline_us=100_000, publish=True, lanes_per_replica=1, forward=small.on_forward)
    t2 = _submit_all(b, pubs, small.on_pub, False)
    st2 = b.stats()
    b.close()
    assert st2["failed_batches"] == 0 and len(small.plans) == st2["batches"] >= 8
    assert all(big.pubs[i] == small.pubs[i] for i in range(64))
    # the one-shot plan is the small batches' plans merged: the same (node, To, publish) triples
    def triples(sink, tk):
        index = {t: i for i, t in enumerate(tk)}
        return sorted((tg, to, index[p[0][q]]) for p in sink.plans for tg, to, first, count in p[2]
                      for q in p[3][first:first + count])
    assert triples(big, tickets) == triples(small, t2)
    w.close()
