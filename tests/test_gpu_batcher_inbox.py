"""The micro-batcher's inbox mode on the GPU (TM_BATCHER_INBOX,
tm_batcher_open_inbox): per batch the plan of the batch's local sends, grouped
per receiving session, before the per-publish callbacks; against
tests/inbox_ref.py over tests/pickword_world.py's world, and against an
options batcher without the flag for everything the per-publish callbacks
still carry.  The round-robin case forces a rerun of the plan alone and checks
that the cursors advanced once."""
import os
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from inbox_ref import grouped, grouped_plan, reference_sends  # noqa: E402
from pickword_ref import outcome_word, route_pick_words  # noqa: E402
from pickword_world import NODE, build_world, deliver_of, publishes  # noqa: E402
from sticky_ref import StickySub  # noqa: E402
from emqx_amd import Engine  # noqa: E402
from emqx_amd import _lib as L  # noqa: E402
from emqx_amd.batcher import Batcher  # noqa: E402

pytestmark = pytest.mark.gpu


class Sink:
    """what an inbox batcher's callbacks saw, in the order each lane thread made them"""

    def __init__(self):
        self.lock = threading.Lock()
        self.by_thread = {}          # thread id -> [("inbox", plan) | ("pub", index)]
        self.plans = []              # (tickets, hdr, inbox rows, ent_pub, ent_to, ent_word): copies
        self.pubs = {}               # submit index -> (status, deliveries, pick_words, pairs, n_pairs)

    def on_inbox(self, status, tickets, hdr, inbox, ent_pub, ent_to, ent_word):
        assert status == L.TM_OK
        plan = ([int(t) for t in tickets], [int(x) for x in hdr], inbox.tolist(), ent_pub.copy(), ent_to.copy(),
                ent_word.copy())                                 # the views die with the call
        with self.lock:
            self.plans.append(plan)
            self.by_thread.setdefault(threading.get_ident(), []).append(("inbox", plan[0]))

    def on_pub(self, i):
        def cb(status, deliv, pick_words, pairs, n_pairs):
            with self.lock:
                self.pubs[i] = (status, deliv, pick_words, pairs, n_pairs)
                self.by_thread.setdefault(threading.get_ident(), []).append(("pub", i))
        return cb


def _submit_all(b, pubs, cb_of, upgrade, flush_every=None):
    pf, fr, _fl = deliver_of(pubs, upgrade)
    tickets = []
    for i, (topic, key, _msg) in enumerate(pubs):
        tickets.append(b.submit_publish_opts(topic, int(key), int(pf[i]), int(fr[i]), cb_of(i)))
        if flush_every and i % flush_every == flush_every - 1:
            b.flush()
    b.flush()
    return tickets


def _check_order(sink, tickets):
    """per lane thread: a batch's plan, then exactly that batch's publishes, then the next plan"""
    index = {t: i for i, t in enumerate(tickets)}
    batches = 0
    for seq in sink.by_thread.values():
        at = 0
        while at < len(seq):
            kind, tk = seq[at]
            assert kind == "inbox"
            rows = seq[at + 1:at + 1 + len(tk)]
            assert [r[0] for r in rows] == ["pub"] * len(tk)
            assert sorted(r[1] for r in rows) == sorted(index[t] for t in tk)
            at += 1 + len(tk)
            batches += 1
    assert batches == len(sink.plans)
    assert sorted(t for p in sink.plans for t in p[0]) == sorted(tickets)   # every publish in exactly one plan


def _check_plans(w, sink, tickets, pubs, strategy, upgrade):
    """each batch's plan, mapped through tickets[], against the reference's sends
    of that batch's publishes in ticket order (the model advances batch by batch)"""
    index = {t: i for i, t in enumerate(tickets)}
    for tk, hdr, inbox, ent_pub, ent_to, ent_word in sink.plans:
        batch = [pubs[index[t]] for t in tk]
        ref = reference_sends(w.o, w.so, w.sh, NODE, strategy, batch, upgrade)
        name = lambda to, pub: w.to_bytes(to, batch[pub][0])   # noqa: E731
        assert grouped_plan(inbox, ent_pub, ent_to, ent_word, name) == grouped(ref)
        picks = sum(1 for s in ref if s[2])
        assert hdr == [len(ref), len(grouped(ref)), len(ref) - picks, picks]
        assert len(ent_pub) == len(ref) and max(int(x) & ~Engine.INBOX_PICK for x in ent_pub) < len(tk)


def test_plan_per_batch_before_the_publish_callbacks(gpu_device):
    w = build_world(gpu_device)
    w.e.commit()
    base = publishes(w)
    pubs = [base[i % len(base)] for i in range(300)]
    sink = Sink()
    b = Batcher(w.e, max_topics=64, deadline_us=200, publish=True, opts=True, inbox=sink.on_inbox)
    tickets = _submit_all(b, pubs, sink.on_pub, False)
    st = b.stats()
    b.close()
    assert st["topics"] == 300 and st["failed_batches"] == 0 and len(sink.plans) == st["batches"] >= 5
    _check_order(sink, tickets)
    _check_plans(w, sink, tickets, pubs, "keyed", False)
    # the same submits through an options batcher without the flag
    plain = {}

    def keep(i):
        def cb(status, deliv, pick_words, pairs, pair_words):
            plain[i] = (status, deliv, pick_words, pairs, pair_words)
        return cb

    b = Batcher(w.e, max_topics=64, deadline_us=200, publish=True, opts=True)
    _submit_all(b, pubs, keep, False)
    b.close()
    want_pairs = w.want_pairs(pubs, False)
    assert any(len(p) for p in want_pairs)
    for i in range(300):
        status, deliv, pick_words, pairs, n_pairs = sink.pubs[i]
        assert status == L.TM_OK and plain[i][0] == L.TM_OK
        assert pairs is None and n_pairs == len(plain[i][3]) == len(want_pairs[i])
        assert deliv == plain[i][1] and pick_words == plain[i][2]
    w.close()


def test_round_robin_plan_rerun_leaves_the_cursors_alone(gpu_device):
    """one lane, round robin.  The first batch holds subscriber ids above 65535,
    so the lane's first sub_bits (16) makes the plan report state 2 and run
    again alone; had the publish call run again too, the cursors would have
    advanced twice and the picks of this batch and the next would skip."""
    w = build_world(gpu_device)
    w.e.commit()
    base = publishes(w)
    pubs = [base[i % len(base)] for i in range(128)]
    assert any(m > 65535 for _g, _to, _t, ms in w.sets for m in ms)
    picks_model = StickySub()                                 # a second publisher process for the per-publish picks
    picks_model.tab, picks_model.alive = w.sh.tab, w.sh.alive
    sink = Sink()
    b = Batcher(w.e, max_topics=64, deadline_us=100_000, publish=True, opts=True, round_robin=True, upgrade_qos=True,
                lanes_per_replica=1, inbox=sink.on_inbox)
    tickets = _submit_all(b, pubs, sink.on_pub, True, flush_every=64)
    st = b.stats()
    b.close()
    assert len(sink.plans) == 2 and [len(p[0]) for p in sink.plans] == [64, 64]
    assert max(int(r[0]) for r in sink.plans[0][2]) > 65535   # the id that did not fit sixteen bits
    assert st["reruns"] >= 1 and st["failed_batches"] == 0
    _check_order(sink, tickets)
    _check_plans(w, sink, tickets, pubs, "round_robin", True)
    # every delivery's pick and word, dropped ones included, in submission order
    for i, (topic, key, msg) in enumerate(pubs):
        rows = route_pick_words(w.o, picks_model, w.so, "round_robin", int(key), topic, msg, True)
        _status, deliv, pick_words, _pairs, _n = sink.pubs[i]
        assert [d[3] for d in deliv] == [Engine.NO_MEMBER if m is None else m for m, _oc in rows], i
        assert pick_words == [outcome_word(oc) for _m, oc in rows], i
    w.close()
