"""Subscription options on a host-only engine: the emqx_suboption entries
(engine.cpp; do_subscribe/4, do_unsubscribe/3, get_subopts/2, set_subopts/3,
src/emqx_broker.erl:279-291, 407-415) against the reference suite's known
answers (tests/golden/kat_subopts.json) and tests/subopts_ref.py, the in-place
option pool under churn (tm_debug_check_subs after every burst), and the pure
delivery word (tm_deliver_word) against run_dispatch_steps over its whole
input space."""
import itertools
import json
import os
import random

import pytest

from dispatch_ref import SubscriberBag
from emqx_amd import Engine
from emqx_amd import _lib as L
from emqx_amd.emqx_broker import Broker, pack_msgs, pack_subopts, unpack_deliver, unpack_subopts
from emqx_amd.emqx_router import Router
from emqx_amd.engine import pack
from subopts_ref import SubOptionTable, run_dispatch_steps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kat_cases():
    with open(os.path.join(ROOT, "tests", "golden", "kat_subopts.json")) as f:
        return json.load(f)["cases"]


def _qos(opts):
    return None if opts is None else {"qos": opts["qos"]}


@pytest.mark.parametrize("case", kat_cases(), ids=lambda c: c["name"])
def test_broker_suite_subopts_known_answers(case):
    e = Engine(device=-1)
    b = Broker(e, Router(e, node="n1"))
    ref = SubOptionTable()
    for step in case["steps"]:
        op, t, rest = step[0], step[1].encode(), step[2:]
        if op == "subscribe":
            assert b.subscribe(t, rest[0], opts=rest[1]) == "ok"
            ref.do_subscribe(None, t, rest[0], rest[1])
        elif op == "unsubscribe":
            assert b.unsubscribe(t, rest[0]) == "ok"
            ref.do_unsubscribe(None, t, rest[0])
        elif op == "get_subopts":
            assert _qos(b.get_subopts(t, rest[0])) == rest[1], step
            assert _qos(ref.get_subopts(t, rest[0])) == rest[1], step
        elif op == "set_subopts":
            assert b.set_subopts(t, rest[0], rest[1]) is rest[2]
            assert ref.set_subopts(t, rest[0], rest[1]) is rest[2]
        elif op == "subscribers":
            assert b.subscribers(t) == rest[0], step          # a single bag entry after the re-subscribe
            assert ref.bag.subscribers(t) == rest[0], step
        else:
            raise AssertionError(op)
        e.debug_check_subs()
    assert e.sub_count == 0
    e.close()


def test_deliver_word_truth_table():
    """tm_deliver_word == run_dispatch_steps over stored qos 0-2 plus NONE x nl
    x rap x subid {0, 1, 2^28-1} x PubQoS 0-2 x retain x retained x same x
    upgrade"""
    e = Engine(device=-1)
    n = 0
    for sq, nl, rap, subid in itertools.product([0, 1, 2, None], [0, 1], [0, 1], [0, 1, (1 << 28) - 1]):
        if sq is None:
            word = Engine.SUBOPT_NONE | (nl << 2) | (rap << 3) | (subid << 4)   # no entry: the other bits are noise
            opts = None
        else:
            opts = {"qos": sq, "nl": nl, "rap": rap}
            if subid:
                opts["subid"] = subid
            word = pack_subopts(opts)
            assert unpack_subopts(word) == dict(opts, subid=subid or None)
        for pq, retain, retained, same, upgrade in itertools.product([0, 1, 2], [0, 1], [0, 1], [False, True],
                                                                     [False, True]):
            msg = (pq, retain, retained, 5 if same else None)
            pf, _ = pack_msgs([msg])
            got = e.deliver_word(word, pf[0], same, Engine.DELIVER_UPGRADE_QOS if upgrade else 0)
            want = run_dispatch_steps(opts, msg, same, upgrade)
            assert unpack_deliver(got) == want, (opts, msg, same, upgrade, got)
            if want is None:
                assert got == Engine.DELIVER_DROP      # exactly 8
            else:
                assert got == want[0] | want[1] << 2 | (want[2] or 0) << 4
            n += 1
    assert n == 4 * 2 * 2 * 3 * 3 * 2 * 2 * 2 * 2
    e.close()


def test_subopts_quirks():
    e = Engine(device=-1)
    t = b"a/+"
    # an option entry written through a suppressed add (:410 runs unconditionally)
    e.sub_add(t, 7)
    assert e.sub_get_opts(t, 7) is None
    e.sub_add_opts(t, 7, pack_subopts({"qos": 1, "subid": 9}), b"g1")     # suppressed by the plain 7
    assert e.subscribers(t) == [(7, Engine.NO_GROUP)]
    assert e.sub_get_opts(t, 7) == pack_subopts({"qos": 1, "subid": 9})
    e.debug_check_subs()
    # tm_sub_del with an unknown group still erases the entry, and leaves the bag
    assert e.sub_del(t, 7, b"nobody") == 1
    assert e.sub_get_opts(t, 7) is None and e.subscribers(t) == [(7, Engine.NO_GROUP)]
    e.debug_check_subs()
    # set_opts on an absent entry, and on an absent topic
    assert e.sub_set_opts(t, 7, 3, 2) is False and e.sub_get_opts(t, 7) is None
    assert e.sub_set_opts(b"no/topic", 7, 3, 2) is False
    # qos 3 refused with nothing changed: add, batch add, set
    with pytest.raises(L.TopicMatchError) as ex:
        e.sub_add_opts(t, 8, 3)
    assert ex.value.code == L.TM_EINVAL and e.subscribers(t) == [(7, Engine.NO_GROUP)]
    e.sub_add_opts(t, 8, pack_subopts({"qos": 2, "nl": 1}))
    with pytest.raises(L.TopicMatchError) as ex:
        e.sub_set_opts(t, 8, 3, 3)
    assert ex.value.code == L.TM_EINVAL and e.sub_get_opts(t, 8) == pack_subopts({"qos": 2, "nl": 1})
    with pytest.raises(L.TopicMatchError) as ex:
        e.sub_set_opts(t, 8, 1, 1)                     # 2 | 1 = 3
    assert ex.value.code == L.TM_EINVAL and e.sub_get_opts(t, 8) == pack_subopts({"qos": 2, "nl": 1})
    tb, to = pack([t, t])
    with pytest.raises(L.TopicMatchError) as ex:
        e.sub_add_opts_many(tb, to, [20, 21], [1, 7])
    assert ex.value.code == L.TM_EINVAL and e.sub_get_opts(t, 21) is None
    # merge keeps the bits outside the mask
    assert e.sub_set_opts(t, 8, Engine.SUBOPT_RAP | 0xFFFFFFF0, Engine.SUBOPT_RAP | (77 << 4)) is True
    assert unpack_subopts(e.sub_get_opts(t, 8)) == {"qos": 2, "nl": 1, "rap": 1, "subid": 77}
    e.debug_check_subs()
    # a subscriber holding both shared and plain entries shares one word
    u = b"x/y"
    e.sub_add_opts(u, 5, pack_subopts({"qos": 1}), b"g1")
    e.sub_add_opts(u, 5, pack_subopts({"qos": 2}), b"g2")          # overwrites
    e.sub_add(u, 5)                                                 # the plain entry inherits the word
    assert len(e.subscribers(u)) == 3 and e.sub_get_opts(u, 5) == 2
    e.debug_check_subs()
    assert e.sub_set_opts(u, 5, 3, 0) is True and e.sub_get_opts(u, 5) == 0
    e.debug_check_subs()
    assert e.sub_del(u, 5, b"g1") == 2                              # one shared entry goes: the word with it
    assert e.sub_get_opts(u, 5) is None
    e.debug_check_subs()
    e.close()


def test_subopts_random_churn_vs_ref():
    """3,000 ops (add with opts, add plain, del, set) over 40 topics x 60
    subscribers against the ref, the image checked after every burst; the pool
    compacts and a bag's segment doubles twice on the way"""
    rng = random.Random(1234)
    e = Engine(device=-1)
    e.set_option("route_gc", 16)
    b = Broker(e, Router(e, node="n1"))      # set_subopts' dict -> (mask, value)
    ref = SubOptionTable()
    topics = [b"t/%d" % i for i in range(36)] + [b"t/+", b"#", b"t/#", b"+/1"]
    groups = [None, None, None, b"g1", b"g2"]
    longest = hi_cap = 0

    def rand_opts():
        o = {"qos": rng.randrange(3), "nl": rng.randrange(2), "rap": rng.randrange(2)}
        if rng.random() < 0.5:
            o["subid"] = rng.choice([1, 2, 300, (1 << 28) - 1])
        return o

    for step in range(3000):
        # a few topics take most of the adds: long bags, and short ones that empty out
        t = topics[rng.randrange(4)] if rng.random() < 0.3 else rng.choice(topics)
        s, g = rng.randrange(60), rng.choice(groups)
        x = rng.random()
        held = ref.bag.subscribers(t)
        if step % 1000 >= 600 and x < 0.8 and held:
            # a draining phase: entries that exist go, bags empty and leave garbage for the compaction
            ent = rng.choice(held)
            s, g = (ent[2], ent[1]) if isinstance(ent, tuple) else (ent, None)
            assert e.sub_del(t, s, g) == ref.do_unsubscribe(g, t, s)
        elif x < 0.35:
            o = rand_opts()
            e.sub_add_opts(t, s, pack_subopts(o), g)
            ref.do_subscribe(g, t, s, o)
        elif x < 0.5:
            e.sub_add(t, s, g)
            ref.bag.insert_subscriber(g, t, s)
        elif x < 0.85:
            assert e.sub_del(t, s, g) == ref.do_unsubscribe(g, t, s)
        else:
            o = rand_opts()
            o = {k: o[k] for k in rng.sample(sorted(o), rng.randint(1, len(o)))}
            assert b.set_subopts(t, s, o) is ref.set_subopts(t, s, o)
        longest = max(longest, len([x for x in ref.bag.subscribers(t) if not isinstance(x, tuple)]))
        if step % 100 == 99:
            e.debug_check_subs()
            hi_cap = max(hi_cap, e.debug_sub_pool_stats()[4])
            for tp in topics:
                want = ref.bag.subscribers(tp)
                got = [sub if grp == Engine.NO_GROUP else ("share", e.sub_group_bytes(grp), sub)
                       for sub, grp in e.subscribers(tp)]
                assert got == want, (step, tp)
                for sub in range(60):
                    w = e.sub_get_opts(tp, sub)
                    ro = ref.get_subopts(tp, sub)
                    assert (None if w is None else unpack_subopts(w)) == \
                        (None if ro is None else dict(ro, subid=ro.get("subid"))), (step, tp, sub)
    _size, _garbage, compactions, moves, _cap = e.debug_sub_pool_stats()
    assert compactions >= 1, "the churn never compacted the pool"
    assert longest >= 5 and hi_cap >= 8 and moves >= 2, "no bag grew through two doublings (2 -> 4 -> 8)"
    e.close()


def test_legacy_calls_agree_with_dispatch_ref():
    """sub_add / sub_del without options: the bag as before, no option entry,
    and TM_SUBOPT_NONE words in the image (tm_debug_check_subs)"""
    rng = random.Random(5)
    e = Engine(device=-1)
    bag = SubscriberBag()
    topics = [b"a/%d" % i for i in range(10)] + [b"a/+", b"#"]
    for step in range(800):
        t, s = rng.choice(topics), rng.randrange(30)
        g = rng.choice([None, None, b"g1"])
        if rng.random() < 0.6:
            e.sub_add(t, s, g)
            bag.insert_subscriber(g, t, s)
        else:
            assert e.sub_del(t, s, g) == bag.delete_object(g, t, s)
    e.debug_check_subs()
    for t in topics:
        got = [sub if grp == Engine.NO_GROUP else ("share", e.sub_group_bytes(grp), sub) for sub, grp in e.subscribers(t)]
        assert got == bag.subscribers(t)
        assert all(e.sub_get_opts(t, s) is None for s in range(30))
    assert e.sub_count == bag.size()
    e.close()


def test_opts_calls_refuse_host_only_and_bad_arguments():
    e = Engine(device=-1)
    Broker(e, Router(e, node="n1"))
    tb, to = pack([b"a/b"])
    with pytest.raises(L.TopicMatchError) as ex:
        e.match_dispatch_batch(tb, to, deliver=([0], None, 0))
    assert ex.value.code == L.TM_EDEVICE                      # no CPU fallback
    with pytest.raises(L.TopicMatchError) as ex:
        e.match_dispatch_batch(tb, to, deliver=([3], None, 0))    # PubQoS 3
    assert ex.value.code == L.TM_EINVAL
    with pytest.raises(L.TopicMatchError) as ex:
        e.dispatch_batch(tb, to, deliver=([0], None, 2))          # an unknown flag
    assert ex.value.code == L.TM_EINVAL
    e.close()


def test_gpu_corpus_shows_every_outcome_in_the_reference_alone():
    """the corpus tests/test_gpu_subopts.py replays: by the reference
    restatement alone it shows all seven outcomes (downgraded without
    upgrade_qos, upgraded with it), so the GPU test's own assertion can hold"""
    import subopts_corpus as C
    from oracle import pytrie
    from subopts_ref import route_dispatch_opts
    for upgrade, never in ((False, "upgraded"), (True, "downgraded")):
        seen = set()
        for steps in C.corpus():
            o, ref = pytrie.RouteTable(), SubOptionTable()
            for step in steps:
                if step[0] != "check":
                    C.apply_ref(step, o, ref)
                    continue
                for tp, msg in zip(step[1], step[2]):
                    for to, s, res in route_dispatch_opts(o, ref, b"n1", tp, msg, upgrade)[1]:
                        seen |= C.outcomes(ref.get_subopts(to, s), msg, res)
        assert seen == set(C.OUTCOMES) - {never}, (upgrade, sorted(seen))
