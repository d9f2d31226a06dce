"""The member option pool (engine.cpp sh_opt: the emqx_suboption word of every
$share member for its set's topic, parallel to the member pool) on a host-only
engine, against tests/subopts_ref.py and tests/sticky_ref.py: random churn of
the option calls and the share calls interleaved, with tm_debug_check_shares
(which verifies the pool against the option table) and the words themselves
compared after every commit; both call orders for one (topic, subscriber);
tm_sub_del's reach; the argument checks of tm_share_pick_words and of
tm_publish_stream_opts_device with its workspace need; and the composed
reference model (tests/pickword_ref.py) on its own."""
import ctypes
import random

import numpy as np
import pytest

from pickword_ref import NO_WORD, outcome_word, pick_outcome, route_pick_words
from sticky_ref import StickySub
from subopts_corpus import rand_opts
from subopts_ref import SubOptionTable
from emqx_amd import Engine
from emqx_amd import _lib as L
from emqx_amd.emqx_broker import pack_subopts
from emqx_amd.engine import pack
from oracle import pytrie

GROUPS = [b"g1", b"g2", b"g3", b"", b"n1"]
# the awkward topics of test_shared_sub.py: empty, '#', $SYS/x, 70 bytes, an embedded NUL
TOPICS = [b"a/b", b"a/+", b"#", b"a/#", b"", b"a/b\x00", b"$SYS/x", b"+/+", b"x" * 70, b"a/b/c"]
NONE = Engine.SUBOPT_NONE


def _fid(e, filt):
    info = L.TmNodeInfo()
    rc = e.lib.tm_lookup(e.h, filt, len(filt), ctypes.byref(info))
    return None if rc == L.TM_ENOENT or info.filter_id == L.TM_NO_FILTER else info.filter_id


def _word(so, topic, sub):
    o = so.get_subopts(topic, sub)
    return NONE if o is None else pack_subopts(o)


def _same(e, sh, so):
    """the host mirror's words, set by set, against the option table"""
    for g in GROUPS:
        for t in TOPICS:
            ms = sh.subscribers(g, t)
            assert e.share_members(g, t) == ms, (g, t)
            assert e.debug_share_opts(g, t) == [_word(so, t, m) for m in ms], (g, t)
            for m in ms:                                       # and the table itself
                w = e.sub_get_opts(t, m)
                assert (NONE if w is None else w) == _word(so, t, m)


def test_new_symbols_exist():
    lib = L.load()
    for name in ("tm_share_pick_words", "tm_share_pick_words_device", "tm_debug_share_opts",
                 "tm_publish_stream_opts_device", "tm_publish_stream_opts_workspace_bytes",
                 "tm_publish_pack_opts_device", "tm_batcher_submit_publish_opts"):
        assert hasattr(lib, name), name
    assert L.TM_NO_WORD == 0xFFFFFFFF == Engine.NO_WORD


def test_member_option_pool_churn_vs_oracle():
    rng = random.Random(77)
    e, sh, so = Engine(device=-1), StickySub(), SubOptionTable()
    e.set_option("route_gc", 8)                               # pool and arena compactions happen in this test
    sub_groups = [None, b"g1", b"g2"]
    seen = set()
    for step in range(4000):
        g, t, m = rng.choice(GROUPS), rng.choice(TOPICS), rng.randrange(24)
        x = rng.random()
        if x < 0.18:                                          # do_subscribe/4: bag entry + option entry
            sg, o = rng.choice(sub_groups), rand_opts(rng)
            e.sub_add_opts(t, m, pack_subopts(o), sg)
            so.do_subscribe(None if sg is None else sg.decode(), t, m, o)
            seen.add("add_opts")
        elif x < 0.26:                                        # set_subopts/3, often without an entry
            o = rand_opts(rng)
            mask = 3 | Engine.SUBOPT_NL | Engine.SUBOPT_RAP | (0xFFFFFFF0 if "subid" in o else 0)
            assert e.sub_set_opts(t, m, mask, pack_subopts(o)) == so.set_subopts(t, m, o)
            seen.add("set_opts")
        elif x < 0.38:                                        # do_unsubscribe/3: erases the entry whatever the group
            sg = rng.choice(sub_groups)
            assert e.sub_del(t, m, sg) == so.do_unsubscribe(None if sg is None else sg.decode(), t, m)
            seen.add("sub_del")
        elif x < 0.44:                                        # insert_subscriber/3 alone: no entry
            sg = rng.choice(sub_groups)
            e.sub_add(t, m, sg)
            so.bag.insert_subscriber(None if sg is None else sg.decode(), t, m)
            seen.add("sub_add")
        elif x < 0.74:
            e.share_add(g, t, m)
            sh.subscribe(g, t, m)
            seen.add("share_add")
        elif x < 0.88:
            assert e.share_del(g, t, m) == sh.unsubscribe(g, t, m)
            seen.add("share_del")
        elif x < 0.93:
            assert e.share_member_down(m) == sh.cleanup_down(m)
            seen.add("member_down")
        else:                                                 # the trie changes behind the tables' backs
            f = rng.choice([tp for tp in TOPICS if b"+" in tp or b"#" in tp])
            if _fid(e, f) is None:
                e.insert(f)
            else:
                e.delete(f)
            seen.add("trie")
        if step % 50 == 49:
            e.commit()
            e.debug_check_shares()
            e.debug_check_subs()
        if step % 400 == 399:
            _same(e, sh, so)
    assert len(seen) == 8
    _same(e, sh, so)
    for m in range(24):
        assert e.share_member_down(m) == sh.cleanup_down(m)
    e.commit()
    e.debug_check_shares()
    assert e.share_count == 0
    e.close()


@pytest.mark.parametrize("order", ["option_first", "share_first"])
def test_both_call_orders(order):
    """the two tables are independent: whichever is fed first, the member's
    word is the option entry; tm_sub_del turns it to TM_SUBOPT_NONE in every
    set of that topic and in no other topic's sets"""
    e = Engine(device=-1)
    w = pack_subopts({"qos": 2, "nl": 1, "rap": 1, "subid": 17})
    w2 = pack_subopts({"qos": 1, "rap": 1})
    if order == "option_first":
        e.sub_add_opts(b"t/+", 5, w, b"g1")
        e.sub_add_opts(b"u", 5, w2, b"g1")
    for g in (b"g1", b"g2"):
        e.share_add(g, b"t/+", 4)                             # a neighbour without an entry
        e.share_add(g, b"t/+", 5)
    e.share_add(b"g1", b"u", 5)
    if order == "share_first":
        e.commit()
        assert e.debug_share_opts(b"g1", b"t/+") == [NONE, NONE]
        e.sub_add_opts(b"t/+", 5, w, b"g1")
        e.sub_add_opts(b"u", 5, w2, b"g1")
    e.commit()
    e.debug_check_shares()
    assert e.sub_get_opts(b"t/+", 5) == w
    for g in (b"g1", b"g2"):
        assert e.debug_share_opts(g, b"t/+") == [NONE, w]
    assert e.debug_share_opts(b"g1", b"u") == [w2]
    # set_subopts reaches every set of the topic
    assert e.sub_set_opts(b"t/+", 5, 3, 0)
    e.commit()
    e.debug_check_shares()
    for g in (b"g1", b"g2"):
        assert e.debug_share_opts(g, b"t/+") == [NONE, (w & ~3)]
    assert e.debug_share_opts(b"g1", b"u") == [w2]
    # the segment doubles (2 -> 4 -> 8): the words move with the members
    for m in range(10, 16):
        e.share_add(b"g1", b"t/+", m)
    e.commit()
    e.debug_check_shares()
    assert e.debug_share_opts(b"g1", b"t/+") == [NONE, (w & ~3)] + [NONE] * 6
    # do_unsubscribe/3 erases the entry whatever the group: the word goes in every set of t/+, u keeps its own
    e.sub_del(b"t/+", 5, b"g2")
    e.commit()
    e.debug_check_shares()
    assert e.sub_get_opts(b"t/+", 5) is None
    assert e.debug_share_opts(b"g1", b"t/+") == [NONE] * 8
    assert e.debug_share_opts(b"g2", b"t/+") == [NONE, NONE]
    assert e.debug_share_opts(b"g1", b"u") == [w2]
    # the topic's last subscriber goes, and its record with it, while the set still holds the member
    assert e.sub_del(b"u", 5, b"g1") == 0
    e.commit()
    e.debug_check_shares()
    assert e.debug_share_opts(b"g1", b"u") == [NONE]
    assert e.debug_share_opts(b"nobody", b"u") == []
    e.close()


def test_pick_words_argument_checks_host_only():
    e = Engine(device=-1)
    lib = e.lib
    tb, to = pack([b"a"])
    one = np.zeros(1, dtype=np.uint32)
    off = np.zeros(2, dtype=np.uint64)
    pf = np.zeros(1, dtype=np.uint32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)   # noqa: E731

    def call(dv, topic_off=to, offs=off, words=one, out_cap=1):
        return lib.tm_share_pick_words(e.h, p(tb), None if topic_off is None else p(topic_off), 1, p(one),
                                       None if offs is None else p(offs), p(one), p(one), p(one), out_cap, 1,
                                       None if dv is None else ctypes.byref(dv), None if words is None else p(words))

    good = L.TmDeliver(p(pf), None, 0, 0, None)
    assert call(good) == L.TM_EDEVICE                         # host-only: the pass runs on the GPU only
    assert call(None) == L.TM_EINVAL
    assert call(L.TmDeliver(None, None, 0, 0, None)) == L.TM_EINVAL          # no pub_flags
    assert call(L.TmDeliver(p(pf), None, 2, 0, None)) == L.TM_EINVAL         # unknown flag
    assert call(L.TmDeliver(p(pf), None, 0, 0, p(one))) == L.TM_EINVAL       # sub_deliver must be NULL
    assert call(good, topic_off=None) == L.TM_EINVAL
    assert call(good, offs=None) == L.TM_EINVAL
    assert call(good, words=None) == L.TM_EINVAL
    assert call(good, words=None, out_cap=0) == L.TM_EDEVICE
    bad_qos = np.array([3], dtype=np.uint32)
    assert call(L.TmDeliver(p(bad_qos), None, 0, 0, None)) == L.TM_EINVAL    # PubQoS 3, host form
    # the device form: the same descriptor checks, null planes
    dcall = lambda dv, tot=p(off): lib.tm_share_pick_words_device(   # noqa: E731
        e.h, None, p(off), 1, p(one), p(off), p(one), p(one), p(one), 1, tot,
        None if dv is None else ctypes.byref(dv), p(one), None)
    assert dcall(good) == L.TM_EDEVICE
    assert dcall(None) == L.TM_EINVAL
    assert dcall(good, None) == L.TM_EINVAL
    assert dcall(L.TmDeliver(p(pf), None, 0, 0, p(one))) == L.TM_EINVAL
    with pytest.raises(L.TopicMatchError):
        e.share_pick_words(tb, to, one, off, one, one, one, (pf, None, 0))
    e.close()


def test_stream_opts_workspace_and_host_only():
    """the call with options has a workspace need of its own (the plain one's
    is what it was: a prefix of it), and is refused host-only after its checks"""
    e = Engine(device=-1)
    for n, caps in ((1, (8, 8, 8, 0)), (700, (50_000, 40_000, 30_000, 5_000)), (0, (0, 0, 0, 0))):
        plain = e.publish_stream_workspace_bytes(n, 64, caps)
        need = e.publish_stream_opts_workspace_bytes(n, 64, caps)
        # two more planes of caps.routes + 1 words, each rounded up to 256 B
        assert need == plain + 2 * (((caps[1] + 1) * 4 + 255) // 256 * 256)
    one = np.zeros(16, dtype=np.uint32)
    off = np.zeros(2, dtype=np.uint64)
    ws = np.zeros(e.publish_stream_opts_workspace_bytes(1, 1, (8, 8, 8, 0)), dtype=np.uint8)
    args = (one, off, 1, 1, Engine.SHARE_KEYED, one, None, (8, 8, 8, 0), ws, len(ws), one, one, one, one, one)
    as_ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    good = (as_ptr(one), None, 0, as_ptr(one))
    with pytest.raises(L.TopicMatchError) as ei:
        e.publish_stream_opts_device(*[as_ptr(x) if isinstance(x, np.ndarray) else x for x in args], good, as_ptr(one))
    assert ei.value.code == L.TM_EDEVICE
    for dv, pkw in ((None, as_ptr(one)), ((None, None, 0, as_ptr(one)), as_ptr(one)),
                    ((as_ptr(one), None, 0, None), as_ptr(one)), ((as_ptr(one), None, 8, as_ptr(one)), as_ptr(one)),
                    (good, None)):
        with pytest.raises(L.TopicMatchError) as ei:
            e.publish_stream_opts_device(*[as_ptr(x) if isinstance(x, np.ndarray) else x for x in args], dv, pkw)
        assert ei.value.code == L.TM_EINVAL
    e.close()


def test_batcher_flags_and_submit_kinds():
    """tm_batcher_open / submit: the TM_EINVAL matrix of the options mode; on a
    host-only engine an options submit completes with TM_EDEVICE and nothing"""
    from emqx_amd.batcher import Batcher
    e = Engine(device=-1)
    for kw in (dict(opts=True), dict(opts=True, deliveries=True), dict(publish=True, upgrade_qos=True),
               dict(upgrade_qos=True)):
        with pytest.raises(L.TopicMatchError) as ei:
            Batcher(e, **kw)
        assert ei.value.code == L.TM_EINVAL, kw
    nop = lambda *a: None   # noqa: E731
    for kw in (dict(publish=True, opts=True), dict(publish=True, opts=True, upgrade_qos=True, sticky=True),
               dict(publish=True, opts=True, round_robin=True)):
        b = Batcher(e, max_topics=8, deadline_us=50, **kw)
        for bad in (lambda: b.submit(b"a", nop), lambda: b.submit_publish(b"a", 1, nop),
                    lambda: b.submit_publish_opts(b"a", 1, 3, 0, nop),           # PubQoS 3
                    lambda: b.submit_publish_opts(b"a", 1, 7 | 8, 0, nop)):
            with pytest.raises(L.TopicMatchError) as ei:
                bad()
            assert ei.value.code == L.TM_EINVAL
        got = []
        b.submit_publish_opts(b"a/b", 1, 2 | 4, 0xFFFFFFFF, lambda *a: got.append(a))
        b.submit_publish_opts(b"", 2, 0, 5, lambda *a: got.append(a))
        b.flush()
        assert got == [(L.TM_EDEVICE, None, None, None, None)] * 2
        st = b.stats()
        assert st["topics"] == 2 and st["failed_batches"] >= 1      # nothing was queued by the refused submits
        b.close()
    for kw in (dict(publish=True), dict(), dict(publish=True, sticky=True)):     # without the flag: the reverse
        b = Batcher(e, max_topics=8, deadline_us=50, **kw)
        with pytest.raises(L.TopicMatchError) as ei:
            b.submit_publish_opts(b"a", 1, 0, 0, nop)
        assert ei.value.code == L.TM_EINVAL
        b.close()
    e.close()


def test_reference_model_alone():
    """the composed model on its own: no pick and a stuck member outside its
    set have no word; a no-local member that published is dropped (exactly
    TM_DELIVER_DROP); a member without an entry gets the message as it is"""
    o, sh, so = pytrie.RouteTable(), StickySub(), SubOptionTable()
    o.add_route(b"s/+", ("g", "n1"))
    o.add_route(b"s/+", "n2")
    for m in (1, 2, 3):
        sh.subscribe(b"g", b"s/+", m)
    so.do_subscribe("g", b"s/+", 2, {"qos": 1, "nl": 1, "rap": 0, "subid": 9})
    msg = (2, 1, 0, 2)
    assert pick_outcome(so, sh, b"g", b"s/+", None, msg) == NO_WORD
    assert outcome_word(pick_outcome(so, sh, b"g", b"s/+", 2, msg)) == 8
    assert pick_outcome(so, sh, b"g", b"s/+", 2, (2, 1, 0, None)) == (1, 0, 9)
    assert pick_outcome(so, sh, b"g", b"s/+", 2, (2, 1, 0, None), upgrade=True) == (2, 0, 9)
    assert outcome_word(pick_outcome(so, sh, b"g", b"s/+", 1, msg)) == 2 | 4
    rows = route_pick_words(o, sh, so, "sticky", 1, b"s/x", (0, 0, 1, None))
    assert sorted(rows, key=str) == sorted([(None, NO_WORD), (2, (0, 1, 9))], key=str)
    sh.unsubscribe(b"g", b"s/+", 2)                           # stuck, alive, no longer a member
    rows = route_pick_words(o, sh, so, "sticky", 0, b"s/x", (0, 0, 1, None))
    assert (2, NO_WORD) in rows
    assert outcome_word(NO_WORD) == 0xFFFFFFFF
