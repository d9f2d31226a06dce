"""The delivery word of a $share pick on the GPU (share.hip
tm_share_pick_words over the member option pool, ShareView::opt) against
tests/pickword_ref.py: for every live slot of a publish call's planes,
handle_dispatch/3 + run_dispatch_steps/3 (src/emqx_session.erl:667-684,
797-819) over the picked member's option entry for the set's topic; no word
for a slot without a pick and for a stuck member outside its set; holes and
slots past the bound untouched.  Member sets of 1, 2, 7, 8, 9, 63, 64, 65 and
130 members sit on both sides of the kernel's lane-scan / wave-scan switch and
of a wave boundary."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pickword_world import (GUARD, STRATEGIES, DevPublish, build_world, check_planes, deliver_of, publishes,  # noqa: E402
                            u32)
from emqx_amd import Engine  # noqa: E402
from emqx_amd.engine import pack  # noqa: E402

pytestmark = pytest.mark.gpu

DROP = Engine.DELIVER_DROP
NO_WORD = Engine.NO_WORD


def _host(w, pubs, strategy, upgrade, tag=None):
    """the host publish call + the host post-pass against the model (which
    advances with it) -> (planes, words, (worded, bare))"""
    buf, off = pack([t for t, _k, _m in pubs])
    dv = deliver_of(pubs, upgrade)
    want = w.want(strategy, pubs, upgrade)
    out = w.e.match_publish_batch(buf, off, STRATEGIES[strategy], keys=[k for _t, k, _m in pubs], deliver=dv)
    counts, offs, to, tg, pick = out[0], out[1], out[2], out[3], out[9]
    words = np.full(len(to) + 8, GUARD, dtype=np.uint32)
    w.e.share_pick_words(buf, off, counts, offs, to, tg, pick, dv, pick_word=words)
    stats = check_planes(want, counts, offs, pick, words, len(to), tag)
    return out, words, stats


@pytest.mark.parametrize("upgrade", [False, True])
@pytest.mark.parametrize("strategy", ["keyed", "round_robin", "sticky"])
def test_post_pass_host_and_device(gpu_device, strategy, upgrade):
    w = build_world(gpu_device)
    pubs = publishes(w)
    out, words, (worded, bare) = _host(w, pubs, strategy, upgrade, "host")
    assert worded >= 40 and bare >= 50, (worded, bare)
    total = len(out[2])
    assert int(out[1][-1]) > int(out[0].sum())               # the planes have holes
    if strategy == "keyed":
        # the forced picks: first, middle and last member of every set; the last is the publisher with
        # no-local set, its word exactly TM_DELIVER_DROP
        drops = 0
        for t, (topic, key, msg) in enumerate(pubs):
            for g, _to, tp, ms in w.sets:
                if tp == topic:
                    a, c = int(out[1][t]), int(out[0][t])
                    got = [int(p) for p in out[9][a:a + c] if int(p) != Engine.NO_MEMBER]
                    assert got == [ms[key % len(ms)]] == [msg[3]], topic
                    if msg[3] == ms[-1]:
                        wd = [int(x) for x in words[a:a + c] if int(x) != NO_WORD]
                        assert wd == [DROP], topic
                        drops += 1
        assert drops == len(w.sets)
        # the convenience form returns the same words
        buf, off = pack([t for t, _k, _m in pubs])
        res = w.e.match_publish_batch(buf, off, Engine.SHARE_KEYED, keys=[k for _t, k, _m in pubs],
                                      deliver=deliver_of(pubs, upgrade), pick_words=True)
        assert len(res) == 12
        live = words[:total] != GUARD
        assert (res[11][live] == words[:total][live]).all()
        # and the broker mirror hands each pick its session-side outcome
        from emqx_amd.emqx_broker import unpack_deliver
        got = w.b.publish_shared_many([t for t, _k, _m in pubs], "keyed", [k for _t, k, _m in pubs],
                                      msgs=[m for _t, _k, m in pubs], upgrade_qos=upgrade)
        for pub, rows in zip(got, w.want("keyed", pubs, upgrade)):
            assert [x for x in pub.pick_deliver if x is not False] == [unpack_deliver(wd) for m, wd in rows
                                                                       if m != Engine.NO_MEMBER]
    # the device form over the device call's planes (the model advances once more)
    want = w.want(strategy, pubs, upgrade)
    d = DevPublish(w.e, gpu_device, pubs, STRATEGIES[strategy], total + 16, 4096)
    pw = u32(d.words(deliver_of(pubs, upgrade)))
    assert int(d.tot.item()) == total
    check_planes(want, u32(d.c), u32(d.o).view(np.uint64), u32(d.pk), pw, total, "device")
    w.close()


def test_out_cap_below_the_total(gpu_device):
    """slots at or past min(total, out_cap) are not written, in both forms"""
    w = build_world(gpu_device)
    pubs = publishes(w)
    out, words, _ = _host(w, pubs, "keyed", False)
    total = len(out[2])
    cap = total - 37
    want = w.want("keyed", pubs)
    d = DevPublish(w.e, gpu_device, pubs, Engine.SHARE_KEYED, cap, 4096)
    assert int(d.tot.item()) == total > cap
    pw = u32(d.words(deliver_of(pubs, False), extra=64))
    check_planes(want, u32(d.c), u32(d.o).view(np.uint64), u32(d.pk), pw, cap, "device cap")
    # the host form over the full planes with a smaller out_cap
    buf, off = pack([t for t, _k, _m in pubs])
    hw = np.full(total + 8, GUARD, dtype=np.uint32)
    w.e.share_pick_words(buf, off, out[0], out[1], out[2], out[3], out[9], deliver_of(pubs, False), total=total,
                         out_cap=cap, pick_word=hw)
    check_planes(want, out[0], out[1], out[9], hw, cap, "host cap")
    assert (hw[:cap] == words[:cap]).all()
    # an empty batch writes nothing
    e0 = np.zeros(0, dtype=np.uint32)
    hw[:] = GUARD
    w.e.share_pick_words(np.zeros(8, np.uint8), np.zeros(1, np.uint64), e0, np.zeros(1, np.uint64), e0, e0, e0,
                         (e0, None, 0), total=0, out_cap=0, pick_word=hw)
    assert (hw == GUARD).all()
    w.close()


def test_sticky_member_outside_its_set(gpu_device):
    """a stuck member that unsubscribed from its set is still picked (as the
    reference allows) and gets TM_NO_WORD: the one case the device does not
    answer; back in the set, the word is the model's again"""
    w = build_world(gpu_device)
    g, to, topic, ms = next(s for s in w.sets if len(s[3]) == 65)
    m = ms[64]                                               # the member a key of 64 draws, in the second wave step
    pubs = [(topic, 64, (1, 1, 0, None)), (topic, 3, (2, 0, 0, m))]
    out, words, _ = _host(w, pubs, "sticky", False, "stuck")
    assert [int(p) for p in out[9] if int(p) != Engine.NO_MEMBER] == [m, m]
    assert sorted(int(x) for x in words[:len(out[2])] if int(x) not in (NO_WORD, GUARD)) == sorted(
        [w.e.deliver_word(w.e.sub_get_opts(to, m), 1 | 4, False), DROP])
    w.unshare(g, to, m)                                      # the set keeps 64 members
    w.e.commit()
    out, words, _ = _host(w, pubs, "sticky", False, "outside")
    assert [int(p) for p in out[9] if int(p) != Engine.NO_MEMBER] == [m, m]
    assert all(int(x) in (NO_WORD, GUARD) for x in words)    # no word at all for these two publishes' picks
    # the caller's fallback gives the outcome
    assert w.e.deliver_word(w.e.sub_get_opts(to, m), 2, True) == DROP
    pub = w.b.publish_shared_many([topic], "sticky", [3], msgs=[(2, 0, 0, m)])[0]     # the broker mirror does that
    assert pub.picks == [(to, g, m)] and pub.pick_deliver == [None]
    w.e.share_add(g, to, m)
    w.sh.subscribe(g, to, m)
    w.e.commit()
    out, words, (worded, _bare) = _host(w, pubs, "sticky", False, "back")
    assert worded == 2
    w.close()


def test_options_follow_changes(gpu_device):
    w = build_world(gpu_device)
    pubs = publishes(w)
    out0, words0, _ = _host(w, pubs, "keyed", False, "before")
    # set_subopts + commit changes exactly the affected words: the first member of the 64-member wildcard set
    g, to, topic, ms = next(s for s in w.sets if len(s[3]) == 64 and s[1].endswith(b"+"))
    old = w.so.get_subopts(to, ms[0])
    new = {"qos": (old["qos"] + 1) % 3, "nl": 0, "subid": 4097}
    w.set_opts(to, ms[0], new)
    w.e.commit()
    out1, words1, _ = _host(w, pubs, "keyed", False, "set_opts")
    changed = np.nonzero(words0 != words1)[0]
    t = next(i for i, p in enumerate(pubs) if p[0] == topic and p[1] % 64 == 0)
    assert len(changed) == 1 and int(out1[1][t]) <= int(changed[0]) < int(out1[1][t]) + int(out1[0][t])
    assert int(words1[changed[0]]) >> 4 == 4097
    # a set grown past its segment capacity (9 -> 17 members: 16 doubles to 32) keeps every word right
    g9, to9, _topic9, ms9 = next(s for s in w.sets if len(s[3]) == 9 and s[1].endswith(b"t"))
    for k in range(8):
        w.member(g9, to9, 900000 + k, {"qos": 2, "rap": 1, "subid": 1 + k} if k % 2 else None, share_first=bool(k % 4))
    ms9.extend(900000 + k for k in range(8))
    w.e.commit()
    w.e.debug_check_shares()
    pubs2 = pubs + [(to9, 9 + k, (1, 1, 0, None)) for k in range(8)]
    _host(w, pubs2, "keyed", True, "doubled")
    # a compaction: the segments' doublings left garbage just under half of the pool; the largest set
    # dropped whole takes it past half, and a shrunken set stays in place
    w.e.set_option("route_gc", 8)
    g130, to130, _t, ms130 = next(s for s in w.sets if len(s[3]) == 130 and s[1].endswith(b"+"))
    for m in ms130[1:100]:
        w.unshare(g130, to130, m)
    del ms130[1:100]
    gx, tox, _t, msx = next(s for s in w.sets if len(s[3]) == 130 and s[1].endswith(b"t"))
    for m in msx:
        w.unshare(gx, tox, m)
    del msx[:]
    w.e.commit()
    w.e.debug_check_shares()
    _host(w, pubs2, "keyed", False, "compacted")
    w.close()


def test_batch_enqueued_before_a_commit_keeps_its_words(gpu_device):
    """two epochs: the pass reads the image it was launched on while the host
    changes an option and commits"""
    import torch
    w = build_world(gpu_device)
    pubs = publishes(w)
    dv = deliver_of(pubs, False)
    want_old = w.want("keyed", pubs)
    d = DevPublish(w.e, gpu_device, pubs, Engine.SHARE_KEYED, 4096, 4096)
    total = int(d.tot.item())
    st = torch.cuda.Stream(device=gpu_device)
    d.prepare(dv)
    with torch.cuda.stream(st):
        torch.cuda._sleep(5_000_000)                         # a short spin ahead of the pass
    d.launch(stream=st)
    pw = d.pw
    g, to, topic, ms = next(s for s in w.sets if len(s[3]) == 7 and s[1].endswith(b"+"))
    w.set_opts(to, ms[0], {"qos": (w.so.get_subopts(to, ms[0])["qos"] + 1) % 3, "subid": 77})
    w.e.commit()
    st.synchronize()
    torch.cuda.synchronize()
    # the model's words as they were before the change
    check_planes(want_old, u32(d.c), u32(d.o).view(np.uint64), u32(d.pk), u32(pw), total, "old epoch")
    want_new = w.want("keyed", pubs)
    assert want_new != want_old
    pw2 = u32(d.words(dv)).copy()
    check_planes(want_new, u32(d.c), u32(d.o).view(np.uint64), u32(d.pk), pw2, total, "new epoch")
    w.close()
