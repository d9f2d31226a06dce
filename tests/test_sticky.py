"""`sticky` and the retry picks without a GPU: the oracle (tests/sticky_ref.py)
on sequences worked out by hand from src/emqx_shared_sub.erl:211-249 and
:327-334, the argument checks of the new entries on a host-only engine, the
batcher's flag combinations, and the ctypes mirror against the header."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from sticky_ref import StickySub, route_pick  # noqa: E402
from emqx_amd import Engine  # noqa: E402
from emqx_amd import _lib as L  # noqa: E402
from emqx_amd.emqx_shared_sub import STRATEGIES, SharedSub  # noqa: E402
from emqx_amd.engine import pack  # noqa: E402
from oracle import pytrie  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, T = b"g", b"t"
KEY = ("shared_sub_sticky", G, T)


def _set(members):
    sh = StickySub()
    for m in members:
        sh.subscribe(G, T, m)
    return sh


# ---- the oracle, by hand ----------------------------------------------------------------------------------

def test_oracle_sticks_and_ignores_membership():
    sh = _set([1, 2, 3])
    assert sh.pick("sticky", 4, G, T) == 2              # undefined: random, member (4 rem 3) = the second
    assert sh.pd[KEY] == 2
    assert sh.pick("sticky", 0, G, T) == 2              # is_active_sub(2, []): alive -> Sub0, the key plays no part
    assert sh.unsubscribe(G, T, 2) == 2                 # still a process: is_active_sub does not look at the table
    assert [sh.pick("sticky", k, G, T) for k in (0, 1, 5)] == [2, 2, 2]
    assert sh.subscribers(G, T) == [1, 3]


def test_oracle_down_picks_again_with_the_publishs_key():
    sh = _set([1, 2, 3])
    assert sh.pick("sticky", 1, G, T) == 2
    assert sh.cleanup_down(2) == 1
    assert sh.pick("sticky", 3, G, T) == 3              # [1, 3]: member (3 rem 2) = the second
    assert sh.pick("sticky", 0, G, T) == 3
    sh.subscribe(G, T, 2)                               # the same u32 again is a new process: 3 stays
    assert sh.pick("sticky", 2, G, T) == 3
    sh.cleanup_down(3)
    sh.cleanup_down(9)                                  # never a member: nothing to do
    assert sh.pick("sticky", 1, G, T) == 2              # [1, 2]: member (1 rem 2)


def test_oracle_a_stuck_number_that_comes_back_is_a_new_process():
    sh = _set([1, 2])
    assert sh.pick("sticky", 1, G, T) == 2
    sh.unsubscribe(G, T, 2)                             # unsubscribed everywhere, alive: still picked
    assert sh.pick("sticky", 0, G, T) == 2
    assert sh.cleanup_down(2) == 0                      # then it exits: no record left, the entry goes all the same
    sh.subscribe(G, T, 2)                               # [1, 2] again, 2 a new process
    assert sh.pick("sticky", 0, G, T) == 1              # undefined: member (0 rem 2)


def test_oracle_single_member_sticks_through_growth():
    sh = _set([7])
    assert sh.pick("sticky", 5, G, T) == 7              # [Sub] -> Sub, and put all the same (:222)
    assert sh.pd[KEY] == 7
    sh.subscribe(G, T, 8)
    sh.subscribe(G, T, 9)
    assert [sh.pick("sticky", k, G, T) for k in (1, 2)] == [7, 7]


def test_oracle_failed_subs_cover_everyone_and_the_stuck_member():
    sh = _set([1, 2])
    assert sh.pick("sticky", 0, G, T, [1, 2]) is None   # [] -> false, stored: reads as undefined
    assert sh.pd[KEY] is None
    assert sh.pick("sticky", 1, G, T) == 2              # picks again: member (1 rem 2)
    assert sh.pick("sticky", 0, G, T, [2]) == 1         # the stuck member failed: [1] -> 1, stored
    assert sh.pick("sticky", 1, G, T) == 1
    assert sh.pick("sticky", 1, G, T, [5]) == 1         # a failed non-member changes nothing
    assert sh.pick("sticky", 0, b"none", T, [1]) is None


def test_oracle_retry_of_keyed_and_round_robin():
    sh = _set([1, 2, 3, 4])
    assert sh.pick("keyed", 5, G, T, [2]) == 4          # [1, 3, 4]: member (5 rem 3) = the third
    assert sh.pick("keyed", 5, G, T, [1, 2, 4]) == 3    # [Sub] -> Sub
    assert sh.pick("keyed", 5, G, T, [4, 3, 2, 1]) is None
    sh = _set([1, 2, 3])
    assert sh.pick("round_robin", 0, G, T) == 1         # undefined -> Rem 0
    assert sh.pick("round_robin", 0, G, T, [1]) == 3    # [2, 3], Count' = 2: (0 + 1) rem 2 = 1
    assert sh.pick("round_robin", 0, G, T, [1, 2]) == 3  # [Sub] -> Sub: the cursor stays 1
    assert sh.pd[("shared_sub_round_robin", G, T)] == 1
    assert sh.pick("round_robin", 0, G, T, [1, 2, 3]) is None
    assert sh.pick("round_robin", 0, G, T) == 3         # (1 + 1) rem 3 = 2


def test_oracle_emptied_set_forgets_and_a_publish_goes_through_route():
    sh = _set([1, 2])
    o = pytrie.RouteTable()
    o.add_route(T, ("g", "n1"))
    o.add_route(T, "n2")
    for key in (1, 0):                                  # the second publish finds the entry
        assert sorted(route_pick(o, sh, "sticky", key, T), key=lambda m: m is None) == [2, None]
    sh.unsubscribe(G, T, 1)
    sh.unsubscribe(G, T, 2)
    assert KEY not in sh.pd                             # the stated deviation: the entry goes with the set
    sh.subscribe(G, T, 1)
    sh.subscribe(G, T, 2)
    assert sh.pick("sticky", 0, G, T) == 1              # 2 is alive, but nothing remembers it


# ---- the new entries on a host-only engine --------------------------------------------------------------------

@pytest.fixture()
def eng():
    e = Engine(device=-1)
    e.set_local_node(b"n1")
    yield e
    e.close()


P = ctypes.c_void_p(4096)       # a non-null pointer no check may follow


def _pick(e, **kw):
    off = (ctypes.c_uint64 * 3)(0, 1, 2)
    foff = (ctypes.c_uint64 * 3)(0, 0, 0)
    a = dict(h=e.h, strategy=Engine.SHARE_STICKY, cursors=None, groups=b"gg", goff=off, topics=b"tt", toff=off,
             keys=(ctypes.c_uint32 * 2)(1, 2), failed=None, foff=foff, n=2, out=(ctypes.c_uint32 * 2)())
    a.update(kw)
    c = lambda x: ctypes.cast(x, ctypes.c_void_p) if x is not None and not isinstance(x, ctypes.c_void_p) else x  # noqa: E731
    return e.lib.tm_share_pick_batch(a["h"], a["strategy"], a["cursors"], c(a["groups"]), c(a["goff"]), c(a["topics"]),
                                     c(a["toff"]), c(a["keys"]), c(a["failed"]), c(a["foff"]), a["n"], c(a["out"]))


def test_pick_batch_needs_a_device(eng):
    for strategy in (Engine.SHARE_KEYED, Engine.SHARE_ROUND_ROBIN, Engine.SHARE_STICKY):
        assert _pick(eng, strategy=strategy) == L.TM_EDEVICE
    assert _pick(eng, strategy=Engine.SHARE_ROUND_ROBIN, keys=None) == L.TM_EDEVICE   # round robin takes no key
    assert _pick(eng, n=0, goff=None, toff=None, foff=None, keys=None, out=None) == L.TM_EDEVICE
    with pytest.raises(L.TopicMatchError) as ei:
        SharedSub(eng, "sticky").pick("g", b"t", 1, [2])
    assert ei.value.code == L.TM_EDEVICE


@pytest.mark.parametrize("kw", [
    dict(strategy=0), dict(strategy=4),                                                # an unknown strategy
    dict(goff=None), dict(toff=None), dict(foff=None), dict(out=None),                 # null arrays with n > 0
    dict(keys=None), dict(strategy=Engine.SHARE_KEYED, keys=None),                     # a keyed strategy without keys
    dict(groups=None), dict(topics=None),                                              # bytes named by the offsets
    dict(foff=(ctypes.c_uint64 * 3)(0, 2, 3)),                                         # failed members, no array
    dict(foff=(ctypes.c_uint64 * 3)(0, 2, 1), failed=(ctypes.c_uint32 * 4)()),         # offsets not monotone
    dict(h=None),
], ids=lambda kw: ",".join(sorted(kw)) + "=" + str(kw.get("strategy", "")))
def test_pick_batch_argument_checks(eng, kw):
    assert _pick(eng, **kw) == L.TM_EINVAL


def test_publish_calls_take_the_strategy(eng):
    buf, off = pack([b"a"])
    with pytest.raises(L.TopicMatchError) as ei:
        eng.match_publish_batch(buf, off, Engine.SHARE_STICKY, [5])
    assert ei.value.code == L.TM_EDEVICE                 # past the argument checks
    with pytest.raises(L.TopicMatchError) as ei:
        eng.match_publish_batch(buf, off, Engine.SHARE_STICKY, None)
    assert ei.value.code == L.TM_EINVAL                  # pub_key is required as for KEYED
    assert STRATEGIES["sticky"] == Engine.SHARE_STICKY == 3
    assert SharedSub(eng, "sticky").strategy == "sticky"


def test_member_down_of_a_member_without_records(eng):
    assert eng.share_member_down(77) == 0                # reported all the same; the commit has nothing to reset
    eng.commit()
    eng.share_add(b"g", b"t", 77)
    assert eng.share_member_down(77) == 1
    eng.commit()
    assert eng.share_count == 0


# ---- the batcher's flag ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [L.TM_BATCHER_STICKY,
                                   L.TM_BATCHER_STICKY | L.TM_BATCHER_EAGER,
                                   L.TM_BATCHER_STICKY | L.TM_BATCHER_STREAM,
                                   L.TM_BATCHER_STICKY | L.TM_BATCHER_PUBLISH | L.TM_BATCHER_ROUND_ROBIN,
                                   L.TM_BATCHER_STICKY | L.TM_BATCHER_PUBLISH | L.TM_BATCHER_DELIVERIES])
def test_batcher_sticky_flag_refused(eng, flags):
    cfg = L.TmBatcherConfig(100, 100, 0, flags, 1, 0)
    h = ctypes.c_void_p()
    assert eng.lib.tm_batcher_open(eng.h, ctypes.byref(cfg), ctypes.byref(h)) == L.TM_EINVAL
    assert not h.value


@pytest.mark.parametrize("more", [0, L.TM_BATCHER_EAGER, L.TM_BATCHER_STREAM])
def test_batcher_sticky_flag_opens_with_publish_mode(eng, more):
    from emqx_amd.batcher import Batcher
    b = Batcher(eng, publish=True, sticky=True, flags=more, lanes_per_replica=1)
    got = []
    b.submit_publish(b"a/b", 7, lambda status, d, p: got.append((status, d, p)))
    b.flush()
    assert got == [(L.TM_EDEVICE, None, None)]           # host-only: the stream-ordered call's answer
    b.close()


# ---- the mirror against the header -----------------------------------------------------------------------------

def _header():
    txt = open(os.path.join(ROOT, "include", "topicmatch.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_mirror_matches_the_header():
    txt = _header()
    defs = dict(re.findall(r"#define\s+(TM_[A-Z_]+)\s+(\d+)u\b", txt))
    assert int(defs["TM_SHARE_STICKY"]) == Engine.SHARE_STICKY == 3
    assert int(defs["TM_SHARE_KEYED"]) == Engine.SHARE_KEYED and int(defs["TM_SHARE_ROUND_ROBIN"]) == Engine.SHARE_ROUND_ROBIN
    assert int(defs["TM_BATCHER_STICKY"]) == L.TM_BATCHER_STICKY == 128
    flags = [int(defs[k]) for k in ("TM_BATCHER_ROUTES", "TM_BATCHER_DELIVERIES", "TM_BATCHER_EAGER", "TM_BATCHER_CSR",
                                    "TM_BATCHER_PUBLISH", "TM_BATCHER_ROUND_ROBIN", "TM_BATCHER_STREAM",
                                    "TM_BATCHER_STICKY")]
    assert len(set(flags)) == 8 and all(f & (f - 1) == 0 for f in flags)   # one bit each
    m = re.search(r"int\s+tm_share_pick_batch\s*\((.*?)\)\s*;", txt, flags=re.S)
    params = [p.strip() for p in m.group(1).split(",")]
    sig = {name: (res, args) for name, res, args in L.SIGNATURES}["tm_share_pick_batch"]
    assert sig[0] is ctypes.c_int and len(sig[1]) == len(params) == 12
    for p, a in zip(params, sig[1]):
        if "*" in p:
            assert a is ctypes.c_void_p, p
        else:
            assert p.startswith("uint32_t") and a is ctypes.c_uint32, p
    assert hasattr(L.load(), "tm_share_pick_batch")
    assert "`sticky` stays with the caller" not in open(os.path.join(ROOT, "include", "topicmatch.h")).read()


def test_engine_wrapper_shapes():
    e = Engine(device=-1)
    with pytest.raises(ValueError):
        e.share_pick_batch(Engine.SHARE_KEYED, np.zeros(1, np.uint8), [0, 1], np.zeros(1, np.uint8), [0, 1], [1, 2],
                           [], [0, 0])
    with pytest.raises(ValueError):
        e.share_pick_batch(Engine.SHARE_KEYED, np.zeros(1, np.uint8), [0, 1], np.zeros(1, np.uint8), [0, 1], [1],
                           [], [0, 0, 0])
    e.close()
