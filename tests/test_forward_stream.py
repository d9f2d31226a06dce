"""The stream-ordered forward plan and the batcher's forward mode without a GPU:
the three entry points in the header, the library and the ctypes table; the
workspace function; every status code tm_forward_plan_stream_device and the
three open calls give before they look for a device; and the callback order of
a forward batcher on a host-only engine."""
import ctypes
import os
import re
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from emqx_amd import Engine  # noqa: E402
from emqx_amd import _lib as L  # noqa: E402
from emqx_amd.batcher import Batcher  # noqa: E402

NAMES = ("tm_forward_plan_stream_workspace_bytes", "tm_forward_plan_stream_device", "tm_batcher_open_plans")
TOP = 2 ** 32 - 2
STEPS = (0, 1, 255, 256, 4095, 4096, 4097, 32768, 32769, 1 << 22)


def _engine(local=True):
    e = Engine(device=-1)
    if local:
        e.set_local_node(b"n1")
    return e


def test_symbols_in_header_library_and_signatures():
    with open(os.path.join(ROOT, "include", "topicmatch.h")) as f:
        hdr = f.read()
    sigs = {name for name, _res, _args in L.SIGNATURES}
    e = Engine(device=-1)
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in sigs, name
        assert hasattr(e.lib, name), name
    assert re.search(r"#define TM_FORWARD_STREAM_HDR_WORDS 8\b", hdr)
    assert re.search(r"#define TM_BATCHER_FORWARD\s+2048u", hdr) and L.TM_BATCHER_FORWARD == 2048
    assert "tm_forward_done_fn" in hdr and Engine.FORWARD_STREAM_HDR_WORDS == 8
    assert hasattr(L, "FORWARD_DONE_FN")
    # the contract states the equality with the read-back form, and what a commit between the calls does
    flat = re.sub(r"[\s*]+", " ", hdr)
    assert "bit for bit what tm_forward_plan_device writes for the equivalent planes" in flat
    assert "does NOT change the plan" in flat and "tm_set_local_node between the two calls DOES change it" in flat
    e.close()


def test_workspace_bytes_monotone_and_zero_out_of_range():
    e = Engine(device=-1)
    ws = e.forward_plan_stream_workspace_bytes
    base = ws(100, 1000, 2000)
    assert base > 0 and base % 256 == 0
    z = ws(0, 0, 0)
    assert z > 0 and z % 256 == 0                            # the state words
    for k in range(3):
        for rest in ((100, 1000, 2000), (0, 0, 0), (1 << 20, 1 << 22, 1 << 22)):
            last = 0
            for v in STEPS:
                a = list(rest)
                a[k] = v
                got = ws(*a)
                assert got >= last and got > 0 and got % 256 == 0, (k, v)
                last = got
    # out of range: a capacity at or above 2^32 - 2, n at or above 2^31
    assert ws(1, TOP, 0) == 0 and ws(1, 0, TOP) == 0 and ws(1, 2 ** 40, 0) == 0 and ws(1, 0, 2 ** 63) == 0
    assert ws(2 ** 31, 1, 1) == 0 and ws(2 ** 32 - 1, 1, 1) == 0
    assert ws(2 ** 31 - 1, 1, 1) > 0 and ws(1, TOP - 1, 1) > 0 and ws(1, 1, TOP - 1) > 0
    e.close()


def _arrays():
    u32 = lambda k: np.zeros(k, dtype=np.uint32)   # noqa: E731
    u64 = lambda k: np.zeros(k, dtype=np.uint64)   # noqa: E731
    return dict(pub_hdr=u64(8), doff=u64(2), deliv=u32(16), ws=np.zeros(1 << 16, dtype=np.uint8),
                hdr=np.full(8, 7, dtype=np.uint64), groups=u32(32), pub=u32(8))


def _call(e, a, n=1, deliv_cap=4, ws_bytes=None, group_cap=8, pub_cap=8, h=True, **nulls):
    # host arrays stand in for device memory: a call that is refused reads none of them
    g = lambda k: None if k in nulls else ctypes.c_void_p(a[k].ctypes.data)   # noqa: E731
    if ws_bytes is None:
        ws_bytes = len(a["ws"])
    return e.lib.tm_forward_plan_stream_device(e.h if h else None, n, g("pub_hdr"), g("doff"), g("deliv"), deliv_cap,
                                               g("ws"), ws_bytes, g("hdr"), g("groups"), group_cap, g("pub"),
                                               pub_cap, None)


def test_plan_stream_host_only_engine_is_edevice():
    e = _engine()
    a = _arrays()
    assert _call(e, a) == L.TM_EDEVICE
    assert b"host-only" in e.lib.tm_last_error(e.h)
    assert _call(e, a, n=0) == L.TM_EDEVICE
    assert list(a["hdr"]) == [7] * 8                         # nothing written
    d = lambda k: a[k].ctypes.data   # noqa: E731
    try:
        e.forward_plan_stream_device(1, d("pub_hdr"), d("doff"), d("deliv"), 4, d("ws"), len(a["ws"]), d("hdr"),
                                     d("groups"), 8, d("pub"), 8)
        raise AssertionError("no error")
    except L.TopicMatchError as ex:
        assert ex.code == L.TM_EDEVICE
    e.close()


def test_plan_stream_einval():
    e = _engine()
    a = _arrays()
    ok = L.TM_EDEVICE                                        # what a call that passes the checks returns here
    assert _call(e, a) == ok
    for k in ("pub_hdr", "doff", "hdr", "ws"):
        assert _call(e, a, **{k: 1}) == L.TM_EINVAL, k
    # a null record or result array with its capacity non-zero
    for k in ("deliv", "groups", "pub"):
        assert _call(e, a, **{k: 1}) == L.TM_EINVAL, k
    assert _call(e, a, deliv=1, deliv_cap=0) == ok and _call(e, a, groups=1, group_cap=0) == ok
    assert _call(e, a, pub=1, pub_cap=0) == ok
    # the workspace
    need = e.forward_plan_stream_workspace_bytes(1, 4, 8)
    assert 0 < need <= len(a["ws"])
    assert _call(e, a, ws_bytes=need) == ok and _call(e, a, ws_bytes=need - 1) == L.TM_EINVAL
    assert _call(e, a, ws_bytes=0) == L.TM_EINVAL
    assert _call(e, a, h=False) == L.TM_EINVAL               # a null engine
    assert list(a["hdr"]) == [7] * 8
    e.close()
    # tm_set_local_node not called yet
    e = _engine(local=False)
    assert _call(e, a) == L.TM_EINVAL and b"tm_set_local_node" in e.lib.tm_last_error(e.h)
    e.set_local_node(b"n1")
    assert _call(e, a) == ok
    assert list(a["hdr"]) == [7] * 8
    e.close()


def test_plan_stream_erange():
    e = _engine()
    a = _arrays()
    big = 2 ** 62
    assert _call(e, a, deliv_cap=TOP, ws_bytes=big) == L.TM_ERANGE
    assert b"forward" in e.lib.tm_last_error(e.h)
    assert _call(e, a, pub_cap=TOP, ws_bytes=big) == L.TM_ERANGE
    assert _call(e, a, group_cap=TOP, ws_bytes=big) == L.TM_ERANGE
    assert _call(e, a, deliv_cap=2 ** 40, ws_bytes=big) == L.TM_ERANGE
    assert _call(e, a, n=2 ** 31, ws_bytes=big) == L.TM_ERANGE
    assert _call(e, a, n=2 ** 31 - 1, ws_bytes=big) == L.TM_EDEVICE
    assert _call(e, a, pub_cap=TOP - 1, group_cap=TOP - 1, ws_bytes=big) == L.TM_EDEVICE
    # the order of tm_inbox_plan_stream_device: null arguments, then the ranges, then the workspace
    assert _call(e, a, deliv_cap=TOP, ws_bytes=0) == L.TM_ERANGE
    assert _call(e, a, deliv_cap=TOP, hdr=1) == L.TM_EINVAL
    assert list(a["hdr"]) == [7] * 8
    e.close()


IFN = L.INBOX_DONE_FN(lambda *a: None)
FFN = L.FORWARD_DONE_FN(lambda *a: None)
NO_IFN = ctypes.cast(None, L.INBOX_DONE_FN)
NO_FFN = ctypes.cast(None, L.FORWARD_DONE_FN)


def _open(e, flags, how, ifn=NO_IFN, ffn=NO_FFN, cfg=True):
    c = L.TmBatcherConfig(64, 200, 0, flags, 1, 0)
    ref = ctypes.byref(c) if cfg else None
    h = ctypes.c_void_p()
    if how == "plans":
        rc = e.lib.tm_batcher_open_plans(e.h, ref, ifn, ffn, None, ctypes.byref(h))
    elif how == "inbox":
        rc = e.lib.tm_batcher_open_inbox(e.h, ref, ifn, None, ctypes.byref(h))
    else:
        rc = e.lib.tm_batcher_open(e.h, ref, ctypes.byref(h))
    if rc == L.TM_OK:
        e.lib.tm_batcher_close(h)
    else:
        assert not h.value
    return rc


def test_batcher_open_flag_rules():
    e = _engine()
    P, O, I, F = L.TM_BATCHER_PUBLISH, L.TM_BATCHER_OPTS, L.TM_BATCHER_INBOX, L.TM_BATCHER_FORWARD
    # tm_batcher_open_plans: each callback exactly with its flag, at least one flag
    assert _open(e, P | F, "plans", ffn=FFN) == L.TM_OK
    assert _open(e, P | O | F, "plans", ffn=FFN) == L.TM_OK
    assert _open(e, P | O | I | F, "plans", IFN, FFN) == L.TM_OK
    assert _open(e, P | O | I, "plans", IFN) == L.TM_OK      # the inbox plan alone
    assert _open(e, P | F, "plans") == L.TM_EINVAL           # the flag without its callback
    assert _open(e, P, "plans", ffn=FFN) == L.TM_EINVAL      # the callback without its flag
    assert _open(e, P | F, "plans", IFN, FFN) == L.TM_EINVAL
    assert _open(e, P | O | I | F, "plans", IFN) == L.TM_EINVAL
    assert _open(e, P | O | I | F, "plans", ffn=FFN) == L.TM_EINVAL
    assert _open(e, P | O | I, "plans", IFN, FFN) == L.TM_EINVAL
    assert _open(e, P | O, "plans") == L.TM_EINVAL           # neither flag
    assert _open(e, F, "plans", ffn=FFN) == L.TM_EINVAL      # without PUBLISH
    assert _open(e, O | F, "plans", ffn=FFN) == L.TM_EINVAL
    assert _open(e, P | I | F, "plans", IFN, FFN) == L.TM_EINVAL   # INBOX needs OPTS as before
    assert _open(e, P | F, "plans", ffn=FFN, cfg=False) == L.TM_EINVAL
    for more in (L.TM_BATCHER_ROUND_ROBIN, L.TM_BATCHER_STICKY, L.TM_BATCHER_EAGER, L.TM_BATCHER_STREAM):
        assert _open(e, P | F | more, "plans", ffn=FFN) == L.TM_OK
        assert _open(e, P | O | I | F | more, "plans", IFN, FFN) == L.TM_OK
    assert _open(e, P | O | F | L.TM_BATCHER_UPGRADE_QOS, "plans", ffn=FFN) == L.TM_OK
    assert _open(e, P | F | L.TM_BATCHER_UPGRADE_QOS, "plans", ffn=FFN) == L.TM_EINVAL   # needs OPTS, as before
    assert _open(e, P | F | L.TM_BATCHER_ROUND_ROBIN | L.TM_BATCHER_STICKY, "plans", ffn=FFN) == L.TM_EINVAL
    assert _open(e, P | F | L.TM_BATCHER_ROUTES, "plans", ffn=FFN) == L.TM_EINVAL
    # the two older open calls refuse the flag and are otherwise what they were
    assert _open(e, P | F, "open") == L.TM_EINVAL and _open(e, P | O | F, "open") == L.TM_EINVAL
    assert _open(e, F, "open") == L.TM_EINVAL
    assert _open(e, P | O | I | F, "inbox", IFN) == L.TM_EINVAL
    assert _open(e, P, "open") == L.TM_OK and _open(e, P | O, "open") == L.TM_OK and _open(e, 0, "open") == L.TM_OK
    assert _open(e, P | O | I, "open") == L.TM_EINVAL
    assert _open(e, P | O | I, "inbox", IFN) == L.TM_OK and _open(e, P | O | I, "inbox") == L.TM_EINVAL
    assert _open(e, P | O, "inbox", IFN) == L.TM_EINVAL
    e.close()


def _host_only_order(opts, inbox):
    e = _engine()
    log, lock = [], threading.Lock()

    def on_inbox(status, tickets, hdr, rows, ent_pub, ent_to, ent_word):
        with lock:
            log.append(("inbox", status, [int(t) for t in tickets], hdr, rows, ent_pub, ent_to, ent_word))

    def on_forward(status, tickets, hdr, groups, pub):
        with lock:
            log.append(("forward", status, [int(t) for t in tickets], hdr, groups, pub))

    def on_pub(i):
        def cb(status, *rest):
            with lock:
                log.append(("pub", status, i) + rest)
        return cb

    b = Batcher(e, max_topics=4, deadline_us=100, publish=True, opts=opts, lanes_per_replica=1,
                inbox=on_inbox if inbox else None, forward=on_forward)
    tickets = []
    for i in range(10):
        if opts:
            tickets.append(b.submit_publish_opts(b"a/%d" % i, i, 1, L.TM_NO_SUBSCRIBER, on_pub(i)))
        else:
            tickets.append(b.submit_publish(b"a/%d" % i, i, on_pub(i)))
        if i % 4 == 3:
            b.flush()
    b.flush()
    st = b.stats()
    b.close()
    e.close()
    assert st["topics"] == 10 and st["failed_batches"] == st["batches"] >= 3
    assert len(set(tickets)) == 10
    # one lane: a batch's inbox callback (if any), its forward callback, its one to four publishes, then the next
    heads = [i for i, row in enumerate(log) if row[0] == "forward"]
    assert len(heads) == st["batches"] and heads[0] == (1 if inbox else 0)
    for a, z in zip(heads, heads[1:] + [len(log) + (1 if inbox else 0)]):
        assert log[a][1] == L.TM_EDEVICE and log[a][2] == [] and all(x is None for x in log[a][3:])
        if inbox:
            assert log[a - 1][0] == "inbox" and log[a - 1][1] == L.TM_EDEVICE and log[a - 1][2] == []
            assert all(x is None for x in log[a - 1][3:])
        body = log[a + 1:z - (1 if inbox else 0)]
        assert 1 <= len(body) <= 4 and all(r[0] == "pub" for r in body)
    assert len([r for r in log if r[0] == "inbox"]) == (st["batches"] if inbox else 0)
    pubs = [row for row in log if row[0] == "pub"]
    assert [r[2] for r in pubs] == list(range(10))           # submission order, each exactly once
    assert all(r[1] == L.TM_EDEVICE and all(x is None for x in r[3:]) for r in pubs)


def test_forward_batcher_on_a_host_only_engine():
    """PUBLISH|FORWARD: every batch the forward callback first, with TM_EDEVICE
    and no arrays, then the per-publish callbacks with TM_EDEVICE and no arrays"""
    _host_only_order(opts=False, inbox=False)


def test_inbox_and_forward_batcher_on_a_host_only_engine():
    """PUBLISH|OPTS|INBOX|FORWARD: inbox callback, forward callback, per-publish callbacks"""
    _host_only_order(opts=True, inbox=True)


def test_batcher_without_forward_opens_as_before():
    e = _engine()
    b = Batcher(e, max_topics=4, publish=True)
    assert b.forward is None and not hasattr(b, "_fdone") and not hasattr(b, "_idone")
    b.close()
    b = Batcher(e, max_topics=4, publish=True, opts=True, inbox=lambda *a: None)
    assert b.forward is None and not hasattr(b, "_fdone")
    b.close()
    e.close()
