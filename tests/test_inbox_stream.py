"""The stream-ordered inbox plan and the batcher's inbox mode without a GPU:
the three entry points in the header, the library and the ctypes table; the
workspace function; every status code tm_inbox_plan_stream_device and the two
open calls give before they look for a device; and the callback order of an
inbox batcher on a host-only engine."""
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

NAMES = ("tm_inbox_plan_stream_workspace_bytes", "tm_inbox_plan_stream_device", "tm_batcher_open_inbox")
TOP = 2 ** 32 - 2


def test_symbols_in_header_library_and_signatures():
    with open(os.path.join(ROOT, "include", "topicmatch.h")) as f:
        hdr = f.read()
    sigs = {name for name, _res, _args in L.SIGNATURES}
    e = Engine(device=-1)
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in sigs, name
        assert hasattr(e.lib, name), name
    assert re.search(r"#define TM_INBOX_STREAM_HDR_WORDS 8\b", hdr)
    assert re.search(r"#define TM_BATCHER_INBOX\s+1024u", hdr) and L.TM_BATCHER_INBOX == 1024
    assert "tm_inbox_done_fn" in hdr and Engine.INBOX_STREAM_HDR_WORDS == 8
    # the contract states the equality with the read-back form and keeps the one deviation
    assert "what tm_inbox_plan_device writes for the equivalent planes" in hdr and "ONE DEVIATION" in hdr
    e.close()


def test_workspace_bytes_monotone_and_zero_out_of_range():
    e = Engine(device=-1)
    ws = e.inbox_plan_stream_workspace_bytes
    base = ws(100, 1000, 2000, 3000)
    assert base > 0 and base % 256 == 0
    assert ws(0, 0, 0, 0) > 0                                # the state words
    steps = (0, 1, 255, 256, 4095, 4096, 4097, 32768, 32769, 100000, 1 << 22)
    for k in range(4):
        last = 0
        for v in steps:
            a = [100, 1000, 2000, 3000]
            a[k] = v
            got = ws(*a)
            assert got >= last > -1 and got > 0, (k, v)
            last = got
    assert ws(100, 1 << 20, 1 << 20, 1 << 21) >= ws(100, 1 << 20, 1 << 20, 1 << 20) >= ws(100, 1000, 1 << 20, 1 << 20)
    # out of range: a capacity (or the two position capacities together) at or above 2^32 - 2, n at or above 2^31
    assert ws(1, TOP, 0, 0) == 0 and ws(1, 0, TOP, 0) == 0 and ws(1, 0, 0, TOP) == 0
    assert ws(1, 2 ** 40, 0, 0) == 0 and ws(2 ** 31, 1, 1, 1) == 0
    assert ws(1, TOP - 1, 1, 0) == 0 and ws(1, TOP // 2, TOP // 2, 0) == 0
    assert ws(2 ** 31 - 1, 1, 1, 1) > 0 and ws(1, TOP - 2, 1, 1) > 0
    e.close()


def _arrays():
    u32 = lambda k: np.zeros(k, dtype=np.uint32)   # noqa: E731
    u64 = lambda k: np.zeros(k, dtype=np.uint64)   # noqa: E731
    return dict(pub_hdr=u64(8), doff=u64(2), sub_off=u64(2), deliv=u32(16), pick_word=u32(4), pairs=u32(8),
                pair_word=u32(4), ws=np.zeros(1 << 16, dtype=np.uint8), hdr=np.full(8, 7, dtype=np.uint64),
                inbox=u32(32), ent_pub=u32(8), ent_to=u32(8), ent_word=u32(8))


def _call(e, a, n=1, deliv_cap=4, pair_cap=4, sub_bits=16, ws_bytes=None, inbox_cap=8, ent_cap=8, h=True, **nulls):
    # host arrays stand in for device memory: a call that is refused reads none of them
    g = lambda k: None if k in nulls else ctypes.c_void_p(a[k].ctypes.data)   # noqa: E731
    if ws_bytes is None:
        ws_bytes = len(a["ws"])
    return e.lib.tm_inbox_plan_stream_device(e.h if h else None, n, g("pub_hdr"), g("doff"), g("sub_off"), g("deliv"),
                                             g("pick_word"), deliv_cap, g("pairs"), g("pair_word"), pair_cap,
                                             sub_bits, g("ws"), ws_bytes, g("hdr"), g("inbox"), inbox_cap,
                                             g("ent_pub"), g("ent_to"), g("ent_word"), ent_cap, None)


def test_plan_stream_host_only_engine_is_edevice():
    e = Engine(device=-1)
    a = _arrays()
    assert _call(e, a) == L.TM_EDEVICE
    assert b"host-only" in e.lib.tm_last_error(e.h)
    assert _call(e, a, n=0) == L.TM_EDEVICE
    assert list(a["hdr"]) == [7] * 8                         # nothing written
    d = lambda k: a[k].ctypes.data   # noqa: E731
    try:
        e.inbox_plan_stream_device(1, d("pub_hdr"), d("doff"), d("sub_off"), d("deliv"), d("pick_word"), 4,
                                   d("pairs"), d("pair_word"), 4, 16, d("ws"), len(a["ws"]), d("hdr"), d("inbox"), 8,
                                   d("ent_pub"), d("ent_to"), d("ent_word"), 8)
        raise AssertionError("no error")
    except L.TopicMatchError as ex:
        assert ex.code == L.TM_EDEVICE
    e.close()


def test_plan_stream_einval():
    e = Engine(device=-1)
    a = _arrays()
    ok = L.TM_EDEVICE                                        # what a call that passes the checks returns here
    assert _call(e, a) == ok
    for k in ("pub_hdr", "doff", "sub_off", "hdr", "ws"):
        assert _call(e, a, **{k: 1}) == L.TM_EINVAL, k
    # a null record or result array with its capacity non-zero
    for k in ("deliv", "pairs", "inbox", "ent_pub", "ent_to"):
        assert _call(e, a, **{k: 1}) == L.TM_EINVAL, k
    assert _call(e, a, deliv=1, deliv_cap=0) == ok and _call(e, a, pairs=1, pair_cap=0) == ok
    assert _call(e, a, inbox=1, inbox_cap=0) == ok
    assert _call(e, a, ent_pub=1, ent_to=1, ent_word=1, ent_cap=0) == ok
    # the three word planes may be null
    assert _call(e, a, pick_word=1) == ok and _call(e, a, pair_word=1) == ok and _call(e, a, ent_word=1) == ok
    # sub_bits 0..32
    for bits in (0, 1, 8, 31, 32):
        assert _call(e, a, sub_bits=bits) == ok
    assert _call(e, a, sub_bits=33) == L.TM_EINVAL and _call(e, a, sub_bits=2 ** 32 - 1) == L.TM_EINVAL
    # the workspace
    need = e.inbox_plan_stream_workspace_bytes(1, 4, 4, 8)
    assert 0 < need <= len(a["ws"])
    assert _call(e, a, ws_bytes=need) == ok and _call(e, a, ws_bytes=need - 1) == L.TM_EINVAL
    assert _call(e, a, ws_bytes=0) == L.TM_EINVAL
    assert _call(e, a, h=False) == L.TM_EINVAL
    assert list(a["hdr"]) == [7] * 8
    e.close()


def test_plan_stream_erange():
    e = Engine(device=-1)
    a = _arrays()
    big = 2 ** 62
    assert _call(e, a, deliv_cap=TOP, ws_bytes=big) == L.TM_ERANGE
    assert b"inbox" in e.lib.tm_last_error(e.h)
    assert _call(e, a, pair_cap=TOP, ws_bytes=big) == L.TM_ERANGE
    assert _call(e, a, ent_cap=TOP, ws_bytes=big) == L.TM_ERANGE
    assert _call(e, a, inbox_cap=TOP, ws_bytes=big) == L.TM_ERANGE
    assert _call(e, a, pair_cap=2 ** 40, ws_bytes=big) == L.TM_ERANGE
    assert _call(e, a, n=2 ** 31, ws_bytes=big) == L.TM_ERANGE  # bit 31 of ent_pub is the kind
    assert _call(e, a, n=2 ** 31 - 1, ws_bytes=big) == L.TM_EDEVICE
    assert _call(e, a, ent_cap=TOP - 1, inbox_cap=TOP - 1, ws_bytes=big) == L.TM_EDEVICE
    e.close()


def _open(e, flags, inbox, fn=None):
    cfg = L.TmBatcherConfig(64, 200, 0, flags, 1, 0)
    h = ctypes.c_void_p()
    if inbox:
        rc = e.lib.tm_batcher_open_inbox(e.h, ctypes.byref(cfg), fn, None, ctypes.byref(h))
    else:
        rc = e.lib.tm_batcher_open(e.h, ctypes.byref(cfg), ctypes.byref(h))
    if rc == L.TM_OK:
        e.lib.tm_batcher_close(h)
    return rc


def test_batcher_open_flag_rules():
    e = Engine(device=-1)
    P, O, I = L.TM_BATCHER_PUBLISH, L.TM_BATCHER_OPTS, L.TM_BATCHER_INBOX
    fn = L.INBOX_DONE_FN(lambda *a: None)
    none = ctypes.cast(None, L.INBOX_DONE_FN)
    assert _open(e, P | O, False) == L.TM_OK
    assert _open(e, P | O | I, False) == L.TM_EINVAL         # the flag needs its own open call
    assert _open(e, I, False) == L.TM_EINVAL
    assert _open(e, P | O | I, True, fn) == L.TM_OK
    assert _open(e, P | O, True, fn) == L.TM_EINVAL          # without the flag
    assert _open(e, P | I, True, fn) == L.TM_EINVAL          # without OPTS
    assert _open(e, O | I, True, fn) == L.TM_EINVAL          # without PUBLISH
    assert _open(e, P | O | I, True, none) == L.TM_EINVAL    # a NULL fn
    h = ctypes.c_void_p()
    assert e.lib.tm_batcher_open_inbox(e.h, None, fn, None, ctypes.byref(h)) == L.TM_EINVAL
    for more in (L.TM_BATCHER_ROUND_ROBIN, L.TM_BATCHER_STICKY, L.TM_BATCHER_UPGRADE_QOS, L.TM_BATCHER_EAGER):
        assert _open(e, P | O | I | more, True, fn) == L.TM_OK
    assert _open(e, P | O | I | L.TM_BATCHER_ROUND_ROBIN | L.TM_BATCHER_STICKY, True, fn) == L.TM_EINVAL
    assert _open(e, P | O | I | L.TM_BATCHER_ROUTES, True, fn) == L.TM_EINVAL
    e.close()


def test_inbox_batcher_on_a_host_only_engine():
    """every batch: the inbox callback first, with TM_EDEVICE and no arrays,
    then the per-publish callbacks with TM_EDEVICE and no arrays"""
    e = Engine(device=-1)
    log, lock = [], threading.Lock()

    def on_inbox(status, tickets, hdr, inbox, ent_pub, ent_to, ent_word):
        with lock:
            log.append(("inbox", status, [int(t) for t in tickets], hdr, inbox, ent_pub, ent_to, ent_word))

    def on_pub(i):
        def cb(status, deliv, pick_words, pairs, pair_words):
            with lock:
                log.append(("pub", status, i, deliv, pick_words, pairs, pair_words))
        return cb

    b = Batcher(e, max_topics=4, deadline_us=100, publish=True, opts=True, lanes_per_replica=1, inbox=on_inbox)
    tickets = []
    for i in range(10):
        tickets.append(b.submit_publish_opts(b"a/%d" % i, i, 1, L.TM_NO_SUBSCRIBER, on_pub(i)))
        if i % 4 == 3:
            b.flush()
    b.flush()
    st = b.stats()
    b.close()
    assert st["topics"] == 10 and st["failed_batches"] == st["batches"] >= 3
    assert len(set(tickets)) == 10
    # one lane: a batch's inbox callback, then its one to four publishes, then the next batch's
    heads = [i for i, row in enumerate(log) if row[0] == "inbox"]
    assert heads[0] == 0 and len(heads) == st["batches"]
    for a, b in zip(heads, heads[1:] + [len(log)]):
        assert log[a][1] == L.TM_EDEVICE and log[a][2] == [] and all(x is None for x in log[a][3:])
        assert 1 <= b - a - 1 <= 4
    pubs = [row for row in log if row[0] == "pub"]
    assert [r[2] for r in pubs] == list(range(10))           # submission order, each exactly once
    assert all(r[1] == L.TM_EDEVICE and r[3:] == (None, None, None, None) for r in pubs)
    e.close()
