"""The stream-ordered publish call and the cursor contexts on a host-only
engine: the codes of tm_share_cursors_open and tm_publish_stream_device
without a device, every argument check of the call (they come before the
device check, so they are visible here), and the workspace size as a function
of the batch and the capacities."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from emqx_amd import Engine  # noqa: E402
from emqx_amd import _lib as L  # noqa: E402

P = 0x1000   # a non-null "device pointer": no argument check dereferences one


@pytest.fixture()
def eng():
    e = Engine(device=-1)
    yield e
    e.close()


def _caps(ids=64, routes=64, pairs=64, rr=64):
    return L.TmPublishCaps(ids, routes, pairs, rr)


def _call(e, **kw):
    a = dict(bytes=P, off=P, n=4, nbytes=16, strategy=Engine.SHARE_ROUND_ROBIN, keys=None, cursors=None,
             caps=_caps(), ws=P, ws_bytes=None, hdr=P, doff=P, soff=P, deliv=P, pairs=P)
    a.update(kw)
    caps = a["caps"]
    if a["ws_bytes"] is None:
        a["ws_bytes"] = e.lib.tm_publish_stream_workspace_bytes(e.h, a["n"], a["nbytes"], ctypes.byref(_caps())) \
            if caps is None else e.lib.tm_publish_stream_workspace_bytes(e.h, a["n"], a["nbytes"], ctypes.byref(caps))
    return e.lib.tm_publish_stream_device(e.h, a["bytes"], a["off"], a["n"], a["nbytes"], a["strategy"], a["keys"],
                                          a["cursors"], None if caps is None else ctypes.byref(caps), a["ws"],
                                          a["ws_bytes"], a["hdr"], a["doff"], a["soff"], a["deliv"], a["pairs"], None)


def test_cursor_context_needs_a_device(eng):
    h = ctypes.c_void_p()
    assert eng.lib.tm_share_cursors_open(eng.h, 0, ctypes.byref(h)) == L.TM_EDEVICE
    assert not h.value
    with pytest.raises(L.TopicMatchError):
        eng.share_cursors(0)
    eng.lib.tm_share_cursors_close(None)          # closing nothing is allowed


def test_cursor_context_null_arguments(eng):
    assert eng.lib.tm_share_cursors_open(eng.h, 0, None) == L.TM_EINVAL
    h = ctypes.c_void_p()
    assert eng.lib.tm_share_cursors_open(None, 0, ctypes.byref(h)) == L.TM_EINVAL


def test_publish_stream_needs_a_device(eng):
    assert _call(eng) == L.TM_EDEVICE
    assert _call(eng, strategy=Engine.SHARE_KEYED, keys=P) == L.TM_EDEVICE
    assert _call(eng, n=0) == L.TM_EDEVICE


@pytest.mark.parametrize("kw", [
    dict(off=None), dict(hdr=None), dict(doff=None), dict(soff=None),                # null outputs / offsets
    dict(caps=None), dict(ws=None),
    dict(strategy=Engine.SHARE_KEYED, keys=None),                                     # keyed without keys
    dict(deliv=None), dict(pairs=None),                                               # a capacity with a null plane
    dict(strategy=0), dict(strategy=3),                                               # neither strategy
    dict(ws_bytes=0),
], ids=lambda kw: ",".join("%s=%s" % kv for kv in kw.items()))
def test_publish_stream_argument_checks(eng, kw):
    assert _call(eng, **kw) == L.TM_EINVAL


def test_publish_stream_null_planes_without_capacity_pass_the_checks(eng):
    assert _call(eng, caps=_caps(routes=0), deliv=None) == L.TM_EDEVICE
    assert _call(eng, caps=_caps(pairs=0), pairs=None) == L.TM_EDEVICE


def test_publish_stream_workspace_one_byte_short(eng):
    caps = _caps(1000, 2000, 3000, 500)
    need = eng.lib.tm_publish_stream_workspace_bytes(eng.h, 100, 4096, ctypes.byref(caps))
    assert _call(eng, n=100, nbytes=4096, caps=caps, ws_bytes=need - 1) == L.TM_EINVAL
    assert _call(eng, n=100, nbytes=4096, caps=caps, ws_bytes=need) == L.TM_EDEVICE


def test_publish_stream_capacity_out_of_range(eng):
    assert eng.publish_stream_workspace_bytes(4, 16, (64, 2 ** 32, 64, 64)) == 0
    assert eng.lib.tm_publish_stream_workspace_bytes(eng.h, 4, 16, None) == 0
    assert _call(eng, caps=_caps(routes=2 ** 32), ws_bytes=1 << 40) == L.TM_ERANGE


def test_workspace_bytes_grow_with_the_batch_and_every_capacity(eng):
    def need(n, caps):
        return eng.publish_stream_workspace_bytes(n, 64 * n, caps)

    base = (100, 200, 300, 50)
    assert need(0, (0, 0, 0, 0)) > 0 and need(1, base) > 0
    prev = 0
    for n in (0, 1, 63, 64, 65, 256, 257, 600, 5000, 100_000, 2_000_000):
        b = need(n, base)
        assert b >= prev
        prev = b
    assert need(2_000_000, base) > need(1, base)
    for k in range(4):
        prev = 0
        for v in (0, 1, 255, 256, 257, 4095, 4096, 4097, 100_000, 5_000_000, 2 ** 32 - 3):
            caps = list(base)
            caps[k] = v
            b = need(600, caps)
            assert b >= prev, (k, v)
            prev = b
        lo, hi = list(base), list(base)
        hi[k] = 5_000_000
        assert need(600, hi) > need(600, lo), k


# ---- the batcher's new flags and the appended counter ---------------------------------------------------------

@pytest.mark.parametrize("flags", [L.TM_BATCHER_ROUND_ROBIN, L.TM_BATCHER_STREAM,
                                   L.TM_BATCHER_ROUND_ROBIN | L.TM_BATCHER_STREAM,
                                   L.TM_BATCHER_ROUND_ROBIN | L.TM_BATCHER_EAGER,
                                   L.TM_BATCHER_STREAM | L.TM_BATCHER_DELIVERIES])
def test_batcher_flags_need_publish_mode(eng, flags):
    cfg = L.TmBatcherConfig(100, 100, 0, flags, 1, 0)
    h = ctypes.c_void_p()
    assert eng.lib.tm_batcher_open(eng.h, ctypes.byref(cfg), ctypes.byref(h)) == L.TM_EINVAL
    assert not h.value


@pytest.mark.parametrize("flags", [L.TM_BATCHER_ROUND_ROBIN, L.TM_BATCHER_STREAM])
def test_batcher_flags_open_with_publish_mode(eng, flags):
    """host-only: the batcher opens (no lane has a device or a cursor context) and every publish fails with TM_EDEVICE"""
    from emqx_amd.batcher import Batcher
    b = Batcher(eng, publish=True, flags=flags, lanes_per_replica=1)
    got = []
    b.submit_publish(b"a/b", 7, lambda status, d, p: got.append((status, d, p)))
    b.flush()
    assert got == [(L.TM_EDEVICE, None, None)]
    st = b.stats()
    assert st["reruns"] == 0 and st["failed_batches"] == 1
    b.close()


def test_batcher_get_stats_writes_the_v1_prefix_only(eng):
    from emqx_amd.batcher import Batcher
    assert ctypes.sizeof(L.TmBatcherStats) == 19 * 8 and L.TmBatcherStats.reruns.offset == 18 * 8
    b = Batcher(eng, publish=True, round_robin=True)
    s = L.TmBatcherStats()
    ctypes.memset(ctypes.byref(s), 0x5A, ctypes.sizeof(s))
    assert eng.lib.tm_batcher_get_stats(b.h, ctypes.byref(s)) == L.TM_OK
    raw = bytes(s)
    assert raw[:13 * 8] == b"\0" * (13 * 8)                       # the V1 prefix, all counters still zero
    assert raw[13 * 8:] == b"\x5a" * (6 * 8)                      # max_* and reruns untouched
    assert eng.lib.tm_batcher_get_stats2(b.h, ctypes.byref(s), ctypes.sizeof(s), 0) == L.TM_OK
    assert s.reruns == 0 and s.max_sync_ns == 0
    # a caller built against the header before `reruns` passes the shorter struct: nothing past it is written
    ctypes.memset(ctypes.byref(s), 0x5A, ctypes.sizeof(s))
    assert eng.lib.tm_batcher_get_stats2(b.h, ctypes.byref(s), 18 * 8, 0) == L.TM_OK
    assert bytes(s)[18 * 8:] == b"\x5a" * 8 and s.max_sync_ns == 0
    b.close()
