"""Micro-batcher publish mode on CPU (TM_BATCHER_PUBLISH, tm_batcher_submit_publish,
tm_publish_pack_device): a host-only engine cannot publish, so every submit
completes with TM_EDEVICE and no records; the two submit kinds do not mix; the
flag excludes the other result kinds at open; the pack refuses bad calls."""
import ctypes
import threading

import pytest

from emqx_amd import Engine, _lib
from emqx_amd.batcher import Batcher


def test_publish_submits_fail_loudly_without_gpu_exactly_once():
    e = Engine(device=-1)
    e.insert(b"a/+")
    b = Batcher(e, max_topics=100, deadline_us=300, publish=True)
    seen = {}
    lock = threading.Lock()

    def producer(k):
        for i in range(250):
            t = k * 1000 + i

            def cb(status, deliveries, pairs, t=t):
                with lock:
                    seen.setdefault(t, []).append((status, deliveries, pairs))
            b.submit_publish(b"a/%d" % t, t, cb)
    ts = [threading.Thread(target=producer, args=(k,)) for k in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    b.flush()
    assert len(seen) == 1000
    assert all(v == [(_lib.TM_EDEVICE, None, None)] for v in seen.values())
    st = b.stats()
    assert st["topics"] == 1000 and st["batches"] >= 1 and st["failed_batches"] == st["batches"]
    assert st["results"] == 0
    b.close()
    e.close()


def test_mismatched_submit_kinds_are_refused_and_queue_nothing():
    e = Engine(device=-1)
    fired = []
    pub = Batcher(e, max_topics=100, deadline_us=100, publish=True)
    plain = Batcher(e, max_topics=100, deadline_us=100)
    with pytest.raises(_lib.TopicMatchError) as ei:
        pub.submit(b"a/b", lambda *a: fired.append(a))
    assert ei.value.code == _lib.TM_EINVAL
    with pytest.raises(_lib.TopicMatchError) as ei:
        plain.submit_publish(b"a/b", 7, lambda *a: fired.append(a))
    assert ei.value.code == _lib.TM_EINVAL
    for b in (pub, plain):
        b.flush()
        st = b.stats()
        assert st["topics"] == 0 and st["batches"] == 0
        b.close()
    assert fired == []
    e.close()


@pytest.mark.parametrize("other", ["TM_BATCHER_ROUTES", "TM_BATCHER_DELIVERIES", "TM_BATCHER_CSR"])
def test_publish_flag_excludes_the_other_result_kinds(other):
    e = Engine(device=-1)
    with pytest.raises(_lib.TopicMatchError) as ei:
        Batcher(e, flags=_lib.TM_BATCHER_PUBLISH | getattr(_lib, other))
    assert ei.value.code == _lib.TM_EINVAL
    e.close()


def test_publish_with_eager_opens():
    e = Engine(device=-1)
    b = Batcher(e, flags=_lib.TM_BATCHER_PUBLISH | _lib.TM_BATCHER_EAGER)
    got = []
    b.submit_publish(b"x", 1, lambda *a: got.append(a))
    b.flush()
    assert got == [(_lib.TM_EDEVICE, None, None)]
    b.close()
    e.close()


def test_pack_refuses_bad_calls():
    """a null d_hdr, d_doff, d_off or d_total: TM_EINVAL, before anything else
    is looked at; complete arguments on a host-only engine: TM_EDEVICE.  The
    pointers are never dereferenced (nothing runs without a device)."""
    e = Engine(device=-1)
    word = (ctypes.c_uint64 * 8)()
    p = ctypes.addressof(word)
    names = ["d_counts", "d_offs", "d_to", "d_target", "d_ndisp", "d_pick", "d_total", "d_sub_off", "d_sub_to",
             "d_sub_id", "d_sub_total", "d_hdr", "d_doff", "d_deliv", "d_pairs"]

    def call(**null):
        a = {k: (None if k in null else p) for k in names}
        return e.lib.tm_publish_pack_device(e.h, 1, a["d_counts"], a["d_offs"], a["d_to"], a["d_target"], a["d_ndisp"],
                                            a["d_pick"], 1, a["d_total"], a["d_sub_off"], a["d_sub_to"], a["d_sub_id"],
                                            1, a["d_sub_total"], a["d_hdr"], a["d_doff"], a["d_deliv"], 1,
                                            a["d_pairs"], 1, None)
    for k in ("d_hdr", "d_doff", "d_offs", "d_total"):
        assert call(**{k: True}) == _lib.TM_EINVAL, k
    assert call() == _lib.TM_EDEVICE
    assert call(d_pick=True) == _lib.TM_EDEVICE          # a null pick plane is allowed
    with pytest.raises(_lib.TopicMatchError) as ei:
        e.publish_pack(1, p, p, p, p, p, None, 1, p, p, p, p, 1, p, p, p, p, 1, p, 1)
    assert ei.value.code == _lib.TM_EDEVICE
    e.close()
