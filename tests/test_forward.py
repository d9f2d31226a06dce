"""forward/3's plan without a GPU: the status codes of tm_forward_plan /
tm_forward_plan_device on a host-only engine, and the reference model
(tests/forward_ref.py) on hand-worked cases."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from forward_ref import ROUTE_TOPIC, bundles, expected_plan, forward_deliveries  # noqa: E402
from emqx_amd import Engine  # noqa: E402
from emqx_amd import _lib as L  # noqa: E402
from oracle import pytrie  # noqa: E402


def _planes():
    return dict(count=np.array([1], dtype=np.uint32), off=np.array([0, 1], dtype=np.uint64),
                to=np.array([ROUTE_TOPIC], dtype=np.uint32), tg=np.array([0], dtype=np.uint32),
                hdr=np.zeros(4, dtype=np.uint64), groups=np.zeros((4, 4), dtype=np.uint32),
                pub=np.zeros(4, dtype=np.uint32), total=np.array([1], dtype=np.uint64))


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _host(e, a, n=1, out_cap=1, group_cap=4, pub_cap=4, **nulls):
    g = lambda k: None if k in nulls else _p(a[k])   # noqa: E731
    return e.lib.tm_forward_plan(e.h, n, g("count"), g("off"), g("to"), g("tg"), out_cap, 1, g("hdr"), g("groups"),
                                 group_cap, g("pub"), pub_cap)


def _dev(e, a, n=1, out_cap=1, group_cap=4, pub_cap=4, **nulls):
    # host arrays stand in for device memory: a call that is refused reads none of them
    g = lambda k: None if k in nulls else _p(a[k])   # noqa: E731
    return e.lib.tm_forward_plan_device(e.h, n, g("count"), g("off"), g("to"), g("tg"), out_cap, g("total"), g("hdr"),
                                        g("groups"), group_cap, g("pub"), pub_cap, None)


def test_forward_plan_needs_the_local_node_then_a_device():
    e = Engine(device=-1)
    a = _planes()
    assert _host(e, a) == L.TM_EINVAL and _dev(e, a) == L.TM_EINVAL      # tm_set_local_node not called yet
    assert b"tm_set_local_node" in e.lib.tm_last_error(e.h)
    e.set_local_node(b"n1")
    assert _host(e, a) == L.TM_EDEVICE and _dev(e, a) == L.TM_EDEVICE    # host-only: no CPU fallback
    with pytest.raises(L.TopicMatchError) as ex:
        e.forward_plan(a["count"], a["off"], a["to"], a["tg"])
    assert ex.value.code == L.TM_EDEVICE
    with pytest.raises(L.TopicMatchError) as ex:
        e.forward_plan_device(1, a["count"].ctypes.data, a["off"].ctypes.data, a["to"].ctypes.data,
                              a["tg"].ctypes.data, 1, a["total"].ctypes.data, a["hdr"].ctypes.data,
                              a["groups"].ctypes.data, 4, a["pub"].ctypes.data, 4)
    assert ex.value.code == L.TM_EDEVICE
    assert list(a["hdr"]) == [0, 0, 0, 0]
    e.close()


def test_forward_plan_null_arguments():
    e = Engine(device=-1)
    e.set_local_node(b"n1")
    a = _planes()
    for call in (_host, _dev):
        assert call(e, a, hdr=1) == L.TM_EINVAL
        assert call(e, a, off=1) == L.TM_EINVAL
        assert call(e, a, count=1) == L.TM_EINVAL                       # n != 0
        assert call(e, a, n=0, count=1) == L.TM_EDEVICE                 # n == 0: count may be null
        assert call(e, a, to=1) == L.TM_EINVAL and call(e, a, tg=1) == L.TM_EINVAL
        assert call(e, a, out_cap=0, to=1, tg=1) == L.TM_EDEVICE        # no capacity: the planes may be null
        assert call(e, a, groups=1) == L.TM_EINVAL and call(e, a, pub=1) == L.TM_EINVAL
        assert call(e, a, group_cap=0, pub_cap=0, groups=1, pub=1) == L.TM_EDEVICE
    assert _dev(e, a, total=1) == L.TM_EINVAL
    assert e.lib.tm_forward_plan(None, 1, _p(a["count"]), _p(a["off"]), _p(a["to"]), _p(a["tg"]), 1, 1, _p(a["hdr"]),
                                 _p(a["groups"]), 4, _p(a["pub"]), 4) == L.TM_EINVAL
    e.close()


def _table(routes):
    o = pytrie.RouteTable()
    for t, d in routes:
        o.add_route(t, d)
    return o


def _triples(fd):
    return [x[:3] for x in fd]


def test_model_local_remote_and_group_delivery():
    o = _table([(b"a/b", "n1"), (b"a/+", "n2"), (b"#", ("g1", "n1"))])
    dels = o.match_deliveries(b"a/b")
    assert sorted(dels) == [(b"#", (1, b"g1")), (b"a/+", (0, b"n2")), (b"a/b", (0, b"n1"))]
    fd = forward_deliveries(o, b"n1", [b"a/b"])
    assert _triples(fd) == [(b"n2", b"a/+", 0)]                     # not the local node, not the group
    assert dels[fd[0][3]] == (b"a/+", (0, b"n2"))
    # seen from n2 the forward is the delivery to n1
    assert _triples(forward_deliveries(o, b"n2", [b"a/b"])) == [(b"n1", b"a/b", 0)]
    hdr, groups, pub = expected_plan([(5, 7, 0)])
    assert hdr == [1, 1, 1, 0] and groups == [(5, 7, 0, 1)] and pub == [0]


def test_model_same_to_from_two_publishes_and_the_topic_itself():
    o = _table([(b"a/+", "n2"), (b"a/b", "n3"), (b"#", "n3"), (b"a/+", "n1")])
    topics = [b"a/b", b"x", b"a/c", b"a/b"]
    fd = forward_deliveries(o, b"n1", topics)
    assert sorted(_triples(fd)) == [(b"n2", b"a/+", 0), (b"n2", b"a/+", 2), (b"n2", b"a/+", 3),
                                    (b"n3", b"#", 0), (b"n3", b"#", 1), (b"n3", b"#", 2), (b"n3", b"#", 3),
                                    (b"n3", b"a/b", 0), (b"n3", b"a/b", 3)]
    for nd, to, t, k in fd:
        assert o.match_deliveries(topics[t])[k] == (to, (0, nd))
    # ids as an engine could hand them out: n3 before n2, '#' a late filter id;
    # the To b"a/b" of the publishes of b"a/b" is the topic itself
    node_id = {b"n2": 9, b"n3": 4}
    to_id = {b"a/+": 2, b"#": 300}
    triples = [(node_id[nd], ROUTE_TOPIC if to == topics[t] else to_id[to], t) for nd, to, t, _ in fd]
    hdr, groups, pub = expected_plan(triples)
    assert hdr == [9, 3, 2, 0]
    assert groups == [(4, 300, 0, 4), (4, ROUTE_TOPIC, 4, 2), (9, 2, 6, 3)]    # ROUTE_TOPIC after every filter id
    assert pub == [0, 1, 2, 3, 0, 3, 0, 2, 3]                                   # batch order within a group
    names = {4: b"n3", 9: b"n2"}
    assert bundles(groups, pub, names.get, {2: b"a/+", 300: b"#"}.get) == [
        (b"n3", [(b"#", [0, 1, 2, 3]), (None, [0, 3])]),
        (b"n2", [(b"a/+", [0, 2, 3])])]


def test_model_empty_and_duplicates():
    assert expected_plan([]) == ([0, 0, 0, 0], [], [])
    # aggre/1 keeps a {To, Node} the literal topic and the trie both produced: two forwards of one publish
    hdr, groups, pub = expected_plan([(1, 3, 5), (1, 3, 5), (1, 3, 2)])
    assert hdr == [3, 1, 1, 0] and groups == [(1, 3, 0, 3)] and pub == [2, 5, 5]
