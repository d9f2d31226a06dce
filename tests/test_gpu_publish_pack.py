"""tm_publish_pack_device (pack.hip) on the GPU: the header, the dense offsets
and both record streams against a numpy compaction of what
tm_match_publish_batch_device(TM_SHARE_KEYED) itself left, and a sample of
topics against tests/dispatch_ref.py and tests/shared_ref.py directly; the
batch sizes cross the wave and block edges, one topic has more than 256
deliveries, one bag more than 1,024 pairs; each capacity one short in turn
leaves the header and offsets exact and writes nothing past the record
buffers."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from publish_util import GUARD, DevicePublish, World  # noqa: E402
from emqx_amd import Engine  # noqa: E402
from emqx_amd.engine import pack  # noqa: E402

pytestmark = pytest.mark.gpu

DEEP = [b"l%d" % i for i in range(9)]
DEEP_TOPIC = b"/".join(DEEP)


def _build(device):
    w = World(device)
    wild = [b"a/+", b"a/#", b"+/b", b"c/+/d", b"c/#", b"+/+", b"d/+", b"a/b/#", b"+/c/+", b"e/#", b"e/+", b"s/#"]
    exact = [b"t/%d" % i for i in range(20)] + [b"a/b", b"c/x/d", b"e/f", b"d"]
    for i, f in enumerate(wild + exact):
        w.route(f, ("n1", "n2", "n1")[i % 3])                    # local and other-node routes
        if i % 3 != 1 or i % 2 == 0:
            w.sub(f, 100 + i)
        if i % 4 == 0:
            w.sub(f, 200 + i)
            w.sub(f, 300 + i, b"g1")                             # a shared entry: counts, no pair
        if i % 2 == 0:
            g = ("g1", "g2")[i // 2 % 2]
            w.route(f, (g, "n1"))
            w.members(g.encode(), f, [1000 + 8 * i + k for k in range((1, 2, 7)[i // 2 % 3])])
    # {g, n1} and {g, n2} on one To: aggre/1 keeps one {To, g} and leaves a hole behind the list
    for f in (b"a/#", b"t/3", b"+/+"):
        w.route(f, ("g3", "n1"))
        w.route(f, ("g3", "n2"))
    w.members(b"g3", b"a/#", [71, 72, 73])
    w.route(b"q", ("g9", "n2"))                                  # a group without members: `false`
    w.route(b"rr/only/here", "n2")                               # remote only: no pair
    w.route(b"rr/+/+", "n3")
    # 2^9 filters of '+' and literals over a 9-level topic: 512 deliveries for DEEP_TOPIC
    for m in range(512):
        f = b"/".join(b"+" if m >> i & 1 else DEEP[i] for i in range(9))
        w.route(f, "n1" if m % 2 else "n2")
        if m % 64 == 1:
            w.sub(f, 5000 + m)
    w.route(b"big", "n1")                                        # one bag of more than 1,024 pairs
    w.subs(b"big", list(range(20000, 21100)))
    w.e.commit()
    w.pool = exact + [b"a/c", b"x/b", b"c/y/d", b"c/z", b"q", b"rr/only/here", b"rr/x/y", b"d/e", b"a/b/c", b"z/c/z",
                      b"e/g", b"nothing/at/all/here", b"s/1", b"t/3"]
    return w


@pytest.fixture(scope="module")
def world(gpu_device):
    w = _build(gpu_device)
    yield w
    w.close()


def _batch(w, n, extra=()):
    ts = list(extra) + [w.pool[(7 * i) % len(w.pool)] for i in range(n - len(extra))]
    return ts, [(i * 2654435761 + 17) % 2 ** 32 for i in range(len(ts))]


def _compaction(h, n):
    """numpy restatement: the kept slots of every topic in order, the pairs as they are"""
    c, o = h["c"].astype(np.int64), h["o"].astype(np.int64)
    doff = np.concatenate([[0], np.cumsum(c)]).astype(np.uint64)
    idx = np.concatenate([np.arange(o[t], o[t] + c[t]) for t in range(n)] + [np.zeros(0, np.int64)]).astype(np.int64)
    deliv = np.stack([h["to"][idx], h["tg"][idx], h["nd"][idx], h["pk"][idx]], axis=1) if len(idx) else \
        np.zeros((0, 4), np.uint32)
    P = h["stot"]
    pairs = np.stack([h["sto"][:P], h["sid"][:P]], axis=1)
    return doff, deliv, pairs


def _totals(w, ts, keys):
    """(route total, pair total) of the batch, from the host-buffer call"""
    buf, off = pack(ts)
    out = w.e.match_publish_batch(buf, off, Engine.SHARE_KEYED, keys)
    return len(out[2]), len(out[7])


def _run(w, dev, ts, keys, slack=3):
    """a fitting publish + pack, compared with the compaction; returns the publish and its host copy"""
    n = len(ts)
    tot, stot = _totals(w, ts, keys)
    cap, scap = tot + slack, stot + slack
    pub = DevicePublish(w.e, dev, ts, keys, cap, scap)
    h = pub.host()
    assert h["tot"] == tot and h["stot"] == stot
    doff, deliv, pairs = _compaction(h, n)
    D, P = int(doff[n]), h["stot"]
    assert D <= h["tot"]
    hdr, got_doff, got_deliv, got_pairs = pub.pack(D + slack - 2, P + 1)   # the record capacity as roomy as out_cap
    assert list(hdr) == [h["tot"], P, D, P]
    assert np.array_equal(got_doff, doff)
    assert np.array_equal(got_deliv[:D], deliv)
    assert np.array_equal(got_pairs[:P], pairs)
    assert (got_deliv[D:] == GUARD).all() and (got_pairs[P:] == GUARD).all()   # nothing past D / P either
    return pub, h, (doff, deliv, pairs)


def _check_refs(w, ts, keys, doff, soff, deliv, pairs, sample):
    for t in sample:
        d = [tuple(int(x) for x in r) for r in deliv[int(doff[t]):int(doff[t + 1])]]
        p = [tuple(int(x) for x in r) for r in pairs[int(soff[t]):int(soff[t + 1])]]
        assert w.got(ts[t], d, p) == w.want(ts[t], keys[t]), (t, ts[t])


def test_pack_empty_batch(world, gpu_device):
    pub = DevicePublish(world.e, gpu_device, [], [], 4, 4)
    hdr, doff, deliv, pairs = pub.pack(4, 4)
    assert list(hdr) == [0, 0, 0, 0] and list(doff) == [0]
    assert (deliv == GUARD).all() and (pairs == GUARD).all()


def test_pack_one_topic_without_delivery(world, gpu_device):
    pub, h, _ = _run(world, gpu_device, [b"nothing/at/all/here"], [5])
    assert h["tot"] == 0 and h["stot"] == 0


def test_pack_three_topics_middle_one_empty(world, gpu_device):
    ts, keys = [b"a/b", b"nothing/at/all/here", b"t/3"], [1, 2, 3]
    pub, h, (doff, deliv, pairs) = _run(world, gpu_device, ts, keys)
    assert doff[1] == doff[2] and doff[1] > 0 and doff[3] > doff[2]
    assert int(doff[3]) < h["tot"]                               # aggre/1 shortened a list: there was a hole to remove
    _check_refs(world, ts, keys, doff, h["so"], deliv, pairs, range(3))


@pytest.mark.parametrize("n", [64, 65, 256, 257])
def test_pack_across_wave_and_block_edges(world, gpu_device, n):
    ts, keys = _batch(world, n)
    pub, h, (doff, deliv, pairs) = _run(world, gpu_device, ts, keys)
    assert int(doff[n]) < h["tot"] and h["stot"] > 0
    picked = deliv[:, 3] != Engine.NO_MEMBER
    assert picked.any() and not picked.all()
    _check_refs(world, ts, keys, doff, h["so"], deliv, pairs, list(range(0, n, 9)) + [n - 1])


def test_pack_one_topic_with_more_than_256_deliveries(world, gpu_device):
    ts, keys = _batch(world, 70, extra=[b"a/b", DEEP_TOPIC, b"t/3"])
    pub, h, (doff, deliv, pairs) = _run(world, gpu_device, ts, keys)
    assert int(doff[2] - doff[1]) == 512
    _check_refs(world, ts, keys, doff, h["so"], deliv, pairs, [0, 1, 2, 3, 69])


@pytest.mark.parametrize("n,slack", [(70, 20000), (70, 200000), (257, 20000)])
def test_pack_several_thread_blocks_share_a_block_of_topics(world, gpu_device, n, slack):
    """the launch gives every 256 topics one thread block per 1,024 records the
    capacities allow (at most 64): roomy capacities make 21 and 64 blocks share
    the 512-delivery topic's block of topics, and 10 each of two blocks"""
    ts, keys = _batch(world, n, extra=[b"a/b", DEEP_TOPIC, b"t/3"])
    pub, h, (doff, deliv, pairs) = _run(world, gpu_device, ts, keys, slack=slack)
    assert int(doff[2] - doff[1]) == 512
    _check_refs(world, ts, keys, doff, h["so"], deliv, pairs, [1, n - 1])


def test_pack_one_bag_with_more_than_1024_pairs(world, gpu_device):
    ts, keys = _batch(world, 300, extra=[b"t/1", b"big"])
    pub, h, (doff, deliv, pairs) = _run(world, gpu_device, ts, keys)
    assert int(h["so"][2] - h["so"][1]) == 1100
    _check_refs(world, ts, keys, doff, h["so"], deliv, pairs, [0, 1, 2, 299])


def test_pack_batch_without_pairs(world, gpu_device):
    ts, keys = [b"rr/only/here", b"q", b"rr/x/y", b"nothing/at/all/here"] * 20, list(range(80))
    pub, h, (doff, deliv, pairs) = _run(world, gpu_device, ts, keys)
    assert h["stot"] == 0 and int(doff[80]) > 0
    _check_refs(world, ts, keys, doff, h["so"], deliv, pairs, range(4))


def test_pack_null_pick_plane_gives_no_member(world, gpu_device):
    ts, keys = _batch(world, 65)
    pub, h, (doff, deliv, pairs) = _run(world, gpu_device, ts, keys)
    D, P = int(doff[65]), h["stot"]
    hdr, got_doff, got_deliv, got_pairs = pub.pack(D, P, pick=False)
    assert list(hdr) == [h["tot"], P, D, P] and np.array_equal(got_doff, doff)
    assert np.array_equal(got_deliv[:D, :3], deliv[:, :3])
    assert (got_deliv[:D, 3] == Engine.NO_MEMBER).all() and (deliv[:, 3] != Engine.NO_MEMBER).any()
    assert np.array_equal(got_pairs[:P], pairs)


@pytest.mark.parametrize("short", ["out_cap", "sub_cap", "deliv_cap", "pair_cap"])
def test_pack_one_element_too_few(world, gpu_device, short):
    """the header and doff stay exact, and the guard words right after both
    record buffers are unchanged"""
    ts, keys = _batch(world, 257, extra=[b"big", DEEP_TOPIC])
    n = len(ts)
    tot, stot = _totals(world, ts, keys)
    fit = DevicePublish(world.e, gpu_device, ts, keys, tot, stot)
    doff, deliv, pairs = _compaction(fit.host(), n)
    D, P = int(doff[n]), stot
    assert D > 512 and P > 1100
    cap = tot - 1 if short == "out_cap" else tot
    scap = stot - 1 if short == "sub_cap" else stot
    pub = fit if (cap, scap) == (tot, stot) else DevicePublish(world.e, gpu_device, ts, keys, cap, scap)
    h = pub.host()
    dcap = D - 1 if short == "deliv_cap" else D
    pcap = P - 1 if short == "pair_cap" else P
    hdr, got_doff, got_deliv, got_pairs = pub.pack(dcap, pcap)
    # {*d_total, *d_sub_total, D, P}: with deliveries dropped the call's own pair total covers the kept ones
    assert list(hdr) == [tot, h["stot"], D, h["stot"]]
    if short != "out_cap":
        assert h["stot"] == stot
    assert np.array_equal(got_doff, doff)
    fits = hdr[0] <= cap and hdr[1] <= scap and hdr[2] <= dcap and hdr[3] <= pcap
    assert not fits
    assert (got_deliv[dcap:] == GUARD).all() and (got_pairs[pcap:] == GUARD).all()
    assert len(got_deliv) == dcap + 4 and len(got_pairs) == pcap + 4
