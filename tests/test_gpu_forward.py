"""forward/3's sending half on the GPU (forward.hip): tm_forward_plan and
tm_forward_plan_device against the reference model (tests/forward_ref.py),
element for element, and a three-node round trip through the Broker."""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from dispatch_ref import SubscriberBag, dispatch  # noqa: E402
from forward_ref import ROUTE_TOPIC, expected_plan, forward_deliveries  # noqa: E402
from emqx_amd import Engine  # noqa: E402
from emqx_amd import _lib as L  # noqa: E402
from emqx_amd.emqx_broker import Broker  # noqa: E402
from emqx_amd.emqx_router import Router, _enc  # noqa: E402
from emqx_amd.engine import pack  # noqa: E402
from oracle import pytrie  # noqa: E402

pytestmark = pytest.mark.gpu

DESTS = ["n1", "n2", ("g1", "n1"), ("g1", "n2"), ("g2", "n2"), "n3", ("a", "n3"), "g1"]
GUARD = 8


def _pool(rng, k):
    words = [b"a", b"b", b"", b"+", b"#", b"$SYS", b"c", b"d"]
    pool = set()
    while len(pool) < k:
        ws = [rng.choice(words) for _ in range(rng.randint(1, 5))]
        if b"#" in ws[:-1]:
            continue
        pool.add(b"/".join(ws))
    return sorted(pool)


def _topics(rng, k):
    words = [b"a", b"b", b"", b"$SYS", b"c", b"d", b"x"]
    return [b"/".join(rng.choice(words) for _ in range(rng.randint(1, 6))) for _ in range(k)]


class Net:
    """an engine with its Router / Broker and the oracle's route table beside it"""

    def __init__(self, gpu_device, node="n1"):
        self.e = Engine(device=gpu_device)
        self.r = Router(self.e, node=node)
        self.b = Broker(self.e, self.r)
        self.o = pytrie.RouteTable()
        self.node = node.encode()
        self.fnames = {}

    def add(self, topic, dest):
        self.r.add_route(topic, dest)
        self.o.add_route(topic, dest)

    def rem(self, topic, dest):
        self.r.del_route(topic, dest)
        self.o.del_route(topic, dest)

    def fname(self, fid):
        if fid not in self.fnames:
            self.fnames[fid] = self.e.filter_bytes(fid)
        return self.fnames[fid]

    def node_id(self, name):
        # tm_dest_target of a declared dest returns its target id and changes nothing
        return self.e.dest_target(_enc(name.decode()), Engine.TARGET_NODE, name)

    def expected(self, topics, counts, offs, to, tg, out_cap=None):
        """the model's plan in engine ids: the k-th delivery of topic t is slot
        offs[t] + k of the planes, whose To and target must be the model's"""
        triples = []
        for nd, tob, t, k in forward_deliveries(self.o, self.node, topics):
            assert k < int(counts[t])
            slot = int(offs[t]) + k
            if out_cap is not None and slot >= out_cap:
                continue                      # a slot at or past the capacity contributes nothing
            tid = int(to[slot])
            assert (topics[t] if tid == ROUTE_TOPIC else self.fname(tid)) == tob
            assert int(tg[slot]) == self.node_id(nd)
            triples.append((int(tg[slot]), tid, t))
        return expected_plan(triples)


def _same(got, want):
    hdr, groups, pub = got
    assert [int(x) for x in hdr] == want[0]
    assert [tuple(g) for g in np.asarray(groups).reshape(-1, 4).tolist()] == want[1]
    assert [int(x) for x in pub] == want[2]


def _dev_planes(e, dev, topics, out_cap, strategy=None, keys=None):
    """tm_match_dispatch_batch_device (or the publish call, keyed) -> the planes as tensors"""
    import torch
    tb, to = pack(topics)
    n = len(topics)
    i32 = lambda k, v=0: torch.full((max(k, 1),), v, dtype=torch.int32, device=dev)   # noqa: E731
    i64 = lambda k: torch.full((k,), -1, dtype=torch.int64, device=dev)               # noqa: E731
    t = dict(c=i32(n), o=i64(n + 1), to=i32(out_cap), tg=i32(out_cap), nd=i32(out_cap), tot=i64(1), sc=i32(n),
             so=i64(n + 1), sto=i32(1 << 12), sid=i32(1 << 12), stot=i64(1), pick=i32(out_cap))
    d_b = torch.from_numpy(np.concatenate([tb, np.zeros(8, np.uint8)])).to(dev)
    d_o = torch.from_numpy(to.view(np.int64).copy()).to(dev)
    torch.cuda.synchronize()
    if strategy is None:
        e.match_dispatch_batch_device(d_b, d_o, n, int(to[-1]), t["c"], t["o"], t["to"], t["tg"], t["nd"], out_cap,
                                      t["tot"], t["sc"], t["so"], t["sto"], t["sid"], 1 << 12, t["stot"])
    else:
        d_k = torch.from_numpy(np.asarray(keys, dtype=np.uint32).view(np.int32).copy()).to(dev)
        e.match_publish_batch_device(d_b, d_o, n, int(to[-1]), t["c"], t["o"], t["to"], t["tg"], t["nd"], out_cap,
                                     t["tot"], t["sc"], t["so"], t["sto"], t["sid"], 1 << 12, t["stot"], strategy,
                                     d_k, t["pick"])
    torch.cuda.synchronize()
    return t


def _dev_plan(e, dev, n, t, out_cap, group_cap, pub_cap):
    """tm_forward_plan_device over the planes t -> (hdr, groups[:group_cap],
    pub[:pub_cap]); the guard words after each result array must be intact"""
    import torch
    hdr = torch.full((4 + GUARD,), -7, dtype=torch.int64, device=dev)
    groups = torch.full(((group_cap + GUARD) * 4,), -7, dtype=torch.int32, device=dev)
    pub = torch.full((pub_cap + GUARD,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    e.forward_plan_device(n, t["c"], t["o"], t["to"], t["tg"], out_cap, t["tot"], hdr, groups, group_cap, pub,
                          pub_cap)
    torch.cuda.synchronize()
    hdr, groups, pub = hdr.cpu().numpy(), groups.cpu().numpy(), pub.cpu().numpy()
    assert list(hdr[4:]) == [-7] * GUARD
    assert list(groups[group_cap * 4:]) == [-7] * (GUARD * 4)
    assert list(pub[pub_cap:]) == [-7] * GUARD
    return hdr[:4], groups[:group_cap * 4].view(np.uint32).reshape(-1, 4), pub[:pub_cap].view(np.uint32)


def _both(net, dev, topics, slack=5):
    """the host form and the device form against the model; returns (want, counts, offs)"""
    tb, to = pack(topics)
    counts, offs, to_, tg = net.e.match_dispatch_batch(tb, to)[:4]
    want = net.expected(topics, counts, offs, to_, tg)
    _same(net.e.forward_plan(counts, offs, to_, tg), want)
    M, G = want[0][0], want[0][1]
    cap = len(to_) + slack                    # capacity above the route total: the flags past it are zero
    t = _dev_planes(net.e, dev, topics, cap)
    assert int(t["tot"][0]) == len(to_)
    hdr, groups, pub = _dev_plan(net.e, dev, len(topics), t, cap, G + 3, M + 3)
    _same((hdr, groups[:G], pub[:M]), want)
    assert (groups[G:] == 0xFFFFFFF9).all() and (pub[M:] == 0xFFFFFFF9).all()      # -7: untouched
    return want, counts, offs


def test_forward_random_ops_vs_model(gpu_device):
    import torch
    dev = torch.device("cuda", gpu_device)
    rng = random.Random(177)
    seen_m = seen_multi = seen_topic = seen_holes = 0
    for rep in range(2):
        net = Net(gpu_device)
        if rep % 2:
            net.e.set_option("layout", 2)
        pool = _pool(rng, 60)
        for step in range(600):
            t, d = rng.choice(pool), rng.choice(DESTS)
            if rng.random() < 0.7:
                net.add(t, d)
            else:
                net.rem(t, d)
            if step % 150 == 149:
                topics = _topics(rng, 300) + pool
                want, counts, offs = _both(net, dev, topics)
                (M, G, _, _), groups, _ = want
                seen_m += M > 0
                seen_multi += G < M
                seen_topic += any(g[1] == ROUTE_TOPIC for g in groups)
                seen_holes += any(int(counts[i]) < int(offs[i + 1]) - int(offs[i]) for i in range(len(topics)))
        net.e.close()
    assert seen_m == 8 and seen_multi == 8 and seen_topic > 0 and seen_holes > 0


@pytest.mark.parametrize("k", [63, 64, 65, 257, 4097])
def test_forward_run_lengths_across_wave_block_and_tile(gpu_device, k):
    """one remote route on '#' published k times, a second remote node behind
    it: a run of k pairs ends, and the next starts, on either side of a wave
    (64), a block (256) and a sort tile (4096)"""
    import torch
    dev = torch.device("cuda", gpu_device)
    net = Net(gpu_device)
    net.add(b"#", "n2")
    net.add(b"+/x", "n3")
    want, _, _ = _both(net, dev, [b"a/x"] * k)
    n2, n3 = sorted([net.node_id(b"n2"), net.node_id(b"n3")])
    assert want[0] == [2 * k, 2, 2, 0] and [g[2:] for g in want[1]] == [(0, k), (k, k)]
    assert [g[0] for g in want[1]] == [n2, n3]
    net.e.close()


def test_forward_runs_spanning_sort_tiles(gpu_device):
    """300 topics x 20 remote filters: M > 4096, runs of up to 300 pairs that
    start in one 4096-pair tile and end in the next"""
    import torch
    dev = torch.device("cuda", gpu_device)
    net = Net(gpu_device)
    filters = [b"#", b"a/#", b"a/b/#", b"a/b/c/#"]
    for m in range(16):
        filters.append(b"/".join(b"+" if m >> i & 1 else w for i, w in enumerate([b"a", b"b", b"c", b"d"])))
    for i, f in enumerate(filters):
        net.add(f, ["n2", "n3", "n4"][i % 3])
    rng = random.Random(5)
    topics = [b"a/b/c/d" if rng.random() < 0.8 else b"a/b/c/x" for _ in range(300)]
    want, _, _ = _both(net, dev, topics)
    assert want[0][0] > 4096 and want[0][1] == 20 and want[0][2] == 3
    firsts = [g[2] for g in want[1]]
    assert any(a // 4096 != (a + g[3] - 1) // 4096 for a, g in zip(firsts, want[1]))
    net.e.close()


def test_forward_target_key_needs_a_second_digit(gpu_device):
    import torch
    dev = torch.device("cuda", gpu_device)
    net = Net(gpu_device)
    names = ["m%03d" % i for i in range(300)]
    random.Random(3).shuffle(names)
    for nm in names:
        net.add(b"#", nm)
    net.add(b"a", "m007")
    want, _, _ = _both(net, dev, [b"a", b"b", b"a"])
    assert want[0] == [902, 301, 300, 0]
    nodes = [g[0] for g in want[1]]
    assert nodes == sorted(nodes) and max(nodes) >= 256 and min(nodes) < 256
    net.e.close()


def test_forward_to_key_needs_a_third_digit(gpu_device):
    """70,000 filters; remote routes on filters with ids below 256, between 256
    and 65,535 and from 65,536 on, and on the publish topic itself, which
    sorts after all of them"""
    import torch
    dev = torch.device("cuda", gpu_device)
    net = Net(gpu_device)
    net.add(b"k/+/0", "n2")

    def fill(a, b):
        net.e.insert_many(*pack([b"f/%d/+" % i for i in range(a, b)]))
    fill(0, 1000)
    net.add(b"k/+/+", "n2")
    fill(1000, 70000)
    net.add(b"k/#", "n2")
    net.add(b"k/x/0", "n2")
    net.add(b"+/x/0", "n3")
    assert net.e.filter_count >= 70000
    topics = [b"k/x/0", b"k/y/0", b"k/x/0", b"f/5/q"]
    want, _, _ = _both(net, dev, topics)
    n2 = net.node_id(b"n2")
    tos = [g[1] for g in want[1] if g[0] == n2]
    assert len(tos) == 4 and tos == sorted(tos) and tos[3] == ROUTE_TOPIC
    assert tos[0] < 256 <= tos[1] < 65536 <= tos[2] < ROUTE_TOPIC
    assert [g[2:] for g in want[1] if g[0] == n2] == [(0, 3), (3, 3), (6, 3), (9, 2)]
    net.e.close()


def test_forward_exclusions(gpu_device):
    import torch
    dev = torch.device("cuda", gpu_device)
    topics = [b"a/b", b"x", b"a/c"]
    # only the local node, only a group, only duplicate routes that leave holes: nothing to forward
    for routes in ([(b"#", "n1"), (b"a/+", "n1")], [(b"#", ("g1", "n2")), (b"a/b", ("g2", "n3"))],
                   [(b"a/#", ("g", "n2")), (b"a/#", ("g", "n1")), (b"a/+", ("g", "n3")), (b"a/+", ("g", "n1"))]):
        net = Net(gpu_device)
        for t, d in routes:
            net.add(t, d)
        want, counts, offs = _both(net, dev, topics)
        assert want == ([0, 0, 0, 0], [], [])
        if routes[0][0] == b"a/#":
            assert int(counts[0]) < int(offs[1]) - int(offs[0])          # the hole
        # n == 0, host and device form
        z = np.zeros(0, dtype=np.uint32)
        _same(net.e.forward_plan(z, np.zeros(1, dtype=np.uint64), z, z), ([0, 0, 0, 0], [], []))
        t = _dev_planes(net.e, dev, [], 4)
        hdr, _, _ = _dev_plan(net.e, dev, 0, t, 4, 2, 2)
        assert list(hdr) == [0, 0, 0, 0]
        net.e.close()
    # a dest declared as a group is one, whatever its bytes look like
    net = Net(gpu_device)
    net.add(b"#", "n2")
    net.e.dest_target(b"raw-n9", Engine.TARGET_GROUP, b"n9")
    net.e.route_add(b"#", b"raw-n9")
    tb, to = pack(topics)
    counts, offs, to_, tg = net.e.match_dispatch_batch(tb, to)[:4]
    kinds = {net.e.target_bytes(int(x)) for x in tg}
    assert kinds == {(0, b"n2"), (1, b"n9")}
    hdr, groups, pub = net.e.forward_plan(counts, offs, to_, tg)
    assert list(hdr) == [3, 1, 1, 0] and groups.tolist() == [[net.node_id(b"n2"), int(to_[0]), 0, 3]]
    assert pub.tolist() == [0, 1, 2]
    net.e.close()


def test_forward_follows_the_local_node(gpu_device):
    import torch
    dev = torch.device("cuda", gpu_device)
    net = Net(gpu_device)
    for t, d in [(b"#", "n1"), (b"a/+", "n2"), (b"a/b", "n3"), (b"+/b", ("g1", "n2"))]:
        net.add(t, d)
    topics = [b"a/b", b"x", b"a/c"]
    want, _, _ = _both(net, dev, topics)
    n1, n2 = net.node_id(b"n1"), net.node_id(b"n2")
    assert n1 not in {g[0] for g in want[1]} and n2 in {g[0] for g in want[1]}
    net.e.set_local_node(b"n2")               # published by the next batch's commit
    net.node = b"n2"
    want, _, _ = _both(net, dev, topics)
    assert n1 in {g[0] for g in want[1]} and n2 not in {g[0] for g in want[1]}
    assert want[0] == [4, 2, 2, 0]            # '#' -> n1 for all three topics, a/b -> n3
    net.e.close()


def test_forward_capacities(gpu_device):
    import torch
    dev = torch.device("cuda", gpu_device)
    net = Net(gpu_device)
    for t, d in [(b"#", "n2"), (b"a/+", "n3"), (b"a/b", "n2"), (b"+/b", "n1"), (b"a/#", ("g", "n2"))]:
        net.add(t, d)
    topics = [b"a/b", b"x", b"a/c", b"a/b", b"q/b", b"a/c"]
    n = len(topics)
    tb, to = pack(topics)
    counts, offs, to_, tg = net.e.match_dispatch_batch(tb, to)[:4]
    total = len(to_)
    full = net.expected(topics, counts, offs, to_, tg)
    (M, G, T, _), groups, pub = full
    assert M >= 8 and G >= 3 and T == 2
    # out_cap below the route total, in the middle of a topic's list
    cut = int(offs[3]) + 1
    assert cut < total
    want = net.expected(topics, counts, offs, to_, tg, out_cap=cut)
    assert 0 < want[0][0] < M
    _same(net.e.forward_plan(counts, offs, to_[:cut], tg[:cut], total=total, out_cap=cut), want)
    t = _dev_planes(net.e, dev, topics, cut)
    assert int(t["tot"][0]) == total
    hdr, g, p = _dev_plan(net.e, dev, n, t, cut, G, M)
    _same((hdr, g[:want[0][1]], p[:want[0][0]]), want)
    # short result arrays: TM_ENOSPC with an exact header from the host form
    for gc, pc in ((G - 1, M), (G, M - 1), (0, 0)):
        with pytest.raises(L.TopicMatchError) as ex:
            net.e.forward_plan(counts, offs, to_, tg, group_cap=gc, pub_cap=pc)
        assert ex.value.code == L.TM_ENOSPC and list(ex.value.hdr) == [M, G, T, 0]
    _same(net.e.forward_plan(counts, offs, to_, tg, group_cap=G, pub_cap=M), full)
    # the device form writes nothing at or past the capacities (_dev_plan's guards), its header is exact
    t = _dev_planes(net.e, dev, topics, total)
    for gc, pc in ((G - 1, M - 1), (1, 2), (0, 0)):
        hdr, g, p = _dev_plan(net.e, dev, n, t, total, gc, pc)
        assert list(hdr) == [M, G, T, 0]
        assert [tuple(x) for x in g.tolist()] == groups[:gc] and p.tolist() == pub[:pc]
    hdr, g, p = _dev_plan(net.e, dev, n, t, total, int(hdr[1]), int(hdr[0]))       # sized from the header
    _same((hdr, g, p), full)
    net.e.close()


def test_forward_plan_over_publish_planes(gpu_device):
    """the plan over tm_match_publish_batch_device's planes (keyed picks)
    equals the plan over the dispatch planes of the same batch"""
    import torch
    dev = torch.device("cuda", gpu_device)
    net = Net(gpu_device)
    rng = random.Random(11)
    pool = _pool(rng, 40)
    for _ in range(200):
        net.add(rng.choice(pool), rng.choice(DESTS))
    for i, f in enumerate(pool[:10]):
        net.b.subscribe(f, 100 + i, "g1")
        net.o.add_route(f, ("g1", "n1"))
    topics = _topics(rng, 120) + pool
    want, _, _ = _both(net, dev, topics)
    M, G = want[0][0], want[0][1]
    assert M > 0
    cap = 1 << 14
    t = _dev_planes(net.e, dev, topics, cap, Engine.SHARE_KEYED, [rng.randrange(1 << 32) for _ in topics])
    assert int(t["tot"][0]) <= cap
    _same(_dev_plan(net.e, dev, len(topics), t, cap, G, M), want)
    net.e.close()


def test_forward_three_node_round_trip(gpu_device):
    """three engines n1, n2, n3 with the same route table and a subscriber
    bag each: n1 publishes, every bundle goes to its node's
    dispatch_forwarded; together with n1's own pairs that is, per publish,
    dispatch(bag[Node], To) of every node delivery {To, Node}"""
    rng = random.Random(23)
    nodes = ["n1", "n2", "n3"]
    nets = {nm: Net(gpu_device, node=nm) for nm in nodes}
    bags = {nm.encode(): SubscriberBag() for nm in nodes}
    o = pytrie.RouteTable()
    pool = _pool(rng, 40)
    for i in range(260):
        nm, f = rng.choice(nodes), rng.choice(pool)
        g = rng.choice(["g1", "g2"]) if rng.random() < 0.2 else None
        nets[nm].b.subscribe(f, i, g)                       # the bag and the node's own route
        bags[nm.encode()].insert_subscriber(g, f, i)
        dest = nm if g is None else (g, nm)
        o.add_route(f, dest)
        for other in nodes:                                 # the replicated route table
            if other != nm:
                nets[other].r.add_route(f, dest)
    topics = _topics(rng, 160) + pool
    assert len(topics) == 200
    published, forwards = nets["n1"].b.publish_forward_many(topics)
    got = [(b"n1", t, to, s) for t, pub in enumerate(published) for to, s in pub.pairs]
    assert [nd for nd, _ in forwards] and {nd for nd, _ in forwards} <= {b"n2", b"n3"}
    for nd, groups in forwards:
        for to, pubs in groups:
            assert pubs == sorted(pubs)                     # batch order within a (node, To) pair
        for t, to, count, subs in nets[nd.decode()].b.dispatch_forwarded(groups, topics):
            assert count == dispatch(bags[nd], to)[0]
            got.extend((nd, t, to, s) for s in subs)
    want = []
    for t, tp in enumerate(topics):
        for to, x in o.match_deliveries(tp):
            if x[0] == 0:
                want.extend((x[1], t, to, s) for s in dispatch(bags[x[1]], to)[1])
    assert sorted(got) == sorted(want) and len({w[0] for w in want}) == 3
    assert any(to is None for _, groups in forwards for to, _ in groups)
    for net in nets.values():
        net.e.close()
