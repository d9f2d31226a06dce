"""tm_forward_plan_stream_device on the GPU (forward.hip): the forward plan
computed from the packed outputs of the stream-ordered publish call, against
the reference model (tests/forward_ref.py: expected_plan over the forward
deliveries the packed records define; over a real world also
forward_deliveries over oracle.pytrie), and in state 0 byte for byte against
tm_forward_plan_device fed the same data as planes.  Every output and the
workspace carry guard words, and every result array is filled before the call:
what a state must not write has to come back unchanged."""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from forward_ref import ROUTE_TOPIC, expected_plan, forward_deliveries  # noqa: E402
from pickword_world import NODE, STRATEGIES, build_world, deliver_of, publishes  # noqa: E402
from emqx_amd import Engine  # noqa: E402
from emqx_amd.emqx_router import _enc  # noqa: E402
from emqx_amd.engine import pack  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 8
FILL = 0xFFFFFFF9                 # -7: what the result arrays hold before a call
FILL64 = 0xFFFFFFFFFFFFFFF9
NO_MEMBER = 0xFFFFFFFF


class World:
    """an engine whose image holds `nodes` node targets (the local node n1
    first, ids 0 .. nodes - 1), then one $share group, and `filters` filter ids"""

    def __init__(self, device, nodes=4, filters=10, group=True, filter_names=None):
        self.e = Engine(device=device)
        self.e.set_local_node(b"n1")
        self.local = self.node(b"n1")
        self.remote = [self.node(b"r%03d" % i) for i in range(nodes - 1)]
        assert sorted([self.local] + self.remote) == list(range(nodes))
        self.group = self.e.dest_target(_enc(("g1", "n1")), Engine.TARGET_GROUP, b"g1") if group else None
        self.n_targets = nodes + (1 if group else 0)
        names = [b"f/%d/+" % i for i in range(filters)] if filter_names is None else filter_names
        if names[:-1]:
            self.e.insert_many(*pack(names[:-1]))
        # the last filter through a route: the image's filter count (the TM_ROUTE_TOPIC key) covers the ids
        # handed out when a route was last added
        self.e.route_add(names[-1], _enc("r000"))
        self.n_filters = len(names)
        assert self.e.filter_count == self.n_filters
        self.e.commit()

    def node(self, name):
        return self.e.dest_target(_enc(name.decode()), Engine.TARGET_NODE, name)

    def forwards(self):
        return set(self.remote)

    def close(self):
        self.e.close()


@pytest.fixture(scope="module")
def world(gpu_device):
    w = World(gpu_device)
    yield w
    w.close()


class Packed:
    """topics = [[(to, target)]] -> the packed outputs of a publish call as host arrays"""

    def __init__(self, topics, state=0):
        deliv, doff = [], [0]
        for recs in topics:
            for to, tg in recs:
                deliv.append((to, tg, 2, NO_MEMBER))
            doff.append(len(deliv))
        self.n = len(topics)
        self.doff = np.asarray(doff, dtype=np.uint64)
        self.deliv = np.asarray(deliv, dtype=np.uint32).reshape(-1, 4)
        self.hdr = np.asarray([len(deliv) + 3, 5, len(deliv), 5, 9, 0, state, 0], dtype=np.uint64)


def packed_forwards(K, deliv_cap, fwd):
    """the forward-delivery definition of tm_forward_plan_stream_device over host copies of the packed arrays"""
    hi = min(int(K.doff[K.n]), int(K.hdr[2]), deliv_cap)
    out = []
    for t in range(K.n):
        for d in range(int(K.doff[t]), int(K.doff[t + 1])):
            if int(K.doff[0]) <= d < hi and int(K.deliv[d][1]) in fwd:
                out.append((int(K.deliv[d][1]), int(K.deliv[d][0]), t))
    return out


class Dev:
    """the packed arrays on the device, cut (or padded with decoy rows) to deliv_cap"""

    def __init__(self, K, device, deliv_cap, decoy):
        import torch
        dev = torch.device("cuda", device)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(dev)   # noqa: E731
        rows = np.zeros((max(deliv_cap, 1), 4), dtype=np.uint32)
        rows[:] = (0, decoy, 2, NO_MEMBER)                   # a record past a bound: a forward, were it read
        k = min(deliv_cap, len(K.deliv))
        if k:
            rows[:k] = K.deliv[:k]
        self.rows = rows
        self.device, self.deliv_cap = device, deliv_cap
        self.hdr, self.doff = up(K.hdr, np.int64), up(K.doff, np.int64)
        self.deliv = up(rows.reshape(-1), np.int32)


def run_plan(e, d, n, group_cap, pub_cap, stream=None):
    """one call -> (hdr[8], group rows, pub), each cut where the header says the
    call wrote; everything else must hold its fill"""
    import torch
    dev = torch.device("cuda", d.device)
    ws_bytes = e.forward_plan_stream_workspace_bytes(n, d.deliv_cap, pub_cap)
    assert ws_bytes > 0 and ws_bytes % 256 == 0
    ws = torch.full((ws_bytes // 8 + GUARD,), -7, dtype=torch.int64, device=dev)
    hdr = torch.full((8 + GUARD,), -7, dtype=torch.int64, device=dev)
    groups = torch.full(((group_cap + GUARD) * 4,), -7, dtype=torch.int32, device=dev)
    pub = torch.full((pub_cap + GUARD,), -7, dtype=torch.int32, device=dev)
    if stream is None:
        torch.cuda.synchronize()
    else:
        torch.cuda.default_stream(dev).synchronize()         # the fills above only: nothing on `stream` is waited for
    e.forward_plan_stream_device(n, d.hdr, d.doff, d.deliv if d.deliv_cap else None, d.deliv_cap, ws, ws_bytes, hdr,
                                 groups if group_cap else None, group_cap, pub if pub_cap else None, pub_cap,
                                 stream=stream)
    torch.cuda.synchronize()
    hdr = hdr.cpu().numpy().view(np.uint64)
    groups = groups.cpu().numpy().view(np.uint32)
    pub = pub.cpu().numpy().view(np.uint32)
    assert (hdr[8:] == FILL64).all()
    assert (ws.cpu().numpy().view(np.uint64)[ws_bytes // 8:] == FILL64).all()
    h = [int(x) for x in hdr[:8]]
    state = h[6]
    assert state in (0, 1, 3, 4) and h[3] == h[4] == h[5] == h[7] == 0
    pn = min(h[0], pub_cap) if state in (0, 4) else 0
    gn = min(h[1], group_cap) if state in (0, 4) else 0
    assert (groups[gn * 4:] == FILL).all() and (pub[pn:] == FILL).all()
    return h, groups[:gn * 4].reshape(-1, 4), pub[:pn]


def _same(got, want):
    """a state 0 result against the model's plan"""
    h, groups, pub = got
    assert h == want[0] + [0, 0, 0, 0]
    assert [tuple(r) for r in groups.tolist()] == want[1]
    assert [int(x) for x in pub] == want[2]


def _read_back_form(e, K, d, group_cap, pub_cap):
    """tm_forward_plan_device over the same data as planes (a dense record is a
    slot without holes): count = the spans, out_cap = min(deliv_cap, D), total = D"""
    import torch
    dev = torch.device("cuda", d.device)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(dev)   # noqa: E731
    out_cap = min(d.deliv_cap, int(K.hdr[2]))
    counts = up(np.diff(K.doff.astype(np.int64)).astype(np.uint32), np.int32)
    to, tg = up(d.rows[:max(out_cap, 1), 0], np.int32), up(d.rows[:max(out_cap, 1), 1], np.int32)
    total = up(K.hdr[2:3], np.int64)
    hdr = torch.full((4,), -7, dtype=torch.int64, device=dev)
    groups = torch.full((max(group_cap, 1) * 4,), -7, dtype=torch.int32, device=dev)
    pub = torch.full((max(pub_cap, 1),), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    e.forward_plan_device(K.n, counts, d.doff, to, tg, out_cap, total, hdr, groups, group_cap, pub, pub_cap)
    torch.cuda.synchronize()
    return (hdr.cpu().numpy().view(np.uint64), groups.cpu().numpy().view(np.uint32),
            pub.cpu().numpy().view(np.uint32))


def check(w, device, K, deliv_cap=None, slack=(2, 3)):
    """state 0: the model, then tm_forward_plan_device byte for byte; at exact,
    roomy and deliv_cap-sized result capacities -> the model's plan"""
    deliv_cap = len(K.deliv) + 5 if deliv_cap is None else deliv_cap
    want = expected_plan(packed_forwards(K, deliv_cap, w.forwards()))
    M, G = want[0][0], want[0][1]
    d = Dev(K, device, deliv_cap, w.remote[0])
    for gc, pc in ((G, M), (G + slack[0], M + slack[1]), (deliv_cap, deliv_cap)):
        got = run_plan(w.e, d, K.n, gc, pc)
        assert got[0][6] == 0
        _same(got, want)
        if K.n and min(deliv_cap, int(K.hdr[2])) and len(K.deliv):
            hdr, groups, pub = _read_back_form(w.e, K, d, gc, pc)
            assert [int(x) for x in hdr] == got[0][:4]
            assert groups[:G * 4].tobytes() == got[1].tobytes() and pub[:M].tobytes() == got[2].tobytes()
    return want


# ---- synthetic packed records --------------------------------------------------------

def test_empty_batch(world, gpu_device):
    K = Packed([])
    for caps in ((0, 0, 0), (4, 3, 3)):
        got = run_plan(world.e, Dev(K, gpu_device, caps[0], world.remote[0]), 0, caps[1], caps[2])
        assert got[0] == [0] * 8 and len(got[1]) == 0 and len(got[2]) == 0


def test_batch_with_only_local_and_share_records(world, gpu_device):
    K = Packed([[(1, world.local), (2, world.group)], [], [(ROUTE_TOPIC, world.local)] * 70 + [(3, world.group)] * 2])
    assert check(world, gpu_device, K)[0] == [0, 0, 0, 0]
    got = run_plan(world.e, Dev(K, gpu_device, 0, world.remote[0]), K.n, 0, 0)   # no capacity at all
    assert got[0] == [0] * 8


@pytest.mark.parametrize("n", [257, 513])
def test_spans_across_topic_blocks(world, gpu_device, n):
    """0..3 records per topic, empty topics on both sides of every 256-topic block edge"""
    rng = random.Random(n)
    tgs = [world.local, world.group] + world.remote
    topics = [[(rng.choice([ROUTE_TOPIC] + list(range(world.n_filters))), rng.choice(tgs))
               for _ in range(rng.randint(0, 3))] for t in range(n)]
    for t in (0, 255, 256, 511, 512, n - 1):
        if t < n:
            topics[t] = []
    topics[254] = [(1, world.remote[0])] * 3
    topics[257 if n > 258 else 1] = [(1, world.remote[1])] * 3
    want = check(world, gpu_device, Packed(topics))
    assert want[0][0] > n // 2 and want[0][2] == 3 and any(g[1] == ROUTE_TOPIC for g in want[1])
    assert max(want[2]) > 256 or n == 257


def test_one_run_across_a_wave_a_block_and_a_sort_tile(world, gpu_device):
    """one (node, To) run of 4,097 publishes behind a 1-entry group"""
    a, b = sorted(world.remote[:2])
    topics = [[(3, a)]] + [[(7, world.local), (5, b)] for _ in range(4097)]
    want = check(world, gpu_device, Packed(topics))
    assert want[0] == [4098, 2, 2, 0] and want[1] == [(a, 3, 0, 1), (b, 5, 1, 4097)]
    assert want[2] == [0] + list(range(1, 4098))


@pytest.mark.parametrize("nodes", [2, 256, 257])
def test_target_sort_widths(gpu_device, nodes):
    """2, 256 and 257 node targets (257 needs a second target digit); with 256, a
    live target id 255 and pub_cap > M: every sorted digit ties with the padding's"""
    w = World(gpu_device, nodes=nodes, filters=10, group=False)
    rng = random.Random(nodes)
    top = nodes - 1
    assert top in w.forwards()
    topics = [[(rng.randrange(10), rng.choice([w.local, top, rng.randrange(nodes)])) for _ in range(rng.randint(0, 4))]
              for _ in range(90)]
    topics[5] = [(2, top), (1, top), (ROUTE_TOPIC, top)]
    K = Packed(topics)
    want = check(w, gpu_device, K, slack=(3, 9000))          # pub_cap far above M, through more than one sort tile
    assert want[1][-1][0] == top and want[1][-1][1] == ROUTE_TOPIC
    assert w.local not in {g[0] for g in want[1]}
    nodes_seen = [g[0] for g in want[1]]
    assert nodes_seen == sorted(nodes_seen)
    w.close()


@pytest.mark.parametrize("filters", [255, 256, 257])
def test_to_sort_widths(gpu_device, filters):
    """the TM_ROUTE_TOPIC key is the filter count: 255 is a key whose one sorted
    digit is all ones (a tie with the padding, pub_cap > M), 256 and 257 need a
    second digit; TM_ROUTE_TOPIC entries sort last within their node"""
    w = World(gpu_device, nodes=4, filters=filters)
    assert w.e.filter_count == filters
    rng = random.Random(filters)
    ids = [0, 1, filters - 2, filters - 1, ROUTE_TOPIC]
    topics = [[(rng.choice(ids), rng.choice(w.remote + [w.local])) for _ in range(rng.randint(0, 4))]
              for _ in range(120)]
    want = check(w, gpu_device, Packed(topics), slack=(3, 5000))
    for node in w.remote:
        tos = [g[1] for g in want[1] if g[0] == node]
        assert tos == sorted(tos) and tos[-1] == ROUTE_TOPIC and filters - 1 in tos
    w.close()


def test_to_key_needs_a_third_digit(gpu_device):
    """70,000 filters: To ids below 256, between 256 and 65,535, from 65,536 on, and
    the publish topic itself, which sorts after all of them"""
    w = World(gpu_device, nodes=3, filter_names=[b"f/%d/+" % i for i in range(70000)])
    assert w.e.filter_count >= 70000
    a, b = sorted(w.remote)
    tos = [ROUTE_TOPIC, 69999, 300, 7, 65536, 255, 256, 65535]
    topics = [[(to, b), (to, a)] for to in tos] + [[(to, a)] for to in tos]
    want = check(w, gpu_device, Packed(topics))
    assert [g[1] for g in want[1] if g[0] == a] == sorted(tos) and sorted(tos)[-1] == ROUTE_TOPIC
    assert [g[3] for g in want[1]] == [2] * 8 + [1] * 8
    w.close()


def test_exclusions(world, gpu_device):
    """the local node, the $share group, a target id at or past the table, decoy
    records at or past min(D, deliv_cap), d_doff[n] above D, D above deliv_cap"""
    r = world.remote
    past = [world.n_targets, world.n_targets + 1, 1 << 20, 0xFFFFFFFE, 0xFFFFFFFF]
    topics = [[(1, r[0]), (1, world.local), (1, world.group)], [(2, p) for p in past], [(2, r[1]), (ROUTE_TOPIC, r[0])]]
    topics += [[(3, r[t % 3]), (4, world.group)] for t in range(40)]
    K = Packed(topics)
    full = check(world, gpu_device, K)
    assert full[0] == [43, 6, 3, 0] and {g[0] for g in full[1]} == set(r)
    dlen = len(K.deliv)
    # D above deliv_cap: the array holds fewer records than the publish call counted
    cut = check(world, gpu_device, K, deliv_cap=dlen - 31)
    assert 0 < cut[0][0] < full[0][0]
    # d_doff[n] above D, D below deliv_cap: what lies at or past D is stale (Dev's decoy rows past the array too)
    K.deliv[dlen - 30:, 1] = r[2]
    K.deliv[dlen - 30:, 0] = 9
    K.hdr[2] = dlen - 30
    cut = check(world, gpu_device, K)
    assert 9 not in [g[1] for g in cut[1]] and 0 < cut[0][0] < full[0][0]
    # d_doff[n] below D: the records between them belong to no publish
    K = Packed(topics)
    K.hdr[2] = dlen + 4
    assert check(world, gpu_device, K, deliv_cap=dlen + 9) == full
    # d_doff[0] above 0: the records before it belong to no publish
    K = Packed(topics)
    K.doff = K.doff.copy()
    K.doff[0] = 2
    cut = check(world, gpu_device, K)
    assert cut[0][0] == full[0][0] - 1


def test_follows_the_local_node(gpu_device):
    w = World(gpu_device, nodes=4, filters=10)
    K = Packed([[(1, w.local), (1, w.remote[0]), (2, w.remote[1])] for _ in range(5)])
    want = check(w, gpu_device, K)
    assert {g[0] for g in want[1]} == {w.remote[0], w.remote[1]}
    w.e.set_local_node(b"r000")                              # published by the plan's own commit
    w.local, w.remote = w.remote[0], [w.local] + w.remote[1:]
    want = check(w, gpu_device, K)
    assert {g[0] for g in want[1]} == {w.remote[0], w.remote[1]} and w.local not in {g[0] for g in want[1]}
    assert want[0] == [10, 2, 2, 0]
    w.close()


# ---- the three states other than 0 -----------------------------------------------------

def _small(w):
    """M = 7 forward deliveries in G = 4 groups on 2 nodes"""
    a, b = sorted(w.remote[:2])
    K = Packed([[(1, a), (1, w.local), (2, b)], [(1, a), (ROUTE_TOPIC, a), (2, b), (3, w.group)], [(1, a), (1, b)]])
    return K, [(a, 1, 0, 3), (a, ROUTE_TOPIC, 3, 1), (b, 1, 4, 1), (b, 2, 5, 2)], [0, 1, 2, 1, 2, 0, 1]


def test_state_1_publish_call_did_not_fit(world, gpu_device):
    K, _g, _p = _small(world)
    K.hdr[6] = 2
    d = Dev(K, gpu_device, len(K.deliv), world.remote[0])
    got = run_plan(world.e, d, K.n, 8, 8)                    # run_plan: every result array still holds its fill
    assert got[0] == [0, 0, 0, 0, 0, 0, 1, 0]


def test_state_3_entries_do_not_fit(world, gpu_device):
    K, groups, pub = _small(world)
    d = Dev(K, gpu_device, len(K.deliv), world.remote[0])
    _same(run_plan(world.e, d, K.n, 4, 7), ([7, 4, 2, 0], groups, pub))
    for pub_cap in (6, 0):                                   # pub_cap = M - 1; none
        got = run_plan(world.e, d, K.n, 8, pub_cap)
        assert got[0] == [7, 0, 0, 0, 0, 0, 3, 0]            # nothing else written (run_plan)
    got = run_plan(world.e, d, K.n, 3, 6)                    # the first condition that applies wins
    assert got[0][6] == 3


def test_state_4_groups_do_not_fit(world, gpu_device):
    K, groups, pub = _small(world)
    d = Dev(K, gpu_device, len(K.deliv), world.remote[0])
    for group_cap in (3, 0):                                 # group_cap = G - 1; none
        h, g, p = run_plan(world.e, d, K.n, group_cap, 7)
        assert h == [7, 4, 2, 0, 0, 0, 4, 0]
        assert [tuple(r) for r in g.tolist()] == groups[:group_cap]   # exactly the first group_cap records
        assert [int(x) for x in p] == pub                    # pub is complete


# ---- behind a real publish call, on one stream, without a wait between them -----------

ROOMY = (20_000, 20_000, 20_000, 10_000)


class StreamPublish:
    """tm_publish_stream_opts_device into torch buffers, enqueued on `stream`"""

    def __init__(self, w, device, pubs, strategy, upgrade, stream):
        import torch
        dev = torch.device("cuda", device)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(dev)   # noqa: E731
        buf, off = pack([t for t, _k, _m in pubs])
        n = self.n = len(pubs)
        _ids, cr, cp, _rr = ROOMY
        self.device, self.deliv_cap = device, cr
        d_b = up(np.concatenate([buf, np.zeros(8, np.uint8)]), np.uint8)
        d_o = up(off, np.int64)
        d_k = up(np.asarray([k for _t, k, _m in pubs], dtype=np.uint32), np.int32)
        pf, fr, fl = deliver_of(pubs, upgrade)
        d_pf, d_fr = up(pf, np.int32), up(fr, np.int32)
        ws_bytes = w.e.publish_stream_opts_workspace_bytes(n, int(off[-1]), ROOMY)
        i32 = lambda k: torch.full((k,), -7, dtype=torch.int32, device=dev)   # noqa: E731
        i64 = lambda k: torch.full((k,), -7, dtype=torch.int64, device=dev)   # noqa: E731
        self.ws = torch.zeros(ws_bytes // 8 + 1, dtype=torch.int64, device=dev)
        self.hdr, self.doff, self.soff = i64(8), i64(n + 1), i64(n + 1)
        self.deliv, self.pairs, self.pickw, self.pairw = i32(cr * 4), i32(cp * 2), i32(cr), i32(cp)
        self.keep = (d_b, d_o, d_k, d_pf, d_fr)
        torch.cuda.default_stream(dev).synchronize()         # the uploads and fills above
        w.e.publish_stream_opts_device(d_b, d_o, n, int(off[-1]), STRATEGIES[strategy], d_k, None, ROOMY, self.ws,
                                       ws_bytes, self.hdr, self.doff, self.soff, self.deliv, self.pairs,
                                       (d_pf, d_fr, fl, self.pairw), self.pickw, stream=stream)

    def host(self):
        """the outputs as a Packed-like object for packed_forwards (after a synchronize)"""
        g = lambda t, dt: t.cpu().numpy().view(dt)   # noqa: E731
        K = Packed([])
        K.n, K.hdr, K.doff = self.n, g(self.hdr, np.uint64), g(self.doff, np.uint64)
        K.deliv = g(self.deliv, np.uint32).reshape(-1, 4)
        self.rows = K.deliv
        return K


@pytest.mark.parametrize("strategy", ["keyed", "round_robin", "sticky"])
def test_behind_the_publish_call_on_one_stream(gpu_device, strategy):
    import torch
    w = build_world(gpu_device)
    w.e.commit()
    base = publishes(w)
    pubs = [base[i % len(base)] for i in range(300)]
    topics = [t for t, _k, _m in pubs]
    ref = forward_deliveries(w.o, NODE, topics)
    assert {nd for nd, _to, _t, _k in ref} == {b"n2", b"n3"}
    st = torch.cuda.Stream(device=torch.device("cuda", gpu_device))
    d = StreamPublish(w, gpu_device, pubs, strategy, strategy == "round_robin", st)
    cap = d.deliv_cap
    got = run_plan(w.e, d, d.n, cap, cap, stream=st)         # enqueued behind the publish call: no wait between
    K = d.host()
    assert int(K.hdr[6]) == 0 and got[0][6] == 0
    fwd = {w.e.dest_target(_enc(nm), Engine.TARGET_NODE, nm.encode()) for nm in ("n2", "n3")}
    want = expected_plan(packed_forwards(K, cap, fwd))
    _same(got, want)
    M, G = want[0][0], want[0][1]
    hdr, groups, pub = _read_back_form(w.e, K, d, cap, cap)
    assert [int(x) for x in hdr] == got[0][:4]
    assert groups[:G * 4].tobytes() == got[1].tobytes() and pub[:M].tobytes() == got[2].tobytes()
    # the plan over names against the route oracle
    named = []
    for tg, to, first, count in got[1].tolist():
        kind, node = w.e.target_bytes(tg)
        assert kind == Engine.TARGET_NODE
        named += [(node, w.to_bytes(to, topics[p]), int(p)) for p in got[2][first:first + count]]
    assert sorted(named) == sorted((nd, tob, t) for nd, tob, t, _k in ref) and len(named) == M > 300
    # a second run over the same outputs gives the same plan
    again = run_plan(w.e, d, d.n, cap, cap, stream=st)
    assert again[0] == got[0] and again[1].tobytes() == got[1].tobytes() and again[2].tobytes() == got[2].tobytes()
    # a commit that adds a route to a new node (a new target, a new filter id) between the two calls: the same plan
    w.route(b"brand/new/+", "n9")
    w.e.commit()
    after = run_plan(w.e, d, d.n, cap, cap, stream=st)
    assert after[0] == got[0] and after[1].tobytes() == got[1].tobytes() and after[2].tobytes() == got[2].tobytes()
    w.close()
