"""The inbox plan on the GPU (inbox.hip): tm_inbox_plan and tm_inbox_plan_device
against the reference model (tests/inbox_ref.py), element for element.  Every
case runs the host form and the device form over the same planes.  The first
eleven cases build synthetic planes (the plan reads no engine state); the last
four run a real publish call over a world of plain and $share subscribers with
options (tests/pickword_world.py) after random table operations."""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from inbox_ref import (DROP, NO_MEMBER, NO_WORD, PICK, ROUTE_TOPIC, expected_plan, grouped, grouped_plan,  # noqa: E402
                       reference_sends, sends_of_planes)
from pickword_world import NODE, STRATEGIES, build_world, deliver_of, publishes  # noqa: E402
from subopts_corpus import rand_opts  # noqa: E402
from emqx_amd import Engine  # noqa: E402
from emqx_amd import _lib as L  # noqa: E402
from emqx_amd.engine import pack  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 8
FILL = 0xFFFFFFF9                 # -7: what the result arrays hold before a call
DECOY = 424242                    # a pick value in a hole or past a bound: never sent


@pytest.fixture(scope="module")
def eng(gpu_device):
    e = Engine(device=gpu_device)
    yield e
    e.close()


def _planes(topics):
    """topics = [(pairs, slots, hole)]: pairs = [(sub, to, word)], slots =
    [(pick, to, word)] (the topic's live slots), hole = dead slots after them,
    which hold a pick value and a word as a live slot would"""
    P = dict(sub_off=[0], sub_to=[], sub_id=[], sub_word=[], counts=[], offs=[0], to=[], pick=[], pick_word=[])
    for pairs, slots, hole in topics:
        for s, to, word in pairs:
            P["sub_id"].append(s)
            P["sub_to"].append(to)
            P["sub_word"].append(word)
        P["sub_off"].append(len(P["sub_id"]))
        for m, to, word in list(slots) + [(DECOY, 77, 1)] * hole:
            P["pick"].append(m)
            P["to"].append(to)
            P["pick_word"].append(word)
        P["counts"].append(len(slots))
        P["offs"].append(len(P["pick"]))
    for k in ("sub_off", "offs"):
        P[k] = np.asarray(P[k], dtype=np.uint64)
    for k in ("sub_to", "sub_id", "sub_word", "counts", "to", "pick", "pick_word"):
        P[k] = np.asarray(P[k], dtype=np.uint32)
    return P


def _same(got, want, words=True):
    hdr, inbox, ent_pub, ent_to, ent_word = got
    assert [int(x) for x in hdr] == want[0]
    assert [tuple(r) for r in np.asarray(inbox).reshape(-1, 4).tolist()] == want[1]
    assert [int(x) for x in ent_pub] == want[2]
    assert [int(x) for x in ent_to] == want[3]
    if words:
        assert [int(x) for x in ent_word] == want[4]
    else:
        assert ent_word is None


def _dev(x, device, n=None):
    """a u32 / u64 numpy array as an int32 / int64 tensor of at least one element"""
    import torch
    a = np.ascontiguousarray(x)
    if n is not None:
        a = a[:n]
    if len(a) == 0:
        a = np.zeros(1, dtype=a.dtype)
    return torch.from_numpy(a.view(np.int64 if a.dtype == np.uint64 else np.int32).copy()).to(
        torch.device("cuda", device))


def _device_plan(e, device, n, d, sub_cap, out_cap, inbox_cap, ent_cap, words, null_out=False):
    """tm_inbox_plan_device over the device planes d -> (hdr, inbox, ent_pub,
    ent_to, ent_word) cut at the capacities; the guard words after each result
    array, and everything from min(capacity, needed) on, must be untouched"""
    import torch
    dev = torch.device("cuda", device)
    hdr = torch.full((4 + GUARD,), -7, dtype=torch.int64, device=dev)
    inbox = torch.full(((inbox_cap + GUARD) * 4,), -7, dtype=torch.int32, device=dev)
    ent = [torch.full((ent_cap + GUARD,), -7, dtype=torch.int32, device=dev) for _ in range(3)]
    torch.cuda.synchronize()
    e.inbox_plan_device(n, d["sub_off"], d.get("sub_to"), d.get("sub_id"), d.get("sub_word"), sub_cap, d["sub_total"],
                        d.get("counts"), d.get("offs"), d.get("to"), d.get("pick"), d.get("pick_word"), out_cap,
                        d.get("total"), hdr, None if null_out else inbox, inbox_cap, None if null_out else ent[0],
                        None if null_out else ent[1], ent[2] if words and not null_out else None, ent_cap)
    torch.cuda.synchronize()
    hdr = hdr.cpu().numpy()
    inbox = inbox.cpu().numpy().view(np.uint32)
    ent = [x.cpu().numpy().view(np.uint32) for x in ent]
    assert list(hdr[4:]) == [-7] * GUARD
    E, S = int(hdr[0]), int(hdr[1])
    en, sn = min(E, ent_cap), min(S, inbox_cap)
    assert (inbox[sn * 4:] == FILL).all()
    assert (ent[0][en:] == FILL).all() and (ent[1][en:] == FILL).all()
    assert (ent[2][en if words else 0:] == FILL).all()
    return hdr[:4], inbox[:sn * 4].reshape(-1, 4), ent[0][:en], ent[1][:en], ent[2][:en] if words else None


def _upload(P, device, sub_word, pick, pick_word, sub_total, sub_cap, total, out_cap):
    d = dict(sub_off=_dev(P["sub_off"], device), sub_to=_dev(P["sub_to"], device, sub_cap),
             sub_id=_dev(P["sub_id"], device, sub_cap), sub_total=_dev(np.array([sub_total], dtype=np.uint64), device))
    if sub_word:
        d["sub_word"] = _dev(P["sub_word"], device, sub_cap)
    if pick:
        d.update(counts=_dev(P["counts"], device), offs=_dev(P["offs"], device), to=_dev(P["to"], device, out_cap),
                 pick=_dev(P["pick"], device, out_cap), total=_dev(np.array([total], dtype=np.uint64), device))
        if pick_word:
            d["pick_word"] = _dev(P["pick_word"], device, out_cap)
    return d


def _both(e, device, P, sub_word=True, pick=True, pick_word=True, sub_total=None, sub_cap=None, total=None,
          out_cap=None):
    """the host form and the device form over planes P against the model -> the model's plan"""
    plen, klen = len(P["sub_id"]), len(P["pick"])
    sub_total = plen if sub_total is None else sub_total
    sub_cap = plen if sub_cap is None else sub_cap
    total = klen if total is None else total
    out_cap = klen if out_cap is None else out_cap
    words = sub_word or (pick and pick_word)
    g = lambda k, on=True: P[k] if on else None   # noqa: E731
    want = expected_plan(sends_of_planes(P["sub_off"], P["sub_to"], P["sub_id"], g("sub_word", sub_word), P["counts"],
                                         P["offs"], P["to"], g("pick", pick), g("pick_word", pick and pick_word),
                                         sub_total, sub_cap, total, out_cap))
    got = e.inbox_plan(P["sub_off"], P["sub_to"][:sub_cap], P["sub_id"][:sub_cap],
                       P["sub_word"][:sub_cap] if sub_word else None, g("counts", pick), g("offs", pick),
                       P["to"][:out_cap] if pick else None, P["pick"][:out_cap] if pick else None,
                       P["pick_word"][:out_cap] if pick and pick_word else None, sub_total=sub_total, sub_cap=sub_cap,
                       total=total, out_cap=out_cap)
    _same(got, want, words)
    d = _upload(P, device, sub_word, pick, pick_word, sub_total, sub_cap, total, out_cap)
    E, S = want[0][0], want[0][1]
    got = _device_plan(e, device, len(P["sub_off"]) - 1, d, sub_cap, out_cap, S + 2, E + 3, words)
    _same(got, want, words)
    return want


# ---- synthetic planes ----------------------------------------------------------------

def test_empty_batch(eng, gpu_device):
    P = _planes([])
    assert _both(eng, gpu_device, P)[0] == [0, 0, 0, 0]
    assert _both(eng, gpu_device, P, pick=False)[0] == [0, 0, 0, 0]


def test_every_pair_dropped(eng, gpu_device):
    P = _planes([([(5, 1, DROP), (6, 1, DROP)], [], 0), ([], [], 0), ([(5, ROUTE_TOPIC, DROP)] * 70, [], 0)])
    assert _both(eng, gpu_device, P)[0] == [0, 0, 0, 0]              # the result arrays keep their fill
    assert _both(eng, gpu_device, P, pick=False)[0] == [0, 0, 0, 0]


def test_every_pick_no_member(eng, gpu_device):
    P = _planes([([], [(NO_MEMBER, 3, NO_WORD)] * 3, 2), ([], [], 1), ([], [(NO_MEMBER, 4, NO_WORD)] * 300, 0)])
    assert _both(eng, gpu_device, P)[0] == [0, 0, 0, 0]
    assert _both(eng, gpu_device, P, pick_word=False)[0] == [0, 0, 0, 0]


@pytest.mark.parametrize("k", [63, 64, 65, 257, 4097])
def test_one_run_across_wave_block_and_tile_edges(eng, gpu_device, k):
    """subscriber 500 receives k entries, one per publish, between two other
    subscribers' runs that put its run at an odd offset"""
    topics = [([(100, 9, 1)] * 3, [], 0)]
    topics += [([(500, t, 2), (900, 9, 3)], [(500, 1000 + t, 4)] if t % 7 == 0 else [], t % 2) for t in range(k)]
    want = _both(eng, gpu_device, _planes(topics))
    npick = len(range(0, k, 7))
    assert want[1][1] == (500, 3, k + npick, npick)
    pubs = [x & ~PICK for x in want[2][3:3 + k + npick]]
    assert pubs == sorted(pubs)


def test_one_subscriber_takes_the_whole_batch(eng, gpu_device):
    """more than 8,192 sends to one subscriber: the sort's tiles keep publish order"""
    rng = random.Random(3)
    topics = [([(42, rng.randrange(50), rng.randrange(4)) for _ in range(rng.randint(3, 8))],
               [(42, 60 + t % 5, 1)] * (t % 3 == 0), 0) for t in range(1600)]
    want = _both(eng, gpu_device, _planes(topics))
    E = want[0][0]
    assert 8192 < E < 20000 and want[0][1] == 1 and want[1] == [(42, 0, E, want[0][3])]
    pubs = [x & ~PICK for x in want[2]]
    assert pubs == sorted(pubs)


def test_every_subscriber_receives_one_send(eng, gpu_device):
    rng = random.Random(4)
    ids = rng.sample(range(1, 1 << 20), 5000)
    topics, at = [], 0
    while at < len(ids):
        c = rng.randint(0, 9)
        pairs = [(s, at, 1) for s in ids[at:at + c]]
        at += c
        slots = [(ids[at], 7, 2)] if at < len(ids) and rng.random() < 0.3 else []
        at += len(slots)
        topics.append((pairs, slots, 0))
    want = _both(eng, gpu_device, _planes(topics))
    assert want[0][0] == want[0][1] == 5000 and all(r[2] == 1 for r in want[1])


def test_ids_of_every_sort_width(eng, gpu_device):
    """largest id 200 / 60,000 / 2^20 + 3 / 0xFFFFFFFE: one to four radix passes; the last batch holds all four"""
    rng = random.Random(5)
    ranges = [(0, 200), (256, 60000), (65536, (1 << 20) + 3), (1 << 24, 0xFFFFFFFE)]
    for r in range(4):
        lo_hi = ranges[:r + 1] if r == 3 else [ranges[r]]
        topics = []
        for t in range(60):
            ids = [rng.randint(*rng.choice(lo_hi)) for _ in range(rng.randint(0, 12))]
            if t == 7:
                ids += [hi for _lo, hi in lo_hi] + [lo_hi[0][0]]
            topics.append(([(s, t % 9, t % 3) for s in ids[1:]], [(s, 3, NO_WORD) for s in ids[:1]], t % 2))
        want = _both(eng, gpu_device, _planes(topics))
        assert want[1][-1][0] == lo_hi[-1][1]


def test_plain_subscriber_and_picked_member_in_one_publish(eng, gpu_device):
    """subscriber 7 of publish 1: three pairs and two picks, among other
    subscribers' -- its pairs first in pair order, then its picks in slot order"""
    topics = [([(7, 1, 1), (8, 1, 1)], [(9, 2, 2)], 0),
              ([(7, 10, 1), (6, 11, 1), (7, 12, 2), (8, 13, 1), (7, 14, 3)],
               [(7, 20, 4), (NO_MEMBER, 21, NO_WORD), (6, 22, 1), (7, 23, 5)], 1),
              ([(7, ROUTE_TOPIC, 0)], [(7, 30, 6)], 0)]
    want = _both(eng, gpu_device, _planes(topics))
    rec = next(r for r in want[1] if r[0] == 7)
    assert rec[2:] == (8, 3)
    a = rec[1]
    assert want[2][a:a + 8] == [0, 1, 1, 1, 1 | PICK, 1 | PICK, 2, 2 | PICK]
    assert want[3][a:a + 8] == [1, 10, 12, 14, 20, 23, ROUTE_TOPIC, 30]
    assert want[4][a:a + 8] == [1, 1, 2, 3, 4, 5, 0, 6]


def test_holes_and_bounds(eng, gpu_device):
    rng = random.Random(6)
    topics = [([(rng.randrange(40), t, 1) for _ in range(rng.randint(0, 5))],
               [(rng.choice([NO_MEMBER, rng.randrange(40)]), t, 2) for _ in range(rng.randint(0, 4))],
               rng.randint(0, 3)) for t in range(300)]
    P = _planes(topics)
    assert int(P["offs"][-1]) > int(P["counts"].sum())               # the spans have holes, each with a DECOY pick
    want = _both(eng, gpu_device, P)
    assert DECOY not in [r[0] for r in want[1]]
    plen, klen = len(P["sub_id"]), len(P["pick"])
    # the planes hold fewer positions than the totals: the call was short of capacity
    cut = _both(eng, gpu_device, P, sub_total=plen, sub_cap=plen - 57, total=klen, out_cap=klen - 41)
    assert 0 < cut[0][2] < want[0][2] and 0 < cut[0][3] < want[0][3]
    # the totals below the capacities: what lies past them is stale
    for k in ("sub_id", "pick"):
        P[k] = P[k].copy()
    P["sub_id"][plen - 30:] = DECOY
    P["pick"][klen - 30:] = DECOY
    cut = _both(eng, gpu_device, P, sub_total=plen - 30, total=klen - 30)
    assert DECOY not in [r[0] for r in cut[1]]


def test_word_planes(eng, gpu_device):
    topics = [([(3, 1, DROP), (4, 1, 5)], [(3, 2, DROP), (5, 3, NO_WORD), (6, 4, 1 | 17 << 4)], 1),
              ([(3, 5, 2)] * 2, [(4, 6, DROP)], 0)] * 40
    P = _planes(topics)
    full = _both(eng, gpu_device, P)
    # per two topics: 4 pairs of which one dropped, 4 live slots of which two dropped; subscribers 3, 4, 5, 6
    assert full[0] == [40 * 5, 4, 40 * 3, 40 * 2] and NO_WORD in full[4] and DROP not in full[4]
    bare = _both(eng, gpu_device, P, sub_word=False, pick_word=False)   # every pair and pick kept, ent_word NULL
    assert bare[0] == [40 * 8, 4, 40 * 4, 40 * 4]
    half = _both(eng, gpu_device, P, pick_word=False)                 # pair words only: a pick's word is 0
    assert half[0] == [40 * 7, 4, 40 * 3, 40 * 4]
    assert all(w == 0 for p, w in zip(half[2], half[4]) if p & PICK)
    half = _both(eng, gpu_device, P, sub_word=False)                  # pick words only: a pair's word is 0
    assert half[0] == [40 * 6, 4, 40 * 4, 40 * 2]
    assert all(w == 0 for p, w in zip(half[2], half[4]) if not p & PICK)
    assert _both(eng, gpu_device, P, pick=False)[0] == [40 * 3, 2, 40 * 3, 0]


def test_capacities(eng, gpu_device):
    rng = random.Random(7)
    topics = [([(rng.randrange(90), t, 1) for _ in range(rng.randint(0, 6))], [(rng.randrange(90), t, 2)] * (t % 2), 0)
              for t in range(200)]
    P = _planes(topics)
    want = _both(eng, gpu_device, P)
    E, S = want[0][0], want[0][1]
    plen, klen, n = len(P["sub_id"]), len(P["pick"]), len(topics)
    d = _upload(P, gpu_device, True, True, True, plen, plen, klen, klen)
    host = lambda ic, ec: eng.inbox_plan(P["sub_off"], P["sub_to"], P["sub_id"], P["sub_word"], P["counts"],   # noqa: E731
                                         P["offs"], P["to"], P["pick"], P["pick_word"], inbox_cap=ic, ent_cap=ec)
    for ic, ec in ((S - 1, E), (S, E - 1), (0, E), (S, 0), (0, 0)):
        with pytest.raises(L.TopicMatchError) as ex:
            host(ic, ec)
        assert ex.value.code == L.TM_ENOSPC and [int(x) for x in ex.value.hdr] == want[0]
        got = _device_plan(eng, gpu_device, n, d, plen, klen, ic, ec, True, null_out=(ic == 0 and ec == 0))
        assert [int(x) for x in got[0]] == want[0]                    # exact, and nothing at or past a capacity
        assert [tuple(r) for r in got[1].tolist()] == want[1][:ic]
        assert [int(x) for x in got[2]] == want[2][:ec] and [int(x) for x in got[4]] == want[4][:ec]
    # the host form with NULL arrays and zero capacities reports the sizes; a second call sized from them fits
    hdr = np.zeros(4, dtype=np.uint64)
    p = lambda a: a.ctypes.data   # noqa: E731
    rc = eng.lib.tm_inbox_plan(eng.h, n, p(P["sub_off"]), p(P["sub_to"]), p(P["sub_id"]), p(P["sub_word"]), plen,
                               plen, p(P["counts"]), p(P["offs"]), p(P["to"]), p(P["pick"]), p(P["pick_word"]), klen,
                               klen, p(hdr), None, 0, None, None, None, 0)
    assert rc == L.TM_ENOSPC and [int(x) for x in hdr] == want[0]
    _same(host(int(hdr[1]), int(hdr[0])), want)
    _same(_device_plan(eng, gpu_device, n, d, plen, klen, int(hdr[1]), int(hdr[0]), True), want)


# ---- over a real publish call ---------------------------------------------------------

def _world(gpu_device, seed):
    """pickword_world's world after random subscribe / unsubscribe / share add
    / share del / set-opts operations; some $share members also subscribe
    plainly to a filter their set's publishes match"""
    w = build_world(gpu_device)
    rng = random.Random(seed)
    local = [t for j, t in enumerate(w.plain_topics) if j % 3 == 0] + [b"+/t"]
    mine = []                                                  # the plain entries added here
    for g, to, topic, ms in w.sets:
        if to == topic and len(ms) >= 7:
            for m in (ms[0], ms[len(ms) // 2]):
                w.plain(b"+/t", m, rand_opts(rng) if m % 2 else None)
    big = [s for s in w.sets if len(s[3]) >= 8]
    grow = [s for s in w.sets if len(s[3]) > 1]                # a one-member set keeps its no-local publisher
    for i in range(240):
        op = rng.randrange(6)
        if op == 0:
            t, s = rng.choice(local), 3000 + i
            w.plain(t, s, rand_opts(rng) if rng.random() < 0.7 else None)
            mine.append((t, s))
        elif op == 1 and mine:
            t, s = mine.pop(rng.randrange(len(mine)))
            assert w.e.sub_del(t, s) == w.so.do_unsubscribe(None, t, s)
        elif op == 2:
            g, to, _topic, ms = rng.choice(grow)
            m = 2_000_000 + i
            w.member(g, to, m, rand_opts(rng) if rng.random() < 0.7 else None, share_first=bool(i % 2))
            ms.append(m)
        elif op == 3:
            g, to, _topic, ms = rng.choice(big)
            if len(ms) > 4:
                w.unshare(g, to, ms.pop(rng.randrange(1, len(ms) - 1)))
        elif op == 4 and mine:
            t, s = rng.choice(mine)
            w.set_opts(t, s, {"qos": rng.randrange(3), "nl": rng.randrange(2), "subid": rng.randrange(1, 5000)})
        else:
            g, to, _topic, ms = rng.choice(w.sets)
            w.set_opts(to, rng.choice(ms), {"qos": rng.randrange(3), "rap": rng.randrange(2)})
    w.e.commit()
    w.e.debug_check_subs()
    w.e.debug_check_shares()
    return w


class DevPub:
    """tm_match_publish_batch_opts_device + tm_share_pick_words_device into
    torch buffers that stay on the device for the plan"""

    def __init__(self, w, device, pubs, strategy, upgrade, cap=8192, scap=8192):
        import torch
        dev = torch.device("cuda", device)
        topics = [t for t, _k, _m in pubs]
        buf, off = pack(topics)
        n = self.n = len(topics)
        self.cap, self.scap, self.device = cap, scap, device
        i32 = lambda k, v=-7: torch.full((max(k, 1),), v, dtype=torch.int32, device=dev)   # noqa: E731
        i64 = lambda k: torch.full((k,), -1, dtype=torch.int64, device=dev)                 # noqa: E731
        self.d = dict(counts=i32(n), offs=i64(n + 1), to=i32(cap), tg=i32(cap), nd=i32(cap), pick=i32(cap),
                      total=i64(1), sc=i32(n), sub_off=i64(n + 1), sub_to=i32(scap), sub_id=i32(scap),
                      sub_word=i32(scap), sub_total=i64(1), pick_word=i32(cap))
        d = self.d
        d_b = torch.from_numpy(np.concatenate([buf, np.zeros(8, np.uint8)])).to(dev)
        d_o = _dev(off, device)
        pf, fr, fl = deliver_of(pubs, upgrade)
        d_pf, d_fr = _dev(pf, device), _dev(fr, device)
        d_k = _dev(np.asarray([k for _t, k, _m in pubs], dtype=np.uint32), device)
        torch.cuda.synchronize()
        w.e.match_publish_batch_device(d_b, d_o, n, int(off[-1]), d["counts"], d["offs"], d["to"], d["tg"], d["nd"],
                                       cap, d["total"], d["sc"], d["sub_off"], d["sub_to"], d["sub_id"], scap,
                                       d["sub_total"], STRATEGIES[strategy], d_k, d["pick"],
                                       deliver=(d_pf, d_fr, fl, d["sub_word"]))
        w.e.share_pick_words_device(d_b, d_o, n, d["counts"], d["offs"], d["to"], d["tg"], d["pick"], cap, d["total"],
                                    (d_pf, d_fr, fl), d["pick_word"])
        torch.cuda.synchronize()
        self.total, self.sub_total = int(d["total"].item()), int(d["sub_total"].item())
        assert self.total <= cap and self.sub_total <= scap

    def host(self):
        """the planes as the host forms return them"""
        g = lambda k, dt=np.uint32: self.d[k].cpu().numpy().view(dt)   # noqa: E731
        return dict(sub_off=g("sub_off", np.uint64), sub_to=g("sub_to")[:self.sub_total],
                    sub_id=g("sub_id")[:self.sub_total], sub_word=g("sub_word")[:self.sub_total],
                    counts=g("counts")[:self.n], offs=g("offs", np.uint64), to=g("to")[:self.total],
                    pick=g("pick")[:self.total], pick_word=g("pick_word")[:self.total])

    def plan(self, e, inbox_cap, ent_cap):
        return _device_plan(e, self.device, self.n, self.d, self.scap, self.cap, inbox_cap, ent_cap, True)


def _host_plan(e, P):
    return e.inbox_plan(P["sub_off"], P["sub_to"], P["sub_id"], P["sub_word"], P["counts"], P["offs"], P["to"],
                        P["pick"], P["pick_word"])


def _plane_sends(P):
    return sends_of_planes(P["sub_off"], P["sub_to"], P["sub_id"], P["sub_word"], P["counts"], P["offs"], P["to"],
                           P["pick"], P["pick_word"])


@pytest.mark.parametrize("strategy", ["keyed", "round_robin", "sticky"])
def test_publish_call_against_the_reference(gpu_device, strategy):
    w = _world(gpu_device, 21)
    pubs = publishes(w)
    topics = [t for t, _k, _m in pubs]
    assert len(pubs) <= 2000
    name = lambda to, pub: w.to_bytes(to, topics[pub])   # noqa: E731
    upgrade = strategy == "round_robin"
    buf, off = pack(topics)
    if strategy == "sticky":
        # a first batch sticks a member to every set; those of the larger sets then leave their sets and
        # are still picked: their picks are sends with TM_NO_WORD
        first = reference_sends(w.o, w.so, w.sh, NODE, strategy, pubs, upgrade)
        w.e.match_publish_batch(buf, off, STRATEGIES[strategy], keys=[k for _t, k, _m in pubs])
        for g, to, topic, ms in w.sets:
            stuck = [s[0] for s in first if s[2] == 1 and s[4] == to and topics[s[1]] == topic]
            if len(ms) >= 7 and stuck and stuck[-1] in ms:
                w.unshare(g, to, stuck[-1])
        w.e.commit()
    # the host chain: tm_match_publish_batch_opts + tm_share_pick_words + tm_inbox_plan
    ref = reference_sends(w.o, w.so, w.sh, NODE, strategy, pubs, upgrade)
    assert (strategy == "sticky") == any(s[5] == NO_WORD for s in ref)
    out = w.e.match_publish_batch(buf, off, STRATEGIES[strategy], keys=[k for _t, k, _m in pubs],
                                  deliver=deliver_of(pubs, upgrade), pick_words=True)
    P = dict(sub_off=out[6], sub_to=out[7], sub_id=out[8], sub_word=out[10], counts=out[0], offs=out[1], to=out[2],
             pick=out[9], pick_word=out[11])
    got = _host_plan(w.e, P)
    _same(got, expected_plan(_plane_sends(P)))
    assert grouped_plan(got[1].tolist(), got[2], got[3], got[4], name) == grouped(ref)
    dropped = int((P["sub_word"] == DROP).sum()), sum(
        1 for t in range(len(pubs)) for s in range(int(P["offs"][t]), int(P["offs"][t]) + int(P["counts"][t]))
        if int(P["pick_word"][s]) == DROP)
    assert dropped[0] > 0 and dropped[1] > 0 and len(ref) < 20000     # no-local publishers: sends left out
    if strategy == "keyed":
        both = [s for s, rows in grouped(ref).items()
                if any(a[0] == b[0] and not a[3] and b[3] for a in rows for b in rows)]
        assert both                                                   # a pair and a pick of one publish to one subscriber
    # the device chain over the device call's planes (the model advances once more)
    ref = reference_sends(w.o, w.so, w.sh, NODE, strategy, pubs, upgrade)
    d = DevPub(w, gpu_device, pubs, strategy, upgrade)
    P = d.host()
    want = expected_plan(_plane_sends(P))
    got = d.plan(w.e, want[0][1] + 2, want[0][0] + 3)
    _same(got, want)
    _same(_host_plan(w.e, P), want)                                   # the host form over the same planes
    assert grouped_plan(got[1].tolist(), got[2], got[3], got[4], name) == grouped(ref)
    w.close()


def test_broker_publish_inbox_many(gpu_device):
    w = _world(gpu_device, 22)
    pubs = publishes(w)
    topics, keys, msgs = ([p[i] for p in pubs] for i in range(3))
    named = lambda res: {s: [(t, topics[t] if to is None else to, wd, pk) for t, to, wd, pk in rows]   # noqa: E731
                         for s, rows in res.items()}
    for upgrade in (False, True):
        ref = reference_sends(w.o, w.so, w.sh, NODE, "keyed", pubs, upgrade)
        assert named(w.b.publish_inbox_many(topics, msgs, "keyed", keys, upgrade_qos=upgrade)) == grouped(ref)
    ref = reference_sends(w.o, w.so, w.sh, NODE, "keyed", pubs, words=False)
    got = w.b.publish_inbox_many(topics, None, "keyed", keys)
    assert named(got) == grouped(ref)                                 # no words: nothing is left out
    w.close()


def test_plan_is_stateless(gpu_device):
    w = _world(gpu_device, 23)
    pubs = publishes(w)
    d = DevPub(w, gpu_device, pubs, "round_robin", False)
    want = expected_plan(_plane_sends(d.host()))
    for _ in range(2):
        _same(d.plan(w.e, want[0][1], want[0][0]), want)
    w.close()


def test_commit_between_the_publish_call_and_the_plan(gpu_device):
    """the plan reads no image: changes committed after the publish call leave it as it was"""
    w = _world(gpu_device, 24)
    pubs = publishes(w)
    d = DevPub(w, gpu_device, pubs, "sticky", True)
    P = d.host()
    want = expected_plan(_plane_sends(P))
    g, to, _topic, ms = w.sets[-1]
    for m in ms[:5]:
        w.unshare(g, to, m)
    w.plain(b"+/t", 123456, {"qos": 2, "nl": 1})
    w.set_opts(b"+/t", 799, {"nl": 0, "qos": 2})
    w.e.commit()
    _same(d.plan(w.e, want[0][1] + 1, want[0][0] + 1), want)
    _same(_host_plan(w.e, P), want)
    w.close()
