"""tm_inbox_plan_stream_device on the GPU (inbox.hip): the plan computed from
the packed outputs of the stream-ordered publish call, against the reference
model (tests/inbox_ref.py: expected_plan over the sends the packed arrays
define; over a real world also reference_sends), and in state 0 bit for bit
against tm_inbox_plan fed the same data as planes.  Every output and the
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
from inbox_ref import (DROP, NO_MEMBER, NO_WORD, PICK, ROUTE_TOPIC, expected_plan, grouped, grouped_plan,  # noqa: E402
                       reference_sends)
from pickword_world import NODE, STRATEGIES, build_world, deliver_of, publishes  # noqa: E402
from emqx_amd import Engine  # noqa: E402
from emqx_amd.engine import pack  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 8
FILL = 0xFFFFFFF9                 # -7: what the result arrays hold before a call
FILL64 = 0xFFFFFFFFFFFFFFF9
DECOY = 424242                    # an id in a record past a bound: never sent


@pytest.fixture(scope="module")
def eng(gpu_device):
    e = Engine(device=gpu_device)
    yield e
    e.close()


class Packed:
    """topics = [(pairs, recs)]: pairs = [(sub, to, word)], recs = [(pick, to,
    word)] -> the packed outputs of a publish call as host arrays"""

    def __init__(self, topics, state=0):
        pairs, pairw, deliv, pickw, soff, doff = [], [], [], [], [0], [0]
        for prs, recs in topics:
            for sub, to, word in prs:
                pairs.append((to, sub))
                pairw.append(word)
            soff.append(len(pairs))
            for pick, to, word in recs:
                deliv.append((to, 5, 2, pick))
                pickw.append(word)
            doff.append(len(deliv))
        self.n = len(topics)
        self.soff, self.doff = np.asarray(soff, dtype=np.uint64), np.asarray(doff, dtype=np.uint64)
        self.pairs = np.asarray(pairs, dtype=np.uint32).reshape(-1, 2)
        self.deliv = np.asarray(deliv, dtype=np.uint32).reshape(-1, 4)
        self.pairw, self.pickw = np.asarray(pairw, dtype=np.uint32), np.asarray(pickw, dtype=np.uint32)
        self.hdr = np.asarray([len(deliv) + 3, len(pairs), len(deliv), len(pairs), 9, 0, state, 0], dtype=np.uint64)


def packed_sends(K, deliv_cap, pair_cap, pair_word=True, pick_word=True):
    """the send definition of tm_inbox_plan_stream_device over host copies of the packed arrays"""
    P, D = min(int(K.hdr[3]), pair_cap), min(int(K.hdr[2]), deliv_cap)
    sends = []
    for t in range(K.n):
        for p in range(int(K.soff[t]), int(K.soff[t + 1])):
            if p >= P:
                continue
            word = int(K.pairw[p]) if pair_word else None
            if word == DROP:
                continue
            sends.append((int(K.pairs[p][1]), t, 0, p, int(K.pairs[p][0]), word))
    for t in range(K.n):
        for d in range(int(K.doff[t]), int(K.doff[t + 1])):
            if d >= D or int(K.deliv[d][3]) == NO_MEMBER:
                continue
            word = int(K.pickw[d]) if pick_word else None
            if word == DROP:
                continue                                       # NO_WORD is kept
            sends.append((int(K.deliv[d][3]), t, 1, d, int(K.deliv[d][0]), word))
    return sends


def _rows(a, cap, width, fill):
    """the first cap rows of a (decoy rows past its end), as an int32 tensor source"""
    out = np.full((max(cap, 1), width), fill, dtype=np.uint32)
    k = min(cap, len(a))
    if k:
        out[:k] = np.asarray(a[:k]).reshape(k, width)
    return out.reshape(-1)


class Dev:
    """the packed arrays on the device, cut (or padded with decoys) to the capacities"""

    def __init__(self, K, device, deliv_cap, pair_cap):
        import torch
        dev = torch.device("cuda", device)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(dev)   # noqa: E731
        self.device, self.deliv_cap, self.pair_cap = device, deliv_cap, pair_cap
        self.hdr, self.doff, self.soff = up(K.hdr, np.int64), up(K.doff, np.int64), up(K.soff, np.int64)
        self.deliv = up(_rows(K.deliv, deliv_cap, 4, DECOY), np.int32)
        self.pairs = up(_rows(K.pairs, pair_cap, 2, DECOY), np.int32)
        self.pickw = up(_rows(K.pickw, deliv_cap, 1, 1), np.int32)
        self.pairw = up(_rows(K.pairw, pair_cap, 1, 1), np.int32)


def run_plan(e, d, n, sub_bits, inbox_cap, ent_cap, pair_word=True, pick_word=True, ent_word=True, stream=None):
    """one call -> (hdr[8], inbox rows, ent_pub, ent_to, ent_word | None), each
    cut where the header says the call wrote; everything else must hold its fill"""
    import torch
    dev = torch.device("cuda", d.device)
    ws_bytes = e.inbox_plan_stream_workspace_bytes(n, d.deliv_cap, d.pair_cap, ent_cap)
    assert ws_bytes > 0 and ws_bytes % 8 == 0
    ws = torch.full((ws_bytes // 8 + GUARD,), -7, dtype=torch.int64, device=dev)
    hdr = torch.full((8 + GUARD,), -7, dtype=torch.int64, device=dev)
    inbox = torch.full(((inbox_cap + GUARD) * 4,), -7, dtype=torch.int32, device=dev)
    ent = [torch.full((ent_cap + GUARD,), -7, dtype=torch.int32, device=dev) for _ in range(3)]
    if stream is None:
        torch.cuda.synchronize()
    e.inbox_plan_stream_device(n, d.hdr, d.doff, d.soff, d.deliv if d.deliv_cap else None,
                               d.pickw if pick_word else None, d.deliv_cap, d.pairs if d.pair_cap else None,
                               d.pairw if pair_word else None, d.pair_cap, sub_bits, ws, ws_bytes, hdr,
                               inbox if inbox_cap else None, inbox_cap, ent[0] if ent_cap else None,
                               ent[1] if ent_cap else None, ent[2] if ent_word and ent_cap else None, ent_cap,
                               stream=stream)
    torch.cuda.synchronize()
    hdr = hdr.cpu().numpy().view(np.uint64)
    inbox = inbox.cpu().numpy().view(np.uint32)
    ent = [x.cpu().numpy().view(np.uint32) for x in ent]
    assert (hdr[8:] == FILL64).all()
    assert (ws.cpu().numpy().view(np.uint64)[ws_bytes // 8:] == FILL64).all()
    h = [int(x) for x in hdr[:8]]
    state = h[6]
    assert state in (0, 1, 2, 3, 4) and h[5] == 0 and h[7] == 0
    en = min(h[0], ent_cap) if state in (0, 4) else 0
    sn = min(h[1], inbox_cap) if state in (0, 4) else 0
    assert (inbox[sn * 4:] == FILL).all()
    assert (ent[0][en:] == FILL).all() and (ent[1][en:] == FILL).all()
    assert (ent[2][en if ent_word else 0:] == FILL).all()
    return h, inbox[:sn * 4].reshape(-1, 4), ent[0][:en], ent[1][:en], ent[2][:en] if ent_word else None


def _same(got, want, words=True):
    """a state 0 result against the model's plan"""
    h, inbox, ent_pub, ent_to, ent_word = got
    top = max([r[0] for r in want[1]], default=0)
    assert h == want[0] + [top, 0, 0, 0]
    assert [tuple(r) for r in inbox.tolist()] == want[1]
    assert [int(x) for x in ent_pub] == want[2]
    assert [int(x) for x in ent_to] == want[3]
    if words:
        assert [int(x) for x in ent_word] == want[4]
    else:
        assert ent_word is None


def _host_form(e, K, deliv_cap, pair_cap, pair_word, pick_word):
    """tm_inbox_plan over the same data as planes (a dense record is a slot without holes)"""
    pc, dc = min(pair_cap, len(K.pairs)), min(deliv_cap, len(K.deliv))
    return e.inbox_plan(K.soff, K.pairs[:pc, 0], K.pairs[:pc, 1], K.pairw[:pc] if pair_word else None,
                        np.diff(K.doff.astype(np.int64)).astype(np.uint32), K.doff, K.deliv[:dc, 0], K.deliv[:dc, 3],
                        K.pickw[:dc] if pick_word else None, sub_total=int(K.hdr[3]), sub_cap=pc,
                        total=int(K.hdr[2]), out_cap=dc, words=True)


def check(e, device, K, sub_bits=0, deliv_cap=None, pair_cap=None, pair_word=True, pick_word=True, ent_word=True):
    """state 0 at roomy capacities: the model, and the host form bit for bit -> the model's plan"""
    deliv_cap = len(K.deliv) + 5 if deliv_cap is None else deliv_cap
    pair_cap = len(K.pairs) + 7 if pair_cap is None else pair_cap
    want = expected_plan(packed_sends(K, deliv_cap, pair_cap, pair_word, pick_word))
    d = Dev(K, device, deliv_cap, pair_cap)
    got = run_plan(e, d, K.n, sub_bits, want[0][1] + 2, want[0][0] + 3, pair_word, pick_word, ent_word)
    assert got[0][6] == 0
    _same(got, want, ent_word)
    # ent_cap = pair_cap + deliv_cap cannot overflow, whatever the sends
    got = run_plan(e, d, K.n, sub_bits, pair_cap + deliv_cap, pair_cap + deliv_cap, pair_word, pick_word, ent_word)
    _same(got, want, ent_word)
    if K.n and min(pair_cap, len(K.pairs)) and min(deliv_cap, len(K.deliv)):
        host = _host_form(e, K, deliv_cap, pair_cap, pair_word, pick_word)
        assert [int(x) for x in host[0]] == got[0][:4]
        assert host[1].tobytes() == got[1].tobytes() and host[2].tobytes() == got[2].tobytes()
        assert host[3].tobytes() == got[3].tobytes()
        if ent_word:
            assert host[4].tobytes() == got[4].tobytes()
    return want


# ---- synthetic packed records --------------------------------------------------------

def test_empty_batch(eng, gpu_device):
    K = Packed([])
    for caps in ((0, 0), (4, 4)):
        got = run_plan(eng, Dev(K, gpu_device, *caps), 0, 16, 3, 3)
        assert got[0] == [0] * 8 and len(got[1]) == 0


def test_batch_without_a_send(eng, gpu_device):
    K = Packed([([(5, 1, DROP), (6, 1, DROP)], [(NO_MEMBER, 3, NO_WORD)] * 3), ([], []),
                ([(5, ROUTE_TOPIC, DROP)] * 70, [(9, 4, DROP)] * 2)])
    assert check(eng, gpu_device, K)[0] == [0, 0, 0, 0]
    got = run_plan(eng, Dev(K, gpu_device, 0, 0), K.n, 16, 0, 0)   # no capacity at all
    assert got[0] == [0] * 8


def test_spans_across_topic_blocks(eng, gpu_device):
    """600 topics with 0..5 pairs and 0..3 records each: blocks of 256 topics are crossed"""
    rng = random.Random(11)
    topics = [([(rng.randrange(1, 400), t, rng.choice([0, 1, 2, DROP])) for _ in range(rng.randint(0, 5))],
               [(rng.choice([NO_MEMBER, rng.randrange(1, 400)]), 1000 + t, rng.choice([1, NO_WORD, DROP]))
                for _ in range(rng.randint(0, 3))]) for t in range(600)]
    K = Packed(topics)
    want = check(eng, gpu_device, K, sub_bits=9)
    assert want[0][2] > 500 and want[0][3] > 150 and want[0][1] > 300
    assert NO_WORD in want[4] and DROP not in want[4]          # dropped words of both kinds left out, TM_NO_WORD picks kept
    assert (K.pairw == DROP).any() and (K.pickw == DROP).any()


def test_one_run_across_a_block_and_a_sort_tile(eng, gpu_device):
    """subscriber 500 receives more than 4096 entries, between two other subscribers' runs"""
    topics = [([(100, 9, 1)] * 3, [])]
    topics += [([(500, t, 2), (900, 9, 3), (500, t, 1)], [(500, 1000 + t, 4)] if t % 7 == 0 else []) for t in range(2300)]
    want = check(eng, gpu_device, Packed(topics), sub_bits=10)
    npick = len(range(0, 2300, 7))
    assert want[1][1] == (500, 3, 4600 + npick, npick) and 4600 + npick > 4096
    pubs = [x & ~PICK for x in want[2][3:3 + 4600 + npick]]
    assert pubs == sorted(pubs)


@pytest.mark.parametrize("bits,top", [(8, 200), (16, 60000), (20, (1 << 19) + 3), (32, 0xFFFFFFFE), (0, 0xFFFFFFFE)])
def test_ids_of_every_sort_width(eng, gpu_device, bits, top):
    """ids that need one, two, three and four radix passes, 0xFFFFFFFE among them"""
    rng = random.Random(bits)
    topics = []
    for t in range(60):
        ids = [rng.randint(0, top) for _ in range(rng.randint(0, 12))]
        if t == 7:
            ids += [top, 0, top]
        topics.append(([(s, t % 9, t % 3) for s in ids[1:]], [(s, 3, NO_WORD) for s in ids[:1]]))
    want = check(eng, gpu_device, Packed(topics), sub_bits=bits)
    assert want[1][-1][0] == top and want[1][0][0] == 0


def test_id_that_ties_with_the_padding(eng, gpu_device):
    """id 0xFFFF with sub_bits = 16: every sorted digit equals the padding's; the
    padding lies behind the live entries and the sort is stable"""
    topics = [([(0xFFFF, t, 1), (3, t, 2), (0xFFFF, 50 + t, 0)], [(0xFFFF, 9, 4)] if t % 2 else [(0xFF, 9, 4)])
              for t in range(40)]
    K = Packed(topics)
    want = check(eng, gpu_device, K, sub_bits=16)
    assert want[1][-1] == (0xFFFF, 60, 100, 20)
    # the same with far more padding than entries, through more than one sort tile
    d = Dev(K, gpu_device, len(K.deliv), len(K.pairs))
    _same(run_plan(eng, d, K.n, 16, 9000, 9000), want)


def test_null_word_planes(eng, gpu_device):
    topics = [([(3, 1, DROP), (4, 1, 5)], [(3, 2, DROP), (5, 3, NO_WORD), (6, 4, 1 | 17 << 4)]),
              ([(3, 5, 2)] * 2, [(4, 6, DROP)])] * 40
    K = Packed(topics)
    full = check(eng, gpu_device, K, sub_bits=3)
    assert full[0] == [40 * 5, 4, 40 * 3, 40 * 2]
    bare = check(eng, gpu_device, K, pair_word=False, pick_word=False)   # every pair and record kept, word 0
    assert bare[0] == [40 * 8, 4, 40 * 4, 40 * 4] and set(bare[4]) == {0}
    half = check(eng, gpu_device, K, pick_word=False)
    assert half[0] == [40 * 7, 4, 40 * 3, 40 * 4]
    assert all(w == 0 for p, w in zip(half[2], half[4]) if p & PICK)
    half = check(eng, gpu_device, K, pair_word=False)
    assert half[0] == [40 * 6, 4, 40 * 4, 40 * 2]
    assert all(w == 0 for p, w in zip(half[2], half[4]) if not p & PICK)
    check(eng, gpu_device, K, ent_word=False)                            # d_ent_word NULL: not written


def test_header_totals_below_and_above_the_capacities(eng, gpu_device):
    rng = random.Random(6)
    topics = [([(rng.randrange(1, 40), t, 1) for _ in range(rng.randint(0, 5))],
               [(rng.choice([NO_MEMBER, rng.randrange(1, 40)]), t, 2) for _ in range(rng.randint(0, 4))])
              for t in range(300)]
    K = Packed(topics)
    want = check(eng, gpu_device, K)
    plen, dlen = len(K.pairs), len(K.deliv)
    # P and D above the capacities: the arrays hold fewer positions than the publish call counted
    cut = check(eng, gpu_device, K, deliv_cap=dlen - 41, pair_cap=plen - 57)
    assert 0 < cut[0][2] < want[0][2] and 0 < cut[0][3] < want[0][3]
    # P and D below the capacities: what lies past them is stale
    K.pairs[plen - 30:, 1] = DECOY
    K.deliv[dlen - 30:, 3] = DECOY
    K.hdr[3], K.hdr[2] = plen - 30, dlen - 30
    cut = check(eng, gpu_device, K)
    assert DECOY not in [r[0] for r in cut[1]] and cut[0][0] < want[0][0]


# ---- the four states other than 0 ----------------------------------------------------

def _small():
    """E = 8 sends (5 pairs, 3 picks) to S = 4 subscribers (5, 7, 9, 300), one pair dropped"""
    return Packed([([(7, 1, 1), (300, 1, 1)], [(9, 2, 2)]),
                   ([(7, 10, 1), (6, 11, DROP), (7, 12, 2), (5, 13, 0)], [(7, 20, 4), (NO_MEMBER, 21, NO_WORD), (300, 22, 1)])])


def test_state_1_publish_call_did_not_fit(eng, gpu_device):
    K = _small()
    K.hdr[6] = 2
    d = Dev(K, gpu_device, len(K.deliv), len(K.pairs))
    got = run_plan(eng, d, K.n, 16, 8, 8)                      # run_plan: every result array still holds its fill
    assert got[0] == [0, 0, 0, 0, 0, 0, 1, 0]


def test_state_2_id_wider_than_sub_bits(eng, gpu_device):
    K = _small()
    want = expected_plan(packed_sends(K, len(K.deliv), len(K.pairs)))
    assert want[0] == [8, 4, 5, 3]
    d = Dev(K, gpu_device, len(K.deliv), len(K.pairs))
    got = run_plan(eng, d, K.n, 8, 8, 8)
    assert got[0] == [8, 0, 5, 3, 300, 0, 2, 0]                # nothing else written (run_plan)
    _same(run_plan(eng, d, K.n, 16, 8, 8), want)
    _same(run_plan(eng, d, K.n, 9, 8, 8), want)                # 300 needs nine bits
    # an id whose low sub_bits bits are all ones and a bit above them: detected, never mis-sorted
    K = Packed([([(0x1FF, 1, 1), (2, 1, 1)], [])])
    got = run_plan(eng, Dev(K, gpu_device, 1, 2), 1, 8, 4, 4)
    assert got[0] == [2, 0, 2, 0, 0x1FF, 0, 2, 0]


def test_state_3_entries_do_not_fit(eng, gpu_device):
    K = _small()
    d = Dev(K, gpu_device, len(K.deliv), len(K.pairs))
    got = run_plan(eng, d, K.n, 16, 8, 7)                      # ent_cap = E - 1
    assert got[0] == [8, 0, 5, 3, 300, 0, 3, 0]
    got = run_plan(eng, d, K.n, 16, 8, 0)
    assert got[0] == [8, 0, 5, 3, 300, 0, 3, 0]
    got = run_plan(eng, d, K.n, 8, 8, 7)                       # the first condition that applies wins
    assert got[0][6] == 2


def test_state_4_records_do_not_fit(eng, gpu_device):
    K = _small()
    want = expected_plan(packed_sends(K, len(K.deliv), len(K.pairs)))
    d = Dev(K, gpu_device, len(K.deliv), len(K.pairs))
    h, inbox, ent_pub, ent_to, ent_word = run_plan(eng, d, K.n, 16, 3, 8)   # inbox_cap = S - 1
    assert h == [8, 4, 5, 3, 300, 0, 4, 0]
    assert [tuple(r) for r in inbox.tolist()] == want[1][:3]   # exactly S - 1 records
    assert [int(x) for x in ent_pub] == want[2] and [int(x) for x in ent_to] == want[3]
    assert [int(x) for x in ent_word] == want[4]               # the entries are complete


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
        self.device, self.deliv_cap, self.pair_cap = device, cr, cp
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
        w.e.publish_stream_opts_device(d_b, d_o, n, int(off[-1]), STRATEGIES[strategy], d_k, None, ROOMY, self.ws,
                                       ws_bytes, self.hdr, self.doff, self.soff, self.deliv, self.pairs,
                                       (d_pf, d_fr, fl, self.pairw), self.pickw, stream=stream)

    def host(self):
        """the outputs as a Packed-like object for packed_sends (after a synchronize)"""
        g = lambda t, dt: t.cpu().numpy().view(dt)   # noqa: E731
        K = Packed([])
        K.n, K.hdr, K.doff, K.soff = self.n, g(self.hdr, np.uint64), g(self.doff, np.uint64), g(self.soff, np.uint64)
        K.deliv, K.pairs = g(self.deliv, np.uint32).reshape(-1, 4), g(self.pairs, np.uint32).reshape(-1, 2)
        K.pickw, K.pairw = g(self.pickw, np.uint32), g(self.pairw, np.uint32)
        return K


@pytest.mark.parametrize("strategy,sub_bits", [("keyed", 0), ("round_robin", 18), ("sticky", 24)])
def test_behind_the_publish_call_on_one_stream(gpu_device, strategy, sub_bits):
    import torch
    w = build_world(gpu_device)
    w.e.commit()
    pubs = publishes(w)
    topics = [t for t, _k, _m in pubs]
    upgrade = strategy == "round_robin"
    ref = reference_sends(w.o, w.so, w.sh, NODE, strategy, pubs, upgrade)
    assert max(s[0] for s in ref) > 65535 and any(s[2] for s in ref) and any(not s[2] for s in ref)
    st = torch.cuda.Stream(device=torch.device("cuda", gpu_device))
    d = StreamPublish(w, gpu_device, pubs, strategy, upgrade, st)
    ecap = d.deliv_cap + d.pair_cap
    got = run_plan(w.e, d, d.n, sub_bits, ecap, ecap, stream=st)   # enqueued behind the publish call: no wait between
    K = d.host()
    assert int(K.hdr[6]) == 0 and got[0][6] == 0
    want = expected_plan(packed_sends(K, d.deliv_cap, d.pair_cap))
    _same(got, want)
    host = _host_form(w.e, K, d.deliv_cap, d.pair_cap, True, True)
    assert host[1].tobytes() == got[1].tobytes() and host[2].tobytes() == got[2].tobytes()
    assert host[3].tobytes() == got[3].tobytes() and host[4].tobytes() == got[4].tobytes()
    name = lambda to, pub: w.to_bytes(to, topics[pub])   # noqa: E731
    assert grouped_plan(got[1].tolist(), got[2], got[3], got[4], name) == grouped(ref)
    # too narrow a width is reported with the widest id, and the plan may simply run again
    narrow = run_plan(w.e, d, d.n, 16, ecap, ecap, stream=st)
    assert narrow[0][6] == 2 and narrow[0][4] == want[1][-1][0] and narrow[0][0] == want[0][0]
    # the plan reads no image: subscribers deleted and committed after the publish call change nothing
    g, to, _topic, ms = w.sets[-1]
    for m in ms[:5]:
        w.unshare(g, to, m)
    w.e.sub_del(b"+/t", 700)
    w.e.commit()
    _same(run_plan(w.e, d, d.n, sub_bits, ecap, ecap, stream=st), want)
    w.close()
