"""tests/collision_corpus.py on the CPU: (1) its port of word_hash is the
engine's (tm_route_of exposes hash >> 32 mod n_shards; three coprime moduli
pin the high half, which holds the dictionary tag); (2) every class holds
what its name promises, recomputed with the port, so a later edit of the
generator cannot quietly thin it; (3) oracle.O1 and oracle.pytrie agree on
every corpus topic, every stored topic has a match and every absent one
matches wildcard-only filters; (4) the host's exact-topic tables (MirrorTable
under the route, subscriber and share images) keep equal-hash keys apart
through adds, deletes in every order (backward shifts over runs of one home,
the wrapped run's head included), re-adds and a regrow, against the three
Python references, with the debug checks after every step."""
import ctypes
import itertools
import math
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import collision_corpus as K  # noqa: E402
from emqx_amd import _lib as L  # noqa: E402
from emqx_amd.engine import pack  # noqa: E402

D_CLASSES = ["D-head0", "D-head0-long", "D-head1", "D-head1-long", "D-arena", "D-len255"]
E_CLASSES = ["E-first", "E-mid", "E-partial", "E-triple", "E-wrap"]


# ---- 1. the port ----------------------------------------------------------------------

def test_port_equals_the_engines_word_hash():
    lib = L.load()
    rng = random.Random(K.SEED)
    lengths = list(range(41)) + [255, 256, 300]
    words = [bytes(c if c != 0x2F else 0x2E for c in rng.randbytes(n)) for n in lengths for _ in range(46)]
    words += [w for g in K.dict_groups() for w in K.strings(g)]
    assert len(set(words)) >= 2000 and {len(w) for w in words} >= set(lengths)
    mods = [2 ** 32 - 1, 2 ** 32 - 2, 2 ** 32 - 3]          # pairwise coprime, product > 2^32: the residues pin hash >> 32
    assert all(math.gcd(a, b) == 1 for a, b in itertools.combinations(mods, 2))
    for w in words:
        hi = K.word_hash(w) >> 32
        for n in mods:
            assert lib.tm_route_of(w, len(w), n, 1, 0) == hi % n, (w[:40], len(w), n)


def test_port_primitives():
    # the worked pair of the hash's two-chunk inversion, and the numpy port against the scalar one
    assert K.word_hash(b"ieqh524yng5by1a2") == K.word_hash(b"rogubbb8\x1a\x18\x39\xcf\x07\xf0\xbb\xb1") == \
        0x82EF724160BD23B8
    assert K.KA * K.KA_INV % 2 ** 32 == 1 and K.KB * K.KB_INV % 2 ** 32 == 1
    rng = random.Random(K.SEED + 1)
    for _ in range(200):
        s, t, c = (rng.getrandbits(64) for _ in range(3))
        assert K.word_hash_step(s, K.solve_chunk(s, t)) == t
        assert K.solve_chunk(s, K.word_hash_step(s, c)) == c
        assert K.solve_chunk(t, K.word_hash_step(s, c)) == c ^ s ^ t     # the step reads h ^ chunk only
    chunks = np.array([rng.getrandbits(64) for _ in range(500)], dtype=np.uint64)
    for n in (1, 8, 9, 255, 256, 300):
        s = rng.getrandbits(64)
        k = n % 8 or 8
        cs = chunks & np.uint64((1 << 8 * k) - 1)
        got = K.np_hash_tail(s, cs, n)
        assert got.tolist() == [K.word_hash_final(K.word_hash_step(s, int(c)), n) for c in cs]
        assert K.np_step(s, cs).tolist() == [K.word_hash_step(s, int(c)) for c in cs]
    assert K.dict_tag(0x123456789ABCDEF0, 7) == 0x12345607 and K.dict_tag(0x123456789ABCDEF0, 300) == 0x123456FF


# ---- 2. the classes --------------------------------------------------------------------

def _lens(gs):
    return sorted({len(s) for g in gs for s in K.strings(g)})


def test_every_class_is_there_and_deterministic():
    g = K.groups()
    assert list(g) == D_CLASSES + E_CLASSES
    assert K.groups() is g                                   # cached per process
    assert K._build() == g                                   # seeded: a second build gives the same bytes
    for name, gs in g.items():
        assert len(gs) >= 4, name
        for x in gs:
            ss = K.strings(x)
            assert x.cls == name and 2 <= len(ss) <= 4 and len(set(ss)) == len(ss), name
            assert len(x.members) >= 1
        assert any(x.absent is not None for x in gs), name   # D-absent / E-absent: in every class
    for name in E_CLASSES:
        assert all(x.absent is not None and len(x.members) >= 2 for x in g[name]), name


@pytest.mark.parametrize("name", D_CLASSES)
def test_dictionary_groups_share_tag_and_home(name):
    for x in K.groups()[name]:
        ss = K.strings(x)
        hs = [K.word_hash(s) for s in ss]
        assert len({K.dict_tag(h, len(s)) for h, s in zip(hs, ss)}) == 1, ss
        assert len({h & 0xFFF for h in hs}) == 1, ss         # one home slot up to 4096 slots
        assert len({K.key36(h) for h in hs}) == 1
        for s in ss:
            assert b"/" not in s and s not in (b"+", b"#") and s[:1] != b"$", s


def _diffs(x):
    ss = K.strings(x)
    return {K.first_diff(a, b) for a, b in itertools.combinations(ss, 2)}


def test_dictionary_classes_reach_the_branch_they_are_named_for():
    g = K.groups()
    # head0 rejects: words of <= 8 bytes, and of 16 that differ in bytes 0-7 (all 64 hash bits equal)
    assert _lens(g["D-head0"]) == [3, 6, 8]
    assert _lens(g["D-head0-long"]) == [16]
    for x in g["D-head0-long"]:
        assert _diffs(x) == {0} and len({K.word_hash(s) for s in K.strings(x)}) == 1
    # head1 rejects: bytes 0-7 equal, bytes 8-15 differ
    assert _lens(g["D-head1"]) == [12, 16] and _lens(g["D-head1-long"]) == [24, 32]
    for x in g["D-head1"] + g["D-head1-long"]:
        assert _diffs(x) == {1}
    for x in g["D-head1-long"]:
        assert len({K.word_hash(s) for s in K.strings(x)}) == 1
    # the arena loop rejects: 16 equal bytes, the first difference at i = 16 or i = 24, whole and partial last chunks
    assert _lens(g["D-arena"]) == [21, 29, 32, 40]
    by_len = {}
    for x in g["D-arena"]:
        by_len.setdefault(len(x.members[0]), set()).update(_diffs(x))
    assert by_len == {32: {2}, 40: {3}, 21: {2}, 29: {3}}
    # the exact length decides: one tag length byte (255) for 255, 256 and 300 bytes
    pairs = sorted(tuple(len(s) for s in K.strings(x)) for x in g["D-len255"])
    assert pairs.count((255, 256)) >= 3 and (255, 300) in pairs and (256, 300) in pairs
    for x in g["D-len255"]:
        a, b = K.strings(x)
        assert (a[:16] == b[:16]) == (len(a) == 255), (len(a), len(b))     # the 256 / 300 pair differs in its head
        assert K.dict_tag(K.word_hash(a), len(a)) & 0xFF == 255
    # ... and one pair that nothing but the stored length tells apart: w and w + NUL (heads and arena are zero padded)
    nul = [x for x in g["D-len255"] if x.members[-1] == x.members[0] + b"\0"]
    assert len(nul) == 1 and len(nul[0].members[0]) == 255


@pytest.mark.parametrize("name", E_CLASSES)
def test_exact_groups_share_length_and_all_64_bits(name):
    for x in K.groups()[name]:
        ss = K.strings(x)
        assert len({len(s) for s in ss}) == 1 and len({K.word_hash(s) for s in ss}) == 1, ss
        lv = [w for s in ss for w in s.split(b"/")]
        assert b"+" not in lv and b"#" not in lv


def test_exact_classes_hold_their_shapes():
    g = K.groups()
    assert _lens(g["E-first"]) == [16] and all(_diffs(x) == {0} for x in g["E-first"])
    assert sorted((len(x.members[0]), min(_diffs(x))) for x in g["E-mid"]) == [(24, 1), (24, 1), (32, 2), (32, 2)]
    assert _lens(g["E-partial"]) == [14, 15, 23]             # the solved last chunk has zero high bytes: it fits
    assert _lens(g["E-triple"]) == [16, 32] and all(len(x.members) == 3 for x in g["E-triple"])
    assert all(len(x.members) == 3 for x in g["E-wrap"])
    for x in g["E-wrap"]:                                    # home = the last slot of a 16-slot table
        assert {K.word_hash(s) & 15 for s in K.strings(x)} == {15}


def test_workload_stays_inside_a_4096_slot_dictionary():
    fs = K.filters()
    words = {w for f in fs for w in f.split(b"/")}
    stored = {w for x in K.dict_groups() for w in x.members}
    assert stored <= words and len(words) < K.MAX_WORDS == 2048
    assert sorted(K.filters(reverse=True)) == sorted(fs) and K.filters(reverse=True) != fs
    ts = K.topics()
    assert 200 <= len(ts) <= 600
    absent = {w for x in K.dict_groups() if x.absent is not None for w in [x.absent]}
    assert not absent & words
    assert {t for _, a, t in ts if a} == {f % w for w in absent for f in (b"%s", b"p/%s/q", b"x/%s")}
    # partners side by side: every group's strings are consecutive topics
    flat = [t for _, _, t in ts]
    for x in K.dict_groups():
        i = flat.index(x.members[0])
        assert flat[i:i + len(K.strings(x))] == list(K.strings(x))


class _DictModel:
    """engine.cpp's dictionary placement (word_id / dict_place / dict_grow:
    1024 slots, doubled past load 1/2, linear probing, words interned in the
    order the filters' levels arrive) and kernels.hip's dict_end as a model,
    with switches for the checks a wrong kernel could leave out"""

    def __init__(self, fs):
        self.slots = [None] * 1024
        self.words = []
        for f in fs:
            for w in f.split(b"/"):
                if w not in (b"+", b"#") and w not in self.words:
                    if (len(self.words) + 1) * 2 > len(self.slots):
                        old, self.slots = self.slots, [None] * (2 * len(self.slots))
                        for k in old:
                            if k is not None:
                                self._place(k)
                    self.words.append(w)
                    self._place(len(self.words) - 1)

    def _place(self, k):
        s = K.word_hash(self.words[k]) & (len(self.slots) - 1)
        while self.slots[s] is not None:
            s = (s + 1) & (len(self.slots) - 1)
        self.slots[s] = k

    def lookup(self, w, verify_bytes=True, verify_len=True):
        """(word id or None, slots of equal tag the probe passed over)"""
        h = K.word_hash(w)
        s, n, passed = h & (len(self.slots) - 1), len(w), 0
        while self.slots[s] is not None:
            k = self.slots[s]
            x = self.words[k]
            if K.dict_tag(K.word_hash(x), len(x)) == K.dict_tag(h, n):
                pad = x + b"\0" * (-len(x) % 8 + 64)         # heads and arena are zero padded,
                wp = w + b"\0" * (-n % 8)                    # and so is the topic's last chunk
                eq = not verify_bytes or n == 0 or wp[:8] == pad[:8]
                if eq and n > 8:
                    eq = (not verify_len or len(x) == n) and (not verify_bytes or wp[8:16] == pad[8:16])
                    if eq and n > 16 and verify_bytes:
                        eq = wp[16:] == pad[16:len(wp)]
                if eq:
                    return k, passed
                passed += 1
            s = (s + 1) & (len(self.slots) - 1)
        return None, passed


@pytest.mark.parametrize("reverse", [False, True])
def test_lookups_reach_the_reject_branch_and_a_lookup_without_it_goes_wrong(reverse):
    """on a model of the dictionary as the engine fills it: the probe of every
    group's later partner passes over the earlier one's slot (equal tag, other
    bytes), an absent word's over every stored partner; a lookup that skips
    the byte compares returns a wrong id in every class of one length (the
    exact-length test still parts D-len255), one that skips only the
    exact-length test in D-len255 alone (w / w + NUL)"""
    fs = K.filters(reverse)
    m = _DictModel(fs)
    assert len(m.slots) <= 4096
    # the model interns as the engine does: every word's id (its interning rank) is the host dictionary's,
    # an absent word has none
    from emqx_amd import Engine
    e = Engine(device=-1)
    e.insert_many(*pack(fs))
    ws = [w for x in K.dict_groups() for w in K.strings(x)] + [b"p", b"q", b""]
    wb, wo = pack(ws)
    lv, ids = np.zeros(len(ws), dtype=np.uint32), np.zeros(len(ws), dtype=np.uint32)
    rc = e.lib.tm_debug_words(e.h, wb.ctypes.data_as(ctypes.c_void_p), wo.ctypes.data_as(ctypes.c_void_p), len(ws),
                              lv.ctypes.data_as(ctypes.c_void_p), ids.ctypes.data_as(ctypes.c_void_p),
                              ctypes.c_uint64(len(ws)))
    e.close()
    assert rc == 0 and lv.tolist() == [1] * len(ws)
    assert ids.tolist() == [m.words.index(w) if w in m.words else 0xFFFFFFFF for w in ws]
    wrong_bytes, wrong_len = set(), set()
    for x in K.dict_groups():
        order = x.members[::-1] if reverse else x.members
        for i, w in enumerate(order):
            k, passed = m.lookup(w)
            assert m.words[k] == w and passed == i, (x.cls, w)
        if x.absent is not None:
            assert m.lookup(x.absent) == (None, len(x.members)), (x.cls, x.absent)
        for w in K.strings(x):
            want = m.words.index(w) if w in m.words else None
            if m.lookup(w, verify_bytes=False)[0] != want:
                wrong_bytes.add(x.cls)
            if m.lookup(w, verify_len=False)[0] != want:
                wrong_len.add(x.cls)
                assert w + b"\0" in x.members or w[:-1] in x.members, w[-20:]
    assert wrong_bytes == set(D_CLASSES) - {"D-len255"} and wrong_len == {"D-len255"}


def test_batches_fit_the_wave_tokenizers_window():
    """a wave whose bytes or levels pass the LDS window is tokenized per lane:
    every batch must stay inside, at both envelope offsets, or wave_dict_end
    would never meet the words of 255 bytes and more"""
    import byte_corpus as C
    bs = K.batches()
    assert [x for _, rows in bs for x in rows if x[0] != "D-len255"] + \
        [x for _, rows in bs for x in rows if x[0] == "D-len255"] == K.topics()
    assert len(bs) >= 3 and sum(1 for name, _ in bs if name.startswith("len255")) >= 2
    for name, rows in bs:
        ts = [t for _, _, t in rows]
        for lead in (0, 5):
            for w in range((len(ts) + 63) // 64):
                assert C.wave_words(ts, lead, w)[0] <= C.TOK_WIN_WORDS, (name, lead, w)
                assert C.wave_levels(ts, w) <= C.TOK_LMAX


# ---- 3. the oracles --------------------------------------------------------------------

def test_o1_and_pytrie_agree_on_every_corpus_topic():
    from oracle import O1, pytrie
    fs = K.filters()
    fb, fo = pack(fs)
    o1 = O1(len(fs))
    o1.insert_many(fb, fo)
    ts = K.topics()
    tb, to = pack([t for _, _, t in ts])
    oc, oo, oi = o1.match_ids(tb, to, threads=4)
    o1.close()
    trie = pytrie.Trie()
    for f in fs:
        trie.insert(f)
    wild = set(K.WILD)
    hit = 0
    for i, (cls, absent, t) in enumerate(ts):
        want = [fs[int(k)] for k in oi[int(oo[i]):int(oo[i + 1])]]
        assert trie.match(t) == want, (cls, t)
        assert want, (cls, t)                                # comparing empty lists proves nothing
        if absent:
            assert set(want) <= wild, (cls, t)
        else:
            hit += bool(set(want) - wild)
    assert hit == sum(1 for _, a, _ in ts if not a)          # every stored word is found by a filter of its own


# ---- 4. the host tables ----------------------------------------------------------------

class _Tables:
    """one host-only engine and the three references, fed together: per
    topic two routes, two plain and one shared subscriber, two share members,
    all derived from the topic's number so that a wrong slot shows"""

    def __init__(self):
        from test_gpu_shared import World
        self.w = World(-1)
        self.num = {}

    def add(self, t):
        w, i = self.w, self.num.setdefault(t, len(self.num))
        for d in ("n%d" % i, ("g1", "n%d" % i)):
            w.route(t, d)
        for s, g in ((10 * i + 1, None), (10 * i + 2, "g1"), (10 * i + 3, None)):
            w.e.sub_add(t, s, g.encode() if g else None)
            w.bag.insert_subscriber(g, t, s)
        w.members(b"g1", t, [100 * i + 1, 100 * i + 2])

    def drop(self, t):
        w, i = self.w, self.num[t]
        for d in ("n%d" % i, ("g1", "n%d" % i)):
            w.route(t, d, add=False)
        for s, g in ((10 * i + 1, None), (10 * i + 2, "g1"), (10 * i + 3, None)):
            assert w.e.sub_del(t, s, g.encode() if g else None) == w.bag.delete_object(g, t, s)
        for m in (100 * i + 1, 100 * i + 2):
            w.member(b"g1", t, m, add=False)

    def check(self, keys, tag):
        w = self.w
        w.e.commit()
        w.e.debug_check_routes()
        w.e.debug_check_subs()
        w.e.debug_check_shares()
        for t in keys:
            assert [r.dest for r in w.r.get_routes(t)] == w.o.get_routes(t), (tag, t)
            want = [("share", x[1].encode(), x[2]) if isinstance(x, tuple) else x for x in w.bag.subscribers(t)]
            assert w.b.subscribers(t) == want, (tag, t)
            assert w.e.share_members(b"g1", t) == w.sh.subscribers(b"g1", t), (tag, t)


@pytest.mark.parametrize("name", E_CLASSES)
def test_host_tables_keep_equal_hash_keys_apart(name):
    for x in K.groups()[name]:
        tb = _Tables()
        keys = list(K.strings(x))                            # the absent one too: it must stay empty
        for t in x.members:
            tb.add(t)
        tb.check(keys, "added")
        assert tb.w.o.get_routes(x.absent) == [] and all(tb.w.o.get_routes(t) for t in x.members)
        for order in itertools.permutations(x.members):      # deletes in every order, each from the full run
            for t in order:
                tb.drop(t)
                tb.check(keys, ("dropped", order, t))
            assert tb.w.e.route_count == 0 and tb.w.e.sub_count == 0 and tb.w.e.share_count == 0
            for t in order:
                tb.add(t)
                tb.check(keys, ("re-added", order, t))
        fill = [b"fill/%d" % i for i in range(24)]           # past the tables' first 16 slots: a regrow
        for t in fill:
            tb.add(t)
        tb.check(keys + fill, "regrown")
        tb.drop(x.members[0])
        tb.check(keys + fill, "regrown, first dropped")
        tb.w.close()
