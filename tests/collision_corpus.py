"""One seeded corpus of forced hash collisions for the two byte-verified
lookups of the device code: the tokenizer's dictionary (kernels.hip dict_end
and wave_dict_end) and the exact-topic table (device_bytes.h exact_find),
shared by tests/test_collision_corpus.py (CPU: the port, the classes, the
oracles, the host tables) and tests/test_gpu_collisions.py (every device entry).

A plain helper module: numpy and the standard library only, fixed seeds.

The hash (image.h, TM_WHASH32 = 1) folds 8-byte chunks with
word_hash_step(h, chunk), which reads h and chunk only as h ^ chunk and is a
bijection of that value (two odd multiplies, two xorshifts).  So for states
s1 != s2 and any chunk c1, the chunk c2 = solve_chunk(s2, step(s1, c1))
(= c1 ^ s1 ^ s2) brings both to one state: words of one length that agree
from there on have the same 64-bit hash.  Classes that cannot use that (the
differing chunk is the last one, or the lengths differ) are searched with
numpy: 24 tag bits + 12 home bits = 36 bits, a birthday over ~2^20 last chunks.

    groups()            {class name: [Group(cls, members, absent)]}
    filters(reverse)    the dictionary workload's filters, in insertion order
    topics()            [(class, is_absent, topic)] of the dictionary workload
    batches()           the same cut into batches whose waves fit the tokenizer's LDS window
    exact_groups()      the E classes' groups (exact-topic keys), flat

A dictionary group's strings share dict_tag and the low 12 hash bits (one
home slot while the dictionary has <= 4096 slots); an exact group's strings
share the length and all 64 hash bits.  `members` are stored (as filters /
table keys), `absent` (bytes or None) collides with them and never is.
"""
import collections

import numpy as np

SEED = 52026
M32 = 0xFFFFFFFF
IV = 0x243F6A8885A308D3
KA, KB = 0x9E3779B1, 0x85EBCA77                  # word_hash_step's multipliers
KA_INV, KB_INV = pow(KA, -1, 1 << 32), pow(KB, -1, 1 << 32)
KLEN, KHI = 0x27D4EB2F, 0x165667B1               # word_hash_final's
MAX_WORDS = 2048                                 # the dictionary grows past 4096 slots at 2,049 words

Group = collections.namedtuple("Group", "cls members absent")

# the filters every topic can match without a dictionary hit (a D-absent
# topic's whole list), and the frame the workload puts around each word
WILD = [b"#", b"+", b"+/+", b"+/#", b"p/+/q", b"+/+/+"]


def strings(g):
    return g.members + ((g.absent,) if g.absent is not None else ())


# ---- the port (python ints) ---------------------------------------------------------

def fmix32(h):
    h ^= h >> 16
    h = h * 0x85EBCA6B & M32
    h ^= h >> 13
    h = h * 0xC2B2AE35 & M32
    h ^= h >> 16
    return h


def word_hash_step(h, chunk):
    a = ((h ^ chunk) & M32) * KA & M32
    b = ((h ^ chunk) >> 32) * KB & M32
    a ^= b >> 15
    b ^= a >> 13
    return b << 32 | a


def word_hash_final(h, n):
    a = fmix32((h & M32) ^ (n * KLEN & M32) ^ ((h >> 32) * KHI & M32))
    b = fmix32((h >> 32) ^ a)
    return (b << 32 | a) or 1


def state_of(bs):
    """the state after folding bs (8-byte little-endian chunks, the last zero padded)"""
    h = IV
    for i in range(0, len(bs), 8):
        h = word_hash_step(h, int.from_bytes(bs[i:i + 8], "little"))
    return h


def word_hash(bs):
    return word_hash_final(state_of(bs), len(bs))


def dict_tag(h, n):
    return (h >> 40) << 8 | min(n, 255)


def key36(h):
    """what two words of one tag length byte must share to meet in the dictionary"""
    return (h >> 40) << 12 | (h & 0xFFF)


def solve_chunk(state, target):
    """the chunk c with word_hash_step(state, c) == target"""
    a, b = target & M32, target >> 32
    b ^= a >> 13
    a ^= b >> 15
    return ((b * KB_INV & M32) << 32 | (a * KA_INV & M32)) ^ state


def first_diff(x, y):
    """the first 8-byte chunk in which x and y differ (None: equal)"""
    for i in range(0, max(len(x), len(y)), 8):
        if x[i:i + 8] != y[i:i + 8]:
            return i // 8
    return None


# ---- the port (numpy, over many last chunks at once) ------------------------------------

def _np_fmix32(h):
    h = h ^ (h >> 16)
    h = h * np.uint32(0x85EBCA6B)
    h = h ^ (h >> 13)
    h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> 16)


def _np_step(state, chunks):
    x = chunks ^ np.uint64(state)
    a = (x & np.uint64(M32)).astype(np.uint32) * np.uint32(KA)
    b = (x >> np.uint64(32)).astype(np.uint32) * np.uint32(KB)
    a = a ^ (b >> 15)
    return a, b ^ (a >> 13)


def np_step(state, chunks):
    """word_hash_step(state, c) (u64 array) for every c of `chunks` (u64 array)"""
    a, b = _np_step(state, chunks)
    return b.astype(np.uint64) << np.uint64(32) | a.astype(np.uint64)


def np_hash_tail(state, chunks, n):
    """word_hash (u64 array) of the n-byte words that reach `state` before
    their last chunk, one per last chunk in `chunks` (u64 array)"""
    a, b = _np_step(state, chunks)
    fa = _np_fmix32(a ^ np.uint32(n * KLEN & M32) ^ (b * np.uint32(KHI)))
    fb = _np_fmix32(b ^ fa)
    r = fb.astype(np.uint64) << np.uint64(32) | fa.astype(np.uint64)
    r[r == 0] = 1
    return r


def _np_key36(h):
    return (h >> np.uint64(40)) << np.uint64(12) | (h & np.uint64(0xFFF))


# ---- bytes ---------------------------------------------------------------------------------

def _clean(a, first):
    """random bytes made fit for a word: no '/', and no '$' as the word's
    first byte (a '$' topic matches no root wildcard: its list would be empty)"""
    a[a == 0x2F] = 0x2E
    if first:
        col = a[:, 0]
        col[col == 0x24] = 0x25
    return a


def _rand(rng, n, first=True):
    return _clean(rng.integers(0, 256, (1, n), dtype=np.uint8), first)[0].tobytes() if n else b""


def _chunks(rng, count, k, first):
    """up to `count` distinct k-byte last chunks: (u64 values, their bytes as (n, k) u8)"""
    pad = np.zeros((count, 8), dtype=np.uint8)
    pad[:, :k] = _clean(rng.integers(0, 256, (count, k), dtype=np.uint8), first)
    v = np.unique(pad.view("<u8").reshape(count))
    return v, v.view(np.uint8).reshape(len(v), 8)[:, :k]


def _repeated(key):
    """the values that occur more than once in `key`, ascending"""
    ks = np.sort(key)
    return np.unique(ks[1:][ks[1:] == ks[:-1]])


def _word_ok(w):
    return b"/" not in w and w not in (b"+", b"#") and w[:1] != b"$"


def _topic_ok(t):
    lv = t.split(b"/")
    return b"+" not in lv and b"#" not in lv          # a publish topic, not a trie filter


# ---- collisions by inversion: all 64 bits ----------------------------------------------------

def _solve(prefixes, tail, rng, ok, want_low4=None):
    """prefixes: distinct byte strings of one length, a multiple of 8 -> the
    strings prefix + chunk + tail with one word_hash: a random chunk after the
    first prefix, the solved one after each other"""
    assert len({len(p) for p in prefixes}) == 1 and len(prefixes[0]) % 8 == 0 and len(set(prefixes)) == len(prefixes)
    st = [state_of(p) for p in prefixes]
    assert len(set(st)) == len(st)
    for _ in range(100000):
        c0 = int.from_bytes(_rand(rng, 8, first=False), "little")
        target = word_hash_step(st[0], c0)
        out = [p + solve_chunk(s, target).to_bytes(8, "little") + tail for p, s in zip(prefixes, st)]
        if want_low4 is not None and word_hash(out[0]) & 15 != want_low4:
            continue
        if all(ok(w) for w in out):
            return out
    raise AssertionError("no solved chunk passed the filter")


def _solve_partial(head, k, n, rng, ok):
    """n strings head + chunk (8 bytes) + last (k < 8 bytes) with one
    word_hash: the solved last chunk c0 ^ s0 ^ si has zero high bytes only
    when the states agree there, so the free 8-byte chunk is searched: 2^18
    of them fall into 2^(8 (8 - k)) <= 2^16 classes of states"""
    assert len(head) % 8 == 0 and 0 < k < 8
    base = state_of(head)
    for _ in range(64):
        v, raw = _chunks(rng, 1 << 18, 8, first=not head)
        top = np_step(base, v) >> np.uint64(8 * k)
        order = np.argsort(top, kind="stable")
        ts = top[order]
        run = np.flatnonzero(ts[n - 1:] == ts[:len(ts) - n + 1])      # n states that agree in the high bytes
        if not len(run):
            continue
        free = [raw[int(order[int(run[0]) + i])].tobytes() for i in range(n)]
        if len(set(free)) < n:
            continue
        s0 = word_hash_step(base, int.from_bytes(free[0], "little"))
        c0 = int.from_bytes(_rand(rng, k, first=False), "little")
        target = word_hash_step(s0, c0)
        out = []
        for f in free:
            c = solve_chunk(word_hash_step(base, int.from_bytes(f, "little")), target)
            assert c >> (8 * k) == 0
            out.append(head + f + c.to_bytes(8, "little")[:k])
        if all(ok(w) for w in out):
            return out
    raise AssertionError("no partial chunk passed the filter")


# ---- collisions by search: tag + home, 36 bits ---------------------------------------------------

def _birthday(prefix, k, rng, need, first):
    """`need` pairs of words prefix + chunk (k bytes, the last chunk) of equal key36"""
    assert len(prefix) % 8 == 0 and 0 < k <= 8
    count, n = 1 << 20, len(prefix) + k                  # 2^40 / 2 pairs of 36-bit keys: about 8 collide
    while True:
        v, raw = _chunks(rng, count, k, first)
        key = _np_key36(np_hash_tail(state_of(prefix), v, n))
        pairs = []
        for val in _repeated(key):
            ws = sorted({raw[i].tobytes() for i in np.flatnonzero(key == val).tolist()})
            if len(ws) >= 2:
                pairs.append((prefix + ws[0], prefix + ws[1]))
        if len(pairs) >= need:
            return pairs[:need]
        count *= 2


def _birthday2(pa, ka, pb, kb, rng, need):
    """`need` pairs (pa + chunk of ka bytes, pb + chunk of kb bytes) of equal
    key36: words of two lengths, both >= 255 (one tag length byte)"""
    count = 1 << 19                                      # 2^38 pairs of 36-bit keys: about 4 collide
    na, nb = len(pa) + ka, len(pb) + kb
    assert min(na, nb) >= 255 and len(pa) % 8 == 0 and len(pb) % 8 == 0
    while True:
        va, ra = _chunks(rng, count, ka, False)
        vb, rb = _chunks(rng, count, kb, False)
        keya = _np_key36(np_hash_tail(state_of(pa), va, na))
        keyb = _np_key36(np_hash_tail(state_of(pb), vb, nb))
        sa = np.sort(keya)
        both = np.unique(keyb[sa[np.minimum(np.searchsorted(sa, keyb), len(sa) - 1)] == keyb])
        if len(both) >= need:
            return [(pa + ra[int(np.flatnonzero(keya == val)[0])].tobytes(),
                     pb + rb[int(np.flatnonzero(keyb == val)[0])].tobytes()) for val in both[:need]]
        count *= 2


def _len_prefix_pair(rng):
    """(w, w + NUL) of 255 and 256 bytes with equal key36.  Both reach one
    state (the zero padded 7-byte chunk is the 8-byte chunk with a NUL), their
    heads agree and the arena is zero padded: between these two only the
    stored exact length decides.  The state is searched in word_hash_final's
    own terms: x = lo ^ hi * KHI gives the low halves a = fmix32(x ^ len * KLEN),
    then y = hi ^ a255 must give high halves that agree in their top 24 bits"""
    l255, l256 = 255 * KLEN & M32, 256 * KLEN & M32
    xs = rng.integers(0, 1 << 32, 1 << 17, dtype=np.uint64).astype(np.uint32)
    a1, a2 = _np_fmix32(xs ^ np.uint32(l255)), _np_fmix32(xs ^ np.uint32(l256))
    for i in np.flatnonzero(((a1 ^ a2) & np.uint32(0xFFF)) == 0).tolist():
        x, p, d = int(xs[i]), int(a1[i]), int(a1[i] ^ a2[i])
        for blk in range(64):
            y = np.arange(blk << 22, (blk + 1) << 22, dtype=np.uint32)
            ok = np.flatnonzero((_np_fmix32(y) ^ _np_fmix32(y ^ np.uint32(d))) >> 8 == 0)
            for j in ok.tolist():
                hi = int(y[j]) ^ p
                target = hi << 32 | (x ^ (hi * KHI & M32))      # the state before word_hash_final
                for _ in range(64):
                    head = _rand(rng, 240)
                    last = _rand(rng, 7, first=False)
                    # the state after chunk 30 that the last chunk takes to `target`
                    mid = solve_chunk(0, target) ^ int.from_bytes(last, "little")
                    w = head + solve_chunk(state_of(head), mid).to_bytes(8, "little") + last
                    if _word_ok(w):
                        assert state_of(w) == target == state_of(w + b"\0")
                        return w, w + b"\0"
    raise AssertionError("no 255 / 256 prefix pair")


# ---- the classes -----------------------------------------------------------------------------------

def _rng(k):
    return np.random.default_rng(SEED + k)


def _differ(rng, head, n, first):
    """n distinct strings head + 8 random bytes"""
    out = []
    while len(out) < n:
        c = head + _rand(rng, 8, first)
        if c not in out:
            out.append(c)
    return out


def _inverted(cls, rng, shapes, ok, count, want_low4=None):
    """`count` groups per shape (equal head bytes, tail bytes): three strings
    that differ in the chunk after the head and collide through the next,
    two stored and the third absent"""
    out = []
    for head_len, tail_len in shapes:
        for _ in range(count):
            head = _rand(rng, head_len)
            ws = _solve(_differ(rng, head, 3, first=not head_len), _rand(rng, tail_len, first=False), rng, ok, want_low4)
            out.append(Group(cls, (ws[0], ws[1]), ws[2]))
    return out


def _searched(cls, rng, shapes, count):
    """`count` stored pairs per shape (equal head bytes, last chunk bytes), and
    after the last shape one pair more of which only the first is stored"""
    out = []
    for head_len, k in shapes:
        extra = (head_len, k) == shapes[-1]
        for pair in _birthday(_rand(rng, head_len), k, rng, count + extra, first=not head_len):
            out.append(Group(cls, pair, None))
    a, b = out.pop().members
    out.append(Group(cls, (a,), b))
    return out


def _build():
    g = collections.OrderedDict()
    # dictionary classes, each named by the branch that must reject its partners
    g["D-head0"] = _searched("D-head0", _rng(1), [(0, 3), (0, 6), (0, 8)], 2)
    g["D-head0-long"] = _inverted("D-head0-long", _rng(2), [(0, 0)], _word_ok, 4)
    g["D-head1"] = _searched("D-head1", _rng(3), [(8, 4), (8, 8)], 2)
    g["D-head1-long"] = _inverted("D-head1-long", _rng(4), [(8, 0), (8, 8)], _word_ok, 2)
    rng = _rng(5)
    g["D-arena"] = _inverted("D-arena", rng, [(16, 0), (24, 0)], _word_ok, 2) + \
        _searched("D-arena", rng, [(16, 5), (24, 5)], 2)
    rng = _rng(6)
    head = _rand(rng, 16)
    p255, p256, p300 = (head + _rand(rng, n - 16, first=False) for n in (248, 248, 296))
    q300 = _rand(rng, 296)
    assert q300[:8] != p256[:8]
    pairs = _birthday2(p255, 7, p256, 8, rng, 3) + _birthday2(p255, 7, p300, 4, rng, 1) + \
        _birthday2(p256, 8, q300, 4, rng, 1)
    # The searched pairs above differ in their last chunk, so the arena compare rejects them too: a lookup
    # without the exact-length test would still pass on them.  Only w / w + NUL fails such a lookup, which
    # is why _len_prefix_pair's search is here.
    g["D-len255"] = [Group("D-len255", p, None) for p in pairs[1:]] + [Group("D-len255", _len_prefix_pair(rng), None)]
    g["D-len255"].append(Group("D-len255", pairs[0][:1], pairs[0][1]))
    # exact-topic classes: one length, all 64 bits; stored members and one absent topic each
    rng = _rng(7)
    g["E-first"] = [Group("E-first", tuple(ws[:2]), ws[2]) for ws in
                    (_solve(_differ(rng, b"", 3, True), b"", rng, _topic_ok) for _ in range(4))]
    g["E-mid"] = [Group("E-mid", tuple(ws[:2]), ws[2]) for n in (8, 16) for ws in
                  (_solve(_differ(rng, _rand(rng, n), 3, False), b"", rng, _topic_ok) for _ in range(2))]
    g["E-partial"] = [Group("E-partial", tuple(ws[:2]), ws[2]) for hl, k, reps in ((0, 7, 2), (0, 6, 1), (8, 7, 1))
                      for ws in (_solve_partial(_rand(rng, hl), k, 3, rng, _topic_ok) for _ in range(reps))]
    g["E-triple"] = [Group("E-triple", tuple(ws[:3]), ws[3]) for n in (0, 16) for ws in
                     (_solve(_differ(rng, _rand(rng, n), 4, not n), b"", rng, _topic_ok) for _ in range(2))]
    g["E-wrap"] = [Group("E-wrap", tuple(ws[:3]), ws[3]) for n in (0, 0, 8, 16) for ws in
                   (_solve(_differ(rng, _rand(rng, n), 4, not n), b"", rng, _topic_ok, want_low4=15),)]
    return g


_CACHE = {}


def groups():
    """the corpus by class (built once per process)"""
    if "g" not in _CACHE:
        _CACHE["g"] = _build()
    return _CACHE["g"]


def dict_groups():
    return [x for name, gs in groups().items() if name.startswith("D-") for x in gs]


def exact_groups():
    return [x for name, gs in groups().items() if name.startswith("E-") for x in gs]


# ---- the dictionary workload -------------------------------------------------------------------------

def filters(reverse=False):
    """WILD, then per group and per frame the partners side by side: W, p/W/q,
    +/W and W/# of every stored word.  reverse: the partners of each group in
    the opposite order, so the other one takes the home slot"""
    fs = list(WILD)
    for g in dict_groups():
        ws = g.members[::-1] if reverse else g.members
        for frame in (b"%s", b"p/%s/q", b"+/%s", b"%s/#"):
            fs += [frame % w for w in ws]
    assert len(set(fs)) == len(fs)
    words = {w for f in fs for w in f.split(b"/")}
    assert len(words) < MAX_WORDS, len(words)
    return fs


def topics():
    """[(class, is_absent, topic)]: W, p/W/q and x/W of every word, stored or
    absent, the partners of a group side by side (one wave tokenizes them)"""
    out = []
    for g in dict_groups():
        for frame in (b"%s", b"p/%s/q", b"x/%s"):
            out += [(g.cls, w == g.absent, frame % w) for w in strings(g)]
    return out


def batches():
    """[(name, [(class, is_absent, topic)])]: topics() in order, the words of
    255 bytes and more two groups to a batch -- a wave of 64 topics whose
    bytes pass the tokenizer's 4 KiB LDS window is tokenized per lane, and
    the wave copy of the lookup would never meet them"""
    ts = topics()
    out = [("short", [x for x in ts if x[0] != "D-len255"])]
    long_ = [x for x in ts if x[0] == "D-len255"]
    per = 2 * 3 * 2                                      # two groups, three frames, two strings
    out += [("len255_%d" % (i // per), long_[i:i + per]) for i in range(0, len(long_), per)]
    return out
