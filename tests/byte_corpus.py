"""One seeded corpus hostile to the byte code of the device paths that read
topic bytes (the SWAR chunk loaders, '/' scans, word hashes and byte-verifies
of kernels.hip, routes.hip, dispatch.hip and route.hip), shared by
tests/test_byte_corpus.py (CPU: coverage and oracle agreement) and
tests/test_gpu_bytes.py (every device entry against the CPU oracles).

A plain helper module: no fixtures, fixed seeds, nothing from time or the
environment.  The reference validates no bytes on the publish path, so every
byte pattern is in the domain of a topic; filters keep to what
emqx_topic:validate/2 lets reach the trie ('#' only as the last level).

    topics(seed)        ~6,000 ordered topics (their order fixes every byte's
                        absolute offset once packed; do not shuffle)
    filters(topics)     each topic's exact text, its one-'+' variants, its
                        <first word>/#, and '#', '+', '+/#', '+/+'
    wave_batches()      ordered batches on the limits tm_tokenize branches on
    envelope(ts, lead)  pack with off[0] = lead and '/' all around
"""
import random

import numpy as np

# kernels.hip: the LDS byte window of one wave (8-byte words) and the wave's
# level list; a wave past either takes the per-lane path
TOK_WIN_WORDS = 512
TOK_LMAX = 1000

SEED = 20260

# 0x2E = '/' ^ 0x01 and 0x30 = '/' + 1 defeat borrow-based zero-byte tests;
# 0xAF = '/' | 0x80 defeats a test that masks the top bit; 0x00 / 0xFF are the
# padding and the saturated byte; 0x80 the lone top bit
DENSE = bytes([0x00, 0x01, ord("#"), ord("$"), ord("+"), 0x2E, 0x30, 0x7F, 0x80, 0xAF, 0xFF])
ASCII = b"abcdefghijklmnopqrstuvwxyz0123456789_-"
# the edges of a dictionary slot (first half <= 8, second half <= 16, arena
# beyond), of the 8-byte chunks, and of dict_tag's length byte (capped at 255)
WORD_LENGTHS = [0, 1, 2, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 63, 64, 65, 254, 255, 256, 257]
NUL_LENGTHS = [1, 7, 8, 15, 16, 254, 255, 256]
LEVEL_COUNTS = [1, 2, 3, 8, 15, 16, 17, 31, 32, 33, 64]
LONG_LEVEL = 65535      # topicmatch.h states no limit on a level: MQTT's topic limit
DEEP_LEVELS = 2000

# the shapes of tests/test_gpu_tokenize.py
FIXED = [b"", b"/", b"//", b"a//b", b"a/", b"/a", b"$SYS/x/y", b"$", b"$a/+/#", b"+", b"#", b"a/+/b", b"a/#",
         b"+/+", b"/./", b"a/.b/..c/...", b"./.", b"///", b"$/", b"/$", b"$SYS", b"+/x", b"x/+", b"x/#",
         b"+x/x+", b"#x/x#", b"a/b/c/", b"/a/b/c"]
# minimal reproducers of bugs this corpus found, kept as named cases (none so far)
REGRESSIONS = []


def _noslash(bs):
    return bytes(0x2E if c == 0x2F else c for c in bs)


def _word(rng, n, kind):
    """n bytes without '/': kind 0 the dense alphabet, 1 uniform random bytes,
    2 plain ASCII, 3 a mix of all three"""
    if kind == 0:
        return bytes(rng.choice(DENSE) for _ in range(n))
    if kind == 1:
        return _noslash(rng.randbytes(n))
    if kind == 2:
        return bytes(rng.choice(ASCII) for _ in range(n))
    return bytes(rng.choice(DENSE) if rng.random() < 0.4 else rng.choice(ASCII) if rng.random() < 0.5
                 else _noslash(rng.randbytes(1))[0] for _ in range(n))


class _Builder:
    """appends topics while tracking the absolute offset each will have once
    packed from offset 0"""

    def __init__(self):
        self.out = []
        self.pos = 0

    def add(self, t):
        self.out.append(t)
        self.pos += len(t)

    def align(self, r):
        """a filler topic so that the next topic starts at offset r mod 8"""
        k = (r - self.pos) % 8
        if k:
            self.add(b"f" * k)


def slash_topics():
    """every byte value but '/' directly before and directly after a '/', the
    '/' at each absolute offset mod 8 (topics packed from offset 0 in order)"""
    b = _Builder()
    for r in range(8):
        for c in range(256):
            if c == 0x2F:
                continue
            k = (r - b.pos - 1) % 8          # pad so that the '/' lands on r
            b.add(b"p" * k + bytes([c]) + b"/" + bytes([c]) + b"q" * (c & 1))
    return b.out


def length_topics(rng):
    """a word of every length class starting at each absolute offset mod 8:
    inside a topic (after a pad word and a '/'), as a topic's first word, and
    as a whole single-level topic; dense, random and ASCII bytes in turn"""
    b = _Builder()
    for n in WORD_LENGTHS:
        for r in range(8):
            kind = (n + r) % 3
            w = _word(rng, n, kind)
            k = (r - b.pos - 1) % 8
            b.add(b"p" * k + b"/" + w + (b"/t" if r & 1 else b""))
            assert (b.pos - len(b.out[-1]) + k + 1) % 8 == r
            b.align(r)
            b.add(_word(rng, n, (kind + 1) % 3) + b"/" + _word(rng, r, 3))
            b.align(r)
            b.add(_word(rng, n, (kind + 2) % 3))
    return b.out


def nul_topics(rng):
    """w, w + NUL and w[:-1] + NUL: heads and the arena are zero padded, so
    only the length tells them apart"""
    out = []
    for n in NUL_LENGTHS:
        for kind in (2, 3):
            w = _word(rng, n - 1, kind) + b"w"
            sib = [w, w + b"\0", w[:-1] + b"\0", w + b"\0\0"]
            out += sib
            out += [b"x/" + s + b"/y" for s in sib]
            out += [s + b"/" + s[::-1] for s in sib]
    out += [b"\0", b"\0\0", b"\0/\0", b"\0/", b"/\0", b"\0" * 8, b"\0" * 9, b"\0" * 16, b"\0" * 17]
    return out


def level_topics(rng):
    """the level counts around WREG (16) and the key words (32, 64), with
    empty levels at the start, middle and end, '$' first words and the atoms"""
    words = [b"", b".", b"a", b"ab", b"abcdefg", b"abcdefgh", b"abcdefghi", b"0123456789abcdef",
             b"0123456789abcdefg", b"\x00", b"\x2e", b"\xff", b"\x80\xaf", b"+", b"#", b"$x", b"+x", b"x#"]
    out = []
    for n in LEVEL_COUNTS:
        for rep in range(6):
            lv = [rng.choice(words) for _ in range(n)]
            if rep == 1:
                lv[0] = b""
            if rep == 2:
                lv[-1] = b""
            if rep == 3:
                lv[n // 2] = b""
            if rep == 4:
                lv[0] = b"$" + lv[0]
            if rep == 5:
                lv = [rng.choice([b"+", b"#", b"a"]) for _ in range(n)]
            out.append(b"/".join(lv))
        out.append(b"/".join([b""] * n))
    return out


def random_topics(rng, k):
    """1-24 levels of words drawn from a shared vocabulary (so filters of one
    topic meet words of others) of every length class up to 65"""
    vocab = [_word(rng, n, rng.randrange(4)) for n in WORD_LENGTHS[:18] for _ in range(12)]
    vocab += [b"", b"", b"+", b"#", b"$", b"$SYS"]
    out = []
    for _ in range(k):
        n = rng.choice([1, 2, 3, 3, 4, 5, 8, 8, 12, 16, 17, 24])
        out.append(b"/".join(rng.choice(vocab) for _ in range(n)))
    return out


def long_level(seed=SEED):
    """one level of the longest length (mixed bytes, no '/')"""
    return _word(random.Random(seed + 1), LONG_LEVEL, 3)


def deep_topic(seed=SEED):
    rng = random.Random(seed + 2)
    return b"/".join(bytes([rng.choice(b"abc")]) for _ in range(DEEP_LEVELS))


_CACHE = {}


def sections(seed=SEED):
    """the corpus by class, in corpus order: the '/'-neighbour topics first
    (their offsets are absolute), then the length classes (self-aligning from
    an offset 0 mod 8), the rest, and the two giants last"""
    if seed not in _CACHE:
        rng = random.Random(seed)
        b = _Builder()
        for t in slash_topics():
            b.add(t)
        b.align(0)
        sec = [("slash", tuple(b.out)),
               ("length", tuple(length_topics(rng))),
               ("fixed", tuple(FIXED + REGRESSIONS)),
               ("nul", tuple(nul_topics(rng))),
               ("levels", tuple(level_topics(rng)))]
        have = sum(len(ts) for _, ts in sec)
        sec.append(("random", tuple(random_topics(rng, 6000 - have - 2))))
        sec.append(("giant", (long_level(seed), deep_topic(seed))))
        _CACHE[seed] = tuple(sec)
    return dict(_CACHE[seed])


def topics(seed=SEED):
    """the corpus, in its fixed order"""
    return [t for ts in sections(seed).values() for t in ts]


def valid_filter(f):
    """'#' only as the last level (emqx_topic:validate/2 runs before the trie)"""
    return b"#" not in f.split(b"/")[:-1]


def filters(ts):
    fs = set()
    for t in ts:
        lv = t.split(b"/")
        fs.add(t)
        for i in range(min(len(lv), 3)):
            fs.add(b"/".join(lv[:i] + [b"+"] + lv[i + 1:]))
        fs.add(b"/".join(lv[:1] + [b"#"]))
    fs.update([b"#", b"+", b"+/#", b"+/+"])
    return sorted(f for f in fs if valid_filter(f))


def stratified(seed=SEED, k=1500):
    """about k corpus topics in which every class survives: the length
    classes first and whole (packed from offset 0 they keep every length at
    every start offset mod 8), every 12th '/'-neighbour topic (all eight
    offsets), the fixed, NUL-sibling and level-count topics, the giants, and
    random ones up to k"""
    sec = sections(seed)
    out = list(sec["length"])          # whole and in order, repeats (the fillers, the empty word) included
    pick = list(sec["slash"][::12]) + list(sec["fixed"]) + list(sec["nul"]) + list(sec["levels"]) + \
        list(sec["giant"])
    rnd = sec["random"]
    pick += rnd[::max(1, len(rnd) // max(1, k - len(out) - len(pick)))]
    seen = set(out)
    for t in pick:
        if t not in seen:
            seen.add(t)
            out.append(t)
    return out


# ---- batches on the tokenizer's limits ------------------------------------------

def wave_words(ts, lead, w):
    """8-byte words tm_tokenize stages for wave w of the packed batch: from
    off[64 w] & ~7 to off[min(64 w + 64, n)]"""
    off = lead + np.concatenate([[0], np.cumsum([len(t) for t in ts])])
    t0, t1 = 64 * w, min(64 * w + 64, len(ts))
    return int(off[t1] - (off[t0] & ~7) + 7) >> 3, int(off[t0] % 8)


def wave_levels(ts, w):
    return sum(t.count(b"/") + 1 for t in ts[64 * w:64 * w + 64])


def _wave_of_bytes(rng, total):
    """64 topics of `total` bytes in all, 2-4 levels each"""
    lens = [total // 64] * 64
    for i in range(total - sum(lens)):
        lens[i] += 1
    out = []
    for n in lens:
        w = bytearray(_word(rng, n, 3))
        for p in rng.sample(range(n), min(n, rng.randrange(1, 4))):
            w[p] = 0x2F
        out.append(bytes(w))
    assert sum(len(t) for t in out) == total
    return out


def window_batch(lead):
    """256 topics = one block of tm_tokenize, for a buffer whose off[0] = lead
    (0 or 5): two waves that start at lead mod 8, the first filling exactly
    TOK_WIN_WORDS (512) words and the second 513, then two waves that start
    at the other of 0 / 5 mod 8, filling 512 and 513"""
    rng = random.Random(SEED + 10 + lead)
    W = 8 * TOK_WIN_WORDS
    # lead 0: [0, 4096) 512 words; 4101 bytes from 0: 513, ends at 5; 5 + 4088 = 4093: 512, ends at 5;
    #         5 + 4092 = 4097: 513
    # lead 5: 5 + 4088 = 4093: 512, ends at 5; 5 + 4099 = 4104: 513, ends at 0; 4096: 512; 4101: 513
    sizes = {0: [W, W + 5, W - 8, W - 4], 5: [W - 8, W + 3, W, W + 5]}[lead]
    return [t for total in sizes for t in _wave_of_bytes(rng, total)]


def level_batch():
    """256 topics = one block: wave 0 totals exactly TOK_LMAX (1000) levels,
    wave 1 totals 1001 (both fit the byte window), wave 2 holds one topic
    longer than 4 KiB among 63 short ones, wave 3 is 64 empty topics"""
    rng = random.Random(SEED + 30)

    def lv(n):
        return b"/".join(bytes([rng.choice(b"ab\x00\xff.")]) for _ in range(n))
    w0 = [lv(16) for _ in range(40)] + [lv(15) for _ in range(24)]          # 640 + 360
    w1 = [lv(16) for _ in range(41)] + [lv(15) for _ in range(23)]          # 656 + 345
    rng.shuffle(w0)
    rng.shuffle(w1)
    big = b"/".join(_word(rng, n, 3) for n in (1500, 0, 9, 2600, 17))
    w2 = [_word(rng, 5, 2) + b"/" + _word(rng, 3, 0) for _ in range(64)]
    w2[37] = big
    return w0 + w1 + w2 + [b""] * 64


def wave_batches():
    """[(name, lead the batch is built for, ordered topics)]: wave w of a
    batch is topics [64 w, 64 w + 64); callers must not shuffle"""
    rng = random.Random(SEED + 40)
    short = [t for t in random_topics(rng, 2000) if len(t) <= 40][:257]   # (waves that fit the byte window)
    assert len(short) == 257
    out = [("window_lead0", 0, window_batch(0)),
           ("window_lead5", 5, window_batch(5)),
           ("levels", 0, level_batch())]
    for n in (1, 63, 64, 65, 257):
        out.append(("partial_%d" % n, 0, short[:n]))
    return out


def all_topics(seed=SEED):
    """the corpus and every wave batch's topics: what the filter set is built over"""
    out = topics(seed)
    for _, _, ts in wave_batches():
        out += ts
    return out


def envelope(ts, lead):
    """(bytes u8, offsets u64) with off[0] = lead: the lead bytes before the
    first topic and 16 bytes after the last are all '/', so a kernel that
    takes one byte outside [off[t], off[t+1]) as content miscounts levels"""
    body = b"".join(ts)
    buf = np.frombuffer(b"/" * lead + body + b"/" * 16, dtype=np.uint8)
    off = np.zeros(len(ts) + 1, dtype=np.uint64)
    off[0] = lead
    if ts:
        off[1:] = lead + np.cumsum([len(t) for t in ts], dtype=np.uint64)
    return buf, off
