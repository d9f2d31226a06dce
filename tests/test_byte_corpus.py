"""tests/byte_corpus.py on the CPU: (1) the corpus holds every class it
promises, asserted on the packed buffer, so a later edit of the generator
cannot quietly thin it; (2) the two independent oracles (oracle.O1, the C
restatement, and oracle.pytrie, the Python transcription) give the same
ordered list for every corpus topic, so the GPU tests of
tests/test_gpu_bytes.py compare against a reference that two implementations
agree on; (3) nearly every topic has a match (a condition: comparing empty
lists proves nothing); (4) the host's tm_route_of places each exact filter
on its own topic's shard."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import byte_corpus as C  # noqa: E402
from emqx_amd.engine import pack  # noqa: E402


def _levels(buf, off):
    """(topic, start, length) of every level of the packed batch"""
    out = []
    b = buf.tobytes()
    for t in range(len(off) - 1):
        s = int(off[t])
        for w in b[s:int(off[t + 1])].split(b"/"):
            out.append((t, s, len(w)))
            s += len(w) + 1
    return out


@pytest.mark.parametrize("lead", [0, 5])
def test_every_byte_on_both_sides_of_a_slash_at_every_offset(lead):
    buf, off = C.envelope(C.topics(), lead)
    pos = np.flatnonzero(buf == 0x2F)
    pos = pos[(pos >= int(off[0])) & (pos < int(off[-1]))]
    t = np.searchsorted(off, pos, side="right") - 1
    before = pos - 1 >= off[t].astype(np.int64)          # the neighbour lies inside the same topic
    after = pos + 1 < off[t + 1].astype(np.int64)
    seen_b = set(zip(buf[pos[before] - 1].tolist(), (pos[before] % 8).tolist()))
    seen_a = set(zip(buf[pos[after] + 1].tolist(), (pos[after] % 8).tolist()))
    want = {(c, r) for c in range(256) if c != 0x2F for r in range(8)}
    assert not want - seen_b, sorted(want - seen_b)[:8]
    assert not want - seen_a, sorted(want - seen_a)[:8]


@pytest.mark.parametrize("lead", [0, 5])
def test_every_word_length_class_at_every_start_offset(lead):
    buf, off = C.envelope(C.topics(), lead)
    lv = _levels(buf, off)
    seen = {(n, s % 8) for _, s, n in lv}
    want = {(n, r) for n in C.WORD_LENGTHS for r in range(8)}
    assert not want - seen, sorted(want - seen)[:8]
    # ... and as a topic's first word, and as a whole single-level topic
    first = {(int(off[t + 1] - off[t]), int(off[t]) % 8) for t in range(len(off) - 1)
             if 0x2F not in buf[int(off[t]):int(off[t + 1])]}
    assert not want - first, sorted(want - first)[:8]


def test_stratified_subset_keeps_every_length_and_alignment():
    sub = C.stratified()
    assert 1000 <= len(sub) <= 1700
    buf, off = pack(sub)
    whole = {(int(off[t + 1] - off[t]), int(off[t]) % 8) for t in range(len(sub)) if b"/" not in sub[t]}
    want = {(n, r) for n in C.WORD_LENGTHS for r in range(8)}
    assert not want - whole, sorted(want - whole)[:8]
    sl = {int(off[t]) % 8 for t in range(len(sub)) if b"/" in sub[t]}
    assert sl == set(range(8))
    assert C.long_level() in sub and C.deep_topic() in sub
    assert set(sub) <= set(C.topics())
    for n in C.NUL_LENGTHS:
        assert any(len(w) == n and w + b"\0" in sub and w[:-1] + b"\0" in sub for w in sub), n


def test_corpus_size_alphabet_and_shapes():
    ts = C.topics()
    assert ts == C.topics(C.SEED) and ts != C.topics(C.SEED + 1)        # seeded, deterministic
    assert 5500 <= len(ts) <= 6500 and sum(len(t) for t in ts) < 1_000_000
    words = [w for t in ts[:-2] for w in t.split(b"/")]
    wset = set(words)
    # the dense alphabet, mixed with random bytes and with plain ASCII inside words
    for c in C.DENSE:
        assert sum(1 for w in words if c in w) >= 200, hex(c)
    dense = set(C.DENSE)
    assert sum(1 for w in words if len(w) >= 8 and set(w) & dense and set(w) - dense) >= 500
    assert sum(1 for w in words if len(w) >= 8 and any(c >= 0x80 for c in w)) >= 500
    assert sum(1 for w in words if len(w) >= 8 and set(w) <= set(C.ASCII)) >= 200
    # trailing-NUL siblings, as whole topics and as inner levels
    for n in C.NUL_LENGTHS:
        sib = [w for w in wset if len(w) == n and w[-1:] != b"\0" and w + b"\0" in wset and w[:-1] + b"\0" in wset]
        assert sib, n
        assert any(w in ts and w + b"\0" in ts and w[:-1] + b"\0" in ts for w in sib), n
        assert any(b"x/" + w + b"/y" in ts and b"x/" + w + b"\0/y" in ts for w in sib), n
    # the shapes of the tokenizer test
    for t in [b"", b"/", b"//", b"a//b", b"a/", b"/a", b"$SYS/x/y", b"$", b"$a/+/#", b"+", b"#", b"a/+/b", b"a/#",
              b"+/+", b"/./", b"a/.b/..c/...", b"./."]:
        assert t in ts, t
    for t in C.REGRESSIONS:
        assert t in ts, t
    counts = {t.count(b"/") + 1 for t in ts}
    assert set(C.LEVEL_COUNTS) <= counts
    for n in C.LEVEL_COUNTS[2:]:
        same = [t.split(b"/") for t in ts if t.count(b"/") + 1 == n]
        assert any(lv[0] == b"" for lv in same) and any(lv[-1] == b"" for lv in same), n
        assert any(b"" in lv[1:-1] for lv in same) and any(lv[0][:1] == b"$" for lv in same), n
        assert any(b"+" in lv for lv in same) and any(b"#" in lv for lv in same), n


def test_the_two_giants():
    ts = C.topics()
    long = [t for t in ts if len(t) == C.LONG_LEVEL]
    assert C.LONG_LEVEL == 65535 and len(long) == 1 and b"/" not in long[0] and long[0] == C.long_level()
    assert len(set(long[0])) > 200                        # mixed bytes, not a run of one
    deep = [t for t in ts if t.count(b"/") + 1 == C.DEEP_LEVELS]
    assert C.DEEP_LEVELS == 2000 and len(deep) == 1 and all(len(w) == 1 for w in deep[0].split(b"/"))
    assert max(t.count(b"/") + 1 for t in ts) == C.DEEP_LEVELS


def test_filters_are_valid_and_name_every_topic():
    ts = C.all_topics()
    fs = C.filters(ts)
    fset = set(fs)
    assert fs == sorted(fset)
    assert all(b"#" not in f.split(b"/")[:-1] for f in fs)
    assert {b"#", b"+", b"+/#", b"+/+"} <= fset
    for t in ts:
        lv = t.split(b"/")
        if b"#" not in lv[:-1]:
            assert t in fset, t
            assert b"/".join([b"+"] + lv[1:]) in fset, t
            assert lv[0] == b"#" or b"/".join(lv[:1] + [b"#"]) in fset, t
            if len(lv) > 2:
                assert b"/".join(lv[:2] + [b"+"] + lv[3:]) in fset, t
    invalid = [t for t in ts if b"#" in t.split(b"/")[:-1]]
    assert 0 < len(invalid) < len(ts) // 20               # topics stay unrestricted; few lose their exact filter


def test_wave_batches_sit_on_the_tokenizer_limits():
    assert C.TOK_WIN_WORDS == 512 and C.TOK_LMAX == 1000   # kernels.hip TOK_WIN_WORDS, TOK_LMAX
    src = open(os.path.join(ROOT, "emqx_amd", "csrc", "kernels.hip")).read()
    assert "TOK_WIN_WORDS = %d;" % C.TOK_WIN_WORDS in src and "TOK_LMAX = %d;" % C.TOK_LMAX in src
    wb = {name: (lead, ts) for name, lead, ts in C.wave_batches()}
    # the byte window: exact fit and one word over, from offsets 0 and 5 mod 8, all four
    # waves inside one 256-thread block (waves 0-3), fit next to over
    lead, ts = wb["window_lead0"]
    assert lead == 0 and len(ts) == 256
    assert [C.wave_words(ts, 0, w) for w in range(4)] == [(512, 0), (513, 0), (512, 5), (513, 5)]
    lead, ts = wb["window_lead5"]
    assert lead == 5 and len(ts) == 256
    assert [C.wave_words(ts, 5, w) for w in range(4)] == [(512, 5), (513, 5), (512, 0), (513, 0)]
    for name in ("window_lead0", "window_lead5"):          # the level list is not what sends these per lane
        assert all(C.wave_levels(wb[name][1], w) <= C.TOK_LMAX for w in range(4))
    # wave_words is the kernel's own arithmetic on the envelope's offsets
    for name in ("window_lead0", "window_lead5"):
        lead, ts = wb[name]
        buf, off = C.envelope(ts, lead)
        for w in range(4):
            wbase = int(off[64 * w]) & ~7
            assert ((int(off[64 * w + 64]) - wbase + 7) >> 3, int(off[64 * w]) % 8) == C.wave_words(ts, lead, w)
    # the level list: exactly 1,000 and 1,001 levels, both inside the byte window
    lead, ts = wb["levels"]
    assert lead == 0 and len(ts) == 256
    assert [C.wave_levels(ts, w) for w in range(2)] == [1000, 1001]
    for ld in (0, 5):
        assert all(C.wave_words(ts, ld, w)[0] <= C.TOK_WIN_WORDS for w in range(2))
    # one topic past 4 KiB among 63 short ones; an empty wave
    big = [t for t in ts[128:192] if len(t) > 4096]
    assert len(big) == 1 and all(len(t) <= 16 for t in ts[128:192] if t is not big[0])
    assert ts[192:] == [b""] * 64
    # partial last waves, of topics that fit the window (so the wave path takes them)
    assert sorted(len(wb[k][1]) for k in wb if k.startswith("partial_")) == [1, 63, 64, 65, 257]
    for k in wb:
        if k.startswith("partial_"):
            ts = wb[k][1]
            for w in range((len(ts) + 63) // 64):
                assert C.wave_words(ts, 0, w)[0] <= C.TOK_WIN_WORDS and C.wave_words(ts, 5, w)[0] <= C.TOK_WIN_WORDS
                assert C.wave_levels(ts, w) <= C.TOK_LMAX


@pytest.mark.parametrize("lead", [0, 5])
def test_envelope_surrounds_the_topics_with_slashes(lead):
    ts = C.topics()[:300] + [b""]
    buf, off = C.envelope(ts, lead)
    assert int(off[0]) == lead and len(off) == len(ts) + 1
    assert bytes(buf[:lead]) == b"/" * lead
    assert len(buf) - int(off[-1]) >= 16 and bytes(buf[int(off[-1]):]) == b"/" * (len(buf) - int(off[-1]))
    b = buf.tobytes()
    assert [b[int(off[i]):int(off[i + 1])] for i in range(len(ts))] == ts
    buf0, off0 = C.envelope([], lead)
    assert list(off0) == [lead] and bytes(buf0) == b"/" * (lead + 16)


# ---- the oracles on these bytes ---------------------------------------------------

@pytest.fixture(scope="module")
def o1_lists():
    """O1's ordered lists (as filter bytes) of the corpus and the wave batches"""
    from oracle import O1
    ts = C.all_topics()
    fs = C.filters(ts)
    fb, fo = pack(fs)
    o1 = O1(len(fs))
    o1.insert_many(fb, fo)
    tb, to = pack(ts)
    oc, oo, oi = o1.match_ids(tb, to, threads=8)
    o1.close()
    return ts, fs, oc, oo, oi


def test_o1_and_pytrie_agree_on_every_topic(o1_lists):
    from oracle import pytrie
    ts, fs, oc, oo, oi = o1_lists
    trie = pytrie.Trie()
    for f in fs:
        trie.insert(f)
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 3 * C.DEEP_LEVELS + 1000))   # match_node/3 recurses once per level
    try:
        done = {}
        for t, topic in enumerate(ts):
            if topic not in done:
                done[topic] = trie.match(topic)
            want = [fs[int(i)] for i in oi[int(oo[t]):int(oo[t + 1])]]
            assert done[topic] == want, "topic %d %r" % (t, topic[:80])
    finally:
        sys.setrecursionlimit(old)


def test_nearly_every_topic_has_a_match(o1_lists):
    ts, fs, oc, oo, oi = o1_lists
    n = len(C.topics())
    assert (oc[:n] > 0).mean() >= 0.95
    assert (oc > 0).mean() >= 0.95
    # and its own exact filter is among them
    fid = {f: i for i, f in enumerate(fs)}
    for t, topic in enumerate(ts):
        if C.valid_filter(topic):
            assert fid[topic] in oi[int(oo[t]):int(oo[t + 1])], topic[:80]


@pytest.mark.parametrize("S,depth", [(2, 1), (3, 2), (64, 2)])
def test_host_route_of_places_a_filter_with_its_topic(S, depth):
    from emqx_amd import shard
    owners = set()
    for t in C.topics():
        own = shard.topic_route(t, S, depth)
        assert 0 <= own < S
        owners.add(own)
        if C.valid_filter(t):
            f = shard.filter_route(t, S, depth)
            lv = t.split(b"/")[:depth]
            if b"+" in lv or b"#" in lv:
                assert f == -1, t[:80]
            else:
                assert f == own, t[:80]
        # the key is the first `depth` levels: a topic that shares them shares the owner
        assert shard.topic_route(b"/".join(t.split(b"/")[:depth]) + b"/zz", S, depth) == own or \
            t.count(b"/") + 1 < depth, t[:80]
    assert len(owners) >= min(S, 2)


def test_host_topic_algebra_agrees_with_pytrie_on_these_bytes():
    """tm_topic_match / tm_topic_wildcard (the host C of emqx_topic:match/2 and
    wildcard/1) against the Python transcription, each topic against its own
    filters and against its neighbour's (mostly non-matching) ones"""
    from emqx_amd import emqx_topic as T
    from oracle import pytrie
    sec = C.sections()
    ts = list(sec["slash"][::4] + sec["length"] + sec["fixed"] + sec["nul"] + sec["levels"] + sec["random"][::4])
    ts.append(C.long_level())
    prev = [b"#"]
    hits = 0
    for t in ts:
        mine = C.filters([t])
        for f in mine + prev:
            want = pytrie.match(t, f)
            assert T.match(t, f) == want, (t[:80], f[:80])
            hits += want
        assert T.wildcard(t) == pytrie.wildcard(t), t[:80]
        prev = mine[:6]
    assert hits > 4 * len(ts)
