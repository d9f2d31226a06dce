"""tests/acl_corpus.py on the CPU: the cases hold every class they promise,
asserted on the oracles (oracle/pyacl.py, oracle/pytrie.py) alone, so a later
edit of the generator cannot quietly thin what tests/test_gpu_acl_edges.py and
tests/test_gpu_rewrite_bytes.py compare on the device; and the status codes
of the ACL builder and of tm_acl_check_batch's argument checks on a host-only
handle (they run before the device check, so no GPU is needed)."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import acl_corpus as A  # noqa: E402
import byte_corpus as C  # noqa: E402
from emqx_amd import _lib  # noqa: E402
from emqx_amd.emqx_access import WHO, AclRules  # noqa: E402
from oracle import pyacl, pytrie  # noqa: E402


# ---- who terms ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def who_cases():
    return A.who_shapes()


def _match(case, cred):
    return pyacl.match_who(A.oracle_cred(cred), pyacl.compile_who(case.who))


def test_who_cases_state_their_own_peak(who_cases):
    names = [c.name for c in who_cases]
    assert len(set(names)) == len(names)
    for c in who_cases:
        assert c.peak == A.peak_live(c.who), c.name
        assert c.peak <= A.STACK_MAX, c.name
    # the helper's count on terms worked by hand
    T = ("client", b"c1")
    assert A.peak_live("all") == 1 and A.peak_live(("and", [])) == 1 and A.peak_live(("or", [T])) == 1
    assert A.peak_live(("and", [T] * 16 + [("and", [T] * 17)])) == 33
    assert A.peak_live(("and", [("or", [T] * 8)] + [T] * 30)) == 31
    assert A.peak_live(("and", [T, ("or", [T, ("and", [T, T])]), T])) == 4
    assert A.stack_trace(("and", [T, ("or", [T, T]), T]))[1] == [3, 2, 1, 1]


def test_who_cases_cover_the_widths_and_peaks(who_cases):
    by = {c.name: c for c in who_cases}
    for op in ("and", "or"):
        for w in (0, 1, 2, 31, A.STACK_MAX):
            assert "flat_%s_%d/all_true" % (op, w) in by and "flat_%s_%d/all_false" % (op, w) in by
    for kind in ("tail_", "tail3_", "head_"):
        peaks = {c.peak for c in who_cases if c.name.startswith(kind)}
        assert {31, 32, 33, 40, 64} <= peaks, (kind, peaks)
    assert A.STACK_MAX == 64                                   # the documented limit is one of the peaks
    src = open(os.path.join(ROOT, "include", "topicmatch.h")).read()
    assert "#define TM_ACL_WHO_STACK_MAX %du" % A.STACK_MAX in src and _lib.TM_ACL_WHO_STACK_MAX == A.STACK_MAX
    # the terms of the issue's table: three past a 32-entry stack, one that still fits it
    assert [by[n].peak for n in ("table/and_T16_and_T17", "table/and_T20_or_T20", "table/or_T_F19_and_T19_F",
                                 "table/and_T16_and_T16")] == [33, 40, 40, 32]
    for n in ("table/and_T16_and_T17", "table/and_T20_or_T20", "table/or_T_F19_and_T19_F", "table/and_T16_and_T16"):
        assert _match(by[n], A.FULL) is True, n
    for name, _, _ in A.WHO_REGRESSIONS:
        assert name in by


def test_who_cases_truth_values(who_cases):
    seen = {}
    for c in who_cases:
        for cred in c.creds:
            seen.setdefault(c.peak, set()).add(_match(c, cred))
    assert all(v == {True, False} for v in seen.values()), seen       # both answers at every peak
    by = {c.name: c for c in who_cases}
    for c in who_cases:
        shape, _, tag = c.name.partition("/")
        if tag == "all_true" and c.peak > 1:
            assert _match(c, A.FULL) is True, c.name
        if tag == "all_false" and c.peak > 1:
            assert _match(c, A.FULL) is False, c.name
        if tag.endswith("_decides_true"):                              # one leaf's value is the term's value
            other = by[c.name[:-len("true")] + "false"]
            assert _match(c, A.FULL) is True and _match(other, A.FULL) is False, c.name
            flipped = sum(1 for x, y in zip(_leaves(c.who), _leaves(other.who)) if (x in A._TRUE) != (y in A._TRUE))
            assert flipped == 1, c.name
    # the deciding leaf sits first, last and 31 / 32 / 33 deep wherever the shape is that deep
    for name, shape in A._shapes():
        n = A._shape_leaves(shape)
        _, deepest = A.stack_trace(A._fill(shape, [True] * n))
        for place in (31, 32, 33):
            assert (place in deepest) == ("%s/place%d_decides_true" % (name, place) in by), (name, place)
        assert (n > 0) == ("%s/first_decides_false" % name in by) == ("%s/last_decides_true" % name in by)
    deep = [c for c in who_cases if "/place33_" in c.name]
    assert len(deep) >= 20 and any(c.name.startswith("head_") for c in deep)


def _leaves(who):
    if A._is_group(who):
        return [x for c in who[1] for x in _leaves(c)]
    return [who]


def test_who_leaves_are_of_every_kind(who_cases):
    kinds = set()
    for c in who_cases:
        for leaf in _leaves(c.who):
            kinds.add(leaf if leaf == "all" else leaf[0] + ("_all" if leaf[1] == "all" else ""))
    assert kinds == {"all", "client", "user", "client_all", "user_all", "ipaddr"}


# ---- CIDRs ------------------------------------------------------------------------------

def _cidr_expected(text, cred):
    return pyacl.match_who(A.oracle_cred(cred), pyacl.compile_who(("ipaddr", text)))


def test_cidr_cases_cover_every_prefix_both_ways():
    cases = A.cidr_cases()
    assert len({n for n, _, _ in cases}) == len(cases)
    for ver, prefixes in ((4, A.V4_PREFIXES), (6, A.V6_PREFIXES)):
        assert prefixes[0] == 0 and prefixes[-1] == (32 if ver == 4 else 128)
        for p in prefixes:
            mine = [(n, t, c) for n, t, c in cases if n.startswith("v%d/%d/" % (ver, p))]
            got = {n.rsplit("/", 1)[1]: _cidr_expected(t, c) for n, t, c in mine}
            text = mine[0][1]
            net = ipaddress_network(text)
            if p < net.max_prefixlen:                                  # the text's host bits are set
                assert int(ipaddress_address(text.split("/")[0])) != int(net.network_address), text
            if p == 0:
                assert got == {"start": True, "end": True}, (ver, p, got)     # nothing of the family lies outside
            else:
                assert got["start"] is True and got["end"] is True, (ver, p, got)
                assert False in got.values() and all(got[k] is False for k in got if k in ("below", "above")), got
    want = {n: _cidr_expected(t, c) for n, t, c in cases}
    assert want["zero/v4_any"] and want["zero/v4_top"] and want["zero/v6_any"] and want["zero/v6_top"]
    assert not any(v for n, v in want.items() if n.startswith("family/") and n != "family/v6_mapped_rule_mapped_peer")
    assert want["family/v6_mapped_rule_mapped_peer"]
    assert not any(v for n, v in want.items() if n.startswith("nopeer/"))
    assert sum(1 for n in want if n.startswith("nopeer/")) == 8
    assert want["host/v4_same"] and want["host/v6_same"]
    assert not any(v for n, v in want.items() if n.startswith("host/") and not n.endswith("_same"))
    for name, _, _ in A.CIDR_REGRESSIONS:
        assert want[name] is True


def ipaddress_network(text):
    import ipaddress
    return ipaddress.ip_network(text, strict=False)


def ipaddress_address(text):
    import ipaddress
    return ipaddress.ip_address(text)


# ---- the thinned byte corpus ------------------------------------------------------------------

def test_subset_keeps_the_classes():
    sub = A.subset()
    assert sub == A.subset() and set(sub) <= set(C.topics()) and len(sub) == len(set(sub))
    assert 340 <= len(sub) <= 400                              # the module docstring states 372
    before, after = set(), set()
    for t in sub[:-2]:
        for i, c in enumerate(t):
            if c == 0x2F:
                if i:
                    before.add(t[i - 1])
                if i + 1 < len(t):
                    after.add(t[i + 1])
    every = set(range(256)) - {0x2F}
    assert every <= before and every <= after
    for n in C.WORD_LENGTHS:
        assert any(len(t) == n and b"/" not in t for t in sub), n
        assert any(b"/" in t and len(t.split(b"/")[0]) == n for t in sub), n
        assert any(b"/" in t and any(len(w) == n for w in t.split(b"/")[1:]) for t in sub), n
    assert sub[-2] == C.long_level() and sub[-1] == C.deep_topic()
    assert sum(1 for t in sub if len(t) == C.LONG_LEVEL) == 1
    assert sum(1 for t in sub if t.count(b"/") + 1 == C.DEEP_LEVELS) == 1
    assert {t.count(b"/") + 1 for t in sub} >= set(C.LEVEL_COUNTS)
    assert set(C.FIXED) <= set(sub)


@pytest.fixture(scope="module")
def byte_set():
    bs = A.byte_checks()
    rules = [pyacl.compile_rule(r) for r in bs.rules]
    with A.deep():
        want = [pyacl.check_acl(rules, A.oracle_cred(c), p, t) for c, p, t in bs.checks]
    return bs, rules, want


def test_byte_checks_credentials_and_topics():
    bs = A.byte_checks()
    assert bs.checks == A.byte_checks().checks and bs.rules == A.byte_checks(A.SEED).rules       # seeded
    assert 100 <= len(bs.rules) <= 160 and 600 <= len(bs.checks) <= 700          # the docstring: 126 and 619
    sub = A.subset()
    words = {w for t in sub for w in t.split(b"/")}
    ids = [c.get(k, "missing") for c, _, _ in bs.checks for k in ("client_id", "username")]
    for w in (b"+", b"#", b"%c", b"%u", b"", None, "missing"):
        assert w in ids, w
    real = [w for w in ids if isinstance(w, bytes)]
    assert any(any(x >= 0x80 for x in w) for w in real)
    assert {255, 256, 257} <= {len(w) for w in real}
    assert all(w in words or w in (b"%c", b"%u", A.GIANT_CLIENT, A.GIANT_OTHER, b"c1", b"u1") for w in real)
    assert set(sub) <= {t for _, _, t in bs.checks}                      # every subset topic is checked
    assert [len(t) for _, _, t in bs.checks[-2:]] == [C.LONG_LEVEL] * 2   # the costly ones last: batch cuts skip them
    assert all(len(t) < C.LONG_LEVEL for _, _, t in bs.checks[:-2])
    # rule topics: corpus filters, {eq, T}, and one level of a corpus topic replaced by a variable
    fset = set(C.filters(sub))
    for r, kind in zip(bs.rules, bs.fkind):
        for f in r[3]:
            if kind == "eq":
                assert f[0] == "eq" and f[1] in sub
            elif kind == "plain":
                assert f in fset or f in sub or f[:-1] + bytes([f[-1] ^ 1]) == sub[-2] or f.endswith(b"/#"), f[:40]
            else:
                var = b"%c" if kind == "pattern_c" else b"%u"
                lv = f.split(b"/")
                assert lv.count(var) == 1
                i = lv.index(var)
                assert any(t.split(b"/")[:i] == lv[:i] and t.split(b"/")[i + 1:] == lv[i + 1:] and
                           t.count(b"/") == f.count(b"/") for t in sub), f[:40]


def test_byte_checks_every_kind_decides_a_first_match(byte_set):
    bs, rules, want = byte_set
    fk, wk, acc, undef = set(), set(), set(), set()
    results = set()
    with A.deep():
        for (cred, pubsub, topic), (res, idx) in zip(bs.checks, want):
            results.add(res)
            if idx is None:
                continue
            without = pyacl.check_acl(rules[idx + 1:], A.oracle_cred(cred), pubsub, topic)[0]
            if without == res:
                continue                                       # a later rule gives the same answer: not decisive
            fk.add(bs.fkind[idx])
            wk.add(bs.wkind[idx])
            acc.add((bs.rules[idx][2], pubsub))
            key = {"pattern_c": "client_id", "pattern_u": "username"}.get(bs.fkind[idx])
            if key and cred.get(key) is None:
                undef.add((bs.fkind[idx], key in cred))
    assert fk == {"plain", "eq", "pattern_c", "pattern_u"}
    assert undef == {("pattern_c", True), ("pattern_c", False), ("pattern_u", True), ("pattern_u", False)}
    assert wk == {"all", "client", "user", "client_all", "user_all", "ipaddr", "and", "or"}
    assert acc == {("publish", "publish"), ("subscribe", "subscribe"), ("pubsub", "publish"), ("pubsub", "subscribe")}
    assert results == {"allow", "deny", "nomatch"}
    n = len(want)
    assert 0.2 * n < sum(1 for r, _ in want if r == "nomatch") < 0.8 * n
    # the giants: the eq rule takes the long level, its last-byte sibling does not; a late rule takes the deep one
    assert want[-2] == ("allow", 0) and want[-1] == ("deny", 2)
    deep = [w for (c, p, t), w in zip(bs.checks, want) if t == C.deep_topic()]
    assert any(i is not None and i > 2 for _, i in deep)


def test_closed_rule_set_never_ends_nomatch(byte_set):
    bs, rules, want = byte_set
    crules = [pyacl.compile_rule(r) for r in A.closed(bs.rules)]
    last = len(crules) - 1
    decided = 0
    with A.deep():
        for (cred, pubsub, topic), (res, idx) in list(zip(bs.checks, want))[::4]:
            got = pyacl.check_acl(crules, A.oracle_cred(cred), pubsub, topic)
            assert got == ((res, idx) if idx is not None else ("deny", last))
            decided += idx is None                              # without {deny, all} the answer was nomatch
    assert decided > 20


def test_late_rule_set():
    rules, late, checks = A.late_rule_set()
    assert len(rules) == 2000 and late == 1990
    assert sum(len(w) for r in rules for f in r[3] for w in f.split(b"/")) > 65536       # the arena's bytes
    comp = [pyacl.compile_rule(r) for r in rules]
    want = [pyacl.check_acl(comp, A.oracle_cred(c), p, t) for c, p, t in checks]
    assert set(want) == {("allow", late), ("nomatch", None)}
    assert sum(1 for w in want if w[1] == late) >= 15
    # the late rule's topic under the other credentials falls through every rule
    assert any(t == rules[late][3][0] and w[1] is None for (c, p, t), w in zip(checks, want))


# ---- rewrite -------------------------------------------------------------------------------------

def test_rewrite_rules_first_match_spread():
    fs = A.rewrite_rules()
    assert fs == A.rewrite_rules() and len(fs) == 72 and len(set(fs)) == 72
    sub = A.subset()
    fset = set(C.filters(sub))
    assert all(f in fset for f in fs[:64]) and all(C.valid_filter(f) for f in fs)
    for f in (b"#", b"+", b"+/#", b"$SYS/#", b""):
        assert f in fs
    assert any(f[:2] == b"+x" for f in fs) and any(f[:2] == b"#y" for f in fs)
    with A.deep():
        want = [pytrie.rewrite_rule_index(t, fs) for t in sub]
    hit = [w for w in want if w is not None]
    assert None in want and len(set(hit)) >= 20
    assert sum(1 for w in hit if w > 0) > len(sub) // 2                 # a later rule is the first match
    first = {fs[w] for w in hit}
    assert {b"+", b"+/#", b"$SYS/#", b""} <= first                       # ('#' stands behind '+' and '+/#')
    assert any(w is not None and w < 64 for w in want)
    # the '$' clause is about the first byte: "+x/..." is no wildcard, yet never takes a '$' topic
    assert pytrie.match(b"+x/x+", b"+x/x+") and not pytrie.match(b"$x", b"+x/#") and b"+x/x+" in sub
    assert want[sub.index(b"+x/x+")] <= fs.index(b"+x/x+")               # its own text, or a '+' variant before it
    assert [t for t, w in zip(sub, want) if w is None and t[:1] != b"$"] == []


# ---- status codes on a host-only handle ---------------------------------------------------------

def _who_calls(who):
    """the tm_acl_who calls of one who term, in order: (kind, arg)"""
    if who == "all":
        return [(WHO["all"], None)]
    kind, arg = who
    if kind in ("and", "or"):
        return [(WHO[kind], None)] + [c for w in arg for c in _who_calls(w)] + [(WHO["end"], None)]
    if arg == "all":
        return [(WHO[kind + "_all"], None)]
    return [(WHO[kind], arg.encode() if isinstance(arg, str) else arg)]


@pytest.fixture()
def host():
    a = AclRules(device=-1)
    yield a
    a.close()


def test_who_past_the_stack_limit_is_refused_at_its_call(host):
    lib = host.lib
    for name, who, refused in A.over_limit_whos():
        assert A.peak_live(who) == A.STACK_MAX + 1, name
        before = lib.tm_acl_rule_count(host.h)
        assert lib.tm_acl_rule_begin(host.h, 1, 3) == _lib.TM_OK
        calls = _who_calls(who)
        rcs = [lib.tm_acl_who(host.h, k, a, len(a) if a else 0, 0) for k, a in calls[:refused + 1]]
        assert rcs == [_lib.TM_OK] * refused + [_lib.TM_ERANGE], (name, rcs[-3:])
        # the rule is gone: nothing is open, the count is back
        assert lib.tm_acl_rule_count(host.h) == before
        assert lib.tm_acl_who(host.h, WHO["all"], None, 0, 0) == _lib.TM_EINVAL
        assert lib.tm_acl_rule_end(host.h) == _lib.TM_EINVAL
        with pytest.raises(_lib.TopicMatchError) as e:
            host.add(("deny", who, "pubsub", [b"a"]))
        assert e.value.code == _lib.TM_ERANGE, name
        assert lib.tm_acl_rule_count(host.h) == before
    # every case of who_shapes() builds, the ones at the limit included, and the handle stays usable
    cases = A.who_shapes()
    for c in cases:
        host.add(("allow", c.who, "pubsub", [b"a"]))
    assert lib.tm_acl_rule_count(host.h) == len(cases)
    assert max(c.peak for c in cases) == A.STACK_MAX


def test_cidr_prefixes_build_or_are_refused(host):
    lib = host.lib
    assert lib.tm_acl_rule_begin(host.h, 1, 3) == _lib.TM_OK

    def who(text, prefix=0):
        return lib.tm_acl_who(host.h, WHO["ipaddr"], text, len(text), prefix)
    for text in (b"0.0.0.0/0", b"::/0", b"10.1.2.3/0", b"10.1.2.3/32", b"::1/128", b"fe80::/10", b"10.1.2.3", b"::1"):
        assert who(text) == _lib.TM_OK, text
    for text in (b"0.0.0.0/33", b"::/129", b"10.0.0.0/", b"10.0.0.0/8/8", b"10.0.0.0/-1", b"10.0.0.0/ 8",
                 b"10.0.0.0/4294967296", b"/8", b"10.0.0/8", b"nonsense"):
        assert who(text) == _lib.TM_EINVAL, text
    # a bare address keeps `prefix`: 0 = the host, else the bits
    assert who(b"10.0.0.0", 8) == _lib.TM_OK and who(b"10.0.0.0", 32) == _lib.TM_OK and who(b"::", 128) == _lib.TM_OK
    assert who(b"10.0.0.0", 33) == _lib.TM_EINVAL and who(b"::", 129) == _lib.TM_EINVAL
    assert lib.tm_acl_rule_end(host.h) == _lib.TM_OK
    for n, text, _ in A.cidr_cases():
        host.add(("allow", ("ipaddr", text), "pubsub", [b"a"]))


def _call(a, arrs, n, device=False):
    P = lambda x: None if x is None else ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    out = np.zeros(n, dtype=np.int8)
    rule = np.zeros(n, dtype=np.uint32)
    if device:
        return a.lib.tm_acl_check_batch_device(a.h, n, *[P(arrs[k]) for k in a.ARGS], P(out), P(rule), None)
    return a.lib.tm_acl_check_batch(a.h, n, *[P(arrs[k]) for k in a.ARGS], P(out), P(rule))


def test_check_batch_argument_checks(host):
    host.add(("allow", ("ipaddr", "10.0.0.0/8"), "pubsub", [b"a/#"]))
    creds = [dict(A.FULL), dict(A.FULL), dict(A.FULL)]
    arrs = AclRules.pack(creds, ["publish"] * 3, [b"a/b", b"a", b"a/c/d"])
    assert _call(host, arrs, 3) == _lib.TM_EDEVICE               # well formed: only the device is missing
    assert _call(host, dict(arrs, peers=None, peer_family=None), 3) == _lib.TM_EDEVICE
    assert _call(host, dict(arrs, peer_family=None), 3) == _lib.TM_EDEVICE
    assert _call(host, dict(arrs, peers=None), 3) == _lib.TM_EINVAL          # a family without the addresses
    for key in ("topic_off", "client_off", "user_off"):
        for at in (1, 2, 3):
            off = arrs[key].copy()
            off[at - 1] = off[at] + np.uint64(1)                 # entry `at` lies below the one before it
            assert _call(host, dict(arrs, **{key: off}), 3) == _lib.TM_EINVAL, (key, at)
        lifted = arrs[key] + np.uint64(5)                        # a non-zero first offset is fine
        assert _call(host, dict(arrs, **{key: lifted}), 3) == _lib.TM_EDEVICE
    # the device entry cannot read its offsets; it still refuses a family without addresses
    assert _call(host, dict(arrs, peers=None), 3, device=True) == _lib.TM_EINVAL
    assert _call(host, dict(arrs, peers=None, peer_family=None), 3, device=True) == _lib.TM_EDEVICE
