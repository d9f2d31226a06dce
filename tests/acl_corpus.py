"""Seeded cases hostile to the two device paths the byte corpus left out:
acl.hip (its own '/' scanner, byte compare, CIDR masks and the and/or stack
of who_match) and rewrite.hip (its own scanner and compare).  Shared by
tests/test_acl_corpus.py (CPU: coverage pinned on the oracles alone) and by
tests/test_gpu_acl_edges.py / tests/test_gpu_rewrite_bytes.py (the device
entries against oracle/pyacl.py and oracle/pytrie.py).

A plain helper module: no fixtures, fixed seeds, nothing from time or the
environment, and nothing from the product package.  Credentials are in the
product's form (client_id / username bytes or None, peername (ip text, port)
or None, a missing key = the map lacks it); oracle_cred() gives the oracle's.

    who_shapes()      493 named who terms with their peak live stack count
    cidr_cases()      111 (name, CIDR text, credentials)
    subset()          372 corpus topics: 255 '/'-neighbour topics (every byte
                      value before and after a '/'), 67 that hold every length
                      class of byte_corpus.WORD_LENGTHS as an inner level, a
                      first word and a whole topic, the 28 fixed shapes, 28
                      NUL-sibling and level-count topics, the LONG_LEVEL and
                      the DEEP_LEVELS topic (a few topics serve two classes)
    byte_checks()     126 rules over that subset and 619 checks of them
    late_rule_set()   2,000 rules, a 97 KiB arena, 120 checks, only rule 1,990
                      ever matches
    rewrite_rules()   64 filters of the subset + the fixed ones, 72 in all
"""
import collections
import contextlib
import ipaddress
import random
import sys

import byte_corpus as C

SEED = 20261
STACK_MAX = 64          # TM_ACL_WHO_STACK_MAX (include/topicmatch.h)

WhoCase = collections.namedtuple("WhoCase", "name peak who creds")
ByteSet = collections.namedtuple("ByteSet", "rules fkind wkind checks")

# the credentials the who leaves are written against, and one with nothing in it
FULL = {"client_id": b"c1", "username": b"u1", "peername": ("10.1.2.3", 1883)}
BARE = {}
_TRUE = [("client", b"c1"), ("user", b"u1"), ("client", "all"), ("user", "all"), "all", ("ipaddr", "10.0.0.0/8")]
_FALSE = [("client", b"nobody"), ("user", b"nobody"), ("ipaddr", "192.168.0.0/16")]
# minimal reproducers of bugs these cases found in acl.hip / rewrite.hip, kept as named cases:
# (name, who, credentials) and (name, CIDR text, credentials)
WHO_REGRESSIONS = [
    # a 32-bit stack shifted the first leaf out: the group read it back as false
    ("regress/and_33_flat_over_two_levels", ("and", [("client", b"c1")] * 16 + [("and", [("client", b"c1")] * 17)]),
     [FULL]),
]
CIDR_REGRESSIONS = [
    # prefix 0 meant "host": allow-everyone matched 0.0.0.0 alone
    ("regress/v4_slash0_any_peer", "0.0.0.0/0", {"peername": ("10.1.2.3", 1883)}),
]


def oracle_cred(c):
    out = {k: c[k] for k in ("client_id", "username") if k in c}
    if "peername" in c:
        p = c["peername"]
        out["peername"] = None if p is None else (ipaddress.ip_address(p[0]).packed, p[1])
    return out


@contextlib.contextmanager
def deep():
    """the oracles recurse once per level: room for the 2,000-level topic"""
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 3 * C.DEEP_LEVELS + 1000))
    try:
        yield
    finally:
        sys.setrecursionlimit(old)


# ---- who terms -----------------------------------------------------------------------

def _is_group(w):
    return isinstance(w, tuple) and w[0] in ("and", "or")


def stack_trace(who):
    """(peak, deepest): the postfix evaluation of `who` on a stack, a leaf
    pushing one result and a group replacing its children's by one.  peak is
    the most results alive at once; deepest[i] is the lowest place, counted
    from the top (1 = the top), that leaf i (in evaluation order) ever has"""
    stack, deepest, peak = [], [], 0

    def push(x):
        nonlocal peak
        stack.append(x)
        peak = max(peak, len(stack))
        for at, e in enumerate(stack):
            if e is not None:
                deepest[e] = max(deepest[e], len(stack) - at)

    def walk(w):
        if _is_group(w):
            for c in w[1]:
                walk(c)
            if w[1]:
                del stack[-len(w[1]):]
            push(None)
        else:
            deepest.append(0)
            push(len(deepest) - 1)
    walk(who)
    return peak, deepest


def peak_live(who):
    return stack_trace(who)[0]


def _shape_leaves(shape):
    return 1 if shape is None else sum(_shape_leaves(c) for c in shape[1])


def _fill(shape, values):
    """shape: None (a leaf) | (op, [shape...]); values: one bool per leaf in
    evaluation order -> the who term, each leaf a condition that holds /
    fails for FULL, its kind rotating with its index"""
    it = iter(enumerate(values))

    def go(s):
        if s is None:
            i, v = next(it)
            return _TRUE[i % len(_TRUE)] if v else _FALSE[i % len(_FALSE)]
        return (s[0], [go(c) for c in s[1]])
    return go(shape)


def _decided_by(shape, target, value):
    """leaf values under which leaf `target` alone decides the term: every
    subtree beside the path to it evaluates to its parent's identity (true
    under 'and', false under 'or'), so the term's value is `value`"""
    out = []

    def force(s, v):
        if s is None:
            out.append(v)
        else:
            for c in s[1]:
                force(c, v)

    def count(s):
        return _shape_leaves(s)

    def go(s, first):
        if s is None:
            out.append(value)
            return
        ident = s[0] == "and"
        at = first
        for c in s[1]:
            k = count(c)
            if at <= target < at + k:
                go(c, at)
            else:
                force(c, ident)
            at += k
    go(shape, 0)
    return out


def _tail(ops, widths):
    """(op0, [leaf x w0, (op1, [leaf x w1, (op2, ...)])]): peak = sum(widths)"""
    s = (ops[-1], [None] * widths[-1])
    for op, w in zip(reversed(ops[:-1]), reversed(widths[:-1])):
        s = (op, [None] * w + [s])
    return s


def _head(ops, inner, outer):
    """(op0, [(op1, [leaf x inner]), leaf x outer]): the outer operator is
    applied to outer + 1 results, peak = max(inner, outer + 1)"""
    return (ops[0], [(ops[1], [None] * inner)] + [None] * outer)


def _shapes():
    out = []
    for op in ("and", "or"):
        for w in (0, 1, 2, 31, STACK_MAX):
            out.append(("flat_%s_%d" % (op, w), (op, [None] * w)))
    for peak, (a, b) in ((31, (15, 16)), (32, (16, 16)), (33, (16, 17)), (40, (20, 20)), (STACK_MAX, (32, 32))):
        for ops in (("and", "and"), ("and", "or"), ("or", "and"), ("or", "or")):
            out.append(("tail_%s_%d_%s_%d" % (ops[0], a, ops[1], b), _tail(ops, (a, b))))
    for peak, ws in ((31, (10, 10, 11)), (32, (10, 11, 11)), (33, (11, 11, 11)), (40, (13, 13, 14)),
                     (STACK_MAX, (21, 21, 22))):
        for ops in (("and", "or", "and"), ("or", "and", "or")):
            out.append(("tail3_%s_%s" % ("_".join(ops), "_".join(map(str, ws))), _tail(ops, ws)))
    for peak in (31, 32, 33, 40, STACK_MAX):
        for ops in (("and", "or"), ("or", "and")):
            out.append(("head_%s_%d_%s_8" % (ops[0], peak - 1, ops[1]), _head(ops, 8, peak - 1)))
    return out


def who_shapes():
    """[WhoCase(name, peak, who, credentials)]: per shape all leaves true, all
    false, and each of the first leaf, the last leaf and the leaves whose
    deepest place on the stack is 31, 32 and 33 from the top (for the outer
    leaves of a head_ shape that is their place when the outer operator is
    applied) deciding the term alone, once as true and once as false"""
    out = []
    for name, shape in _shapes():
        n = _shape_leaves(shape)
        probe = _fill(shape, [True] * n)
        peak, deepest = stack_trace(probe)
        out.append(WhoCase(name + "/all_true", peak, probe, [FULL, BARE]))
        out.append(WhoCase(name + "/all_false", peak, _fill(shape, [False] * n), [FULL, BARE]))
        targets = {}
        if n:
            targets["first"] = 0
            targets["last"] = n - 1
        for place in (31, 32, 33):
            if place in deepest:
                targets["place%d" % place] = deepest.index(place)
        for tag, leaf in targets.items():
            for v in (True, False):
                out.append(WhoCase("%s/%s_decides_%s" % (name, tag, "true" if v else "false"), peak,
                                   _fill(shape, _decided_by(shape, leaf, v)), [FULL]))
    T, F = ("client", b"c1"), ("client", b"nobody")
    table = [("table/and_T16_and_T17", ("and", [T] * 16 + [("and", [T] * 17)])),
             ("table/and_T20_or_T20", ("and", [T] * 20 + [("or", [T] * 20)])),
             ("table/or_T_F19_and_T19_F", ("or", [T] + [F] * 19 + [("and", [T] * 19 + [F])])),
             ("table/and_T16_and_T16", ("and", [T] * 16 + [("and", [T] * 16)]))]
    for name, who in table:
        out.append(WhoCase(name, peak_live(who), who, [FULL]))
    for name, who, creds in WHO_REGRESSIONS:
        out.append(WhoCase(name, peak_live(who), who, creds))
    return out


def over_limit_whos():
    """terms one past the stack limit, with the index (in tm_acl_who call
    order: a group's opening call, its conditions, its END) of the refused call"""
    T = ("client", b"c1")
    return [("flat_65", ("and", [T] * (STACK_MAX + 1)), STACK_MAX + 1),
            ("tail_33_32", ("and", [T] * 33 + [("or", [T] * 32)]), 1 + 33 + 1 + 31),
            ("empty_group_at_64", ("or", [T] * STACK_MAX + [("and", [])]), 1 + STACK_MAX + 1)]


# ---- CIDRs ------------------------------------------------------------------------------

V4_PREFIXES = [0, 1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32]
V6_PREFIXES = [0, 1, 7, 8, 9, 63, 64, 65, 127, 128]
_V4_BASE = int(ipaddress.IPv4Address("198.51.100.85"))
_V6_BASE = int(ipaddress.IPv6Address("2001:db8:85a3:8d3:1319:8a2e:370:7349"))


def cidr_cases():
    """[(name, CIDR text, credentials)]: per prefix a network text with host
    bits set and the peers at start - 1, start, end and end + 1 of its range
    where they exist; family mismatches; no peername; bare hosts"""
    out = []
    for ver, prefixes, base in ((4, V4_PREFIXES, _V4_BASE), (6, V6_PREFIXES, _V6_BASE)):
        addr = ipaddress.IPv4Address if ver == 4 else ipaddress.IPv6Address
        top = (1 << (32 if ver == 4 else 128)) - 1
        for p in prefixes:
            text = "%s/%d" % (addr(base), p)           # the base's low bit is set: host bits for every p below the width
            net = ipaddress.ip_network(text, strict=False)
            lo, hi = int(net.network_address), int(net.broadcast_address)
            for tag, v in (("below", lo - 1), ("start", lo), ("end", hi), ("above", hi + 1)):
                if 0 <= v <= top:
                    out.append(("v%d/%d/%s" % (ver, p, tag), text, {"peername": (str(addr(v)), 1883)}))
    out += [("zero/v4_any", "0.0.0.0/0", {"peername": ("10.1.2.3", 1883)}),
            ("zero/v4_top", "0.0.0.0/0", {"peername": ("255.255.255.255", 1883)}),
            ("zero/v6_any", "::/0", {"peername": ("fe80::5", 1883)}),
            ("zero/v6_top", "::/0", {"peername": ("ffff:ffff:ffff:ffff:ffff:ffff:ffff:ffff", 1883)}),
            ("family/v4_rule_mapped_peer", "10.0.0.0/8", {"peername": ("::ffff:10.1.2.3", 1883)}),
            ("family/v6_mapped_rule_v4_peer", "::ffff:10.0.0.0/104", {"peername": ("10.1.2.3", 1883)}),
            ("family/v6_mapped_rule_mapped_peer", "::ffff:10.0.0.0/104", {"peername": ("::ffff:10.1.2.3", 1883)}),
            ("family/v4_zero_v6_peer", "0.0.0.0/0", {"peername": ("::1", 1883)}),
            ("family/v6_zero_v4_peer", "::/0", {"peername": ("10.1.2.3", 1883)}),
            ("host/v4_same", "10.1.2.3", {"peername": ("10.1.2.3", 1883)}),
            ("host/v4_below", "10.1.2.3", {"peername": ("10.1.2.2", 1883)}),
            ("host/v4_above", "10.1.2.3", {"peername": ("10.1.2.4", 1883)}),
            ("host/v4_high_byte", "10.1.2.3", {"peername": ("138.1.2.3", 1883)}),
            ("host/v6_same", "::1", {"peername": ("::1", 1883)}),
            ("host/v6_above", "::1", {"peername": ("::2", 1883)}),
            ("host/v6_high_byte", "::1", {"peername": ("8000::1", 1883)})]
    for text in ("0.0.0.0/0", "::/0", "10.0.0.0/8", "10.1.2.3"):
        out.append(("nopeer/%s/missing" % text, text, {"client_id": b"c1"}))
        out.append(("nopeer/%s/undefined" % text, text, {"client_id": b"c1", "peername": None}))
    out += CIDR_REGRESSIONS
    return out


# ---- the byte corpus, thinned ---------------------------------------------------------------

def subset(seed=C.SEED):
    """the smallest corpus subset that keeps every byte value on both sides of
    a '/', every word-length class (as an inner level, a first word and a
    whole topic), the fixed shapes, a few NUL siblings and level counts, and
    the two giants; in corpus order"""
    sec = C.sections(seed)
    slash = sec["slash"]
    per = len(slash) // 8                               # one topic per byte value and offset mod 8
    keep = {slash[(k % 8) * per + k] for k in range(per)}
    for n in C.WORD_LENGTHS:
        inner = first = whole = None
        for t in sec["length"]:
            lv = t.split(b"/")
            if whole is None and len(lv) == 1 and len(t) == n:
                whole = t
            if first is None and len(lv) > 1 and len(lv[0]) == n:
                first = t
            if inner is None and len(lv) > 1 and any(len(w) == n for w in lv[1:]):
                inner = t
        keep.update((inner, first, whole))
    keep.update(sec["fixed"])
    keep.update(sec["nul"][::16])
    keep.update(sec["levels"][::7])                      # one topic per level count
    keep.update(sec["giant"])
    out, seen = [], set()
    for t in C.topics(seed):
        if t in keep and t not in seen:
            seen.add(t)
            out.append(t)
    return out


def _atomic(w):
    return w in (b"", b"+", b"#")


def cred_words(ts, rng):
    """client ids / usernames: words of the topics themselves, the ones that
    look like wildcards or variables, and None for the undefined credential"""
    words = sorted({w for t in ts[:-2] for w in t.split(b"/")})
    by_len = {n: [w for w in words if len(w) == n] for n in (255, 256, 257)}
    high = [w for w in words if 2 <= len(w) <= 16 and any(c >= 0x80 for c in w)]
    short = [w for w in words if 1 <= len(w) <= 64 and not _atomic(w)]
    return [b"+", b"#", b"%c", b"%u", b"", None, high[0], high[len(high) // 2], by_len[255][0], by_len[256][0],
            by_len[257][0]] + rng.sample(short, 21)


PEERS = [("10.1.2.3", 1883), ("192.168.1.7", 1883), ("2001:db8::5", 1883), None]
_NETS = {"10.1.2.3": "10.1.2.200/8", "192.168.1.7": "192.168.1.0/24", "2001:db8::5": "2001:db8::/32"}
GIANT_CLIENT, GIANT_OTHER = b"giant-eq", b"giant-sibling"


def _who_for(k, cred):
    """a who of kind k % 8 that holds for cred (where the kind can)"""
    cid, usr, peer = cred.get("client_id"), cred.get("username"), cred.get("peername")
    net = ("ipaddr", _NETS[peer[0]]) if peer else ("ipaddr", "10.0.0.0/8")
    c = ("client", cid) if cid is not None else ("client", "all")
    u = ("user", usr) if usr is not None else ("user", "all")
    k %= 8
    if k == 0:
        return "all", "all"
    if k == 1:
        return c, "client" if cid is not None else "client_all"
    if k == 2:
        return u, "user" if usr is not None else "user_all"
    if k == 3:
        return ("client", "all"), "client_all"
    if k == 4:
        return ("user", "all"), "user_all"
    if k == 5:
        return net, "ipaddr"
    if k == 6:
        return ("and", [c, ("or", [("user", b"nobody"), u]), "all"]), "and"
    return ("or", [("client", b"nobody"), ("and", [u, c]), ("ipaddr", "203.0.113.0/24")]), "or"


def byte_checks(seed=SEED):
    """ByteSet(rules, fkind, wkind, checks) over subset(): rule r has filters
    of one kind fkind[r] ("plain" | "eq" | "pattern_c" | "pattern_u" | None for
    {A, all}) and a who of kind wkind[r]; checks are (credentials, pubsub,
    topic), the two that hold the 65,535-byte level last.  No rule is
    {A, all}: closed(rules) appends one"""
    rng = random.Random(seed)
    ts = subset()
    long_t, deep_t = ts[-2], ts[-1]
    assert len(long_t) == C.LONG_LEVEL and deep_t.count(b"/") + 1 == C.DEEP_LEVELS
    cw = cred_words(ts, rng)
    rules, fkind, wkind, checks = [], [], [], []

    def add(allow, who, wk, access, topics, fk):
        rules.append(("allow" if allow else "deny", who, access, topics))
        fkind.append(fk)
        wkind.append(wk)

    # the 65,535-byte level costs a lane 64 KiB per filter it is held against: its two checks end at rules 0-2
    sibling = long_t[:-1] + bytes([long_t[-1] ^ 1])
    add(True, ("client", GIANT_CLIENT), "client", "pubsub", [("eq", long_t)], "eq")
    add(True, ("client", GIANT_OTHER), "client", "pubsub", [sibling], "plain")
    add(False, ("client", GIANT_OTHER), "client", "pubsub", [b"#"], "plain")
    small = ts[:-2]
    anchors = rng.sample(small, 110) + [deep_t, b"a/+/b", b"+", b"#", b"", b"a//b", b"/"]
    # levels worth substituting: a 255-, 256- and 257-byte one, one with a high byte, and the atoms
    want = [t for n in (255, 256, 257) for t in small if any(len(w) == n for w in t.split(b"/"))][:6]
    anchors += want
    for k, t in enumerate(anchors):
        lv = t.split(b"/")
        kind = ("plain", "eq", "pattern_c", "pattern_u", "pattern_undef")[k % 5]
        cred = {"client_id": cw[(3 * k) % len(cw)], "username": cw[(5 * k + 1) % len(cw)],
                "peername": PEERS[k % len(PEERS)]}
        if cred["client_id"] in (GIANT_CLIENT, GIANT_OTHER):
            cred["client_id"] = b"c1"
        if k % 11 == 0:
            del cred["username"]
        if k % 8 == 5 and not cred["peername"]:
            cred["peername"] = PEERS[0]
        topic = t
        at = max(range(len(lv)), key=lambda i: (len(lv[i]), -i)) if k % 3 else rng.randrange(len(lv))
        if kind == "plain":
            cand = C.filters([t]) if C.valid_filter(t) else [b"/".join(lv[:1] + [b"#"])]
            own = [f for f in cand if f not in (b"#", b"+", b"+/#", b"+/+")] or [t]
            fs = [own[k % len(own)]] + ([small[(7 * k) % len(small)]] if k % 4 == 0 else [])
            fk = "plain"
        elif kind == "eq":
            fs = [("eq", t)] + ([("eq", small[(7 * k) % len(small)])] if k % 4 == 1 else [])
            fk = "eq"
        else:
            var = b"%u" if kind == "pattern_u" or (kind == "pattern_undef" and k % 2) else b"%c"
            key = "username" if var == b"%u" else "client_id"
            fs = [b"/".join(lv[:at] + [var] + lv[at + 1:])]
            fk = "pattern_u" if var == b"%u" else "pattern_c"
            if kind == "pattern_undef":
                cred[key] = None                         # feed_var leaves the word: the topic must hold "%c" itself
                if k % 4 >= 2:
                    del cred[key]
                topic = fs[0]
            else:
                cred[key] = lv[at]                       # substitution reproduces the topic (unless the level is an atom)
        who, wk = _who_for(k, cred)
        access = ("publish", "subscribe", "pubsub")[k % 3]
        add(k % 2 == 0, who, wk, access, fs, fk)
        pubsub = "subscribe" if access == "subscribe" else "publish"
        checks.append((cred, pubsub, topic))
        other = dict(cred)
        other["client_id"] = cw[(3 * k + 1) % len(cw)]   # the same topic as somebody else
        checks.append((other, "publish" if pubsub == "subscribe" else "subscribe", topic))
    # every subset topic once more, as a rotating somebody
    for i, t in enumerate(small + [deep_t]):
        cred = {"client_id": cw[i % len(cw)], "username": cw[(7 * i + 3) % len(cw)]}
        if i % 5 != 4:
            cred["peername"] = PEERS[i % len(PEERS)]
        if i % 13 == 0:
            del cred["client_id"]
        checks.append((cred, ("publish", "subscribe")[i % 2], t))
    checks.append(({"client_id": GIANT_CLIENT, "username": b"u1", "peername": PEERS[0]}, "publish", long_t))
    checks.append(({"client_id": GIANT_OTHER, "username": None}, "subscribe", long_t))
    return ByteSet(rules, fkind, wkind, checks)


def closed(rules):
    """the rule set with {deny, all} at its end: no check ends nomatch"""
    return list(rules) + [("deny", "all")]


def late_rule_set():
    """(rules, late, checks): 2,000 rules whose filter words fill more than
    64 KiB of arena; rule `late` is the only one any check matches"""
    rng = random.Random(SEED + 1)
    rules = []
    for r in range(2000):
        w = bytes(rng.choice(C.ASCII) for _ in range(40))
        who = ("all", ("client", b"c%d" % r), ("user", "all"), ("ipaddr", "10.0.0.0/8"))[r % 4]
        rules.append((("allow", "deny")[r % 2], who, "pubsub", [b"late/%d/" % r + w]))
    late = 1990
    hit = rules[late][3][0]
    rules[late] = ("allow", ("and", [("client", b"c1"), ("user", b"u1")]), "pubsub", [hit])
    checks = []
    for i in range(120):
        t = hit if i % 3 == 0 else rules[rng.randrange(2000)][3][0][:-1] + b"!"
        cred = dict(FULL) if i % 2 == 0 else {"client_id": b"c1", "username": b"u2", "peername": ("10.1.2.3", 1)}
        checks.append((cred, ("publish", "subscribe")[i % 2], t))
    return rules, late, checks


# ---- rewrite ------------------------------------------------------------------------------------

def rewrite_rules(seed=SEED):
    """64 filters of the subset (fixed seed), then filters whose first BYTE is
    '+' / '#' without being the wildcard (the binary '$' clause tests the
    byte), '$SYS/#' and the empty filter, and the catch-alls last: a later
    rule is the first match of most topics, '$...' topics outside $SYS match
    none"""
    rng = random.Random(seed + 2)
    fs = [f for f in C.filters(subset()) if f not in (b"#", b"+", b"+/#", b"+/+", b"")]
    return rng.sample(fs, 64) + [b"+x/x+", b"#y", b"+x/#", b"$SYS/#", b"", b"+", b"+/#", b"#"]
