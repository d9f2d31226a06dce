"""A seeded churn model of the subscription trie (a plain module, no test):
a base trie, rounds of (op, filter) lists each followed by one commit, the
model of the live set and the topics that walk what each round changed.

The base trie (about 6,000 filters over about 400 words plus '+', '#', empty
levels and '$' first levels; depths 1 to 7 and a handful of 18 to 20 levels;
literal fan-outs from 1 to about 40, several parents at 14 to 15 children) is
the smallest that keeps a round of about 100 ops under the commit's scatter
bound (engine.cpp upload_plan: the two logs' elements times (4 + element
bytes) times 4 within the table's bytes) and still has a few hundred WIDE
nodes.

Small rounds (at most 120 ops) are built to reach the mutation paths whose
dirty marks lie far from the filter just changed:
  fresh     a new filter with a fresh word under an existing node (the
            dictionary grows, nodes are created)
  again     delete and re-insert of the same filter, in one round and across
            two (filter-id quarantine and reuse)
  step      chosen parents' literal children 0 -> 1 -> 2 -> 3 -> 2 -> 1 -> 0
            over consecutive rounds (the inline pair spills, the node goes
            WIDE, then narrow again with the Bloom mask cleared)
  flip      x/# added and removed beside x/+/y and x/z (field 1 flips between
            a filter id and the summaries)
  branch    a whole branch deleted while other nodes are created in the same
            and in the next round (node-id reuse)
  dense     deletes and later re-inserts of literal children of the widest
            parents (backward shifts in the edge tables' probe runs)
  nfmin     parents at 14 to 15 literal children carried across NF_MIN and
            back
Large rounds touch more than a quarter of a table or push the cold edge table
and the dictionary across a power of two (whole-table copies); each is
followed at once by a small round; one is a scripted relayout.
"""
import random

SEED = 20261021
ROUNDS = 40
LARGE = {10: "grow", 20: "shrink", 30: "relayout"}   # round -> kind
WORDS = [b"w%d" % i for i in range(330)]     # about 400 words with the scripted names below
STEP = [1, 2, 3, 2, 1, 0]          # literal children of a stepped parent, per phase
N_STEP, N_FLIP, N_BRANCH, N_NF = 6, 6, 40, 6


def _path(rng, depth):
    """a random filter of `depth` levels: a skewed choice per level, so fan-outs run from 1 to about 40"""
    ws = []
    for lv in range(depth):
        x = rng.random()
        if lv == depth - 1 and depth > 1 and x < 0.08:
            ws.append(b"#")
        elif x < 0.20 and lv > 0:
            ws.append(b"+")
        elif x < 0.215 and lv > 0:
            ws.append(b"")
        elif lv == 0:
            ws.append(WORDS[int(rng.random() ** 2 * 12)])
        else:
            span = (40, 24, 12, 8, 6, 6)[min(lv - 1, 5)]
            base = (sum(len(w) + sum(w) for w in ws) * 7) % (len(WORDS) - span)    # the siblings depend on the prefix
            ws.append(WORDS[base + int(rng.random() ** 1.5 * span)])
    return b"/".join(ws)


def base_filters():
    rng = random.Random(SEED)
    fs = []
    while len(fs) < 5200:
        fs.append(_path(rng, rng.choice((1, 2, 3, 3, 4, 4, 4, 5, 5, 6, 7))))
    fs += [b"$SYS/" + _path(rng, rng.randint(1, 4)) for _ in range(150)] + [b"$SYS/#", b"$share/+/w1", b"+/+", b"#", b"+"]
    fs += [b"deep/" + b"/".join(rng.choice(WORDS[:6]) for _ in range(rng.randint(17, 19))) for _ in range(6)]
    fs += [b"deep/" + b"/".join([b"+"] * 17) + b"/#"]
    for j in range(N_STEP):         # the stepped parents stay alive through their '+' child
        fs.append(b"st/p%d/+" % j)
    for j in range(N_FLIP):
        fs += [b"hf/x%d/+/y" % j, b"hf/x%d/z" % j]
    for j in range(N_BRANCH):
        fs += [b"br/b%d/%s/%s" % (j, WORDS[a], WORDS[b]) for a in range(3) for b in range(4)] + [b"br/b%d/+/#" % j]
    for j in range(N_NF):
        fs += [b"nf/k%d/c%d" % (j, i) for i in range(14 + j % 2)] + [b"+/k%d/c1/#" % j]
    out, seen = [], set()
    for f in fs:
        if f not in seen:
            seen.add(f)
            out.append(f)
    return out


class Model:
    """the live set and the rounds; rounds() is deterministic (SEED)"""

    def __init__(self):
        self.base = base_filters()
        self.live = dict.fromkeys(self.base)     # insertion-ordered set
        self.rng = random.Random(SEED + 1)
        self.fresh = 0
        self.pending = []       # filters deleted last round, re-inserted in this one
        self.dense_out = {}     # round -> filters to re-insert
        self.bulk = []          # the grow round's filters (the shrink round deletes them)
        wide = {}
        for f in self.base:     # the widest literal parents: candidates of the dense deletes
            p, _, last = f.rpartition(b"/")
            if p and last not in (b"+", b"#", b""):
                wide.setdefault(p, []).append(f)
        self.dense = [f for p, kids in wide.items() if len(kids) >= 8 and not p.startswith((b"nf/", b"br/", b"st/", b"hf/"))
                      for f in kids]

    def _apply(self, ops):
        """the ops that change the live set (an insert of a live filter and a delete of an absent one
        are dropped: the reference's delete of an unknown filter aborts), applied"""
        done = []
        for op, f in ops:
            if (op == "insert") == (f in self.live):
                continue
            if op == "insert":
                self.live[f] = None
            else:
                del self.live[f]
            done.append((op, f))
        return done

    def _fresh_word(self):
        self.fresh += 1
        return b"f%d" % self.fresh

    def _small(self, r):
        rng, ops = self.rng, []
        live = list(self.live)
        # again, across two rounds: last round's deletes come back
        ops += [("insert", f) for f in self.pending]
        self.pending = [f for f in rng.sample(live, 8) if not f.startswith((b"st/", b"hf/", b"nf/", b"br/"))]
        ops += [("delete", f) for f in self.pending]
        # again, within the round
        for f in rng.sample(live, 4):
            if f not in self.pending:
                ops += [("delete", f), ("insert", f)]
        # fresh words under existing nodes
        for f in rng.sample(live, 8):
            ws = f.split(b"/")
            cut = rng.randint(1, len(ws))
            tail = [self._fresh_word()] + ([rng.choice(WORDS)] if rng.random() < 0.3 else [])
            ops.append(("insert", b"/".join([w for w in ws[:cut] if w != b"#"] + tail)))
        # step
        for j in range(N_STEP):
            have = [f for f in (b"st/p%d/s%d" % (j, i) for i in range(3)) if f in self.live]
            want = STEP[(r + j) % len(STEP)]
            for i in range(len(have), want):
                ops.append(("insert", b"st/p%d/s%d" % (j, i)))
            for f in have[want:]:
                ops.append(("delete", f))
        # flip
        for j in range(N_FLIP):
            f = b"hf/x%d/#" % j
            if (r + j) % 2:
                ops.append(("delete" if f in self.live else "insert", f))
        # branch: one whole branch goes, other nodes come
        b = (r * 7) % N_BRANCH
        ops += [("delete", f) for f in live if f.startswith(b"br/b%d/" % b)]
        ops += [("insert", b"nb/r%d/n%d" % (r, i)) for i in range(5)]
        # dense: literal children of the widest parents out, those of two rounds ago back in
        for due in [k for k in self.dense_out if k <= r]:
            ops += [("insert", f) for f in self.dense_out.pop(due)]
        gone = {f for op, f in ops if op == "delete"}
        out = [f for f in rng.sample(self.dense, 16) if f in self.live and f not in gone]
        self.dense_out[r + 2] = out
        ops += [("delete", f) for f in out]
        # nfmin: 14..15 children up past 16 and back
        for j in range(N_NF):
            extra = [b"nf/k%d/e%d" % (j, i) for i in range(3)]
            if (r + j) % 4 == 0:
                ops += [("insert", f) for f in extra if f not in self.live]
            elif (r + j) % 4 == 2:
                ops += [("delete", f) for f in extra if f in self.live]
        assert len(ops) <= 120, len(ops)
        return ops

    def _large(self, r, kind):
        rng = self.rng
        if kind == "grow":      # new words past the dictionary's and the cold table's next power of two
            new = [self._fresh_word() for _ in range(700)]
            self.bulk = [b"/".join([rng.choice(WORDS[:12]), rng.choice(new), rng.choice(new)] +
                                   ([b"+"] if rng.random() < 0.2 else [])) for _ in range(4000)]
            return [("insert", f) for f in self.bulk]
        if kind == "shrink":    # more than a quarter of the nodes and edges go
            return [("delete", f) for f in self.bulk]
        return [("insert", b"nb/r%d/n%d" % (r, i)) for i in range(5)]     # (with the scripted relayout)

    def rounds(self):
        """yields (round, kind, ops): kind "small" or a LARGE kind; the model's live set is then the
        round's"""
        for r in range(ROUNDS):
            kind = LARGE.get(r, "small")
            ops = self._small(r) if kind == "small" else self._large(r, kind)
            yield r, kind, self._apply(ops)


def fixed_topics():
    """about 1,000 topics over the vocabulary; some with out-of-domain '+' / '#' levels, some longer
    than 16 levels"""
    rng = random.Random(SEED + 2)
    ts = []
    for _ in range(900):
        t = _path(rng, rng.choice((1, 2, 3, 4, 4, 5, 6, 7)))
        if rng.random() > 0.08:     # most without wildcard levels
            t = b"/".join(w if w not in (b"+", b"#") else rng.choice(WORDS) for w in t.split(b"/"))
        ts.append(t)
    ts += [b"deep/" + b"/".join(rng.choice(WORDS[:6]) for _ in range(rng.randint(15, 21))) for _ in range(40)]
    ts += [b"$SYS/" + _path(rng, rng.randint(1, 3)).replace(b"+", b"w3").replace(b"#", b"w4") for _ in range(30)]
    ts += [b"st/p%d/s%d" % (j, i) for j in range(N_STEP) for i in range(3)] + [b"st/p%d/zz" % j for j in range(N_STEP)]
    ts += [b"hf/x%d/%s" % (j, s) for j in range(N_FLIP) for s in (b"z", b"q/y", b"z/w1/w2", b"")] + [b"hf/x0", b"", b"/"]
    ts += [b"nf/k%d/%s" % (j, s) for j in range(N_NF) for s in (b"c1", b"c13", b"c14", b"e0", b"e2", b"c99", b"c1/w1")]
    return ts


def round_topics(rng, changed, dead_words):
    """for every filter in `changed`: a topic that instantiates it ('+' a vocabulary word, '#' 0 to 2
    words) and a near miss (the last word swapped for a sibling or for a word just deleted)"""
    ts = []
    for f in changed:
        ws = []
        for w in f.split(b"/"):
            if w == b"+":
                ws.append(rng.choice(WORDS))
            elif w == b"#":
                ws += [rng.choice(WORDS) for _ in range(rng.randint(0, 2))]
            else:
                ws.append(w)
        ts.append(b"/".join(ws))
        miss = list(ws) or [b""]
        miss[-1] = rng.choice(dead_words) if dead_words and rng.random() < 0.5 else rng.choice(WORDS)
        ts.append(b"/".join(miss))
    return ts


def schedule():
    """the whole run, computed once: (base filters, [(round, kind, ops, topics)])"""
    m = Model()
    rng = random.Random(SEED + 3)
    fixed = fixed_topics()
    out, last = [], []
    for r, kind, ops in m.rounds():
        changed = list(dict.fromkeys(f for _, f in ops))
        dead = [f.rpartition(b"/")[2] for op, f in ops if op == "delete"]
        if len(changed) > 300:      # a large round: a sample walks it
            changed = rng.sample(changed, 300)
        out.append((r, kind, ops, fixed + round_topics(rng, changed + last, dead)))
        last = changed
    return m.base, out


def packed(strings):
    from emqx_amd import pack
    return pack(strings)


def read_back(eng, seen):
    """commit, compare the live device image with the host tables (tm_debug_check_device) and note
    every table's upload decision in seen: {table: set of decisions}"""
    eng.commit()
    eng.debug_check_device()
    for t, (how, _, _) in eng.debug_commit_stats().items():
        seen.setdefault(t, set()).add(how)


def hot_options(hot_edges):
    """the options that put the parents of depth < hot_edges in the `hot` edge table: the depth-based
    table does not apply under the default heat order (option "order" bit 2), so that goes too"""
    return (("hot_edges", hot_edges), ("order", 3)) if hot_edges else ()


# the trie tables of tm_debug_commit_stats whose upload decisions the churn tests pin
TRIE_TABLES = ("nodes", "edges", "hot_edges", "dict")


def check_decisions(r, kind, stats, prev_stats, hot_on, exempt=False):
    """The cap on the generator: a small round scatters (decision 1 or 2) the node table and every
    other trie table it changed, unless that table's previous commit was a whole copy (the round
    follows a regrow: the other epoch's log is `all`); a large round copies at least one whole."""
    tables = [t for t in TRIE_TABLES if t != "hot_edges" or hot_on]
    if kind == "small":
        if exempt:
            return
        for t in tables:
            how = stats[t][0]
            if prev_stats[t][0] == 3:
                continue
            assert how in (1, 2) or (how == 0 and t != "nodes"), \
                "round %d: table %s decision %d (%d scattered of %d)" % ((r, t) + stats[t])
    else:
        assert any(stats[t][0] == 3 for t in tables), "large round %d (%s): %r" % (r, kind, {t: stats[t] for t in tables})
