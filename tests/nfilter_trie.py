"""The trie and the topics of test_nfilter.py and test_gpu_nfilter.py (option
"nfilter", image.h): nodes with 7 ... 1,500 literal children -- below, at and
above the least children count of a filtered node -- under each kind of
reference the walk takes a node's filter class from:

    the root itself                      (ImageView::root_cls)
    p<c>/+      reached through a '+' edge, at once or by a pop from the path
    t/<c>n      reached through a table edge at depth 2
    $sys        reached by the '$' rule's start (walk_begin)

and topics whose word at such a node is a child, a dictionary word that is no
child, bytes in no filter, or a literal '+' / '#' level; some of more than 16
levels (the global path)."""
import random

from emqx_amd import pack

COUNTS = [7, 8, 15, 16, 17, 33, 64, 200, 1500]
ROOT_FILL = 1290
SYS_CHILDREN = 64
LONG = b"/".join([b"a"] * 18)     # 18 levels below a depth-3 node: topics of 21 levels


def filters():
    fs = []
    for c in COUNTS:
        fs += [b"p%d/+/w%d" % (c, i) for i in range(c)]
        fs += [b"t/%dn/w%d" % (c, i) for i in range(c)]
        fs += [b"p%d/lit/x" % c, b"p%d/#" % c, b"p%d/+/#" % c, b"t/%dn/#" % c, b"t/%dn/+" % c,
               b"p%d/+/w3/#" % c, b"t/%dn/w1/" % c + LONG, b"t/%dn/w2/+/y" % c]
    fs += [b"r%d" % i for i in range(ROOT_FILL)]
    fs += [b"$sys/w%d" % i for i in range(SYS_CHILDREN)] + [b"$sys/#", b"$sys/+/z"]
    fs += [b"#", b"+/#", b"+/+/#", b"+/+/+", b"t/#", b"t/+/#", b"+", b"r5/x"]
    return fs


def topics(seed=7, per=6):
    rng = random.Random(seed)
    ts = [b"r5", b"r5/x", b"r77/w1", b"nope", b"nope/w1", b"+", b"#", b"+/w1", b"w1", b"", b"/", b"t", b"t/nope",
          b"t/+/w1", b"t/#", b"$sys", b"$sys/nope", b"$sys/+", b"$sys/#", b"$nope/w1", b"$sys/w1/z", b"$sys/r3"]
    ts += [b"$sys/w%d" % rng.randrange(SYS_CHILDREN + 40) for _ in range(4 * per)]
    for c in COUNTS:
        def words():
            child = [b"w%d" % rng.randrange(c) for _ in range(per)]
            absent = [b"w%d" % (c + rng.randrange(1500 - c + 20)) for _ in range(per)] + [b"r%d" % rng.randrange(ROOT_FILL)
                                                                                         for _ in range(per)]
            return child + absent + [b"nope", b"zz%d" % rng.randrange(99), b"+", b"#", b"", b"w3", b"w1", b"w2"]
        for w in words():
            ts.append(b"p%d/zz/%s" % (c, w))        # '+' edge taken at once (bytes in no filter)
        for w in words():
            ts.append(b"p%d/w1/%s" % (c, w))        # '+' edge taken at once (a dictionary word, no child)
        for w in words():
            ts.append(b"p%d/lit/%s" % (c, w))       # '+' edge taken by a pop from the path
        for w in words():
            ts.append(b"t/%dn/%s" % (c, w))         # table edge
        for w in words()[:per]:
            ts.append(b"p%d/lit/%s/x/y" % (c, w))
            ts.append(b"t/%dn/%s/q/y" % (c, w))
        # more than 16 levels: through a filtered node, matching and not
        ts += [b"t/%dn/w1/" % c + LONG, b"t/%dn/w1/" % c + LONG + b"/a", b"t/%dn/w4/" % c + LONG,
               b"p%d/lit/w3/" % c + LONG, b"p%d/zz/w5/" % c + LONG, b"p%d/lit/nope/" % c + LONG]
    assert len(ts) <= 4096
    return ts


def churn_adds():
    """50 new children under a filtered node of each kind and under unfiltered ones"""
    fs = []
    for k in range(50):
        fs += [b"p64/+/n%d" % k, b"p7/+/n%d" % k, b"t/200n/n%d" % k, b"t/8n/n%d" % k, b"n%d" % k, b"$sys/n%d" % k]
    return fs


def churn_dels():
    """children of filtered and unfiltered nodes (their bits stay set)"""
    return [b"p64/+/w%d" % i for i in range(0, 64, 3)] + [b"p1500/+/w%d" % i for i in range(0, 1500, 2)] + \
           [b"t/33n/w%d" % i for i in range(5, 33)] + [b"p8/+/w%d" % i for i in range(8)] + \
           [b"r%d" % i for i in range(100, 400)]


def churn_topics():
    ts = []
    for k in range(0, 60, 7):
        ts += [b"p64/zz/n%d" % k, b"p64/lit/n%d" % k, b"p7/zz/n%d" % k, b"t/200n/n%d" % k, b"t/8n/n%d" % k,
               b"n%d" % k, b"$sys/n%d" % k]
    return ts


def packed(xs):
    return pack(list(xs))
