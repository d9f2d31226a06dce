"""TEST ORACLE for the inbox plan (include/topicmatch.h tm_inbox_plan): our own
Python, in three parts.

    expected_plan      the plan of a list of sends, by sorted() over (sub, pub,
                       kind, pos): header, subscriber records and entry planes
                       exactly as the contract states them
    sends_of_planes    the send definition applied to host planes: dropped
                       words, TM_NO_MEMBER, holes, the capacity bounds
    reference_sends    the sends of a batch from the restatements beside this
                       file, per publish:
                         subopts_ref.route_dispatch_opts  the plain subscribers of every local
                                                          delivery (dispatch_ref.dispatch) with
                                                          what each session makes of the message
                         pickword_ref.route_pick_words    the picked member of every $share
                                                          delivery (shared_ref / sticky_ref) with
                                                          the same
                       grouped per subscriber

A send is (sub, pub, kind, pos, to, word): kind 0 = pair send, 1 = pick send;
pos = the pair index p or the delivery slot s (for reference_sends, the ordinal
within the publish, which orders the same way); word None = no word reported.

The one deviation from the reference (a publish's pairs before its picks, not
interleaved by delivery slot) is the contract's, so it is this oracle's too.
"""
from pickword_ref import outcome_word, route_pick_words
from shared_ref import NO_MEMBER as REF_NO_MEMBER
from subopts_ref import route_dispatch_opts

NO_MEMBER = 0xFFFFFFFF
NO_WORD = 0xFFFFFFFF
DROP = 8
PICK = 0x80000000
ROUTE_TOPIC = 0xFFFFFFFF


def expected_plan(sends):
    """-> (hdr [E, S, pairs, picks], inbox [(sub, first, count, picks)],
    ent_pub, ent_to, ent_word); ent_pub carries PICK on a pick send, a send
    without a word has ent_word 0"""
    rows = sorted(sends, key=lambda s: (s[0], s[1], s[2], s[3]))
    inbox = []
    for i, (sub, _pub, kind, _pos, _to, _word) in enumerate(rows):
        if not inbox or inbox[-1][0] != sub:
            inbox.append([sub, i, 0, 0])
        inbox[-1][2] += 1
        inbox[-1][3] += kind
    picks = sum(s[2] for s in rows)
    hdr = [len(rows), len(inbox), len(rows) - picks, picks]
    ent_pub = [pub | (PICK if kind else 0) for _s, pub, kind, _p, _t, _w in rows]
    ent_to = [to for _s, _pub, _k, _p, to, _w in rows]
    ent_word = [0 if word is None else word for _s, _pub, _k, _p, _t, word in rows]
    return hdr, [tuple(r) for r in inbox], ent_pub, ent_to, ent_word


def sends_of_planes(sub_off, sub_to, sub_id, sub_word=None, counts=None, offs=None, to=None, pick=None,
                    pick_word=None, sub_total=None, sub_cap=None, total=None, out_cap=None):
    """the sends of host planes; totals / capacities default to the planes' lengths"""
    n = len(sub_off) - 1
    plen = 0 if sub_id is None else len(sub_id)
    pbound = min(plen if sub_total is None else sub_total, plen if sub_cap is None else sub_cap)
    sends = []
    for t in range(n):
        for p in range(int(sub_off[t]), int(sub_off[t + 1])):
            if p >= pbound:
                continue                                       # at or past min(sub_total, sub_cap)
            word = None if sub_word is None else int(sub_word[p])
            if word == DROP:
                continue
            sends.append((int(sub_id[p]), t, 0, p, int(sub_to[p]), word))
    if pick is None:
        return sends
    kbound = min(len(pick) if total is None else total, len(pick) if out_cap is None else out_cap)
    for t in range(n):
        for k in range(int(counts[t])):                       # the live slots: a hole is past count[t]
            s = int(offs[t]) + k
            if s >= int(offs[t + 1]) or s >= kbound or int(pick[s]) == NO_MEMBER:
                continue
            word = None if pick_word is None else int(pick_word[s])
            if word == DROP:
                continue                                       # NO_WORD is kept
            sends.append((int(pick[s]), t, 1, s, int(to[s]), word))
    return sends


def reference_sends(table, subopts, shared, node, strategy, pubs, upgrade=False, words=True):
    """pubs = [(topic, key, msg)] -> the batch's sends with To as bytes and the
    word as the engine packs it (pickword_ref.outcome_word); the picks advance
    `shared` (a sticky_ref.StickySub) as the device's do"""
    sends = []
    for t, (topic, key, msg) in enumerate(pubs):
        _counts, pairs = route_dispatch_opts(table, subopts, node, topic, msg, upgrade)
        for p, (to, s, oc) in enumerate(pairs):
            if words and oc is None:
                continue                                       # dropped by no-local
            sends.append((s, t, 0, p, to, outcome_word(oc) if words else None))
        rows = route_pick_words(table, shared, subopts, strategy, int(key), topic, msg, upgrade)
        for k, ((to, _x), (m, oc)) in enumerate(zip(table.match_deliveries(topic), rows)):
            if m is REF_NO_MEMBER or m is None:
                continue
            if words and oc is None:
                continue
            sends.append((m, t, 1, k, to, outcome_word(oc) if words else None))
    return sends


def grouped(sends):
    """{sub: [(pub, to, word, is_pick)]} in plan order"""
    out = {}
    for sub, pub, kind, _pos, to, word in sorted(sends, key=lambda s: (s[0], s[1], s[2], s[3])):
        out.setdefault(sub, []).append((pub, to, word, bool(kind)))
    return out


def grouped_plan(inbox, ent_pub, ent_to, ent_word, to_bytes):
    """a plan in the shape of grouped(); to_bytes(to id, publish index) names a To"""
    out = {}
    for sub, first, count, _picks in inbox:
        rows = []
        for e in range(int(first), int(first) + int(count)):
            pub = int(ent_pub[e]) & ~PICK
            rows.append((pub, to_bytes(int(ent_to[e]), pub), None if ent_word is None else int(ent_word[e]),
                         bool(int(ent_pub[e]) & PICK)))
        out[int(sub)] = rows
    return out
