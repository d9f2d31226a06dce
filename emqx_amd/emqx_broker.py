"""emqx_broker — the subscriber bag and publish/1's local dispatch
(src/emqx_broker.erl), same names and semantics, backed by the MI355X engine:
the emqx_subscriber duplicate_bag lives in the engine (tm_sub_add / tm_sub_del,
subscribers/1) and publish/1 runs on the GPU end to end (trie walk, route
expansion, aggre and the subscriber fan-out, dispatch.hip).

    subscribe(Topic, Sub[, Group])     handle_cast #subscribe :332-345: insert_subscriber/3
                                       :398-405, then emqx_router:add_route(Topic, dest(Group));
                                       with opts: do_subscribe/4 :407-410, the emqx_suboption entry
    get_subopts / set_subopts          :279-291 over the entries the engine keeps (qos, nl, rap, subid)
    unsubscribe(Topic, Sub[, Group])   handle_cast #unsubscribe :347-358: delete_object :414,
                                       then del_route when ets:member(?SUBSCRIBER, Topic) is false
    subscribers(Topic)                 :245-247 -> [Sub | {share, Group, Sub}] in bag order
    publish_many(Topics[, Msgs])       publish/1 :148-157 per topic: route(aggre(match_routes(T)));
                                       with msgs, every pair with the outcome of the session's
                                       handle_dispatch/3 (src/emqx_session.erl:667-684, 797-819)
    publish_shared_many(Topics, ...)   the same with route/2's $share clause :187-189: the member
                                       emqx_shared_sub:dispatch/3 picks for every {To, Group} delivery
    publish_admitted_many(...)         the same behind emqx_packet:validate/1, check_pub_caps and
                                       check_pub_acl (src/emqx_protocol.erl:769-794): the codes, and
                                       the admitted publishes' results; a refused one leaves no trace
    dispatch_many(Tos)                 dispatch/2 :218-238 as a remote node's forward/3 calls it
    publish_forward_many(Topics)       publish_many plus route/2's {To, Node} clause :185-186: the
                                       batch's forward/3 calls :209-216 as one bundle per remote node
    dispatch_forwarded(Groups, Topics) the receiving node's side of such a bundle: one dispatch_many

A subscriber is a u32 chosen by the caller (the NIF keeps id <-> {SubPid,
SubId}); groups are byte strings.  The counterpart of emqx_router.py.
"""
from collections import namedtuple

from .emqx_router import Router, _key
from .emqx_shared_sub import STRATEGIES, SharedSub
from .engine import Engine, pack

# one delivery of publish/1: target = (kind, key) as Router.match_deliveries_many
# tags it; count = the Count of {dispatch, To, Count}, 0 = message.dropped, None =
# not the local node's (a forward or a $share delivery, left to the caller)
Delivery = namedtuple("Delivery", "to target count")
Published = namedtuple("Published", "deliveries pairs")


class SharedPublished(Published):
    """a Published (the same two fields, equal to the plain one) with .picks:
    [(To, Group, member | None)] of the $share deliveries in delivery order,
    None = do_pick/5's `false`; and, for a publish with its message,
    .pick_deliver parallel to .picks: what the picked member's session makes of
    the message -- False without a member, None = dropped by no-local, else
    (qos, retain, subid | None)"""

    def __new__(cls, deliveries, pairs, picks, pick_deliver=None):
        self = super().__new__(cls, deliveries, pairs)
        self.picks = picks
        self.pick_deliver = pick_deliver
        return self


def pack_subopts(opts) -> int:
    """{qos, nl, rap, subid} (missing keys: ?DEFAULT_SUBOPTS, no subid) -> the engine's option word"""
    qos, subid = int(opts.get("qos", 0)), opts.get("subid")
    if qos not in (0, 1, 2) or not (subid is None or 1 <= int(subid) < (1 << 28)):
        raise ValueError("subopts: qos 0..2, subid 1..2^28-1")
    return (qos | (Engine.SUBOPT_NL if opts.get("nl") else 0) | (Engine.SUBOPT_RAP if opts.get("rap") else 0)
            | (int(subid or 0) << 4))


def unpack_subopts(word: int):
    return {"qos": word & 3, "nl": (word >> 2) & 1, "rap": (word >> 3) & 1, "subid": (word >> 4) or None}


def pack_msgs(msgs):
    """[(qos, retain, retained, from_sub | None)] -> (pub_flags, pub_from)"""
    pf = [int(q) | (Engine.MSG_RETAIN if r else 0) | (Engine.MSG_RETAINED if rd else 0) for q, r, rd, _ in msgs]
    fr = [Engine.NO_SUBSCRIBER if f is None else int(f) for _, _, _, f in msgs]
    return pf, fr


def unpack_deliver(word: int):
    """a delivery word -> None (dropped by no-local) or (qos, retain, subid | None)"""
    if word & Engine.DELIVER_DROP:
        return None
    return (word & 3, (word >> 2) & 1, (word >> 4) or None)


class Broker:
    def __init__(self, engine: Engine, router: Router):
        self.engine = engine
        self.router = router
        self.shared = SharedSub(engine)
        engine.set_local_node(_key(router.node))

    def _dest(self, group):
        # dest(undefined) -> node(); dest(Group) -> {Group, node()}   (:444-445)
        return self.router.node if group is None else (group, self.router.node)

    # handle_cast({From, #subscribe{}}) — :332-345
    # opts {qos, nl, rap, subid}: do_subscribe/4 :407-410 (the emqx_suboption
    # entry, written even when the bag already held the plain entry); None:
    # insert_subscriber/3 alone, no entry
    def subscribe(self, topic: bytes, sub: int, group=None, opts=None):
        g = None if group is None else _key(group)
        if opts is None:
            self.engine.sub_add(topic, sub, g)
        else:
            self.engine.sub_add_opts(topic, sub, pack_subopts(opts), g)
        self.shared.subscribe(group, topic, sub)          # :394
        self.router.add_route(topic, self._dest(group))
        return "ok"

    # handle_cast({From, #unsubscribe{}}) — :347-358
    def unsubscribe(self, topic: bytes, sub: int, group=None):
        left = self.engine.sub_del(topic, sub, None if group is None else _key(group))
        self.shared.unsubscribe(group, topic, sub)        # :353
        if left == 0:                      # ets:member(?SUBSCRIBER, Topic) -> false
            self.router.del_route(topic, self._dest(group))
        return "ok"

    # get_subopts/2 — :279-283 ([] -> None)
    def get_subopts(self, topic: bytes, sub: int):
        w = self.engine.sub_get_opts(topic, sub)
        return None if w is None else unpack_subopts(w)

    # set_subopts/3 — :285-291: maps:merge over the keys given; False without an entry
    def set_subopts(self, topic: bytes, sub: int, opts) -> bool:
        mask = value = 0
        if "qos" in opts:
            mask, value = mask | 3, value | pack_subopts({"qos": opts["qos"]})
        if "nl" in opts:
            mask, value = mask | Engine.SUBOPT_NL, value | (Engine.SUBOPT_NL if opts["nl"] else 0)
        if "rap" in opts:
            mask, value = mask | Engine.SUBOPT_RAP, value | (Engine.SUBOPT_RAP if opts["rap"] else 0)
        if "subid" in opts:
            mask, value = mask | 0xFFFFFFF0, value | (pack_subopts({"subid": opts["subid"]}) & 0xFFFFFFF0)
        return self.engine.sub_set_opts(topic, sub, mask, value)

    @staticmethod
    def _deliver(msgs, n, upgrade_qos):
        if msgs is None:
            return None
        msgs = list(msgs)
        if len(msgs) != n:
            raise ValueError("msgs: one (qos, retain, retained, from_sub) per entry")
        pf, fr = pack_msgs(msgs)
        return pf, fr, Engine.DELIVER_UPGRADE_QOS if upgrade_qos else 0

    # subscribers/1 — :245-247
    def subscribers(self, topic: bytes):
        names = {}
        out = []
        for sub, g in self.engine.subscribers(topic):
            if g == Engine.NO_GROUP:
                out.append(sub)
            else:
                if g not in names:
                    names[g] = self.engine.sub_group_bytes(g)
                out.append(("share", names[g], sub))
        return out

    # publish/1 — :148-157
    def publish(self, topic: bytes):
        return self.publish_many([topic])[0]

    def publish_many(self, topics, msgs=None, upgrade_qos=False):
        """one device batch for all topics -> [Published(deliveries, pairs)]:
        deliveries in aggre's order, pairs = [(To, Sub)] in dispatch order.
        msgs[i] = (qos, retain, retained, from_sub | None) of publish i: pairs =
        [(To, Sub, None | (qos, retain, subid | None))], None = dropped by
        no-local; upgrade_qos: the sessions' zone setting, for the whole batch"""
        topics = list(topics)
        buf, off = pack(topics)
        dv = self._deliver(msgs, len(topics), upgrade_qos)
        out = self.engine.match_dispatch_batch(buf, off, deliver=dv)
        return self._published(topics, out[:9], None, out[9] if dv else None)

    def publish_shared_many(self, topics, strategy=None, keys=None, msgs=None, upgrade_qos=False):
        """publish_many with the $share clause: Published.picks = [(To, Group,
        member | None)] per $share delivery.  strategy: "round_robin", or
        "hash" / "random" / "keyed" / "sticky" with keys = one u32 per topic
        (erlang:phash2(ClientId), or a uniform draw); default: self.shared.strategy.
        msgs / upgrade_qos: as publish_many; the picks then come with
        .pick_deliver, from the device's pick words (tm_share_pick_words).  The
        one case the device does not answer -- a stuck member that left its set
        -- is looked up here (get_subopts/2 + tm_deliver_word)"""
        topics = list(topics)
        buf, off = pack(topics)
        dv = self._deliver(msgs, len(topics), upgrade_qos)
        out = self.engine.match_publish_batch(buf, off, STRATEGIES[strategy or self.shared.strategy], keys,
                                              deliver=dv, pick_words=dv is not None)
        return self._published(topics, out[:9], out[9], out[10] if dv else None, out[11] if dv else None, dv)

    # emqx_protocol:process_packet's validate + check_publish in front of do_publish — src/emqx_protocol.erl:217, 769-794
    def publish_admitted_many(self, topics, creds, msgs, zones, acl=None, mounts=None, admit=None, strategy=None,
                              keys=None, upgrade_qos=False, cursors=None):
        """publish_shared_many behind the admission checks, as one chain on one
        stream without a wait between its calls: ACL check (tm_acl_check_batch_device
        on the unmounted topics) -> tm_admit_batch_device -> tm_publish_stream_gated_device.
        topics[i] = MountPoint ++ T and mounts[i] the mountpoint's length (None:
        0); creds[i] a credentials dict as emqx_access.AclRules takes it; msgs
        as publish_many's (the QoS and retain bit feed the caps); zones an
        emqx_access.Zones; admit[i] = (zone index, is_super, alias | None)
        (None: zone 0, not super, no alias); acl an AclRules on this engine's
        device (None: every check is nomatch); cursors: the publisher's
        ShareCursors (None: the replica's built-in array).  -> (codes, rules, published):
        codes[i] the TM_ADMIT_* code, rules[i] the index of the ACL rule that
        matched (None without one), published[i] what publish_shared_many
        returns for an admitted publish and None for a refused one, which
        reached no cursor and no sticky entry."""
        import numpy as np
        import torch

        from . import _lib as L
        from .emqx_access import AclRules, pub_admit
        topics = list(topics)
        n = len(topics)
        dv = self._deliver(msgs, n, upgrade_qos)
        if dv is None or len(creds) != n:
            raise ValueError("one message and one credentials dict per publish")
        if n == 0:
            return [], [], []
        e, dev = self.engine, torch.device("cuda", self.engine.device)
        st = torch.cuda.current_stream(dev)
        signed = {1: np.int8, 4: np.int32, 8: np.int64}

        def up(a):
            a = np.ascontiguousarray(a)
            return torch.from_numpy(a.view(signed[a.dtype.itemsize]).copy() if a.dtype.kind == "u" and
                                    a.dtype.itemsize > 1 else a.copy()).to(dev)

        def zeros(k, dt):
            return torch.zeros(max(int(k), 1), dtype=dt, device=dev)
        mounts = [0] * n if mounts is None else [int(m) for m in mounts]
        admit = [(0, False, None)] * n if admit is None else list(admit)
        buf, off = pack(topics)
        d_b, d_o = up(buf), up(off)
        d_ml, d_pf, d_fr = up(np.asarray(mounts, np.uint32)), up(np.asarray(dv[0], np.uint32)), \
            up(np.asarray(dv[1], np.uint32))
        d_pa = up(np.asarray([pub_admit(*a) for a in admit], np.uint32))
        d_acl, d_rule = None, zeros(n, torch.int32)
        d_code, d_ahdr = zeros(n, torch.uint8), zeros(8, torch.int64)
        if acl is not None:
            # the ACL sees T unmounted: the topics' own CSR unless some publish has a mountpoint
            packed = AclRules.pack(creds, ["publish"] * n, [t[m:] for t, m in zip(topics, mounts)] if any(mounts) else None)
            d = {k: up(v) for k, v in packed.items() if v is not None}
            d.setdefault("topics", d_b)
            d.setdefault("topic_off", d_o)
            d_acl = zeros(n, torch.int8)
            acl.check_device(n, d, d_acl, d_rule, stream=st)
        Engine.admit_batch_device(d_b, d_o, n, d_ml, d_pf, d_pa, zones, d_acl, d_code, d_ahdr, stream=st)
        s = STRATEGIES[strategy or self.shared.strategy]
        d_k = None if keys is None else up(np.asarray(keys, np.uint32))
        caps = [max(64, 4 * n)] * 4
        nbytes = int(off[-1] - off[0])
        doff, soff, hdr = zeros(n + 1, torch.int64), zeros(n + 1, torch.int64), zeros(L.TM_PUBLISH_HDR_WORDS, torch.int64)
        while True:
            wsb = e.publish_stream_opts_workspace_bytes(n, nbytes, caps)
            ws = zeros(wsb, torch.uint8)
            deliv, pairs = zeros(4 * caps[1], torch.int32), zeros(2 * caps[2], torch.int32)
            pkw, prw = zeros(caps[1], torch.int32), zeros(caps[2], torch.int32)
            e.publish_stream_gated_device(d_b, d_o, n, nbytes, s, d_k, cursors, caps, ws, wsb, hdr, doff, soff, deliv,
                                          pairs, (d_pf, d_fr, dv[2], prw), pkw, d_code, stream=st)
            st.synchronize()
            h = [int(x) for x in hdr.cpu().numpy().view(np.uint64)]
            if h[6] == 0:
                break
            # the stage named did not fit and no cursor moved: the totals up to it are exact, so each of
            # those capacities grows to its need (and a quarter), the later ones stay, and the call runs again
            need = (h[4], h[0], h[1], h[5])
            caps = [max(c, x + x // 4 + 64) if i < h[6] else c for i, (c, x) in enumerate(zip(caps, need))]
        u32 = lambda t: t.cpu().numpy().view(np.uint32)      # noqa: E731
        u64 = lambda t: t.cpu().numpy().view(np.uint64)      # noqa: E731
        code = d_code.cpu().numpy()
        rule = u32(d_rule) if acl is not None else np.full(n, 0xFFFFFFFF, np.uint32)
        doff, soff = u64(doff), u64(soff)
        rec, pr = u32(deliv).reshape(-1, 4), u32(pairs).reshape(-1, 2)
        planes = ((doff[1:] - doff[:-1]).astype(np.uint32), doff[:-1], rec[:, 0], rec[:, 1], rec[:, 2],
                  (soff[1:] - soff[:-1]).astype(np.uint32), soff[:-1], pr[:, 0], pr[:, 1])
        res = self._published(topics, planes, rec[:, 3], u32(prw), u32(pkw), dv)
        return ([int(c) for c in code], [None if int(r) == 0xFFFFFFFF else int(r) for r in rule[:n]],
                [None if code[t] else res[t] for t in range(n)])

    def _pick_deliver(self, to, member, word, t, dv):
        if member == Engine.NO_MEMBER:
            return False
        if word == Engine.NO_WORD:                       # the caller's fallback
            opts = self.engine.sub_get_opts(to, member)
            pf, fr, fl = dv
            word = self.engine.deliver_word(Engine.SUBOPT_NONE if opts is None else opts, int(pf[t]),
                                            int(fr[t]) != Engine.NO_SUBSCRIBER and int(fr[t]) == member, fl)
        return unpack_deliver(word)

    def _published(self, topics, out, pick, words=None, pick_words=None, dv=None):
        counts, offs, to, tg, nd, scount, soff, sto, sid = out
        names, tnames, res = {}, {}, []

        def name_of(s, topic):
            if s == Engine.TOPIC_ROUTE:
                return topic
            if s not in names:
                names[s] = self.engine.filter_bytes(s)
            return names[s]

        for t, topic in enumerate(topics):
            dels = []
            picks = None if pick is None else []
            pdv = None if pick_words is None else []
            for k in range(int(offs[t]), int(offs[t]) + int(counts[t])):
                g = int(tg[k])
                if g not in tnames:
                    tnames[g] = self.engine.target_bytes(g)
                c = int(nd[k])
                dels.append(Delivery(name_of(int(to[k]), topic), tnames[g], None if c == Engine.NOT_LOCAL else c))
                if pick is not None and tnames[g][0] == Engine.TARGET_GROUP:
                    m = int(pick[k])
                    picks.append((dels[-1].to, tnames[g][1], None if m == Engine.NO_MEMBER else m))
                    if pdv is not None:
                        pdv.append(self._pick_deliver(dels[-1].to, m, int(pick_words[k]), t, dv))
            a = int(soff[t])
            pairs = [(name_of(int(sto[k]), topic), int(sid[k])) for k in range(a, a + int(scount[t]))]
            if words is not None:
                pairs = [pr + (unpack_deliver(int(words[a + k])),) for k, pr in enumerate(pairs)]
            res.append(Published(dels, pairs) if pick is None else SharedPublished(dels, pairs, picks, pdv))
        return res

    # route/2's {To, Node} clause and forward/3 — :185-186, :209-216
    def publish_forward_many(self, topics):
        """publish_many plus the batch's forwards, one bundle per remote node ->
        ([Published], forwards); forwards = [(node bytes, [(To bytes | None,
        [publish index, ...]), ...])] ordered as the plan is (tm_forward_plan:
        target id, then To, then publish index).  To None = each of the named
        publishes' own topic.  A bundle's second field is what the node's
        Broker.dispatch_forwarded takes."""
        topics = list(topics)
        buf, off = pack(topics)
        out = self.engine.match_dispatch_batch(buf, off)
        _hdr, groups, pub = self.engine.forward_plan(out[0], out[1], out[2], out[3])
        ids = [int(g[1]) for g in groups if int(g[1]) != Engine.TOPIC_ROUTE]
        names = dict(zip(ids, self.engine.filters_bytes(ids))) if ids else {}
        forwards = []
        last = None
        for node, to, first, count in groups.tolist():
            if node != last:
                forwards.append((self.engine.target_bytes(node)[1], []))
                last = node
            forwards[-1][1].append((None if to == Engine.TOPIC_ROUTE else names[to],
                                    [int(x) for x in pub[first:first + count]]))
        return self._published(topics, out, None), forwards

    # dispatch/2's SubPid ! {dispatch, Topic, Msg} and the $share send — :225-236, emqx_shared_sub:121-140
    def publish_inbox_many(self, topics, msgs=None, strategy=None, keys=None, upgrade_qos=False):
        """the batch's local sends, one bundle per receiving subscriber ->
        {subscriber: [(publish index, To bytes | None, word | None, is_pick)]}
        ordered as the plan is (tm_inbox_plan: publish index, a publish's plain
        sends before its $share picks, then position).  To None = the publish's
        own topic.  msgs / upgrade_qos: as publish_many; word is then the
        delivery word (tm_deliver_word's layout) and the sends no-local drops
        are left out; without msgs word is None.  strategy / keys: as
        publish_shared_many.  The one word the device does not answer -- a
        stuck member that left its set -- is looked up here."""
        topics = list(topics)
        buf, off = pack(topics)
        dv = self._deliver(msgs, len(topics), upgrade_qos)
        out = self.engine.match_publish_batch(buf, off, STRATEGIES[strategy or self.shared.strategy], keys,
                                              deliver=dv, pick_words=dv is not None)
        _hdr, inbox, ent_pub, ent_to, ent_word = self.engine.inbox_plan(
            out[6], out[7], out[8], out[10] if dv else None, out[0], out[1], out[2], out[9],
            out[11] if dv else None)
        ids = sorted({int(x) for x in ent_to.tolist()} - {Engine.TOPIC_ROUTE})
        names = dict(zip(ids, self.engine.filters_bytes(ids))) if ids else {}
        res = {}
        for sub, first, count, _picks in inbox.tolist():
            ents = []
            for e in range(first, first + count):
                t, is_pick = int(ent_pub[e]) & ~Engine.INBOX_PICK, bool(int(ent_pub[e]) & Engine.INBOX_PICK)
                to = int(ent_to[e])
                word = None if dv is None else int(ent_word[e])
                if word == Engine.NO_WORD:               # the caller's fallback
                    opts = self.engine.sub_get_opts(topics[t] if to == Engine.TOPIC_ROUTE else names[to], sub)
                    pf, fr, fl = dv
                    word = self.engine.deliver_word(Engine.SUBOPT_NONE if opts is None else opts, int(pf[t]),
                                                    int(fr[t]) != Engine.NO_SUBSCRIBER and int(fr[t]) == sub, fl)
                    if word == Engine.DELIVER_DROP:
                        continue
                ents.append((t, None if to == Engine.TOPIC_ROUTE else names[to], word, is_pick))
            if ents:
                res[sub] = ents
        return res

    def dispatch_forwarded(self, groups, topics):
        """the receiving end of forward/3 (the RPC replaced by a call): groups =
        one bundle of publish_forward_many, topics = that batch's topics (a
        forwarded message carries its own) -> [(publish index, To, Count,
        [Sub])] in bundle order, from one dispatch_many call"""
        tos, rows = [], []
        for to, pubs in groups:
            if to is None:
                for p in pubs:
                    rows.append((p, len(tos)))
                    tos.append(topics[p])
            else:
                rows.extend((p, len(tos)) for p in pubs)
                tos.append(to)
        res = self.dispatch_many(tos) if tos else []
        return [(p, tos[i], res[i][0], list(res[i][1])) for p, i in rows]

    # dispatch/2 — :218-238
    def dispatch_many(self, tos, msgs=None, upgrade_qos=False):
        """[(Count, [Sub])] per To (given by its bytes): Count counts shared
        entries too, the list holds the plain subscribers in bag order.
        msgs[i] = the message forwarded with To i, as publish_many's (a To may
        be listed once per message): the lists hold (Sub, None | (qos, retain,
        subid | None))"""
        tos = list(tos)
        buf, off = pack(tos)
        dv = self._deliver(msgs, len(tos), upgrade_qos)
        if dv is None:
            nd, soff, sid = self.engine.dispatch_batch(buf, off)
            return [(int(nd[i]), [int(x) for x in sid[int(soff[i]):int(soff[i + 1])]]) for i in range(len(tos))]
        nd, soff, sid, words = self.engine.dispatch_batch(buf, off, deliver=dv)
        return [(int(nd[i]), [(int(sid[k]), unpack_deliver(int(words[k])))
                              for k in range(int(soff[i]), int(soff[i + 1]))]) for i in range(len(tos))]
