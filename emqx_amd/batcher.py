"""Publish micro-batcher (include/topicmatch.h tm_batcher_*).

Many publisher threads submit single topics; the native worker thread seals
device batches (by size or deadline) and calls back once per topic with its
ordered match list (emqx_trie:match/1 filter ids), its match_routes/1
routes, or (deliveries=True) aggre(match_routes/1): To ids + target ids, or
(publish=True, submit_publish) publish/1 up to the sends: the deliveries with
their dispatch Count and $share pick, and the (To, subscriber) pairs; with
round_robin=True the picks are the reference's default strategy, each lane a
publisher process with its own cursors (sticky=True: `sticky` picks, a lane
likewise a publisher with its own entries); every publish batcher runs the
stream-ordered publish call, and stream=True (TM_BATCHER_STREAM, which once
chose that call for the keyed picks) is accepted and changes nothing; opts=True
(submit_publish_opts) brings the delivery word of every pair and of every
$share pick with the records; inbox=callable (with publish=True, opts=True)
opens the inbox mode (tm_batcher_open_inbox): per batch the callable gets the
batch's local sends grouped per receiving session before the per-publish
callbacks run, which then carry no pairs; forward=callable (with publish=True;
tm_batcher_open_plans, combines with inbox=) likewise hands over the batch's
remote-node deliveries grouped per (node, To), after the inbox callback and
before the per-publish callbacks, which are unchanged; admit=(zones, acl)
(with publish=True, opts=True; tm_batcher_open_admit, combines with all of the
above) puts the admission stage in front: submit_publish_admit carries the
publish's mount length, admission word and credentials, a lane runs the ACL
check, the admission and the gated publish call on its stream, and every
callback ends with the publish's admission code and ACL rule index.  This is the NIF's path: the callback there builds
the Erlang list and enif_send()s it to the waiting process."""
import ctypes
import itertools

import numpy as np

from . import _lib as L


class Batcher:
    def __init__(self, engine, max_topics=65536, deadline_us=200, max_bytes=0, routes=False, deliveries=False,
                 lanes_per_replica=0, callback_threads=0, publish=False, eager=False, flags=0, round_robin=False,
                 stream=False, sticky=False, opts=False, upgrade_qos=False, inbox=None, forward=None, admit=None):
        self.engine = engine
        self.lib = engine.lib
        flags |= (L.TM_BATCHER_ROUTES if routes else 0) | (L.TM_BATCHER_DELIVERIES if deliveries else 0) | \
            (L.TM_BATCHER_PUBLISH if publish else 0) | (L.TM_BATCHER_EAGER if eager else 0) | \
            (L.TM_BATCHER_ROUND_ROBIN if round_robin else 0) | (L.TM_BATCHER_STREAM if stream else 0) | \
            (L.TM_BATCHER_STICKY if sticky else 0) | (L.TM_BATCHER_OPTS if opts else 0) | \
            (L.TM_BATCHER_UPGRADE_QOS if upgrade_qos else 0) | (L.TM_BATCHER_INBOX if inbox is not None else 0) | \
            (L.TM_BATCHER_FORWARD if forward is not None else 0) | (L.TM_BATCHER_ADMIT if admit is not None else 0)
        cfg = L.TmBatcherConfig(max_topics, deadline_us, max_bytes, flags, lanes_per_replica, callback_threads)
        h = ctypes.c_void_p()
        self.inbox = inbox
        self.forward = forward
        self.admit = admit
        if admit is not None:
            # admit = (Zones, acl): acl None, one AclRules, or one per replica; kept alive with the batcher
            what = "tm_batcher_open_admit"
            zones, acl = admit
            self._ztab, nz = zones.table()
            acls = [] if acl is None else list(acl) if isinstance(acl, (list, tuple)) else [acl]
            self._acls = acls
            self._aclv = (ctypes.c_void_p * max(len(acls), 1))(*[a.h for a in acls])
            ac = L.TmAdmitConfig(self._ztab, nz, len(acls), self._aclv if acls else None)
            self._idone = L.INBOX_DONE_FN(self._on_inbox_done) if inbox is not None else \
                ctypes.cast(None, L.INBOX_DONE_FN)
            self._fdone = L.FORWARD_DONE_FN(self._on_forward_done) if forward is not None else \
                ctypes.cast(None, L.FORWARD_DONE_FN)
            rc = self.lib.tm_batcher_open_admit(engine.h, ctypes.byref(cfg), ctypes.byref(ac), self._idone,
                                                self._fdone, None, ctypes.byref(h))
        elif forward is not None:
            what = "tm_batcher_open_plans"
            self._idone = L.INBOX_DONE_FN(self._on_inbox_done) if inbox is not None else \
                ctypes.cast(None, L.INBOX_DONE_FN)
            self._fdone = L.FORWARD_DONE_FN(self._on_forward_done)   # kept alive with the batcher
            rc = self.lib.tm_batcher_open_plans(engine.h, ctypes.byref(cfg), self._idone, self._fdone, None,
                                                ctypes.byref(h))
        elif inbox is not None:
            what = "tm_batcher_open_inbox"
            self._idone = L.INBOX_DONE_FN(self._on_inbox_done)   # kept alive with the batcher
            rc = self.lib.tm_batcher_open_inbox(engine.h, ctypes.byref(cfg), self._idone, None, ctypes.byref(h))
        else:
            what = "tm_batcher_open"
            rc = self.lib.tm_batcher_open(engine.h, ctypes.byref(cfg), ctypes.byref(h))
        if rc != L.TM_OK:
            raise L.TopicMatchError(rc, what)
        self.h = h
        self.routes = routes
        self._cbs = {}
        self._keys = itertools.count(1)
        self._done = L.DONE_FN(self._on_done)     # one trampoline, kept alive with the batcher
        self._pdone = L.PUBLISH_DONE_FN(self._on_publish_done)
        self._odone = L.PUBLISH_OPTS_DONE_FN(self._on_publish_opts_done)
        self._adone = L.PUBLISH_ADMIT_DONE_FN(self._on_publish_admit_done)

    def _on_done(self, ctx, ticket, status, ids, dests, n):
        cb = self._cbs.pop(ctx)
        if status != L.TM_OK:
            cb(status, None, None)
            return
        a = [ids[i] for i in range(n)]
        d = [dests[i] for i in range(n)] if dests else None
        cb(status, a, d)

    def submit(self, topic: bytes, callback):
        """callback(status, ids, dests) runs on the worker thread"""
        t = ctypes.c_uint64()
        key = next(self._keys)              # the callback may fire before submit returns
        self._cbs[key] = callback
        rc = self.lib.tm_batcher_submit(self.h, topic, len(topic), self._done, key, ctypes.byref(t))
        if rc != L.TM_OK:
            del self._cbs[key]
            raise L.TopicMatchError(rc, "tm_batcher_submit")
        return t.value

    def _on_publish_done(self, ctx, ticket, status, deliv, n_deliv, pairs, n_pairs):
        cb = self._cbs.pop(ctx)
        if status != L.TM_OK:
            cb(status, None, None)
            return
        # the records are valid only during the callback: copied out here
        def rows(ptr, n, width):
            if not n:
                return []
            raw = ctypes.string_at(ctypes.addressof(ptr.contents), n * width * 4)
            return list(map(tuple, np.frombuffer(raw, dtype=np.uint32).reshape(n, width).tolist()))
        cb(status, rows(deliv, n_deliv, 4), rows(pairs, n_pairs, 2))

    def submit_publish(self, topic: bytes, key: int, callback):
        """publish=True batchers: callback(status, deliveries, pairs) runs on
        the worker thread; deliveries = [(to, target, ndisp, pick)], pairs =
        [(to, sub)], both None on error.  key picks the $share members
        (SHARE_KEYED: member key rem Count; ignored by a round_robin batcher)"""
        t = ctypes.c_uint64()
        k = next(self._keys)
        self._cbs[k] = callback
        rc = self.lib.tm_batcher_submit_publish(self.h, topic, len(topic), key & 0xFFFFFFFF, self._pdone, k,
                                                ctypes.byref(t))
        if rc != L.TM_OK:
            del self._cbs[k]
            raise L.TopicMatchError(rc, "tm_batcher_submit_publish")
        return t.value

    def _on_inbox_done(self, _ctx, status, n_pub, tickets, hdr, inbox, n_inbox, ent_pub, ent_to, ent_word, n_ent):
        """inbox(status, tickets, hdr, inbox, ent_pub, ent_to, ent_word) on the
        lane's thread: numpy views of the lane's buffers, valid during the
        call only (tickets u64[n_pub]; hdr u64[4]; inbox u32[S, 4] = rows {sub,
        first, count, picks}; the entry planes u32[E]); on a failed batch
        tickets is empty and everything else but status is None"""
        def view(ptr, n, dtype):
            if not n:
                return np.zeros(0, dtype=dtype)
            return np.ctypeslib.as_array(ptr, shape=(n,)).view(dtype)
        tk = view(tickets, n_pub, np.uint64)
        if status != L.TM_OK:
            self.inbox(status, tk, None, None, None, None, None)
            return
        self.inbox(status, tk, view(hdr, 4, np.uint64), view(inbox, n_inbox * 4, np.uint32).reshape(-1, 4),
                   view(ent_pub, n_ent, np.uint32), view(ent_to, n_ent, np.uint32), view(ent_word, n_ent, np.uint32))

    def _on_forward_done(self, _ctx, status, n_pub, tickets, hdr, groups, n_groups, pub, n_fwd):
        """forward(status, tickets, hdr, groups, pub) on the lane's thread, after
        the batch's inbox callback and before its per-publish callbacks: numpy
        views of the lane's buffers, valid during the call only (tickets
        u64[n_pub]; hdr u64[4] = {M, G, targets, 0}; groups u32[G, 4] = rows
        {node target, To, first, count}; pub u32[M], indices into tickets); on a
        failed batch tickets is empty and everything else but status is None"""
        def view(ptr, n, dtype):
            if not n:
                return np.zeros(0, dtype=dtype)
            return np.ctypeslib.as_array(ptr, shape=(n,)).view(dtype)
        tk = view(tickets, n_pub, np.uint64)
        if status != L.TM_OK:
            self.forward(status, tk, None, None, None)
            return
        self.forward(status, tk, view(hdr, 4, np.uint64), view(groups, n_groups * 4, np.uint32).reshape(-1, 4),
                     view(pub, n_fwd, np.uint32))

    def _on_publish_opts_done(self, ctx, ticket, status, deliv, pick_word, n_deliv, pairs, pair_word, n_pairs):
        cb = self._cbs.pop(ctx)
        if status != L.TM_OK:
            cb(status, None, None, None, None)
            return
        if self.inbox is not None:   # the plan carries the pairs: only their count comes here
            raw = ctypes.string_at(ctypes.addressof(deliv.contents), n_deliv * 16) if n_deliv else b""
            cb(status, list(map(tuple, np.frombuffer(raw, dtype=np.uint32).reshape(n_deliv, 4).tolist())),
               [pick_word[i] for i in range(n_deliv)], None, n_pairs)
            return
        # records and words are valid only during the callback: copied out here
        def rows(ptr, n, width):
            if not n:
                return []
            raw = ctypes.string_at(ctypes.addressof(ptr.contents), n * width * 4)
            return list(map(tuple, np.frombuffer(raw, dtype=np.uint32).reshape(n, width).tolist()))
        cb(status, rows(deliv, n_deliv, 4), [pick_word[i] for i in range(n_deliv)], rows(pairs, n_pairs, 2),
           [pair_word[i] for i in range(n_pairs)])

    def submit_publish_opts(self, topic: bytes, key: int, pub_flags: int, pub_from: int, callback):
        """opts=True batchers: callback(status, deliveries, pick_words, pairs,
        pair_words) runs on the worker thread; pick_words[i] is the delivery
        word of deliveries[i]'s pick (NO_WORD without one, and for a stuck
        member outside its set), pair_words[i] that of pairs[i]; all None on
        error.  An inbox batcher calls callback(status, deliveries, pick_words,
        None, n_pairs): the pairs are in the batch's plan.  pub_flags / pub_from: the publish's words (tm_deliver)"""
        t = ctypes.c_uint64()
        k = next(self._keys)
        self._cbs[k] = callback
        rc = self.lib.tm_batcher_submit_publish_opts(self.h, topic, len(topic), key & 0xFFFFFFFF, pub_flags,
                                                     pub_from & 0xFFFFFFFF, self._odone, k, ctypes.byref(t))
        if rc != L.TM_OK:
            del self._cbs[k]
            raise L.TopicMatchError(rc, "tm_batcher_submit_publish_opts")
        return t.value

    def _on_publish_admit_done(self, ctx, ticket, status, deliv, pick_word, n_deliv, pairs, pair_word, n_pairs,
                               admit_code, acl_rule):
        user = self._cbs[ctx]
        rule = None if acl_rule == 0xFFFFFFFF else acl_rule
        self._cbs[ctx] = lambda st, *rest: user(st, *rest, admit_code, rule)
        self._on_publish_opts_done(ctx, ticket, status, deliv, pick_word, n_deliv, pairs, pair_word, n_pairs)

    @staticmethod
    def creds(c):
        """a credentials dict as emqx_access.AclRules takes it (client_id,
        username: str / bytes / None = undefined; peername: (ip text, port) or
        None) -> tm_pub_creds"""
        import ipaddress
        b = lambda x: x.encode() if isinstance(x, str) else bytes(x)   # noqa: E731
        cid, usr, peer = c.get("client_id"), c.get("username"), c.get("peername")
        cb, ub = b(cid or b""), b(usr or b"")
        out = L.TmPubCreds(cb, ub, len(cb), len(ub), cid is not None, usr is not None, 0, 0)
        if peer:
            ip = ipaddress.ip_address(peer[0])
            out.peer_family = 4 if ip.version == 4 else 6
            out.peer[:len(ip.packed)] = list(ip.packed)
        return out

    def submit_publish_admit(self, topic: bytes, mount_len: int, key: int, pub_flags: int, pub_admit: int,
                             pub_from: int, creds, callback):
        """admit= batchers: topic = MountPoint ++ T, mount_len the mountpoint's
        length, pub_admit the admission word (emqx_access.pub_admit), creds a
        credentials dict or a TmPubCreds.  callback(status, deliveries,
        pick_words, pairs, pair_words, admit_code, acl_rule) as
        submit_publish_opts' (an inbox batcher: None, n_pairs for the pairs);
        a refused publish gets empty lists and its code"""
        t = ctypes.c_uint64()
        k = next(self._keys)
        self._cbs[k] = callback
        cr = creds if isinstance(creds, L.TmPubCreds) else self.creds(creds)
        rc = self.lib.tm_batcher_submit_publish_admit(self.h, topic, len(topic), mount_len, key & 0xFFFFFFFF, pub_flags,
                                                      pub_admit, pub_from & 0xFFFFFFFF, ctypes.byref(cr), self._adone,
                                                      k, ctypes.byref(t))
        if rc != L.TM_OK:
            del self._cbs[k]
            raise L.TopicMatchError(rc, "tm_batcher_submit_publish_admit")
        return t.value

    def flush(self):
        rc = self.lib.tm_batcher_flush(self.h)
        if rc != L.TM_OK:
            raise L.TopicMatchError(rc, "tm_batcher_flush")

    def stats(self, reset_max=False):
        """tm_batcher_get_stats2: every counter; the max_* fields cover the
        batches since the open or the last read with reset_max=True"""
        s = L.TmBatcherStatsAdmit()
        rc = self.lib.tm_batcher_get_stats2(self.h, ctypes.byref(s), ctypes.sizeof(s),
                                            L.TM_BATCHER_STATS_RESET_MAX if reset_max else 0)
        if rc != L.TM_OK:
            raise L.TopicMatchError(rc, "tm_batcher_get_stats2")
        return {k: getattr(s, k) for k, _ in s._fields_}

    def close(self):
        if self.h:
            self.lib.tm_batcher_close(self.h)
            self.h = None
