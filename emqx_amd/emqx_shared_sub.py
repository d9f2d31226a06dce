"""emqx_shared_sub — the $share member table (src/emqx_shared_sub.erl), same
names and semantics, backed by the engine: the emqx_shared_subscription bag
lives in the engine (tm_share_add / tm_share_del) and the member of a $share
delivery is picked on the GPU with the rest of publish/1 (share.hip,
Broker.publish_shared_many).

    subscribe(Group, Topic, Sub)      subscribe/3      :75-79   (Group None = undefined: ok)
    unsubscribe(Group, Topic, Sub)    unsubscribe/3    :81-84
    subscribers(Group, Topic)         subscribers/2    :251-252, insertion order
    cleanup_down(Sub)                 cleanup_down/1   :316-321
    strategy                          strategy/0       :113-115 (default round_robin)
    pick(Group, Topic, Key, Failed)   pick/5           :211-249 (the retry of dispatch/4, :92-111)

A member is the u32 the caller chose for the subscriber; groups are byte
strings.  The sends and acks of do_dispatch stay with the caller
(INTEGRATION.md).
"""
import numpy as np

from .emqx_router import _key
from .engine import Engine

STRATEGIES = {"hash": Engine.SHARE_KEYED, "random": Engine.SHARE_KEYED, "keyed": Engine.SHARE_KEYED,
              "round_robin": Engine.SHARE_ROUND_ROBIN, "sticky": Engine.SHARE_STICKY}


class SharedSub:
    def __init__(self, engine: Engine, strategy="round_robin"):
        if strategy not in STRATEGIES:
            raise ValueError("strategy %r: the engine offers %s" % (strategy, sorted(STRATEGIES)))
        self.engine = engine
        self.strategy = strategy

    def subscribe(self, group, topic: bytes, sub: int):
        if group is None:
            return "ok"
        self.engine.share_add(_key(group), topic, sub)
        return "ok"

    def unsubscribe(self, group, topic: bytes, sub: int):
        if group is None:
            return "ok"
        self.engine.share_del(_key(group), topic, sub)
        return "ok"

    def subscribers(self, group, topic: bytes):
        return self.engine.share_members(_key(group), topic)

    def cleanup_down(self, sub: int):
        self.engine.share_member_down(sub)
        return "ok"

    def cursors(self, replica=0):
        """one publisher process's dictionary (round-robin cursors :243-249,
        sticky entries :211-224) on a replica, for Engine.publish_stream_device
        and pick; close() it before the engine"""
        return self.engine.share_cursors(replica)

    def pick(self, group, topic: bytes, key=0, failed=(), strategy=None, cursors=None):
        """pick(Strategy, ClientId, Group, Topic, FailedSubs) (:211-249): the
        member a retry of dispatch/4 sends to, None for `false`.  key: the
        publish's u32 (hash / random / sticky); failed: the members that
        nacked, timed out or went down during this delivery"""
        return self.pick_many([(group, topic, key, failed)], strategy, cursors)[0]

    def pick_many(self, requests, strategy=None, cursors=None):
        """[(group, topic, key, failed)] -> [member | None], one device call;
        the requests count in order, as one pick each would"""
        requests = list(requests)
        groups = [_key(g) for g, _, _, _ in requests]
        topics = [t for _, t, _, _ in requests]
        fails = [list(f) for _, _, _, f in requests]
        goff = np.cumsum([0] + [len(g) for g in groups], dtype=np.uint64)
        toff = np.cumsum([0] + [len(t) for t in topics], dtype=np.uint64)
        foff = np.cumsum([0] + [len(f) for f in fails], dtype=np.uint64)
        out = self.engine.share_pick_batch(
            STRATEGIES[strategy or self.strategy], np.frombuffer(b"".join(groups), dtype=np.uint8), goff,
            np.frombuffer(b"".join(topics), dtype=np.uint8), toff, [k for _, _, k, _ in requests],
            np.array([m for f in fails for m in f], dtype=np.uint32), foff, cursors)
        return [None if int(m) == Engine.NO_MEMBER else int(m) for m in out]
