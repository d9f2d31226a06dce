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

A member is the u32 the caller chose for the subscriber; groups are byte
strings.  `sticky` and the nack retry stay with the caller.
"""
from .emqx_router import _key
from .engine import Engine

STRATEGIES = {"hash": Engine.SHARE_KEYED, "random": Engine.SHARE_KEYED, "keyed": Engine.SHARE_KEYED,
              "round_robin": Engine.SHARE_ROUND_ROBIN}


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
        """one publisher process's round-robin dictionary (:243-249) on a
        replica, for Engine.publish_stream_device; close() it before the engine"""
        return self.engine.share_cursors(replica)
