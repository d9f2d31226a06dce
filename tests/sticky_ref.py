"""TEST ORACLE for the `sticky` strategy and the retry picks: the clauses of
src/emqx_shared_sub.erl that tests/shared_ref.py leaves out, restated one by
one on top of its SharedSub.

    StickySub.pick            pick/5                          :211-226
    StickySub.do_pick_failed  do_pick/5, any FailedSubs       :228-233
    StickySub.is_active_sub   is_active_sub/2                 :327-328
    StickySub.is_alive_sub    is_alive_sub/1                  :330-334
    route_pick                route/2's third clause (src/emqx_broker.erl:187-189) over a publish

Liveness: the object keeps the set of live subscriber processes.  subscribe
adds to it (a process that subscribes is alive), cleanup_down removes from it
(cleanup_down/1 is what the 'DOWN' message runs, :316-321) and unsubscribe
does not touch it: a process that unsubscribed is still a process.

A member is a u32 the caller chose, and a u32 that subscribes again after its
cleanup_down stands for a NEW process.  A pid is never reused, so the entry
that named the old process must not name the new one: cleanup_down also
erases every sticky entry equal to the member, which is is_alive_sub
evaluated at once instead of at the next pick (for one and the same process
the two are the same: dead stays dead).

The deviations of shared_ref.py hold for the sticky key as for the cursor: one
process dictionary (one publisher), and _forget erases the entry with the set.
"""
from shared_ref import NO_MEMBER, SharedSub


class StickySub(SharedSub):
    def __init__(self):
        super().__init__()
        self.alive = set()

    def subscribe(self, group, topic, sub):
        if group is None:
            return
        self.alive.add(sub)
        super().subscribe(group, topic, sub)

    def cleanup_down(self, sub):
        self.alive.discard(sub)
        for k in [k for k, v in self.pd.items() if k[0] == "shared_sub_sticky" and v == sub]:
            del self.pd[k]                            # is_alive_sub(Sub0) = false from now on, evaluated here
        return super().cleanup_down(sub)

    def _forget(self, group, topic):
        super()._forget(group, topic)
        self.pd.pop(("shared_sub_sticky", group, topic), None)   # DEVIATION 2, as for the cursor

    # is_alive_sub(Pid) -> [] =/= ets:lookup(?ALIVE_SUBS, Pid); false and undefined are no pids
    def is_alive_sub(self, pid):
        return pid is not NO_MEMBER and pid in self.alive

    # is_active_sub(Pid, FailedSubs) -> is_alive_sub(Pid) andalso not lists:member(Pid, FailedSubs)
    def is_active_sub(self, pid, failed):
        return self.is_alive_sub(pid) and pid not in failed

    # pick(sticky, ClientId, Group, Topic, FailedSubs); pick(Strategy, ...) -> do_pick(Strategy, ...)
    def pick(self, strategy, key, group, topic, failed=()):
        if strategy == "sticky":
            sub0 = self.pd.get(("shared_sub_sticky", group, topic))          # erlang:get
            if self.is_active_sub(sub0, failed):
                return sub0                                                  # true -> Sub0
            sub = self.do_pick_failed("keyed", key, group, topic, failed)     # do_pick(random, ...)
            self.pd[("shared_sub_sticky", group, topic)] = sub               # erlang:put; `false` reads as undefined
            return sub
        return self.do_pick_failed(strategy, key, group, topic, failed)

    # do_pick(Strategy, ClientId, Group, Topic, FailedSubs)
    def do_pick_failed(self, strategy, key, group, topic, failed):
        subs = [s for s in self.subscribers(group, topic) if s not in failed]   # subscribers(Group, Topic) -- FailedSubs
        if not subs:                                                         # [] -> false
            return NO_MEMBER
        if len(subs) == 1:                                                   # [Sub] -> Sub
            return subs[0]
        nth = self.do_pick_subscriber(group, topic, strategy, key, len(subs))
        return subs[nth - 1]                                                 # lists:nth(Nth, Subs)


def route_pick(table, shared, strategy, key, topic):
    """shared_ref.route_shared through pick/5 with FailedSubs = []"""
    picks = []
    for to, (kind, x) in table.match_deliveries(topic):
        picks.append(shared.pick(strategy, key, x, to) if kind == 1 else NO_MEMBER)
    return picks
