"""TEST ORACLE for the shared-subscription member table and pick: our own
Python restatement of src/emqx_shared_sub.erl, clause by clause, beside
tests/dispatch_ref.py (over oracle.pytrie.RouteTable.match_deliveries).

    SharedSub.subscribe            subscribe/3                    :75-79
    SharedSub.unsubscribe          unsubscribe/3                  :81-84
    SharedSub.subscribers          subscribers/2                  :251-252
    SharedSub.cleanup_down         cleanup_down/1                 :316-321
    SharedSub.do_pick              do_pick/5, FailedSubs = []     :228-233
    SharedSub.do_pick_subscriber   do_pick_subscriber/5           :239-249
    route_shared                   route/2's third clause (src/emqx_broker.erl:187-189) over a publish

The table is a mnesia bag: the members of one (Group, Topic) keep insertion
order and never repeat.  A member is any hashable value (the tests use ints).

Strategies: "keyed" takes one integer Key per publish, Nth = 1 + Key rem Count
-- `hash` with Key = erlang:phash2(ClientId), `random` with a uniform Key --
and "round_robin".  The object keeps ONE process dictionary (self.pd): every
publish comes from one publisher process, so the reference's per-process
cursor {shared_sub_round_robin, Group, Topic} is a cursor per set.  That is
the engine's first stated deviation, written here as what it is; the second
is explicit in _forget: the entry is erased when the set loses its last
member (the reference never erases it).
"""
NO_MEMBER = None


class SharedSub:
    def __init__(self):
        self.tab = {}     # (group, topic) -> [member] in insertion order
        self.pd = {}      # the publisher's process dictionary

    # subscribe(undefined, _Topic, _SubPid) -> ok;
    # subscribe(Group, Topic, SubPid) -> mnesia:dirty_write(?TAB, record(Group, Topic, SubPid))
    def subscribe(self, group, topic, sub):
        if group is None:
            return
        members = self.tab.setdefault((group, topic), [])
        if sub not in members:                # a bag: writing a record already present changes nothing
            members.append(sub)

    # unsubscribe(Group, Topic, SubPid) -> mnesia:dirty_delete_object(?TAB, record(Group, Topic, SubPid))
    def unsubscribe(self, group, topic, sub):
        """returns the members left in the set"""
        if group is None:
            return 0
        members = self.tab.get((group, topic))
        if members is None:
            return 0
        if sub in members:
            members.remove(sub)
        if not members:
            self._forget(group, topic)
        return len(members)

    def _forget(self, group, topic):
        del self.tab[(group, topic)]
        self.pd.pop(("shared_sub_round_robin", group, topic), None)   # DEVIATION 2: the cursor goes with the set

    # subscribers(Group, Topic) -> ets:select(?TAB, [{{emqx_shared_subscription, Group, Topic, '$1'}, [], ['$1']}])
    def subscribers(self, group, topic):
        return list(self.tab.get((group, topic), []))

    # cleanup_down(SubPid) -> every record whose subpid is SubPid is deleted
    def cleanup_down(self, sub):
        """returns the records deleted"""
        gone = 0
        for (group, topic), members in list(self.tab.items()):
            if sub in members:
                members.remove(sub)
                gone += 1
                if not members:
                    self._forget(group, topic)
        return gone

    def size(self):
        return sum(len(v) for v in self.tab.values())

    # do_pick(Strategy, ClientId, Group, Topic, FailedSubs = [])
    def do_pick(self, strategy, key, group, topic):
        subs = self.subscribers(group, topic)
        if not subs:                          # [] -> false
            return NO_MEMBER
        if len(subs) == 1:                    # [Sub] -> Sub
            return subs[0]
        nth = self.do_pick_subscriber(group, topic, strategy, key, len(subs))
        return subs[nth - 1]                  # lists:nth(Nth, Subs)

    def do_pick_subscriber(self, group, topic, strategy, key, count):
        if strategy == "keyed":               # hash: 1 + erlang:phash2(ClientId) rem Count
            return 1 + key % count
        assert strategy == "round_robin"
        n = self.pd.get(("shared_sub_round_robin", group, topic))   # erlang:get
        rem = 0 if n is None else (n + 1) % count                   # undefined -> 0; N -> (N + 1) rem Count
        self.pd[("shared_sub_round_robin", group, topic)] = rem     # erlang:put
        return rem + 1


def route_shared(table, shared, strategy, key, topic):
    """the picks of one publish: per delivery of aggre(match_routes(Topic)),
    in order, the member for a {To, Group} delivery (NO_MEMBER for `false`)
    and NO_MEMBER for a {To, Node} one.  Group keys are bytes, as _x_term
    leaves them."""
    picks = []
    for to, (kind, x) in table.match_deliveries(topic):
        picks.append(shared.do_pick(strategy, key, x, to) if kind == 1 else NO_MEMBER)
    return picks
