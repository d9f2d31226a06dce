"""TEST ORACLE for the subscriber bag and publish/1's local dispatch: our own
Python restatement of src/emqx_broker.erl, clause by clause, over
oracle.pytrie.RouteTable.match_deliveries (= aggre(match_routes(T))).

    SubscriberBag.insert_subscriber   insert_subscriber/3        :398-405
    SubscriberBag.delete_object       ets:delete_object(?SUBSCRIBER, ...) of do_unsubscribe/3 :412-415
    SubscriberBag.subscribers         subscribers/1              :245-247
    route_dispatch                    route/2 :175-192 + dispatch/2 :218-238

The table is a duplicate_bag (src/emqx_broker_sup.erl:55-67): entries of one
topic keep insertion order and may repeat.  A subscriber is any hashable value
(the tests use ints); a shared entry is ("share", Group, Sub).
"""
NOT_LOCAL = None


def shared(group, name):
    # shared(undefined, Name) -> Name; shared(Group, Name) -> {share, Group, Name}   :447-448
    return name if group is None else ("share", group, name)


class SubscriberBag:
    def __init__(self):
        self.tab = {}     # topic -> [entry] in insertion order

    def subscribers(self, topic):
        # try ets:lookup_element(?SUBSCRIBER, Topic, 2) catch error:badarg -> [] end
        return list(self.tab.get(topic, []))

    def insert_subscriber(self, group, topic, subscriber):
        subscribers = self.subscribers(topic)
        if subscriber in subscribers:            # lists:member(Subscriber, Subscribers): the BARE subscriber
            return                               # _ -> ok
        self.tab.setdefault(topic, []).append(shared(group, subscriber))   # false -> ets:insert

    def delete_object(self, group, topic, subscriber):
        """every object equal to {Topic, shared(Group, Subscriber)} goes; returns the entries left"""
        obj = shared(group, subscriber)
        left = [x for x in self.tab.get(topic, []) if x != obj]
        if left:
            self.tab[topic] = left
        else:
            self.tab.pop(topic, None)
        return len(left)

    def member(self, topic):
        return topic in self.tab

    def size(self):
        return sum(len(v) for v in self.tab.values())


def dispatch(bag, topic):
    """dispatch/2: (Count, [plain subscribers that get {dispatch, Topic, Msg}]).
    Count 0 is the message.dropped clause; a {share, _, _} entry counts and is
    ignored (dispatch/3's second clause)."""
    subs = bag.subscribers(topic)
    sent = [s for s in subs if not (isinstance(s, tuple) and len(s) == 3 and s[0] == "share")]
    return len(subs), sent


def route_dispatch(table, bag, node, topic):
    """route(aggre(match_routes(Topic)), Delivery) for the parts the engine
    answers: per delivery, in aggre's order (route/2 folds left over them), the
    dispatch Count when the delivery is {To, node()} else NOT_LOCAL (a forward
    to another node or a $share group delivery), and the (To, Sub) pairs in
    the order the messages are sent.  node: the local node's name as bytes."""
    counts, pairs = [], []
    for to, x in table.match_deliveries(topic):
        if x == (0, node):                       # when Node =:= node() -> dispatch(To, Delivery)
            n, sent = dispatch(bag, to)
            counts.append(n)
            pairs.extend((to, s) for s in sent)
        else:                                    # forward/3, or emqx_shared_sub:dispatch/3
            counts.append(NOT_LOCAL)
    return counts, pairs
