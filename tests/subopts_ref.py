"""TEST ORACLE for subscription options and the per-pair dispatch steps: our
own Python restatement, clause by clause, beside dispatch_ref.py.

    SubOptionTable.do_subscribe      do_subscribe/4      src/emqx_broker.erl:407-410
    SubOptionTable.do_unsubscribe    do_unsubscribe/3    :412-415
    SubOptionTable.get_subopts       get_subopts/2       :279-283
    SubOptionTable.set_subopts       set_subopts/3       :285-291
    run_dispatch_steps               handle_dispatch/3 + run_dispatch_steps/3
                                     src/emqx_session.erl:667-684, 797-819
    route_dispatch_opts              dispatch_ref.route_dispatch with the third element per pair

Options are dicts {qos, nl, rap[, subid]} as the session keeps them; a message
is (qos, retain, retained, from_sub | None).  The emqx_subscription reverse
table (:408, :413) is not restated: nothing here reads it.
"""
from dispatch_ref import NOT_LOCAL, SubscriberBag, dispatch

DEFAULT_SUBOPTS = {"qos": 0, "nl": 0, "rap": 0}   # ?DEFAULT_SUBOPTS without rh / rc: dispatch never reads them


class SubOptionTable:
    """emqx_suboption, a set keyed {Topic, Subscriber}, over a SubscriberBag"""

    def __init__(self, bag=None):
        self.bag = SubscriberBag() if bag is None else bag
        self.tab = {}

    def do_subscribe(self, group, topic, subscriber, subopts):
        self.bag.insert_subscriber(group, topic, subscriber)                   # :409
        self.tab[(topic, subscriber)] = dict(DEFAULT_SUBOPTS, **subopts)       # :410, whatever :409 did

    def do_unsubscribe(self, group, topic, subscriber):
        left = self.bag.delete_object(group, topic, subscriber)                # :414
        self.tab.pop((topic, subscriber), None)                                # :415, whatever the group
        return left

    def get_subopts(self, topic, subscriber):
        # try ets:lookup_element(...) catch error:badarg -> [] end
        return self.tab.get((topic, subscriber))

    def set_subopts(self, topic, subscriber, opts):
        old = self.tab.get((topic, subscriber))
        if old is None:
            return False                                                       # [] -> false
        self.tab[(topic, subscriber)] = dict(old, **opts)                      # maps:merge(OldOpts, Opts)
        return True


def run_dispatch_steps(opts, msg, same_client, upgrade):
    """-> None when the session drops the message (no-local), else (qos,
    retain, subid | None) of the message it goes on to dispatch/2 with.
    opts None: maps:find(Topic, SubMap) -> error, the message as it is."""
    qos, retain, retained, _from = msg
    if opts is None:                                  # :679-680
        return (qos, 1 if retain else 0, None)
    # [{nl, Nl}, {qos, QoS}, {rap, Rap}] (++ [{subid, SubId}]) in this order  :675-678
    if opts["nl"] == 1 and same_client:               # :799-800
        return None
    if not upgrade:                                   # :803-809
        qos = min(opts["qos"], qos)
    else:                                             # :810-811
        qos = max(opts["qos"], qos)
    if retained:                                      # :812-813  headers = #{retained := true}
        retain = 1
    elif opts["rap"] == 0:                            # :814-815
        retain = 0
    else:                                             # :816-817
        retain = 1 if retain else 0
    return (qos, retain, opts.get("subid"))           # :818-819


def route_dispatch_opts(table, subopts, node, topic, msg, upgrade=False):
    """dispatch_ref.route_dispatch over subopts.bag, every pair with what the
    subscriber's session makes of the message: (To, Sub, None | (qos, retain,
    subid | None))"""
    counts, pairs = [], []
    for to, x in table.match_deliveries(topic):
        if x == (0, node):
            n, sent = dispatch(subopts.bag, to)
            counts.append(n)
            for s in sent:
                same = msg[3] is not None and s == msg[3]
                pairs.append((to, s, run_dispatch_steps(subopts.get_subopts(to, s), msg, same, upgrade)))
        else:
            counts.append(NOT_LOCAL)
    return counts, pairs


def dispatch_opts(subopts, to, msg, upgrade=False):
    """dispatch/2 of a forwarded message: (Count, [(Sub, outcome)])"""
    n, sent = dispatch(subopts.bag, to)
    return n, [(s, run_dispatch_steps(subopts.get_subopts(to, s), msg, msg[3] is not None and s == msg[3], upgrade))
               for s in sent]
