"""TEST ORACLE for the sending half of forward/3: our own Python restatement of
route/2's {To, Node} clause (src/emqx_broker.erl:185-186) and forward/3
(:209-216) over oracle.pytrie.RouteTable.match_deliveries (=
aggre(match_routes(T))), and of the plan contract of tm_forward_plan.

    forward_deliveries   per topic of a batch in order, every delivery
                         {To, Node} with Node an atom other than node()
    expected_plan        those deliveries as (target id, To id, publish index)
                         grouped and ordered as the engine's plan is
    bundles              the same over names: what Broker.publish_forward_many returns

A $share delivery {To, Group} (kind 1) and the local node's deliveries are
never forwards.  aggre/1 only usorts once a group delivery follows, so one
topic's list may hold the same {To, Node} twice: both are forwards.
"""
ROUTE_TOPIC = 0xFFFFFFFF   # the To id of "the publish topic itself": sorts after every filter id


def forward_deliveries(table, node, topics):
    """[(Node bytes, To bytes, publish index, k)]: k = the delivery's position
    in its topic's list (the engine's slot is the topic's route offset + k).
    node: the local node's name as bytes."""
    out = []
    for t, topic in enumerate(topics):
        for k, (to, x) in enumerate(table.match_deliveries(topic)):
            if x[0] == 0 and x[1] != node:       # when is_atom(Node) -> forward(Node, To, Delivery)
                out.append((x[1], to, t, k))
    return out


def expected_plan(triples):
    """triples: [(target id, To id, publish index)] in any order -> (hdr,
    groups, pub): hdr = [M, G, distinct targets, 0], groups = [(target, To,
    first, count)], pub = [publish index], sorted by all three ascending"""
    s = sorted(triples)
    groups = []
    for p, (tg, to, _) in enumerate(s):
        if groups and groups[-1][0] == tg and groups[-1][1] == to:
            groups[-1][3] += 1
        else:
            groups.append([tg, to, p, 1])
    hdr = [len(s), len(groups), len({g[0] for g in groups}), 0]
    return hdr, [tuple(g) for g in groups], [x[2] for x in s]


def bundles(groups, pub, node_name, to_name):
    """a plan over names: [(node bytes, [(To bytes | None, [publish index])])],
    None for ROUTE_TOPIC; node_name / to_name map the ids back"""
    out = []
    for tg, to, first, count in groups:
        if not out or out[-1][0] != node_name(tg):
            out.append((node_name(tg), []))
        out[-1][1].append((None if to == ROUTE_TOPIC else to_name(to), list(pub[first:first + count])))
    return out
