"""TEST ORACLE for the delivery word of a $share pick, composed from the
restatements beside it:

    sticky_ref.route_pick            pick/5 per {To, Group} delivery   src/emqx_shared_sub.erl:211-249
    subopts_ref.SubOptionTable       emqx_suboption                    src/emqx_broker.erl:279-291, 407-415
    subopts_ref.run_dispatch_steps   handle_dispatch/3 + run_dispatch_steps/3
                                                                       src/emqx_session.erl:667-684, 797-819

emqx_shared_sub:dispatch/4 sends the picked member the same {dispatch, Topic,
Msg} (:121-140) and that member's session runs the same handle_dispatch/3, so
the outcome of a pick is run_dispatch_steps over the member's option entry for
the set's topic.  A member id is the subscriber id.

NO_WORD is the engine's stated boundary, written here as what it is: a slot
without a pick has no outcome, and for a picked member that is not in the set
(a stuck member that unsubscribed, which pick/5 keeps returning) the device
gives no answer and the caller computes the outcome itself.
"""
from shared_ref import NO_MEMBER
from sticky_ref import route_pick
from subopts_ref import run_dispatch_steps

NO_WORD = "no word"

TM_NO_WORD = 0xFFFFFFFF
TM_DELIVER_DROP = 8


def pick_outcome(subopts, shared, group, to, member, msg, upgrade=False):
    """NO_WORD, None (dropped by no-local) or (qos, retain, subid | None) for
    the member picked for the {To, Group} delivery of message msg = (qos,
    retain, retained, from_sub | None)"""
    if member is NO_MEMBER:
        return NO_WORD
    if member not in shared.subscribers(group, to):           # the one case the device does not answer
        return NO_WORD
    same = msg[3] is not None and member == msg[3]
    return run_dispatch_steps(subopts.get_subopts(to, member), msg, same, upgrade)


def route_pick_words(table, shared, subopts, strategy, key, topic, msg, upgrade=False):
    """one publish: per delivery of aggre(match_routes(Topic)), in order,
    (member | NO_MEMBER, outcome).  `shared` is a sticky_ref.StickySub: the
    picks advance its cursors and sticky entries as route_pick does."""
    picks = route_pick(table, shared, strategy, key, topic)
    out = []
    for (to, (kind, x)), m in zip(table.match_deliveries(topic), picks):
        out.append((m, pick_outcome(subopts, shared, x, to, m, msg, upgrade) if kind == 1 else NO_WORD))
    return out


def outcome_word(outcome):
    """the outcome as the engine's word: NO_WORD -> TM_NO_WORD, a drop is
    exactly TM_DELIVER_DROP, else qos | retain << 2 | subid << 4"""
    if outcome == NO_WORD:
        return TM_NO_WORD
    if outcome is None:
        return TM_DELIVER_DROP
    qos, retain, subid = outcome
    return qos | retain << 2 | (subid or 0) << 4
