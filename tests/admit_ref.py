"""TEST ORACLE for the publish admission stage: a literal Python transcription
of the three checks a PUBLISH passes before emqx_protocol:do_publish, in the
reference's order.  It does not call the library: the topic test goes through
emqx_amd.emqx_topic.words / wildcard on the word list (pure Python).  The one
ACL module's answer is an argument: the tests compute it with the Python rule
matcher the ACL tests use (oracle/pyacl.py through tests/acl_util.py's
credential terms), or enumerate all three answers.

    validate        emqx_packet:validate/1, the PUBLISH clauses   src/emqx_packet.erl:58-64
    check_pub       emqx_mqtt_caps:check_pub/2 + do_check_pub/2   src/emqx_mqtt_caps.erl:54-75
    check_pub_acl   emqx_protocol:check_pub_acl/2                 src/emqx_protocol.erl:785-794
    do_check_acl    emqx_access_control:do_check_acl/4            src/emqx_access_control.erl:104-111
    admit           process_packet's validate, then check_publish src/emqx_protocol.erl:217, 340-371, 769-771

A zone is a dict: max_qos_allowed, max_topic_alias, mqtt_retain_available,
enable_acl, acl_nomatch ("allow" | "deny").  The codes are the TM_ADMIT_* values.
"""
from emqx_amd.emqx_topic import wildcard, words

OK, TOPIC_NAME, QOS, TOPIC_ALIAS, RETAIN, ACL = range(6)

DEFAULT_ZONE = dict(max_qos_allowed=2, max_topic_alias=0, mqtt_retain_available=True, enable_acl=True,
                    acl_nomatch="deny")


def validate(topic: bytes, props: dict):
    """validate(?PUBLISH_PACKET(_QoS, <<>>, _, #{'Topic-Alias':= _I}, _)) -> true  -- the codec's clause: the
    caller has resolved the alias to its topic, so the clause never applies to what is submitted
    validate(?PUBLISH_PACKET(_QoS, <<>>, _, _, _)) -> error(topic_name_invalid);
    validate(?PUBLISH_PACKET(_QoS, Topic, _, Properties, _)) ->
        ((not emqx_topic:wildcard(Topic)) orelse error(topic_name_invalid)) andalso ..."""
    if topic == b"":
        return "topic_name_invalid"
    if wildcard(words(topic)):
        return "topic_name_invalid"
    return True


def check_pub(zone: dict, props: dict):
    # maps:to_list/1 orders the atom keys: max_qos_allowed < max_topic_alias < mqtt_retain_available
    caps = sorted((k, zone[k]) for k in ("max_qos_allowed", "mqtt_retain_available", "max_topic_alias"))
    return do_check_pub(props, caps)


def do_check_pub(props, caps):
    if not caps:
        return "ok"
    (key, val), rest = caps[0], caps[1:]
    if key == "max_qos_allowed":
        if props["qos"] > val:
            return QOS
        return do_check_pub(props, rest)
    if key == "max_topic_alias" and "topic_alias" in props:
        alias = props["topic_alias"]
        if not (alias <= val and alias > 0):
            return TOPIC_ALIAS
        return do_check_pub(props, rest)
    if key == "mqtt_retain_available" and props.get("retain") is True and val is False:
        return RETAIN
    return do_check_pub(props, rest)


def do_check_acl(zone, answers):
    """answers: what each ACL module returns, in order (one module here)"""
    for a in answers:
        if a == "allow":
            return "allow"
        if a == "deny":
            return "deny"
        assert a in ("ignore", "nomatch")
    return zone.get("acl_nomatch", "deny")


def check_pub_acl(zone, is_super, acl_answer):
    if is_super or not zone["enable_acl"]:
        return "ok"
    return "ok" if do_check_acl(zone, [acl_answer]) == "allow" else ACL


def admit(topic: bytes, qos: int, retain: bool, alias, zone: dict, is_super: bool, acl_answer: str) -> int:
    """topic as the client sent it; alias None = the property is absent;
    acl_answer "allow" | "deny" | "nomatch" -- the one ACL module's answer for
    (credentials, publish, topic), computed by the caller"""
    props = {"qos": qos, "retain": bool(retain)}
    if alias is not None:
        props["topic_alias"] = alias
    if validate(topic, props) is not True:
        return TOPIC_NAME
    r = check_pub(zone, props)
    if r != "ok":
        return r
    r = check_pub_acl(zone, is_super, acl_answer)
    return OK if r == "ok" else r


def header(codes):
    """{admitted, count of code 1..5, 0, 0}"""
    h = [0] * 8
    for c in codes:
        h[int(c)] += 1
    return h
