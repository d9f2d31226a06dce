"""The admission corpus shared by tests/test_admit.py (CPU) and
tests/test_gpu_admit.py: the full product the admission checks branch on, the
zone tables in the oracle's and the library's terms, and the packing of a list
of cases into the batch calls' arrays.  A plain helper module: no fixtures,
nothing random."""
import itertools

import numpy as np

import admit_ref
from emqx_amd.emqx_access import Zones, pub_admit

# levels that only look like wildcards, the wildcard levels, and the edge topics
NOT_WILD = [b"a/+b", b"+a", b"a#", b"a/b+"]
WILD = [b"+", b"#", b"a/+", b"+/a", b"a/#/b", b"/+", b"#/"]
EDGE = [b"", b"/", b"$SYS/+", b"t/" + b"x" * 4095]          # the last: 4097 bytes, admitted (no length check)
TOPICS = NOT_WILD + WILD + EDGE
# no mountpoint; one whose own '+' level must not count; one that puts a '+' right before the topic's first byte
MOUNTS = [b"", b"dev/+/", b"+"]

# every cap both passes and refuses somewhere in the product
ZONES = [
    dict(admit_ref.DEFAULT_ZONE),
    dict(max_qos_allowed=1, max_topic_alias=4, mqtt_retain_available=False, enable_acl=True, acl_nomatch="allow"),
    dict(max_qos_allowed=0, max_topic_alias=5, mqtt_retain_available=True, enable_acl=False, acl_nomatch="deny"),
    dict(max_qos_allowed=2, max_topic_alias=65535, mqtt_retain_available=False, enable_acl=True, acl_nomatch="deny"),
]
ACL_INT = {"allow": 1, "deny": 0, "nomatch": -1}


def zones_table(zones=ZONES):
    z = Zones()
    for i, d in enumerate(zones):
        z.add("z%d" % i, d["max_qos_allowed"], d["max_topic_alias"], d["mqtt_retain_available"], d["enable_acl"],
              d["acl_nomatch"])
    return z


def case(topic, mount=b"", qos=0, retain=False, alias=None, zone=0, is_super=False, acl="nomatch"):
    return dict(topic=topic, mount=mount, qos=qos, retain=retain, alias=alias, zone=zone, is_super=is_super, acl=acl)


def product():
    return [case(t, m, q, r, a, z, s, acl)
            for t, m, q, r, a, z, s, acl in itertools.product(
                TOPICS, MOUNTS, (0, 1, 2), (False, True), (None, 1, 4, 5), range(len(ZONES)), (False, True),
                ("allow", "deny", "nomatch"))]


def want(c, zones=ZONES):
    return admit_ref.admit(c["topic"], c["qos"], c["retain"], c["alias"], zones[c["zone"]], c["is_super"], c["acl"])


def arrays(cases, lead=0):
    """-> dict of the batch calls' host arrays; the mounted topics packed from
    byte offset `lead` of the buffer (the bytes before it are '/')"""
    n = len(cases)
    mounted = [c["mount"] + c["topic"] for c in cases]
    off = np.zeros(n + 1, dtype=np.uint64)
    off[0] = lead
    if n:
        off[1:] = lead + np.cumsum([len(t) for t in mounted], dtype=np.uint64)
    buf = np.frombuffer(b"/" * lead + b"".join(mounted) + b"/" * 8, dtype=np.uint8).copy()
    return dict(
        buf=buf, off=off,
        mount_len=np.array([len(c["mount"]) for c in cases], dtype=np.uint32),
        pub_flags=np.array([c["qos"] | (4 if c["retain"] else 0) for c in cases], dtype=np.uint32),
        pub_admit=np.array([pub_admit(c["zone"], c["is_super"], c["alias"]) for c in cases], dtype=np.uint32),
        acl=np.array([ACL_INT[c["acl"]] for c in cases], dtype=np.int8))
