"""emqx_access_rule / emqx_acl_internal on the GPU: a rule set
compiled like emqx_access_rule:compile/1 (src/emqx_access_rule.erl:38-75),
checked in batches by the acl.hip kernel with emqx_acl_internal:match/3's
first-match semantics (src/emqx_acl_internal.erl:63-87).

Rule terms (the acl.conf shapes): ("allow"|"deny", "all") or
("allow"|"deny", who, "publish"|"subscribe"|"pubsub", topics), who = "all" |
("client", c | "all") | ("user", u | "all") | ("ipaddr", "a.b.c.d[/n]") |
("and"|"or", [who...]); topics = a topic or a list of topics / ("eq", topic).
Credentials: dicts with optional client_id, username (None = undefined) and
peername ((ip_text, port) or None)."""
import ctypes
import ipaddress

import numpy as np

from . import _lib as L

ACCESS = {"publish": 1, "subscribe": 2, "pubsub": 3}
WHO = {"all": 0, "client": 1, "user": 2, "client_all": 3, "user_all": 4, "ipaddr": 5, "and": 6, "or": 7, "end": 8}
RESULT = {1: "allow", 0: "deny", -1: "nomatch"}


def _b(x):
    return x.encode() if isinstance(x, str) else bytes(x)


class AclRules:
    def __init__(self, device=0):
        self.lib = L.load()
        h = ctypes.c_void_p()
        rc = self.lib.tm_acl_open(device, ctypes.byref(h))
        if rc != L.TM_OK:
            raise L.TopicMatchError(rc, "tm_acl_open")
        self.h = h

    def close(self):
        if self.h:
            self.lib.tm_acl_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, what):
        if rc != L.TM_OK:
            raise L.TopicMatchError(rc, what)

    def _who(self, w):
        if w == "all":
            return self._ck(self.lib.tm_acl_who(self.h, WHO["all"], None, 0, 0), "who")
        kind, arg = w
        if kind in ("client", "user"):
            if arg == "all":
                return self._ck(self.lib.tm_acl_who(self.h, WHO[kind + "_all"], None, 0, 0), "who")
            a = _b(arg)
            return self._ck(self.lib.tm_acl_who(self.h, WHO[kind], a, len(a), 0), "who")
        if kind == "ipaddr":
            a = _b(arg)                  # "addr" or "addr/n": the library parses n (0 = the whole family)
            return self._ck(self.lib.tm_acl_who(self.h, WHO["ipaddr"], a, len(a), 0), "who")
        if kind in ("and", "or"):
            self._ck(self.lib.tm_acl_who(self.h, WHO[kind], None, 0, 0), "who")
            for c in arg:
                self._who(c)
            return self._ck(self.lib.tm_acl_who(self.h, WHO["end"], None, 0, 0), "who")
        raise ValueError(w)

    def add(self, rule):
        """one rule, appended after the ones already loaded (file order)"""
        if len(rule) == 2 and rule[1] == "all":
            self._ck(self.lib.tm_acl_rule_begin(self.h, 1 if rule[0] == "allow" else 0, 0), "rule")
            return self._ck(self.lib.tm_acl_rule_end(self.h), "rule_end")
        a, who, access, topics = rule
        self._ck(self.lib.tm_acl_rule_begin(self.h, 1 if a == "allow" else 0, ACCESS[access]), "rule")
        self._who(who)
        if isinstance(topics, (str, bytes)):
            topics = [topics]
        for t in topics:
            eq = isinstance(t, (tuple, list)) and t[0] == "eq"
            tb = _b(t[1] if eq else t)
            self._ck(self.lib.tm_acl_topic(self.h, 1 if eq else 0, tb, len(tb)), "topic")
        return self._ck(self.lib.tm_acl_rule_end(self.h), "rule_end")

    def load(self, rules):
        for r in rules:
            self.add(r)
        return self

    @staticmethod
    def pack(creds, pubsubs, topics):
        """the batch as the C-ABI's arrays (name -> numpy array), in
        tm_acl_check_batch's argument order; topics None: everything but the
        topic CSR, for a caller whose topics are on the device already"""
        n = len(creds) if topics is None else len(topics)

        def strs(items):
            bs = [_b(x) for x in items]
            off = np.zeros(n + 1, dtype=np.uint64)
            if n:
                off[1:] = np.cumsum([len(x) for x in bs])
            return np.frombuffer(b"".join(bs) + b"\0" * 8, dtype=np.uint8).copy(), off
        tb, to = strs(topics) if topics is not None else (None, None)
        cb, co = strs([c.get("client_id") or b"" for c in creds])
        ub, uo = strs([c.get("username") or b"" for c in creds])
        cd = np.array([c.get("client_id") is not None for c in creds], dtype=np.uint8)
        ud = np.array([c.get("username") is not None for c in creds], dtype=np.uint8)
        peers = np.zeros((max(n, 1), 16), dtype=np.uint8)
        fam = np.zeros(max(n, 1), dtype=np.uint8)
        for i, c in enumerate(creds):
            p = c.get("peername")
            if p:
                ip = ipaddress.ip_address(p[0])
                raw = ip.packed
                peers[i, :len(raw)] = np.frombuffer(raw, dtype=np.uint8)
                fam[i] = 4 if ip.version == 4 else 6
        acc = np.array([1 if p == "publish" else 2 for p in pubsubs], dtype=np.uint8)
        return {"access": acc, "topics": tb, "topic_off": to, "client_ids": cb, "client_off": co,
                "client_defined": cd, "usernames": ub, "user_off": uo, "user_defined": ud, "peers": peers,
                "peer_family": fam}

    ARGS = ("access", "topics", "topic_off", "client_ids", "client_off", "client_defined", "usernames", "user_off",
            "user_defined", "peers", "peer_family")

    def check_packed(self, n, arrs, want_rule=True):
        """host arrays from pack() -> (result int8[n], rule u32[n]); a missing
        or None "peers" / "peer_family" goes as NULL, and so does the rule
        output with want_rule=False (then rule is None)"""
        out = np.zeros(max(n, 1), dtype=np.int8)
        rule = np.zeros(max(n, 1), dtype=np.uint32) if want_rule else None
        P = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)  # noqa: E731
        self._ck(self.lib.tm_acl_check_batch(self.h, n, *[P(arrs.get(k)) for k in self.ARGS], P(out), P(rule)),
                 "tm_acl_check_batch")
        return out[:n], rule[:n] if want_rule else None

    def check_device(self, n, d, d_out, d_rule, stream=None):
        """device tensors (the pack() names) -> d_out / d_rule, stream-ordered
        (tm_acl_check_batch_device); None for "peers" / "peer_family" / d_rule goes as NULL"""
        P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
        st = None
        if stream is not None:
            st = ctypes.c_void_p(L.stream_handle(stream))
        self._ck(self.lib.tm_acl_check_batch_device(self.h, n, *[P(d.get(k)) for k in self.ARGS], P(d_out), P(d_rule),
                                                    st), "tm_acl_check_batch_device")

    def check_many(self, creds, pubsubs, topics):
        """-> [(allow|deny|nomatch, rule index or None)] per check (GPU)"""
        n = len(topics)
        out, rule = self.check_packed(n, self.pack(creds, pubsubs, topics))
        return [(RESULT[int(out[i])], None if rule[i] == 0xFFFFFFFF else int(rule[i])) for i in range(n)]


# ---- publish admission: emqx_packet:validate/1, emqx_mqtt_caps:check_pub/2 and
# check_pub_acl (src/emqx_protocol.erl:769-794) in front of emqx_broker:publish/1
ADMIT = {0: "ok", 1: "topic_name_invalid", 2: "qos_not_supported", 3: "topic_alias_invalid",
         4: "retain_not_supported", 5: "not_authorized"}


class Zones:
    """The zone table of the admission calls (tm_zone_caps records): per zone
    the '$mqtt_pub_caps' of emqx_mqtt_caps and the two ACL switches of
    emqx_zone.  Defaults as the reference's: QoS 2, no aliases, retain
    available, ACL enabled, acl_nomatch = deny.  The position of a zone is the
    index a publish's pub_admit word carries."""

    def __init__(self):
        self.names = []
        self.caps = []

    def add(self, name, max_qos_allowed=2, max_topic_alias=0, retain_available=True, enable_acl=True,
            acl_nomatch="deny"):
        if len(self.caps) >= L.TM_ADMIT_MAX_ZONES:
            raise ValueError("more than %d zones" % L.TM_ADMIT_MAX_ZONES)
        if acl_nomatch not in ("allow", "deny"):
            raise ValueError(acl_nomatch)
        self.names.append(name)
        self.caps.append(L.TmZoneCaps(int(max_qos_allowed), int(bool(retain_available)), int(bool(enable_acl)),
                                      int(acl_nomatch == "allow"), int(max_topic_alias), 0))
        return len(self.caps) - 1

    def index(self, name):
        return self.names.index(name)

    def __len__(self):
        return len(self.caps)

    def table(self):
        """-> (ctypes array of TmZoneCaps, count) for the batch calls"""
        return (L.TmZoneCaps * max(len(self.caps), 1))(*self.caps), len(self.caps)


def pub_admit(zone=0, is_super=False, alias=None):
    """the per-publish admission word: zone index, is_super, Topic-Alias
    (None = the property is absent; an alias of 0 cannot be told from that,
    and the codec refuses it before this stage)"""
    return (zone & 0xFF) | (L.TM_ADMIT_SUPER if is_super else 0) | ((alias or 0) << L.TM_ADMIT_ALIAS_SHIFT)


def admit_code(topic, qos, retain, zones, zone=0, is_super=False, alias=None, acl="nomatch"):
    """tm_admit_code for one publish: `topic` as the client sent it
    (unmounted), acl one of "allow" / "deny" / "nomatch" (or 1 / 0 / -1)"""
    lib = L.load()
    t = _b(topic)
    a = {"allow": 1, "deny": 0, "nomatch": -1}.get(acl, acl)
    flags = (qos & 3) | (L.TM_MSG_RETAIN if retain else 0)
    return int(lib.tm_admit_code(t, len(t), flags, pub_admit(zone, is_super, alias),
                                 ctypes.byref(zones.caps[zone]), int(a)))
