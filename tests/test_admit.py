"""Publish admission on the CPU: tm_admit_code and tm_admit_batch (a host loop,
no device) against tests/admit_ref.py, the literal transcription of
emqx_packet:validate/1, emqx_mqtt_caps:check_pub/2 and check_pub_acl, and
against the reference's own known answers (tests/golden/kat_admit.json)."""
import ctypes
import json
import os
from collections import Counter

import numpy as np
import pytest

import admit_corpus as AC
import admit_ref
from emqx_amd import Engine
from emqx_amd import _lib as L
from emqx_amd.emqx_access import ADMIT, Zones, admit_code, pub_admit

HERE = os.path.dirname(os.path.abspath(__file__))


def _code(c, zones):
    return admit_code(c["topic"], c["qos"], c["retain"], zones, c["zone"], c["is_super"], c["alias"], c["acl"])


def test_known_answers():
    with open(os.path.join(HERE, "golden", "kat_admit.json")) as f:
        kat = json.load(f)
    caps = kat["check_pub"]["caps"]
    zone = dict(admit_ref.DEFAULT_ZONE, **caps)
    zones = AC.zones_table([zone])
    assert len(kat["check_pub"]["cases"]) == 4
    for k in kat["check_pub"]["cases"]:
        props = {"qos": k["qos"], "retain": k["retain"]}
        if k["topic_alias"] is not None:
            props["topic_alias"] = k["topic_alias"]
        r = admit_ref.check_pub(zone, props)
        assert (0 if r == "ok" else r) == k["code"], k["name"]
        c = AC.case(b"t", qos=k["qos"], retain=k["retain"], alias=k["topic_alias"], acl="allow")
        assert AC.want(c, [zone]) == k["code"] == _code(c, zones), k["name"]
    assert len(kat["topic_name_invalid"]) == 2
    dflt = AC.zones_table([admit_ref.DEFAULT_ZONE])
    for k in kat["topic_name_invalid"]:
        c = AC.case(k["topic"].encode(), qos=k["qos"], acl="allow")
        assert admit_ref.validate(c["topic"], {}) == "topic_name_invalid"
        assert AC.want(c, [admit_ref.DEFAULT_ZONE]) == k["code"] == _code(c, dflt) == 1


def test_cross_product():
    cases = AC.product()
    zones = AC.zones_table()
    want = [AC.want(c) for c in cases]
    hist = Counter(want)
    for code in range(6):
        assert hist[code] >= 20, (code, hist)
    # the topic classes, stated outright
    for t in AC.NOT_WILD + [b"/", b"t/" + b"x" * 4095]:
        assert admit_ref.validate(t, {}) is True, t
    for t in AC.WILD + [b"", b"$SYS/+"]:
        assert admit_ref.validate(t, {}) == "topic_name_invalid", t
    # the batch form over the whole product, topics mounted
    a = AC.arrays(cases)
    code, hdr = Engine.admit_batch(a["buf"], a["off"], a["pub_flags"], zones, a["mount_len"], a["pub_admit"], a["acl"])
    bad = np.nonzero(code != np.array(want, dtype=np.uint8))[0]
    assert len(bad) == 0, (cases[bad[0]], int(code[bad[0]]), want[bad[0]])
    assert [int(x) for x in hdr] == admit_ref.header(want)
    # offsets that do not start at 0, and the NULL forms: no mount, zone 0 / not super / no alias, every check nomatch
    sub = [c for c in cases if c["mount"] == b"" and c["zone"] == 0 and not c["is_super"] and c["alias"] is None
           and c["acl"] == "nomatch"]
    assert len(sub) >= 60
    a = AC.arrays(sub, lead=5)
    code, hdr = Engine.admit_batch(a["buf"], a["off"], a["pub_flags"], zones)
    assert [int(x) for x in code] == [AC.want(c) for c in sub]
    assert [int(x) for x in hdr] == admit_ref.header(code)


def test_every_single_check_the_product_takes():
    """tm_admit_code, one publish at a time, over the whole product"""
    cases = AC.product()
    zones = AC.zones_table()
    lib = L.load()
    for c in cases:
        t = c["topic"]
        flags = c["qos"] | (4 if c["retain"] else 0)
        got = lib.tm_admit_code(t, len(t), flags, pub_admit(c["zone"], c["is_super"], c["alias"]),
                                ctypes.byref(zones.caps[c["zone"]]), AC.ACL_INT[c["acl"]])
        assert got == AC.want(c), c


def test_precedence():
    """one publish that fails all five checks gets code 1; removing the failures one at a time gives 2, 3, 4, 5, 0"""
    zone = dict(max_qos_allowed=0, max_topic_alias=4, mqtt_retain_available=False, enable_acl=True,
                acl_nomatch="deny")
    zones = AC.zones_table([zone])
    c = AC.case(b"a/+", qos=2, retain=True, alias=5, acl="deny")
    steps = [{}, dict(topic=b"a/b"), dict(qos=0), dict(alias=4), dict(retain=False), dict(acl="allow")]
    for want, change in zip((1, 2, 3, 4, 5, 0), steps):
        c.update(change)
        assert AC.want(c, [zone]) == want == _code(c, zones), (want, c)
        a = AC.arrays([c])
        code, hdr = Engine.admit_batch(a["buf"], a["off"], a["pub_flags"], zones, a["mount_len"], a["pub_admit"],
                                       a["acl"])
        assert int(code[0]) == want and int(hdr[want]) == 1 and int(hdr.sum()) == 1
    assert ADMIT[1] == "topic_name_invalid" and ADMIT[5] == "not_authorized"
    # nomatch follows the zone's acl_nomatch; is_super and enable_acl = false pass a deny
    c.update(acl="nomatch")
    assert _code(c, zones) == 5
    assert _code(c, AC.zones_table([dict(zone, acl_nomatch="allow")])) == 0
    c.update(acl="deny")
    assert _code(dict(c, is_super=True), zones) == 0
    assert _code(c, AC.zones_table([dict(zone, enable_acl=False)])) == 0


def test_argument_errors():
    zones = AC.zones_table()
    a = AC.arrays([AC.case(b"a/b", b"m/", qos=1, zone=3, acl="allow"), AC.case(b"c")])

    def run(zones=zones, **kw):
        b = dict(a, **kw)
        return Engine.admit_batch(b["buf"], b["off"], b["pub_flags"], zones, b["mount_len"], b["pub_admit"], b["acl"])
    code, _ = run()
    assert list(code) == [0, 5]

    def einval(**kw):
        with pytest.raises(L.TopicMatchError) as ei:
            run(**kw)
        assert ei.value.code == L.TM_EINVAL
    einval(pub_admit=np.array([len(zones), 0], dtype=np.uint32))            # a zone index >= n_zones
    einval(pub_admit=np.array([0, 255], dtype=np.uint32))
    einval(pub_flags=np.array([3, 0], dtype=np.uint32))                      # QoS 3
    einval(pub_flags=np.array([0, 7], dtype=np.uint32))
    einval(mount_len=np.array([6, 0], dtype=np.uint32))                      # past the topic ("m/a/b" is 5 bytes)
    einval(off=np.array([0, 5, 4], dtype=np.uint64))                         # decreasing offsets
    einval(zones=Zones())                                                    # no zone at all
    assert list(run(mount_len=np.array([5, 0], dtype=np.uint32))[0]) == [1, 5]   # the whole topic is mountpoint: empty
    lib = L.load()
    # tm_admit_code has no error channel but its code
    z0 = ctypes.byref(zones.caps[0])
    assert lib.tm_admit_code(b"a", 1, 3, 0, z0, 1) == L.TM_ADMIT_BAD_ARG == 0xFFFFFFFF
    assert lib.tm_admit_code(b"a", 1, 0, 0, None, 1) == L.TM_ADMIT_BAD_ARG
    assert lib.tm_admit_code(b"a", 1, 2, 0, z0, 1) == 0
    tab, nz = zones.table()
    ok = (ctypes.c_void_p(a["buf"].ctypes.data), ctypes.c_void_p(a["off"].ctypes.data), 2, None,
          ctypes.c_void_p(a["pub_flags"].ctypes.data), None)
    out = np.zeros(2, np.uint8)
    assert lib.tm_admit_batch(*ok, tab, nz, None, ctypes.c_void_p(out.ctypes.data), None) == L.TM_OK   # hdr may be NULL
    assert lib.tm_admit_batch(*ok, tab, L.TM_ADMIT_MAX_ZONES + 1, None, ctypes.c_void_p(out.ctypes.data),
                              None) == L.TM_EINVAL
    assert lib.tm_admit_batch(*ok, None, nz, None, ctypes.c_void_p(out.ctypes.data), None) == L.TM_EINVAL
    assert lib.tm_admit_batch(*ok, tab, nz, None, None, None) == L.TM_EINVAL
    assert lib.tm_admit_batch(None, None, 0, None, None, None, tab, nz, None, None, None) == L.TM_OK    # n == 0
    # the device forms check their host arguments before they touch a device
    assert lib.tm_admit_batch_device(None, None, 0, None, None, None, tab, nz, None, None, None, None) == L.TM_EINVAL
    assert lib.tm_admit_batch_device(None, None, 0, None, None, None, None, nz, None, None,
                                     ctypes.c_void_p(out.ctypes.data), None) == L.TM_EINVAL
    e = Engine(device=-1)
    caps = L.TmPublishCaps(8, 8, 8, 8)
    one = ctypes.c_void_p(out.ctypes.data)          # any non-NULL address: the checks come before any use
    plain = [e.h, one, one, 1, 1, Engine.SHARE_ROUND_ROBIN, None, None, ctypes.byref(caps), one, 1 << 30, one, one,
             one, one, one]
    assert e.lib.tm_publish_stream_gated_device(*plain, None, one, one, None) == L.TM_EINVAL   # a pick-word plane, no deliver
    assert e.lib.tm_publish_stream_gated_device(*plain, None, None, one, None) == L.TM_EDEVICE  # host-only engine
    e.close()
