"""The publish lane's exact-size read-back on the GPU: one batch of more than
32,768 publishes reads the headers first and then exactly what they count.
tests/test_gpu_publish_stream_opts.py covers that for the options mode; here
the same batch goes through a batcher opened with OPTS | INBOX | FORWARD |
ADMIT, a handful of refused publishes among the 33,000 -- the inbox plan
against the model's sends, the forward plan against the records the
per-publish callbacks carried, codes and rules against tests/admit_ref.py and
the Python ACL matcher, every publish of a kind with that kind's answer --
and once through the bare keyed batcher against Engine.match_publish_batch."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import admit_corpus as AC  # noqa: E402
import admit_ref  # noqa: E402
from acl_util import oracle_cred  # noqa: E402
from forward_ref import expected_plan  # noqa: E402
from inbox_ref import grouped, grouped_plan, reference_sends  # noqa: E402
from pickword_ref import outcome_word, route_pick_words  # noqa: E402
from pickword_world import NODE, build_world, publishes  # noqa: E402
from publish_util import slices  # noqa: E402
from test_gpu_batcher_forward import Sink  # noqa: E402
from emqx_amd import Engine  # noqa: E402
from emqx_amd import _lib as L  # noqa: E402
from emqx_amd.batcher import Batcher  # noqa: E402
from emqx_amd.emqx_access import AclRules, pub_admit  # noqa: E402
from emqx_amd.emqx_broker import pack_msgs  # noqa: E402
from emqx_amd.emqx_router import _enc  # noqa: E402
from emqx_amd.engine import pack  # noqa: E402
from oracle import pyacl  # noqa: E402

pytestmark = pytest.mark.gpu

N = 33_000
RULES = [("deny", ("user", "bad"), "publish", ["#"]), ("allow", "all", "publish", ["#"])]
ZONES = [dict(admit_ref.DEFAULT_ZONE),
         dict(max_qos_allowed=1, max_topic_alias=0, mqtt_retain_available=True, enable_acl=True, acl_nomatch="deny")]
GOOD = {"client_id": "c1", "username": "u1", "peername": ("10.1.2.3", 1883)}
BAD = {"client_id": "c2", "username": "bad", "peername": None}
MOUNT = b"tenant/7/"
# index -> (topic, mount_len, creds, msg, zone): one refusal of each kind, on both sides of the 32,768th publish
REFUSED = {
    7: (b"w0/z", 0, GOOD, (2, 0, 0, None), 1),                      # QoS 2 where the zone allows 1
    4_999: (b"p0/t", 0, BAD, (0, 0, 0, None), 0),                   # the ACL denies this user
    32_767: (b"p0/+", 0, GOOD, (1, 0, 0, None), 0),                 # a wildcard in a topic name
    32_768: (MOUNT, len(MOUNT), GOOD, (0, 0, 0, None), 0),          # an empty topic behind its mountpoint
    32_999: (b"x1/t", 0, BAD, (1, 1, 0, None), 1),
}


@pytest.fixture(scope="module")
def world(gpu_device):
    w = build_world(gpu_device)
    w.e.commit()
    acl = AclRules(gpu_device).load(RULES)
    base = publishes(w)
    # two publishers picked as the no-local member of their set; a picked member that gets the message, its id
    # above 65535 (the lane's first sort width: the plan runs again alone); plain topics; a topic nobody wants
    kinds = [base[0], base[28], base[5], base[-1], base[-4], (b"nothing/at/all", 1, (1, 0, 0, None))]
    assert kinds[1][0] == b"x5/t" and kinds[1][2][3] > 65535
    yield w, acl, kinds
    acl.close()
    w.close()


def test_every_mode_past_the_read_back_threshold(world):
    w, acl, kinds = world
    assert all(i >= len(kinds) for i in REFUSED)
    # (topic, mount_len, creds, key, msg, zone)
    pubs = [REFUSED[i][:3] + (i,) + REFUSED[i][3:] if i in REFUSED else
            (kinds[i % len(kinds)][0], 0, GOOD, kinds[i % len(kinds)][1], kinds[i % len(kinds)][2], 0) for i in range(N)]
    sink = Sink()
    b = Batcher(w.e, max_topics=40_000, deadline_us=5_000_000, publish=True, opts=True, lanes_per_replica=1,
                inbox=sink.on_inbox, forward=sink.on_forward, admit=(AC.zones_table(ZONES), acl))
    pf, fr = pack_msgs([p[4] for p in pubs])
    tickets = [b.submit_publish_admit(t, ml, int(key), int(pf[i]), pub_admit(zone), int(fr[i]), cred, sink.on_pub(i))
               for i, (t, ml, cred, key, _msg, zone) in enumerate(pubs)]
    b.flush()
    st = b.stats()
    b.close()
    assert st["batches"] == 1 and st["max_batch"] == N and st["failed_batches"] == 0 and st["refused"] == len(REFUSED)
    assert st["reruns"] >= 1                                          # the inbox plan, at the width of the wide id
    assert len(sink.pubs) == N and len(sink.inboxes) == 1 and len(sink.plans) == 1
    # codes and rules: admit_ref over the Python ACL matcher's answer, once per distinct publish
    compiled = [pyacl.compile_rule(r) for r in RULES]
    memo = {}

    def want(t, ml, cred, msg, zone):
        k = (t, ml, cred["username"], msg[:2], zone)
        if k not in memo:
            ans, idx = pyacl.check_acl(compiled, oracle_cred(cred), "publish", t[ml:])
            memo[k] = (admit_ref.admit(t[ml:], msg[0], bool(msg[1]), None, ZONES[zone], False, ans), idx)
        return memo[k]
    codes = []
    for i, (t, ml, cred, _key, msg, zone) in enumerate(pubs):
        code, rule = want(t, ml, cred, msg, zone)
        assert sink.pubs[i][0] == L.TM_OK and sink.pubs[i][5:] == (code, rule), i
        assert (code != 0) == (i in REFUSED), i
        codes.append(code)
    assert sorted({codes[i] for i in REFUSED}) == [admit_ref.TOPIC_NAME, admit_ref.QOS, admit_ref.ACL]
    # a refused publish carries nothing; every admitted one carries its kind's answer, and the kinds the model's
    for i in range(N):
        if codes[i]:
            assert sink.pubs[i][1:5] == ([], [], None, 0), i
        else:
            assert sink.pubs[i][:5] == sink.pubs[i % len(kinds)][:5], i
    want_pairs = w.want_pairs(kinds)
    for k, (topic, key, msg) in enumerate(kinds):
        rows = route_pick_words(w.o, w.sh, w.so, "keyed", int(key), topic, msg, False)
        _status, deliv, pick_words, pairs, n_pairs = sink.pubs[k][:5]
        assert [d[3] for d in deliv] == [Engine.NO_MEMBER if m is None else m for m, _oc in rows], k
        assert pick_words == [outcome_word(oc) for _m, oc in rows], k
        assert pairs is None and n_pairs == len(want_pairs[k]), k
    assert any(want_pairs) and any(x != L.TM_NO_WORD for k in range(len(kinds)) for x in sink.pubs[k][2])
    # the inbox plan: the model's sends of each kind (keyed picks: a publish's sends do not depend on its batch),
    # at every admitted publish of that kind, in the batch's ticket order
    index = {t: i for i, t in enumerate(tickets)}
    tk, hdr, inbox, ent_pub, ent_to, ent_word = sink.inboxes[0]
    order = [index[t] for t in tk]
    assert sorted(order) == list(range(N))
    per_kind = [reference_sends(w.o, w.so, w.sh, NODE, "keyed", [kd]) for kd in kinds]
    sends = [(sub, p, kind, pos, to, word) for p, i in enumerate(order) if not codes[i]
             for sub, _p, kind, pos, to, word in per_kind[i % len(kinds)]]
    ref = grouped(sends)
    name = lambda to, pub: w.to_bytes(to, pubs[order[pub]][0])   # noqa: E731
    assert grouped_plan(inbox, ent_pub, ent_to, ent_word, name) == ref
    picks = sum(1 for s in sends if s[2])
    assert hdr == [len(sends), len(ref), len(sends) - picks, picks] and picks > 5000 and len(sends) - picks > N
    # the forward plan: the TM_NOT_LOCAL node records the per-publish callbacks carried, grouped per (node, To)
    remote = {w.e.dest_target(_enc(nm), Engine.TARGET_NODE, nm.encode()) for nm in ("n2", "n3")}
    tk, hdr, groups, pub = sink.plans[0]
    assert [index[t] for t in tk] == order
    triples = [(target, to, p) for p, i in enumerate(order) for to, target, ndisp, _pick in sink.pubs[i][1]
               if ndisp == Engine.NOT_LOCAL and target in remote]
    assert (hdr, groups, pub) == expected_plan(triples) and hdr[0] > N and hdr[2] == 2


def test_bare_keyed_batch_past_the_read_back_threshold(world):
    w, _acl, kinds = world
    got = [None] * N
    b = Batcher(w.e, max_topics=40_000, deadline_us=5_000_000, publish=True, lanes_per_replica=1)
    for i in range(N):
        def cb(status, deliveries, pairs, i=i):
            got[i] = (status, deliveries, pairs) if got[i] is None else "twice"
        b.submit_publish(kinds[i % len(kinds)][0], int(kinds[i % len(kinds)][1]), cb)
    b.flush()
    st = b.stats()
    b.close()
    assert st["batches"] == 1 and st["max_batch"] == N and st["failed_batches"] == 0
    buf, off = pack([k[0] for k in kinds])
    keys = np.asarray([k[1] for k in kinds], dtype=np.uint32)
    want = slices(w.e.match_publish_batch(buf, off, Engine.SHARE_KEYED, keys), len(kinds))
    assert any(d for d, _p in want) and any(p for _d, p in want)
    assert st["results"] == sum(len(want[i % len(kinds)][0]) for i in range(N))
    for i in range(N):
        assert got[i] == (0, want[i % len(kinds)][0], want[i % len(kinds)][1]), i
