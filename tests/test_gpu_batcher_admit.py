"""The batcher's admission mode on the GPU (TM_BATCHER_PUBLISH | OPTS | ADMIT):
keyed, ROUND_ROBIN with one lane, and INBOX | FORWARD.  A few hundred
single-topic publishes with all six codes, two zones and some mountpoints go
through tm_batcher_submit_publish_admit; the rule set holds a %c pattern, so the
credentials matter.  Every callback's code and rule against tests/admit_ref.py
and the Python ACL matcher; the admitted publishes' records and words against
an options batcher (tm_publish_stream_opts_device) fed the admitted publishes
alone; the refused ones with zero counts; round-robin picks over the admitted
publishes in submission order; stats().refused."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import admit_corpus as AC  # noqa: E402
from test_gpu_publish_admitted import RULES, ZONES, _publishes, _want  # noqa: E402
from emqx_amd import Engine  # noqa: E402
from emqx_amd import _lib as L  # noqa: E402
from emqx_amd.batcher import Batcher  # noqa: E402
from emqx_amd.emqx_access import AclRules, pub_admit  # noqa: E402
from emqx_amd.emqx_broker import Broker  # noqa: E402
from emqx_amd.emqx_router import Router  # noqa: E402

pytestmark = pytest.mark.gpu
MEMBERS = [301, 302, 303]


@pytest.fixture(scope="module")
def world(gpu_device):
    e = Engine(device=gpu_device)
    b = Broker(e, Router(e, node="n1"))
    for i, f in enumerate([b"dev/+/up", b"dev/#", b"open/#", b"open/a", b"s/t", b"tenant/+/open/#", b"other/x"]):
        b.subscribe(f, 100 + i, opts={"qos": i % 3})
        if i % 2 == 0:
            b.subscribe(f, 200 + i)
    for m in MEMBERS:
        b.subscribe(b"open/#", m, group="g")
    b.router.add_route(b"open/#", "n2")              # a remote node: the forward plan has something to group
    b.router.add_route(b"dev/+/up", "n3")
    e.commit()
    acl = AclRules(gpu_device).load(RULES)
    yield e, acl
    acl.close()
    e.close()


def _submit_all(bt, pubs, keys, admit=True):
    got = {}
    for i, (t, ml, cred, (qos, retain), (zone, sup, alias)) in enumerate(pubs):
        flags = qos | (4 if retain else 0)
        cb = lambda *a, i=i: got.setdefault(i, []).append(a)   # noqa: E731
        if admit:
            bt.submit_publish_admit(t, ml, keys[i], flags, pub_admit(zone, sup, alias), 0xFFFFFFFF, cred, cb)
        else:
            bt.submit_publish_opts(t, keys[i], flags, 0xFFFFFFFF, cb)
    bt.flush()
    assert sorted(got) == list(range(len(pubs))) and all(len(v) == 1 for v in got.values())
    return [got[i][0] for i in range(len(pubs))]


def _check_codes(res, pubs):
    want_codes, want_rules = _want(pubs)
    assert [r[0] for r in res] == [L.TM_OK] * len(pubs)
    assert [r[5] for r in res] == want_codes and [r[6] for r in res] == want_rules
    assert sorted(set(want_codes)) == [0, 1, 2, 3, 4, 5]
    assert any(p[1] for p in pubs) and {p[4][0] for p in pubs} == {0, 1}            # mountpoints, two zones
    return want_codes


@pytest.mark.parametrize("mode", ["keyed", "round_robin"])
def test_codes_rules_and_records(world, mode):
    e, acl = world
    zones = AC.zones_table(ZONES)
    pubs = _publishes()
    keys = [(i * 2654435761) % 2 ** 32 for i in range(len(pubs))]
    kw = dict(round_robin=True, lanes_per_replica=1) if mode == "round_robin" else {}
    bt = Batcher(e, publish=True, opts=True, admit=(zones, acl), max_topics=128, **kw)
    res = _submit_all(bt, pubs, keys)
    codes = _check_codes(res, pubs)
    refused = sum(1 for c in codes if c)
    st = bt.stats()
    assert st["refused"] == refused and st["topics"] == len(pubs) and st["failed_batches"] == 0 and st["batches"] >= 3
    bt.close()
    for r, c in zip(res, codes):
        if c:
            assert r[1:5] == ([], [], [], [])                                           # zero counts, no arrays
    # the admitted publishes alone through an options batcher: tm_publish_stream_opts_device on the admitted topics
    keep = [i for i, c in enumerate(codes) if c == 0]
    ref_b = Batcher(e, publish=True, opts=True, max_topics=128, **kw)
    ref = _submit_all(ref_b, [pubs[i] for i in keep], [keys[i] for i in keep], admit=False)
    ref_b.close()
    for i, want in zip(keep, ref):
        assert res[i][:5] == want[:5], i
    assert any(r[3] for r in ref) and any(w != L.TM_NO_WORD for r in ref for w in r[2])
    if mode == "round_robin":       # one lane is one publisher: the set's members in turn over the admitted publishes
        picks = [d[3] for i in keep for d in res[i][1] if d[3] in MEMBERS]
        assert len(picks) > 20 and picks == [MEMBERS[k % 3] for k in range(len(picks))]


def test_inbox_and_forward_plans_hold_no_refused_publish(world):
    e, acl = world
    zones = AC.zones_table(ZONES)
    pubs = _publishes()
    keys = list(range(len(pubs)))
    plans = {"i": [], "f": []}

    def inbox(st, tickets, hdr, rows, ent_pub, ent_to, ent_word):
        plans["i"].append((st, [int(t) for t in tickets], [int(tickets[int(p) & 0x7FFFFFFF]) for p in ent_pub]))

    def forward(st, tickets, hdr, groups, pub):
        plans["f"].append((st, [int(t) for t in tickets], [int(tickets[int(p)]) for p in pub]))
    bt = Batcher(e, publish=True, opts=True, admit=(zones, acl), max_topics=128, lanes_per_replica=1, inbox=inbox,
                 forward=forward)
    tickets, got = [], {}
    for i, (t, ml, cred, (qos, retain), (zone, sup, alias)) in enumerate(pubs):
        tickets.append(bt.submit_publish_admit(t, ml, keys[i], qos | (4 if retain else 0), pub_admit(zone, sup, alias),
                                               0xFFFFFFFF, cred, lambda *a, i=i: got.setdefault(i, []).append(a)))
    bt.flush()
    res = [got[i][0] for i in range(len(pubs))]
    codes = _check_codes(res, pubs)
    assert bt.stats()["refused"] == sum(1 for c in codes if c)
    bt.close()
    refused = {tickets[i] for i, c in enumerate(codes) if c}
    admitted = set(tickets) - refused
    for kind in ("i", "f"):
        assert plans[kind] and all(st == L.TM_OK for st, _, _ in plans[kind])
        listed = [t for _, tk, _ in plans[kind] for t in tk]
        assert sorted(listed) == sorted(tickets)                      # tickets[] still lists every publish of its batch
        used = {t for _, _, ents in plans[kind] for t in ents}
        assert used and used <= admitted and not used & refused
    for r, c in zip(res, codes):                                      # inbox mode: the pairs are in the plan, their count here
        if c:
            assert r[1] == [] and r[2] == [] and r[3] is None and r[4] == 0
    with_pairs = {tickets[i] for i, r in enumerate(res) if not codes[i] and r[4]}
    assert with_pairs and with_pairs <= {t for _, _, ents in plans["i"] for t in ents}
