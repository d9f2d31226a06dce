"""The cases of tests/acl_corpus.py through both ACL entries of acl.hip,
tm_acl_check_batch (host buffers) and tm_acl_check_batch_device (device
buffers, on a side stream), result and rule index against
oracle/pyacl.py:check_acl and against each other:

    a  every who shape: flat and nested and/or up to the stack limit, one leaf deciding
    b  every CIDR prefix, the range's edges, family mismatches, no peername
    c  the thinned byte corpus: bytes >= 0x80, words up to 65,535 bytes, 2,000 levels,
       credentials that look like wildcards and variables
    d  batch sizes around the 256-thread block; no rule output; no peers
    e  offsets that do not start at 0, '/' all around (host: rebased; device: absolute)
    f  rules added between two checks (the re-upload), and 2,000 rules / a 97 KiB arena

The rejected buffer combinations are tested for their status code on the CPU
(tests/test_acl_corpus.py); none reaches a device call here."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import acl_corpus as A  # noqa: E402
import byte_corpus as C  # noqa: E402
from emqx_amd.emqx_access import AclRules  # noqa: E402
from oracle import pyacl  # noqa: E402

pytestmark = pytest.mark.gpu

CODE = {"allow": 1, "deny": 0, "nomatch": -1}
NO_RULE = 0xFFFFFFFF


def _show(t):
    return repr(t) if len(t) <= 80 else "%r... (%d bytes)" % (t[:80], len(t))


def _oracle(rules, checks):
    """compiled rules x checks -> (result int8[n], rule u32[n])"""
    res = np.zeros(len(checks), dtype=np.int8)
    idx = np.zeros(len(checks), dtype=np.uint32)
    with A.deep():
        for i, (cred, pubsub, topic) in enumerate(checks):
            r, k = pyacl.check_acl(rules, A.oracle_cred(cred), pubsub, topic)
            res[i], idx[i] = CODE[r], NO_RULE if k is None else k
    return res, idx


def _pack(checks):
    return AclRules.pack([c for c, _, _ in checks], [p for _, p, _ in checks], [t for _, _, t in checks])


def _device(a, arrs, n, dev, want_rule=True):
    """tm_acl_check_batch_device on a side stream, synchronised before the read"""
    import torch
    d = torch.device("cuda", dev)
    t = {k: (None if v is None else
             torch.from_numpy(np.ascontiguousarray(v).view(np.int64 if v.dtype == np.uint64 else v.dtype).copy()).to(d))
         for k, v in arrs.items()}
    d_out = torch.full((max(n, 1),), -7, dtype=torch.int8, device=d)
    d_rule = torch.full((max(n, 1),), -9, dtype=torch.int32, device=d) if want_rule else None
    side = torch.cuda.Stream(device=d)
    a.check_device(n, t, d_out, d_rule, stream=side)
    side.synchronize()
    out = d_out.cpu().numpy()[:n]
    return out, (d_rule.cpu().numpy().view(np.uint32)[:n] if want_rule else None)


def _agree(tag, checks, got, want):
    res, idx = got
    wres, widx = want
    for i, (cred, pubsub, topic) in enumerate(checks):
        if res[i] != wres[i] or (idx is not None and idx[i] != widx[i]):
            raise AssertionError("%s: check %d %r %s %s: got (%d, %s) want (%d, %d)"
                                 % (tag, i, cred if len(repr(cred)) < 200 else "(long credentials)", pubsub,
                                    _show(topic), res[i], None if idx is None else int(idx[i]), wres[i], widx[i]))
    assert len(res) == len(checks)


def _both(tag, a, dev, checks, want, arrs=None):
    """host entry and device entry against the oracle, and against each other"""
    n = len(checks)
    arrs = _pack(checks) if arrs is None else arrs
    host = a.check_packed(n, arrs)
    _agree(tag + " (host entry)", checks, host, want)
    device = _device(a, arrs, n, dev)
    _agree(tag + " (device entry)", checks, device, want)
    assert np.array_equal(host[0], device[0]) and np.array_equal(host[1], device[1]), tag


# ---- a. who shapes ---------------------------------------------------------------------

def test_who_shapes_vs_oracle(gpu_device):
    cases = A.who_shapes()
    seen = set()
    for at in range(0, len(cases), 48):                       # one rule set per 48 shapes: rule i asks for topic w/i
        part = cases[at:at + 48]
        rules = [(("allow", "deny")[i % 2], c.who, "pubsub", [b"w/%d" % i]) for i, c in enumerate(part)]
        checks = [(cred, ("publish", "subscribe")[(i + j) % 2], b"w/%d" % i)
                  for i, c in enumerate(part) for j, cred in enumerate(c.creds)]
        want = _oracle([pyacl.compile_rule(r) for r in rules], checks)
        a = AclRules(gpu_device).load(rules)
        try:
            _both("who shapes %s.." % part[0].name, a, gpu_device, checks, want)
        finally:
            a.close()
        seen.update(want[0].tolist())
    assert seen == {1, 0, -1}


# ---- b. CIDRs --------------------------------------------------------------------------------

def test_cidr_cases_vs_oracle(gpu_device):
    cases = A.cidr_cases()
    rules = [("allow", ("ipaddr", text), "pubsub", [b"c/%d" % i]) for i, (_, text, _) in enumerate(cases)]
    checks = [(cred, "publish", b"c/%d" % i) for i, (_, _, cred) in enumerate(cases)]
    want = _oracle([pyacl.compile_rule(r) for r in rules], checks)
    assert 40 < int((want[0] == 1).sum()) < len(cases) - 40
    a = AclRules(gpu_device).load(rules)
    try:
        _both("cidr", a, gpu_device, checks, want)
        got = a.check_packed(len(checks), _pack(checks))[0]
        for (name, text, cred), g, w in zip(cases, got, want[0]):
            assert g == w, (name, text, cred)
    finally:
        a.close()


# ---- c. the byte corpus -------------------------------------------------------------------------

class _Bytes:
    def __init__(self, dev):
        self.set = A.byte_checks()
        self.checks = self.set.checks
        self.compiled = [pyacl.compile_rule(r) for r in self.set.rules]
        self.want = _oracle(self.compiled, self.checks)
        self.acl = AclRules(dev).load(self.set.rules)

    def cut(self, n):
        return self.checks[:n], (self.want[0][:n], self.want[1][:n])


@pytest.fixture(scope="module")
def world(gpu_device):
    w = _Bytes(gpu_device)
    yield w
    w.acl.close()


def test_byte_checks_vs_oracle(world, gpu_device):
    assert set(world.want[0].tolist()) == {1, 0, -1}
    assert len({int(k) for k in world.want[1] if k != NO_RULE}) > 60      # (tests/test_acl_corpus.py pins the kinds)
    _both("byte checks", world.acl, gpu_device, world.checks, world.want)


# ---- d. batch sizes, no rule output, no peers -------------------------------------------------------

@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_batch_sizes_around_the_block(world, gpu_device, n):
    checks, want = world.cut(n)
    _both("first %d byte checks" % n, world.acl, gpu_device, checks, want)
    # the same batch without the rule output
    arrs = _pack(checks)
    res, rule = world.acl.check_packed(n, arrs, want_rule=False)
    assert rule is None
    _agree("first %d, out_rule NULL (host entry)" % n, checks, (res, None), want)
    res, rule = _device(world.acl, arrs, n, gpu_device, want_rule=False)
    _agree("first %d, d_out_rule NULL (device entry)" % n, checks, (res, None), want)


def test_no_peers_reads_as_no_peername(world, gpu_device):
    assert "ipaddr" in world.set.wkind
    checks, with_peers = world.cut(257)
    bare = [({k: v for k, v in c.items() if k != "peername"}, p, t) for c, p, t in checks]
    want = _oracle(world.compiled, bare)
    assert not np.array_equal(want[1], with_peers[1])          # some first match hung on an address
    arrs = dict(_pack(checks), peers=None, peer_family=None)
    _both("peers = peer_family = NULL", world.acl, gpu_device, bare, want, arrs=arrs)


# ---- e. offsets that do not start at 0 -----------------------------------------------------------------

def _enveloped(checks, leads):
    arrs = _pack(checks)
    ids = [c.get("client_id") or b"" for c, _, _ in checks]
    usr = [c.get("username") or b"" for c, _, _ in checks]
    for key, off, items, lead in (("topics", "topic_off", [t for _, _, t in checks], leads[0]),
                                  ("client_ids", "client_off", ids, leads[1]),
                                  ("usernames", "user_off", usr, leads[2])):
        arrs[key], arrs[off] = C.envelope(items, lead)
        assert int(arrs[off][0]) == lead and bytes(arrs[key][:lead]) == b"/" * lead
    return arrs


@pytest.mark.parametrize("leads", [(5, 3, 7), (8, 1, 0)])
def test_offsets_into_an_envelope(world, gpu_device, leads):
    """the host entry rebases topic_off / client_off / user_off; the device entry
    takes them as absolute offsets into its buffers; every byte around is '/'"""
    arrs = _enveloped(world.checks, leads)
    _both("envelope leads %s" % (leads,), world.acl, gpu_device, world.checks, world.want, arrs=arrs)


# ---- f. growing and large rule sets ---------------------------------------------------------------------

@pytest.mark.parametrize("entry", ["host", "device"])
def test_rules_added_between_checks(world, gpu_device, entry):
    checks, before = world.cut(257)
    more = [("allow", ("client", "all"), "publish", [b"+/#", ("eq", b"")]), ("deny", "all")]
    after = _oracle(world.compiled + [pyacl.compile_rule(r) for r in more], checks)
    n0 = len(world.set.rules)
    assert {n0, n0 + 1} <= set(after[1].tolist()) and NO_RULE not in after[1] and NO_RULE in before[1]
    a = AclRules(gpu_device).load(world.set.rules)
    arrs = _pack(checks)

    def run():
        return a.check_packed(len(checks), arrs) if entry == "host" else _device(a, arrs, len(checks), gpu_device)
    try:
        _agree("before the add (%s entry)" % entry, checks, run(), before)
        for r in more:
            a.add(r)
        _agree("after the add (%s entry)" % entry, checks, run(), after)
    finally:
        a.close()


def test_late_rule_of_a_large_set(gpu_device):
    rules, late, checks = A.late_rule_set()
    want = _oracle([pyacl.compile_rule(r) for r in rules], checks)
    assert set(want[1].tolist()) == {late, NO_RULE}
    a = AclRules(gpu_device).load(rules)
    try:
        _both("2,000 rules", a, gpu_device, checks, want)
    finally:
        a.close()
