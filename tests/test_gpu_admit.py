"""tm_admit_batch_device on the GPU against tests/admit_ref.py, code for code
and header for header: the CPU corpus of tests/admit_corpus.py (the full
product the checks branch on), tests/byte_corpus.py's fixed and random-byte
topics (all 256 byte values, '/' at every offset mod 8, levels of 7-9 and 15-17
bytes, the wave batches on the LDS window's limit), the batch sizes around the
wave and block edges, and a buffer whose topics start at an offset that is no
multiple of 8.  64 guard elements after d_code and d_hdr are pre-filled and
must come back unchanged."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import admit_corpus as AC  # noqa: E402
import admit_ref  # noqa: E402
import byte_corpus as C  # noqa: E402
from emqx_amd import Engine  # noqa: E402

pytestmark = pytest.mark.gpu

G = 64
GUARD8, GUARD64 = 0xA5, 0xA5A5A5A5A5A5A5A5


def _dev(a, dev, view=None):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy((a.view(view) if view else a).copy()).to(torch.device("cuda", dev))


def _run(dev, cases, zones, zone_dicts, lead=0, nulls=False, shift=0):
    """one device call over `cases` -> the codes; checks the header and the guards.
    shift: the topic buffer's base pointer is that many bytes past an aligned address"""
    import torch
    n = len(cases)
    a = AC.arrays(cases, lead)
    d_keep, d_o = _dev(np.concatenate([np.full(shift, 0x2F, np.uint8), a["buf"]]), dev), _dev(a["off"], dev, np.int64)
    d_b = d_keep.data_ptr() + shift
    assert d_keep.data_ptr() % 8 == 0
    d_ml, d_pf = _dev(a["mount_len"] if n else np.zeros(1, np.uint32), dev, np.int32), \
        _dev(a["pub_flags"] if n else np.zeros(1, np.uint32), dev, np.int32)
    d_pa, d_acl = _dev(a["pub_admit"] if n else np.zeros(1, np.uint32), dev, np.int32), \
        _dev(a["acl"] if n else np.zeros(1, np.int8), dev)
    d_code = _dev(np.full(n + G, GUARD8, dtype=np.uint8), dev)
    d_hdr = _dev(np.full(8 + G, GUARD64, dtype=np.uint64), dev, np.int64)
    torch.cuda.synchronize()
    if nulls:
        Engine.admit_batch_device(d_b, d_o, n, None, d_pf, None, zones, None, d_code, d_hdr)
    else:
        Engine.admit_batch_device(d_b, d_o, n, d_ml, d_pf, d_pa, zones, d_acl, d_code, d_hdr)
    torch.cuda.synchronize()
    code, hdr = d_code.cpu().numpy(), d_hdr.cpu().numpy().view(np.uint64)
    assert (code[n:] == GUARD8).all() and len(code) == n + G
    assert (hdr[8:] == np.uint64(GUARD64)).all() and len(hdr) == 8 + G
    want = [AC.want(c, zone_dicts) for c in cases]
    bad = np.nonzero(code[:n] != np.array(want, dtype=np.uint8))[0]
    assert len(bad) == 0, (len(bad), int(bad[0]), {k: v if k != "topic" else v[:80] for k, v in cases[bad[0]].items()},
                           int(code[bad[0]]), want[bad[0]])
    assert [int(x) for x in hdr[:8]] == admit_ref.header(want)
    return code[:n]


def _dress(topics, salt=0, mounts=True):
    """byte-corpus topics as publishes: flags, zone, alias, super and ACL answer
    cycle with the index; mounts=False keeps every topic's byte offset"""
    acl = ("allow", "deny", "nomatch")
    out = []
    for i, t in enumerate(topics):
        k = i + salt
        out.append(AC.case(t, AC.MOUNTS[k % 3] if mounts and k % 5 == 0 else b"", k % 3, k % 7 == 3, (None, 1, 4, 5)[k // 3 % 4]
                           if k % 11 == 0 else None, k // 2 % len(AC.ZONES), k % 13 == 0, acl[k // 4 % 3]))
    return out


@pytest.fixture(scope="module")
def zones():
    return AC.zones_table()


def test_cpu_corpus(gpu_device, zones):
    cases = AC.product()
    code = _run(gpu_device, cases, zones, AC.ZONES)
    assert sorted(set(int(c) for c in code)) == [0, 1, 2, 3, 4, 5]
    host, _ = Engine.admit_batch(*[AC.arrays(cases)[k] for k in ("buf", "off", "pub_flags")], zones,
                                 *[AC.arrays(cases)[k] for k in ("mount_len", "pub_admit", "acl")])
    assert (host == code).all()


def test_byte_corpus(gpu_device, zones):
    """every topic admitted by the caps, so the code is the wildcard test's alone; then dressed as publishes"""
    ts = C.FIXED + C.topics()
    open_zone = [dict(admit_ref.DEFAULT_ZONE, enable_acl=False)]
    code = _run(gpu_device, [AC.case(t) for t in ts], AC.zones_table(open_zone), open_zone)
    assert 0 < int((code == 1).sum()) < len(ts)
    _run(gpu_device, _dress(ts), zones, AC.ZONES)
    for name, lead, wts in C.wave_batches():        # the waves on the window's limit, at the lead they are built for
        _run(gpu_device, _dress(wts, 1, mounts=False), zones, AC.ZONES, lead=lead)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_batch_sizes(gpu_device, zones, n):
    mixed = _dress((C.FIXED + C.stratified())[:2000], 2)
    prod = AC.product()[::13]
    cases = [x for pair in zip(mixed, prod) for x in pair][n:2 * n]
    assert len(cases) == n
    _run(gpu_device, cases, zones, AC.ZONES)


def test_buffer_offset_and_null_planes(gpu_device, zones):
    cases = _dress(C.FIXED + C.stratified(k=600), 3) + AC.product()[::29]
    for lead in (5, 3):
        _run(gpu_device, cases, zones, AC.ZONES, lead=lead)
    # a base pointer that is not 8-byte aligned: the words are aligned by address
    for shift, lead in ((3, 0), (5, 5), (1, 7)):
        _run(gpu_device, cases, zones, AC.ZONES, lead=lead, shift=shift)
    # NULL planes: no mountpoint, zone 0 / not super / no alias, every check nomatch
    plain = [AC.case(c["topic"], qos=c["qos"], retain=c["retain"]) for c in cases]
    _run(gpu_device, plain, zones, AC.ZONES, lead=5, nulls=True)


def test_unchecked_inputs_are_clamped(gpu_device, zones):
    """the device form does not validate its per-publish words: a zone index
    past the table reads the last zone, a mount_len past the topic leaves an
    empty topic; neither reads outside the table or the topic"""
    import torch
    last = len(AC.ZONES) - 1
    cases = [AC.case(b"a/b", qos=2, retain=True, zone=last, acl="allow"), AC.case(b"a/b", b"mnt/", acl="allow")]
    a = AC.arrays(cases)
    a["pub_admit"][0] = 0xFF
    a["mount_len"][1] = 1000
    dev = gpu_device
    d_code, d_hdr = _dev(np.full(2 + G, GUARD8, dtype=np.uint8), dev), _dev(np.zeros(8, np.uint64), dev, np.int64)
    Engine.admit_batch_device(_dev(a["buf"], dev), _dev(a["off"], dev, np.int64), 2, _dev(a["mount_len"], dev, np.int32),
                              _dev(a["pub_flags"], dev, np.int32), _dev(a["pub_admit"], dev, np.int32), zones,
                              _dev(a["acl"], dev), d_code, d_hdr)
    torch.cuda.synchronize()
    code = d_code.cpu().numpy()
    assert list(code[:2]) == [AC.want(cases[0]), 1] and (code[2:] == GUARD8).all()
    assert AC.want(cases[0]) == 4       # the last zone has no retain
