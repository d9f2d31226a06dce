"""The thinned byte corpus of tests/acl_corpus.py through both entries of
rewrite.hip, tm_rewrite_match_batch (host buffers) and
tm_rewrite_match_batch_device (device buffers, on a side stream), against
oracle/pytrie.py:rewrite_rule_index: rewrite.hip holds its own '/' scanner
and byte compare, which until now met ASCII words of 1-4 bytes only.  The
rules are 64 corpus filters and, behind them, filters whose first byte is
'+' / '#' without being a wildcard, '$SYS/#', the empty filter and the
catch-alls, so a later rule is the first match of most topics and '$' topics
outside $SYS match none (tests/test_acl_corpus.py pins that on the CPU)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import acl_corpus as A  # noqa: E402
import byte_corpus as C  # noqa: E402
from emqx_amd.emqx_mod_rewrite import NO_RULE, Rewrite  # noqa: E402
from emqx_amd.engine import pack  # noqa: E402
from oracle import pytrie  # noqa: E402

pytestmark = pytest.mark.gpu


class _Ref:
    def __init__(self, dev):
        self.topics = A.subset()
        self.filters = A.rewrite_rules()
        with A.deep():
            idx = [pytrie.rewrite_rule_index(t, self.filters) for t in self.topics]
        self.want = np.array([NO_RULE if k is None else k for k in idx], dtype=np.uint32)
        self.rw = Rewrite([(f, b"(.*)", b"r/$1") for f in self.filters], device=dev)


@pytest.fixture(scope="module")
def ref(gpu_device):
    r = _Ref(gpu_device)
    yield r
    r.rw.close()


def _agree(tag, topics, got, want):
    assert len(got) == len(topics), tag
    for i, t in enumerate(topics):
        if int(got[i]) != int(want[i]):
            raise AssertionError("%s: topic %d %s: got rule %d want %d"
                                 % (tag, i, repr(t) if len(t) <= 80 else "%r... (%d bytes)" % (t[:80], len(t)),
                                    got[i], want[i]))


def _device(rw, buf, off, dev):
    """tm_rewrite_match_batch_device on a side stream, offsets as given"""
    import torch
    d = torch.device("cuda", dev)
    n = len(off) - 1
    d_b = torch.from_numpy(np.ascontiguousarray(buf).copy()).to(d)
    d_o = torch.from_numpy(np.ascontiguousarray(off).view(np.int64).copy()).to(d)
    d_out = torch.full((max(n, 1),), -9, dtype=torch.int32, device=d)
    side = torch.cuda.Stream(device=d)
    rw.rule_index_device(d_b, d_o, n, d_out, stream=side)
    side.synchronize()
    return d_out.cpu().numpy().view(np.uint32)[:n]


def test_corpus_topics_vs_oracle(ref, gpu_device):
    assert NO_RULE in ref.want and len(set(ref.want.tolist())) > 20
    buf, off = pack(ref.topics)
    host = ref.rw.rule_index_batch(buf, off)
    _agree("host entry", ref.topics, host, ref.want)
    device = _device(ref.rw, buf, off, gpu_device)
    _agree("device entry", ref.topics, device, ref.want)
    assert np.array_equal(host, device)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_batch_sizes_around_the_block(ref, gpu_device, n):
    ts = ref.topics[-2 - n:-2]                                  # the topics before the two giants
    want = ref.want[-2 - n:-2]
    buf, off = pack(ts)
    _agree("%d topics (host entry)" % n, ts, ref.rw.rule_index_batch(buf, off), want)
    _agree("%d topics (device entry)" % n, ts, _device(ref.rw, buf, off, gpu_device), want)


@pytest.mark.parametrize("lead", [5, 8])
def test_first_offset_not_zero(ref, gpu_device, lead):
    """the host entry rebases topic_off, the device entry reads absolute offsets; '/' all around"""
    buf, off = C.envelope(ref.topics, lead)
    assert int(off[0]) == lead
    _agree("lead %d (host entry)" % lead, ref.topics, ref.rw.rule_index_batch(buf, off), ref.want)
    _agree("lead %d (device entry)" % lead, ref.topics, _device(ref.rw, buf, off, gpu_device), ref.want)


def test_no_rules(ref, gpu_device):
    rw = Rewrite([], device=gpu_device)
    try:
        ts = ref.topics[:257]
        buf, off = C.envelope(ts, 5)
        none = np.full(len(ts), NO_RULE, dtype=np.uint32)
        _agree("0 rules (host entry)", ts, rw.rule_index_batch(buf, off), none)
        _agree("0 rules (device entry)", ts, _device(rw, buf, off, gpu_device), none)
    finally:
        rw.close()
