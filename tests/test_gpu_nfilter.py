"""Per-node filters inside the node's own cache line (option "nfilter",
image.h) on the device: the trie of nfilter_trie.py -- filtered nodes reached
through a '+' edge at once and by a pop, through a table edge, by the '$'
rule's start, and the root -- matched through every walk: the per-lane queue
walk (both workspace slots), the small-batch kernel, the wave walk, the
copy-out's re-walk (lists longer than the stage row, spill off) and the keyed
walk of a two-shard set.  Every list equals emqx_trie:match/1's (O1) id for
id, with the option on and off, and again after children were added and
deleted without a relayout, on both image epochs."""
import numpy as np
import pytest

from emqx_amd import Engine
from nfilter_trie import churn_adds, churn_dels, churn_topics, filters, packed, topics
from oracle import O1
from test_gpu_small import _small

pytestmark = pytest.mark.gpu

PATHS = {
    "lane": {"wave_walk_max": 0, "slots": 2},
    "wave": {"wave_walk_max": 1 << 30},
    "rewalk": {"wave_walk_max": 0, "stage_k": 4, "stage_auto": 0, "spill": 0},
}


@pytest.fixture(scope="module")
def case():
    """filters, topics and O1's lists before and after the churn (computed once, never changed)"""
    fs, ts = filters(), topics()
    ts2 = ts + churn_topics()
    o1 = O1()
    o1.insert_many(*packed(fs))
    want = o1.match_ids(*packed(ts), threads=4)
    for f in churn_adds():
        o1.insert(f)
    for f in churn_dels():
        o1.delete(f)
    want2 = o1.match_ids(*packed(ts2), threads=4)
    o1.close()
    assert int(want[0].max()) > 4     # lists past the re-walk variant's stage row
    return fs, ts, want, ts2, want2


def same(got, want, ts):
    for g, w, name in zip(got, want, ("counts", "offsets", "ids")):
        if not np.array_equal(g, w):
            oc, oo, oi = want
            bad = [t for t in range(len(oc)) if got[0][t] != oc[t] or
                   not np.array_equal(got[2][got[1][t]:got[1][t + 1]], oi[oo[t]:oo[t + 1]])]
            raise AssertionError("%s differ: %d of %d topics, first %r" % (name, len(bad), len(oc), ts[bad[0]]))


def check_small(c, o, ids, total, oc, oo, oi):
    """the small path places its lists in completion order: counts, total, every list, and the lists
    tile [0, total) (empty lists, which the '$' rule makes, sort before the list at their offset)"""
    assert np.array_equal(c, oc)
    assert total == int(oc.sum())
    order = np.lexsort((c, o))
    ends = o[order] + c[order].astype(np.uint64)
    assert o[order][0] == 0 and np.all(o[order][1:] == ends[:-1]) and ends[-1] == total
    for t in range(len(oc)):
        assert np.array_equal(ids[o[t]:o[t] + c[t]], oi[oo[t]:oo[t] + oc[t]]), t


def churn(e):
    for f in churn_adds():
        e.insert(f)
    for f in churn_dels():
        e.delete(f)


@pytest.mark.parametrize("nfilter", [1, 0])
@pytest.mark.parametrize("path", list(PATHS))
def test_walks_equal_o1(gpu_device, case, path, nfilter):
    fs, ts, want, ts2, want2 = case
    e = Engine(device=gpu_device)
    e.set_option("nfilter", nfilter)
    for k, v in PATHS[path].items():
        e.set_option(k, v)
    e.insert_many(*packed(fs))
    tb, to = packed(ts)
    same(e.match_batch(tb, to), want, ts)
    same(e.match_batch(tb, to), want, ts)          # the other workspace slot
    # children added and deleted without a relayout: the delta goes to the other image epoch, the next one
    # back to the first
    churn(e)
    tb2, to2 = packed(ts2)
    same(e.match_batch(tb2, to2), want2, ts2)
    e.insert(b"p64/+/again")
    e.delete(b"p64/+/again")
    same(e.match_batch(tb2, to2), want2, ts2)
    e.close()


@pytest.mark.parametrize("nfilter", [1, 0])
def test_small_batch_equals_o1(gpu_device, case, nfilter):
    fs, ts, want, ts2, want2 = case
    e = Engine(device=gpu_device)
    e.set_option("nfilter", nfilter)
    e.insert_many(*packed(fs))
    e.commit()
    check_small(*_small(e, *packed(ts), dev=gpu_device), *want)
    churn(e)
    e.commit()
    check_small(*_small(e, *packed(ts2), dev=gpu_device), *want2)
    e.close()


@pytest.mark.parametrize("nfilter", [1, 0])
def test_keyed_walk_of_two_shards_equals_o1(gpu_device, case, nfilter):
    from emqx_amd import shard
    fs, ts, want, ts2, want2 = case
    S = 2
    engs = [shard.ShardEngine(gpu_device, S, s) for s in range(S)]
    for e in engs:
        e.set_option("nfilter", nfilter)
    ss = shard.ShardSet([gpu_device] * S, engines=engs)
    ss.insert_many(*packed(fs))
    counts, offs, gids = ss.match_batch(*packed(ts))
    oc, oo, oi = want
    assert np.array_equal(counts, oc)
    got = [ss.filter_bytes(int(g)) for g in gids[:int(offs[-1])]]
    assert got == [fs[int(i)] for i in oi]
    ss.close()
