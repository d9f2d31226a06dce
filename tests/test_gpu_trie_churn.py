"""The commit path on the device under the churn of trie_churn.py: the delta
scatter of this commit's and the previous commit's dirty logs into the image
epoch no batch reads, which production churn takes and one whole-table upload
never does.

After every commit tm_debug_check_device reads the live image back and
compares every table byte for byte with the host's; after every round the
round's topics (instances and near misses of every filter the last two rounds
touched, beside about 1,000 fixed ones) are matched and compared, as ordered
lists of filter bytes, with emqx_trie:match/1's (O1 kept in step) -- through
the per-lane queue walk, the wave walk and the small-batch kernel in rotation.
tm_debug_commit_stats proves the scatter is what ran: every small round that
does not follow a whole-table copy scatters the node table and every other
trie table it changed (two logs with two image epochs, one with
double_buffer 0), every large round copies one whole (test_trie_churn.py
pins the same on the CPU).

Variants: the defaults, double_buffer 0, hot_edges 3 (the second edge table
under deltas), split 0, summaries 0, nfilter 0, and one run that switches
double_buffer 1 -> 0 -> 1 (the `stale` branch of the upload) and split 0 -> 1
with no delta pending (commit() derives the halves of the live image); and
two replicas on the one GPU, both read back."""
import numpy as np
import pytest

from emqx_amd import Engine
from oracle import O1
from test_gpu_small import _small
from trie_churn import TRIE_TABLES, check_decisions, hot_options, packed, schedule

pytestmark = pytest.mark.gpu

WALKS = ({"wave_walk_max": 0}, {"wave_walk_max": 1 << 30}, None)     # lane, wave, small-batch kernel


@pytest.fixture(scope="module")
def run():
    """the base filters, the rounds with their topics packed, and O1's lists (filter bytes, reference
    order) and node count after each round (computed once, never changed)"""
    base, rounds = schedule()
    o1 = O1()
    o1.insert_many(*packed(base))
    want = []
    for _, _, ops, topics in rounds:
        for op, f in ops:
            getattr(o1, op)(f)
        want.append(([o1.match(t) for t in topics], o1.node_count))
    o1.close()
    return base, [(r, kind, ops, packed(topics)) for r, kind, ops, topics in rounds], want


def lists(eng, counts, offs, ids):
    """per topic the filter bytes of ids[offs[t] : offs[t] + counts[t]]"""
    uniq, inv = np.unique(ids, return_inverse=True)
    names = eng.filters_bytes(uniq)
    return [[names[k] for k in inv[int(offs[t]):int(offs[t]) + int(counts[t])]] for t in range(len(counts))]


def match(eng, r, tb, to, dev):
    walk = WALKS[r % len(WALKS)]
    if walk is None:
        c, o, ids, total = _small(eng, tb, to, dev=dev)
        assert total == int(c.sum()) and total <= len(ids)
        return lists(eng, c, o, ids[:total])
    for k, v in walk.items():
        eng.set_option(k, v)
    c, o, ids = eng.match_batch(tb, to)
    return lists(eng, c, o, ids)


def same(got, want, r, what):
    if got != want:
        bad = [t for t in range(len(want)) if got[t] != want[t]]
        raise AssertionError("round %d (%s): %d of %d lists differ, first topic #%d: %r, oracle %r" %
                             (r, what, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]]))


def churn(eng, run, dev, hot_on=False, switches=None, exempt=(), rounds=None, matches=True):
    base, sched, want = run
    switches = switches or {}
    eng.insert_many(*packed(base))
    eng.commit()
    eng.debug_check_device()
    prev = eng.debug_commit_stats()
    seen = {}     # table -> the decisions of the small rounds that do not follow a whole copy of it
    for r, kind, ops, (tb, to) in sched[:rounds]:
        for k, v in switches.get(("before", r), ()):
            eng.set_option(k, v)
        for op, f in ops:
            getattr(eng, op)(f)
        if kind == "relayout":
            eng.set_option("relayout", 1)
        eng.commit()
        eng.debug_check_device()
        stats = eng.debug_commit_stats()
        check_decisions(r, kind, stats, prev, hot_on, exempt=r in exempt)
        if kind == "small" and r not in exempt:
            for t in TRIE_TABLES:
                if prev[t][0] != 3:
                    seen.setdefault(t, set()).add(stats[t][0])
        prev = stats
        assert eng.node_count == want[r][1]
        if matches:
            same(match(eng, r, tb, to, dev), want[r][0], r, "walk %d" % (r % len(WALKS)))
        for k, v in switches.get(("after", r), ()):     # with no delta pending
            eng.set_option(k, v)
            eng.commit()
            eng.debug_check_device()
            same(match(eng, r, tb, to, dev), want[r][0], r, "after %s = %d" % (k, v))
    return seen


VARIANTS = {
    "defaults": (),
    "double_buffer0": (("double_buffer", 0),),
    "hot_edges3": hot_options(3),
    "split0": (("split", 0),),
    "summaries0": (("summaries", 0),),
    "nfilter0": (("nfilter", 0),),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_device_image_and_lists_under_churn(gpu_device, run, variant):
    eng = Engine(device=gpu_device)
    for k, v in VARIANTS[variant]:
        eng.set_option(k, v)
    seen = churn(eng, run, gpu_device, hot_on=variant == "hot_edges3")
    how = 1 if variant == "double_buffer0" else 2       # the scatter of one log / of both epochs' logs
    assert seen["nodes"] == {how} and seen["edges"] == {how} and how in seen["dict"]
    if variant == "hot_edges3":
        assert seen["hot_edges"] == {how}               # the second table is in use and scattered
    eng.close()


def test_switching_epochs_and_split_mid_churn(gpu_device, run):
    """double_buffer 1 -> 0 -> 1: the commit after the second switch finds the other image several
    commits behind (`stale`: a whole copy, so that round is exempt from the scatter cap); split 0, then
    1 with no delta pending: commit() derives the halves of the live image in place"""
    eng = Engine(device=gpu_device)
    seen = churn(eng, run, gpu_device, exempt={12}, switches={
        ("before", 5): [("double_buffer", 0)],
        ("before", 8): [("split", 0)],
        ("before", 12): [("double_buffer", 1)],
        ("after", 15): [("split", 1)],
    })
    assert seen["nodes"] == {1, 2} and seen["edges"] == {1, 2}
    eng.close()


def test_two_replicas_read_back(gpu_device, run):
    eng = Engine(devices=[gpu_device, gpu_device])
    assert eng.replicas == 2
    churn(eng, run, gpu_device, rounds=10, matches=False)
    _, sched, want = run
    r, _, _, (tb, to) = sched[9]
    c, o, ids = eng.match_batch(tb, to)     # cut across both replicas
    same(lists(eng, c, o, ids), want[9][0], r, "two replicas")
    eng.close()
