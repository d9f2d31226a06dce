"""bench.py's own machinery: the filter set generated as growing prefixes and
inserted as they arrive builds the trie of one insert of all of it, and
--dump-outputs writes the lists of the last timed step."""
import os

import numpy as np
import pytest

from emqx_amd import Engine
from emqx_amd import workload as W


@pytest.mark.parametrize("cfg,n", [(1, 7), (3, 20_003), (5, 10_000)])
def test_filter_prefixes_are_stable(cfg, n):
    """the first k filters do not depend on how many are asked for"""
    fb, fo = W.filters(cfg, n=n)
    for k in (1, n // 8, n // 2, n - 1):
        pb, po = W.filters(cfg, n=max(1, k))
        assert np.array_equal(po, fo[:len(po)])
        assert np.array_equal(pb[:int(po[-1])], fb[:int(po[-1])])


@pytest.mark.parametrize("n,chunk", [(7, 10), (20_003, 3_000)])
def test_generate_and_insert_equals_one_insert(n, chunk):
    import bench
    fb, fo = W.filters(3, n=n)
    one = Engine(device=-1, filters_hint=n)
    one.insert_many(fb, fo)
    staged = Engine(device=-1, filters_hint=n)
    gb, go = bench.generate_and_insert(staged, 3, n, 0, chunk=chunk)
    assert np.array_equal(gb, fb) and np.array_equal(go, fo)
    assert staged.filter_count == one.filter_count == n
    assert staged.node_count == one.node_count
    for fid in range(n):
        assert staged.filter_bytes(fid) == one.filter_bytes(fid)
    one.close()
    staged.close()


def load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.gpu
def test_dump_is_the_last_steps_lists(gpu_device, tmp_path, monkeypatch):
    import torch

    import bench
    from oracle import O1
    n_filters, n_topics = 10_000, 3_001
    dev = torch.device("cuda", gpu_device)
    eng = Engine(device=gpu_device, filters_hint=n_filters)
    fb, fo = bench.generate_and_insert(eng, 1, n_filters, 0)
    eng.commit()
    eng.set_option("slots", 3)   # a workspace slot per lane, as bench.py sets it
    batches = [W.topics(1, n=n_topics + b, stream=b) for b in range(2)]
    reg = bench.Region(eng, dev, batches, [bench.Region.make_stream(dev, "prio") for _ in range(3)])
    reg.warm(1)
    reg.timed(3)          # steps 0..3: the last one walks batch 1 on lane 0
    reg.dump_last_step(str(tmp_path / "all"), 0)
    o1 = O1(n_filters)
    o1.insert_many(fb, fo)
    oc, oo, oi = o1.match_ids(*batches[1], threads=2)
    o1.close()
    got = load(str(tmp_path / "all"))
    assert sorted(got) == ["counts", "ids", "offsets", "total"]
    assert all(x.dtype == np.float64 for x in got.values())
    assert got["total"][0] == len(oi) > 0
    assert np.array_equal(got["counts"], oc) and np.array_equal(got["offsets"], oo) and np.array_equal(got["ids"], oi)

    # past the limits: a sample of the same lists, the same one every time
    monkeypatch.setattr(bench, "DUMP_TOPICS", 500)
    monkeypatch.setattr(bench, "DUMP_IDS", 2_000)
    reg.dump_last_step(str(tmp_path / "s1"), 0)
    reg.dump_last_step(str(tmp_path / "s2"), 0)
    s1, s2 = load(str(tmp_path / "s1")), load(str(tmp_path / "s2"))
    assert len(s1["counts"]) == len(s1["offsets"]) == 500 and len(s1["ids"]) == min(2_000, len(oi))
    for name in s1:
        assert np.array_equal(s1[name], s2[name])
    assert np.all(np.diff(s1["offsets"]) >= 0) and np.all(np.isin(s1["offsets"], oo))
    assert np.all(np.isin(s1["ids"], oi)) and s1["total"][0] == len(oi)
    reg.free()
    eng.close()
