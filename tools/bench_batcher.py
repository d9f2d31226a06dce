"""Micro-batcher sweep (the NIF's publish path): P producer
threads submit single topics of a C3 batch to tm_batcher_submit, one
completion callback per topic (tools/ubench/batchdrive.cpp), after a warm-up
run; one JSON line per (lanes, max_topics, deadline, producers) point.

Run: python tools/bench_batcher.py [--topics 8000000]

--publish: the TM_BATCHER_DELIVERIES and TM_BATCHER_PUBLISH batchers side by
side on the workload of tools/bench_shared.py (C2: one local route per filter,
a group route with a member set of 1 .. 7 on a tenth of them, '#' with two
groups of 64) plus a plain subscriber on every fourth filter: a flood from 16
threads on 4 lanes, and an open loop at --rate publishes/s with deadline 200
us and eager sealing (tools/ubench/pubdrive.cpp).  The publish leg beside the
deliveries leg is the cost of dispatch, picks and pack on top of deliveries.
Per batch: device_us split into launch_us and sync_us, and packed_bytes, the
header, offsets and records a publish batch brings back (a batch of up to
32768 topics reads up to its capacities instead, about 1.25 x + 24 KiB).
--legs deliveries runs on a commit without the publish mode (the baseline).
One further leg rides the publish leg's workload: publish_rr, round robin
with one cursor context per lane (TM_BATCHER_ROUND_ROBIN); both run the
stream-ordered publish call, and every leg reports its reruns.

Run: python tools/bench_batcher.py --publish [--topics 1000000 --rate 1e6 --rounds 3 --out FILE]"""
import argparse
import ctypes
import itertools
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from emqx_amd import Engine  # noqa: E402
from emqx_amd import workload as W  # noqa: E402


NODE = b"emqx@node00"
LEGS = {"deliveries": 0, "publish": 1, "publish_rr": 2}   # tools/ubench/pubdrive.cpp
GROUPS = [b"grp%d" % i for i in range(8)]
HOT = [b"hot0", b"hot1"]


def publish_world(a):
    """the engine of tools/bench_shared.py, with subscriber bags"""
    import numpy as np
    from emqx_amd.engine import pack
    nf = a.filters or W.CONFIGS[a.config]["filters"]
    rng = np.random.default_rng(23)
    fb, fo = W.filters(a.config, n=nf)
    filters = W.unpack(fb, fo)
    gdest = lambda g: b"\x01" + g + b"\x00" + NODE  # noqa: E731
    e = Engine(device=0, filters_hint=nf + 1)
    db = np.concatenate([np.tile(np.frombuffer(NODE, dtype=np.uint8), nf), np.zeros(8, dtype=np.uint8)])
    do = np.arange(nf + 1, dtype=np.uint64) * np.uint64(len(NODE))
    e.route_add_many(fb, fo, db, do)
    e.dest_target(NODE, Engine.TARGET_NODE, NODE)
    e.set_local_node(NODE)
    for g in GROUPS + HOT:
        e.dest_target(gdest(g), Engine.TARGET_GROUP, g)
    shared = np.nonzero(rng.random(nf) < 0.1)[0]
    grp = rng.integers(0, len(GROUPS), size=len(shared))
    sizes = rng.integers(1, 8, size=len(shared))
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    sb, so = pack([filters[i] for i in shared])
    gb, go = pack([gdest(GROUPS[g]) for g in grp])
    e.route_add_many(sb, so, gb, go)
    for k in range(int(sizes.max())):
        idx = np.nonzero(sizes > k)[0]
        mb, mo = pack([filters[shared[i]] for i in idx])
        kb, ko = pack([GROUPS[grp[i]] for i in idx])
        e.share_add_many(kb, ko, mb, mo, (start[idx] + k).astype(np.uint32))
    hot_base = int(start[-1])
    for j, g in enumerate(HOT):
        e.route_add(b"#", gdest(g))
        kb, ko = pack([g] * 64)
        mb, mo = pack([b"#"] * 64)
        e.share_add_many(kb, ko, mb, mo, (hot_base + 64 * j + np.arange(64)).astype(np.uint32))
    ub, uo = pack(filters[::4])                               # a plain subscriber on every fourth filter
    e.sub_add_many(ub, uo, np.arange(len(uo) - 1, dtype=np.uint32))
    e.commit()
    return e, nf


def publish_main(a):
    t0 = time.time()
    e, nf = publish_world(a)
    print("[batcher] publish world of %d filters built in %.1fs" % (nf, time.time() - t0), file=sys.stderr)
    tb, to = W.topics(a.config, n=a.topics)
    n = len(to) - 1
    drv = ctypes.CDLL(os.path.join(ROOT, "tools", "ubench", "libpubdrive.so"))
    drv.tm_bench_publish.restype = ctypes.c_int
    drv.tm_bench_publish.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                                     ctypes.c_double, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                     ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
    lines = []
    for rnd in range(a.rounds):
        for leg in a.legs.split(","):
            for run in a.runs.split(","):
                res = (ctypes.c_double * 16)()
                flood = run == "flood"
                rc = drv.tm_bench_publish(e.h, tb.ctypes.data, to.ctypes.data, n, 16, 0.0 if flood else a.rate,
                                          0 if flood else int(a.rate * a.secs), 200,
                                          int(a.max_topics.split(",")[0]), 4, LEGS[leg],
                                          0 if flood else 1, res)
                mean_batch, results = res[3], res[13]
                line = {"leg": leg, "run": run, "round": rnd, "rc": rc, "filters": nf, "topics": n,
                        "producers": 16, "lanes": 4, "deadline_us": 200, "eager": int(not flood),
                        "offered_per_s": None if flood else a.rate, "secs": res[0], "topics_per_s": res[1],
                        "batches": int(res[2]), "mean_batch": mean_batch, "lat_us_p50": res[4], "lat_us_p99": res[5],
                        "failed": int(res[6]), "deliveries_per_topic": res[7], "pairs_per_topic": res[8],
                        "per_batch": {"device_us": res[9], "launch_us": res[10], "sync_us": res[11],
                                      "callbacks_us": res[12], "results": results},
                        "reruns": int(res[14])}
                if leg != "deliveries":    # header + both offset arrays + 16 B records + 8 B pairs
                    line["per_batch"]["packed_bytes"] = 64 + 16 * (mean_batch + 1) + 16 * results + \
                        8 * res[8] * mean_batch
                else:                   # total + counts + offsets + To ids + target ids
                    line["per_batch"]["result_bytes"] = 8 + 4 * mean_batch + 8 * (mean_batch + 1) + 8 * results
                lines.append(line)
                print(json.dumps(line), flush=True)
    e.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--publish", action="store_true", help="deliveries and publish batchers on the C2 publish world")
    ap.add_argument("--legs", default="deliveries,publish,publish_rr")
    ap.add_argument("--runs", default="flood,paced")
    ap.add_argument("--rate", type=float, default=1e6)
    ap.add_argument("--secs", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--filters", type=int, default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--topics", type=int, default=8_000_000)
    ap.add_argument("--lanes", default="2,4")
    ap.add_argument("--max-topics", default="65536,262144")
    ap.add_argument("--deadline-us", default="200")
    ap.add_argument("--producers", default="16")
    ap.add_argument("--cb-threads", default="0")
    ap.add_argument("--eager", default="0", help="comma list of 0/1: TM_BATCHER_EAGER")
    ap.add_argument("--replicas", default="0", help="HIP ordinals of the engine's replicas (repeats: one GPU shared)")
    a = ap.parse_args()
    if a.publish:
        if "--config" not in sys.argv:
            a.config = 2
        if "--topics" not in sys.argv:
            a.topics = 1_000_000
        return publish_main(a)
    fb, fo = W.filters(a.config)
    devs = [int(x) for x in a.replicas.split(",")]
    e = Engine(device=devs[0]) if len(devs) == 1 else Engine(devices=devs)
    t0 = time.time()
    e.insert_many(fb, fo)
    e.commit()
    print("[batcher] trie built in %.1fs" % (time.time() - t0), file=sys.stderr)
    tb, to = W.topics(a.config, n=a.topics)
    drv = ctypes.CDLL(os.path.join(ROOT, "tools", "ubench", "libbatchdrive.so"))
    drv.tm_bench_batcher.restype = ctypes.c_int
    drv.tm_bench_batcher.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                     ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                     ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_double)]
    ints = lambda s: [int(x) for x in s.split(",")]  # noqa: E731
    for lanes, mt, dl, prod, cbt, eager in itertools.product(ints(a.lanes), ints(a.max_topics), ints(a.deadline_us),
                                                             ints(a.producers), ints(a.cb_threads), ints(a.eager)):
        print("[batcher] lanes %d, max_topics %d, deadline %d us, producers %d, callback threads %d ..." % (
            lanes, mt, dl, prod, cbt), file=sys.stderr, flush=True)
        res = (ctypes.c_double * 14)()
        rc = drv.tm_bench_batcher(e.h, tb.ctypes.data, to.ctypes.data, len(to) - 1, prod, dl, mt, lanes,
                                  4 if eager else 0, cbt, res)
        print(json.dumps({"replicas": devs, "eager": eager, "lanes": lanes, "max_topics": mt, "deadline_us": dl,
                          "producers": prod,
                          "callback_threads": cbt, "rc": rc,
                          "topics": len(to) - 1, "secs": res[0], "topics_per_s": res[1], "batches": int(res[2]),
                          "mean_batch": res[3], "lat_us_p50": res[4], "lat_us_p99": res[5], "failed": int(res[6]),
                          "matches": int(res[7]),
                          "per_batch_us": {"sealed_to_lane": res[8], "pack": res[9], "device": res[10],
                                           "callbacks": res[11], "device_launch": res[12],
                                           "device_wait": res[13]}}), flush=True)
    e.close()


if __name__ == "__main__":
    main()
