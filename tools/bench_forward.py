"""The forward plan (forward.hip) next to the dispatch call it follows, on one
MI355X in one process.

Setup: the C2 filters (1M), one route each, the routes spread evenly over the
local node and R remote nodes (R = 4 and R = 64: a 5-node and a 65-node
cluster), no subscribers.  Timed on the same 1M-topic HBM-resident batch,
interleaved, HIP events around each call, 3 warm-ups then the median of 10:
    dispatch        tm_match_dispatch_batch_device
    dispatch_plan   the same followed by tm_forward_plan_device
    plan            tm_forward_plan_device alone over the planes left
Next to it the regrouping the plan replaces, done on the host: the four planes
read back, the forward slots picked out and ordered with numpy lexsort (read-back
and sort timed apart, wall clock, median of 3).

Before anything is timed, the plan of the first 20K topics of the batch is
checked against tests/forward_ref.py (route/2's {To, Node} clause over oracle
aggre/1 of O1's ordered match lists).

Run: python tools/bench_forward.py [--topics N --check K]
Writes profiles/forward/bench_forward.json and prints it."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from emqx_amd import Engine  # noqa: E402
from emqx_amd import workload as W  # noqa: E402

ROUTE_TOPIC = 0xFFFFFFFF


def log(*a):
    print("[forward]", *a, file=sys.stderr, flush=True)


def node_name(i):
    return b"emqx@node%02d" % i


def build_engine(fb, fo, nf, remotes):
    """filter i routes to node i % (remotes + 1); node 0 is node()"""
    e = Engine(device=0, filters_hint=nf)
    names = [node_name(i) for i in range(remotes + 1)]
    owner = np.arange(nf) % (remotes + 1)
    db = np.concatenate([np.frombuffer(b"".join(names[i] for i in owner), dtype=np.uint8), np.zeros(8, dtype=np.uint8)])
    do = np.arange(nf + 1, dtype=np.uint64) * np.uint64(len(names[0]))
    e.route_add_many(fb, fo, db, do)
    ids = [e.dest_target(nm, Engine.TARGET_NODE, nm) for nm in names]
    e.set_local_node(names[0])
    e.commit()
    return e, owner, ids


class Batch:
    """the device buffers of the calls on the batch"""

    def __init__(self, e, tb, to, dev, st):
        self.e, self.dev, self.st = e, dev, st
        self.n = n = len(to) - 1
        self.nbytes = int(to[-1])
        self.d_b = torch.from_numpy(tb).to(dev)
        self.d_o = torch.from_numpy(to.view(np.int64)).to(dev)
        i32 = dict(dtype=torch.int32, device=dev)
        i64 = dict(dtype=torch.int64, device=dev)
        self.c, self.o, self.tot = torch.empty(n, **i32), torch.empty(n + 1, **i64), torch.zeros(1, **i64)
        self.sc, self.so, self.stot = torch.empty(n, **i32), torch.empty(n + 1, **i64), torch.zeros(1, **i64)
        e.match_deliveries_batch_device(self.d_b, self.d_o, n, self.nbytes, self.c, self.o, None, None, 0, self.tot,
                                        stream=st)
        torch.cuda.synchronize(dev)
        self.slots = int(self.tot.item())
        self.cap = self.slots + 1024
        self.to, self.tg, self.nd = (torch.empty(self.cap, **i32) for _ in range(3))
        self.sto, self.sid = torch.empty(1024, **i32), torch.empty(1024, **i32)
        self.hdr = torch.zeros(4, **i64)
        self.dispatch()
        self.groups, self.pub = torch.empty(4, **i32), torch.empty(1, **i32)
        self.plan(self.n, 0, 0)                      # sizes only
        torch.cuda.synchronize(dev)
        self.M, self.G, self.T = (int(x) for x in self.hdr[:3].cpu())
        self.groups, self.pub = torch.empty((self.G + 1) * 4, **i32), torch.empty(self.M + 1, **i32)

    def dispatch(self):
        self.e.match_dispatch_batch_device(self.d_b, self.d_o, self.n, self.nbytes, self.c, self.o, self.to, self.tg,
                                           self.nd, self.cap, self.tot, self.sc, self.so, self.sto, self.sid, 1024,
                                           self.stot, stream=self.st)

    def plan(self, n=None, gcap=None, pcap=None):
        self.e.forward_plan_device(self.n if n is None else n, self.c, self.o, self.to, self.tg, self.cap, self.tot,
                                   self.hdr, self.groups, self.G if gcap is None else gcap, self.pub,
                                   self.M if pcap is None else pcap, stream=self.st)

    def both(self):
        self.dispatch()
        self.plan()

    def time(self, warmups=3, runs=10):
        """median ms of each call, interleaved, HIP events on the stream"""
        fns = {"dispatch": self.dispatch, "dispatch_plan": self.both, "plan": self.plan}
        ms = {k: [] for k in fns}
        for it in range(warmups + runs):
            for name, fn in fns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(self.dev)
                a.record(self.st)
                fn()
                b.record(self.st)
                torch.cuda.synchronize(self.dev)
                if it >= warmups:
                    ms[name].append(a.elapsed_time(b))
        return {k: float(np.median(v)) for k, v in ms.items()}, {k: [min(v), max(v)] for k, v in ms.items()}

    def host_regroup(self, fwd, runs=3):
        """the same regrouping on the host from the read-back planes; fwd: target id -> forwardable"""
        rb, srt, res = [], [], None
        for _ in range(runs):
            torch.cuda.synchronize(self.dev)
            t0 = time.perf_counter()
            cnt = self.c.cpu().numpy()
            off = self.o.cpu().numpy()
            to = self.to[: self.slots].cpu().numpy().view(np.uint32)
            tg = self.tg[: self.slots].cpu().numpy().view(np.uint32)
            t1 = time.perf_counter()
            span = np.diff(off)
            pubidx = np.repeat(np.arange(self.n, dtype=np.uint32), span)
            live = (np.arange(self.slots, dtype=np.int64) - np.repeat(off[:-1], span)) < np.repeat(cnt, span)
            keep = np.nonzero(live & fwd[np.minimum(tg, len(fwd) - 1)] & (tg < len(fwd)))[0]
            order = keep[np.lexsort((pubidx[keep], to[keep], tg[keep]))]
            tgs, tos = tg[order], to[order]
            head = np.ones(len(order), dtype=bool)
            head[1:] = (tgs[1:] != tgs[:-1]) | (tos[1:] != tos[:-1])
            first = np.nonzero(head)[0]
            res = (len(order), len(first), pubidx[order], tgs[first], tos[first], first)
            t2 = time.perf_counter()
            rb.append((t1 - t0) * 1e3)
            srt.append((t2 - t1) * 1e3)
        return float(np.median(rb)), float(np.median(srt)), res


def parity(bt, fb, fo, nf, tb, to, owner, ids, k):
    """the plan of the batch's first k topics against forward_ref over oracle aggre/1 of O1's lists"""
    from forward_ref import expected_plan
    from oracle import O1
    from oracle.pytrie import aggre
    o1 = O1(nf)
    o1.insert_many(fb, fo)
    oc, oo, oi = o1.match_ids(tb, to[: k + 1], threads=16)
    filters = W.unpack(fb, fo)
    triples = []
    for t in range(k):
        fl = [int(f) for f in oi[int(oo[t]):int(oo[t + 1])]]
        fid = {filters[f]: f for f in fl}
        for name, x in aggre([(filters[f], node_name(int(owner[f])).decode()) for f in fl]):
            if x[0] == 0 and x[1] != node_name(0):
                triples.append((ids[int(x[1][-2:])], fid[name], t))
    hdr, groups, pub = expected_plan(triples)
    bt.plan(k)
    torch.cuda.synchronize(bt.dev)
    got_hdr = [int(x) for x in bt.hdr.cpu()]
    if got_hdr != hdr:
        return False, "header %s, model %s" % (got_hdr, hdr)
    g = bt.groups[: hdr[1] * 4].cpu().numpy().view(np.uint32).reshape(-1, 4)
    if [tuple(r) for r in g.tolist()] != groups:
        return False, "groups"
    if bt.pub[: hdr[0]].cpu().numpy().view(np.uint32).tolist() != pub:
        return False, "pub"
    return True, "%d topics, M %d, G %d, %d targets" % (k, hdr[0], hdr[1], hdr[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--filters", type=int, default=None)
    ap.add_argument("--topics", type=int, default=1_000_000)
    ap.add_argument("--remotes", type=int, nargs="+", default=[4, 64])
    ap.add_argument("--check", type=int, default=20_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forward", "bench_forward.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)   # a stream of the caller's, so that its events bracket the calls
    nf = a.filters or W.CONFIGS[a.config]["filters"]
    fb, fo = W.filters(a.config, n=nf)
    tb, to = W.topics(a.config, n=a.topics)
    runs = {}
    for remotes in a.remotes:
        t0 = time.time()
        e, owner, ids = build_engine(fb, fo, nf, remotes)
        log("%d remote nodes: %d filters, built in %.1fs" % (remotes, nf, time.time() - t0))
        bt = Batch(e, tb, to, dev, st)
        check = None
        if a.check:
            ok, what = parity(bt, fb, fo, nf, tb, to, owner, ids, min(a.check, bt.n))
            log("parity vs forward_ref:", ok, what)
            check = {"ok": ok, "what": what}
            if not ok:
                raise SystemExit("parity failed: " + what)
        ms, spread = bt.time()
        bt.both()
        torch.cuda.synchronize(dev)
        fwd = np.zeros(max(ids) + 1, dtype=bool)
        fwd[ids[1:]] = True
        rb_ms, sort_ms, host = bt.host_regroup(fwd)
        g = bt.groups[: bt.G * 4].cpu().numpy().view(np.uint32).reshape(-1, 4)
        same = (host[0] == bt.M and host[1] == bt.G and
                np.array_equal(host[2], bt.pub[: bt.M].cpu().numpy().view(np.uint32)) and
                np.array_equal(host[3], g[:, 0]) and np.array_equal(host[4], g[:, 1]) and
                np.array_equal(host[5], g[:, 2]))
        log("host regroup equals the plan:", same)
        if not same:
            raise SystemExit("the host regrouping and the plan differ")
        runs["remotes_%d" % remotes] = {
            "delivery_slots": bt.slots, "M": bt.M, "G": bt.G, "targets": bt.T,
            "ms_median": ms, "ms_min_max": spread, "plan_cost_ms": ms["dispatch_plan"] - ms["dispatch"],
            "ns_per_forward": ms["plan"] * 1e6 / bt.M if bt.M else None,
            "host_baseline_ms": {"read_back": rb_ms, "regroup_lexsort": sort_ms, "total": rb_ms + sort_ms},
            "host_over_plan": (rb_ms + sort_ms) / ms["plan"] if ms["plan"] > 0 else None,
            "host_equals_plan": bool(same), "check": check}
        e.close()
        del bt
    out = {"workload": "C%d: %d filters, one route each over node() and R remote nodes; %d-topic batch" % (
               a.config, nf, a.topics),
           "method": "HIP events around each call, 3 warm-ups, median of 10, the three calls interleaved; "
                     "host baseline wall clock, median of 3",
           "runs": runs}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
