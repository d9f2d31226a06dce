"""The local dispatch (dispatch.hip) next to the deliveries step it extends, on
one MI355X in one process.

Setup: the C2 filters (1M), one local-node route each; subscribers drawn so
that the mean bag holds 4 (the EVEN layout).  A second engine holds the same
filters and routes with the same total of subscribers on 16 filters only (the
SKEW layout: 250,000 per bag), the 16 chosen so that the batch's pair total
comes as close to the even layout's as their hit counts allow.

Timed on the same 1M-topic HBM-resident batch, interleaved, HIP events around
each call, 3 warm-ups then the median of 10:
    deliveries   tm_match_deliveries_batch_device  (walk + routes + aggre)
    count_only   tm_match_dispatch_batch_device with sub_cap 0 (the count pass, the scan
                 and the per-topic offsets, no emit)
    dispatch     tm_match_dispatch_batch_device
dispatch - deliveries is the dispatch cost, dispatch - count_only the emit
pass; its bytes (per pair 4 B read and 8 B written, per delivery slot 16 B of
prefix and segment reads) over that time stand next to the device copy ceiling
of profiles/r06_k/copy_ceiling.json.

Before anything is timed, 20K topics of the batch are checked against
tests/dispatch_ref.py (route/2 + dispatch/2 over oracle aggre/1 of O1's
ordered match lists).

Run: python tools/bench_dispatch.py [--topics N --check K]
Writes profiles/dispatch/bench_dispatch.json and prints it."""
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
from emqx_amd.engine import pack  # noqa: E402

NODE = b"emqx@node00"


def log(*a):
    print("[dispatch]", *a, file=sys.stderr, flush=True)


def build_engine(fb, fo, nf):
    e = Engine(device=0, filters_hint=nf)
    db = np.concatenate([np.tile(np.frombuffer(NODE, dtype=np.uint8), nf), np.zeros(8, dtype=np.uint8)])
    do = np.arange(nf + 1, dtype=np.uint64) * np.uint64(len(NODE))
    e.route_add_many(fb, fo, db, do)
    e.dest_target(NODE, Engine.TARGET_NODE, NODE)
    e.set_local_node(NODE)
    return e


class Batch:
    """the device buffers of one engine's calls on the batch"""

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
        self.cap = int(self.tot.item()) + 1024
        self.to, self.tg, self.nd = (torch.empty(self.cap, **i32) for _ in range(3))
        self.dispatch(0)
        torch.cuda.synchronize(dev)
        self.pairs = int(self.stot.item())
        self.scap = self.pairs + 1024
        self.sto, self.sid = torch.empty(self.scap, **i32), torch.empty(self.scap, **i32)

    def deliveries(self):
        self.e.match_deliveries_batch_device(self.d_b, self.d_o, self.n, self.nbytes, self.c, self.o, self.to, self.tg,
                                             self.cap, self.tot, stream=self.st)

    def dispatch(self, scap=None):
        scap = self.scap if scap is None else scap
        self.e.match_dispatch_batch_device(self.d_b, self.d_o, self.n, self.nbytes, self.c, self.o, self.to, self.tg,
                                           self.nd, self.cap, self.tot, self.sc, self.so,
                                           self.sto if scap else None, self.sid if scap else None, scap, self.stot,
                                           stream=self.st)

    def time(self, warmups=3, runs=10):
        """median ms of each call, interleaved, HIP events on the stream"""
        fns = {"deliveries": self.deliveries, "count_only": lambda: self.dispatch(0), "dispatch": self.dispatch}
        ms = {k: [] for k in fns}
        host = {k: [] for k in fns}
        for it in range(warmups + runs):
            for name, fn in fns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(self.dev)
                t0 = time.perf_counter()
                a.record(self.st)
                fn()
                b.record(self.st)
                torch.cuda.synchronize(self.dev)
                t1 = time.perf_counter()
                if it >= warmups:
                    ms[name].append(a.elapsed_time(b))
                    host[name].append((t1 - t0) * 1e3)
        return ({k: float(np.median(v)) for k, v in ms.items()}, {k: [min(v), max(v)] for k, v in ms.items()},
                {k: float(np.median(v)) for k, v in host.items()})


def parity(e, bt, fb, fo, nf, tb, to, bag_of, k):
    """k topics of the batch against dispatch_ref over oracle aggre/1 of O1's lists"""
    from dispatch_ref import SubscriberBag, dispatch
    from oracle import O1
    from oracle.pytrie import aggre
    o1 = O1(nf)
    o1.insert_many(fb, fo)
    oc, oo, oi = o1.match_ids(tb, to[: k + 1], threads=16)
    filters = W.unpack(fb, fo)
    off = bt.o[: k + 1].cpu().numpy()
    cnt = bt.c[:k].cpu().numpy()
    soff = bt.so[: k + 1].cpu().numpy()
    scnt = bt.sc[:k].cpu().numpy()
    hi, shi = int(off[k]), int(soff[k])
    tov, ndv = bt.to[:hi].cpu().numpy().view(np.uint32), bt.nd[:hi].cpu().numpy().view(np.uint32)
    stov, sidv = bt.sto[:shi].cpu().numpy().view(np.uint32), bt.sid[:shi].cpu().numpy().view(np.uint32)
    bag = SubscriberBag()
    for t in range(k):
        ids = [int(f) for f in oi[int(oo[t]):int(oo[t + 1])]]
        want_del = aggre([(filters[f], NODE) for f in ids])      # match_routes: one local route per filter
        fid = {filters[f]: f for f in ids}
        for f in ids:
            if filters[f] not in bag.tab and bag_of(f):
                bag.tab[filters[f]] = bag_of(f)
        want_nd, want_pairs = [], []
        for name, _x in want_del:
            c, sent = dispatch(bag, name)
            want_nd.append(c)
            want_pairs.extend((fid[name], s) for s in sent)
        a = int(off[t])
        got_to = [int(x) for x in tov[a:a + int(cnt[t])]]
        if got_to != [fid[name] for name, _x in want_del] or [int(x) for x in ndv[a:a + int(cnt[t])]] != want_nd:
            return False, "deliveries / ndisp of topic %d" % t
        s = int(soff[t])
        got = list(zip((int(x) for x in stov[s:s + int(scnt[t])]), (int(x) for x in sidv[s:s + int(scnt[t])])))
        if got != want_pairs:
            return False, "pairs of topic %d" % t
    return True, "%d topics, %d deliveries, %d pairs" % (k, hi, shi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--filters", type=int, default=None)
    ap.add_argument("--topics", type=int, default=1_000_000)
    ap.add_argument("--mean-bag", type=int, default=4)
    ap.add_argument("--skew-filters", type=int, default=16)
    ap.add_argument("--check", type=int, default=20_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dispatch", "bench_dispatch.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    # a stream of the caller's: torch's default stream (handle 0) would select the engine's own stream,
    # which events recorded on the default stream do not bracket
    st = torch.cuda.Stream(device=dev)
    nf = a.filters or W.CONFIGS[a.config]["filters"]
    rng = np.random.default_rng(17)
    fb, fo = W.filters(a.config, n=nf)
    tb, to = W.topics(a.config, n=a.topics)
    filters = W.unpack(fb, fo)

    # ---- even layout: bag sizes uniform on 1 .. 2 * mean - 1
    t0 = time.time()
    e = build_engine(fb, fo, nf)
    sizes = rng.integers(1, 2 * a.mean_bag, size=nf)
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    for k in range(int(sizes.max())):
        idx = np.nonzero(sizes > k)[0]
        sb, so = pack([filters[i] for i in idx])
        e.sub_add_many(sb, so, (start[idx] + k).astype(np.uint32))
    e.commit()
    n_subs = int(e.sub_count)
    log("even: %d filters, %d subscribers, built in %.1fs" % (nf, n_subs, time.time() - t0))
    even = Batch(e, tb, to, dev, st)
    check = None
    if a.check:
        k = min(a.check, even.n)
        even.dispatch()
        torch.cuda.synchronize(dev)
        ok, what = parity(e, even, fb, fo, nf, tb, to, lambda f: list(range(int(start[f]), int(start[f + 1]))), k)
        log("parity vs dispatch_ref:", ok, what)
        check = {"ok": ok, "what": what}
        if not ok:
            raise SystemExit("parity failed: " + what)
    even_ms, even_spread, even_host = even.time()
    # the filters the batch hits, for the skew layout's choice
    even.dispatch()
    torch.cuda.synchronize(dev)
    slots_even = even.cap - 1024
    tos = even.to[:slots_even]
    hits = torch.bincount(tos[tos >= 0].to(torch.int64), minlength=nf).cpu().numpy()[:nf]   # < 0: the topic itself
    pairs_even = even.pairs
    e.close()
    del even

    # ---- skew layout: the same subscribers on 16 filters
    per = n_subs // a.skew_filters
    target = pairs_even / per                       # hits the 16 filters should total
    order = np.argsort(hits, kind="stable")
    order = order[hits[order] > 0]
    cs = np.concatenate([[0], np.cumsum(hits[order])])
    win = cs[a.skew_filters:] - cs[:-a.skew_filters]
    w0 = int(np.argmin(np.abs(win - target)))
    chosen = order[w0:w0 + a.skew_filters]
    t0 = time.time()
    e2 = build_engine(fb, fo, nf)
    for j, f in enumerate(chosen):
        sb, so = pack([filters[int(f)]] * per)
        e2.sub_add_many(sb, so, (np.arange(per) + j * per).astype(np.uint32))
    e2.commit()
    log("skew: %d subscribers on %d filters (hits %s), built in %.1fs" % (e2.sub_count, len(chosen),
                                                                          hits[chosen].tolist(), time.time() - t0))
    skew = Batch(e2, tb, to, dev, st)
    if a.check:
        skew.dispatch()
        torch.cuda.synchronize(dev)
        pos = {int(f): j for j, f in enumerate(chosen)}
        ok, what = parity(e2, skew, fb, fo, nf, tb, to,
                          lambda f: list(range(pos[f] * per, pos[f] * per + per)) if f in pos else [], min(2000, skew.n))
        log("skew parity vs dispatch_ref:", ok, what)
        check["skew_ok"] = ok
        if not ok:
            raise SystemExit("skew parity failed: " + what)
    skew_ms, skew_spread, skew_host = skew.time()
    pairs_skew = skew.pairs
    e2.close()

    with open(os.path.join(ROOT, "profiles", "r06_k", "copy_ceiling.json")) as f:
        ceiling = json.load(f)["copy_"]["TB_s"]

    def layout(ms, spread, host, pairs, slots):
        cost = ms["dispatch"] - ms["deliveries"]
        emit = ms["dispatch"] - ms["count_only"]
        eb = pairs * 12 + slots * 16
        return {"ms_median": ms, "ms_min_max": spread, "host_clock_ms_median": host, "pairs": pairs, "delivery_slots": slots,
                "dispatch_cost_ms": cost, "count_scan_ms": ms["count_only"] - ms["deliveries"], "emit_ms": emit,
                "pairs_per_s": pairs / (cost * 1e-3) if cost > 0 else None,
                "ns_per_pair": cost * 1e6 / pairs if pairs else None,
                "emit_bytes": eb, "emit_TB_s": eb / (emit * 1e-3) / 1e12 if emit > 0 else None}
    ev = layout(even_ms, even_spread, even_host, pairs_even, slots_even)
    sk = layout(skew_ms, skew_spread, skew_host, pairs_skew, slots_even)
    out = {"workload": "C%d: %d filters, one local route each, %d subscribers; %d-topic batch" % (
               a.config, nf, n_subs, a.topics),
           "method": "HIP events around each call, 3 warm-ups, median of 10, the three calls interleaved",
           "even": ev, "skew": sk, "skew_filters": int(a.skew_filters), "skew_bag": int(per),
           "copy_ceiling_TB_s": ceiling,
           "skew_over_even_dispatch_cost": sk["dispatch_cost_ms"] / ev["dispatch_cost_ms"],
           "skew_over_even_pairs": pairs_skew / pairs_even,
           "skew_over_even_ns_per_pair": (sk["ns_per_pair"] / ev["ns_per_pair"]) if sk["ns_per_pair"] else None,
           "check": check}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
