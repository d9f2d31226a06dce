"""The shared-subscription pick (share.hip) next to the dispatch call it extends,
on one MI355X in one process.

Setup: the C2 filters (1M), one local-node route each, as tools/bench_dispatch.py.
A fraction of them (--share-frac, default 0.1) also carries a {Group, Node}
route of one of 8 groups, with a member set of 1 .. 7 members (mean 4) on that
(group, filter); the filter '#', matched by every topic of the batch, carries
two more groups with 64 members each, so two sets occur once per publish and
their round-robin runs are as long as the batch.

Timed on the same 1M-topic HBM-resident batch, interleaved, HIP events around
each call on the caller's stream, 3 warm-ups then the median of 10:
    dispatch      tm_match_dispatch_batch_device
    keyed         tm_match_publish_batch_device, TM_SHARE_KEYED
    round_robin   tm_match_publish_batch_device, TM_SHARE_ROUND_ROBIN (includes its
                  one wait for the stream, so the host clock is reported beside the events)
    sticky        tm_match_publish_batch_device, TM_SHARE_STICKY in the steady state: every
                  entry defined, so no slot is flagged and nothing is sorted (the same one
                  wait for the stream as round robin)
keyed - dispatch, round_robin - dispatch and sticky - dispatch are the added milliseconds.
The cold sticky batch -- the first of the process on this engine, every entry
undefined, every group delivery with a set flagged, compacted and sorted -- can
be taken once only: one sample, timed the same way, after a one-topic sticky
publish on a throw-away engine has loaded every kernel of the path.

After those, the same batch runs through tm_publish_stream_device (the batcher's
call for round robin and sticky) with each strategy, interleaved and timed the
same way on the built-in arrays, so sticky is in its steady state there too.

Before anything is timed, --check topics of the batch are compared with
tests/shared_ref.py over oracle aggre/1 of O1's ordered match lists: the keyed
picks, and the round-robin picks of the first call (cursors undefined; the
picks of a batch's first k topics depend on no later topic), and the sticky
picks of the cold batch against tests/sticky_ref.py.

Run:  python tools/bench_shared.py [--topics N --check K --out FILE]
      python tools/bench_shared.py --write-design FILE   (no GPU: puts the figures of FILE into DESIGN.md)
Writes profiles/shared/bench_shared.json and prints it."""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NODE = b"emqx@node00"
GROUPS = [b"grp%d" % i for i in range(8)]
HOT = [b"hot0", b"hot1"]
MARK = ("<!-- bench_shared:begin -->", "<!-- bench_shared:end -->")


def log(*a):
    print("[shared]", *a, file=sys.stderr, flush=True)


def gdest(g):
    return b"\x01" + g + b"\x00" + NODE


def write_design(path):
    with open(path) as f:
        r = json.load(f)
    ms, add = r["ms_median"], r["added_ms"]
    text = ("Measured with `tools/bench_shared.py` (%s): dispatch %.2f ms; the keyed pick adds %.2f ms, round robin "
            "%.2f ms (events on the caller's stream; host clock %.2f / %.2f / %.2f ms). %d delivery slots, %d group "
            "deliveries, %d of them ranked by the round-robin sort." %
            (r["workload"], ms["dispatch"], add["keyed"], add["round_robin"], r["host_clock_ms_median"]["dispatch"],
             r["host_clock_ms_median"]["keyed"], r["host_clock_ms_median"]["round_robin"], r["delivery_slots"],
             r["group_deliveries"], r["rr_ranked"]))
    if "sticky" in add:
        cold = r["sticky_cold"]
        text += (" Sticky in the steady state (every entry defined, nothing flagged) adds %.2f ms (host clock %.2f ms); "
                 "the cold first batch, one sample, %d slots flagged and sorted (derived, not read from the device: "
                 "with every entry undefined that is every group delivery with a set), took %.2f ms (host clock %.2f ms), "
                 "%.2f ms over the dispatch median." %
                 (add["sticky"], r["host_clock_ms_median"]["sticky"], cold["flagged"], cold["ms"], cold["host_clock_ms"],
                  cold["ms"] - ms["dispatch"]))
    if "stream_call" in r:
        sc = r["stream_call"]
        text += (" The same batch through `tm_publish_stream_device` (match, routes, aggre, dispatch, picks and pack in "
                 "one call; built-in arrays, sticky in its steady state with %d slots flagged; caps.rr %d): keyed %.2f ms, "
                 "round robin %.2f ms (%d slots ranked), sticky %.2f ms." %
                 (sc["flagged_slots_hdr5"]["sticky"], sc["caps_rr"], sc["ms_median"]["keyed"],
                  sc["ms_median"]["round_robin"], sc["flagged_slots_hdr5"]["round_robin"], sc["ms_median"]["sticky"]))
    p = os.path.join(ROOT, "DESIGN.md")
    s = open(p).read()
    pat = re.compile(re.escape(MARK[0]) + ".*?" + re.escape(MARK[1]), re.S)
    if not pat.search(s):
        raise SystemExit("DESIGN.md has no %s ... %s block" % MARK)
    open(p, "w").write(pat.sub(lambda m: MARK[0] + "\n" + text + "\n" + MARK[1], s))
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--filters", type=int, default=None)
    ap.add_argument("--topics", type=int, default=1_000_000)
    ap.add_argument("--share-frac", type=float, default=0.1)
    ap.add_argument("--check", type=int, default=20_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shared", "bench_shared.json"))
    ap.add_argument("--write-design", default=None)
    a = ap.parse_args()
    if a.write_design:
        return write_design(a.write_design)

    import torch
    from emqx_amd import Engine
    from emqx_amd import workload as W
    from emqx_amd.engine import pack
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)   # a stream of the caller's, as tools/bench_dispatch.py
    nf = a.filters or W.CONFIGS[a.config]["filters"]
    rng = np.random.default_rng(23)
    fb, fo = W.filters(a.config, n=nf)
    tb, to = W.topics(a.config, n=a.topics)
    filters = W.unpack(fb, fo)
    hot_id = filters.index(b"#") if b"#" in set(filters) else nf      # '#': the workload's own, or added last

    # ---- engine: local routes, group routes on a fraction, '#' with two groups
    t0 = time.time()
    e = Engine(device=0, filters_hint=nf + 1)
    db = np.concatenate([np.tile(np.frombuffer(NODE, dtype=np.uint8), nf), np.zeros(8, dtype=np.uint8)])
    do = np.arange(nf + 1, dtype=np.uint64) * np.uint64(len(NODE))
    e.route_add_many(fb, fo, db, do)
    e.dest_target(NODE, Engine.TARGET_NODE, NODE)
    e.set_local_node(NODE)
    for g in GROUPS + HOT:
        e.dest_target(gdest(g), Engine.TARGET_GROUP, g)
    shared = np.nonzero(rng.random(nf) < a.share_frac)[0]
    grp = rng.integers(0, len(GROUPS), size=len(shared))
    sizes = rng.integers(1, 8, size=len(shared))
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    sb, so = pack([filters[i] for i in shared])
    gb, go = pack([gdest(GROUPS[g]) for g in grp])
    e.route_add_many(sb, so, gb, go)
    for k in range(int(sizes.max())):                      # member k of every set that has one, in list order
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
    e.commit()
    log("%d filters, %d with a group route, %d members, built in %.1fs" % (nf, len(shared), e.share_count,
                                                                         time.time() - t0))

    # ---- device buffers
    n = len(to) - 1
    nbytes = int(to[-1])
    d_b = torch.from_numpy(tb).to(dev)
    d_o = torch.from_numpy(to.view(np.int64)).to(dev)
    i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
    c, o, tot = torch.empty(n, **i32), torch.empty(n + 1, **i64), torch.zeros(1, **i64)
    sc, so_, stot = torch.empty(n, **i32), torch.empty(n + 1, **i64), torch.zeros(1, **i64)
    e.match_deliveries_batch_device(d_b, d_o, n, nbytes, c, o, None, None, 0, tot, stream=st)
    torch.cuda.synchronize(dev)
    slots = int(tot.item())
    cap = slots + 1024
    dto, dtg, dnd, dpk = (torch.empty(cap, **i32) for _ in range(4))
    keys = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    d_k = torch.from_numpy(keys.view(np.int32)).to(dev)

    def dispatch(scap, sto=None, sid=None):
        e.match_dispatch_batch_device(d_b, d_o, n, nbytes, c, o, dto, dtg, dnd, cap, tot, sc, so_, sto, sid, scap, stot,
                                      stream=st)
    dispatch(0)
    torch.cuda.synchronize(dev)
    scap = int(stot.item()) + 1024
    sto, sid = torch.empty(scap, **i32), torch.empty(scap, **i32)

    def publish(strategy):
        e.match_publish_batch_device(d_b, d_o, n, nbytes, c, o, dto, dtg, dnd, cap, tot, sc, so_, sto, sid, scap, stot,
                                     strategy, None if strategy == Engine.SHARE_ROUND_ROBIN else d_k, dpk, stream=st)

    # the sticky kernels loaded by a one-topic publish on a throw-away engine, so
    # that the one cold batch below pays for its work only
    w = Engine(device=0)
    w.route_add(b"w", gdest(b"w"))
    w.dest_target(gdest(b"w"), Engine.TARGET_GROUP, b"w")
    w.dest_target(NODE, Engine.TARGET_NODE, NODE)
    w.set_local_node(NODE)
    kb, ko = pack([b"x"] * 300)                            # 300 more sets: the set indices need a radix pass
    mb, mo = pack([b"x/%d" % i for i in range(300)])
    w.share_add_many(kb, ko, mb, mo, np.arange(300, dtype=np.uint32))
    w.share_add(b"w", b"w", 1001)
    w.share_add(b"w", b"w", 1002)
    wb, wo = pack([b"w"])
    assert int(w.match_publish_batch(wb, wo, Engine.SHARE_STICKY, [1])[9][0]) == 1002
    w.close()

    def timed(fn):
        ea, eb = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        ea.record(st)
        fn()
        eb.record(st)
        torch.cuda.synchronize(dev)
        return ea.elapsed_time(eb), (time.perf_counter() - t0) * 1e3
    cold_ms, cold_host = timed(lambda: publish(Engine.SHARE_STICKY))   # the only batch that finds no entry defined
    cold_off, cold_cnt = o.cpu().numpy(), c.cpu().numpy()
    cold_pk = dpk[:slots].cpu().numpy().view(np.uint32).copy()

    # ---- parity of the first k topics
    check = None
    if a.check:
        from oracle import O1
        from oracle.pytrie import aggre
        from shared_ref import SharedSub
        from sticky_ref import StickySub
        k = min(a.check, n)
        names = filters + ([b"#"] if hot_id == nf else [])
        fb2, fo2 = pack(names)
        o1 = O1(len(names))
        o1.insert_many(fb2, fo2)
        oc, oo, oi = o1.match_ids(tb, to[: k + 1], threads=16)
        gof = {int(f): int(g) for f, g in zip(shared, grp)}
        ref = SharedSub()
        for i, f in enumerate(shared):
            for m in range(int(start[i]), int(start[i + 1])):
                ref.subscribe(GROUPS[grp[i]], filters[f], m)
        for j, g in enumerate(HOT):
            for m in range(64):
                ref.subscribe(g, b"#", hot_base + 64 * j + m)
        sref = StickySub()
        sref.tab, sref.alive = ref.tab, {m for ms_ in ref.tab.values() for m in ms_}
        want = {"keyed": [], "round_robin": [], "sticky": []}
        for t in range(k):
            routes = []
            for f in (int(x) for x in oi[int(oo[t]):int(oo[t + 1])]):
                if f < nf:
                    routes.append((names[f], NODE))
                    if f in gof:
                        routes.append((names[f], (GROUPS[gof[f]], NODE)))
                if f == hot_id:
                    routes += [(b"#", (g, NODE)) for g in HOT]
            dels = aggre(routes)
            for s in want:
                if s == "sticky":
                    want[s].append([sref.pick(s, int(keys[t]), x, name) if kind == 1 else None for name, (kind, x) in dels])
                    continue
                want[s].append([ref.do_pick(s, int(keys[t]), x, name) if kind == 1 else None
                                for name, (kind, x) in dels])
        check = {"topics": k}
        for s, strategy in (("keyed", Engine.SHARE_KEYED), ("round_robin", Engine.SHARE_ROUND_ROBIN), ("sticky", None)):
            if strategy is None:                           # the cold batch above: it cannot be run again
                off, cnt, pk = cold_off[: k + 1], cold_cnt[:k], cold_pk
            else:
                publish(strategy)
                torch.cuda.synchronize(dev)
                off, cnt = o[: k + 1].cpu().numpy(), c[:k].cpu().numpy()
                pk = dpk[: int(off[k])].cpu().numpy().view(np.uint32)
            for t in range(k):
                got = [None if int(x) == Engine.NO_MEMBER else int(x) for x in pk[int(off[t]):int(off[t]) + int(cnt[t])]]
                if got != want[s][t]:
                    raise SystemExit("parity failed: %s picks of topic %d: %s, want %s" % (s, t, got, want[s][t]))
            check[s] = True
        log("parity vs shared_ref:", check)

    # ---- timing
    fns = {"dispatch": lambda: dispatch(scap, sto, sid), "keyed": lambda: publish(Engine.SHARE_KEYED),
           "round_robin": lambda: publish(Engine.SHARE_ROUND_ROBIN), "sticky": lambda: publish(Engine.SHARE_STICKY)}
    ms, host = {k_: [] for k_ in fns}, {k_: [] for k_ in fns}
    warmups, runs = 3, 10
    for it in range(warmups + runs):
        for name, fn in fns.items():
            dev_ms, host_ms = timed(fn)
            if it >= warmups:
                ms[name].append(dev_ms)
                host[name].append(host_ms)
    med = {k_: float(np.median(v)) for k_, v in ms.items()}
    hmed = {k_: float(np.median(v)) for k_, v in host.items()}

    # ---- the same batch through tm_publish_stream_device (the batcher's call for round robin and sticky), the
    # three strategies interleaved in the same way; built-in arrays, so sticky is in its steady state.  That call
    # reads nothing back: with nothing flagged it still scans the flags and sorts caps.rr padding pairs.
    caps = (cap, cap, scap, int(slots // 8) + 1024)        # match ids <= routes here: every filter has a local route
    wsb = e.publish_stream_workspace_bytes(n, nbytes, caps)
    d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    d_hdr, d_doff, d_soff = torch.zeros(8, **i64), torch.empty(n + 1, **i64), torch.empty(n + 1, **i64)
    d_deliv, d_pairs = torch.empty(cap * 4, **i32), torch.empty(scap * 2, **i32)

    def stream(strategy):
        e.publish_stream_device(d_b, d_o, n, nbytes, strategy, None if strategy == Engine.SHARE_ROUND_ROBIN else d_k,
                                None, caps, d_ws, wsb, d_hdr, d_doff, d_soff, d_deliv, d_pairs, stream=st)
    sfns = {"keyed": Engine.SHARE_KEYED, "round_robin": Engine.SHARE_ROUND_ROBIN, "sticky": Engine.SHARE_STICKY}
    sms, sflag = {k_: [] for k_ in sfns}, {}
    for it in range(warmups + runs):
        for name, strategy in sfns.items():
            dev_ms, _ = timed(lambda: stream(strategy))
            h = [int(x) for x in d_hdr.cpu().numpy()]
            if h[6] != 0:
                raise SystemExit("stream call %s: state %d, header %s" % (name, h[6], h))
            sflag[name] = h[5]
            if it >= warmups:
                sms[name].append(dev_ms)
    smed = {k_: float(np.median(v)) for k_, v in sms.items()}
    publish(Engine.SHARE_KEYED)
    torch.cuda.synchronize(dev)
    tg_h = dtg[:slots].cpu().numpy()
    pk_h = dpk[:slots].cpu().numpy().view(np.uint32)
    off_h, cnt_h = o.cpu().numpy(), c.cpu().numpy()
    live = np.zeros(slots, dtype=bool)                     # slots that hold a delivery (the rest are aggre's holes)
    pos = np.arange(slots) - np.repeat(off_h[:-1], np.diff(off_h))
    live[:] = pos < np.repeat(cnt_h, np.diff(off_h))
    group_tg = {t for t in np.unique(tg_h[live]) if e.target_bytes(int(t))[0] == Engine.TARGET_GROUP}
    is_group = live & np.isin(tg_h, list(group_tg))
    out = {"workload": "C%d: %d filters, one local route each, %d with a group route and a member set (mean 4), "
                       "'#' with 2 groups of 64; %d-topic batch" % (a.config, nf, len(shared), a.topics),
           "method": "HIP events around each call on the caller's stream, 3 warm-ups, median of 10, the four calls "
                     "interleaved; sticky_cold: the engine's first sticky batch, one sample",
           "ms_median": med, "ms_min_max": {k_: [min(v), max(v)] for k_, v in ms.items()},
           "host_clock_ms_median": hmed,
           "added_ms": {k_: med[k_] - med["dispatch"] for k_ in ("keyed", "round_robin", "sticky")},
           "added_host_clock_ms": {k_: hmed[k_] - hmed["dispatch"] for k_ in ("keyed", "round_robin", "sticky")},
           "stream_call": {"ms_median": smed, "ms_min_max": {k_: [min(v), max(v)] for k_, v in sms.items()},
                           "flagged_slots_hdr5": sflag, "caps_rr": caps[3]},
           "delivery_slots": slots, "group_deliveries": int(is_group.sum()),
           "picks": int((is_group & (pk_h != Engine.NO_MEMBER)).sum()),
           "members": int(e.share_count), "check": check}
    # the slots round robin ranks: group deliveries whose set has >= 2 members
    one = {(GROUPS[grp[i]], int(shared[i])) for i in np.nonzero(sizes == 1)[0]}
    to_h = dto[:slots].cpu().numpy().view(np.uint32)
    tname = {int(t): e.target_bytes(int(t))[1] for t in group_tg}
    gi = np.nonzero(is_group)[0]
    # the cold sticky batch flags every group delivery that has a set = every one with a pick:
    # derived from the keyed batch's picks, the call does not report its own count
    out["sticky_cold"] = {"ms": cold_ms, "host_clock_ms": cold_host, "flagged": out["picks"],
                          "flagged_is": "derived: group deliveries with a pick, every entry being undefined"}
    out["rr_ranked"] = int(sum(1 for j in gi if (tname[int(tg_h[j])], int(to_h[j])) not in one))
    e.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
