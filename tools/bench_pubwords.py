#!/usr/bin/env python3
"""The stream-ordered publish call with the delivery words against the plain
one: tm_publish_stream_opts_device vs tm_publish_stream_device, interleaved in
one process, for the three pick strategies.

Workload: tools/bench_shared.py's -- a C2 trie, one local route per filter, a
fraction of the filters with a $share group route and a member set of 1..7
members (mean 4), '#' with two groups of 64 -- plus what the words need: every
filter has one plain subscriber and every member its emqx_suboption entry, so
each pair and each pick has an option word to read.  Random pub_flags, a
publisher id on every fourth publish.

Method: HIP events on the caller's stream around each call, 3 warm-ups, median
of 10, plain and options calls alternating.  Before the timing a sample of the
words is checked: every pair word and pick word of the first --check publishes
against tm_deliver_word over tm_sub_get_opts (the composition
tests/pickword_ref.py states), and the records against the plain call's.

--plain-only [--lib PATH]: the plain call alone, optionally on another build of
the library (the parent commit's, for "the plain call has not slowed"): one
JSON line, three of which from alternating fresh processes make
profiles/pubwords/ab_plain.jsonl.

Writes profiles/pubwords/bench_pubwords.json and prints it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NODE = b"emqx@node00"
GROUPS = [b"grp%d" % i for i in range(8)]
HOT = [b"hot0", b"hot1"]
WARMUPS, RUNS = 3, 10


def log(*a):
    print("[pubwords]", *a, file=sys.stderr, flush=True)


def gdest(g):
    return b"\x01" + g + b"\x00" + NODE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--filters", type=int, default=None)
    ap.add_argument("--topics", type=int, default=1_000_000)
    ap.add_argument("--share-frac", type=float, default=0.1)
    ap.add_argument("--check", type=int, default=2_000)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--lib", default=None, help="another build of libtopicmatch.so (with --plain-only)")
    ap.add_argument("--tag", default=None, help="--plain-only: a label for the JSON line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pubwords", "bench_pubwords.json"))
    a = ap.parse_args()
    if a.lib:
        if not a.plain_only:
            raise SystemExit("--lib goes with --plain-only: an older build has no call with options")
        from emqx_amd import _lib
        _lib.LIB_PATH = os.path.abspath(a.lib)

    import torch
    from emqx_amd import Engine
    from emqx_amd import workload as W
    from emqx_amd.engine import pack
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    nf = a.filters or W.CONFIGS[a.config]["filters"]
    rng = np.random.default_rng(23)
    fb, fo = W.filters(a.config, n=nf)
    tb, to = W.topics(a.config, n=a.topics)
    filters = W.unpack(fb, fo)

    # ---- engine: bench_shared's routes and member sets ...
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
    member_base = 1 << 24                                  # member ids above the plain subscribers'

    def opt_words(k):
        w = rng.integers(0, 3, size=k) | (rng.integers(0, 2, size=k) << 2) | (rng.integers(0, 2, size=k) << 3)
        return (w | (rng.integers(0, 1 << 20, size=k) << 4) * (rng.random(k) < 0.4)).astype(np.uint32)

    for k in range(int(sizes.max())):                      # member k of every set that has one, in list order
        idx = np.nonzero(sizes > k)[0]
        mb, mo = pack([filters[shared[i]] for i in idx])
        kb, ko = pack([GROUPS[grp[i]] for i in idx])
        ids = (member_base + start[idx] + k).astype(np.uint32)
        e.share_add_many(kb, ko, mb, mo, ids)
        if not a.plain_only:                               # ... and each member's option entry
            e.sub_add_opts_many(mb, mo, ids, opt_words(len(idx)), kb, ko, np.ones(len(idx), dtype=np.uint8))
    hot_base = member_base + int(start[-1])
    for j, g in enumerate(HOT):
        e.route_add(b"#", gdest(g))
        kb, ko = pack([g] * 64)
        mb, mo = pack([b"#"] * 64)
        ids = (hot_base + 64 * j + np.arange(64)).astype(np.uint32)
        e.share_add_many(kb, ko, mb, mo, ids)
        if not a.plain_only:
            e.sub_add_opts_many(mb, mo, ids, opt_words(64), kb, ko, np.ones(64, dtype=np.uint8))
    subs = np.arange(nf, dtype=np.uint32)                  # one plain subscriber per filter
    if a.plain_only:
        e.sub_add_many(fb, fo, subs)
    else:
        e.sub_add_opts_many(fb, fo, subs, opt_words(nf))
    e.commit()
    log("%d filters, %d with a group route, %d members, %d subscribers, built in %.1fs"
        % (nf, len(shared), e.share_count, e.sub_count, time.time() - t0))

    # ---- device buffers, capacities from one sizing pass
    n = len(to) - 1
    nbytes = int(to[-1])
    d_b = torch.from_numpy(tb.copy()).to(dev)
    d_o = torch.from_numpy(to.view(np.int64).copy()).to(dev)
    i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
    c, o, tot = torch.empty(n, **i32), torch.empty(n + 1, **i64), torch.zeros(1, **i64)
    sc, so_, stot = torch.empty(n, **i32), torch.empty(n + 1, **i64), torch.zeros(1, **i64)
    e.match_deliveries_batch_device(d_b, d_o, n, nbytes, c, o, None, None, 0, tot, stream=st)
    torch.cuda.synchronize(dev)
    slots = int(tot.item())
    cap = slots + 1024
    dto, dtg, dnd = (torch.empty(cap, **i32) for _ in range(3))
    e.match_dispatch_batch_device(d_b, d_o, n, nbytes, c, o, dto, dtg, dnd, cap, tot, sc, so_, None, None, 0, stot,
                                  stream=st)
    torch.cuda.synchronize(dev)
    pairs_total = int(stot.item())
    scap = pairs_total + 1024
    keys = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    d_k = torch.from_numpy(keys.view(np.int32)).to(dev)
    pf = (rng.integers(0, 3, size=n) | (rng.integers(0, 2, size=n) << 2) | ((rng.random(n) < 0.2) << 3)).astype(np.uint32)
    fr = np.where(np.arange(n) % 4 == 0, rng.integers(0, nf, size=n), 0xFFFFFFFF).astype(np.uint32)
    d_pf, d_fr = torch.from_numpy(pf.view(np.int32)).to(dev), torch.from_numpy(fr.view(np.int32)).to(dev)
    caps = (cap, cap, scap, int(slots // 8) + 1024)        # match ids <= routes here: every filter has a local route
    wsb = e.publish_stream_workspace_bytes(n, nbytes, caps)
    wso = 0 if a.plain_only else e.publish_stream_opts_workspace_bytes(n, nbytes, caps)
    d_ws = torch.empty(max(wsb, wso), dtype=torch.uint8, device=dev)
    d_hdr, d_doff, d_soff = torch.zeros(8, **i64), torch.empty(n + 1, **i64), torch.empty(n + 1, **i64)
    d_deliv, d_pairs = torch.empty(cap * 4, **i32), torch.empty(scap * 2, **i32)
    d_pkw, d_prw = torch.empty(cap, **i32), torch.empty(scap, **i32)
    strategies = {"keyed": Engine.SHARE_KEYED, "round_robin": Engine.SHARE_ROUND_ROBIN, "sticky": Engine.SHARE_STICKY}

    def plain(s):
        e.publish_stream_device(d_b, d_o, n, nbytes, s, None if s == Engine.SHARE_ROUND_ROBIN else d_k, None, caps,
                                d_ws, wsb, d_hdr, d_doff, d_soff, d_deliv, d_pairs, stream=st)

    def opts(s):
        e.publish_stream_opts_device(d_b, d_o, n, nbytes, s, None if s == Engine.SHARE_ROUND_ROBIN else d_k, None,
                                     caps, d_ws, wso, d_hdr, d_doff, d_soff, d_deliv, d_pairs,
                                     (d_pf, d_fr, 0, d_prw), d_pkw, stream=st)

    def timed(fn):
        ea, eb = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        ea.record(st)
        fn()
        eb.record(st)
        torch.cuda.synchronize(dev)
        h = [int(x) for x in d_hdr.cpu().numpy()]
        if h[6] != 0:
            raise SystemExit("stream call: state %d, header %s" % (h[6], h))
        return ea.elapsed_time(eb), h

    check = None
    if not a.plain_only:
        # ---- a sample of the words, and the records against the plain call's
        plain(Engine.SHARE_KEYED)
        torch.cuda.synchronize(dev)
        ref = (d_hdr.cpu().numpy().copy(), d_doff.cpu().numpy().copy(), d_deliv.cpu().numpy().copy(),
               d_pairs.cpu().numpy().copy())
        opts(Engine.SHARE_KEYED)
        torch.cuda.synchronize(dev)
        hdr = d_hdr.cpu().numpy()
        D, P = int(hdr[2]), int(hdr[3])
        assert (hdr == ref[0]).all() and (d_doff.cpu().numpy() == ref[1]).all()
        assert (d_deliv.cpu().numpy()[:D * 4] == ref[2][:D * 4]).all() and (d_pairs.cpu().numpy()[:P * 2] == ref[3][:P * 2]).all()
        doff, soff = d_doff.cpu().numpy(), d_soff.cpu().numpy()
        deliv = d_deliv.cpu().numpy().view(np.uint32)[:D * 4].reshape(-1, 4)
        prs = d_pairs.cpu().numpy().view(np.uint32)[:P * 2].reshape(-1, 2)
        pkw, prw = d_pkw.cpu().numpy().view(np.uint32), d_prw.cpu().numpy().view(np.uint32)
        names = {}

        def to_bytes(s, t):
            if s == Engine.TOPIC_ROUTE:
                return bytes(tb[int(to[t]):int(to[t + 1])])
            if s not in names:
                names[s] = e.filter_bytes(s)
            return names[s]

        def word(topic, sub, t):
            w = e.sub_get_opts(topic, sub)
            return e.deliver_word(Engine.SUBOPT_NONE if w is None else w, int(pf[t]),
                                  int(fr[t]) != 0xFFFFFFFF and int(fr[t]) == sub, 0)
        pair_n = pick_n = none_n = 0
        for t in range(min(a.check, n)):
            for p in range(int(soff[t]), int(soff[t + 1])):
                assert int(prw[p]) == word(to_bytes(int(prs[p][0]), t), int(prs[p][1]), t), ("pair word", t, p)
                pair_n += 1
            for g in range(int(doff[t]), int(doff[t + 1])):
                m = int(deliv[g][3])
                if m == Engine.NO_MEMBER:
                    assert int(pkw[g]) == Engine.NO_WORD, ("no pick", t, g)
                    none_n += 1
                else:
                    assert int(pkw[g]) == word(to_bytes(int(deliv[g][0]), t), m, t), ("pick word", t, g)
                    pick_n += 1
        check = {"publishes": min(a.check, n), "pair_words": pair_n, "pick_words": pick_n, "slots_without_pick": none_n}
        log("checked", check)

    ms = {("plain", k): [] for k in strategies}
    if not a.plain_only:
        ms.update({("opts", k): [] for k in strategies})
    hdrs = {}
    for it in range(WARMUPS + RUNS):
        for name, s in strategies.items():
            for kind, fn in (("plain", plain), ("opts", opts)):
                if (kind, name) not in ms:
                    continue
                dt, h = timed(lambda: fn(s))
                hdrs[name] = h
                if it >= WARMUPS:
                    ms[(kind, name)].append(dt)
    med = {"%s_%s" % k: float(np.median(v)) for k, v in ms.items()}
    rng_ = {"%s_%s" % k: [min(v), max(v)] for k, v in ms.items()}
    h = hdrs["keyed"]
    out = {"workload": "C%d: %d filters, one local route and one plain subscriber each, %d with a group route and a "
                       "member set (mean 4), '#' with 2 groups of 64; %d-topic batch"
                       % (a.config, nf, len(shared), a.topics),
           "method": "HIP events around each call on the caller's stream, 3 warm-ups, median of 10, the calls interleaved",
           "ms_median": med, "ms_min_max": rng_, "route_total": h[0], "pairs": h[1], "records": h[2],
           "flagged_slots_hdr5": {k: v[5] for k, v in hdrs.items()}, "members": int(e.share_count)}
    if a.plain_only:
        out["tag"] = a.tag or (os.path.basename(a.lib) if a.lib else "this")
        e.close()
        print(json.dumps(out), flush=True)
        return
    out["added_ms"] = {k: med["opts_" + k] - med["plain_" + k] for k in strategies}
    out["check"] = check
    d_pk = d_deliv.cpu().numpy().view(np.uint32)[:h[2] * 4].reshape(-1, 4)[:, 3]
    out["picks"] = int((d_pk != Engine.NO_MEMBER).sum())
    e.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
