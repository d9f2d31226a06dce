"""Publish admission (admit.hip, tm_admit_batch_device) and the gated stream
call (tm_publish_stream_gated_device) next to what they replace, on one MI355X
in one process.

Setup: that of tools/bench_inbox_stream.py -- the C2 filters (1M), one
local-node route each, about 4M subscribers with random option words; a
1M-topic HBM-resident batch, every publish with a QoS and a publisher id.  The
ACL rule set denies one client id and allows the rest, so the share of refused
publishes is the share of publishes that carry that id.

All variants run on one stream, interleaved, 3 warm-ups then the median of 10;
device time from HIP events on that stream, wall time from before the first
call until the stream is idle.

(a) the gate when nothing is refused: tm_publish_stream_opts_device (the
    ungated entry: its route kernels get a NULL plane) against
    tm_publish_stream_gated_device with a plane of zeros, same batch, same
    capacities.  The ungated side's spread (max - min of its 10) is reported
    beside the difference of the medians.  Both sides come from the library of
    this checkout: a library built from another commit is not loaded.
(b) the admission kernel alone, next to tm_tokenize's time for the same batch
    (tm_last_kernel_times of a timed match): both read the topic bytes once.
(c) the chain ACL check -> admission -> gated call with 1 % and 10 % refused,
    against ACL check -> read-back -> compaction of the batch on the host ->
    H2D -> ungated call.  The outputs of the two must agree on every total.

Run: python tools/bench_admit.py [--topics 1000000]
Writes profiles/admit/bench_admit.json and prints it."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from emqx_amd import Engine  # noqa: E402
from emqx_amd import workload as W  # noqa: E402
from emqx_amd.emqx_access import AclRules, Zones  # noqa: E402
from emqx_amd.engine import pack  # noqa: E402
from bench_inbox import build_engine  # noqa: E402

WARMUPS, RUNS = 3, 10


def log(*a):
    print("[admit]", *a, file=sys.stderr, flush=True)


class Out:
    """the outputs and workspace of one stream call with options"""

    def __init__(self, e, n, nbytes, caps, dev):
        i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
        self.caps = caps
        self.ws_bytes = e.publish_stream_opts_workspace_bytes(n, nbytes, caps)
        assert self.ws_bytes > 0
        self.ws = torch.empty(self.ws_bytes // 8 + 1, **i64)
        self.hdr, self.doff, self.soff = (torch.zeros(k, **i64) for k in (8, n + 1, n + 1))
        self.deliv, self.pairs = torch.empty(caps[1] * 4, **i32), torch.empty(caps[2] * 2, **i32)
        self.pickw, self.pairw = torch.empty(caps[1], **i32), torch.empty(caps[2], **i32)

    def header(self):
        return [int(x) for x in self.hdr.cpu()]


def publish(e, d, n, nbytes, o, st, code=False):
    """d = (bytes, offsets, keys, flags, from); code False: the ungated entry, else the gated one with that plane"""
    a = (d[0], d[1], n, nbytes, Engine.SHARE_KEYED, d[2], None, o.caps, o.ws, o.ws_bytes, o.hdr, o.doff, o.soff, o.deliv,
         o.pairs, (d[3], d[4], 0, o.pairw), o.pickw)
    if code is False:
        e.publish_stream_opts_device(*a, stream=st)
    else:
        e.publish_stream_gated_device(*a, code, stream=st)


def timed(sides, dev, st):
    """sides: {name: callable}; -> {name: {device_ms: [...], wall_ms: [...]}} over RUNS interleaved runs"""
    out = {k: {"device_ms": [], "wall_ms": []} for k in sides}
    for it in range(WARMUPS + RUNS):
        for name, fn in sides.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            ev[0].record(st)
            fn()
            ev[1].record(st)
            st.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            if it >= WARMUPS:
                out[name]["device_ms"].append(ev[0].elapsed_time(ev[1]))
                out[name]["wall_ms"].append(wall)
    return out


def summary(runs):
    return {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in runs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--filters", type=int, default=None)
    ap.add_argument("--topics", type=int, default=1_000_000)
    ap.add_argument("--mean-bag", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "admit", "bench_admit.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    nf = a.filters or W.CONFIGS[a.config]["filters"]
    n = a.topics
    rng = np.random.default_rng(23)
    fb, fo = W.filters(a.config, n=nf)
    tb, to = W.topics(a.config, n=n)
    filters = W.unpack(fb, fo)
    t0 = time.time()
    e = build_engine(fb, fo, nf)
    sizes = rng.integers(1, 2 * a.mean_bag, size=nf)
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    for k in range(int(sizes.max())):
        idx = np.nonzero(sizes > k)[0]
        sb, so = pack([filters[i] for i in idx])
        opts = (rng.integers(0, 3, size=len(idx)) | rng.integers(0, 2, size=len(idx)) << 2 |
                rng.integers(0, 2, size=len(idx)) << 3).astype(np.uint32)
        e.sub_add_opts_many(sb, so, (start[idx] + k).astype(np.uint32), opts)
    e.commit()
    n_subs = int(e.sub_count)
    log("%d filters, %d subscribers, built in %.1fs" % (nf, n_subs, time.time() - t0))
    nbytes = int(to[n])
    pf = rng.integers(0, 3, size=n).astype(np.uint32)
    fr = rng.integers(0, n_subs, size=n).astype(np.uint32)
    keys = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    up = lambda x, dt=None: torch.from_numpy(np.ascontiguousarray(x).view(dt) if dt else np.ascontiguousarray(x)).to(dev)  # noqa: E731,E501
    hb = np.concatenate([tb[:nbytes], np.zeros(8, np.uint8)])
    d = (up(hb), up(to[:n + 1], np.int64), up(keys, np.int32), up(pf, np.int32), up(fr, np.int32))

    # capacities: a roomy run learns the totals, then the batcher's rule (1.25 x + 1024)
    room = [16 * n + 1024] * 3 + [0]
    for _ in range(4):   # as a batcher lane does: the stage the header names grows to its total
        o = Out(e, n, nbytes, tuple(room), dev)
        publish(e, d, n, nbytes, o, st)
        st.synchronize()
        h = o.header()
        if h[6] == 0:
            break
        room[h[6] - 1] = {1: h[4], 2: h[0], 3: h[1]}[h[6]] + 1024
        del o
        torch.cuda.empty_cache()
    assert h[6] == 0, "the sizing runs did not fit: %s" % h
    caps = tuple(int(x * 1.25) + 1024 for x in (h[4], h[0], h[1])) + (0,)
    del o
    torch.cuda.empty_cache()
    o = Out(e, n, nbytes, caps, dev)
    zero = torch.zeros(n, dtype=torch.uint8, device=dev)

    # (a) the gate with nothing refused
    ra = timed({"opts_ungated": lambda: publish(e, d, n, nbytes, o, st),
                "gated_zero_plane": lambda: publish(e, d, n, nbytes, o, st, zero)}, dev, st)
    sa = {k: summary(v) for k, v in ra.items()}
    spread = sa["opts_ungated"]["device_ms"]["max"] - sa["opts_ungated"]["device_ms"]["min"]
    diff = sa["gated_zero_plane"]["device_ms"]["median"] - sa["opts_ungated"]["device_ms"]["median"]
    gate = {"ms": sa, "gated_minus_ungated_median_ms": diff, "ungated_spread_ms": spread,
            "within_spread": bool(diff <= spread), "totals": h[:6]}
    log(json.dumps(gate))

    # (b) the admission kernel alone, next to tm_tokenize
    zones = Zones()
    zones.add("default")
    d_code, d_ahdr = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(8, dtype=torch.int64, device=dev)
    d_pa = torch.zeros(n, dtype=torch.int32, device=dev)
    rb = timed({"admit": lambda: Engine.admit_batch_device(d[0], d[1], n, None, d[3], d_pa, zones, None, d_code, d_ahdr,
                                                           stream=st)}, dev, st)
    e.set_timing(True)
    e.match_batch(hb, to[:n + 1])
    kt = e.last_kernel_times()
    e.set_timing(False)
    kernel = {"admit_ms": summary(rb["admit"])["device_ms"], "match_kernel_times_ms": kt, "topic_bytes": nbytes,
              "admit_GBps": nbytes / (np.median(rb["admit"]["device_ms"]) * 1e-3) / 1e9}
    log(json.dumps(kernel))

    # (c) the chain against read-back and host compaction
    acl = AclRules(0).load([("deny", ("client", "bad"), "publish", ["#"]), ("allow", "all", "publish", ["#"])])
    chains = []
    for pct in (1, 10):
        bad = rng.random(n) < pct / 100.0
        creds = [{"client_id": "bad" if b else "ok", "username": None} for b in bad]
        pk = AclRules.pack(creds, ["publish"] * n, [b""] * n)
        dd = {k: up(pk[k]) for k in AclRules.ARGS if k not in ("topics", "topic_off")}
        dd["topics"], dd["topic_off"] = d[0], d[1]
        d_acl, d_rule = torch.zeros(n, dtype=torch.int8, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
        o2 = Out(e, n, nbytes, caps, dev)

        def new_chain():
            acl.check_device(n, dd, d_acl, d_rule, stream=st)
            Engine.admit_batch_device(d[0], d[1], n, None, d[3], d_pa, zones, d_acl, d_code, d_ahdr, stream=st)
            publish(e, d, n, nbytes, o, st, d_code)
        kept = {}

        def old_chain():
            acl.check_device(n, dd, d_acl, d_rule, stream=st)
            st.synchronize()
            keep = d_acl.cpu().numpy() == 1                          # the read-back
            ln = (to[1:n + 1] - to[:n]).astype(np.int64)[keep]       # the compaction on the host
            off2 = np.concatenate([[0], np.cumsum(ln)]).astype(np.uint64)
            src = np.repeat(to[:n][keep].astype(np.int64) - off2[:-1].astype(np.int64), ln) + np.arange(int(off2[-1]))
            hb2 = np.concatenate([hb[src], np.zeros(8, np.uint8)])
            m = int(keep.sum())
            with torch.cuda.stream(st):
                d2 = (up(hb2), up(off2, np.int64), up(keys[keep], np.int32), up(pf[keep], np.int32),
                      up(fr[keep], np.int32))
            kept["d2"], kept["m"] = d2, m
            publish(e, d2, m, int(off2[-1]), o2, st)
        rc = timed({"acl_admit_gated": new_chain, "acl_readback_compact_ungated": old_chain}, dev, st)
        hn, ho = o.header(), o2.header()
        acodes = [int(x) for x in d_ahdr.cpu()]
        assert hn[6] == 0 == ho[6] and hn[:4] == ho[:4], (hn, ho)
        assert acodes[0] + acodes[5] == n == acodes[0] + int(bad.sum()), acodes
        row = {"refused_pct": pct, "refused": acodes[5], "admitted": acodes[0], "ms": {k: summary(v) for k, v in rc.items()},
               "totals": hn[:4]}
        log(json.dumps(row))
        chains.append(row)
        del o2

    out = {"workload": "C%d: %d filters, one local route each, %d subscribers; %d-topic batch, %d topic bytes"
                       % (a.config, nf, n_subs, n, nbytes),
           "method": "HIP events on one stream and wall clock, %d warm-ups, %d runs, variants interleaved" % (WARMUPS, RUNS),
           "gate_nothing_refused": gate, "admission_kernel": kernel, "chain": chains,
           "not_measured": "the parent commit's own library in the same session; the batcher's admission mode (no flood driver for it)"}
    acl.close()
    e.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
