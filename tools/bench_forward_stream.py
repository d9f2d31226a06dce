"""The stream-ordered forward plan (forward.hip, tm_forward_plan_stream_device)
and the batcher's forward mode next to what they replace, on one MI355X in one
process.

Setup: that of tools/bench_forward.py -- the C2 filters (1M), one route each,
the routes spread evenly over the local node and R remote nodes (R = 4 and 64),
no subscribers.

(a) per batch size, on one stream, interleaved, 3 warm-ups then the median of 10:
      readback  tm_publish_stream_device, then tm_forward_plan_device over the
                same batch's results as planes (split out of the packed records
                once, outside the timed part; out_cap is the exact D, its result
                arrays the exact M and G: the best case for this side).  Its one
                read-back and host wait are inside.
      stream    the same publish call, then tm_forward_plan_stream_device over
                the packed outputs, nothing between them; capacities by the
                batcher's rule (1.25 x the totals + 1024), pub_cap = group_cap =
                deliv_cap.
    Device time from HIP events (publish and plan apart), host wall time from
    before the publish call until the stream is idle.  pub_cap / M is reported
    beside the times: the stream form sorts pub_cap pairs, the other M.  The two
    plans must be equal byte for byte.
(b) the flood of tools/bench_batcher.py (16 producer threads, 4 lanes, deadline
    200 us) through a publish batcher on the stream-ordered call whose callbacks
    collect the TM_NOT_LOCAL records and regroup them per node on the host, and
    through the forward mode (tools/ubench/fwddrive.cpp), interleaved rounds:
    topics/s, p50, p99, device and callback time per batch.

Run: python tools/bench_forward_stream.py [--topics 4096,32768,131072 --flood-topics 1048576 --rounds 3]
Writes profiles/forward_stream/bench_forward_stream.json and prints it."""
import argparse
import ctypes
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
from bench_forward import build_engine  # noqa: E402


def log(*a):
    print("[forward-stream]", *a, file=sys.stderr, flush=True)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


class Batch:
    """the first n topics of the batch through both chains"""

    def __init__(self, e, tb, to, n, keys, dev, st):
        self.e, self.dev, self.st, self.n = e, dev, st, n
        self.nbytes = int(to[n])
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)   # noqa: E731
        self.d_b = torch.from_numpy(np.concatenate([tb[: self.nbytes], np.zeros(8, np.uint8)])).to(dev)
        self.d_o = up(to[: n + 1], np.int64)
        self.d_k = up(keys[:n], np.int32)
        self.i32 = dict(dtype=torch.int32, device=dev)
        self.i64 = dict(dtype=torch.int64, device=dev)
        # a first run with room learns the totals; then the batcher's rule sizes the capacities
        caps = [64 * n + 1024, 64 * n + 1024, 1024, 0]
        for _ in range(4):   # as a batcher lane does: the stage the header names grows to its total
            self.alloc(tuple(caps))
            self.publish()
            torch.cuda.synchronize(dev)
            h = [int(x) for x in self.hdr.cpu()]
            if h[6] == 0:
                break
            caps[h[6] - 1] = {1: h[4], 2: h[0], 3: h[1]}[h[6]] + 1024
        assert h[6] == 0, "the sizing runs did not fit: %s" % h
        self.alloc(tuple(int(x * 1.25) + 1024 for x in (h[4], h[0], h[1])) + (0,))
        self.publish()
        torch.cuda.synchronize(dev)
        h = [int(x) for x in self.hdr.cpu()]
        assert h[6] == 0
        self.D = h[2]
        # the same results as planes, for the read-back form (a dense record is a slot without holes)
        deliv = self.deliv.view(-1, 4)
        self.p_to, self.p_tg = deliv[: self.D, 0].contiguous(), deliv[: self.D, 1].contiguous()
        self.p_cnt = (self.doff[1:] - self.doff[:-1]).to(torch.int32).contiguous()
        self.p_tot = torch.tensor([self.D], **self.i64)
        self.b_hdr = torch.zeros(4, **self.i64)
        self.b_groups, self.b_pub = torch.empty(4, **self.i32), torch.empty(1, **self.i32)
        self.M = self.G = 0
        self.plan_readback()                         # sizes only
        torch.cuda.synchronize(dev)
        self.M, self.G, self.T = (int(x) for x in self.b_hdr[:3].cpu())
        self.b_groups, self.b_pub = torch.empty((self.G + 1) * 4, **self.i32), torch.empty(self.M + 1, **self.i32)
        # the stream form's outputs and workspace
        self.cap = self.caps[1]
        self.fws_bytes = e.forward_plan_stream_workspace_bytes(n, self.cap, self.cap)
        self.fws = torch.empty(self.fws_bytes // 8 + 1, **self.i64)
        self.s_hdr = torch.zeros(8, **self.i64)
        self.s_groups, self.s_pub = torch.empty((self.cap + 1) * 4, **self.i32), torch.empty(self.cap + 1, **self.i32)

    def alloc(self, caps):
        self.caps = caps
        n = self.n
        self.ws_bytes = self.e.publish_stream_workspace_bytes(n, self.nbytes, caps)
        assert self.ws_bytes > 0
        self.ws = torch.empty(self.ws_bytes // 8 + 1, **self.i64)
        self.hdr, self.doff, self.soff = (torch.zeros(k, **self.i64) for k in (8, n + 1, n + 1))
        self.deliv, self.pairs = torch.empty(caps[1] * 4, **self.i32), torch.empty(caps[2] * 2, **self.i32)

    def publish(self):
        self.e.publish_stream_device(self.d_b, self.d_o, self.n, self.nbytes, Engine.SHARE_KEYED, self.d_k, None,
                                     self.caps, self.ws, self.ws_bytes, self.hdr, self.doff, self.soff, self.deliv,
                                     self.pairs, stream=self.st)

    def plan_readback(self):
        self.e.forward_plan_device(self.n, self.p_cnt, self.doff, self.p_to, self.p_tg, self.D, self.p_tot, self.b_hdr,
                                   self.b_groups, self.G, self.b_pub, self.M, stream=self.st)

    def plan_stream(self):
        self.e.forward_plan_stream_device(self.n, self.hdr, self.doff, self.deliv, self.cap, self.fws, self.fws_bytes,
                                          self.s_hdr, self.s_groups, self.cap, self.s_pub, self.cap, stream=self.st)

    def equal(self):
        self.publish()
        self.plan_readback()
        self.plan_stream()
        torch.cuda.synchronize(self.dev)
        s = [int(x) for x in self.s_hdr.cpu()]
        b = [int(x) for x in self.b_hdr.cpu()]
        if s[6] != 0 or s[:4] != b:
            return False, "headers %s / %s" % (s, b)
        M, G = b[0], b[1]
        if not np.array_equal(u32(self.s_groups[: G * 4]), u32(self.b_groups[: G * 4])):
            return False, "groups"
        if not np.array_equal(u32(self.s_pub[:M]), u32(self.b_pub[:M])):
            return False, "pub"
        return True, "%d forwards, %d groups, %d nodes" % (M, G, b[2])

    def time(self, warmups=3, runs=10):
        sides = {"readback": self.plan_readback, "stream": self.plan_stream}
        out = {k: {"device_publish_ms": [], "device_plan_ms": [], "wall_ms": []} for k in sides}
        for it in range(warmups + runs):
            for name, plan in sides.items():
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                torch.cuda.synchronize(self.dev)
                t0 = time.perf_counter()
                ev[0].record(self.st)
                self.publish()
                ev[1].record(self.st)
                plan()
                ev[2].record(self.st)
                self.st.synchronize()
                wall = (time.perf_counter() - t0) * 1e3
                if it >= warmups:
                    out[name]["device_publish_ms"].append(ev[0].elapsed_time(ev[1]))
                    out[name]["device_plan_ms"].append(ev[1].elapsed_time(ev[2]))
                    out[name]["wall_ms"].append(wall)
        return {k: {m: float(np.median(v)) for m, v in d.items()} for k, d in out.items()}


def flood(e, tb, to, a):
    drv = ctypes.CDLL(os.path.join(ROOT, "tools", "ubench", "libfwddrive.so"))
    drv.tm_bench_forward_flood.restype = ctypes.c_int
    drv.tm_bench_forward_flood.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                           ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                           ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
    n = len(to) - 1
    lines = []
    for rnd in range(a.rounds):
        for mode, name in ((0, "publish_host_regroup"), (1, "forward")):
            res = (ctypes.c_double * 12)()
            rc = drv.tm_bench_forward_flood(e.h, tb.ctypes.data, to.ctypes.data, n, 16, 200, a.max_topics, 4, mode, res)
            line = {"side": name, "round": rnd, "rc": rc, "topics": n, "producers": 16, "lanes": 4, "deadline_us": 200,
                    "max_topics": a.max_topics, "secs": res[0], "topics_per_s": res[1], "batches": int(res[2]),
                    "mean_batch": res[3], "lat_us_p50": res[4], "lat_us_p99": res[5], "failed": int(res[6]),
                    "bundles": int(res[7]), "forwards": int(res[8]),
                    "per_batch": {"device_us": res[9], "callbacks_us": res[10]}, "reruns": int(res[11])}
            log(json.dumps(line))
            lines.append(line)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--filters", type=int, default=None)
    ap.add_argument("--topics", default="4096,32768,131072")
    ap.add_argument("--remotes", type=int, nargs="+", default=[4, 64])
    ap.add_argument("--flood-topics", type=int, default=1_048_576)   # 262,144 topics are through in a few ms
    ap.add_argument("--max-topics", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forward_stream", "bench_forward_stream.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    nf = a.filters or W.CONFIGS[a.config]["filters"]
    sizes_n = [int(x) for x in a.topics.split(",")]
    rng = np.random.default_rng(17)
    fb, fo = W.filters(a.config, n=nf)
    tb, to = W.topics(a.config, n=max(max(sizes_n), a.flood_topics))
    keys = rng.integers(0, 2 ** 32, size=len(to) - 1, dtype=np.uint64).astype(np.uint32)
    runs = {}
    for remotes in a.remotes:
        t0 = time.time()
        e, _owner, _ids = build_engine(fb, fo, nf, remotes)
        log("%d remote nodes: %d filters, built in %.1fs" % (remotes, nf, time.time() - t0))
        per_size = []
        for n in sizes_n:
            bt = Batch(e, tb, to, n, keys, dev, st)
            ok, what = bt.equal()
            log("R = %d, n = %d: stream plan equals the read-back plan: %s (%s)" % (remotes, n, ok, what))
            if not ok:
                raise SystemExit("the two plans differ: " + what)
            ms = bt.time()
            row = {"topics": n, "deliveries": bt.D, "forwards": bt.M, "groups": bt.G, "targets": bt.T,
                   "caps": {"deliv": bt.cap, "pub": bt.cap, "group": bt.cap},
                   "pub_cap_over_M": bt.cap / bt.M if bt.M else None, "ms_median": ms,
                   "stream_over_readback": {m: ms["stream"][m] / ms["readback"][m] if ms["readback"][m] > 0 else None
                                            for m in ("device_plan_ms", "wall_ms")}}
            log(json.dumps(row))
            per_size.append(row)
            del bt
            torch.cuda.empty_cache()
        lines = flood(e, tb, to[: a.flood_topics + 1], a) if a.flood_topics else []
        runs["remotes_%d" % remotes] = {"plan_after_publish": per_size, "batcher_flood": lines}
        e.close()
    out = {"workload": "C%d: %d filters, one route each over node() and R remote nodes, no subscribers" % (a.config, nf),
           "method": "(a) HIP events and wall clock per batch, 3 warm-ups, median of 10, the two chains interleaved; "
                     "(b) flood from 16 threads on 4 lanes, interleaved rounds",
           "runs": runs}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
