"""The inbox plan (inbox.hip) next to the publish call it follows, on one MI355X
in one process.

Setup: the dispatch bench's even layout (tools/bench_dispatch.py): the C2
filters (1M), one local-node route each, subscribers drawn so that the mean bag
holds 4 (about 4M subscribers), each with a random option word (QoS, no-local,
retain-as-published); every publish carries a QoS and a publisher drawn from
the subscriber ids, so a few pairs are dropped by no-local.  No $share sets:
the pick planes are all TM_NO_MEMBER, and the plan's pick passes run over them
and keep nothing.

Timed on the same 1M-topic HBM-resident batch, interleaved, HIP events around
each call, 3 warm-ups then the median of 10:
    publish     tm_match_publish_batch_opts_device alone
    pick_words  tm_share_pick_words_device alone over the planes left
    plan        tm_inbox_plan_device alone over the planes left (its one
                read-back and host wait included)
Next to it the regrouping the plan replaces, done on the host as a caller does
today: the pair planes read back, then a numpy stable argsort by subscriber id
and the gathers through it (read-back and regrouping timed apart, wall clock,
median of 3).  The host result must equal the plan.

Before anything is timed, the plan of the batch's first 20K topics is checked
against tests/inbox_ref.py over the planes read back.

Run: python tools/bench_inbox.py [--topics N --check K]
Writes profiles/inbox/bench_inbox.json and prints it."""
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
DROP = 8
PICK = 0x80000000


def log(*a):
    print("[inbox]", *a, file=sys.stderr, flush=True)


def build_engine(fb, fo, nf):
    e = Engine(device=0, filters_hint=nf)
    db = np.concatenate([np.tile(np.frombuffer(NODE, dtype=np.uint8), nf), np.zeros(8, dtype=np.uint8)])
    do = np.arange(nf + 1, dtype=np.uint64) * np.uint64(len(NODE))
    e.route_add_many(fb, fo, db, do)
    e.dest_target(NODE, Engine.TARGET_NODE, NODE)
    e.set_local_node(NODE)
    return e


def u32(t):
    return t.cpu().numpy().view(np.uint32)


class Batch:
    """the device buffers of the calls on the batch"""

    def __init__(self, e, tb, to, pf, fr, keys, dev, st):
        self.e, self.dev, self.st = e, dev, st
        self.n = n = len(to) - 1
        self.nbytes, self.off = int(to[-1]), to
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)   # noqa: E731
        self.d_b, self.d_o = torch.from_numpy(tb).to(dev), up(to, np.int64)
        self.d_pf, self.d_fr, self.d_k = up(pf, np.int32), up(fr, np.int32), up(keys, np.int32)
        i32 = dict(dtype=torch.int32, device=dev)
        i64 = dict(dtype=torch.int64, device=dev)
        self.c, self.o, self.tot = torch.empty(n, **i32), torch.empty(n + 1, **i64), torch.zeros(1, **i64)
        self.sc, self.so, self.stot = torch.empty(n, **i32), torch.empty(n + 1, **i64), torch.zeros(1, **i64)
        e.match_deliveries_batch_device(self.d_b, self.d_o, n, self.nbytes, self.c, self.o, None, None, 0, self.tot,
                                        stream=st)
        torch.cuda.synchronize(dev)
        self.slots = int(self.tot.item())
        self.cap = self.slots + 1024
        self.to, self.tg, self.nd, self.pk, self.pw = (torch.empty(self.cap, **i32) for _ in range(5))
        self.scap = 0
        self.sto = self.sid = self.sw = None
        self.publish()                                   # sizes only
        torch.cuda.synchronize(dev)
        self.pairs = int(self.stot.item())
        self.scap = self.pairs + 1024
        self.sto, self.sid, self.sw = (torch.empty(self.scap, **i32) for _ in range(3))
        self.hdr = torch.zeros(4, **i64)
        self.inbox = self.ent = None
        self.E = self.S = 0

    def publish(self, n=None):
        nbytes = self.nbytes if n is None else int(self.off[n])
        self.e.match_publish_batch_device(self.d_b, self.d_o, self.n if n is None else n, nbytes, self.c, self.o,
                                          self.to, self.tg, self.nd, self.cap, self.tot, self.sc, self.so, self.sto,
                                          self.sid, self.scap, self.stot, Engine.SHARE_KEYED, self.d_k, self.pk,
                                          stream=self.st, deliver=(self.d_pf, self.d_fr, 0, self.sw))

    def pick_words(self, n=None):
        self.e.share_pick_words_device(self.d_b, self.d_o, self.n if n is None else n, self.c, self.o, self.to,
                                       self.tg, self.pk, self.cap, self.tot, (self.d_pf, self.d_fr, 0), self.pw,
                                       stream=self.st)

    def plan(self, n=None, sized=True):
        ic, ec = (self.S, self.E) if sized else (0, 0)
        g = lambda t: t if sized else None   # noqa: E731
        ent = self.ent or (None, None, None)
        self.e.inbox_plan_device(self.n if n is None else n, self.so, self.sto, self.sid, self.sw, self.scap,
                                 self.stot, self.c, self.o, self.to, self.pk, self.pw, self.cap, self.tot, self.hdr,
                                 g(self.inbox), ic, g(ent[0]), g(ent[1]), g(ent[2]), ec, stream=self.st)

    def size_plan(self, n=None):
        """a first call with no capacity reports E and S; the arrays are made to fit"""
        self.plan(n, sized=False)
        torch.cuda.synchronize(self.dev)
        self.E, self.S = int(self.hdr[0].item()), int(self.hdr[1].item())
        i32 = dict(dtype=torch.int32, device=self.dev)
        self.inbox = torch.empty((self.S + 1) * 4, **i32)
        self.ent = tuple(torch.empty(self.E + 1, **i32) for _ in range(3))

    def time(self, warmups=3, runs=10):
        """median ms of each call, interleaved, HIP events on the stream"""
        fns = {"publish": self.publish, "pick_words": self.pick_words, "plan": self.plan}
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

    def host_regroup(self, runs=3):
        """what a caller does today: the pair planes read back and regrouped by
        subscriber with a stable argsort (this setup has no pick sends)"""
        rb, srt, res = [], [], None
        for _ in range(runs):
            torch.cuda.synchronize(self.dev)
            t0 = time.perf_counter()
            soff = self.so.cpu().numpy()
            sid, sto, sw = (u32(x[: self.pairs]) for x in (self.sid, self.sto, self.sw))
            t1 = time.perf_counter()
            pub = np.repeat(np.arange(self.n, dtype=np.uint32), np.diff(soff))
            keep = np.nonzero(sw != DROP)[0]
            order = keep[np.argsort(sid[keep], kind="stable")]
            subs = sid[order]
            head = np.ones(len(order), dtype=bool)
            head[1:] = subs[1:] != subs[:-1]
            first = np.nonzero(head)[0]
            res = (subs[first], first, pub[order], sto[order], sw[order])
            t2 = time.perf_counter()
            rb.append((t1 - t0) * 1e3)
            srt.append((t2 - t1) * 1e3)
        return float(np.median(rb)), float(np.median(srt)), res


def parity(bt, k):
    """the plan of the batch's first k topics against inbox_ref over the planes read back"""
    from inbox_ref import expected_plan, sends_of_planes
    bt.publish(k)
    bt.pick_words(k)
    bt.size_plan(k)
    bt.plan(k)
    torch.cuda.synchronize(bt.dev)
    soff, off = bt.so[: k + 1].cpu().numpy().view(np.uint64), bt.o[: k + 1].cpu().numpy().view(np.uint64)
    p, s = int(bt.stot.item()), int(bt.tot.item())
    want = expected_plan(sends_of_planes(soff, u32(bt.sto[:p]), u32(bt.sid[:p]), u32(bt.sw[:p]), u32(bt.c[:k]), off,
                                         u32(bt.to[:s]), u32(bt.pk[:s]), u32(bt.pw[:s])))
    hdr = [int(x) for x in bt.hdr.cpu()]
    if hdr != want[0]:
        return False, "header %s, model %s" % (hdr, want[0])
    if [tuple(r) for r in u32(bt.inbox[: hdr[1] * 4]).reshape(-1, 4).tolist()] != want[1]:
        return False, "inbox records"
    for i, what in enumerate(("ent_pub", "ent_to", "ent_word")):
        if u32(bt.ent[i][: hdr[0]]).tolist() != want[2 + i]:
            return False, what
    return True, "%d topics, %d sends, %d subscribers, %d pairs dropped" % (k, hdr[0], hdr[1], p - hdr[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--filters", type=int, default=None)
    ap.add_argument("--topics", type=int, default=1_000_000)
    ap.add_argument("--mean-bag", type=int, default=4)
    ap.add_argument("--check", type=int, default=20_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inbox", "bench_inbox.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)   # a stream of the caller's, so that its events bracket the calls
    nf = a.filters or W.CONFIGS[a.config]["filters"]
    rng = np.random.default_rng(17)
    fb, fo = W.filters(a.config, n=nf)
    tb, to = W.topics(a.config, n=a.topics)
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
    n = len(to) - 1
    pf = rng.integers(0, 3, size=n).astype(np.uint32)
    fr = rng.integers(0, n_subs, size=n).astype(np.uint32)
    keys = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    bt = Batch(e, tb, to, pf, fr, keys, dev, st)
    check = None
    if a.check:
        ok, what = parity(bt, min(a.check, bt.n))
        log("parity vs inbox_ref:", ok, what)
        check = {"ok": ok, "what": what}
        if not ok:
            raise SystemExit("parity failed: " + what)
    bt.publish()
    bt.pick_words()
    bt.size_plan()
    ms, spread = bt.time()
    torch.cuda.synchronize(dev)
    hdr = [int(x) for x in bt.hdr.cpu()]
    rb_ms, sort_ms, host = bt.host_regroup()
    inbox = u32(bt.inbox[: bt.S * 4]).reshape(-1, 4)
    same = (hdr[3] == 0 and len(host[0]) == bt.S and len(host[2]) == bt.E and
            np.array_equal(host[0], inbox[:, 0]) and np.array_equal(host[1], inbox[:, 1]) and
            np.array_equal(host[2], u32(bt.ent[0][: bt.E])) and np.array_equal(host[3], u32(bt.ent[1][: bt.E])) and
            np.array_equal(host[4], u32(bt.ent[2][: bt.E])))
    log("host regroup equals the plan:", same)
    if not same:
        raise SystemExit("the host regrouping and the plan differ")
    top = int(inbox[-1, 0]) if bt.S else 0
    passes = max(1, (top.bit_length() + 7) // 8)
    # HBM bytes the passes move per pair and per send, by reading inbox.hip (the sort's passes apart):
    # flag 12 + scan 12 per pair; emit 20 read + 24 written, gather 24 read + 20 written, head / pick scans 24,
    # records 8 per send
    model = {"per_pair_flag_scan": 24, "per_send_emit_gather_records": 120,
             "per_send_per_sort_pass": 24, "sort_passes": passes}
    moved = bt.pairs * 24 + bt.E * (120 + 24 * passes)
    out = {"workload": "C%d: %d filters, one local route each, %d subscribers with option words; %d-topic batch" % (
               a.config, nf, n_subs, a.topics),
           "method": "HIP events around each call, 3 warm-ups, median of 10, the three calls interleaved; "
                     "host baseline wall clock, median of 3",
           "delivery_slots": bt.slots, "pairs": bt.pairs, "sends": bt.E, "subscribers_reached": bt.S,
           "pairs_dropped": bt.pairs - hdr[2], "largest_subscriber_id": top,
           "ms_median": ms, "ms_min_max": spread,
           "plan_over_publish": ms["plan"] / ms["publish"] if ms["publish"] > 0 else None,
           "ns_per_send": ms["plan"] * 1e6 / bt.E if bt.E else None,
           "bytes_model": model, "bytes_moved_model": moved, "bytes_per_send_model": moved / bt.E if bt.E else None,
           "plan_TB_s_model": moved / (ms["plan"] * 1e-3) / 1e12 if ms["plan"] > 0 else None,
           "host_baseline_ms": {"read_back": rb_ms, "regroup_argsort": sort_ms, "total": rb_ms + sort_ms},
           "host_over_plan": (rb_ms + sort_ms) / ms["plan"] if ms["plan"] > 0 else None,
           "host_regroup_over_plan": sort_ms / ms["plan"] if ms["plan"] > 0 else None,
           "host_equals_plan": bool(same), "check": check}
    e.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
