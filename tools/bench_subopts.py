"""The per-pair delivery word (dispatch.hip tm_dispatch_emit_opts) next to the
plain dispatch call it extends, on one MI355X in one process.

Setup as tools/bench_dispatch.py: the C2 filters (1M), one local-node route
each, 4.0M subscribers in the EVEN layout (mean bag 4) and the same total on 16
filters in the SKEW layout (250,000 per bag); a 1M-topic HBM-resident batch;
HIP events on the caller's stream, 3 warm-ups, median of 10.

Two legs interleaved, plus each one's count-only form (sub_cap 0):
    plain   tm_match_dispatch_batch_device
    opts    tm_match_dispatch_batch_opts_device: every subscriber carries an
            option word, every publish its own (qos, retain, retained), and 1 %
            of the publishes come from a subscriber of their own pairs
emit = call - count-only; the opts emit's bytes are counted as 20 B per pair
(pool id, option word, sub_to, sub_id, sub_deliver) plus 20 B per delivery slot
(prefix, segment, To, publish index) and stand next to the device copy ceiling
of profiles/r06_k/copy_ceiling.json.

Before anything is timed, 20K topics are checked: the pairs against
tests/dispatch_ref.py (bench_dispatch.parity) and every pair's word against
tests/subopts_ref.py run_dispatch_steps.

One host baseline, the alternative this replaces and NOT a tuned CPU path: the
pairs of a 20K-topic sample read back, then one option lookup per pair through
a numpy table (vectorised) and through a Python dict.

--plain-only [--lib L]: only the even layout, subscribers without options,
only the plain leg, one JSON line: the A/B of the plain call across builds.

Run: python tools/bench_subopts.py [--topics N --check K]
Writes profiles/subopts/bench_subopts.json (--out) and prints it."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def log(*a):
    print("[subopts]", *a, file=sys.stderr, flush=True)


def word_of(ids):
    """the option word of subscriber id: qos id % 3, no-local, rap on every other pair of ids, a subid"""
    ids = np.asarray(ids, dtype=np.uint64)
    return ((ids % 3) | 4 | (((ids >> 1) & 1) << 3) | ((ids % 1000 + 1) << 4)).astype(np.uint32)


def deliver_np(opt, pf, same):
    """deliver.h over arrays (upgrade_qos off; every opt word is an entry)"""
    qos = np.minimum(opt & 3, pf & 3)
    retain = np.where(pf & 8, 1, np.where(opt & 8, (pf >> 2) & 1, 0)).astype(np.uint32)
    w = qos | (retain << 2) | (opt & np.uint32(0xFFFFFFF0))
    return np.where((opt & 4).astype(bool) & same, np.uint32(8), w).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--filters", type=int, default=None)
    ap.add_argument("--topics", type=int, default=1_000_000)
    ap.add_argument("--mean-bag", type=int, default=4)
    ap.add_argument("--skew-filters", type=int, default=16)
    ap.add_argument("--check", type=int, default=20_000)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--tag", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subopts", "bench_subopts.json"))
    a = ap.parse_args()
    if a.lib:
        from emqx_amd import _lib
        _lib.LIB_PATH = os.path.abspath(a.lib)
    import bench_dispatch as BD
    from emqx_amd import Engine
    from emqx_amd import workload as W
    from emqx_amd.engine import pack

    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    nf = a.filters or W.CONFIGS[a.config]["filters"]
    rng = np.random.default_rng(17)
    fb, fo = W.filters(a.config, n=nf)
    tb, to = W.topics(a.config, n=a.topics)
    filters = W.unpack(fb, fo)

    class Batch(BD.Batch):
        """bench_dispatch's buffers plus the delivery descriptor's"""

        def prepare(self):
            n = self.n
            self.dispatch()
            torch.cuda.synchronize(self.dev)
            pf = rng.integers(0, 3, size=n).astype(np.uint32) | (rng.integers(0, 2, size=n).astype(np.uint32) << 2) \
                | ((rng.random(n) < 0.1).astype(np.uint32) << 3)
            fr = np.full(n, Engine.NO_SUBSCRIBER, dtype=np.uint32)
            so = self.so.cpu().numpy()
            sc = self.sc.cpu().numpy()
            sid = self.sid[: self.pairs].cpu().numpy().view(np.uint32)
            own = np.nonzero((rng.random(n) < 0.01) & (sc > 0))[0]      # 1 %: a subscriber of its own pairs
            fr[own] = sid[so[own] + (rng.integers(0, 1 << 30, size=len(own)) % sc[own])]
            self.pf, self.fr = pf, fr
            self.d_pf = torch.from_numpy(pf.view(np.int32)).to(self.dev)
            self.d_fr = torch.from_numpy(fr.view(np.int32)).to(self.dev)
            self.sdv = torch.empty(self.scap, dtype=torch.int32, device=self.dev)

        def opts(self, scap=None):
            scap = self.scap if scap is None else scap
            self.e.match_dispatch_batch_device(self.d_b, self.d_o, self.n, self.nbytes, self.c, self.o, self.to, self.tg,
                                               self.nd, self.cap, self.tot, self.sc, self.so,
                                               self.sto if scap else None, self.sid if scap else None, scap, self.stot,
                                               stream=self.st, deliver=(self.d_pf, self.d_fr, 0, self.sdv))

        def time(self, legs, warmups=3, runs=10):
            ms = {k: [] for k in legs}
            for it in range(warmups + runs):
                for name, fn in legs.items():
                    x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize(self.dev)
                    x.record(self.st)
                    fn()
                    y.record(self.st)
                    torch.cuda.synchronize(self.dev)
                    if it >= warmups:
                        ms[name].append(x.elapsed_time(y))
            return {k: float(np.median(v)) for k, v in ms.items()}, {k: [min(v), max(v)] for k, v in ms.items()}

        def legs(self):
            return {"plain": self.dispatch, "opts": self.opts, "plain_count_only": lambda: self.dispatch(0),
                    "opts_count_only": lambda: self.opts(0)}

    def check_words(bt, k):
        """every pair's word of the first k topics against subopts_ref.run_dispatch_steps"""
        from subopts_ref import run_dispatch_steps
        soff = bt.so[: k + 1].cpu().numpy()
        hi = int(soff[k])
        sid = bt.sid[:hi].cpu().numpy().view(np.uint32)
        sdv = bt.sdv[:hi].cpu().numpy().view(np.uint32)
        ow = word_of(sid)
        shown = set()
        for t in range(k):
            pfw, frm = int(bt.pf[t]), int(bt.fr[t])
            msg = (pfw & 3, (pfw >> 2) & 1, (pfw >> 3) & 1, None if frm == Engine.NO_SUBSCRIBER else frm)
            for j in range(int(soff[t]), int(soff[t + 1])):
                w, s = int(ow[j]), int(sid[j])
                opts = {"qos": w & 3, "nl": (w >> 2) & 1, "rap": (w >> 3) & 1, "subid": w >> 4}
                want = run_dispatch_steps(opts, msg, msg[3] is not None and s == msg[3], False)
                got = int(sdv[j])
                g = None if got & 8 else (got & 3, (got >> 2) & 1, (got >> 4) or None)
                if g != want:
                    return False, "word of pair %d (topic %d): %r, want %r" % (j, t, g, want)
                shown.add("dropped" if want is None else "kept")
        return True, "%d topics, %d words, outcomes %s" % (k, hi, sorted(shown))

    def host_baseline(bt, k):
        """read the sample's pairs back and look every one up on the host"""
        soff = bt.so[: k + 1].cpu().numpy()
        hi = int(soff[k])
        table = word_of(np.arange(n_subs))
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        sid = bt.sid[:hi].cpu().numpy().view(np.uint32)
        t1 = time.perf_counter()
        pub = np.repeat(np.arange(k), np.diff(soff).astype(np.int64))
        w = deliver_np(table[sid], bt.pf[pub], sid == bt.fr[pub])
        t2 = time.perf_counter()
        d = {int(s): int(x) for s, x in enumerate(table)}           # the caller's map, built outside the clock
        t3 = time.perf_counter()
        m = min(hi, 1_000_000)
        out = [d[int(s)] for s in sid[:m]]
        t4 = time.perf_counter()
        dev_w = bt.sdv[:hi].cpu().numpy().view(np.uint32)
        return {"label": "the alternative being replaced, not a tuned CPU path", "topics": k, "pairs": hi,
                "readback_ms": (t1 - t0) * 1e3, "numpy_table_and_word_ms": (t2 - t1) * 1e3,
                "numpy_ns_per_pair": (t2 - t0) * 1e9 / max(hi, 1),
                "python_dict_lookup_pairs": m, "python_dict_lookup_ms": (t4 - t3) * 1e3,
                "python_dict_ns_per_pair": (t4 - t3) * 1e9 / max(m, 1),
                "agrees_with_device": bool(np.array_equal(w, dev_w)) and len(out) == m}

    # ---- even layout
    t0 = time.time()
    e = BD.build_engine(fb, fo, nf)
    sizes = rng.integers(1, 2 * a.mean_bag, size=nf)
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    for k in range(int(sizes.max())):
        idx = np.nonzero(sizes > k)[0]
        sb, so = pack([filters[i] for i in idx])
        ids = (start[idx] + k).astype(np.uint32)
        if a.plain_only:
            e.sub_add_many(sb, so, ids)
        else:
            e.sub_add_opts_many(sb, so, ids, word_of(ids))
    e.commit()
    n_subs = int(e.sub_count)
    log("even: %d filters, %d subscribers, built in %.1fs" % (nf, n_subs, time.time() - t0))
    even = Batch(e, tb, to, dev, st)
    if a.plain_only:
        ms, spread = even.time({"plain": even.dispatch, "plain_count_only": lambda: even.dispatch(0)})
        print(json.dumps({"tag": a.tag, "lib": a.lib or "in-tree", "pairs": even.pairs, "ms_median": ms,
                          "ms_min_max": spread}), flush=True)
        e.close()
        return
    even.prepare()
    check = None
    if a.check:
        k = min(a.check, even.n)
        even.opts()
        torch.cuda.synchronize(dev)
        ok, what = BD.parity(e, even, fb, fo, nf, tb, to, lambda f: list(range(int(start[f]), int(start[f + 1]))), k)
        log("pairs vs dispatch_ref:", ok, what)
        ok2, what2 = check_words(even, k)
        log("words vs subopts_ref:", ok2, what2)
        ok2 = ok2 and "dropped" in what2          # the sample must show a no-local drop
        check = {"pairs_ok": ok, "pairs": what, "words_ok": ok2, "words": what2}
        if not (ok and ok2):
            raise SystemExit("check failed: %s / %s" % (what, what2))
    even_ms, even_spread = even.time(even.legs())
    even.opts()
    torch.cuda.synchronize(dev)
    baseline = host_baseline(even, min(a.check or 20_000, even.n))
    slots_even = even.cap - 1024
    tos = even.to[:slots_even]
    hits = torch.bincount(tos[tos >= 0].to(torch.int64), minlength=nf).cpu().numpy()[:nf]
    pairs_even = even.pairs
    e.close()
    del even

    # ---- skew layout: the same subscribers on 16 filters (bench_dispatch's choice of filters)
    per = n_subs // a.skew_filters
    target = pairs_even / per
    order = np.argsort(hits, kind="stable")
    order = order[hits[order] > 0]
    cs = np.concatenate([[0], np.cumsum(hits[order])])
    win = cs[a.skew_filters:] - cs[:-a.skew_filters]
    w0 = int(np.argmin(np.abs(win - target)))
    chosen = order[w0:w0 + a.skew_filters]
    t0 = time.time()
    e2 = BD.build_engine(fb, fo, nf)
    for j, f in enumerate(chosen):
        sb, so = pack([filters[int(f)]] * per)
        ids = (np.arange(per) + j * per).astype(np.uint32)
        e2.sub_add_opts_many(sb, so, ids, word_of(ids))
    e2.commit()
    log("skew: %d subscribers on %d filters, built in %.1fs" % (e2.sub_count, len(chosen), time.time() - t0))
    skew = Batch(e2, tb, to, dev, st)
    skew.prepare()
    if a.check:
        skew.opts()
        torch.cuda.synchronize(dev)
        ok, what = check_words(skew, min(2000, skew.n))
        log("skew words vs subopts_ref:", ok, what)
        check["skew_words_ok"] = ok
        if not ok:
            raise SystemExit("skew check failed: " + what)
    skew_ms, skew_spread = skew.time(skew.legs())
    pairs_skew = skew.pairs
    e2.close()

    with open(os.path.join(ROOT, "profiles", "r06_k", "copy_ceiling.json")) as f:
        ceiling = json.load(f)["copy_"]["TB_s"]

    def layout(ms, spread, pairs, slots):
        emit_p = ms["plain"] - ms["plain_count_only"]
        emit_o = ms["opts"] - ms["opts_count_only"]
        eb_p, eb_o = pairs * 12 + slots * 16, pairs * 20 + slots * 20
        return {"ms_median": ms, "ms_min_max": spread, "pairs": pairs, "delivery_slots": slots,
                "added_ms_per_batch": ms["opts"] - ms["plain"],
                "added_count_pass_ms": ms["opts_count_only"] - ms["plain_count_only"],
                "emit_plain_ms": emit_p, "emit_opts_ms": emit_o,
                "emit_opts_over_plain": emit_o / emit_p if emit_p > 0 else None,
                "emit_bytes_predicted_ratio": eb_o / eb_p,
                "emit_plain_bytes": eb_p, "emit_opts_bytes": eb_o,
                "emit_plain_TB_s": eb_p / (emit_p * 1e-3) / 1e12 if emit_p > 0 else None,
                "emit_opts_TB_s": eb_o / (emit_o * 1e-3) / 1e12 if emit_o > 0 else None,
                "emit_opts_fraction_of_copy_ceiling": eb_o / (emit_o * 1e-3) / 1e12 / ceiling if emit_o > 0 else None}
    out = {"workload": "C%d: %d filters, one local route each, %d subscribers, each with an option word; %d-topic "
                       "batch, 1 %% of the publishes from a subscriber of their own pairs" % (a.config, nf, n_subs,
                                                                                             a.topics),
           "method": "HIP events around each call on the caller's stream, 3 warm-ups, median of 10, the four calls "
                     "interleaved; emit = call - its count-only form (sub_cap 0)",
           "even": layout(even_ms, even_spread, pairs_even, slots_even),
           "skew": layout(skew_ms, skew_spread, pairs_skew, slots_even),
           "copy_ceiling_TB_s": ceiling, "host_baseline_even": baseline, "check": check}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
