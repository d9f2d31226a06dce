"""Python handle on one libtopicmatch engine (one engine per GPU).

Thin wrapper over the C-ABI: numpy arrays for host batches, torch tensors
(or raw device pointers) for HBM-resident batches.  No matching logic lives
here; every match runs in the HIP kernels of emqx_amd/csrc/kernels.hip.
"""
import ctypes

import numpy as np

from . import _lib as L


def pack(strings):
    """Concatenate byte strings -> (bytes ndarray u8, offsets ndarray u64)."""
    bs = [s if isinstance(s, (bytes, bytearray)) else s.encode() for s in strings]
    off = np.zeros(len(bs) + 1, dtype=np.uint64)
    if bs:
        off[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
    buf = np.frombuffer(b"".join(bs) + b"\0" * 8, dtype=np.uint8)
    return buf, off


def check_total(d_total, cap, what="match"):
    """the exact total a two-pass device call wrote (a 1-element device tensor
    whose stream the caller has synchronised) against the capacity of the
    output it sized from the first pass: the device API drops ids past cap and
    reports the exact total, so a total past cap means lists were cut (e.g. a
    first-pass total overwritten by a late fill) -- raise instead of
    returning them"""
    total = int(d_total.item()) if hasattr(d_total, "item") else int(d_total)
    if total > cap:
        raise RuntimeError("%s: %d ids past an output of %d (lists would be cut)" % (what, total, cap))
    return total


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


class Engine:
    """One subscription trie + its HBM image on `device` (-1 = host-only:
    insert/delete/lookup work, matching raises TM_EDEVICE)."""

    def __init__(self, device=0, filters_hint=0, batch_topics=0, batch_bytes=0, devices=None):
        """devices: a list of HIP ordinals opens one engine with a replica on
        each (tm_open_devices; host batches are cut across them)"""
        self.lib = L.load()
        cfg = L.TmConfig(device, 0, filters_hint, batch_topics, batch_bytes)
        h = ctypes.c_void_p()
        if devices is not None:
            arr = (ctypes.c_int32 * max(len(devices), 1))(*devices)
            rc = self.lib.tm_open_devices(ctypes.byref(cfg), arr, len(devices), ctypes.byref(h))
            what = "tm_open_devices(%s)" % list(devices)
            device = devices[0] if devices else -1
        else:
            rc = self.lib.tm_open(ctypes.byref(cfg), ctypes.byref(h))
            what = "tm_open(device=%d)" % device
        if rc != L.TM_OK:
            raise L.TopicMatchError(rc, what)
        self.h = h
        self.device = device

    @property
    def replicas(self):
        return self.lib.tm_engine_replicas(self.h)

    # -- lifetime ---------------------------------------------------------
    def close(self):
        if self.h:
            self.lib.tm_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != L.TM_OK:
            raise L.TopicMatchError(rc, "%s: %s" % (what, self.lib.tm_last_error(self.h).decode()))
        return rc

    # -- emqx_trie:insert/1, delete/1, lookup/1 ---------------------------
    def insert(self, filt: bytes):
        return self._check(self.lib.tm_insert(self.h, filt, len(filt)), "tm_insert")

    def insert_many(self, buf, off):
        n = len(off) - 1
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        return self._check(self.lib.tm_insert_batch(self.h, _ptr(buf), _ptr(off), n), "tm_insert_batch")

    def insert_many_ids(self, buf, off, ids):
        """tm_insert_batch_ids: filter i under the caller's (global) id ids[i]"""
        n = len(off) - 1
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        return self._check(self.lib.tm_insert_batch_ids(self.h, _ptr(buf), _ptr(off), n, _ptr(ids)),
                           "tm_insert_batch_ids")

    def delete(self, filt: bytes):
        return self._check(self.lib.tm_delete(self.h, filt, len(filt)), "tm_delete")

    def delete_many(self, buf, off):
        n = len(off) - 1
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        return self._check(self.lib.tm_delete_batch(self.h, _ptr(buf), _ptr(off), n), "tm_delete_batch")

    def lookup(self, node_id: bytes):
        """[] or [(edge_count, topic_bytes_or_None)] like emqx_trie:lookup/1"""
        info = L.TmNodeInfo()
        rc = self.lib.tm_lookup(self.h, node_id, len(node_id), ctypes.byref(info))
        if rc == L.TM_ENOENT:
            return []
        self._check(rc, "tm_lookup")
        topic = None if info.filter_id == L.TM_NO_FILTER else self.filter_bytes(info.filter_id)
        return [(info.edge_count, topic)]

    def lease(self):
        """a filter id lease (tm_lease_begin/end), as a context manager: ids
        returned by matches inside it keep naming their filters (a deleted
        filter's id is not reused, its bytes stay gatherable) until it ends"""
        eng = self

        class _Lease:
            def __enter__(self):
                x = ctypes.c_uint64()
                eng._check(eng.lib.tm_lease_begin(eng.h, ctypes.byref(x)), "tm_lease_begin")
                self.x = x.value
                return self

            def __exit__(self, *a):
                eng.lib.tm_lease_end(eng.h, self.x)
        return _Lease()

    def commit(self):
        ep = ctypes.c_uint64()
        self._check(self.lib.tm_commit(self.h, ctypes.byref(ep)), "tm_commit")
        return ep.value

    def filter_bytes(self, fid: int) -> bytes:
        n = ctypes.c_uint32()
        p = self.lib.tm_filter_bytes(self.h, fid, ctypes.byref(n))
        if not p:
            raise KeyError(fid)
        return ctypes.string_at(p, n.value)

    @property
    def filter_count(self):
        return self.lib.tm_filter_count(self.h)

    @property
    def node_count(self):
        return self.lib.tm_node_count(self.h)

    @property
    def image_bytes(self):
        return self.lib.tm_image_bytes(self.h)

    # -- emqx_trie:match/1 over a batch ------------------------------------
    def match_batch(self, buf, off, out_cap=None, counts=None, offs=None, keep=False):
        """Host batch -> (counts u32[n], offsets u64[n+1], filter ids u32[total]).
        counts / offs: caller arrays to fill (e.g. pinned); keep=True returns
        the ids as a view of the library's pinned output buffer, released
        when the array is garbage-collected (no copy)."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = len(off) - 1
        counts = np.zeros(max(n, 1), dtype=np.uint32) if counts is None else counts
        offs = np.zeros(n + 1, dtype=np.uint64) if offs is None else offs
        if out_cap is None:   # library-sized output: one walk, no retry (tm_match_batch_owned)
            p, total = ctypes.c_void_p(), ctypes.c_uint64()
            rc = self.lib.tm_match_batch_owned(self.h, _ptr(buf), _ptr(off), n, _ptr(counts), _ptr(offs),
                                               ctypes.byref(p), ctypes.byref(total))
            if rc != L.TM_OK:
                self.lib.tm_free(p)
                self._check(rc, "tm_match_batch_owned")
            k = int(total.value)
            ids = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint32)), shape=(max(k, 1),))
            if keep:
                import weakref
                view = ids[:k]
                weakref.finalize(view, self.lib.tm_free, ctypes.c_void_p(p.value))
                return counts[:n], offs, view
            try:
                return counts[:n], offs, ids[:k].copy()
            finally:
                self.lib.tm_free(p)
        ids = np.zeros(max(out_cap, 1), dtype=np.uint32)
        needed = ctypes.c_uint64()
        rc = self.lib.tm_match_batch(self.h, _ptr(buf), _ptr(off), n, _ptr(counts), _ptr(offs), _ptr(ids),
                                     out_cap, ctypes.byref(needed))
        self._check(rc, "tm_match_batch")
        return counts[:n], offs, ids[: int(needed.value)]

    def filters_bytes(self, ids):
        """bytes of many filter ids, copied under the engine lock (tm_filters_gather)"""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        n = len(ids)
        off = np.zeros(n + 1, dtype=np.uint64)
        cap = n * 48 + 64
        while True:
            buf = np.zeros(max(cap, 1), dtype=np.uint8)
            rc = self.lib.tm_filters_gather(self.h, _ptr(ids), n, _ptr(buf), cap, _ptr(off))
            if rc == L.TM_ENOSPC:
                cap = int(off[-1])
                continue
            self._check(rc, "tm_filters_gather")
            b = buf.tobytes()
            return [b[int(off[i]):int(off[i + 1])] for i in range(n)]

    def match(self, topics):
        """list of topics -> list of lists of filter bytes, reference order."""
        buf, off = pack(topics)
        counts, offs, ids = self.match_batch(buf, off)
        uniq, inv = np.unique(ids, return_inverse=True)
        names = self.filters_bytes(uniq)
        out = []
        for t in range(len(topics)):
            a, b = int(offs[t]), int(offs[t]) + int(counts[t])
            out.append([names[int(k)] for k in inv[a:b]])
        return out

    def match_batch_device(self, d_bytes, d_off, n, topic_bytes, d_counts, d_offs, d_ids, out_cap, d_total,
                           stream=None):
        """All arguments are device pointers (ints) or torch tensors; stream-
        ordered, no synchronisation."""
        def p(x):
            if x is None:
                return None
            if hasattr(x, "data_ptr"):
                return ctypes.c_void_p(x.data_ptr())
            return ctypes.c_void_p(int(x))
        st = None
        if stream is not None:
            st = ctypes.c_void_p(L.stream_handle(stream))
        rc = self.lib.tm_match_batch_device(self.h, p(d_bytes), p(d_off), n, topic_bytes, p(d_counts), p(d_offs),
                                            p(d_ids), out_cap, p(d_total), st)
        return self._check(rc, "tm_match_batch_device")

    def match_small_device(self, d_bytes, d_off, n, topic_bytes, d_counts, d_offs, d_ids, out_cap, d_total,
                           stream=None):
        """tm_match_small_device: the lists of a small batch in one launch;
        topic t's list is d_ids[d_offs[t] : d_offs[t] + d_counts[t]] (lists
        in completion order, d_offs has n entries)"""
        def p(x):
            if x is None:
                return None
            if hasattr(x, "data_ptr"):
                return ctypes.c_void_p(x.data_ptr())
            return ctypes.c_void_p(int(x))
        st = None if stream is None else ctypes.c_void_p(L.stream_handle(stream))
        rc = self.lib.tm_match_small_device(self.h, p(d_bytes), p(d_off), n, topic_bytes, p(d_counts), p(d_offs),
                                            p(d_ids), out_cap, p(d_total), st)
        return self._check(rc, "tm_match_small_device")

    # -- emqx_router: the route bag and match_routes/1 ----------------------
    TOPIC_ROUTE = 0xFFFFFFFF    # route source = the publish topic itself

    def route_add(self, topic: bytes, dest: bytes):
        return self._check(self.lib.tm_route_add(self.h, topic, len(topic), dest, len(dest)), "tm_route_add")

    def route_add_many(self, tbuf, toff, dbuf, doff):
        """route i = (topic i of (tbuf, toff), dest i of (dbuf, doff))"""
        n = len(toff) - 1
        tbuf = np.ascontiguousarray(tbuf, dtype=np.uint8)
        toff = np.ascontiguousarray(toff, dtype=np.uint64)
        dbuf = np.ascontiguousarray(dbuf, dtype=np.uint8)
        doff = np.ascontiguousarray(doff, dtype=np.uint64)
        return self._check(self.lib.tm_route_add_batch(self.h, _ptr(tbuf), _ptr(toff), _ptr(dbuf), _ptr(doff), n),
                           "tm_route_add_batch")

    def route_del(self, topic: bytes, dest: bytes):
        return self._check(self.lib.tm_route_del(self.h, topic, len(topic), dest, len(dest)), "tm_route_del")

    def route_del_many(self, tbuf, toff, dbuf, doff):
        """route i = (topic i of (tbuf, toff), dest i of (dbuf, doff)), removed in order"""
        n = len(toff) - 1
        tbuf = np.ascontiguousarray(tbuf, dtype=np.uint8)
        toff = np.ascontiguousarray(toff, dtype=np.uint64)
        dbuf = np.ascontiguousarray(dbuf, dtype=np.uint8)
        doff = np.ascontiguousarray(doff, dtype=np.uint64)
        return self._check(self.lib.tm_route_del_batch(self.h, _ptr(tbuf), _ptr(toff), _ptr(dbuf), _ptr(doff), n),
                           "tm_route_del_batch")

    # the emqx_route table events of the delta feed (route bag only, never
    # the trie: emqx_trie_gpu_feed.erl drives the trie from emqx_trie_node)
    def route_write(self, topic: bytes, dest: bytes):
        """mnesia:write(emqx_route, #route{}) (add_trie_route/1 :231, add_direct_route/1 :223-224)"""
        return self._check(self.lib.tm_route_write(self.h, topic, len(topic), dest, len(dest)), "tm_route_write")

    def route_delete_object(self, topic: bytes, dest: bytes):
        """mnesia:delete_object(emqx_route, #route{}) (del_trie_route/1 :255-258,
        emqx_router_helper:cleanup_routes/1 :156-160): the filter stays in the trie"""
        return self._check(self.lib.tm_route_delete_object(self.h, topic, len(topic), dest, len(dest)),
                           "tm_route_delete_object")

    def route_write_many(self, tbuf, toff, dbuf, doff):
        n = len(toff) - 1
        tbuf = np.ascontiguousarray(tbuf, dtype=np.uint8)
        toff = np.ascontiguousarray(toff, dtype=np.uint64)
        dbuf = np.ascontiguousarray(dbuf, dtype=np.uint8)
        doff = np.ascontiguousarray(doff, dtype=np.uint64)
        return self._check(self.lib.tm_route_write_batch(self.h, _ptr(tbuf), _ptr(toff), _ptr(dbuf), _ptr(doff), n),
                           "tm_route_write_batch")

    def get_routes(self, topic: bytes):
        """dest ids of topic's routes, insertion order (get_routes/1)"""
        n = ctypes.c_uint32()
        cap = 16
        while True:
            out = np.zeros(cap, dtype=np.uint32)
            rc = self.lib.tm_get_routes(self.h, topic, len(topic), out.ctypes.data, cap, ctypes.byref(n))
            if rc == L.TM_ENOSPC:
                cap = n.value
                continue
            self._check(rc, "tm_get_routes")
            return [int(x) for x in out[: n.value]]

    @property
    def route_count(self):
        return self.lib.tm_route_count(self.h)

    def dest_bytes(self, dest_id: int) -> bytes:
        n = ctypes.c_uint32()
        p = self.lib.tm_dest_bytes(self.h, dest_id, ctypes.byref(n))
        if not p:
            raise KeyError(dest_id)
        return ctypes.string_at(p, n.value)

    def match_routes_batch(self, buf, off, out_cap=None):
        """Host batch -> (counts u32[n], offsets u64[n+1], src u32[total],
        dest u32[total]): emqx_router:match_routes/1 per topic, src =
        TOPIC_ROUTE for the literal topic's routes, else the filter id."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = len(off) - 1
        counts = np.zeros(max(n, 1), dtype=np.uint32)
        offs = np.zeros(n + 1, dtype=np.uint64)
        cap = 1 << 16 if out_cap is None else out_cap
        while True:
            src = np.zeros(max(cap, 1), dtype=np.uint32)
            dst = np.zeros(max(cap, 1), dtype=np.uint32)
            needed = ctypes.c_uint64()
            rc = self.lib.tm_match_routes_batch(self.h, _ptr(buf), _ptr(off), n, _ptr(counts), _ptr(offs), _ptr(src),
                                                _ptr(dst), cap, ctypes.byref(needed))
            if rc == L.TM_ENOSPC and out_cap is None:
                cap = int(needed.value)
                continue
            self._check(rc, "tm_match_routes_batch")
            k = int(needed.value)
            return counts[:n], offs, src[:k], dst[:k]

    def match_routes_batch_device(self, d_bytes, d_off, n, topic_bytes, d_counts, d_offs, d_src, d_dest, out_cap,
                                  d_total, stream=None):
        def p(x):
            if x is None:
                return None
            return ctypes.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))
        st = None
        if stream is not None:
            st = ctypes.c_void_p(L.stream_handle(stream))
        rc = self.lib.tm_match_routes_batch_device(self.h, p(d_bytes), p(d_off), n, topic_bytes, p(d_counts),
                                                   p(d_offs), p(d_src), p(d_dest), out_cap, p(d_total), st)
        return self._check(rc, "tm_match_routes_batch_device")

    # -- emqx_broker:aggre/1 (aggre.hip) --------------------------------------
    TARGET_NODE, TARGET_GROUP = 0, 1

    def debug_check_routes(self):
        """host-side consistency check of the in-place route image (diagnostic,
        tm_debug_check_routes): raises TopicMatchError naming the first defect"""
        return self._check(self.lib.tm_debug_check_routes(self.h), "tm_debug_check_routes")

    def debug_check_device(self):
        """the live image of every replica read back and compared byte for byte
        with the host tables (diagnostic, tm_debug_check_device): raises
        TopicMatchError naming the first difference, or when deltas are
        uncommitted or no image is written yet"""
        self.lib.tm_debug_check_device.argtypes = [ctypes.c_void_p]
        return self._check(self.lib.tm_debug_check_device(self.h), "tm_debug_check_device")

    def debug_check_trie(self):
        """host-side check of the trie image (nodes, edge tables, Bloom masks,
        summaries, dictionary) against the logical trie (diagnostic,
        tm_debug_check_trie): raises TopicMatchError naming the first defect"""
        self.lib.tm_debug_check_trie.argtypes = [ctypes.c_void_p]
        return self._check(self.lib.tm_debug_check_trie(self.h), "tm_debug_check_trie")

    # the upload decisions tm_debug_commit_stats reports
    UP_NONE, UP_SCATTER, UP_SCATTER_TWO, UP_COPY = 0, 1, 2, 3

    def debug_commit_stats(self):
        """how the last commit uploaded each image table (diagnostic,
        tm_debug_commit_stats): {table name: (decision, elements scattered,
        table elements)}, decision one of UP_NONE / UP_SCATTER (that commit's
        log) / UP_SCATTER_TWO (that and the previous one's) / UP_COPY"""
        cap = 64
        out = (ctypes.c_uint64 * (3 * cap))()
        f, name = self.lib.tm_debug_commit_stats, self.lib.tm_debug_table_name
        f.restype, f.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
        name.restype, name.argtypes = ctypes.c_char_p, [ctypes.c_void_p, ctypes.c_uint32]
        n = f(self.h, out, cap)
        if n < 0:
            self._check(n, "tm_debug_commit_stats")
        return {name(self.h, k).decode(): (int(out[3 * k]), int(out[3 * k + 1]), int(out[3 * k + 2]))
                for k in range(n)}

    def dest_target(self, dest: bytes, kind: int, key: bytes) -> int:
        """declare dest's aggre target: a node atom (TARGET_NODE, key = its
        text) or a $share group (TARGET_GROUP, key = the group binary)"""
        t = ctypes.c_uint32()
        self._check(self.lib.tm_dest_target(self.h, dest, len(dest), kind, key, len(key), ctypes.byref(t)),
                    "tm_dest_target")
        return t.value

    def target_bytes(self, target_id: int):
        """target id -> (kind, key bytes)"""
        kind, n = ctypes.c_uint32(), ctypes.c_uint32()
        p = self.lib.tm_target_bytes(self.h, target_id, ctypes.byref(kind), ctypes.byref(n))
        if not p:
            raise KeyError(target_id)
        return kind.value, ctypes.string_at(p, n.value)

    def match_deliveries_batch(self, buf, off, out_cap=None):
        """Host batch -> (counts u32[n], offsets u64[n+1], to u32[total],
        target u32[total]): aggre(emqx_router:match_routes(T)) per topic; to =
        TOPIC_ROUTE for the literal topic, else the filter id."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = len(off) - 1
        counts = np.zeros(max(n, 1), dtype=np.uint32)
        offs = np.zeros(n + 1, dtype=np.uint64)
        cap = 1 << 16 if out_cap is None else out_cap
        while True:
            to = np.zeros(max(cap, 1), dtype=np.uint32)
            tg = np.zeros(max(cap, 1), dtype=np.uint32)
            needed = ctypes.c_uint64()
            rc = self.lib.tm_match_deliveries_batch(self.h, _ptr(buf), _ptr(off), n, _ptr(counts), _ptr(offs),
                                                    _ptr(to), _ptr(tg), cap, ctypes.byref(needed))
            if rc == L.TM_ENOSPC and out_cap is None:
                cap = int(needed.value)
                continue
            self._check(rc, "tm_match_deliveries_batch")
            k = int(needed.value)
            return counts[:n], offs, to[:k], tg[:k]

    def match_deliveries_batch_device(self, d_bytes, d_off, n, topic_bytes, d_counts, d_offs, d_to, d_target,
                                      out_cap, d_total, stream=None):
        def p(x):
            if x is None:
                return None
            return ctypes.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))
        st = None
        if stream is not None:
            st = ctypes.c_void_p(L.stream_handle(stream))
        rc = self.lib.tm_match_deliveries_batch_device(self.h, p(d_bytes), p(d_off), n, topic_bytes, p(d_counts),
                                                       p(d_offs), p(d_to), p(d_target), out_cap, p(d_total), st)
        return self._check(rc, "tm_match_deliveries_batch_device")

    # -- emqx_broker: the subscriber bag and the local dispatch (dispatch.hip) ---
    NO_GROUP = 0xFFFFFFFF     # group of a plain entry
    NOT_LOCAL = 0xFFFFFFFF    # ndisp of a delivery that is not the local node's

    def sub_add(self, topic: bytes, sub: int, group=None):
        """insert_subscriber/3: group None = undefined (a plain entry)"""
        return self._check(self.lib.tm_sub_add(self.h, topic, len(topic), sub, group, len(group) if group else 0),
                           "tm_sub_add")

    def sub_del(self, topic: bytes, sub: int, group=None) -> int:
        """ets:delete_object of {Topic, shared(Group, Sub)}; returns the entries left in the topic's bag"""
        left = ctypes.c_uint32()
        self._check(self.lib.tm_sub_del(self.h, topic, len(topic), sub, group, len(group) if group else 0,
                                        ctypes.byref(left)), "tm_sub_del")
        return left.value

    def _sub_many(self, fn, what, tbuf, toff, subs, gbuf, goff, shared):
        n = len(toff) - 1
        tbuf = np.ascontiguousarray(tbuf, dtype=np.uint8)
        toff = np.ascontiguousarray(toff, dtype=np.uint64)
        subs = np.ascontiguousarray(subs, dtype=np.uint32)
        if shared is not None:
            gbuf = np.ascontiguousarray(gbuf, dtype=np.uint8)
            goff = np.ascontiguousarray(goff, dtype=np.uint64)
            shared = np.ascontiguousarray(shared, dtype=np.uint8)
        else:
            gbuf = goff = None
        return self._check(fn(self.h, _ptr(tbuf), _ptr(toff), _ptr(subs), _ptr(gbuf), _ptr(goff), _ptr(shared), n),
                           what)

    def sub_add_many(self, tbuf, toff, subs, gbuf=None, goff=None, shared=None):
        """entry i = (topic i, subs[i]), shared with group i of (gbuf, goff) where shared[i]"""
        return self._sub_many(self.lib.tm_sub_add_batch, "tm_sub_add_batch", tbuf, toff, subs, gbuf, goff, shared)

    def sub_del_many(self, tbuf, toff, subs, gbuf=None, goff=None, shared=None):
        return self._sub_many(self.lib.tm_sub_del_batch, "tm_sub_del_batch", tbuf, toff, subs, gbuf, goff, shared)

    # -- emqx_suboption: one option word per (topic, subscriber) ------------------
    SUBOPT_NONE = L.TM_SUBOPT_NONE
    SUBOPT_NL = L.TM_SUBOPT_NL
    SUBOPT_RAP = L.TM_SUBOPT_RAP
    MSG_RETAIN = L.TM_MSG_RETAIN
    MSG_RETAINED = L.TM_MSG_RETAINED
    DELIVER_DROP = L.TM_DELIVER_DROP
    DELIVER_UPGRADE_QOS = L.TM_DELIVER_UPGRADE_QOS
    NO_SUBSCRIBER = L.TM_NO_SUBSCRIBER

    def sub_add_opts(self, topic: bytes, sub: int, opts: int, group=None):
        """do_subscribe/4: sub_add, then the option word of (topic, sub) is written
        (also when a plain entry suppressed the add)"""
        return self._check(self.lib.tm_sub_add_opts(self.h, topic, len(topic), sub, group, len(group) if group else 0,
                                                    opts), "tm_sub_add_opts")

    def sub_add_opts_many(self, tbuf, toff, subs, opts, gbuf=None, goff=None, shared=None):
        """sub_add_many with opts[i] for entry i"""
        opts = np.ascontiguousarray(opts, dtype=np.uint32)
        if len(opts) != len(toff) - 1:
            raise ValueError("opts: one u32 per entry")

        def fn(h, t, to, sb, g, go, sh, n):
            return self.lib.tm_sub_add_opts_batch(h, t, to, sb, g, go, sh, _ptr(opts), n)
        return self._sub_many(fn, "tm_sub_add_opts_batch", tbuf, toff, subs, gbuf, goff, shared)

    def sub_set_opts(self, topic: bytes, sub: int, mask: int, value: int) -> bool:
        """set_subopts/3: (old & ~mask) | (value & mask); False without an entry"""
        found = ctypes.c_int()
        self._check(self.lib.tm_sub_set_opts(self.h, topic, len(topic), sub, mask, value, ctypes.byref(found)),
                    "tm_sub_set_opts")
        return bool(found.value)

    def sub_get_opts(self, topic: bytes, sub: int):
        """get_subopts/2: the option word, None without an entry"""
        w, found = ctypes.c_uint32(), ctypes.c_int()
        self._check(self.lib.tm_sub_get_opts(self.h, topic, len(topic), sub, ctypes.byref(w), ctypes.byref(found)),
                    "tm_sub_get_opts")
        return int(w.value) if found.value else None

    def deliver_word(self, opts: int, pub_flags: int, same_client: bool, flags: int = 0) -> int:
        """tm_deliver_word: handle_dispatch/3 + run_dispatch_steps/3 for one pair"""
        return int(self.lib.tm_deliver_word(opts, pub_flags, 1 if same_client else 0, flags))

    @staticmethod
    def _host_deliver(deliver, n):
        """deliver=(pub_flags, pub_from | None, flags) -> (pub_flags, pub_from, flags) as u32 arrays"""
        pf, fr, fl = deliver
        pf = np.ascontiguousarray(pf, dtype=np.uint32)
        if len(pf) != n:
            raise ValueError("deliver: one pub_flags word per publish")
        if fr is not None:
            fr = np.ascontiguousarray(fr, dtype=np.uint32)
            if len(fr) != n:
                raise ValueError("deliver: one pub_from word per publish")
        return pf, fr, int(fl)

    @staticmethod
    def _deliver_struct(pf, fr, fl, out):
        return L.TmDeliver(pf, fr, fl, 0, out)

    def subscribers(self, topic: bytes):
        """subscribers/1: [(sub, group id or NO_GROUP)] in bag order"""
        n = ctypes.c_uint32()
        cap = 16
        while True:
            sub = np.zeros(cap, dtype=np.uint32)
            grp = np.zeros(cap, dtype=np.uint32)
            rc = self.lib.tm_subscribers(self.h, topic, len(topic), _ptr(sub), _ptr(grp), cap, ctypes.byref(n))
            if rc == L.TM_ENOSPC:
                cap = n.value
                continue
            self._check(rc, "tm_subscribers")
            return [(int(s), int(g)) for s, g in zip(sub[: n.value], grp[: n.value])]

    def sub_group_bytes(self, group_id: int) -> bytes:
        n = ctypes.c_uint32()
        p = self.lib.tm_sub_group_bytes(self.h, group_id, ctypes.byref(n))
        if not p:
            raise KeyError(group_id)
        return ctypes.string_at(p, n.value)

    @property
    def sub_count(self):
        return self.lib.tm_sub_count(self.h)

    def set_local_node(self, node: bytes):
        """the node() of route/2's Node =:= node() guard"""
        return self._check(self.lib.tm_set_local_node(self.h, node, len(node)), "tm_set_local_node")

    def debug_check_subs(self):
        """host-side consistency check of the in-place subscriber image
        (diagnostic, tm_debug_check_subs)"""
        self.lib.tm_debug_check_subs.argtypes = [ctypes.c_void_p]
        return self._check(self.lib.tm_debug_check_subs(self.h), "tm_debug_check_subs")

    def debug_sub_pool_stats(self):
        """(pool entries, garbage, compactions, segment moves, largest segment
        capacity) of the subscriber pool (diagnostic, tm_debug_sub_pool_stats)"""
        out = (ctypes.c_uint64 * 5)()
        self.lib.tm_debug_sub_pool_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self._check(self.lib.tm_debug_sub_pool_stats(self.h, out), "tm_debug_sub_pool_stats")
        return tuple(int(x) for x in out)

    def match_dispatch_batch(self, buf, off, out_cap=None, sub_cap=None, deliver=None):
        """Host batch -> (counts u32[n], offsets u64[n+1], to, target, ndisp
        (one per delivery slot), sub_count u32[n], sub_off u64[n+1], sub_to,
        sub_id): publish/1's deliveries with the local dispatch.  out_cap /
        sub_cap None: retried at the needed sizes; given: one call
        (TopicMatchError TM_ENOSPC when either is short).
        deliver=(pub_flags u32[n], pub_from u32[n] | None, flags): the tuple
        gains sub_deliver, the delivery word of every pair."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = len(off) - 1
        if deliver is not None:
            pf, fr, fl = self._host_deliver(deliver, n)
        counts = np.zeros(max(n, 1), dtype=np.uint32)
        offs = np.zeros(n + 1, dtype=np.uint64)
        scount = np.zeros(max(n, 1), dtype=np.uint32)
        soff = np.zeros(n + 1, dtype=np.uint64)
        cap = 1 << 16 if out_cap is None else out_cap
        scap = 1 << 16 if sub_cap is None else sub_cap
        while True:
            to, tg, nd = (np.zeros(max(cap, 1), dtype=np.uint32) for _ in range(3))
            sto, sid = (np.zeros(max(scap, 1), dtype=np.uint32) for _ in range(2))
            needed, sneeded = ctypes.c_uint64(), ctypes.c_uint64()
            if deliver is not None:
                sdv = np.zeros(max(scap, 1), dtype=np.uint32)
                dv = self._deliver_struct(_ptr(pf), _ptr(fr), fl, _ptr(sdv))
                rc = self.lib.tm_match_dispatch_batch_opts(self.h, _ptr(buf), _ptr(off), n, _ptr(counts), _ptr(offs),
                                                           _ptr(to), _ptr(tg), _ptr(nd), cap, ctypes.byref(needed),
                                                           _ptr(scount), _ptr(soff), _ptr(sto), _ptr(sid), scap,
                                                           ctypes.byref(sneeded), ctypes.byref(dv))
            else:
                rc = self.lib.tm_match_dispatch_batch(self.h, _ptr(buf), _ptr(off), n, _ptr(counts), _ptr(offs),
                                                      _ptr(to), _ptr(tg), _ptr(nd), cap, ctypes.byref(needed),
                                                      _ptr(scount), _ptr(soff), _ptr(sto), _ptr(sid), scap,
                                                      ctypes.byref(sneeded))
            if rc == L.TM_ENOSPC and (out_cap is None or needed.value <= cap) and \
                    (sub_cap is None or sneeded.value <= scap):
                cap = max(cap, int(needed.value))
                scap = max(scap, int(sneeded.value))
                continue
            if rc == L.TM_ENOSPC:
                e = L.TopicMatchError(rc, "tm_match_dispatch_batch: needs %d deliveries, %d pairs"
                                      % (needed.value, sneeded.value))
                e.needed, e.sub_needed = int(needed.value), int(sneeded.value)
                raise e
            self._check(rc, "tm_match_dispatch_batch")
            k, sk = int(needed.value), int(sneeded.value)
            res = (counts[:n], offs, to[:k], tg[:k], nd[:k], scount[:n], soff, sto[:sk], sid[:sk])
            return res if deliver is None else res + (sdv[:sk],)

    def match_dispatch_batch_device(self, d_bytes, d_off, n, topic_bytes, d_counts, d_offs, d_to, d_target, d_ndisp,
                                    out_cap, d_total, d_sub_count, d_sub_off, d_sub_to, d_sub_id, sub_cap,
                                    d_sub_total, stream=None, deliver=None):
        """deliver=(d_pub_flags, d_pub_from | None, flags, d_sub_deliver): device
        arrays; d_sub_deliver is written parallel to d_sub_id"""
        def p(x):
            if x is None:
                return None
            return ctypes.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))
        st = None
        if stream is not None:
            st = ctypes.c_void_p(L.stream_handle(stream))
        if deliver is not None:
            dv = self._deliver_struct(p(deliver[0]), p(deliver[1]), int(deliver[2]), p(deliver[3]))
            rc = self.lib.tm_match_dispatch_batch_opts_device(
                self.h, p(d_bytes), p(d_off), n, topic_bytes, p(d_counts), p(d_offs), p(d_to), p(d_target),
                p(d_ndisp), out_cap, p(d_total), p(d_sub_count), p(d_sub_off), p(d_sub_to), p(d_sub_id), sub_cap,
                p(d_sub_total), ctypes.byref(dv), st)
            return self._check(rc, "tm_match_dispatch_batch_opts_device")
        rc = self.lib.tm_match_dispatch_batch_device(self.h, p(d_bytes), p(d_off), n, topic_bytes, p(d_counts),
                                                     p(d_offs), p(d_to), p(d_target), p(d_ndisp), out_cap, p(d_total),
                                                     p(d_sub_count), p(d_sub_off), p(d_sub_to), p(d_sub_id), sub_cap,
                                                     p(d_sub_total), st)
        return self._check(rc, "tm_match_dispatch_batch_device")

    def dispatch_batch(self, buf, off, cap=None, deliver=None):
        """dispatch/2 by To bytes -> (ndisp u32[n], sub_off u64[n+1], sub_id);
        deliver=(pub_flags, pub_from | None, flags), entry i = (To i, message
        i): plus sub_deliver"""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = len(off) - 1
        if deliver is not None:
            pf, fr, fl = self._host_deliver(deliver, n)
        nd = np.zeros(max(n, 1), dtype=np.uint32)
        soff = np.zeros(n + 1, dtype=np.uint64)
        c = 1 << 16 if cap is None else cap
        while True:
            sid = np.zeros(max(c, 1), dtype=np.uint32)
            needed = ctypes.c_uint64()
            if deliver is not None:
                sdv = np.zeros(max(c, 1), dtype=np.uint32)
                dv = self._deliver_struct(_ptr(pf), _ptr(fr), fl, _ptr(sdv))
                rc = self.lib.tm_dispatch_batch_opts(self.h, _ptr(buf), _ptr(off), n, _ptr(nd), _ptr(soff), _ptr(sid),
                                                     c, ctypes.byref(needed), ctypes.byref(dv))
            else:
                rc = self.lib.tm_dispatch_batch(self.h, _ptr(buf), _ptr(off), n, _ptr(nd), _ptr(soff), _ptr(sid), c,
                                                ctypes.byref(needed))
            if rc == L.TM_ENOSPC and cap is None:
                c = int(needed.value)
                continue
            self._check(rc, "tm_dispatch_batch")
            res = (nd[:n], soff, sid[: int(needed.value)])
            return res if deliver is None else res + (sdv[: int(needed.value)],)

    # -- emqx_broker:forward/3, the sending half (forward.hip) ----------------------
    FORWARD_HDR_WORDS = 4

    def forward_plan(self, counts, offs, to, target, total=None, out_cap=None, group_cap=None, pub_cap=None):
        """tm_forward_plan over the host planes match_dispatch_batch /
        match_publish_batch returned -> (hdr u64[4] = {M, G, targets, 0},
        groups u32[G, 4] = rows {node target, To, first, count}, pub u32[M]):
        the batch's remote-node deliveries grouped per (target, To).  total:
        the route total (default len(to)); out_cap: the planes' capacity
        (default len(to)).  group_cap / pub_cap None: retried at the sizes the
        header reports; given: one call (TopicMatchError TM_ENOSPC when short,
        with .hdr)."""
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        to = np.ascontiguousarray(to, dtype=np.uint32)
        target = np.ascontiguousarray(target, dtype=np.uint32)
        n = len(offs) - 1
        total = len(to) if total is None else total
        out_cap = len(to) if out_cap is None else out_cap
        gc = 1 << 12 if group_cap is None else group_cap
        pc = 1 << 14 if pub_cap is None else pub_cap
        hdr = np.zeros(self.FORWARD_HDR_WORDS, dtype=np.uint64)
        while True:
            groups = np.zeros((max(gc, 1), 4), dtype=np.uint32)
            pub = np.zeros(max(pc, 1), dtype=np.uint32)
            rc = self.lib.tm_forward_plan(self.h, n, _ptr(counts), _ptr(offs), _ptr(to), _ptr(target), out_cap, total,
                                          _ptr(hdr), _ptr(groups), gc, _ptr(pub), pc)
            if rc == L.TM_ENOSPC and (group_cap is None or int(hdr[1]) <= gc) and \
                    (pub_cap is None or int(hdr[0]) <= pc):
                gc, pc = max(gc, int(hdr[1])), max(pc, int(hdr[0]))
                continue
            if rc == L.TM_ENOSPC:
                e = L.TopicMatchError(rc, "tm_forward_plan: needs %d groups, %d entries" % (hdr[1], hdr[0]))
                e.hdr = hdr.copy()
                raise e
            self._check(rc, "tm_forward_plan")
            return hdr, groups[: int(hdr[1])], pub[: int(hdr[0])]

    def forward_plan_device(self, n, d_counts, d_offs, d_to, d_target, out_cap, d_total, d_hdr, d_groups, group_cap,
                            d_pub, pub_cap, stream=None):
        """tm_forward_plan_device over device pointers (tensors or ints; None =
        NULL): the plan of the planes a *_batch_device publish call left"""
        def p(x):
            if x is None:
                return None
            return ctypes.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))
        st = None
        if stream is not None:
            st = ctypes.c_void_p(L.stream_handle(stream))
        rc = self.lib.tm_forward_plan_device(self.h, n, p(d_counts), p(d_offs), p(d_to), p(d_target), out_cap,
                                             p(d_total), p(d_hdr), p(d_groups), group_cap, p(d_pub), pub_cap, st)
        return self._check(rc, "tm_forward_plan_device")

    FORWARD_STREAM_HDR_WORDS = 8

    def forward_plan_stream_workspace_bytes(self, n, deliv_cap, pub_cap):
        """tm_forward_plan_stream_workspace_bytes (0: an argument out of range)"""
        return int(self.lib.tm_forward_plan_stream_workspace_bytes(n, deliv_cap, pub_cap))

    def forward_plan_stream_device(self, n, d_pub_hdr, d_doff, d_deliv, deliv_cap, d_workspace, workspace_bytes,
                                   d_hdr, d_groups, group_cap, d_pub, pub_cap, stream=None):
        """tm_forward_plan_stream_device over device pointers (tensors or ints;
        None = NULL): the forward plan of the packed outputs
        publish_stream[_opts]_device left, enqueued on `stream` without a host
        wait.  d_hdr: 8 u64, [0..3] = {M, G, targets, 0}, [6] the state (0
        complete, 1 the publish did not fit, 3 M > pub_cap, 4 G > group_cap)."""
        def p(x):
            if x is None:
                return None
            return ctypes.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))
        st = None
        if stream is not None:
            st = ctypes.c_void_p(L.stream_handle(stream))
        rc = self.lib.tm_forward_plan_stream_device(self.h, n, p(d_pub_hdr), p(d_doff), p(d_deliv), deliv_cap,
                                                    p(d_workspace), workspace_bytes, p(d_hdr), p(d_groups), group_cap,
                                                    p(d_pub), pub_cap, st)
        return self._check(rc, "tm_forward_plan_stream_device")

    # -- the inbox plan: a batch's local sends per subscriber (inbox.hip) -----------
    INBOX_HDR_WORDS = 4
    INBOX_PICK = 0x80000000           # ent_pub bit 31: the entry is a pick send

    def inbox_plan(self, sub_off, sub_to, sub_id, sub_deliver=None, counts=None, offs=None, to=None, pick=None,
                   pick_word=None, sub_total=None, sub_cap=None, total=None, out_cap=None, inbox_cap=None,
                   ent_cap=None, words=None):
        """tm_inbox_plan over the host planes match_dispatch_batch /
        match_publish_batch (+ share_pick_words) returned -> (hdr u64[4] = {E,
        S, pair sends, pick sends}, inbox u32[S, 4] = rows {sub, first, count,
        picks}, ent_pub u32[E] (bit 31 = INBOX_PICK on a pick send), ent_to
        u32[E], ent_word u32[E] | None): the batch's local sends grouped per
        subscriber.  sub_deliver / pick_word None: no words for that kind;
        pick None: no pick sends (counts / offs / to unused).  words: whether
        ent_word is produced (default: when a word plane is given).  sub_total
        / total: the totals the publish call reported (default the planes'
        lengths); sub_cap / out_cap: the planes' capacities (default their
        lengths).  inbox_cap / ent_cap None: retried at the sizes the header
        reports; given: one call (TopicMatchError TM_ENOSPC when short, with
        .hdr)."""
        u32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.uint32)   # noqa: E731
        u64 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.uint64)   # noqa: E731
        sub_off, offs = u64(sub_off), u64(offs)
        sub_to, sub_id, sub_deliver, counts, to, pick, pick_word = (u32(a) for a in (sub_to, sub_id, sub_deliver,
                                                                                     counts, to, pick, pick_word))
        n = len(sub_off) - 1
        plen = 0 if sub_id is None else len(sub_id)
        klen = 0 if pick is None else len(pick)
        sub_total = plen if sub_total is None else sub_total
        sub_cap = plen if sub_cap is None else sub_cap
        total = klen if total is None else total
        out_cap = klen if out_cap is None else out_cap
        if words is None:
            words = sub_deliver is not None or pick_word is not None
        ic = 1 << 12 if inbox_cap is None else inbox_cap
        ec = 1 << 14 if ent_cap is None else ent_cap
        hdr = np.zeros(self.INBOX_HDR_WORDS, dtype=np.uint64)
        while True:
            inbox = np.zeros((max(ic, 1), 4), dtype=np.uint32)
            ent_pub, ent_to = (np.zeros(max(ec, 1), dtype=np.uint32) for _ in range(2))
            ent_word = np.zeros(max(ec, 1), dtype=np.uint32) if words else None
            rc = self.lib.tm_inbox_plan(self.h, n, _ptr(sub_off), _ptr(sub_to), _ptr(sub_id), _ptr(sub_deliver),
                                        sub_cap, sub_total, _ptr(counts), _ptr(offs), _ptr(to), _ptr(pick),
                                        _ptr(pick_word), out_cap, total, _ptr(hdr), _ptr(inbox), ic, _ptr(ent_pub),
                                        _ptr(ent_to), _ptr(ent_word), ec)
            if rc == L.TM_ENOSPC and (inbox_cap is None or int(hdr[1]) <= ic) and \
                    (ent_cap is None or int(hdr[0]) <= ec):
                ic, ec = max(ic, int(hdr[1])), max(ec, int(hdr[0]))
                continue
            if rc == L.TM_ENOSPC:
                e = L.TopicMatchError(rc, "tm_inbox_plan: needs %d subscribers, %d entries" % (hdr[1], hdr[0]))
                e.hdr = hdr.copy()
                raise e
            self._check(rc, "tm_inbox_plan")
            E, S = int(hdr[0]), int(hdr[1])
            return hdr, inbox[:S], ent_pub[:E], ent_to[:E], (ent_word[:E] if words else None)

    def inbox_plan_device(self, n, d_sub_off, d_sub_to, d_sub_id, d_sub_deliver, sub_cap, d_sub_total, d_counts,
                          d_offs, d_to, d_pick, d_pick_word, out_cap, d_total, d_hdr, d_inbox, inbox_cap, d_ent_pub,
                          d_ent_to, d_ent_word, ent_cap, stream=None):
        """tm_inbox_plan_device over device pointers (tensors or ints; None =
        NULL): the plan of the planes a *_batch_device publish call left"""
        def p(x):
            if x is None:
                return None
            return ctypes.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))
        st = None
        if stream is not None:
            st = ctypes.c_void_p(L.stream_handle(stream))
        rc = self.lib.tm_inbox_plan_device(self.h, n, p(d_sub_off), p(d_sub_to), p(d_sub_id), p(d_sub_deliver),
                                           sub_cap, p(d_sub_total), p(d_counts), p(d_offs), p(d_to), p(d_pick),
                                           p(d_pick_word), out_cap, p(d_total), p(d_hdr), p(d_inbox), inbox_cap,
                                           p(d_ent_pub), p(d_ent_to), p(d_ent_word), ent_cap, st)
        return self._check(rc, "tm_inbox_plan_device")

    INBOX_STREAM_HDR_WORDS = 8

    def inbox_plan_stream_workspace_bytes(self, n, deliv_cap, pair_cap, ent_cap):
        """tm_inbox_plan_stream_workspace_bytes (0: an argument out of range)"""
        return int(self.lib.tm_inbox_plan_stream_workspace_bytes(n, deliv_cap, pair_cap, ent_cap))

    def inbox_plan_stream_device(self, n, d_pub_hdr, d_doff, d_sub_off, d_deliv, d_pick_word, deliv_cap, d_pairs,
                                 d_pair_word, pair_cap, sub_bits, d_workspace, workspace_bytes, d_hdr, d_inbox,
                                 inbox_cap, d_ent_pub, d_ent_to, d_ent_word, ent_cap, stream=None):
        """tm_inbox_plan_stream_device over device pointers (tensors or ints;
        None = NULL): the plan of the packed outputs publish_stream[_opts]_device
        left, enqueued on `stream` without a host wait.  d_hdr: 8 u64, [6] the
        state (0 complete, 1 the publish did not fit, 2 an id wider than
        sub_bits, 3 E > ent_cap, 4 S > inbox_cap)."""
        def p(x):
            if x is None:
                return None
            return ctypes.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))
        st = None
        if stream is not None:
            st = ctypes.c_void_p(L.stream_handle(stream))
        rc = self.lib.tm_inbox_plan_stream_device(self.h, n, p(d_pub_hdr), p(d_doff), p(d_sub_off), p(d_deliv),
                                                  p(d_pick_word), deliv_cap, p(d_pairs), p(d_pair_word), pair_cap,
                                                  sub_bits, p(d_workspace), workspace_bytes, p(d_hdr), p(d_inbox),
                                                  inbox_cap, p(d_ent_pub), p(d_ent_to), p(d_ent_word), ent_cap, st)
        return self._check(rc, "tm_inbox_plan_stream_device")

    # -- emqx_shared_sub: the $share member table and the pick (share.hip) ---------
    NO_MEMBER = 0xFFFFFFFF            # pick: `false`, or not a $share delivery
    SHARE_KEYED, SHARE_ROUND_ROBIN, SHARE_STICKY = 1, 2, 3

    def share_add(self, group: bytes, topic: bytes, member: int):
        """subscribe/3: a record already in the bag leaves it as it was"""
        return self._check(self.lib.tm_share_add(self.h, group, len(group), topic, len(topic), member),
                           "tm_share_add")

    def share_del(self, group: bytes, topic: bytes, member: int) -> int:
        """unsubscribe/3; returns the members left in the (group, topic) set"""
        left = ctypes.c_uint32()
        self._check(self.lib.tm_share_del(self.h, group, len(group), topic, len(topic), member, ctypes.byref(left)),
                    "tm_share_del")
        return left.value

    def _share_many(self, fn, what, gbuf, goff, tbuf, toff, members):
        n = len(toff) - 1
        gbuf = np.ascontiguousarray(gbuf, dtype=np.uint8)
        goff = np.ascontiguousarray(goff, dtype=np.uint64)
        tbuf = np.ascontiguousarray(tbuf, dtype=np.uint8)
        toff = np.ascontiguousarray(toff, dtype=np.uint64)
        members = np.ascontiguousarray(members, dtype=np.uint32)
        return self._check(fn(self.h, _ptr(gbuf), _ptr(goff), _ptr(tbuf), _ptr(toff), _ptr(members), n), what)

    def share_add_many(self, gbuf, goff, tbuf, toff, members):
        """record i = (group i of (gbuf, goff), topic i of (tbuf, toff), members[i])"""
        return self._share_many(self.lib.tm_share_add_batch, "tm_share_add_batch", gbuf, goff, tbuf, toff, members)

    def share_del_many(self, gbuf, goff, tbuf, toff, members):
        return self._share_many(self.lib.tm_share_del_batch, "tm_share_del_batch", gbuf, goff, tbuf, toff, members)

    def share_member_down(self, member: int) -> int:
        """cleanup_down/1; returns the records deleted"""
        k = ctypes.c_uint32()
        self._check(self.lib.tm_share_member_down(self.h, member, ctypes.byref(k)), "tm_share_member_down")
        return k.value

    def share_members(self, group: bytes, topic: bytes, cap=None):
        """subscribers/2 in insertion order.  cap given: one call
        (TopicMatchError TM_ENOSPC when the set is larger)"""
        n = ctypes.c_uint32()
        c = 16 if cap is None else cap
        while True:
            out = np.zeros(max(c, 1), dtype=np.uint32)
            rc = self.lib.tm_share_members(self.h, group, len(group), topic, len(topic), _ptr(out), c, ctypes.byref(n))
            if rc == L.TM_ENOSPC and cap is None:
                c = n.value
                continue
            self._check(rc, "tm_share_members")
            return [int(x) for x in out[: n.value]]

    @property
    def share_count(self):
        return self.lib.tm_share_count(self.h)

    def debug_check_shares(self):
        """host-side consistency check of the in-place share image
        (diagnostic, tm_debug_check_shares)"""
        self.lib.tm_debug_check_shares.argtypes = [ctypes.c_void_p]
        return self._check(self.lib.tm_debug_check_shares(self.h), "tm_debug_check_shares")

    NO_WORD = L.TM_NO_WORD            # pick word: no pick, or a picked member outside its set

    def debug_share_opts(self, group: bytes, topic: bytes):
        """the option words of a set's members in list order, from the host
        mirror of the member option pool (diagnostic, tm_debug_share_opts)"""
        n = ctypes.c_uint32()
        c = 16
        while True:
            out = np.zeros(max(c, 1), dtype=np.uint32)
            rc = self.lib.tm_debug_share_opts(self.h, group, len(group), topic, len(topic), _ptr(out), c,
                                              ctypes.byref(n))
            if rc == L.TM_ENOSPC:
                c = n.value
                continue
            self._check(rc, "tm_debug_share_opts")
            return [int(x) for x in out[: n.value]]

    def share_pick_words(self, buf, off, counts, offs, to, target, pick, deliver, total=None, out_cap=None,
                         pick_word=None):
        """tm_share_pick_words over the host planes match_publish_batch
        returned -> pick_word u32 (one per delivery slot): the delivery word of
        every $share pick, NO_WORD for a slot without a pick and for a picked
        member that is not in its set.  deliver=(pub_flags u32[n], pub_from
        u32[n] | None, flags).  total: the route total (default len(to));
        out_cap: the planes' capacity (default len(to)).  pick_word: the array
        to write into (holes and slots past the bound keep what it holds)."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        to = np.ascontiguousarray(to, dtype=np.uint32)
        target = np.ascontiguousarray(target, dtype=np.uint32)
        pick = np.ascontiguousarray(pick, dtype=np.uint32)
        n = len(off) - 1
        pf, fr, fl = self._host_deliver(deliver, n)
        total = len(to) if total is None else total
        out_cap = len(to) if out_cap is None else out_cap
        live = min(total, out_cap)
        own = pick_word is None
        if own:
            pick_word = np.full(max(live, 1), L.TM_NO_WORD, dtype=np.uint32)
        elif pick_word.dtype != np.uint32 or not pick_word.flags.c_contiguous or len(pick_word) < live:
            raise ValueError("pick_word: a contiguous u32 array of at least min(total, out_cap) words")
        dv = self._deliver_struct(_ptr(pf), _ptr(fr), fl, None)
        rc = self.lib.tm_share_pick_words(self.h, _ptr(buf), _ptr(off), n, _ptr(counts), _ptr(offs), _ptr(to),
                                          _ptr(target), _ptr(pick), out_cap, total, ctypes.byref(dv),
                                          _ptr(pick_word))
        self._check(rc, "tm_share_pick_words")
        return pick_word[:live] if own else pick_word

    def share_pick_words_device(self, d_bytes, d_off, n, d_counts, d_offs, d_to, d_target, d_pick, out_cap, d_total,
                                deliver, d_pick_word, stream=None):
        """tm_share_pick_words_device over device pointers (tensors or ints;
        None = NULL): deliver=(d_pub_flags, d_pub_from | None, flags)"""
        def p(x):
            if x is None:
                return None
            return ctypes.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))
        st = None
        if stream is not None:
            st = ctypes.c_void_p(L.stream_handle(stream))
        dv = None
        if deliver is not None:
            dv = ctypes.byref(self._deliver_struct(p(deliver[0]), p(deliver[1]), int(deliver[2]),
                                                   p(deliver[3]) if len(deliver) > 3 else None))
        rc = self.lib.tm_share_pick_words_device(self.h, p(d_bytes), p(d_off), n, p(d_counts), p(d_offs), p(d_to),
                                                 p(d_target), p(d_pick), out_cap, p(d_total), dv, p(d_pick_word), st)
        return self._check(rc, "tm_share_pick_words_device")

    def match_publish_batch(self, buf, off, strategy, keys=None, out_cap=None, sub_cap=None, deliver=None,
                            pick_words=False):
        """match_dispatch_batch's tuple plus pick u32 (one per delivery slot):
        the member picked for a $share delivery, NO_MEMBER otherwise.
        strategy SHARE_KEYED and SHARE_STICKY take keys (u32[n]);
        SHARE_ROUND_ROBIN none.  A short out_cap / sub_cap: as
        match_dispatch_batch (no cursor moves, no sticky entry is stored).
        deliver: as match_dispatch_batch, sub_deliver goes last.
        pick_words=True (with deliver): the tuple gains, after sub_deliver,
        pick_word u32 (one per delivery slot) from the share_pick_words
        post-pass.  That is a second, synchronous device call (the planes go
        up again) on the epoch current at that moment: a commit between the
        two calls changes the words, not the picks."""
        if pick_words:
            if deliver is None:
                raise ValueError("pick_words needs deliver")
            res = self.match_publish_batch(buf, off, strategy, keys=keys, out_cap=out_cap, sub_cap=sub_cap,
                                           deliver=deliver)
            words = self.share_pick_words(buf, off, res[0], res[1], res[2], res[3], res[9], deliver)
            return res + (words[: len(res[2])],)
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = len(off) - 1
        if deliver is not None:
            pf, fr, fl = self._host_deliver(deliver, n)
        if keys is not None:
            keys = np.ascontiguousarray(keys, dtype=np.uint32)
            if len(keys) != n:
                raise ValueError("keys: one u32 per topic")
        counts = np.zeros(max(n, 1), dtype=np.uint32)
        offs = np.zeros(n + 1, dtype=np.uint64)
        scount = np.zeros(max(n, 1), dtype=np.uint32)
        soff = np.zeros(n + 1, dtype=np.uint64)
        cap = 1 << 16 if out_cap is None else out_cap
        scap = 1 << 16 if sub_cap is None else sub_cap
        while True:
            to, tg, nd, pick = (np.zeros(max(cap, 1), dtype=np.uint32) for _ in range(4))
            sto, sid = (np.zeros(max(scap, 1), dtype=np.uint32) for _ in range(2))
            needed, sneeded = ctypes.c_uint64(), ctypes.c_uint64()
            if deliver is not None:
                sdv = np.zeros(max(scap, 1), dtype=np.uint32)
                dv = self._deliver_struct(_ptr(pf), _ptr(fr), fl, _ptr(sdv))
                rc = self.lib.tm_match_publish_batch_opts(self.h, _ptr(buf), _ptr(off), n, _ptr(counts), _ptr(offs),
                                                          _ptr(to), _ptr(tg), _ptr(nd), cap, ctypes.byref(needed),
                                                          _ptr(scount), _ptr(soff), _ptr(sto), _ptr(sid), scap,
                                                          ctypes.byref(sneeded), strategy, _ptr(keys), _ptr(pick),
                                                          ctypes.byref(dv))
            else:
                rc = self.lib.tm_match_publish_batch(self.h, _ptr(buf), _ptr(off), n, _ptr(counts), _ptr(offs),
                                                     _ptr(to), _ptr(tg), _ptr(nd), cap, ctypes.byref(needed),
                                                     _ptr(scount), _ptr(soff), _ptr(sto), _ptr(sid), scap,
                                                     ctypes.byref(sneeded), strategy, _ptr(keys), _ptr(pick))
            if rc == L.TM_ENOSPC and (out_cap is None or needed.value <= cap) and \
                    (sub_cap is None or sneeded.value <= scap):
                cap = max(cap, int(needed.value))
                scap = max(scap, int(sneeded.value))
                continue
            if rc == L.TM_ENOSPC:
                e = L.TopicMatchError(rc, "tm_match_publish_batch: needs %d deliveries, %d pairs"
                                      % (needed.value, sneeded.value))
                e.needed, e.sub_needed = int(needed.value), int(sneeded.value)
                raise e
            self._check(rc, "tm_match_publish_batch")
            k, sk = int(needed.value), int(sneeded.value)
            res = (counts[:n], offs, to[:k], tg[:k], nd[:k], scount[:n], soff, sto[:sk], sid[:sk], pick[:k])
            return res if deliver is None else res + (sdv[:sk],)

    def match_publish_batch_device(self, d_bytes, d_off, n, topic_bytes, d_counts, d_offs, d_to, d_target, d_ndisp,
                                   out_cap, d_total, d_sub_count, d_sub_off, d_sub_to, d_sub_id, sub_cap,
                                   d_sub_total, strategy, d_keys, d_pick, stream=None, deliver=None):
        """deliver: as match_dispatch_batch_device"""
        def p(x):
            if x is None:
                return None
            return ctypes.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))
        st = None
        if stream is not None:
            st = ctypes.c_void_p(L.stream_handle(stream))
        if deliver is not None:
            dv = self._deliver_struct(p(deliver[0]), p(deliver[1]), int(deliver[2]), p(deliver[3]))
            rc = self.lib.tm_match_publish_batch_opts_device(
                self.h, p(d_bytes), p(d_off), n, topic_bytes, p(d_counts), p(d_offs), p(d_to), p(d_target),
                p(d_ndisp), out_cap, p(d_total), p(d_sub_count), p(d_sub_off), p(d_sub_to), p(d_sub_id), sub_cap,
                p(d_sub_total), strategy, p(d_keys), p(d_pick), ctypes.byref(dv), st)
            return self._check(rc, "tm_match_publish_batch_opts_device")
        rc = self.lib.tm_match_publish_batch_device(self.h, p(d_bytes), p(d_off), n, topic_bytes, p(d_counts),
                                                    p(d_offs), p(d_to), p(d_target), p(d_ndisp), out_cap, p(d_total),
                                                    p(d_sub_count), p(d_sub_off), p(d_sub_to), p(d_sub_id), sub_cap,
                                                    p(d_sub_total), strategy, p(d_keys), p(d_pick), st)
        return self._check(rc, "tm_match_publish_batch_device")

    def publish_pack(self, n, d_counts, d_offs, d_to, d_target, d_ndisp, d_pick, out_cap, d_total, d_sub_off,
                     d_sub_to, d_sub_id, sub_cap, d_sub_total, d_hdr, d_doff, d_deliv, deliv_cap, d_pairs, pair_cap,
                     stream=None):
        """tm_publish_pack_device over device pointers (tensors or ints; None =
        NULL): the publish call's planes as dense 16 B delivery and 8 B pair
        records, header and offsets"""
        def p(x):
            if x is None:
                return None
            return ctypes.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))
        st = None
        if stream is not None:
            st = ctypes.c_void_p(L.stream_handle(stream))
        rc = self.lib.tm_publish_pack_device(self.h, n, p(d_counts), p(d_offs), p(d_to), p(d_target), p(d_ndisp),
                                             p(d_pick), out_cap, p(d_total), p(d_sub_off), p(d_sub_to), p(d_sub_id),
                                             sub_cap, p(d_sub_total), p(d_hdr), p(d_doff), p(d_deliv), deliv_cap,
                                             p(d_pairs), pair_cap, st)
        return self._check(rc, "tm_publish_pack_device")

    def share_cursors(self, replica=0):
        """tm_share_cursors_open: one publisher's dictionary (round-robin
        cursors and sticky entries) on a replica"""
        return ShareCursors(self, replica)

    def share_pick_batch(self, strategy, gbuf, goff, tbuf, toff, keys, failed, failed_off, cursors=None):
        """tm_share_pick_batch: pick/5 with FailedSubs (the retry of
        dispatch/4).  Request i = (group i of (gbuf, goff), To i of (tbuf,
        toff), keys[i], failed[failed_off[i]:failed_off[i+1]]); returns
        pick u32[n], NO_MEMBER for `false` and for a set that does not exist.
        cursors: a ShareCursors on the first replica, None = the built-in arrays"""
        n = len(toff) - 1
        gbuf = np.ascontiguousarray(gbuf, dtype=np.uint8)
        goff = np.ascontiguousarray(goff, dtype=np.uint64)
        tbuf = np.ascontiguousarray(tbuf, dtype=np.uint8)
        toff = np.ascontiguousarray(toff, dtype=np.uint64)
        if keys is not None:
            keys = np.ascontiguousarray(keys, dtype=np.uint32)
            if len(keys) != n:
                raise ValueError("keys: one u32 per request")
        failed = np.ascontiguousarray(failed, dtype=np.uint32)
        failed_off = np.ascontiguousarray(failed_off, dtype=np.uint64)
        if len(goff) != n + 1 or len(failed_off) != n + 1:
            raise ValueError("group and failed offsets: n + 1 entries each")
        pick = np.zeros(max(n, 1), dtype=np.uint32)
        rc = self.lib.tm_share_pick_batch(self.h, strategy, cursors.h if cursors is not None else None, _ptr(gbuf),
                                          _ptr(goff), _ptr(tbuf), _ptr(toff), _ptr(keys),
                                          _ptr(failed) if len(failed) else None, _ptr(failed_off), n, _ptr(pick))
        self._check(rc, "tm_share_pick_batch")
        return pick[:n]

    def publish_stream_workspace_bytes(self, n, topic_bytes, caps):
        """caps: (ids, routes, pairs, rr)"""
        c = L.TmPublishCaps(*[int(x) for x in caps])
        return int(self.lib.tm_publish_stream_workspace_bytes(self.h, n, topic_bytes, ctypes.byref(c)))

    def publish_stream_device(self, d_bytes, d_off, n, topic_bytes, strategy, d_keys, cursors, caps, d_workspace,
                              workspace_bytes, d_hdr, d_doff, d_sub_off, d_deliv, d_pairs, stream=None):
        """tm_publish_stream_device over device pointers (tensors or ints; None
        = NULL): publish/1 up to the sends, enqueued on `stream` without a
        host wait.  caps: (ids, routes, pairs, rr); cursors: a ShareCursors or
        None (the replica's built-in array).  The header's state word says
        whether every stage fitted."""
        def p(x):
            if x is None:
                return None
            return ctypes.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))
        st = None
        if stream is not None:
            st = ctypes.c_void_p(L.stream_handle(stream))
        c = L.TmPublishCaps(*[int(x) for x in caps])
        rc = self.lib.tm_publish_stream_device(self.h, p(d_bytes), p(d_off), n, topic_bytes, strategy, p(d_keys),
                                               cursors.h if cursors is not None else None, ctypes.byref(c),
                                               p(d_workspace), workspace_bytes, p(d_hdr), p(d_doff), p(d_sub_off),
                                               p(d_deliv), p(d_pairs), st)
        return self._check(rc, "tm_publish_stream_device")

    def publish_stream_opts_workspace_bytes(self, n, topic_bytes, caps):
        """the workspace need of publish_stream_opts_device; caps: (ids, routes, pairs, rr)"""
        c = L.TmPublishCaps(*[int(x) for x in caps])
        return int(self.lib.tm_publish_stream_opts_workspace_bytes(self.h, n, topic_bytes, ctypes.byref(c)))

    def publish_stream_opts_device(self, d_bytes, d_off, n, topic_bytes, strategy, d_keys, cursors, caps,
                                   d_workspace, workspace_bytes, d_hdr, d_doff, d_sub_off, d_deliv, d_pairs, deliver,
                                   d_pick_word, stream=None):
        """tm_publish_stream_opts_device: publish_stream_device with the
        delivery words.  deliver=(d_pub_flags, d_pub_from | None, flags,
        d_pair_word): d_pair_word (caps.pairs words) is written parallel to
        d_pairs, d_pick_word (caps.routes words) parallel to d_deliv"""
        def p(x):
            if x is None:
                return None
            return ctypes.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))
        st = None
        if stream is not None:
            st = ctypes.c_void_p(L.stream_handle(stream))
        c = L.TmPublishCaps(*[int(x) for x in caps])
        dv = None
        if deliver is not None:
            dv = ctypes.byref(self._deliver_struct(p(deliver[0]), p(deliver[1]), int(deliver[2]), p(deliver[3])))
        rc = self.lib.tm_publish_stream_opts_device(self.h, p(d_bytes), p(d_off), n, topic_bytes, strategy, p(d_keys),
                                                    cursors.h if cursors is not None else None, ctypes.byref(c),
                                                    p(d_workspace), workspace_bytes, p(d_hdr), p(d_doff),
                                                    p(d_sub_off), p(d_deliv), p(d_pairs), dv, p(d_pick_word), st)
        return self._check(rc, "tm_publish_stream_opts_device")

    def publish_stream_gated_device(self, d_bytes, d_off, n, topic_bytes, strategy, d_keys, cursors, caps,
                                    d_workspace, workspace_bytes, d_hdr, d_doff, d_sub_off, d_deliv, d_pairs, deliver,
                                    d_pick_word, d_code, stream=None):
        """tm_publish_stream_gated_device: the stream call behind an admission
        verdict.  d_code: n device bytes, non-zero = refused (None: ungated).
        deliver and d_pick_word both None select the plain call, both given
        (deliver as publish_stream_opts_device takes it) the call with options"""
        def p(x):
            if x is None:
                return None
            return ctypes.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))
        st = None
        if stream is not None:
            st = ctypes.c_void_p(L.stream_handle(stream))
        c = L.TmPublishCaps(*[int(x) for x in caps])
        dv = None
        if deliver is not None:
            dv = ctypes.byref(self._deliver_struct(p(deliver[0]), p(deliver[1]), int(deliver[2]), p(deliver[3])))
        rc = self.lib.tm_publish_stream_gated_device(self.h, p(d_bytes), p(d_off), n, topic_bytes, strategy,
                                                     p(d_keys), cursors.h if cursors is not None else None,
                                                     ctypes.byref(c), p(d_workspace), workspace_bytes, p(d_hdr),
                                                     p(d_doff), p(d_sub_off), p(d_deliv), p(d_pairs), dv,
                                                     p(d_pick_word), p(d_code), st)
        return self._check(rc, "tm_publish_stream_gated_device")

    # -- publish admission (admit.hip): validate/1, check_pub/2, check_pub_acl --
    @staticmethod
    def admit_batch(buf, off, pub_flags, zones, mount_len=None, pub_admit=None, acl_result=None):
        """tm_admit_batch on host arrays (no device): -> (code u8[n], hdr
        u64[8]).  zones: an emqx_access.Zones; acl_result: int8 1 / 0 / -1 per
        publish as the ACL check writes them (None: every check nomatch)"""
        lib = L.load()
        n = len(off) - 1
        code = np.zeros(max(n, 1), dtype=np.uint8)
        hdr = np.zeros(8, dtype=np.uint64)
        tab, nz = zones.table()

        def arr(a, dt):
            return None if a is None else np.ascontiguousarray(a, dtype=dt)
        off = arr(off, np.uint64)
        ml, pf, pa, ar = arr(mount_len, np.uint32), arr(pub_flags, np.uint32), arr(pub_admit, np.uint32), \
            arr(acl_result, np.int8)
        rc = lib.tm_admit_batch(_ptr(buf), _ptr(off), n, _ptr(ml), _ptr(pf), _ptr(pa), tab, nz, _ptr(ar), _ptr(code),
                                _ptr(hdr))
        if rc != L.TM_OK:
            raise L.TopicMatchError(rc, "tm_admit_batch")
        return code[:n], hdr

    @staticmethod
    def admit_batch_device(d_bytes, d_off, n, d_mount_len, d_pub_flags, d_pub_admit, zones, d_acl_result, d_code,
                           d_hdr, stream=None):
        """tm_admit_batch_device over device pointers (tensors or ints; None =
        NULL), stream-ordered: d_code[n] bytes and d_hdr[8] = {admitted, count
        of code 1..5, 0, 0}.  zones: an emqx_access.Zones (a host table)"""
        lib = L.load()

        def p(x):
            if x is None:
                return None
            return ctypes.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))
        st = None
        if stream is not None:
            st = ctypes.c_void_p(L.stream_handle(stream))
        tab, nz = zones.table()
        rc = lib.tm_admit_batch_device(p(d_bytes), p(d_off), n, p(d_mount_len), p(d_pub_flags), p(d_pub_admit), tab,
                                       nz, p(d_acl_result), p(d_code), p(d_hdr), st)
        if rc != L.TM_OK:
            raise L.TopicMatchError(rc, "tm_admit_batch_device")

    def publish_pack_opts(self, n, d_counts, d_offs, d_to, d_target, d_ndisp, d_pick, out_cap, d_total, d_sub_off,
                          d_sub_to, d_sub_id, sub_cap, d_sub_total, d_hdr, d_doff, d_deliv, deliv_cap, d_pairs,
                          pair_cap, d_sub_deliver, d_pick_word_slots, d_pair_word, d_pick_word, stream=None):
        """tm_publish_pack_opts_device: publish_pack plus the two dense word
        planes (d_pair_word parallel to d_pairs, d_pick_word parallel to
        d_deliv) from the publish call's pair words and the pick-word pass's
        slot plane"""
        def p(x):
            if x is None:
                return None
            return ctypes.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))
        st = None
        if stream is not None:
            st = ctypes.c_void_p(L.stream_handle(stream))
        rc = self.lib.tm_publish_pack_opts_device(self.h, n, p(d_counts), p(d_offs), p(d_to), p(d_target), p(d_ndisp),
                                                  p(d_pick), out_cap, p(d_total), p(d_sub_off), p(d_sub_to),
                                                  p(d_sub_id), sub_cap, p(d_sub_total), p(d_hdr), p(d_doff),
                                                  p(d_deliv), deliv_cap, p(d_pairs), pair_cap, p(d_sub_deliver),
                                                  p(d_pick_word_slots), p(d_pair_word), p(d_pick_word), st)
        return self._check(rc, "tm_publish_pack_opts_device")

    # walk variants (A/B knobs of tm_walk_queue): one global dequeue head, or
    # per-XCD heads over contiguous ranges of the batch
    WALKS = {"queue": 0, "queue_xcd": 1}

    def set_option(self, name: str, value: int):
        self._check(self.lib.tm_set_option(self.h, name.encode(), int(value)), "tm_set_option(%s)" % name)

    def set_walk(self, walk: str):
        self.set_option("xcdq", self.WALKS[walk])

    # -- instrumentation ----------------------------------------------------
    def set_stats(self, on=True):
        self._check(self.lib.tm_set_stats(self.h, 1 if on else 0), "tm_set_stats")

    def last_stats(self):
        s = L.TmBatchStats()
        self._check(self.lib.tm_last_stats(self.h, ctypes.byref(s)), "tm_last_stats")
        return {k: getattr(s, k) for k, _ in s._fields_}

    def set_timing(self, on=True):
        self._check(self.lib.tm_set_timing(self.h, 1 if on else 0), "tm_set_timing")

    def last_kernel_times(self):
        names = (ctypes.c_char_p * 16)()
        ms = (ctypes.c_float * 16)()
        k = self.lib.tm_last_kernel_times(self.h, names, ms, 16)
        if k < 0:
            self._check(k, "tm_last_kernel_times")
        return {names[i].decode(): ms[i] for i in range(k)}


class ShareCursors:
    """One publisher process's round-robin cursors and sticky entries on one
    replica (tm_share_cursors; src/emqx_shared_sub.erl:243-249, :211-224).  Close it before the
    engine; closing it afterwards only frees the host handle."""

    def __init__(self, engine, replica=0):
        self.lib = engine.lib
        self.replica = replica
        h = ctypes.c_void_p()
        rc = self.lib.tm_share_cursors_open(engine.h, replica, ctypes.byref(h))
        if rc != L.TM_OK:
            raise L.TopicMatchError(rc, "tm_share_cursors_open")
        self.h = h

    def close(self):
        if self.h:
            self.lib.tm_share_cursors_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
