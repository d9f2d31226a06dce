"""The publish lane's two memory blocks (emqx_amd/csrc/batcher_layout.h:
up_block, down_block) on the CPU, through tm_debug_batcher_layout: the
invariants every user of an offset relies on, and equality, field for field,
with tests/golden/batcher_layout.json -- the offsets the lane computed before
the two descriptions existed, recorded once from that commit's own formulas
(its block_layout, admit_up_layout, ps_head, keyb_of and upb_of behind the
same export, dumped over the same cases)."""
import ctypes
import itertools
import json
import os

import pytest

from emqx_amd import _lib as L

UP = ["off", "key", "pflags", "pfrom", "bytes", "mlen", "padmit", "coff", "uoff", "access", "cdef", "udef", "fam", "peers",
      "cbytes", "ubytes", "utoff", "utbytes", "end"]
DOWN = ["hdr", "doff", "sub_off", "deliv", "pairs", "pickw", "pairw", "ihdr", "inbox", "epub", "eto", "ewd", "fhdr",
        "fgroups", "fpub", "ahdr", "rule", "code", "aclres", "a_back", "backb", "outb", "ecap"]
O, I, F, A = L.TM_BATCHER_OPTS, L.TM_BATCHER_INBOX, L.TM_BATCHER_FORWARD, L.TM_BATCHER_ADMIT
MODES = [0, O, O | I, F, O | F, O | I | F, O | A, O | I | A, O | F | A, O | I | F | A]
NS = [0, 1, 7, 8, 9, 32768, 32769]
CAPS = [(1024, 4096), (1045, 3003)]          # (cap, scap); the second pair odd
CREDS = [(0, 5), (5, 8), (8, 0)]             # (client bytes, user bytes) of the batch
MOUNTED = [0, 1]


def topic_bytes(n):
    return 13 * n + 3 if n else 0            # no multiple of 8


def cases():
    return itertools.product(MODES, NS, CAPS, CREDS, MOUNTED)


def up_key(flags, n, cred, mounted):
    """the block that goes up depends on OPTS and ADMIT alone, and on the credentials and the mountpoint
    only with ADMIT"""
    adm = bool(flags & A)
    return "%d,%d,%d,%d,%d,%d" % (bool(flags & O), adm, n, cred[0] if adm else 0, cred[1] if adm else 0,
                                  mounted if adm else 0)


def down_key(flags, n, caps):
    return "%d,%d,%d,%d" % (flags, n, caps[0], caps[1])


def layout(lib, flags, n, caps, cred, mounted):
    out = (ctypes.c_uint64 * (len(UP) + len(DOWN)))()
    rc = lib.tm_debug_batcher_layout(flags, n, caps[0], caps[1], topic_bytes(n), cred[0], cred[1], mounted, out, len(out))
    assert rc == L.TM_OK
    v = [int(x) for x in out]
    return v[:len(UP)], v[len(UP):]


@pytest.fixture(scope="module")
def lib():
    return L.load()


def test_export_checks_its_arguments(lib):
    out = (ctypes.c_uint64 * 64)()
    assert lib.tm_debug_batcher_layout(0, 1, 1, 1, 1, 0, 0, 0, None, 64) == L.TM_EINVAL
    assert lib.tm_debug_batcher_layout(0, 1, 1, 1, 1, 0, 0, 0, out, len(UP) + len(DOWN) - 1) == L.TM_EINVAL


def _pieces_up(u, flags, n, cred, mounted):
    """(name, offset, bytes, alignment) of every piece of the block that goes up, in order"""
    tb = topic_bytes(n)
    p = [("off", u["off"], 8 * (n + 1), 8), ("key", u["key"], 4 * n, 4)]
    if flags & O:
        p += [("pflags", u["pflags"], 4 * n, 4), ("pfrom", u["pfrom"], 4 * n, 4)]
    p.append(("bytes", u["bytes"], tb + 8, 1))
    if flags & A:
        p += [("mlen", u["mlen"], 4 * n, 4), ("padmit", u["padmit"], 4 * n, 4), ("coff", u["coff"], 8 * (n + 1), 8),
              ("uoff", u["uoff"], 8 * (n + 1), 8), ("access", u["access"], n, 1), ("cdef", u["cdef"], n, 1),
              ("udef", u["udef"], n, 1), ("fam", u["fam"], n, 1), ("peers", u["peers"], 16 * n, 1),
              ("cbytes", u["cbytes"], cred[0] + 8, 1), ("ubytes", u["ubytes"], cred[1] + 8, 1)]
        if mounted:
            p += [("utoff", u["utoff"], 8 * (n + 1), 8), ("utbytes", u["utbytes"], tb + 8, 1)]
    return p


def _pieces_down(d, flags, n, caps):
    """the same for the packed block; the pieces at or after backb stay on the device"""
    cap, scap = caps
    wb = 4 if flags & O else 0
    p = [("hdr", d["hdr"], 64, 16), ("doff", d["doff"], 8 * (n + 1), 8), ("sub_off", d["sub_off"], 8 * (n + 1), 8),
         ("deliv", d["deliv"], 16 * cap, 16)]
    pairs = [("pairs", d["pairs"], 8 * scap, 8), ("pairw", d["pairw"], wb * scap, 4)]
    pickw = [("pickw", d["pickw"], wb * cap, 4)]
    if flags & I:
        e = d["ecap"]
        assert e == cap + scap
        p += pickw + [("ihdr", d["ihdr"], 64, 16), ("inbox", d["inbox"], 16 * e, 16), ("epub", d["epub"], 4 * e, 4),
                      ("eto", d["eto"], 4 * e, 4), ("ewd", d["ewd"], 4 * e, 4)]
    else:
        p += [pairs[0]] + pickw + [pairs[1]]
    if flags & F:
        p += [("fhdr", d["fhdr"], 64, 16), ("fgroups", d["fgroups"], 16 * cap, 16), ("fpub", d["fpub"], 4 * cap, 4)]
    if flags & A:
        n8 = (n + 7) & ~7
        p += [("ahdr", d["ahdr"], 64, 16), ("rule", d["rule"], 4 * n, 4), ("code", d["code"], n, 1),
              ("aclres", d["aclres"], n8, 1)]
    if flags & I:
        p += pairs
    return p


def _in_order(pieces):
    at = 0
    for name, off, size, align in pieces:
        assert off >= at and off % align == 0, (name, off, at)
        at = off + size
    return at


def test_invariants(lib):
    for flags, n, caps, cred, mounted in cases():
        uv, dv = layout(lib, flags, n, caps, cred, mounted)
        u, d = dict(zip(UP, uv)), dict(zip(DOWN, dv))
        where = (flags, n, caps, cred, mounted)
        # the block that goes up: in order, disjoint, aligned, and `end` covers the last piece with its spare bytes
        up = _pieces_up(u, flags, n, cred, mounted)
        last = _in_order(up)
        assert u["end"] >= last, where
        if not flags & A:
            assert u["end"] == last and all(u[k] == 0 for k in UP[5:18]), where
        elif not mounted:
            assert u["utoff"] == 0 and u["utbytes"] == 0, where
        if not flags & O:
            assert u["pflags"] == 0 and u["pfrom"] == 0, where
        # the packed block
        down = _pieces_down(d, flags, n, caps)
        assert _in_order(down) <= d["outb"], where
        assert d["backb"] <= d["outb"] and d["deliv"] == 64 + 16 * (n + 1), where
        if flags & I:
            assert d["pairs"] >= d["backb"] and d["pairw"] >= d["backb"], where
            assert d["ewd"] + 4 * d["ecap"] <= d["backb"], where
        else:
            assert d["backb"] == d["outb"] and d["ecap"] == 0, where
        if flags & A:                                   # what comes back of the admission outputs: header, rules, codes
            assert d["a_back"] == d["aclres"] - d["ahdr"] and d["ahdr"] + d["a_back"] <= d["backb"], where
        for name, mode in (("ihdr", I), ("inbox", I), ("fhdr", F), ("fgroups", F), ("ahdr", A), ("rule", A)):
            assert (d[name] != 0) == bool(flags & mode), (name, where)


def test_equals_the_recorded_offsets(lib):
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batcher_layout.json")) as f:
        gold = json.load(f)
    assert gold["up_fields"] == UP and gold["down_fields"] == DOWN
    seen_up, seen_down = set(), set()
    for flags, n, caps, cred, mounted in cases():
        uv, dv = layout(lib, flags, n, caps, cred, mounted)
        ku, kd = up_key(flags, n, cred, mounted), down_key(flags, n, caps)
        assert uv == gold["up"][ku], (flags, n, cred, mounted)
        assert dv == gold["down"][kd], (flags, n, caps)
        seen_up.add(ku)
        seen_down.add(kd)
    assert seen_up == set(gold["up"]) and seen_down == set(gold["down"])
