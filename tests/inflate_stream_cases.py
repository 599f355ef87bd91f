"""Cases for the streaming inflate (include/mi355_deflate.h mi355_inflate_stream_*): seeded, shared by the CPU test of the host build
(test_inflate_stream_cases.py) and the GPU test (test_inflate_stream_gpu.py).  TEST INFRASTRUCTURE.

A case is a Script: a wrapper, a preset dictionary or None, and steps [(chunk, cap)] that one handle is driven through, a finish()
behind them.  run(handle, script) gives the trace -- per step the return value, the bytes handed over, the report, the state, the
canary -- and judge(script, trace) says what the trace must be:
  kind "valid"    the judge is zlib.decompressobj (wbits -15 / 15 / 31, zdict=) fed the same chunks: the bytes handed over
                  concatenate to zlib's; at every step that ends at a block end (found with the host build's own records,
                  inflstream_binding.block_ends, and every Z_SYNC_FLUSH point of the base streams is cross-checked to be one) total_out
                  equals what zlib has returned so far; the handle ends done, finish() is OK
  kind "prefix"   a proper prefix fed whole leaves the handle alive, and finish() says FRAME or TRUNCATED
  kind "fail"     the one-shot host build (tests/inflwrite) names the failure: status, bit, out_pos, and the bytes in front of it
  kind "explicit" want = per step (rc, bytes handed over or None, report status, need_out or None)
The BFINAL block of a framed stream counts as complete once its trailer is there (the header says so): the step that ends behind
it hands its bytes over, and zlib, which hands them out before the trailer, is compared at the trailer's end.
"""
import collections
import functools
import random
import struct
import zlib

import inflate_cases as icase
import inflstream_binding as sb
import inflwrite_binding as wb
import verify_cases as vc
from inflate_cases import fixed_open, put_lits, put_match, stored
from verify_cases import WBITS, BitWriter, fixed_ll

Script = collections.namedtuple("Script", "name cells wrapper zdict steps kind want gpu")
OK, E_DATA, E_OUT_TOO_SMALL, E_STATE = sb.OK, sb.E_DATA, sb.E_OUT_TOO_SMALL, sb.E_STATE
CELLS = [
    "split2:raw", "split2:zlib", "split2:gzip", "split2:oracle", "bytewise:raw", "bytewise:zlib", "bytewise:gzip", "random_splits",
    "prefix:raw", "prefix:zlib", "prefix:gzip", "hist:dist_1", "hist:dist_hist_len", "hist:dist_hist_len_plus_1", "hist:straddle",
    "hist:len_gt_dist_seam", "hist:dist_32768", "hist:dist_32769", "hist:short_history_distance",
    "update:0", "update:1", "update:32767", "update:32768", "update:32769", "update:70000", "update:5x10000", "update:empty_stored_between",
    "room:exact", "room:one_less", "room:zero", "room:too_small_then_need_out", "room:first_of_two",
    "dict:1", "dict:32768", "dict:40000", "dict:missing", "fail:one_piece", "fail:two_pieces", "checksum:adler", "checksum:crc",
    "checksum:isize", "trailer:same_write", "trailer:after_done", "finish:frame", "finish:truncated", "reset",
]


# ---- the base streams ------------------------------------------------------------------------------------------------------------
GZ_HEADER = bytes([0x1f, 0x8b, 8, 2 | 4 | 8, 1, 2, 3, 4, 0, 3]) + struct.pack("<H", 5) + b"AB\x01\x00z" + b"name.txt\0"
GZ_HEADER += struct.pack("<H", zlib.crc32(GZ_HEADER) & 0xFFFF)  # FEXTRA + FNAME + FHCRC


def _seg(data, level, strategy, how):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(data) + c.flush(how)


@functools.lru_cache(maxsize=None)
def composite():
    """(raw stream, data, sync points): a dynamic block, a fixed one (Z_FIXED), a stored one and a dynamic BFINAL one, an empty stored
    block (the sync marker) behind each of the first three; the segments are independent raw streams that end on a byte"""
    t = vc.pg11()
    parts = [(t[1000:1420], 6, zlib.Z_DEFAULT_STRATEGY), (t[3000:3220], 6, zlib.Z_FIXED), (t[5000:5120], 0, zlib.Z_DEFAULT_STRATEGY)]
    raw, data, syncs = b"", b"", []
    for d, level, strategy in parts:
        raw += _seg(d, level, strategy, zlib.Z_SYNC_FLUSH)
        data += d
        syncs.append((len(raw), len(data)))
    raw += _seg(t[7000:7450], 6, zlib.Z_DEFAULT_STRATEGY, zlib.Z_FINISH)
    data += t[7000:7450]
    _rc, _n, rep, _buf, _ok = wb.inflate(raw, 0, len(data))
    assert rep["status"] == "OK" and rep["n_dynamic"] >= 2 and rep["n_fixed"] >= 1 and rep["n_stored"] >= 4, rep
    assert 300 <= len(raw) <= 900, len(raw)
    return raw, data, syncs


def frame(raw, data, wrapper):
    if wrapper == 1:
        return b"\x78\x9c" + raw + struct.pack(">I", zlib.adler32(data) & 0xFFFFFFFF)
    return vc.gzip_frame(raw, data, GZ_HEADER) if wrapper == 2 else raw


def hdr_len(wrapper):
    return (0, 2, len(GZ_HEADER))[wrapper]


@functools.lru_cache(maxsize=None)
def oracle_stream():
    """a raw stream of the oracle at Default, 300 to 900 bytes"""
    import oracle_binding as ob

    data = vc.pg11()[9000:10400]
    raw = ob.encode(data, level=ob.DEFAULT)
    assert 300 <= len(raw) <= 900, len(raw)
    return raw, data


@functools.lru_cache(maxsize=None)
def bases():
    """[(tag, stream, wrapper, data)]"""
    raw, data, _ = composite()
    oraw, odata = oracle_stream()
    return [("raw", raw, 0, data), ("zlib", frame(raw, data, 1), 1, data), ("gzip", frame(raw, data, 2), 2, data), ("oracle", oraw, 0, odata)]


def room(data):
    return len(data) + 64


def cut(stream, cuts, cap):
    at = [0] + list(cuts) + [len(stream)]
    return [(stream[a:b], cap) for a, b in zip(at, at[1:])]


# ---- hand-assembled history streams ---------------------------------------------------------------------------------------------
def stored_run(w, data):
    """non-final stored blocks holding data (an empty one for no data)"""
    if not data:
        return stored(w, b"")
    for a in range(0, len(data), 65535):
        stored(w, data[a:a + 65535])
    return w


def hist_script(name, cells, commits, tail, seed, want_fail=False, gpu=True):
    """writes that commit commits[k] random bytes each (stored blocks), then one write with a BFINAL fixed block made by tail(w, total)"""
    rnd = random.Random(seed)
    steps, total, w = [], 0, BitWriter()
    biggest = max(commits + [0]) + 4096
    for n in commits:
        before = len(w.bytes())
        stored_run(w, bytes(rnd.getrandbits(8) for _ in range(n)))
        total += n
        steps.append((before, biggest))
    before = len(w.bytes())
    tail(fixed_open(w, 1), total)
    fixed_ll(w, 256)
    s = w.bytes()
    at = [b for b, _ in steps] + [before, len(s)]
    steps = [(s[a:b], biggest) for a, b in zip(at, at[1:])]
    if want_fail:
        return Script(name, cells, 0, None, steps, "fail", s, gpu)
    return Script(name, cells, 0, None, steps, "valid", s, gpu)


def _tail_matches(*pairs):
    """tail: pairs of (literals in front, length, distance or a function of the total)"""
    def tail(w, total):
        for nlit, length, dist in pairs:
            put_lits(w, bytes((37 * k + 11) & 255 for k in range(nlit)))
            put_match(w, length, dist(total) if callable(dist) else dist)
    return tail


# ---- all scripts ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scripts():
    out = []
    rnd = random.Random(20250611)
    # two-piece splits at every byte, bytewise, random splits, prefixes
    for tag, s, w, data in bases():
        every = tag != "oracle"
        for k in range(1, len(s)):
            out.append(Script("split2:%s@%d" % (tag, k), ["split2:" + tag], w, None, cut(s, [k], room(data)), "valid", s, every or k % 7 == 0))
        if tag != "oracle":
            out.append(Script("bytewise:" + tag, ["bytewise:" + tag], w, None, cut(s, range(1, len(s)), room(data)), "valid", s, True))
            for k in range(1, len(s)):
                out.append(Script("prefix:%s@%d" % (tag, k), ["prefix:" + tag], w, None, [(s[:k], room(data))], "prefix", s, k % 5 == 0 or k < 40))
        for j in range(6):
            cuts = sorted(rnd.sample(range(1, len(s)), rnd.randint(2, 8)))
            out.append(Script("random:%s#%d" % (tag, j), ["random_splits"], w, None, cut(s, cuts, room(data)), "valid", s, True))
    # history: a first write of 1000 bytes (hist_len 1000), then matches counted from the start of the later write
    H = 1000
    out.append(hist_script("hist:dist_1", ["hist:dist_1"], [H], _tail_matches((0, 10, 1)), 1))
    out.append(hist_script("hist:dist_hist_len", ["hist:dist_hist_len"], [H], _tail_matches((0, 20, H)), 2))
    out.append(hist_script("hist:dist_hist_len_plus_1", ["hist:dist_hist_len_plus_1"], [H], _tail_matches((1, 30, H + 1)), 3))
    out.append(hist_script("hist:straddle", ["hist:straddle"], [H], _tail_matches((4, 9, 10), (0, 70, 75)), 4))
    out.append(hist_script("hist:len_gt_dist_seam", ["hist:len_gt_dist_seam"], [H], _tail_matches((2, 30, 5), (0, 258, 33)), 5))
    out.append(hist_script("hist:dist_32768", ["hist:dist_32768", "update:32768"], [32768], _tail_matches((0, 258, 32768), (3, 5, 32768)), 6))
    out.append(hist_script("hist:dist_32769", ["hist:dist_32769"], [32767], _tail_matches((0, 3, 32768)), 7, want_fail=True))
    out.append(hist_script("hist:short_history", ["hist:short_history_distance"], [10], _tail_matches((0, 3, 11)), 8, want_fail=True))
    out.append(hist_script("hist:short_history_equal", ["hist:short_history_distance"], [10], _tail_matches((2, 3, 13)), 9, want_fail=True))
    # history update: a second commit of n bytes behind 1000, then matches that read the oldest and the newest byte it must hold
    far = lambda total: min(total, 32768)
    for n in (0, 1, 32767, 32769, 70000):
        out.append(hist_script("update:%d" % n, ["update:%d" % n], [H, n], _tail_matches((0, 258, far), (1, 40, 1), (0, 7, lambda t: min(t, 32768) // 2 + 1)), 10 + n))
    out.append(hist_script("update:5x10000", ["update:5x10000"], [10000] * 5, _tail_matches((0, 258, 32768), (0, 258, 32768)), 20))
    out.append(hist_script("update:empty_between", ["update:empty_stored_between"], [500, 0, 300], _tail_matches((0, 100, 800), (0, 5, 1)), 21))
    # room
    raw, data, _syncs = composite()
    ends = sb.block_ends(raw, 0, len(data))
    assert all(dict(ends).get(k) == o for k, o in _syncs), (ends, _syncs)  # every Z_SYNC_FLUSH point is a block end
    (k1, o1), (k2, o2) = next((a, b) for a, b in zip(ends, ends[1:]) if a[1] > 0 and b[1] > a[1])
    rest = [(raw[k2:], room(data))]
    big = room(data)
    out.append(Script("room:exact", ["room:exact"], 0, None, [(raw[:k1], o1)] + [(raw[k1:], big)], "explicit",
                      [(OK, data[:o1], "OK", 0), (OK, data[o1:], "OK", 0)], True))
    for name, cap in (("room:one_less", o1 - 1), ("room:zero", 0)):
        out.append(Script(name, [name, "room:too_small_then_need_out"], 0, None, [(raw[:k1], cap), (b"", o1), (raw[k1:], big)], "explicit",
                          [(E_OUT_TOO_SMALL, b"", "OK", o1), (OK, data[:o1], "OK", 0), (OK, data[o1:], "OK", 0)], True))
    out.append(Script("room:first_of_two", ["room:first_of_two"], 0, None, [(raw[:k2], o1), (b"", o2 - o1)] + rest, "explicit",
                      [(OK, data[:o1], "OK", o2 - o1), (OK, data[o1:o2], "OK", 0), (OK, data[o2:], "OK", 0)], True))
    # dictionary: the first token a match into it, hand-assembled, and a stream zlib made against it
    for n in (1, 32768, 40000):
        zd = bytes(random.Random(30 + n).getrandbits(8) for _ in range(n))
        w = fixed_open(BitWriter(), 1)
        put_match(w, 20, min(n, 32768))
        put_match(put_lits(w, b"xy"), 9, 1)
        s = fixed_ll(w, 256).bytes()
        out.append(Script("dict:%d:hand" % n, ["dict:%d" % n], 0, zd, cut(s, [1], 4096), "valid", s, True))
        out.append(Script("dict:%d:missing" % n, ["dict:missing"], 0, None, cut(s, [], 4096), "fail", s, True))
        if n > 1:
            c = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_DEFAULT_STRATEGY, zd)
            payload = zd[-300:] + b" and then something new " + zd[:200]
            s = c.compress(payload) + c.flush()
            out.append(Script("dict:%d:zlib" % n, ["dict:%d" % n], 0, zd, cut(s, [len(s) // 2], 4096), "valid", s, True))
    # failures: the mutated streams of inflate_cases whose failing element lies wholly in front of the last 8 bytes
    for c in icase.corpus():
        if c.group != "mutations" or c.want is not None:
            continue
        _rc, _n, rep, _buf, _ok = wb.inflate(c.stream, c.wrapper, 0)
        if rep["status"] in ("OK", "FRAME", "TRUNCATED", "TRAILER", "CHECKSUM"):
            continue
        margin = 600 if rep["status"] == "LENGTHS" else 8  # (a dynamic header is at most 4 451 bits long)
        at = hdr_len(c.wrapper) + rep["bit"] // 8
        if at + margin > len(c.stream) - 8:
            continue
        big = rep["out_pos"] + 4096
        out.append(Script("fail1:" + c.name, ["fail:one_piece"], c.wrapper, None, [(c.stream, big)], "fail", c.stream, True))
        for d in (0, 1):
            out.append(Script("fail2+%d:%s" % (d, c.name), ["fail:two_pieces"], c.wrapper, None, cut(c.stream, [at + d], big), "fail", c.stream, d == 0))
    # checksums, at the write that completes the trailer; bytes behind the end
    zs, gs = frame(raw, data, 1), frame(raw, data, 2)
    last_commit = ends[-2][1]
    for name, s, w in (("checksum:adler", zs[:-1] + bytes([zs[-1] ^ 1]), 1), ("checksum:crc", gs[:-8] + bytes([gs[-8] ^ 1]) + gs[-7:], 2),
                       ("checksum:isize", gs[:-1] + bytes([gs[-1] ^ 1]), 2)):
        out.append(Script(name, [name], w, None, cut(s, [len(s) - 1], room(data)), "explicit",
                          [(OK, data[:last_commit], "OK", 0), (E_DATA, data[last_commit:], "CHECKSUM", 0)], True))
    for tag, s, w, d in bases()[:3]:
        out.append(Script("trailer:same_write:" + tag, ["trailer:same_write"], w, None, [(s + b"\0", room(d))], "explicit",
                          [(E_DATA, d, "TRAILER", 0)], True))
        out.append(Script("trailer:after_done:" + tag, ["trailer:after_done"], w, None, [(s, room(d)), (b"", 0), (b"\0", 16), (b"", 0)], "explicit",
                          [(OK, d, "OK", 0), (OK, b"", "OK", 0), (E_DATA, b"", "TRAILER", 0), (E_STATE, b"", "OK", 0)], True))
        out.append(Script("finish:frame:" + tag, ["finish:frame"] if w else ["finish:truncated"], w, None, [(s[:1], 64)], "prefix", s, True))
        out.append(Script("finish:truncated:" + tag, ["finish:truncated"], w, None, [(s[:hdr_len(w) + 40], room(d))], "prefix", s, True))
        out.append(Script("reset:" + tag, ["reset"], w, None, cut(s, [len(s) // 3], room(d)), "reset", s, True))
    return out


def coverage():
    got = set()
    for s in scripts():
        got.update(s.cells)
    return got


assert set(CELLS) <= coverage(), sorted(set(CELLS) - coverage())


# ---- driving a handle and judging what it did ---------------------------------------------------------------------------------------
def run(h, script):
    """h: inflstream_binding.Model, or anything with its methods.  The trace: per step (rc, bytes handed over, report, state, canary
    intact), then ("finish", rc, report, state)"""
    trace = []
    for chunk, cap in script.steps:
        rc, data, rep, ok = h.write(chunk, cap)
        trace.append((rc, data, rep, h.state(), ok))
    rc, rep = h.finish()
    trace.append(("finish", rc, rep, h.state()))
    if script.kind == "reset":
        h.reset()
        trace.append(("reset", h.state()))
        for chunk, cap in script.steps:
            rc, data, rep, ok = h.write(chunk, cap)
            trace.append((rc, data, rep, h.state(), ok))
    return trace


@functools.lru_cache(maxsize=None)
def _ends(stream, wrapper, total, zdict):
    return dict(sb.block_ends(stream, wrapper, total, zdict))


def one_shot_failure(stream, wrapper):
    """what the one-shot host build says of a stream that fails: (report, the bytes in front of the failing element)"""
    _rc, _n, rep, _buf, _ok = wb.inflate(stream, wrapper, 0)
    rc, n, rep, buf, _ok = wb.inflate(stream, wrapper, max(rep["out_pos"], 1))
    assert rc == E_DATA and n == rep["out_pos"], (rc, n, rep)
    return rep, buf[:n]


def judge(script, trace):
    """asserts that the trace is what the script must give"""
    steps, fin = trace[:len(script.steps)], trace[len(script.steps)]
    assert all(t[4] for t in steps), "canary"
    got = b"".join(t[1] for t in steps)
    fed = sum(len(c) for c, _ in script.steps)
    if script.kind in ("valid", "reset"):
        d = zlib.decompressobj(WBITS[script.wrapper], **({"zdict": script.zdict} if script.zdict else {}))
        want, at = b"", 0
        ends = _ends(script.want, script.wrapper, 200000, script.zdict) if len(script.want) < 4096 else {}
        every = script.name.startswith(("hist:", "update:"))  # (every step of these ends at a block end)
        for (chunk, _cap), (rc, _data, rep, st, _ok) in zip(script.steps, steps):
            want += d.decompress(chunk)
            at += len(chunk)
            assert rc == OK and rep["status"] == "OK" and st["failed"] == "OK", (script.name, at, rc, rep, st)
            assert st["total_in"] == at and rep["out_pos"] == st["total_out"] and st["need_out"] == 0
            assert want.startswith(got[:st["total_out"]]) and st["total_out"] <= len(want)
            if every or at in ends or at == len(script.want):
                assert st["total_out"] == len(want), (script.name, at, st, len(want))
        assert got == want and d.eof and steps[-1][3]["done"] == 1, (script.name, len(got), len(want))
        assert steps[-1][3]["pending_in"] == 0
        if script.wrapper:
            assert steps[-1][3]["adler_or_crc"] == (zlib.adler32(want) if script.wrapper == 1 else zlib.crc32(want)) & 0xFFFFFFFF
        assert fin[1] == OK, fin
        if script.kind == "reset":
            again = trace[len(script.steps) + 2:]
            assert trace[len(script.steps) + 1][1] == dict(steps[0][3], total_in=0, total_out=0, pending_in=0, need_out=0, done=0, adler_or_crc=1 if script.wrapper == 1 else 0)
            assert [t[:4] for t in again] == [t[:4] for t in steps], script.name
    elif script.kind == "prefix":
        (rc, data, rep, st, _ok), = steps
        d = zlib.decompressobj(WBITS[script.wrapper])
        want = d.decompress(script.steps[0][0])
        assert rc == OK and st["failed"] == "OK" and st["done"] == 0 and rep["status"] == "OK", (script.name, rc, rep, st)
        assert want.startswith(data) and st["total_out"] == len(data) and st["total_in"] == fed
        assert fin[1] == E_DATA and fin[3]["failed"] == fin[2]["status"], fin
        assert fin[2]["status"] == ("FRAME" if fed < hdr_len(script.wrapper) else "TRUNCATED"), (script.name, fin)
        if script.wrapper == 0:
            _rc, _n, one, _buf, _ok2 = wb.inflate(script.steps[0][0], 0, 0)
            assert (one["status"], one["bit"], one["out_pos"]) == (fin[2]["status"], fin[2]["bit"], fin[2]["out_pos"]), (script.name, one, fin)
    elif script.kind == "fail":
        one, front = one_shot_failure(script.want, script.wrapper)
        failed = [k for k, t in enumerate(steps) if t[0] != OK]
        assert failed and steps[failed[0]][0] == E_DATA, (script.name, [t[0] for t in steps])
        rc, _data, rep, st, _ok = steps[failed[0]]
        assert (rep["status"], rep["bit"], rep["out_pos"]) == (one["status"], one["bit"], one["out_pos"]), (script.name, rep, one)
        assert got == front, (script.name, len(got), len(front))
        assert st["failed"] == one["status"] and st["total_out"] == len(front)
        assert all(t[0] == E_STATE and t[1] == b"" for t in steps[failed[0] + 1:]) and fin[1] == E_STATE, script.name
    else:
        assert len(script.want) == len(steps)
        for k, ((rc, data, status, need), t) in enumerate(zip(script.want, steps)):
            assert (t[0], t[2]["status"]) == (rc, status), (script.name, k, t[0], t[2], t[3])
            assert t[1] == data, (script.name, k, len(t[1]), len(data))
            assert t[3]["need_out"] == need, (script.name, k, t[3])
            assert t[0] == E_STATE or t[2]["out_pos"] == t[3]["total_out"] or t[0] == E_DATA
        last = steps[-1]
        assert fin[1] == (OK if last[3]["done"] and last[3]["failed"] == "OK" else E_STATE if last[3]["failed"] != "OK" else E_DATA), (script.name, fin)


def fuzz_corpus():
    """(stream, wrapper, zdict, [(piece length, cap)]) of every script whose steps are its stream cut in pieces"""
    for k, s in enumerate(scripts()):
        if s.kind == "reset" or b"".join(c for c, _ in s.steps) != s.want:
            continue
        if s.name.startswith(("split2:", "prefix:", "fail")) and k % 4:  # (thinned: the program runs under a sanitizer)
            continue
        yield s.want, s.wrapper, s.zdict, [(len(c), cap) for c, cap in s.steps]
