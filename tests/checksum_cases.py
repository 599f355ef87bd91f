"""Cases, references and a model for the checksum kernels (deflate_kernels.hip k_adler_part / k_adler_fold, k_crc_part / k_crc_fold;
deflate_batch.inc kb_adler_part / kb_crc over the same body text body_k_adler_part.inc / body_k_crc_part.inc), shared by the CPU
test (test_checksum_cases.py) and the GPU test (test_checksum_gpu.py).  TEST INFRASTRUCTURE; everything is generated from fixed
seeds, no data file is committed.

The sizes come from the kernels, not from a workload -- each constant with what it is in the kernels:
  16                 a thread's piece of k_adler_part, and a lane's load of the CRC staging
  4096               one round of the Adler workgroup (256 threads x 16 bytes)
  ADLER_CHUNK 16384  a workgroup of k_adler_part (four rounds); `after` = the bytes behind a chunk, reduced mod 65521
  CRC_PIECE 128      a thread's bytes per staging round     CRC_CHUNK 512   a thread's chunk (four pieces)
  32768              the 64 chunks of a wave                131072          the 256 chunks of a workgroup (a tile)
They are read from deflate_kernels.hip below: the lists are built on 16384 / 512 / 128 and must be rebuilt if those change.

A case is a buffer of n bytes of one pattern inside an arena: GUARD bytes of 0xEE in front and behind, its first byte at a chosen
offset from a 32-byte boundary (offset 16: 16-byte aligned, but not where offset 0 sits).  An arena holds every case of one
(kind, family); a test uploads it once and addresses the cases by pointer.

The models repeat the kernels' partition and arithmetic in numpy, with 32-bit wraparound where the kernel computes in uint32_t,
and read the arena through the kernel's bounds tests.  A mutant is the model with one rule wrong; every mutant must be noticed by
a case of the lists (test_checksum_cases.py), so that a kernel wrong in that rule fails the GPU test.
"""
import collections
import functools
import os
import re
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KERNELS = os.path.join(ROOT, "deflate-rs_amd", "csrc", "deflate_kernels.hip")


def kernel_constants():
    with open(KERNELS) as f:
        src = f.read()
    out = {}
    for name in ("ADLER_CHUNK", "CRC_CHUNK", "CRC_PIECE"):
        m = re.findall(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)\s*;" % name, src)
        if len(m) != 1:
            raise AssertionError("deflate_kernels.hip: %s is defined %d times" % (name, len(m)))
        out[name] = int(m[0])
    return out


_K = kernel_constants()
if (_K["ADLER_CHUNK"], _K["CRC_CHUNK"], _K["CRC_PIECE"]) != (16384, 512, 128):
    raise AssertionError("checksum_cases.py is built on ADLER_CHUNK 16384, CRC_CHUNK 512, CRC_PIECE 128; the kernels have %r: rebuild "
                         "ADLER_SIZES, CRC_SIZES and UNITS" % (_K,))
ADLER_CHUNK, CRC_CHUNK, CRC_PIECE = 16384, 512, 128
CRC_TILE = 256 * CRC_CHUNK
BASE = 65521
CRC_POLY = 0xEDB88320

# ---- the lists ---------------------------------------------------------------------------------------------------------------------------
ADLER_SIZES = ([0, 1, 15, 16, 17, 31, 4095, 4096, 4097, 4111, 4112, 8192, 12287, 12288, 12289, 16383, 16384, 16385, 16400, 32767, 32768,
                32769, 49153]
               + list(range(ADLER_CHUNK + BASE - 2, ADLER_CHUNK + BASE + 3))               # `after` of chunk 0 at 65519 .. 65523
               + list(range(2 * ADLER_CHUNK + BASE, 2 * ADLER_CHUNK + BASE + 3))           # ... of chunk 1 at 65521 .. 65523
               + list(range(ADLER_CHUNK + 2 * BASE, ADLER_CHUNK + 2 * BASE + 3)))          # ... of chunk 0 at 2 * 65521 .. + 2
CRC_SIZES = [0, 1, 3, 4, 5, 15, 16, 17, 127, 128, 129, 131, 255, 256, 257, 383, 384, 385, 511, 512, 513, 515, 1023, 1024, 1025,
             32767, 32768, 32769, 131071, 131072, 131073, 131075, 262143, 262144, 262145, 393217]
assert ADLER_SIZES[23:] == [81903, 81904, 81905, 81906, 81907, 98289, 98290, 98291, 147426, 147427, 147428]
SIZES = {"adler": ADLER_SIZES, "crc": CRC_SIZES}
OFFSETS = (0, 1, 3, 4, 8, 15, 16)
FAMILIES = ("zeros", "ff", "ramp", "random", "onehot", "hot")
UNITS = (16, 128, 512, 4096, 16384)
HOT_CHUNKS = (0, 63, 64, 255, 256)  # and the last
GUARD, GUARD_BYTE = 64, 0xEE
MAX_PATTERN = 400 * 1000

Case = collections.namedtuple("Case", "kind family detail n off at")  # detail: the hot byte / the hot chunk; at: its place in the arena


def case_id(c):
    return "%s-%s%s-n%d-off%d" % (c.kind, c.family, "" if c.detail is None else "@%d" % c.detail, c.n, c.off)


def onehot_positions(n):
    """the first and last byte of the buffer and of the 16-, 128-, 512-, 4096- and 16384-byte units next to the end of n bytes: the
    unit that holds byte n - 1 and the one in front of it"""
    js = {0, n - 1}
    for u in UNITS:
        e = (n - 1) // u * u
        js |= {e - u, e - 1, e}
    return sorted(j for j in js if 0 <= j < n)


def hot_chunks(n):
    nch = -(-n // CRC_CHUNK)
    return sorted({c for c in HOT_CHUNKS + (nch - 1,) if 0 <= c < nch})


def details(family, n):
    if family == "onehot":
        return onehot_positions(n)
    if family == "hot":
        return hot_chunks(n)
    return [None]


def pattern(family, detail, n):
    """the n bytes of a case"""
    assert n <= MAX_PATTERN
    if family == "zeros":
        return np.zeros(n, np.uint8)
    if family == "ff":
        return np.full(n, 0xFF, np.uint8)
    if family == "ramp":
        return (np.arange(n) & 0xFF).astype(np.uint8)
    if family == "random":
        return np.random.default_rng(1000003 + n).integers(0, 256, n, dtype=np.uint8)
    d = np.zeros(n, np.uint8)
    if family == "onehot":
        d[detail] = 0xFF
    elif family == "hot":
        lo, hi = detail * CRC_CHUNK, min(n, (detail + 1) * CRC_CHUNK)
        d[lo:hi] = np.random.default_rng(7 * n + detail).integers(1, 256, hi - lo, dtype=np.uint8)
    else:
        raise ValueError(family)
    return d


def build_arena(specs, kind="any", align=32):
    """specs: (family, detail, n, off).  Returns (arena, cases): every buffer with at least GUARD bytes of GUARD_BYTE on both sides,
    its first byte at `off` behind a multiple of `align`.  The arena's own first byte is taken to lie on such a multiple."""
    cases, cur = [], 0
    for family, detail, n, off in specs:
        at = cur + GUARD
        at += (off - at) % align
        cases.append(Case(kind, family, detail, n, off, at))
        cur = at + n
    buf = np.full(cur + GUARD + align, GUARD_BYTE, np.uint8)
    for c in cases:
        buf[c.at:c.at + c.n] = pattern(c.family, c.detail, c.n)
    return buf, cases


def specs(kind, family, offsets=OFFSETS):
    return [(family, d, n, off) for n in SIZES[kind] for d in details(family, n) for off in offsets]


def arena(kind, family, offsets=OFFSETS):
    """every case of one kind and family -- sizes x details x offsets -- in one arena"""
    return build_arena(specs(kind, family, offsets), kind)


def case_bytes(buf, c):
    return buf[c.at:c.at + c.n].tobytes()


def reference(kind, data):
    return (zlib.adler32(data) if kind == "adler" else zlib.crc32(data)) & 0xFFFFFFFF


# ---- references in Python integers -------------------------------------------------------------------------------------------------------
def adler_const(n, v):
    """Adler-32 of n bytes of value v: a_i = 1 + i v after i bytes, b = the sum of a_1 .. a_n"""
    return ((n + v * n * (n + 1) // 2) % BASE) << 16 | (1 + n * v) % BASE


def adler_combine_ref(s1, s2, len2):
    """Adler-32 of A || B.  a = 1 + sum of the bytes; b = the sum of a over the positions: behind A every step of B's own b runs
    with a higher by a1 - 1"""
    a1, b1, a2, b2 = s1 & 0xFFFF, s1 >> 16, s2 & 0xFFFF, s2 >> 16
    return ((b1 + b2 + len2 * (a1 - 1)) % BASE) << 16 | (a1 + a2 - 1) % BASE


_P = 0x104C11DB7  # x^32 + x^26 + ... + 1, bit k = the coefficient of x^k


def _rev32(x):
    return int("{:032b}".format(x)[::-1], 2)


def _pmod(a):
    while a.bit_length() > 32:
        a ^= _P << (a.bit_length() - 33)
    return a


def _pmul(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        a <<= 1
        b >>= 1
    return _pmod(r)


def _xpow(e):
    r, s = 1, 2
    while e:
        if e & 1:
            r = _pmul(r, s)
        s = _pmul(s, s)
        e >>= 1
    return r


def crc_combine_ref(c1, c2, len2):
    """crc(A || B) = x^(8|B|) crc(A) + crc(B) over GF(2)[x] mod P.  A CRC-32 value holds the coefficient of x^k in bit 31 - k."""
    return _rev32(_pmul(_xpow(8 * len2), _rev32(c1))) ^ c2


@functools.lru_cache(maxsize=None)
def _crc_mib(v):
    return zlib.crc32(bytes([v]) * (1 << 20))


def crc_const(n, v):
    """CRC-32 of n bytes of value v: zlib's CRC of 1 MiB, doubled with crc_combine_ref up to the bits of n >> 20, and the rest"""
    acc, c, ln, q = 0, _crc_mib(v), 1 << 20, n >> 20
    while q:
        if q & 1:
            acc = crc_combine_ref(acc, c, ln)
        c = crc_combine_ref(c, c, ln)
        ln *= 2
        q >>= 1
    rest = n & ((1 << 20) - 1)
    return crc_combine_ref(acc, zlib.crc32(bytes([v]) * rest), rest)


# ---- the model of k_adler_part / k_adler_fold ------------------------------------------------------------------------------------------
ADLER_MUTANTS = {
    "adler_len_is_chunk": "(len - o) with ADLER_CHUNK for len",
    "adler_w_from_one": "w weighted k + 1",
    "adler_tail_unmasked": "the tail piece read without the o + k < len mask",
    "adler_no_thread_mod": "the per-thread b %= 65521 dropped",
    "adler_after_from_start": "after taken from the chunk's start",
    "adler_fold_without_n": "the n of the fold dropped",
    "adler_after_a_32bit": "after * A not reduced and computed in 32 bits",
}


def model_adler(buf, off, n, mutant=None, stray=None):
    """Adler-32 of buf[off : off + n) as k_adler_part and k_adler_fold compute it.  stray: a list that gets the number of bytes read
    outside the n bytes.  (The uint4 load and the byte loads of a piece give the same sixteen values; which of them runs is decided
    by (off & 15) == 0 and o + 16 <= len, and the tail piece of the call always takes the byte loads.)"""
    assert mutant is None or mutant in ADLER_MUTANTS
    nch = -(-n // ADLER_CHUNK)
    sum_a = sum_b = 0  # sc->adler_a, sc->adler_b: 64-bit, no wrap below 2^64
    read = n
    if nch:
        if mutant == "adler_tail_unmasked":
            read = -(-n // 16) * 16  # (`if (o >= len) break` stays: whole pieces behind len are not read)
        d = np.zeros(nch * ADLER_CHUNK, np.uint32)
        d[:read] = buf[off:off + read]
        d = d.reshape(nch, ADLER_CHUNK // 4096, 256, 16)  # [chunk, round i, tid, k]
        k = np.arange(16, dtype=np.uint32)
        s = d.sum(axis=3, dtype=np.uint32)
        w = (d * (k + 1 if mutant == "adler_w_from_one" else k)).sum(axis=3, dtype=np.uint32)
        c0 = np.arange(nch, dtype=np.int64) * ADLER_CHUNK
        ln = np.minimum(n - c0, ADLER_CHUNK).astype(np.uint32).reshape(nch, 1, 1)
        o = (np.arange(ADLER_CHUNK // 16, dtype=np.uint32) * 16).reshape(1, ADLER_CHUNK // 4096, 256)
        live = o < ln
        first = np.uint32(ADLER_CHUNK) if mutant == "adler_len_is_chunk" else ln
        term = np.where(live, (first - o) * s - w, np.uint32(0)).astype(np.uint32)  # uint32_t arithmetic, wraps
        a = np.where(live, s, np.uint32(0)).sum(axis=1, dtype=np.uint32)  # per thread, [chunk, tid]
        b = term.sum(axis=1, dtype=np.uint32)
        if mutant != "adler_no_thread_mod":
            b = b % np.uint32(BASE)
        wa = a.reshape(nch, 4, 64).sum(axis=2, dtype=np.uint32)  # the wave's shuffles: uint32_t
        wb = b.reshape(nch, 4, 64).sum(axis=2, dtype=np.uint32)
        for c in range(nch):
            A = sum(int(x) for x in wa[c]) % BASE  # tid 0: 64-bit
            B = sum(int(x) for x in wb[c]) % BASE
            after = n - int(c0[c]) - (0 if mutant == "adler_after_from_start" else int(ln[c, 0, 0]))
            aa = (after * A) & 0xFFFFFFFF if mutant == "adler_after_a_32bit" else (after % BASE) * A
            sum_a += A
            sum_b += (B + aa) % BASE
    if stray is not None:
        stray.append(read - n)
    n32 = n & 0xFFFFFFFF
    a = (1 + sum_a) % BASE
    b = ((0 if mutant == "adler_fold_without_n" else n32) + sum_b) % BASE
    return b << 16 | a


# ---- the model of k_crc_part / k_crc_fold and kb_crc -----------------------------------------------------------------------------------
CRC_MUTANTS = {
    "crc_after_tile_end": "after taken from the tile's end",
    "crc_after_full_chunk": "after taken from CRC_CHUNK instead of mylen for the last chunk",
    "crc_no_tail_bytes": "the tail bytes of a piece skipped",
    "crc_here_without_done": "here computed without the done offset",
    "crc_skip_zero_register": "a chunk with crc == 0 before the complement skipped instead of mylen == 0",
    "crc_stage_unmasked": "staging read without the g + b < n mask",
}


def _mulmod(a, b):
    """a(x) b(x) mod P, reflected (bit 31 = x^0), on Python integers -- crc_mulmod of the kernels"""
    p = 0
    for _ in range(32):
        if a & 0x80000000:
            p ^= b
        a = (a << 1) & 0xFFFFFFFF
        b = (b >> 1) ^ (CRC_POLY if b & 1 else 0)
    return p


def _vmulmod(a, b):
    """the same on uint32 arrays"""
    a, b = a.astype(np.uint32), b.astype(np.uint32)
    p = np.zeros(a.shape, np.uint32)
    poly = np.uint32(CRC_POLY)
    for _ in range(32):
        p ^= b * (a >> np.uint32(31))
        a = a << np.uint32(1)
        b = (b >> np.uint32(1)) ^ (poly * (b & np.uint32(1)))
    return p


@functools.lru_cache(maxsize=None)
def _tables():
    t0 = np.zeros(256, np.uint32)
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ (CRC_POLY if c & 1 else 0)
        t0[i] = c
    T = [t0]
    for _ in range(3):
        v = T[-1]
        T.append((v >> np.uint32(8)) ^ t0[v & np.uint32(0xFF)])
    # x^(8 * byte * 256^k) for the eight bytes of a 64-bit `after`: crc_xpow8's squarings, eight at a time
    pw, base = [], 0x00800000  # x^8
    for _ in range(8):
        row = [0x80000000]
        for _ in range(255):
            row.append(_mulmod(row[-1], base))
        pw.append(np.array(row, np.uint32))
        base = _mulmod(row[-1], base)  # base^256
    return T, pw


def _vxpow8(after):
    """x^(8 * after) mod P for a uint64 array"""
    _, pw = _tables()
    r = pw[0][(after & np.uint64(0xFF)).astype(np.int64)]
    for k in range(1, 8):
        byte = ((after >> np.uint64(8 * k)) & np.uint64(0xFF)).astype(np.int64)
        if byte.any():
            r = _vmulmod(r, pw[k][byte])
    return r


def model_crc_many(buf, items, mutant=None, stray=None):
    """CRC-32 of buf[off : off + n) for every (off, n) of items, as k_crc_part + k_crc_fold and kb_crc compute it: the chunks of all
    items side by side in one set of arrays, a row a thread.  (A thread with mylen == 0 keeps the register 0xFFFFFFFF and adds
    ~crc = 0 or nothing: it is left out here.  The two kernel forms differ in where `after` is worked out, not in its value.)"""
    assert mutant is None or mutant in CRC_MUTANTS
    T, _ = _tables()
    rows, mylen, after, start = [], [], [], []
    total = 0
    for off, n in items:
        nch = -(-n // CRC_CHUNK)
        start.append(total)
        total += nch
        read = n
        if nch:
            tiles = -(-nch // 256)
            d = np.zeros(nch * CRC_CHUNK, np.uint8)
            if mutant == "crc_stage_unmasked":  # every lane of every round loads its 16 bytes: the whole tile
                read = tiles * CRC_TILE
            take = min(read, nch * CRC_CHUNK, len(buf) - off)
            d[:take] = buf[off:off + take]
            rows.append(d.reshape(nch, CRC_CHUNK))
            my0 = np.arange(nch, dtype=np.int64) * CRC_CHUNK
            ml = np.minimum(n - my0, CRC_CHUNK)
            mylen.append(ml)
            if mutant == "crc_after_tile_end":
                end = (my0 // CRC_TILE + 1) * CRC_TILE
                af = np.where(end < n, n - end, 0)
            elif mutant == "crc_after_full_chunk":
                af = n - (my0 + CRC_CHUNK)  # (wraps below zero in uint64_t)
            else:
                af = n - (my0 + ml)
            after.append(af.astype(np.int64).view(np.uint64))
        if stray is not None:
            stray.append(read - n)
    if not total:
        return [0] * len(items)
    rows, mylen, after = np.concatenate(rows), np.concatenate(mylen), np.concatenate(after)
    crc = np.full(total, 0xFFFFFFFF, np.uint32)
    for piece in range(CRC_CHUNK // CRC_PIECE):
        done = piece * CRC_PIECE
        if mutant == "crc_here_without_done":
            here = np.where(mylen > done, np.minimum(mylen, CRC_PIECE), 0)
        else:
            here = np.where(mylen > done, np.minimum(mylen - done, CRC_PIECE), 0)
        stage = rows[:, done:done + CRC_PIECE]
        words = np.ascontiguousarray(stage).view("<u4")
        for w in range(CRC_PIECE // 4):
            live = w * 4 + 4 <= here
            if not live.any():
                break
            x = crc ^ words[:, w]
            x = T[3][x & np.uint32(0xFF)] ^ T[2][(x >> np.uint32(8)) & np.uint32(0xFF)] ^ T[1][(x >> np.uint32(16)) & np.uint32(0xFF)] ^ T[0][x >> np.uint32(24)]
            crc = np.where(live, x, crc)
        if mutant == "crc_no_tail_bytes":
            continue
        nw = here // 4
        for t in range(3):
            b = nw * 4 + t
            live = b < here
            if not live.any():
                break
            d = np.take_along_axis(stage, np.minimum(b, CRC_PIECE - 1).reshape(-1, 1), axis=1)[:, 0].astype(np.uint32)
            x = T[0][(crc ^ d) & np.uint32(0xFF)] ^ (crc >> np.uint32(8))
            crc = np.where(live, x, crc)
    v = ~crc
    if mutant == "crc_skip_zero_register":
        v = np.where(crc == 0, np.uint32(0), v)
    v = np.where(after != 0, _vmulmod(_vxpow8(after), v), v)
    # the XOR of the contributions; the kernels leave a zero out, which changes nothing
    out = []
    for k, (off, n) in enumerate(items):
        hi = start[k + 1] if k + 1 < len(items) else total
        out.append(int(np.bitwise_xor.reduce(v[start[k]:hi])) if hi > start[k] else 0)
    return out


def model_crc(buf, off, n, mutant=None, stray=None):
    return model_crc_many(buf, [(off, n)], mutant, stray)[0]


def model_many(kind, buf, cases, mutant=None, stray=None):
    if kind == "adler":
        return [model_adler(buf, c.at, c.n, mutant, stray) for c in cases]
    out = []
    for k in range(0, len(cases), 256):  # (a set of rows at a time: the staged bytes of a whole arena are too many at once)
        out += model_crc_many(buf, [(c.at, c.n) for c in cases[k:k + 256]], mutant, stray)
    return out


# ---- the batches of the GPU test (verify / inflate / encode) ------------------------------------------------------------------------------
BATCH_FAMILIES = ("ff", "ramp", "random", "onehot", "hot", "zeros")
BATCH_OFFSETS = (1, 0, 3, 15, 4, 8, 16)


def batch_specs():
    """every size of both lists once, the families and the offsets rotating; empty items between full ones: one behind the largest
    item of the 8-workgroup Adler grids, one between the two largest items, one at the very end behind a full item's neighbour.  The
    sizes whose Adler grid has 8 workgroups and whose CRC grid has 1 (114689 .. 131072) are those of the CRC list."""
    sizes = sorted(set(ADLER_SIZES) | set(CRC_SIZES))
    sizes.remove(0)
    assert [n for n in sizes if -(-n // ADLER_CHUNK) == 8 and -(-n // CRC_TILE) == 1] == [131071, 131072]
    order = []
    for n in sizes:
        order.append(n)
        if n in (17, 16384, 131072, 262145):
            order.append(0)
    out = []
    for k, n in enumerate(order):
        family = BATCH_FAMILIES[k % len(BATCH_FAMILIES)] if n else "zeros"
        d = details(family, n)
        out.append((family, d[(k // len(BATCH_FAMILIES)) % len(d)] if n else None, n, BATCH_OFFSETS[k % len(BATCH_OFFSETS)]))
    return out


def frame(data, wrapper, level):
    """a zlib (wrapper 1) or gzip (wrapper 2) stream of data from Python's zlib"""
    co = zlib.compressobj(level, zlib.DEFLATED, 15 if wrapper == 1 else 31)
    return co.compress(data) + co.flush()


def flip_trailer(stream, wrapper, which):
    """one bit of the trailer flipped.  which 0 / 1: the low / high half of the Adler-32 (wrapper 1), the CRC-32 / ISIZE (wrapper 2)"""
    s = bytearray(stream)
    at = {(1, 0): -1, (1, 1): -4, (2, 0): -6, (2, 1): -3}[(wrapper, which)]
    s[at] ^= 0x10
    return bytes(s)


def encode_specs():
    """the all-0xFF, ramp and one-hot buffers of the sizes next to 16384 and 131072, at pointer offsets 0 and 1"""
    out = []
    for n in (16383, 16384, 16385, 131071, 131072, 131073):
        for family, d in (("ff", None), ("ramp", None), ("onehot", n - 1), ("onehot", (n - 1) // ADLER_CHUNK * ADLER_CHUNK)):
            for off in (0, 1):
                out.append((family, d, n, off))
    return out
