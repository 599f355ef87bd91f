"""Inputs that drive the hash sort (k_sort / kb_sort: k_sort_body, sort_pass, sort_pass_rtn in csrc/deflate_kernels.hip) to the edges
its code has, and a plain reference of the tables it leaves: S (an epoch's positions by (hash, position), stored x 2) and B (bucket
starts, J, the run flag, the mark for the permuted pair table).

Everything is generated here from fixed seeds; no data file is committed.  A case is a dict(name, family, data, opts, offsets, claims
[, params, targets]): `offsets` are the distances from a 16-byte boundary at which the GPU tests place the input in device memory,
`claims` the cells (tuples, see COVERAGE) the case is there for.  facts() derives the cells an input reaches from the reference and
from a restatement of how the kernel cuts an epoch into pieces, waves and batches; check() holds a case to its claims on the CPU,
so a case that stops forcing its edge fails instead of passing empty.  tests/test_sort_cases.py (CPU), tests/test_sort_gpu.py and
tests/test_match_walk_swz_gpu.py use the cases.

The reference, per epoch e of an input of n bytes placed `offset` bytes behind a 16-byte boundary (reference()):
  E = 32768 e, J = clamp(max(n - 2, 0) - E, 0, 32768), h[i] = hash3(in[E + i], in[E + i + 1], in[E + i + 2])
  S[:J] = 2 * stable argsort of h[:J]                       (entries from J on are unspecified)
  B[x]  = number of keys with a hash below x, x = 0 .. 32767;  B[32768] = J
  B[32769], the run flag = 1 iff more than 32 of the 64 aligned pieces [E + 512 k, E + 512 k + 516) are one byte repeated -- on the
          `whole` path only: a full epoch, offset % 16 == 0 and E + 32768 + 4 <= n; else 0
  B[32770], the mark = J >= 1024 and, with nb_q = the number of distinct (pos >> 1) & 63 among the 64 sorted positions from rank
          (2 q + 1) * (J // 8) on, q = 0 .. 3: two or more nb_q <= 14, or any nb_q <= 7

What the generators rest on.  hash3(a, b, c) = ((a & 31) << 10 ^ b << 5 ^ c) & 0x7fff, so a key's LOW digit (bits 0..7, the first
pass) is c ^ (b & 7) << 5 and its HIGH digit (bits 8..14, the second pass) is (a & 31) << 2 ^ b >> 3.
  * The low digit of position i depends on bytes i + 1 and i + 2 alone: given byte i + 1, byte i + 2 = d ^ (byte[i + 1] & 7) << 5
    gives position i any digit d.  _low_digits() writes a stretch of bytes whose positions have exactly the digits asked for; a batch
    of the first pass is 64 consecutive positions from a multiple of 64.  (The first pass looks for a hot digit only in an epoch with
    a run piece, and a run piece needs the `whole` path, i.e. a full epoch: its batches are never partly valid.)
  * The second pass ranks the keys in the order the first pass left them: by low digit, then position.  _high_digits() writes
    triples (a, b, c) with c = 255 ^ t << 5 and b = (H & 3) << 3 | t, t in 1..6, a = 0x80 | H >> 2: every third position has the
    low digit 255 and the high digit H, and the two positions between -- (b, c, a'), (c, a', b') -- have low digits a' ^ 0xe0 != 255
    and one whose low three bits are t' != 7.  So the designed keys are the last of the first pass's output, in position order, the
    2 m others in front of them; with m a multiple of 32 the designed keys begin on a batch boundary, all keys of their batches share
    the low digit 255, and the batch's high digits are the H written.  m an odd multiple of 32 makes J = 3 m end 32 lanes into a
    batch: the last, partly valid batch of a short epoch.
  * A mark edge is one trigram put at positions whose banks (pos >> 1) & 63 cycle through k values, so any 64 neighbours of its
    bucket sit on exactly k banks; the trigram's hash is searched (on the reference) so that the keys with smaller hashes -- noise
    -- put a sample window inside the bucket.
"""
import functools

import numpy as np

import datagen
import match_cases as mc
import oracle_binding as ob

EPOCH = 32768
BSTRIDE = EPOCH + 8
DEFAULT = (128, 32, 1)
SWZ_BANKS = 14  # MI355_SWZ_BANKS
SORT_HOT = 4    # MI355_SORT_HOT
NKS = (3, 4, 5, 63, 64)


def hash3(a, b, c):
    return (((a & 31) << 10) ^ (b << 5) ^ c) & 0x7FFF


def hashes(data):
    d = np.frombuffer(bytes(data), dtype=np.uint8).astype(np.uint32)
    if len(d) < 3:
        return np.zeros(0, dtype=np.uint32)
    return (((d[:-2] & 31) << 10) ^ (d[1:-1] << 5) ^ d[2:]) & 0x7FFF


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def run_pieces(data, e):
    """which of epoch e's 64 aligned pieces [E + 512 k, E + 512 k + 516) are one byte repeated (False where the input ends sooner)"""
    E = EPOCH * e
    return [E + 512 * k + 516 <= len(data) and len(set(data[E + 512 * k:E + 512 * k + 516])) == 1 for k in range(64)]


def samples(order, J):
    """nb_q, q = 0..3: distinct banks among the 64 sorted positions from rank (2 q + 1) * (J // 8) on (None below 512 keys: no window)"""
    if J < 512:
        return None
    return tuple(len(set(((order[(2 * q + 1) * (J // 8):(2 * q + 1) * (J // 8) + 64] >> 1) & 63).tolist())) for q in range(4))


@functools.lru_cache(maxsize=64)
def reference(data, offset=0):
    """[dict(J, S, B, runs, mark, nb, whole)] per epoch: S = int array of J entries, B = int array of 32769 entries (B[32768] = J)"""
    n, h, out = len(data), hashes(data), []
    for e in range((n + EPOCH - 1) // EPOCH):
        E = EPOCH * e
        J = min(max(max(n - 2, 0) - E, 0), EPOCH)
        he = h[E:E + J].astype(np.int64)
        order = np.argsort(he, kind="stable")
        counts = np.bincount(he, minlength=EPOCH)
        B = np.concatenate(([0], np.cumsum(counts)[:-1], [J]))
        whole = J == EPOCH and offset % 16 == 0 and E + EPOCH + 4 <= n
        runs = 1 if whole and sum(run_pieces(data, e)) > 32 else 0
        nb = samples(order, J)
        few = sum(1 for x in nb if x <= SWZ_BANKS) if nb else 0
        very = sum(1 for x in nb if x <= SWZ_BANKS // 2) if nb else 0
        mark = 1 if J >= 1024 and (few >= 2 or very >= 1) else 0
        out.append(dict(J=J, S=2 * order, B=B, runs=runs, mark=mark, nb=nb, whole=whole))
    return out


def brute(data):
    """[(S, B)] per epoch from sorted() and a count per bucket"""
    n, out = len(data), []
    for e in range((n + EPOCH - 1) // EPOCH):
        E = EPOCH * e
        J = min(max(max(n - 2, 0) - E, 0), EPOCH)
        hs = [hash3(data[E + i], data[E + i + 1], data[E + i + 2]) for i in range(J)]
        order = sorted(range(J), key=lambda i: (hs[i], i))
        ss = sorted(hs)
        B, at = [], 0
        for x in range(EPOCH):
            while at < J and ss[at] < x:
                at += 1
            B.append(at)
        out.append(([2 * i for i in order], B + [J]))
    return out


# ---- how the kernel cuts an epoch up: batches of 64 keys and the lanes on the first lane's digit ---------------------------------------
def _batches(dig, J):
    """per batch of 64 keys (digits in rank order): (valid lanes, the first lane's digit, lanes on it, the other lanes' counts)"""
    out = []
    for s in range(0, J, 64):
        d = dig[s:min(s + 64, J)]
        vals, cnt = np.unique(d, return_counts=True)
        nk = int(cnt[vals == d[0]][0])
        out.append((len(d), int(d[0]), nk, sorted(int(x) for v, x in zip(vals, cnt) if v != d[0])))
    return out


def hot_batches(data, e, offset=0):
    """{'low': [...], 'high': [...]}: the batches of epoch e in which sort_pass_rtn looks for a hot digit"""
    r = reference(data, offset)[e]
    J, E = r["J"], EPOCH * e
    h = hashes(data)[E:E + J].astype(np.int64)
    hot_low = r["whole"] and any(run_pieces(data, e))
    order1 = np.argsort(h & 255, kind="stable")
    return dict(low=_batches(h & 255, J) if hot_low else [], high=_batches(h[order1] >> 8, J))


# ---- facts: the cells an input reaches -----------------------------------------------------------------------------------------------
def facts(c):
    data, n, cells = c["data"], len(c["data"]), set()
    h = hashes(data)
    if n <= 5:
        cells.add(("n", n))
    ref0 = reference(data, 0)
    if not ref0:
        cells.add(("J", 0, 0))
    for e, r in enumerate(ref0):
        E, J = EPOCH * e, r["J"]
        if e == len(ref0) - 1 or J < EPOCH:
            cells.add(("J", J, e))  # the keys of an epoch that is not full, or of the last one, behind e others
        if e == 0 and 2 <= n - EPOCH <= 4:
            cells.add(("whole_edge", n - EPOCH, r["whole"]))
        if e == 0 and J == EPOCH:
            for off in c["offsets"]:
                cells.add(("load", off, "whole" if reference(data, off)[0]["whole"] else "clamped"))
        if J == 0:
            continue
        he = h[E:E + J].astype(np.int64)
        counts = np.bincount(he, minlength=EPOCH)
        top = int(counts.argmax())
        if counts[top] == EPOCH:
            cells.add(("hist_full", "odd" if top & 1 else "even"))
        pair = np.nonzero((counts[0::2] == EPOCH // 2) & (counts[1::2] == EPOCH // 2))[0]
        if len(pair):
            cells.add(("hist_pair", EPOCH // 2))
        for x in (0, EPOCH - 1):
            cells.add(("bucket", x, "used" if counts[x] else "empty"))
        if r["whole"]:
            rp = run_pieces(data, e)
            cells.add(("run_pieces", sum(rp), r["runs"]))
            for k in range(64):
                a = E + 512 * k
                if rp[k] and (k == 0 or data[a - 1] != data[a]) and data[a + 516] != data[a]:
                    cells.add(("run", "exact_516"))
                if not rp[k] and len(set(data[a:a + 515])) == 1 and (k == 0 or data[a - 1] != data[a]):
                    cells.add(("run", "short_515"))
                if not rp[k] and k < 63 and rp[k + 1] and len(set(data[a + 1:a + 512])) == 1 and data[a] != data[a + 1] == data[a + 512]:
                    cells.add(("run", "late_by_1"))
                if not rp[k] and k < 63 and rp[k + 1] and len(set(data[a:a + 512])) == 1 and data[a] != data[a + 512]:
                    cells.add(("run", "neighbours_differ"))
        for which, bs in hot_batches(data, e).items():
            for valid, d0, nk, others in bs:
                if nk in NKS:
                    cells.add(("hot", which, nk, "full" if valid == 64 else "partial"))
                    if others:
                        cells.add(("hot_others", which, "shared" if max(others) > 1 else "distinct"))
                if nk >= SORT_HOT and others and min(others) > nk:
                    cells.add(("hot_rarest", which))
                if nk >= SORT_HOT and valid > nk:
                    cells.add(("hot_digit", which, d0))
        # a bucket in which two trigrams that hash alike take turns
        big = np.nonzero(counts >= 8)[0]
        for x in big.tolist()[:64]:
            pos = np.nonzero(he == x)[0]
            tri = [bytes(data[E + p:E + p + 3]) for p in pos.tolist()]
            if len(set(tri)) >= 2 and sum(1 for a, b in zip(tri, tri[1:]) if a != b) >= 4 and sum(1 for a, b in zip(tri, tri[1:]) if a == b) >= 2:
                cells.add(("stable", "alike_interleaved"))
        if r["nb"]:
            lows = tuple(sorted(x for x in r["nb"] if x <= SWZ_BANKS + 1))
            if lows or J in (1023, 1024):
                cells.add(("mark", J if J in (1023, 1024) else "J", lows, r["mark"]))
    p = c.get("params", {})
    if "natural" in p:
        cells.add(("natural", p["natural"], tuple(r["mark"] for r in ref0)))
    for t in c.get("targets", ()):
        q = t["p"]
        bucket = np.nonzero(h[:q] == h[q])[0]
        if q // EPOCH == 1 and len(bucket) and all(int(x) // EPOCH == 0 for x in bucket):
            cells.add(("prev_bucket", int(h[q])))
    return cells


def check(c):
    """assert a case on the CPU: every claim is a cell the input reaches; the oracle takes no second pass over it (Q1: no block but
    the last may end inside the first 32 768 bytes); a target's match is a token of the oracle's.  Returns the cells."""
    cells = facts(c)
    missing = [x for x in c["claims"] if x not in cells]
    assert not missing, "%s no longer reaches %s (it reaches %s)" % (c["name"], missing, sorted(cells, key=repr))
    ob.encode(c["data"], opts=ob.make_opts(*c["opts"]))
    blocks = ob.trace_blocks()
    assert len(blocks) <= 1 or blocks[0]["in_bytes"] > EPOCH, (c["name"], blocks[:2])
    if c.get("targets"):
        toks = mc.tokens_at(c["data"], c["opts"])
        for t in c["targets"]:
            assert toks.get(t["p"]) == t["tok"], "%s: the oracle has %s at %d, the case declares %s" % (c["name"], toks.get(t["p"]), t["p"], t["tok"])
    return cells


# ---- building blocks -----------------------------------------------------------------------------------------------------------------
def _text(n, seed):
    return bytearray(datagen.text_like(n, seed)[:n])


def _case(name, family, data, claims, offsets=(0,), **kw):
    return dict(name=name, family=family, data=bytes(data), opts=DEFAULT, offsets=tuple(offsets), claims=list(claims), **kw)


def _digit_batches(ndig, seed, first=()):
    """batches of 64 digits below ndig: for every nk of NKS one whose other lanes hold distinct digits and one where they share two;
    one whose first lane's digit is the rarest; and for every digit of `first` one with five lanes on it"""
    r = np.random.default_rng(seed)
    out = []

    def batch(d0, nk, others):
        lanes = [0] + sorted((r.choice(63, size=nk - 1, replace=False) + 1).tolist())
        b, it = [None] * 64, iter(others)
        for k in lanes:
            b[k] = d0
        return [x if x is not None else next(it) for x in b]

    for nk in NKS:
        d0 = int(r.integers(ndig))
        free = [x for x in r.permutation(ndig).tolist() if x != d0]
        out.append(batch(d0, nk, free[:64 - nk]))
        if nk < 63:
            rest = 64 - nk
            out.append(batch(d0, nk, r.permutation([free[0]] * (rest // 2) + [free[1]] * (rest - rest // 2)).tolist()))
    d0 = int(r.integers(ndig))
    free = [x for x in r.permutation(ndig).tolist() if x != d0]
    out.append(batch(d0, 4, r.permutation([free[0]] * 20 + [free[1]] * 20 + [free[2]] * 20).tolist()))
    for d0 in first:
        free = [x for x in r.permutation(ndig).tolist() if x != d0]
        out.append(batch(d0, 5, free[:59]))
    return out


def _low_digits(buf, at, digits):
    """bytes at + 2 .. so that positions at, at + 1, .. have these low digits (byte at + 1 stays)"""
    for k, d in enumerate(digits):
        buf[at + k + 2] = d ^ ((buf[at + k + 1] & 7) << 5)


def _high_digits(H, seed):
    """3 len(H) + 2 bytes: positions 0, 3, 6, .. have the low digit 255 and the high digits H; no other position has the low digit 255"""
    r = np.random.default_rng(seed)
    out = bytearray()
    for x in H:
        t = int(r.integers(1, 7))
        out += bytes([0x80 | (x >> 2), ((x & 3) << 3) | t, 255 ^ (t << 5)])
    return out + b"\x80\x01"


def tri_of(h):
    """a trigram with hash h"""
    return bytes([0xE0 | (h >> 10), (h >> 5) & 31, h & 31])


# ---- the families --------------------------------------------------------------------------------------------------------------------
def _length(n):
    d = _text(max(n, 1), 0x50A0)[:n]
    cl = [("n", n)] if n <= 5 else []
    ep = max((n + EPOCH - 1) // EPOCH, 1)
    js = [min(max(max(n - 2, 0) - EPOCH * e, 0), EPOCH) for e in range(ep)]
    cl += [("J", j, e) for e, j in enumerate(js) if j < EPOCH or e == ep - 1]  # (32 769 bytes: a second epoch without a key)
    if 2 <= n - EPOCH <= 4:
        cl.append(("whole_edge", n - EPOCH, n - EPOCH == 4))
    return _case("len_%d" % n, "length", d, cl)


def _load():
    return _case("load_text", "load", _text(EPOCH + 100, 0x50A1), [("load", 0, "whole"), ("load", 1, "clamped"), ("load", 8, "clamped"),
                                                                  ("load", 15, "clamped")], offsets=(0, 1, 8, 15))


def _hist(kind):
    if kind == "even":
        d, cl = bytes(EPOCH + 4), [("hist_full", "even"), ("bucket", 0, "used"), ("bucket", EPOCH - 1, "empty"), ("run_pieces", 64, 1)]
    elif kind == "odd":
        d, cl = b"\x01" * (EPOCH + 4), [("hist_full", "odd"), ("bucket", 0, "empty")]
    else:  # 0x00 0x21 in turn: the trigrams 00 21 00 and 21 00 21 have the hashes 1056 and 1057
        d, cl = b"\x00\x21" * (EPOCH // 2 + 2), [("hist_pair", EPOCH // 2)]
    # (offset 1: the same counts from one add per key instead of one per wave)
    return _case("hist_" + kind, "histogram", d, cl, offsets=(0, 1))


def _wave_run(kind):
    d = _text(EPOCH + 64, 0x50A2)

    def run(lo, hi, byte):
        d[lo:hi] = bytes([byte]) * (hi - lo)
    if kind == "edges":
        run(512 * 3, 512 * 3 + 516, 0x5A)           # exactly a piece and its look-ahead
        run(512 * 10, 512 * 10 + 515, 0x5A)         # one byte short
        run(512 * 20 + 1, 512 * 21 + 516, 0x59)     # begins one byte behind a piece's start
        run(512 * 30, 512 * 31, 0x58)               # a piece of one byte whose look-ahead is the next piece's other byte
        run(512 * 31, 512 * 31 + 516, 0x57)
        cl = [("run", "exact_516"), ("run", "short_515"), ("run", "late_by_1"), ("run", "neighbours_differ"), ("run_pieces", 3, 0)]
    elif kind == "one":
        run(512 * 5, 512 * 5 + 516, 0x5A)
        cl = [("run_pieces", 1, 0)]
    else:
        k = int(kind)
        run(0, 512 * k + 4, 0)
        cl = [("run_pieces", k, 1 if k > 32 else 0)]
    return _case("wave_run_" + kind, "wave_run", d, cl)


HOT_LOW_AT = 576  # the first designed batch of _hot_low (a multiple of 64 behind the run piece)


def _hot_low():
    """a full epoch of text with one run piece in front -- the first pass then looks for a hot digit in every batch -- and batches
    of designed low digits behind it"""
    d = _text(EPOCH + 64, 0x50A3)
    d[0:516] = bytes(516)
    bs = _digit_batches(256, 0x50A4, first=(0, 255))
    _low_digits(d, HOT_LOW_AT, [x for b in bs for x in b])
    cl = [("hot", "low", nk, "full") for nk in NKS] + [("hot_others", "low", "distinct"), ("hot_others", "low", "shared"),
                                                       ("hot_rarest", "low"), ("hot_digit", "low", 0), ("hot_digit", "low", 255), ("run_pieces", 1, 0)]
    return _case("hot_low", "hot", d, cl, params=dict(batches=bs))


def _hot_high():
    """18 batches of designed high digits and the 32 keys of a last, partly valid one, behind 1216 = 19 * 64 other keys"""
    bs = _digit_batches(128, 0x50A5, first=(127,))
    bs += [[(7 * k + b) % 128 for k in range(64)] for b in range(18 - len(bs))]
    H = [x for b in bs for x in b] + [127] * 3 + list(range(29))
    assert len(H) % 64 == 32
    cl = [("hot", "high", nk, "full") for nk in NKS] + [("hot_others", "high", "distinct"), ("hot_others", "high", "shared"),
                                                        ("hot_rarest", "high"), ("hot_digit", "high", 127), ("hot", "high", 3, "partial")]
    return _case("hot_high", "hot", _high_digits(H, 0x50A6), cl, params=dict(batches=bs))


def _hot_high_partial(nk):
    """J = 96: 64 other keys, then the 32 designed ones as the last, partly valid batch"""
    r = np.random.default_rng(0x50A7 + nk)
    H = [5] + r.permutation([5] * (nk - 1) + [10 + k for k in range(32 - nk)]).tolist()
    return _case("hot_high_partial_%d" % nk, "hot", _high_digits(H, 0x50A8 + nk), [("hot", "high", nk, "partial"), ("J", 96, 0)])


def _stable():
    """units a b c s / a^0x20 b c s / a b c s ..: two trigrams with one hash take turns and repeat; the bucket is in position order"""
    r = np.random.default_rng(0x50A9)
    out = bytearray()
    for _ in range(12):
        a, b, c = int(r.integers(0xC0, 0xE0)), int(r.integers(0x80, 0xA0)), int(r.integers(0x80, 0xA0))
        for k in range(24):
            out += bytes([a ^ (0x20 if k % 3 == 1 else 0), b, c, 0x30 + int(r.integers(10)), 0x41 + int(r.integers(26))])
    return _case("stable_alike", "stability", out, [("stable", "alike_interleaved")])


def _lows(data):
    r = reference(bytes(data))[0]
    return tuple(sorted(x for x in r["nb"] if x <= SWZ_BANKS + 1)), r["mark"]


def _mark(name, J, specs, claim, seed, per=160):
    """noise of J + 2 bytes; for every (q, k) of specs one trigram at `per` positions whose banks cycle through k values.  Its hash
    is searched, from the seed, so that the keys with smaller hashes put sample window q inside its bucket: the trigram's bytes
    change the hashes of the positions around every copy too, so the number of keys in front is found by trying."""
    rng = np.random.default_rng(seed)
    base = bytearray(rng.integers(0, 256, size=J + 2, dtype=np.uint8).tobytes())
    want = [(2 * q + 1) * (J // 8) - (per - 64) // 2 for q, _ in specs]  # keys in front of the bucket
    for _ in range(4000):
        d = bytearray(base)
        for s, ((q, k), w) in enumerate(zip(specs, want)):
            hv = int(EPOCH * w / J + rng.integers(-20 * EPOCH // J, 20 * EPOCH // J + 1)) % EPOCH
            for j in range(per):
                p = 128 * (j // k) + 8 * (j % k) + 4 * s
                assert p + 3 <= J
                d[p:p + 3] = tri_of(hv)
        if _lows(d) == claim[2:] and (J != 1024 or _lows(d[:-1]) == (claim[2], 0)):
            return _case(name, "mark", d, [claim])
    raise RuntimeError("no hash found for %s" % name)


def records(n, width, seed):
    """rows of fixed-length records (tests/test_gpu_parity.py test_rows_of_records_take_the_permuted_pair_table)"""
    r = np.random.default_rng(seed)
    rows = n // width + 1
    a = np.tile(r.integers(0, 256, size=width, dtype=np.uint8), (rows, 1))
    a[:, 4:8] = np.arange(rows, dtype=np.uint32).view(np.uint8).reshape(rows, 4)
    cols = r.choice(np.arange(8, width), size=max(1, width // 8), replace=False)
    a[:, cols] = r.integers(0, 16, size=(rows, len(cols)), dtype=np.uint8)
    return a.reshape(-1)[:n].tobytes()


# the reference's verdict per epoch on three epochs of each (the mark of epoch 0, 1, 2)
NATURAL = {"rows_96": (1, 1, 1), "rows_256": (1, 1, 1), "rows_1024": (1, 1, 1), "rows_48": (1, 1, 1), "rows_40": (0, 0, 0), "text": (0, 0, 0)}


def _natural(kind):
    d = datagen.text_like(3 * EPOCH, 0x50AA)[:3 * EPOCH] if kind == "text" else records(3 * EPOCH, int(kind[5:]), 0x5EC0 + int(kind[5:]))
    return _case("natural_" + kind, "natural", d, [("natural", kind, NATURAL[kind])], params=dict(natural=kind))


def _prev_bucket(hv):
    """a target early in epoch 1 whose bucket -- hash 32767: the walk reads Bprev[32768], the J slot, as the bucket's end; or hash 0
    -- holds one candidate, late in epoch 0"""
    tri = {EPOCH - 1: b"\xdb\x9b\x9f", 0: b"\xc4\x84\x80"}[hv]
    assert hash3(*tri) == hv
    T = tri + bytes(range(0xA1, 0xAA))
    d = _text(EPOCH + 600, 0x50AB + (hv & 1))
    q, p = EPOCH - 400, EPOCH + 200
    d[q - 1:q + 10] = b"\x01" + T[:9] + b"\x30"
    d[p - 1:p + 13] = b"\x02" + T[:12] + b"\x31"
    for _ in range(8):  # (text that happens to fall into the bucket is changed by a letter)
        others = [int(x) for x in np.nonzero(hashes(d) == hv)[0] if x not in (q, p)]
        for x in others:
            assert not (q - 4 < x < q + 11 or p - 4 < x < p + 14)
            d[x + 2] = 0x61 + (d[x + 2] - 0x61 + 1) % 26
        if not others:
            break
    assert not others
    return _case("prev_bucket_%d" % hv, "prev_bucket", d, [("prev_bucket", hv), ("bucket", hv, "used")],
                 targets=[dict(p=p, tok=("ld", 9, p - q))])


J_ALONE = (1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 32767)
MARKS = [("mark_7", 4096, [(1, 7)], ("mark", "J", (7,), 1)),
         ("mark_8", 4096, [(1, 8)], ("mark", "J", (8,), 0)),
         ("mark_14_14", 4096, [(0, 14), (2, 14)], ("mark", "J", (14, 14), 1)),
         ("mark_14_15", 4096, [(0, 14), (2, 15)], ("mark", "J", (14, 15), 0)),
         ("mark_15_15", 4096, [(0, 15), (2, 15)], ("mark", "J", (15, 15), 0)),
         ("mark_14_14_J1024", 1024, [(0, 14), (2, 14)], ("mark", 1024, (14, 14), 1))]


def _table_of_cases():
    t = {}
    for n in (0, 1, 2, 3, 4, 5) + tuple(j + 2 for j in J_ALONE) + (EPOCH + 2, EPOCH + 3, EPOCH + 4, 2 * EPOCH + 3, 2 * EPOCH + 67):
        t["len_%d" % n] = lambda n=n: _length(n)
    t["load_text"] = _load
    for k in ("even", "odd", "pair"):
        t["hist_" + k] = lambda k=k: _hist(k)
    for k in ("edges", "one", "32", "33"):
        t["wave_run_" + k] = lambda k=k: _wave_run(k)
    t["hot_low"] = _hot_low
    t["hot_high"] = _hot_high
    for nk in (3, 4, 5):
        t["hot_high_partial_%d" % nk] = lambda nk=nk: _hot_high_partial(nk)
    t["stable_alike"] = _stable
    for k, (name, J, specs, claim) in enumerate(MARKS):
        t[name] = lambda name=name, J=J, specs=specs, claim=claim, k=k: _mark(name, J, specs, claim, 0x50B0 + k, per=160 if J > 1024 else 80)
    t["mark_14_14_J1023"] = _mark_1023
    for k in NATURAL:
        t["natural_" + k] = lambda k=k: _natural(k)
    for hv in (EPOCH - 1, 0):
        t["prev_bucket_%d" % hv] = lambda hv=hv: _prev_bucket(hv)
    return t


def _mark_1023():
    """the J = 1024 layout less its last byte: the samples would mark the epoch, 1023 keys do not"""
    c = case("mark_14_14_J1024")
    return _case("mark_14_14_J1023", "mark", c["data"][:-1], [("mark", 1023, (14, 14), 0), ("J", 1023, 0)])


_CASES = _table_of_cases()
FAMILIES = ("length", "load", "histogram", "wave_run", "hot", "stability", "mark", "natural", "prev_bucket")


def names():
    return list(_CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    c = _CASES[name]()
    assert c["name"] == name and c["opts"] == DEFAULT and len(c["data"]) <= 3 * EPOCH + 4096
    return c


def natural_names():
    return ["natural_" + k for k in NATURAL]


# ---- the coverage table: every cell must be claimed by at least one case ----------------------------------------------------------------
COVERAGE = (
    [("n", n) for n in range(6)]
    + [("J", j, 0) for j in (0,) + J_ALONE] + [("J", 0, 1), ("J", 1, 2), ("J", 65, 2)]
    + [("whole_edge", 2, False), ("whole_edge", 3, False), ("whole_edge", 4, True)]
    + [("load", 0, "whole"), ("load", 1, "clamped"), ("load", 8, "clamped"), ("load", 15, "clamped")]
    + [("hist_full", "even"), ("hist_full", "odd"), ("hist_pair", EPOCH // 2)]
    + [("bucket", x, u) for x in (0, EPOCH - 1) for u in ("used", "empty")]
    + [("run", k) for k in ("exact_516", "short_515", "late_by_1", "neighbours_differ")]
    + [("run_pieces", 32, 0), ("run_pieces", 33, 1), ("run_pieces", 1, 0), ("run_pieces", 64, 1)]
    + [("hot", w, nk, "full") for w in ("low", "high") for nk in NKS] + [("hot", "high", nk, "partial") for nk in (3, 4, 5)]
    + [("hot_others", w, k) for w in ("low", "high") for k in ("distinct", "shared")]
    + [("hot_rarest", "low"), ("hot_rarest", "high"), ("hot_digit", "low", 0), ("hot_digit", "low", 255), ("hot_digit", "high", 127)]
    + [("stable", "alike_interleaved")]
    + [m[3] for m in MARKS] + [("mark", 1023, (14, 14), 0)]
    + [("natural", k, v) for k, v in NATURAL.items()]
    + [("prev_bucket", EPOCH - 1), ("prev_bucket", 0)]
)


def claimed():
    """{cell: [names of the cases that claim it]}"""
    out = {}
    for n in names():
        for cell in case(n)["claims"]:
            out.setdefault(cell, []).append(n)
    return out


# ---- what a failing table comparison prints ------------------------------------------------------------------------------------------
def table_diff(c, offset, S, B):
    """None, or the first difference between the tables read back (S: uint16 [epochs, 32768], B: uint16 [epochs, BSTRIDE]) and the
    reference of case c at that offset: the epoch, the first differing rank or bucket, and the case's claims"""
    for e, r in enumerate(reference(c["data"], offset)):
        J, what = r["J"], None
        s, b = S[e].astype(np.int64), B[e].astype(np.int64)
        bad = np.nonzero(s[:J] != r["S"])[0]
        if len(bad):
            k = int(bad[0])
            what = "S: rank %d holds position %d, the reference %d" % (k, s[k] // 2, r["S"][k] // 2)
        bad = np.nonzero(b[:EPOCH + 1] != r["B"] % 65536)[0]
        if what is None and len(bad):
            k = int(bad[0])
            what = "B[%d] = %d, the reference %d" % (k, b[k], r["B"][k])
        if what is None and b[EPOCH + 1] != r["runs"]:
            what = "the run flag is %d, the reference %d" % (b[EPOCH + 1], r["runs"])
        if what is None and b[EPOCH + 2] != r["mark"]:
            what = "the mark is %d, the reference %d (banks of the samples %s)" % (b[EPOCH + 2], r["mark"], r["nb"])
        if what:
            return "%s at offset %d, epoch %d (J = %d): %s; the case claims %s" % (c["name"], offset, e, J, what, c["claims"])
    return None
