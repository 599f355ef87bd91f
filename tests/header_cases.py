"""Inputs that drive the block-header stage (stages.h build_header, kernels k_block_header / kb_block_header) into the
cases ordinary data never reaches: Huffman trees deeper than the limit (15 for literal/length and distance codes, 7 for
the code-length code), numbers of used symbols at the edges of the kernel's 64-lane chunks, ties, and runs of equal code
lengths of every coded form, placed on the 64-entry chunk seams of the kernel's run coder.

Everything is generated here from fixed seeds; no data file is committed.  A case is (name, data, level, target):
`target` is a list with one dict per block of the oracle's stream and says what the case must provoke there.  check()
asserts it on the oracle alone, so a case that stops provoking its behaviour fails instead of passing empty-handed.
tests/test_header_cases.py (CPU: preconditions, host build of stages.h) and tests/test_block_header_gpu.py use the cases.

Keys of a block's target (all optional but btype):
  btype                    block type in the oracle's stream (2 = dynamic)
  ll_unl, d_unl, cl_unl    depth of the unlimited Huffman tree (max of huffman_lengths(freqs, 31)) of the three histograms
  m_ll, m_d                number of used literal/length and distance symbols (end-of-block included)
  runs                     [(start, end, value)]: maximal runs of equal lengths in ll_lens + d_lens, end exclusive
  seam                     True: one run of non-zero lengths covers the last literal/length and the first distance length
"""
import functools
import random
from collections import Counter

import oracle_binding as ob

LV = {"fast": (1, 0, 0), "default": (128, 32, 1), "best": (1768, 128, 1), "rle": (0, 0, 1), "huffman_only": (0, 0, 0)}
BLOCK_TOKENS = 31744

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
         8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
TREES = ("code-length", "literal/length", "distance")


# ---- a small inflate that keeps what the encoder chose (the logic of tools/tokdump.py, table driven) ---------------------------
class _Bits:
    def __init__(self, raw, pos=0):
        self.b = bytes(raw) + bytes(8)
        self.n = 8 * len(raw)
        self.p = pos

    def peek(self, n):
        i = self.p >> 3
        return (int.from_bytes(self.b[i:i + 4], "little") >> (self.p & 7)) & ((1 << n) - 1)

    def get(self, n):
        v = self.peek(n)
        self.p += n
        if self.p > self.n:
            raise ValueError("read past the end of the stream")
        return v


def _rev(c, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (c & 1)
        c >>= 1
    return r


def _table(lengths):
    """canonical code -> (table indexed by the next `width` bits of the stream, width); an entry is sym << 4 | length"""
    width = max(lengths) if lengths else 0
    if width == 0:
        return None, 0
    count = [0] * (width + 1)
    for l in lengths:
        if l:
            count[l] += 1
    code, nxt = 0, [0] * (width + 2)
    for bits in range(1, width + 1):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    tab = [-1] * (1 << width)
    for s, l in enumerate(lengths):
        if l:
            c = nxt[l]
            nxt[l] += 1
            if c >> l:
                raise ValueError("over-subscribed code")
            for k in range(_rev(c, l), 1 << width, 1 << l):
                tab[k] = (s << 4) | l
    return tab, width


def _sym(br, tw):
    tab, width = tw
    if tab is None:
        raise ValueError("symbol of an empty code at bit %d" % br.p)
    e = tab[br.peek(width)]
    if e < 0:
        raise ValueError("bad code at bit %d" % br.p)
    br.get(e & 15)
    return e >> 4


def read_header(br):
    """the header of a dynamic block, behind its three type bits: dict(cl_lens[19], ll_lens, d_lens).  A header that
    cannot be read to its end comes back with what was read and an 'error'."""
    h = dict(cl_lens=None, ll_lens=None, d_lens=None)
    try:
        hl, hd, hc = br.get(5) + 257, br.get(5) + 1, br.get(4) + 4
        cl = [0] * 19
        for i in range(hc):
            cl[ORDER[i]] = br.get(3)
        h["cl_lens"] = cl
        ct = _table(cl)
        ls = []
        while len(ls) < hl + hd:
            s = _sym(br, ct)
            if s < 16:
                ls.append(s)
            elif s == 16:
                ls += [ls[-1]] * (3 + br.get(2))
            elif s == 17:
                ls += [0] * (3 + br.get(3))
            else:
                ls += [0] * (11 + br.get(7))
        if len(ls) != hl + hd:
            raise ValueError("a run of lengths crosses the end of the table")
        h["ll_lens"], h["d_lens"] = ls[:hl], ls[hl:]
    except (ValueError, IndexError) as e:
        h["error"] = str(e)
    return h


_FIXED = None


def decode(raw, strict=True, positions=False, start=0, blocks=0):
    """-> list of blocks: dict(btype, bfinal, bit_start, bit_end, toks=[(0, byte) | (length, distance)], ll_syms, d_syms
    and, for a dynamic block, cl_lens / ll_lens / d_lens).  strict=False: a stream that cannot be read ends with a block
    that holds what was read of it and an 'error'.  positions=True: a compressed block also gets tok_pos, the bit its
    every token begins at with the end-of-block code's bit as the last entry (so tok_pos[0] is where the header ends), and
    a stored block gets payload, the byte offset of its first payload byte.  start: the bit the first block to read begins
    at; blocks: read no more than that many (0: up to the final one)."""
    global _FIXED
    br = _Bits(raw, start)
    out = []
    while True:
        blk = dict(btype=None, bfinal=0, bit_start=br.p, toks=[], ll_syms=[], d_syms=[])
        out.append(blk)
        try:
            blk["bfinal"], blk["btype"] = br.get(1), br.get(2)
            bt = blk["btype"]
            if bt == 0:
                br.p = (br.p + 7) & ~7
                n = br.get(16)
                br.get(16)
                blk["stored"] = n
                if positions:
                    blk["payload"] = br.p >> 3
                br.p += 8 * n
            elif bt in (1, 2):
                if bt == 1:
                    if _FIXED is None:
                        _FIXED = (_table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _table([5] * 30))
                    lt, dt = _FIXED
                else:
                    h = read_header(br)
                    blk.update(h)
                    if "error" in h:
                        raise ValueError(h["error"])
                    lt, dt = _table(h["ll_lens"]), _table(h["d_lens"])
                toks, lls, ds = blk["toks"], blk["ll_syms"], blk["d_syms"]
                pos = blk.setdefault("tok_pos", []) if positions else None
                while True:
                    if positions:
                        pos.append(br.p)
                    s = _sym(br, lt)
                    lls.append(s)
                    if s == 256:
                        break
                    if s < 256:
                        toks.append((0, s))
                    else:
                        ln = LBASE[s - 257] + br.get(LEXT[s - 257])
                        d = _sym(br, dt)
                        ds.append(d)
                        toks.append((ln, DBASE[d] + br.get(DEXT[d])))
            else:
                raise ValueError("block type 3")
            if br.p > br.n:
                raise ValueError("the block ends behind the stream")
        except (ValueError, IndexError) as e:
            if strict:
                raise
            blk["error"] = str(e)
            break
        blk["bit_end"] = br.p
        if blk["bfinal"] or len(out) == blocks:
            break
    return out


def header_diff(got, want):
    """Where the dynamic headers of two streams part: the first block, which of the three trees, the first symbol whose
    lengths differ, with both lengths; failing that, what else differs first.  None for streams that read the same."""
    bg, bw = decode(got, strict=False), decode(want, strict=False)
    for b, (g, w) in enumerate(zip(bg, bw)):
        where = "block %d (bit %d)" % (b, w["bit_start"])
        if g["bit_start"] != w["bit_start"] or g["btype"] != w["btype"]:
            return "%s: begins at bit %d with type %s, expected type %s" % (where, g["bit_start"], g["btype"], w["btype"])
        for key, tree in zip(("cl_lens", "ll_lens", "d_lens"), TREES):
            x, y = g.get(key), w.get(key)
            if x is None and y is None:
                continue
            if x is None or y is None:
                return "%s: the %s lengths cannot be read (%s), expected %s" % (where, tree, g.get("error"), y)
            if len(x) != len(y):
                return "%s, %s tree: %d lengths, expected %d" % (where, tree, len(x), len(y))
            for s, (lx, ly) in enumerate(zip(x, y)):
                if lx != ly:
                    return "%s, %s tree: symbol %d has length %d, expected %d" % (where, tree, s, lx, ly)
        if g["toks"] != w["toks"] or g.get("stored") != w.get("stored"):
            i = next((i for i, (p, q) in enumerate(zip(g["toks"], w["toks"])) if p != q), min(len(g["toks"]), len(w["toks"])))
            return "%s: same header, token %d differs (%d tokens, expected %d; %s)" % (where, i, len(g["toks"]), len(w["toks"]), g.get("error"))
        if g.get("error") or g["bfinal"] != w["bfinal"] or g.get("bit_end") != w.get("bit_end"):
            return "%s: same header and tokens, but %s / final %d, expected %d" % (where, g.get("error"), g["bfinal"], w["bfinal"])
    if len(bg) != len(bw):
        return "%d blocks, expected %d" % (len(bg), len(bw))
    return None if got == want else "the same blocks, other bytes behind them (%d bytes, expected %d)" % (len(got), len(want))


def inflate(blocks):
    """the bytes a decode()d stream of compressed blocks stands for (no stored block among them)"""
    out = bytearray()
    for blk in blocks:
        assert blk["btype"] != 0
        for ln, v in blk["toks"]:
            if ln == 0:
                out.append(v)
            else:
                for _ in range(ln):
                    out.append(out[-v])
    return bytes(out)


# ---- what the oracle's stream says about each block -----------------------------------------------------------------------------
def block_histograms(stream):
    """per block of a stream: dict(btype, llf, df, clf, ll_lens, d_lens, cl_lens).  llf / df are the literal/length and
    distance frequencies as the encoder saw them -- end-of-block counted once, trimmed behind the last used symbol but never
    below 257 and 1 entries (huffman_lengths.rs:44-47) --, clf the frequencies of the run-coded ll_lens + d_lens.  A stored
    block has no histograms (None)."""
    out = []
    for blk in decode(stream):
        e = dict(btype=blk["btype"], llf=None, df=None, clf=None, ll_lens=blk.get("ll_lens"), d_lens=blk.get("d_lens"),
                 cl_lens=blk.get("cl_lens"), n_tok=len(blk["toks"]))
        if blk["btype"] != 0:
            llf, df = [0] * 286, [0] * 30
            for s in blk["ll_syms"]:
                llf[s] += 1
            for d in blk["d_syms"]:
                df[d] += 1
            n_ll = max(257, max(i + 1 for i in range(286) if llf[i]))
            n_d = max([1] + [i + 1 for i in range(30) if df[i]])
            e["llf"], e["df"] = llf[:n_ll], df[:n_d]
        if blk["btype"] == 2:
            assert len(e["ll_lens"]) == n_ll and len(e["d_lens"]) == n_d
            e["clf"] = ob.encode_lengths(e["ll_lens"] + e["d_lens"])[1]
        out.append(e)
    return out


def unlimited(freqs):
    """depth of the Huffman tree of a histogram before any limiter"""
    return max(ob.huffman_lengths(list(freqs), 31))


def runs_of(chain):
    """maximal runs of equal entries: [(start, end, value)]"""
    out, i = [], 0
    while i < len(chain):
        e = i + 1
        while e < len(chain) and chain[e] == chain[i]:
            e += 1
        out.append((i, e, chain[i]))
        i = e
    return out


def measure(data, level):
    """the figures a target speaks of, per block of the oracle's stream"""
    stream = ob.encode(data, opts=ob.make_opts(*LV[level]))
    out = []
    for h in block_histograms(stream):
        m = dict(btype=h["btype"])
        if h["btype"] == 2:
            m.update(ll_unl=unlimited(h["llf"]), d_unl=unlimited(h["df"]) if any(h["df"]) else 0, cl_unl=unlimited(h["clf"]),
                     m_ll=sum(1 for f in h["llf"] if f), m_d=sum(1 for f in h["df"] if f), n_tok=h["n_tok"],
                     chain=h["ll_lens"] + h["d_lens"], n_ll=len(h["ll_lens"]))
        out.append(m)
    return out


def check(case):
    """assert a case's target on the oracle's stream; returns measure()'s figures"""
    name, data, level, target = case
    got = measure(data, level)
    assert [m["btype"] for m in got] == [t["btype"] for t in target], (name, [m["btype"] for m in got])
    for b, (m, t) in enumerate(zip(got, target)):
        for key in ("ll_unl", "d_unl", "cl_unl", "m_ll", "m_d"):
            if key in t:
                assert m[key] == t[key], "%s block %d: %s is %d, the case wants %d" % (name, b, key, m[key], t[key])
        if "runs" in t:
            have = set(runs_of(m["chain"]))
            for r in t["runs"]:
                assert tuple(r) in have, "%s block %d: no run %s in %s" % (name, b, r, sorted(have))
        if t.get("seam"):
            n_ll = m["n_ll"]
            assert any(s < n_ll < e and v for s, e, v in runs_of(m["chain"])), (name, m["chain"][n_ll - 2:n_ll + 2])
    return got


# ---- generators ---------------------------------------------------------------------------------------------------------------------
def fib(k, first=(1, 2)):
    """k terms of the Fibonacci sequence that begins with `first`"""
    out = list(first)
    while len(out) < k:
        out.append(out[-1] + out[-2])
    return out[:k]


def hist_bytes(counts, seed):
    """bytes with exactly this histogram ({value: count}), shuffled"""
    a = bytearray()
    for v, c in sorted(counts.items()):
        a += bytes([v]) * c
    a = list(a)
    random.Random(seed).shuffle(a)
    return bytes(a)


def fib_block(k, seed, pad_to=0):
    """k byte values with counts 1, 2, 3, 5, 8, ...: with end-of-block's 1 in front the literal/length tree is one chain of
    depth k.  pad_to: more of the heaviest value up to that many bytes (the chain stays: only its last leaf grows)."""
    vals = random.Random(seed).sample(range(256), k)
    counts = dict(zip(vals, fib(k)))
    n = sum(counts.values())
    if pad_to:
        assert n <= pad_to
        counts[vals[-1]] += pad_to - n
    return hist_bytes(counts, seed + 1)


@functools.lru_cache(maxsize=None)
def fib_ll(k, seed):
    return fib_block(k, seed)


@functools.lru_cache(maxsize=None)
def fib_ll_three(ks, seed):
    """one full block of BLOCK_TOKENS literals per k, every block with a sample of byte values of its own"""
    return b"".join(fib_block(k, seed + 10 * i, pad_to=BLOCK_TOKENS) for i, k in enumerate(ks))


class _Lz:
    """Bytes whose LZ77 parse is known: literals that never complete a trigram seen before, and copies of chosen length and
    distance.  A count of every trigram is kept; a copy's source is taken only where all its trigrams have occurred once
    (so the hash chain offers this one candidate), the literal in front of a copy must make three new trigrams, and the byte
    behind a copy differs from the byte behind its source (so the match ends where it should)."""

    def __init__(self, seed, alphabet):
        self.r = random.Random(seed)
        self.out = bytearray()
        self.tri = Counter()
        self.alpha = list(alphabet)
        self.forbid = None

    def _push(self, b):
        o = self.out
        if len(o) >= 2:
            self.tri[(o[-2], o[-1], b)] += 1
        o.append(b)

    def lit(self, alphabet=None):
        o = self.out
        al = list(alphabet or self.alpha)
        self.r.shuffle(al)
        for b in al:
            if b != self.forbid and (len(o) < 2 or self.tri[(o[-2], o[-1], b)] == 0):
                self._push(b)
                self.forbid = None
                return b
        raise RuntimeError("no literal makes a new trigram here")

    def lits(self, n, alphabet=None):
        for _ in range(n):
            self.lit(alphabet)

    def match(self, lo, hi, length=4, tries=64):
        """one literal, then a copy of `length` bytes from a distance in lo..hi (fresh literals first where no source is
        eligible yet)"""
        o, tri = self.out, self.tri
        for _ in range(1000):
            p = len(o) + 1  # (where the copy will begin)
            d0, d1 = max(lo, length + 1), min(hi, p)
            if len(o) < 2 or d0 > d1:
                self.lits(max(1, d0 - d1 + 8))  # (nothing that far back yet)
                continue
            for _ in range(tries):
                d = self.r.randint(d0, d1)
                s = p - d
                if any(tri[(o[s + i], o[s + i + 1], o[s + i + 2])] != 1 for i in range(length - 2)):
                    continue
                b = self.r.choice(self.alpha)
                new = {(o[-2], o[-1], b), (o[-1], b, o[s]), (b, o[s], o[s + 1])}
                if b == self.forbid or len(new) != 3 or any(tri[t] for t in new):
                    continue
                self._push(b)
                for i in range(length):
                    self._push(o[s + i])
                self.forbid = o[s + length]
                return d
            self.lit()
        raise RuntimeError("no eligible source for a copy from %d..%d" % (lo, hi))

    def near(self, d, length=4, tries=400):
        """d fresh literals, then `length` bytes that repeat them: a match at distance d <= length.  No trigram of the unit
        has occurred before it (inside it they repeat, which is the match)"""
        o = self.out
        for _ in range(tries):
            unit = [self.r.choice(self.alpha) for _ in range(d)]
            for i in range(length):
                unit.append(unit[i])
            lead = len(o[-2:])
            seq = list(o[-2:]) + unit
            tris = [tuple(seq[i:i + 3]) for i in range(len(seq) - 2)]
            if unit[0] == self.forbid or any(self.tri[t] for t in tris) or len(set(tris[:lead]) | set(tris[lead:])) != lead + d:
                continue  # (the trigrams that reach back over the unit's start must not be the unit's own either)
            for b in unit:
                self._push(b)
            self.forbid = unit[length]  # (what the period would bring next)
            return
        raise RuntimeError("no fresh unit of period %d" % d)

    def done(self):
        self.lit()
        return bytes(self.out)


ALPHA64 = tuple(range(48, 112))


def code_range(c):
    return DBASE[c], DBASE[c] + (1 << DEXT[c]) - 1


@functools.lru_cache(maxsize=None)
def dist_counts(counts, seed, spare=0.0):
    """matches of length 4, counts[i] of them with distance code 4 + i (so the short distances, which need fresh literals
    in front, get the small counts), in shuffled order, one literal between two matches -- and a second one with
    probability `spare`: a match uses up one source and leaves about one new one behind, which is too few where thousands
    of matches draw on a window of 1 024 distances"""
    g = _Lz(seed, ALPHA64)
    g.lits(8)
    codes = [4 + i for i, c in enumerate(counts) for _ in range(c)]
    g.r.shuffle(codes)
    for c in codes:
        g.match(*code_range(c))
        if spare and g.r.random() < spare:
            g.lit()
    return g.done()


@functools.lru_cache(maxsize=None)
def dist_all30(seed):
    """every distance code used: two matches each, the distances below 5 as periodic runs"""
    g = _Lz(seed, ALPHA64)
    g.lits(8)
    for rep in range(2):
        for c in range(30):
            if c < 4:
                g.near(c + 1)
            else:
                g.match(*code_range(c))
    return g.done()


@functools.lru_cache(maxsize=None)
def all_286(seed):
    """every byte value and one match for every one of the 29 length codes (the base length of each) in one block"""
    g = _Lz(seed, range(256))
    perm = list(range(256))
    g.r.shuffle(perm)
    for b in perm:
        g._push(b)
    common = perm[:24]
    g.lits(3000, common)
    for ln in LBASE:
        g.match(ln + 1, len(g.out), length=ln, tries=400)
        g.lits(3, common)
    return g.done()


@functools.lru_cache(maxsize=None)
def seam_periods(seed, units, length):
    """matches of one length at the distances 1, 2, 3, 4 in equal numbers, 1 to 4 literals in front of each: the distance
    lengths are 2, 2, 2, 2, and the one length code -- the last literal/length symbol, more than a quarter of all tokens --
    gets length 2 as well"""
    g = _Lz(seed, ALPHA64)
    for u in range(units):
        g.near(1 + u % 4, length)
    return g.done()


@functools.lru_cache(maxsize=None)
def seam_runs(seed, units, length):
    """runs of 1 + length equal bytes, a new byte each: a literal and a match of `length` at distance 1, nothing else.  The
    one length code is half of all tokens and the one distance code is alone: both get length 1"""
    vals = random.Random(seed).sample(range(256), units)  # (every byte once: a run's trigram never comes back)
    return b"".join(bytes([b]) * (1 + length) for b in vals)


def used_symbols(m, seed):
    """m used literal/length symbols at huffman_only: m - 1 byte values (end-of-block is the m-th), one of them about 4 000
    times so that the dynamic block wins, the others 8 to 18 times"""
    vals = random.Random(seed).sample(range(256), m - 1)
    counts = {v: 8 + (7 * i) % 11 for i, v in enumerate(vals)}
    counts[vals[0]] = 4000
    return hist_bytes(counts, seed + 1)


def ties(n, each, heavy, seed):
    """n byte values `each` times each, and `heavy` times one more value (0: none)"""
    vals = random.Random(seed).sample(range(256), n + (1 if heavy else 0))
    counts = {v: each for v in vals[:n]}
    if heavy:
        counts[vals[n]] = heavy
    return hist_bytes(counts, seed + 1)


# Code lengths chosen outright: frequencies 2^(top - length), which sum to 2^top with end-of-block's 1.  The entropy bound is
# then met with equality, and only by these lengths, so every Huffman builder must find exactly them.
F = ("f",)


def layout(segments, top, seed):
    """256 code lengths from segments ('z', n) n unused values, ('r', n, length) n values of one length, F one value whose
    length is chosen here: the F values share what the others and end-of-block leave of 2^top, each a power of two"""
    fixed = sum(s[1] << (top - s[2]) for s in segments if s[0] == "r")
    slots = sum(1 for s in segments if s == F)
    rest = (1 << top) - 1 - fixed
    assert rest >= 0 and slots > 0
    parts = [1 << j for j in range(top) if rest >> j & 1]
    assert rest < (1 << top) and len(parts) <= slots, (rest, slots)
    while len(parts) < slots:  # split the smallest part that can be split: the heavy values stay heavy
        parts.sort()
        i = next(i for i, p in enumerate(parts) if p > 1)
        p = parts.pop(i)
        parts += [p // 2, p // 2]
    random.Random(seed).shuffle(parts)
    lens, runs = [], []
    for s in segments:
        if s == F:
            lens.append(top - parts.pop().bit_length() + 1)
        elif s[0] == "z":
            runs.append((len(lens), len(lens) + s[1], 0))
            lens += [0] * s[1]
        else:
            runs.append((len(lens), len(lens) + s[1], s[2]))
            lens += [s[2]] * s[1]
    assert len(lens) == 256, len(lens)
    if lens[255] == top:  # (end-of-block, entry 256, has the top length: the run goes on over it)
        runs[-1] = (runs[-1][0], 257, top)
    return lens, runs


def dyadic_bytes(lens, seed):
    top = max(lens)
    counts = {v: 1 << (top - l) for v, l in enumerate(lens) if l}
    assert sum(counts.values()) + 1 == 1 << top
    return hist_bytes(counts, seed)


def tail(n):
    """n entries: single values between short runs of unused ones, a value first and last"""
    segs, left, k = [], n, 0
    while left > 0:
        segs.append(F)
        left -= 1
        z = min(1 + k % 3, left - 1)
        if z > 0:
            segs.append(("z", z))
            left -= z
        k += 1
    return segs


def Z(n):
    return ("z", n)


def R(n, l):
    return ("r", n, l)


TOP = 12  # 4 095 bytes a case
RUN_LAYOUTS = {
    # zero runs of every coded form: literal zeros (1, 2), symbol 17 (3, 10), symbol 18 (11, 138); non-zero runs 3 (one
    # copy symbol), 4, 6 (literal + 3 / 5 copies), 7 (a full copy of 6), 8 (6 and a literal)
    "zero_1_2_3_10_11_138": [F, Z(1), F, Z(2), F, Z(3), F, Z(10), F, Z(11), F, Z(138), F, R(3, 9), F, R(4, 10), F, R(6, 9), F,
                             R(7, 10), F, R(8, 9), F, Z(50), F],
    "zero_139": [Z(139)] + tail(117),
    "zero_140": tail(41) + [Z(140)] + tail(75),
    "zero_141": tail(60) + [Z(141)] + tail(55),
    "zero_149": tail(40) + [Z(149)] + tail(67),
    # from below 64 to beyond 128 and 192: the chunks 64..127 and 128..191 hold no run start
    "zero_10_to_200": tail(10) + [Z(190)] + tail(56),
    # non-zero: 128 equal lengths over two chunk seams
    "run_128": tail(31) + [R(128, 8)] + tail(97),
    "run_128_from_0": [R(128, 8)] + tail(128),
    # a run start at exactly 64 (zeros), 128 (non-zero), 192 (zeros); 256 is end-of-block, a run of its own behind a zero
    "starts_64_128_192_256": tail(64) + [Z(30)] + tail(34) + [R(6, 10)] + tail(58) + [Z(11)] + tail(52) + [Z(1)],
    # the same seams met from the other side: runs that end exactly at 64, 128, 192 and one over 256 (value 255 and
    # end-of-block share the top length)
    "ends_64_128_192": tail(50) + [Z(14)] + tail(50) + [R(7, 9), Z(7)] + tail(49) + [Z(15)] + tail(61) + [R(3, TOP)],
}
CL_AT_LIMIT = ("zero_139", "zero_140", "zero_141", "run_128", "starts_64_128_192_256")  # code-length tree of depth 7: no limiter
RUN_SEEDS = {"zero_1_2_3_10_11_138": 2, "zero_139": 6, "zero_141": 6, "run_128": 2, "run_128_from_0": 2, "ends_64_128_192": 12}


@functools.lru_cache(maxsize=None)
def run_case(name):
    lens, runs = layout(RUN_LAYOUTS[name], TOP, RUN_SEEDS.get(name, 1))
    return dyadic_bytes(lens, 7), tuple(runs)


@functools.lru_cache(maxsize=None)
def cl_case(per_length, seed):
    """per_length[i] values of code length i + 1 (end-of-block is one of the longest), the other values unused, in an order
    drawn from seed: the search of family c varies these until the code-length histogram's tree is deeper than 7"""
    lens = [l + 1 for l, n in enumerate(per_length) for _ in range(n)]
    top = max(lens)
    lens.remove(top)
    assert len(lens) <= 256 and sum(1 << (top - l) for l in lens) + 1 == 1 << top
    lens += [0] * (256 - len(lens))
    random.Random(seed).shuffle(lens)
    return dyadic_bytes(lens, seed + 1)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
CL_HITS = (  # (values per code length 1, 2, 3, ...; seed of the order; unlimited depth of the code-length tree)
    ((0, 0, 0, 1, 25, 1, 14, 5, 2, 8), 685620, 8),
    ((0, 0, 1, 8, 8, 4, 3, 1, 11, 7, 14), 24726, 8),
    ((0, 0, 0, 1, 2, 5, 62, 37, 59, 54), 806886, 8),
    ((0, 0, 1, 2, 3, 23, 20, 19, 11, 33, 5, 18, 34, 28), 328755, 8),
    ((0, 0, 1, 1, 3, 21, 36, 12, 4, 33, 46), 267210, 9),
    ((0, 0, 1, 0, 8, 23, 4, 32, 37, 30, 1, 23, 14), 374892, 9),
    ((0, 0, 2, 1, 2, 24, 5, 28, 30, 20, 24, 35, 9, 34), 695328, 9),
)


def _dyn(**kw):
    return [dict(btype=2, **kw)]


def _table_of_cases():
    """name -> (data maker, level, target).  The figures are what the oracle gives for these seeds (measure()); check()
    holds every case to them."""
    t = {}
    # a. literal/length limiter.  k byte values + end-of-block: unlimited depth k -- 15 (the limiter must not fire), 16, 17,
    #    20 (the deepest one block can hold: depth 21 needs 46 366 tokens).  Sizes 2 582, 4 179, 6 763, 28 655 bytes.
    for k in (15, 16, 17, 20):
        t["a_fib%d" % k] = (lambda k=k: fib_ll(k, 100 + k), "huffman_only", _dyn(ll_unl=k, m_ll=k + 1, m_d=0))
    #    three full blocks in one input, a chain of its own in each; the reference closes the input with an empty fixed block
    t["a_three_blocks"] = (lambda: fib_ll_three((17, 15, 20), 300), "huffman_only",
                           [dict(btype=2, ll_unl=17), dict(btype=2, ll_unl=15), dict(btype=2, ll_unl=20), dict(btype=1)])
    #    the same bytes at default: equal neighbours become matches, the tree gets length codes (depths 9, 10, 11, 13 with
    #    distance trees of depth 9, 8, 9, 11: nothing over the limit, a plain parity case with 22 to 30 distance codes)
    for k, ll, d, m_d in ((15, 9, 9, 22), (16, 10, 8, 24), (17, 11, 9, 25), (20, 13, 11, 30)):
        t["a_fib%d_default" % k] = (lambda k=k: fib_ll(k, 100 + k), "default", _dyn(ll_unl=ll, d_unl=d, m_d=m_d))
    # b. distance limiter.  n distance codes with counts 1, 1, 2, 3, 5, ...: unlimited depth n - 1 -- 15 (no limiter), 16,
    #    17, 18 at default and best (14 018, 22 136, 35 897, 60 160 bytes; 6 269 to 27 325 tokens, one block).  At fast the
    #    parse differs (depth 15, 15, 16, 16): parity, and the limiter for the last two.
    for n, spare in ((16, 0.0), (17, 0.0), (18, 0.0), (19, 0.3)):
        mk = lambda n=n, spare=spare: dist_counts(tuple(fib(n, (1, 1))), 500 + n, spare)
        for level in ("default", "best"):
            t["b_dist%d_%s" % (n, level)] = (mk, level, _dyn(d_unl=n - 1, m_d=n))
        t["b_dist%d_fast" % n] = (mk, "fast", _dyn(m_d=n))
    # c. code-length limiter (max 7).  Found by a walk over complete length profiles (split a length into two of the next,
    #    or join two) that keeps what deepens the tree of the run-coded table; per_length, seed -> unlimited depth below.
    for i, (per_length, seed, depth) in enumerate(CL_HITS):
        t["c_cl%d_depth%d" % (i, depth)] = (lambda p=per_length, s=seed: cl_case(p, s), "huffman_only", _dyn(cl_unl=depth))
    # d. number of used symbols: the rank sort takes (m + 63) / 64 keys a lane, and 0 / 1 symbols are cases of their own
    for m in (2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257):
        t["d_m%d" % m] = (lambda m=m: used_symbols(m, 1000 + m), "huffman_only", _dyn(m_ll=m, m_d=0))
    t["d_m286"] = (lambda: all_286(11), "default", _dyn(m_ll=286, m_d=9, cl_unl=7))
    t["d_dist_1_code"] = (lambda: dist_counts((0, 0, 0, 0, 0, 0, 40), 13), "default", _dyn(m_d=1))
    t["d_dist_2_codes"] = (lambda: dist_counts((0, 0, 0, 0, 30, 0, 0, 0, 0, 0, 0, 50), 14), "default", _dyn(m_d=2))
    t["d_dist_30_codes"] = (lambda: dist_all30(12), "default", _dyn(m_d=30))
    t["d_tie_64"] = (lambda: ties(64, 100, 0, 5), "huffman_only", _dyn(m_ll=65, ll_unl=7))
    t["d_tie_128_and_heavy"] = (lambda: ties(128, 50, 4000, 6), "huffman_only", _dyn(m_ll=130, ll_unl=9))
    t["d_tie_256_stored"] = (lambda: ties(256, 20, 0, 7), "huffman_only", [dict(btype=0)])  # (parity of the cost fields only)
    # e. the run coder.  Every run a layout names must be there, from its first to its last entry (the layouts' own short
    #    zero runs between single values included)
    for name in RUN_LAYOUTS:
        t["e_" + name] = (lambda name=name: run_case(name)[0], "huffman_only", name)
    t["e_zero_255"] = (lambda: bytes([255]) * 4000, "huffman_only", _dyn(m_ll=2, runs=[(0, 255, 0), (255, 257, 1), (257, 258, 0)]))
    #    over the seam between the literal/length and the distance lengths (entry 258, 259, 263 and 265 of the chain)
    for ln, n_ll in ((3, 258), (4, 259), (8, 263)):
        t["e_seam_periods_len%d" % ln] = (lambda ln=ln: seam_periods(15, 240, ln), "default",
                                          _dyn(m_d=4, seam=True, runs=[(n_ll - 1, n_ll + 4, 2)]))
    for level in ("default", "rle"):
        t["e_seam_runs_" + level] = (lambda: seam_runs(16, 128, 10), level, _dyn(m_d=1, seam=True, runs=[(264, 266, 1)]))
    return t


_CASES = None


def names():
    global _CASES
    if _CASES is None:
        _CASES = _table_of_cases()
    return list(_CASES)


def level_of(name):
    names()
    return _CASES[name][1]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (name, data, level, target)"""
    names()
    make, level, target = _CASES[name]
    if isinstance(target, str):  # a run layout: its runs are its target
        target = _dyn(runs=list(run_case(target)[1]), **({"cl_unl": 7} if target in CL_AT_LIMIT else {}))
    return name, make(), level, target


def cases():
    return [case(n) for n in names()]
