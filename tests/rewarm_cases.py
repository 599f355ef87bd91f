"""Inputs whose first block fills its 31 744 tokens inside the first window, so that the reference warms its rolling hash up again
with data[0], data[1] (quirk Q1, lz77.rs:628-638) and files the next two positions, w and w + 1, under hashes that are not their
bytes'.  Three things follow, and the one-shot path has code for each that no other input reaches: the predicate (kernels
q1_rewarm in k_small_fix / k_block_bounds, and the host's in run_encode, run_streamed and the batch), the second pass
(launch_match_tables with ident and redo_head: k_links_a files w and w + 1 through stages.h rewarm_ab, k_links_b starts every
bucket at the head table's identity entry, k_match<HAS_Q> walks the first MI355_IDENT_EPOCHS epochs plus 4 096 positions, k_sort
and k_match3 take over from there), and the identity hops: a chain that runs out goes on at "the position numbered like the
hash", which after a re-warm can be w or w + 1 -- a real match that no bucket holds.

Everything is generated here from fixed seeds; no data file is committed.  A case is dict(name, family, data, opts, targets,
claims).  `claims` holds in_bytes (the bytes of block 0, asserted on the oracle's trace_blocks() with n_lz == 31 744), fires and w
(what q1() must give on the oracle's own tokens; w is where the re-warm happens or would have happened), and kinds, the claim
kinds of CLAIM_KINDS the case as a whole stands for.  A target is dict(p, kind, mutant, tok): the position whose token the
oracle decides, its claim kind, the mutant of the model that must predict another token there (None for a control), and -- where
the builder knows it -- the token itself.

The model.  q1() restates the predicate.  filing() is the hash every position is filed under (rewarm_ab).  chain() is the list
of positions longest_match visits from p: the bucket, nearest first, and behind its oldest entry the head table's identity entry
(chained_hash_table.rs:64-69 head[h] = h and prev[n] = n; :118-158 a new entry's predecessor is head[h]; :197-219 a slide turns
every entry that pointed below the buffer into "the position numbered like its index").  Before position 65 536 an empty bucket h
goes on at position h, from 65 536 on at 32 768 + h (the buffer's start after each slide, + h), and from there down that
position's own chain; an entry filed before the last slide has lost its identity successor (it points at itself: the walk
ends).  match_cases.walk runs over that list with the window and the budget.  predict() gives the token at a target, from the
match of p - 1 on a lazy level.  check() holds every case to the oracle alone: block 0, the predicate, every target's token,
and that the named mutant predicts another one -- a case that stops provoking its situation fails instead of passing
empty-handed.  tests/test_rewarm_cases.py (CPU) and tests/test_rewarm_gpu.py use the cases.

The builder generalises the Filler of tests/golden/gen_identity_hop.py: bytes over 64 symbols (0x40..0x7F: the blocks come out
dynamic, not stored) in which no three bytes occur twice and no reserved hash is produced; first_block() makes a head whose
first 31 744 tokens -- literals and matches of exactly three bytes from a fixed distance back, each of which moves w by two, one
of four bytes for odd shifts -- end where asked, on a literal or on a match.
"""
import functools
import random
import zlib

import numpy as np

import datagen
import match_cases as mc
import oracle_binding as ob
from header_cases import decode

W = 32768        # stages.h WINDOW_SIZE
BLOCK = 31744    # stages.h MAX_BUFFER_LENGTH (output_writer.rs:19)
IDENT_EPOCHS = 3  # deflate_host.inc MI355_IDENT_EPOCHS
LINK_TAIL = 4096  # launch_match_tables: n_old = e_first * WINDOW_SIZE + 4096
HOST_PIECEWISE_FROM = 16 << 20  # deflate_host.inc HOST_PIECEWISE_FROM: the streamed host call
FAST, DEFAULT, BEST, GREEDY128 = (1, 0, 0), (128, 32, 1), (1768, 128, 1), (128, 0, 0)
TWO = (2, 8, 1)  # the custom level: two checks, lazy below 8
LEVEL_NAMES = {FAST: "fast", DEFAULT: "default", BEST: "best", GREEDY128: "greedy128", TWO: "two"}
MUTANTS = ("no_rewarm", "no_hops", "hops_two_epochs", "second_not_refiled", "rewarm_anyway")
LIMIT = 140000   # inputs are no longer, but in the family `paths`

hash3 = mc.hash3


# ---- the model -----------------------------------------------------------------------------------------------------------------------
def tokens_of(stream, blocks=0):
    """[(position, token)] of a raw stream, in order; blocks: of its first blocks only"""
    out, pos = [], 0
    for blk in decode(stream, blocks=blocks):
        if blk.get("stored") is not None:
            if blk["stored"]:
                out.append((pos, ("stored", blk["stored"])))
                pos += blk["stored"]
            continue
        for ln, v in blk["toks"]:
            out.append((pos, ("lit", v) if ln == 0 else ("ld", ln, v)))
            pos += ln or 1
    return out


def q1(tokens, opts, n):
    """(fires, w): q1_rewarm of deflate_kernels.hip on the 31 744th token of the stream, where there is one.  lz77.rs:628-638:
    the call of lz77_compress_block that follows a full block warms the hash up again if it is still in the first window; the
    position it files next is w.  Lazy (lz77.rs:310-420): the encoder stands one behind the last token's first byte, a literal
    leaves it at tp + 1 with tp + 2 the next position to file -- tp + 1 if that has no third byte; greedy: at tp."""
    if len(tokens) < BLOCK:
        return False, None
    tp, tok = tokens[BLOCK - 1]
    cover = tok[1] if tok[0] == "ld" else 1
    if opts[2] == 1:
        lp = tp + 1
        w = tp + cover if tok[0] == "ld" else (tp + 2 if (tp + 1) + 2 < n else tp + 1)
    else:
        lp, w = tp, tp + cover
    return (lp < W and w <= W), w


def filing(data, w, mutant=None):
    """the hash every position is filed under after a re-warm at w (stages.h rewarm_ab): w under data[0], data[1] and its own
    third byte, w + 1 under data[1] and its own second and third"""
    fh = mc._hashes(data).astype(np.int64).copy()
    if w is None or mutant == "no_rewarm":
        return fh
    if w + 2 < len(data):
        fh[w] = hash3(data[0], data[1], data[w + 2])
    if w + 3 < len(data) and mutant != "second_not_refiled":
        fh[w + 1] = hash3(data[1], data[w + 2], data[w + 3])
    return fh


def base_of(p):
    """the stream position of the reference's buffer start while it looks at p (input_buffer.rs slide: one window at a time,
    from the end of the second on)"""
    return 0 if p < 2 * W else (p // W - 1) * W


def chain(fh, p, mutant=None):
    """(positions longest_match visits from p, nearest first -- window and budget not applied --, the hops among them)"""
    B, cur, out, hops = base_of(p), p, [], []
    ident = mutant != "no_hops" and not (mutant == "hops_two_epochs" and p >= 2 * W)
    while cur < len(fh):
        H = int(fh[cur])
        idx = (np.nonzero(fh[B:cur] == H)[0][::-1] + B).tolist()
        out += idx
        e0 = idx[-1] if idx else cur
        if not ident or base_of(e0) != B:  # (:197-219: the oldest entry was filed before the last slide and points at itself)
            break
        q = B + H
        if q >= e0 or p - q > W:  # matching.rs:127-132: not below the entry it came from, or out of the window
            break
        out.append(q)
        hops.append(q)
        if q == p - W:  # (prev[] is indexed modulo the window: p's own entry has replaced q's)
            break
        cur = q
    return out, hops


def _model(c, mutant=None):
    cl = c["claims"]
    on = cl["fires"] or mutant == "rewarm_anyway"
    return filing(c["data"], cl["w"] if on else None, mutant)


def predict(c, t, mutant=None, detail=False):
    """(position, token) the model gives for a target; detail: and the walk's visits and hops"""
    data, opts, p = c["data"], c["opts"], t["p"]
    fh = _model(c, mutant)
    prev = (0, 0)
    if opts[2] == 1 and p > 0:  # the walk at p starts from the match of p - 1
        prev = mc.walk(data, p - 1, opts[0], chain=chain(fh, p - 1, mutant)[0])[0]
        if prev[0] < 3 or (prev[0] == 3 and prev[1] > 8192):
            prev = (0, 0)
    ch, hops = chain(fh, p, mutant)
    res = mc.predict(data, dict(p=p, prev=prev), opts, chain=ch)
    if detail:
        return res, mc.walk(data, p, mc.quarter(opts, prev[0]), prev[0], chain=ch)[1], hops
    return res


def chain_text(c, p):
    """the model's chain for a position, for the diff helper"""
    cl = c["claims"]
    (_, tok), visits, hops = predict(c, dict(p=p), detail=True)
    vs = ["%d%s%s" % (v["q"], "*" if v["q"] in hops else "", ("=%d" % v["length"]) if v["hit"] else "") for v in visits[:12]]
    return "w %s (%s), the model's token %s, its chain position[*: through an identity entry][=compared length] %s%s" % (
        cl["w"], "fires" if cl["fires"] else "does not fire", tok, " ".join(vs) or "(empty)", " ..." if len(visits) > 12 else "")


def rewarm_diff(got, want, c):
    """Where two streams of a case part: the first differing token, its input position and epoch, w, and the model's chain for
    that position.  None for streams that read the same."""
    if got == want:
        return None
    fg, fw = mc._flat(got), mc._flat(want)
    pos = 0
    for i, (g, w) in enumerate(zip(fg, fw)):
        if g != w:
            break
        pos += w[1][1] if w[1][0] in ("ld", "stored") else 1
    else:
        i = min(len(fg), len(fw))
        if len(fg) == len(fw):
            return "%s: the same tokens in other bytes (%d bytes, expected %d): a header or a block boundary differs" % (c["name"], len(got), len(want))
    g = fg[i][1] if i < len(fg) else None
    w = fw[i][1] if i < len(fw) else None
    msg = "%s: token %d at input position %d (epoch %d, offset %d): got %s, expected %s" % (c["name"], i, pos, pos // W, pos % W, g, w)
    if pos < len(c["data"]):
        msg += "; " + chain_text(c, pos)
    for t in c["targets"]:
        if t["p"] - 1 <= pos <= t["p"] + 1:
            msg += "; target at %d (%s, mutant %s)" % (t["p"], t["kind"], t["mutant"])
            break
    return msg


# ---- the builder ---------------------------------------------------------------------------------------------------------------------
class Filler:
    """bytes over 0x40..0x7F whose trigrams are all different (no match of three bytes anywhere) and never hash to a reserved
    value; copies and fixed bytes where asked"""

    def __init__(self, seed, reserved=(), o=b"", seen=(), avoid=()):
        self.r = random.Random(seed)
        self.reserved = set(reserved)
        self.o = bytearray(o)
        self.seen = set(seen)
        self.avoid = set(avoid)  # the byte that would lengthen the copy just made

    def new(self, *tris):
        return len(set(tris)) == len(tris) and all(t not in self.seen and hash3(*t) not in self.reserved for t in tris)

    def push(self, bs):
        for x in bs:
            self.o.append(x)
            if len(self.o) >= 3:
                self.seen.add(tuple(self.o[-3:]))

    def lit(self, n=1, follow=(), avoid=()):
        """n new bytes; the last one so that its trigrams with the known bytes behind it are new as well"""
        for i in range(n):
            fol = list(follow[:2]) if i == n - 1 else []
            av = self.avoid | (set(avoid) if i == n - 1 else set())
            for _try in range(4000):
                x = 0x40 + self.r.randrange(64)
                if x in av:
                    continue
                seq = list(self.o[-2:]) + [x] + fol
                if len(seq) < 3 or self.new(*[tuple(seq[j:j + 3]) for j in range(len(seq) - 2)]):
                    break
            else:
                raise RuntimeError("no byte fits at %d" % len(self.o))
            self.avoid = set()
            self.push([x])

    def fixed(self, bs, fresh=True):
        """those bytes; fresh: every trigram they complete must be new"""
        assert not self.avoid or bs[0] not in self.avoid
        self.avoid = set()
        for x in bs:
            if fresh and len(self.o) >= 2 and not self.new((self.o[-2], self.o[-1], x)):
                raise RuntimeError("the fixed bytes at %d repeat a trigram or make a reserved hash" % len(self.o))
            self.push([x])

    def to(self, pos, follow=(), avoid=()):
        assert pos >= len(self.o), "%d bytes too late for %d" % (len(self.o) - pos, pos)
        if pos > len(self.o):
            self.lit(pos - len(self.o), follow, avoid)

    def copy_at(self, P, src, m):
        """m bytes of src at P exactly: the byte in front differs from the one in front of src, the one behind will differ too"""
        if len(self.o) < src + m + 1:
            self.to(src + m + 1)
        cp = bytes(self.o[src:src + m])
        assert len(cp) == m and P > len(self.o)
        self.to(P, follow=cp, avoid=(self.o[src - 1],) if src else ())
        self.push(cp)
        self.avoid = {self.o[src + m]}
        return P


@functools.lru_cache(maxsize=None)
def first_block(total, last="lit", seed=1, back=40, reserved=(), lead=b"", plants=()):
    """A head of `total` bytes that the parse of every level takes as exactly 31 744 tokens: literals, matches of exactly three
    bytes from `back` positions back, one of four where total - 31 744 is odd; the 31 744th token is a literal or a match, as
    asked.  lead: the first bytes; plants: ((position, bytes), ...) inside a stretch of literals.  -> (bytes, trigrams, avoid)"""
    extra = total - BLOCK
    four = extra % 2
    three = (extra - 3 * four) // 2
    assert extra >= 0 and three >= 0, total
    nm = three + four
    assert nm or last == "lit"
    slots = nm if last == "match" else nm + 1
    match_at = {BLOCK * k // slots - 1: (4 if (k == 1 and four) else 3) for k in range(1, nm + 1)}
    assert len(match_at) == nm and (not nm or min(match_at) > back + 4)
    plants = dict(plants)
    f = Filler(seed, reserved)
    forced = list(lead)
    for t in range(BLOCK):
        o = f.o
        if t in match_at:
            m = match_at[t]
            src = len(o) - back
            f.push(bytes(o[src:src + m]))
            f.avoid = {o[src + m]}
        elif forced:
            f.fixed([forced.pop(0)], fresh=len(o) >= len(lead))
        elif t + 1 in match_at:
            src = len(o) + 1 - back
            f.lit(1, follow=bytes(o[src:src + 2]), avoid=(o[src - 1],))
        elif len(o) + 1 in plants:
            forced = list(plants.pop(len(o) + 1))
            f.lit(1, follow=forced)
        else:
            f.lit(1)
    assert len(f.o) == total and not forced and not plants, (len(f.o), total, plants)
    return bytes(f.o), frozenset(f.seen), frozenset(f.avoid)


def head_total(opts, w, last="lit"):
    """the bytes of a first block that leaves the re-warm (or what would have been one) at w"""
    return w - 1 if (opts[2] == 1 and last == "lit") else w


def resume(opts, w, last="lit", seed=1, reserved=(), **kw):
    """a Filler that stands behind such a head"""
    total = head_total(opts, w, last)
    o, seen, avoid = first_block(total, last, seed, reserved=tuple(sorted(reserved)), **kw)
    return Filler(seed + 1000, reserved, o, seen, avoid), total


def tri_for(h, g=None, second=None, first_of=(0x40, 0x80)):
    """three bytes that hash to h (second: four bytes, the last three of which hash to that) -- new ones for the Filler g, from the
    alphabet where that can be had"""
    for lo, hi in (first_of, (0, 256)):
        for b in range(lo, hi):
            for a in range(lo, hi):
                c = (h ^ ((a & 31) << 10) ^ (b << 5)) & 0x7FFF
                if c > 255 or hash3(a, b, c) != h:
                    continue
                out = [a, b, c]
                if second is not None:
                    d = (second ^ ((b & 31) << 10) ^ (c << 5)) & 0x7FFF
                    if d > 255 or hash3(b, c, d) != second:
                        continue
                    out.append(d)
                tris = [tuple(out[i:i + 3]) for i in range(len(out) - 2)]
                if g is None or all(t not in g.seen for t in tris):
                    return bytes(out)
    raise RuntimeError("no trigram for %s" % h)


def _case(name, family, opts, g, n, targets, in_bytes, fires, w, kinds):
    g.to(n)
    data = bytes(g.o)
    assert len(data) == n and (n <= LIMIT or family == "paths"), (name, n)
    return dict(name=name, family=family, data=data, opts=opts, targets=targets,
                claims=dict(in_bytes=in_bytes, fires=fires, w=w, kinds=tuple(kinds)))


def T(p, kind, mutant, tok=None):
    return dict(p=p, kind=kind, mutant=mutant, tok=tok)


def _probe(g, P, w, fires, m=9):
    """a copy of data[w .. w + m) at P: with the re-warm w and w + 1 are in no bucket a copy of them looks into -- literals at P and
    P + 1, the rest from P + 2; without it the whole copy"""
    g.copy_at(P, w, m)
    if fires:
        return [T(P, "probe_missing", "no_rewarm", ("lit", g.o[P])), T(P + 1, "probe_missing_second", "second_not_refiled", ("lit", g.o[P + 1])),
                T(P + 2, "probe_rest", None, ("ld", m - 2, P - w))]
    return [T(P, "probe_found", "rewarm_anyway", ("ld", m, P - w))]


# ---- predicate: each edge of q1_rewarm as a pair, one fires and one does not -----------------------------------------------------------
def _predicate(name, opts, w, last, fires, n=45000, P=40000):
    """w: where the re-warm happens, or would have: the pair differs by one byte of the head"""
    g, total = resume(opts, w, last, seed=11 + w % 7, back=6 if opts[0] < 3 else 40)
    ts = _probe(g, P, w, fires)
    edge = "%s_%s" % ("lazy" if opts[2] else "greedy", last)
    return _case(name, "predicate", opts, g, n, ts, total, fires, w, ["%s_%s" % (edge, "fires" if fires else "quiet")])


def _clause(name, n):
    """the clause (tp + 1) + 2 < n of the lazy arm, tp = 31 743: an input that ends 0 to 4 bytes behind the full block"""
    o, seen, avoid = first_block(BLOCK, "lit", 12)
    g = Filler(13, (), o, seen, avoid)
    tp = BLOCK - 1
    w = tp + 2 if (tp + 1) + 2 < n else tp + 1
    return _case(name, "predicate", DEFAULT, g, n, [], BLOCK, True, w, ["clause_n_tp_plus_%d" % (n - tp)])


def _beyond(name):
    """block 0 is full, but ends beyond the first window: no Q1"""
    w = W + 300
    g, total = resume(DEFAULT, w, "lit", seed=14)
    ts = _probe(g, 40000, w, False)
    c = _case(name, "predicate", DEFAULT, g, 45000, ts, total, False, w, ["full_beyond_window"])
    for t in c["targets"]:  # (no re-warm can happen beyond the window: nothing to mutate)
        t["mutant"] = None
    return c


# ---- filing: where w and w + 1 lie in the batches of k_links_a, and what else lies in their foreign buckets ------------------------------
def _filing_mod(name, w):
    g, total = resume(DEFAULT, w, "lit", seed=21 + w % 5)
    ts = _probe(g, 40000, w, True)
    kinds = ["w_mod64_%d" % (w % 64)] + (["w_mod256_255"] if w % 256 == 255 else [])
    return _case(name, "filing", DEFAULT, g, 45000, ts, total, True, w, kinds)


LEAD = bytes([0x41, 0x52])  # data[0], data[1] where the foreign hash has to be known while the head is made
C_W2 = 0x63                 # and data[w + 2]


def _foreign_tris():
    """two different trigrams with the foreign hash F = hash3(data[0], data[1], data[w + 2]): the real candidate's and a miss"""
    b0, b1 = LEAD
    t1, t2 = bytes([b0 ^ 0x20, b1, C_W2]), bytes([b0 ^ 0x20, b1 ^ 1, C_W2 ^ 0x20])
    assert hash3(*t1) == hash3(*t2) == hash3(b0, b1, C_W2) and t1 != t2
    return t1, t2


def _foreign(name, dx, kind):
    """Level `two` (two checks).  Y, far in front of w, holds the trigram of the foreign hash F and six more bytes; X = w + dx holds
    a miss of hash F; the target is a copy of Y.  Its chain is X and w in either order, then Y: with w filed under F the two
    checks are gone before Y and the token is a literal, without the re-warm it is the match."""
    w, Y = 31765, 20000
    t1, t2 = _foreign_tris()
    X = w + dx
    plants = [(Y, t1)] + ([(X, t2)] if X < w - 8 else [])
    g, total = resume(TWO, w, "lit", seed=31, lead=LEAD, plants=tuple(plants))
    if X > w:
        g.to(w + 2, follow=[C_W2])
        g.fixed([C_W2])
        g.to(X, follow=t2)
        g.fixed(t2)
    else:
        assert X < w - 8
        g.to(w + 2, follow=[C_W2])
        g.fixed([C_W2])
    P = 36000
    g.copy_at(P, Y, 9)
    assert {"in_batch_below": X // 64 == w // 64 and X < w, "in_batch_above": X // 64 == w // 64 and X > w, "batch_before": X // 64 == w // 64 - 1,
            "other_group_of_512": abs(X - w) >= 512}[kind], (name, X, w)
    return _case(name, "filing", TWO, g, 40000, [T(P, "foreign_" + kind, "no_rewarm", ("lit", g.o[P]))], total, True, w, ["foreign_" + kind])


def _foreign_fast(name):
    """Fast (one check, greedy): a target in bucket F with its real candidate in front of w -- the one check goes to w"""
    w, Y = BLOCK, 20000
    t1, _ = _foreign_tris()
    g, total = resume(FAST, w, "lit", seed=32, lead=LEAD, plants=((Y, t1),))
    g.to(w + 2, follow=[C_W2])
    g.fixed([C_W2])
    P = 36000
    g.copy_at(P, Y, 9)
    return _case(name, "filing", FAST, g, 40000, [T(P, "foreign_fast", "no_rewarm", ("lit", g.o[P]))], total, True, w, ["foreign_fast"])


def _own_hash(name, second):
    """controls: the bytes at w (at w + 1) are such that the foreign hash is the hash of the position's own three bytes -- Q1 fires,
    and that position is found where it always was"""
    w = 32001
    g, total = resume(DEFAULT, w, "lit", seed=33 + second)
    b0, b1 = g.o[0], g.o[1]
    if not second:  # data[w] = data[0] mod 32, data[w + 1] = data[1]
        g.to(w, follow=[b0 ^ 0x20, b1])
        g.fixed([b0 ^ 0x20, b1])
    else:           # data[w + 1] = data[1] mod 32
        g.to(w + 1, follow=[b1 ^ 0x20])
        g.fixed([b1 ^ 0x20])
    P = 40000
    g.copy_at(P, w, 9)
    if not second:
        ts = [T(P, "own_hash_first", None, ("ld", 9, P - w))]
    else:
        ts = [T(P, "probe_missing", "no_rewarm", ("lit", g.o[P])), T(P + 1, "own_hash_second", None, ("ld", 8, P - w))]
    return _case(name, "filing", DEFAULT, g, 45000, ts, total, True, w, ["own_hash_second" if second else "own_hash_first"])


# ---- hop: the identity entry leads to w or w + 1 -------------------------------------------------------------------------------------------
def _hop(name, opts, w, where, P, n, kinds, last="lit", misses=0, found=True, back=40):
    """where: `w` (the three bytes at w hash to w mod 32 768, the target is a copy of them), `w1` (those at w + 1 hash to w + 1) or
    `both`.  misses: that many positions of the target's hash between w and the target -- real chain entries in front of the hop."""
    hw, hw1 = w % W, (w + 1) % W
    res = {hw, hw1} if where == "both" else {hw} if where == "w" else {hw1}
    g, total = resume(opts, w, last, seed=41 + w % 11 + len(where), reserved=res, back=back)
    g.reserved = set()
    if where == "w1":
        z = tri_for(hw1, g)
        g.to(w + 1, follow=z)
        g.fixed(z)
        src = w + 1
    else:
        z = tri_for(hw, g, second=hw1 if where == "both" else None)
        g.to(w, follow=z)
        g.fixed(z)
        src = w
    g.reserved = set(res)
    if misses:  # the same hash, another first byte: five bytes apart
        miss = bytes([z[0] ^ 0x20, z[1], z[2]])
        assert hash3(*miss) == hash3(*z[:3]) and where != "both"
        g.lit(40)
        g.reserved = set()
        for i in range(misses):  # (a byte of its own in front of each: the alphabet has 64 only)
            g.fixed([0x80 + i])
            g.fixed(miss, fresh=False)
        g.fixed([0x3F])
        g.reserved = set(res)
    g.copy_at(P, src, 9)
    if found:
        ts = [T(P, kinds[0], "no_hops", ("ld", 9, P - src))]
        if where == "both":
            ts[0]["tok"] = ("ld", 9, P - w)
    else:
        ts = [T(P, kinds[0], None, ("lit", g.o[P]))]
    if P >= 2 * W and found:
        ts.append(T(P, kinds[0], "hops_two_epochs", ts[0]["tok"]))
    return _case(name, "hop", opts, g, n, ts, total, True, w, kinds)


def _hop_quarter(name, misses, found):
    """Best, a match of 34 at P - 1: the walk at P has a quarter of the budget (lz77.rs:351-355), 442 checks.  P is a copy of 60
    bytes of w; its bucket holds U + 1 -- the second byte of the match of P - 1, 33 bytes of w -- and `misses` misses, and
    behind them the identity entry leads to w: the 442nd check with 440 misses, one too late with 441"""
    opts, w, P = BEST, BLOCK + 1, 40000
    hw = w % W
    g, total = resume(opts, w, "lit", seed=48, reserved={hw})
    g.reserved = set()
    z = tri_for(hw, g)
    g.to(w, follow=z)
    g.fixed(z)
    g.reserved = {hw}
    g.lit(80)
    miss = bytes([z[0] ^ 0x20, z[1], z[2]])
    g.reserved = set()
    for i in range(misses):  # (two bytes of its own in front of each)
        g.fixed(bytes([0x80 + i % 128, 0x80 + i // 128]) + miss, fresh=False)
    g.fixed([0x3F])
    g.reserved = {hw}
    g.lit(8)
    U = len(g.o)
    g.fixed([0x3E])
    g.push(bytes(g.o[w:w + 33]))
    g.avoid = {g.o[w + 33]}
    g.to(P - 1, avoid=(g.o[U - 1],))
    g.fixed([0x3E])
    g.push(bytes(g.o[w:w + 60]))
    g.avoid = {g.o[w + 60]}
    kind = "hop_quarter_budget" if found else "hop_quarter_budget_short"
    ts = [T(P, kind, "no_hops", ("ld", 60, P - w))] if found else [T(P, kind, None)]
    return _case(name, "hop", opts, g, 45000, ts, total, True, w, [kind])


def _hop_65535(name):
    """w = 32 768, its three bytes hash to 0; a copy of them at 65 535, the last position before the slide: the identity entry of
    bucket 0 is position 0 there, not 32 768, and out of the window -- a literal.  (The copy's second position, 65 536, looks for
    the bytes at 32 769 through bucket 1 and finds them.)"""
    w = W
    g, total = resume(DEFAULT, w, "lit", seed=47, reserved={0, 1})
    g.reserved = set()
    z = tri_for(0, g, second=1)
    g.to(w, follow=z)
    g.fixed(z)
    g.reserved = {0, 1}
    P = 2 * W - 1
    g.copy_at(P, w, 9)
    ts = [T(P, "before_slide_identity_is_h", None, ("lit", g.o[P])), T(P + 1, "after_slide_w1", "hops_two_epochs", ("ld", 8, W - 1))]
    return _case(name, "hop", DEFAULT, g, 70000, ts, total, True, w, ["before_slide_identity_is_h"])


# ---- handover: Q1 fires, and text lies behind the head up to the lengths around the end of the link path ----------------------------------
def _text_behind(g, n, seed):
    room = n - len(g.o)
    if room > 0:
        g.lit(min(8, room))
        g.o += datagen.text_like(n - len(g.o) + 8, seed)[:n - len(g.o)]


def _handover_n(name, n):
    w = BLOCK + 1
    g, total = resume(DEFAULT, w, "lit", seed=51)
    ts = _probe(g, 33000, w, True)
    g.lit(16)
    _text_behind(g, n, 52)
    c = _case(name, "handover", DEFAULT, g, n, ts, total, True, w, ["n_%d" % n])
    return c


def _plant(d, at, bs):
    d[at:at + len(bs)] = bs


def _handover_targets(name):
    """text of 140 000 bytes behind the head, with planted pieces over 0xA0..0xDF (
    no text byte, no head byte): a match of 258 that starts at 98 303 - 257 (it ends with the last position the link path walks
    for the sorted path: 3 epochs), a target in epoch 3 whose only candidate lies in epoch 2, and a target in epoch 4, which the
    second pass does not walk again"""
    n = LIMIT
    w = BLOCK + 1
    g, total = resume(DEFAULT, w, "lit", seed=53)
    ts = _probe(g, 33000, w, True)
    g.lit(16)
    _text_behind(g, n, 54)
    d = bytearray(g.o)
    r = random.Random(55)

    def piece(m, lo):
        return bytes(r.randrange(lo, lo + 16) for _ in range(m))
    a, e2, e4 = piece(300, 0xA0), piece(20, 0xC0), piece(20, 0xD0)
    pa = IDENT_EPOCHS * W - 1 - 257
    _plant(d, 70000, a)
    _plant(d, pa - 1, b"\x05" + a[:259] + b"\x01")
    ts.append(T(pa, "match_258_ends_at_seam", None, ("ld", 258, pa - 70000)))
    _plant(d, 74000, e2)
    p2 = IDENT_EPOCHS * W + 262
    _plant(d, p2 - 1, b"\x06" + e2 + b"\x03")
    ts.append(T(p2, "epoch3_candidate_in_epoch2", None, ("ld", 20, p2 - 74000)))
    _plant(d, 120000, e4)
    p4 = 4 * W + 1000
    _plant(d, p4 - 1, b"\x07" + e4 + b"\x04")
    ts.append(T(p4, "epoch4_not_recomputed", None, ("ld", 20, p4 - 120000)))
    g.o = d
    return _case(name, "handover", DEFAULT, g, n, ts, total, True, w, ["match_258_ends_at_seam", "epoch3_candidate_in_epoch2", "epoch4_not_recomputed"])


def _handover_first(name, at, m):
    """a target of m bytes at 98 304, the first position of the sorted path after a re-warm, or at 98 303, the last one of the
    link path (a match of 258 across the seam): its only candidate lies in epoch 2"""
    n = 3 * W + 2000
    w = BLOCK + 1
    g, total = resume(DEFAULT, w, "lit", seed=56)
    ts = _probe(g, 33000, w, True)
    g.lit(16)
    _text_behind(g, n, 57)
    d = bytearray(g.o)
    r = random.Random(58)
    e2 = bytes(r.randrange(0xC0, 0xD0) for _ in range(m + 42))
    kind = "target_at_98304" if at == 3 * W else "match_258_starts_at_seam"
    _plant(d, 80000, e2)
    _plant(d, at - 1, b"\x05" + e2[:m] + b"\x03")
    ts.append(T(at, kind, None, ("ld", m, at - 80000)))
    g.o = d
    return _case(name, "handover", DEFAULT, g, n, ts, total, True, w, [kind])


# ---- paths: the same heads in front of text that takes the call down the large path and the streamed host call ----------------------------
def _paths(name, head, n):
    c = case(head)
    data = c["data"] + datagen.text_like(n - len(c["data"]) + 8, 61)[:n - len(c["data"])]
    return dict(name=name, family="paths", data=data, opts=c["opts"], targets=[dict(t) for t in c["targets"]],
                claims=dict(c["claims"], kinds=("large_path" if n < HOST_PIECEWISE_FROM else "streamed_host_call",)))


N_LARGE = (2 << 20) + 1024  # 2 049 segments of 1 KiB: one more than k_small_fix takes


def _table_of_cases():
    t = {}

    def add(name, fn, *a, **kw):
        t[name] = lambda: fn(name, *a, **kw)

    add("predicate_default_lit_tp32766_fires", _predicate, DEFAULT, W, "lit", True)
    add("predicate_default_lit_tp32767_quiet", _predicate, DEFAULT, W + 1, "lit", False)
    add("predicate_default_match_ends_32768_fires", _predicate, DEFAULT, W, "match", True)
    add("predicate_default_match_ends_32769_quiet", _predicate, DEFAULT, W + 1, "match", False)
    add("predicate_best_lit_tp32766_fires", _predicate, BEST, W, "lit", True)
    add("predicate_best_lit_tp32767_quiet", _predicate, BEST, W + 1, "lit", False)
    add("predicate_fast_lit_tp32767_fires", _predicate, FAST, W, "lit", True)
    add("predicate_fast_lit_tp32768_quiet", _predicate, FAST, W + 1, "lit", False)
    add("predicate_two_lit_tp32766_fires", _predicate, TWO, W, "lit", True)
    add("predicate_two_lit_tp32767_quiet", _predicate, TWO, W + 1, "lit", False)
    add("predicate_greedy128_lit_tp32767_fires", _predicate, GREEDY128, W, "lit", True)
    add("predicate_greedy128_lit_tp32768_quiet", _predicate, GREEDY128, W + 1, "lit", False)
    add("predicate_greedy128_match_ends_32768_fires", _predicate, GREEDY128, W, "match", True)
    add("predicate_greedy128_match_ends_32769_quiet", _predicate, GREEDY128, W + 1, "match", False)
    for n in (BLOCK, BLOCK + 1, BLOCK + 2, BLOCK + 3, BLOCK + 4):
        add("predicate_default_clause_n%d" % n, _clause, n)
    add("predicate_default_full_beyond_window", _beyond)
    for w in (W, 32705, 32766, 32767):
        add("filing_default_w%d_mod64_%d" % (w, w % 64), _filing_mod, w)
    for dx, kind in ((-10, "in_batch_below"), (20, "in_batch_above"), (-40, "batch_before"), (-600, "other_group_of_512")):
        add("filing_two_foreign_%s" % kind, _foreign, dx, kind)
    add("filing_fast_foreign_candidate_in_front_of_w", _foreign_fast)
    add("filing_default_own_hash_first", _own_hash, 0)
    add("filing_default_own_hash_second", _own_hash, 1)
    w0 = BLOCK + 1
    add("hop_default_w_epoch0", _hop, DEFAULT, w0, "w", 32400, 36000, ["hop_to_w", "target_epoch0"])
    add("hop_default_w_epoch1", _hop, DEFAULT, w0, "w", 40000, 45000, ["hop_to_w", "target_epoch1"])
    add("hop_default_w1_epoch1", _hop, DEFAULT, w0, "w1", 40000, 45000, ["hop_to_w1", "target_epoch1"])
    add("hop_default_dist32768", _hop, DEFAULT, w0, "w", w0 + W, 70000, ["hop_dist_32768"])
    add("hop_default_dist32769", _hop, DEFAULT, w0, "w", w0 + W + 1, 70000, ["hop_dist_32769"], found=False)
    add("hop_default_behind_1_miss", _hop, DEFAULT, w0, "w", 40000, 45000, ["hop_behind_1_miss"], misses=1)
    add("hop_default_behind_127_misses", _hop, DEFAULT, w0, "w", 40000, 45000, ["hop_behind_checks_minus_1"], misses=127)
    add("hop_default_behind_128_misses", _hop, DEFAULT, w0, "w", 40000, 45000, ["hop_behind_checks"], misses=128, found=False)
    for opts in (DEFAULT, BEST, FAST, GREEDY128):
        add("hop_%s_after_slide_w32768" % LEVEL_NAMES[opts], _hop, opts, W, "both", 2 * W, 70000, ["hop_after_slide", "level_" + LEVEL_NAMES[opts]],
            back=40 if opts != FAST else 6)
    add("hop_default_after_slide_w32767", _hop, DEFAULT, W - 1, "w1", 2 * W, 70000, ["hop_after_slide_w32767"])
    add("hop_default_target_65535", _hop_65535)
    add("hop_best_quarter_budget_behind_441_entries", _hop_quarter, 440, True)
    add("hop_best_quarter_budget_behind_442_entries", _hop_quarter, 441, False)
    for n in (3 * W, 3 * W + 1, 3 * W + 2, 3 * W + LINK_TAIL - 1, 3 * W + LINK_TAIL, 3 * W + LINK_TAIL + 1, 4 * W + 5):
        add("handover_default_n%d" % n, _handover_n, n)
    add("handover_default_targets", _handover_targets)
    add("handover_default_target_at_98304", _handover_first, 3 * W, 20)
    add("handover_default_match_258_from_98303", _handover_first, 3 * W - 1, 258)
    add("paths_default_hop_large", _paths, "hop_default_after_slide_w32768", N_LARGE)
    add("paths_two_filing_large", _paths, "filing_two_foreign_in_batch_below", N_LARGE)
    add("paths_default_hop_streamed", _paths, "hop_default_after_slide_w32768", HOST_PIECEWISE_FROM)
    return t


_CASES = _table_of_cases()
FAMILIES = ("predicate", "filing", "hop", "handover", "paths")

CLAIM_KINDS = (
    # predicate
    "lazy_lit_fires", "lazy_lit_quiet", "lazy_match_fires", "lazy_match_quiet", "greedy_lit_fires", "greedy_lit_quiet", "greedy_match_fires",
    "greedy_match_quiet", "clause_n_tp_plus_1", "clause_n_tp_plus_2", "clause_n_tp_plus_3", "clause_n_tp_plus_4", "clause_n_tp_plus_5",
    "full_beyond_window", "probe_missing", "probe_missing_second", "probe_rest", "probe_found",
    # filing
    "w_mod64_0", "w_mod64_1", "w_mod64_62", "w_mod64_63", "w_mod256_255", "foreign_in_batch_below", "foreign_in_batch_above",
    "foreign_batch_before", "foreign_other_group_of_512", "foreign_fast", "own_hash_first", "own_hash_second",
    # hop
    "hop_to_w", "hop_to_w1", "target_epoch0", "target_epoch1", "hop_dist_32768", "hop_dist_32769", "hop_behind_1_miss",
    "hop_behind_checks_minus_1", "hop_behind_checks", "hop_after_slide", "level_default", "level_best", "level_fast", "level_greedy128",
    "hop_after_slide_w32767", "before_slide_identity_is_h", "after_slide_w1", "hop_quarter_budget", "hop_quarter_budget_short", "hop_lands_on_an_ordinary_position",
    # handover
    "n_98304", "n_98305", "n_98306", "n_102399", "n_102400", "n_102401", "n_131077", "match_258_ends_at_seam", "match_258_starts_at_seam", "epoch3_candidate_in_epoch2",
    "epoch4_not_recomputed", "target_at_98304",
    # paths
    "large_path", "streamed_host_call",
)


def names():
    return list(_CASES)


def family_of(name):
    return name.split("_")[0]


def opts_of(name):
    """the options of a case, without building it"""
    return {v: k for k, v in LEVEL_NAMES.items()}[name.split("_")[1]]


@functools.lru_cache(maxsize=None)
def case(name):
    c = _CASES[name]()
    assert c["name"] == name and c["family"] == family_of(name) and c["opts"] == opts_of(name), name
    return c


def quiet_twin(opts):
    """the case of a level whose first block ends one byte too late for the re-warm"""
    return case(next(n for n in names() if opts_of(n) == opts and n.endswith("_quiet")))


# ---- preconditions, on the oracle alone ----------------------------------------------------------------------------------------------
_REF = {}


def oracle(c, wrapper=0):
    key = (c["name"], wrapper)
    if key not in _REF:
        _REF[key] = ob.encode(c["data"], opts=ob.make_opts(*c["opts"], wrapper))
        if wrapper == 0:
            _REF[c["name"], "blocks"] = ob.trace_blocks()
    return _REF[key]


def oracle_blocks(c):
    oracle(c)
    return _REF[c["name"], "blocks"]


def check(c):
    """assert a case on the oracle: block 0, the predicate on the oracle's own tokens, every target's token, its mutant; returns
    the claim kinds the case has shown"""
    data, opts, cl = c["data"], c["opts"], c["claims"]
    n = len(data)
    ref = oracle(c)
    assert zlib.decompress(ref, -15) == data
    b0 = oracle_blocks(c)[0]
    assert (b0["n_lz"], b0["in_bytes"]) == (BLOCK, cl["in_bytes"]), (c["name"], b0)
    order = tokens_of(ref, blocks=8 if c["family"] == "paths" else 0)
    toks = dict(order)
    assert q1(order, opts, n) == (cl["fires"], cl["w"]), (c["name"], q1(order, opts, n), cl)
    shown = set(cl["kinds"])
    for t in c["targets"]:
        what = "%s, target at %d (%s)" % (c["name"], t["p"], t["kind"])
        (at, tok), visits, hops = predict(c, t, detail=True)
        assert toks.get(at) == tok, "%s: the oracle has %s at %d, the model %s; %s" % (what, toks.get(at), at, tok, chain_text(c, t["p"]))
        if t["tok"] is not None:
            assert (at, tok) == (t["p"], t["tok"]), "%s: the model gives %s at %d, the case declares %s" % (what, tok, at, t["tok"])
        if t["mutant"] is not None:
            assert predict(c, t, t["mutant"]) != (at, tok), "%s: the mutant %s gives %s as well" % (what, t["mutant"], tok)
        shown.add(t["kind"])
        # a hop that the walk took and that landed on neither of the two re-filed positions: it must have changed nothing
        took = [v["q"] for v in visits if v["q"] in hops]
        if took and cl["fires"] and not (set(took) & {cl["w"], cl["w"] + 1}):
            assert predict(c, t, "no_hops") == (at, tok), what
            shown.add("hop_lands_on_an_ordinary_position")
        if t["kind"] in ("hop_to_w", "hop_after_slide", "hop_dist_32768"):
            assert cl["w"] in took, (what, took)
        if t["kind"] in ("hop_to_w1", "hop_after_slide_w32767", "after_slide_w1"):
            assert cl["w"] + 1 in took, (what, took)
    _case_claims_hold(c, toks)
    return shown


def _case_claims_hold(c, toks):
    cl, n, data = c["claims"], len(c["data"]), c["data"]
    w = cl["w"]
    for k in cl["kinds"]:
        if k.startswith("w_mod64_"):
            assert w % 64 == int(k[8:]), (c["name"], w)
        if k == "w_mod256_255":
            assert w % 256 == 255
        if k.startswith("n_"):
            assert n == int(k[2:]) and cl["fires"]
        if k == "hop_dist_32768" or k == "hop_dist_32769":
            assert c["targets"][0]["p"] - w == int(k[9:])
        if k == "target_epoch0" or k == "target_epoch1":
            assert c["targets"][0]["p"] // W == int(k[-1])
        if k in ("hop_after_slide", "hop_after_slide_w32767"):
            assert c["targets"][0]["p"] == 2 * W
        if k.startswith("hop_behind_"):
            t = c["targets"][0]
            _, visits, hops = predict(c, t, detail=True)
            real = visits[:next((i for i, v in enumerate(visits) if v["q"] in hops), len(visits))]
            want = {"hop_behind_1_miss": 1, "hop_behind_checks_minus_1": c["opts"][0] - 1, "hop_behind_checks": c["opts"][0]}[k]
            assert len(real) == want and all(not v["hit"] or v["length"] < 3 for v in real), (c["name"], len(real))
            assert (w in [v["q"] for v in visits]) == (k != "hop_behind_checks")
        if k in ("hop_quarter_budget", "hop_quarter_budget_short"):
            t = c["targets"][0]
            (at, tok), visits, hops = predict(c, t, detail=True)
            q = c["opts"][0] >> 2
            assert len(visits) == q and (visits[-1]["q"] == w) == (k == "hop_quarter_budget"), (c["name"], len(visits), visits[-1])
            if k == "hop_quarter_budget_short":  # the match of P - 1 stays; with the whole budget the hop would have been reached
                assert at == t["p"] - 1 and tok[:2] == ("ld", 34), (at, tok)
                ch = chain(_model(c), t["p"])[0]
                assert mc.walk(data, t["p"], c["opts"][0], 34, chain=ch)[0] == (60, t["p"] - w)
        if k == "full_beyond_window":
            assert cl["in_bytes"] > W and not cl["fires"]
        if k == "large_path":
            assert (n + 1023) // 1024 == 2049
        if k == "streamed_host_call":
            assert n == HOST_PIECEWISE_FROM
        if k == "epoch4_not_recomputed":
            t = next(t for t in c["targets"] if t["kind"] == k)
            assert t["p"] // W == 4 and predict(c, t, "no_rewarm") == predict(c, t)
        if k in ("target_at_98304", "epoch3_candidate_in_epoch2"):
            t = next(t for t in c["targets"] if t["kind"] == k)
            assert t["p"] // W == 3 and (t["p"] - t["tok"][2]) // W == 2 and (k != "target_at_98304" or t["p"] == 3 * W)
        if k in ("match_258_ends_at_seam", "match_258_starts_at_seam"):
            t = next(t for t in c["targets"] if t["kind"] == k)
            assert t["tok"][1] == 258 and t["p"] == (3 * W - 258 if k.endswith("ends_at_seam") else 3 * W - 1)


@functools.lru_cache(maxsize=None)
def shown(name):
    """check() of a case, once: the claim kinds it has shown"""
    return frozenset(check(case(name)))


def covered():
    """assert that every claim kind is shown by at least one case; the kinds by case"""
    by = {nm: shown(nm) for nm in names()}
    got = set().union(*by.values())
    assert set(CLAIM_KINDS) <= got, sorted(set(CLAIM_KINDS) - got)
    return by
