"""Inputs that drive the match walk (stages.h swg_*, kernels k_match3 / k_match3_both / kb_walk) into the situations in which it
can be wrong by one entry: a probe hit in a given slot of a group behind a false hit, the own-epoch part of a bucket ending a
given number of entries behind the last hit, the window's edge inside a group, the budget ending on the decisive candidate, the
near / far halves of a small call's walk, lengths and alignments of the 16-byte compare, ties.

Everything is generated here from fixed seeds; no data file is committed.  A case is a dict(name, family, data, opts, targets):
`opts` = (max_hash_checks, lazy_if_less_than, matching_type), and every target is a position p whose match the oracle emits as
a token, so a wrong table entry at p changes the stream.  A target is a dict:
  p        the position whose chain is walked
  tok      the token the case declares: ('ld', length, distance) or ('lit', byte)
  at       where that token begins (p, or p - 1 where the match of p - 1 is the one that stays)
  prev     (length, distance) of the match at p - 1 the walk starts from ((0, 0) but in the quarter family)
  claims   what the case must provoke there, read off the model's visit list by check(): see CLAIM_KEYS

walk() is a direct statement of the reference's longest_match (matching.rs:87-166) as oracle/deflref.cpp restates it; it runs on
target positions only.  check() holds every case to its claims on the oracle alone, so a case that stops provoking its situation
fails instead of passing empty-handed.  tests/test_match_cases.py (CPU) and tests/test_match_walk_gpu.py use the cases.

How a target is built.  Its position starts with a trigram abc of its own (a in 0xC0..0xDF, b and c in 0x80..0x9F: 32 768 trigrams
with 32 768 different hashes) followed by a body over 0xA0..0xBF in which no pair of neighbours occurs twice, so the two-byte
probe of matching.rs:141 hits only where a copy of the target lies aligned with it.  The candidates are earlier occurrences:
  miss        a ^ 0x20, b, c: the same hash (a & 31 is kept), another first byte
  real hit    l >= 3 bytes of the target, then a byte of the filler alphabet
  false hit   the target's bytes at l - 1 and l (what the probe reads behind a hit of length l), another byte at 3
Candidates are 5 or more filler bytes apart (capitals and digits).  In front of p stands a byte from 1..17 that forms a pair with a
nowhere else, so nothing begins at p - 1; behind the match the candidate has filler where the target has body.  A longer match
that the walk must NOT reach is longer by one byte only: at p + 1 it offers nothing better than what p found.  Padding is
datagen.text_like (lower case and punctuation: disjoint from all of the above), checked to fill none of the targets' buckets.
"""
import functools
import random

import numpy as np

import datagen
import oracle_binding as ob
from header_cases import decode

WINDOW = 32768
EPOCH = 32768
MAX_MATCH = 258
DEFAULT, GREEDY, BEST = (128, 32, 1), (128, 32, 0), (1768, 128, 1)

FILL = bytes(range(0x30, 0x3A)) + bytes(range(0x41, 0x5B))
GUARD = bytes(list(range(1, 10)) + list(range(11, 18)))
BODY = bytes(range(0xA0, 0xC0))
SEP = 5

CLAIM_KEYS = """
  first        rank of the first real hit
  gap          chain entries between the first and the second real hit
  false, real  entries between the first real hit and each false hit / the next real hit
  false_last   the bucket's very last entry is a false hit
  own_end      own-epoch entries behind the last probe hit in the own epoch
  n1           own-epoch entries of the bucket
  prev_rank    entries of the previous epoch's part in front of the decisive one
  variant      epoch0 / empty_prev / prev_decisive / n1_zero
  dist         distance of the decisive candidate
  beyond       distance of a longer candidate just outside the window
  win_last     in-window entries behind the last hit, a longer probe hit right behind the window's edge; slot = win_last % 8
  decisive     rank of the decisive candidate
  longer_at    rank of a longer candidate that the budget (or the quarter budget) must not reach
  budget       True: one check less gives another token
  half, side   half = checks / 2; side = decisive rank - half (-1, 0, 1), 'tie' or 'far_longer'
  length       the match length; p16, q16 = position and candidate mod 16; left = bytes from p to the end of the input
  equal        number of candidates of the decisive length; where = group / seam / batch64
  run_pieces   at least that many of the 64 aligned 512-byte pieces of the target's epoch are a run of one byte
  run_break    the target is the second byte of a run of that many bytes; run_edge: of a run of 258 + that many over an epoch's edge,
               epoch_pos = the target's position relative to the edge
  J            positions of the last epoch that have a hash byte; last64: the target is among the last 64 entries of its sorted
               epoch; whole: the input's length
"""


def hash3(a, b, c):
    return (((a & 31) << 10) ^ (b << 5) ^ c) & 0x7FFF


@functools.lru_cache(maxsize=4)
def _hashes(data):
    d = np.frombuffer(data, dtype=np.uint8).astype(np.uint32)
    if len(d) < 3:
        return np.zeros(0, dtype=np.uint32)
    return (((d[:-2] & 31) << 10) ^ (d[1:-1] << 5) ^ d[2:]) & 0x7FFF


def common(data, p, q, maxl=MAX_MATCH):
    """get_match_length (matching.rs:67-72), no further than maxl"""
    ln = 0
    while ln < maxl and p + ln < len(data) and data[p + ln] == data[q + ln]:
        ln += 1
    return ln


# ---- the model -----------------------------------------------------------------------------------------------------------------------
def walk(data, p, checks, prev_length=0, window=WINDOW, maxlen=MAX_MATCH, mutant=None, first=0, filing=None, holes=(), end=None, chain=None):
    """longest_match (matching.rs:87-166) at position p: ((length, distance), visits).  The chain is the earlier positions with
    p's 3-byte hash, nearest first; a visit is dict(rank, q, dist, hit, length): `hit` = the two-byte probe at best - 1, best
    passed, `length` = what was then compared (None without a hit), `best` = the best length the probe stood on.
    first: skip that many chain entries (the far half of a split walk).  mutant: one thing wrong, for the sensitivity tests.
    filing, holes, end (tests/flush_cases.py): the hash every position was filed under where that is not the hash of its own
    three bytes, positions that were never filed, and the end of the data the encoder had when it looked at p.
    chain (tests/rewarm_cases.py): the positions the walk visits, nearest first, where they are not p's bucket alone -- the bucket
    and what lies behind the head table's identity entry; window and budget apply to them as to any chain."""
    n = len(data) if end is None else end
    if prev_length >= MAX_MATCH or p + prev_length >= n or p + 2 >= n:
        return (0, 0), []
    if chain is None:
        h = _hashes(data) if filing is None else filing
        chain = np.nonzero(h[:p] == h[p])[0][::-1]
    if len(holes):
        chain = np.array([q for q in chain if int(q) not in holes], dtype=np.int64)
    floor = best = max(prev_length, 1)
    bestd, maxl, visits = 0, min(n - p, maxlen), []
    i, used = first, 0
    while i < len(chain) and used < checks:
        q = int(chain[i])
        if p - q > window:
            break
        hit = data[p + best - 1] == data[q + best - 1] and data[p + best] == data[q + best]
        if mutant == "farthest_among_equals" and best >= 3:  # (a walk that looks at every candidate and takes ">=")
            hit = hit or common(data, p, q, maxl) >= best
        v = dict(rank=i, q=q, dist=p - q, hit=hit, length=None, best=best)
        visits.append(v)
        i, used = i + 1, used + 1
        if not hit:
            continue
        v["length"] = ln = common(data, p, q, maxl)
        if ln > best or (mutant == "farthest_among_equals" and ln == best and bestd):
            best, bestd = ln, p - q
            if ln == maxl:
                break
        elif mutant == "false_hit_ends":
            break
        if mutant == "resume_late":  # the entry right behind a hit is never looked at
            i, used = i + 1, used + 1
        if mutant == "resume_early":  # the hit is looked at once more: one check of the budget gone
            used += 1
    return ((best, bestd) if best > floor else (0, 0)), visits


def quarter(opts, prev_length):
    """the budget of a position whose predecessor holds a match (lz77.rs:351-355)"""
    return opts[0] >> 2 if prev_length >= 32 else opts[0]


def predict(data, t, opts, d_checks=0, d_quarter=0, far_wins_ties=False, **kw):
    """(position, token) the model gives for a target: the walk at p from the match of p - 1, match_too_far, and the lazy
    rule of lz77.rs:388 between the two.  d_checks / d_quarter / far_wins_ties / kw (window, maxlen, mutant): the mutants."""
    p = t["p"]
    pl, pd = t.get("prev", (0, 0))
    c = (opts[0] >> 2) + d_quarter if pl >= 32 else opts[0] + d_checks
    (ln, d), _ = walk(data, p, max(c, 0), pl, **kw)
    if far_wins_ties and c >= 16:
        (l1, d1), _ = walk(data, p, c // 2, pl, **kw)
        (l2, d2), _ = walk(data, p, c - c // 2, pl, first=c // 2, **kw)
        ln, d = (l2, d2) if l2 >= l1 and l2 else (l1, d1)
    if ln == 3 and d > 8192:
        ln = d = 0
    if pl >= 3 and pl >= ln:
        return p - 1, ("ld", pl, pd)
    return (p, ("ld", ln, d)) if ln >= 3 else (p, ("lit", data[p]))


def tokens_at(data, opts):
    """{position: token} of the oracle's parse"""
    out, pos = {}, 0
    for tok in ob.lz77(data, *opts):
        out[pos] = tok
        pos += 1 if tok[0] == "lit" else tok[1]
    assert pos == len(data)
    return out


# ---- building blocks -----------------------------------------------------------------------------------------------------------------
class _Build:
    """Bytes with targets whose buckets hold exactly the candidates put there: a new trigram's hash is in no bucket used so far,
    and every byte that is free to choose (filler, body) is chosen so that its trigrams fall into no target's bucket."""

    def __init__(self, seed, lead=b""):
        self.r = random.Random(seed)
        self.o = bytearray(lead)
        self.used = set(np.unique(_hashes(bytes(lead))).tolist())
        self.res = set()
        self.pairs = set()
        self.targets = []
        self.texts = {}

    def ok(self, *tris):
        return all(hash3(*t) not in self.res for t in tris)

    def push(self, bs):
        o = self.o
        for b in bs:
            o.append(b)
            if len(o) >= 3:
                self.used.add(hash3(o[-3], o[-2], o[-1]))

    def pick(self, alphabet, follow=()):
        """one byte of the alphabet whose trigrams -- with the two bytes before it and up to two known bytes behind it -- fall
        into no target's bucket"""
        o, al = self.o, list(alphabet)
        self.r.shuffle(al)
        for x in al:
            seq = list(o[-2:]) + [x] + list(follow[:2])
            if self.ok(*[tuple(seq[i:i + 3]) for i in range(len(seq) - 2)]):
                self.push([x])
                return x
        raise RuntimeError("no free byte here")

    def fill(self, n, follow=()):
        for i in range(n):
            self.pick(FILL, follow if i == n - 1 else ())

    def text(self, seed, n=EPOCH + 1024):
        """text for pad(): made before the targets it must keep clear of, so that their trigrams avoid its buckets"""
        t = datagen.text_like(n, seed)[:n]
        self.texts[seed] = t
        self.used |= set(np.unique(_hashes(t)).tolist())

    def pad(self, n, seed):
        """n bytes: a separator and the beginning of the text of that seed"""
        assert n >= SEP + 3, "no room for the padding (%d)" % n
        t = self.texts[seed][:n - SEP]
        assert len(t) == n - SEP and not (set(np.unique(_hashes(t)).tolist()) & self.res)
        self.fill(SEP, t)
        j = len(self.o)
        self.o += t
        self.used |= {hash3(*self.o[i - 2:i + 1]) for i in (j, j + 1)}

    def pad_to(self, offset, seed):
        self.pad(offset - len(self.o), seed)

    def new_target(self, tlen, run=False, pre=False, a5=None):
        """a trigram with an empty bucket, a guard byte, and tlen bytes of target text; run: the text is one byte repeated;
        pre: one more byte s in front of the text whose trigram s, a, b has an empty bucket too (a match can begin at p - 1);
        a5: the low five bits of a (27: the hash's top five bits are all set, the bucket is among the last of the sorted epoch)"""
        for _ in range(10000):
            a, b, c = 0xC0 + (self.r.randrange(32) if a5 is None else a5), 0x80 + self.r.randrange(32), 0x80 + self.r.randrange(32)
            if run:
                b = c = a
            g = self.r.choice(GUARD)
            h = hash3(a, b, c)
            s0 = 0xC0 + self.r.randrange(32)
            front = [s0, a, b] if pre else [a, b]
            if pre and (hash3(s0, a, b) in self.used or hash3(s0, a, b) in self.res or hash3(s0, a, b) == h):
                continue
            if h in self.used or h in self.res or (g, front[0]) in self.pairs or not self.ok((g, front[0], front[1])):
                continue
            text = [a, b, c]
            pairs = {(a, b), (b, c)}
            self.res.add(h)
            while len(text) < tlen:
                al = list(BODY)
                self.r.shuffle(al)
                x = a if run else next((x for x in al if (text[-1], x) not in pairs and self.ok((text[-2], text[-1], x))), None)
                if x is None:
                    break
                pairs.add((text[-1], x))
                text.append(x)
            if len(text) < tlen:
                self.res.discard(h)
                continue
            self.pairs.add((g, front[0]))
            self.used |= {hash3(g, front[0], front[1])} | {hash3(*text[i:i + 3]) for i in range(len(text) - 2)}
            if pre:
                self.res.add(hash3(s0, a, b))
            return dict(tri=(a, b, c), g=g, text=bytes(text), run=run, pre=bytes([s0]) if pre else b"")
        raise RuntimeError("no free trigram")

    # an item of a chain: ('m',) miss, ('r', l) real hit of length l, ('f', l) false hit behind a hit of length l, ('raw', bytes),
    # ('u', l): the byte in front of the target and l - 1 bytes of it -- a match of length l for p - 1, whose second byte is one
    # more entry of p's chain (a miss for a walk that starts from that match)
    def item_bytes(self, tg, item):
        a, b, c = tg["tri"]
        T = tg["text"]
        if item[0] == "m":
            return bytes([a ^ 0x20, b, c])
        if item[0] == "r":
            return T[:item[1]]
        if item[0] == "f":
            ln = item[1]
            assert ln >= 5
            return bytes([a, b, c, 0]) + T[4:ln + 1]  # (the 0 is replaced by a free filler byte when the item is placed)
        if item[0] == "u":
            return tg["pre"] + T[:item[1] - 1]
        return item[1]

    def item_len(self, tg, item):
        return len(self.item_bytes(tg, item))

    def put(self, tg, item):
        """a separator and the item; returns the item's position"""
        bs = self.item_bytes(tg, item)
        self.fill(SEP, bs)
        q = len(self.o)
        if item[0] == "f":
            self.push(bs[:3])
            self.pick(FILL, bs[4:])
            self.push(bs[4:])
        else:
            self.push(bs)
        if item[0] in ("r", "raw", "u"):  # the byte that ends the match: filler (never the target's next byte)
            self.pick(FILL)
        return q

    def put_chain(self, tg, chain):
        """the items of a chain given in walk order (nearest first): placed farthest first; their positions in walk order"""
        return [self.put(tg, it) for it in reversed(chain)][::-1]

    def chain_len(self, tg, chain):
        return sum(SEP + self.item_len(tg, it) + (1 if it[0] in ("r", "raw", "u") else 0) for it in chain)

    def put_target(self, tg, tlen, at=None, end=False):
        """the guard byte and tlen bytes of the target's text; at: more filler first so that the target lies there"""
        extra = 0 if at is None else at - (len(self.o) + SEP + 1 + len(tg["pre"]))
        assert extra >= 0, "the target cannot lie at %s: %d bytes too late" % (at, -extra)
        self.fill(SEP - 1 + extra)
        self.pick(FILL, [tg["g"], (tg["pre"] + tg["text"])[0]])
        self.push([tg["g"]])
        self.push(tg["pre"])
        p = len(self.o)
        self.push(tg["text"][:tlen])
        if not end:
            self.pick(FILL)
        return p

    def target(self, p, tok, claims, at=None, prev=(0, 0)):
        self.targets.append(dict(p=p, at=p if at is None else at, tok=tok, prev=prev, claims=claims))

    def simple(self, chain, decisive, claims, a5=None):
        """one target in one place: its chain, then the target; the token is the real hit chain[decisive]"""
        ln = chain[decisive][1]
        tlen = max(it[1] for it in chain if it[0] in ("r", "f")) + 3
        tg = self.new_target(tlen + 1, a5=a5)
        pos = self.put_chain(tg, chain)
        p = self.put_target(tg, tlen)
        self.target(p, ("ld", ln, p - pos[decisive]), claims)
        return p, pos

    def case(self, name, family, opts):
        return dict(name=name, family=family, data=bytes(self.o), opts=opts, targets=self.targets)


M = ("m",)


def R(ln):
    return ("r", ln)


def F(ln):
    return ("f", ln)


# ---- the families --------------------------------------------------------------------------------------------------------------------
def _gap(name, opts, seed):
    g = _Build(seed)
    for gap in range(34):
        first = gap % 18
        g.simple([M] * first + [R(6)] + [M] * gap + [R(9)] + [M] * 2, first + 1 + gap, dict(first=first, gap=gap))
    return g.case(name, "gap", opts)


def _false_then_real(part):
    g = _Build(200 + part)
    pairs = [(i, j) for j in range(1, 16) for i in range(j)]
    for i, j in pairs[part::2]:
        g.simple([R(6)] + [M] * i + [F(6)] + [M] * (j - i - 1) + [R(9), M], j + 1, dict(false=[i], real=j))
    if part == 0:
        g.simple([R(6), M, F(6), F(6), M, R(9), M], 5, dict(false=[1, 2], real=4))
        g.simple([R(6), F(6), M, F(6), F(6), M, M, R(9)], 7, dict(false=[0, 2, 3], real=6))
        g.simple([R(6), M, M, F(6)], 0, dict(false=[2], false_last=True))
    return g.case("false_then_real_%d" % part, "false_then_real", DEFAULT)


def _own_end_epoch0():
    g = _Build(300)
    for k in range(17):
        g.simple([R(6), M, R(9)] + [M] * k, 2, dict(own_end=k, variant="epoch0"))
    return g.case("own_end_epoch0", "own_end", DEFAULT)


def _seam(g, specs, seed):
    """targets whose buckets lie on both sides of the seam between epoch 0 and epoch 1.  A spec is (prev, own, decisive, claims):
    the chains in the previous and in the own epoch in walk order, and the index in own + prev of the real hit that decides.
    Text, the previous-epoch parts right in front of the seam (inside the window of their targets), the seam, own parts and targets."""
    g.text(seed)
    g.text(seed + 1, 64)
    tgs = [g.new_target(13) for _ in specs]
    g.pad(EPOCH - 16 - sum(g.chain_len(tg, s[0]) for tg, s in zip(tgs, specs)) - len(g.o), seed)
    ppos = [g.put_chain(tg, s[0]) for tg, s in zip(tgs, specs)]
    g.pad_to(EPOCH, seed + 1)
    for tg, (prev, own, decisive, claims), pp in zip(tgs, specs, ppos):
        pos = g.put_chain(tg, own) + pp
        p = g.put_target(tg, 12)
        g.target(p, ("ld", (own + prev)[decisive][1], p - pos[decisive]), claims)


def _own_end_seam():
    """epoch 0: the previous-epoch parts of all targets, then text up to the seam; epoch 1: own parts and targets"""
    g = _Build(310)
    # the decisive entry has j entries of the previous epoch's part in front of it, and the own part ends j behind its hit
    specs = [([M] * j + [R(9), M, M], [R(6)] + [M] * j, 2 * j + 1, dict(own_end=j, n1=j + 1, prev_rank=j, variant="prev_decisive"))
             for j in range(17)]
    specs.append(([M, R(6), M, R(9), M], [], 3, dict(n1=0, variant="n1_zero")))
    _seam(g, specs, 311)
    for k in range(17):
        g.simple([R(6), M, R(9)] + [M] * k, 2, dict(own_end=k, n1=3 + k, variant="empty_prev"))
    return g.case("own_end_seam", "own_end", DEFAULT)


def _window():
    """far parts at the start of epoch 0, text, near parts and targets in epoch 1, every target at an exact distance from one entry
    of its far part"""
    g = _Build(400)
    g.text(401)
    plan = []

    def far(tg, chain, anchor, dist, near, tlen, ln, decisive, claims):
        """the far part of a target now, its near part later: chain[anchor] will lie `dist` bytes in front of the target; the
        token is `ln` bytes from entry `decisive` of near + chain (None: from 32 768 back)"""
        # (the far parts lie further apart than the near parts with their targets will)
        g.fill(g.chain_len(tg, near) + (plan[-1][4] + 32 if plan else 96))
        pos = g.put_chain(tg, chain)
        plan.append((tg, near, pos, pos[anchor] + dist, tlen, ln, decisive, claims))

    for dist in (32768, 32767):
        far(g.new_target(13), [R(9), M], 0, dist, [M, R(6), M], 12, 9, 3, dict(dist=dist))
    # a run of 40 bytes whose second byte is 32 768 back: 39 from there, 40 from one byte further, which is outside
    tg = g.new_target(61, run=True)
    far(tg, [("raw", tg["text"][:40])], 0, 32769, [], 60, 39, None, dict(dist=32768, beyond=32769, length=39))
    # the last entry inside the window lies k entries behind the hit; right behind it, outside, a longer match
    far(g.new_target(14), [R(6), R(10)], 0, 32768, [], 13, 6, 0, dict(win_last=0))
    for k in range(1, 17):
        far(g.new_target(14), [M, R(10)], 0, 32768, [R(6)] + [M] * (k - 1), 13, 6, 0, dict(win_last=k))
    g.pad_to(EPOCH + 8, 401)
    for tg, near, pos, at, tlen, ln, decisive, claims in plan:
        pos = g.put_chain(tg, near) + pos
        p = g.put_target(tg, tlen, at=at)
        g.target(p, ("ld", ln, WINDOW if decisive is None else p - pos[decisive]), claims)
    return g.case("window", "window", DEFAULT)


def _window_p(p_abs):
    """the target at 32 768 / 32 769 exactly, a run of 40 bytes at the very start of the input: the limit of matching.rs:102
    (40, not fewer: a match of 32 or more is taken without a look at p + 1, where the run would match itself one byte back)"""
    g = _Build(410 + p_abs % 7)
    g.text(411)
    tg = g.new_target(61, run=True)
    g.push(tg["text"][:40])
    g.pick(FILL)
    g.pad_to(p_abs - 80, 411)
    p = g.put_target(tg, 60, at=p_abs)
    assert p == p_abs
    ln = 40 if p_abs == WINDOW else 39
    g.target(p, ("ld", ln, 32768), dict(dist=32768, length=ln, p_abs=p_abs, **({"beyond": 32769} if ln == 39 else {})))
    return g.case("window_p%d" % p_abs, "window", DEFAULT)


BUDGETS = (1, 2, 5, 8, 9, 15, 16, 17, 24, 128, 1768)


def _budget(checks):
    g = _Build(500 + checks)
    lead = [R(6)] if checks >= 3 else []  # (a hit in front of the decisive one: the walk has resumed once when the budget ends)
    g.simple(lead + [M] * (checks - 1 - len(lead)) + [R(8), R(9), M], checks - 1, dict(decisive=checks - 1, longer_at=checks, budget=True))
    if checks in (16, 17, 128, 1768):
        half = checks // 2
        for side in (-1, 0, 1):
            g.simple([M] * (half + side) + [R(8), M], half + side, dict(half=half, side=side, decisive=half + side))
        g.simple([M] * (half - 2) + [R(8), M, M, M, R(8), M], half - 2, dict(half=half, side="tie", equal=2))
        g.simple([M] * (half - 2) + [R(8), M, M, M, R(9), M], half + 2, dict(half=half, side="far_longer"))
    return g.case("budget_%d" % checks, "budget", (checks, 32, 1))


def _budget_seam():
    """checks = 16 and n1 = 16 - k own-epoch entries: the budget ends k entries into the previous epoch's part"""
    g = _Build(560)
    _seam(g, [([M] * (k - 1) + [R(8), R(9), M], [R(6)] + [M] * (15 - k), 15, dict(decisive=15, longer_at=16, budget=True, n1=16 - k))
              for k in (1, 3, 8)], 561)
    return g.case("budget_seam", "budget", (16, 32, 1))


def _quarter_chain(q, lp, side, variant):
    """walk order: the match of p - 1 first (rank 0 of p's chain, a miss there), misses, the longer match at rank q + side"""
    n = max(q + side, 0) + 1 + (0 if variant == "no_hit_behind" else 3)
    chain = [M] * n
    chain[0] = ("u", lp)
    if variant == "hits":  # probe hits that are no better, in front of the boundary and behind it
        chain[q - 3] = chain[q + 2] = F(lp)
    chain[q + side] = R(lp + 5)
    return chain


def _quarter_target(g, tg, pos, chain, p, q, lp, side, variant, budget=False):
    u, r = chain.index(("u", lp)), chain.index(R(lp + 5))
    prev = (lp, p - 1 - pos[u])
    claims = dict(q=q, q_side=side, prev_length=lp, q_variant=variant, **({"budget": True} if budget else {}))
    if side < 0:
        g.target(p, ("ld", lp + 5, p - pos[r]), claims, prev=prev)
    else:
        g.target(p, ("ld",) + prev, claims, at=p - 1, prev=prev)


def _quarter_best():
    g = _Build(600)
    q = BEST[0] >> 2
    for lp, side, variant in ((100, -2, "plain"), (40, -1, "plain"), (32, 0, "plain"), (127, 1, "plain"), (64, -1, "hits"), (50, 0, "hits"),
                              (33, -1, "no_hit_behind")):
        tg = g.new_target(lp + 9, pre=True)
        chain = _quarter_chain(q, lp, side, variant)
        pos = g.put_chain(tg, chain)
        p = g.put_target(tg, lp + 8)
        _quarter_target(g, tg, pos, chain, p, q, lp, side, variant, budget=(side == -1 and variant == "plain"))
    return g.case("quarter_best", "quarter", BEST)


def _quarter_seam():
    """the quarter budget ends in the previous epoch's part: 100 own-epoch entries, the rest in front of the seam"""
    g = _Build(610)
    g.text(611)
    g.text(612, 64)
    q = BEST[0] >> 2
    plan = []
    for lp, side in ((45, -1), (46, 0)):
        tg = g.new_target(lp + 9, pre=True)
        chain = _quarter_chain(q, lp, side, "plain")
        plan.append((tg, chain, lp, side))
    g.pad(EPOCH - 16 - sum(g.chain_len(tg, ch[100:]) for tg, ch, _, _ in plan) - len(g.o), 611)
    ppos = [g.put_chain(tg, ch[100:]) for tg, ch, _, _ in plan]
    g.pad_to(EPOCH, 612)
    for (tg, chain, lp, side), pp in zip(plan, ppos):
        pos = g.put_chain(tg, chain[:100]) + pp
        p = g.put_target(tg, lp + 8)
        _quarter_target(g, tg, pos, chain, p, q, lp, side, "prev_epoch")
    return g.case("quarter_seam", "quarter", BEST)


def _quarter_custom(checks):
    """(6, 64): a quarter budget of one check; (3, 64): of none -- the walk from a match of 32 or more finds nothing at all.
    The match of p - 1 is the chain's far end here, so that rank 0 is free for the longer one."""
    g = _Build(620 + checks)
    q = checks >> 2
    for lp, side in ((32, -1), (40, 0)) if q else ((32, 0), (50, 1)):
        tg = g.new_target(lp + 9, pre=True)
        chain = [M] * (q + side) + [R(lp + 5), M, ("u", lp)]
        pos = g.put_chain(tg, chain)
        p = g.put_target(tg, lp + 8)
        _quarter_target(g, tg, pos, chain, p, q, lp, side, "plain")
    return g.case("quarter_%d" % checks, "quarter", (checks, 64, 1))


LENGTHS = (3, 4, 15, 16, 17, 18, 31, 32, 33, 34, 47, 48, 49, 50, 255, 256, 257, 258)


def _lengths():
    g = _Build(700)
    for ln in LENGTHS:
        if ln == 258:  # the data goes on equal beyond 258
            tg = g.new_target(301)
            q = g.put(tg, ("raw", tg["text"][:300]))
            p = g.put_target(tg, 300)
            g.target(p, ("ld", 258, p - q), dict(length=258, beyond_max=True))
        else:
            g.simple([R(ln)], 0, dict(length=ln))
    return g.case("lengths", "length", DEFAULT)


def _align(part):
    """p mod 16 x candidate mod 16 at length 20: the 16-byte loads of the compare at every pair of alignments"""
    g = _Build(710 + part)
    for q16 in range(8 * part, 8 * part + 8):
        for p16 in range(16):
            tg = g.new_target(24)
            g.fill((q16 - (len(g.o) + SEP)) % 16)
            q = g.put(tg, R(20))
            at = len(g.o) + SEP + 1
            p = g.put_target(tg, 23, at=at + (p16 - at) % 16)
            assert (p % 16, q % 16) == (p16, q16)
            g.target(p, ("ld", 20, p - q), dict(length=20, p16=p16, q16=q16))
    return g.case("align_%d" % part, "length", DEFAULT)


LEFT = tuple(range(3, 21)) + (257, 258, 259)


def _cut(left):
    """the match cut by the end of the input: left = n - p bytes, the candidate goes on equal"""
    g = _Build(720 + left)
    tg = g.new_target(left + 9)
    q = g.put(tg, ("raw", tg["text"][:left + 8]))
    p = g.put_target(tg, left, end=True)
    ln = min(left, MAX_MATCH)
    g.target(p, ("ld", ln, p - q), dict(left=left, length=ln))
    if left == 259:
        g.target(p + 258, ("lit", g.o[p + 258]), dict(left=1))
    return g.case("cut_%d" % left, "length", DEFAULT)


def _last_two():
    """the last two positions of the input begin no trigram: literals, whatever lies before them"""
    g = _Build(760)
    tg = g.new_target(10)
    g.put(tg, R(8))
    p = g.put_target(tg, 2, end=True)
    g.target(p, ("lit", g.o[p]), dict(left=2))
    g.target(p + 1, ("lit", g.o[p + 1]), dict(left=1))
    return g.case("last_two", "length", DEFAULT)


def _ties():
    g = _Build(800)
    g.simple([M, R(8), M, R(8), M], 1, dict(equal=2, where="group"))
    g.simple([R(8), R(8), M, R(8)], 0, dict(equal=3, where="group"))
    g.simple([M] * 6 + [R(8), R(8)] + [M], 6, dict(equal=2, where="group"))
    # a bucket of more than 64 entries: the equal pair is entries 63 and 64 of the bucket, counted from its far end
    g.simple([M, M, R(8), R(8)] + [M] * 63, 2, dict(equal=2, where="batch64"))
    g.simple([M, R(8)] + [M] * 62 + [R(8), M, M], 1, dict(equal=2, where="batch64"))
    return g.case("ties", "ties", DEFAULT)


def _ties_seam():
    g = _Build(810)
    _seam(g, [([R(8), M], [M, R(8)], 1, dict(equal=2, where="seam")), ([M, R(8), R(8)], [R(8), M], 0, dict(equal=3, where="seam")),
              ([R(8), R(8)], [M, M], 2, dict(equal=2, where="seam"))], 811)
    return g.case("ties_seam", "ties", DEFAULT)


def _one_back(g, run, claims):
    """a run of `run` equal bytes: its second position finds the first one byte back, run - 1 long"""
    tg = g.new_target(run + 1, run=True)
    s = g.put_target(tg, run)
    g.target(s + 1, ("ld", min(run - 1, MAX_MATCH), 1), dict(dist=1, length=min(run - 1, MAX_MATCH), **claims))
    return s


def _run_mix():
    """40 of the epoch's 64 aligned pieces of 512 positions are zeros (k_sort marks such an epoch: the walk's service for runs of
    one byte); behind them targets of the families gap, false_then_real and own_end, and runs that break before 258"""
    g = _Build(900, lead=bytes(512 * 40))
    mark = dict(run_pieces=40)
    for gap in range(0, 34, 3):
        first = (5 * gap) % 18
        g.simple([M] * first + [R(6)] + [M] * gap + [R(9)] + [M] * 2, first + 1 + gap, dict(first=first, gap=gap, **mark))
    for i, j in ((0, 1), (0, 7), (3, 8), (6, 7), (2, 15), (14, 15)):
        g.simple([R(6)] + [M] * i + [F(6)] + [M] * (j - i - 1) + [R(9), M], j + 1, dict(false=[i], real=j, **mark))
    for k in (0, 1, 7, 8, 9, 16):
        g.simple([R(6), M, R(9)] + [M] * k, 2, dict(own_end=k, variant="epoch0", **mark))
    for run in (4, 5, 18, 33, 101, 257, 258):
        _one_back(g, run, dict(run_break=run, **mark))
    assert len(g.o) <= EPOCH
    return g.case("run_mix", "run_mix", DEFAULT)


def _run_edge(name, start, run, seed):
    """a run of 258 + k bytes over the seam between two epochs: a match of 258 one byte back, then what is left of the run"""
    g = _Build(seed)
    g.text(seed + 1)
    tg = g.new_target(run + 1, run=True)
    g.pad_to(start - SEP - 1, seed + 1)
    s = g.put_target(tg, run)
    assert s == start and s < EPOCH < s + run
    p, left = s + 1, run - 1
    while left >= 3:
        ln = min(left, MAX_MATCH)
        g.target(p, ("ld", ln, 1), dict(dist=1, length=ln, run_edge=run - MAX_MATCH, epoch_pos=p - EPOCH))
        p, left = p + ln, left - ln
    return g.case(name, "run_mix", DEFAULT)


TAIL_J = (63, 64, 65, 511, 512, 513)


def _tail(j):
    """an input of j + 2 bytes: j positions of the last (only) epoch have a hash byte; the target's bucket is among the last 64
    entries of the sorted epoch"""
    g = _Build(1000 + j)
    g.simple([M, R(6), M, R(9)], 3, dict(J=j, last64=True), a5=27)
    g.fill(j + 2 - len(g.o))
    return g.case("tail_%d" % j, "tail", DEFAULT)


def _whole(n):
    """inputs of 3 to 6 bytes in whole (3 and 4 bytes: one and two positions with a hash byte)"""
    data = {3: b"\xc1\xc1\xc1", 4: b"\xc1\xc1\xc1\xc1", 5: b"\xc1\xc1\xc1\xc1\xc1", 6: b"\xc1\x81\x82\xc1\x81\x82"}[n]
    tok = {3: ("lit", 0xC1), 4: ("ld", 3, 1), 5: ("ld", 4, 1), 6: ("ld", 3, 3)}[n]
    p = {3: 0, 4: 1, 5: 1, 6: 3}[n]
    t = [dict(p=p, at=p, tok=tok, prev=(0, 0), claims=dict(whole=n, J=n - 2))]
    if n == 3:
        t += [dict(p=q, at=q, tok=tok, prev=(0, 0), claims=dict(whole=n, left=3 - q)) for q in (1, 2)]
    return dict(name="whole_%d" % n, family="tail", data=data, opts=DEFAULT, targets=t)


def _table_of_cases():
    t = {}
    t["gap_default"] = lambda: _gap("gap_default", DEFAULT, 100)
    t["gap_greedy"] = lambda: _gap("gap_greedy", GREEDY, 101)
    for part in (0, 1):
        t["false_then_real_%d" % part] = lambda part=part: _false_then_real(part)
    t["own_end_epoch0"] = _own_end_epoch0
    t["own_end_seam"] = _own_end_seam
    t["window"] = _window
    for p_abs in (32768, 32769):
        t["window_p%d" % p_abs] = lambda p_abs=p_abs: _window_p(p_abs)
    for c in BUDGETS:
        t["budget_%d" % c] = lambda c=c: _budget(c)
    t["budget_seam"] = _budget_seam
    t["quarter_best"] = _quarter_best
    t["quarter_seam"] = _quarter_seam
    for c in (6, 3):
        t["quarter_%d" % c] = lambda c=c: _quarter_custom(c)
    t["lengths"] = _lengths
    for part in (0, 1):
        t["align_%d" % part] = lambda part=part: _align(part)
    for left in LEFT:
        t["cut_%d" % left] = lambda left=left: _cut(left)
    t["last_two"] = _last_two
    t["ties"] = _ties
    t["run_mix"] = _run_mix
    t["run_edge_a"] = lambda: _run_edge("run_edge_a", EPOCH - 130, MAX_MATCH + 300, 910)
    t["run_edge_b"] = lambda: _run_edge("run_edge_b", EPOCH - 259, MAX_MATCH + 5, 920)
    for j in TAIL_J:
        t["tail_%d" % j] = lambda j=j: _tail(j)
    for n in (3, 4, 5, 6):
        t["whole_%d" % n] = lambda n=n: _whole(n)
    t["ties_seam"] = _ties_seam
    return t


_CASES = _table_of_cases()
FAMILIES = ("gap", "false_then_real", "own_end", "window", "budget", "quarter", "length", "ties", "run_mix", "tail")


def names():
    return list(_CASES)


def opts_of(name):
    """the options of a case, without building it"""
    kind, _, last = name.rpartition("_")
    if kind in ("budget", "quarter") and last.isdigit():
        return (int(last), 32 if kind == "budget" else 64, 1)
    return {"gap_greedy": GREEDY, "budget_seam": (16, 32, 1), "quarter_best": BEST, "quarter_seam": BEST}.get(name, DEFAULT)


@functools.lru_cache(maxsize=None)
def case(name):
    c = _CASES[name]()
    assert c["name"] == name and c["opts"] == opts_of(name)
    return c


def cases():
    return [case(n) for n in names()]


# ---- preconditions, on the oracle alone ----------------------------------------------------------------------------------------------
def visits_of(c, t):
    if "part" in t:  # (a target of a train: the visits of the stand-alone case)
        c = case(t["part"])
        t = next(u for u in c["targets"] if u["claims"] is t["claims"])
    return walk(c["data"], t["p"], quarter(c["opts"], t["prev"][0]), t["prev"][0])[1]


def _claims_hold(c, t, visits):
    """the structural claims of a target, read off the model's visit list"""
    cl, p, data = t["claims"], t["p"], c["data"]
    what = "%s, target at %d: %s" % (c["name"], p, cl)
    hits = [v["rank"] for v in visits if v["hit"]]
    real = [v["rank"] for v in visits if v["hit"] and v["length"] > v["best"]]
    false = [v["rank"] for v in visits if v["hit"] and v["length"] <= v["best"]]
    h = _hashes(data)
    bucket = [int(q) for q in np.nonzero(h[:p] == h[p])[0][::-1]] if p + 2 < len(data) else []
    own = [q for q in bucket if q // EPOCH == p // EPOCH]
    if "first" in cl:
        assert real[0] == cl["first"] and hits[0] == real[0], what
    if "gap" in cl:
        assert real[1] - real[0] - 1 == cl["gap"] and not false, what
    if "false" in cl:
        assert [r - real[0] - 1 for r in false] == cl["false"], what
        assert all(visits[r]["length"] >= 3 for r in false), what
    if "real" in cl:
        assert real[1] - real[0] - 1 == cl["real"] and len(real) == 2, what
    if cl.get("false_last"):
        assert false[-1] == len(bucket) - 1 == visits[-1]["rank"], what
    if "n1" in cl:
        assert len(own) == cl["n1"], (what, len(own))
    if "own_end" in cl:
        own_hits = [r for r in hits if r < len(own)]
        assert len(own) - 1 - own_hits[-1] == cl["own_end"], what
    v = cl.get("variant")
    if v == "epoch0":
        assert p < EPOCH and len(bucket) == len(own), what
    if v == "empty_prev":
        assert p >= EPOCH and len(bucket) == len(own), what
    if v in ("prev_decisive", "n1_zero"):
        assert p >= EPOCH and len(bucket) > len(own) and all(q // EPOCH == p // EPOCH - 1 for q in bucket[len(own):]), what
        assert real[-1] >= len(own), what
    if "prev_rank" in cl:
        assert real[-1] - len(own) == cl["prev_rank"], what
    if "dist" in cl:
        assert t["tok"][2] == cl["dist"], what
    if "beyond" in cl:
        far = p - cl["beyond"]
        assert far in bucket and all(data[far + i] == data[p + i] for i in range(t["tok"][1] + 1)), what
        assert all(v["q"] != far for v in visits), what
    if "win_last" in cl:
        k = cl["win_last"]
        assert visits[-1]["dist"] == WINDOW and visits[-1]["rank"] - hits[-1] == k, what
        nxt = bucket[len(visits)]
        assert p - nxt > WINDOW and bytes(data[nxt:nxt + 10]) == bytes(data[p:p + 10]), what
    if "decisive" in cl:
        assert real[-1] == cl["decisive"], what
    if "longer_at" in cl:
        q = bucket[cl["longer_at"]]
        assert len(visits) == cl["longer_at"] and all(data[q + i] == data[p + i] for i in range(t["tok"][1] + 1)), what
    if "half" in cl:
        assert cl["half"] == c["opts"][0] // 2 and c["opts"][0] >= 16, what
        lens = [(v["rank"] >= cl["half"], v["length"]) for v in visits if v["hit"]]
        if cl["side"] == "tie":
            assert [v["rank"] >= cl["half"] for v in visits if common(data, p, v["q"]) == 8] == [False, True] and lens == [(False, 8)], what
        elif cl["side"] == "far_longer":
            assert lens == [(False, 8), (True, 9)], what
        else:
            assert real == [cl["half"] + cl["side"]], what
    if "q" in cl:
        q, lp = cl["q"], cl["prev_length"]
        assert q == c["opts"][0] >> 2 and c["opts"][1] > 32 and t["prev"][0] == lp and 32 <= lp < c["opts"][1], what
        would = [r for r, x in enumerate(bucket) if p - x <= WINDOW and data[x + lp - 1] == data[p + lp - 1] and data[x + lp] == data[p + lp]]
        longer = [r for r in would if common(data, p, bucket[r]) > lp]
        assert longer == [q + cl["q_side"]] and len(visits) == min(q, len(bucket)), (what, longer, len(visits))
        if cl["q_variant"] == "hits":
            assert any(r < q for r in would if r not in longer) and any(r >= q for r in would if r not in longer), (what, would)
        if cl["q_variant"] == "no_hit_behind":
            assert longer[0] == len(bucket) - 1, what
        if cl["q_variant"] == "prev_epoch":
            assert 0 < len(own) < q - 2, what
    if "length" in cl:
        assert t["tok"][1] == cl["length"], what
    if "run_pieces" in cl:
        e = p // EPOCH * EPOCH
        runs = sum(1 for k in range(e, min(e + EPOCH, len(data) - 511), 512) if len(set(data[k:k + 512])) == 1)
        assert runs >= cl["run_pieces"] >= 40, (what, runs)
    if "run_break" in cl:
        assert len(set(data[p - 1:p - 1 + cl["run_break"]])) == 1 and data[p - 1 + cl["run_break"]] != data[p] != data[p - 2], what
    if "run_edge" in cl:
        lo, hi = p, p
        while data[lo - 1] == data[p]:
            lo -= 1
        while hi < len(data) and data[hi] == data[p]:
            hi += 1
        assert lo < EPOCH < hi and hi - lo == MAX_MATCH + cl["run_edge"] and cl["epoch_pos"] == p - EPOCH, (what, lo, hi)
        assert visits[0]["dist"] == 1 and visits[0]["length"] == t["tok"][1], what
    if "J" in cl:
        e = (len(data) - 1) // EPOCH * EPOCH
        assert min(len(data) - 2 - e, EPOCH) == cl["J"], what
    if cl.get("last64"):
        order = sorted((int(h[x]), x) for x in range((len(data) - 1) // EPOCH * EPOCH, len(data) - 2))
        assert order.index((int(h[p]), p)) >= len(order) - 64, (what, order.index((int(h[p]), p)), len(order))
    if "whole" in cl:
        assert len(data) == cl["whole"], what
    if "p16" in cl:
        assert (p % 16, (p - t["tok"][2]) % 16) == (cl["p16"], cl["q16"]), what
    if "left" in cl:
        assert len(data) - p == cl["left"], what
    if cl.get("beyond_max"):
        q = p - t["tok"][2]
        assert bytes(data[q:q + 280]) == bytes(data[p:p + 280]), what
    if "equal" in cl:
        ln = t["tok"][1]
        eq = [v for v in visits if common(data, p, v["q"]) == ln]
        assert len(eq) == cl["equal"] and eq[0]["dist"] == t["tok"][2], what
        if cl.get("where") == "seam":
            assert eq[0]["q"] // EPOCH != eq[-1]["q"] // EPOCH or len(own) <= eq[0]["rank"], what
        if cl.get("where") == "batch64":
            idx = sorted(len(bucket) - 1 - v["rank"] for v in eq)
            assert len(bucket) > 64 and idx[0] < 64 <= idx[-1], (what, idx)


def check(c):
    """assert a case on the oracle: (a) the oracle's token at every target is the model's and the declared one, (b) the
    structural claims hold on the model's visit list, (c) a claim about the budget: one check less gives another token.  The
    case must not take the first-window re-warm (Q1): no block of the oracle's ends inside the first 32 768 bytes but the last."""
    data, opts = c["data"], c["opts"]
    toks = tokens_at(data, opts)
    ob.encode(data, opts=ob.make_opts(*opts))
    blocks = ob.trace_blocks()
    assert len(blocks) == 1 or blocks[0]["in_bytes"] > WINDOW, (c["name"], blocks[:2])
    fewer = None
    for t in c["targets"]:
        what = "%s, target at %d" % (c["name"], t["p"])
        if t["prev"] != (0, 0):
            assert walk(data, t["p"] - 1, opts[0])[0] == t["prev"], (what, walk(data, t["p"] - 1, opts[0])[0])
        at, tok = predict(data, t, opts)
        assert (at, tok) == (t["at"], t["tok"]), "%s: the model gives %s at %d, the case declares %s at %d" % (what, tok, at, t["tok"], t["at"])
        assert toks.get(at) == tok, "%s: the oracle has %s at %d, the model %s" % (what, toks.get(at), at, tok)
        _claims_hold(c, t, visits_of(c, t))
        if t["claims"].get("budget"):
            if fewer is None:
                fewer = tokens_at(data, (opts[0] - 1,) + tuple(opts[1:]))
            assert fewer.get(at) != tok, "%s: one check less and the oracle still has %s" % (what, tok)
    return toks


def covered(family):
    """{claim key: set of values} over all targets of a family"""
    out = {}
    for n in names():
        c = case(n)
        if c["family"] != family:
            continue
        out.setdefault("opts", set()).add(c["opts"])
        for t in c["targets"]:
            for k, v in t["claims"].items():
                out.setdefault(k, set()).update(v if isinstance(v, list) else [v])
    return out


# ---- trains: all cases of a level in one input, behind a lead-in ------------------------------------------------------------------------
TRAINS = {"default": DEFAULT, "best": BEST}
RUN_EPOCH_RUNS = 40  # of the 64 aligned 512-byte pieces of the run epoch


def run_epochs(k, seed):
    """k epochs of which 40 of the 64 aligned 512-byte pieces are a run of one byte (the sort marks an epoch with more than 32)"""
    rest = EPOCH - 512 * RUN_EPOCH_RUNS
    text = datagen.text_like(k * rest + 8, seed)
    return b"".join(bytes(512 * RUN_EPOCH_RUNS) + text[e * rest:(e + 1) * rest] for e in range(k))


def in_train(c):
    """cases about the end of the input stay out of the trains"""
    return not c["name"].startswith(("cut_", "last_two", "tail_", "whole_"))


@functools.lru_cache(maxsize=None)
def train(level, lead_epochs=2, lead="text"):
    """lead-in (text, or run epochs), then every case of the level: a guard epoch of zeros -- it shares no bucket with any case and
    puts everything before it out of the window and out of the previous epoch --, the case, text up to the next epoch.  The
    targets keep their claims; `part` names the case a target came from."""
    opts = TRAINS[level]
    parts = [run_epochs(lead_epochs, 900) if lead == "run" else datagen.text_like(lead_epochs * EPOCH + 8, 901)[:lead_epochs * EPOCH]]
    n, targets = lead_epochs * EPOCH, []
    for name in names():
        c = case(name)
        if c["opts"] != opts or not in_train(c):
            continue
        fill = -len(c["data"]) % EPOCH
        parts += [bytes(EPOCH), c["data"], datagen.text_like(fill + 8, 902)[:fill]]
        targets += [dict(t, p=t["p"] + n + EPOCH, at=t["at"] + n + EPOCH, part=name) for t in c["targets"]]
        n += EPOCH + len(c["data"]) + fill
    data = b"".join(parts)
    assert len(data) == n and n % EPOCH == 0
    return dict(name="train_%s_%d_%s" % (level, lead_epochs, lead), family="train", data=data, opts=opts, targets=targets)


# The trains of tests/test_match_walk_gpu.py: (level, epochs in all, lead-in, the (split, single, both-tables kernel) the host's
# rules give for that many epochs on 256 compute units, the form in words).  The lead-in is what is left of `epochs`.
TRAIN_FORMS = [
    ("default", 256, "text", (1, False, True), "whole epochs in the both-tables kernel: two fibres a wave, the results turned round through the LDS"),
    ("default", 511, "run", (1, False, False), "k_match3 proper, whole epochs (just under the 16 MiB from which a host call goes over in pieces)"),
    ("default", 300, "text", (3, False, False), "k_match3 in parts, no turn-round"),
    ("best", 256, "run", (1, False, True), "whole epochs in the both-tables kernel, quarter table"),
    ("best", 9, "text", (16, False, True), "the both-tables kernel in 16 parts without SINGLE"),
]
SMALL_TRAINS = [("default", "text"), ("default", "run"), ("best", "text")]  # (two epochs of lead-in)


def train_of(level, epochs, lead):
    """the train of a level with a lead-in that makes it `epochs` epochs long"""
    body = len(train(level, 0, lead)["data"]) // EPOCH
    assert epochs >= body, (epochs, body)
    return train(level, epochs - body, lead)


def check_train(tr):
    """the oracle's token at every target of the train is the token of the stand-alone case"""
    toks = tokens_at(tr["data"], tr["opts"])
    for t in tr["targets"]:
        assert toks.get(t["at"]) == t["tok"], "%s, target at %d (%s): the oracle has %s, alone %s" % (tr["name"], t["p"], t["part"], toks.get(t["at"]), t["tok"])
    return len(tr["targets"])


# ---- the host's rules, restated (tests/test_match_walk_gpu.py, tests/test_match_walk_swz_gpu.py) ----------------------------------------
def plan(n_ep, n_cu):
    """deflate_host.inc:457-471 match3_split, :568-573 walk_plan, :585 the both-tables launch -> (split, single, both)"""
    costs = [((n_ep * s + n_cu - 1) // n_cu) * (1.35 + 16.0 / s) for s in range(1, 17)]
    split = 1
    for s in range(2, 17):
        if costs[s - 1] < costs[split - 1] - 1e-9:
            split = s
    return split, split >= 16 and n_ep * split * 2 <= n_cu, n_ep * split <= 256


# ---- the permuted-table form (k_match3_swz, PairWinT<true>): only an epoch of 1024 or more positions can carry k_sort's mark -------------
SWZ_MIN_J = 1024


def in_long_epochs(c):
    """the targets of a case or train that lie in an epoch with 1024 or more positions that have a hash byte"""
    n = len(c["data"])
    return [t for t in c["targets"] if min(max(n - 2 - t["p"] // EPOCH * EPOCH, 0), EPOCH) >= SWZ_MIN_J]


def needs_padding(c):
    """a case of the trains' kind (not about the end of the input) with a target in a short last epoch"""
    return in_train(c) and len(in_long_epochs(c)) < len(c["targets"])


@functools.lru_cache(maxsize=None)
def padded(name):
    """the case with text behind it up to the end of its last epoch, as in a train: every target then lies in a full epoch"""
    c = case(name)
    fill = -len(c["data"]) % EPOCH
    return dict(c, name="padded_" + name, family="padded", data=c["data"] + datagen.text_like(fill + 8, 903)[:fill],
                targets=[dict(t, part=name) for t in c["targets"]])


# ---- what a failing parity test prints -------------------------------------------------------------------------------------------------
def _flat(stream):
    out = []
    for b, blk in enumerate(decode(stream, strict=False)):
        if blk.get("stored") is not None:
            out.append((b, ("stored", blk["stored"])))
        out += [(b, ("lit", v) if ln == 0 else ("ld", ln, v)) for ln, v in blk["toks"]]
        if blk.get("error"):
            out.append((b, ("error", blk["error"])))
    return out


def match_diff(got, want, c=None):
    """Where two streams part: the first differing token, its input position, and -- for a case -- the target it belongs to with
    the model's visit list around the decisive rank.  None for streams that read the same."""
    if got == want:
        return None
    fg, fw = _flat(got), _flat(want)
    pos = 0
    for i, (g, w) in enumerate(zip(fg, fw)):
        if g != w:
            break
        pos += w[1][1] if w[1][0] in ("ld", "stored") else 1
    else:
        i = min(len(fg), len(fw))
        if len(fg) == len(fw):
            return "the same tokens in other bytes (%d bytes, expected %d): a header or a block boundary differs" % (len(got), len(want))
    g = fg[i] if i < len(fg) else None
    w = fw[i] if i < len(fw) else None
    msg = "token %d at input position %d: got %s, expected %s" % (i, pos, g and g[1], w and w[1])
    for t in (c["targets"] if c else ()):
        if t["at"] - 1 <= pos <= t["p"] + 1:
            visits = visits_of(c, t)
            dec = next((k for k, v in enumerate(visits) if v["dist"] == (t["tok"][2] if t["tok"][0] == "ld" else -1)), len(visits) - 1)
            near = ["%d:%s%s" % (v["rank"], "d%d" % v["dist"], ("=%d" % v["length"]) if v["hit"] else "") for v in visits[max(0, dec - 9):dec + 10]]
            msg += "; target at %d of %s, declared %s, claims %s; visits rank:distance[=compared length] %s" % (
                t["p"], c["name"], t["tok"], t["claims"], " ".join(near))
            break
    return msg
