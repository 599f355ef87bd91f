"""Inputs that drive the parse (k_emit<0|1|2> with emit_body.inc, k_spec_check, k_small_fix, k_scan_a, k_compact, the exact way
through k_seg_exit / k_level_up / k_level_down / k_tree_top, and the batch forms kb_emit and kb_small_fix) onto its edges: the
seam between two segments, the run-up of 128 positions, the check and the repair of speculative entries, the lazy step from
nine lengths and its escalation, the steps filed by k_adv, the token slot of a segment, the tree of the exact way.

Everything is generated here from fixed seeds; no data file is committed.  A case is a dict(name, family, data, opts, claims):
`opts` = (max_hash_checks, lazy_if_less_than, matching_type); `claims` says what the case must force, in terms of the model, and
check() holds the case to it -- a generator that misses fails on the CPU instead of emptying the GPU test.

The model (model()) is plain Python over the restart steps of every position, which tests/hostsim exports (hostsim_binding.steps:
stages.h adv_pack(parse_step(...)) from the tables hostsim_encode uses).  It restates the rules of the kernels -- each constant
with the line that sets it:
  SEG = 1024         deflate_kernels.hip SEG      positions per segment; a segment's tokens are those of the steps that START in it
  SPEC_W = 128       deflate_kernels.hip SPEC_W   the run-up: segment k > 0 follows the steps from k * SEG - 128 and takes the first
                                               restart position at or behind k * SEG as its entry (emit_body.inc:9-11, :105-115)
  heads              deflate_kernels.hip          spec_run_head: entry != the exit before it, and segment i - 1 is not such a one
                                               (or i == 1)
  FIX_MAX = 1024     deflate_kernels.hip FIX_MAX  more heads than that: nothing is repaired (k_spec_check, k_small_fix, body_k_emit.inc)
  FIX_HOPS = 24      deflate_kernels.hip FIX_HOPS a repair wave parses its head from the exit the check saw and goes on into the next
                                               segment unless: the data ends, 24 segments are done, the next one is listed, or its
                                               entry is where this one was left (emit_body.inc:203-207)
  SMALL_SEGS = 2048  deflate_kernels.hip k_small_fix  up to that many segments the check and repair are k_small_fix's
  SPEC_PAUSE = 16    deflate_host.inc:478      what is still inconsistent after the repair sends the call the exact way and sets the
                                               context's counter to 17; every call takes one off first and speculates at 0
                                               (:483, :835-836): the call itself again and the next 15 are exact, the 16th speculates
  ADV_RUN_MANY = 31  stages.h:868              deferrals an entry of k_adv holds; from 31 on k_emit runs the step itself
  nine lengths       emit_body.inc:62-82       STEPS form: the step of position r0 + q (r0 a multiple of 4) from the lengths at
                                               r0 .. r0 + 8; a chain with q + deferrals >= 8 runs parse_step
A call that falls back is run again with a cleared state (deflate_host.inc:966, :1127-1131), so it reports spec_repaired == 0.

Building blocks.  Literal stretches come from a 14-bit counter written as two bytes (0x80 | high six bits, low eight bits): no
trigram of the stretch occurs twice within a window, and every trigram holds a byte that text never has.  A climb of c deferrals
from length L0 at a target: T over 0xC0..0xFF, pieces T[i : i + L0 + i] + a byte 0x01 for i = c .. 0 in front of it, T followed by
0x02 -- position p + i finds piece i, of length L0 + i, and p + c + 1 finds nothing longer.  Periodic gaps are zero bytes in text
(datagen.text_like).  In the trains a case stands behind 32 KiB + of text that it shares nothing with.
"""
import functools
import random

import numpy as np

import datagen
import hostsim_binding as hs
import oracle_binding as ob
from match_cases import _flat

SEG, SPEC_W, FIX_HOPS, FIX_MAX, SMALL_SEGS, SPEC_PAUSE, ADV_RUN_MANY, NINE = 1024, 128, 24, 1024, 2048, 16, 31, 9
EXACT_CALLS = SPEC_PAUSE - 1  # calls behind one that fell back that parse the exact way
MAX_BUFFER_LENGTH = 31744
DEFAULT, FAST, BEST, GREEDY, NOHASH = (128, 32, 1), (1, 0, 0), (1768, 128, 1), (128, 32, 0), (0, 0, 0)
LAZY8, LAZY64 = (128, 8, 1), (128, 64, 1)  # custom lazy_if_less_than: the STEPS form / the steps of k_adv with the quarter table
LEVEL = {"default": DEFAULT, "fast": FAST, "best": BEST, "greedy": GREEDY, "nohash": NOHASH, "lazy8": LAZY8, "lazy64": LAZY64}


# ---- the model -------------------------------------------------------------------------------------------------------------------------
def steps_of(data, opts):
    """(adv, ntok, run) per position: the step's length, its tokens, the deferrals as the entry files them"""
    st, nl = hs.steps(data, *opts, with_nlit=True)
    adv = (st & 1023).astype(np.int64)
    ntok = np.where(adv == 1, 1, nl.astype(np.int64) + 1)
    return adv, ntok, ((st >> 10) & 31).astype(np.int64), (st >> 15).astype(np.int64)


def model(adv, n, ntok=None, spec_w=SPEC_W, hops=FIX_HOPS, fix_max=FIX_MAX, head_i1=True):
    """The parse of n bytes with the steps adv, as the kernels find it.  Returns a dict:
      path       the true restart positions            true_E / true_X  every segment's true entry and exit
      E, X       the speculative entry (after the run-up) and the exit from it
      bad        the failed boundaries                  heads            the first of every run of them (spec_run_head)
      hops       per head: the segments its wave parsed, and why it stopped ('end', 'hops', 'listed', 'met')
      still      the boundaries still inconsistent after the repair
      fallback   the call goes the exact way           repaired         what info reports: len(heads), 0 after a fallback
      tokens     tokens per segment on the true path"""
    adv = [int(x) for x in adv]
    K = (n + SEG - 1) // SEG
    path, j = [], 0
    while j < n:
        path.append(j)
        j += adv[j]
    tE, tX, tok = [n] * K, [n] * K, [0] * K
    for p in path:
        k = p // SEG
        tE[k] = min(tE[k], p)
        tok[k] += int(ntok[p]) if ntok is not None else 0
    nxt = n
    for k in range(K - 1, -1, -1):  # (a segment no step starts in: entered and left where the next one is entered)
        if tE[k] == n:
            tE[k] = nxt
        nxt = tE[k]
    for k in range(K):
        tX[k] = tE[k + 1] if k + 1 < K else max(n, path[-1] + adv[path[-1]] if path else 0)
    E, X = [0] * K, [0] * K

    def leave(j, b):
        while j < b:
            j += adv[j]
        return j

    for k in range(K):
        a0, b = k * SEG, min(n, (k + 1) * SEG)
        E[k] = leave(a0 - spec_w, a0) if k else 0
        X[k] = leave(E[k], b)
    bad = [k for k in range(1, K) if E[k] != X[k - 1]]
    heads = [k for k in bad if (head_i1 and k == 1) or (k >= 2 and E[k - 1] == X[k - 2])]
    E2, X2, hop_log = E[:], X[:], {}
    if len(heads) <= fix_max:
        listed = set(heads)
        for h in heads:
            k, given, hop, segs = h, X[h - 1], 0, []
            while True:
                E2[k] = given
                X2[k] = x = leave(given, min(n, (k + 1) * SEG))
                segs.append(k)
                k += 1
                if k >= K:
                    why = "end"
                elif hop + 1 >= hops:
                    why = "hops"
                elif k in listed:
                    why = "listed"
                elif E2[k] == x:
                    why = "met"
                else:
                    given, hop = x, hop + 1
                    continue
                break
            hop_log[h] = (segs, why)
    still = [k for k in range(1, K) if E2[k] != X2[k - 1]]
    fallback = bool(still)
    return dict(K=K, path=path, true_E=tE, true_X=tX, E=E, X=X, bad=bad, heads=heads, hops=hop_log, still=still, fallback=fallback,
                repaired=0 if fallback else len(heads), tokens=tok, E2=E2, X2=X2)


def four_step_jumps(adv, n, k, spec_w=SPEC_W):
    """emit_body.inc, lane 0 of the run-up of segment k: P[r] is four steps from r (fewer where they leave the segment); from
    a0 - 128 a jump is taken while it lands in front of a0.  Returns (the landings taken, the landing refused)."""
    a, a0, b = k * SEG - spec_w, k * SEG, min(n, (k + 1) * SEG)

    def four(r):
        t = r
        for _ in range(4):
            t += int(adv[t]) if t < b else 0
        return t

    j, taken = a, []
    while four(j) < a0:
        j = four(j)
        taken.append(j)
    return taken, four(j)


def lazy_steps_from_lengths(L, far, n, lazy_lt, lazy=True, window=NINE):
    """emit_body.inc:56-84: the steps of all positions from the lengths of the full-budget table (far: "too far"), those of the
    four positions r0 .. r0 + 3 from the `window` lengths at r0 .. r0 + window - 1; -1 where the kernel runs parse_step instead
    (q + run reaches 8: the chain may go on behind the ninth length)"""
    out = np.ones(n, dtype=np.int64)
    for j in range(n):
        if not (j + 2 < n and L[j] >= 3 and not far[j]):
            continue
        q, run = j % 4, 0
        while lazy and q + run < window - 1 and L[j + run] < lazy_lt and j + run + 3 < n and L[j + run + 1] > L[j + run]:
            run += 1
        out[j] = -1 if q + run >= NINE - 1 else run + L[j + run]
    return out


def lazy_form(c, window=NINE):
    """the STEPS form's steps of a case at Default or a custom lazy level without the quarter table"""
    tab = hs.match_table(c["data"], c["opts"][0])
    L = np.array([t & 0xFFFF for t in tab] + [0] * 16)
    far = np.array([(t & 0xFFFF) == 3 and (t >> 16) > 8192 for t in tab] + [False] * 16)
    return lazy_steps_from_lengths(L, far, len(c["data"]), c["opts"][1], c["opts"][2] == 1, window)


def escalated(c, many=ADV_RUN_MANY):
    """path positions whose step k_emit runs itself because the entry cannot hold its deferrals (emit_body.inc:173)"""
    adv, ntok, run, fromq = steps_cached(c)
    return [p for p in model_of(c)["path"] if adv[p] > 1 and ntok[p] - 1 >= many]


def over_slot(c, slot=SEG):
    """segments with more tokens than a slot of `slot` words holds"""
    return [k for k, t in enumerate(model_of(c)["tokens"]) if t > slot]


# ---- building blocks -------------------------------------------------------------------------------------------------------------------
class B:
    def __init__(self, seed=1):
        self.o = bytearray()
        self.ctr = (seed * 2654435761) % 32768 & ~1
        self.r = random.Random(seed)

    def __len__(self):
        return len(self.o)

    def lit(self, n):
        """n literal bytes: the counter stretch goes on"""
        k = np.arange(self.ctr, self.ctr + n)
        u = (k // 2) % 16384
        self.o += np.where(k % 2 == 0, 0x80 | (u >> 8), u & 0xFF).astype(np.uint8).tobytes()
        self.ctr += n
        return self

    def lit_to(self, pos):
        assert pos >= len(self.o), (pos, len(self.o))
        return self.lit(pos - len(self.o))

    def raw(self, bs):
        self.o += bs
        return self

    def text_to(self, pos, seed):
        return self.raw(datagen.text_like(pos - len(self.o) + 8, seed)[:pos - len(self.o)])

    def target(self, c, L0=3, last=0):
        """T for a climb of c deferrals from length L0, and its pieces (longest first: piece 0 stands next to what follows);
        last: the length of the climb's last match, piece c, where it is to be longer than L0 + c"""
        m = c + max(L0 + c, last)
        while True:
            t = bytes(0xC0 + self.r.randrange(64) for _ in range(m))
            if len({t[i:i + 3] for i in range(m - 2)}) == m - 2:
                break
        return t, b"".join(t[i:i + (L0 + i if i < c else m - c)] + b"\x01" for i in range(c, -1, -1))

    def match_of(self, ln):
        """a match of ln bytes (ln <= 258) at the current position: its source, a literal, the copy, a breaking byte"""
        t, _ = self.target(0, ln)
        return t


def _seg_up(x):
    return (x + SEG - 1) // SEG * SEG


# ---- the families ----------------------------------------------------------------------------------------------------------------------
def _case(name, family, b, opts, **claims):
    return dict(name=name, family=family, data=bytes(b.o if isinstance(b, B) else b), opts=opts, claims=claims)


def _max_chain(opts):
    return opts[1] - 3


def _slot(level, c, back, place, seed):
    """a segment of literals from its first byte with a climb of c deferrals at b - back: 1024 - back + c + 1 tokens (c == 0 and
    back == 0: literals only, 1024 tokens); place: the segment is the first one, a middle one, or stands in front of the last"""
    opts = LEVEL[level]
    b = B(seed)
    t, pieces = b.target(c) if back else (b"", b"")
    if place == "first":
        # (the pieces cannot stand in front: the climb's lengths are given by copies BEHIND each other inside the segment -- the
        # first segment is literals, pieces, literals, and its tokens are counted by the model)
        s = 0
    else:
        b.raw(pieces).lit_to(_seg_up(len(pieces) + 200))
        s = len(b) // SEG
    if place == "first":
        b.raw(pieces)
    b.lit_to((s + 1) * SEG - back).raw(t + b"\x02" if back else b"")
    tail = {"first": 2 * SEG + 77, "middle": 2 * SEG + 77, "last": 0}[place]
    b.lit_to(_seg_up(len(b)) + tail if place != "last" else max(len(b) + 1, (s + 1) * SEG + 300))
    want = SEG - back + c + 1 if back else SEG
    return _case("slot_%s_c%d_b%d_%s" % (level, c, back, place), "slot", b, opts, slot_seg=s, slot_tokens=want, chain=(c, (s + 1) * SEG - back) if back else None,
                 over=bool(back and c >= back), before_last=place == "last")


def _slot_block0(level):
    """the 31 744th token -- the last of block 0 -- at an index of 1024 or more of its segment's slot (the level without a hash,
    the control: at index 1023, no slot can hold more): literal segments, one in which a run of one byte saves as many tokens as
    it takes, then the segment whose climb at b - 1 puts 1023 + 29 + 1 tokens into its slot"""
    opts = LEVEL[level]
    if not opts[0]:
        return _case("slot_%s_block0" % level, "slot", B(77).lit(33 * SEG + 5), opts, block0=(30, SEG - 1), over=False)
    s, c, x = 31, 29, 15
    run = 0
    for attempt in range(3):
        b = B(77)
        t, pieces = b.target(c)
        b.lit_to((s - 2) * SEG + 10).raw(b"\x03" * run).lit_to((s - 1) * SEG + 10).raw(pieces).lit_to((s + 1) * SEG - 1).raw(t + b"\x02").lit_to((s + 3) * SEG + 5)
        cs = _case("slot_%s_block0" % level, "slot", b, opts, block0=(s, SEG + x), over=True)
        adv, ntok, _, _ = steps_of(cs["data"], opts)
        before = sum(model(adv, len(cs["data"]), ntok)["tokens"][:s])
        short = (MAX_BUFFER_LENGTH - 1 - (SEG + x)) - before  # tokens still to come in front of segment s (negative: to save)
        if short == 0:
            return cs
        # a run of R bytes is a literal and ceil((R - 1) / 258) matches
        want = -short + (run - 1 - (run + 256) // 258 if run else 0)
        run = next(R for R in range(3, 4 * SEG) if R - 1 - (R + 256) // 258 >= want)
    raise AssertionError("slot_block0: %d tokens off" % short)


def _chain_at(level, q, c, L0=3, seed=5, end_after=None, name=None, family="lazy", t_front=None):
    """a climb of c deferrals at a position p with p % 4 == q (t_front: p = segment end - t_front)"""
    opts = LEVEL[level]
    b = B(seed + 17 * c + q)
    t, pieces = b.target(c, L0)
    b.raw(pieces).lit_to(_seg_up(len(pieces) + 200))
    p = len(b) + SEG + 400 + q if t_front is None else len(b) + 2 * SEG - t_front
    b.lit_to(p).raw(t)
    if end_after is None:
        b.raw(b"\x02").lit_to(_seg_up(len(b)) + 333)
    elif end_after >= 0:
        b.raw(b"\x02"[:min(1, end_after)]).lit(max(0, end_after - 1))
    else:
        del b.o[end_after:]
    return _case(name or "%s_%s_q%d_c%d" % (family, level, q, c), family, b, opts, chain=(c, p), L0=L0, clipped=end_after is not None and end_after < 0)


TOO_FAR = 8192  # stages.h match_too_far: a match of three bytes further back than that is none (lz77.rs:275-278)


def _far(level, kind, dist, c=5, seed=83):
    """a copy of three bytes `dist` back, on the path between literals.  'alone': nothing else -- at dist > 8192 the position is a
    literal step, at 8192 a match of three (the control).  'climb': the three bytes are piece 0 of a climb of c deferrals whose
    other pieces stand near: at dist > 8192 its first position is a literal and the chain starts one further, with c - 1
    deferrals; at 8192 it starts there, with c.  The nine-length form reads `far` only at a step's first position: behind it a
    length that beats the one before is at least 4."""
    opts = LEVEL[level]
    b = B(seed + dist % 7 + c)
    p = 10 * SEG + 401
    if kind == "alone":
        t = bytes(0xC0 + b.r.randrange(64) for _ in range(3))
        b.lit_to(p - dist).raw(t + b"\x01").lit_to(p).raw(t + b"\x02").lit_to(12 * SEG + 9)
        return _case("lazy_%s_far_alone_%d" % (level, dist), "lazy", b, opts, far=(p, dist > TOO_FAR, 1 if dist > TOO_FAR else 3))
    t, pieces = b.target(c)
    near = b"".join(t[i:i + 3 + i] + b"\x01" for i in range(c, 0, -1))
    b.lit_to(p - dist).raw(t[:3] + b"\x01").lit_to(p - 400).raw(near).lit_to(p).raw(t + b"\x02").lit_to(12 * SEG + 9)
    isfar = dist > TOO_FAR
    return _case("lazy_%s_far_climb_%d" % (level, dist), "lazy", b, opts, far=(p, isfar, 1 if isfar else c + 3 + c),
                 chain=(c - 1, p + 1) if isfar else (c, p))


def _gap(name, level, lead_segs, gaps, tail_segs, family="repair", seed=41, total=None, **claims):
    """text with zero gaps: gaps = [(start in bytes from the end of the lead-in, length), ...] written over the text"""
    n = total or (lead_segs + tail_segs) * SEG + max((s + g for s, g in gaps), default=0)
    data = bytearray(datagen.text_like(n + 8, seed)[:n])
    for s, g in gaps:
        data[lead_segs * SEG + s:lead_segs * SEG + s + g] = bytes(g)
    return _case(name, family, data, LEVEL[level], text=True, **claims)


def _runs(level, r, lead_segs=3, tail_segs=4):
    """a zero gap of r + 0.5 segments from 300 bytes into a segment: r failed boundaries in a row, one head"""
    return _gap("repair_%s_r%d%s" % (level, r, "_head1" if lead_segs == 0 else "_to_end" if tail_segs == 0 else ""), level, lead_segs, [(300, r * SEG + 512)], tail_segs, run=r, nheads=1, head=lead_segs + 1,
                fallback=r > FIX_HOPS)


def _heads(name, level, heads, tail_segs=3, total=None, **claims):
    """an isolated head at each listed segment: 700 zero bytes across the boundary"""
    return _gap(name, level, 0, [(h * SEG - 350, 700) for h in heads], max(heads) + tail_segs, total=total, heads_at=list(heads), fallback=False, **claims)


def _seam(level, d, seed=9):
    """the previous segment is left d bytes into this one: a match of d + m bytes that starts m bytes in front of the boundary"""
    opts = LEVEL[level]
    b = B(seed + d)
    m = min(3, 258 - d)
    ln = d + m
    src = b.match_of(ln)
    b.lit(100).raw(src).raw(b"\x01").lit_to(3 * SEG - (ln - d)).raw(src).raw(b"\x02").lit_to(5 * SEG + 55)
    return _case("seam_%s_d%d" % (level, d), "seam", b, opts, seam=(3, d))


def _seam_chain(level, c=None, seed=19):
    """a step from the last position of a segment with c deferrals and a match of 258 bytes: the segment is left c + 257 bytes
    into the next one.  c = 1: d = 258, which no step without a deferral reaches; c = None: the level's longest chain, its largest
    step -- lazy_if_less_than - 3 deferrals, since the lengths in front of the last rise strictly from 3 and stay under
    lazy_if_less_than: d = 286 at Default, 382 at Best (MAX_JUMP - 1 = 519 is a bound no level reaches)"""
    opts = LEVEL[level]
    b = B(seed)
    name = "seam_%s_maxstep" % level if c is None else "seam_%s_d%d" % (level, c + 257)
    c = _max_chain(opts) if c is None else c
    t, pieces = b.target(c, 3, 258)
    b.raw(pieces).lit_to(_seg_up(len(pieces) + 200))
    s = len(b) // SEG + 2
    b.lit_to(s * SEG - 1).raw(t + b"\x02").lit_to((s + 3) * SEG + 55)
    assert len(t) == c + 258
    return _case(name, "seam", b, opts, seam=(s, c + 257), chain=(c, s * SEG - 1), step=(s * SEG - 1, c + 258))


def _covered_last(level, tail):
    """a last segment of `tail` bytes that the previous segment's last match covers whole: entered at its end, no tokens"""
    opts = LEVEL[level]
    b = B(23 + tail)
    ln = max(3, min(258, tail + 1))
    src = b.match_of(ln)
    b.lit(50).raw(src).raw(b"\x01").lit_to(2 * SEG - (ln - tail)).raw(src)
    assert len(b) == 2 * SEG + tail
    return _case("seam_%s_last%d" % (level, tail), "seam", b, opts, covered_last=tail)


def _tiny(level, n):
    return _case("seam_%s_n%d" % (level, n), "seam", datagen.text_like(n + 8, 3)[:n], LEVEL[level], n=n)


def _runup(level, kind, seed=31):
    opts = LEVEL[level]
    b = B(seed)
    a0 = 4 * SEG
    w0 = a0 - SPEC_W
    if kind == "on_path":  # the position a0 - 128 is itself on the path, literals all the way
        b.lit_to(6 * SEG + 9)
        return _case("runup_%s_%s" % (level, kind), "runup", b, opts, runup_literals=4, on_path=4)
    if kind.startswith("land"):  # a match ends on a0 - 1, a0, a0 + 1 behind literals
        # (lane 0 jumps four steps at a time from a0 - 128 while the jump stays in front of a0: on literals it stands on a0 - 128
        # + 4 i; the match starts three literals behind such a position, so ONE jump -- three literals and the match -- lands on
        # a0 + off: taken at a0 - 1, refused at a0 and a0 + 1, from where single steps go on)
        off = {"land-1": -1, "land0": 0, "land+1": 1}[kind]
        ln = 41 + off
        src = b.match_of(ln)
        b.lit(64).raw(src + b"\x01").lit_to(a0 + off - ln).raw(src + b"\x02").lit_to(6 * SEG + 9)
        assert (a0 + off - ln - w0) % 4 == 3
        return _case("runup_%s_%s" % (level, kind), "runup", b, opts, entry=(4, a0 + max(off, 0)), land=(4, a0 + off, off < 0))
    if kind == "covered":  # one match of 200 bytes over the whole run-up
        src = b.match_of(200)
        b.lit(64).raw(src + b"\x01").lit_to(w0 - 30).raw(src + b"\x02").lit_to(6 * SEG + 9)
        return _case("runup_%s_%s" % (level, kind), "runup", b, opts, no_restart_in_runup=4)
    if kind == "chain":  # a deferral chain straddles a0
        t, pieces = b.target(9)
        b.raw(pieces).lit_to(a0 - 4).raw(t + b"\x02").lit_to(6 * SEG + 9)
        return _case("runup_%s_%s" % (level, kind), "runup", b, opts, chain=(9, a0 - 4))
    # a path that is off at a0 - 128 and merges m positions into the run-up (m = 129: just behind it, a failed boundary):
    # a match that jumps over a0 - 128 and ends at a0 - 128 + m', inside which the run-up starts on literals ... here: zero run
    m = int(kind[5:])
    data = bytearray(datagen.text_like(7 * SEG + 8, seed)[:7 * SEG])
    # zeros from far in front of the run-up to w0 + m: the true path leaves the zeros by matches of 258 from their start, the
    # run-up's by matches of 258 from w0 -- the two meet where the zeros end only if they end within one match of both
    z0 = w0 - 258 * 2 - 100
    data[z0:w0 + m] = bytes(w0 + m - z0)
    return _case("runup_%s_%s" % (level, kind), "runup", data, opts, merge=m)


def _two_chains(name, first, plan, tail_segs=3, seed=51, family="repair", **claims):
    """A stretch in which two paths run side by side and never meet: D over 0xC0..0xFF with restart positions A_i (32 or 40 apart)
    and B_i = A_i + 16, and in front of it a copy of every D[A_i : A_i+1] and D[B_i : B_i+1], each behind a byte 0x01 -- at A_i the
    longest match ends at A_i+1, at B_i at B_i+1, and anywhere between the longer of the two wins.  The true path comes in on
    literals and takes the A's.  plan: for the boundaries first, first + 1, ... whether the run-up's first position (128 in front
    of the boundary) joins 'A' (8 behind an A_i) or 'B' (24 behind): segments that enter on B are consistent with each other
    and wrong.  Lengths of 32 and more: no lazy step at lazy_if_less_than = 32."""
    off = {"A": 8, "B": 24, "a": 14}  # ("a": the last position that joins the A chain -- one further defers to B_i, the lazy step)
    r0 = (first - 1) * SEG + 512
    r0 += (first * SEG - SPEC_W - off[plan[0]] - r0) % 8
    A, pos = [r0], r0
    for i, ch in enumerate(plan):
        t = (first + i) * SEG - SPEC_W - off[ch]
        d = t - pos
        assert d >= 160 and d % 8 == 0, (name, d)
        while d:
            st = 32 if d % 32 == 0 else 40
            pos, d = pos + st, d - st
            A.append(pos)
    while pos < (first + len(plan) - 1) * SEG + 300:
        pos += 32
        A.append(pos)
    b = B(seed)
    m = A[-1] - r0
    D = bytes(0xC0 + b.r.randrange(64) for _ in range(m))  # (a few trigrams occur twice: check() holds the case to its claims)
    Bs = [a + 16 for a in A[:-1]] + [A[-1]]
    dic = b"".join(D[x - r0:y - r0] + b"\x01" for x, y in zip(A, A[1:])) + b"".join(D[x - r0:y - r0] + b"\x01" for x, y in zip(Bs, Bs[1:]))
    assert len(dic) + 64 <= r0 and A[-1] - 64 < 32768, (name, len(dic), r0)
    b.lit(64).raw(dic).lit_to(r0).raw(D + b"\x02").lit_to(_seg_up(len(b)) + tail_segs * SEG + 9)
    return _case(name, family, b, DEFAULT, two_chains=(first, plan), **claims)


def _merge(m):
    """the run-up of segment 4 starts inside a match of the true path that ends m positions into the run-up (m <= 127: the paths
    are one from there on); 'behind': the run-up's first position finds a longer copy than the rest of that match, which ends 20
    bytes into the segment where the true match ends 5 bytes into it: one failed boundary, and the paths meet inside the segment"""
    b = B(61 + (m if m != "behind" else 0))
    a0 = 4 * SEG
    w0 = a0 - SPEC_W
    if m == "behind":
        ln, k = 200, 200 - (SPEC_W + 5)
        src, f = b.match_of(ln), bytes(0xC0 + b.r.randrange(64) for _ in range(15))
        b.lit(64).raw(src + b"\x01").lit(9).raw(src[k:] + f + b"\x01").lit_to(a0 + 5 - ln).raw(src + f + b"\x02").lit_to(7 * SEG + 9)
        return _case("runup_default_merge_behind", "runup", b, DEFAULT, heads_at=[4], hop_why={4: ([4], "met")}, fallback=False)
    ln = m + 40
    src = b.match_of(ln)
    b.lit(64).raw(src + b"\x01").lit_to(w0 + m - ln).raw(src + b"\x02").lit_to(7 * SEG + 9)
    return _case("runup_default_merge%d" % m, "runup", b, DEFAULT, merge=(4, w0 + m))


def _met_in_run(seed=43):
    """zeros from 300 bytes into segment 3 to 512 bytes into segment 6, begun where the run-up of segment 6 starts on the true
    path (a multiple of 258 behind the run's second byte): boundaries 4, 5 and 6 fail -- 6 only because segment 5 was entered wrong
    -- and the wave that repairs 4 and 5 finds segment 6 entered where it now leaves 5: it stops before the run ends"""
    z0 = 3 * SEG + 300
    z0 += (6 * SEG - SPEC_W - (z0 + 1)) % 258
    n = 10 * SEG
    data = bytearray(datagen.text_like(n + 8, seed)[:n])
    data[z0:6 * SEG + 512] = bytes(6 * SEG + 512 - z0)
    return _case("repair_default_met_in_run", "repair", data, DEFAULT, text=True, run=3, head=4, nheads=1, hop_why={4: ([4, 5], "met")}, fallback=False)


def _exact(K):
    n = (K - 1) * SEG + 517
    return _case("exact_K%d" % K, "exact", datagen.text_like(n + 8, 1000 + K)[:n], DEFAULT, K=K)


def _fixmax(nheads):
    """700 zero bytes across every second boundary, 1348 bytes of text between: one isolated head each"""
    K = 2 * nheads + 4
    n = K * SEG - 100
    data = bytearray(datagen.text_like(n + 8, 71)[:n])
    for i in range(nheads):
        at = (2 * i + 2) * SEG - 350
        data[at:at + 700] = bytes(700)
    return _case("fixmax_%d" % nheads, "fixmax", data, DEFAULT, text=True, nheads=nheads, fallback=nheads > FIX_MAX, K=K)


def _all_cases():
    out = []
    # token slot
    for level, cs in (("default", (0, 1, 2, 9, 29)), ("best", (1, 33, 125))):
        for c in cs:
            for back in ((1, 2) if c else (0,)):
                for place in ("first", "middle", "last"):
                    if (c in (9, 33) and (back == 2 or place != "middle")) or (place == "first" and (c > 1 or back > 1)):
                        continue  # (the first segment holds its climb's pieces itself, and from c = 2 on they save more tokens than the climb adds)
                    out.append(functools.partial(_slot, level, c, back, place, 3))
    out.append(functools.partial(_slot, "nohash", 0, 0, "middle", 3))
    out.append(functools.partial(_slot_block0, "default"))
    out.append(functools.partial(_slot_block0, "nohash"))
    # lazy step from nine lengths
    for level in ("default", "lazy8"):
        mx = _max_chain(LEVEL[level])
        for q in range(4):
            for c in range(0, 10):
                if c <= mx:
                    out.append(functools.partial(_chain_at, level, q, c))
        out.append(functools.partial(_chain_at, level, 2, mx, name="lazy_%s_longest" % level))
    out.append(functools.partial(_chain_at, "default", 2, 4, 28, name="lazy_default_reaches_lazy_lt"))
    for tf in range(12):
        out.append(functools.partial(_chain_at, "default", 0, 7, t_front=tf, name="lazy_default_front%d" % tf))
    out.append(functools.partial(_chain_at, "default", 0, 5, t_front=SEG - 255 - SPEC_W, name="lazy_default_chunk_lane"))
    for e in (0, 1, 2, 3, 4, -1, -3, -8):
        out.append(functools.partial(_chain_at, "default", 3, 6, end_after=e, name="lazy_default_end%+d" % e))
    # a match of three that is too far: alone and as the first piece of a climb, with the controls at the limit
    for level in ("default", "lazy8"):
        for kind in ("alone", "climb"):
            for dist in (TOO_FAR, TOO_FAR + 1):
                out.append(functools.partial(_far, level, kind, dist, 5 if level == "default" else 4))
    # steps filed by k_adv
    for level, cs in (("best", (29, 30, 31, 32, 33, 64, 125)), ("lazy64", (29, 30, 31, 33, 61))):
        for c in cs:
            out.append(functools.partial(_chain_at, level, c % 4, c, family="adv"))
    # seam
    for level in ("default", "best"):
        for d in (0, 1, 2, 3, 127, 128, 129, 257):
            out.append(functools.partial(_seam, level, d))
        out.append(functools.partial(_seam_chain, level, 1))
        out.append(functools.partial(_seam_chain, level, None))
    for tail in (1, 2, 3, 257):
        out.append(functools.partial(_covered_last, "default", tail))
    for n in (1023, 1024, 1025, 1500):
        out.append(functools.partial(_tiny, "default", n))
    # run-up
    for kind in ("on_path", "land-1", "land0", "land+1", "covered", "chain"):
        out.append(functools.partial(_runup, "default", kind))
    for m in (1, 64, 127, "behind"):
        out.append(functools.partial(_merge, m))
    # check and repair
    out.append(_met_in_run)
    # (one failed boundary and h segments entered on the wrong one of two paths behind it: the wave hops through all of them)
    for h in (2, 4):
        out.append(functools.partial(_two_chains, "repair_default_hops%d" % (h + 1), 12, "B" * (h + 1), nheads=1, hop_why={12: (list(range(12, 13 + h)), "met" if h < 23 else "hops")},
                                     fallback=h > 23))
    # (two runs with one good boundary between them: the second head's segment is entered right, the one before it wrong)
    out.append(functools.partial(_two_chains, "runup_default_last_on_A", 12, "a", family="runup", heads_at=[]))
    out.append(functools.partial(_two_chains, "repair_default_stops_at_listed", 14, "BBABB", heads=[14, 16], hop_why={14: ([14, 15], "listed")}))
    for level in ("default", "fast"):
        for r in (1, 2, 3, 23, 24, 25):
            out.append(functools.partial(_runs, level, r))
    out.append(functools.partial(_runs, "default", 2, 0, 4))   # the head is segment 1
    out.append(functools.partial(_runs, "default", 3, 3, 0))   # the run ends on segment K - 1
    for hd in ((63,), (64,), (65,), (255,), (256,), (257,), (3, 5, 8)):
        out.append(functools.partial(_heads, "heads_default_%s" % "_".join(map(str, hd)), "default", hd))
    for K in (64, 65, 128, 129):
        out.append(functools.partial(_heads, "heads_default_K%d" % K, "default", (K - 2,), total=K * SEG - 100, K=K))
    return out


TRAIN_ONLY = [functools.partial(_fixmax, h) for h in (1023, 1024, 1025)]
EXACT_K = (1, 2, 16, 17, 256, 257, 4096, 4097)


@functools.lru_cache(maxsize=None)
def _built():
    cs = [f() for f in _all_cases()]
    names_ = [c["name"] for c in cs]
    assert len(set(names_)) == len(names_), sorted(n for n in names_ if names_.count(n) > 1)
    return {c["name"]: c for c in cs}


def names():
    return list(_built())


def case(name):
    return _built()[name]


def opts_of(name):
    return case(name)["opts"]


@functools.lru_cache(maxsize=None)
def fixmax(nheads):
    return _fixmax(nheads)


@functools.lru_cache(maxsize=None)
def exact(K):
    return _exact(K)


_MODEL = {}


def model_of(c, **kw):
    """the model of a case (made once; with keywords: a mutant, made afresh)"""
    key = c["name"]
    if key not in _MODEL:
        adv, ntok, run, fromq = steps_of(c["data"], c["opts"])
        _MODEL[key] = (adv, ntok, run, fromq, model(adv, len(c["data"]), ntok))
    adv, ntok, run, fromq, m = _MODEL[key]
    if kw:
        return model(kw.pop("adv", adv), len(c["data"]), ntok, **kw)
    return m


def steps_cached(c):
    model_of(c)
    return _MODEL[c["name"]][:4]


# ---- preconditions ---------------------------------------------------------------------------------------------------------------------
def check(c):
    """the case forces what its claims say -- on the model, and the model's path is the oracle's"""
    data, cl, name = c["data"], c["claims"], c["name"]
    n = len(data)
    adv, ntok, run, fromq = steps_cached(c)
    m = model_of(c)
    # the oracle: the model's path is where its tokens start, and a segment's tokens are the oracle's that start in it
    if n <= (1 << 18):
        pos, starts, per = 0, np.zeros(n + 1, dtype=np.int64), [0] * m["K"]
        for tok in ob.lz77(data, *c["opts"]):
            starts[pos] = 1
            pos += 1 if tok[0] == "lit" else tok[1]
        assert pos == n and all(starts[p] for p in m["path"]), name
        cum = np.concatenate([[0], np.cumsum(starts)])
        for p in m["path"]:  # (a step's tokens -- its deferred literals and its match -- belong to the segment the step starts in)
            per[p // SEG] += int(cum[min(n, p + int(adv[p]))] - cum[p])
        assert per == m["tokens"], (name, [(k, a, b) for k, (a, b) in enumerate(zip(per, m["tokens"])) if a != b][:4])
    if "chain" in cl and cl["chain"]:
        cc, p = cl["chain"]
        assert p in set(m["path"]), (name, "the chain's first position is not on the path", p)
        got = int(ntok[p]) - 1 if adv[p] > 1 else 0
        if cl.get("clipped"):  # (the data ends inside the climb: the lengths stop rising where the room ends)
            assert 0 < got < cc, (name, "deferrals", got, "of", cc)
        else:
            assert got == cc, (name, "deferrals", got, "wanted", cc)
            assert int(run[p]) == min(cc, ADV_RUN_MANY), name
    if cl.get("slot_tokens") is not None:
        s = cl["slot_seg"]
        assert m["true_E"][s] == s * SEG and m["tokens"][s] == cl["slot_tokens"], (name, m["true_E"][s], m["tokens"][s], cl["slot_tokens"])
        assert not m["bad"], (name, m["bad"])
        if cl.get("before_last"):
            assert s == m["K"] - 2, name
    if "over" in cl:
        assert (max(m["tokens"]) > SEG) == bool(cl["over"]), (name, max(m["tokens"]))
    if "seam" in cl:
        s, d = cl["seam"]
        assert m["true_E"][s] == s * SEG + d and m["E"][s] == m["true_E"][s], (name, m["true_E"][s] - s * SEG, d)
    if "covered_last" in cl:
        assert m["K"] == 3 and m["true_E"][2] == n and m["tokens"][2] == 0 and n - 2 * SEG == cl["covered_last"], (name, m["true_E"], n)
    if "n" in cl:
        assert n == cl["n"] and m["K"] == (2 if n > SEG else 1)
    if "runup_literals" in cl:
        k = cl["runup_literals"]
        assert all(adv[j] == 1 for j in range(k * SEG - SPEC_W, k * SEG)) and (k * SEG - SPEC_W) in set(m["path"]), name
    if "entry" in cl:
        k, e = cl["entry"]
        assert m["E"][k] == e == m["true_E"][k], (name, m["E"][k], m["true_E"][k], e)
    if "land" in cl:
        k, at, is_taken = cl["land"]
        taken, refused = four_step_jumps(adv, n, k)
        assert (at in taken) if is_taken else (refused == at), (name, taken[-3:], refused, at)
        assert (k * SEG - SPEC_W) in set(m["path"]), name
    if "step" in cl:
        p, ln = cl["step"]
        assert p in set(m["path"]) and int(adv[p]) == ln, (name, int(adv[p]), ln)
    if "far" in cl:
        p, isfar, ln = cl["far"]
        t = hs.match_table(data, c["opts"][0])[p]
        assert ((t & 0xFFFF) == 3 and (t >> 16) > TOO_FAR) == isfar and (t & 0xFFFF) == 3, (name, t & 0xFFFF, t >> 16)
        assert p in set(m["path"]) and int(adv[p]) == ln, (name, int(adv[p]), ln)
    if c["family"] == "adv":
        # (parse_step: the match that beats a pending one of 32 or more is looked up in the quarter-budget table.  A climb from
        # length 3: the pending match in front of the last deferral is c + 2 long)
        cc, p = cl["chain"]
        assert c["opts"][0] >> 2 and int(fromq[p]) == (1 if cc + 2 >= 32 else 0), (name, cc, int(fromq[p]))
    if "no_restart_in_runup" in cl:
        k = cl["no_restart_in_runup"]
        assert not [p for p in m["path"] if k * SEG - SPEC_W <= p < k * SEG], name
    if "run" in cl:
        h, r = cl["head"], cl["run"]
        assert m["bad"] == list(range(h, h + r)) and m["heads"] == [h], (name, m["bad"], m["heads"])
    if "heads_at" in cl:
        assert m["heads"] == cl["heads_at"] == m["bad"], (name, m["heads"], m["bad"])
    if "heads" in cl:
        assert m["heads"] == cl["heads"], (name, m["heads"], m["bad"])
    if "nheads" in cl:
        assert len(m["heads"]) == cl["nheads"], (name, len(m["heads"]))
    if "fallback" in cl:
        assert m["fallback"] == cl["fallback"], (name, m["still"], m["hops"])
    if "hop_why" in cl:
        for h, want in cl["hop_why"].items():
            assert m["hops"].get(h) == want, (name, m["hops"])
    if "merge" in cl:
        k, at = cl["merge"]
        mine, j = [], k * SEG - SPEC_W
        while j < k * SEG:
            mine.append(j)
            j += int(adv[j])
        on = set(m["path"])
        assert (k * SEG - SPEC_W) not in on and [p for p in mine if p in on][0] == at and all(p not in on for p in mine if p < at), (name, mine[:5], at)
    if "block0" in cl:
        s, idx = cl["block0"]
        assert sum(m["tokens"][:s]) + idx == MAX_BUFFER_LENGTH - 1 and m["tokens"][s] > idx, (name, sum(m["tokens"][:s]), m["tokens"][s])
    if "K" in cl:
        assert m["K"] == cl["K"], (name, m["K"])
    return m


# ---- trains: the cases of a level behind a lead-in that puts K above 2048 -----------------------------------------------------------------
TRAINS = [("default", "slot seam runup"), ("default", "lazy"), ("default", "repair"), ("best", "slot adv seam"), ("fast", "repair"),
          ("lazy8", "lazy"), ("lazy64", "adv")]
GUARD = 33 * SEG
TRAIN_SEGS = 2100


@functools.lru_cache(maxsize=None)
def train(level, families, extra=None):
    """text, then every case of the level and the families, each behind a guard of 33 segments of text: more than a window, so a
    case finds nothing of what stands in front of it, and a whole number of segments, so its segments stay its segments.  The
    lead-in is what is left of 2100 segments: the check and the repair of a train are k_spec_check's and k_emit<2>'s.
    extra: one of the three FIX_MAX inputs instead of the cases"""
    opts = LEVEL[level]
    cs = [case(nm) for nm in names() if case(nm)["opts"] == opts and case(nm)["family"] in families.split() and "_end" not in nm
          and "covered_last" not in case(nm)["claims"] and "n" not in case(nm)["claims"]]
    if extra is not None:
        cs = [fixmax(extra)]
    body = sum(GUARD + _seg_up(len(c["data"])) for c in cs) // SEG
    lead_segs = max(40, TRAIN_SEGS - body)
    parts, n, where = [datagen.text_like(lead_segs * SEG + 8, 901)[:lead_segs * SEG]], lead_segs * SEG, []
    for i, c in enumerate(cs):
        g = datagen.text_like(GUARD + 8, 902 + i)[:GUARD]
        fill = -len(c["data"]) % SEG
        parts += [g, c["data"], datagen.text_like(fill + 8, 903)[:fill]]
        where.append((c["name"], n + GUARD))
        n += GUARD + len(c["data"]) + fill
    data = b"".join(parts)
    assert len(data) == n and n < (5 << 20) and cs, (level, families, n)
    return dict(name="train_%s_%s_%s" % (level, families.replace(" ", "_"), extra), family="train", data=data, opts=opts, claims={}, where=where)


def check_train(tr):
    """in the train every case keeps its steps (so its chains, seams and slots), and its heads are the train's heads there"""
    adv, ntok, run, fromq = steps_cached(tr)
    m = model_of(tr)
    for name, at in tr["where"]:
        c = case(name) if name in _built() else fixmax(int(name.split("_")[1]))
        cadv = steps_cached(c)[0]
        lo = 3  # (the first positions of a case see the guard's last bytes in their trigrams' buckets only through hashes: no match)
        text = c["claims"].get("text") or c["family"] == "fixmax"  # (text finds the guard's text: the gaps keep their boundaries)
        same = text or np.array_equal(adv[at + lo:at + len(cadv) - 3], cadv[lo:-3])  # (and its last ones the fill behind it)
        assert same, (tr["name"], name, "the steps of the case change in the train", int(np.argmax(adv[at:at + len(cadv)] != cadv)))
        mc_ = model_of(c)
        k0 = at // SEG
        assert [h - k0 for h in m["heads"] if k0 <= h < k0 + mc_["K"]] == mc_["heads"], (tr["name"], name)
        assert text or [t for t in m["tokens"][k0 + 1:k0 + mc_["K"] - 1]] == mc_["tokens"][1:-1], (tr["name"], name)
    assert m["K"] > SMALL_SEGS
    return m


# ---- what a failing parity test prints ----------------------------------------------------------------------------------------------------
def parse_diff(got, want, c=None):
    """Where two streams part: the first differing token, its input position, its segment, and the model's entries and exits
    around it.  None for streams that read the same."""
    if got == want:
        return None
    fg, fw = _flat(got), _flat(want)
    pos, i = 0, 0
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
    msg = "token %d at input position %d (segment %d, byte %d of it): got %s, expected %s" % (i, pos, pos // SEG, pos % SEG, g and g[1], w and w[1])
    if c is not None:
        m = model_of(c)
        k = pos // SEG
        near = ["seg %d: entry %+d (speculative %+d) exit %+d tokens %d%s" % (
            s, m["true_E"][s] - s * SEG, m["E"][s] - s * SEG, m["true_X"][s] - (s + 1) * SEG, m["tokens"][s],
            " head" if s in m["heads"] else " bad" if s in m["bad"] else "") for s in range(max(0, k - 2), min(m["K"], k + 3))]
        msg += "; model of %s: %s; heads %s, still %s" % (c["name"], "; ".join(near), m["heads"][:8], m["still"][:8])
    return msg
