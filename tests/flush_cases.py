"""Streams that are written in pieces and flushed (deflate_host.inc mi355_deflate_stream_write / _flush / stream_encode), on write
patterns that put a flush point, a position the pattern files differently, or the end of the kept history on the geometry of the
kernels that read them: the cut of a match or a run at the end of the data the encoder had (k_match3 / k_match TileLimit, k_rle left,
k_adv, k_emit rel_end), the hash lists of stages.h HashOverride (hol, skw, pts), the hand-over from the link path to the sorted path
in launch_match_tables (e_first, n_old), the trim of the history (base), the block stage's m segment ends.

Everything is generated here from fixed seeds; no data file is committed.  A case is dict(name, family, data, opts, script, targets,
claims): `script` is a list of write lengths and "F" (a flush) that ends with the rest of the data; `plain` is the script a target's
token is compared with -- the same flush points, every segment in one write; where the pattern is a flush itself (a flush after the
stream's first one or two bytes, two flushes one or two bytes apart) that flush is left out of it.  A target is dict(p, kind, claim,
q): the position whose token the oracle decides, the quirk kind (KINDS; cut, defer, quarter, edge, control and the like elsewhere),
the affected position q, and one of
  changes     the oracle's token at p under the script differs from its token under `plain`; the model predicts both
  unchanged   the two tokens are equal: what the oracle does on an edge; the model predicts both
  cut         the token is min(L, F - p) long, a literal where that is less than 3
  defer       the declared token `tok` at `at`, which the lazy rule would not give if the data went on behind the flush point
where_of() says where a target lies: first (q in the first window), mid (epochs 1-2 of an untrimmed stream) or trim (the segment
of p is encoded from a base > 0).  Data is datagen.text_like with planted targets in the vocabulary of tests/match_cases.py
(a trigram of the target's own, a body with no repeated pair, a guard byte in front, filler behind, padding that fills none of the
targets' buckets); the families blocks and window_per3 say where they use other data.

The model is replay() -- the rules of mi355_deflate_stream_write, _flush and stream_encode restated, each constant with the line that
sets it -- filing(), the hash every position is filed under (stages.h skewed_ab, rewarm_ab), and predict(), match_cases.walk over
those hashes without the holes, no further than the segment's end.  Identity hops are not modelled.  check() holds every claim to
the oracle alone: oracle_binding.Stream with the same script, read back with header_cases.decode.  tests/test_flush_cases.py (CPU) and
tests/test_flush_gpu.py use the cases.
"""
import functools
import random
import zlib

import numpy as np

import datagen
import match_cases as mc
import oracle_binding as ob
from header_cases import LV, decode

WINDOW = 32768             # stages.h WINDOW_SIZE
MAX_MATCH = 258            # stages.h MAX_MATCH
IN_BUF = 2 * WINDOW + 258  # mi355_deflate_stream_write: f + n < 2 * WINDOW_SIZE + MAX_MATCH (input_buffer.rs:9)
TRIM_FROM = 3 * WINDOW     # stream_encode: s->emitted >= 3ull * WINDOW_SIZE
IDENT_EPOCHS = 3           # deflate_host.inc MI355_IDENT_EPOCHS
LINK_TAIL = 4096           # launch_match_tables: n_old = e_first * WINDOW_SIZE + 4096
BLOCK = 31744              # stages.h MAX_BUFFER_LENGTH
SEP = mc.SEP
FAST, DEFAULT, BEST, GREEDY, RLE = LV["fast"], LV["default"], LV["best"], mc.GREEDY, LV["rle"]
LEVEL_NAMES = {FAST: "fast", DEFAULT: "default", BEST: "best", GREEDY: "greedy", RLE: "rle"}
KINDS = ("hole", "skew", "rewarm", "early", "moved")

REPLAY_MUTANTS = ("rewarm_not_moved", "drop_at_base_plus_1", "skew_at_base_minus_1_dropped", "skew_at_base_without_its_byte")
MUTANTS = ("holes_ignored", "skew_ignored", "rewarm_ignored", "cut_ignored", "window_32767", "window_32769") + REPLAY_MUTANTS


# ---- the model -----------------------------------------------------------------------------------------------------------------------
def replay(script, mutant=None):
    """The stream handle's lists over a script, one dict per encode call (every flush, then finish): lo, end = the segment the call
    emits (stream positions), base, n = bytes in the buffer, ends (buffer positions), pts / skw / hol (stream positions), quirk_end
    (buffer position, quirk_reach), e_first and n_old (launch_match_tables)."""
    total = base = emitted = 0
    fps, pts, skw, hol, calls = [], [], [], [], []
    after = False
    drop = 1 if mutant == "drop_at_base_plus_1" else 0

    def ins(v, x):
        if x not in v:
            v.append(x)
            v.sort()

    def rem(v, x):
        if x in v:
            v.remove(x)

    def call(finish):
        lo = base + (drop if base else 0)  # stream_encode: if (f >= s->base)
        s_abs, h_abs = [f for f in skw if f >= lo], [f for f in hol if f >= lo]
        n = total - base
        ends = [f - base for f in fps] + ([n] if finish else [])
        p_abs = list(pts) if base == 0 else []  # stream_encode: s->base == 0 ? &s->rewarm : nullptr
        qe = 0  # quirk_reach
        if s_abs:
            qe = s_abs[-1] - base + 2
        if h_abs:
            qe = max(qe, h_abs[-1] - base + 1)
        n_ep = (n + WINDOW - 1) // WINDOW
        e_first = IDENT_EPOCHS if (p_abs and n >= 2) else 0  # ident = ov.on | ov.m
        if s_abs or h_abs:
            eq = (qe - 1) // WINDOW + 2
            e_first = max(eq, e_first) if eq < n_ep else n_ep
        sorted_path = e_first < n_ep or n_ep == 0
        n_old = 0
        if e_first:
            n_old = e_first * WINDOW + LINK_TAIL
            if n_old > n or not sorted_path:
                n_old = n
        calls.append(dict(flush=len(calls), finish=finish, lo=emitted, end=total, base=base, n=n, ends=ends, pts=p_abs, skw=s_abs,
                          hol=h_abs, quirk_end=qe, e_first=e_first, n_old=n_old, mid_stream=base != 0))

    for op in script:
        if op == "F":  # mi355_deflate_stream_flush, stream_encode
            fps.append(total)
            after = True
            call(False)
            emitted = total
            want = (emitted - WINDOW) // WINDOW * WINDOW if emitted >= TRIM_FROM else 0
            # (a skew point at want - 1 or at want files position `want` late, under d[want - 1]: one more window stays)
            if (want - 1 in skw and mutant != "skew_at_base_minus_1_dropped") or (want in skw and mutant != "skew_at_base_without_its_byte"):
                want -= WINDOW
            if want > base:
                base = want
                fps = [emitted]
                pts = []
                skw = [f for f in skw if f >= base + drop]
                hol = [f for f in hol if f >= base + drop]
            continue
        n, f = op, total  # mi355_deflate_stream_write
        assert n > 0
        if after and f > 2:
            rem(hol, f - 2)
            if n >= 2:
                rem(hol, f - 1)
            if skw and skw[-1] == f - 1:
                skw.pop()
            pprev = max([q for q in fps if q < f], default=0)
            if 0 < pprev <= WINDOW and f - pprev <= 2 and mutant != "rewarm_not_moved":
                rem(pts, pprev)
                ins(pts, f - 2)
            if n == 1:
                ins(hol, f - 1)
                ins(skw, f)
            if f <= WINDOW and f + n < IN_BUF:
                ins(pts, f)
        elif after and f > 0:
            hol = list(range(f))
            pts = [f]
        after = False
        total += n
    call(True)
    return calls


def filing(data, call, mutant=None):
    """the hash every position is filed under in that encode call (stages.h position_hash: skewed_ab, then rewarm_ab)"""
    fh = mc._hashes(data).astype(np.int64).copy()
    skw = [] if mutant == "skew_ignored" else call["skw"]
    pts = [] if mutant == "rewarm_ignored" else call["pts"]
    for p in sorted({p for F in skw for p in (F, F + 1)} | {p for P in pts for p in (P, P + 1)}):
        if p + 2 >= len(data):
            continue
        a, b = data[p], data[p + 1]
        if p in skw:  # skewed_ab
            # (the mutant: the buffer begins at the skew point, and a zero stands for the byte in front of it)
            a, b = (0 if mutant == "skew_at_base_without_its_byte" and p == call["base"] else data[p - 1]), a
        elif p - 1 in skw:
            a = data[p - 1]
        if p <= WINDOW + 1:  # rewarm_ab
            if p in pts:
                a, b = data[0], data[1]
            elif p - 1 in pts:
                a = data[1]
        fh[p] = mc.hash3(a, b, data[p + 2])
    return fh


def call_of(calls, p):
    return next(s for s in calls if s["end"] > p)


def predict(c, t, script=None, mutant=None):
    """((position, token), encode call) the model gives for a target under a script (the case's own by default)"""
    data, opts, p = c["data"], c["opts"], t["p"]
    calls = replay(c["script"] if script is None else script, mutant if mutant in REPLAY_MUTANTS else None)
    s = call_of(calls, p)
    end = len(data) if mutant == "cut_ignored" else s["end"]
    if opts == RLE:  # the run of the byte in front, no further than 258 and the end of the data
        ln = 0
        while p and ln < min(MAX_MATCH, end - p) and data[p + ln] == data[p - 1]:
            ln += 1
        return ((p, ("ld", ln, 1)) if ln >= 3 else (p, ("lit", data[p]))), s
    kw = {"window_32767": dict(window=32767), "window_32769": dict(window=32769)}.get(mutant, {})
    holes = set() if mutant == "holes_ignored" else set(s["hol"])
    kw.update(filing=filing(data, s, mutant), holes=holes, end=end)
    prev = (0, 0)
    if t.get("pre"):  # a match can begin at p - 1: the walk at p starts from it (with a quarter of the budget from 32 bytes on)
        prev = mc.walk(data, p - 1, opts[0], **kw)[0]
        if prev[0] == 3 and prev[1] > 8192:
            prev = (0, 0)
    return mc.predict(data, dict(p=p, prev=prev), opts, **kw), s


def model_lists(c, p):
    """the model's lists for the call that emits position p, for the diff helper"""
    s = call_of(replay(c["script"]), p)
    return "flush %d%s [%d, %d) base %d ends %s pts %s skw %s hol %s quirk_end %d e_first %d n_old %d" % (
        s["flush"], " (finish)" if s["finish"] else "", s["lo"], s["end"], s["base"], _short(s["ends"]), _short(s["pts"]),
        _short(s["skw"]), _short(s["hol"]), s["quirk_end"], s["e_first"], s["n_old"])


def _short(v):
    return str(v) if len(v) <= 8 else "[%s, ... %d in all]" % (", ".join(map(str, v[:6])), len(v))


# ---- the oracle ------------------------------------------------------------------------------------------------------------------------
def plain_of(script):
    out, acc = [], 0
    for op in script:
        if op == "F":
            out += ([acc] if acc else []) + ["F"]
            acc = 0
        else:
            acc += op
    return out + ([acc] if acc else [])


def run_oracle(data, opts, script, wrapper=0, header=None):
    """-> (the finished stream, [length of the output after every flush], [checksum() after every flush])"""
    ref = ob.Stream(ob.make_opts(*opts, wrapper))
    if header is not None:
        ref.gzip_header(header)
    p, marks, sums = 0, [], []
    for op in script:
        if op == "F":
            ref.flush()
            marks.append(len(ref.output()))
            sums.append(ref.checksum())
        else:
            ref.write_all(data[p:p + op])
            p += op
    assert p == len(data), (p, len(data))
    out = ref.finish()
    return out, marks, sums


_REF = {}


def oracle(c, wrapper=0):
    key = (c["name"], wrapper)
    if key not in _REF:
        _REF[key] = run_oracle(c["data"], c["opts"], c["script"], wrapper)
    return _REF[key]


def tokens_at(stream):
    """({position: token}, [tokens of every flush segment]) of a raw stream; a segment ends at an empty stored block"""
    out, segs, pos, k = {}, [], 0, 0
    for blk in decode(stream):
        if blk.get("stored") is not None:
            if blk["stored"] == 0 and not blk["bfinal"]:
                segs.append(k)
                k = 0
            else:
                out[pos] = ("stored", blk["stored"])
                pos += blk["stored"]
                k += 1
            continue
        for ln, v in blk["toks"]:
            out[pos] = ("lit", v) if ln == 0 else ("ld", ln, v)
            pos += ln or 1
            k += 1
    segs.append(k)
    return out, segs


def flush_diff(got, want, c, flush=None):
    """Where two streams of a case part: the flush index, the first differing token, its input position and epoch, the target it
    belongs to, and the model's lists for the call that emits that position.  None for streams that read the same."""
    if got == want:
        return None
    fg, fw = mc._flat(got), mc._flat(want)
    pos, i, seg = 0, 0, 0
    for i, (g, w) in enumerate(zip(fg, fw)):
        if g != w:
            break
        if w[1] == ("stored", 0):
            seg += 1
        pos += w[1][1] if w[1][0] in ("ld", "stored") else 1
    else:
        i = min(len(fg), len(fw))
        if len(fg) == len(fw):
            return "%s: the same tokens in other bytes (%d bytes, expected %d): a header or a block boundary differs" % (c["name"], len(got), len(want))
    g = fg[i][1] if i < len(fg) else None
    w = fw[i][1] if i < len(fw) else None
    msg = "%s%s: flush segment %d, token %d at input position %d (epoch %d, offset %d): got %s, expected %s" % (
        c["name"], "" if flush is None else " after flush %d" % flush, seg, i, pos, pos // WINDOW, pos % WINDOW, g, w)
    if pos < len(c["data"]):
        msg += "; model: " + model_lists(c, pos)
    for t in c["targets"]:
        if t["p"] - 1 <= pos <= t["p"] + 1:
            msg += "; target at %d (%s, %s, affected position %s), the model's token %s" % (t["p"], t["kind"], t["claim"], t.get("q"), predict(c, t)[0][1])
            break
    return msg


# ---- building blocks -------------------------------------------------------------------------------------------------------------------
class _B(mc._Build):
    """match_cases._Build with placements at exact positions and one long text as padding, taken piece by piece"""

    def __init__(self, seed, n):
        super().__init__(seed)
        self.long = datagen.text_like(n + 64, seed)[:n]
        self.used |= set(np.unique(mc._hashes(self.long)).tolist())
        self.cur = 0
        self.plan = []
        self.trail = {}  # the byte behind every copy of a text: the byte behind its target is another one

    def to(self, offset):
        n = offset - len(self.o)
        assert n >= 0, "%d bytes too late for %d" % (-n, offset)
        if n < SEP + 3:
            self.fill(n)
            return
        t = self.long[self.cur:self.cur + n - SEP]
        self.cur += len(t)
        assert len(t) == n - SEP
        self.fill(SEP, t)
        j = len(self.o)
        self.o += t
        self.used |= {mc.hash3(*self.o[i - 2:i + 1]) for i in (j, j + 1)}

    def raw_at(self, q, bs):
        """those bytes at q exactly, a filler byte behind them"""
        self.plan.append((q - SEP, lambda: self._raw(q, bs)))

    def _raw(self, q, bs):
        if q < SEP:  # (right behind the stream's start)
            self.fill(q, bs)
            self.push(bs)
            self.trail.setdefault(bytes(bs[:3]), set()).add(self.pick(mc.FILL))
            return
        self.to(q - SEP)
        assert self.put(dict(tri=(0, 0, 0), text=b""), ("raw", bytes(bs))) == q
        self.trail.setdefault(bytes(bs[:3]), set()).add(self.o[-1])

    def copy_at(self, tg, q, ln):
        self.raw_at(q, tg["text"][:ln])

    def target_at(self, tg, t, ln, end=False, **claims):
        def place():
            self.to(t - SEP - 1 - len(tg["pre"]))
            assert self.put_target(tg, ln, at=t, end=True) == t
            if not end:
                self.pick([x for x in mc.FILL if x not in self.trail.get(tg["text"][:3], ())])
        self.plan.append((t - SEP - 1 - len(tg["pre"]), place))
        self.targets.append(dict(p=t, **claims))

    def lead(self, bs):
        """the stream's first bytes"""
        self.plan.append((-1, lambda: (self.push(bs), self.trail.setdefault(bytes(bs[:3]), set()).add(self.pick(mc.FILL)))))

    def build(self, n):
        for _, fn in sorted(self.plan, key=lambda x: x[0]):
            fn()
        self.to(n)
        assert len(self.o) == n
        assert not (set(np.unique(mc._hashes(self.long[:self.cur])).tolist()) & self.res), "padding in a target's bucket"
        return bytes(self.o)

    def flush_case(self, name, family, opts, head, n, plain=None, **extra):
        data = self.build(n)
        script = list(head) + [n - sum(x for x in head if x != "F")]
        assert script[-1] > 0
        return dict(name=name, family=family, data=data, opts=opts, script=script, plain=plain_of(script) if plain is None else plain,
                    targets=sorted(self.targets, key=lambda t: t["p"]), claims=dict(extra))


def no_repeat(n, seed, alphabet=64):
    """n bytes over `alphabet` values in which no three bytes occur twice: every token of every level is a literal"""
    r, seen, o = random.Random(seed), set(), bytearray()
    while len(o) < n:
        x = 0x40 + r.randrange(alphabet)
        if len(o) >= 2:
            k = (o[-2], o[-1], x)
            if k in seen:
                continue
            seen.add(k)
        o.append(x)
    return bytes(o)


# ---- filing: the five quirk kinds, each with a target whose only near candidate is the affected position -----------------------------
TL = 15   # a target's length
FAR = 3000  # the second, farther copy lies that far in front of the affected position
DIST = 5000  # the target behind the affected position


def _one(g, q, kind, claim, far=True, dist=DIST, **more):
    """a target text at q, a farther copy in front of it, the target `dist` behind q"""
    tg = g.new_target(TL + 1)
    if far and q - FAR > 64:
        g.copy_at(tg, q - FAR, TL)
    if q == 0:
        g.lead(tg["text"][:TL])
    else:
        g.copy_at(tg, q, TL)
    g.target_at(tg, q + dist, TL, kind=kind, claim=claim, q=q, **more)
    return tg


def _ghost(g, P, form, r, at, kind, claim="changes", **more):
    """a target whose own hash is the foreign hash position P is filed under: form (a, b, x, c) -> bytes at P - 1 (a skew at P),
    form (x, y, c) -> bytes at P behind a stream that begins a, b (a re-warm at P); its real copy at r, the ghost target at `at`"""
    tg = g.new_target(TL + 1)
    a, b, c = tg["tri"]

    def place():
        if form == "skew":
            g.to(P - 1 - SEP)
            g.fill(SEP, [a, b])
            assert len(g.o) == P - 1
            g.push([a, b])
            g.pick(mc.FILL, [c])
            g.push([c])
        else:
            g.to(P - SEP)
            g.fill(SEP)
            g.pick(mc.FILL)
            g.pick(mc.FILL, [c])
            assert len(g.o) == P + 2
            g.push([c])
        g.pick(mc.FILL)
    if P == 2:  # a flush after the first two bytes: a, b, two filler bytes, c
        g.plan.append((-1, lambda: (g.push([a, b]), g.pick(mc.FILL), g.pick(mc.FILL, [c]), g.push([c]), g.pick(mc.FILL))))
    else:
        g.plan.append((P - 1 - SEP, place))
        if form != "skew":
            g.lead([a, b])
    g.copy_at(tg, r, TL)
    g.target_at(tg, at, TL, kind=kind, claim=claim, q=P, ghost=True, **more)


def _filing_cases(t):
    def add(name, fn):
        t["filing_" + name] = lambda: fn("filing_" + name)

    # a one-byte write after a flush at F: a hole at F - 1, F and F + 1 filed a byte late
    for F in (5000, 32767, 32768, 32769, 50000, 65535, 65536, 98303):
        for kind, dq in (("hole", -1), ("skew", 0), ("skew", 1)):
            def fn(name, F=F, kind=kind, dq=dq):
                n = max(F + DIST + 3000, IN_BUF + 1000 if F <= WINDOW else 0)  # (the plain write fills the input buffer)
                g = _B(1000 + F % 997 + dq, n + 64)
                # (inside the first window the one-byte write re-warms the hash at F as well, and the re-warm wins: rewarm_ab)
                _one(g, F + dq, kind, "changes", **({"covered_by": "rewarm"} if kind == "skew" and F <= WINDOW else {}))
                return g.flush_case(name, "filing", DEFAULT, [F, "F", 1], n)
            add("%s_F%d_q%d" % (kind, F, F + dq), fn)
    for F in (40000, 65535, 65536):
        def fn(name, F=F):
            g = _B(1100 + F % 997, F + DIST + 4000)
            _ghost(g, F, "skew", F - 2000, F + 3000, "skew")
            return g.flush_case(name, "filing", FAST, [F, "F", 1], F + DIST + 3000)
        add("skew_ghost_F%d" % F, fn)
    # a two-byte write after the flush changes nothing
    def fn(name):
        g = _B(1150, 20000 + DIST + 4000 + IN_BUF)
        _one(g, 19999, "hole", "unchanged")
        return g.flush_case(name, "filing", DEFAULT, [20000, "F", 2], 20000 + IN_BUF + 100)
    add("two_byte_write_F20000", fn)

    # a small write after a flush at F <= 32768: the re-warm at F
    N = IN_BUF + 5000
    for F, w, dq, claim in ((20000, 3, 0, "changes"), (20000, 50, 1, "changes"), (32767, 3, 0, "changes"), (32768, 3, 0, "changes"),
                            (32768, 50, 1, "changes"), (32769, 3, 0, "unchanged"), (32769, 50, 1, "unchanged"), (3, 3, 0, "changes"),
                            (30000, 65793 - 30000, 0, "changes"), (30000, 65794 - 30000, 0, "unchanged")):
        def fn(name, F=F, w=w, dq=dq, claim=claim):
            g = _B(1200 + F % 997 + w % 13, N + 64)
            _one(g, F + dq, "rewarm", claim)
            return g.flush_case(name, "filing", DEFAULT, [F, "F", w], N, f_plus_n=F + w)
        add("rewarm_F%d_w%d_q%d%s" % (F, w, F + dq, "_fn%d" % (F + w) if w > 100 else ""), fn)
    for F in (20000, 32768):
        def fn(name, F=F):
            g = _B(1300 + F % 997, N + 64)
            _ghost(g, F, "rewarm", F - 2000, F + 3000, "rewarm")
            return g.flush_case(name, "filing", FAST, [F, "F", 3], N)
        add("rewarm_ghost_F%d" % F, fn)

    # a flush after the stream's first one or two bytes: every earlier position a hole, the re-warm at F
    for F, q, kind in ((1, 0, "hole"), (2, 0, "hole"), (2, 1, "hole"), (1, 1, "rewarm"), (1, 2, "rewarm"), (2, 2, "rewarm"), (2, 3, "rewarm")):
        def fn(name, F=F, q=q):
            g = _B(1400 + 10 * F + q, N + 64)
            _one(g, q, "early", "changes", far=False)
            return g.flush_case(name, "filing", DEFAULT, [F, "F"], N, plain=[N])
        add("early_F%d_%s_q%d" % (F, kind, q), fn)
    def fn(name):  # (nothing lies in front of an early flush: its ghost cannot be the nearer candidate, and the token stays)
        g = _B(1450, N + 64)
        _ghost(g, 2, "rewarm", 1000, 4000, "early", claim="unchanged")
        return g.flush_case(name, "filing", FAST, [2, "F"], N, plain=[N])
    add("early_F2_ghost", fn)

    # two flushes one or two bytes apart inside the first window: the re-warm moves to F' - 2
    for F, gap in ((20000, 1), (20000, 2), (32767, 1), (32766, 2)):
        def fn(name, F=F, gap=gap):
            g = _B(1500 + F % 997 + gap, N + 64)
            _one(g, F + gap - 2, "moved", "changes", gap=gap)
            return g.flush_case(name, "filing", DEFAULT, [F, "F", gap, "F"], N, plain=[F, "F", N - F])
        add("moved_F%d_gap%d" % (F, gap), fn)
    def fn(name):
        g = _B(1550, N + 64)
        _ghost(g, 19999, "rewarm", 18000, 23000, "moved", gap=1)
        return g.flush_case(name, "filing", FAST, [20000, "F", 1, "F"], N, plain=[20000, "F", N - 20000])
    add("moved_ghost_F20000_gap1", fn)


# ---- cut: a match of 258 or more, or a run, across a flush point ------------------------------------------------------------------------
CUT_K = (0, 1, 2, 3, 4, 15, 16, 17, 257, 258, 259)
MODS = (16, 256, 1024, 4096, 32768)


def _cut_points(part):
    """eleven flush points, ascending: the 15 residues 0, +1, -1 mod 16 .. 32768 dealt round over the parts, each an odd multiple of
    its modulus where that fits (so that it is no multiple of the next one)"""
    res = [(m, r) for m in MODS for r in (0, 1, -1)]
    pts, at = [], 2000
    for i in range(len(CUT_K)):
        m, r = res[(part * len(CUT_K) + i) % len(res)]
        base = m if m == WINDOW else ((at + 1500) // (2 * m) * 2 * m + m)
        while base + r < at + 1500:
            base += m if m == WINDOW else 2 * m
        pts.append((base + r, m, r))
        at = base + r
    return pts


def _cut(name, opts, part):
    pts = _cut_points(part)
    n = pts[-1][0] + 3000
    g = _B(2000 + part, n + 64)
    head, at = [], 0
    for (F, m, r), k in zip(pts, CUT_K):
        run = opts == RLE
        tg = g.new_target(301, run=run)
        p = F - k
        if run:  # the target is the second byte of the run
            g.target_at(tg, p - 1, 300, kind="cut", claim="cut", k=k, L=MAX_MATCH, mod=(m, r), q=None)
            g.targets[-1]["p"] = p
        else:
            g.copy_at(tg, p - 700, 300)
            g.target_at(tg, p, 300, kind="cut", claim="cut", k=k, L=MAX_MATCH, mod=(m, r), q=None)
        head += [F - at, "F"]
        at = F
    return g.flush_case(name, "cut", opts, head, n)


def _cut_defer(name):
    """The lazy rule across a flush point.  A match of 4 begins at p - 1 and one of 10 at p: with all the data the parse defers.
    F = p + 3: the better match starts at F - 3, has a hash byte and 3 bytes left, and the match of 4 stays.  F = p + 2: it starts
    at F - 2 and has no hash byte; the match at p - 1 has 3 bytes left and stays as that."""
    g = _B(2100, 12000)
    head, at = [], 0
    for p, k, label in ((3000, 3, "F-3"), (6000, 2, "F-2")):
        tg = g.new_target(21, pre=True)
        g.raw_at(p - 900, tg["pre"] + tg["text"][:3])
        g.raw_at(p - 500, tg["text"][:10])
        g.target_at(tg, p, 20, kind="defer", claim="defer", pre=True, at=p - 1, tok=("ld", min(4, k + 1), 899), better_at=label, q=None)
        head += [p + k - at, "F"]
        at = p + k
    return g.flush_case(name, "cut", DEFAULT, head, 10000)


def _cut_best(name):
    """Best, a match of 40 at p - 1 and one of 60 at p, which the walk looks for with a quarter of the budget (the table Mq):
    the flush at p + 43 leaves it 43 bytes, still more than 40"""
    g = _B(2200, 9000)
    p, k = 4000, 43
    tg = g.new_target(71, pre=True)
    g.raw_at(p - 1500, tg["pre"] + tg["text"][:39])
    g.raw_at(p - 700, tg["text"][:60])
    g.target_at(tg, p, 70, kind="quarter", claim="defer", pre=True, at=p, tok=("ld", k, 700), q=None)
    return g.flush_case(name, "cut", BEST, [p + k, "F"], 8000)


def _cut_cases(t):
    t["cut_default_defer_F_minus_3_F_minus_2"] = lambda: _cut_defer("cut_default_defer_F_minus_3_F_minus_2")
    t["cut_best_behind_a_match_of_40_k43"] = lambda: _cut_best("cut_best_behind_a_match_of_40_k43")
    for part, opts in enumerate((DEFAULT, FAST, BEST, GREEDY, RLE)):
        mods = sorted({m for _, m, _ in _cut_points(part)})  # (each residue 0, +1, -1 of them; all fifteen over the five cases)
        name = "cut_%s_k0_1_2_3_4_15_16_17_257_258_259_F_on_%s" % (LEVEL_NAMES[opts], "_".join("m%d" % m for m in mods))
        t[name] = lambda name=name, opts=opts, part=part: _cut(name, opts, part)


# ---- window: the affected position at the window's edge of its target; inputs that end around the end of the link path ----------------
def _window_cases(t):
    for q in (65535, 65536, 65537):
        for dist in (32767, 32768, 32769):
            for kind, F in (("hole", q + 1), ("skew", q)):
                def fn(name, q=q, dist=dist, kind=kind, F=F):
                    n = 4 * WINDOW + 258  # e_first = 4 of five epochs: the targets lie in the link path's last epochs, k_sort and
                    g = _B(3000 + q % 7 + dist % 5 + len(kind), n + 64)  # k_match3 take the fifth, with a target of its own
                    _one(g, q, kind, "changes" if dist <= WINDOW else "unchanged", far=False, dist=dist, qmod=q % WINDOW)
                    _one(g, q + 200, "control", "unchanged", far=False, dist=dist)  # (a position the pattern leaves alone)
                    tg = g.new_target(TL + 1)
                    g.copy_at(tg, n - 3000, TL)
                    g.target_at(tg, n - 30, TL, kind="sorted", claim="cut", k=None, L=TL, q=None)
                    return g.flush_case(name, "window", DEFAULT, [F, "F", 1], n, e_first=4, n_old=n)
                t["window_%s_q%d_mod%d_dist%d" % (kind, q, q % WINDOW, dist)] = lambda fn=fn, n="window_%s_q%d_mod%d_dist%d" % (kind, q, q % WINDOW, dist): fn(n)
    # the length of the input around the end of the link path: a hole at 39999 gives e_first = 3
    for dn, label in ((-1, "e_first_x_32768_minus_1"), (1, "e_first_x_32768_plus_1"), (4095, "e_first_x_32768_plus_4095"),
                      (4096, "e_first_x_32768_plus_4096"), (4097, "e_first_x_32768_plus_4097_match_of_258_below_e_first_x_32768")):
        def fn(name, dn=dn):
            n = 3 * WINDOW + dn
            g = _B(3100 + dn % 11, n + 64)
            _one(g, 39999, "hole", "changes")
            tg = g.new_target(301)  # a match of 258 that starts in the last 258 positions below e_first * 32768
            p = 3 * WINDOW - 100
            g.copy_at(tg, p - 2000, 300)
            g.target_at(tg, p, min(300, n - p), end=n - p <= 300, kind="seam258", claim="cut", k=None, L=min(MAX_MATCH, n - p), q=None)
            if dn >= 4095:  # and one in the last positions of the input
                tg = g.new_target(TL + 1)
                g.copy_at(tg, n - 3000, TL)
                g.target_at(tg, n - 30, TL, kind="tail", claim="cut", k=None, L=TL, q=None)
            return g.flush_case(name, "window", DEFAULT, [40000, "F", 1], n, e_first=3, n_old=min(3 * WINDOW + LINK_TAIL, n))
        t["window_n_" + label] = lambda fn=fn, n="window_n_" + label: fn(n)
    # the one periodic pattern of test_tiny_flush_gaps (period 3, a one-byte write after the flush): a whole-stream comparison only
    for F in (65535, 65536):
        def fn(name, F=F):
            n = 4 * WINDOW + 258
            data = (datagen.rng_bytes(3, 1) * n)[:n]
            script = [F, "F", 1, n - F - 1]
            return dict(name=name, family="window", data=data, opts=FAST, script=script, plain=plain_of(script), targets=[],
                        claims=dict(whole_stream=True))
        t["window_per3_whole_stream_F%d" % F] = lambda fn=fn, n="window_per3_whole_stream_F%d" % F: fn(n)


# ---- trim: the flush that lets go of history, and what lies at the new base -----------------------------------------------------------
def _q_at(E, q):
    """what the candidate q is to the flush that reaches E emitted bytes"""
    base = (E - WINDOW) // WINDOW * WINDOW if E >= TRIM_FROM else 0
    return [w for x, w in ((base, "base"), (base + 1, "base+1"), (E - WINDOW, "emitted-32768")) if x == q and base]


def _own_hash_target(g, a, b, tlen):
    """a target that begins a, b: a third byte whose bucket is empty, a body with no repeated pair"""
    for c in range(0x80, 0xA0):
        h = mc.hash3(a, b, c)
        if h in g.used or h in g.res:
            continue
        text, pairs = [a, b, c], {(a, b), (b, c)}
        g.res.add(h)
        while len(text) < tlen:
            x = next((x for x in mc.BODY if (text[-1], x) not in pairs and g.ok((text[-2], text[-1], x))), None)
            if x is None:
                break
            pairs.add((text[-1], x))
            text.append(x)
        if len(text) < tlen:
            g.res.discard(h)
            continue
        g.used |= {mc.hash3(*text[i:i + 3]) for i in range(len(text) - 2)}
        return dict(tri=(a, b, c), g=g.r.choice(mc.GUARD), text=bytes(text), run=False, pre=b"")
    raise RuntimeError("no free trigram")


def _trim_cases(t):
    def add(name, fn):
        t["trim_" + name] = lambda: fn("trim_" + name)

    # the flush that reaches E emitted bytes, a target right behind it whose candidate lies at the far end of its window
    for E, q, tp in ((98303, 65536, 98303), (98304, 65536, 98304), (98304, 65537, 98305), (98305, 65537, 98305), (98305, 65540, 98308),
                     (131071, 98304, 131071), (131072, 98304, 131072), (131072, 98305, 131073)):
        def fn(name, E=E, q=q, tp=tp):
            n = E + 6000
            g = _B(4000 + E % 13 + q % 7, n + 64)
            tg = g.new_target(TL + 1)
            g.copy_at(tg, q, TL)
            g.target_at(tg, tp, TL, kind="edge", claim="cut", k=None, L=TL, q=q)
            base = (E - WINDOW) // WINDOW * WINDOW if E >= TRIM_FROM else 0
            return g.flush_case(name, "trim", DEFAULT, [E, "F"], n, emitted=E, base=base, q_at=_q_at(E, q))
        add("emitted%d_q%d_t%d%s" % (E, q, tp, "".join("_q_at_" + w.replace("+", "_plus_").replace("-", "_minus_") for w in _q_at(E, q))), fn)
    # a hole and a skew at 65536 and at 65535, where the second flush, at 98304, would trim to.  A hole at 65536 stays in the lists,
    # one at 65535 is out of every later window.  A skew at either files 65536 late, under d[65535]: one more window stays.
    for kind, F, q, claim in (("hole", 65537, 65536, "changes"), ("skew", 65536, 65536, "changes"), ("hole", 65536, 65535, "unchanged"),
                              ("skew", 65535, 65536, "changes")):
        def fn(name, kind=kind, F=F, q=q, claim=claim):
            n = 98304 + 6000
            g = _B(4100 + F % 11 + len(kind), n + 64)
            base = 65536 if F == 65537 else 32768  # (the one-byte write behind a flush at 65535 or 65536 leaves a skew point there)
            _one(g, q, kind, claim, far=False, dist=98304 - q, base=base)
            return g.flush_case(name, "trim", DEFAULT, [F, "F", 1, 98304 - F - 1, "F"], n, base=base)
        add("%s_at_base%s_F%d_q%d" % (kind, "" if (F if kind == "skew" else F - 1) == 65536 else "_minus_1", F, q), fn)
    # the skew at 65536 with d[65535..65537] = 0x82, 0x83, 0xA3: hash3(0x82, 0x83, c) == hash3(0x83, 0xA3, c), so the late filing of
    # 65536 is the filing under its own three bytes, and the copy at 98304 finds it -- if the byte at 65535 is still there
    def fn(name):
        n = 98304 + 6000
        g = _B(4150, n + 64)
        tg = _own_hash_target(g, 0x83, 0xA3, TL + 1)
        g.raw_at(65535, bytes([0x82]) + tg["text"][:TL])
        g.target_at(tg, 98304, TL, kind="skew", claim="unchanged", q=65536, ghost=True, base=32768)
        assert mc.hash3(0x82, 0x83, tg["tri"][2]) == mc.hash3(*tg["tri"])
        return g.flush_case(name, "trim", DEFAULT, [65536, "F", 1, 32767, "F"], n, base=32768)
    add("skew_at_base_own_hash_F65536_q65536", fn)
    # a hole and a skew behind the trim, inside the kept history
    for kind, dq in (("hole", -1), ("skew", 0)):
        def fn(name, kind=kind, dq=dq):
            F = 110000
            n = F + DIST + 3000
            g = _B(4200 + dq, n + 64)
            _one(g, F + dq, kind, "changes")
            return g.flush_case(name, "trim", DEFAULT, [100000, "F", F - 100000, "F", 1], n, base=65536)
        add("%s_behind_F110000" % kind, fn)
    # a literal-only stretch behind base: the call's first block fills inside the buffer's first 32768 bytes, and Q1 must not fire
    def fn(name):
        n = 98304 + 30000
        g = _B(4300, n + 64)
        _one(g, 98304 + 5000, "q1", "unchanged", far=False)
        data = bytearray(g.build(n))
        data[65536 + 8:98304 - 8] = no_repeat(32768 - 16, 4301)
        script = [98304, "F", 20000, "F", n - 118304]
        return dict(name=name, family="trim", data=bytes(data), opts=DEFAULT, script=script, plain=plain_of(script), targets=g.targets,
                    claims=dict(q1_zero=True, base=65536))
    add("literal_stretch_behind_base_no_q1", fn)


# ---- blocks: flush segments of 0, 1, 31743, 31744, 31745 and 2 x 31744 tokens (literal-only data: a token is a byte) -----------------
def _blocks_cases(t):
    def lit(name, segs, seed):
        n = sum(segs) + 1000
        script = []
        for s in segs:
            script += ([s] if s else []) + ["F"]
        script.append(1000)
        return dict(name=name, family="blocks", data=no_repeat(n, seed), opts=DEFAULT, script=script, plain=plain_of(script), targets=[],
                    claims=dict(seg_tokens=list(segs) + [1000]))
    t["blocks_seg_1_0_31743_31744_31745_tokens_flush_behind_a_full_block"] = lambda: lit(
        "blocks_seg_1_0_31743_31744_31745_tokens_flush_behind_a_full_block", (1, 0, 31743, 31744, 31745), 5000)
    t["blocks_seg_2x31744_tokens"] = lambda: lit("blocks_seg_2x31744_tokens", (2 * BLOCK, 0, 1), 5001)


# ---- many: flush points by the hundred inside two windows ----------------------------------------------------------------------------
MANY = (63, 64, 65, 256, 257, 1025)


def _many_cases(t):
    for opts in (DEFAULT, RLE):
        for m in MANY:
            def fn(name, opts=opts, m=m):
                n = 70000
                w = 64 if m * 64 < 2 * WINDOW else 63
                data = datagen.text_like(n + 64, 6000 + m)[:n]
                if opts == RLE:  # runs for k_rle to cut: every 100th byte begins a run of 3 to 70
                    d, r = bytearray(data), random.Random(m)
                    for i in range(50, n - 100, 100):
                        d[i:i + 3 + (i // 100) % 68] = bytes([r.randrange(256)]) * (3 + (i // 100) % 68)
                    data = bytes(d)
                script, left = [], n
                for _ in range(m):
                    script += [w, "F"]
                    left -= w
                while left > 0:
                    script.append(min(64, left))
                    left -= script[-1]
                assert m * w < 2 * WINDOW and len(data) == n
                return dict(name=name, family="many", data=data, opts=opts, script=script, plain=plain_of(script), targets=[],
                            claims=dict(flushes=m))
            name = "many_%d_flushes_%s" % (m, LEVEL_NAMES[opts])
            t[name] = lambda fn=fn, name=name: fn(name)


def _table_of_cases():
    t = {}
    _cut_cases(t)
    _filing_cases(t)
    _window_cases(t)
    _trim_cases(t)
    _blocks_cases(t)
    _many_cases(t)
    return t


_CASES = _table_of_cases()
FAMILIES = ("cut", "filing", "window", "trim", "blocks", "many")


def names():
    return list(_CASES)


def family_of(name):
    return name.split("_")[0]


def opts_of(name):
    """the options of a case, without building it"""
    if name.startswith(("cut_", "many_")):
        return {v: k for k, v in LEVEL_NAMES.items()}[name.split("_")[1] if name.startswith("cut_") else name.rsplit("_", 1)[1]]
    return FAST if ("ghost" in name or "per3" in name) else DEFAULT


@functools.lru_cache(maxsize=None)
def case(name):
    c = _CASES[name]()
    assert c["name"] == name and c["family"] == family_of(name) and c["opts"] == opts_of(name), name
    return c


def cases():
    return [case(n) for n in names()]


# ---- preconditions, on the oracle alone ----------------------------------------------------------------------------------------------
def where_of(c, t):
    s = call_of(replay(c["script"]), t["p"])
    if s["base"]:
        return "trim"
    return "first" if t["q"] < WINDOW else "mid" if t["q"] < 3 * WINDOW else "late"


def check(c):
    """assert a case on the oracle: its limits, every target's claim, the claims of the case"""
    data, opts, script, fam = c["data"], c["opts"], c["script"], c["family"]
    n, flushes = len(data), script.count("F")
    assert sum(op for op in script if op != "F") == n and script[-1] != "F"
    assert n <= (70000 if fam == "many" else 7 * WINDOW if fam == "trim" else 4 * WINDOW + 258), (c["name"], n)
    assert fam == "many" or flushes <= 12, (c["name"], flushes)
    ref, marks, _ = oracle(c)
    assert zlib.decompress(ref, -15) == data and len(marks) == flushes
    toks, segs = tokens_at(ref)
    assert len(segs) == flushes + 1
    ptoks = None
    for t in c["targets"]:
        what = "%s, target at %d (%s, %s)" % (c["name"], t["p"], t["kind"], t["claim"])
        p = t["p"]
        (at, tok), s = predict(c, t)
        got = toks.get(at)
        assert got == tok, "%s: the oracle has %s at %d, the model %s; %s" % (what, got, at, tok, model_lists(c, p))
        if t["claim"] == "defer":  # the declared token, and another one where the data does not end at the flush point
            assert (at, tok) == (t["at"], t["tok"]) and predict(c, t, mutant="cut_ignored")[0] != (at, tok), (what, at, tok)
            continue
        assert at == p, what
        if t["claim"] == "cut":
            if t["k"] == 0:  # the flush point is the target itself: the first position of the next segment, whose token the model
                assert s["lo"] == p, what  # gives (a literal where the write behind the flush re-warms the hash there)
                continue
            ln = min(t["L"], s["end"] - p)
            assert not t["k"] or s["end"] - p == t["k"], what
            assert (got[0] == "ld" and got[1] == ln) if ln >= 3 else got == ("lit", data[p]), "%s: the oracle has %s, %d bytes are left" % (what, got, s["end"] - p)
            if t["k"] is not None and ln < t["L"]:  # the data goes on equal behind the flush point
                d = got[2] if got[0] == "ld" else (1 if opts == RLE else 700)
                assert data[p:p + ln + 1] == data[p - d:p - d + ln + 1], what
            continue
        if ptoks is None:
            ptoks = tokens_at(run_oracle(data, opts, c["plain"])[0])[0]
        (pat, ptok), _ = predict(c, t, c["plain"])
        assert (pat, ptoks.get(p)) == (p, ptok), "%s: with plain writes the oracle has %s, the model %s" % (what, ptoks.get(p), ptok)
        if t["claim"] == "changes":
            assert got != ptoks.get(p), "%s: the oracle has %s either way" % (what, got)
        else:
            assert t["claim"] == "unchanged" and got == ptoks.get(p), "%s: the oracle has %s, with plain writes %s" % (what, got, ptoks.get(p))
        if "base" in t:
            assert s["base"] == t["base"], what
    cl = c["claims"]
    calls = replay(script)
    if "seg_tokens" in cl:
        assert segs == cl["seg_tokens"], (c["name"], segs)
    if "flushes" in cl:
        assert flushes == cl["flushes"] and all(op == "F" or op <= 64 for op in script) and calls[flushes - 1]["end"] < 2 * WINDOW
    if "e_first" in cl:
        assert (calls[-1]["e_first"], calls[-1]["n_old"]) == (min(cl["e_first"], (n + WINDOW - 1) // WINDOW), cl["n_old"]), (c["name"], calls[-1])
    if "base" in cl:
        assert calls[-1]["base"] == cl["base"], (c["name"], calls[-1]["base"])
    if "f_plus_n" in cl:
        assert (cl["f_plus_n"] < IN_BUF) == bool(calls[-1]["pts"]) or script[0] > WINDOW, c["name"]
    if cl.get("q1_zero"):  # the call behind the trim: its first block fills inside the first 32768 bytes of its buffer
        s = calls[1]
        k = sum(1 for pos in toks if s["base"] <= pos < s["base"] + WINDOW - 8)
        assert s["base"] and s["mid_stream"] and k >= BLOCK + 8, (c["name"], k)
    return toks


def covered():
    """{(kind, where)} of the targets that claim `changes`, and every case name"""
    out = set()
    for c in cases():
        for t in c["targets"]:
            if t["claim"] == "changes" and t["kind"] in KINDS:
                out.add((t["kind"], where_of(c, t)))
    return out
