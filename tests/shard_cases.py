"""Inputs and cuts that drive the per-rank phases of the sharded (P1) encode -- mi355_shard_begin / _spec / _exit_table / _emit /
_blocks_ex / _pack with k_cover, k_shard_bounds, k_shard_costs and k_seg_exit / k_level_up / k_level_down / k_emit<0> over a range,
and mi355_plan_blocks -- onto the edges of the stage that joins ranges: the seam between two ranks, a token count that is 0 or
+-1 mod 31744 at a cut, an empty final block owned by a range with no token, a block whose last token arrives in the tail, ranges
of one segment, a look-ahead of a few bytes.

Everything is generated here from fixed seeds; no data file is committed.  A case is a dict(name, family, data, opts, cuts,
claims): `cuts` are the global byte positions where the ranks begin (the first is 0, every one a multiple of 1024, the last range
ends at len(data)); `g_lo` / `g_hi`, where given, are per-rank overrides (None: the default) of the bytes a rank holds; the
defaults are those of shard.p1_layout -- one window of history in front of the range, rounded down to a multiple of 32768 as
deflate_long.inc does, 128 KiB of look-ahead.  `claims` says what the case must force, in terms of the model, and check() holds
the case to it: a generator that misses fails on the CPU instead of emptying the GPU test.

The model (model()) is plain Python over the restart steps of every position (hostsim_binding.steps, as parse_cases.steps_of)
and over the oracle (encode, trace_blocks, lz77, last_hazards).  It restates what the phases promise -- each constant with the
line that sets it:
  SEG = 1024        deflate_kernels.hip SEG       a range begins on a segment: mi355_shard_begin refuses any other parse_lo
  SPEC_W = 128      deflate_kernels.hip SPEC_W    the run-up: a range that has history follows the steps from its start - 128 and
                                                  takes the first restart position at or behind its start as its entry
  ZONE = 576        deflate_kernels.hip ZONE      entries of an exit table: X[e] = leave(a + e, b) - b for a range [a, b)
  BLOCK = 31744     stages.h MAX_BUFFER_LENGTH    tokens per block; a block belongs to the rank that holds its first token, an
                                                  empty last block to the last rank (shard.p1_token_plan)
  Q13               k_shard_bounds                a full block whose last token is a match that crosses the end of a window that
                                                  is not the first: flag 1, or 2 where the reference's read 32768 bytes further on
                                                  runs past the buffer it holds (65794 bytes from the window's start, or the input's
                                                  end); the position looked at is one behind the token's start for a lazy parse
  Q1                q1_rewarm                     block 0 ends inside the first window: hashes are re-warmed; only the rank that owns
                                                  position 0 looks for it, and only if it holds all 31744 tokens of block 0
"""
import functools
import os
import sys

import numpy as np

import datagen
import hostsim_binding as hs  # noqa: F401  (steps_of goes through it)
import oracle_binding as ob
import parse_cases as pc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deflate-rs_amd"))
import shard  # noqa: E402

SEG, SPEC_W, ZONE, BLOCK, WINDOW = 1024, 128, 576, 31744, 32768
DEFAULT, FAST, BEST, GREEDY, RLE, HUFF = (128, 32, 1), (1, 0, 0), (1768, 128, 1), (128, 32, 0), (0, 0, 1), (0, 0, 0)
LEVEL = {"default": DEFAULT, "fast": FAST, "best": BEST, "greedy": GREEDY, "rle": RLE, "huffman": HUFF}
MAX_RANKS, MAX_BYTES = 8, 400_000
FAMILIES = ("seam", "count", "last", "short", "halo", "q13", "stored", "levels")


# ---- layouts ---------------------------------------------------------------------------------------------------------------------------
def layouts(c):
    """the ranks' layouts, as shard.p1_layout's dicts"""
    total, cuts = len(c["data"]), c["cuts"]
    out = []
    for r, a in enumerate(cuts):
        b = cuts[r + 1] if r + 1 < len(cuts) else total
        g_lo = c.get("g_lo", [None] * len(cuts))[r]
        g_hi = c.get("g_hi", [None] * len(cuts))[r]
        out.append(shard.layout_of(a, b, total, g_lo, g_hi))
    return out


# ---- the model -------------------------------------------------------------------------------------------------------------------------
def tok_word(t):
    """an oracle token as the device's word (stages.h tok_literal / tok_match)"""
    return t[1] if t[0] == "lit" else (t[1] - 3) | (t[2] << 16)


def q13_flag(tp, ln, lazy, n):
    """k_shard_bounds: the flag of a full block whose last token is a match of ln bytes at tp (global positions)"""
    mend = tp + ln
    lp = tp + 1 if lazy else tp
    wdx = lp // WINDOW
    if wdx < 1 or mend <= (wdx + 1) * WINDOW:
        return 0
    return 2 if mend + WINDOW > min(wdx * WINDOW + 65794, n) else 1


def model(c):
    """-> dict: per rank `entry` (global), `count`, `first` (index of its first token), `table` (the exit table, min(576, b - a)
    entries), `spec_entry`, `spec_exit`, `spec_true`, `tokens` (device words); from shard.p1_token_plan `skip`, `tail`, `owns`,
    `pieces`; per block `blocks` = dict(owner, in_bytes, btype, bfinal, bit_start, q13); per rank `nblocks` and `bits` = the bit
    range of its blocks in the stream (None: it owns none); `ref` the oracle's stream (None: the reference panics), `hazards`."""
    data, opts, cuts = c["data"], c["opts"], c["cuts"]
    n, world = len(data), len(cuts)
    lay = layouts(c)
    adv, ntok, _, _ = pc.steps_of(data, opts)
    adv = [int(x) for x in adv]
    on = np.zeros(n + 1, dtype=bool)
    j = 0
    while j < n:
        on[j] = True
        j += adv[j]
    on[n] = True
    path = np.flatnonzero(on)
    toks = ob.lz77(data, *opts)
    words = np.array([tok_word(t) for t in toks], dtype=np.int64)
    cover = np.array([1 if t[0] == "lit" else t[1] for t in toks], dtype=np.int64)
    tstart = np.concatenate([[0], np.cumsum(cover)])  # tstart[i] = where token i starts; tstart[T] = n
    T = len(toks)
    assert int(tstart[-1]) == n
    entry, first, count, table, spec_e, spec_x = [], [], [], [], [], []
    for L in lay:
        a, b = L["a"], L["b"]
        J = {}
        for p in range(b - 1, a - 1, -1):  # J[p] = where the steps from p leave [a, b)
            t = p + adv[p]
            J[p] = t if t >= b else J[t]

        def leave(p, hi, J=J, a=a, b=b):
            if hi == b and a <= p < b:
                return J[p]
            while p < hi:
                p += adv[p]
            return p

        e = int(path[np.searchsorted(path, a)])
        entry.append(e)
        first.append(int(np.searchsorted(tstart, e)))
        table.append([leave(a + k, b) - b for k in range(min(ZONE, b - a))])
        se = leave(a - SPEC_W, a) if a >= SPEC_W else 0
        spec_e.append(se)
        spec_x.append(leave(se, b))
    for r in range(world):
        nxt = first[r + 1] if r + 1 < world else T
        count.append(nxt - first[r])
        # (the same from the steps: the tokens of the steps that start in [entry, b))
        own = path[(path >= entry[r]) & (path < lay[r]["b"])]
        assert int(sum(int(ntok[p]) for p in own)) == count[r], (c["name"], r, count[r])
    skip, tail, owns, pieces = shard.p1_token_plan(count)
    lazy = opts[2] == 1 and opts[0] > 0
    try:
        ref = ob.encode(data, opts=ob.make_opts(*opts))
        rb, hazards = ob.trace_blocks(), ob.last_hazards()
    except ob.RefPanic:
        ref, rb, hazards = None, None, None
    nb = T // BLOCK + 1
    blocks = []
    for k in range(nb):
        t0, t1 = k * BLOCK, min(T, (k + 1) * BLOCK)
        owner = world - 1 if t0 == T else max(r for r in range(world) if first[r] <= t0)
        while t0 < T and count[owner] == 0:  # (ranks without a token share their first index with the rank that has it)
            owner -= 1
        flag = 0
        if t1 - t0 == BLOCK and toks[t1 - 1][0] == "ld":
            flag = q13_flag(int(tstart[t1 - 1]), toks[t1 - 1][1], lazy, n)
        blk = dict(owner=owner, in_bytes=int(tstart[t1] - tstart[t0]), q13=flag, start=int(tstart[t0]), n_lz=t1 - t0)
        if rb is not None:
            assert len(rb) == nb and rb[k]["in_bytes"] == blk["in_bytes"] and rb[k]["n_lz"] == blk["n_lz"], (c["name"], k, rb[k], blk)
            blk.update(btype=rb[k]["btype"], bfinal=rb[k]["bfinal"], bit_start=rb[k]["bit_start"])
        blocks.append(blk)
    nblocks = [sum(1 for blk in blocks if blk["owner"] == r) for r in range(world)]
    bits = [None] * world
    if ref is not None:
        for r in range(world):
            mine = [k for k, blk in enumerate(blocks) if blk["owner"] == r]
            if mine:
                assert mine == list(range(mine[0], mine[-1] + 1))
                bits[r] = (blocks[mine[0]]["bit_start"], blocks[mine[-1] + 1]["bit_start"] if mine[-1] + 1 < nb else 8 * len(ref))
    q1 = False
    if T >= BLOCK and opts[0] > 0 and n >= 2:  # q1_rewarm on the last token of block 0
        tk, tp = toks[BLOCK - 1], int(tstart[BLOCK - 1])
        cov = 1 if tk[0] == "lit" else tk[1]
        if lazy:
            lp, wpos = tp + 1, (tp + cov if tk[0] == "ld" else (tp + 2 if tp + 3 < n else tp + 1))
        else:
            lp, wpos = tp, tp + cov
        q1 = lp < WINDOW and wpos <= WINDOW
    return dict(world=world, lay=lay, T=T, entry=entry, first=first, count=count, table=table, spec_entry=spec_e, spec_exit=spec_x,
                spec_true=[spec_e[r] == entry[r] for r in range(world)], skip=skip, tail=tail, owns=owns, pieces=pieces,
                tokens=[words[first[r]:first[r] + count[r]] for r in range(world)], words=words, tstart=tstart, blocks=blocks,
                nblocks=nblocks, bits=bits, ref=ref, hazards=hazards, q1=q1, adv=adv)


_MODEL = {}


def model_of(c):
    if c["name"] not in _MODEL:
        _MODEL[c["name"]] = model(c)
    return _MODEL[c["name"]]


def masked(ref, lo_bit, hi_bit):
    """the stream with every bit outside [lo_bit, hi_bit) cleared"""
    bits = np.unpackbits(np.frombuffer(ref, dtype=np.uint8), bitorder="little")
    keep = np.zeros_like(bits)
    keep[lo_bit:hi_bit] = 1
    return np.packbits(bits & keep, bitorder="little").tobytes()


def stitched(c):
    """the model's stream: every rank's piece is the oracle's stream masked to the rank's bit range, the pieces OR-ed together"""
    m = model_of(c)
    out = np.zeros(len(m["ref"]), dtype=np.uint8)
    for r in range(m["world"]):
        if m["bits"][r] is not None:
            out |= np.frombuffer(masked(m["ref"], *m["bits"][r]), dtype=np.uint8)
    return out.tobytes()


# ---- building blocks -------------------------------------------------------------------------------------------------------------------
class Lits:
    """literal stretches of any length: parse_cases' 14-bit counter in two bytes, the first of them marked 0x80 or 0x40 -- the mark
    changes before the counter comes round (32768 bytes), and every trigram holds a marked byte, so none occurs twice at all"""

    def __init__(self, start=0):
        self.k = start * 2

    def take(self, n):
        k = np.arange(self.k, self.k + n)
        u = (k // 2) % 16384
        mark = np.where((k // 32768) % 2 == 0, 0x80, 0x40)
        assert self.k + n <= 65536, "two marks: 65536 literal bytes"
        self.k += n
        return np.where(k % 2 == 0, mark | (u >> 8), u & 0xFF).astype(np.uint8).tobytes()


def run_tokens(R):
    """tokens of a run of R equal bytes behind something else: a literal and matches of at most 258"""
    return 0 if R == 0 else R if R < 4 else 1 + (R - 1 + 257) // 258


def _case(name, family, data, opts, cuts, g_lo=None, g_hi=None, **claims):
    c = dict(name=name, family=family, data=bytes(data), opts=opts, cuts=list(cuts), claims=claims)
    if g_lo is not None:
        c["g_lo"] = list(g_lo)
    if g_hi is not None:
        c["g_hi"] = list(g_hi)
    return c


def _text(n, seed):
    return datagen.text_like(n + 8, seed)[:n]


# ---- seam: the cases of parse_cases, cut at the segment their claims name --------------------------------------------------------------
SEAM_D = (0, 1, 2, 127, 128, 257, 258)
SEAM_FROM_PARSE = (["seam_%s_d%d" % (lv, d) for lv in ("default", "best") for d in SEAM_D] + ["seam_%s_maxstep" % lv for lv in ("default", "best")]
                   + ["runup_default_%s" % k for k in ("on_path", "land-1", "land0", "land+1", "covered", "chain")]
                   + ["runup_default_merge%s" % m for m in ("1", "64", "127", "_behind")]
                   + ["repair_default_r1", "repair_default_r3", "repair_default_met_in_run", "repair_default_hops3", "repair_fast_r2"])


def _seam(name):
    p = pc.case(name)
    cl = p["claims"]
    if "seam" in cl:
        seg, extra = cl["seam"][0], dict(entry_off={1: cl["seam"][1]}, spec_true=True)
    elif name.startswith("runup_default_land"):
        seg, extra = 4, dict(entry_off={1: max(0, cl["land"][1] - 4 * SEG)}, spec_true=True)
    elif "two_chains" in cl:
        seg, extra = cl["two_chains"][0], dict(spec_true=False)
    elif "head" in cl or name == "runup_default_merge_behind":
        seg, extra = cl.get("head", 4), dict(spec_true=False)
    else:
        seg, extra = 4, dict(spec_true=True)
    return _case("seam/" + name, "seam", p["data"], p["opts"], [0, seg * SEG], **extra)


# ---- count: one token per byte, so the cuts can be put on the edges of the 31744-token blocks -------------------------------------------
def _counted(name, cuts, total, want_at=None, T=None, opts=DEFAULT, family="count", **claims):
    """a run of R zero bytes, then literals to `total` bytes: R is chosen so that the token index at cut `want_at[0]` is
    want_at[1] mod 31744 (or so that the input has T tokens)"""
    for R in range(0, 6000):
        if want_at is not None and (run_tokens(R) + cuts[want_at[0]] - R) % BLOCK == want_at[1] % BLOCK:
            break
        if T is not None and run_tokens(R) + total - R == T:
            break
    else:
        raise AssertionError(name)
    data = bytes(R) + Lits().take(total - R)
    return _case(name, family, data, opts, cuts, q1=False, **claims)


def _count_cases():
    out = []
    for t in (0, 1, BLOCK - 1):  # (the cut lies behind the first window's end, so block 0 does not end inside it: no Q1)
        out.append(functools.partial(_counted, "count/first_mod_%d" % t, [0, 34816], 40000, want_at=(1, t), first_mod={1: t}))
    # rank 1 has exactly the 2048 tokens that complete block 0: it owns nothing, rank 2 starts on the boundary
    out.append(functools.partial(_counted, "count/exact_to_boundary", [0, 34816, 36864], 40000, want_at=(2, 0), first_mod={2: 0}, owns_none=[1],
                                 pieces={0: [(1, 2048)]}))
    # ranks 1, 2 and 3 are one segment each and fall short of the boundary: rank 0's tail comes from four heads
    out.append(functools.partial(_counted, "count/three_fall_short", [0, 28672, 29696, 30720, 31744], 48000, want_at=(4, BLOCK - 1300), owns_none=[1, 2, 3],
                                 npieces={0: 4}))
    out.append(functools.partial(_counted, "count/T_below_a_block", [2048 * r for r in range(8)], 16384 + 77, T=16384 + 77, T_is=16384 + 77, owns_none=list(range(1, 8)),
                                 npieces={0: 7}, final_owner=0))
    # T = 31744: the empty final block goes to the last rank, which has tokens (all of them block 0's)
    out.append(functools.partial(_counted, "count/T_mod_0", [0, 20480], 34816, T=BLOCK, T_is=BLOCK, final_owner=1, final_empty=True, pieces={0: "all of rank 1"}))
    out.append(functools.partial(_counted, "count/T_mod_0_two_blocks", [0, 34816, 50176], 2 * BLOCK + 2048, T=2 * BLOCK, T_is=2 * BLOCK, final_owner=2, final_empty=True))
    return out


# ---- last: a last range that a match from before it jumps over -----------------------------------------------------------------------------
def _last(tail, ranks):
    p = pc._covered_last("default", tail)
    cuts = [0, 2 * SEG] if ranks == 2 else [0, SEG, 2 * SEG]
    return _case("last/covered_%d_r%d" % (tail, ranks), "last", p["data"], DEFAULT, cuts, jumped=[ranks - 1], last_len=tail, final_owner=0)


def _last_empty_final():
    """31743 literals and their first 200 bytes, cut at 31744: 31744 tokens -- a block and an empty final one --, the step at 31743
    is 200 long, the last range of 199 bytes has no token and owns the empty final block.  (Block 0 ends inside the first window:
    Q1, which rank 0 finds, since it holds all of the block's tokens.)"""
    lit = Lits().take(31743)
    return _case("last/empty_final_block_of_an_empty_rank", "last", lit + lit[:200], DEFAULT, [0, 31744], jumped=[1], last_len=199, T_is=BLOCK, final_owner=1,
                 final_empty=True, q1=True, step=(31743, 200))


# ---- short: ranges of one segment, and of 16 / 17 / 256 / 257 segments (the levels of the table tree at a fan of 16) -------------------------
def _kind(kind, n, seed):
    if kind == "text":
        return _text(n, seed)
    if kind == "zeros":
        return bytes(n)
    return (datagen.rng_bytes(300, seed) * (n // 300 + 1))[:n]


def _short(kind, segs, seed=11):
    cuts, at = [0], 4 * SEG if isinstance(segs, tuple) else SEG
    for s in (segs if isinstance(segs, tuple) else (segs,)):
        cuts.append(at)
        at += s * SEG
    cuts.append(at)
    total = at + 3 * SEG + 100
    nm = "x".join(map(str, segs)) if isinstance(segs, tuple) else str(segs)
    return _case("short/%s_%s" % (kind, nm), "short", _kind(kind, total, seed), DEFAULT, cuts, segs={r + 1: s for r, s in enumerate(segs if isinstance(segs, tuple) else (segs,))},
                 **({"spec_true": False} if kind != "text" else {}))


# ---- halo: history and look-ahead ------------------------------------------------------------------------------------------------------
def _halo_lo(a, lo):
    return _case("halo/parse_lo_%d" % lo, "halo", _text(a + 9000, 61), DEFAULT, [0, a], lo={1: lo})


def _halo_first_window():
    return _case("halo/inside_the_first_window", "halo", _text(50000, 62), DEFAULT, [0, 8192], lo={1: 8192}, g_lo_is={1: 0})


def _halo_ahead(k):
    return _case("halo/look_ahead_%d" % k, "halo", _text(8192 + k, 63), DEFAULT, [0, 4096, 8192], look_ahead={1: k}, last_len=k)


# ---- q13: test_stages_vs_oracle.q13_case --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _q13_data(seed, total):
    import test_stages_vs_oracle as so
    d = so.q13_case(seed, total=total)
    assert d is not None, (seed, total)
    return d


def _q13(seed, cuts, total=140000):
    nm = "q13/seed%d_%s%s" % (seed, "_".join(str(x) for x in cuts[1:]), "" if total == 140000 else "_total%d" % total)
    # (the block begins at 66507 and ends with the match across 98304: cut at 66560 or 97280 it is rank 0's and its last token comes
    # in the tail; cut at 65536 and 98304 it is rank 1's, whose own last token ends it)
    return _case(nm, "q13", _q13_data(seed, total), DEFAULT, cuts, q13_flag=1 if total == 140000 else 2, q13_block_at=98304, q13_owner=len(cuts) - 2,
                 q13_tail=len(cuts) == 2)


# ---- stored: noise across a cut ----------------------------------------------------------------------------------------------------------
def _token_at(data, opts, idx):
    pos = 0
    for i, t in enumerate(ob.lz77(data, *opts)):
        if i == idx:
            return pos
        pos += 1 if t[0] == "lit" else t[1]
    return None


@functools.lru_cache(maxsize=None)
def _stored(quarter):
    """zeros, then noise: the run's length puts token 31744 -- the first of block 1, which is Stored -- on the byte in front of the cut
    at 34816, so block 1 belongs to rank 0 and all its bytes but one lie in rank 0's look-ahead; rank 1 owns block 2, which begins on a
    byte (behind a Stored block); the noise's seed is varied until that byte is `quarter` mod 4"""
    cut = 34816
    for seed in range(200, 260):
        noise = datagen.rng_bytes(BLOCK * 2 + 9000, seed)
        R = 3100
        for _ in range(8):
            data = bytes(R) + noise[:BLOCK * 2 + 6000]
            p = _token_at(data, DEFAULT, BLOCK)
            if p == cut - 1:
                break
            R += cut - 1 - p
        else:
            continue
        c = _case("stored/byte_%d_mod_4" % quarter, "stored", data, DEFAULT, [0, cut], stored_before_cut=(1, 1), first_bit_quarter={1: quarter}, q1=False)
        m = model(c)
        b2 = m["blocks"][2]
        if m["blocks"][1]["btype"] == 0 and b2["owner"] == 1 and b2["bit_start"] % 32 // 8 == quarter and b2["bit_start"] % 8 == 0:
            return c
    raise AssertionError("stored: no seed for quarter %d" % quarter)


@functools.lru_cache(maxsize=None)
def _stored_behind_text():
    """text, then noise: rank 1's first block begins inside a byte, behind a Dynamic block, and a Stored block straddles the cut"""
    for seed in range(300, 330):
        data = _text(100000, seed) + datagen.rng_bytes(60000, seed)
        c = _case("stored/behind_a_dynamic_block", "stored", data, DEFAULT, [0, 65536, 131072], first_bit_mod8_nonzero=1, stored_straddles=2)
        m = model(c)
        k = next((i for i, b in enumerate(m["blocks"]) if b["owner"] == 1), None)
        if k and m["blocks"][k]["bit_start"] % 8 and any(b["btype"] == 0 and b["start"] < 131072 < b["start"] + b["in_bytes"] for b in m["blocks"]):
            return c
    raise AssertionError("stored_behind_text")


# ---- levels ----------------------------------------------------------------------------------------------------------------------------
def _level_seam(level):
    if level in ("fast", "greedy"):
        p = pc._seam({"fast": "fast", "greedy": "greedy"}[level], 128)
        return _case("levels/seam_%s" % level, "levels", p["data"], LEVEL[level], [0, 3 * SEG], entry_off={1: 128})
    # rle: a run of one byte across the cut -- a literal at 3000, matches of 258 from 3001: the first one ends 187 bytes behind the
    # cut at 3072.  Huffman only: nothing but literals, the range is entered on its first byte
    lit = Lits()
    data = lit.take(3000) + (b"\xee" * 600 if level == "rle" else lit.take(600)) + lit.take(2000)
    return _case("levels/seam_%s" % level, "levels", data, LEVEL[level], [0, 3 * SEG], entry_off={1: 3001 + 258 - 3 * SEG if level == "rle" else 0})


def _level_count(level):
    c = _counted("levels/count_%s" % level, [2048 * r for r in range(8)], 16384 + 77, T=16384 + 77, T_is=16384 + 77, opts=LEVEL[level], family="levels",
                 owns_none=list(range(1, 8)), npieces={0: 7}, final_owner=0)
    return c


def _all_cases():
    out = [functools.partial(_seam, nm) for nm in SEAM_FROM_PARSE]
    out += _count_cases()
    out += [functools.partial(_last, t, 2) for t in (1, 2, 199, 257)] + [functools.partial(_last, 1, 3), _last_empty_final]
    for kind in ("text", "zeros", "period"):
        out.append(functools.partial(_short, kind, (1, 1, 1)))
    out.append(functools.partial(_short, "zeros", (1, 1)))
    for kind in ("zeros", "period"):
        out += [functools.partial(_short, kind, (16, 17)), functools.partial(_short, kind, 256), functools.partial(_short, kind, 257)]
    out += [functools.partial(_halo_lo, 98304, 32768), functools.partial(_halo_lo, 99328, 33792), functools.partial(_halo_lo, 130048, 64512), _halo_first_window]
    out += [functools.partial(_halo_ahead, k) for k in (1, 257, 258, 259)]
    for seed in (1, 3):
        out += [functools.partial(_q13, seed, [0, 66560]), functools.partial(_q13, seed, [0, 97280]), functools.partial(_q13, seed, [0, 65536, 98304])]
    out.append(functools.partial(_q13, 1, [0, 66560], 120000))
    out += [functools.partial(_stored, q) for q in range(4)] + [_stored_behind_text]
    for level in ("fast", "greedy", "rle", "huffman"):
        out += [functools.partial(_level_seam, level), functools.partial(_level_count, level)]
    return out


@functools.lru_cache(maxsize=None)
def _built():
    cs = [f() for f in _all_cases()]
    names_ = [c["name"] for c in cs]
    assert len(set(names_)) == len(names_), sorted(n for n in names_ if names_.count(n) > 1)
    return {c["name"]: c for c in cs}


def names(family=None):
    return [n for n, c in _built().items() if family is None or c["family"] == family]


def case(name):
    return _built()[name]


# ---- preconditions ---------------------------------------------------------------------------------------------------------------------
def check(c):
    """the case is well formed and forces what its claims say -- on the model"""
    data, cl, name, cuts = c["data"], c["claims"], c["name"], c["cuts"]
    n = len(data)
    m = model_of(c)
    lay, world = m["lay"], m["world"]
    assert n <= MAX_BYTES and world <= MAX_RANKS and cuts[0] == 0 and cuts == sorted(set(cuts)) and cuts[-1] < n, name
    for L in lay:
        assert L["a"] % SEG == 0 and L["g_lo"] % WINDOW == 0 and (L["g_lo"] == 0 or L["g_lo"] <= L["a"] - WINDOW), (name, L)
        assert L["lo"] == L["a"] - L["g_lo"] and L["g_lo"] <= L["a"] < L["b"] <= L["g_hi"] <= n, (name, L)
    # what a rank works out from the bytes it holds is what the whole input gives: its steps from the run-up to the end of its range
    for L in lay:
        if L["g_lo"] or L["g_hi"] < n:
            mine = pc.steps_of(data[L["g_lo"]:L["g_hi"]], c["opts"])[0]
            s = max(L["a"] - SPEC_W, L["g_lo"])
            assert [int(x) for x in mine[s - L["g_lo"]:L["hi"]]] == m["adv"][s:L["b"]], (name, L, "the rank's steps are not the input's")
    assert sum(m["count"]) == m["T"] == len(ob.lz77(data, *c["opts"])), name
    assert sum(m["nblocks"]) == len(m["blocks"]) == m["T"] // BLOCK + 1, name
    for r in range(world):  # (the exchange math gives every rank the blocks the oracle's table gives it)
        own = m["count"][r] - m["skip"][r] + m["tail"][r]
        assert own // BLOCK + (1 if m["owns"][r] else 0) == m["nblocks"][r] and (m["owns"][r] or own % BLOCK == 0), (name, r)
        assert all(0 <= x < 65536 for x in m["table"][r]) and len(m["table"][r]) == min(ZONE, lay[r]["b"] - lay[r]["a"]), (name, r)
        assert m["entry"][r] - lay[r]["a"] < ZONE or m["entry"][r] >= lay[r]["b"], (name, r, "entry outside the entry zone")
    assert m["q1"] == bool(cl.get("q1", False)), (name, "Q1", m["q1"])
    if m["q1"]:  # (only rank 0 looks for it, and it must hold block 0's tokens to see it)
        assert m["count"][0] >= BLOCK and lay[0]["g_hi"] >= BLOCK, name
    for r, d in cl.get("entry_off", {}).items():
        assert m["entry"][r] - lay[r]["a"] == d, (name, r, m["entry"][r] - lay[r]["a"], d)
    if "spec_true" in cl:
        assert all(m["spec_true"]) == cl["spec_true"], (name, m["spec_true"])
    for r, t in cl.get("first_mod", {}).items():
        assert m["first"][r] % BLOCK == t and m["count"][r] > 0, (name, r, m["first"][r] % BLOCK)
    for r in cl.get("owns_none", []):
        assert m["nblocks"][r] == 0 and m["count"][r] > 0 and m["skip"][r] == m["count"][r], (name, r)
    for r, want in cl.get("pieces", {}).items():
        assert m["pieces"][r] == ([(r + 1, m["count"][r + 1])] if isinstance(want, str) else want), (name, r, m["pieces"][r])
    for r, k in cl.get("npieces", {}).items():
        assert len(m["pieces"][r]) == k, (name, r, m["pieces"][r])
    if "T_is" in cl:
        assert m["T"] == cl["T_is"], (name, m["T"])
    if "final_owner" in cl:
        assert m["blocks"][-1]["owner"] == cl["final_owner"] and m["owns"][cl["final_owner"]], (name, m["blocks"][-1])
    if cl.get("final_empty"):
        assert m["blocks"][-1]["n_lz"] == 0 and m["blocks"][-1]["in_bytes"] == 0 and m["T"] % BLOCK == 0, name
    for r in cl.get("jumped", []):
        assert m["entry"][r] >= lay[r]["b"] and m["count"][r] == 0, (name, r, m["entry"][r])
    if "last_len" in cl:
        assert lay[-1]["b"] - lay[-1]["a"] == cl["last_len"], name
    if "step" in cl:
        p, ln = cl["step"]
        assert m["adv"][p] == ln and p in m["entry"] + [int(x) for x in m["tstart"]], name
    for r, s in cl.get("segs", {}).items():
        assert lay[r]["b"] - lay[r]["a"] == s * SEG, (name, r)
    for r, lo in cl.get("lo", {}).items():
        assert lay[r]["lo"] == lo, (name, r, lay[r]["lo"])
    for r, g in cl.get("g_lo_is", {}).items():
        assert lay[r]["g_lo"] == g and 0 < lay[r]["a"] < WINDOW, (name, r)
    for r, k in cl.get("look_ahead", {}).items():
        assert lay[r]["g_hi"] - lay[r]["b"] == k and lay[r]["g_hi"] == n and r == world - 2, (name, r)
    if "q13_flag" in cl:
        hit = [k for k, b in enumerate(m["blocks"]) if b["q13"]]
        assert len(hit) == 1 and m["blocks"][hit[0]]["q13"] == cl["q13_flag"], (name, [b["q13"] for b in m["blocks"]])
        b = m["blocks"][hit[0]]
        assert b["start"] < cl["q13_block_at"] < b["start"] + b["in_bytes"], (name, b)
        if cl["q13_flag"] == 1:  # (the reference reads the wrong bytes and says so)
            assert b["btype"] == 0 and m["hazards"] == 1, (name, b, m["hazards"])
            assert b["owner"] == cl["q13_owner"] and (m["tail"][b["owner"]] > 0) == cl["q13_tail"], (name, b, m["tail"])
        else:
            assert m["ref"] is None, name
    elif m["ref"] is not None:
        assert not m["hazards"] and not any(b["q13"] for b in m["blocks"] if b["btype"] == 0), name
    if "stored_before_cut" in cl:
        k, r = cl["stored_before_cut"]
        b = m["blocks"][k]
        assert b["btype"] == 0 and b["start"] == lay[r]["a"] - 1 and b["owner"] == r - 1, (name, b)
        assert b["start"] + b["in_bytes"] > lay[r - 1]["b"] + 30000, name
    for r, q in cl.get("first_bit_quarter", {}).items():
        assert m["bits"][r][0] % 32 // 8 == q and m["bits"][r][0] % 8 == 0, (name, m["bits"][r])
    if "first_bit_mod8_nonzero" in cl:
        assert m["bits"][cl["first_bit_mod8_nonzero"]][0] % 8 != 0, name
    if "stored_straddles" in cl:
        a = lay[cl["stored_straddles"]]["a"]
        assert any(b["btype"] == 0 and b["start"] < a < b["start"] + b["in_bytes"] for b in m["blocks"]), name
    return m
