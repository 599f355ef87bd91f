"""Inputs that drive the last two stages of the encoder -- plan_blocks (k_plan / kb_plan: every block's type and bit offset)
and the pack (body_k_pack.inc: k_pack<1024>, k_pack<256>, kb_pack, fed by k_block_hist) -- onto their phase and word edges,
and a model of the stream's geometry that says whether an input reaches them.

Everything is generated here from fixed seeds; no data file is committed.  A case is a dict(name, data, level, claims and,
for a stream driven through the writer, cuts = the byte offsets a flush follows).  model() reads the ORACLE's stream only
and gives per block its type, bit offsets, stored payload geometry, and for a compressed block the first and last bit of
every part (7 936 tokens: a k_pack workgroup), of every round (1 024 tokens for k_pack<256>, 4 096 for k_pack<1024>) and
every token of 34 bits or more.  facts() turns the model into cells -- tuples like ("stored_align", 1, 3) --, a case's
claims are the cells it is there for, and check() asserts them, so a case that stops forcing its edge fails instead of
passing empty-handed.  tests/test_pack_cases.py (CPU) and tests/test_pack_gpu.py use the cases.

Huffman-only is the main vehicle: a token is a byte, block b is bytes [31744 b, 31744 (b + 1)), and a block's type and
length follow from its own bytes (and, for a stored block, the bit phase it starts at).  T(seed) is a block of text
(dynamic at every phase), R(seed) one of noise (stored at every phase), P a block of noise whose first bytes are masked to
seven bits, just enough for the dynamic estimate to land within a byte of the stored cost: stored at some phases, dynamic
at the others.

The cells
  ("plain", N)                  N blocks, none depends on its phase: the workgroup path of plan_blocks up to 1024, above it
                                the wave walk with every group on the fixed-length shortcut
  ("stored_group", phase, kind) a 64-aligned group of blocks that are stored whatever the phase, its first block starting
                                at `phase`; kind "full" (64 blocks), "cnt1", "cnt63" (the stream's last, partly filled group:
                                its last block is the final one), "final_full" (64 blocks, the last is the final one)
  ("stored_mixed", phase)       a stored block starting at `phase` in a group that takes the serial path
  ("phase_dep", type, phase)    a block of kind P that has `type` at `phase` -- and another type at another phase, which
                                check() sees by encoding the same 31 744 bytes behind another front block
  ("phase_dep_big", type)       the same inside an otherwise plain stream of at most 1024 blocks
  ("sync", phase), ("sync_mod4", m), ("sync_after", type)   a sync marker behind a block that ends at `phase`; the byte offset
                                of the marker's 00 00 FF FF mod 4; the type of the block in front
  ("stored_align", ob % 4, (ob + length) % 4)   ob = byte offset of a stored block's first payload byte
  ("stored_head", ob % 4, value), ("stored_tail", end % 4, value)  every payload byte in the shared first / last word is
                                `value` (0: the OR is skipped; 255: every bit of the byte is set)
  ("stored_final",), ("stored_len", n)   a stored block is the final one (its last byte the input's last); its length
  ("stored_then", type)         a stored block ends inside a word and a block of `type` begins there
  ("part_end_aligned", q)       part q (0, 1, 2, or "last") of a block ends on a word boundary: no tail OR, and what follows
                                begins with rel0 = 0
  ("part_start_31",)            a part q > 0 begins at bit 31 of a word
  ("round_end_aligned", size)   a round that is not its part's last ends on a word boundary (size 1024 or 4096)
  ("tiny_last_part", k, j)      nt = 7936 k + j, j in 1..3, and the last part's bits stay inside the word it begins in:
                                first_shared is never cleared
  ("nt0",)                      a block without tokens (the input is a multiple of 31 744 tokens)
  ("long3", where)              a token of 34 bits or more that spans three words, as the first token of a part
                                ("part_first"), a wave's last token (index 255 mod 256 in a round: "wave_last"), a round's
                                last token ("round_last": index 1023 mod 1024 in its part), the block's last ("block_last")
  ("n_enc", n), ("used_hclens", u)   a dynamic header with that many run-coded lengths / code-length code lengths

What the searches gave (all on the oracle)
  * The smallest stored block: see SMALLEST_STORED below -- the final block behind a dynamic block that ends at phase 5
    (no padding), its bytes distinct values of 144 and above (nine bits each in the fixed code).
  * n_enc: no case of header_cases.py goes beyond 255.  At huffman_only the chain has 258 entries and a run saves two or
    more, so 257 is out of reach there; the cases here reach 258 (no run at all, huffman_only), 257 and 259 and more (rle
    level).  316 needs all 286 + 30 symbols without one run of equal lengths and was not reached; the largest is
    N_ENC_MAX below.  used_hclens = 4 cannot occur (some non-zero length must be sent as itself, and the first of them in
    the order, 8, is entry 5, and 5 would need every used symbol at 8 bits: 255 byte values once each, which the stored
    form beats); the cases reach 6 and 19 (USED_HCLENS below).
  * The longest token the oracle's limiter lets a case reach: LONGEST_TOKEN below.
  * A stored block of more than 32 767 bytes (second stored piece, and with it the `w1 <= w0` branch of the stored path,
    which needs a piece of under four bytes) and a fixed block of more than 7 936 tokens (part > 0 of a fixed block):
    see UNREACHED below for what was tried.  No case reaches them and no test claims them either way.
  * Trains: see the section "trains" below.  Only a stream's last block can be partial, so a train is the body (the cases
    made of whole blocks) plus at most one case that ends with a partial block; the rle and default cases, and the
    input of the piece-wise host path (streamed_input), run alone and in batches only.
"""
import functools
import random

import numpy as np

import datagen
import header_cases as hc
import oracle_binding as ob

LV = hc.LV
B = hc.BLOCK_TOKENS
PQ = B // 4
ROUNDS = (1024, 4096)
LONG_BITS = 34
H = "huffman_only"


# ---- the oracle's stream and its model ---------------------------------------------------------------------------------------------
def oracle(data, level, cuts=(), wrapper=0):
    """(stream, block table or None) of the oracle; with cuts through its writer, a flush behind every data[:cut]"""
    opts = ob.make_opts(*LV[level], wrapper)
    if not cuts:
        return ob.encode(data, opts=opts), ob.trace_blocks()
    s = ob.Stream(opts)
    prev = 0
    for c in cuts:
        s.write_all(data[prev:c])
        s.flush()
        prev = c
    s.write_all(data[prev:])
    return s.finish(), None


def model(stream, start=0, blocks=0):
    """per block of a raw deflate stream: dict(btype, bfinal, bit_start, bit_end, phase = bit_start % 8) and
    stored:   ob (byte offset of the first payload byte), length, sync (an empty stored block that is not final: a marker)
    coded:    nt, hdr_bits, parts [(first bit, last bit)] per 7 936 tokens, rounds {size: [(part, round, first, last)]},
              long [(token index, bit, bits)] for the tokens of LONG_BITS or more, eob (bit of the end-of-block code)
    start: the bit the first block to read begins at, blocks: how many to read (a train's members are read from their first
    bit, not the whole train)"""
    out = []
    for blk in hc.decode(stream, positions=True, start=start, blocks=blocks):
        m = dict(btype=blk["btype"], bfinal=blk["bfinal"], bit_start=blk["bit_start"], bit_end=blk["bit_end"],
                 phase=blk["bit_start"] & 7)
        if blk["btype"] == 0:
            m.update(ob=blk["payload"], length=blk["stored"], sync=blk["stored"] == 0 and not blk["bfinal"])
        else:
            pos = blk["tok_pos"]
            nt = len(pos) - 1
            m.update(nt=nt, hdr_bits=pos[0] - blk["bit_start"], eob=pos[nt], parts=[], rounds={r: [] for r in ROUNDS}, long=[])
            for q in range(max(1, (nt + PQ - 1) // PQ)):
                t0, t1 = q * PQ, min((q + 1) * PQ, nt)
                m["parts"].append((pos[t0], pos[t1]))
                for size in ROUNDS:
                    for r, a in enumerate(range(t0, t1, size)):
                        m["rounds"][size].append((q, r, pos[a], pos[min(a + size, t1)]))
            m["long"] = [(i, pos[i], pos[i + 1] - pos[i]) for i in range(nt) if pos[i + 1] - pos[i] >= LONG_BITS]
            if blk["btype"] == 2:
                m.update(n_enc=len(ob.encode_lengths(blk["ll_lens"] + blk["d_lens"])[0]), used_hclens=_used_hclens(blk["cl_lens"]))
        out.append(m)
    return out


def spans_three_words(bit, nbits):
    return (bit & 31) + nbits > 64


def always_stored(block):
    """True where a block of bytes (one literal each) is stored at every phase: the literal/length code alone, with the
    shortest header there is, costs more than the stored form with its longest padding -- and so does the fixed code"""
    n = len(block)
    f = np.bincount(np.frombuffer(block, dtype=np.uint8), minlength=256).tolist() + [1]
    lens = ob.huffman_lengths(f, 15)
    dyn_low = sum(a * b for a, b in zip(f, lens)) + 14 + 3 * 4
    static = sum(c * (8 if v < 144 else 9) for v, c in enumerate(f[:256])) + 7
    stored_high = 8 * (n + 4 * ((n - 1) // 32767 + 1)) + 7
    return n > 4 and dyn_low > stored_high and static > stored_high


def pack_diff(got, want):
    """Where two streams part: the block, the part of it (stored: head / words / tail) and the first differing bit; None for
    equal streams.  The oracle's stream (`want`) gives the geometry."""
    if got == want:
        return None
    n = min(len(got), len(want))
    byte = next((i for i in range(n) if got[i] != want[i]), n)
    bit = 8 * byte + (((got[byte] ^ want[byte]) & -(got[byte] ^ want[byte])).bit_length() - 1 if byte < n else 0)
    try:
        ms = model(want)
    except (ValueError, IndexError) as e:
        return "first differing bit %d (the expected stream cannot be read: %s)" % (bit, e)
    for b, m in enumerate(ms):
        if not (m["bit_start"] <= bit < m["bit_end"]) and not (b + 1 == len(ms) and bit >= m["bit_start"]):
            continue
        where = "block %d (type %d, bits %d..%d)" % (b, m["btype"], m["bit_start"], m["bit_end"])
        if m["btype"] == 0:
            o, e = 8 * m["ob"], 8 * (m["ob"] + m["length"])
            w0, w1 = (m["ob"] + 3) // 4 * 32, (m["ob"] + m["length"]) // 4 * 32
            part = "header" if bit < o else "head bytes" if bit < w0 else "whole words" if bit < w1 else "tail bytes" if bit < e else "behind it"
        elif bit < m["bit_start"] + m["hdr_bits"]:
            part = "header (%d bits)" % m["hdr_bits"]
        elif bit >= m["eob"]:
            part = "end-of-block code"
        else:
            q = max(i for i, (a, _) in enumerate(m["parts"]) if a <= bit)
            r = max((x for x in m["rounds"][1024] if x[0] == q and x[2] <= bit), key=lambda x: x[1])
            part = "part %d (bits %d..%d), round %d of 1024 tokens (bits %d..%d)" % (q, m["parts"][q][0], m["parts"][q][1], r[1], r[2], r[3])
        return "%s, %s: first differing bit %d (word %d, bit %d of it); %d vs %d bytes" % (where, part, bit, bit >> 5, bit & 31, len(got), len(want))
    return "first differing bit %d, behind the last block; %d vs %d bytes" % (bit, len(got), len(want))


# ---- blocks ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def T(seed):
    """a block of text: dynamic at every phase"""
    return datagen.text_like(B, 1000 + seed)


def R(seed, n=B):
    """noise: stored at every phase"""
    return datagen.rng_bytes(n, 77000 + seed)


def P(seed, k):
    """noise whose first k bytes are masked to seven bits"""
    a = np.frombuffer(R(seed), dtype=np.uint8).copy()
    a[:k] &= 0x7F
    return a.tobytes()


@functools.lru_cache(maxsize=None)
def t_len(seed):
    """bits of T(seed) as a dynamic block (the same wherever it stands: nothing of it depends on the phase)"""
    ob.encode(T(seed), opts=ob.make_opts(*LV[H]))
    return ob.trace_blocks()[1]["bit_start"]


# T(seed) by its length mod 8, and by the payload offset mod 4 of a stored block behind it at the head of a stream
T8 = {0: 1, 1: 6, 2: 14, 3: 2, 4: 13, 5: 17, 6: 3, 7: 0}
T_OB4 = {0: 0, 1: 4, 2: 3, 3: 1}
# ... and by its length mod 32: an aligner in a train (the first 105 seeds hold all 32)
T32 = {0: 4, 1: 20, 2: 30, 3: 11, 4: 13, 5: 24, 6: 3, 7: 10, 8: 16, 9: 36, 10: 14, 11: 5, 12: 38, 13: 32, 14: 63, 15: 43, 16: 1,
       17: 6, 18: 67, 19: 2, 20: 26, 21: 104, 22: 95, 23: 0, 24: 53, 25: 66, 26: 21, 27: 102, 28: 27, 29: 17, 30: 35, 31: 19}
# P blocks (bisect k for the flip at phase 0, then the types at all eight phases for k - 60 .. k + 60).
# The stored cost is 8 n + 32 + padding, padding 5 4 3 2 1 0 7 6 for phase 0..7: the phases a block is stored at grow from 5.
P_A = (2, 9196)  # stored at phases 2..5, dynamic at 0, 1, 6, 7
P_B = (3, 9230)  # stored at phases 3..5
P_C = (2, 9193)  # stored at phases 0..5, dynamic at 6, 7
P_D = (1, 8924)  # stored at phase 5 alone


# ---- facts: the cells a stream reaches ----------------------------------------------------------------------------------------------
def token_facts(m):
    """the token-family cells of one compressed block of a model"""
    out = set()
    nt, parts = m["nt"], m["parts"]
    if nt == 0:
        out.add(("nt0",))
        return out
    for q, (a, e) in enumerate(parts):
        if e % 32 == 0:
            out.add(("part_end_aligned", q))
            if q == len(parts) - 1:
                out.add(("part_end_aligned", "last"))
        if q > 0 and a % 32 == 31:
            out.add(("part_start_31",))
    for size in ROUNDS:
        per_part = {}
        for q, r, a, e in m["rounds"][size]:
            per_part[q] = max(per_part.get(q, 0), r)
        for q, r, a, e in m["rounds"][size]:
            if r < per_part[q] and e % 32 == 0:
                out.add(("round_end_aligned", size))
    k, j = divmod(nt, PQ)
    if k >= 1 and 1 <= j <= 3:
        a, e = parts[-1]
        if (a & 31) + (e - a) < 32:
            out.add(("tiny_last_part", k, j))
    for i, bit, nb in m["long"]:
        if spans_three_words(bit, nb):
            if i % PQ == 0:
                out.add(("long3", "part_first"))
            if (i % PQ) % 256 == 255:
                out.add(("long3", "wave_last"))
            if (i % PQ) % 1024 == 1023:
                out.add(("long3", "round_last"))
            if i == nt - 1:
                out.add(("long3", "block_last"))
    return out


# ---- headers with many run-coded lengths ---------------------------------------------------------------------------------------------
def norun_lens(top=14, run4=False):
    """256 code lengths that sum to 1 - 2^-top (end-of-block takes the rest) without three equal neighbours: 45 of 7 bits,
    125 of 8, 81 of 9 and one each of 10..top, dealt out so that the most frequent length still to place goes next unless
    it would make a third in a row"""
    left = {7: 45, 8: 125, 9: 81}
    for l in range(10, top + 1):
        left[l] = 1
    assert sum(left.values()) == 256 and sum(c << (top - l) for l, c in left.items()) + 1 == 1 << top
    lens = list(range(10, top + 1))  # (the single ones first: value 255 must not share end-of-block's length)
    for l in lens:
        left[l] = 0
    if run4:  # one run of four equal lengths: a literal and one copy symbol, two entries less
        lens += [8] * 4
        left[8] -= 4
    while len(lens) < 256:
        for l in sorted(left, key=lambda l: -left[l]):
            if left[l] and lens[-2:] != [l, l]:
                lens.append(l)
                left[l] -= 1
                break
        else:
            raise AssertionError("no length fits")
    return lens


@functools.lru_cache(maxsize=None)
def norun_bytes(seed, top=14, runs=(), run4=False):
    """bytes with norun_lens' code lengths (frequencies 2^(top - length): only these lengths meet the entropy bound), and
    behind them runs of one byte each, runs[i] + 1 long -- at the rle level a literal and a match of runs[i] at distance 1"""
    body = bytearray(hc.dyadic_bytes(norun_lens(top, run4), seed))
    rnd = random.Random(seed)
    for ln in runs:
        v = rnd.choice([x for x in range(256) if x != body[-1]])
        body += bytes([v]) * (ln + 1)
    return bytes(body)


def header_figures(stream):
    """per dynamic block of a stream: (n_enc, used_hclens)"""
    return [(len(ob.encode_lengths(b["ll_lens"] + b["d_lens"])[0]), _used_hclens(b["cl_lens"])) for b in hc.decode(stream)
            if b["btype"] == 2]


def _used_hclens(cl_lens):
    used = 19
    while used > 0 and cl_lens[hc.ORDER[used - 1]] == 0:
        used -= 1
    return used


@functools.lru_cache(maxsize=None)
def _phase_types_cached(block):
    out = []
    for r in range(8):
        ob.encode(T(T8[r]) + block + b"xyz", opts=ob.make_opts(*LV[H]))
        bl = ob.trace_blocks()
        assert bl[1]["bit_start"] % 8 == r
        out.append(bl[1]["btype"])
    return tuple(out)


def phase_types(block):
    """the types the oracle gives one block of 31 744 bytes at huffman_only when it starts at phase 0..7: the same bytes
    behind eight front blocks"""
    assert len(block) == B
    return _phase_types_cached(bytes(block))


def plain_blocks(table, stream_bits, skip=()):
    """number of blocks where no block of an oracle's table can change with its phase (else 0): none stored, and each at
    least 320 bits (more than the header's run-coded lengths, which is all dyn_est can exceed dyn_bits by) under the
    cheapest stored form.  skip: blocks not to look at"""
    for i, (b, e) in enumerate(zip(table, [b["bit_start"] for b in table[1:]] + [stream_bits])):
        if i not in skip and (b["btype"] == 0 or (b["in_bytes"] > 4 and e - b["bit_start"] + 320 >= 8 * b["in_bytes"] + 32)):
            return 0
    return len(table)


def facts(case, stream=None, table=None, ms=None, whole=True):
    """the cells the oracle's stream of a case reaches.  ms: blocks of a model to look at (whole=False: a part of a stream,
    nothing is said about groups of 64 blocks then)"""
    if stream is None:
        stream, table = oracle(case["data"], case["level"], case.get("cuts", ()))
    out = set()
    if table is not None and whole:
        n = plain_blocks(table, 8 * len(stream))
        if n:
            out.add(("plain", n))
    if table is not None and whole:
        for b in case.get("dep", ()):  # (type and phase from the oracle's table)
            ty = phase_types(case["data"][b * B:(b + 1) * B])
            bt, ph = table[b]["btype"], table[b]["bit_start"] % 8
            assert ty[ph] == bt, (case["name"], b, ty, ph, bt)
            if len(set(ty)) > 1:
                out.add(("phase_dep", bt, ph))
                if case.get("dep_big") and plain_blocks(table, 8 * len(stream), skip=(b,)) and len(table) <= 1024:
                    out.add(("phase_dep_big", bt))
    if case.get("big"):
        return out
    if ms is None:
        ms = model(stream)
    real = [m for m in ms if not m.get("sync")]
    for i, m in enumerate(ms):
        nxt = ms[i + 1] if i + 1 < len(ms) else None
        if m.get("sync"):
            out |= {("sync", m["bit_start"] & 7), ("sync_mod4", (m["ob"] - 4) % 4), ("sync_after", ms[i - 1]["btype"] if i else None)}
        elif m["btype"] == 0:
            o, n = m["ob"], m["length"]
            i4, e4 = o % 4, (o + n) % 4
            out.add(("stored_align", i4, e4))
            head, tail = stream[o:o + (4 - i4) % 4], stream[o + n - e4:o + n]
            if n >= 8:
                for key, part, at in (("stored_head", head, i4), ("stored_tail", tail, e4)):
                    for v in (0, 255):
                        if part and part == bytes([v]) * len(part):
                            out.add((key, at, v))
            if m["bfinal"]:
                out |= {("stored_final",), ("stored_len", n)}
            if e4 and nxt is not None:
                out.add(("stored_then", "sync" if nxt.get("sync") else nxt["btype"]))
        else:
            out |= token_facts(m)
            if m["btype"] == 2:
                out |= {("n_enc", m["n_enc"]), ("used_hclens", m["used_hclens"])}
    if whole and not case.get("cuts"):
        for g in range(0, len(real), 64):
            grp = real[g:g + 64]
            if all(m["btype"] == 0 and always_stored(stream[m["ob"]:m["ob"] + m["length"]]) for m in grp):
                last = g + 64 >= len(real)
                kind = ("final_full" if grp[-1]["bfinal"] else "full") if len(grp) == 64 else "cnt%d" % len(grp)
                assert len(grp) == 64 or last
                out.add(("stored_group", grp[0]["phase"], kind))
            else:
                out |= {("stored_mixed", m["phase"]) for m in grp if m["btype"] == 0}
    return out


def check(case):
    """assert a case's claims on the oracle's stream; returns the cells it reaches"""
    got = facts(case)
    missing = sorted(set(case["claims"]) - got, key=str)
    assert not missing, "%s does not reach %s (it reaches %s)" % (case["name"], missing, sorted(got, key=str))
    return got


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
SMALLEST_STORED = 26  # bytes, at phase 5; 27 28 29 30 at phase 4 3 2 1, 31 at phase 0, 32 at 7, 33 at 6
SMALLEST_BYTES = bytes([186, 161, 200, 169, 170, 176, 222, 194, 198, 147, 223, 189, 213, 190, 158, 211, 238, 220, 231, 255, 172,
                        221, 210, 236, 195, 178])
# T(seed) that reach a token-family cell (T(0) .. T(39) searched, every cell met by seed 38), and the seeds s of
# text_like(7936 k + j, 5000 + s) whose last part of j tokens stays in its word (at most three seeds tried a cell)
TOKEN_SEEDS = {16: [("part_end_aligned", 0)], 29: [("part_end_aligned", 1)], 31: [("part_end_aligned", 2)],
               38: [("part_end_aligned", 3), ("part_end_aligned", "last")], 11: [("part_start_31",)],
               2: [("round_end_aligned", 1024)], 10: [("round_end_aligned", 4096)]}
TOKEN_VARIANTS_SEARCHED = 40
TINY_SEEDS = {(1, 1): 0, (1, 2): 0, (1, 3): 0, (2, 1): 1, (2, 2): 2, (2, 3): 2, (3, 1): 0, (3, 2): 0, (3, 3): 0}
# runs of the rle-level header cases: matches of these lengths at distance 1 behind norun_bytes
RUNS_ALL_CODES = tuple(l for i, l in enumerate(hc.LBASE) for _ in range(1 + (i * 7) % 5))
N_ENC_MAX = 284  # of 316: hdr_284 (258 literal/length lengths without a run, 28 more for the length codes and the distance)
USED_HCLENS = (6, 19)  # the smallest and the largest reached (4 and 5 cannot be, see the module docstring)
LONGEST_TOKEN = 35  # bits (long_round, token 4095 of block 1).  It is not the limiter that stops here: a rare symbol under a
#                     flat histogram hangs just below the lightest common one (11 + 5 bits for the length, 6 + 13 for the
#                     distance).  The 48 bits of two limited codes need both histograms skewed like header_cases' families a
#                     and b at once, with the long distances the rare ones; that was not built.
UNREACHED = """
Searched on the oracle and not reached by any case (no test claims them either way):
  * a stored block of more than 32 767 bytes, i.e. a second stored piece, and with it the `w1 <= w0` branch of the stored
    path (a piece of under four bytes).  At huffman_only a block is at most 31 744 bytes.  Tried with 16 custom
    CompressionOptions (max_hash_checks 1, 4, 16, 128 x greedy, lazy below 4, 32, 258): the Q13 inputs of
    test_stages_vs_oracle.q13_case (seeds 0..3), and 140 000 bytes of noise with 500, 1 500, 3 000 and 6 000 copies of
    length 3 and 4 from 2 049 to 32 000 back -- 192 streams.  The largest stored block covered 32 105 bytes (3 000 copies
    of length 3, max_hash_checks 4, greedy); whatever covered more came out dynamic.
  * a fixed block of more than 7 936 tokens (part > 0 of a fixed block).  Not searched again here: only a stream's last
    block or one cut off by a flush has fewer than 31 744 tokens, and over a full block the dynamic header is under 1 % of
    the bits, so the fixed code would have to be within that of the block's own optimum.  None of the 192 streams above
    had a fixed block of more than 7 936 tokens either."""


def Ts(seeds):
    return b"".join(T(s) for s in seeds)


@functools.lru_cache(maxsize=None)
def sync_chunk(r):
    """text that makes a dynamic block of r mod 8 bits (behind a sync marker a block starts at phase 0)"""
    for i in range(400):
        d = datagen.text_like(3000 + i, 900)
        blk = hc.decode(ob.encode(d, opts=ob.make_opts(*LV[H])))
        if len(blk) == 1 and blk[0]["btype"] == 2 and blk[0]["bit_end"] % 8 == r:
            return d
    raise AssertionError("no chunk of %d mod 8 bits" % r)


# ---- long tokens (a level with matches) ----------------------------------------------------------------------------------------------
LONG_NT = 2 * PQ + 300
# role -> [(token index in block 1, match length, least distance)].  One length code each (277..284).  The token the role is
# about gets length 227 (code 284, 5 extra bits) and the one distance code with 13 extra bits that nobody shares, so its
# distance code stays long: 35 bits.  (A distance must reach back into block 0: the later the token, the larger.)
LONG_PLAN = {
    "round": [(255, 67, 4097), (1023, 83, 6145), (4095, 227, 16385), (PQ, 131, 24577), (PQ + 255, 99, 8193), (2 * PQ, 163, 24577),
              (2 * PQ + 255, 115, 24577), (LONG_NT - 1, 195, 24577)],
    "part": [(255, 67, 4097), (1023, 83, 6145), (4095, 131, 8193), (PQ, 227, 16385), (PQ + 255, 99, 12289), (2 * PQ, 163, 24577),
             (2 * PQ + 255, 115, 24577), (LONG_NT - 1, 195, 24577)],
}


@functools.lru_cache(maxsize=None)
def _long_filler():
    """block 0: exactly 31 744 tokens over more than 32 768 bytes (so quirk Q1, a first block that fills inside the first
    window, stays out of it): short periodic matches first, then literals that never repeat a trigram -- the sources of
    block 1's long matches"""
    g = hc._Lz(4242, range(256))
    n = 0
    while n < B:
        if n < 1200:
            g.near(2, 4)
            n += 3
        else:
            g.lit()
            n += 1
    return g


@functools.lru_cache(maxsize=None)
def long_tokens(seed, role="round"):
    """Two blocks at a level with matches.  Block 1 has LONG_NT tokens: literals of 64 values, one token in five a match of
    length 4 at a distance of 2..4 (they make the distance codes 1..3 short and leave long codes for the rest), and at
    the token indices of LONG_PLAN[role] -- a part's first token, a wave's last, a round's last, the block's last -- a match
    of 67 to 227 bytes from 4 097 to 32 768 back.  The seed moves the literals and with them every token's bit."""
    import copy
    g = copy.deepcopy(_long_filler())
    g.r = random.Random(seed)
    g.alpha = list(hc.ALPHA64)
    n = 0
    for at, length, lo in LONG_PLAN[role]:
        while n < at - 1:
            d = g.r.randint(2, 4)  # (period 1 has 64 units in all: one per value)
            if g.r.random() < 0.4 and n + d + 1 <= at - 1:
                g.near(d, 4)
                n += d + 1
            else:
                g.lit()
                n += 1
        before = len(g.out)
        x = len(g.out) - len(_long_filler().out)  # (the source must lie in block 0's literals: nothing in block 1 is eligible)
        g.match(max(lo, x + 300), max(lo + 2047, x + 2300), length, tries=400)
        n += len(g.out) - before - length + 1  # (the literal in front, the match, and any literals match() had to add)
    return bytes(g.out)


def _stored_pair(i, j, v):
    """T, then the final stored block: payload offset i mod 4, end j mod 4, the bytes in the shared words all v"""
    n = 20000 + (j - i) % 4
    a = bytearray(R(100 + 4 * i + j, n))
    head = (4 - i) % 4
    a[:head] = bytes([v]) * head
    if j:
        a[-j:] = bytes([v]) * j
    return T(T_OB4[i]) + bytes(a)


def _table_of_cases():
    t = {}

    def add(name, make, claims, level=H, **kw):
        t[name] = dict(name=name, make=make, level=level, claims=set(claims), **kw)

    # -- plan: plain streams (the last block a few bytes short: exactly N blocks, no empty one behind them)
    #    (big: compared by bytes and block table only, never read by the Python inflate)
    for n in (1, 2, 64, 65):
        add("plain_%d" % n, lambda n=n: Ts(i % 24 for i in range(n))[:-7], [("plain", n)], big=n > 2)
    for n in (1024, 1025):
        add("plain_%d" % n, lambda n=n: (T(0) * n)[:-7], [("plain", n)], big=True)
    # -- plan: groups of blocks stored whatever the phase.  Group 0 is 63 blocks of noise and a block of text that ends at
    #    the phase wanted (it takes the serial path), group 1 is all noise
    tail = T(5)[:1000]
    add("stored_group_p0", lambda: R(1, 128 * B) + tail, [("stored_group", 0, "full")])
    for ph in range(1, 8):
        add("stored_group_p%d" % ph, lambda ph=ph: R(10 + ph, 63 * B) + T(T8[ph]) + R(20 + ph, 64 * B) + tail,
            [("stored_group", ph, "full"), ("stored_mixed", 0)])
    for ph, cnt in ((3, 1), (6, 1), (2, 63), (7, 63)):
        add("stored_group_p%d_cnt%d" % (ph, cnt),
            lambda ph=ph, cnt=cnt: R(30 + ph, 63 * B) + T(T8[ph]) + R(40 + ph, cnt * B - 1234),
            [("stored_group", ph, "cnt%d" % cnt), ("stored_final",)])
    add("stored_group_p5_final", lambda: R(35, 63 * B) + T(T8[5]) + R(45, 64 * B - 4321), [("stored_group", 5, "final_full"), ("stored_final",)])
    # -- plan: groups for the serial path
    add("mixed_stored_phases", lambda: R(50) + b"".join(T(T8[ph]) + R(50 + ph) for ph in range(1, 8)) + b"abc",
        [("stored_mixed", ph) for ph in range(8)] + [("stored_then", 2)])
    #    P_A stored at phase 3 and dynamic at 1, P_B dynamic at 2 and stored at 5, P_C stored at 0 and dynamic at 6, P_D at 4
    #    (dynamic); text and noise between them, a short fixed block last
    #    (a block of noise behind every dynamic P: whatever its length, what follows starts at phase 0)
    add("mixed_phase_dep", lambda: T(T8[3]) + P(*P_A) + T(T8[1]) + P(*P_A) + R(60) + T(T8[2]) + P(*P_B) + R(61) + T(T8[5]) + P(*P_B) +
        P(*P_C) + T(T8[6]) + P(*P_C) + R(62) + T(T8[4]) + P(*P_D) + R(63) + b"ab",
        [("phase_dep", 0, 3), ("phase_dep", 2, 1), ("phase_dep", 2, 2), ("phase_dep", 0, 5), ("phase_dep", 0, 0), ("phase_dep", 2, 6),
         ("phase_dep", 2, 4)], dep=(1, 3, 6, 9, 10, 12, 15))
    #    one P block in an otherwise plain stream: the workgroup path must refuse the piece.  P_A is dynamic at phase 0, the
    #    phase the workgroup path prices it at, and stored at 5
    #    (60 blocks: under the 2 MiB a batch item may have, so kb_plan meets them too)
    add("phase_in_big_stored", lambda: Ts([T8[0]] * 28 + [T8[5]]) + P(*P_A) + Ts([T8[0]] * 30)[:-7], [("phase_dep_big", 0)],
        dep=(29,), dep_big=True, big=True)
    add("phase_in_big_dynamic", lambda: Ts([T8[0]] * 29) + P(*P_A) + Ts([T8[0]] * 30)[:-7], [("phase_dep_big", 2)], dep=(29,), dep_big=True, big=True)
    # -- plan: sync markers, through the writer: a flush behind a dynamic block that ends at each phase, behind a fixed and a
    #    stored block
    def sync_data():
        parts = [sync_chunk(r) for r in range(8)] + [b"abc", R(70, 400), sync_chunk(3), sync_chunk(6), T(2)[:5000]]
        return b"".join(parts), tuple(np.cumsum([len(p) for p in parts[:-1]]).tolist())
    add("sync_phases", lambda: sync_data()[0], [("sync", ph) for ph in range(8)] + [("sync_after", ty) for ty in (0, 1, 2)],
        cuts=lambda: sync_data()[1], tail=True)
    # -- stored
    for i in range(4):
        for j in range(4):
            for v, tag in ((0, "z"), (255, "f")):
                claims = [("stored_align", i, j), ("stored_final",)]
                claims += [("stored_head", i, v)] if i else []
                claims += [("stored_tail", j, v)] if j else []
                add("stored_%d%d%s" % (i, j, tag), lambda i=i, j=j, v=v: _stored_pair(i, j, v), claims, tail=True)
    add("stored_then_dynamic", lambda: T(T_OB4[1]) + R(80) + T(7), [("stored_then", 2), ("stored_align", 1, 1)])
    add("stored_then_stored", lambda: T(T_OB4[3]) + R(81) + R(82), [("stored_then", 0), ("stored_align", 3, 3)])
    add("stored_then_fixed", lambda: T(T_OB4[2]) + R(83) + b"abc", [("stored_then", 1), ("stored_align", 2, 2)], tail=True)
    add("stored_smallest", lambda: T(T8[5]) + SMALLEST_BYTES, [("stored_len", SMALLEST_STORED), ("stored_final",)], tail=True)
    # -- tokens
    for seed, claims in TOKEN_SEEDS.items():
        add("tokens_T%d" % seed, lambda seed=seed: T(seed), claims + [("nt0",)])
    for (k, j), s in TINY_SEEDS.items():
        add("tiny_%d_%d" % (k, j), lambda k=k, j=j, s=s: datagen.text_like(k * PQ + j, 5000 + s), [("tiny_last_part", k, j)], tail=True)
    # -- headers
    add("hdr_258", lambda: norun_bytes(3), [("n_enc", 258)], tail=True)
    add("hdr_256", lambda: norun_bytes(3, run4=True), [("n_enc", 256)], tail=True)
    add("hdr_used6", lambda: hc.ties(128, 64, 0, 5), [("used_hclens", 6)], tail=True)
    add("hdr_used19", lambda: hc.fib_ll(20, 120), [("used_hclens", 19)], tail=True)
    # -- long tokens (seeds 0..99 of each plan tried: a 34-bit token must begin at bit 31 of a word, a 35-bit one at 30 or 31)
    add("long_round", lambda: long_tokens(23, "round"), [("long3", "wave_last"), ("long3", "round_last")], level="default", tail=True)
    add("long_part", lambda: long_tokens(56, "part"), [("long3", "part_first")], level="default", tail=True)
    add("long_last", lambda: long_tokens(74, "part"), [("long3", "block_last")], level="default", tail=True)
    add("hdr_257_rle", lambda: norun_bytes(3, 14, (3,), True), [("n_enc", 257)], level="rle", tail=True)
    add("hdr_260_rle", lambda: norun_bytes(3, 14, (3, 4)), [("n_enc", 260)], level="rle", tail=True)
    add("hdr_284_rle", lambda: norun_bytes(3, 14, RUNS_ALL_CODES), [("n_enc", N_ENC_MAX)], level="rle", tail=True)
    return t


_CASES = None


def names(level=None):
    global _CASES
    if _CASES is None:
        _CASES = _table_of_cases()
    return [n for n, c in _CASES.items() if level is None or c["level"] == level]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(name, data, level, claims, cuts, ...); a train's name is "train:<tail case>" (or "train:")"""
    if name.startswith("train:"):
        return train(name[6:])
    names()
    c = dict(_CASES[name])
    c["data"] = c.pop("make")()
    c["cuts"] = c["cuts"]() if "cuts" in c else ()
    return c


def levels():
    return sorted({c["level"] for c in (_CASES or names() and _CASES).values()})


# ---- trains ----------------------------------------------------------------------------------------------------------------------------
# A train is one input of 65 blocks or more, so that its call launches k_block_hist<256> and k_pack<256>: the body -- every
# huffman_only case made of whole blocks, then noise up to 65 blocks -- and behind it at most one case that ends with a
# partial block (only a stream's last block can be partial).  In front of every member stands one block of text, T32[r], that
# ends on a word boundary: the member begins at a bit that is 0 mod 32, as it does alone, so every offset mod 32 and mod 4
# its claims speak of is the same.  check_train() asserts the claims on the oracle's stream of the train.
BODY = ("tokens_T16", "tokens_T29", "tokens_T31", "tokens_T38", "tokens_T11", "tokens_T2", "tokens_T10", "stored_then_dynamic",
        "stored_then_stored", "mixed_stored_phases", "mixed_phase_dep")
TRAIN_BLOCKS = 65


def _bits_alone(c):
    """bits of a member's whole blocks when it starts at bit 0 (its partial last block, if any, left off)"""
    d = c["data"][:len(c["data"]) // B * B]
    if not d:
        return 0
    ob.encode(d, opts=ob.make_opts(*LV[H]))
    bl = ob.trace_blocks()
    assert bl[-1]["in_bytes"] == 0
    return bl[-1]["bit_start"]


@functools.lru_cache(maxsize=None)
def _body():
    """(bytes, [(name, first block, blocks)], bits)"""
    out, where, cur = bytearray(), [], 0
    for n in BODY:
        c = case(n)
        d = c["data"][:len(c["data"]) // B * B]  # (mixed_*: without their few last bytes, which the body cannot hold)
        if cur % 32:
            s = T32[-cur % 32]
            out += T(s)
            cur += t_len(s)
        assert cur % 32 == 0
        where.append((n, len(out) // B, len(d) // B))
        out += d
        cur += _bits_alone(c)
    pad = max(0, TRAIN_BLOCKS - len(out) // B)
    out += R(90, pad * B)
    cur = (cur + 7) // 8 * 8 + pad * 8 * (B + 5) if pad else cur
    return bytes(out), where, cur


def train(tail=""):
    body, where, cur = _body()
    out = bytearray(body)
    if tail:
        c = case(tail)
        assert c["level"] == H and not c["cuts"]
        if cur % 32:
            s = T32[-cur % 32]
            out += T(s)
        where = where + [(tail, len(out) // B, (len(c["data"]) + B - 1) // B)]
        out += c["data"]
    return dict(name="train:" + tail, data=bytes(out), level=H, claims=set(), members=where, cuts=())


def train_names():
    return ["train:"] + ["train:" + n for n in names(H) if _CASES[n].get("tail") and not _CASES[n].get("cuts")]


_BODY_FACTS = {}


def check_train(tr):
    """every member of a train begins on a word boundary and reaches its claims there; returns {member: cells}"""
    stream, table = oracle(tr["data"], tr["level"])
    got = {}
    for n, b0, nb in tr["members"]:
        assert table[b0]["bit_start"] % 32 == 0, "%s: member %s begins at bit %d" % (tr["name"], n, table[b0]["bit_start"])
        c = case(n)
        first = table[b0]["bit_start"]
        if n in BODY:  # (the body is the same in every train: its members are read once, for the same bits of the stream)
            key = (n, first, hash(stream[first // 8:table[b0 + nb]["bit_start"] // 8 + 1]))
            if key not in _BODY_FACTS:
                _BODY_FACTS[key] = facts(c, stream, None, model(stream, first, nb), whole=False)
            f = set(_BODY_FACTS[key])
        else:
            f = facts(c, stream, None, model(stream, first), whole=False)
        # (what facts() leaves to whole streams -- the serial path's stored blocks and the P blocks -- is looked up in the table below)
        claims = {x for x in c["claims"] if x[0] not in ("stored_mixed", "phase_dep", "plain", "stored_group")}
        if n in BODY:
            claims.discard(("nt0",))  # (the empty block behind a member that is whole blocks: only when it stands alone)
        for x in c["claims"]:
            if x[0] in ("stored_mixed", "phase_dep"):  # (type and phase from the table)
                want = 0 if x[0] == "stored_mixed" else x[1]
                hit = [b for b in table[b0:b0 + nb] if b["btype"] == want and b["bit_start"] % 8 == x[-1]]
                assert hit, "%s: member %s has no block for %s" % (tr["name"], n, x)
        missing = sorted(claims - f, key=str)
        assert not missing, "%s: member %s does not reach %s there" % (tr["name"], n, missing)
        got[n] = f
    assert len(table) * 4 > 256
    return got


# ---- an input for the piece-wise host path -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def streamed_input(n=(16 << 20) + 300000):
    """Just over 16 MiB for a level with matches ("fast"): a one-input call from host memory then plans and packs piece by
    piece (nbcum, the total_bits carried over, bit_base).  huffman_only never goes that way, so this is not one of the
    trains above and claims no cell: text first (the first block must not fill inside the first window: quirk Q1 would
    send the call back to the one-piece path), then text, noise, P-like noise and dyadic bytes in turns, so that the
    pieces' groups of 64 blocks hold stored blocks at whatever phase the text before them leaves."""
    out = bytearray(datagen.text_like(100000, 4000))
    k = 0
    while len(out) < n:
        out += R(200 + k, 70000 + 4 * k)
        out += datagen.text_like(150000 + k, 4001 + k)
        out += P(k % 5, 9000 + 31 * k)
        out += norun_bytes(3 + k % 3)
        out += datagen.text_like(100000, 4100 + k)
        k += 1
    return bytes(out[:n])
