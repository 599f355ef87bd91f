// inflate_check.h -- everything that decides whether a deflate stream is a valid encoding of a given input.
//
// The verify entry points (include/mi355_deflate.h mi355_deflate_verify*) answer the question of `gzip -t`: does this
// stream inflate to these bytes?  Because the expected output is known, nothing is ever written: a literal is right when it
// equals in[p], a match (len, dist) at p when in[p + i] == in[p + i - dist] for i < len, a stored piece when its bytes are
// the input's.  A stream is cut into entries -- restart points (bit offset, input offset), one per encoder block, or one for
// the whole stream -- and an entry is checked independently of the others.
//
// In the style of stages.h the decisions live here as host/device functions: the kernel (deflate_verify.inc, one wave per
// entry) and the host build of tests/inflcheck/ run the same text and differ only in the policy `P` that compares bytes
// (64 lanes at a time, or a plain loop).  Written from RFC 1950 / 1951 / 1952; the validity rules of a dynamic header are
// zlib's.  Nothing in here is a CPU path of the product: the product only ever runs the kernel.
//
// Safety: a corrupted stream is an ordinary input.  Every read of the stream goes through ic_load64 (zeros beyond the end;
// bits taken from there end the entry as TRUNCATED), every read of the input is preceded by a test against the entry's
// limit, every table index is masked to its table's size, and every loop has a bound that is fixed or the stream's length.
#ifndef MI355_INFLATE_CHECK_H
#define MI355_INFLATE_CHECK_H

#include <stdint.h>

#if defined(__HIPCC__)
#define MI355_IC __host__ __device__ inline
#else
#define MI355_IC inline
#endif

namespace mi355 {
namespace ic {

// MI355_VERIFY_* of the C ABI
enum : uint32_t {
    V_OK = 0, V_FRAME = 1, V_BTYPE = 2, V_STORED = 3, V_LENGTHS = 4, V_CODE = 5, V_DISTANCE = 6, V_MISMATCH = 7, V_LENGTH = 8,
    V_TABLE = 9, V_TRUNCATED = 10, V_TRAILER = 11, V_CHECKSUM = 12
};

constexpr uint32_t LL_BITS = 10, D_BITS = 9, CL_BITS = 7;  // index bits of the primary tables
constexpr uint32_t LIT_RUN = 64;                           // literals gathered for one compare
constexpr uint64_t FRAME_SCAN = 65536 + 32;                // a gzip header must end inside this many bytes
constexpr uint32_t NOCODE = 0xFFFFu;

// The decode tables of the current block (LDS of the workgroup; a stack object on the host).  A primary entry is
// symbol << 4 | code length, 0 where no code of at most the index's bits lives; cnt / sym are the canonical form
// (codes per length, symbols in code order) that the slow path walks a bit at a time.
struct Tables {
    uint16_t prim_ll[1u << LL_BITS];
    uint16_t prim_d[1u << D_BITS];  // (the code-length code borrows its first 128 entries while a header is read)
    uint16_t sym_ll[512];
    uint16_t sym_d[32];
    uint16_t sym_cl[32];
    uint16_t cnt_ll[16], cnt_d[16], cnt_cl[16];
    uint16_t offs[16], next[16];  // ic_build's running values
    uint16_t litbit[LIT_RUN];     // where a gathered literal's code began, in bits behind the first one's
    uint8_t lens[512];            // code lengths of a dynamic header (at most 286 + 30)
    uint8_t clens[32];
    uint8_t lit[LIT_RUN];
};  // 5120 bytes

// one entry: a restart point and where its blocks must end
struct Entry {
    uint64_t bit, pos;            // first header bit (raw deflate), first output byte
    uint64_t next_bit, next_pos;  // the next entry's, unless last
    uint32_t last, item;
};
struct Rec {
    uint32_t status, n_stored, n_fixed, n_dynamic;
    uint64_t bit, in_pos;         // the report's
    uint64_t end_bit, end_pos;    // where the entry's last block ended (OK only)
    uint64_t n_blocks;
};

// ---- the bounded reader ------------------------------------------------------------------------------------
MI355_IC uint64_t ic_load64(const uint8_t* s, uint64_t nbytes, uint64_t at) {
    if (at < nbytes && nbytes - at >= 8) {
        uint64_t v;
        __builtin_memcpy(&v, s + at, 8);
        return v;
    }
    uint64_t v = 0;
    for (uint32_t i = 0; i < 8; i++)
        if (at < nbytes && i < nbytes - at) v |= (uint64_t)s[at + i] << (8 * i);
    return v;
}
struct Bits {
    const uint8_t* s;
    uint64_t nbytes, end;  // end = 8 * nbytes
    uint64_t pos;
    uint32_t over;         // bits were taken from beyond the end
    // a window of 16 stream bytes kept in registers: loaded again only when the position has moved more than 8 bytes into it
    uint32_t wok;
    uint64_t wbyte, w0, w1;
};
MI355_IC Bits ic_bits(const uint8_t* s, uint64_t nbytes, uint64_t pos) { return Bits{s, nbytes, nbytes * 8, pos, 0u, 0u, 0, 0, 0}; }
// the next 57 bits at least (zeros beyond the end)
MI355_IC uint64_t ic_peek(Bits& b) {
    const uint64_t byte = b.pos >> 3;
    if (!b.wok || byte < b.wbyte || byte - b.wbyte > 8) {
        b.wok = 1, b.wbyte = byte;
        b.w0 = ic_load64(b.s, b.nbytes, byte);
        b.w1 = ic_load64(b.s, b.nbytes, byte + 8);
    }
    const uint32_t off = (uint32_t)(b.pos - 8 * b.wbyte);  // 0 .. 71: 128 - 71 = 57 bits are there
    if (off == 0) return b.w0;
    if (off < 64) return (b.w0 >> off) | (b.w1 << (64 - off));
    return b.w1 >> (off - 64);
}
MI355_IC void ic_skip(Bits& b, uint32_t n) {
    b.pos += n;
    if (b.pos > b.end) b.over = 1;
}
MI355_IC uint32_t ic_take(Bits& b, uint32_t n) {  // n <= 32
    const uint32_t v = (uint32_t)(ic_peek(b) & ((1ull << n) - 1));
    ic_skip(b, n);
    return v;
}

// ---- tables ------------------------------------------------------------------------------------------------
MI355_IC uint32_t ic_rev(uint32_t code, uint32_t len) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < 15; i++)
        if (i < len) r |= ((code >> i) & 1u) << (len - 1 - i);
    return r;
}
// canonical tables of lens[0..n): 0 = complete, 1 = over-subscribed, 2 = incomplete (the tables are usable all the same:
// bits that are no code decode to NOCODE).  Run by the leader alone.
MI355_IC uint32_t ic_build(Tables& t, const uint8_t* lens, uint32_t n, uint16_t* prim, uint32_t pbits, uint16_t* sym, uint32_t symmask,
                           uint16_t* cnt) {
    for (uint32_t l = 0; l < 16; l++) cnt[l] = 0;
    for (uint32_t i = 0; i < n; i++) cnt[lens[i & 511] & 15]++;
    cnt[0] = 0;
    int32_t left = 1;
    for (uint32_t l = 1; l < 16; l++) {
        left = left * 2 - (int32_t)cnt[l];
        if (left < 0) return 1;
    }
    uint32_t o = 0, code = 0;
    for (uint32_t l = 1; l < 16; l++) {
        code = (code + cnt[l - 1]) << 1;
        t.offs[l] = (uint16_t)o;
        t.next[l] = (uint16_t)code;
        o += cnt[l];
    }
    const uint32_t psize = 1u << pbits;
    for (uint32_t i = 0; i < psize; i++) prim[i] = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t l = lens[i & 511] & 15;
        if (!l) continue;
        sym[t.offs[l]++ & symmask] = (uint16_t)i;
        const uint32_t c = t.next[l]++;
        if (l > pbits) continue;
        for (uint32_t j = ic_rev(c, l) & (psize - 1); j < psize; j += 1u << l) prim[j] = (uint16_t)(i << 4 | l);
    }
    return left ? 2 : 0;
}
// the symbol whose code the low bits of w are, its length in `used`; NOCODE if they are no code of the set
template <class P>
MI355_IC uint32_t ic_decode(const uint16_t* prim, uint32_t pbits, const uint16_t* sym, uint32_t symmask, const uint16_t* cnt, uint64_t w,
                            uint32_t& used) {
    const uint32_t e = P::uni(prim[(uint32_t)w & ((1u << pbits) - 1)]);
    if (e & 15) {
        used = e & 15;
        return e >> 4;
    }
    uint32_t code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l < 16; l++) {  // (a code is read most significant bit first)
        code |= (uint32_t)(w >> (l - 1)) & 1u;
        const uint32_t c = P::uni(cnt[l]);
        if (code < first + c) {
            used = l;
            return P::uni(sym[(index + (code - first)) & symmask]);
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    used = 0;
    return NOCODE;
}
// bits that decoded to NOCODE with fewer than 15 of them inside the stream: could more bits have made a code?
MI355_IC bool ic_longer_code_exists(const uint16_t* cnt, uint64_t avail) {
    uint32_t any = 0;
    for (uint32_t l = 1; l < 16; l++)
        if (l > avail) any |= cnt[l];
    return any != 0;
}

// ---- the compares, as one lane of 64 sees them ---------------------------------------------------------------------
// The kernel compares bytes 64 lanes at a time; what ONE lane finds in a step is here, so that the host build can run the same
// arithmetic lane by lane (tests/inflcheck LaneOps).  A lane's answer is the index of its first differing byte or NONE; the
// indices rise with the lane, so the first lane with an answer has the step's.
constexpr uint32_t NONE = 0xFFFFFFFFu;
MI355_IC uint32_t ic_lane_lits(const uint8_t* lit, const uint8_t* in, uint32_t n, uint32_t lane) {
    return lane < n && lit[lane & (LIT_RUN - 1)] != in[lane] ? lane : NONE;
}
// a match, 64 bytes a step (dist <= p and p + len <= the limit: the caller's)
MI355_IC uint32_t ic_lane_match(const uint8_t* in, uint64_t p, uint32_t len, uint32_t dist, uint32_t base, uint32_t lane) {
    const uint32_t i = base + lane;
    return i < len && in[p + i] != in[p + i - dist] ? i : NONE;
}
// a stored piece of n <= 65535 bytes, eight bytes a lane, 512 a step
MI355_IC uint32_t ic_lane_run(const uint8_t* a, const uint8_t* b, uint32_t n, uint32_t base, uint32_t lane) {
    const uint32_t o = base + lane * 8;
    uint64_t x = 0;
    if (o < n && n - o >= 8) {
        uint64_t va, vb;
        __builtin_memcpy(&va, a + o, 8);
        __builtin_memcpy(&vb, b + o, 8);
        x = va ^ vb;
    } else {
        for (uint32_t k = 0; k < 8; k++)
            if (o < n && k < n - o) x |= (uint64_t)(uint8_t)(a[o + k] ^ b[o + k]) << (8 * k);
    }
    if (!x) return NONE;
    uint32_t k = 0;
    while (k < 7 && !((x >> (8 * k)) & 0xff)) k++;  // the lowest byte of x that is not zero
    return o + k;
}

struct Fail {
    uint32_t status;
    uint64_t bit, in_pos;
};
MI355_IC Fail ic_fail(uint32_t status, uint64_t bit, uint64_t in_pos) { return Fail{status, bit, in_pos}; }

// ---- dynamic header: HLIT, HDIST, HCLEN, the code-length code, the lengths, the two sets (RFC 1951 3.2.7) ------------
template <class P>
MI355_IC Fail ic_dynamic_header(Tables& t, Bits& b, uint64_t p) {
    const uint64_t sect = b.pos;  // the code-length section begins here
    const uint32_t nlen = ic_take(b, 5) + 257, ndist = ic_take(b, 5) + 1, ncl = ic_take(b, 4) + 4;
    if (b.over) return ic_fail(V_TRUNCATED, sect, p);
    if (nlen > 286 || ndist > 30) return ic_fail(V_LENGTHS, sect, p);
    uint32_t cl[19];
    for (uint32_t i = 0; i < 19; i++) cl[i] = i < ncl ? ic_take(b, 3) : 0;
    if (b.over) return ic_fail(V_TRUNCATED, sect, p);
    if (P::leader()) {
        // order of the code-length code's lengths: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
        t.clens[16] = (uint8_t)cl[0], t.clens[17] = (uint8_t)cl[1], t.clens[18] = (uint8_t)cl[2], t.clens[0] = (uint8_t)cl[3];
        for (uint32_t k = 0; k < 7; k++) {
            t.clens[8 + k] = (uint8_t)cl[4 + 2 * k];
            t.clens[7 - k] = (uint8_t)cl[5 + 2 * k];
        }
        t.clens[15] = (uint8_t)cl[18];
        t.offs[0] = (uint16_t)ic_build(t, t.clens, 19, t.prim_d, CL_BITS, t.sym_cl, 31, t.cnt_cl);
    }
    P::sync();
    if (P::uni(t.offs[0])) return ic_fail(V_LENGTHS, sect, p);  // the code-length code must be complete
    const uint32_t total = nlen + ndist;
    uint32_t i = 0, prev = 0;
    for (uint32_t guard = 0; guard < 320 && i < total; guard++) {
        uint32_t used;
        const uint64_t w = ic_peek(b);
        const uint32_t s = ic_decode<P>(t.prim_d, CL_BITS, t.sym_cl, 31, t.cnt_cl, w, used);
        if (s == NOCODE) return ic_fail(b.end - b.pos < 15 || b.pos > b.end ? V_TRUNCATED : V_LENGTHS, sect, p);
        uint32_t rep = 1, val = s;
        if (s == 16) {
            rep = 3 + ((uint32_t)(w >> used) & 3u), used += 2, val = prev;
        } else if (s == 17) {
            rep = 3 + ((uint32_t)(w >> used) & 7u), used += 3, val = 0;
        } else if (s == 18) {
            rep = 11 + ((uint32_t)(w >> used) & 127u), used += 7, val = 0;
        }
        ic_skip(b, used);
        if (b.over) return ic_fail(V_TRUNCATED, sect, p);
        if (s == 16 && i == 0) return ic_fail(V_LENGTHS, sect, p);   // nothing to repeat
        if (i + rep > total) return ic_fail(V_LENGTHS, sect, p);     // a repeat runs past HLIT + HDIST
        if (P::leader())
            for (uint32_t k = 0; k < 138; k++)
                if (k < rep) t.lens[(i + k) & 511] = (uint8_t)val;
        i += rep;
        prev = val;
    }
    if (P::leader()) {
        uint32_t bad = t.lens[256] == 0 ? 1u : 0u;  // no code for the end of the block
        const uint32_t rl = ic_build(t, t.lens, nlen, t.prim_ll, LL_BITS, t.sym_ll, 511, t.cnt_ll);
        // an incomplete set is legal only when it is one code of length 1
        uint32_t nl = 0, nd = 0;
        for (uint32_t l = 1; l < 16; l++) nl += t.cnt_ll[l];
        if (rl == 1 || (rl == 2 && !(nl == 1 && t.cnt_ll[1] == 1))) bad = 1;
        const uint32_t rd = ic_build(t, t.lens + nlen, ndist, t.prim_d, D_BITS, t.sym_d, 31, t.cnt_d);
        for (uint32_t l = 1; l < 16; l++) nd += t.cnt_d[l];
        if (rd == 1 || (rd == 2 && nd != 0 && !(nd == 1 && t.cnt_d[1] == 1))) bad = 1;  // (no distance code at all is legal)
        t.offs[0] = (uint16_t)bad;
    }
    P::sync();
    if (P::uni(t.offs[0])) return ic_fail(V_LENGTHS, sect, p);
    return ic_fail(V_OK, 0, 0);
}

// the fixed code (RFC 1951 3.2.6) as tables: 288 literal/length codes, 32 distance codes -- the symbols that are not in the
// alphabet (286, 287; 30, 31) decode and are refused as symbols
MI355_IC void ic_fixed_tables(Tables& t) {
    for (uint32_t i = 0; i < 288; i++) t.lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
    for (uint32_t i = 0; i < 32; i++) t.lens[288 + i] = 5;
    (void)ic_build(t, t.lens, 288, t.prim_ll, LL_BITS, t.sym_ll, 511, t.cnt_ll);
    (void)ic_build(t, t.lens + 288, 32, t.prim_d, D_BITS, t.sym_d, 31, t.cnt_d);
}

// the gathered literals against the input: MISMATCH at the first that differs
template <class P>
MI355_IC Fail ic_flush_lits(Tables& t, const uint8_t* in, uint64_t lit_p, uint64_t lit_bit, uint32_t& n_lit) {
    const uint32_t n = n_lit;
    n_lit = 0;
    if (!n) return ic_fail(V_OK, 0, 0);
    P::sync();
    const uint32_t d = P::first_diff_lits(t.lit, in + lit_p, n);
    P::sync();  // (the next gather writes t.lit again)
    if (d < n) return ic_fail(V_MISMATCH, lit_bit + P::uni(t.litbit[d & (LIT_RUN - 1)]), lit_p + d);
    return ic_fail(V_OK, 0, 0);
}

// ---- a match token, from its length symbol s (257..285) to a checked (len, dist): the text of ic_match_token.inc, which the
// three symbol loops include, as a function -- what the host test calls (tests/test_match_token_cases.py).  w: the bits from the
// token's first on, avail: how many of them are inside the stream; `used` comes in as the bits of s's code and goes out as the bits
// of the whole token.  Every failure is reported at (at, p).
template <class P>
MI355_IC Fail ic_match_token(const Tables& t, uint64_t w, uint32_t s, uint32_t& used, uint64_t avail, uint64_t at, uint64_t p,
                             uint32_t& len_out, uint32_t& dist_out) {
    Fail f = ic_fail(V_OK, 0, 0);
    do {
#include "ic_match_token.inc"
        len_out = len, dist_out = dist;
    } while (false);
    return f;
}

// ---- the symbols of one Huffman block, up to and including its end-of-block code --------------------------------------
// `limit`: the input offset no token of this entry may pass; `past`: the status of one that does (LENGTH / TABLE)
template <class P>
MI355_IC Fail ic_huffman_block(Tables& t, Bits& b, const uint8_t* in, uint64_t& p, uint64_t limit, uint32_t past) {
    uint32_t n_lit = 0;
    uint64_t lit_p = p, lit_bit = b.pos;
    Fail f = ic_fail(V_OK, 0, 0);
    bool done = false;
    for (uint64_t guard = 0; guard <= b.end && !done; guard++) {  // (a token takes a bit at least)
        const uint64_t at = b.pos;
        const uint64_t w = ic_peek(b);
        uint32_t used;
        const uint32_t s = ic_decode<P>(t.prim_ll, LL_BITS, t.sym_ll, 511, t.cnt_ll, w, used);
        const uint64_t avail = at < b.end ? b.end - at : 0;
        if (s == NOCODE) {
            f = ic_fail(avail < 15 && ic_longer_code_exists(t.cnt_ll, avail) ? V_TRUNCATED : V_CODE, at, p);
            break;
        }
        if (used > avail) {
            f = ic_fail(V_TRUNCATED, at, p);
            break;
        }
        if (s < 256) {  // a literal: gathered, compared LIT_RUN at a time
            if (p >= limit) {
                f = ic_fail(past, at, p);
                break;
            }
            if (!n_lit) lit_p = p, lit_bit = at;
            if (P::leader()) {
                t.lit[n_lit & (LIT_RUN - 1)] = (uint8_t)s;
                t.litbit[n_lit & (LIT_RUN - 1)] = (uint16_t)(at - lit_bit);
            }
            n_lit++, p++;
            ic_skip(b, used);
            if (n_lit == LIT_RUN) {
                f = ic_flush_lits<P>(t, in, lit_p, lit_bit, n_lit);
                if (f.status) return f;
            }
            continue;
        }
        if (s == 256) {
            ic_skip(b, used);
            done = true;
            break;
        }
        if (s >= 286) {
            f = ic_fail(V_CODE, at, p);
            break;
        }
#include "ic_match_token.inc"
        if (len > limit - p) {  // (p <= limit always)
            f = ic_fail(past, at, p);
            break;
        }
        f = ic_flush_lits<P>(t, in, lit_p, lit_bit, n_lit);
        if (f.status) return f;
        const uint32_t d = P::first_diff_match(in, p, len, dist);
        if (d < len) return ic_fail(V_MISMATCH, at, p + d);
        p += len;
        ic_skip(b, used);
    }
    // the literals gathered in front of the failing element, or of the block's end, come first in stream order
    const Fail g = ic_flush_lits<P>(t, in, lit_p, lit_bit, n_lit);
    if (g.status) return g;
    if (f.status) return f;
    if (!done) return ic_fail(V_TRUNCATED, b.pos, p);
    return ic_fail(V_OK, 0, 0);
}

// one stored piece: its header (pad to the byte, LEN, NLEN), LEN bytes
template <class P>
MI355_IC Fail ic_stored_block(Bits& b, const uint8_t* in, uint64_t& p, uint64_t limit, uint32_t past) {
#include "ic_stored_header.inc"
    if (len > limit - p) return ic_fail(past, at, p);
    const uint64_t d = P::first_diff_run(b.s + byte0, in + p, len);
    if (d < len) return ic_fail(V_MISMATCH, at, p + d);
    p += len;
    b.pos += 8ull * len;
    return ic_fail(V_OK, 0, 0);
}

// ---- one entry: its deflate blocks, up to the next entry's restart point or, the last one, through the BFINAL block ------
template <class P>
MI355_IC void ic_entry(Tables& t, const uint8_t* s, uint64_t nbytes, const uint8_t* in, uint64_t in_len, const Entry& e, Rec& r) {
    Bits b = ic_bits(s, nbytes, e.bit);
    uint64_t p = e.pos;
    const uint64_t limit = e.last ? in_len : e.next_pos;
    const uint32_t past = e.last ? V_LENGTH : V_TABLE;
    bool fixed_ready = false;
    Fail f = ic_fail(V_TRUNCATED, e.bit, p);
    r.n_blocks = 0, r.n_stored = r.n_fixed = r.n_dynamic = 0;
    if (p > limit || limit > in_len) f = ic_fail(V_TABLE, e.bit, p);  // (the host driver refuses such a table)
    else
        for (uint64_t guard = 0; guard <= b.end; guard++) {  // (a block takes three bits at least)
            const uint64_t at = b.pos;
            const uint32_t h = ic_take(b, 3);
            if (b.over) {
                f = ic_fail(V_TRUNCATED, at, p);
                break;
            }
            const uint32_t bfinal = h & 1, btype = h >> 1;
            if (bfinal && !e.last) {
                f = ic_fail(V_TABLE, at, p);
                break;
            }
            if (btype == 3) {
                f = ic_fail(V_BTYPE, at, p);
                break;
            }
            if (btype == 0) {
                f = ic_stored_block<P>(b, in, p, limit, past);
                r.n_stored++;
            } else {
                if (btype == 1) {
                    if (!fixed_ready) {
                        if (P::leader()) ic_fixed_tables(t);
                        P::sync();
                    }
                    fixed_ready = true;
                    r.n_fixed++;
                } else {
                    fixed_ready = false;
                    f = ic_dynamic_header<P>(t, b, p);
                    r.n_dynamic++;
                    if (f.status) break;
                }
                f = ic_huffman_block<P>(t, b, in, p, limit, past);
            }
            if (f.status) break;
            r.n_blocks++;
            if (e.last) {
                if (!bfinal) {
                    f = ic_fail(V_TRUNCATED, b.pos, p);  // (what is reported if the guard runs out)
                    continue;
                }
                if (p != in_len) f = ic_fail(V_LENGTH, b.pos, p);  // the BFINAL block ends before in_len
                break;
            }
            if (b.pos == e.next_bit && p == e.next_pos) break;
            if (b.pos > e.next_bit) {  // (p > next_pos is met as a token that passes the limit)
                f = ic_fail(V_TABLE, at, p);
                break;
            }
            f = ic_fail(V_TABLE, b.pos, p);  // (... if the guard runs out)
        }
    r.status = f.status;
    r.bit = f.status ? f.bit : 0;
    r.in_pos = f.status ? f.in_pos : 0;
    r.end_bit = b.pos;
    r.end_pos = p;
}

// ---- frames (RFC 1950, RFC 1952) -------------------------------------------------------------------------------------
// where the deflate data begins and how many trailer bytes follow it; false: FRAME
MI355_IC bool ic_parse_frame(const uint8_t* s, uint64_t n, uint32_t wrapper, uint64_t& hdr, uint64_t& trailer) {
    hdr = 0, trailer = 0;
    if (wrapper == 0) return true;
    if (wrapper == 1) {
        if (n < 6) return false;
        const uint32_t cmf = s[0], flg = s[1];
        if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 0x20)) return false;
        hdr = 2, trailer = 4;
        return true;
    }
    if (n < 18) return false;
    if (s[0] != 0x1f || s[1] != 0x8b || s[2] != 8 || (s[3] & 0xE0)) return false;
    const uint32_t flg = s[3];
    const uint64_t cap = n - 8 < FRAME_SCAN ? n - 8 : FRAME_SCAN;  // the header ends in front of the trailer
    uint64_t i = 10;
    if (flg & 4) {  // FEXTRA
        if (i + 2 > cap) return false;
        i += 2 + (s[i] | (uint64_t)s[i + 1] << 8);
        if (i > cap) return false;
    }
    for (uint32_t f = 8; f <= 16; f <<= 1) {  // FNAME, FCOMMENT: zero-terminated
        if (!(flg & f)) continue;
        bool end = false;
        for (uint64_t k = 0; k < FRAME_SCAN && i < cap && !end; k++) end = s[i++] == 0;
        if (!end) return false;
    }
    if (flg & 2) i += 2;  // FHCRC (skipped)
    if (i > cap) return false;
    hdr = i, trailer = 8;
    return true;
}

// Behind the last entry: the BFINAL block must end in the last byte in front of the trailer, and the trailer must hold the
// input's checksum (adler / crc: of the input, computed elsewhere).
MI355_IC Fail ic_trailer(const uint8_t* s, uint64_t n, uint64_t hdr, uint64_t trailer, uint32_t wrapper, uint64_t end_bit, uint64_t in_len,
                         uint32_t adler, uint32_t crc) {
    const uint64_t data = n - hdr - trailer;
    if ((end_bit + 7) / 8 != data) return ic_fail(V_TRAILER, end_bit, in_len);
    const uint8_t* t = s + hdr + data;
    if (wrapper == 1) {
        const uint32_t v = (uint32_t)t[0] << 24 | (uint32_t)t[1] << 16 | (uint32_t)t[2] << 8 | t[3];
        if (v != adler) return ic_fail(V_CHECKSUM, end_bit, in_len);
    }
    if (wrapper == 2) {
        const uint32_t v = (uint32_t)t[3] << 24 | (uint32_t)t[2] << 16 | (uint32_t)t[1] << 8 | t[0];
        const uint32_t z = (uint32_t)t[7] << 24 | (uint32_t)t[6] << 16 | (uint32_t)t[5] << 8 | t[4];
        if (v != crc || z != (uint32_t)in_len) return ic_fail(V_CHECKSUM, end_bit, in_len);
    }
    return ic_fail(V_OK, 0, 0);
}

// one entry of one framed stream: what a workgroup of the kernel, and a turn of the host loop, does
template <class P>
MI355_IC void ic_verify_entry(Tables& t, const uint8_t* stream, uint64_t stream_len, const uint8_t* in, uint64_t in_len, uint32_t wrapper,
                              uint32_t adler, uint32_t crc, const Entry& e, Rec& r) {
    uint64_t hdr, trailer;
    r = Rec{V_FRAME, 0, 0, 0, 0, 0, 0, 0, 0};
    if (!ic_parse_frame(stream, stream_len, wrapper, hdr, trailer)) return;
    ic_entry<P>(t, stream + hdr, stream_len - hdr - trailer, in, in_len, e, r);
    if (r.status || !e.last) return;
    const Fail f = ic_trailer(stream, stream_len, hdr, trailer, wrapper, r.end_bit, in_len, adler, crc);
    r.status = f.status, r.bit = f.bit, r.in_pos = f.in_pos;
}

// ---- host side of both builds: the entries of a table, and the report from the entries' records ------------------------
// (bit_start non-decreasing and sum in_bytes == in_len are the caller's to check)
template <class GetBit, class GetBytes>
inline void ic_make_entries(GetBit bit_start, GetBytes in_bytes, uint64_t n, uint32_t item, Entry* out /* max(n, 1) */) {
    if (n == 0) {
        out[0] = Entry{0, 0, 0, 0, 1u, item};
        return;
    }
    uint64_t pos = 0;
    for (uint64_t k = 0; k < n; k++) {
        out[k].bit = bit_start(k), out[k].pos = pos;
        pos += in_bytes(k);
        out[k].last = k + 1 == n, out[k].item = item;
        out[k].next_bit = k + 1 < n ? bit_start(k + 1) : 0, out[k].next_pos = k + 1 < n ? pos : 0;
    }
}
// FRAME first (every record of the stream carries it), then the failing entry with the smallest index; TRAILER and CHECKSUM
// can only come from the last entry, which is clean otherwise.  R: mi355_verify_report.
template <class R>
inline void ic_report(const Rec* recs, uint64_t n, R& rep) {
    rep.status = V_OK, rep.entry = 0, rep.bit = 0, rep.in_pos = 0, rep.n_blocks = 0, rep.n_stored = rep.n_fixed = rep.n_dynamic = 0;
    for (uint64_t k = 0; k < n; k++)
        if (recs[k].status) {
            rep.status = recs[k].status, rep.entry = (uint32_t)k, rep.bit = recs[k].bit, rep.in_pos = recs[k].in_pos;
            return;
        }
    for (uint64_t k = 0; k < n; k++) {
        rep.n_blocks += recs[k].n_blocks;
        rep.n_stored += recs[k].n_stored, rep.n_fixed += recs[k].n_fixed, rep.n_dynamic += recs[k].n_dynamic;
    }
}
inline const char* ic_status_name(uint32_t s) {
    static const char* const names[13] = {"ok", "frame", "btype", "stored", "lengths", "code", "distance", "mismatch", "length",
                                          "table", "truncated", "trailer", "checksum"};
    return s < 13 ? names[s] : "?";
}

}  // namespace ic
}  // namespace mi355
#endif
