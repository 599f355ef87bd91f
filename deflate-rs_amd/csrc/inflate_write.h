// inflate_write.h -- the write side of inflate_check.h: decode a raw / zlib / gzip deflate stream to its bytes.
//
// The inflate entry points (include/mi355_deflate.h mi355_inflate*) run this text: the kernel (deflate_inflate.inc k_inflate, one
// wave per stream) and the host build of tests/inflwrite/.  The bit reader, the tables, the dynamic-header rules and the frame
// parsers are inflate_check.h's, and so is everything of a token and of a stored piece that has no sink in it: the text of
// ic_match_token.inc (a length symbol to a checked (len, dist)) and of ic_stored_header.inc (pad, LEN, NLEN) is included here, not
// written again.  What is here is a SIBLING of its symbol loop, stored piece and block loop in which a sink stands where verify has a
// compare: a literal, a match or a stored piece is written, and a match reads what the same wave wrote a moment ago.  (Siblings
// around the shared text and not one loop with two sinks: what verify does with a token, and with it its reports and its kernel's
// code, stays what it was.)  The policy `P` adds to verify's leader / sync / uni:
//   store_lits  the gathered literals, lane i writing byte lit_p + i
//   copy_match  64 bytes a step; byte i of a match (len, dist) at p is out[p - dist + i % dist]: a source index below p whatever
//               dist is, so no step of a match reads what an earlier step of it wrote and an overlapping match needs no serial loop
//   copy_run    a stored piece from the stream, byte-wise up to the destination's first 8-byte boundary, then eight bytes a lane
//   fence       stores of this wave issued so far become loadable by its other lanes (workgroup scope)
//
// Safety, as in inflate_check.h: every stream read goes through the bounded reader (a stored piece is tested against the stream's
// length first), every table index is masked, every loop is bounded, and every output index is tested against `cap` before use:
// no store lands at an index >= cap, and no load of the output happens at an index >= min(p, cap).  Past `cap` the decode goes on
// counting -- p advances, nothing is stored or loaded -- so that the exact size comes out.
#ifndef MI355_INFLATE_WRITE_H
#define MI355_INFLATE_WRITE_H

#include "inflate_check.h"

namespace mi355 {
namespace iw {

using namespace ic;

// where the bytes go; vis: every store at an index below it has been fenced (the same in all lanes)
struct Sink {
    uint8_t* out;
    uint64_t cap, vis;
};
// what the decode of one stream leaves (TRAILER included; CHECKSUM is judged afterwards, iw_check_trailer)
struct Rec {
    uint32_t status, n_stored, n_fixed, n_dynamic;
    uint64_t bit, out_pos;  // the failing element's; OK: 0 and out_len
    uint64_t out_len;       // OK only: the bytes the stream inflates to, whatever cap is
    uint64_t end_bit;       // OK only: where the BFINAL block ended
    uint64_t n_blocks;
};  // 56 bytes

// ---- the writes, as one lane of 64 sees them (the host build replays them lane by lane: tests/inflwrite LaneSink) -----------
MI355_IC void iw_lane_lits(const uint8_t* lit, uint8_t* out, uint64_t cap, uint64_t lit_p, uint32_t n, uint32_t lane) {
    if (lane < n && lit_p + lane < cap) out[lit_p + lane] = lit[lane & (LIT_RUN - 1)];
}
// the source of byte i of a match: below p for every i (dist >= 1, dist <= p: the caller's)
MI355_IC uint64_t iw_match_src(uint64_t p, uint32_t dist, uint32_t i) { return p - dist + (i < dist ? i : i % dist); }
MI355_IC void iw_lane_match(uint8_t* out, uint64_t cap, uint64_t p, uint32_t len, uint32_t dist, uint32_t base, uint32_t lane) {
    const uint32_t i = base + lane;
    if (i < len && p + i < cap) out[p + i] = out[iw_match_src(p, dist, i)];  // (p + i < cap: the source is below min(p, cap))
}
// a stored piece of n <= 65535 bytes to out[p ..]: `head` bytes up to the destination's first 8-byte boundary, one a lane ...
MI355_IC uint32_t iw_run_head(const uint8_t* out, uint64_t p, uint32_t n) {
    const uint32_t h = (uint32_t)((0 - ((uintptr_t)out + p)) & 7);
    return h < n ? h : n;
}
MI355_IC void iw_lane_run_head(const uint8_t* src, uint8_t* out, uint64_t cap, uint64_t p, uint32_t head, uint32_t lane) {
    if (lane < head && p + lane < cap) out[p + lane] = src[lane];
}
// ... then eight bytes a lane, 512 a step; the lane that holds the piece's end, or the byte at cap, goes byte by byte
MI355_IC void iw_lane_run(const uint8_t* src, uint8_t* out, uint64_t cap, uint64_t p, uint32_t n, uint32_t head, uint32_t base, uint32_t lane) {
    const uint32_t o = head + base + lane * 8;
    if (o >= n) return;
    if (n - o >= 8 && p + o < cap && cap - (p + o) >= 8) {
        uint64_t v;
        __builtin_memcpy(&v, src + o, 8);
        __builtin_memcpy(__builtin_assume_aligned(out + p + o, 8), &v, 8);
        return;
    }
    for (uint32_t k = 0; k < 8; k++)
        if (k < n - o && p + o + k < cap) out[p + o + k] = src[o + k];
}

// the gathered literals to out[lit_p ..]
template <class P>
MI355_IC void iw_flush_lits(Tables& t, Sink& o, uint64_t lit_p, uint32_t& n_lit) {
    const uint32_t n = n_lit;
    n_lit = 0;
    if (!n) return;
    P::sync();
    if (lit_p < o.cap) P::store_lits(t.lit, o.out, o.cap, lit_p, n);
    P::sync();  // (the next gather writes t.lit again)
}

// ---- the symbols of one Huffman block, up to and including its end-of-block code (sibling of ic_huffman_block) ---------------
template <class P>
MI355_IC Fail iw_huffman_block(Tables& t, Bits& b, Sink& o, uint64_t& p) {
    uint32_t n_lit = 0;
    uint64_t lit_p = p;
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
        if (s < 256) {  // a literal: gathered, stored LIT_RUN at a time
            if (!n_lit) lit_p = p;
            if (P::leader()) t.lit[n_lit & (LIT_RUN - 1)] = (uint8_t)s;
            n_lit++, p++;
            ic_skip(b, used);
            if (n_lit == LIT_RUN) iw_flush_lits<P>(t, o, lit_p, n_lit);
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
        iw_flush_lits<P>(t, o, lit_p, n_lit);  // the match may source from them
        if (p < o.cap) {
            // the bytes it loads: [p - dist, p - dist + min(len, dist)).  Stores behind the last fence are not loadable yet.
            const uint64_t need = p - dist + (len < dist ? len : dist);
            if (need > o.vis) {
                P::fence(p);
                o.vis = p;
            }
            P::copy_match(o.out, o.cap, p, len, dist);
        }
        p += len;
        ic_skip(b, used);
    }
    // the literals gathered in front of the failing element, or of the block's end, are written before it is reported
    iw_flush_lits<P>(t, o, lit_p, n_lit);
    if (f.status) return f;
    if (!done) return ic_fail(V_TRUNCATED, b.pos, p);
    return ic_fail(V_OK, 0, 0);
}

// one stored piece: its header, LEN bytes (sibling of ic_stored_block)
template <class P>
MI355_IC Fail iw_stored_block(Bits& b, Sink& o, uint64_t& p) {
#include "ic_stored_header.inc"
    if (len && p < o.cap) P::copy_run(b.s + byte0, o.out, o.cap, p, len);
    p += len;
    b.pos += 8ull * len;
    return ic_fail(V_OK, 0, 0);
}

// ---- one framed stream: its frame, its deflate blocks through the BFINAL block, the place of its trailer ----------------------
template <class P>
MI355_IC void iw_inflate(Tables& t, const uint8_t* stream, uint64_t stream_len, uint32_t wrapper, uint8_t* out, uint64_t cap, Rec& r) {
    r = Rec{V_FRAME, 0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t hdr, trailer;
    if (!ic_parse_frame(stream, stream_len, wrapper, hdr, trailer)) return;
    Bits b = ic_bits(stream + hdr, stream_len - hdr - trailer, 0);
    Sink o{out, cap, 0};
    uint64_t p = 0;
    bool fixed_ready = false;
    Fail f = ic_fail(V_TRUNCATED, 0, 0);
    for (uint64_t guard = 0; guard <= b.end; guard++) {  // (a block takes three bits at least)
        const uint64_t at = b.pos;
        const uint32_t h = ic_take(b, 3);
        if (b.over) {
            f = ic_fail(V_TRUNCATED, at, p);
            break;
        }
        const uint32_t bfinal = h & 1, btype = h >> 1;
        if (btype == 3) {
            f = ic_fail(V_BTYPE, at, p);
            break;
        }
        if (btype == 0) {
            f = iw_stored_block<P>(b, o, p);
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
            f = iw_huffman_block<P>(t, b, o, p);
        }
        if (f.status) break;
        r.n_blocks++;
        if (!bfinal) {
            f = ic_fail(V_TRUNCATED, b.pos, p);  // (what is reported if the guard runs out)
            continue;
        }
        // the BFINAL block must end in the last byte in front of the trailer (no checksum is compared here: wrapper 0)
        f = ic_trailer(stream, stream_len, hdr, trailer, 0u, b.pos, p, 0u, 0u);
        break;
    }
    r.status = f.status;
    r.bit = f.status ? f.bit : 0;
    r.out_pos = f.status ? f.in_pos : p;
    r.out_len = f.status ? 0 : p;
    r.end_bit = f.status ? 0 : b.pos;
    if (f.status) r.n_blocks = 0, r.n_stored = r.n_fixed = r.n_dynamic = 0;
}

// After the decode, for a framed stream that is clean and fits: the trailer against the checksums of the OUTPUT (adler / crc: of
// out[0, out_len), computed elsewhere).  CHECKSUM where Adler-32, or CRC-32 or ISIZE, disagree.
MI355_IC void iw_check_trailer(const uint8_t* stream, uint64_t stream_len, uint32_t wrapper, uint32_t adler, uint32_t crc, Rec& r) {
    uint64_t hdr, trailer;
    if (r.status || !wrapper || !ic_parse_frame(stream, stream_len, wrapper, hdr, trailer)) return;
    const Fail f = ic_trailer(stream, stream_len, hdr, trailer, wrapper, r.end_bit, r.out_len, adler, crc);
    if (!f.status) return;
    r.status = f.status, r.bit = f.bit, r.out_pos = f.in_pos;
    r.out_len = 0, r.end_bit = 0, r.n_blocks = 0, r.n_stored = r.n_fixed = r.n_dynamic = 0;
}
// is the checksum of this record's stream judged?  (structurally valid, framed, and all of it stored)
MI355_IC bool iw_judged(const Rec& r, uint32_t wrapper, uint64_t cap) { return !r.status && wrapper && r.out_len <= cap; }

// ---- host side of both builds: the report and the return value from a stream's record ------------------------------------------
enum : int { IW_OK = 0, IW_DATA = 1, IW_TOO_SMALL = 2 };
// R: mi355_inflate_report.  *valid: the bytes of `out` that hold data (out_len; cap; the bytes in front of the failure)
template <class R>
inline int iw_report(const Rec& rec, uint64_t cap, R& rep, uint64_t* valid) {
    rep.status = rec.status, rep.reserved = 0, rep.bit = rec.bit, rep.out_pos = rec.out_pos, rep.out_len = rec.out_len;
    rep.n_blocks = rec.n_blocks, rep.n_stored = rec.n_stored, rep.n_fixed = rec.n_fixed, rep.n_dynamic = rec.n_dynamic;
    rep.ms = 0;
    if (rec.status) {
        *valid = rec.out_pos < cap ? rec.out_pos : cap;
        return IW_DATA;
    }
    *valid = rec.out_len < cap ? rec.out_len : cap;
    return rec.out_len > cap ? IW_TOO_SMALL : IW_OK;
}

}  // namespace iw
}  // namespace mi355
#endif
