// inflate_stream.h -- inflate_write.h for a stream that arrives in pieces: decode from a given bit with up to 32 KiB of history in
// front of the output, and stop cleanly where the input runs out.
//
// The stream handles (include/mi355_deflate.h mi355_inflate_stream_*) run this text: the kernel (deflate_stream_inflate.inc
// k_inflate_resume, one wave per handle) and the host build of tests/inflstream/.  The bit reader, the tables, the dynamic header,
// the text of a match token and of a stored header are inflate_check.h's, the lane writes of literals and of a stored piece are
// inflate_write.h's.  What is here is a SIBLING of iw_inflate's block loop, symbol loop and stored piece in which
//   the output is the virtual buffer  hist ++ out : position p starts at hist_len, so ic_match_token.inc's `dist > p` is exactly
//       "further back than history plus bytes produced"; a match's source index below hist_len loads from hist, else from out --
//       a select per lane, so a source run may straddle the seam, with len > dist too (iw_match_src holds over the virtual index);
//   the end of the input is no failure : a V_TRUNCATED from any element leaves the record PENDING at the COMMIT POINT, the end of
//       the last complete block that is not BFINAL and whose bytes fit; what the partial block stored behind it is scratch;
//   the wave leaves the next history   : the last min(32768, hist_len + committed) bytes of hist ++ out[0, committed) in hist_next,
//       the other half of a ping-pong pair (hist_next and hist never alias), in the same launch.
// The policy `P` adds to inflate_write.h's:
//   copy_match_h  copy_match with the history select
//   copy_hist     the next history, eight bytes a lane where all eight come from one side of the seam
//
// Safety, as in inflate_write.h: every stream read goes through the bounded reader, every table index is masked, every loop is
// bounded; no store lands in out at an index >= cap, no load of out happens at an index >= min(p - hist_len, cap), no load of hist
// at an index >= hist_len, and hist_next gets exactly the bytes counted in the record.  Past `cap` the decode goes on counting.
#ifndef MI355_INFLATE_STREAM_H
#define MI355_INFLATE_STREAM_H

#include "inflate_write.h"

namespace mi355 {
namespace ist {

using namespace iw;

constexpr uint32_t HIST = 32768;
enum : uint32_t { FP_NEED_MORE = 0, FP_BAD = 1, FP_OK = 2 };       // is_frame_prefix
enum : uint32_t { S_PENDING = 0, S_DONE = 1, S_FAILED = 2 };    // Rec2::state

// what one handle brings to one write
struct Resume {
    const uint8_t* s;    // its pending compressed bytes: everything from the byte that holds the commit bit (frame_open: from the
    uint64_t nbytes;     //   frame's first byte)
    uint64_t bit;        // where to start in them (0..7; frame_open: ignored, the decode starts behind the header)
    uint64_t bit_base, out_base;  // the absolute raw-deflate bit of s's first bit and output position of out[0], for reports
    const uint8_t* hist;
    uint8_t* hist_next;
    uint8_t* out;
    uint64_t cap;
    uint32_t hist_len;   // <= HIST
    uint32_t wrapper;
    uint32_t frame_open; // the frame header has not been passed yet: is_frame_prefix first
    uint32_t skip;       // the handle takes no part in this launch (batch: an item left alone); the record is untouched
    uint32_t fin;        // no more input will come: what cannot be completed is a failure (FRAME / TRUNCATED), reported where it begins
    uint32_t pad;
};  // 96 bytes

// what the wave leaves
struct Rec2 {
    uint32_t state, status;   // S_*; FAILED: V_*
    uint64_t bit, out_pos;    // FAILED: the failing element's, absolute.  DONE: where the BFINAL block ended, and the stream's length
    uint64_t commit_bit;      // PENDING, DONE: the commit point, in bits from the first bit of the DEFLATE data in s (behind hdr_len)
    uint64_t committed;       // ... and the bytes of out in front of it.  FAILED: the bytes of out that hold data (<= cap)
    uint64_t need_out;        // 0, or the end of the first uncommitted block that is complete but ends beyond cap: the room that suffices
    uint32_t hist_next_len;   // PENDING, DONE: the bytes hist_next holds
    uint32_t hdr_len;         // frame_open and the header complete: its bytes (else 0)
    uint32_t frame;           // frame_open: what is_frame_prefix said (F_*); else FP_OK
    uint32_t n_blocks;        // the blocks in front of the commit point
    uint8_t trailer[8];       // DONE: the 4 (zlib) or 8 (gzip) bytes behind the BFINAL block
};  // 72 bytes

// ---- the frame header of a stream that may not be all there yet (rules: ic_parse_frame's) ------------------------------------
// every test reads only bytes below n; a header that is wrong in the bytes that ARE there is BAD at once
MI355_IC uint32_t is_frame_prefix(const uint8_t* s, uint64_t n, uint32_t wrapper, uint64_t& hdr_len) {
    hdr_len = 0;
    if (wrapper == 0) return FP_OK;
    if (wrapper == 1) {
        if (n >= 1 && ((s[0] & 15) != 8 || (s[0] >> 4) > 7)) return FP_BAD;
        if (n < 2) return FP_NEED_MORE;
        if ((((uint32_t)s[0] << 8) | s[1]) % 31 != 0 || (s[1] & 0x20)) return FP_BAD;
        hdr_len = 2;
        return FP_OK;
    }
    if (wrapper != 2) return FP_BAD;
    if ((n >= 1 && s[0] != 0x1f) || (n >= 2 && s[1] != 0x8b) || (n >= 3 && s[2] != 8) || (n >= 4 && (s[3] & 0xE0))) return FP_BAD;
    if (n < 10) return FP_NEED_MORE;
    const uint32_t flg = s[3];
    uint64_t i = 10;
    if (flg & 4) {  // FEXTRA
        if (i + 2 > n) return FP_NEED_MORE;
        i += 2 + (s[i] | (uint64_t)s[i + 1] << 8);
        if (i > FRAME_SCAN) return FP_BAD;
        if (i > n) return FP_NEED_MORE;
    }
    for (uint32_t f = 8; f <= 16; f <<= 1) {  // FNAME, FCOMMENT: zero-terminated
        if (!(flg & f)) continue;
        bool end = false;
        for (uint64_t k = 0; k < FRAME_SCAN && i < n && i < FRAME_SCAN && !end; k++) end = s[i++] == 0;
        if (!end) return i >= FRAME_SCAN ? FP_BAD : FP_NEED_MORE;
    }
    if (flg & 2) i += 2;  // FHCRC (skipped)
    if (i > FRAME_SCAN) return FP_BAD;
    if (i > n) return FP_NEED_MORE;
    hdr_len = i;
    return FP_OK;
}

// ---- the writes, as one lane of 64 sees them ----------------------------------------------------------------------------------
// where the virtual buffer's byte v lies (v < hist_len + the bytes of out that hold data: the caller's)
MI355_IC const uint8_t* is_src(const uint8_t* hist, uint64_t hist_len, const uint8_t* out, uint64_t v) {
    return v < hist_len ? hist + v : out + (v - hist_len);
}
// iw_lane_match over the virtual buffer; p, vcap: virtual (vcap = hist_len + cap), p >= hist_len
MI355_IC void is_lane_match(const uint8_t* hist, uint64_t hist_len, uint8_t* out, uint64_t vcap, uint64_t p, uint32_t len, uint32_t dist,
                            uint32_t base, uint32_t lane) {
    const uint32_t i = base + lane;
    if (i < len && p + i < vcap) out[p + i - hist_len] = *is_src(hist, hist_len, out, iw_match_src(p, dist, i));
}
// the next history: byte j of it is the virtual buffer's byte from + j, j < n; eight a lane, 512 a step
MI355_IC void is_lane_hist(const uint8_t* hist, uint64_t hist_len, const uint8_t* out, uint8_t* hist_next, uint64_t from, uint32_t n,
                           uint32_t base, uint32_t lane) {
    const uint32_t j = base + lane * 8;
    if (j >= n) return;
    const uint64_t v = from + j;
    if (n - j >= 8 && (v + 8 <= hist_len || v >= hist_len)) {  // all eight on one side of the seam (hist_next is 8-byte aligned)
        uint64_t w;
        __builtin_memcpy(&w, is_src(hist, hist_len, out, v), 8);
        __builtin_memcpy(__builtin_assume_aligned(hist_next + j, 8), &w, 8);
        return;
    }
    for (uint32_t k = 0; k < 8; k++)
        if (k < n - j) hist_next[j + k] = *is_src(hist, hist_len, out, v + k);
}

// where the bytes go, in virtual positions; vis: every store below it has been fenced (the history was, by the launch that wrote it)
struct HSink {
    const uint8_t* hist;
    uint64_t hist_len;
    uint8_t* out;
    uint64_t cap, vcap, vis;
};

template <class P>
MI355_IC void is_flush_lits(Tables& t, HSink& o, uint64_t lit_p, uint32_t& n_lit) {
    const uint32_t n = n_lit;
    n_lit = 0;
    if (!n) return;
    P::sync();
    if (lit_p < o.vcap) P::store_lits(t.lit, o.out, o.cap, lit_p - o.hist_len, n);
    P::sync();  // (the next gather writes t.lit again)
}

// ---- the symbols of one Huffman block (sibling of iw_huffman_block) -------------------------------------------------------------
template <class P>
MI355_IC Fail is_huffman_block(Tables& t, Bits& b, HSink& o, uint64_t& p) {
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
        if (s < 256) {
            if (!n_lit) lit_p = p;
            if (P::leader()) t.lit[n_lit & (LIT_RUN - 1)] = (uint8_t)s;
            n_lit++, p++;
            ic_skip(b, used);
            if (n_lit == LIT_RUN) is_flush_lits<P>(t, o, lit_p, n_lit);
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
        is_flush_lits<P>(t, o, lit_p, n_lit);  // the match may source from them
        if (p < o.vcap) {
            // the bytes it loads: [p - dist, p - dist + min(len, dist)); those of out behind the last fence are not loadable yet
            const uint64_t need = p - dist + (len < dist ? len : dist);
            if (need > o.vis) {
                P::fence(p);
                o.vis = p;
            }
            P::copy_match_h(o.hist, o.hist_len, o.out, o.vcap, p, len, dist);
        }
        p += len;
        ic_skip(b, used);
    }
    is_flush_lits<P>(t, o, lit_p, n_lit);
    if (f.status) return f;
    if (!done) return ic_fail(V_TRUNCATED, b.pos, p);
    return ic_fail(V_OK, 0, 0);
}

// one stored piece (sibling of iw_stored_block)
template <class P>
MI355_IC Fail is_stored_block(Bits& b, HSink& o, uint64_t& p) {
#include "ic_stored_header.inc"
    if (len && p < o.vcap) P::copy_run(b.s + byte0, o.out, o.cap, p - o.hist_len, len);
    p += len;
    b.pos += 8ull * len;
    return ic_fail(V_OK, 0, 0);
}

// ---- one write of one handle: from the commit point through every block that is complete ---------------------------------------
template <class P>
MI355_IC void is_resume(Tables& t, const Resume& q, Rec2& r) {
    r = Rec2{S_PENDING, V_OK, 0, 0, 0, 0, 0, q.hist_len, 0, FP_OK, 0, {0, 0, 0, 0, 0, 0, 0, 0}};
    const uint8_t* s = q.s;
    uint64_t nbytes = q.nbytes, bit0 = q.bit;
    const uint64_t H = q.hist_len <= HIST ? q.hist_len : HIST;
    if (q.frame_open) {
        uint64_t hdr;
        r.frame = is_frame_prefix(s, nbytes, q.wrapper, hdr);
        if (r.frame == FP_BAD || (r.frame == FP_NEED_MORE && q.fin)) {
            r.state = S_FAILED, r.status = V_FRAME, r.bit = q.bit_base, r.out_pos = q.out_base;
            return;
        }
        if (r.frame == FP_NEED_MORE) hdr = nbytes;  // (nothing to decode: the history is copied, the record stays PENDING at 0)
        else r.hdr_len = (uint32_t)hdr;
        s += hdr, nbytes -= hdr, bit0 = 0;
    }
    Bits b = ic_bits(s, nbytes, bit0);
    HSink o{q.hist, H, q.out, q.cap, H + q.cap, H};
    uint64_t p = H, c_bit = bit0, c_p = H;
    uint32_t c_blocks = 0, n_blocks = 0;
    bool fixed_ready = false, finished = false;
    Fail f = ic_fail(V_TRUNCATED, bit0, p);
    for (uint64_t guard = 0; guard <= b.end && !(q.frame_open && r.frame != FP_OK); guard++) {  // (a block takes three bits at least)
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
            f = is_stored_block<P>(b, o, p);
        } else {
            if (btype == 1) {
                if (!fixed_ready) {
                    if (P::leader()) ic_fixed_tables(t);
                    P::sync();
                }
                fixed_ready = true;
            } else {
                fixed_ready = false;
                f = ic_dynamic_header<P>(t, b, p);
                if (f.status) break;
            }
            f = is_huffman_block<P>(t, b, o, p);
        }
        if (f.status) break;
        n_blocks++;
        if (p - H > q.cap && !r.need_out) r.need_out = p - H;  // the first complete block that ends beyond cap (p only grows)
        if (!bfinal) {
            if (p - H <= q.cap) c_bit = b.pos, c_p = p, c_blocks = n_blocks;
            f = ic_fail(V_TRUNCATED, b.pos, p);  // (what holds if the guard runs out)
            continue;
        }
        // the BFINAL block is complete: the trailer must be all there, and nothing behind it
        f = ic_fail(V_TRUNCATED, b.pos, p);
        if (p - H > q.cap) break;
        const uint64_t tb = (b.pos + 7) >> 3, tn = q.wrapper == 1 ? 4 : q.wrapper == 2 ? 8 : 0;
        if (nbytes - tb < tn) break;  // (tb <= nbytes: the block ended inside the stream)
        if (nbytes - tb > tn) {
            f = ic_fail(V_TRAILER, b.pos, p);
            break;
        }
        for (uint32_t k = 0; k < 8; k++) r.trailer[k] = k < tn ? s[tb + k] : 0;
        r.bit = q.bit_base + b.pos, r.out_pos = q.out_base + (p - H);
        c_bit = 8 * (tb + tn), c_p = p, c_blocks = n_blocks;
        finished = true;
        break;
    }
    if (!finished && (f.status != V_TRUNCATED || q.fin)) {
        r.state = S_FAILED, r.status = f.status, r.bit = q.bit_base + f.bit, r.out_pos = q.out_base + (f.in_pos - H);
        r.committed = f.in_pos - H < q.cap ? f.in_pos - H : q.cap;
        r.need_out = 0;
        return;
    }
    r.state = finished ? S_DONE : S_PENDING;
    r.commit_bit = c_bit, r.committed = c_p - H, r.n_blocks = c_blocks;
    // the next history: the last min(HIST, H + committed) bytes of hist ++ out[0, committed)
    const uint64_t have = H + r.committed;
    const uint32_t n = (uint32_t)(have < HIST ? have : HIST);
    r.hist_next_len = n;
    P::fence(p);  // the copy loads what other lanes stored
    P::copy_hist(q.hist, H, q.out, q.hist_next, have - n, n);
}

// ---- host side of both builds: what a handle keeps between writes besides its buffers, and what a record does to it -----------
struct HState {
    uint32_t wrapper, frame_open, done, failed;  // failed: the V_* status the handle died of (sticky)
    uint64_t total_in, total_out;
    uint64_t abs_bit;    // the commit point as an absolute raw-deflate bit; done: where the BFINAL block ended
    uint64_t need_out;   // room that lets the next write commit a block, 0 if none is known to be waiting
    uint64_t front, end; // the pending buffer: its live part is [front, end), front the byte that holds the commit bit
    uint32_t hist_len, hist_cur;  // the history in use: its bytes, which half of the pair
    uint32_t sum, n_dict;         // the running Adler-32 / CRC-32 of the bytes handed over; the dictionary's bytes (reset)
};
inline void is_hstate_init(HState& h, uint32_t wrapper, uint32_t n_dict) {
    h = HState{wrapper, wrapper ? 1u : 0u, 0, 0, 0, 0, 0, 0, 0, 0, n_dict, 0, wrapper == 1 ? 1u : 0u, n_dict};
}
// the handle's part of a launch; pending: the buffer's base, hist0 / hist1: the pair
inline Resume is_arm(const HState& h, const uint8_t* pending, uint8_t* hist0, uint8_t* hist1, uint8_t* out, uint64_t cap, bool fin) {
    Resume q;
    q.s = pending + h.front, q.nbytes = h.end - h.front;
    q.bit = h.frame_open ? 0 : h.abs_bit & 7, q.bit_base = h.frame_open ? 0 : h.abs_bit & ~7ull, q.out_base = h.total_out;
    q.hist = h.hist_cur ? hist1 : hist0, q.hist_next = h.hist_cur ? hist0 : hist1;
    q.out = out, q.cap = cap, q.hist_len = h.hist_len, q.wrapper = h.wrapper, q.frame_open = h.frame_open;
    q.skip = 0, q.fin = fin ? 1u : 0u, q.pad = 0;
    return q;
}
// The record of a launch into the handle and the report.  R: mi355_inflate_report.  *got: the bytes of out that the write hands
// over.  IW_OK, IW_DATA or IW_TOO_SMALL (nothing committed, and a complete block waits for room).  The checksum of a framed stream
// is not judged here: is_judge, once the sums of the bytes handed over are folded into h.sum.
template <class R>
inline int is_settle(HState& h, const Resume& q, const Rec2& rec, R& rep, uint64_t* got) {
    rep.status = V_OK, rep.reserved = 0, rep.bit = 0, rep.out_pos = 0, rep.out_len = 0;
    rep.n_blocks = 0, rep.n_stored = rep.n_fixed = rep.n_dynamic = 0, rep.ms = 0;
    if (h.frame_open && rec.frame == FP_OK) h.frame_open = 0, h.front += rec.hdr_len;
    *got = rec.committed;
    h.total_out += rec.committed;
    if (rec.state == S_FAILED) {
        h.failed = rec.status, h.need_out = 0;
        rep.status = rec.status, rep.bit = rec.bit, rep.out_pos = rec.out_pos;
        return IW_DATA;
    }
    h.front += rec.commit_bit >> 3;
    h.abs_bit = rec.state == S_DONE ? rec.bit : q.bit_base + rec.commit_bit;
    h.hist_len = rec.hist_next_len, h.hist_cur ^= 1u;
    h.need_out = rec.need_out ? rec.need_out - rec.committed : 0;
    h.done = rec.state == S_DONE;
    rep.out_pos = h.total_out, rep.out_len = rec.committed, rep.n_blocks = rec.n_blocks;
    return !rec.committed && rec.need_out ? IW_TOO_SMALL : IW_OK;
}
// DONE, framed: h.sum and ISIZE mod 2^32 against the trailer words of the record.  IW_OK, or IW_DATA with CHECKSUM in the report.
template <class R>
inline int is_judge(HState& h, const Rec2& rec, R& rep) {
    const uint8_t* t = rec.trailer;
    bool ok = true;
    if (h.wrapper == 1) ok = ((uint32_t)t[0] << 24 | (uint32_t)t[1] << 16 | (uint32_t)t[2] << 8 | t[3]) == h.sum;
    if (h.wrapper == 2)
        ok = ((uint32_t)t[3] << 24 | (uint32_t)t[2] << 16 | (uint32_t)t[1] << 8 | t[0]) == h.sum &&
             ((uint32_t)t[7] << 24 | (uint32_t)t[6] << 16 | (uint32_t)t[5] << 8 | t[4]) == (uint32_t)h.total_out;
    if (ok) return IW_OK;
    h.failed = V_CHECKSUM;
    rep.status = V_CHECKSUM, rep.bit = rec.bit, rep.out_pos = h.total_out, rep.out_len = 0, rep.n_blocks = 0;
    return IW_DATA;
}
// a write behind the end of the stream: bytes there are TRAILER, as in the one-shot
template <class R>
inline int is_after_done(HState& h, uint64_t in_len, R& rep) {
    rep.status = V_OK, rep.reserved = 0, rep.bit = 0, rep.out_pos = h.total_out, rep.out_len = 0;
    rep.n_blocks = 0, rep.n_stored = rep.n_fixed = rep.n_dynamic = 0, rep.ms = 0;
    if (!in_len) return IW_OK;
    h.failed = V_TRAILER;
    rep.status = V_TRAILER, rep.bit = h.abs_bit;
    return IW_DATA;
}

}  // namespace ist
}  // namespace mi355
#endif
