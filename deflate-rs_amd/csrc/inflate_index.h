// inflate_index.h -- the block table of ANY deflate stream, found on the device: where the tabled inflate gets its table from when
// nobody kept one.
//
// The index entry points (include/mi355_deflate.h mi355_inflate_index*, mi355_inflate_parallel*) run this text: the two kernels of
// deflate_index_inflate.inc and the host build of tests/inflindex/.  The deflate data behind the frame header is cut into SPANS of S
// compressed bytes; span k owns the bits [8kS, 8(k+1)S).
//   find   one wave per span: the span's CANDIDATE c_k, the smallest bit offset of the span at which a non-final dynamic block with a
//          valid header begins (BFINAL 0, BTYPE 2, ic_dynamic_header OK: inflate_check.h's rules, its reader and its tables).  64 lanes
//          test 64 neighbouring offsets with a register-only prefilter; what a ballot leaves gets the full parse in ascending order.
//          Span 0's candidate is the first deflate bit, whatever stands there.
//   walk   one wave per candidate: inflate_write.h's blocks in COUNTING mode (a sink of capacity 0: nothing is stored or loaded) from
//          c_k on, the output counted from 0.  At a block boundary b in a span j > k it stops if b == c_j; it also stops behind the
//          BFINAL block and at a failure.  One record each.
//   link   on the host: from span 0's walker along the links.  Entry 0 is the stream's start and a walker on the true walk only ever
//          stands on true boundaries, so the chain IS the serial walk; walkers not on it (false candidates, true starts a false
//          candidate shadowed) are ignored.
// The walker cannot test `dist > bytes produced` (it does not know its absolute position): the tabled pass does.  Nothing in here
// decides a byte: mi355_inflate_tabled refuses every table that is not the stream's serial walk, so a bad candidate costs time only.
//
// Safety, as in inflate_check.h: the stream is read through the bounded reader only, the candidates are read at an index below
// n_spans only, every loop is bounded, and nothing but a span's own candidate and record is written.
#ifndef MI355_INFLATE_INDEX_H
#define MI355_INFLATE_INDEX_H

#include "inflate_write.h"

namespace mi355 {
namespace ix {

using namespace ic;

constexpr uint64_t NOCAND = ~0ull;           // a span without a candidate
constexpr uint64_t SPAN_MIN = 256;           // MI355_CFG_INFLATE_INDEX_SPAN_BYTES: at least, at most, default
constexpr uint64_t SPAN_MAX = 1ull << 30;
constexpr uint64_t SPAN_DEFAULT = 16384;    // (the best of 16 .. 128 KiB on 100 MB of text from zlib -6: DESIGN.md section 14)
constexpr uint64_t BIAS = 1ull << 62;        // where a walker's output count begins: no distance is ever larger than it
enum : uint32_t { END_LINK = 0, END_FINAL = 1, END_FAILED = 2, END_NONE = 3 };  // (NONE: the span has no candidate, nothing walked)
constexpr uint32_t END_EDGE = 4;             // a walker of a bounded extent (inflate_bigmembers.h) at a boundary at or beyond its edge
constexpr uint64_t NOEDGE = ~0ull;           // the extent of a whole stream has no edge

// what a walker leaves
struct Walk {
    uint64_t start, end_bit;  // the candidate; where the walk stopped (link: == c_link; final: behind the BFINAL block)
    uint64_t count;           // output bytes counted (failed: in front of the failing element)
    uint32_t how, link;       // END_*; the span linked to
    uint32_t btype, status;   // of the first block; the failure's (ic::Rec's fields from here on)
    uint32_t n_stored, n_fixed, n_dynamic, pad;
    uint64_t n_blocks, bit, in_pos;  // in_pos: relative, == count
};  // 80 bytes

// the two decisions a mutant of the model changes (tests/inflindex): the three header bits of a candidate, and a walker's stop rule
struct Rules {
    static MI355_IC bool head(uint32_t h) { return h == 4; }  // BFINAL 0, BTYPE 2
    static MI355_IC bool stop(uint64_t b, uint64_t c) { return b == c; }
};

MI355_IC uint64_t ix_n_spans(uint64_t nbytes, uint64_t S) {
    const uint64_t n = nbytes / S + (nbytes % S ? 1 : 0);
    return n ? n : 1;
}

// ---- find ---------------------------------------------------------------------------------------------------------------------------
// What one lane sees at one bit offset: the three header bits, HLIT / HDIST in range and the Kraft sum of the code-length code's
// lengths (74 bits, zeros beyond the stream).  Never false where ix_is_start is true: these are ic_dynamic_header's first tests on
// the same bits -- nlen <= 286, ndist <= 30, ic_build() == 0 (left ends at 0 and is never negative: the sum of 2^-l is exactly 1).
template <class P>
MI355_IC bool ix_lane_prefilter(const uint8_t* s, uint64_t nbytes, uint64_t bit) {
    const uint64_t byte = bit >> 3;
    const uint32_t off = (uint32_t)(bit & 7);
    const uint64_t w0 = ic_load64(s, nbytes, byte), w1 = ic_load64(s, nbytes, byte + 8);
    const uint64_t lo = off ? (w0 >> off) | (w1 << (64 - off)) : w0;  // bits 0 .. 63 from `bit` on
    const uint64_t hi = w1 >> off;                                    // bits 64 .. (57 of them at least)
    if (!P::head((uint32_t)lo & 7u)) return false;
    if (((lo >> 3) & 31) > 29 || ((lo >> 8) & 31) > 29) return false;
    const uint32_t ncl = (uint32_t)((lo >> 13) & 15) + 4;
    const uint64_t tail = (lo >> 62) | (hi << 2);  // lengths 15 .. 18: bits 62 .. 73
    uint32_t kraft = 0;
    for (uint32_t i = 0; i < 19; i++) {
        const uint32_t l = i >= ncl ? 0 : i < 15 ? (uint32_t)(lo >> (17 + 3 * i)) & 7u : (uint32_t)(tail >> (3 * (i - 15))) & 7u;
        kraft += l ? 128u >> l : 0;
    }
    return kraft == 128;
}
// the predicate itself: does a non-final dynamic block with a valid header, wholly inside the stream, begin at `bit`?
template <class P>
MI355_IC bool ix_is_start(Tables& t, const uint8_t* s, uint64_t nbytes, uint64_t bit) {
    Bits b = ic_bits(s, nbytes, bit);
    const uint32_t h = ic_take(b, 3);
    if (b.over || !P::head(h)) return false;
    return ic_dynamic_header<P>(t, b, 0).status == V_OK;
}
// span k's candidate.  P::survivors(s, nbytes, base, end): bit l set = offset base + l is below `end` and passes the prefilter.
template <class P>
MI355_IC uint64_t ix_find(Tables& t, const uint8_t* s, uint64_t nbytes, uint64_t k, uint64_t S) {
    if (k == 0) return 0;
    const uint64_t lo = 8 * k * S, end = (k + 1) * S < nbytes ? 8 * (k + 1) * S : 8 * nbytes;
    for (uint64_t base = lo; base < end; base += 64) {  // (8 S / 64 steps at most)
        uint64_t m = P::survivors(s, nbytes, base, end);
        for (uint32_t guard = 0; guard < 64 && m; guard++) {
            const uint32_t l = (uint32_t)__builtin_ctzll(m);
            m &= m - 1;
            if (ix_is_start<P>(t, s, nbytes, base + l)) return base + l;
        }
    }
    return NOCAND;
}
// ... of one framed stream: what a workgroup of the find kernel does.  A stream whose frame is refused has span 0's candidate alone
// (its walker reports FRAME).
template <class P>
MI355_IC uint64_t ix_find_span(Tables& t, const uint8_t* stream, uint64_t stream_len, uint32_t wrapper, uint64_t k, uint64_t S) {
    uint64_t hdr, trailer;
    if (!ic_parse_frame(stream, stream_len, wrapper, hdr, trailer)) return k ? NOCAND : 0;
    return ix_find<P>(t, stream + hdr, stream_len - hdr - trailer, k, S);
}

// ---- walk: the blocks from candidate c of span k on (sibling of iw_inflate's loop; iw's blocks with a sink that holds nothing) -----
// edge: the spans below it have been searched (cand[j] is read for j < min(n_spans, edge) only); a boundary in span `edge` or behind it
// ends the walk as END_EDGE, with the count up to there.  NOEDGE: the whole stream was searched.
template <class P>
MI355_IC void ix_walk_to(Tables& t, const uint8_t* s, uint64_t nbytes, const uint64_t* cand, uint64_t n_spans, uint64_t S, uint64_t k, uint64_t c,
                         uint64_t edge, Walk& r) {
    Bits b = ic_bits(s, nbytes, c);
    iw::Sink o{nullptr, 0, 0};
    uint64_t p = BIAS;
    bool fixed_ready = false;
    Fail f = ic_fail(V_TRUNCATED, c, p);
    r.how = END_FAILED;
    for (uint64_t guard = 0; guard <= b.end; guard++) {  // (a block takes three bits at least)
        const uint64_t at = b.pos;
        const uint32_t h = ic_take(b, 3);
        if (b.over) {
            f = ic_fail(V_TRUNCATED, at, p);
            break;
        }
        const uint32_t bfinal = h & 1, btype = h >> 1;
        if (!guard) r.btype = btype;
        if (btype == 3) {
            f = ic_fail(V_BTYPE, at, p);
            break;
        }
        if (btype == 0) {
            f = iw::iw_stored_block<P>(b, o, p);
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
            f = iw::iw_huffman_block<P>(t, b, o, p);
        }
        if (f.status) break;
        r.n_blocks++;
        if (bfinal) {
            r.how = END_FINAL;
            break;
        }
        // a boundary: does the walker of the span it lies in begin here?
        const uint64_t j = b.pos / (8 * S);
        if (j >= edge) {
            r.how = END_EDGE;
            break;
        }
        if (j > k && j < n_spans && P::stop(b.pos, cand[j])) {
            r.how = END_LINK, r.link = (uint32_t)j;
            break;
        }
        f = ic_fail(V_TRUNCATED, b.pos, p);  // (what is reported if the guard runs out)
    }
    r.end_bit = b.pos;
    if (r.how != END_FAILED) {
        r.count = p - BIAS;
        return;
    }
    r.status = f.status, r.bit = f.bit, r.in_pos = r.count = f.in_pos - BIAS;
    r.n_blocks = 0, r.n_stored = r.n_fixed = r.n_dynamic = 0;
}
template <class P>
MI355_IC void ix_walk(Tables& t, const uint8_t* s, uint64_t nbytes, const uint64_t* cand, uint64_t n_spans, uint64_t S, uint64_t k, uint64_t c,
                      Walk& r) {
    ix_walk_to<P>(t, s, nbytes, cand, n_spans, S, k, c, NOEDGE, r);
}
// ... of one framed stream: what a workgroup of the walk kernel does (c: the span's candidate, NOCAND: none)
template <class P>
MI355_IC void ix_walk_span(Tables& t, const uint8_t* stream, uint64_t stream_len, uint32_t wrapper, const uint64_t* cand, uint64_t n_spans,
                           uint64_t S, uint64_t k, uint64_t c, Walk& r) {
    r = Walk{c, 0, 0, END_NONE, 0, 0, V_OK, 0, 0, 0, 0, 0, 0, 0};
    if (c == NOCAND) return;
    uint64_t hdr, trailer;
    if (!ic_parse_frame(stream, stream_len, wrapper, hdr, trailer)) {
        r.how = END_FAILED, r.status = V_FRAME;
        return;
    }
    ix_walk<P>(t, stream + hdr, stream_len - hdr - trailer, cand, n_spans, S, k, c, r);
}

// ---- link: host side of all builds ------------------------------------------------------------------------------------------------------
// The chain from span 0: emit(span) for every walker on it, in stream order; the last one emitted is final or failed.  (A link leads
// to a later span that has a walker: anything else -- never, from these kernels -- ends the chain as a failure would.)
template <class Emit>
inline void ix_link(const Walk* w, uint64_t n_spans, Emit emit) {
    uint64_t k = 0;
    for (uint64_t guard = 0; guard < n_spans; guard++) {
        emit(k);
        if (w[k].how != END_LINK || w[k].link <= k || w[k].link >= n_spans || w[w[k].link].how == END_NONE) return;
        k = w[k].link;
    }
}
// the stream's record from the chain's walkers, as iw_inflate would leave it for a buffer that holds nothing (no TRAILER: the tabled
// pass, or the one-wave inflate, judges the end)
inline void ix_report(const Walk* w, const uint64_t* chain, uint64_t n, iw::Rec& acc) {
    acc = iw::Rec{V_OK, 0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t sum = 0;
    for (uint64_t e = 0; e < n; e++) {
        const Walk& x = w[chain[e]];
        if (e + 1 == n && x.how != END_FINAL) {
            acc = iw::Rec{x.how == END_FAILED ? x.status : (uint32_t)V_TABLE, 0, 0, 0, x.how == END_FAILED ? x.bit : x.end_bit, sum + x.count, 0, 0, 0};
            return;
        }
        sum += x.count;
        acc.n_blocks += x.n_blocks, acc.n_stored += x.n_stored, acc.n_fixed += x.n_fixed, acc.n_dynamic += x.n_dynamic;
        acc.out_pos = acc.out_len = sum, acc.end_bit = x.end_bit;
    }
}

}  // namespace ix
}  // namespace mi355
#endif
