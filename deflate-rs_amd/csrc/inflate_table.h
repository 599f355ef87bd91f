// inflate_table.h -- inflate ONE stream from its encoder block table, every entry of the table decoded on its own.
//
// The tabled inflate entry points (include/mi355_deflate.h mi355_inflate_tabled*) run this text: the three kernels of
// deflate_table_inflate.inc and the host builds of tests/infltable/.  Entry e of the table starts at bit bit_start[e] and at output
// position pos_e = sum of in_bytes[k], k < e, both known before anything runs; what it does not have is the 32 KiB of output in
// front of pos_e, which its predecessors produce.  So nothing waits for them.  Three passes:
//   1. decode   every entry on its own into 16-bit SYMBOLS sym[pos_e, pos_e + len_e): a value below 256 is a byte, 256 + j is
//               "byte j of the 32 KiB window in front of this entry" (output position pos_e - 32768 + j).  A match copies symbols,
//               bytes and markers alike; a source in front of pos_e loads nothing, its marker is computed.
//   2. windows  the resolved window W_e (real bytes) behind every entry from W_{e-1} and the entry's symbols: the one serial part.
//   3. resolve  out[q] = sym[q] < 256 ? sym[q] : W_{e-1}[sym[q] - 256], flat over the output.
// The bit reader, the tables, the header rules, the frame parsers, the match token (ic_match_token.inc) and the stored header
// (ic_stored_header.inc) are inflate_check.h's and the match's source index is inflate_write.h's; the symbol loop, the stored piece and
// the entry loop around them are SIBLINGS of theirs once more, with verify's end-of-entry tests and inflate's sink.  Every entry
// must end exactly at the next one's bit and output position -- anything else is TABLE --, so a table that passes describes the one
// serial walk of the stream: a wrong table cannot yield wrong bytes with OK.
//
// Safety, as in inflate_write.h: the stream is read through the bounded reader; a symbol is stored only at a position below the
// entry's limit (a token that would pass it is TABLE before it stores) and below `cap`, and loaded only at a position in
// [pos_e, min(p, cap)); a marker is masked to the window's size where it is used.  Past `cap` the decode goes on counting.
#ifndef MI355_INFLATE_TABLE_H
#define MI355_INFLATE_TABLE_H

#include <string.h>

#include <vector>

#include "inflate_write.h"

namespace mi355 {
namespace it {

using namespace ic;

constexpr uint32_t WIN = 32768;           // the window of a deflate stream
constexpr uint32_t MARK = 256;            // sym >= MARK: byte sym - MARK of the window in front of the entry
constexpr uint32_t GROUP_ENTRIES = 4096;  // entries of one group at most
constexpr uint32_t RESOLVE_RUN = 16;      // output bytes of one resolve step

// where an entry's symbols go.  sym[0] is output position `base` (the group's first); vis: every store at a position below it has
// been fenced (the same in all lanes; it begins at the entry's start: sources in front of it are computed, not loaded)
struct Sink {
    uint16_t* sym;
    uint8_t* out;  // (the serial model's: plain bytes, element 0 is output position 0)
    uint64_t base, start, cap, vis;
};

// ---- the writes of pass 1, as one lane of 64 sees them (tests/infltable replays them lane by lane) ------------------------------
// the symbol at a source position: loaded inside the entry, computed in front of it (src >= start - WIN: dist <= 32768)
MI355_IC uint16_t it_lane_src(const uint16_t* sym, uint64_t base, uint64_t start, uint64_t src) {
    return src >= start ? sym[src - base] : (uint16_t)(MARK + (uint32_t)(src + WIN - start));
}
MI355_IC void it_lane_lits(const uint8_t* lit, uint16_t* sym, uint64_t base, uint64_t cap, uint64_t lit_p, uint32_t n, uint32_t lane) {
    if (lane < n && lit_p + lane < cap) sym[lit_p + lane - base] = lit[lane & (LIT_RUN - 1)];
}
MI355_IC void it_lane_match(uint16_t* sym, uint64_t base, uint64_t start, uint64_t cap, uint64_t p, uint32_t len, uint32_t dist, uint32_t at,
                            uint32_t lane) {
    const uint32_t i = at + lane;
    if (i < len && p + i < cap) sym[p + i - base] = it_lane_src(sym, base, start, iw::iw_match_src(p, dist, i));
}
// a stored piece widens bytes to symbols: `head` of them up to the destination's first 16-byte boundary, one a lane ...
MI355_IC uint32_t it_run_head(const uint16_t* sym, uint64_t base, uint64_t p, uint32_t n) {
    const uint32_t h = (uint32_t)((0 - (((uintptr_t)sym >> 1) + (p - base))) & 7);
    return h < n ? h : n;
}
MI355_IC void it_lane_run_head(const uint8_t* src, uint16_t* sym, uint64_t base, uint64_t cap, uint64_t p, uint32_t head, uint32_t lane) {
    if (lane < head && p + lane < cap) sym[p + lane - base] = src[lane];
}
// ... then eight a lane, 512 a step, as two aligned 8-byte stores; the lane that holds the piece's end, or the symbol at cap, goes one by one
MI355_IC void it_lane_run(const uint8_t* src, uint16_t* sym, uint64_t base, uint64_t cap, uint64_t p, uint32_t n, uint32_t head, uint32_t at,
                          uint32_t lane) {
    const uint32_t o = head + at + lane * 8;
    if (o >= n) return;
    if (n - o >= 8 && p + o < cap && cap - (p + o) >= 8) {
        uint64_t v, lo = 0, hi = 0;
        __builtin_memcpy(&v, src + o, 8);
        for (uint32_t k = 0; k < 4; k++) {
            lo |= ((v >> (8 * k)) & 0xffull) << (16 * k);
            hi |= ((v >> (32 + 8 * k)) & 0xffull) << (16 * k);
        }
        uint16_t* d = (uint16_t*)__builtin_assume_aligned(sym + (p + o - base), 16);
        __builtin_memcpy(d, &lo, 8);
        __builtin_memcpy(d + 4, &hi, 8);
        return;
    }
    for (uint32_t k = 0; k < 8; k++)
        if (k < n - o && p + o + k < cap) sym[p + o + k - base] = src[o + k];
}

// the gathered literals to positions lit_p ..
template <class P>
MI355_IC void it_flush_lits(Tables& t, Sink& o, uint64_t lit_p, uint32_t& n_lit) {
    const uint32_t n = n_lit;
    n_lit = 0;
    if (!n) return;
    P::sync();
    if (lit_p < o.cap) P::store_lits(t.lit, o, lit_p, n);
    P::sync();  // (the next gather writes t.lit again)
}

// ---- the symbols of one Huffman block (sibling of iw_huffman_block; `limit`: the position no token of this entry may pass) -----
template <class P>
MI355_IC Fail it_huffman_block(Tables& t, Bits& b, Sink& o, uint64_t& p, uint64_t limit) {
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
            if (p >= limit) {
                f = ic_fail(V_TABLE, at, p);
                break;
            }
            if (!n_lit) lit_p = p;
            if (P::leader()) t.lit[n_lit & (LIT_RUN - 1)] = (uint8_t)s;
            n_lit++, p++;
            ic_skip(b, used);
            if (n_lit == LIT_RUN) it_flush_lits<P>(t, o, lit_p, n_lit);
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
        // (p is the position in the whole output: DISTANCE where a marker would point in front of the stream)
#include "ic_match_token.inc"
        if (len > limit - p) {  // (p <= limit always)
            f = ic_fail(V_TABLE, at, p);
            break;
        }
        it_flush_lits<P>(t, o, lit_p, n_lit);  // the match may source from them
        if (p < o.cap) {
            // the symbols it loads: [max(p - dist, start), p - dist + min(len, dist)).  Stores behind the last fence are not loadable yet.
            const uint64_t need = p - dist + (len < dist ? len : dist);
            if (need > o.vis) {
                P::fence(p);
                o.vis = p;
            }
            P::copy_match(o, p, len, dist);
        }
        p += len;
        ic_skip(b, used);
    }
    // the literals gathered in front of the failing element, or of the block's end, are written before it is reported
    it_flush_lits<P>(t, o, lit_p, n_lit);
    if (f.status) return f;
    if (!done) return ic_fail(V_TRUNCATED, b.pos, p);
    return ic_fail(V_OK, 0, 0);
}

// one stored piece (sibling of iw_stored_block)
template <class P>
MI355_IC Fail it_stored_block(Bits& b, Sink& o, uint64_t& p, uint64_t limit) {
#include "ic_stored_header.inc"
    if (len > limit - p) return ic_fail(V_TABLE, at, p);
    if (len && p < o.cap) P::copy_run(b.s + byte0, o, p, len);
    p += len;
    b.pos += 8ull * len;
    return ic_fail(V_OK, 0, 0);
}

// ---- one entry: its deflate blocks, up to the next entry's restart point or, the last one, through the BFINAL block, which must
// end at `total` = the sum of the table's in_bytes (sibling of ic_entry; every end-of-entry failure is TABLE) ------------------------
template <class P>
MI355_IC void it_entry(Tables& t, const uint8_t* s, uint64_t nbytes, Sink& o, const Entry& e, uint64_t total, ic::Rec& r) {
    Bits b = ic_bits(s, nbytes, e.bit);
    uint64_t p = e.pos;
    const uint64_t limit = e.last ? total : e.next_pos;
    bool fixed_ready = false;
    Fail f = ic_fail(V_TRUNCATED, e.bit, p);
    r.n_blocks = 0, r.n_stored = r.n_fixed = r.n_dynamic = 0;
    if (p > limit) f = ic_fail(V_TABLE, e.bit, p);  // (the positions are running sums: never)
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
                f = it_stored_block<P>(b, o, p, limit);
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
                f = it_huffman_block<P>(t, b, o, p, limit);
            }
            if (f.status) break;
            r.n_blocks++;
            if (e.last) {
                if (!bfinal) {
                    f = ic_fail(V_TRUNCATED, b.pos, p);  // (what is reported if the guard runs out)
                    continue;
                }
                if (p != total) f = ic_fail(V_TABLE, b.pos, p);  // the BFINAL block ends before the table's total
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

// one entry of one framed stream: what a workgroup of pass 1, and a turn of the host loops, does.  The last entry's BFINAL block must
// end in the last byte in front of the trailer (TRAILER; the checksum is judged afterwards over the output, iw_check_trailer).
template <class P>
MI355_IC void it_decode_entry(Tables& t, const uint8_t* stream, uint64_t stream_len, uint32_t wrapper, Sink& o, const Entry& e, uint64_t total,
                              ic::Rec& r) {
    uint64_t hdr, trailer;
    r = ic::Rec{V_FRAME, 0, 0, 0, 0, 0, 0, 0, 0};
    if (!ic_parse_frame(stream, stream_len, wrapper, hdr, trailer)) return;
    it_entry<P>(t, stream + hdr, stream_len - hdr - trailer, o, e, total, r);
    if (r.status || !e.last) return;
    const Fail f = ic_trailer(stream, stream_len, hdr, trailer, 0u, r.end_bit, r.end_pos, 0u, 0u);
    r.status = f.status, r.bit = f.bit, r.in_pos = f.in_pos;
}

// ---- pass 2: one window step.  Byte j of W_e is output position start + len - WIN + j: inside the entry it is the entry's symbol,
// looked up in W_{e-1} (`prev`) when it is a marker; in front of it, it is W_{e-1}[j + len] (entries shorter than the window, empty
// ones included).  Positions at or beyond cap hold no symbol and read as 0: nothing below cap refers to them. -------------------------
MI355_IC uint8_t it_window_byte(const uint16_t* sym, uint64_t base, uint64_t start, uint64_t len, uint64_t cap, const uint8_t* prev, uint32_t j) {
    if (len >= WIN || j >= WIN - len) {
        const uint64_t q = start + len + j - WIN;  // (>= start)
        if (q >= cap) return 0;
        const uint32_t s = sym[q - base];
        return s < MARK ? (uint8_t)s : prev[(s - MARK) & (WIN - 1)];
    }
    return prev[j + (uint32_t)len];
}
// one chain of entries, as the walk over it (it_window_walk.inc) takes it
struct Walk {
    const uint16_t* sym;  // element 0 is output position `base`
    const Entry* ents;
    const ic::Rec* recs;
    uint32_t n;
    uint64_t base, cap;
    uint8_t* win;        // the windows' slots: slot0 + k + 1 is the window behind entry k
    uint32_t slot0;
    uint32_t last_slot;  // the workspace's last slot, the one the next group reads: the window behind the chain's last entry is stored
                         // only where that is its slot (the windows behind the other entries always are)
    bool last_made;      // false: the window behind the chain's last entry is not made at all
};

// ---- pass 3: one resolve step, RESOLVE_RUN output bytes from q0 on, below `end` = min(limit, cap) -------------------------------------
MI355_IC uint64_t it_align(uint64_t v) { return (v + RESOLVE_RUN - 1) / RESOLVE_RUN * RESOLVE_RUN; }
// the entry of the group that holds position q: the last one that begins at or before it (the empty ones in front of it begin there too)
MI355_IC uint32_t it_entry_of(const Entry* ents, uint32_t n, uint64_t q) {
    uint32_t lo = 0, hi = n;
    for (uint32_t guard = 0; guard < 32 && hi - lo > 1; guard++) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (ents[mid].pos <= q) lo = mid;
        else hi = mid;
    }
    return lo;
}
// the part that holds symbol element f0 (is::Part, ib::Part): the last one that begins at or before it (parts without symbols in front
// of it begin there too)
template <class Part>
MI355_IC uint32_t it_part_of(const Part* parts, uint32_t n, uint64_t f0) {
    uint32_t lo = 0, hi = n;
    for (uint32_t guard = 0; guard < 32 && hi - lo > 1; guard++) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (parts[mid].sym_off <= f0) lo = mid;
        else hi = mid;
    }
    return lo;
}
// pass 3's lower bound (a seek read's lead-in is decoded and never written; the tabled and the members callers have none: lo = 0)
struct Writes {
    static MI355_IC bool writes(uint64_t q, uint64_t lo) { return q >= lo; }
};
// win: the group's windows, slot k = the window in front of entry k (W_{k-1}; slot 0 comes from the group before).  out[q - lo] for q
// in [max(q0, lo), end) of the run.  The aligned fast path is judged on the address the run's first byte goes to; a run that begins
// below lo goes byte by byte and forms no pointer below out.
template <class R = Writes>
MI355_IC void it_resolve_run(const uint16_t* sym, const uint8_t* win, const Entry* ents, uint32_t n, uint64_t base, uint64_t end, uint64_t lo,
                             uint8_t* out, uint64_t q0) {
    if (q0 >= end || !n) return;
    const uint32_t cnt = end - q0 < RESOLVE_RUN ? (uint32_t)(end - q0) : RESOLVE_RUN;
    if (!R::writes(q0 + cnt - 1, lo)) return;  // the whole run is lead-in
    uint32_t k = it_entry_of(ents, n, q0);
    uint8_t v[RESOLVE_RUN];
    for (uint32_t i = 0; i < RESOLVE_RUN; i++) {
        v[i] = 0;
        if (i >= cnt) continue;
        const uint64_t q = q0 + i;
        for (uint32_t guard = 0; guard < RESOLVE_RUN && k + 1 < n && ents[k + 1].pos <= q; guard++) k = it_entry_of(ents, n, q);
        const uint32_t s = sym[q - base];
        v[i] = s < MARK ? (uint8_t)s : win[(uint64_t)k * WIN + ((s - MARK) & (WIN - 1))];
    }
    if (cnt == RESOLVE_RUN && R::writes(q0, lo) && (((uintptr_t)out + (q0 - lo)) & 7) == 0) {
        uint64_t a, b;
        __builtin_memcpy(&a, v, 8);
        __builtin_memcpy(&b, v + 8, 8);
        uint64_t* d = (uint64_t*)__builtin_assume_aligned(out + (q0 - lo), 8);
        d[0] = a, d[1] = b;
        return;
    }
    for (uint32_t i = 0; i < RESOLVE_RUN; i++)
        if (i < cnt && R::writes(q0 + i, lo)) out[q0 + i - lo] = v[i];
}
// the call form from before the lower bound.  Nothing in this tree uses it: host builds written against the earlier headers
// (tests/infltable of the commit before) do, and it can go once none is left.
MI355_IC void it_resolve_run(const uint16_t* sym, const uint8_t* win, const Entry* ents, uint32_t n, uint64_t base, uint64_t end, uint8_t* out,
                             uint64_t q0) {
    it_resolve_run(sym, win, ents, n, base, end, 0, out, q0);
}

// ---- host side of all builds ------------------------------------------------------------------------------------------------------
// the group that begins with entry k0 ends in front of the returned entry: closed at group_bytes output bytes or GROUP_ENTRIES
// entries, whichever comes first; an entry larger than group_bytes is a group of its own
template <class GetBytes>
inline uint64_t it_group_end(GetBytes in_bytes, uint64_t n, uint64_t k0, uint64_t group_bytes) {
    uint64_t k = k0, sum = 0;
    while (k < n && k - k0 < GROUP_ENTRIES && (k == k0 || in_bytes(k) <= group_bytes - sum)) {
        sum += in_bytes(k++);
        if (sum > group_bytes) break;
    }
    return k;
}
// the records of one group folded into the stream's record (`acc`: zeroed before the first group).  The report is the first failing
// entry's in stream order; a clean stream's block counts are the sums.  false: an entry failed, the call ends here.
inline bool it_report(const ic::Rec* recs, uint64_t n, iw::Rec& acc) {
    for (uint64_t k = 0; k < n; k++) {
        if (recs[k].status) {
            acc = iw::Rec{recs[k].status, 0, 0, 0, recs[k].bit, recs[k].in_pos, 0, 0, 0};
            return false;
        }
        acc.n_blocks += recs[k].n_blocks;
        acc.n_stored += recs[k].n_stored, acc.n_fixed += recs[k].n_fixed, acc.n_dynamic += recs[k].n_dynamic;
        acc.out_pos = acc.out_len = recs[k].end_pos;
        acc.end_bit = recs[k].end_bit;
    }
    return true;
}
// what the windows pass finds on the device, and the host builds with it: the end of the group's last good entry, or the failing
// entry's out_pos -- nothing is resolved at or beyond it
MI355_IC uint64_t it_limit(const ic::Rec* recs, uint32_t n, uint64_t base) {
    uint64_t limit = base;
    for (uint32_t k = 0; k < n; k++) {
        if (recs[k].status) return recs[k].in_pos;
        limit = recs[k].end_pos;
    }
    return limit;
}
// ... and the walk itself for the host builds: the text the three window kernels run, by one caller that takes every word of a
// window and needs no barrier; `step(k)` is called where the workgroup's barrier stands.  first: the window in front of entry 0
// (nullptr: zeros).  It returns the walk's limit.  The text stores a window a 32-bit word at a time: wk.win must be 4-byte aligned
// (the two windows here are, as vectors' storage).
template <class Step>
struct SerialWalk {
    static constexpr uint32_t turns = WIN / 4;
    Step& step;
    uint32_t word(uint32_t i) const { return 4 * i; }
    void step_done(uint32_t k) const { step(k); }
};
template <class Step>
inline uint64_t it_window_walk(const Walk& wk, const uint8_t* first, Step&& step) {
    std::vector<uint8_t> w[2] = {std::vector<uint8_t>(WIN, 0), std::vector<uint8_t>(WIN)};
    if (first) memcpy(w[0].data(), first, WIN);
    uint8_t* const s_w[2] = {w[0].data(), w[1].data()};
    const SerialWalk<Step> wp{step};
#include "it_window_walk.inc"
    return limit;
}
inline uint64_t it_window_walk(const Walk& wk, const uint8_t* first) {
    return it_window_walk(wk, first, [](uint32_t) {});
}

}  // namespace it
}  // namespace mi355
#endif
