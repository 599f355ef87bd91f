// inflate_cut.h -- CUTS: places inside a table entry where pass 1 of a seek read may begin and end.
//
// A seek read (inflate_seek.h) decodes whole table entries, and an entry begins at a block header: a read of 4 KiB costs what one wave
// needs for the block it lies in, and a stream of fixed or stored blocks is ONE entry.  The build walks every token boundary with
// the bit and the output position in hand; a CUT is such a place it remembers, the triple (bit, pos, hdr_bit):
//   bit      where decoding resumes
//   pos      the output position there
//   hdr_bit  the bit of the 3-bit header of the block it lies in.  bit == hdr_bit: the cut stands at a block header (HEADER);
//            otherwise at a token start inside a fixed or dynamic block (TOKEN), and a wave that begins there first parses the header
//            at hdr_bit again -- the tables, nothing stored, nothing counted -- and then sets its reader to `bit`.
// There is no cut inside a stored piece.
// CUT RULE (what the Python model of the tests, the host build and the kernels share): the first cut of an entry is the entry's
// start; the walk tests  p - pos(last cut of this entry) >= cut_bytes  at every block header and at every token start of a Huffman
// block, before the token is decoded, and records a cut where it holds.  An entry of L bytes has at most L / cut_bytes + 1 cuts, so
// the slots of every entry are known from the table: nothing is appended through a counter.
// A read with cuts:
//   1. decode   every cut on its own, one wave each, into the symbols of inflate_table.h -- but a marker 256 + j of cut k means
//               "byte j of the window in front of THE CUT" (output position c_k - 32768 + j).  A cut that has a successor in its entry
//               must stop at a header or token start with bit == next.bit and p == next.pos; passing next.bit, or a token that
//               would pass next.pos, is TABLE (inflate_table.h's end-of-entry rule).
//   1b. flatten one workgroup per entry, the entry's cuts in order: a marker of cut k that names a position inside the entry takes
//               the symbol there (an earlier cut's, already flat), any other becomes the entry's marker.  Afterwards the entry's
//               symbols are what inflate_table.h's pass 1 leaves; the cuts' records are folded into the entry's and the chain of
//               cuts is checked (ict_follows).  Passes 2 and 3 of inflate_seek.h run unchanged.
// Safety, as in inflate_table.h: the bounded reader; a symbol is stored only below the cut's limit and the piece's cap; flatten loads
// only positions in [pos_e, c_k) and stores only positions in [c_k, min(end_k, cap)).
#ifndef MI355_INFLATE_CUT_H
#define MI355_INFLATE_CUT_H

#include "inflate_seek.h"

namespace mi355 {
namespace icut {

using namespace ic;

constexpr uint64_t CUT_MIN = 64, CUT_MAX = 1ull << 30;  // MI355_CFG_INFLATE_SEEK_CUT_BYTES: 0 (off) or this range

struct Cut {
    uint64_t bit, pos, hdr_bit;
};  // 24 bytes: mi355_seek_cut
// what a cut's wave leaves: ic::Rec's fields, the header of the block it ended in, whether it ended on a block boundary, and -- the
// build's walk -- how many cuts it recorded
struct Rec : ic::Rec {
    uint64_t hdr_bit;
    uint32_t boundary, n_cuts;
};  // 72 bytes
// one cut of a read's launch set
struct Item {
    Cut c, next;             // (next: the cut behind it in its entry, where it must stop)
    uint32_t ent, has_next;  // its entry in the set
};  // 56 bytes
// mi355_inflate_seek_last_read_cuts
struct Counts {
    uint64_t cuts, symbols, steps, launches;
};

// the decisions a mutant of the model changes (tests/inflcut)
struct Rules {
    static MI355_IC bool cut_here(uint64_t p, uint64_t last_cut, uint64_t entry_pos, uint64_t cut_bytes) { return p - last_cut >= cut_bytes; }
    static MI355_IC bool stops(uint64_t bit, uint64_t p, const Cut& next) { return bit == next.bit && p == next.pos; }
    static MI355_IC bool flat_inside(uint64_t q, uint64_t entry_pos) { return q >= entry_pos; }  // flatten: the position holds a symbol
};

// 0: off; false: not a legal value of the key
MI355_IC bool ict_cut_bytes_ok(uint64_t v) { return v == 0 || (v >= CUT_MIN && v <= CUT_MAX); }
// the slots of an entry of `len` output bytes
MI355_IC uint64_t ict_slots(uint64_t len, uint64_t cut_bytes) { return len / cut_bytes + 1; }

// what a wave carries through one cut, or through one entry of the build
struct Walk {
    uint64_t limit;      // the position no token may pass
    Cut next;
    uint32_t has_next;
    Cut* slots;          // the build: where the entry's cuts go (slot 0: the entry's start); nullptr: a read
    uint32_t n_slots, n_rec;
    uint64_t last, entry_pos, cut_bytes;
    uint32_t stopped;    // the walk stands on `next`
};

// a PLACE: a block header or a token start.  0: go on; 1: the walk stands on its successor; 2: it has passed it (TABLE)
template <class P, class R>
MI355_IC uint32_t ict_place(Walk& w, uint64_t bit, uint64_t p, uint64_t hdr_bit) {
    if (w.has_next) {
        if (R::stops(bit, p, w.next)) return 1;
        if (bit >= w.next.bit) return 2;
    }
    if (w.slots && R::cut_here(p, w.last, w.entry_pos, w.cut_bytes)) {
        if (w.n_rec < w.n_slots && P::leader()) w.slots[w.n_rec] = Cut{bit, p, hdr_bit};
        w.n_rec++;  // (never beyond n_slots by the rule; a mutant's surplus is counted and not stored)
        w.last = p;
    }
    return 0;
}

// ---- the symbols of one Huffman block from the reader's position on (sibling of it_huffman_block: a place test in front of every
// token).  w.stopped: the walk stands on w.next, the block is not over ----------------------------------------------------------------
template <class P, class R>
MI355_IC Fail ict_huffman_block(Tables& t, Bits& b, it::Sink& o, uint64_t& p, Walk& wk, uint64_t hdr_bit) {
    uint32_t n_lit = 0;
    uint64_t lit_p = p;
    const uint64_t limit = wk.limit;
    Fail f = ic_fail(V_OK, 0, 0);
    bool done = false;
    for (uint64_t guard = 0; guard <= b.end && !done; guard++) {  // (a token takes a bit at least)
        const uint64_t at = b.pos;
        const uint32_t pl = ict_place<P, R>(wk, at, p, hdr_bit);
        if (pl == 1) {
            wk.stopped = 1;
            break;
        }
        if (pl == 2) {
            f = ic_fail(V_TABLE, at, p);
            break;
        }
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
            if (n_lit == LIT_RUN) it::it_flush_lits<P>(t, o, lit_p, n_lit);
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
        {
#include "ic_match_token.inc"
            if (len > limit - p) {  // (p <= limit always)
                f = ic_fail(V_TABLE, at, p);
                break;
            }
            it::it_flush_lits<P>(t, o, lit_p, n_lit);  // the match may source from them
            if (p < o.cap) {
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
    }
    // the literals gathered in front of a stop, of the failing element or of the block's end are written before it is reported
    it::it_flush_lits<P>(t, o, lit_p, n_lit);
    if (f.status) return f;
    if (wk.stopped) return ic_fail(V_OK, 0, 0);
    if (!done) return ic_fail(V_TRUNCATED, b.pos, p);
    return ic_fail(V_OK, 0, 0);
}

// ---- one cut c of entry e (sibling of it_entry).  w.has_next: up to w.next; otherwise to the entry's end under it_entry's rules.
// With c the entry's start, no successor and w.slots set this is the build's walk of the whole entry: it_entry's record, and the
// entry's cuts in w.slots. -----------------------------------------------------------------------------------------------------------
template <class P, class R>
MI355_IC void ict_cut(Tables& t, const uint8_t* s, uint64_t nbytes, it::Sink& o, const Entry& e, uint64_t total, const Cut& c, Walk& w, Rec& r) {
    Bits b = ic_bits(s, nbytes, c.bit);
    uint64_t p = c.pos;
    const uint64_t elimit = e.last ? total : e.next_pos;
    w.limit = w.has_next && w.next.pos < elimit ? w.next.pos : elimit;
    w.stopped = 0;
    bool fixed_ready = false, in_block = false;
    uint32_t bfinal = 0;
    uint64_t hdr = c.hdr_bit;
    Fail f = ic_fail(V_TRUNCATED, c.bit, p);
    r.n_blocks = 0, r.n_stored = r.n_fixed = r.n_dynamic = 0;
    r.boundary = 1;
    bool go = true;
    if (p > w.limit || p < e.pos || c.hdr_bit > c.bit) {  // (the host's cut list: never)
        f = ic_fail(V_TABLE, c.bit, p);
        go = false;
    } else if (c.bit != c.hdr_bit) {  // TOKEN: the tables of the block it lies in, nothing stored, nothing counted
        Bits hb = ic_bits(s, nbytes, c.hdr_bit);
        const uint32_t h = ic_take(hb, 3);
        bfinal = h & 1;
        const uint32_t btype = h >> 1;
        go = false;
        if (hb.over) f = ic_fail(V_TRUNCATED, c.hdr_bit, p);
        else if (bfinal && !e.last) f = ic_fail(V_TABLE, c.hdr_bit, p);
        else if (btype == 3) f = ic_fail(V_BTYPE, c.hdr_bit, p);
        else if (btype == 0) f = ic_fail(V_TABLE, c.hdr_bit, p);  // (no cut lies inside a stored piece)
        else {
            if (btype == 1) {
                if (P::leader()) ic_fixed_tables(t);
                P::sync();
                fixed_ready = true;
                f = ic_fail(V_OK, 0, 0);
            } else {
                f = ic_dynamic_header<P>(t, hb, p);
            }
            if (!f.status) {
                if (hb.pos > c.bit) f = ic_fail(V_TABLE, c.hdr_bit, p);  // the first token of the block lies behind the cut
                else go = in_block = true;
            }
        }
    }
    if (go)
        for (uint64_t guard = 0; guard <= b.end; guard++) {  // (a block takes three bits at least)
            uint64_t at = b.pos;
            uint32_t btype = 1;
            if (!in_block) {
                const uint32_t pl = ict_place<P, R>(w, at, p, at);
                if (pl == 1) {
                    w.stopped = 1;
                    f = ic_fail(V_OK, 0, 0);
                    break;
                }
                if (pl == 2) {
                    f = ic_fail(V_TABLE, at, p);
                    break;
                }
                const uint32_t h = ic_take(b, 3);
                if (b.over) {
                    f = ic_fail(V_TRUNCATED, at, p);
                    break;
                }
                bfinal = h & 1, btype = h >> 1;
                hdr = at;
                if (bfinal && !e.last) {
                    f = ic_fail(V_TABLE, at, p);
                    break;
                }
                if (btype == 3) {
                    f = ic_fail(V_BTYPE, at, p);
                    break;
                }
                if (btype == 0) {
                    f = it::it_stored_block<P>(b, o, p, w.limit);
                    r.n_stored++;
                } else if (btype == 1) {
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
            }
            if (btype) {
                in_block = false;
                f = ict_huffman_block<P, R>(t, b, o, p, w, hdr);
                if (w.stopped) {
                    r.boundary = 0;
                    break;
                }
            }
            if (f.status) break;
            r.n_blocks++;
            if (w.has_next) {  // (the next header's place test ends the cut)
                f = ic_fail(V_TABLE, b.pos, p);  // (... if the guard runs out, or the stream ends here)
                if (bfinal) break;
                continue;
            }
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
    r.hdr_bit = hdr;
    r.n_cuts = w.n_rec;
}

// one cut of one framed stream: what a workgroup of the cuts' pass 1, and a turn of the host loops, does (it_decode_entry's sibling)
template <class P, class R>
MI355_IC void ict_decode_cut(Tables& t, uint16_t* sym, const is::Part& pt, const Entry& e, const Item& it_, Rec& r) {
    uint64_t hdr, trailer;
    r = Rec{{V_FRAME, 0, 0, 0, 0, 0, 0, 0, 0}, 0, 1u, 0u};
    if (!ic_parse_frame(pt.stream, pt.stream_len, pt.wrapper, hdr, trailer)) return;
    it::Sink o{sym + pt.sym_off, nullptr, pt.base, it_.c.pos, pt.cap, it_.c.pos};
    Walk w{0, it_.next, it_.has_next, nullptr, 0u, 0u, it_.c.pos, e.pos, 0, 0u};
    ict_cut<P, R>(t, pt.stream + hdr, pt.stream_len - hdr - trailer, o, e, pt.total, it_.c, w, r);
    if (r.status || !e.last || it_.has_next) return;
    const Fail f = ic_trailer(pt.stream, pt.stream_len, hdr, trailer, 0u, r.end_bit, r.end_pos, 0u, 0u);
    r.status = f.status, r.bit = f.bit, r.in_pos = f.in_pos;
}
// the build's pass 1 of one entry: it_decode_entry's record and symbols, and the entry's cuts into slots[0, n_slots)
template <class P, class R>
MI355_IC void ict_build_entry(Tables& t, const uint8_t* stream, uint64_t stream_len, uint32_t wrapper, it::Sink& o, const Entry& e, uint64_t total,
                              uint64_t cut_bytes, Cut* slots, uint32_t n_slots, Rec& r) {
    uint64_t hdr, trailer;
    r = Rec{{V_FRAME, 0, 0, 0, 0, 0, 0, 0, 0}, 0, 1u, 0u};
    if (!ic_parse_frame(stream, stream_len, wrapper, hdr, trailer)) return;
    const Cut c{e.bit, e.pos, e.bit};
    if (n_slots && P::leader()) slots[0] = c;
    Walk w{0, c, 0u, slots, n_slots, 1u, e.pos, e.pos, cut_bytes, 0u};
    ict_cut<P, R>(t, stream + hdr, stream_len - hdr - trailer, o, e, total, c, w, r);
    if (r.status || !e.last) return;
    const Fail f = ic_trailer(stream, stream_len, hdr, trailer, 0u, r.end_bit, r.end_pos, 0u, 0u);
    r.status = f.status, r.bit = f.bit, r.in_pos = f.in_pos;
}

// ---- flatten ----------------------------------------------------------------------------------------------------------------------
// cut k follows cut k - 1 (`prev`: its record): a TOKEN cut lies in the block its predecessor ended inside, a HEADER cut where its
// predecessor ended on a block boundary, and either way where its predecessor stopped
MI355_IC bool ict_follows(const Rec& prev, const Cut& c) {
    if (prev.end_bit != c.bit || prev.end_pos != c.pos) return false;
    return c.bit == c.hdr_bit ? prev.boundary != 0 : (!prev.boundary && prev.hdr_bit == c.hdr_bit);
}
// the flat symbol at position q of a cut that begins at c_pos, from the symbol its wave stored (sym: element 0 is position `base`)
template <class R>
MI355_IC uint16_t ict_flat(const uint16_t* sym, uint64_t base, uint64_t entry_pos, uint64_t c_pos, uint64_t q) {
    const uint32_t s = sym[q - base];
    if (s < it::MARK) return (uint16_t)s;
    const uint64_t src = c_pos + ((s - it::MARK) & (it::WIN - 1));  // the position named, plus WIN
    if (src >= it::WIN && R::flat_inside(src - it::WIN, entry_pos) && src - it::WIN >= base && src - it::WIN < c_pos) return sym[src - it::WIN - base];
    return (uint16_t)(it::MARK + (uint32_t)((src - entry_pos) & (it::WIN - 1)));
}
// the fold of an entry's cuts, one at a time in order (every thread of flatten's workgroup runs it with the same values).  acc: zeroed
// with status OK and end = the entry's start.  Returns the position up to which cut k's symbols are to be flattened (its start: none)
// and sets `more` = false at the entry's first failing cut.
MI355_IC uint64_t ict_fold(ic::Rec& acc, const Rec* recs, const Item* items, uint32_t k, bool& more) {
    const Rec& r = recs[k];
    const Cut& c = items[k].c;
    if (k && !ict_follows(recs[k - 1], c)) {
        acc.status = V_TABLE, acc.bit = c.bit, acc.in_pos = c.pos;
        more = false;
        return c.pos;
    }
    if (r.status) {
        acc.status = r.status, acc.bit = r.bit, acc.in_pos = r.in_pos;
        more = false;
        return r.in_pos > c.pos ? r.in_pos : c.pos;
    }
    acc.n_blocks += r.n_blocks;
    acc.n_stored += r.n_stored, acc.n_fixed += r.n_fixed, acc.n_dynamic += r.n_dynamic;
    acc.end_bit = r.end_bit, acc.end_pos = r.end_pos;
    return r.end_pos;
}

// ---- host side of all builds ------------------------------------------------------------------------------------------------------
// The cuts of a launch set of is_plan: for every entry of the set its cuts in order -- all of them, but in a part's last entry only
// through the cut that holds the part's last byte.  cut0[g] .. cut0[g + 1]: the cuts of the stream's entry g in `cuts`; ent0[j]: the
// stream's entry that part j of the set begins with.  first[k] .. first[k + 1]: the items of the set's entry k.
inline void ict_items(const is::Set& s, const std::vector<uint64_t>& ent0, const std::vector<uint64_t>& cut0, const std::vector<Cut>& cuts,
                      std::vector<Item>& items, std::vector<uint32_t>& first) {
    items.clear();
    first.assign(s.ents.size() + 1, 0);
    for (size_t j = 0; j < s.parts.size(); j++) {
        const is::Part& pt = s.parts[j];
        for (uint32_t k = 0; k < pt.n; k++) {
            const uint64_t g = ent0[j] + k, a = cut0[g];
            uint64_t b = cut0[g + 1];
            if (k + 1 == pt.n)  // (cap > the entry's start: is_plan's b is the entry that holds cap - 1)
                while (b - a > 1 && cuts[b - 1].pos >= pt.cap) b--;
            first[pt.e0 + k] = (uint32_t)items.size();
            for (uint64_t i = a; i < b; i++) {
                const bool has_next = i + 1 < cut0[g + 1];
                items.push_back(Item{cuts[i], has_next ? cuts[i + 1] : Cut{0, 0, 0}, pt.e0 + k, has_next ? 1u : 0u});
            }
        }
    }
    first[s.ents.size()] = (uint32_t)items.size();
}

}  // namespace icut
}  // namespace mi355
#endif
