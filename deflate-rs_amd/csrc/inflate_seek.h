// inflate_seek.h -- SEEK POINTS: any byte range of one large stream, decoded from the nearest restart point that has its window.
//
// The seek entry points (include/mi355_deflate.h mi355_inflate_seek_*) run this text: the kernels of deflate_seek_inflate.inc and the
// host build of tests/inflseek/.  It sits on inflate_table.h: a table entry (bit_start, in_bytes) is a place where a decode can begin
// once the 32 KiB of output in front of it are known, and pass 2 of the tabled inflate computes exactly those 32 KiB behind every
// entry.  A restart point WITH its window is a seek point: decoding from it needs nothing in front of it.
//   build   the tabled decode of the whole stream, group by group, with cap = total and no output buffer; the windows in front of
//           the entries the POINT RULE names are kept, 32 KiB each, the rest are dropped with the group's workspace.
//   read    [off, off + len): the entries from the last point at or before `off` through the entry that holds the range's last
//           byte, in inflate_table.h's three passes.  The lead-in [pos of the point, off) is decoded to symbols -- matches inside
//           the range copy from it -- and never written: pass 3 has a LOWER bound beside its upper one.
// Point rule: the entries are ic_make_entries' over the table.  Entry 0 is a point (its window is zeros and is not stored); entry
// k > 0 is a point iff pos_k - pos_(last point) >= spacing.  The default spacing, 1 MiB of output between points, is zran's
// convention (zlib's examples/zran.c: "#define SPAN 1048576L"): DERIVED, not measured on this device.
// Range plan: a range whose symbols (its end less the position of its point) fit the group budget is one PIECE; a longer one is cut
// at points into consecutive pieces, each at most the budget's worth, each from its own point with the window the build kept.  The
// pieces are independent -- no window is carried between pieces or launch sets -- and a gap between two points that is larger than
// the budget is a piece and a set of its own (inflate_table.h's "an entry larger than this is a group of its own").
//
// Safety, as in inflate_table.h: the stream is read through the bounded reader; a symbol is stored only below its entry's limit and
// its piece's cap; pass 3 stores out[q - lo] only for q in [lo, min(limit, cap)), so no pointer below `out` is formed and nothing
// lands at or beyond out + (cap - lo).
#ifndef MI355_INFLATE_SEEK_H
#define MI355_INFLATE_SEEK_H

#include <vector>

#include "inflate_table.h"

namespace mi355 {
namespace is {

using namespace ic;

constexpr uint64_t SPACING_DEFAULT = 1ull << 20;  // output bytes between points: zran's SPAN (derived, see above)
constexpr uint64_t SPACING_MIN = it::WIN;         // (a point costs a window: closer points than a window apart store more than they save)
constexpr uint64_t SPACING_MAX = 1ull << 30;
constexpr uint32_t WSLOT_ZEROS = 0xffffffffu;     // Part::wslot of point 0: the window in front of the stream

// the decisions a mutant of the model changes (tests/inflseek)
struct Rules {
    static MI355_IC uint64_t point_pos(const Entry& e) { return e.pos; }           // the position the point rule measures an entry by
    static MI355_IC bool writes(uint64_t q, uint64_t lo) { return q >= lo; }      // pass 3's lower bound
};

// 0: the default; false: not a legal spacing
MI355_IC bool is_spacing(uint64_t given, uint64_t& spacing) {
    spacing = given ? given : SPACING_DEFAULT;
    return spacing >= SPACING_MIN && spacing <= SPACING_MAX;
}

// the entries of one piece of one range inside one launch set
struct Part {
    const uint8_t* stream;  // the framed stream, as it_decode_entry takes it
    uint64_t stream_len;
    uint8_t* out;           // where position `lo` goes
    uint64_t lo, cap;       // the piece's bytes: positions [lo, cap) of the stream's output
    uint64_t total;         // of the stream
    uint64_t base;          // the position of the piece's point: element sym_off of the set's symbols
    uint64_t sym_off;       // (a multiple of RESOLVE_RUN)
    uint32_t e0, n;         // its entries in the set
    uint32_t w0;            // its windows in the set: slot w0 + k is the window in front of its entry k
    uint32_t wslot;         // its point's window in the handle's store; WSLOT_ZEROS: point 0
    uint32_t wrapper, range;  // (range: the caller's range it is a piece of)
};  // 88 bytes
struct Set {  // one launch set
    std::vector<Entry> ents;  // (item: the part)
    std::vector<Part> parts;
    uint64_t syms = 0;        // symbol elements
    uint32_t slots = 0;       // windows
};
struct Range {  // what a caller asks for
    uint64_t off, len;
    uint8_t* out;
};
// mi355_inflate_seek_last_read
struct Counts {
    uint64_t entries, symbols, steps, sets;
};

// pread's count
MI355_IC uint64_t is_got(uint64_t off, uint64_t len, uint64_t total) { return off >= total ? 0 : (len < total - off ? len : total - off); }

// ---- device side ------------------------------------------------------------------------------------------------------------------
// pass 1: one entry, its part in hand.  cap stops the stores at the end of the piece; the entry runs on to its end, counting.
template <class P>
MI355_IC void is_decode_entry(Tables& t, uint16_t* sym, const Part& pt, const Entry& e, ic::Rec& r) {
    it::Sink o{sym + pt.sym_off, nullptr, pt.base, e.pos, pt.cap, e.pos};
    it::it_decode_entry<P>(t, pt.stream, pt.stream_len, pt.wrapper, o, e, pt.total, r);
}

// pass 3's earlier name.  Nothing in this tree uses it: host builds written against the earlier headers (tests/inflseek and
// tests/inflcut of the commit before) do, and it can go once none is left.
template <class R>
MI355_IC void is_resolve_run(const uint16_t* sym, const uint8_t* win, const Entry* ents, uint32_t n, uint64_t base, uint64_t end, uint64_t lo,
                             uint8_t* out, uint64_t q0) {
    it::it_resolve_run<R>(sym, win, ents, n, base, end, lo, out, q0);
}
// one resolve step of a set: RESOLVE_RUN symbols from element f0 on (a multiple of RESOLVE_RUN, so inside one part), through
// it_resolve_run with the part's lower bound
template <class R>
MI355_IC void is_resolve_set(const uint16_t* sym, const uint8_t* win, const Entry* ents, const Part* parts, uint32_t n_parts,
                             const uint64_t* limits, uint64_t f0) {
    if (!n_parts) return;
    const uint32_t j = it::it_part_of(parts, n_parts, f0);
    const Part& pt = parts[j];
    if (f0 < pt.sym_off || !pt.n) return;
    const uint64_t lim = limits[j];
    it::it_resolve_run<R>(sym + pt.sym_off, win + (uint64_t)pt.w0 * it::WIN, ents + pt.e0, pt.n, pt.base, lim < pt.cap ? lim : pt.cap, pt.lo,
                          pt.out, pt.base + (f0 - pt.sym_off));
}

// ---- host side of all builds ------------------------------------------------------------------------------------------------------
// the point rule: the entries that are points, ascending; pts[0] == 0
template <class R>
inline void is_points(const Entry* ents, uint64_t n, uint64_t spacing, std::vector<uint32_t>& pts) {
    pts.clear();
    if (!n) return;
    pts.push_back(0);
    uint64_t last = ents[0].pos;
    for (uint64_t k = 1; k < n; k++)
        if (R::point_pos(ents[k]) - last >= spacing && R::point_pos(ents[k]) >= last) {
            pts.push_back((uint32_t)k);
            last = ents[k].pos;
        }
}
// the last point at or before position q
inline uint32_t is_point_of(const Entry* ents, const std::vector<uint32_t>& pts, uint64_t q) {
    uint32_t lo = 0, hi = (uint32_t)pts.size();
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (ents[pts[mid]].pos <= q) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The plan of a batch of ranges: pieces, packed into launch sets in the caller's order.  A set is closed when the next piece would
// pass `budget` symbols; a piece larger than the budget is a set of its own.  Two pieces of one range never share a set: a range is
// cut only when it exceeds the budget, and each piece but the last reaches as far as the budget lets it.  So when a piece fails, the
// host drops the range's later pieces before their set is launched (is_drop) and nothing is stored beyond the failure.
// stream / out: device addresses in the device build -- nothing is read through them here.
inline void is_plan(const Entry* ents, uint64_t n, uint64_t total, const std::vector<uint32_t>& pts, const Range* ranges, uint64_t n_ranges,
                    uint64_t budget, const uint8_t* stream, uint64_t stream_len, uint32_t wrapper, std::vector<Set>& sets, Counts& cnt) {
    sets.clear();
    cnt = Counts{0, 0, 0, 0};
    const auto point_pos = [&](uint64_t i) { return i < pts.size() ? ents[pts[i]].pos : total; };
    for (uint64_t r = 0; r < n_ranges; r++) {
        const uint64_t off = ranges[r].off, end = off + is_got(off, ranges[r].len, total);
        for (uint64_t cur = off, guard = 0; cur < end && guard <= pts.size(); guard++) {
            const uint64_t i = is_point_of(ents, pts, cur);
            const uint64_t base = point_pos(i);
            uint64_t pe = end;
            if (end - base > budget) {  // cut at the farthest point the budget reaches, at the next one at least
                uint64_t c = i + 1;
                while (c < pts.size() && point_pos(c + 1) - base <= budget) c++;
                if (point_pos(c) < pe) pe = point_pos(c);
            }
            const uint32_t a = pts[i], b = it::it_entry_of(ents, (uint32_t)n, pe - 1);  // (pe > cur >= base: b >= a)
            const uint64_t syms = it::it_align(pe - base);
            if (sets.empty() || (!sets.back().parts.empty() && sets.back().syms + syms > budget)) sets.emplace_back();
            Set& s = sets.back();
            s.parts.push_back(Part{stream, stream_len, ranges[r].out + (cur - off), cur, pe, total, base, s.syms, (uint32_t)s.ents.size(), b - a + 1,
                                   s.slots, i ? (uint32_t)(i - 1) : WSLOT_ZEROS, wrapper, (uint32_t)r});
            for (uint32_t k = a; k <= b; k++) {
                s.ents.push_back(ents[k]);
                s.ents.back().item = (uint32_t)(s.parts.size() - 1);
            }
            s.syms += syms, s.slots += b - a + 2;
            cnt.entries += b - a + 1, cnt.symbols += pe - base, cnt.steps += b - a + 1;
            cur = pe;
        }
    }
    cnt.sets = sets.size();
}
// a range has failed in an earlier set: its pieces in this one store nothing (their symbols are the lead-in's only)
inline void is_drop(Set& s, const std::vector<uint8_t>& failed) {
    for (Part& pt : s.parts)
        if (failed[pt.range]) pt.cap = pt.lo;
}
// the records of one part folded into its range's record (it_report's rule); false: an entry failed
inline bool is_report(const ic::Rec* recs, const Part& pt, iw::Rec& acc) { return it::it_report(recs + pt.e0, pt.n, acc); }
// what a read leaves of a range: the bytes of out that hold data, and the record's out_pos / out_len (positions of the stream)
inline uint64_t is_give(iw::Rec& acc, uint64_t off, uint64_t len, uint64_t total) {
    const uint64_t got = is_got(off, len, total);
    if (acc.status) {
        const uint64_t v = acc.out_pos > off ? acc.out_pos - off : 0;
        return v < got ? v : got;
    }
    acc.out_pos = (off < total ? off : total) + got;
    acc.out_len = got;
    return got;
}

// the trailer of a framed stream against the sums the build folded over its groups (t: the stream's last 8 bytes, or 4 of zlib)
inline bool is_trailer_ok(uint32_t wrapper, const uint8_t* t, uint32_t adler, uint32_t crc, uint64_t total) {
    if (wrapper == 1) return ((uint32_t)t[0] << 24 | (uint32_t)t[1] << 16 | (uint32_t)t[2] << 8 | t[3]) == adler;
    if (wrapper == 2) {
        const uint32_t v = (uint32_t)t[3] << 24 | (uint32_t)t[2] << 16 | (uint32_t)t[1] << 8 | t[0];
        const uint32_t z = (uint32_t)t[7] << 24 | (uint32_t)t[6] << 16 | (uint32_t)t[5] << 8 | t[4];
        return v == crc && z == (uint32_t)total;
    }
    return true;
}
// ... and the record of a stream whose sums disagree (iw_check_trailer's)
inline void is_checksum_failed(iw::Rec& r) {
    r = iw::Rec{V_CHECKSUM, 0, 0, 0, r.end_bit, r.out_len, 0, 0, 0};
}

}  // namespace is
}  // namespace mi355
#endif
