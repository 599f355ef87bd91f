// inflate_bigmembers.h -- the large PLAIN members of a gzip file: a member that does not state its size is found and decoded in
// parallel, many members in one launch set.  The third way of producing inflate_members.h's serial walk.
//
// inflate_members.h's Path B asks its backend for chain(o, p, ...): the rows and records im_chain would produce from byte o on.
// ib_chain produces the same rows by other means and hands to im_chain what it cannot decide:
//   discover  a member at byte o: its gzip header (ib_head), then inflate_index.h's finder and walkers over a BOUNDED EXTENT of the
//             deflate data behind it -- E spans of S bytes, the grid anchored at the member's first deflate byte.  The chain from span
//             0 (ix_link's rule) ends FINAL: the member's end bit, its size and its table are known, the next member begins 8 bytes
//             behind the byte in which the BFINAL block ends.  It ends EDGE (ix::END_EDGE: a block boundary at or behind the extent's
//             edge): the extent doubles, the finder runs over the new spans only, that last link and the new spans' walkers walk, and
//             the chain goes on where it stood.  Anything else ends discovery at this member.  A member's first extent is E0 spans,
//             the threshold's worth, or what the member in front needed where the spans saved so far pay for it (ib_next_extent);
//             a member of L compressed bytes never searches 2 L / S spans or more by doubling, so a file costs 2 n / S + members x
//             E0 spans at most and not members x n / S.
//   decode    the tables of all members found, flat, cut into groups like a single stream's (it_group_end); a group holds PARTS: the
//             entries of one member that lie in it.  Three passes, inflate_table.h's, per group:
//               1. one wave per entry, its part's descriptor in hand: positions count from the MEMBER's first byte, so a distance is
//                  limited by what this member has produced and a member's first entry has nothing in front of it
//               2. one workgroup per PART: the part's window chain, from zeros or -- the group's first part, when its member began in
//                  the group before -- from the window that group left
//               3. flat over the group's symbols: the only writes of `out`, below each part's limit and its member's cap
//   judge     a member stands if every entry of it is clean and its last one ends at the bit and the size discovery found (the
//             trailer's bytes are there: the walkers' reader ends 8 bytes in front of the file's end, im_member_open's rule).  The
//             FIRST member that does not -- in discovery or in decode -- is not reported from here: im_chain goes on from its (o, p),
//             so a failure's status, bit and position are the serial walk's own.
//   small     when a member found is shorter than the threshold, discovery ends behind it and im_chain takes the rest of the call:
//             a file of many small members pays one discovery a chain call, not one a member.
// Speculation costs time and never a byte: what the passes wrote for members that do not stand lies at or behind the position where
// im_chain goes on.
//
// Safety, as in inflate_members.h: bounded reads only (the frame on an extent tested against the file's length, the walkers' and the
// entries' reader on [o + hdr, n - 8)), every loop bounded by the file's length, candidates read below the extent's edge only, a
// symbol stored only below its entry's limit and its member's cap.
#ifndef MI355_INFLATE_BIGMEMBERS_H
#define MI355_INFLATE_BIGMEMBERS_H

#include <vector>

#include "inflate_index.h"
#include "inflate_members.h"
#include "inflate_table.h"

namespace mi355 {
namespace ib {

using namespace ic;

constexpr uint64_t PAR_MIN = 1024;                        // MI355_CFG_INFLATE_MEMBER_PARALLEL_BYTES: at least, at most, default
constexpr uint64_t PAR_MAX = 1ull << 30;
constexpr uint64_t PAR_DEFAULT = 4 * ix::SPAN_DEFAULT;   // (derived: a few index spans, so that a table of two entries is likely)

// what the first round of a discovery leaves about the member's frame
struct Head {
    uint64_t hdr;               // the header's bytes (frame_ok)
    uint32_t frame_ok, hinted;  // ic_parse_frame on [o, n); im_hint at o
};
struct Link {  // a row of a member's table
    uint64_t bit, bytes;
};
struct Found {  // a member as discovery leaves it
    uint64_t o, p;             // its first byte in the file, its first byte in the output
    uint64_t hdr, data_len;    // the reader's extent: [o + hdr, o + hdr + data_len)
    uint64_t end_bit, total;   // where the BFINAL block ends, the member's size
    uint64_t in_len;           // header through trailer
    uint64_t first, count;     // its rows in the links
};
// the entries of one member inside one group
struct Part {
    const uint8_t* data;  // the member's deflate data and the reader's extent
    uint64_t nbytes;
    uint8_t* out;         // where the member's position 0 goes
    uint64_t cap, total;  // of the member, counted like its positions
    uint64_t base;        // the position of the part's first entry: element sym_off of the group's symbols
    uint64_t sym_off;     // (a multiple of RESOLVE_RUN)
    uint32_t e0, n;       // its entries in the group
    uint32_t carried;     // the window in front of its first entry is the one the group before left (slot 0)
    uint32_t pad;
};  // 72 bytes
struct Plan {  // one group
    std::vector<Entry> ents;  // (item: the part)
    std::vector<Part> parts;
    uint64_t syms = 0;        // symbol elements
    bool carry_out = false;   // the last part's member goes on in the next group
};
// mi355_inflate_members_last_parallel
struct Stats {
    uint64_t parallel, handed, spans, walkers, entries, sets;
};

// the decisions a mutant of the model changes (tests/inflbig)
struct Rules {
    static MI355_IC uint64_t trailer_at(uint64_t end_bit) { return (end_bit + 7) / 8; }  // deflate bytes in front of the trailer
    static MI355_IC uint64_t origin(uint64_t p) { return 0 * p; }                        // where a member's positions begin to count
};

// the spans of a member's first extent: the threshold's worth, one at least ...
MI355_IC uint64_t ib_first_extent(uint64_t threshold, uint64_t S) {
    const uint64_t e = threshold / S;
    return e ? e : 1;
}
// ... or, behind a member of this launch set that needed `prev` spans, that many and an eighth more -- members of one file are often of
// one size, and a round of discovery is two launches and a wait -- as far as the set's CREDIT allows: twice the spans of the bytes
// walked so far less the spans searched so far, so that the spans searched stay below 2 n / S + members x first extent whatever the
// sizes are.  (A member that is larger after all doubles its extent from there: below twice what it needs, as from any start.)
MI355_IC uint64_t ib_next_extent(uint64_t first, uint64_t prev, uint64_t walked_bytes, uint64_t searched, uint64_t S) {
    const uint64_t earned = 2 * (walked_bytes / S), credit = earned > searched ? earned - searched : 0;
    uint64_t want = prev + prev / 8 + 1;
    if (want > credit) want = credit;
    return want > first ? want : first;
}

// ---- discovery, device side ------------------------------------------------------------------------------------------------------
template <class P>
MI355_IC void ib_head(const uint8_t* s, uint64_t n, uint64_t o, Head& h) {
    uint64_t hdr = 0, trailer = 0, t;
    uint32_t z;
    h.frame_ok = o < n && ic_parse_frame(s + o, n - o, 2, hdr, trailer) ? 1u : 0u;
    h.hdr = hdr;
    h.hinted = im::im_hint<P>(s, n, o, t, z) ? 1u : 0u;
}
// span k's candidate on the grid of the member at o (o < n)
template <class P>
MI355_IC uint64_t ib_find_span(Tables& t, const uint8_t* s, uint64_t n, uint64_t o, uint64_t k, uint64_t S) {
    return ix::ix_find_span<P>(t, s + o, n - o, 2, k, S);
}
// span k's walker in an extent of `edge` spans (sibling of ix_walk_span: the frame of the member at o, the edge)
template <class P>
MI355_IC void ib_walk_span(Tables& t, const uint8_t* s, uint64_t n, uint64_t o, const uint64_t* cand, uint64_t S, uint64_t k, uint64_t edge,
                           ix::Walk& r) {
    const uint64_t c = k < edge ? cand[k] : ix::NOCAND;
    r = ix::Walk{c, 0, 0, ix::END_NONE, 0, 0, V_OK, 0, 0, 0, 0, 0, 0, 0};
    if (c == ix::NOCAND) return;
    uint64_t hdr, trailer;
    if (o >= n || !ic_parse_frame(s + o, n - o, 2, hdr, trailer)) {
        r.how = ix::END_FAILED, r.status = V_FRAME;
        return;
    }
    ix::ix_walk_to<P>(t, s + o + hdr, n - o - hdr - trailer, cand, edge, S, k, c, edge, r);
}

// ---- the three passes over a group of parts, device side ------------------------------------------------------------------------------
// pass 1: one entry, its part in hand
template <class P>
MI355_IC void ib_decode_entry(Tables& t, uint16_t* sym, const Part& pt, const Entry& e, ic::Rec& r) {
    it::Sink o{sym + pt.sym_off, nullptr, pt.base, e.pos, pt.cap, e.pos};
    it::it_entry<P>(t, pt.data, pt.nbytes, o, e, pt.total, r);
}
// pass 3: one resolve step: RESOLVE_RUN symbols from element f0 on (a multiple of RESOLVE_RUN, so inside one part)
MI355_IC void ib_resolve_run(const uint16_t* sym, const uint8_t* win, const Entry* ents, const Part* parts, uint32_t n_parts,
                             const uint64_t* limits, uint64_t f0) {
    if (!n_parts) return;
    const uint32_t j = it::it_part_of(parts, n_parts, f0);
    const Part& pt = parts[j];
    if (f0 < pt.sym_off || !pt.n) return;
    const uint64_t lim = limits[j];
    it::it_resolve_run(sym + pt.sym_off, win + (uint64_t)pt.e0 * it::WIN, ents + pt.e0, pt.n, pt.base, lim < pt.cap ? lim : pt.cap, 0, pt.out,
                       pt.base + (f0 - pt.sym_off));
}

// ---- host side of all builds ------------------------------------------------------------------------------------------------------
// One member from byte o on.  The backend's head(o, head): ib_head alone.  Its round(o, first, rewalk, k_lo, k_hi, head, w): the finder over spans [k_lo, k_hi) -- first:
// and the head, span 0's candidate with it --, then the walkers of span `rewalk` and of [k_lo, k_hi) in an extent of k_hi spans, their
// records into w.  ok: the member is found, its rows appended to the links.  stop_hinted: a hinted header ends it behind the head.
template <class R, class B>
inline int ib_discover(B& be, uint64_t n, uint64_t S, uint64_t o, uint64_t p, uint64_t first_extent, bool stop_hinted, Head& head,
                       std::vector<Link>& links, Found& f, iw::Rec& rec, bool& ok, Stats& st) {
    ok = false;
    head = Head{0, 0, 0};
    const size_t keep = links.size();
    const uint64_t n_all = ix::ix_n_spans(n - o, S);  // (the frame's bytes make it a span too many at most)
    uint64_t E = first_extent < n_all ? first_extent : n_all;
    // the head alone first: a bad frame, or a hinted header where the chain stops at one, costs no round
    if (const int rc = be.head(o, head)) return rc;
    if (!head.frame_ok || (stop_hinted && head.hinted)) return 0;
    std::vector<ix::Walk> w(E);
    if (const int rc = be.round(o, true, 0, 1, E, head, w)) return rc;
    st.spans += E, st.walkers += E;
    if (!head.frame_ok) return 0;  // (never: the same bytes)
    if (head.hdr > n - o || n - o - head.hdr < 8) return 0;  // (never: the frame parser left room for the trailer)
    rec = iw::Rec{V_OK, 0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t k = 0, sum = 0;
    for (uint64_t guard = 0; guard < 2 * n_all + 128; guard++) {  // (a turn follows a link or doubles the extent)
        const ix::Walk x = w[k];
        if (x.how == ix::END_EDGE) {
            if (E >= n_all) break;  // (never: no boundary lies behind the data)
            const uint64_t E2 = E > n_all / 2 ? n_all : 2 * E;
            w.resize(E2);
            if (const int rc = be.round(o, false, k, E, E2, head, w)) return rc;
            st.spans += E2 - E, st.walkers += E2 - E + 1;
            E = E2;
            continue;
        }
        if (x.how != ix::END_LINK && x.how != ix::END_FINAL) break;
        links.push_back(Link{x.start, x.count});
        sum += x.count;
        rec.n_blocks += x.n_blocks, rec.n_stored += x.n_stored, rec.n_fixed += x.n_fixed, rec.n_dynamic += x.n_dynamic;
        if (x.how == ix::END_FINAL) {
            const uint64_t data_len = n - o - head.hdr - 8;
            const uint64_t in_len = head.hdr + R::trailer_at(x.end_bit) + 8;
            if (in_len > n - o) break;  // (never: the reader ends in front of the file's last 8 bytes)
            f = Found{o, p, head.hdr, data_len, x.end_bit, sum, in_len, keep, links.size() - keep};
            rec.out_pos = rec.out_len = sum, rec.end_bit = x.end_bit;
            ok = true;
            return 0;
        }
        if (x.link <= k || x.link >= E || w[x.link].how == ix::END_NONE) break;  // (never, from these kernels)
        k = x.link;
    }
    links.resize(keep);
    return 0;
}

// the entries of the members found, flat, in file order (item: the member's index in `found`)
template <class R>
inline void ib_entries(const std::vector<Found>& found, const std::vector<Link>& links, std::vector<Entry>& all) {
    all.clear();
    for (size_t m = 0; m < found.size(); m++) {
        const Found& f = found[m];
        uint64_t pos = R::origin(f.p);
        for (uint64_t k = 0; k < f.count; k++) {
            const Link& l = links[f.first + k];
            const bool last = k + 1 == f.count;
            all.push_back(Entry{l.bit, pos, last ? 0 : links[f.first + k + 1].bit, last ? 0 : pos + l.bytes, last ? 1u : 0u, (uint32_t)m});
            pos += l.bytes;
        }
    }
}
// the group of entries [k0, k1) of `all` as parts.  s / out / out_cap: the file and the call's output (device addresses in the
// device build: nothing is read through them here)
template <class R>
inline void ib_plan(const std::vector<Found>& found, const std::vector<Entry>& all, uint64_t k0, uint64_t k1, const uint8_t* s, uint8_t* out,
                    uint64_t out_cap, Plan& g) {
    g.ents.assign(all.begin() + k0, all.begin() + k1);
    g.parts.clear();
    g.syms = 0;
    const auto close = [&]() {
        Part& pt = g.parts.back();
        const Entry& e = g.ents[pt.e0 + pt.n - 1];
        const uint64_t end = e.last ? pt.total : e.next_pos;
        const uint64_t stored = pt.base < pt.cap ? (end < pt.cap ? end : pt.cap) - pt.base : 0;
        g.syms += it::it_align(stored);
    };
    for (uint64_t f = k0; f < k1; f++) {
        const uint32_t m = all[f].item;
        if (f == k0 || all[f - 1].item != m) {
            if (!g.parts.empty()) close();
            const Found& F = found[m];
            const uint64_t org = R::origin(F.p);
            const bool carried = f != 0 && all[f - 1].item == m;  // (f == k0: the member began in the group before)
            g.parts.push_back(Part{s + F.o + F.hdr, F.data_len, im::im_out_at(out, out_cap, F.p) - org, im::im_room_at(out_cap, F.p) + org,
                                   F.total + org, all[f].pos, g.syms, (uint32_t)(f - k0), 0u, carried ? 1u : 0u, 0u});
        }
        g.parts.back().n++;
        g.ents[f - k0].item = (uint32_t)(g.parts.size() - 1);
    }
    if (!g.parts.empty()) close();
    g.carry_out = k1 < all.size() && k1 > k0 && all[k1].item == all[k1 - 1].item;
}

// The chain launch of im_run by other means.  The backend B:
//   head(...) round(...)                                   see ib_discover
//   decode(plan, first, recs)                              the three passes over one group; first: no group of this set ran before
//   serial(o, p, ignore_hints, behind, room, rows, recs, end)   im_chain_behind
//   threshold() span() group_bytes()                       the settings
// rows / recs / e: what im_chain(o, p, ...) with `room` rows would leave (a failing member's row comes from im_chain itself).
template <class R, class B>
inline int ib_chain(B& be, const uint8_t* s, uint64_t n, uint64_t o, uint64_t p, uint8_t* out, uint64_t out_cap, bool ignore_hints, uint32_t room,
                    std::vector<im::Member>& rows, std::vector<iw::Rec>& recs, im::ChainEnd& e, Stats& st) {
    rows.clear(), recs.clear();
    const uint64_t T = be.threshold(), S = be.span();
    std::vector<Found> found;
    std::vector<iw::Rec> frecs;
    std::vector<Link> links;
    uint64_t co = o, cp = p, prev_spans = 0;
    const uint64_t searched0 = st.spans, E0 = ib_first_extent(T, S);
    uint32_t how = im::STOP_ROOM;
    bool hand = false, small = false;
    // discover
    for (uint64_t guard = 0; guard <= room; guard++) {
        if (co >= n) {
            how = im::STOP_FILE;
            break;
        }
        if (found.size() >= room) break;
        if (small || n - co < T) {
            hand = true;
            break;
        }
        Head head;
        Found f;
        iw::Rec r;
        bool ok;
        const uint64_t extent = found.empty() ? E0 : ib_next_extent(E0, prev_spans, co - o, st.spans - searched0, S);
        if (const int rc = ib_discover<R>(be, n, S, co, cp, extent, !found.empty() && !ignore_hints, head, links, f, r, ok, st)) return rc;
        if (!found.empty() && !ignore_hints && head.hinted) {
            how = im::STOP_HINT;
            break;
        }
        if (!ok) {
            hand = true;
            break;
        }
        found.push_back(f), frecs.push_back(r);
        co += f.in_len, cp += f.total;
        prev_spans = ix::ix_n_spans((f.end_bit + 7) / 8, S);
        small = f.in_len < T;
    }
    // decode, group after group, up to the first group that holds a failure; judge
    std::vector<Entry> all;
    ib_entries<R>(found, links, all);
    std::vector<uint8_t> clean(found.size(), 1);
    std::vector<ic::Rec> got;
    Plan g;
    bool failed = false;
    for (uint64_t k0 = 0, k1; k0 < all.size() && !failed; k0 = k1) {
        k1 = it::it_group_end([&](uint64_t k) { return links[k].bytes; }, all.size(), k0, be.group_bytes());  // (all[k] is links[k])
        ib_plan<R>(found, all, k0, k1, s, out, out_cap, g);
        if (const int rc = be.decode(g, k0 == 0, got)) return rc;
        st.entries += k1 - k0, st.sets++;
        for (uint64_t k = k0; k < k1; k++) {
            const ic::Rec& r = got[k - k0];
            const Found& F = found[all[k].item];
            bool good = r.status == V_OK;
            if (good && all[k].last) good = r.end_bit == F.end_bit && r.end_pos == F.total + R::origin(F.p);
            if (!good) clean[all[k].item] = 0, failed = true;
        }
        if (failed)
            for (size_t m = all[k1 - 1].item + 1; m < found.size(); m++) clean[m] = 0;  // (not decoded)
    }
    size_t acc = 0;
    while (acc < found.size() && clean[acc]) acc++;
    for (size_t m = 0; m < acc; m++) {
        rows.push_back(im::Member{found[m].o, found[m].in_len, found[m].p, found[m].total, 0u, V_OK});
        recs.push_back(frecs[m]);
    }
    st.parallel += acc;
    if (acc < found.size()) hand = true, co = found[acc].o, cp = found[acc].p;
    e = im::ChainEnd{co, cp, (uint32_t)acc, how};
    if (!hand || acc >= room) return 0;
    std::vector<im::Member> srows;
    std::vector<iw::Rec> srecs;
    im::ChainEnd se;
    if (const int rc = be.serial(co, cp, ignore_hints, (uint32_t)acc, room - (uint32_t)acc, srows, srecs, se)) return rc;
    for (uint32_t i = 0; i < se.count; i++) rows.push_back(srows[i]), recs.push_back(srecs[i]);
    st.handed += se.count;
    e = im::ChainEnd{se.o, se.p, (uint32_t)acc + se.count, se.how};
    return 0;
}

}  // namespace ib
}  // namespace mi355
#endif
