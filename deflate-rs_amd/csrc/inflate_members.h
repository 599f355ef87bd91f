// inflate_members.h -- a gzip FILE: a sequence of members (RFC 1952 2.2), decoded member after member, BGZF members in parallel.
//
// The member entry points (include/mi355_deflate.h mi355_inflate_members*) run this text: the four kernels of
// deflate_members_inflate.inc and the host build of tests/inflmembers/.  The contract is the SERIAL WALK: member m begins at byte o
// of the file, its header is ic_parse_frame's gzip header on stream[o, stream_len), its deflate blocks run through the BFINAL block by
// iw_inflate's rules, the 8 trailer bytes follow the byte in which that block ends, the next member begins behind them; the walk ends
// at the end of the file or at the first failure.  Whatever path produced a result, it is this walk's.
//   Path A  a run of HINTED members -- members that state their own size in a 'BC' extra subfield, as BGZF's do (im_hint) -- is found
//           without decoding anything: the file is cut into SPANS of S compressed bytes;
//             find  one wave per span: the span's CANDIDATE, the smallest byte offset in it that is hinted
//             walk  one lane per candidate hops pos += total while pos is hinted, counting members and summing ISIZE, until pos is the
//                   candidate of a later span (link), the end of the file, or a byte that is not hinted (open)
//             link  on the host, from the span that holds the run's start o (whose candidate is o itself): that chain is the run
//             fill  one lane per walker on the chain hops again and writes (offset, size, ISIZE) rows at its index
//           and its members are decoded by the batched one-wave inflate, member k into out + the sum of the ISIZEs in front of it under
//           the cap min(room left, ISIZE).  A hint is a claim: the run is ACCEPTED up to the first member that is not both structurally
//           clean and exactly ISIZE bytes long -- a clean member ends in the last byte in front of its trailer, so its BSIZE was true,
//           and with a true ISIZE the next member's offset was true as well -- and from that member on Path B decides.
//   Path B  im_member_open: a member decoded without being told where it ends, one after the other by one wave (im_chain), until the
//           end of the file, a failure, a full table, or -- behind at least one member -- a hinted header, where Path A resumes.  A call
//           resumes at most RESUMES times; after that hints are ignored, which bounds the launches and changes no result.
// Speculation costs time and never a byte: what Path A wrote for members it did not accept lies at or behind the output position
// where Path B goes on, and Path B writes every byte from there on again, or the call fails and those bytes are unspecified.
//
// Safety, as in inflate_check.h: the file is read through bounded reads only (im_byte, ic_load64, ic_parse_frame on an extent that
// was tested against the file's length), every loop is bounded by the file's length, and every store goes through iw's sink.
#ifndef MI355_INFLATE_MEMBERS_H
#define MI355_INFLATE_MEMBERS_H

#include <vector>

#include "inflate_write.h"

namespace mi355 {
namespace im {

using namespace ic;

constexpr uint64_t NOCAND = ~0ull;          // a span without a candidate
constexpr uint64_t SPAN_MIN = 16;           // MI355_CFG_INFLATE_MEMBER_SPAN_BYTES: at least, at most, default
constexpr uint64_t SPAN_MAX = 1ull << 30;
constexpr uint64_t SPAN_DEFAULT = 65536;    // (derived: a BGZF member is 64 KiB at most, so every interior span holds a true start)
constexpr uint32_t HINTED = 1;              // MI355_MEMBER_HINTED
constexpr uint32_t RESUMES = 8;             // Path A resumes of one call
constexpr uint64_t HOP_MIN = 26;            // a hinted member: 12 header bytes, the 6 of its subfield, 8 of trailer
enum : uint32_t { END_LINK = 0, END_FILE = 1, END_OPEN = 2, END_NONE = 3 };       // how a walker stopped (NONE: nothing walked)
enum : uint32_t { STOP_FILE = 0, STOP_FAIL = 1, STOP_ROOM = 2, STOP_HINT = 3 };   // how a chain launch stopped

struct Member {  // mi355_member_info
    uint64_t in_off, in_len, out_off, out_len;
    uint32_t flags, status;
};  // 40 bytes
struct Hint {  // a row of the fill: a member as its header claims it
    uint64_t in_off;
    uint32_t in_len, isize;
};  // 16 bytes
struct Walk {
    uint64_t start, end;            // the candidate; where the walker stopped
    uint64_t n_members, out_bytes;  // members hopped over, the sum of their ISIZEs
    uint32_t how, link;             // END_*; the span linked to
};  // 40 bytes
struct Seg {  // a walker on the chain, for the fill: where it starts, its first row, its rows
    uint64_t start, first, count;
};
struct ChainEnd {
    uint64_t o, p;        // where the next member begins, the output position there
    uint32_t count, how;  // rows written (a failing member's included); STOP_*
};

// the three decisions a mutant of the model changes (tests/inflmembers)
struct Rules {
    static MI355_IC uint64_t total(uint32_t bsize) { return (uint64_t)bsize + 1; }
    static MI355_IC bool stop(uint64_t pos, uint64_t c) { return pos == c; }
    static MI355_IC bool first() { return true; }  // the finder takes the span's FIRST hinted offset
};

MI355_IC uint64_t im_n_spans(uint64_t n, uint64_t S) {
    const uint64_t k = n / S + (n % S ? 1 : 0);
    return k ? k : 1;
}
MI355_IC uint32_t im_byte(const uint8_t* s, uint64_t n, uint64_t at) { return at < n ? s[at] : 0u; }

// ---- a hinted member ---------------------------------------------------------------------------------------------------------------
// the four fixed bytes: magic, CM 8, the reserved FLG bits clear and FEXTRA set (register only; the finder's prefilter)
MI355_IC bool im_fixed4(const uint8_t* s, uint64_t n, uint64_t o) {
    if (o >= n || n - o < 4) return false;
    uint32_t v;
    __builtin_memcpy(&v, s + o, 4);
    return (v & 0xE4FFFFFFu) == 0x04088B1Fu;
}
// Is a member hinted at byte o?  total: its claimed extent, header through trailer; isize: the last four bytes of that extent.
template <class P>
MI355_IC bool im_hint(const uint8_t* s, uint64_t n, uint64_t o, uint64_t& total, uint32_t& isize) {
    total = 0, isize = 0;
    if (!im_fixed4(s, n, o) || n - o < 18) return false;
    const uint64_t qe = o + 12 + (im_byte(s, n, o + 10) | (uint64_t)im_byte(s, n, o + 11) << 8);
    uint64_t q = o + 12;
    uint32_t bsize = 0;
    bool found = false;
    for (uint32_t guard = 0; guard < 16384 && q + 4 <= qe && !found; guard++) {  // (XLEN / 4 subfields at most)
        const uint64_t slen = im_byte(s, n, q + 2) | (uint64_t)im_byte(s, n, q + 3) << 8;
        if (im_byte(s, n, q) == 'B' && im_byte(s, n, q + 1) == 'C' && slen == 2 && q + 6 <= qe) {
            bsize = im_byte(s, n, q + 4) | im_byte(s, n, q + 5) << 8;
            found = true;
        }
        q += 4 + slen;
    }
    if (!found) return false;
    const uint64_t t = P::total(bsize);
    if (t > n - o) return false;
    uint64_t hdr, trailer;
    if (!ic_parse_frame(s + o, t, 2, hdr, trailer)) return false;  // (t >= 26 behind this: 12 + 6 + 8)
    total = t;
    isize = im_byte(s, n, o + t - 4) | im_byte(s, n, o + t - 3) << 8 | im_byte(s, n, o + t - 2) << 16 | im_byte(s, n, o + t - 1) << 24;
    return true;
}

// ---- find: span k's candidate.  P::survivors(s, n, base, end): bit l set = offset base + l is below `end` and passes im_fixed4 ------
template <class P>
MI355_IC uint64_t im_find(const uint8_t* s, uint64_t n, uint64_t k, uint64_t S) {
    if (k >= im_n_spans(n, S) || k * S >= n) return NOCAND;
    const uint64_t lo = k * S, end = n - lo > S ? lo + S : n;
    uint64_t c = NOCAND;
    for (uint64_t base = lo; base < end; base += 64) {  // (S / 64 steps at most)
        uint64_t m = P::survivors(s, n, base, end);
        for (uint32_t guard = 0; guard < 64 && m; guard++) {
            const uint32_t l = (uint32_t)__builtin_ctzll(m);
            m &= m - 1;
            uint64_t t;
            uint32_t z;
            if (!im_hint<P>(s, n, base + l, t, z)) continue;
            c = base + l;
            if (P::first()) return c;
        }
    }
    return c;
}

// ---- walk: the hops of span k's walker from c on (the run's start o in its own span, else the span's candidate) --------------------
template <class P>
MI355_IC void im_walk(const uint8_t* s, uint64_t n, const uint64_t* cand, uint64_t n_spans, uint64_t S, uint64_t k, uint64_t c, Walk& r) {
    r = Walk{c, c, 0, 0, END_NONE, 0};
    if (c == NOCAND) return;
    r.how = END_OPEN;
    uint64_t pos = c;
    for (uint64_t guard = 0; guard <= n / HOP_MIN; guard++) {  // (a hop advances HOP_MIN bytes at least)
        if (pos >= n) {
            r.how = END_FILE;
            break;
        }
        const uint64_t j = pos / S;
        if (guard && j > k && j < n_spans && P::stop(pos, cand[j])) {
            r.how = END_LINK, r.link = (uint32_t)j;
            break;
        }
        uint64_t t;
        uint32_t z;
        if (!im_hint<P>(s, n, pos, t, z)) break;
        pos += t, r.n_members++, r.out_bytes += z;
    }
    r.end = pos;
}
// what lane k of the walk kernel does for a run that starts at o: spans in front of o's are not walked
template <class P>
MI355_IC void im_walk_span(const uint8_t* s, uint64_t n, const uint64_t* cand, uint64_t n_spans, uint64_t S, uint64_t o, uint64_t k, Walk& r) {
    const uint64_t k0 = o / S;
    im_walk<P>(s, n, cand, n_spans, S, k, k < k0 ? NOCAND : k == k0 ? o : cand[k], r);
}
// ---- fill: the rows of one walker on the chain -----------------------------------------------------------------------------------------
template <class P>
MI355_IC void im_fill(const uint8_t* s, uint64_t n, const Seg& g, Hint* rows, uint64_t n_rows) {
    uint64_t pos = g.start;
    for (uint64_t i = 0; i < g.count && g.first + i < n_rows; i++) {
        uint64_t t;
        uint32_t z;
        const bool ok = im_hint<P>(s, n, pos, t, z);  // (true: the walker hopped here)
        rows[g.first + i] = Hint{pos, ok ? (uint32_t)t : 0u, z};
        pos += t;
    }
}

// ---- link: host side of all builds ----------------------------------------------------------------------------------------------------
// The chain from span k0: emit(span) for every walker on it, in file order.  (A link leads to a later span that has a walker:
// anything else -- never, from these kernels -- ends the chain.)
template <class Emit>
inline void im_link(const Walk* w, uint64_t n_spans, uint64_t k0, Emit emit) {
    uint64_t k = k0;
    for (uint64_t guard = 0; guard < n_spans && k < n_spans; guard++) {
        emit(k);
        if (w[k].how != END_LINK || w[k].link <= k || w[k].link >= n_spans || w[w[k].link].how == END_NONE) return;
        k = w[k].link;
    }
}

// ---- Path B: one member from byte o on, open ended (sibling of iw_inflate: its frame, its block loop, its record) ---------------------
// out / cap: where THIS member's bytes go and how many fit; the record counts from the member's first byte and first deflate bit.
// in_len: header through trailer (OK only).  The last 8 bytes of the file can only be a trailer, so the bit reader ends in front of
// them: bits needed from there on are TRUNCATED, as they are for mi355_inflate.
template <class P>
MI355_IC void im_member_open(Tables& t, const uint8_t* s, uint64_t n, uint64_t o, uint8_t* out, uint64_t cap, iw::Rec& r, uint64_t& in_len) {
    r = iw::Rec{V_FRAME, 0, 0, 0, 0, 0, 0, 0, 0};
    in_len = 0;
    uint64_t hdr, trailer;
    if (o >= n || !ic_parse_frame(s + o, n - o, 2, hdr, trailer)) return;
    Bits b = ic_bits(s + o + hdr, n - o - hdr - trailer, 0);
    iw::Sink sink{out, cap, 0};
    uint64_t p = 0;
    bool fixed_ready = false, done = false;
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
            f = iw::iw_stored_block<P>(b, sink, p);
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
            f = iw::iw_huffman_block<P>(t, b, sink, p);
        }
        if (f.status) break;
        r.n_blocks++;
        if (bfinal) {
            done = true;
            break;
        }
        f = ic_fail(V_TRUNCATED, b.pos, p);  // (what is reported if the guard runs out)
    }
    if (done) {
        r.status = V_OK, r.bit = 0, r.out_pos = r.out_len = p, r.end_bit = b.pos;
        in_len = hdr + (b.pos + 7) / 8 + trailer;  // (the trailer's 8 bytes are there: the reader ended in front of them)
        return;
    }
    r = iw::Rec{f.status, 0, 0, 0, f.bit, f.in_pos, 0, 0, 0};
}

// where member bytes for the output position p go: nothing is addressed at or beyond out_cap
MI355_IC uint8_t* im_out_at(uint8_t* out, uint64_t out_cap, uint64_t p) { return p < out_cap ? out + p : out; }
MI355_IC uint64_t im_room_at(uint64_t out_cap, uint64_t p) { return p < out_cap ? out_cap - p : 0; }

// what the one wave of the chain kernel does: members from (o, p) on into rows[0, room) / recs[0, room).  behind: members that the
// same launch set has walked in front of o by other means (inflate_bigmembers.h) -- a hinted header at o itself then stops the chain too
template <class P>
MI355_IC void im_chain_behind(Tables& t, const uint8_t* s, uint64_t n, uint64_t o, uint64_t p, uint8_t* out, uint64_t out_cap, bool ignore_hints,
                              uint32_t behind, Member* rows, iw::Rec* recs, uint32_t room, ChainEnd& e) {
    e = ChainEnd{o, p, 0, STOP_ROOM};
    for (uint32_t m = 0; m < room; m++) {
        uint64_t t_, in_len;
        uint32_t z_;
        if ((m || behind) && !ignore_hints && im_hint<P>(s, n, e.o, t_, z_)) {
            e.how = STOP_HINT;
            return;
        }
        iw::Rec r;
        im_member_open<P>(t, s, n, e.o, im_out_at(out, out_cap, e.p), im_room_at(out_cap, e.p), r, in_len);
        P::sync();  // (the next member builds its tables in the same room)
        if (P::leader()) {
            rows[m] = Member{e.o, in_len, e.p, r.status ? r.out_pos : r.out_len, 0u, r.status};
            recs[m] = r;
        }
        e.count = m + 1;
        if (r.status) {
            e.how = STOP_FAIL;
            return;
        }
        e.o += in_len, e.p += r.out_len;
        if (e.o >= n) {
            e.how = STOP_FILE;
            return;
        }
    }
}
template <class P>
MI355_IC void im_chain(Tables& t, const uint8_t* s, uint64_t n, uint64_t o, uint64_t p, uint8_t* out, uint64_t out_cap, bool ignore_hints,
                       Member* rows, iw::Rec* recs, uint32_t room, ChainEnd& e) {
    im_chain_behind<P>(t, s, n, o, p, out, out_cap, ignore_hints, 0u, rows, recs, room, e);
}

// ---- the call: host side of all builds ----------------------------------------------------------------------------------------------------
// The backend B is the device (deflate_members_inflate.inc) or the host build's loops; every method returns 0 or the call's error:
//   find(n_spans)                                 the candidates, kept by the backend
//   walk(o, w)                                    n_spans walkers' records for a run that starts at o
//   fill(segs, n_rows, rows)                      the rows of the chain's walkers
//   decode(rows, k, p, recs)                      k hinted members by the batched one-wave inflate, the first at output position p
//   chain(o, p, ignore_hints, rows, recs, end)    one launch of Path B
// mem / recs: one entry per member walked, a failing last one included; recs count from their member's start.
template <class B>
inline int im_run(B& be, uint64_t n, uint64_t S, std::vector<Member>& mem, std::vector<iw::Rec>& recs) {
    mem.clear(), recs.clear();
    if (n == 0) {  // an empty file: member 0 has no header
        mem.push_back(Member{0, 0, 0, 0, 0u, V_FRAME});
        recs.push_back(iw::Rec{V_FRAME, 0, 0, 0, 0, 0, 0, 0, 0});
        return 0;
    }
    const uint64_t n_spans = im_n_spans(n, S);
    uint64_t o = 0, p = 0;
    uint32_t resumes = 0;
    bool path_a = true, found = false;
    std::vector<Walk> w;
    std::vector<Seg> segs;
    std::vector<Hint> rows;
    std::vector<Member> crows;
    std::vector<iw::Rec> got;
    while (o < n) {  // (every turn of Path B walks a member or ends the call)
        if (path_a) {
            path_a = false;
            if (!found)
                if (const int rc = be.find(n_spans)) return rc;
            found = true;
            if (const int rc = be.walk(o, w)) return rc;
            segs.clear();
            uint64_t cnt = 0;
            im_link(w.data(), n_spans, o / S, [&](uint64_t k) {
                if (w[k].n_members) segs.push_back(Seg{w[k].start, cnt, w[k].n_members});
                cnt += w[k].n_members;
            });
            if (!cnt) continue;
            if (const int rc = be.fill(segs, cnt, rows)) return rc;
            bool open = false;
            for (uint64_t done = 0; done < cnt && !open;) {
                const uint64_t g = cnt - done < be.group() ? cnt - done : be.group();
                if (const int rc = be.decode(rows.data() + done, g, p, got)) return rc;
                for (uint64_t i = 0; i < g && !open; i++) {
                    const Hint& h = rows[done + i];
                    const iw::Rec& r = got[i];
                    if (r.status != V_OK || r.out_len != h.isize || h.in_off != o) {
                        open = true;  // not clean, or not ISIZE bytes long: the walk decides from here
                        break;
                    }
                    mem.push_back(Member{h.in_off, h.in_len, p, r.out_len, HINTED, V_OK});
                    recs.push_back(r);
                    o = h.in_off + h.in_len, p += r.out_len;
                }
                done += g;
            }
            continue;
        }
        ChainEnd e;
        if (const int rc = be.chain(o, p, resumes >= RESUMES, crows, got, e)) return rc;
        for (uint32_t i = 0; i < e.count; i++) mem.push_back(crows[i]), recs.push_back(got[i]);
        if (e.how == STOP_FAIL) break;
        if (e.how != STOP_HINT && e.how != STOP_ROOM && e.how != STOP_FILE) break;  // (never)
        if (e.count == 0 && e.how != STOP_HINT) break;                             // (never: a launch walks a member at least)
        o = e.o, p = e.p;
        if (e.how == STOP_HINT) resumes++, path_a = true;
    }
    return 0;
}

// is member j's checksum judged?  It is clean and all of it was stored.
inline bool im_judged(const Member& m, uint64_t out_cap) { return m.status == V_OK && m.out_off + m.out_len <= out_cap; }
// the members' total, if no member failed its structure
inline bool im_total(const std::vector<Member>& mem, uint64_t& total) {
    total = mem.empty() ? 0 : mem.back().out_off + mem.back().out_len;
    return !mem.empty() && mem.back().status == V_OK;
}

// The end of a call, behind the checksum pass (which has turned the records of judged members whose trailer disagrees into CHECKSUM;
// it is skipped, and nothing is judged, when the file is structurally valid and longer than out_cap): the first failure in file
// order cuts the table behind it, and the report and return value follow mi355_inflate's.  R: mi355_inflate_report.
template <class R>
inline int im_report(std::vector<Member>& mem, const std::vector<iw::Rec>& recs, uint64_t out_cap, R& rep, uint64_t* valid) {
    iw::Rec acc{V_OK, 0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t j = 0; j < mem.size(); j++) {
        const iw::Rec& r = recs[j];
        if (r.status) {
            mem[j].status = r.status;  // (CHECKSUM: a member Path A accepted stays HINTED, its size was true)
            acc = iw::Rec{r.status, 0, 0, 0, r.bit, mem[j].out_off + r.out_pos, 0, 0, 0};
            mem.resize(j + 1);
            return iw::iw_report(acc, out_cap, rep, valid);
        }
        acc.n_blocks += r.n_blocks, acc.n_stored += r.n_stored, acc.n_fixed += r.n_fixed, acc.n_dynamic += r.n_dynamic;
        acc.out_pos = acc.out_len = mem[j].out_off + mem[j].out_len, acc.end_bit = r.end_bit;
    }
    return iw::iw_report(acc, out_cap, rep, valid);
}

}  // namespace im
}  // namespace mi355
#endif
