// bgzf_read.h -- BGZF reads: byte ranges of the uncompressed data of a blocked gzip file, decoding only the members that hold them.
//
// The BGZF read entry points (include/mi355_deflate.h mi355_bgzf_index_*, mi355_bgzf_read*) run this text: the kernel and its driver
// (deflate_bgzf_read.inc) and the host build of tests/bgzfread/.  What is here:
//   the INDEX    the member table (in_off, in_len, out_off, out_len) in host memory, made from a table somebody holds (br_from_members)
//                or from the file's own claims by Path A of inflate_members.h -- find, walk, link, fill from byte 0, nothing decoded
//                (br_build) --, and htslib's virtual offsets over it (br_voffset, br_uoffset)
//   the PLAN     from the ranges of a call to DISTINCT members: a member is decoded once however many ranges want parts of it.  A
//                member wanted by exactly one range that covers all of it goes IN PLACE, decoded straight into that range's buffer;
//                every other member goes into a 16-byte aligned SCRATCH slot of align_up(out_len, 16) bytes and carries a list of
//                PIECES (lo, hi, dst), one per range that wants [lo, hi) of it.  Launch sets hold at most SET_MEMBERS members and at
//                most `budget` bytes of scratch (br_plan)
//   the CLIP     what the wave that decoded a member does with its pieces, lane by lane: bytes up to the destination's first 16-byte
//                boundary, aligned 16-byte stores put together from aligned source words with funnel shifts, bytes behind the last
//                boundary (br_lane_piece).  No store lands outside [dst, dst + hi - lo), no load outside the member's padded slot
//   the VERDICT  a touched member is accepted iff it is structurally clean, exactly out_len bytes long and its CRC-32 and ISIZE match
//                (br_valid, br_judge), and a range's report, status and got from the verdicts of the members it touches (br_give)
// The member itself is decoded by iw_inflate (inflate_write.h) as a wrapper-2 stream under the cap out_len: this is no second decoder.
#ifndef MI355_BGZF_READ_H
#define MI355_BGZF_READ_H

#include <algorithm>
#include <vector>

#include "inflate_members.h"

namespace mi355 {
namespace br {

using namespace ic;

constexpr uint32_t SET_MEMBERS = 16384;          // members of one launch set (the descriptor room of a members call)
constexpr uint64_t MEMBER_MAX = 0xFFFF0000ull;   // what the checksum kernels take of one member
constexpr uint64_t NONE = ~0ull;
// what a call returns for a range (the values of include/mi355_deflate.h; the host build has no other source for them)
enum : int { RC_OK = 0, RC_ARG = -1, RC_UNSUPPORTED = -4, RC_DATA = -8 };

struct Index {
    std::vector<im::Member> mem;
    uint64_t file_len = 0, total = 0, max_out = 0;
};
struct Range {
    uint64_t off, len;
    uint8_t* out;
};
struct Piece {  // [lo, hi) of a member's bytes to dst
    uint64_t lo, hi;
    uint8_t* dst;
};  // 24 bytes
struct Ref {  // a member's pieces in its set's array; none for a member in place
    uint32_t piece0, n_pieces;
};
struct Dec {  // a distinct member of a call
    uint64_t member;
    uint64_t slot;  // offset of its scratch slot in the set's scratch; NONE: in place, at `dst`
    uint8_t* dst;
    Ref ref;
};
struct Set {
    std::vector<Dec> decs;
    std::vector<Piece> pieces;
    uint64_t scratch = 0;
};
struct Counts {
    uint64_t distinct, in_place, scratch, pieces, sets;
};
struct Verdict {  // of a decoded member: status 0 = accepted; pos counts from the member's first byte
    uint32_t status;
    uint64_t bit, pos;
};

// the three decisions a mutant of the model changes (tests/bgzfread)
struct Rules {
    static MI355_IC bool in_place(uint64_t wants, bool covered) { return wants == 1 && covered; }
    static MI355_IC uint64_t seam_src(uint64_t s, uint32_t head) { return s; }  // the source offset of the first aligned granule
    static MI355_IC bool accept(uint64_t got, uint64_t claimed) { return got == claimed; }
};

MI355_IC uint64_t br_align16(uint64_t v) { return (v + 15) & ~15ull; }
MI355_IC uint64_t br_got(uint64_t off, uint64_t len, uint64_t total) { return off >= total ? 0 : (len < total - off ? len : total - off); }

// ---- the index: host side of all builds -------------------------------------------------------------------------------------------
inline void br_seal(Index& ix, uint64_t file_len) {
    ix.file_len = file_len, ix.total = 0, ix.max_out = 0;
    for (const im::Member& m : ix.mem) {
        ix.total = m.out_off + m.out_len;
        ix.max_out = m.out_len > ix.max_out ? m.out_len : ix.max_out;
    }
}
// a table somebody holds: M is mi355_member_info or im::Member
template <class M>
inline bool br_from_members(const M* m, uint64_t n, uint64_t file_len, Index& ix) {
    if (!m || n < 1 || m[0].in_off != 0 || m[0].out_off != 0) return false;
    for (uint64_t k = 0; k < n; k++) {
        if (m[k].status != 0 || m[k].in_len < 18 || m[k].in_len > file_len - (m[k].in_off <= file_len ? m[k].in_off : file_len)) return false;
        if (m[k].out_len > ~0ull - m[k].out_off) return false;
        const uint64_t in_end = m[k].in_off + m[k].in_len, out_end = m[k].out_off + m[k].out_len;
        if (k + 1 < n ? (m[k + 1].in_off != in_end || m[k + 1].out_off != out_end) : in_end != file_len) return false;
    }
    ix.mem.resize(n);
    for (uint64_t k = 0; k < n; k++) ix.mem[k] = im::Member{m[k].in_off, m[k].in_len, m[k].out_off, m[k].out_len, m[k].flags, 0u};
    br_seal(ix, file_len);
    return true;
}
// The file's own claims: Path A from byte 0.  be: find / walk / fill of im_run's backend.  0 and a sealed index, or the backend's
// error, or RC_DATA: the run does not reach the end of the file -- *pos: the sum of the ISIZEs in front of the byte that begins no
// hinted member
template <class B>
inline int br_build(B& be, uint64_t n, uint64_t S, Index& ix, uint64_t* pos) {
    *pos = 0;
    ix.mem.clear();
    if (n == 0) return RC_DATA;
    const uint64_t n_spans = im::im_n_spans(n, S);
    if (const int rc = be.find(n_spans)) return rc;
    std::vector<im::Walk> w;
    if (const int rc = be.walk(0, w)) return rc;
    std::vector<im::Seg> segs;
    uint64_t cnt = 0, sum = 0, last = 0;
    im::im_link(w.data(), n_spans, 0, [&](uint64_t k) {
        if (w[k].n_members) segs.push_back(im::Seg{w[k].start, cnt, w[k].n_members});
        cnt += w[k].n_members, sum += w[k].out_bytes, last = k;
    });
    *pos = sum;
    if (!cnt || w[last].how != im::END_FILE || w[last].end != n) return RC_DATA;
    std::vector<im::Hint> rows;
    if (const int rc = be.fill(segs, cnt, rows)) return rc;
    ix.mem.resize(cnt);
    uint64_t o = 0, p = 0;
    for (uint64_t k = 0; k < cnt; k++) {
        if (rows[k].in_off != o || rows[k].in_len < im::HOP_MIN) return RC_DATA;  // (never: the fill hops as the walk did)
        ix.mem[k] = im::Member{o, rows[k].in_len, p, rows[k].isize, im::HINTED, 0u};
        o += rows[k].in_len, p += rows[k].isize;
    }
    if (o != n) return RC_DATA;  // (never)
    br_seal(ix, n);
    return RC_OK;
}

// the member that holds byte u < total: out_off <= u < out_off + out_len (the last member that begins at or below u: never an empty one)
inline uint64_t br_member_of(const Index& ix, uint64_t u) {
    uint64_t lo = 0, hi = ix.mem.size() - 1;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (ix.mem[mid].out_off <= u)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}
// htslib's virtual offset, coffset << 16 | offset inside the member
inline int br_voffset(const Index& ix, uint64_t u, uint64_t* v) {
    if (u > ix.total) return RC_ARG;
    if (u == ix.total) {
        if (ix.file_len >> 48) return RC_UNSUPPORTED;
        *v = ix.file_len << 16;
        return RC_OK;
    }
    const im::Member& m = ix.mem[br_member_of(ix, u)];
    if (m.out_len > 65536 || m.in_off >> 48) return RC_UNSUPPORTED;
    *v = m.in_off << 16 | (u - m.out_off);
    return RC_OK;
}
inline int br_uoffset(const Index& ix, uint64_t v, uint64_t* u) {
    const uint64_t co = v >> 16, within = v & 0xFFFF;
    if (co == ix.file_len) {
        if (within) return RC_ARG;
        *u = ix.total;
        return RC_OK;
    }
    uint64_t lo = 0, hi = ix.mem.size();
    while (lo < hi) {  // the first member with in_off >= co
        const uint64_t mid = lo + (hi - lo) / 2;
        if (ix.mem[mid].in_off < co)
            lo = mid + 1;
        else
            hi = mid;
    }
    if (lo >= ix.mem.size() || ix.mem[lo].in_off != co) return RC_ARG;
    const im::Member& m = ix.mem[lo];
    if (within >= m.out_len && !(within == 0 && m.out_len == 0)) return RC_ARG;
    *u = m.out_off + within;
    return RC_OK;
}

// ---- the plan: host side of all builds --------------------------------------------------------------------------------------------
// the members range (off, got) touches: [k0, k1], empty ones among them are skipped by the caller; got >= 1
inline void br_touched(const Index& ix, uint64_t off, uint64_t got, uint64_t& k0, uint64_t& k1) {
    k0 = br_member_of(ix, off), k1 = br_member_of(ix, off + got - 1);
}
// sets: the launch sets in file order; unsupported[i]: range i wants a member no set can take (a scratch claim above the budget, or a
// member above MEMBER_MAX)
template <class R>
inline void br_plan(const Index& ix, const Range* r, uint64_t n, uint64_t budget, std::vector<Set>& sets, std::vector<uint8_t>& unsupported,
                    Counts& cnt) {
    sets.clear();
    unsupported.assign(n, 0);
    cnt = Counts{0, 0, 0, 0, 0};
    struct Want {
        uint64_t member, range;
    };
    std::vector<Want> wants;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t got = br_got(r[i].off, r[i].len, ix.total);
        if (!got) continue;
        uint64_t k0, k1;
        br_touched(ix, r[i].off, got, k0, k1);
        for (uint64_t k = k0; k <= k1; k++)
            if (ix.mem[k].out_len) wants.push_back(Want{k, i});
    }
    if (n > 1) std::sort(wants.begin(), wants.end(), [](const Want& a, const Want& b) { return a.member != b.member ? a.member < b.member : a.range < b.range; });
    for (size_t a = 0; a < wants.size();) {
        size_t b = a;
        while (b < wants.size() && wants[b].member == wants[a].member) b++;
        const im::Member& m = ix.mem[wants[a].member];
        size_t cov = a;  // the first range that covers all of the member
        for (; cov < b; cov++) {
            const Range& q = r[wants[cov].range];
            if (q.off <= m.out_off && q.off + br_got(q.off, q.len, ix.total) >= m.out_off + m.out_len) break;
        }
        const bool place = R::in_place(b - a, cov < b);
        const Range& r0 = r[wants[cov < b ? cov : a].range];
        const uint64_t need = place ? 0 : br_align16(m.out_len);
        if (m.out_len > MEMBER_MAX || need > budget) {
            for (size_t j = a; j < b; j++) unsupported[wants[j].range] = 1;
            a = b;
            continue;
        }
        if (sets.empty() || sets.back().decs.size() >= SET_MEMBERS || sets.back().scratch + need > budget) sets.push_back(Set());
        Set& s = sets.back();
        Dec d{wants[a].member, NONE, nullptr, Ref{(uint32_t)s.pieces.size(), 0}};
        if (place) {
            d.dst = r0.out + (m.out_off - r0.off);
            cnt.in_place++;
        } else {
            d.slot = s.scratch;
            s.scratch += need;
            for (size_t j = a; j < b; j++) {
                const Range& q = r[wants[j].range];
                const uint64_t end = q.off + br_got(q.off, q.len, ix.total);
                const uint64_t lo = q.off > m.out_off ? q.off - m.out_off : 0;
                const uint64_t hi = (end < m.out_off + m.out_len ? end : m.out_off + m.out_len) - m.out_off;
                s.pieces.push_back(Piece{lo, hi, q.out + (m.out_off + lo - q.off)});
            }
            d.ref.n_pieces = (uint32_t)(b - a);
            cnt.scratch++, cnt.pieces += b - a;
        }
        s.decs.push_back(d);
        cnt.distinct++;
        a = b;
    }
    cnt.sets = sets.size();
}

// ---- the clip, as one lane of 64 sees it (the host build replays it lane by lane) --------------------------------------------------
// the bytes of a decoded member that hold data, for its pieces: all of it when it is clean and as long as claimed; up to a structural
// failure inside the claim (as every inflate call leaves the bytes in front of a failure); else none
template <class R>
MI355_IC uint64_t br_valid(const iw::Rec& r, uint64_t claimed) {
    if (!r.status) return R::accept(r.out_len, claimed) ? claimed : 0;
    return r.out_pos <= claimed ? r.out_pos : 0;
}
// Piece (lo, hi, dst) of the member in `slot` (16-byte aligned, align_up(out_len, 16) bytes), clipped to `valid`.  With n = hi - lo:
// `head` bytes up to dst's first 16-byte boundary, lane i the i-th; then the aligned granules, lane l the granules l, l + 64, ...,
// each one 16-byte store of four words put together from five aligned source words; then the bytes behind the last boundary.
template <class R>
MI355_IC void br_lane_piece(const uint8_t* slot, uint64_t lo, uint64_t hi, uint8_t* dst, uint64_t valid, uint32_t lane) {
    if (hi > valid) hi = valid;
    if (lo >= hi) return;
    const uint64_t n = hi - lo;
    const uint32_t h = (uint32_t)((0 - (uintptr_t)dst) & 15);
    const uint32_t head = h < n ? h : (uint32_t)n;
    if (lane < head) dst[lane] = slot[lo + lane];
    const uint64_t grans = (n - head) / 16;
    for (uint64_t g = lane; g < grans; g += 64) {
        const uint64_t s = R::seam_src(lo + head + 16 * g, head);
        const uint8_t* const w = slot + (s & ~3ull);
        const uint32_t sh = 8 * (uint32_t)(s & 3);
        uint32_t x[5], v[4];
        for (int k = 0; k < 5; k++) {
            x[k] = 0;
            if (k < 4 || sh) __builtin_memcpy(&x[k], __builtin_assume_aligned(w + 4 * k, 4), 4);  // (the fifth word only where a shift needs it)
        }
        for (int k = 0; k < 4; k++) v[k] = (uint32_t)(((((uint64_t)x[k + 1]) << 32) | x[k]) >> sh);
        __builtin_memcpy(__builtin_assume_aligned(dst + head + 16 * g, 16), v, 16);
    }
    const uint64_t done = head + 16 * grans;
    if (lane < n - done) dst[done + lane] = slot[lo + done + lane];
}

// ---- the verdict: host side of all builds -----------------------------------------------------------------------------------------
// r: the member's record behind the trailer pass (CHECKSUM is that pass's)
template <class R>
inline Verdict br_judge(const iw::Rec& r, uint64_t claimed) {
    if (r.status == V_CHECKSUM) return Verdict{V_CHECKSUM, r.bit, 0};
    if (r.status) return r.out_pos <= claimed ? Verdict{r.status, r.bit, r.out_pos} : Verdict{V_TABLE, 0, 0};  // (beyond its claim)
    return R::accept(r.out_len, claimed) ? Verdict{V_OK, 0, 0} : Verdict{V_TABLE, 0, 0};
}
// is the member's checksum judged?  (what the accept rule lets through; the trailer pass needs all of it stored)
template <class R>
inline bool br_summed(const iw::Rec& r, uint64_t claimed) { return !r.status && R::accept(r.out_len, claimed) && r.out_len <= claimed; }

// A range's end.  lookup(member) -> (the member's record, its verdict) for the members the plan decoded.  Rep: mi355_inflate_report.
// Returns RC_OK or RC_DATA; *got as the header defines it.
template <class Rep, class Lookup>
inline int br_give(const Index& ix, const Range& q, Lookup lookup, Rep& rep, uint64_t* got) {
    rep = Rep();
    const uint64_t full = br_got(q.off, q.len, ix.total);
    *got = full;
    rep.out_len = full, rep.out_pos = q.off + full;
    if (!full) {
        rep.out_pos = q.off;
        return RC_OK;
    }
    uint64_t k0, k1;
    br_touched(ix, q.off, full, k0, k1);
    for (uint64_t k = k0; k <= k1; k++) {
        if (!ix.mem[k].out_len) continue;
        const iw::Rec* r;
        Verdict v;
        lookup(k, r, v);
        if (v.status) {
            rep = Rep();
            rep.status = v.status, rep.bit = v.bit, rep.out_pos = ix.mem[k].out_off + v.pos;
            const uint64_t g = (rep.out_pos > q.off ? rep.out_pos : q.off) - q.off;
            *got = g < q.len ? g : q.len;
            return RC_DATA;
        }
        rep.n_blocks += r->n_blocks, rep.n_stored += r->n_stored, rep.n_fixed += r->n_fixed, rep.n_dynamic += r->n_dynamic;
    }
    return RC_OK;
}

}  // namespace br
}  // namespace mi355
#endif
