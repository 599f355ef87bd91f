// Host build of deflate-rs_amd/csrc/bgzf_read.h (TEST INFRASTRUCTURE): the BGZF index -- from a member table, or from the file's own
// claims by Path A's find, walk, link and fill as plain loops --, virtual offsets, and a read as the device runs it: the plan, every
// distinct member decoded by iw_inflate with the lane-by-lane sink into its slot (the range's buffer, or a scratch slot of exact
// size), the pieces copied lane by lane, the trailers judged, the ranges' reports.  MUTANTS of the decisions, for the cases that must
// kill them: 1 = an in-place rule that ignores sharing, 2 = a piece copy whose aligned granules begin one source byte late where a
// 16-byte seam exists, 3 = an accept rule that skips the length test.  The product never links this.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../deflate-rs_amd/csrc/bgzf_read.h"
#include "../../include/mi355_deflate.h"

using namespace mi355;

static_assert(sizeof(im::Member) == 40 && sizeof(mi355_member_info) == 40, "a member's row is 40 bytes");
static_assert(sizeof(mi355_inflate_report) == 56 && sizeof(iw::Rec) == 56, "records and report are 56 bytes");
static_assert(br::RC_ARG == MI355_E_ARG && br::RC_UNSUPPORTED == MI355_E_UNSUPPORTED && br::RC_DATA == MI355_E_DATA, "the header's values");

namespace {

uint64_t g_unfenced_loads = 0;  // loads of a match step or of a piece in front of the last fence: must stay 0

struct Scalar {
    static bool leader() { return true; }
    static void sync() {}
    static uint32_t uni(uint32_t v) { return v; }
};
// the writes the kernel's way, a lane at a time (tests/inflwrite's LaneSink: a step of the wave is all its loads, then all its stores)
struct LaneSink : Scalar, im::Rules {
    static uint64_t& fenced() {
        static uint64_t v = 0;
        return v;
    }
    static void fence(uint64_t upto) { fenced() = upto; }
    static void store_lits(const uint8_t* lit, uint8_t* out, uint64_t cap, uint64_t lit_p, uint32_t n) {
        for (uint32_t lane = 0; lane < 64; lane++) iw::iw_lane_lits(lit, out, cap, lit_p, n, lane);
    }
    static void copy_match(uint8_t* out, uint64_t cap, uint64_t p, uint32_t len, uint32_t dist) {
        for (uint32_t base = 0; base < 320 && base < len; base += 64) {
            uint8_t v[64];
            bool on[64];
            for (uint32_t lane = 0; lane < 64; lane++) {
                const uint32_t i = base + lane;
                on[lane] = i < len && p + i < cap;
                if (!on[lane]) continue;
                const uint64_t src = iw::iw_match_src(p, dist, i);
                if (src >= fenced() || src >= p || src >= cap) g_unfenced_loads++;
                v[lane] = src < p && src < cap ? out[src] : 0;
            }
            for (uint32_t lane = 0; lane < 64; lane++) iw::iw_lane_match(out, cap, p, len, dist, base, lane);
            for (uint32_t lane = 0; lane < 64; lane++)
                if (on[lane] && out[p + base + lane] != v[lane]) g_unfenced_loads++;
        }
    }
    static void copy_run(const uint8_t* src, uint8_t* out, uint64_t cap, uint64_t p, uint32_t n) {
        const uint32_t head = iw::iw_run_head(out, p, n);
        for (uint32_t lane = 0; lane < 64; lane++) iw::iw_lane_run_head(src, out, cap, p, head, lane);
        for (uint32_t base = 0; base < 65536 && head + base < n; base += 512)
            for (uint32_t lane = 0; lane < 64; lane++) iw::iw_lane_run(src, out, cap, p, n, head, base, lane);
    }
    static uint64_t survivors(const uint8_t* s, uint64_t n, uint64_t base, uint64_t end) {  // the finder's prefilter, lane by lane
        uint64_t m = 0;
        for (uint32_t lane = 0; lane < 64; lane++)
            if (base + lane < end && im::im_fixed4(s, n, base + lane)) m |= 1ull << lane;
        return m;
    }
};

// the mutants
struct ShareBlind : br::Rules {
    static bool in_place(uint64_t, bool covered) { return covered; }
};
struct SeamLate : br::Rules {
    static uint64_t seam_src(uint64_t s, uint32_t head) { return head ? s + 1 : s; }
};
struct NoLength : br::Rules {
    static bool accept(uint64_t, uint64_t) { return true; }
};

uint32_t crc32(const uint8_t* d, uint64_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (uint64_t i = 0; i < n; i++) {
        c ^= d[i];
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1u) ? 0xEDB88320u : 0u);
    }
    return ~c;
}

// exact-size workspaces on the heap (a sanitizer build sees every index outside them); 16-byte aligned as the device's are
struct Slots {
    uint8_t* p;
    explicit Slots(size_t n) : p((uint8_t*)aligned_alloc(16, n ? (n + 15) & ~(size_t)15 : 16)) {}
    ~Slots() { free(p); }
    Slots(const Slots&) = delete;
    Slots& operator=(const Slots&) = delete;
};

const uint8_t none = 0;

// Path A's steps as plain loops
struct HostBe {
    const uint8_t* s;
    uint64_t n, S, n_spans;
    std::vector<uint64_t> cand;
    int find(uint64_t) {
        cand.assign(n_spans, im::NOCAND);
        for (uint64_t k = n_spans; k-- > 0;) cand[k] = im::im_find<LaneSink>(s, n, k, S);
        return 0;
    }
    int walk(uint64_t o, std::vector<im::Walk>& w) {
        w.resize(n_spans);
        for (uint64_t k = n_spans; k-- > 0;) im::im_walk_span<LaneSink>(s, n, cand.data(), n_spans, S, o, k, w[k]);
        return 0;
    }
    int fill(const std::vector<im::Seg>& segs, uint64_t n_rows, std::vector<im::Hint>& rows) {
        rows.assign(n_rows, im::Hint{0, 0, 0});
        for (size_t k = segs.size(); k-- > 0;) im::im_fill<LaneSink>(s, n, segs[k], rows.data(), n_rows);
        return 0;
    }
};

template <class R>
int run_read(const br::Index& ix, bool slack, const uint8_t* file, const br::Range* ranges, uint64_t n, uint64_t budget, uint64_t* got, int32_t* status,
             mi355_inflate_report* reports, uint64_t counts[5]) {
    std::vector<br::Set> sets;
    std::vector<uint8_t> unsupported;
    br::Counts cnt;
    br::br_plan<R>(ix, ranges, n, budget, sets, unsupported, cnt);
    counts[0] = cnt.distinct, counts[1] = cnt.in_place, counts[2] = cnt.scratch, counts[3] = cnt.pieces, counts[4] = cnt.sets;
    std::vector<uint64_t> ids;
    std::vector<iw::Rec> recs;
    ic::Tables t;
    memset(&t, 0, sizeof t);
    for (const br::Set& s : sets) {
        if (s.decs.empty() || s.decs.size() > br::SET_MEMBERS || s.scratch > budget) abort();
        Slots scratch((size_t)s.scratch + (slack ? 32 : 0));
        memset(scratch.p, 0xEE, (size_t)s.scratch);
        for (size_t j = s.decs.size(); j-- > 0;) {  // (any order: a member cannot touch its neighbour)
            const br::Dec& d = s.decs[j];
            const im::Member& m = ix.mem[d.member];
            uint8_t* slot = d.slot == br::NONE ? d.dst : scratch.p + d.slot;
            if (d.slot != br::NONE && (d.slot % 16 || d.slot + br::br_align16(m.out_len) > s.scratch)) abort();
            iw::Rec r;
            LaneSink::fenced() = 0;
            iw::iw_inflate<LaneSink>(t, file + m.in_off, m.in_len, 2, slot, m.out_len, r);
            const uint64_t valid = br::br_valid<R>(r, m.out_len);
            if (d.ref.n_pieces && valid) {
                LaneSink::fence(valid);
                for (uint32_t q = 0; q < d.ref.n_pieces; q++) {
                    const br::Piece& pc = s.pieces[d.ref.piece0 + q];
                    if (pc.lo > pc.hi || pc.hi > m.out_len) abort();
                    if ((pc.hi < valid ? pc.hi : valid) > LaneSink::fenced()) g_unfenced_loads++;
                    for (uint32_t lane = 0; lane < 64; lane++) br::br_lane_piece<R>(slot, pc.lo, pc.hi, pc.dst, valid, lane);
                }
            }
            if (br::br_summed<R>(r, m.out_len)) iw::iw_check_trailer(file + m.in_off, m.in_len, 2, 0, crc32(slot, m.out_len), r);
            ids.push_back(d.member), recs.push_back(r);
        }
    }
    int first = MI355_OK;
    for (uint64_t i = 0; i < n; i++) {
        int rc = MI355_E_UNSUPPORTED;
        reports[i] = mi355_inflate_report();
        got[i] = 0;
        if (!unsupported[i])
            rc = br::br_give(ix, ranges[i],
                             [&](uint64_t member, const iw::Rec*& rec, br::Verdict& v) {
                                 size_t at = 0;
                                 while (at < ids.size() && ids[at] != member) at++;
                                 if (at == ids.size()) abort();  // (the plan decoded every member a supported range touches)
                                 rec = &recs[at];
                                 v = br::br_judge<R>(recs[at], ix.mem[member].out_len);
                             },
                             reports[i], &got[i]);
        status[i] = rc;
        if (rc != MI355_OK && first == MI355_OK) first = rc;
    }
    return first;
}

}  // namespace

// the index from the file's own claims; *rc: MI355_OK and a handle, else NULL and the report
extern "C" void* bgzfread_build(const uint8_t* file, uint64_t file_len, uint64_t S, int* rc, mi355_inflate_report* report) {
    *rc = MI355_E_ARG;
    if (!report || (!file && file_len) || S < im::SPAN_MIN || S > im::SPAN_MAX) return nullptr;
    *report = mi355_inflate_report();
    br::Index* ix = new br::Index;
    HostBe be{file ? file : &none, file_len, S, im::im_n_spans(file_len, S), {}};
    uint64_t pos = 0;
    *rc = br::br_build(be, file_len, S, *ix, &pos);
    if (*rc != MI355_OK) {
        report->status = MI355_VERIFY_FRAME, report->out_pos = pos;
        delete ix;
        return nullptr;
    }
    report->out_len = report->out_pos = ix->total;
    return ix;
}
extern "C" void* bgzfread_from_members(const mi355_member_info* members, uint64_t n, uint64_t file_len, int* rc) {
    br::Index* ix = new br::Index;
    *rc = br::br_from_members(members, n, file_len, *ix) ? MI355_OK : MI355_E_ARG;
    if (*rc == MI355_OK) return ix;
    delete ix;
    return nullptr;
}
extern "C" void bgzfread_free(void* h) { delete (br::Index*)h; }
// v: total, n_members, file_len, the largest out_len
extern "C" void bgzfread_info(void* hv, uint64_t v[4]) {
    const br::Index& ix = *(br::Index*)hv;
    v[0] = ix.total, v[1] = ix.mem.size(), v[2] = ix.file_len, v[3] = ix.max_out;
}
extern "C" uint64_t bgzfread_members(void* hv, mi355_member_info* out, uint64_t cap) {
    const br::Index& ix = *(br::Index*)hv;
    for (size_t k = 0; k < ix.mem.size() && k < cap; k++) memcpy(&out[k], &ix.mem[k], sizeof(im::Member));
    return ix.mem.size();
}
extern "C" int bgzfread_voffset(void* hv, uint64_t u, uint64_t* v) { return br::br_voffset(*(br::Index*)hv, u, v); }
extern "C" int bgzfread_uoffset(void* hv, uint64_t v, uint64_t* u) { return br::br_uoffset(*(br::Index*)hv, v, u); }

// n ranges (off[i], len[i]) into out + out_at[i] from `file` (file_len bytes: the index's); budget: the scratch of a launch set.
// got / status / reports: n entries; counts: distinct members, in place, to scratch, pieces, launch sets
extern "C" int bgzfread_read(void* hv, int mutant, const uint8_t* file, uint64_t file_len, const uint64_t* off, const uint64_t* len,
                             const uint64_t* out_at, uint64_t n, uint64_t budget, uint8_t* out, uint64_t* got, int32_t* status,
                             mi355_inflate_report* reports, uint64_t counts[5]) {
    const br::Index& ix = *(br::Index*)hv;
    if (!got || !status || !reports || !counts || (n && (!off || !len || !out_at)) || budget < 65536 || file_len != ix.file_len || (!file && file_len))
        return MI355_E_ARG;
    std::vector<br::Range> ranges(n);
    for (uint64_t i = 0; i < n; i++) ranges[i] = br::Range{off[i], len[i], len[i] ? out + out_at[i] : nullptr};
    const uint8_t* s = file ? file : &none;
    if (mutant == 1) return run_read<ShareBlind>(ix, true, s, ranges.data(), n, budget, got, status, reports, counts);
    if (mutant == 2) return run_read<SeamLate>(ix, true, s, ranges.data(), n, budget, got, status, reports, counts);
    if (mutant == 3) return run_read<NoLength>(ix, true, s, ranges.data(), n, budget, got, status, reports, counts);
    return run_read<br::Rules>(ix, false, s, ranges.data(), n, budget, got, status, reports, counts);
}
extern "C" uint64_t bgzfread_unfenced_loads(void) { return g_unfenced_loads; }
extern "C" uint32_t bgzfread_piece_size(void) { return (uint32_t)sizeof(br::Piece); }
extern "C" uint32_t bgzfread_set_members(void) { return br::SET_MEMBERS; }
