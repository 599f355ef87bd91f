// Host build of deflate-rs_amd/csrc/inflate_members.h (TEST INFRASTRUCTURE): the plain serial walk of a gzip file, written out on its
// own; and the call as the device runs it -- im_run over Paths A and B -- with the finder replayed lane by lane with its prefilter, or
// as the plain predicate over every offset of a span.  Candidates live in an exact-size heap block.  MUTANTS of the model, for the
// cases that must kill them: 1 = the finder takes the span's LAST hinted offset, 2 = a walker stops at pos >= c_j, 3 = a hinted
// member's extent is BSIZE instead of BSIZE + 1.  The product never links this.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../deflate-rs_amd/csrc/inflate_members.h"
#include "../../include/mi355_deflate.h"

using namespace mi355;

static_assert(sizeof(im::Member) == 40 && sizeof(mi355_member_info) == 40, "a member's row is 40 bytes");
static_assert(sizeof(im::Walk) == 40 && sizeof(im::Hint) == 16, "the walkers' records and the fill's rows");

namespace {

uint64_t g_group = 16384, g_room = 1024;             // members of one decode turn, of one chain launch (the device's values)
uint64_t g_chains = 0, g_runs = 0, g_accepted = 0;   // chain launches, Path A runs, members Path A accepted
uint64_t g_parses = 0, g_offsets = 0;                // full tests the finder made, offsets it looked at

// a scalar sink: bytes written one at a time
template <int M>
struct Host {
    static bool leader() { return true; }
    static void sync() {}
    static uint32_t uni(uint32_t v) { return v; }
    static void fence(uint64_t) {}
    static void store_lits(const uint8_t* lit, uint8_t* out, uint64_t cap, uint64_t lit_p, uint32_t n) {
        for (uint32_t i = 0; i < n && lit_p + i < cap; i++) out[lit_p + i] = lit[i];
    }
    static void copy_match(uint8_t* out, uint64_t cap, uint64_t p, uint32_t len, uint32_t dist) {
        for (uint32_t i = 0; i < len && p + i < cap; i++) out[p + i] = out[p + i - dist];
    }
    static void copy_run(const uint8_t* src, uint8_t* out, uint64_t cap, uint64_t p, uint32_t n) {
        for (uint32_t i = 0; i < n && p + i < cap; i++) out[p + i] = src[i];
    }
    static bool first() { return M != 1; }
    static bool stop(uint64_t pos, uint64_t c) { return M == 2 ? c != im::NOCAND && pos >= c : im::Rules::stop(pos, c); }
    static uint64_t total(uint32_t bsize) { return M == 3 ? (uint64_t)bsize : im::Rules::total(bsize); }
};
// the finder the kernel's way: 64 lanes, each with the prefilter, a ballot
template <int M>
struct Lanes : Host<M> {
    static uint64_t survivors(const uint8_t* s, uint64_t n, uint64_t base, uint64_t end) {
        uint64_t m = 0;
        for (uint32_t lane = 0; lane < 64; lane++) {
            if (base + lane >= end) continue;
            g_offsets++;
            if (im::im_fixed4(s, n, base + lane)) m |= 1ull << lane, g_parses++;
        }
        return m;
    }
};
// ... and as the definition: every offset gets the full predicate
template <int M>
struct Plain : Host<M> {
    static uint64_t survivors(const uint8_t*, uint64_t, uint64_t base, uint64_t end) {
        return end - base >= 64 ? ~0ull : (1ull << (end - base)) - 1;
    }
};

template <class T>
struct Heap {
    T* p;
    explicit Heap(size_t n) : p((T*)malloc(n ? n * sizeof(T) : 1)) {}
    ~Heap() { free(p); }
    Heap(const Heap&) = delete;
    Heap& operator=(const Heap&) = delete;
};

const uint8_t none = 0;  // (an address the decoder never reads through)

uint32_t crc32(const uint8_t* d, uint64_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (uint64_t i = 0; i < n; i++) {
        c ^= d[i];
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1u) ? 0xEDB88320u : 0u);
    }
    return ~c;
}

// the steps of im_run as plain loops
template <class P>
struct HostBe {
    const uint8_t* s;
    uint64_t n;
    uint8_t* out;
    uint64_t out_cap, S, n_spans;
    uint64_t* cand;
    ic::Tables t;

    uint64_t group() const { return g_group; }
    int find(uint64_t) {
        for (uint64_t k = n_spans; k-- > 0;) cand[k] = im::im_find<P>(s, n, k, S);  // (any order would do)
        return 0;
    }
    int walk(uint64_t o, std::vector<im::Walk>& w) {
        g_runs++;
        w.resize(n_spans);
        for (uint64_t k = n_spans; k-- > 0;) im::im_walk_span<P>(s, n, cand, n_spans, S, o, k, w[k]);
        return 0;
    }
    int fill(const std::vector<im::Seg>& segs, uint64_t n_rows, std::vector<im::Hint>& rows) {
        rows.assign(n_rows, im::Hint{0, 0, 0});
        for (size_t k = segs.size(); k-- > 0;) im::im_fill<P>(s, n, segs[k], rows.data(), n_rows);
        return 0;
    }
    int decode(const im::Hint* rows, uint64_t k, uint64_t p, std::vector<iw::Rec>& got) {
        got.resize(k);
        std::vector<uint64_t> at(k);
        for (uint64_t j = 0; j < k; j++) at[j] = p, p += rows[j].isize;
        for (uint64_t j = k; j-- > 0;) {  // (any order: a member cannot touch its neighbour)
            const uint64_t room = im::im_room_at(out_cap, at[j]);
            iw::iw_inflate<P>(t, s + rows[j].in_off, rows[j].in_len, 2, im::im_out_at(out, out_cap, at[j]), room < rows[j].isize ? room : rows[j].isize,
                              got[j]);
        }
        return 0;
    }
    int chain(uint64_t o, uint64_t p, bool ignore_hints, std::vector<im::Member>& rows, std::vector<iw::Rec>& got, im::ChainEnd& e) {
        g_chains++;
        rows.assign(g_room, im::Member{0, 0, 0, 0, 0, 0});
        got.resize(g_room);
        im::im_chain<P>(t, s, n, o, p, out, out_cap, ignore_hints, rows.data(), got.data(), (uint32_t)g_room, e);
        return 0;
    }
};

// the checksum pass: CRC-32 and ISIZE of every judged member against its trailer
void sums(const uint8_t* s, const uint8_t* out, uint64_t out_cap, const std::vector<im::Member>& mem, std::vector<iw::Rec>& recs) {
    for (size_t j = 0; j < mem.size(); j++)
        if (im::im_judged(mem[j], out_cap))
            iw::iw_check_trailer(s + mem[j].in_off, mem[j].in_len, 2, 0, crc32(mem[j].out_len ? out + mem[j].out_off : s, mem[j].out_len), recs[j]);
}

bool bad_args(const uint8_t* stream, uint64_t len, const uint8_t* out, uint64_t cap, const uint64_t* out_len, const void* members, uint64_t mcap,
              const void* report) {
    return !report || !out_len || (!stream && len) || (!out && cap) || (!members && mcap);
}

void give(const std::vector<im::Member>& mem, mi355_member_info* members, uint64_t mcap, uint64_t* n_members) {
    if (n_members) *n_members = mem.size();
    for (size_t j = 0; j < mem.size() && j < mcap; j++) memcpy(&members[j], &mem[j], sizeof(im::Member));
}

template <class P>
int run(const uint8_t* s, uint64_t n, uint64_t S, uint8_t* out, uint64_t cap, uint64_t* out_len, mi355_member_info* members, uint64_t mcap,
        uint64_t* n_members, mi355_inflate_report* report, uint64_t* cand_out) {
    const uint64_t n_spans = im::im_n_spans(n, S);
    Heap<uint64_t> cand(n_spans);
    for (uint64_t k = 0; k < n_spans; k++) cand.p[k] = im::NOCAND;
    HostBe<P> be{s, n, out, cap, S, n_spans, cand.p, {}};
    memset(&be.t, 0, sizeof be.t);
    std::vector<im::Member> mem;
    std::vector<iw::Rec> recs;
    im::im_run(be, n, S, mem, recs);
    for (const im::Member& m : mem) g_accepted += m.flags & im::HINTED;
    uint64_t total = 0;
    if (!(im::im_total(mem, total) && total > cap)) sums(s, out, cap, mem, recs);
    uint64_t valid = 0;
    const int r = im::im_report(mem, recs, cap, *report, &valid);
    *out_len = r == iw::IW_DATA ? valid : report->out_len;
    give(mem, members, mcap, n_members);
    if (cand_out)
        for (uint64_t k = 0; k < n_spans; k++) cand_out[k] = cand.p[k];
    return r == iw::IW_OK ? MI355_OK : r == iw::IW_DATA ? MI355_E_DATA : MI355_E_OUT_TOO_SMALL;
}

}  // namespace

// ---- the contract: the serial walk, nothing of Paths A and B in it ---------------------------------------------------------------------
extern "C" int inflmembers_serial(const uint8_t* stream, uint64_t stream_len, uint8_t* out, uint64_t out_cap, uint64_t* out_len,
                                  mi355_member_info* members, uint64_t members_cap, uint64_t* n_members, mi355_inflate_report* report) {
    if (bad_args(stream, stream_len, out, out_cap, out_len, members, members_cap, report)) return MI355_E_ARG;
    const uint8_t* s = stream ? stream : &none;
    ic::Tables t;
    memset(&t, 0, sizeof t);
    std::vector<im::Member> mem;
    std::vector<iw::Rec> recs;
    uint64_t o = 0, p = 0;
    bool failed = false;
    do {
        iw::Rec r;
        uint64_t in_len = 0;
        im::im_member_open<Host<0>>(t, s, stream_len, o, im::im_out_at(out, out_cap, p), im::im_room_at(out_cap, p), r, in_len);
        mem.push_back(im::Member{o, in_len, p, r.status ? r.out_pos : r.out_len, 0u, r.status});
        recs.push_back(r);
        failed = r.status != 0;
        o += in_len, p += r.out_len;
    } while (o < stream_len && !failed);
    memset(report, 0, sizeof *report);
    if (!failed && p > out_cap) {  // nothing is judged
        for (const iw::Rec& r : recs)
            report->n_blocks += r.n_blocks, report->n_stored += r.n_stored, report->n_fixed += r.n_fixed, report->n_dynamic += r.n_dynamic;
        report->out_pos = report->out_len = *out_len = p;
        give(mem, members, members_cap, n_members);
        return MI355_E_OUT_TOO_SMALL;
    }
    for (size_t j = 0; j < mem.size(); j++) {
        im::Member& m = mem[j];
        uint32_t status = m.status;
        uint64_t bit = recs[j].bit, pos = m.out_off + m.out_len;
        if (!status && m.out_off + m.out_len <= out_cap) {  // clean and all of it stored: CRC-32 and ISIZE
            const uint8_t* tr = s + m.in_off + m.in_len - 8;
            const uint32_t crc = (uint32_t)tr[0] | (uint32_t)tr[1] << 8 | (uint32_t)tr[2] << 16 | (uint32_t)tr[3] << 24;
            const uint32_t isz = (uint32_t)tr[4] | (uint32_t)tr[5] << 8 | (uint32_t)tr[6] << 16 | (uint32_t)tr[7] << 24;
            if (crc != crc32(m.out_len ? out + m.out_off : s, m.out_len) || isz != (uint32_t)m.out_len)
                status = ic::V_CHECKSUM, bit = recs[j].end_bit;
        }
        if (!status) {
            report->n_blocks += recs[j].n_blocks, report->n_stored += recs[j].n_stored, report->n_fixed += recs[j].n_fixed;
            report->n_dynamic += recs[j].n_dynamic;
            continue;
        }
        m.status = status;
        mem.resize(j + 1);
        memset(report, 0, sizeof *report);
        report->status = status, report->bit = bit, report->out_pos = pos;
        *out_len = pos < out_cap ? pos : out_cap;
        give(mem, members, members_cap, n_members);
        return MI355_E_DATA;
    }
    report->out_pos = report->out_len = *out_len = p;
    give(mem, members, members_cap, n_members);
    return MI355_OK;
}

// mi355_inflate_members as the device runs it; lanes: the finder with its prefilter (else the plain predicate); cand (n_spans entries,
// may be NULL): the candidates, UINT64_MAX where the find never ran or a span has none
extern "C" int inflmembers_run(int mutant, int lanes, uint64_t S, const uint8_t* stream, uint64_t stream_len, uint8_t* out, uint64_t out_cap,
                               uint64_t* out_len, mi355_member_info* members, uint64_t members_cap, uint64_t* n_members,
                               mi355_inflate_report* report, uint64_t* cand) {
    if (bad_args(stream, stream_len, out, out_cap, out_len, members, members_cap, report) || S < im::SPAN_MIN || S > im::SPAN_MAX)
        return MI355_E_ARG;
    const uint8_t* s = stream ? stream : &none;
#define RUN(P) run<P>(s, stream_len, S, out, out_cap, out_len, members, members_cap, n_members, report, cand)
    if (mutant == 1) return lanes ? RUN(Lanes<1>) : RUN(Plain<1>);
    if (mutant == 2) return lanes ? RUN(Lanes<2>) : RUN(Plain<2>);
    if (mutant == 3) return lanes ? RUN(Lanes<3>) : RUN(Plain<3>);
    return lanes ? RUN(Lanes<0>) : RUN(Plain<0>);
#undef RUN
}

// the candidates and the walkers' records of a run that starts at o, n_spans of each
extern "C" int inflmembers_scan(int mutant, int lanes, const uint8_t* stream, uint64_t stream_len, uint64_t S, uint64_t o, uint64_t* cand,
                                im::Walk* walks) {
    if ((!stream && stream_len) || !cand || !walks || S < im::SPAN_MIN || S > im::SPAN_MAX) return MI355_E_ARG;
    const uint8_t* s = stream ? stream : &none;
    const uint64_t n_spans = im::im_n_spans(stream_len, S);
    std::vector<im::Walk> w;
#define SCAN(P)                                                    \
    do {                                                           \
        HostBe<P> be{s, stream_len, nullptr, 0, S, n_spans, cand, {}}; \
        be.find(n_spans), be.walk(o, w);                           \
    } while (0)
    if (mutant == 1) { if (lanes) SCAN(Lanes<1>); else SCAN(Plain<1>); }
    else if (mutant == 2) { if (lanes) SCAN(Lanes<2>); else SCAN(Plain<2>); }
    else if (mutant == 3) { if (lanes) SCAN(Lanes<3>); else SCAN(Plain<3>); }
    else { if (lanes) SCAN(Lanes<0>); else SCAN(Plain<0>); }
#undef SCAN
    for (uint64_t k = 0; k < n_spans; k++) walks[k] = w[k];
    return MI355_OK;
}

// one byte offset: bit 0 = a member is hinted there, bit 1 = the prefilter lets it through; its claimed extent and ISIZE
extern "C" uint32_t inflmembers_hint(const uint8_t* stream, uint64_t stream_len, uint64_t o, uint64_t* total, uint32_t* isize) {
    if (!stream) return 0;
    return (im::im_hint<Host<0>>(stream, stream_len, o, *total, *isize) ? 1u : 0u) | (im::im_fixed4(stream, stream_len, o) ? 2u : 0u);
}

extern "C" uint64_t inflmembers_n_spans(uint64_t stream_len, uint64_t S) { return im::im_n_spans(stream_len, S); }
extern "C" void inflmembers_set_rooms(uint64_t group, uint64_t room) { g_group = group ? group : 16384, g_room = room ? room : 1024; }
extern "C" void inflmembers_reset_counters(void) { g_chains = g_runs = g_accepted = g_parses = g_offsets = 0; }
extern "C" uint64_t inflmembers_chains(void) { return g_chains; }
extern "C" uint64_t inflmembers_runs(void) { return g_runs; }
extern "C" uint64_t inflmembers_accepted(void) { return g_accepted; }
extern "C" uint64_t inflmembers_parses(void) { return g_parses; }
extern "C" uint64_t inflmembers_offsets(void) { return g_offsets; }
extern "C" uint64_t inflmembers_span_min(void) { return im::SPAN_MIN; }
extern "C" uint64_t inflmembers_span_default(void) { return im::SPAN_DEFAULT; }
extern "C" uint32_t inflmembers_resumes(void) { return im::RESUMES; }
extern "C" uint32_t inflmembers_member_size(void) { return (uint32_t)sizeof(im::Member); }
