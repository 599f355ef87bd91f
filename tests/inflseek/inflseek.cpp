// Host build of deflate-rs_amd/csrc/inflate_seek.h (TEST INFRASTRUCTURE): the seek points as the kernels and their driver run them --
// the build group by group with the windows of the points kept, a read as its plan of pieces and launch sets with pass 1 replayed lane
// by lane, pass 2 with the two windows ping-ponged as the workgroup does, pass 3 in runs of 16 bytes with its lower bound --, into
// workspaces of exact size.  Two mutants of the decisions: the point rule off by one entry, and a resolve without the lower bound.
// The product never links this.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../deflate-rs_amd/csrc/inflate_seek.h"
#include "../../include/mi355_deflate.h"

using namespace mi355;

static_assert(sizeof(mi355_inflate_report) == 56 && sizeof(ic::Rec) == 56 && sizeof(iw::Rec) == 56, "records and report are 56 bytes");
static_assert(sizeof(is::Part) == 88, "what the kernels read");

namespace {

uint64_t g_unfenced_loads = 0;  // symbol loads of a match step in front of the last fence, or outside what is stored: must stay 0

struct Scalar {
    static bool leader() { return true; }
    static void sync() {}
    static uint32_t uni(uint32_t v) { return v; }
};

// pass 1 the kernel's way, a lane at a time (tests/infltable's LaneTab: a step of the wave is all its loads, then all its stores)
struct LaneTab : Scalar {
    static uint64_t& fenced() {
        static uint64_t v = 0;
        return v;
    }
    static void fence(uint64_t upto) { fenced() = upto; }
    static void store_lits(const uint8_t* lit, it::Sink& o, uint64_t lit_p, uint32_t n) {
        for (uint32_t lane = 0; lane < 64; lane++) it::it_lane_lits(lit, o.sym, o.base, o.cap, lit_p, n, lane);
    }
    static void copy_match(it::Sink& o, uint64_t p, uint32_t len, uint32_t dist) {
        for (uint32_t at = 0; at < 320 && at < len; at += 64) {
            uint16_t v[64];
            bool on[64];
            for (uint32_t lane = 0; lane < 64; lane++) {
                const uint32_t i = at + lane;
                on[lane] = i < len && p + i < o.cap;
                if (!on[lane]) continue;
                const uint64_t src = iw::iw_match_src(p, dist, i);
                bool ok = true;
                if (src >= o.start && (src >= fenced() || src >= p || src >= o.cap)) ok = false;
                if (src < o.start && (o.start - src > it::WIN)) ok = false;
                if (!ok) g_unfenced_loads++;
                v[lane] = ok ? it::it_lane_src(o.sym, o.base, o.start, src) : 0;
            }
            for (uint32_t lane = 0; lane < 64; lane++) it::it_lane_match(o.sym, o.base, o.start, o.cap, p, len, dist, at, lane);
            for (uint32_t lane = 0; lane < 64; lane++)
                if (on[lane] && o.sym[p + at + lane - o.base] != v[lane]) g_unfenced_loads++;
        }
    }
    static void copy_run(const uint8_t* src, it::Sink& o, uint64_t p, uint32_t n) {
        const uint32_t head = it::it_run_head(o.sym, o.base, p, n);
        for (uint32_t lane = 0; lane < 64; lane++) it::it_lane_run_head(src, o.sym, o.base, o.cap, p, head, lane);
        for (uint32_t at = 0; at < 65536 && head + at < n; at += 512)
            for (uint32_t lane = 0; lane < 64; lane++) it::it_lane_run(src, o.sym, o.base, o.cap, p, n, head, at, lane);
    }
};

// the mutants
struct PointOffByOne : is::Rules {
    static uint64_t point_pos(const ic::Entry& e) { return e.last ? e.pos : e.next_pos; }  // the entry's end: a point one entry early
};
struct NoLowerBound : is::Rules {
    static bool writes(uint64_t, uint64_t) { return true; }
};

uint32_t adler32(uint32_t adler, const uint8_t* d, uint64_t n) {
    uint32_t a = adler & 0xffff, b = adler >> 16;
    for (uint64_t i = 0; i < n; i++) {
        a = (a + d[i]) % 65521u;
        b = (b + a) % 65521u;
    }
    return b << 16 | a;
}
uint32_t crc32(uint32_t crc, const uint8_t* d, uint64_t n) {
    uint32_t c = ~crc;
    for (uint64_t i = 0; i < n; i++) {
        c ^= d[i];
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1u) ? 0xEDB88320u : 0u);
    }
    return ~c;
}

// exact-size workspaces on the heap (a sanitizer build sees every index outside them)
template <class T>
struct Heap {
    T* p;
    explicit Heap(size_t n) : p((T*)malloc(n ? n * sizeof(T) : 1)) {}
    ~Heap() { free(p); }
    Heap(const Heap&) = delete;
    Heap& operator=(const Heap&) = delete;
};

struct Handle {
    std::vector<ic::Entry> ents;
    std::vector<uint32_t> pts;
    std::vector<uint8_t> store;  // pts.size() - 1 windows
    uint64_t total = 0, spacing = 0, stream_len = 0;
    uint32_t wrapper = 0;
    int mutant = 0;
};

// the build as deflate_seek_inflate.inc drives it: passes 1 and 2 group by group with cap = total, the points' windows kept, a framed
// stream's groups resolved into a scratch region and summed
template <class R>
void run_build(Handle& h, const uint8_t* s, const uint64_t* in_bytes, uint64_t group_bytes, iw::Rec& acc) {
    const uint64_t n_all = h.ents.size(), total = h.total;
    is::is_points<R>(h.ents.data(), n_all, h.spacing, h.pts);
    h.store.assign((h.pts.size() - 1) * (size_t)it::WIN, 0xEE);
    ic::Tables t;
    memset(&t, 0, sizeof t);
    std::vector<uint8_t> carry(it::WIN, 0);
    uint32_t adler = 1, crc = 0;
    size_t next_pt = 1;
    for (uint64_t k0 = 0; k0 < n_all;) {
        const uint64_t k1 = it::it_group_end([&](uint64_t k) { return in_bytes[k]; }, n_all, k0, group_bytes);
        const uint32_t n = (uint32_t)(k1 - k0);
        const uint64_t base = h.ents[k0].pos, stored = (k1 < n_all ? h.ents[k1].pos : total) - base;
        Heap<uint16_t> sym(stored);
        Heap<uint8_t> win((size_t)(n + 1) * it::WIN), scratch(stored);
        memset(sym.p, 0xEE, stored * 2);
        memset(win.p, 0xEE, (size_t)(n + 1) * it::WIN);
        memcpy(win.p, carry.data(), it::WIN);
        std::vector<ic::Rec> recs(n);
        const ic::Entry* ge = h.ents.data() + k0;
        for (uint32_t k = n; k-- > 0;) {
            it::Sink o{sym.p, nullptr, base, ge[k].pos, total, ge[k].pos};
            LaneTab::fenced() = ge[k].pos;
            it::it_decode_entry<LaneTab>(t, s, h.stream_len, h.wrapper, o, ge[k], total, recs[k]);
        }
        const uint64_t limit = it::it_window_walk(it::Walk{sym.p, ge, recs.data(), n, base, total, win.p, 0u, n, true}, win.p);  // k_inflate_tab_window
        if (limit != it::it_limit(recs.data(), n, base)) abort();  // (the walk and the header's statement of its rule agree)
        // k_seek_keep
        for (; next_pt < h.pts.size() && h.pts[next_pt] < k1; next_pt++)
            memcpy(h.store.data() + (next_pt - 1) * (size_t)it::WIN, win.p + (size_t)(h.pts[next_pt] - k0) * it::WIN, it::WIN);
        if (h.wrapper && stored) {
            const uint64_t end = limit < base + stored ? limit : base + stored;
            for (uint64_t q0 = base; q0 < base + stored; q0 += it::RESOLVE_RUN)
                it::it_resolve_run<is::Rules>(sym.p, win.p, ge, n, base, end, base, scratch.p, q0);
        }
        carry.assign(win.p + (size_t)n * it::WIN, win.p + (size_t)(n + 1) * it::WIN);
        if (!it::it_report(recs.data(), n, acc)) return;
        if (h.wrapper && stored) adler = adler32(adler, scratch.p, stored), crc = crc32(crc, scratch.p, stored);
        k0 = k1;
    }
    if (h.wrapper) {
        const uint64_t tn = h.wrapper == 1 ? 4 : 8;
        if (h.stream_len >= tn && !is::is_trailer_ok(h.wrapper, s + h.stream_len - tn, adler, crc, total)) is::is_checksum_failed(acc);
    }
}

// one launch set of a read: the three passes
template <class R>
void run_set(const Handle& h, const is::Set& s, std::vector<ic::Rec>& recs) {
    const size_t np = s.parts.size(), ne = s.ents.size();
    Heap<uint16_t> sym(s.syms);
    Heap<uint8_t> win((size_t)s.slots * it::WIN);
    memset(sym.p, 0xEE, s.syms * 2);
    memset(win.p, 0xEE, (size_t)s.slots * it::WIN);
    recs.assign(ne, ic::Rec());
    ic::Tables t;
    memset(&t, 0, sizeof t);
    for (size_t k = ne; k-- > 0;) {  // pass 1: every entry on its own (any order would do)
        LaneTab::fenced() = s.ents[k].pos;
        is::is_decode_entry<LaneTab>(t, sym.p, s.parts[s.ents[k].item], s.ents[k], recs[k]);
    }
    std::vector<uint64_t> limits(np);
    for (size_t j = 0; j < np; j++) {  // pass 2: a workgroup per part
        const is::Part& pt = s.parts[j];
        uint8_t* w0 = win.p + (size_t)pt.w0 * it::WIN;  // the point's window, left in the part's slot 0
        if (pt.wslot != is::WSLOT_ZEROS) memcpy(w0, h.store.data() + (size_t)pt.wslot * it::WIN, it::WIN);
        else memset(w0, 0, it::WIN);
        const ic::Rec* pr = recs.data() + pt.e0;
        limits[j] = it::it_window_walk(it::Walk{sym.p + pt.sym_off, s.ents.data() + pt.e0, pr, pt.n, pt.base, pt.cap, win.p, pt.w0, pt.w0 + pt.n, false}, w0);
        if (limits[j] != it::it_limit(pr, pt.n, pt.base)) abort();  // (the walk and the header's statement of its rule agree)
    }
    for (uint64_t f0 = 0; f0 < s.syms; f0 += it::RESOLVE_RUN)  // pass 3: the only writes of `out`
        is::is_resolve_set<R>(sym.p, win.p, s.ents.data(), s.parts.data(), (uint32_t)np, limits.data(), f0);
}

template <class R>
int run_read(Handle& h, const uint8_t* s, is::Range* ranges, uint64_t n, uint64_t budget, uint64_t* got, mi355_inflate_report* reports,
             uint64_t counts[4]) {
    std::vector<is::Set> sets;
    is::Counts cnt;
    is::is_plan(h.ents.data(), h.ents.size(), h.total, h.pts, ranges, n, budget, s, h.stream_len, h.wrapper, sets, cnt);
    counts[0] = cnt.entries, counts[1] = cnt.symbols, counts[2] = cnt.steps, counts[3] = cnt.sets;
    std::vector<iw::Rec> acc(n, iw::Rec{ic::V_OK, 0, 0, 0, 0, 0, 0, 0, 0});
    std::vector<uint8_t> failed(n, 0);
    std::vector<ic::Rec> recs;
    for (is::Set& set : sets) {
        for (size_t j = 1; j < set.parts.size(); j++)
            if (set.parts[j].range == set.parts[j - 1].range) abort();  // (two pieces of one range never share a set)
        is::is_drop(set, failed);
        run_set<R>(h, set, recs);
        for (const is::Part& pt : set.parts)
            if (!failed[pt.range] && !is::is_report(recs.data(), pt, acc[pt.range])) failed[pt.range] = 1;
    }
    int first = MI355_OK;
    for (uint64_t i = 0; i < n; i++) {
        got[i] = is::is_give(acc[i], ranges[i].off, ranges[i].len, h.total);
        uint64_t valid = 0;
        const int r = iw::iw_report(acc[i], ~0ull, reports[i], &valid);
        const int rc = r == iw::IW_OK ? MI355_OK : MI355_E_DATA;
        if (rc != MI355_OK && first == MI355_OK) first = rc;
    }
    return first;
}

}  // namespace

// mutant 0: none; 1: the point rule off by one entry; 2: a resolve without the lower bound.  *rc: MI355_OK and a handle, else NULL
extern "C" void* inflseek_build(int mutant, const uint8_t* stream, uint64_t stream_len, int wrapper, const uint64_t* bit_start,
                                const uint64_t* in_bytes, uint64_t n, uint64_t spacing, uint64_t group_bytes, int* rc,
                                mi355_inflate_report* report) {
    *rc = MI355_E_ARG;
    uint64_t sp;
    if (!report || wrapper < 0 || wrapper > 2 || (!stream && stream_len) || !n || !bit_start || !in_bytes || group_bytes < 65536) return nullptr;
    if (!is::is_spacing(spacing, sp) || bit_start[0] != 0 || n > 0x7fffffffull) return nullptr;
    uint64_t total = 0;
    for (uint64_t k = 0; k < n; k++) {
        if (k && bit_start[k] < bit_start[k - 1]) return nullptr;
        if (in_bytes[k] > (1ull << 62) - total) return nullptr;
        total += in_bytes[k];
    }
    static const uint8_t none = 0;
    Handle* h = new Handle;
    h->total = total, h->spacing = sp, h->stream_len = stream_len, h->wrapper = (uint32_t)wrapper, h->mutant = mutant;
    h->ents.resize(n);
    ic::ic_make_entries([&](uint64_t k) { return bit_start[k]; }, [&](uint64_t k) { return in_bytes[k]; }, n, 0u, h->ents.data());
    iw::Rec acc = iw::Rec{ic::V_OK, 0, 0, 0, 0, 0, 0, 0, 0};
    if (mutant == 1) run_build<PointOffByOne>(*h, stream ? stream : &none, in_bytes, group_bytes, acc);
    else run_build<is::Rules>(*h, stream ? stream : &none, in_bytes, group_bytes, acc);
    uint64_t valid = 0;
    const int r = iw::iw_report(acc, ~0ull, *report, &valid);
    *rc = r == iw::IW_OK ? MI355_OK : MI355_E_DATA;
    if (*rc != MI355_OK) {
        delete h;
        return nullptr;
    }
    return h;
}
extern "C" void inflseek_free(void* h) { delete (Handle*)h; }
// v: total, n_entries, n_points, spacing, bytes of windows held, stream_len, wrapper
extern "C" void inflseek_info(void* hv, uint64_t v[7]) {
    const Handle& h = *(Handle*)hv;
    v[0] = h.total, v[1] = h.ents.size(), v[2] = h.pts.size(), v[3] = h.spacing, v[4] = h.store.size(), v[5] = h.stream_len, v[6] = h.wrapper;
}
extern "C" uint64_t inflseek_points(void* hv, uint64_t* bit_pos, uint64_t cap) {
    const Handle& h = *(Handle*)hv;
    for (size_t i = 0; i < h.pts.size() && i < cap; i++) bit_pos[2 * i] = h.ents[h.pts[i]].bit, bit_pos[2 * i + 1] = h.ents[h.pts[i]].pos;
    return h.pts.size();
}
// n ranges (off[i], len[i]) into out + out_at[i]; budget: the group budget.  got / reports: n entries; counts: the plan's four.
// *stray: stores outside a range's len bytes, which only the mutant build looks for -- its ranges go through an arena with guards
extern "C" int inflseek_read(void* hv, const uint8_t* stream, uint64_t stream_len, const uint64_t* off, const uint64_t* len, const uint64_t* out_at,
                             uint64_t n, uint64_t budget, uint8_t* out, uint64_t* got, mi355_inflate_report* reports, uint64_t counts[4],
                             uint64_t* stray) {
    Handle& h = *(Handle*)hv;
    if (!got || !reports || !counts || !stray || (n && (!off || !len || !out_at)) || budget < 65536 || stream_len != h.stream_len) return MI355_E_ARG;
    static const uint8_t none = 0;
    const uint8_t* s = stream ? stream : &none;
    *stray = 0;
    std::vector<is::Range> ranges(n);
    if (h.mutant != 2) {
        for (uint64_t i = 0; i < n; i++) ranges[i] = is::Range{off[i], len[i], len[i] ? out + out_at[i] : nullptr};
        return run_read<is::Rules>(h, s, ranges.data(), n, budget, got, reports, counts);
    }
    // the mutant may store below a range's buffer: every range in an arena of [the stream's size of guard] [len] [64 of guard]
    const uint64_t G = h.total + 64;
    std::vector<std::vector<uint8_t>> arena(n);
    for (uint64_t i = 0; i < n; i++) {
        arena[i].assign(G + len[i] + 64, 0x5A);
        if (len[i]) memcpy(arena[i].data() + G, out + out_at[i], len[i]);
        ranges[i] = is::Range{off[i], len[i], arena[i].data() + G};
    }
    const int rc = run_read<NoLowerBound>(h, s, ranges.data(), n, budget, got, reports, counts);
    for (uint64_t i = 0; i < n; i++) {
        for (uint64_t k = 0; k < G; k++) *stray += arena[i][k] != 0x5A;
        for (uint64_t k = 0; k < 64; k++) *stray += arena[i][G + len[i] + k] != 0x5A;
        if (len[i]) memcpy(out + out_at[i], arena[i].data() + G, len[i]);
    }
    return rc;
}
extern "C" uint64_t inflseek_unfenced_loads(void) { return g_unfenced_loads; }
extern "C" uint32_t inflseek_part_size(void) { return (uint32_t)sizeof(is::Part); }
