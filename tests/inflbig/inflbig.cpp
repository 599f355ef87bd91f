// Host build of deflate-rs_amd/csrc/inflate_bigmembers.h (TEST INFRASTRUCTURE): mi355_inflate_members as the device runs it with the
// large plain members found and decoded in parallel.  Paths A and B, the checksum pass and the report are the host build of
// tests/inflmembers/ itself (its text is included, not written again); what is here is Path B's chain() by ib_chain: discovery with the
// index finder replayed lane by lane in an exact-size candidate block, and the three passes over a group of parts -- pass 1 with the
// lanes' writes replayed lane by lane, pass 2 a window chain per part, pass 3 in runs of 16 symbols -- in exact-size workspaces.
// MUTANTS of the new decisions, for the cases that must kill them: 1 = a member's positions count from its place in the output (a
// distance is limited by the file's bytes, not the member's), 2 = the trailer lies one byte further when the BFINAL block ends on a
// byte boundary.  The product never links this.
#include "../inflmembers/inflmembers.cpp"

#include "../../deflate-rs_amd/csrc/inflate_bigmembers.h"

namespace {

uint64_t g_threshold = ib::PAR_DEFAULT, g_index_span = ix::SPAN_DEFAULT, g_group_bytes = 256ull << 20;
ib::Stats g_stats = {0, 0, 0, 0, 0, 0};

// discovery: the index finder's prefilter lane by lane, the walkers' (never executed) sink, a hinted member's extent for the head
struct BigP : Host<0> {
    static bool head(uint32_t h) { return ix::Rules::head(h); }
    static uint64_t survivors(const uint8_t* s, uint64_t nbytes, uint64_t base, uint64_t end) {
        uint64_t m = 0;
        for (uint32_t lane = 0; lane < 64; lane++)
            if (base + lane < end && ix::ix_lane_prefilter<BigP>(s, nbytes, base + lane)) m |= 1ull << lane;
        return m;
    }
};
// pass 1 the kernel's way, a lane at a time
struct TabP {
    static bool leader() { return true; }
    static void sync() {}
    static uint32_t uni(uint32_t v) { return v; }
    static void fence(uint64_t) {}
    static void store_lits(const uint8_t* lit, it::Sink& o, uint64_t lit_p, uint32_t n) {
        for (uint32_t lane = 0; lane < 64; lane++) it::it_lane_lits(lit, o.sym, o.base, o.cap, lit_p, n, lane);
    }
    static void copy_match(it::Sink& o, uint64_t p, uint32_t len, uint32_t dist) {
        for (uint32_t at = 0; at < 320 && at < len; at += 64)
            for (uint32_t lane = 0; lane < 64; lane++) it::it_lane_match(o.sym, o.base, o.start, o.cap, p, len, dist, at, lane);
    }
    static void copy_run(const uint8_t* src, it::Sink& o, uint64_t p, uint32_t n) {
        const uint32_t head = it::it_run_head(o.sym, o.base, p, n);
        for (uint32_t lane = 0; lane < 64; lane++) it::it_lane_run_head(src, o.sym, o.base, o.cap, p, head, lane);
        for (uint32_t at = 0; at < 65536 && head + at < n; at += 512)
            for (uint32_t lane = 0; lane < 64; lane++) it::it_lane_run(src, o.sym, o.base, o.cap, p, n, head, at, lane);
    }
};

template <int M>
struct MutRules {
    static uint64_t trailer_at(uint64_t end_bit) { return M == 2 ? end_bit / 8 + 1 : ib::Rules::trailer_at(end_bit); }
    static uint64_t origin(uint64_t p) { return M == 1 ? p : ib::Rules::origin(p); }
};

// im_run's backend: tests/inflmembers' own, with chain() by ib_chain
template <int M>
struct BigBe : HostBe<Lanes<0>> {
    std::vector<uint64_t> dcand;   // a discovery's candidates: one per span of the member's grid
    std::vector<uint8_t> carry;    // the window a group leaves for the next one
    using HostBe<Lanes<0>>::decode;  // (Path A's, beside the groups')

    uint64_t threshold() const { return g_threshold; }
    uint64_t span() const { return g_index_span; }
    uint64_t group_bytes() const { return g_group_bytes; }

    int chain(uint64_t o, uint64_t p, bool ignore_hints, std::vector<im::Member>& rows, std::vector<iw::Rec>& got, im::ChainEnd& e) {
        if (g_threshold && o < n && n - o >= g_threshold)
            return ib::ib_chain<MutRules<M>>(*this, s, n, o, p, out, out_cap, ignore_hints, (uint32_t)g_room, rows, got, e, g_stats);
        return serial(o, p, ignore_hints, 0u, (uint32_t)g_room, rows, got, e);
    }
    int serial(uint64_t o, uint64_t p, bool ignore_hints, uint32_t behind, uint32_t room, std::vector<im::Member>& rows, std::vector<iw::Rec>& got,
               im::ChainEnd& e) {
        g_chains++;
        rows.assign(room, im::Member{0, 0, 0, 0, 0, 0});
        got.resize(room);
        im::im_chain_behind<Lanes<0>>(t, s, n, o, p, out, out_cap, ignore_hints, behind, rows.data(), got.data(), room, e);
        return 0;
    }
    int head(uint64_t o, ib::Head& h) {
        ib::ib_head<BigP>(s, n, o, h);
        return 0;
    }
    int round(uint64_t o, bool first, uint64_t rewalk, uint64_t k_lo, uint64_t k_hi, ib::Head& head, std::vector<ix::Walk>& w) {
        if (first) {
            dcand.assign(ix::ix_n_spans(n - o, g_index_span), ix::NOCAND);
            dcand.shrink_to_fit();
            ib::ib_head<BigP>(s, n, o, head);
        }
        if (k_hi > dcand.size() || w.size() < k_hi || rewalk >= k_hi) abort();
        for (uint64_t k = first ? 0 : k_lo; k < k_hi; k++) dcand[k] = ib::ib_find_span<BigP>(t, s, n, o, k, g_index_span);
        // (the kernel's walkers see the candidates of [0, k_hi) only: the others are handed over as they are, ib_walk_span must not read them)
        Heap<uint64_t> seen(k_hi);
        for (uint64_t k = 0; k < k_hi; k++) seen.p[k] = dcand[k];
        for (uint64_t b = k_hi - k_lo + 1; b-- > 0;) {  // (any order would do)
            const uint64_t k = b == 0 ? rewalk : k_lo + b - 1;
            ib::ib_walk_span<BigP>(t, s, n, o, seen.p, g_index_span, k, k_hi, w[k]);
        }
        return 0;
    }
    int decode(const ib::Plan& g, bool first, std::vector<ic::Rec>& got) {
        const uint32_t k = (uint32_t)g.ents.size(), np = (uint32_t)g.parts.size();
        got.resize(k);
        Heap<uint16_t> sym(g.syms);
        Heap<uint8_t> win((size_t)(k + 1) * it::WIN);
        Heap<uint64_t> limits(np);
        memset(sym.p, 0xEE, g.syms * 2);
        memset(win.p, 0xEE, (size_t)(k + 1) * it::WIN);
        if (g.parts[0].carried) {
            if (first || carry.size() != it::WIN) abort();
            memcpy(win.p, carry.data(), it::WIN);
        }
        // pass 1: every entry on its own (any order would do)
        for (uint32_t e = k; e-- > 0;) ib::ib_decode_entry<TabP>(t, sym.p, g.parts[g.ents[e].item], g.ents[e], got[e]);
        // pass 2: the kernel's walk per part, from the carried window or from zeros
        for (uint32_t j = np; j-- > 0;) {
            const ib::Part& pt = g.parts[j];
            const ic::Rec* pr = got.data() + pt.e0;
            const it::Walk wk{sym.p + pt.sym_off, g.ents.data() + pt.e0, pr, pt.n, pt.base, pt.cap, win.p, pt.e0, k, true};
            limits.p[j] = it::it_window_walk(wk, pt.carried ? win.p + (size_t)pt.e0 * it::WIN : nullptr);
            if (limits.p[j] != it::it_limit(pr, pt.n, pt.base)) abort();  // (the walk and the header's statement of its rule agree)
        }
        // pass 3: the only writes of `out`
        for (uint64_t f0 = 0; f0 < g.syms; f0 += it::RESOLVE_RUN) ib::ib_resolve_run(sym.p, win.p, g.ents.data(), g.parts.data(), np, limits.p, f0);
        if (g.carry_out) carry.assign(win.p + (size_t)k * it::WIN, win.p + (size_t)(k + 1) * it::WIN);
        return 0;
    }
};

template <int M>
int run_big(const uint8_t* s, uint64_t n, uint64_t S, uint8_t* out, uint64_t cap, uint64_t* out_len, mi355_member_info* members, uint64_t mcap,
            uint64_t* n_members, mi355_inflate_report* report) {
    const uint64_t n_spans = im::im_n_spans(n, S);
    Heap<uint64_t> cand(n_spans);
    for (uint64_t k = 0; k < n_spans; k++) cand.p[k] = im::NOCAND;
    BigBe<M> be;
    be.s = s, be.n = n, be.out = out, be.out_cap = cap, be.S = S, be.n_spans = n_spans, be.cand = cand.p;
    memset(&be.t, 0, sizeof be.t);
    std::vector<im::Member> mem;
    std::vector<iw::Rec> recs;
    im::im_run(be, n, S, mem, recs);
    uint64_t total = 0;
    if (!(im::im_total(mem, total) && total > cap)) sums(s, out, cap, mem, recs);
    uint64_t valid = 0;
    const int r = im::im_report(mem, recs, cap, *report, &valid);
    *out_len = r == iw::IW_DATA ? valid : report->out_len;
    give(mem, members, mcap, n_members);
    return r == iw::IW_OK ? MI355_OK : r == iw::IW_DATA ? MI355_E_DATA : MI355_E_OUT_TOO_SMALL;
}

}  // namespace

// mi355_inflate_members as the device runs it: S the member span, the other settings by inflbig_set
extern "C" int inflbig_run(int mutant, uint64_t S, const uint8_t* stream, uint64_t stream_len, uint8_t* out, uint64_t out_cap, uint64_t* out_len,
                           mi355_member_info* members, uint64_t members_cap, uint64_t* n_members, mi355_inflate_report* report) {
    if (bad_args(stream, stream_len, out, out_cap, out_len, members, members_cap, report) || S < im::SPAN_MIN || S > im::SPAN_MAX)
        return MI355_E_ARG;
    const uint8_t* s = stream ? stream : &none;
    if (mutant == 1) return run_big<1>(s, stream_len, S, out, out_cap, out_len, members, members_cap, n_members, report);
    if (mutant == 2) return run_big<2>(s, stream_len, S, out, out_cap, out_len, members, members_cap, n_members, report);
    return run_big<0>(s, stream_len, S, out, out_cap, out_len, members, members_cap, n_members, report);
}
// MI355_CFG_INFLATE_MEMBER_PARALLEL_BYTES (0: off), MI355_CFG_INFLATE_INDEX_SPAN_BYTES, MI355_CFG_INFLATE_GROUP_BYTES
extern "C" int inflbig_set(uint64_t threshold, uint64_t index_span, uint64_t group_bytes) {
    if ((threshold && (threshold < ib::PAR_MIN || threshold > ib::PAR_MAX)) || index_span < ix::SPAN_MIN || index_span > ix::SPAN_MAX ||
        group_bytes < 65536)
        return MI355_E_ARG;
    g_threshold = threshold, g_index_span = index_span, g_group_bytes = group_bytes;
    return MI355_OK;
}
extern "C" void inflbig_reset_stats(void) { g_stats = ib::Stats{0, 0, 0, 0, 0, 0}; }
extern "C" void inflbig_stats(uint64_t v[6]) {
    v[0] = g_stats.parallel, v[1] = g_stats.handed, v[2] = g_stats.spans, v[3] = g_stats.walkers, v[4] = g_stats.entries, v[5] = g_stats.sets;
}
extern "C" uint64_t inflbig_first_extent(uint64_t threshold, uint64_t S) { return ib::ib_first_extent(threshold, S); }
extern "C" uint64_t inflbig_par_default(void) { return ib::PAR_DEFAULT; }
extern "C" uint32_t inflbig_part_size(void) { return (uint32_t)sizeof(ib::Part); }
