// Host build of deflate-rs_amd/csrc/inflate_index.h (TEST INFRASTRUCTURE): the finder replayed lane by lane with its prefilter, and as
// the plain predicate over every offset of a span; the walkers; the link; and the combined call, whose table is judged by the
// three-pass host build of the tabled inflate (tests/infltable/infltable.cpp, compiled in).  Candidates and records live in
// exact-size heap blocks.  MUTANTS of the model, for the cases that must kill them: 1 = a walker stops at b >= c_j, 2 = the link
// follows the next span's candidate instead of the walker's end, 3 = the finder accepts BFINAL = 1.  The product never links this.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../deflate-rs_amd/csrc/inflate_index.h"
#include "../../include/mi355_deflate.h"

using namespace mi355;

static_assert(sizeof(ix::Walk) == 80 && sizeof(mi355_index_walk) == 80, "a walker's record is 80 bytes");

extern "C" int infltable_inflate(int mode, const uint8_t* stream, uint64_t stream_len, int wrapper, const uint64_t* bit_start,
                                 const uint64_t* in_bytes, uint64_t n, uint64_t group_bytes, uint8_t* out, uint64_t out_cap, uint64_t* out_len,
                                 mi355_inflate_report* report);

namespace {

uint64_t g_parses = 0;   // full header parses the finder made
uint64_t g_offsets = 0;  // offsets it looked at

// the walker's policy: a sink that is never reached (capacity 0) -- a call of it is a bug
template <int M>
struct Host {
    static bool leader() { return true; }
    static void sync() {}
    static uint32_t uni(uint32_t v) { return v; }
    static void fence(uint64_t) { abort(); }
    static void store_lits(const uint8_t*, uint8_t*, uint64_t, uint64_t, uint32_t) { abort(); }
    static void copy_match(uint8_t*, uint64_t, uint64_t, uint32_t, uint32_t) { abort(); }
    static void copy_run(const uint8_t*, uint8_t*, uint64_t, uint64_t, uint32_t) { abort(); }
    static bool head(uint32_t h) { return M == 3 ? (h >> 1) == 2 : ix::Rules::head(h); }
    static bool stop(uint64_t b, uint64_t c) { return M == 1 ? c != ix::NOCAND && b >= c : ix::Rules::stop(b, c); }
};
// the finder the kernel's way: 64 lanes, each with the prefilter, a ballot
template <int M>
struct Lanes : Host<M> {
    static uint64_t survivors(const uint8_t* s, uint64_t nbytes, uint64_t base, uint64_t end) {
        uint64_t m = 0;
        for (uint32_t lane = 0; lane < 64; lane++) {
            if (base + lane >= end) continue;
            g_offsets++;
            if (ix::ix_lane_prefilter<Lanes<M>>(s, nbytes, base + lane)) m |= 1ull << lane;
        }
        for (uint64_t x = m; x; x &= x - 1) g_parses++;  // (an upper bound: the first that passes ends the search)
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

template <class P>
void find_all(const uint8_t* s, uint64_t len, uint32_t wrapper, uint64_t S, uint64_t n_spans, uint64_t* cand) {
    ic::Tables t;
    memset(&t, 0, sizeof t);
    for (uint64_t k = n_spans; k-- > 0;) cand[k] = ix::ix_find_span<P>(t, s, len, wrapper, k, S);  // (any order would do)
}
template <class P>
void walk_all(const uint8_t* s, uint64_t len, uint32_t wrapper, uint64_t S, uint64_t n_spans, const uint64_t* cand, ix::Walk* recs) {
    ic::Tables t;
    memset(&t, 0, sizeof t);
    for (uint64_t k = n_spans; k-- > 0;) ix::ix_walk_span<P>(t, s, len, wrapper, cand, n_spans, S, k, cand[k], recs[k]);
}

void link(int mutant, const ix::Walk* w, const uint64_t* cand, uint64_t n_spans, std::vector<uint64_t>& chain) {
    if (mutant != 2) {
        ix::ix_link(w, n_spans, [&](uint64_t k) { chain.push_back(k); });
        return;
    }
    for (uint64_t k = 0;;) {  // the mutant: to the next span that has a candidate, wherever the walker ended
        chain.push_back(k);
        if (w[k].how != ix::END_LINK) return;
        uint64_t j = k + 1;
        while (j < n_spans && cand[j] == ix::NOCAND) j++;
        if (j >= n_spans) return;
        k = j;
    }
}

template <int M>
void run(int lanes, const uint8_t* s, uint64_t len, uint32_t wrapper, uint64_t S, uint64_t n_spans, uint64_t* cand, ix::Walk* recs) {
    if (lanes) find_all<Lanes<M>>(s, len, wrapper, S, n_spans, cand);
    else find_all<Plain<M>>(s, len, wrapper, S, n_spans, cand);
    walk_all<Host<M>>(s, len, wrapper, S, n_spans, cand, recs);
}
void run_m(int mutant, int lanes, const uint8_t* s, uint64_t len, uint32_t wrapper, uint64_t S, uint64_t n_spans, uint64_t* cand, ix::Walk* recs) {
    if (mutant == 1) run<1>(lanes, s, len, wrapper, S, n_spans, cand, recs);
    else if (mutant == 3) run<3>(lanes, s, len, wrapper, S, n_spans, cand, recs);
    else run<0>(lanes, s, len, wrapper, S, n_spans, cand, recs);
}

bool bad_args(const uint8_t* stream, uint64_t len, int wrapper, uint64_t S, const void* report) {
    return !report || (!stream && len) || wrapper < 0 || wrapper > 2 || S < ix::SPAN_MIN || S > ix::SPAN_MAX;
}

}  // namespace

extern "C" uint64_t inflindex_n_spans(uint64_t stream_len, uint64_t S) { return ix::ix_n_spans(stream_len, S); }

// the candidates and the walkers' records, n_spans of each; lanes: the finder with its prefilter (else the plain predicate)
extern "C" int inflindex_scan(int mutant, int lanes, const uint8_t* stream, uint64_t stream_len, int wrapper, uint64_t S, uint64_t* cand,
                              mi355_index_walk* recs) {
    if (bad_args(stream, stream_len, wrapper, S, recs) || !cand) return MI355_E_ARG;
    run_m(mutant, lanes, stream ? stream : &none, stream_len, (uint32_t)wrapper, S, ix::ix_n_spans(stream_len, S), cand,
          reinterpret_cast<ix::Walk*>(recs));
    return MI355_OK;
}

// mi355_inflate_index; chain_span (cap entries, may be NULL): the span of every entry's walker
extern "C" int inflindex_index(int mutant, const uint8_t* stream, uint64_t stream_len, int wrapper, uint64_t S, mi355_block_info* blocks,
                               uint64_t* chain_span, uint64_t cap, uint64_t* n_blocks, mi355_inflate_report* report) {
    if (bad_args(stream, stream_len, wrapper, S, report) || !n_blocks || (!blocks && cap)) return MI355_E_ARG;
    const uint8_t* s = stream ? stream : &none;
    const uint64_t n_spans = ix::ix_n_spans(stream_len, S);
    Heap<uint64_t> cand(n_spans);
    Heap<ix::Walk> recs(n_spans);
    run_m(mutant, 1, s, stream_len, (uint32_t)wrapper, S, n_spans, cand.p, recs.p);
    std::vector<uint64_t> chain;
    link(mutant, recs.p, cand.p, n_spans, chain);
    iw::Rec acc;
    ix::ix_report(recs.p, chain.data(), chain.size(), acc);
    uint64_t valid = 0;
    const int r = iw::iw_report(acc, ~0ull, *report, &valid);
    *n_blocks = chain.size();
    if (chain.size() > cap) return MI355_E_OUT_TOO_SMALL;
    for (size_t e = 0; e < chain.size(); e++) {
        const ix::Walk& x = recs.p[chain[e]];
        blocks[e] = mi355_block_info{x.btype, e + 1 == chain.size() && x.how == ix::END_FINAL ? 1u : 0u, 0u, 0u, x.count, x.start};
        if (chain_span) chain_span[e] = chain[e];
    }
    return r == iw::IW_DATA ? MI355_E_DATA : MI355_OK;
}

// mi355_inflate_parallel: the index, then the three passes of the tabled inflate from its table (one entry: the table-less inflate)
extern "C" int inflindex_parallel(int mutant, const uint8_t* stream, uint64_t stream_len, int wrapper, uint64_t S, uint64_t group_bytes,
                                  uint8_t* out, uint64_t out_cap, uint64_t* out_len, mi355_inflate_report* report) {
    if (bad_args(stream, stream_len, wrapper, S, report) || !out_len || (!out && out_cap)) return MI355_E_ARG;
    const uint64_t n_spans = ix::ix_n_spans(stream_len, S);
    Heap<mi355_block_info> blocks(n_spans);
    uint64_t n = 0;
    mi355_inflate_report xr;
    const int rc = inflindex_index(mutant, stream, stream_len, wrapper, S, blocks.p, nullptr, n_spans, &n, &xr);
    if (rc != MI355_OK && rc != MI355_E_DATA) return rc;
    if (n < 2) n = 0;
    Heap<uint64_t> bits(n), bytes(n);
    for (uint64_t k = 0; k < n; k++) bits.p[k] = blocks.p[k].bit_start, bytes.p[k] = blocks.p[k].in_bytes;
    return infltable_inflate(1, stream, stream_len, wrapper, bits.p, bytes.p, n, group_bytes, out, out_cap, out_len, report);
}

// every block of the stream's serial walk, for the tests' preconditions: where it begins and its three header bits, until the BFINAL
// block, a failure or `cap` (a third sibling of iw_inflate's loop, counting only; not part of the model)
extern "C" uint64_t inflindex_blocks(const uint8_t* stream, uint64_t stream_len, int wrapper, uint64_t* bits, uint32_t* heads, uint64_t cap) {
    uint64_t hdr, trailer, n = 0;
    if (!stream || !ic::ic_parse_frame(stream, stream_len, (uint32_t)wrapper, hdr, trailer)) return 0;
    ic::Tables t;
    memset(&t, 0, sizeof t);
    ic::Bits b = ic::ic_bits(stream + hdr, stream_len - hdr - trailer, 0);
    iw::Sink o{nullptr, 0, 0};
    uint64_t p = ix::BIAS;
    for (uint64_t guard = 0; guard <= b.end && n < cap; guard++) {
        const uint64_t at = b.pos;
        const uint32_t h = ic::ic_take(b, 3);
        if (b.over || (h >> 1) == 3) break;
        ic::Fail f = ic::ic_fail(ic::V_OK, 0, 0);
        if ((h >> 1) == 0) f = iw::iw_stored_block<Host<0>>(b, o, p);
        else {
            if ((h >> 1) == 1) ic::ic_fixed_tables(t);
            else f = ic::ic_dynamic_header<Host<0>>(t, b, p);
            if (!f.status) f = iw::iw_huffman_block<Host<0>>(t, b, o, p);
        }
        if (f.status) break;
        bits[n] = at, heads[n] = h, n++;
        if (h & 1) break;
    }
    return n;
}

// one bit offset of the raw deflate data: bit 0 = the predicate holds, bit 1 = the prefilter lets it through
extern "C" uint32_t inflindex_is_start(const uint8_t* stream, uint64_t stream_len, int wrapper, uint64_t bit) {
    uint64_t hdr, trailer;
    if (!stream || !ic::ic_parse_frame(stream, stream_len, (uint32_t)wrapper, hdr, trailer)) return 0;
    ic::Tables t;
    memset(&t, 0, sizeof t);
    const uint64_t nbytes = stream_len - hdr - trailer;
    return (ix::ix_is_start<Host<0>>(t, stream + hdr, nbytes, bit) ? 1u : 0u) | (ix::ix_lane_prefilter<Host<0>>(stream + hdr, nbytes, bit) ? 2u : 0u);
}

extern "C" uint64_t inflindex_parses(void) { return g_parses; }
extern "C" uint64_t inflindex_offsets(void) { return g_offsets; }
extern "C" void inflindex_reset_counters(void) { g_parses = g_offsets = 0; }
extern "C" uint32_t inflindex_walk_size(void) { return (uint32_t)sizeof(ix::Walk); }
extern "C" uint64_t inflindex_span_min(void) { return ix::SPAN_MIN; }
extern "C" uint64_t inflindex_span_default(void) { return ix::SPAN_DEFAULT; }
