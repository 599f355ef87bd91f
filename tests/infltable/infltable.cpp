// Host builds of deflate-rs_amd/csrc/inflate_table.h (TEST INFRASTRUCTURE): the tabled inflate as a SERIAL MODEL -- entry after entry
// in stream order into plain bytes, with the same end-of-entry rules -- and as the THREE PASSES the kernels run: pass 1 with the
// lanes' writes replayed lane by lane, pass 2 with the two windows ping-ponged as the workgroup does, pass 3 in runs of 16 bytes,
// in groups as the driver forms them, into workspaces of exact size.  The product never links this.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../deflate-rs_amd/csrc/inflate_table.h"
#include "../../include/mi355_deflate.h"

using namespace mi355;

static_assert(sizeof(mi355_inflate_report) == 56 && sizeof(ic::Rec) == 56 && sizeof(iw::Rec) == 56, "records and report are 56 bytes");

namespace {

// symbol loads of a match step that the lanes replay found at or beyond the last fence's position, outside [start, min(p, cap)), or
// that saw what the same step wrote: must stay 0
uint64_t g_unfenced_loads = 0;
uint64_t g_fences = 0;
uint64_t g_markers = 0;      // markers written by pass 1
uint64_t g_carry_depth = 0;  // the largest number of window steps a byte of a window was carried through
uint64_t g_groups = 0;       // groups the three-pass build has worked on

struct Scalar {
    static bool leader() { return true; }
    static void sync() {}
    static uint32_t uni(uint32_t v) { return v; }
    static void fence(uint64_t) {}
};

// the table-less call: inflate_write.h with plain byte copies
struct ScalarBytes : Scalar {
    static void store_lits(const uint8_t* lit, uint8_t* out, uint64_t cap, uint64_t lit_p, uint32_t n) {
        for (uint32_t i = 0; i < n && lit_p + i < cap; i++) out[lit_p + i] = lit[i];
    }
    static void copy_match(uint8_t* out, uint64_t cap, uint64_t p, uint32_t len, uint32_t dist) {
        for (uint32_t i = 0; i < len && p + i < cap; i++) out[p + i] = out[p + i - dist];
    }
    static void copy_run(const uint8_t* src, uint8_t* out, uint64_t cap, uint64_t p, uint32_t n) {
        for (uint32_t i = 0; i < n && p + i < cap; i++) out[p + i] = src[i];
    }
};

// the serial model: bytes, the plain serial copy of every inflater; the entries come in order, so the window is simply there
struct SerialSink : Scalar {
    static void store_lits(const uint8_t* lit, it::Sink& o, uint64_t lit_p, uint32_t n) {
        for (uint32_t i = 0; i < n && lit_p + i < o.cap; i++) o.out[lit_p + i] = lit[i];
    }
    static void copy_match(it::Sink& o, uint64_t p, uint32_t len, uint32_t dist) {
        for (uint32_t i = 0; i < len && p + i < o.cap; i++) o.out[p + i] = o.out[p + i - dist];
    }
    static void copy_run(const uint8_t* src, it::Sink& o, uint64_t p, uint32_t n) {
        for (uint32_t i = 0; i < n && p + i < o.cap; i++) o.out[p + i] = src[i];
    }
};

// pass 1 the kernel's way, a lane at a time.  A step of the wave is all its loads, then all its stores; the symbol loads of a match
// step must lie below the position of the last fence (the entry's start at first: what lies in front of it is computed, not loaded).
struct LaneTab : Scalar {
    static uint64_t& fenced() {
        static uint64_t v = 0;
        return v;
    }
    static void fence(uint64_t upto) { fenced() = upto, g_fences++; }
    static void store_lits(const uint8_t* lit, it::Sink& o, uint64_t lit_p, uint32_t n) {
        for (uint32_t lane = 0; lane < 64; lane++) it::it_lane_lits(lit, o.sym, o.base, o.cap, lit_p, n, lane);
    }
    static void copy_match(it::Sink& o, uint64_t p, uint32_t len, uint32_t dist) {
        for (uint32_t at = 0; at < 320 && at < len; at += 64) {
            uint16_t v[64];
            bool on[64];
            for (uint32_t lane = 0; lane < 64; lane++) {  // the step's loads
                const uint32_t i = at + lane;
                on[lane] = i < len && p + i < o.cap;
                if (!on[lane]) continue;
                const uint64_t src = iw::iw_match_src(p, dist, i);
                bool ok = true;
                if (src >= o.start && (src >= fenced() || src >= p || src >= o.cap)) ok = false;  // a load: fenced, and inside what is stored
                if (src < o.start && (o.start - src > it::WIN)) ok = false;                        // a marker: inside the window
                if (!ok) g_unfenced_loads++;
                v[lane] = ok ? it::it_lane_src(o.sym, o.base, o.start, src) : 0;
            }
            // the step's stores, by the lane function itself; they must equal what the loads saw
            for (uint32_t lane = 0; lane < 64; lane++) it::it_lane_match(o.sym, o.base, o.start, o.cap, p, len, dist, at, lane);
            for (uint32_t lane = 0; lane < 64; lane++) {
                if (!on[lane]) continue;
                if (o.sym[p + at + lane - o.base] != v[lane]) g_unfenced_loads++;  // (a lane read what this step wrote)
                if (v[lane] >= it::MARK) g_markers++;
            }
        }
    }
    static void copy_run(const uint8_t* src, it::Sink& o, uint64_t p, uint32_t n) {
        const uint32_t head = it::it_run_head(o.sym, o.base, p, n);
        for (uint32_t lane = 0; lane < 64; lane++) it::it_lane_run_head(src, o.sym, o.base, o.cap, p, head, lane);
        for (uint32_t at = 0; at < 65536 && head + at < n; at += 512)
            for (uint32_t lane = 0; lane < 64; lane++) it::it_lane_run(src, o.sym, o.base, o.cap, p, n, head, at, lane);
    }
};

uint32_t adler32(const uint8_t* d, uint64_t n) {
    uint32_t a = 1, b = 0;
    for (uint64_t i = 0; i < n; i++) {
        a = (a + d[i]) % 65521u;
        b = (b + a) % 65521u;
    }
    return b << 16 | a;
}
uint32_t crc32(const uint8_t* d, uint64_t n) {
    uint32_t c = 0xFFFFFFFFu;
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

// does byte j of the window behind an entry lie inside the stream?  (bytes in front of the stream's first byte are carried too and
// mean nothing: they do not count for the depth)
bool q_is_live(uint64_t start, uint64_t len, uint32_t j) { return start + len + j >= it::WIN; }

// the serial model: one entry after the other, the first failing one ends the walk
void run_serial(const uint8_t* s, uint64_t stream_len, uint32_t wrapper, const std::vector<ic::Entry>& ents, uint64_t total, uint8_t* out,
                uint64_t cap, iw::Rec& acc) {
    ic::Tables t;
    memset(&t, 0, sizeof t);
    for (size_t k = 0; k < ents.size(); k++) {
        it::Sink o{nullptr, out, 0, ents[k].pos, cap, ents[k].pos};
        ic::Rec r;
        it::it_decode_entry<SerialSink>(t, s, stream_len, wrapper, o, ents[k], total, r);
        if (!it::it_report(&r, 1, acc)) return;
    }
}

// the three passes, group after group, as deflate_table_inflate.inc drives them
void run_three(const uint8_t* s, uint64_t stream_len, uint32_t wrapper, const std::vector<ic::Entry>& ents, const uint64_t* in_bytes,
               uint64_t total, uint64_t group_bytes, uint8_t* out, uint64_t cap, iw::Rec& acc) {
    const uint64_t n_all = ents.size();
    ic::Tables t;
    memset(&t, 0, sizeof t);
    std::vector<uint8_t> carry(it::WIN, 0);      // the window in front of the group (zeros in front of the stream)
    std::vector<uint32_t> carry_dep(it::WIN, 0);  // ... and how many window steps each of its bytes has come through
    for (uint64_t k0 = 0; k0 < n_all;) {
        const uint64_t k1 = it::it_group_end([&](uint64_t k) { return in_bytes[k]; }, n_all, k0, group_bytes);
        const uint32_t n = (uint32_t)(k1 - k0);
        g_groups++;
        const uint64_t base = ents[k0].pos, gend = k1 < n_all ? ents[k1].pos : total;
        const uint64_t stored = base < cap ? (gend < cap ? gend : cap) - base : 0;
        Heap<uint16_t> sym(stored);
        Heap<uint8_t> win((size_t)(n + 1) * it::WIN);
        memset(sym.p, 0xEE, stored * 2);
        memset(win.p, 0xEE, (size_t)(n + 1) * it::WIN);
        memcpy(win.p, carry.data(), it::WIN);
        std::vector<ic::Rec> recs(n);
        const ic::Entry* ge = ents.data() + k0;
        // pass 1: every entry on its own (any order would do)
        for (uint32_t k = n; k-- > 0;) {
            it::Sink o{sym.p, nullptr, base, ge[k].pos, cap, ge[k].pos};
            LaneTab::fenced() = ge[k].pos;
            it::it_decode_entry<LaneTab>(t, s, stream_len, wrapper, o, ge[k], total, recs[k]);
        }
        // pass 2: the kernel's walk, every window to its slot; behind each step, it_window_byte's case split once more for the depth
        std::vector<uint32_t> dep[2] = {carry_dep, std::vector<uint32_t>(it::WIN)};
        uint32_t cur = 0;
        const it::Walk wk{sym.p, ge, recs.data(), n, base, cap, win.p, 0u, n, true};
        const uint64_t limit = it::it_window_walk(wk, win.p, [&](uint32_t k) {
            const uint64_t start = ge[k].pos, len = recs[k].end_pos - start;
            for (uint32_t j = 0; j < it::WIN; j++) {
                uint32_t d = 0;
                if (len >= it::WIN || j >= it::WIN - len) {
                    const uint64_t q = start + len + j - it::WIN;
                    if (q < cap && sym.p[q - base] >= it::MARK) d = dep[cur][(sym.p[q - base] - it::MARK) & (it::WIN - 1)] + 1;
                } else {
                    d = dep[cur][j + (uint32_t)len] + 1;
                }
                dep[cur ^ 1][j] = d;
                if (q_is_live(start, len, j) && d > g_carry_depth) g_carry_depth = d;
            }
            cur ^= 1;
        });
        if (limit != it::it_limit(recs.data(), n, base)) abort();  // (the walk and the header's statement of its rule agree)
        // pass 3: the only writes of `out`
        const uint64_t end = limit < cap ? limit : cap;
        for (uint64_t q0 = base; q0 < base + stored; q0 += it::RESOLVE_RUN) it::it_resolve_run(sym.p, win.p, ge, n, base, end, 0, out, q0);
        carry.assign(win.p + (size_t)n * it::WIN, win.p + (size_t)(n + 1) * it::WIN);  // (the driver's copy of the last slot)
        carry_dep = dep[cur];
        if (!it::it_report(recs.data(), n, acc)) return;
        k0 = k1;
    }
}

}  // namespace

// mode 0: the serial model; 1: the three passes.  n == 0: no table, the call is the table-less inflate.
// returns MI355_OK, MI355_E_DATA, MI355_E_OUT_TOO_SMALL or MI355_E_ARG like mi355_inflate_tabled
extern "C" int infltable_inflate(int mode, const uint8_t* stream, uint64_t stream_len, int wrapper, const uint64_t* bit_start,
                                 const uint64_t* in_bytes, uint64_t n, uint64_t group_bytes, uint8_t* out, uint64_t out_cap, uint64_t* out_len,
                                 mi355_inflate_report* report) {
    if (!report || !out_len || wrapper < 0 || wrapper > 2 || (!stream && stream_len) || (!out && out_cap)) return MI355_E_ARG;
    if (n && (!bit_start || !in_bytes)) return MI355_E_ARG;
    if (group_bytes < 65536) return MI355_E_ARG;
    if (n && bit_start[0] != 0) return MI355_E_ARG;  // (entry 0 begins where the stream begins)
    uint64_t total = 0;
    for (uint64_t k = 0; k < n; k++) {
        if (k && bit_start[k] < bit_start[k - 1]) return MI355_E_ARG;
        if (in_bytes[k] > (1ull << 62) - total) return MI355_E_ARG;
        total += in_bytes[k];
    }
    static const uint8_t none = 0;  // (an address the decoder never reads through)
    const uint8_t* s = stream ? stream : &none;
    iw::Rec acc = iw::Rec{ic::V_OK, 0, 0, 0, 0, 0, 0, 0, 0};
    if (!n) {
        ic::Tables t;
        memset(&t, 0, sizeof t);
        iw::iw_inflate<ScalarBytes>(t, s, stream_len, (uint32_t)wrapper, out, out_cap, acc);
    } else {
        std::vector<ic::Entry> ents(n);
        ic::ic_make_entries([&](uint64_t k) { return bit_start[k]; }, [&](uint64_t k) { return in_bytes[k]; }, n, 0u, ents.data());
        if (mode == 0)
            run_serial(s, stream_len, (uint32_t)wrapper, ents, total, out, out_cap, acc);
        else
            run_three(s, stream_len, (uint32_t)wrapper, ents, in_bytes, total, group_bytes, out, out_cap, acc);
    }
    if (iw::iw_judged(acc, (uint32_t)wrapper, out_cap))
        iw::iw_check_trailer(s, stream_len, (uint32_t)wrapper, wrapper == 1 ? adler32(out, acc.out_len) : 0,
                             wrapper == 2 ? crc32(out, acc.out_len) : 0, acc);
    uint64_t valid = 0;
    const int r = iw::iw_report(acc, out_cap, *report, &valid);
    *out_len = r == iw::IW_DATA ? valid : report->out_len;
    return r == iw::IW_OK ? MI355_OK : r == iw::IW_DATA ? MI355_E_DATA : MI355_E_OUT_TOO_SMALL;
}
extern "C" uint64_t infltable_unfenced_loads(void) { return g_unfenced_loads; }
extern "C" uint64_t infltable_fences(void) { return g_fences; }
extern "C" uint64_t infltable_markers(void) { return g_markers; }
extern "C" uint64_t infltable_carry_depth(void) { return g_carry_depth; }
extern "C" uint64_t infltable_groups(void) { return g_groups; }
extern "C" void infltable_reset_counters(void) { g_unfenced_loads = g_fences = g_markers = g_carry_depth = g_groups = 0; }
extern "C" uint32_t infltable_report_size(void) { return (uint32_t)sizeof(mi355_inflate_report); }
extern "C" uint32_t infltable_rec_size(void) { return (uint32_t)sizeof(ic::Rec); }
extern "C" uint32_t infltable_group_entries(void) { return it::GROUP_ENTRIES; }
