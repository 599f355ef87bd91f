// Host build of deflate-rs_amd/csrc/inflate_cut.h (TEST INFRASTRUCTURE): the cuts of a seek handle as the kernels and their driver run
// them -- the build's pass 1 recording cuts into slots of exact size, a read as its plan of pieces and sets with one turn per cut,
// flatten thread by thread in steps with all loads of a step in front of its stores, then passes 2 and 3 of inflate_seek.h --, in two
// forms: pass 1 replayed lane by lane (the kernel's writes), or by a serial model that stores a token in one plain loop.  Three
// mutants of the decisions: the cut rule measured from the entry's start, flatten's inside test off by one, the stop test without
// the position.  With cut_bytes 0 the handle is tests/inflseek's: whole entries, three passes.  The product never links this.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../deflate-rs_amd/csrc/inflate_cut.h"
#include "../../include/mi355_deflate.h"

using namespace mi355;

static_assert(sizeof(mi355_inflate_report) == 56 && sizeof(ic::Rec) == 56 && sizeof(iw::Rec) == 56, "records and report are 56 bytes");
static_assert(sizeof(icut::Cut) == 24 && sizeof(mi355_seek_cut) == 24 && sizeof(icut::Item) == 56 && sizeof(icut::Rec) == 72, "the cuts' records");

namespace {

uint64_t g_bad_loads = 0;  // symbol loads of a match step in front of the last fence, or outside what is stored: must stay 0

struct Scalar {
    static bool leader() { return true; }
    static void sync() {}
    static uint32_t uni(uint32_t v) { return v; }
};

// pass 1 the kernel's way, a lane at a time (tests/inflseek's LaneTab)
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
                if (!ok) g_bad_loads++;
                v[lane] = ok ? it::it_lane_src(o.sym, o.base, o.start, src) : 0;
            }
            for (uint32_t lane = 0; lane < 64; lane++) it::it_lane_match(o.sym, o.base, o.start, o.cap, p, len, dist, at, lane);
            for (uint32_t lane = 0; lane < 64; lane++)
                if (on[lane] && o.sym[p + at + lane - o.base] != v[lane]) g_bad_loads++;
        }
    }
    static void copy_run(const uint8_t* src, it::Sink& o, uint64_t p, uint32_t n) {
        const uint32_t head = it::it_run_head(o.sym, o.base, p, n);
        for (uint32_t lane = 0; lane < 64; lane++) it::it_lane_run_head(src, o.sym, o.base, o.cap, p, head, lane);
        for (uint32_t at = 0; at < 65536 && head + at < n; at += 512)
            for (uint32_t lane = 0; lane < 64; lane++) it::it_lane_run(src, o.sym, o.base, o.cap, p, n, head, at, lane);
    }
};
// the serial model: a token's symbols in one plain loop, in order
struct SerialTab : Scalar {
    static void fence(uint64_t) {}
    static void store_lits(const uint8_t* lit, it::Sink& o, uint64_t lit_p, uint32_t n) {
        for (uint32_t i = 0; i < n; i++)
            if (lit_p + i < o.cap) o.sym[lit_p + i - o.base] = lit[i & (ic::LIT_RUN - 1)];
    }
    static void copy_match(it::Sink& o, uint64_t p, uint32_t len, uint32_t dist) {
        for (uint32_t i = 0; i < len; i++) {
            if (p + i >= o.cap) break;
            const uint64_t src = p + i - dist;
            o.sym[p + i - o.base] = src >= o.start ? o.sym[src - o.base] : (uint16_t)(it::MARK + (uint32_t)(src + it::WIN - o.start));
        }
    }
    static void copy_run(const uint8_t* src, it::Sink& o, uint64_t p, uint32_t n) {
        for (uint32_t i = 0; i < n; i++)
            if (p + i < o.cap) o.sym[p + i - o.base] = src[i];
    }
};

// the mutants
struct FromEntryStart : icut::Rules {
    static bool cut_here(uint64_t p, uint64_t, uint64_t entry_pos, uint64_t cut_bytes) { return p - entry_pos >= cut_bytes; }
};
struct InsideOffByOne : icut::Rules {
    static bool flat_inside(uint64_t q, uint64_t entry_pos) { return q > entry_pos; }
};
struct StopIgnoresPos : icut::Rules {
    static bool stops(uint64_t bit, uint64_t, const icut::Cut& next) { return bit == next.bit; }
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
    std::vector<icut::Cut> cuts;
    std::vector<uint64_t> cut0;
    uint64_t total = 0, spacing = 0, stream_len = 0, cut_bytes = 0, surplus = 0;  // (surplus: cuts a walk counted beyond its slots)
    uint32_t wrapper = 0;
    int mutant = 0, serial = 0;
};

// the build as deflate_seek_inflate.inc drives it (tests/inflseek's run_build); with cuts, pass 1 is k_inflate_tab_cut's
template <class P, class R>
void run_build(Handle& h, const uint8_t* s, const uint64_t* in_bytes, uint64_t group_bytes, iw::Rec& acc) {
    const uint64_t n_all = h.ents.size(), total = h.total, cb = h.cut_bytes;
    is::is_points<is::Rules>(h.ents.data(), n_all, h.spacing, h.pts);
    h.store.assign((h.pts.size() - 1) * (size_t)it::WIN, 0xEE);
    if (cb) h.cut0.assign(1, 0);
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
        std::vector<uint64_t> slot0(n + 1, 0);
        for (uint32_t k = 0; k < n && cb; k++) slot0[k + 1] = slot0[k] + icut::ict_slots(in_bytes[k0 + k], cb);
        Heap<icut::Cut> slots(slot0[n]);
        std::vector<uint32_t> n_cut(n, 0);
        const ic::Entry* ge = h.ents.data() + k0;
        for (uint32_t k = n; k-- > 0;) {
            it::Sink o{sym.p, nullptr, base, ge[k].pos, total, ge[k].pos};
            LaneTab::fenced() = ge[k].pos;
            if (!cb) {
                it::it_decode_entry<P>(t, s, h.stream_len, h.wrapper, o, ge[k], total, recs[k]);
                continue;
            }
            icut::Rec r;
            const uint32_t ns = (uint32_t)(slot0[k + 1] - slot0[k]);
            icut::ict_build_entry<P, R>(t, s, h.stream_len, h.wrapper, o, ge[k], total, cb, slots.p + slot0[k], ns, r);
            recs[k] = r;
            n_cut[k] = r.n_cuts < ns ? r.n_cuts : ns;
            h.surplus += r.n_cuts > ns ? r.n_cuts - ns : 0;
        }
        const uint64_t limit = it::it_window_walk(it::Walk{sym.p, ge, recs.data(), n, base, total, win.p, 0u, n, true}, win.p);  // k_inflate_tab_window
        if (limit != it::it_limit(recs.data(), n, base)) abort();  // (the walk and the header's statement of its rule agree)
        for (; next_pt < h.pts.size() && h.pts[next_pt] < k1; next_pt++)
            memcpy(h.store.data() + (next_pt - 1) * (size_t)it::WIN, win.p + (size_t)(h.pts[next_pt] - k0) * it::WIN, it::WIN);
        if (h.wrapper && stored) {
            const uint64_t end = limit < base + stored ? limit : base + stored;
            for (uint64_t q0 = base; q0 < base + stored; q0 += it::RESOLVE_RUN)
                it::it_resolve_run<is::Rules>(sym.p, win.p, ge, n, base, end, base, scratch.p, q0);
        }
        carry.assign(win.p + (size_t)n * it::WIN, win.p + (size_t)(n + 1) * it::WIN);
        if (!it::it_report(recs.data(), n, acc)) return;
        for (uint32_t k = 0; k < n && cb; k++) {
            h.cuts.insert(h.cuts.end(), slots.p + slot0[k], slots.p + slot0[k] + n_cut[k]);
            h.cut0.push_back(h.cuts.size());
        }
        if (h.wrapper && stored) adler = adler32(adler, scratch.p, stored), crc = crc32(crc, scratch.p, stored);
        k0 = k1;
    }
    if (h.wrapper) {
        const uint64_t tn = h.wrapper == 1 ? 4 : 8;
        if (h.stream_len >= tn && !is::is_trailer_ok(h.wrapper, s + h.stream_len - tn, adler, crc, total)) is::is_checksum_failed(acc);
    }
}

// flatten of one entry, the workgroup's: per cut a step of 1024 threads, every load of the step in front of its stores
template <class R>
void flatten_entry(const is::Part& pt, const ic::Entry& e, const icut::Item* items, const icut::Rec* crecs, uint32_t n, uint16_t* sym, ic::Rec& out) {
    uint16_t* psym = sym + pt.sym_off;
    ic::Rec acc{ic::V_OK, 0, 0, 0, 0, 0, e.bit, e.pos, 0};
    bool more = true;
    for (uint32_t k = 0; k < n && more; k++) {
        const uint64_t c_pos = items[k].c.pos;
        uint64_t upto = icut::ict_fold(acc, crecs, items, k, more);
        if (upto > pt.cap) upto = pt.cap;
        if (!k || upto <= c_pos) continue;
        std::vector<uint16_t> v(upto - c_pos);
        for (uint64_t q = c_pos; q < upto; q++) v[q - c_pos] = icut::ict_flat<R>(psym, pt.base, e.pos, c_pos, q);
        for (uint64_t q = c_pos; q < upto; q++) psym[q - pt.base] = v[q - c_pos];
    }
    out = acc;
}

// one launch set of a read
template <class P, class R>
void run_set(const Handle& h, const is::Set& s, std::vector<ic::Rec>& recs, icut::Counts& cc) {
    const size_t np = s.parts.size(), ne = s.ents.size();
    Heap<uint16_t> sym(s.syms);
    Heap<uint8_t> win((size_t)s.slots * it::WIN);
    memset(sym.p, 0xEE, s.syms * 2);
    memset(win.p, 0xEE, (size_t)s.slots * it::WIN);
    recs.assign(ne, ic::Rec());
    ic::Tables t;
    memset(&t, 0, sizeof t);
    cc.launches += h.cut_bytes ? 4 : 3;
    if (!h.cut_bytes) {
        for (size_t k = ne; k-- > 0;) {  // pass 1: every entry on its own (any order would do)
            LaneTab::fenced() = s.ents[k].pos;
            is::is_decode_entry<P>(t, sym.p, s.parts[s.ents[k].item], s.ents[k], recs[k]);
        }
    } else {
        std::vector<uint64_t> ent0(np);
        for (size_t j = 0; j < np; j++) ent0[j] = h.pts[is::is_point_of(h.ents.data(), h.pts, s.parts[j].lo)];
        std::vector<icut::Item> items;
        std::vector<uint32_t> first;
        icut::ict_items(s, ent0, h.cut0, h.cuts, items, first);
        cc.cuts += items.size(), cc.steps += items.size() - ne;
        std::vector<icut::Rec> crecs(items.size());
        for (size_t i = items.size(); i-- > 0;) {  // pass 1 over cuts, any order
            LaneTab::fenced() = items[i].c.pos;
            const ic::Entry& e = s.ents[items[i].ent];
            icut::ict_decode_cut<P, R>(t, sym.p, s.parts[e.item], e, items[i], crecs[i]);
        }
        for (size_t k = 0; k < ne; k++)
            flatten_entry<R>(s.parts[s.ents[k].item], s.ents[k], items.data() + first[k], crecs.data() + first[k], first[k + 1] - first[k], sym.p, recs[k]);
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
        is::is_resolve_set<is::Rules>(sym.p, win.p, s.ents.data(), s.parts.data(), (uint32_t)np, limits.data(), f0);
}

template <class P, class R>
int run_read(Handle& h, const uint8_t* s, is::Range* ranges, uint64_t n, uint64_t budget, uint64_t* got, mi355_inflate_report* reports,
             uint64_t counts[4], uint64_t cut_counts[4]) {
    std::vector<is::Set> sets;
    is::Counts cnt;
    is::is_plan(h.ents.data(), h.ents.size(), h.total, h.pts, ranges, n, budget, s, h.stream_len, h.wrapper, sets, cnt);
    counts[0] = cnt.entries, counts[1] = cnt.symbols, counts[2] = cnt.steps, counts[3] = cnt.sets;
    icut::Counts cc{0, cnt.symbols, 0, 0};
    std::vector<iw::Rec> acc(n, iw::Rec{ic::V_OK, 0, 0, 0, 0, 0, 0, 0, 0});
    std::vector<uint8_t> failed(n, 0);
    std::vector<ic::Rec> recs;
    for (is::Set& set : sets) {
        is::is_drop(set, failed);
        run_set<P, R>(h, set, recs, cc);
        for (const is::Part& pt : set.parts)
            if (!failed[pt.range] && !is::is_report(recs.data(), pt, acc[pt.range])) failed[pt.range] = 1;
    }
    cut_counts[0] = cc.cuts, cut_counts[1] = cc.symbols, cut_counts[2] = cc.steps, cut_counts[3] = cc.launches;
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

template <class P>
void build_by_mutant(Handle& h, const uint8_t* s, const uint64_t* in_bytes, uint64_t group_bytes, iw::Rec& acc) {
    if (h.mutant == 1) run_build<P, FromEntryStart>(h, s, in_bytes, group_bytes, acc);
    else run_build<P, icut::Rules>(h, s, in_bytes, group_bytes, acc);
}
template <class P>
int read_by_mutant(Handle& h, const uint8_t* s, is::Range* ranges, uint64_t n, uint64_t budget, uint64_t* got, mi355_inflate_report* reports,
                   uint64_t counts[4], uint64_t cut_counts[4]) {
    if (h.mutant == 2) return run_read<P, InsideOffByOne>(h, s, ranges, n, budget, got, reports, counts, cut_counts);
    if (h.mutant == 3) return run_read<P, StopIgnoresPos>(h, s, ranges, n, budget, got, reports, counts, cut_counts);
    return run_read<P, icut::Rules>(h, s, ranges, n, budget, got, reports, counts, cut_counts);
}

}  // namespace

// mutant 0: none; 1: the cut rule from the entry's start; 2: flatten's inside test off by one; 3: the stop test without the position.
// serial: pass 1 by the serial model instead of lane by lane.  *rc: MI355_OK and a handle, else NULL
extern "C" void* inflcut_build(int mutant, int serial, const uint8_t* stream, uint64_t stream_len, int wrapper, const uint64_t* bit_start,
                               const uint64_t* in_bytes, uint64_t n, uint64_t spacing, uint64_t group_bytes, uint64_t cut_bytes, int* rc,
                               mi355_inflate_report* report) {
    *rc = MI355_E_ARG;
    uint64_t sp;
    if (!report || wrapper < 0 || wrapper > 2 || (!stream && stream_len) || !n || !bit_start || !in_bytes || group_bytes < 65536) return nullptr;
    if (!is::is_spacing(spacing, sp) || !icut::ict_cut_bytes_ok(cut_bytes) || bit_start[0] != 0 || n > 0x7fffffffull) return nullptr;
    uint64_t total = 0;
    for (uint64_t k = 0; k < n; k++) {
        if (k && bit_start[k] < bit_start[k - 1]) return nullptr;
        if (in_bytes[k] > (1ull << 62) - total) return nullptr;
        total += in_bytes[k];
    }
    static const uint8_t none = 0;
    Handle* h = new Handle;
    h->total = total, h->spacing = sp, h->stream_len = stream_len, h->wrapper = (uint32_t)wrapper, h->mutant = mutant, h->serial = serial;
    h->cut_bytes = cut_bytes;
    h->ents.resize(n);
    ic::ic_make_entries([&](uint64_t k) { return bit_start[k]; }, [&](uint64_t k) { return in_bytes[k]; }, n, 0u, h->ents.data());
    iw::Rec acc = iw::Rec{ic::V_OK, 0, 0, 0, 0, 0, 0, 0, 0};
    if (serial) build_by_mutant<SerialTab>(*h, stream ? stream : &none, in_bytes, group_bytes, acc);
    else build_by_mutant<LaneTab>(*h, stream ? stream : &none, in_bytes, group_bytes, acc);
    uint64_t valid = 0;
    const int r = iw::iw_report(acc, ~0ull, *report, &valid);
    *rc = r == iw::IW_OK ? MI355_OK : MI355_E_DATA;
    if (*rc != MI355_OK) {
        delete h;
        return nullptr;
    }
    return h;
}
extern "C" void inflcut_free(void* h) { delete (Handle*)h; }
// v: total, n_entries, n_points, cut_bytes, cuts, cuts counted beyond their slots
extern "C" void inflcut_info(void* hv, uint64_t v[6]) {
    const Handle& h = *(Handle*)hv;
    v[0] = h.total, v[1] = h.ents.size(), v[2] = h.pts.size(), v[3] = h.cut_bytes, v[4] = h.cuts.size(), v[5] = h.surplus;
}
extern "C" uint64_t inflcut_cuts(void* hv, uint64_t* out, uint64_t cap) {
    const Handle& h = *(Handle*)hv;
    for (size_t i = 0; i < h.cuts.size() && i < cap; i++) out[3 * i] = h.cuts[i].bit, out[3 * i + 1] = h.cuts[i].pos, out[3 * i + 2] = h.cuts[i].hdr_bit;
    return h.cuts.size();
}
// a mutated cut list: cut i of the handle becomes (bit, pos, hdr_bit)
extern "C" int inflcut_set_cut(void* hv, uint64_t i, uint64_t bit, uint64_t pos, uint64_t hdr_bit) {
    Handle& h = *(Handle*)hv;
    if (i >= h.cuts.size()) return MI355_E_ARG;
    h.cuts[i] = icut::Cut{bit, pos, hdr_bit};
    return MI355_OK;
}
// n ranges (off[i], len[i]) into out + out_at[i]; budget: the group budget.  got / reports: n entries; counts: the plan's four;
// cut_counts: mi355_inflate_seek_last_read_cuts' four
extern "C" int inflcut_read(void* hv, const uint8_t* stream, uint64_t stream_len, const uint64_t* off, const uint64_t* len, const uint64_t* out_at,
                            uint64_t n, uint64_t budget, uint8_t* out, uint64_t* got, mi355_inflate_report* reports, uint64_t counts[4],
                            uint64_t cut_counts[4]) {
    Handle& h = *(Handle*)hv;
    if (!got || !reports || !counts || !cut_counts || (n && (!off || !len || !out_at)) || budget < 65536 || stream_len != h.stream_len) return MI355_E_ARG;
    static const uint8_t none = 0;
    const uint8_t* s = stream ? stream : &none;
    std::vector<is::Range> ranges(n);
    for (uint64_t i = 0; i < n; i++) ranges[i] = is::Range{off[i], len[i], len[i] ? out + out_at[i] : nullptr};
    if (h.serial) return read_by_mutant<SerialTab>(h, s, ranges.data(), n, budget, got, reports, counts, cut_counts);
    return read_by_mutant<LaneTab>(h, s, ranges.data(), n, budget, got, reports, counts, cut_counts);
}
extern "C" uint64_t inflcut_bad_loads(void) { return g_bad_loads; }
