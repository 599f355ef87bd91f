// Host build of deflate-rs_amd/csrc/inflate_write.h (TEST INFRASTRUCTURE): the decisions of the inflate kernel with a scalar sink --
// bytes written one at a time -- and with a lanes sink that replays the kernel's writes lane by lane, index arithmetic included.
// The product never links this.
#include <stdint.h>
#include <string.h>

#include "../../deflate-rs_amd/csrc/inflate_write.h"
#include "../../include/mi355_deflate.h"

using namespace mi355;

static_assert(sizeof(mi355_inflate_report) == 56, "mi355_inflate_report is 56 bytes");

namespace {

// loads of the output that the lanes sink found at or beyond the last fence's position, or at or beyond min(p, cap): must stay 0
uint64_t g_unfenced_loads = 0;
uint64_t g_fences = 0;

struct ScalarSink {
    static bool leader() { return true; }
    static void sync() {}
    static uint32_t uni(uint32_t v) { return v; }
    static void fence(uint64_t) {}
    static void store_lits(const uint8_t* lit, uint8_t* out, uint64_t cap, uint64_t lit_p, uint32_t n) {
        for (uint32_t i = 0; i < n && lit_p + i < cap; i++) out[lit_p + i] = lit[i];
    }
    // (the plain serial copy of every inflater: byte i from byte i - dist, overlapping or not)
    static void copy_match(uint8_t* out, uint64_t cap, uint64_t p, uint32_t len, uint32_t dist) {
        for (uint32_t i = 0; i < len && p + i < cap; i++) out[p + i] = out[p + i - dist];
    }
    static void copy_run(const uint8_t* src, uint8_t* out, uint64_t cap, uint64_t p, uint32_t n) {
        for (uint32_t i = 0; i < n && p + i < cap; i++) out[p + i] = src[i];
    }
};

// the kernel's way, a lane at a time.  A step of the wave is all its loads, then all its stores; the loads of a match step must
// lie below the position of the last fence (what the wave stored behind it is not loadable yet).
struct LaneSink : ScalarSink {
    static uint64_t& fenced() {
        static uint64_t v = 0;
        return v;
    }
    static void fence(uint64_t upto) { fenced() = upto, g_fences++; }
    static void store_lits(const uint8_t* lit, uint8_t* out, uint64_t cap, uint64_t lit_p, uint32_t n) {
        for (uint32_t lane = 0; lane < 64; lane++) iw::iw_lane_lits(lit, out, cap, lit_p, n, lane);
    }
    static void copy_match(uint8_t* out, uint64_t cap, uint64_t p, uint32_t len, uint32_t dist) {
        for (uint32_t base = 0; base < 320 && base < len; base += 64) {
            uint8_t v[64];
            bool on[64];
            for (uint32_t lane = 0; lane < 64; lane++) {  // the step's loads
                const uint32_t i = base + lane;
                on[lane] = i < len && p + i < cap;
                if (!on[lane]) continue;
                const uint64_t src = iw::iw_match_src(p, dist, i);
                if (src >= fenced() || src >= p || src >= cap) g_unfenced_loads++;
                v[lane] = src < p && src < cap ? out[src] : 0;
            }
            // the step's stores, by the lane function itself; they must equal what the loads saw
            for (uint32_t lane = 0; lane < 64; lane++) iw::iw_lane_match(out, cap, p, len, dist, base, lane);
            for (uint32_t lane = 0; lane < 64; lane++)
                if (on[lane] && out[p + base + lane] != v[lane]) g_unfenced_loads++;  // (a lane read what this step wrote)
        }
    }
    static void copy_run(const uint8_t* src, uint8_t* out, uint64_t cap, uint64_t p, uint32_t n) {
        const uint32_t head = iw::iw_run_head(out, p, n);
        for (uint32_t lane = 0; lane < 64; lane++) iw::iw_lane_run_head(src, out, cap, p, head, lane);
        for (uint32_t base = 0; base < 65536 && head + base < n; base += 512)
            for (uint32_t lane = 0; lane < 64; lane++) iw::iw_lane_run(src, out, cap, p, n, head, base, lane);
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

}  // namespace

// returns MI355_OK, MI355_E_DATA, MI355_E_OUT_TOO_SMALL or MI355_E_ARG like mi355_inflate
static int inflate_as(bool lanes, const uint8_t* stream, uint64_t stream_len, int wrapper, uint8_t* out, uint64_t out_cap, uint64_t* out_len,
                      mi355_inflate_report* report) {
    if (!report || !out_len || wrapper < 0 || wrapper > 2 || (!stream && stream_len) || (!out && out_cap)) return MI355_E_ARG;
    ic::Tables t;
    memset(&t, 0, sizeof t);
    static const uint8_t none = 0;  // (an address the decoder never reads through)
    const uint8_t* s = stream ? stream : &none;
    iw::Rec rec;
    LaneSink::fenced() = 0;
    if (lanes)
        iw::iw_inflate<LaneSink>(t, s, stream_len, (uint32_t)wrapper, out, out_cap, rec);
    else
        iw::iw_inflate<ScalarSink>(t, s, stream_len, (uint32_t)wrapper, out, out_cap, rec);
    if (iw::iw_judged(rec, (uint32_t)wrapper, out_cap))
        iw::iw_check_trailer(s, stream_len, (uint32_t)wrapper, wrapper == 1 ? adler32(out, rec.out_len) : 0,
                             wrapper == 2 ? crc32(out, rec.out_len) : 0, rec);
    uint64_t valid = 0;
    const int r = iw::iw_report(rec, out_cap, *report, &valid);
    *out_len = r == iw::IW_DATA ? valid : report->out_len;
    return r == iw::IW_OK ? MI355_OK : r == iw::IW_DATA ? MI355_E_DATA : MI355_E_OUT_TOO_SMALL;
}

extern "C" int inflwrite_inflate(const uint8_t* stream, uint64_t stream_len, int wrapper, uint8_t* out, uint64_t out_cap, uint64_t* out_len,
                                 mi355_inflate_report* report) {
    return inflate_as(false, stream, stream_len, wrapper, out, out_cap, out_len, report);
}
// ... with the writes done the kernel's way, lane by lane
extern "C" int inflwrite_inflate_lanes(const uint8_t* stream, uint64_t stream_len, int wrapper, uint8_t* out, uint64_t out_cap,
                                       uint64_t* out_len, mi355_inflate_report* report) {
    return inflate_as(true, stream, stream_len, wrapper, out, out_cap, out_len, report);
}
extern "C" uint64_t inflwrite_unfenced_loads(void) { return g_unfenced_loads; }
extern "C" uint64_t inflwrite_fences(void) { return g_fences; }
extern "C" uint32_t inflwrite_report_size(void) { return (uint32_t)sizeof(mi355_inflate_report); }
extern "C" uint32_t inflwrite_rec_size(void) { return (uint32_t)sizeof(iw::Rec); }
