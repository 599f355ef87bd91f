// Host build of deflate-rs_amd/csrc/inflate_check.h (TEST INFRASTRUCTURE): the decisions of the verify kernel with a scalar loop
// around them -- bytes compared one at a time where the kernel compares 64, entries one after the other where the kernel runs a
// wave each.  The product never links this.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../deflate-rs_amd/csrc/inflate_check.h"
#include "../../include/mi355_deflate.h"

using namespace mi355;

namespace {

struct HostOps {
    static bool leader() { return true; }
    static void sync() {}
    static uint32_t uni(uint32_t v) { return v; }
    static uint32_t first_diff_lits(const uint8_t* lit, const uint8_t* in, uint32_t n) {
        for (uint32_t i = 0; i < n; i++)
            if (lit[i] != in[i]) return i;
        return n;
    }
    static uint32_t first_diff_match(const uint8_t* in, uint64_t p, uint32_t len, uint32_t dist) {
        for (uint32_t i = 0; i < len; i++)
            if (in[p + i] != in[p + i - dist]) return i;
        return len;
    }
    static uint64_t first_diff_run(const uint8_t* a, const uint8_t* b, uint64_t n) {
        for (uint64_t i = 0; i < n; i++)
            if (a[i] != b[i]) return i;
        return n;
    }
};

// the kernel's way of comparing, a lane at a time: the arithmetic of ic_lane_* under the reduction the wave does with a ballot
struct LaneOps : HostOps {
    static uint32_t first_of(const uint32_t* mine, uint32_t none) {
        for (uint32_t lane = 0; lane < 64; lane++)
            if (mine[lane] != ic::NONE) return mine[lane];
        return none;
    }
    static uint32_t first_diff_lits(const uint8_t* lit, const uint8_t* in, uint32_t n) {
        uint32_t v[64];
        for (uint32_t lane = 0; lane < 64; lane++) v[lane] = ic::ic_lane_lits(lit, in, n, lane);
        return first_of(v, n);
    }
    static uint32_t first_diff_match(const uint8_t* in, uint64_t p, uint32_t len, uint32_t dist) {
        for (uint32_t base = 0; base < 320 && base < len; base += 64) {
            uint32_t v[64];
            for (uint32_t lane = 0; lane < 64; lane++) v[lane] = ic::ic_lane_match(in, p, len, dist, base, lane);
            const uint32_t d = first_of(v, ic::NONE);
            if (d != ic::NONE) return d;
        }
        return len;
    }
    static uint64_t first_diff_run(const uint8_t* a, const uint8_t* b, uint64_t n) {
        const uint32_t n32 = (uint32_t)(n < 65535 ? n : 65535);
        for (uint32_t base = 0; base < 65536 && base < n32; base += 512) {
            uint32_t v[64];
            for (uint32_t lane = 0; lane < 64; lane++) v[lane] = ic::ic_lane_run(a, b, n32, base, lane);
            const uint32_t d = first_of(v, ic::NONE);
            if (d != ic::NONE) return d;
        }
        return n;
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

// returns MI355_OK, MI355_E_VERIFY or MI355_E_ARG like mi355_deflate_verify; n == 0: no table
static int verify_as(bool lanes, const uint8_t* stream, uint64_t stream_len, const uint8_t* in, uint64_t in_len, int wrapper,
                     const uint64_t* bit_start, const uint64_t* in_bytes, uint64_t n, mi355_verify_report* report) {
    if (!report || wrapper < 0 || wrapper > 2 || (!stream && stream_len) || (!in && in_len)) return MI355_E_ARG;
    uint64_t sum = 0;
    for (uint64_t k = 0; k < n; k++) {
        if (k && bit_start[k] < bit_start[k - 1]) return MI355_E_ARG;
        if (in_bytes[k] > in_len - sum) return MI355_E_ARG;
        sum += in_bytes[k];
    }
    if (n && sum != in_len) return MI355_E_ARG;
    const uint64_t ne = n ? n : 1;
    std::vector<ic::Entry> ents(ne);
    std::vector<ic::Rec> recs(ne);
    ic::ic_make_entries([&](uint64_t k) { return bit_start[k]; }, [&](uint64_t k) { return in_bytes[k]; }, n, 0u, ents.data());
    const uint32_t adler = wrapper == 1 ? adler32(in, in_len) : 0, crc = wrapper == 2 ? crc32(in, in_len) : 0;
    ic::Tables t;
    memset(&t, 0, sizeof t);
    // (an empty vector's data() may be null: give the decoder an address it never reads through)
    static const uint8_t none = 0;
    for (uint64_t k = 0; k < ne; k++) {
        if (lanes)
            ic::ic_verify_entry<LaneOps>(t, stream ? stream : &none, stream_len, in ? in : &none, in_len, (uint32_t)wrapper, adler, crc,
                                         ents[k], recs[k]);
        else
            ic::ic_verify_entry<HostOps>(t, stream ? stream : &none, stream_len, in ? in : &none, in_len, (uint32_t)wrapper, adler, crc,
                                         ents[k], recs[k]);
    }
    ic::ic_report(recs.data(), ne, *report);
    report->ms = 0;
    return report->status == MI355_VERIFY_OK ? MI355_OK : MI355_E_VERIFY;
}

extern "C" int inflcheck_verify(const uint8_t* stream, uint64_t stream_len, const uint8_t* in, uint64_t in_len, int wrapper,
                                const uint64_t* bit_start, const uint64_t* in_bytes, uint64_t n, mi355_verify_report* report) {
    return verify_as(false, stream, stream_len, in, in_len, wrapper, bit_start, in_bytes, n, report);
}
// ... with the compares done the kernel's way, lane by lane
extern "C" int inflcheck_verify_lanes(const uint8_t* stream, uint64_t stream_len, const uint8_t* in, uint64_t in_len, int wrapper,
                                      const uint64_t* bit_start, const uint64_t* in_bytes, uint64_t n, mi355_verify_report* report) {
    return verify_as(true, stream, stream_len, in, in_len, wrapper, bit_start, in_bytes, n, report);
}

// ic_match_token alone, under a distance set built from 32 code lengths: w holds the token's bits from the length symbol's code on,
// `used` the bits of that code.  out: status, len, dist, used (len / dist / used mean something where the status is OK)
extern "C" void inflcheck_match_token(const uint8_t* dist_lens32, uint64_t w, uint32_t s, uint32_t used, uint64_t avail, uint64_t p,
                                      uint32_t out[4]) {
    ic::Tables t;
    memset(&t, 0, sizeof t);
    (void)ic::ic_build(t, dist_lens32, 32, t.prim_d, ic::D_BITS, t.sym_d, 31, t.cnt_d);
    uint32_t len = 0, dist = 0;
    const ic::Fail f = ic::ic_match_token<HostOps>(t, w, s, used, avail, 0, p, len, dist);
    out[0] = f.status, out[1] = len, out[2] = dist, out[3] = used;
}

extern "C" uint32_t inflcheck_report_size(void) { return (uint32_t)sizeof(mi355_verify_report); }
extern "C" uint32_t inflcheck_tables_size(void) { return (uint32_t)sizeof(ic::Tables); }
