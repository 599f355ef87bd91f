// Host build of deflate-rs_amd/csrc/inflate_stream.h (TEST INFRASTRUCTURE): the decisions of the stream-inflate kernel with a scalar
// sink and with a lanes sink that replays the kernel's writes lane by lane, and a small model of the handle around them -- pending
// bytes, the history pair, totals, running checksum -- that uses the header's own bookkeeping (is_arm, is_settle, is_judge).  The
// product never links this.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../deflate-rs_amd/csrc/inflate_stream.h"
#include "../../include/mi355_deflate.h"

using namespace mi355;

static_assert(sizeof(mi355_inflate_report) == 56, "mi355_inflate_report is 56 bytes");
static_assert(sizeof(mi355_inflate_stream_state) == 48, "mi355_inflate_stream_state is 48 bytes");
static_assert(sizeof(ist::Resume) == 96 && sizeof(ist::Rec2) == 72, "the kernel's item and record");

namespace {

uint64_t g_unfenced_loads = 0;
// mutants of the model, each caught by a named case (tests/test_inflate_stream_cases.py):
//   1 history not shifted on a short commit   2 seam select off by one   3 commit point advanced inside a partial block
//   4 TRUNCATED treated as final              5 dist checked against the bytes of this write only
int g_mutant = 0;

const uint8_t* src_of(const uint8_t* hist, uint64_t H, const uint8_t* out, uint64_t cap, uint64_t v) {
    if (g_mutant == 2 && H && v == H - 1 && cap) return out;  // (the byte on the wrong side of the seam)
    return ist::is_src(hist, H, out, v);
}

struct ScalarSink {
    static bool leader() { return true; }
    static void sync() {}
    static uint32_t uni(uint32_t v) { return v; }
    static void fence(uint64_t) {}
    static void store_lits(const uint8_t* lit, uint8_t* out, uint64_t cap, uint64_t lit_p, uint32_t n) {
        for (uint32_t i = 0; i < n && lit_p + i < cap; i++) out[lit_p + i] = lit[i];
    }
    static void copy_run(const uint8_t* src, uint8_t* out, uint64_t cap, uint64_t p, uint32_t n) {
        for (uint32_t i = 0; i < n && p + i < cap; i++) out[p + i] = src[i];
    }
    // (the plain serial copy of every inflater over the virtual buffer: byte i from byte i - dist)
    static void copy_match_h(const uint8_t* hist, uint64_t H, uint8_t* out, uint64_t vcap, uint64_t p, uint32_t len, uint32_t dist) {
        for (uint32_t i = 0; i < len && p + i < vcap; i++) out[p + i - H] = *src_of(hist, H, out, vcap - H, p + i - dist);
    }
    static void copy_hist(const uint8_t* hist, uint64_t H, const uint8_t* out, uint8_t* hist_next, uint64_t from, uint32_t n) {
        for (uint32_t j = 0; j < n; j++) hist_next[j] = *ist::is_src(hist, H, out, from + j);
    }
};

// the kernel's way, a lane at a time: a step of the wave is all its loads, then all its stores; the loads of out in a match step
// must lie below the position of the last fence (the history was fenced by the launch that wrote it)
struct LaneSink : ScalarSink {
    static uint64_t& fenced() {
        static uint64_t v = 0;
        return v;
    }
    static void fence(uint64_t upto) { fenced() = upto; }
    static void store_lits(const uint8_t* lit, uint8_t* out, uint64_t cap, uint64_t lit_p, uint32_t n) {
        for (uint32_t lane = 0; lane < 64; lane++) iw::iw_lane_lits(lit, out, cap, lit_p, n, lane);
    }
    static void copy_run(const uint8_t* src, uint8_t* out, uint64_t cap, uint64_t p, uint32_t n) {
        const uint32_t head = iw::iw_run_head(out, p, n);
        for (uint32_t lane = 0; lane < 64; lane++) iw::iw_lane_run_head(src, out, cap, p, head, lane);
        for (uint32_t base = 0; base < 65536 && head + base < n; base += 512)
            for (uint32_t lane = 0; lane < 64; lane++) iw::iw_lane_run(src, out, cap, p, n, head, base, lane);
    }
    static void copy_match_h(const uint8_t* hist, uint64_t H, uint8_t* out, uint64_t vcap, uint64_t p, uint32_t len, uint32_t dist) {
        for (uint32_t base = 0; base < 320 && base < len; base += 64) {
            uint8_t v[64];
            bool on[64];
            for (uint32_t lane = 0; lane < 64; lane++) {  // the step's loads
                const uint32_t i = base + lane;
                on[lane] = i < len && p + i < vcap;
                if (!on[lane]) continue;
                const uint64_t src = iw::iw_match_src(p, dist, i);
                if (src >= H && (src >= fenced() || src >= p || src >= vcap)) g_unfenced_loads++;
                v[lane] = src < p && src < vcap ? *src_of(hist, H, out, vcap - H, src) : 0;
            }
            if (g_mutant == 2) {
                for (uint32_t lane = 0; lane < 64; lane++)
                    if (on[lane]) out[p + base + lane - H] = v[lane];
                continue;
            }
            // the step's stores, by the lane function itself; they must equal what the loads saw
            for (uint32_t lane = 0; lane < 64; lane++) ist::is_lane_match(hist, H, out, vcap, p, len, dist, base, lane);
            for (uint32_t lane = 0; lane < 64; lane++)
                if (on[lane] && out[p + base + lane - H] != v[lane]) g_unfenced_loads++;  // (a lane read what this step wrote)
        }
    }
    static void copy_hist(const uint8_t* hist, uint64_t H, const uint8_t* out, uint8_t* hist_next, uint64_t from, uint32_t n) {
        if (n && from + n > H && from + n > fenced()) g_unfenced_loads++;  // (the copy loads out up to the commit point)
        for (uint32_t base = 0; base < ist::HIST && base < n; base += 512)
            for (uint32_t lane = 0; lane < 64; lane++) ist::is_lane_hist(hist, H, out, hist_next, from, n, base, lane);
    }
};

uint32_t adler32_more(uint32_t adler, const uint8_t* d, uint64_t n) {
    uint32_t a = adler & 0xffff, b = adler >> 16;
    for (uint64_t i = 0; i < n; i++) {
        a = (a + d[i]) % 65521u;
        b = (b + a) % 65521u;
    }
    return b << 16 | a;
}
uint32_t crc32_more(uint32_t crc, const uint8_t* d, uint64_t n) {
    uint32_t c = ~crc;
    for (uint64_t i = 0; i < n; i++) {
        c ^= d[i];
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1u) ? 0xEDB88320u : 0u);
    }
    return ~c;
}

// exact-size heap allocations throughout, so that the sanitizer build sees a read or a store one byte outside any of them
struct Model {
    ist::HState h;
    bool lanes;
    uint8_t* pending = nullptr;  // exactly h.end bytes, h.front == 0 after every write (the model compacts always)
    uint8_t* hist[2] = {nullptr, nullptr};
    uint8_t* dict = nullptr;
};

void model_start(Model* m) {
    const uint32_t nd = m->h.n_dict, w = m->h.wrapper;
    ist::is_hstate_init(m->h, w, nd);
    free(m->pending);
    m->pending = nullptr;
    if (nd) memcpy(m->hist[0], m->dict, nd);
}

int rc_of(int r) { return r == iw::IW_OK ? MI355_OK : r == iw::IW_DATA ? MI355_E_DATA : MI355_E_OUT_TOO_SMALL; }

void run(Model* m, const ist::Resume& q, ist::Rec2& rec) {
    ic::Tables t;
    memset(&t, 0, sizeof t);
    LaneSink::fenced() = q.hist_len;
    if (m->lanes)
        ist::is_resume<LaneSink>(t, q, rec);
    else
        ist::is_resume<ScalarSink>(t, q, rec);
}

int model_write(Model* m, const uint8_t* in, uint64_t in_len, uint8_t* out, uint64_t cap, uint64_t* out_len, mi355_inflate_report* rep,
                bool fin) {
    ist::HState& h = m->h;
    *out_len = 0;
    if (h.failed) return MI355_E_STATE;
    if (h.done) return rc_of(ist::is_after_done(h, in_len, *rep));
    // append, compacted: the live part and the new bytes in one exact allocation
    const uint64_t live = h.end - h.front;
    uint8_t* np = (uint8_t*)malloc(live + in_len ? live + in_len : 1);
    if (live) memcpy(np, m->pending + h.front, live);
    if (in_len) memcpy(np + live, in, in_len);
    free(m->pending);
    m->pending = np, h.front = 0, h.end = live + in_len, h.total_in += in_len;
    ist::Resume q = ist::is_arm(h, m->pending, m->hist[0], m->hist[1], out, cap, fin);
    if (g_mutant == 5) q.hist_len = 0;
    ist::Rec2 rec;
    run(m, q, rec);
    if (g_mutant == 3 && rec.state == ist::S_PENDING && !(h.frame_open && rec.frame != ist::FP_OK))
        rec.commit_bit = 8 * (q.nbytes - rec.hdr_len);  // (everything fed counts as used)
    if (g_mutant == 4 && rec.state == ist::S_PENDING && rec.commit_bit < 8 * (q.nbytes - rec.hdr_len))
        rec.state = ist::S_FAILED, rec.status = ic::V_TRUNCATED, rec.bit = q.bit_base + rec.commit_bit, rec.out_pos = q.out_base + rec.committed;
    const uint32_t cur = h.hist_cur, old_len = h.hist_len;
    uint64_t got = 0;
    int r = ist::is_settle(h, q, rec, *rep, &got);
    if (g_mutant == 1 && rec.state != ist::S_FAILED && rec.committed && rec.committed < ist::HIST) h.hist_cur = cur, h.hist_len = old_len;
    if (got && h.wrapper == 1) h.sum = adler32_more(h.sum, out, got);
    if (got && h.wrapper == 2) h.sum = crc32_more(h.sum, out, got);
    if (r != iw::IW_DATA && h.done && h.wrapper) r = ist::is_judge(h, rec, *rep);
    *out_len = got;
    return rc_of(r);
}

}  // namespace

extern "C" {

void* ism_new(int wrapper, const uint8_t* dict, uint64_t dict_len, int lanes) {
    if (wrapper < 0 || wrapper > 2 || (!dict && dict_len) || (dict_len && wrapper)) return nullptr;
    Model* m = new Model();
    m->lanes = lanes != 0;
    m->hist[0] = (uint8_t*)malloc(ist::HIST), m->hist[1] = (uint8_t*)malloc(ist::HIST);
    const uint64_t nd = dict_len < ist::HIST ? dict_len : ist::HIST;
    m->dict = (uint8_t*)malloc(nd ? nd : 1);
    if (nd) memcpy(m->dict, dict + dict_len - nd, nd);
    m->h.n_dict = (uint32_t)nd, m->h.wrapper = (uint32_t)wrapper;
    model_start(m);
    return m;
}
int ism_write(void* p, const uint8_t* in, uint64_t in_len, uint8_t* out, uint64_t cap, uint64_t* out_len, mi355_inflate_report* rep) {
    if (!p || !rep || !out_len || (!in && in_len) || (!out && cap)) return MI355_E_ARG;
    return model_write((Model*)p, in, in_len, out, cap, out_len, rep, false);
}
int ism_finish(void* p, mi355_inflate_report* rep) {
    if (!p || !rep) return MI355_E_ARG;
    Model* m = (Model*)p;
    if (m->h.failed) return MI355_E_STATE;
    if (m->h.done) return rc_of(ist::is_after_done(m->h, 0, *rep));
    uint64_t got = 0;
    return model_write(m, nullptr, 0, nullptr, 0, &got, rep, true);
}
void ism_state(void* p, mi355_inflate_stream_state* st) {
    const ist::HState& h = ((Model*)p)->h;
    *st = mi355_inflate_stream_state{h.total_in, h.total_out, h.end - h.front, h.need_out, h.done, h.failed, h.wrapper ? h.sum : 0, 0};
}
void ism_reset(void* p) { model_start((Model*)p); }
void ism_free(void* p) {
    Model* m = (Model*)p;
    if (!m) return;
    free(m->pending), free(m->hist[0]), free(m->hist[1]), free(m->dict);
    delete m;
}
void ism_set_mutant(int k) { g_mutant = k; }
uint64_t ism_unfenced_loads(void) { return g_unfenced_loads; }
uint32_t ism_frame_prefix(const uint8_t* s, uint64_t n, int wrapper, uint64_t* hdr_len) {
    return ist::is_frame_prefix(s, n, (uint32_t)wrapper, *hdr_len);
}
// The block ends of a stream, from the decoder's own records: for every prefix s[0, k) a fresh resume with room for all of the
// output, whose commit point is the end of the last complete block (of the BFINAL block: once its trailer is there).  Whenever the
// blocks in front of the commit point have become more, (k, the bytes in front of it) goes to ends.  Returns how many pairs there
// are (at most cap are written).
uint64_t ism_block_ends(const uint8_t* s, uint64_t n, int wrapper, const uint8_t* dict, uint64_t dict_len, uint64_t out_total, uint64_t* ends,
                        uint64_t cap) {
    uint64_t n_ends = 0, blocks = 0;
    Model* m = (Model*)ism_new(wrapper, dict, dict_len, 0);
    if (!m) return 0;
    uint8_t* out = (uint8_t*)malloc(out_total ? out_total : 1);
    for (uint64_t k = 1; k <= n; k++) {
        uint8_t* piece = (uint8_t*)malloc(k);
        memcpy(piece, s, k);
        ist::HState h = m->h;
        h.end = k;
        const ist::Resume q = ist::is_arm(h, piece, m->hist[0], m->hist[1], out, out_total, false);
        ist::Rec2 rec;
        run(m, q, rec);
        free(piece);
        if (rec.state == ist::S_FAILED) break;
        if (rec.n_blocks > blocks) {
            if (n_ends < cap) ends[2 * n_ends] = k, ends[2 * n_ends + 1] = rec.committed;
            n_ends++, blocks = rec.n_blocks;
        }
    }
    free(out);
    ism_free(m);
    return n_ends;
}

}  // extern "C"
