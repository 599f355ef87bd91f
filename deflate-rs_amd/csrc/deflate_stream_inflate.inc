// Streaming inflate (include/mi355_deflate.h mi355_inflate_stream_*): decode a stream as it arrives, piece by piece.  k_inflate_resume
// runs inflate_stream.h as one wave per handle -- k_inflate's scalar chain, started at the handle's commit point with its history in
// front of the output, and at its end the wave leaves the next history -- and tests/inflstream/ builds the same text for the host.
// The handle's bookkeeping between launches is the header's too (is_arm, is_settle, is_judge); what is here is its buffers, the one
// driver behind every entry (stream_run: append, one launch for all handles, the records, the checksum kernels of the encode over
// the bytes handed over, folded on the host) and the entries.  DESIGN.md section 20.
#include "inflate_stream.h"

namespace mi355 {

// WaveSink with the history select, and the next history
struct StreamSink : WaveSink {
    static __host__ __device__ void copy_match_h(const uint8_t* hist, uint64_t hist_len, uint8_t* out, uint64_t vcap, uint64_t p, uint32_t len,
                                                 uint32_t dist) {
        for (uint32_t base = 0; base < 320 && base < len; base += 64) ist::is_lane_match(hist, hist_len, out, vcap, p, len, dist, base, lane());
    }
    static __host__ __device__ void copy_hist(const uint8_t* hist, uint64_t hist_len, const uint8_t* out, uint8_t* hist_next, uint64_t from,
                                              uint32_t n) {
        for (uint32_t base = 0; base < ist::HIST && base < n; base += 512) ist::is_lane_hist(hist, hist_len, out, hist_next, from, n, base, lane());
    }
};

using RItem = ist::Resume;

// one workgroup of one wave per handle: from its commit point through every block that is complete, its record, its next history
__global__ __launch_bounds__(64) void k_inflate_resume(const RItem* __restrict__ items, ist::Rec2* __restrict__ recs) {
    __shared__ ic::Tables s_t;
    const RItem q = items[blockIdx.x];
    if (q.skip) return;
    ist::Rec2 r;
    ist::is_resume<StreamSink>(s_t, q, r);
    if (threadIdx.x == 0) recs[blockIdx.x] = r;
}

}  // namespace mi355

struct mi355_inflate_stream {
    mi355_deflate_ctx* c = nullptr;
    ist::HState h{};
    uint8_t* pend = nullptr;  // the pending compressed bytes: live in [h.front, h.end)
    size_t pend_cap = 0;
    uint8_t* hist = nullptr;  // the pair: 2 x 32 KiB
    std::vector<uint8_t> dict;  // the last 32 KiB of the preset dictionary (reset)
};

namespace {

static_assert(sizeof(RItem) == 96 && sizeof(ist::Rec2) == 72, "what k_inflate_resume reads and writes");
static_assert(sizeof(mi355_inflate_stream_state) == 48, "mi355_inflate_stream_state is 48 bytes");
constexpr size_t PEND_MIN = 4096;

// a new stream in the handle: the state, the dictionary as the first history
int stream_start(mi355_inflate_stream* s, hipStream_t st) {
    ist::is_hstate_init(s->h, s->h.wrapper, (uint32_t)s->dict.size());
    if (!s->dict.empty()) {
        HIPCHK(s->c, hipMemcpyAsync(s->hist, s->dict.data(), s->dict.size(), hipMemcpyHostToDevice, st));
        HIPCHK(s->c, hipStreamSynchronize(st));
    }
    return MI355_OK;
}

// n more bytes behind the live part, on st: compacted when the consumed front exceeds the live part (the two do not overlap then),
// grown geometrically.  counted: they are new input (not what a write that decoded from the caller's buffer keeps of it)
int stream_append(mi355_inflate_stream* s, const void* in, size_t n, bool in_on_device, hipStream_t st, bool counted = true) {
    mi355_deflate_ctx* c = s->c;
    ist::HState& h = s->h;
    const uint64_t live = h.end - h.front;
    if (live + n > VERIFY_MAX_IN) return MI355_E_UNSUPPORTED;
    if (h.front && h.front >= live) {
        if (live) HIPCHK(c, hipMemcpyAsync(s->pend, s->pend + h.front, live, hipMemcpyDeviceToDevice, st));
        h.front = 0, h.end = live;
    }
    if (h.end + n > s->pend_cap) {
        size_t want = s->pend_cap * 2 > PEND_MIN ? s->pend_cap * 2 : PEND_MIN;
        while (want < live + n) want *= 2;
        uint8_t* np = nullptr;
        HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&np), want));
        if (live) HIPCHK(c, hipMemcpyAsync(np, s->pend + h.front, live, hipMemcpyDeviceToDevice, st));
        HIPCHK(c, hipStreamSynchronize(st));
        if (s->pend) (void)hipFree(s->pend);
        s->pend = np, s->pend_cap = want, h.front = 0, h.end = live;
    }
    if (n) HIPCHK(c, hipMemcpyAsync(s->pend + h.end, in, n, in_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    h.end += n, h.total_in += counted ? n : 0;
    return MI355_OK;
}

struct StreamJob {
    mi355_inflate_stream* s;
    const void* in;
    size_t in_len;
    uint8_t* out;  // device
    size_t cap;
    // written
    bool direct;  // decoded from `in` where it lies: the handle held no pending byte (see stream_run)
    int rc;
    uint64_t got;
    mi355_inflate_report rep;
};

void stream_say(mi355_deflate_ctx* c, const StreamJob& j, const char* what) {
    char buf[200];
    if (j.rc == MI355_E_DATA)
        snprintf(buf, sizeof buf, "%s: %s at bit %llu, output byte %llu", what, ic::ic_status_name(j.rep.status), (unsigned long long)j.rep.bit,
                 (unsigned long long)j.rep.out_pos);
    else if (j.rc == MI355_E_OUT_TOO_SMALL)
        snprintf(buf, sizeof buf, "%s: the next block needs room for %llu bytes", what, (unsigned long long)j.s->h.need_out);
    else if (j.rc == MI355_E_STATE)
        snprintf(buf, sizeof buf, "%s: the handle is dead (reset revives it)", what);
    else
        return;
    c->err = buf;
}

// The driver behind every entry: the k jobs' input appended (in_on_device: where it lies) -- or, for a handle that holds no pending
// byte and whose chunk is in device memory, decoded where it lies, and only what the write leaves uncommitted of it is kept: a
// connection whose messages end on a flush never copies its input --, one k_inflate_resume launch for all that have something to
// decode, the records back, the wait; then, for the framed handles that handed bytes over, the batch's checksum
// launches over those bytes -- one pass per wrapper in use --, the sums back, a second wait, and the fold.  `fin`: _finish.  Every
// job gets its rc, got and report; the return value is a hard error of the call, or MI355_OK.
int stream_run(mi355_deflate_ctx* c, StreamJob* jobs, size_t k, bool in_on_device, bool fin, hipStream_t st) {
    const auto t0 = std::chrono::steady_clock::now();
    bool framed = false;
    for (size_t j = 0; j < k; j++) framed = framed || jobs[j].s->h.wrapper != 0;
    const BatchSums plan(sizeof(RItem) * k, k, framed, sizeof(ist::Rec2));
    if (const int rc = verify_room(c, plan.bytes)) return rc;
    RItem* hit = reinterpret_cast<RItem*>(c->v_host);
    size_t n_run = 0;
    for (size_t j = 0; j < k; j++) {
        StreamJob& b = jobs[j];
        ist::HState& h = b.s->h;
        b.got = 0, b.rc = MI355_OK, b.direct = false;
        memset(&b.rep, 0, sizeof b.rep);
        memset(&hit[j], 0, sizeof hit[j]);
        hit[j].skip = 1;
        if (h.failed) {
            b.rc = MI355_E_STATE;
            continue;
        }
        if (h.done) {
            b.rc = inflate_rc(ist::is_after_done(h, fin ? 0 : b.in_len, b.rep));
            continue;
        }
        b.direct = in_on_device && h.end == h.front && b.in_len && b.in_len <= VERIFY_MAX_IN;
        if (b.direct)
            h.front = 0, h.end = b.in_len, h.total_in += b.in_len;
        else
            b.rc = stream_append(b.s, b.in, b.in_len, in_on_device, st);
        if (b.rc == MI355_E_HIP) return b.rc;
        if (b.rc) continue;
        b.rep.out_pos = h.total_out;
        if (h.end == h.front && !fin) continue;  // nothing to decode: MI355_OK, no bytes
        hit[j] = ist::is_arm(h, b.direct ? reinterpret_cast<const uint8_t*>(b.in) : b.s->pend, b.s->hist, b.s->hist + ist::HIST, b.out, b.cap, fin);
        n_run++;
    }
    if (!n_run) return MI355_OK;
    const ist::Rec2* recs = reinterpret_cast<const ist::Rec2*>(c->v_host + plan.rec_at);
    HIPCHK(c, hipMemcpyAsync(c->v_dev, c->v_host, sizeof(RItem) * k, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_inflate_resume, dim3((uint32_t)k), dim3(64), 0, st, reinterpret_cast<const RItem*>(c->v_dev),
                       reinterpret_cast<ist::Rec2*>(c->v_dev + plan.rec_at));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->v_host + plan.rec_at, c->v_dev + plan.rec_at, sizeof(ist::Rec2) * k, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    bool sums[3] = {false, false, false}, kept = false;
    for (size_t j = 0; j < k; j++) {
        if (hit[j].skip) continue;
        StreamJob& b = jobs[j];
        ist::HState& h = b.s->h;
        b.rc = inflate_rc(ist::is_settle(h, hit[j], recs[j], b.rep, &b.got));
        if (b.direct) {  // what the write left uncommitted of the caller's chunk becomes the pending bytes
            const uint64_t from = h.front, left = h.end - h.front;
            h.front = h.end = 0;
            if (left) {
                const int rc = stream_append(b.s, reinterpret_cast<const uint8_t*>(b.in) + from, left, true, st, false);
                if (rc) return rc;
                kept = true;
            }
        }
        if (b.got > VERIFY_MAX_IN) return MI355_E_UNSUPPORTED;  // (what the checksum kernels take)
        if (b.got) sums[h.wrapper] = true;
    }
    if (kept && !sums[1] && !sums[2]) HIPCHK(c, hipStreamSynchronize(st));  // (the caller's buffer is its own again when the call returns)
    // the second half of a framed write: the sums of out[0, got), folded into the handle's running checksum
    for (int w = 1; w <= 2; w++) {
        if (!sums[w]) continue;
        const auto mine = [&](size_t j) { return !hit[j].skip && jobs[j].s->h.wrapper == (uint32_t)w && jobs[j].got; };
        const int rc = plan.fill(c, [&](size_t j, const uint8_t** p, uint64_t* len) { *p = jobs[j].out, *len = mine(j) ? jobs[j].got : 0; });
        if (rc) return rc;
        HIPCHK(c, hipMemcpyAsync(c->v_dev + plan.bat_at, c->v_host + plan.bat_at, plan.st_at - plan.bat_at, hipMemcpyHostToDevice, st));
        if (const int rc2 = plan.launch(c, w, st)) return rc2;
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(c->v_host + plan.st_at, c->v_dev + plan.st_at, sizeof(DevState) * k, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        const DevState* hs = reinterpret_cast<const DevState*>(c->v_host + plan.st_at);
        for (size_t j = 0; j < k; j++) {
            if (!mine(j)) continue;
            const DevScalars& sc = hs[j].sc;
            const uint64_t a = (1 + sc.adler_a) % 65521u, bb = (jobs[j].got + sc.adler_b) % 65521u;  // (k_adler_fold's arithmetic)
            const uint32_t piece = w == 1 ? (uint32_t)((bb << 16) | a) : sc.crc;
            jobs[j].s->h.sum = mi355_checksum_combine(w, jobs[j].s->h.sum, piece, jobs[j].got);
        }
    }
    const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (size_t j = 0; j < k; j++) {
        if (hit[j].skip) continue;
        StreamJob& b = jobs[j];
        if (b.rc != MI355_E_DATA && b.s->h.done && b.s->h.wrapper) b.rc = inflate_rc(ist::is_judge(b.s->h, recs[j], b.rep));
        b.rep.ms = ms;
    }
    return MI355_OK;
}

bool stream_args_bad(const mi355_inflate_stream* s, const void* in, size_t in_len, const void* out, size_t out_cap, const size_t* out_len,
                     const mi355_inflate_report* report) {
    return !s || !report || !out_len || (!in && in_len) || (!out && out_cap);
}

// one handle, one job, its output already in device memory
int stream_one(mi355_inflate_stream* s, const void* in, size_t in_len, bool in_on_device, uint8_t* d_out, size_t out_cap, size_t* out_len,
               mi355_inflate_report* report, bool fin, hipStream_t st, const char* what) {
    StreamJob job{s, in, in_len, d_out, out_cap, false, MI355_OK, 0, {}};
    const int rc = stream_run(s->c, &job, 1, in_on_device, fin, st);
    if (rc) return rc;
    *report = job.rep;
    if (out_len) *out_len = (size_t)job.got;
    stream_say(s->c, job, what);
    return job.rc;
}

}  // namespace

extern "C" {

int mi355_inflate_stream_new(mi355_deflate_ctx* c, int wrapper, const uint8_t* dict, size_t dict_len, mi355_inflate_stream** out) {
    if (!out || wrapper < 0 || wrapper > 2 || (!dict && dict_len) || (dict_len && wrapper)) return MI355_E_ARG;
    *out = nullptr;
    DefaultGuard dg_;
    if (const int rc = decode_enter(c, dg_)) return rc;
    std::unique_ptr<mi355_inflate_stream> s(new mi355_inflate_stream());
    s->c = c;
    s->h.wrapper = (uint32_t)wrapper;
    const size_t nd = dict_len < ist::HIST ? dict_len : ist::HIST;
    if (nd) s->dict.assign(dict + dict_len - nd, dict + dict_len);
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&s->hist), 2 * ist::HIST));
    const int rc = stream_start(s.get(), c->own_stream);
    if (rc) {
        (void)hipFree(s->hist);
        return rc;
    }
    *out = s.release();
    return MI355_OK;
}

void mi355_inflate_stream_free(mi355_inflate_stream* s) {
    if (!s) return;
    DefaultGuard dg_;
    (void)use_ctx(s->c, dg_);
    (void)hipSetDevice(s->c->device);
    if (s->pend) (void)hipFree(s->pend);
    if (s->hist) (void)hipFree(s->hist);
    delete s;
}

int mi355_inflate_stream_reset(mi355_inflate_stream* s) {
    if (!s) return MI355_E_ARG;
    DefaultGuard dg_;
    mi355_deflate_ctx* c = s->c;
    if (const int rc = decode_enter(c, dg_)) return rc;
    return stream_start(s, c->own_stream);
}

int mi355_inflate_stream_state_get(mi355_inflate_stream* s, mi355_inflate_stream_state* state) {
    if (!s || !state) return MI355_E_ARG;
    const ist::HState& h = s->h;
    *state = mi355_inflate_stream_state{h.total_in, h.total_out, h.end - h.front, h.need_out, h.done, h.failed, h.wrapper ? h.sum : 0u, 0u};
    return MI355_OK;
}

int mi355_inflate_stream_write_device(mi355_inflate_stream* s, const void* d_in, size_t in_len, void* d_out, size_t out_cap, size_t* out_len,
                                      mi355_inflate_report* report, void* hip_stream) {
    if (stream_args_bad(s, d_in, in_len, d_out, out_cap, out_len, report)) return MI355_E_ARG;
    *out_len = 0;
    DefaultGuard dg_;
    mi355_deflate_ctx* c = s->c;
    if (const int rc = decode_enter(c, dg_)) return rc;
    return stream_one(s, d_in, in_len, true, reinterpret_cast<uint8_t*>(d_out), out_cap, out_len, report, false, call_stream(c, hip_stream),
                      "inflate stream");
}

// host buffers: the chunk goes straight behind the handle's pending bytes, the bytes handed over come back from the context's staging
int mi355_inflate_stream_write(mi355_inflate_stream* s, const uint8_t* in, size_t in_len, uint8_t* out, size_t out_cap, size_t* out_len,
                               mi355_inflate_report* report) {
    if (stream_args_bad(s, in, in_len, out, out_cap, out_len, report)) return MI355_E_ARG;
    *out_len = 0;
    DefaultGuard dg_;
    mi355_deflate_ctx* c = s->c;
    if (const int rc = decode_enter(c, dg_)) return rc;
    if (const int rc = ensure_buf(c, &c->d_out, &c->d_out_cap, out_cap + 64)) return rc;
    const int rc = stream_one(s, in, in_len, false, out_cap ? c->d_out : nullptr, out_cap, out_len, report, false, c->own_stream, "inflate stream");
    return stage_out(c, rc, out, *out_len);
}

int mi355_inflate_stream_finish(mi355_inflate_stream* s, mi355_inflate_report* report) {
    if (!s || !report) return MI355_E_ARG;
    DefaultGuard dg_;
    mi355_deflate_ctx* c = s->c;
    if (const int rc = decode_enter(c, dg_)) return rc;
    return stream_one(s, nullptr, 0, true, nullptr, 0, nullptr, report, true, c->own_stream, "inflate stream finish");
}

int mi355_inflate_stream_write_batch_device(mi355_deflate_ctx* c, mi355_inflate_stream* const* s, mi355_batch_item* items, size_t n,
                                            mi355_inflate_report* reports, void* hip_stream) {
    if ((!s && n) || (!items && n) || n > 0x7fffffffull) return MI355_E_ARG;
    for (size_t i = 0; i < n; i++) {
        if (!s[i]) return MI355_E_ARG;
        if (items[i].status != MI355_OK) continue;
        if ((!items[i].in && items[i].in_len) || (!items[i].out && items[i].out_cap)) return MI355_E_ARG;
    }
    {
        std::vector<const mi355_inflate_stream*> seen(s, s + n);
        std::sort(seen.begin(), seen.end());
        if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return MI355_E_ARG;
    }
    DefaultGuard dg_;
    if (const int rc = decode_enter(c, dg_)) return rc;
    for (size_t i = 0; i < n; i++)
        if (s[i]->c != c) return MI355_E_ARG;
    std::vector<StreamJob> jobs;
    std::vector<uint32_t> act;
    for (size_t i = 0; i < n; i++) {
        if (items[i].status != MI355_OK) continue;  // skipped, left alone
        jobs.push_back(StreamJob{s[i], items[i].in, items[i].in_len, reinterpret_cast<uint8_t*>(items[i].out), items[i].out_cap, false, MI355_OK, 0, {}});
        act.push_back((uint32_t)i);
    }
    if (jobs.empty()) return MI355_OK;
    if (const int rc = stream_run(c, jobs.data(), jobs.size(), true, false, call_stream(c, hip_stream))) return rc;
    int first = MI355_OK;
    for (size_t j = 0; j < jobs.size(); j++) {
        mi355_batch_item& b = items[act[j]];
        b.out_len = (size_t)jobs[j].got, b.status = jobs[j].rc;
        if (reports) reports[act[j]] = jobs[j].rep;
        if (jobs[j].rc != MI355_OK && first == MI355_OK) {
            first = jobs[j].rc;
            char what[48];
            snprintf(what, sizeof what, "inflate stream: item %u", act[j]);
            stream_say(c, jobs[j], what);
        }
    }
    return first;
}

}  // extern "C"
