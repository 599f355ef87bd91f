// Inflate (include/mi355_deflate.h mi355_inflate[_device], mi355_inflate_batch_device): decode a stream, or a batch of them, to its
// bytes in device memory.  k_inflate runs inflate_write.h as one wave per stream -- the scalar chain of k_verify with the lanes
// storing where verify's compare -- and, for a framed stream, the checksum kernels of the encode run over the OUTPUT afterwards and
// k_inflate_trailer compares them with the trailer.  tests/inflwrite/ builds the same text for the host.  The host driver's shared
// steps are in decode_host.inc.  DESIGN.md section 12.
#include "inflate_write.h"

namespace mi355 {

// The lanes' writes.  A load step of a match may read bytes that other lanes of this wave stored earlier: inflate_write.h calls
// fence() between those stores and that load (workgroup scope: both sides are on one compute unit, whose vector L1 serves them
// coherently; what remains is that the stores have left the wave -- the vector-memory counter at zero).
struct WaveSink : WaveOps {
    static __host__ __device__ void store_lits(const uint8_t* lit, uint8_t* out, uint64_t cap, uint64_t lit_p, uint32_t n) {
        iw::iw_lane_lits(lit, out, cap, lit_p, n, lane());
    }
    static __host__ __device__ void copy_match(uint8_t* out, uint64_t cap, uint64_t p, uint32_t len, uint32_t dist) {
        for (uint32_t base = 0; base < 320 && base < len; base += 64) iw::iw_lane_match(out, cap, p, len, dist, base, lane());
    }
    static __host__ __device__ void copy_run(const uint8_t* src, uint8_t* out, uint64_t cap, uint64_t p, uint32_t n) {
        const uint32_t head = iw::iw_run_head(out, p, n);
        iw::iw_lane_run_head(src, out, cap, p, head, lane());
        for (uint32_t base = 0; base < 65536 && head + base < n; base += 512) iw::iw_lane_run(src, out, cap, p, n, head, base, lane());
    }
    static __host__ __device__ void fence(uint64_t) {
#if defined(__HIP_DEVICE_COMPILE__)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the fence's own wait, spelled out)
#endif
    }
};

struct IItem {
    const uint8_t* stream;
    uint64_t stream_len;
    uint8_t* out;
    uint64_t cap;
    const DevScalars* sc;  // where the output's checksum sums land (k_adler_part / k_crc_*; kb_adler_part / kb_crc), nullptr for a raw stream
    uint32_t wrapper, pad;
};

// one workgroup of one wave per stream: the stream's bytes into out[0, cap), the stream's record
__global__ __launch_bounds__(64) void k_inflate(const IItem* __restrict__ items, iw::Rec* __restrict__ recs) {
    __shared__ ic::Tables s_t;
    const IItem it = items[blockIdx.x];
    iw::Rec r;
    iw::iw_inflate<WaveSink>(s_t, it.stream, it.stream_len, it.wrapper, it.out, it.cap, r);
    if (threadIdx.x == 0) recs[blockIdx.x] = r;
}

// a lane per stream, after the checksum kernels: the trailer of every framed stream that is clean and fits against the sums of its output
__global__ __launch_bounds__(64) void k_inflate_trailer(const IItem* __restrict__ items, iw::Rec* __restrict__ recs, uint32_t n) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const IItem it = items[i];
    iw::Rec r = recs[i];
    if (!it.sc || !iw::iw_judged(r, it.wrapper, it.cap)) return;
    const uint64_t a = (1 + it.sc->adler_a) % 65521u, b = (r.out_len + it.sc->adler_b) % 65521u;  // (k_adler_fold's arithmetic)
    iw::iw_check_trailer(it.stream, it.stream_len, it.wrapper, (uint32_t)((b << 16) | a), it.sc->crc, r);
    if (r.status) recs[i] = r;
}

}  // namespace mi355

namespace {

static_assert(sizeof(mi355_inflate_report) == 56 && sizeof(iw::Rec) == 56, "mi355_inflate_report is 56 bytes");

void inflate_say(mi355_deflate_ctx* c, const mi355_inflate_report& r, int rc, const char* what) {
    char buf[200];
    if (rc == MI355_E_DATA)
        snprintf(buf, sizeof buf, "%s: %s at bit %llu, output byte %llu", what, ic::ic_status_name(r.status), (unsigned long long)r.bit,
                 (unsigned long long)r.out_pos);
    else
        snprintf(buf, sizeof buf, "%s: the stream inflates to %llu bytes", what, (unsigned long long)r.out_len);
    c->err = buf;
}

int inflate_rc(int iw_rc) { return iw_rc == iw::IW_OK ? MI355_OK : iw_rc == iw::IW_DATA ? MI355_E_DATA : MI355_E_OUT_TOO_SMALL; }

// the arguments every single-stream decode entry refuses; out / out_cap / out_len are the table's of an index call
bool inflate_args_bad(const void* stream, size_t stream_len, int wrapper, const void* out, size_t out_cap, const size_t* out_len,
                      const mi355_inflate_report* report) {
    return !report || !out_len || (!stream && stream_len) || (!out && out_cap) || wrapper < 0 || wrapper > 2;
}

// The end of a framed call, around the checksum launches over the outputs that are clean and fit (sums()): k_inflate_trailer over the
// k records at rec_at of the descriptor room, whose items are at its front, the records back, the wait.  mark(0) and mark(1) stand
// around the launches (the tabled driver's stage clock).
template <class Sums, class Mark>
int framed_tail(mi355_deflate_ctx* c, hipStream_t st, size_t k, size_t rec_at, Sums sums, Mark mark) {
    HIPCHK(c, mark(0));
    const int rc = sums();
    if (rc) return rc;
    hipLaunchKernelGGL(k_inflate_trailer, dim3(cdiv(k, 64)), dim3(64), 0, st, reinterpret_cast<const IItem*>(c->v_dev),
                       reinterpret_cast<iw::Rec*>(c->v_dev + rec_at), (uint32_t)k);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, mark(1));
    HIPCHK(c, hipMemcpyAsync(c->v_host + rec_at, c->v_dev + rec_at, sizeof(iw::Rec) * k, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return MI355_OK;
}

// k streams, device resident.  The decode launch, the records back (the one wait of a raw call); framed: the checksum launches over
// the outputs that are clean and fit -- `one`: launch_sums_one into the context's scalars, else the batch's plan over one flat grid
// --, and framed_tail.  fill(j, item): the j-th stream.  The records are left in c->v_host, *recs_out.
template <class Fill>
int inflate_run(mi355_deflate_ctx* c, size_t k, int wrapper, bool one, hipStream_t st, Fill fill, const iw::Rec** recs_out) {
    // [IItem k] and, for a framed batch, the checksum plan behind them
    const bool batch_sums = wrapper && !one;
    const BatchSums plan(sizeof(IItem) * k, k, batch_sums, sizeof(iw::Rec));
    const size_t rec_at = plan.rec_at;
    int rc = verify_room(c, plan.bytes);
    if (rc) return rc;
    IItem* hit = reinterpret_cast<IItem*>(c->v_host);
    for (size_t j = 0; j < k; j++) {
        fill(j, hit[j]);
        hit[j].sc = !wrapper ? nullptr : one ? c->d_sc : &plan.states(c)[j].sc;
        hit[j].wrapper = (uint32_t)wrapper, hit[j].pad = 0;
    }
    const iw::Rec* recs = reinterpret_cast<const iw::Rec*>(c->v_host + rec_at);
    *recs_out = recs;
    HIPCHK(c, hipMemcpyAsync(c->v_dev, c->v_host, plan.bat_at, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_inflate, dim3((uint32_t)k), dim3(64), 0, st, reinterpret_cast<const IItem*>(c->v_dev),
                       reinterpret_cast<iw::Rec*>(c->v_dev + rec_at));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->v_host + rec_at, c->v_dev + rec_at, sizeof(iw::Rec) * k, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (!wrapper) return MI355_OK;
    // the second half of a framed call: the output's length is known now
    size_t judged = 0;
    for (size_t j = 0; j < k; j++)
        if (iw::iw_judged(recs[j], (uint32_t)wrapper, hit[j].cap)) {
            if (recs[j].out_len > VERIFY_MAX_IN) return MI355_E_UNSUPPORTED;  // (what the checksum kernels take)
            judged++;
        }
    if (!judged) return MI355_OK;
    return framed_tail(
        c, st, k, rec_at,
        [&]() {
            if (one) return launch_sums_one(c, st, wrapper, hit[0].out, recs[0].out_len);
            const int rc = plan.fill(c, [&](size_t j, const uint8_t** p, uint64_t* n) {
                *p = hit[j].out, *n = iw::iw_judged(recs[j], (uint32_t)wrapper, hit[j].cap) ? recs[j].out_len : 0;
            });
            if (rc) return rc;
            HIPCHK(c, hipMemcpyAsync(c->v_dev + plan.bat_at, c->v_host + plan.bat_at, plan.st_at - plan.bat_at, hipMemcpyHostToDevice, st));
            return plan.launch(c, wrapper, st);
        },
        [](int) { return hipSuccess; });
}

// one stream, device resident, its arguments checked by the entry; *valid: the bytes of d_out that hold data
int inflate_one(mi355_deflate_ctx* c, const uint8_t* d_stream, size_t stream_len, int wrapper, uint8_t* d_out, size_t out_cap, size_t* out_len,
                mi355_inflate_report* report, hipStream_t st, uint64_t* valid) {
    const auto t0 = std::chrono::steady_clock::now();
    const iw::Rec* recs = nullptr;
    int rc = inflate_run(c, 1, wrapper, true, st,
                         [&](size_t, IItem& it) { it.stream = d_stream, it.stream_len = stream_len, it.out = d_out, it.cap = out_cap; }, &recs);
    if (rc) return rc;
    rc = inflate_rc(iw::iw_report(recs[0], out_cap, *report, valid));
    report->ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *out_len = rc == MI355_E_DATA ? (size_t)*valid : (size_t)report->out_len;
    if (rc != MI355_OK) inflate_say(c, *report, rc, "inflate");
    return rc;
}

}  // namespace

extern "C" {

int mi355_inflate_device(mi355_deflate_ctx* c, const void* d_stream, size_t stream_len, int wrapper, void* d_out, size_t out_cap,
                         size_t* out_len, mi355_inflate_report* report, void* hip_stream) {
    DefaultGuard dg_;
    c = use_ctx(c, dg_);
    if (!c) return MI355_E_HIP;
    HIPCHK(c, hipSetDevice(c->device));
    if (inflate_args_bad(d_stream, stream_len, wrapper, d_out, out_cap, out_len, report)) return MI355_E_ARG;
    if (const int rc = shard_refusal(c)) return rc;
    uint64_t valid = 0;
    return inflate_one(c, reinterpret_cast<const uint8_t*>(d_stream), stream_len, wrapper, reinterpret_cast<uint8_t*>(d_out), out_cap, out_len,
                       report, call_stream(c, hip_stream), &valid);
}

// host buffers: staged_call around the one-wave worker
int mi355_inflate(mi355_deflate_ctx* c, const uint8_t* stream, size_t stream_len, int wrapper, uint8_t* out, size_t out_cap, size_t* out_len,
                  mi355_inflate_report* report) {
    DefaultGuard dg_;
    c = use_ctx(c, dg_);
    if (!c) return MI355_E_HIP;
    if (inflate_args_bad(stream, stream_len, wrapper, out, out_cap, out_len, report)) return MI355_E_ARG;
    return staged_call(c, stream, stream_len, out, out_cap, [&](const uint8_t* d_stream, uint8_t* d_out, hipStream_t st, uint64_t* valid) {
        return inflate_one(c, d_stream, stream_len, wrapper, d_out, out_cap, out_len, report, st, valid);
    });
}

// one decode launch for all items, one workgroup per item; the framed items' checksums over one flat grid behind it
int mi355_inflate_batch_device(mi355_deflate_ctx* c, mi355_batch_item* items, size_t n_items, int wrapper, mi355_inflate_report* reports,
                               void* hip_stream) {
    DefaultGuard dg_;
    c = use_ctx(c, dg_);
    if (!c) return MI355_E_HIP;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint32_t> act;
    int rc = batch_active(c, items, n_items, wrapper, act, [](const mi355_batch_item& it) { return !it.out && it.out_cap ? MI355_E_ARG : MI355_OK; });
    if (rc || act.empty()) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const iw::Rec* recs = nullptr;
    rc = inflate_run(c, act.size(), wrapper, false, call_stream(c, hip_stream),
                     [&](size_t j, IItem& it) {
                         const mi355_batch_item& b = items[act[j]];
                         it.stream = reinterpret_cast<const uint8_t*>(b.in), it.stream_len = b.in_len;
                         it.out = reinterpret_cast<uint8_t*>(b.out), it.cap = b.out_cap;
                     },
                     &recs);
    if (rc) return rc;
    const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return batch_give(
        items, act, reports, ms, "inflate",
        [&](size_t j, mi355_batch_item& b, mi355_inflate_report& r) {
            uint64_t valid = 0;
            const int s = inflate_rc(iw::iw_report(recs[j], b.out_cap, r, &valid));
            b.out_len = s == MI355_E_DATA ? (size_t)valid : (size_t)r.out_len;
            return s;
        },
        [&](const mi355_inflate_report& r, int s, const char* what) { inflate_say(c, r, s, what); });
}

}  // extern "C"
