// Inflate (include/mi355_deflate.h mi355_inflate[_device], mi355_inflate_batch_device): decode a stream, or a batch of them, to its
// bytes in device memory.  k_inflate runs inflate_write.h as one wave per stream -- the scalar chain of k_verify with the lanes
// storing where verify's compare -- and, for a framed stream, the checksum kernels of the encode run over the OUTPUT afterwards and
// k_inflate_trailer compares them with the trailer.  tests/inflwrite/ builds the same text for the host.  The host driver's shared
// steps are in decode_host.inc; the two halves of a decode over IItems -- decode_half: upload, a kernel of one wave per item, records
// back, wait; sums_half: the checksum launches and framed_tail, the one place k_inflate_trailer is launched from -- are here, and the
// members and BGZF-read drivers call them too.  DESIGN.md section 12.
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
// k records at rec_at of the descriptor room, whose items are at its front, the records back, the wait.  The stage clock of a
// caller that keeps one: mark(0) in front of the checksum launches, mark(2) between them and k_inflate_trailer, mark(1) behind it.
template <class Sums, class Mark>
int framed_tail(mi355_deflate_ctx* c, hipStream_t st, size_t k, size_t rec_at, Sums sums, Mark mark) {
    HIPCHK(c, mark(0));
    const int rc = sums();
    if (rc) return rc;
    HIPCHK(c, mark(2));
    hipLaunchKernelGGL(k_inflate_trailer, dim3(cdiv(k, 64)), dim3(64), 0, st, reinterpret_cast<const IItem*>(c->v_dev),
                       reinterpret_cast<iw::Rec*>(c->v_dev + rec_at), (uint32_t)k);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, mark(1));
    HIPCHK(c, hipMemcpyAsync(c->v_host + rec_at, c->v_dev + rec_at, sizeof(iw::Rec) * k, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return MI355_OK;
}
const auto no_mark = [](int) { return hipSuccess; };

// The first half of a decode over IItems: the caller's k items at the front of the descriptor room -- and what else of its
// descriptors lies in the first `front` bytes -- go up, launch(items, records) starts a kernel of one wave per item between mark(0)
// and mark(1), the k records at rec_at come back, the wait.  They are left in c->v_host.
template <class Launch, class Mark>
int decode_half(mi355_deflate_ctx* c, hipStream_t st, size_t k, size_t front, size_t rec_at, Launch launch, Mark mark) {
    HIPCHK(c, hipMemcpyAsync(c->v_dev, c->v_host, front, hipMemcpyHostToDevice, st));
    HIPCHK(c, mark(0));
    launch(reinterpret_cast<const IItem*>(c->v_dev), reinterpret_cast<iw::Rec*>(c->v_dev + rec_at));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, mark(1));
    HIPCHK(c, hipMemcpyAsync(c->v_host + rec_at, c->v_dev + rec_at, sizeof(iw::Rec) * k, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return MI355_OK;
}
// k_inflate as decode_half's launch
auto inflate_launch(size_t k, hipStream_t st) {
    return [=](const IItem* items, iw::Rec* recs) { hipLaunchKernelGGL(k_inflate, dim3((uint32_t)k), dim3(64), 0, st, items, recs); };
}

// The second half, of a framed call, once the outputs' lengths are known: the checksum launches over the outputs that are clean
// and fit, and framed_tail.  The plan's k items are at the front of c->v_host and their records at plan.rec_at.  judged(j, &n): is
// item j's checksum judged, and over how many bytes of its out.  None judged: nothing is launched; one longer than the checksum
// kernels take: MI355_E_UNSUPPORTED.  `one`: launch_sums_one into the context's scalars, else the batch's plan over one flat grid,
// uploaded with what lies from `from` in front of it (0: the items again, their sc decided since the first half); recs_up: the
// records too, for a caller whose decode was not the launch in front (a members call).  mark: framed_tail's.
template <class Judged, class Mark>
int sums_half(mi355_deflate_ctx* c, hipStream_t st, const BatchSums& plan, int wrapper, bool one, size_t from, bool recs_up, Judged judged,
              Mark mark) {
    const IItem* hit = reinterpret_cast<const IItem*>(c->v_host);
    size_t n_judged = 0;
    uint64_t n = 0, n0 = 0;
    for (size_t j = 0; j < plan.k; j++)
        if (judged(j, &n)) {
            if (n > VERIFY_MAX_IN) return MI355_E_UNSUPPORTED;  // (what the checksum kernels take)
            if (!j) n0 = n;
            n_judged++;
        }
    if (!n_judged) return MI355_OK;
    if (!one) {
        const int rc = plan.fill(c, [&](size_t j, const uint8_t** p, uint64_t* len) {
            *p = hit[j].out;
            if (!judged(j, len)) *len = 0;
        });
        if (rc) return rc;
        HIPCHK(c, hipMemcpyAsync(c->v_dev + from, c->v_host + from, plan.st_at - from, hipMemcpyHostToDevice, st));
    }
    if (recs_up)
        HIPCHK(c, hipMemcpyAsync(c->v_dev + plan.rec_at, c->v_host + plan.rec_at, sizeof(iw::Rec) * plan.k, hipMemcpyHostToDevice, st));
    return framed_tail(c, st, plan.k, plan.rec_at, [&]() { return one ? launch_sums_one(c, st, wrapper, hit[0].out, n0) : plan.launch(c, wrapper, st); },
                       mark);
}

// k streams, device resident: the two halves in sequence, the second for a framed call.  fill(j, item): the j-th stream.  The
// records are left in c->v_host, *recs_out.
template <class Fill>
int inflate_run(mi355_deflate_ctx* c, size_t k, int wrapper, bool one, hipStream_t st, Fill fill, const iw::Rec** recs_out) {
    // [IItem k] and, for a framed batch, the checksum plan behind them
    const BatchSums plan(sizeof(IItem) * k, k, wrapper && !one, sizeof(iw::Rec));
    int rc = verify_room(c, plan.bytes);
    if (rc) return rc;
    IItem* hit = reinterpret_cast<IItem*>(c->v_host);
    for (size_t j = 0; j < k; j++) {
        fill(j, hit[j]);
        hit[j].sc = !wrapper ? nullptr : one ? c->d_sc : &plan.states(c)[j].sc;
        hit[j].wrapper = (uint32_t)wrapper, hit[j].pad = 0;
    }
    const iw::Rec* recs = reinterpret_cast<const iw::Rec*>(c->v_host + plan.rec_at);
    *recs_out = recs;
    rc = decode_half(c, st, k, plan.bat_at, plan.rec_at, inflate_launch(k, st), no_mark);
    if (rc || !wrapper) return rc;
    return sums_half(
        c, st, plan, wrapper, one, plan.bat_at, false,
        [&](size_t j, uint64_t* n) { return *n = recs[j].out_len, iw::iw_judged(recs[j], (uint32_t)wrapper, hit[j].cap); }, no_mark);
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
    if (const int rc = decode_enter(c, dg_, inflate_args_bad(d_stream, stream_len, wrapper, d_out, out_cap, out_len, report))) return rc;
    uint64_t valid = 0;
    return inflate_one(c, reinterpret_cast<const uint8_t*>(d_stream), stream_len, wrapper, reinterpret_cast<uint8_t*>(d_out), out_cap, out_len,
                       report, call_stream(c, hip_stream), &valid);
}

// host buffers: staged_call around the one-wave worker
int mi355_inflate(mi355_deflate_ctx* c, const uint8_t* stream, size_t stream_len, int wrapper, uint8_t* out, size_t out_cap, size_t* out_len,
                  mi355_inflate_report* report) {
    DefaultGuard dg_;
    if (const int rc = decode_enter(c, dg_, inflate_args_bad(stream, stream_len, wrapper, out, out_cap, out_len, report))) return rc;
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
