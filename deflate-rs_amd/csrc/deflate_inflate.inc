// Inflate (include/mi355_deflate.h mi355_inflate[_device], mi355_inflate_batch_device): decode a stream, or a batch of them, to its
// bytes in device memory.  k_inflate runs inflate_write.h as one wave per stream -- the scalar chain of k_verify with the lanes
// storing where verify's compare -- and, for a framed stream, the checksum kernels of the encode run over the OUTPUT afterwards and
// k_inflate_trailer compares them with the trailer.  tests/inflwrite/ builds the same text for the host.  DESIGN.md section 12.
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

// k streams, device resident.  The decode launch, the records back (the one wait of a raw call); framed: the checksum launches over
// the outputs that are clean and fit -- `one`: k_adler_part / k_crc_part + fold into the context's scalars, else kb_adler_part /
// kb_crc over one flat grid --, k_inflate_trailer, the records back again.  fill(j, item): the j-th stream.  The records are left
// in c->v_host at the offset returned in *recs_at.
template <class Fill>
int inflate_run(mi355_deflate_ctx* c, size_t k, int wrapper, bool one, hipStream_t st, Fill fill, const iw::Rec** recs_out) {
    // [IItem k] | [BatchItem k][running sums BS_N x (k + 1)] | [DevState k] | [Rec k]
    const bool batch_sums = wrapper && !one;
    const size_t bat_at = align_up(sizeof(IItem) * k, 256);
    const size_t pre_at = bat_at + (batch_sums ? sizeof(BatchItem) * k : 0);
    const size_t st_at = align_up(pre_at + (batch_sums ? sizeof(uint32_t) * BS_N * (k + 1) : 0), 256);
    const size_t rec_at = align_up(st_at + (batch_sums ? sizeof(DevState) * k : 0), 256);
    int rc = verify_room(c, rec_at + sizeof(iw::Rec) * k);
    if (rc) return rc;
    IItem* hit = reinterpret_cast<IItem*>(c->v_host);
    DevState* dst = reinterpret_cast<DevState*>(c->v_dev + st_at);
    for (size_t j = 0; j < k; j++) {
        fill(j, hit[j]);
        hit[j].sc = !wrapper ? nullptr : one ? c->d_sc : &dst[j].sc;
        hit[j].wrapper = (uint32_t)wrapper, hit[j].pad = 0;
    }
    const IItem* d_items = reinterpret_cast<const IItem*>(c->v_dev);
    iw::Rec* d_recs = reinterpret_cast<iw::Rec*>(c->v_dev + rec_at);
    const iw::Rec* recs = reinterpret_cast<const iw::Rec*>(c->v_host + rec_at);
    *recs_out = recs;
    HIPCHK(c, hipMemcpyAsync(c->v_dev, c->v_host, bat_at, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_inflate, dim3((uint32_t)k), dim3(64), 0, st, d_items, d_recs);
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
    if (one) {
        const uint64_t n = recs[0].out_len;
        if (wrapper == 2) {
            rc = ensure_buf(c, &c->d_crc, &c->d_crc_cap, ((size_t)cdiv(n, CRC_CHUNK) + 2) * 4 + 512);
            if (rc) return rc;
        }
        HIPCHK(c, hipMemsetAsync(c->d_sc, 0, sizeof(DevScalars), st));
        if (wrapper == 1) launch_adler(c, st, hit[0].out, n);
        if (wrapper == 2) launch_crc(c, st, hit[0].out, n, reinterpret_cast<uint32_t*>(c->d_crc));
    } else {
        BatchItem* hb = reinterpret_cast<BatchItem*>(c->v_host + bat_at);
        uint32_t* hpre = reinterpret_cast<uint32_t*>(c->v_host + pre_at);
        memset(c->v_host + bat_at, 0, st_at - bat_at);
        for (size_t j = 0; j < k; j++) {
            const bool on = iw::iw_judged(recs[j], (uint32_t)wrapper, hit[j].cap);
            const uint64_t n = on ? recs[j].out_len : 0;
            hb[j].in = hit[j].out;
            hb[j].n = (uint32_t)n;
            hb[j].st = dst + j;
            const uint64_t wg[2] = {cdiv(n, ADLER_CHUNK), cdiv(n, 256 * CRC_CHUNK)};
            for (uint32_t s = 0; s < 2; s++) {
                const size_t row = (size_t)(s ? BS_CRC : BS_ADLER) * (k + 1);
                const uint64_t t = (uint64_t)hpre[row + j] + wg[s];
                if (t > 0x7fffffffull) return MI355_E_ARG;
                hpre[row + j + 1] = (uint32_t)t;
            }
        }
        HIPCHK(c, hipMemcpyAsync(c->v_dev + bat_at, c->v_host + bat_at, st_at - bat_at, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemsetAsync(dst, 0, sizeof(DevState) * k, st));
        const BatchArgs a{reinterpret_cast<const BatchItem*>(c->v_dev + bat_at), reinterpret_cast<const uint32_t*>(c->v_dev + pre_at), (uint32_t)k};
        const uint32_t grid = hpre[(size_t)(wrapper == 1 ? BS_ADLER : BS_CRC) * (k + 1) + k];
        if (grid && wrapper == 1) hipLaunchKernelGGL(kb_adler_part, dim3(grid), dim3(256), 0, st, a);
        if (grid && wrapper == 2) hipLaunchKernelGGL(kb_crc, dim3(grid), dim3(256), 0, st, a);
    }
    hipLaunchKernelGGL(k_inflate_trailer, dim3(cdiv(k, 64)), dim3(64), 0, st, d_items, d_recs, (uint32_t)k);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->v_host + rec_at, c->v_dev + rec_at, sizeof(iw::Rec) * k, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return MI355_OK;
}

// one stream, device resident; *valid: the bytes of d_out that hold data
int inflate_one(mi355_deflate_ctx* c, const uint8_t* d_stream, size_t stream_len, int wrapper, uint8_t* d_out, size_t out_cap, size_t* out_len,
                mi355_inflate_report* report, hipStream_t st, uint64_t* valid) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!report || !out_len || (!d_stream && stream_len) || (!d_out && out_cap) || wrapper < 0 || wrapper > 2) return MI355_E_ARG;
    if (c->live_shard) {
        c->err = "the context holds a sharded encode";
        return MI355_E_STATE;
    }
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
    hipStream_t st = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : c->own_stream;
    uint64_t valid = 0;
    return inflate_one(c, reinterpret_cast<const uint8_t*>(d_stream), stream_len, wrapper, reinterpret_cast<uint8_t*>(d_out), out_cap, out_len,
                       report, st, &valid);
}

// host buffers: the stream goes into the context's staging with a plain copy, the bytes that hold data come back with one
int mi355_inflate(mi355_deflate_ctx* c, const uint8_t* stream, size_t stream_len, int wrapper, uint8_t* out, size_t out_cap, size_t* out_len,
                  mi355_inflate_report* report) {
    DefaultGuard dg_;
    c = use_ctx(c, dg_);
    if (!c) return MI355_E_HIP;
    if (!report || !out_len || (!stream && stream_len) || (!out && out_cap) || wrapper < 0 || wrapper > 2) return MI355_E_ARG;
    if (c->live_shard) {
        c->err = "the context holds a sharded encode";
        return MI355_E_STATE;
    }
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure_buf(c, &c->d_in, &c->d_in_cap, stream_len + 64);
    if (rc) return rc;
    rc = ensure_buf(c, &c->d_out, &c->d_out_cap, out_cap + 64);
    if (rc) return rc;
    hipStream_t st = c->own_stream;
    if (stream_len) HIPCHK(c, hipMemcpyAsync(c->d_in, stream, stream_len, hipMemcpyHostToDevice, st));
    uint64_t valid = 0;
    rc = inflate_one(c, c->d_in, stream_len, wrapper, out_cap ? c->d_out : nullptr, out_cap, out_len, report, st, &valid);
    if (rc != MI355_OK && rc != MI355_E_DATA && rc != MI355_E_OUT_TOO_SMALL) {
        (void)hipStreamSynchronize(st);  // (the copy of the caller's buffer may be in flight)
        return rc;
    }
    if (valid) HIPCHK(c, hipMemcpy(out, c->d_out, (size_t)valid, hipMemcpyDeviceToHost));
    return rc;
}

// one decode launch for all items, one workgroup per item; the framed items' checksums over one flat grid behind it
int mi355_inflate_batch_device(mi355_deflate_ctx* c, mi355_batch_item* items, size_t n_items, int wrapper, mi355_inflate_report* reports,
                               void* hip_stream) {
    DefaultGuard dg_;
    c = use_ctx(c, dg_);
    if (!c) return MI355_E_HIP;
    const auto t0 = std::chrono::steady_clock::now();
    if ((!items && n_items) || wrapper < 0 || wrapper > 2 || n_items > 0x7fffffffull) return MI355_E_ARG;
    std::vector<uint32_t> act;
    for (size_t i = 0; i < n_items; i++) {
        if (items[i].status != MI355_OK) continue;  // skipped, left alone
        if ((!items[i].in && items[i].in_len) || (!items[i].out && items[i].out_cap)) return MI355_E_ARG;
        act.push_back((uint32_t)i);
    }
    if (c->live_shard) {
        c->err = "the context holds a sharded encode";
        return MI355_E_STATE;
    }
    if (act.empty()) return MI355_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : c->own_stream;
    const iw::Rec* recs = nullptr;
    int rc = inflate_run(c, act.size(), wrapper, false, st,
                         [&](size_t j, IItem& it) {
                             const mi355_batch_item& b = items[act[j]];
                             it.stream = reinterpret_cast<const uint8_t*>(b.in), it.stream_len = b.in_len;
                             it.out = reinterpret_cast<uint8_t*>(b.out), it.cap = b.out_cap;
                         },
                         &recs);
    if (rc) return rc;
    const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    int first = MI355_OK;
    for (size_t j = 0; j < act.size(); j++) {
        mi355_batch_item& b = items[act[j]];
        mi355_inflate_report r;
        uint64_t valid = 0;
        const int s = inflate_rc(iw::iw_report(recs[j], b.out_cap, r, &valid));
        r.ms = ms;
        if (reports) reports[act[j]] = r;
        b.status = s;
        b.out_len = s == MI355_E_DATA ? (size_t)valid : (size_t)r.out_len;
        if (s != MI355_OK && first == MI355_OK) {
            first = s;
            char what[48];
            snprintf(what, sizeof what, "inflate: item %u", act[j]);
            inflate_say(c, r, s, what);
        }
    }
    return first;
}

}  // extern "C"
