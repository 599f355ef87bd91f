// Verify (include/mi355_deflate.h mi355_deflate_verify[_device], mi355_deflate_verify_batch_device): does this stream inflate to
// this input?  k_verify decodes without writing a byte -- the expected output is the input -- one wave per entry: an entry is a
// restart point of the block table of the encode (mi355_deflate_last_blocks), or the whole stream when there is no table; the
// batched form has one entry per item.  What is valid is decided by inflate_check.h, text that tests/inflcheck/ builds for the
// host; this file adds the wave's way of comparing bytes and the host driver, whose shared steps are in decode_host.inc.  DESIGN.md
// section 11.
#include "inflate_check.h"

namespace mi355 {

// The decode state of inflate_check.h (bit position, output position, the symbol step) is the same in all 64 lanes: the
// lanes run it in step, values read from LDS are made scalar again (uni), and the leader alone writes the tables.  The
// lanes differ in the compares.
struct WaveOps {
    static __host__ __device__ bool leader() {
#if defined(__HIP_DEVICE_COMPILE__)
        return threadIdx.x == 0;
#else
        return true;
#endif
    }
    static __host__ __device__ void sync() {
#if defined(__HIP_DEVICE_COMPILE__)
        wave_lds_fence();
#endif
    }
    static __host__ __device__ uint32_t uni(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
        return __builtin_amdgcn_readfirstlane(v);
#else
        return v;
#endif
    }
    // The compares: every lane asks inflate_check.h what it sees (ic_lane_*), a ballot and a find-first name the first lane with an
    // answer, and that lane's answer -- the first differing byte -- goes to all.
    static __host__ __device__ uint32_t first_of(uint32_t mine, uint32_t none) {
#if defined(__HIP_DEVICE_COMPILE__)
        const uint64_t m = __ballot(mine != ic::NONE);
        return m ? (uint32_t)__shfl((int)mine, (int)__builtin_ctzll(m), 64) : none;
#else
        (void)mine;
        return none;
#endif
    }
    static __host__ __device__ uint32_t lane() {
#if defined(__HIP_DEVICE_COMPILE__)
        return threadIdx.x;
#else
        return 0;
#endif
    }
    static __host__ __device__ uint32_t first_diff_lits(const uint8_t* lit, const uint8_t* in, uint32_t n) {
        return first_of(ic::ic_lane_lits(lit, in, n, lane()), n);
    }
    static __host__ __device__ uint32_t first_diff_match(const uint8_t* in, uint64_t p, uint32_t len, uint32_t dist) {
        for (uint32_t base = 0; base < 320 && base < len; base += 64) {
            const uint32_t d = first_of(ic::ic_lane_match(in, p, len, dist, base, lane()), ic::NONE);
            if (d != ic::NONE) return d;
        }
        return len;
    }
    static __host__ __device__ uint64_t first_diff_run(const uint8_t* a, const uint8_t* b, uint64_t n) {
        const uint32_t n32 = (uint32_t)(n < 65535 ? n : 65535);
        for (uint32_t base = 0; base < 65536 && base < n32; base += 512) {
            const uint32_t d = first_of(ic::ic_lane_run(a, b, n32, base, lane()), ic::NONE);
            if (d != ic::NONE) return d;
        }
        return n;
    }
};

struct VItem {
    const uint8_t* stream;
    uint64_t stream_len;
    const uint8_t* in;
    uint64_t in_len;
    const DevScalars* sc;  // the input's checksum sums (k_adler_part / k_crc_*; kb_adler_part / kb_crc), nullptr for a raw stream
    uint32_t wrapper, pad;
};

// one workgroup of one wave per entry; the batched form has an entry per item.  Nothing but the entry's record is written.
__global__ __launch_bounds__(64) void k_verify(const VItem* __restrict__ items, const ic::Entry* __restrict__ ents, ic::Rec* __restrict__ recs) {
    __shared__ ic::Tables s_t;
    const ic::Entry e = ents[blockIdx.x];
    const VItem it = items[e.item];
    uint32_t adler = 0, crc = 0;
    if (it.sc) {  // (k_adler_fold's arithmetic)
        const uint64_t a = (1 + it.sc->adler_a) % 65521u, b = (it.in_len + it.sc->adler_b) % 65521u;
        adler = (uint32_t)((b << 16) | a);
        crc = it.sc->crc;
    }
    ic::Rec r;
    ic::ic_verify_entry<WaveOps>(s_t, it.stream, it.stream_len, it.in, it.in_len, it.wrapper, adler, crc, e, r);
    if (threadIdx.x == 0) recs[blockIdx.x] = r;
}

}  // namespace mi355

namespace {

static_assert(sizeof(mi355_verify_report) == 48, "mi355_verify_report is 48 bytes");
static_assert(MI355_VERIFY_OK == ic::V_OK && MI355_VERIFY_FRAME == ic::V_FRAME && MI355_VERIFY_BTYPE == ic::V_BTYPE &&
                  MI355_VERIFY_STORED == ic::V_STORED && MI355_VERIFY_LENGTHS == ic::V_LENGTHS && MI355_VERIFY_CODE == ic::V_CODE &&
                  MI355_VERIFY_DISTANCE == ic::V_DISTANCE && MI355_VERIFY_MISMATCH == ic::V_MISMATCH && MI355_VERIFY_LENGTH == ic::V_LENGTH &&
                  MI355_VERIFY_TABLE == ic::V_TABLE && MI355_VERIFY_TRUNCATED == ic::V_TRUNCATED && MI355_VERIFY_TRAILER == ic::V_TRAILER &&
                  MI355_VERIFY_CHECKSUM == ic::V_CHECKSUM,
              "inflate_check.h mirrors MI355_VERIFY_*");

void verify_say(mi355_deflate_ctx* c, const mi355_verify_report& r, const char* what) {
    char buf[200];
    snprintf(buf, sizeof buf, "%s: %s at entry %u, bit %llu, input byte %llu", what, ic::ic_status_name(r.status), r.entry,
             (unsigned long long)r.bit, (unsigned long long)r.in_pos);
    c->err = buf;
}

// what both single entries refuse before any work, in this order; table_bad: a table's length without the table
int verify_refusal(mi355_deflate_ctx* c, const void* stream, size_t stream_len, const void* in, size_t in_len, int wrapper, bool table_bad,
                   const mi355_verify_report* report) {
    if (!report || (!stream && stream_len) || (!in && in_len) || wrapper < 0 || wrapper > 2 || table_bad) return MI355_E_ARG;
    if (in_len > VERIFY_MAX_IN) return MI355_E_UNSUPPORTED;
    return shard_refusal(c);
}

// one stream, device resident, behind verify_refusal: checksum launches, k_verify over the entries, one copy back, one wait
int verify_one(mi355_deflate_ctx* c, const uint8_t* d_stream, size_t stream_len, const uint8_t* d_in, size_t in_len, int wrapper,
               const mi355_block_info* blocks, size_t n_blocks, mi355_verify_report* report, hipStream_t st) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!blocks && n_blocks) return MI355_E_ARG;  // (mi355_deflate_verify has always left this pair to here, behind its copies)
    uint64_t sum = 0;
    for (size_t k = 0; k < n_blocks; k++) {
        if (k && blocks[k].bit_start < blocks[k - 1].bit_start) {
            c->err = "verify: the table's bit_start values do not ascend";
            return MI355_E_ARG;
        }
        if (blocks[k].in_bytes > in_len - sum) {
            c->err = "verify: the table's in_bytes do not sum to in_len";
            return MI355_E_ARG;
        }
        sum += blocks[k].in_bytes;
    }
    if (n_blocks && sum != in_len) {
        c->err = "verify: the table's in_bytes do not sum to in_len";
        return MI355_E_ARG;
    }
    const size_t ne = n_blocks ? n_blocks : 1;
    if (ne > 0x7fffffffull) return MI355_E_ARG;
    const size_t ent_at = align_up(sizeof(VItem), 256), rec_at = align_up(ent_at + sizeof(ic::Entry) * ne, 256);
    const size_t bytes = rec_at + sizeof(ic::Rec) * ne;
    int rc = verify_room(c, bytes);
    if (rc) return rc;
    VItem* hit = reinterpret_cast<VItem*>(c->v_host);
    *hit = VItem{d_stream, stream_len, d_in, in_len, wrapper ? c->d_sc : nullptr, (uint32_t)wrapper, 0u};
    ic::Entry* hent = reinterpret_cast<ic::Entry*>(c->v_host + ent_at);
    ic::ic_make_entries([&](uint64_t k) { return blocks[k].bit_start; }, [&](uint64_t k) { return blocks[k].in_bytes; }, n_blocks, 0u, hent);
    if (wrapper) {
        rc = launch_sums_one(c, st, wrapper, d_in, in_len);
        if (rc) return rc;
    }
    HIPCHK(c, hipMemcpyAsync(c->v_dev, c->v_host, rec_at, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_verify, dim3((uint32_t)ne), dim3(64), 0, st, reinterpret_cast<const VItem*>(c->v_dev),
                       reinterpret_cast<const ic::Entry*>(c->v_dev + ent_at), reinterpret_cast<ic::Rec*>(c->v_dev + rec_at));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->v_host + rec_at, c->v_dev + rec_at, sizeof(ic::Rec) * ne, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    ic::ic_report(reinterpret_cast<const ic::Rec*>(c->v_host + rec_at), ne, *report);
    report->ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (report->status == MI355_VERIFY_OK) return MI355_OK;
    verify_say(c, *report, "verify");
    return MI355_E_VERIFY;
}

}  // namespace

extern "C" {

int mi355_deflate_verify_device(mi355_deflate_ctx* c, const void* d_stream, size_t stream_len, const void* d_in, size_t in_len,
                                int wrapper, const mi355_block_info* blocks, size_t n_blocks, mi355_verify_report* report,
                                void* hip_stream) {
    DefaultGuard dg_;
    c = use_ctx(c, dg_);
    if (!c) return MI355_E_HIP;
    HIPCHK(c, hipSetDevice(c->device));
    if (const int rc = verify_refusal(c, d_stream, stream_len, d_in, in_len, wrapper, !blocks && n_blocks, report)) return rc;
    return verify_one(c, reinterpret_cast<const uint8_t*>(d_stream), stream_len, reinterpret_cast<const uint8_t*>(d_in), in_len, wrapper,
                      blocks, n_blocks, report, call_stream(c, hip_stream));
}

// host buffers: the stream and the input go into the context's staging with plain copies (two inputs and nothing to hand back: not
// the shape of staged_call)
int mi355_deflate_verify(mi355_deflate_ctx* c, const uint8_t* stream, size_t stream_len, const uint8_t* in, size_t in_len, int wrapper,
                         const mi355_block_info* blocks, size_t n_blocks, mi355_verify_report* report) {
    DefaultGuard dg_;
    c = use_ctx(c, dg_);
    if (!c) return MI355_E_HIP;
    int rc = verify_refusal(c, stream, stream_len, in, in_len, wrapper, false, report);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = ensure_buf(c, &c->d_in, &c->d_in_cap, in_len + 64);
    if (rc) return rc;
    rc = ensure_buf(c, &c->d_out, &c->d_out_cap, stream_len + 64);
    if (rc) return rc;
    hipStream_t st = c->own_stream;
    if (in_len) HIPCHK(c, hipMemcpyAsync(c->d_in, in, in_len, hipMemcpyHostToDevice, st));
    if (stream_len) HIPCHK(c, hipMemcpyAsync(c->d_out, stream, stream_len, hipMemcpyHostToDevice, st));
    rc = verify_one(c, c->d_out, stream_len, c->d_in, in_len, wrapper, blocks, n_blocks, report, st);
    if (rc != MI355_OK && rc != MI355_E_VERIFY) (void)hipStreamSynchronize(st);  // (the copies of the caller's buffers may be in flight)
    return rc;
}

// every item without a table: one launch, one workgroup per item; the items' checksums over one flat grid before it
int mi355_deflate_verify_batch_device(mi355_deflate_ctx* c, mi355_batch_item* items, size_t n_items, int wrapper,
                                      mi355_verify_report* reports, void* hip_stream) {
    DefaultGuard dg_;
    c = use_ctx(c, dg_);
    if (!c) return MI355_E_HIP;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint32_t> act;
    int rc = batch_active(c, items, n_items, wrapper, act, [](const mi355_batch_item& it) {
        return !it.out && it.out_len ? MI355_E_ARG : it.in_len > VERIFY_MAX_IN ? MI355_E_UNSUPPORTED : MI355_OK;
    });
    if (rc || act.empty()) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = call_stream(c, hip_stream);
    const size_t k = act.size();
    // [VItem k][Entry k] and the checksum plan behind them
    const size_t ent_at = align_up(sizeof(VItem) * k, 256);
    const BatchSums plan(ent_at + sizeof(ic::Entry) * k, k, wrapper != 0, sizeof(ic::Rec));
    const size_t rec_at = plan.rec_at;
    rc = verify_room(c, plan.bytes);
    if (rc) return rc;
    VItem* hit = reinterpret_cast<VItem*>(c->v_host);
    ic::Entry* hent = reinterpret_cast<ic::Entry*>(c->v_host + ent_at);
    for (size_t j = 0; j < k; j++) {
        const mi355_batch_item& it = items[act[j]];
        hit[j] = VItem{reinterpret_cast<const uint8_t*>(it.out), it.out_len, reinterpret_cast<const uint8_t*>(it.in), it.in_len,
                       wrapper ? &plan.states(c)[j].sc : nullptr, (uint32_t)wrapper, 0u};
        hent[j] = ic::Entry{0, 0, 0, 0, 1u, (uint32_t)j};
    }
    if (wrapper) {
        rc = plan.fill(c, [&](size_t j, const uint8_t** p, uint64_t* n) { *p = hit[j].in, *n = hit[j].in_len; });
        if (rc) return rc;
    }
    HIPCHK(c, hipMemcpyAsync(c->v_dev, c->v_host, plan.st_at, hipMemcpyHostToDevice, st));  // (the descriptors and the plan in one)
    if (wrapper) {
        rc = plan.launch(c, wrapper, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_verify, dim3((uint32_t)k), dim3(64), 0, st, reinterpret_cast<const VItem*>(c->v_dev),
                       reinterpret_cast<const ic::Entry*>(c->v_dev + ent_at), reinterpret_cast<ic::Rec*>(c->v_dev + rec_at));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->v_host + rec_at, c->v_dev + rec_at, sizeof(ic::Rec) * k, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    const ic::Rec* recs = reinterpret_cast<const ic::Rec*>(c->v_host + rec_at);
    return batch_give(
        items, act, reports, ms, "verify",
        [&](size_t j, mi355_batch_item&, mi355_verify_report& r) {
            ic::ic_report(recs + j, 1, r);
            return r.status == MI355_VERIFY_OK ? MI355_OK : MI355_E_VERIFY;
        },
        [&](const mi355_verify_report& r, int, const char* what) { verify_say(c, r, what); });
}

}  // extern "C"
