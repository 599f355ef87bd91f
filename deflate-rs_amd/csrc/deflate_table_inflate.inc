// Tabled inflate (include/mi355_deflate.h mi355_inflate_tabled[_device]): ONE stream decoded from its encoder block table, every
// entry of the table by a wave of its own.  Three kinds of launch, nothing waits inside a kernel (inflate_table.h has the passes and
// their rules; tests/infltable/ builds the same text for the host):
//   k_inflate_tab          one workgroup of one wave per entry: the scalar chain of k_inflate, 16-bit symbols where it has bytes
//   k_inflate_tab_window   ONE workgroup: the resolved 32 KiB window behind every entry of the group, one entry a step
//   k_inflate_tab_resolve  flat over the output: bytes from symbols and windows -- the only kernel that writes `out`
// and then the checksum launches over the output and k_inflate_trailer: framed_tail of deflate_inflate.inc.  The host driver's shared
// steps are in decode_host.inc.  DESIGN.md section 13.
#include "inflate_table.h"

namespace mi355 {

// The lanes' writes of pass 1.  As in WaveSink, a load step of a match may read symbols that other lanes of this wave stored
// earlier: inflate_table.h calls fence() between those stores and that load.
struct TabSink : WaveOps {
    static __host__ __device__ void store_lits(const uint8_t* lit, it::Sink& o, uint64_t lit_p, uint32_t n) {
        it::it_lane_lits(lit, o.sym, o.base, o.cap, lit_p, n, lane());
    }
    static __host__ __device__ void copy_match(it::Sink& o, uint64_t p, uint32_t len, uint32_t dist) {
        for (uint32_t at = 0; at < 320 && at < len; at += 64) it::it_lane_match(o.sym, o.base, o.start, o.cap, p, len, dist, at, lane());
    }
    static __host__ __device__ void copy_run(const uint8_t* src, it::Sink& o, uint64_t p, uint32_t n) {
        const uint32_t head = it::it_run_head(o.sym, o.base, p, n);
        it::it_lane_run_head(src, o.sym, o.base, o.cap, p, head, lane());
        for (uint32_t at = 0; at < 65536 && head + at < n; at += 512) it::it_lane_run(src, o.sym, o.base, o.cap, p, n, head, at, lane());
    }
    static __host__ __device__ void fence(uint64_t) {
#if defined(__HIP_DEVICE_COMPILE__)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the fence's own wait, spelled out: DESIGN.md section 12)
#endif
    }
};

// the stream and the group's workspace, the same for every workgroup of a launch
struct TItem {
    const uint8_t* stream;
    uint64_t stream_len;
    uint16_t* sym;  // element 0 is output position `base`; min(group end, cap) - base elements
    uint8_t* win;   // n + 1 windows of 32 KiB: slot k is the window in front of the group's entry k
    uint64_t base, cap, total;
    uint32_t wrapper, n;
};

// pass 1: one workgroup of one wave per entry: the entry's symbols into sym, the entry's record
__global__ __launch_bounds__(64) void k_inflate_tab(const TItem it, const ic::Entry* __restrict__ ents, ic::Rec* __restrict__ recs) {
    __shared__ ic::Tables s_t;
    const ic::Entry e = ents[blockIdx.x];
    it::Sink o{it.sym, nullptr, it.base, e.pos, it.cap, e.pos};
    ic::Rec r;
    it::it_decode_entry<TabSink>(s_t, it.stream, it.stream_len, it.wrapper, o, e, it.total, r);
    if (threadIdx.x == 0) recs[blockIdx.x] = r;
}

// a thread's part in the window walk of a workgroup of 1024 (it_window_walk.inc): eight of a window's 8192 words, and the barrier
struct WgWalk {
    static constexpr uint32_t turns = it::WIN / 4096;
    uint32_t tid;
    __device__ uint32_t word(uint32_t i) const { return (tid + 1024 * i) * 4; }
    __device__ void step_done(uint32_t) const { __syncthreads(); }
};

// pass 2: ONE workgroup walks the group's entries in order (it_window_walk.inc), two windows ping-ponged in LDS; a step reads the
// window in front of the entry from LDS and the entry's symbols, which pass 1 wrote: no global store of this kernel is read back by
// it.  It stops at the first failing entry and leaves the position up to which pass 3 may write.
__global__ __launch_bounds__(1024) void k_inflate_tab_window(const TItem it, const ic::Entry* __restrict__ ents, const ic::Rec* __restrict__ recs,
                                                             uint64_t* __restrict__ limit_out) {
    __shared__ __attribute__((aligned(16))) uint8_t s_w[2][it::WIN];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = 0; i < it::WIN / 4096; i++) {
        const uint32_t j = (tid + 1024 * i) * 4;
        *reinterpret_cast<uint32_t*>(&s_w[0][j]) = *reinterpret_cast<const uint32_t*>(it.win + j);
    }
    __syncthreads();
    const it::Walk wk{it.sym, ents, recs, it.n, it.base, it.cap, it.win, 0u, it.n, true};  // (every window is made and stored)
    const WgWalk wp{tid};
#include "it_window_walk.inc"
    if (tid == 0) *limit_out = limit;
}

// pass 3: flat over the group's output bytes below cap, 16 a thread
__global__ __launch_bounds__(256) void k_inflate_tab_resolve(const TItem it, const ic::Entry* __restrict__ ents, const uint64_t* __restrict__ limit,
                                                             uint8_t* __restrict__ out) {
    const uint64_t lim = *limit;
    const uint64_t q0 = it.base + ((uint64_t)blockIdx.x * 256 + threadIdx.x) * it::RESOLVE_RUN;
    it::it_resolve_run(it.sym, it.win, ents, it.n, it.base, lim < it.cap ? lim : it.cap, 0, out, q0);
}

}  // namespace mi355

namespace {

// what is wrong with a tabled call's arguments, or nullptr: decided from the arguments alone, before a context or the device is touched
const char* tabled_args(const void* stream, size_t stream_len, int wrapper, const mi355_block_info* blocks, size_t n_blocks, const void* out,
                        size_t out_cap, const size_t* out_len, const mi355_inflate_report* report, uint64_t* total) {
    if (inflate_args_bad(stream, stream_len, wrapper, out, out_cap, out_len, report)) return "inflate: bad argument";
    if (n_blocks > 0x7fffffffull) return "inflate: the table is too long";
    // (entry 0 begins where the stream begins: the first link of the chain that makes a passing table the stream's serial walk)
    if (n_blocks && blocks[0].bit_start != 0) return "inflate: the table's first entry does not begin at bit 0";
    uint64_t sum = 0;
    for (size_t k = 0; k < n_blocks; k++) {
        if (k && blocks[k].bit_start < blocks[k - 1].bit_start) return "inflate: the table's bit_start values do not ascend";
        if (blocks[k].in_bytes > (1ull << 62) - sum) return "inflate: the table's in_bytes do not fit";
        sum += blocks[k].in_bytes;
    }
    *total = sum;
    return nullptr;
}

// MI355_E_ARG of a tabled call; the reason is left for mi355_deflate_last_error when the caller gave a context of its own (the
// default context is not made for the sake of an error)
int tabled_refuse(mi355_deflate_ctx* c, const char* why) {
    if (c) c->err = why;
    return MI355_E_ARG;
}

// one stream with a table, device resident (the arguments have passed tabled_args and the context shard_refusal; total: the sum of
// the table's in_bytes); *valid: the bytes of d_out that hold data
int inflate_tabled_one(mi355_deflate_ctx* c, const uint8_t* d_stream, size_t stream_len, int wrapper, const mi355_block_info* blocks,
                       size_t n_blocks, uint64_t total, uint8_t* d_out, size_t out_cap, size_t* out_len, mi355_inflate_report* report,
                       hipStream_t st, uint64_t* valid) {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<ic::Entry> ents(n_blocks);
    ic::ic_make_entries([&](uint64_t k) { return blocks[k].bit_start; }, [&](uint64_t k) { return blocks[k].in_bytes; }, n_blocks, 0u, ents.data());
    const uint64_t cap = out_cap;
    iw::Rec acc = iw::Rec{ic::V_OK, 0, 0, 0, 0, 0, 0, 0, 0};
    // the largest group's workspace and descriptors, once: the window in front of a group lives in the workspace across groups
    const auto group = [&](uint64_t k0, uint64_t& k1, uint64_t& base, uint64_t& stored) {
        k1 = it::it_group_end([&](uint64_t k) { return blocks[k].in_bytes; }, n_blocks, k0, c->inflate_group_bytes);
        base = ents[k0].pos;
        const uint64_t gend = k1 < n_blocks ? ents[k1].pos : total;
        stored = base < cap ? (gend < cap ? gend : cap) - base : 0;  // the group's positions that hold symbols
    };
    size_t ws = 0, n_max = 0;
    for (uint64_t k0 = 0, k1, base, stored; k0 < n_blocks; k0 = k1) {
        group(k0, k1, base, stored);
        const size_t need = (size_t)(k1 - k0 + 1) * it::WIN + 2 * (size_t)stored + 256;  // [window n + 1] [symbols]
        ws = need > ws ? need : ws;
        n_max = k1 - k0 > n_max ? k1 - k0 : n_max;
    }
    int rc = ensure_buf(c, &c->t_dev, &c->t_dev_cap, ws);
    if (rc) return rc;
    // descriptors: [Entry n] | [limit] [Rec n]
    rc = verify_room(c, align_up(align_up(sizeof(ic::Entry) * n_max, 256) + 256 + sizeof(ic::Rec) * n_max, 256) + 512);
    if (rc) return rc;
    // HIP-event time per launch kind
    StageClocks<4> clk{c->t_ev, c->t_ev_ok, c->t_ms, st, stage_clocks_on(c, total)};
    rc = clk.begin(c);
    if (rc) return rc;
    bool first = true;
    for (uint64_t k0 = 0, k1, base, stored; k0 < n_blocks; k0 = k1) {
        group(k0, k1, base, stored);
        const uint32_t n = (uint32_t)(k1 - k0);
        const size_t sym_at = (size_t)(n + 1) * it::WIN;
        const size_t lim_at = align_up(sizeof(ic::Entry) * n, 256), rec_at = lim_at + 256;
        memcpy(c->v_host, ents.data() + k0, sizeof(ic::Entry) * n);
        const TItem item{d_stream, stream_len, reinterpret_cast<uint16_t*>(c->t_dev + sym_at), c->t_dev, base, cap, total, (uint32_t)wrapper, n};
        const ic::Entry* d_ents = reinterpret_cast<const ic::Entry*>(c->v_dev);
        uint64_t* d_lim = reinterpret_cast<uint64_t*>(c->v_dev + lim_at);
        ic::Rec* d_recs = reinterpret_cast<ic::Rec*>(c->v_dev + rec_at);
        HIPCHK(c, hipMemcpyAsync(c->v_dev, c->v_host, sizeof(ic::Entry) * n, hipMemcpyHostToDevice, st));
        if (first) HIPCHK(c, hipMemsetAsync(c->t_dev, 0, it::WIN, st));  // (nothing refers to the window in front of the stream)
        first = false;
        HIPCHK(c, clk.mark(0));
        hipLaunchKernelGGL(k_inflate_tab, dim3(n), dim3(64), 0, st, item, d_ents, d_recs);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, clk.mark(1));
        hipLaunchKernelGGL(k_inflate_tab_window, dim3(1), dim3(1024), 0, st, item, d_ents, d_recs, d_lim);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, clk.mark(2));
        if (stored) {
            hipLaunchKernelGGL(k_inflate_tab_resolve, dim3(cdiv(stored, 256 * it::RESOLVE_RUN)), dim3(256), 0, st, item, d_ents, d_lim, d_out);
            HIPCHK(c, hipGetLastError());
        }
        HIPCHK(c, clk.mark(3));
        // the group's last window stays on the device as the window in front of the next group
        if (k1 < n_blocks) HIPCHK(c, hipMemcpyAsync(c->t_dev, c->t_dev + (size_t)n * it::WIN, it::WIN, hipMemcpyDeviceToDevice, st));
        HIPCHK(c, hipMemcpyAsync(c->v_host + rec_at, c->v_dev + rec_at, sizeof(ic::Rec) * n, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));  // the one wait of a group
        clk.lap(0, 1, 0), clk.lap(1, 2, 1), clk.lap(2, 3, 2);
        if (!it::it_report(reinterpret_cast<const ic::Rec*>(c->v_host + rec_at), n, acc)) break;
    }
    // the second half of a framed call: the accumulated record goes up as the one record of inflate_run's framed_tail
    if (iw::iw_judged(acc, (uint32_t)wrapper, cap)) {
        if (acc.out_len > VERIFY_MAX_IN) return MI355_E_UNSUPPORTED;  // (what the checksum kernels take)
        const size_t rec_at = align_up(sizeof(IItem), 256);
        rc = verify_room(c, rec_at + sizeof(iw::Rec));
        if (rc) return rc;
        *reinterpret_cast<IItem*>(c->v_host) = IItem{d_stream, stream_len, d_out, cap, c->d_sc, (uint32_t)wrapper, 0u};
        *reinterpret_cast<iw::Rec*>(c->v_host + rec_at) = acc;
        HIPCHK(c, hipMemcpyAsync(c->v_dev, c->v_host, rec_at + sizeof(iw::Rec), hipMemcpyHostToDevice, st));
        rc = framed_tail(c, st, 1, rec_at, [&]() { return launch_sums_one(c, st, wrapper, d_out, acc.out_len); },
                         [&](int k) { return k < 2 ? clk.mark(k) : hipSuccess; });  // (one slot for the checksums and the trailer)
        if (rc) return rc;
        clk.lap(0, 1, 3);
        acc = *reinterpret_cast<const iw::Rec*>(c->v_host + rec_at);
    }
    rc = inflate_rc(iw::iw_report(acc, cap, *report, valid));
    report->ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *out_len = rc == MI355_E_DATA ? (size_t)*valid : (size_t)report->out_len;
    if (rc != MI355_OK) inflate_say(c, *report, rc, "inflate");
    return rc;
}

}  // namespace

extern "C" {

int mi355_inflate_tabled_device(mi355_deflate_ctx* c, const void* d_stream, size_t stream_len, int wrapper, const mi355_block_info* blocks,
                                size_t n_blocks, void* d_out, size_t out_cap, size_t* out_len, mi355_inflate_report* report, void* hip_stream) {
    if (!blocks || !n_blocks) return mi355_inflate_device(c, d_stream, stream_len, wrapper, d_out, out_cap, out_len, report, hip_stream);
    uint64_t total = 0, valid = 0;
    if (const char* why = tabled_args(d_stream, stream_len, wrapper, blocks, n_blocks, d_out, out_cap, out_len, report, &total))
        return tabled_refuse(c, why);
    DefaultGuard dg_;
    if (const int rc = decode_enter(c, dg_)) return rc;
    return inflate_tabled_one(c, reinterpret_cast<const uint8_t*>(d_stream), stream_len, wrapper, blocks, n_blocks, total,
                              reinterpret_cast<uint8_t*>(d_out), out_cap, out_len, report, call_stream(c, hip_stream), &valid);
}

// HIP-event milliseconds of the context's last tabled call per launch kind, summed over its groups: decode, windows, resolve,
// checksums; zeros unless the stage clocks were on (MI355_CFG_STAGE_CLOCKS)
int mi355_inflate_tabled_last_stages(mi355_deflate_ctx* c, float ms[4]) {
    if (!c || !ms) return MI355_E_ARG;
    for (int k = 0; k < 4; k++) ms[k] = c->t_ms[k];
    return MI355_OK;
}

// host buffers: staged_call around the tabled worker
int mi355_inflate_tabled(mi355_deflate_ctx* c, const uint8_t* stream, size_t stream_len, int wrapper, const mi355_block_info* blocks,
                         size_t n_blocks, uint8_t* out, size_t out_cap, size_t* out_len, mi355_inflate_report* report) {
    if (!blocks || !n_blocks) return mi355_inflate(c, stream, stream_len, wrapper, out, out_cap, out_len, report);
    uint64_t total = 0;
    if (const char* why = tabled_args(stream, stream_len, wrapper, blocks, n_blocks, out, out_cap, out_len, report, &total))
        return tabled_refuse(c, why);
    DefaultGuard dg_;
    if (const int rc = decode_enter(c, dg_)) return rc;
    return staged_call(c, stream, stream_len, out, out_cap, [&](const uint8_t* d_stream, uint8_t* d_out, hipStream_t st, uint64_t* valid) {
        return inflate_tabled_one(c, d_stream, stream_len, wrapper, blocks, n_blocks, total, d_out, out_cap, out_len, report, st, valid);
    });
}

}  // extern "C"
