// Index (include/mi355_deflate.h mi355_inflate_index[_device], mi355_inflate_parallel[_device]): the block table of a stream that
// came without one, found on the device, and the tabled inflate run from it.  Two launches and a host link, nothing waits inside a
// kernel (inflate_index.h has the rules; tests/inflindex/ builds the same text for the host):
//   k_index_find  one workgroup of one wave per span: the span's candidate, the first valid non-final dynamic header in it
//   k_index_walk  one workgroup of one wave per span that has a candidate: k_inflate's scalar chain, counting, until it meets the
//                 candidate of a later span, the BFINAL block's end or a failure
// The records come back with one wait; the chain from span 0 is the table.  mi355_inflate_parallel hands it to the tabled driver of
// deflate_table_inflate.inc, which judges it.  The host driver's shared steps are in decode_host.inc.  DESIGN.md section 14.
#include "inflate_index.h"

namespace mi355 {

// the finder's ballot on top of the walker's (never executed) sink
struct IndexOps : WaveSink, ix::Rules {
    static __host__ __device__ uint64_t survivors(const uint8_t* s, uint64_t nbytes, uint64_t base, uint64_t end) {
#if defined(__HIP_DEVICE_COMPILE__)
        const uint64_t bit = base + lane();
        return __ballot(bit < end && ix::ix_lane_prefilter<IndexOps>(s, nbytes, bit));
#else
        return 0;
#endif
    }
};

struct XItem {
    const uint8_t* stream;
    uint64_t stream_len, span, n_spans;
    uint32_t wrapper, pad;
};

__global__ __launch_bounds__(64) void k_index_find(const XItem it, uint64_t* __restrict__ cand) {
    __shared__ ic::Tables s_t;
    const uint64_t c = ix::ix_find_span<IndexOps>(s_t, it.stream, it.stream_len, it.wrapper, blockIdx.x, it.span);
    if (threadIdx.x == 0) cand[blockIdx.x] = c;
}

__global__ __launch_bounds__(64) void k_index_walk(const XItem it, const uint64_t* __restrict__ cand, ix::Walk* __restrict__ recs) {
    __shared__ ic::Tables s_t;
    ix::Walk r;
    ix::ix_walk_span<IndexOps>(s_t, it.stream, it.stream_len, it.wrapper, cand, it.n_spans, it.span, blockIdx.x, cand[blockIdx.x], r);
    if (threadIdx.x == 0) recs[blockIdx.x] = r;
}

}  // namespace mi355

namespace {

static_assert(sizeof(ix::Walk) == 80 && sizeof(mi355_index_walk) == 80, "mi355_index_walk mirrors ix::Walk");
static_assert(ix::SPAN_DEFAULT == 16384 && ix::SPAN_MIN == 256 && ix::SPAN_MAX == (1ull << 30), "the setting's default and range");

// one stream, device resident (the entry has asked shard_refusal): its table (the chain's entries, a failing last link included), its record
int index_run(mi355_deflate_ctx* c, const uint8_t* d_stream, size_t stream_len, int wrapper, hipStream_t st, std::vector<mi355_block_info>& table,
              iw::Rec& acc) {
    const uint64_t S = c->index_span;
    const uint64_t n_spans = ix::ix_n_spans(stream_len, S);  // (of the whole stream: the frame's bytes make a span too many at most)
    if (n_spans > 0x7fffffffull) {
        c->err = "inflate index: the stream has too many spans";
        return MI355_E_UNSUPPORTED;
    }
    // [candidate n] | [Walk n]
    const size_t rec_at = align_up(sizeof(uint64_t) * n_spans, 256);
    int rc = verify_room(c, rec_at + sizeof(ix::Walk) * n_spans);
    if (rc) return rc;
    StageClocks<3> clk{c->x_ev, c->x_ev_ok, c->x_ms, st, stage_clocks_on(c, stream_len)};
    rc = clk.begin(c);
    if (rc) return rc;
    const XItem item{d_stream, stream_len, S, n_spans, (uint32_t)wrapper, 0u};
    uint64_t* d_cand = reinterpret_cast<uint64_t*>(c->v_dev);
    ix::Walk* d_recs = reinterpret_cast<ix::Walk*>(c->v_dev + rec_at);
    HIPCHK(c, clk.mark(0));
    hipLaunchKernelGGL(k_index_find, dim3((uint32_t)n_spans), dim3(64), 0, st, item, d_cand);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, clk.mark(1));
    hipLaunchKernelGGL(k_index_walk, dim3((uint32_t)n_spans), dim3(64), 0, st, item, d_cand, d_recs);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, clk.mark(2));
    HIPCHK(c, hipMemcpyAsync(c->v_host + rec_at, c->v_dev + rec_at, sizeof(ix::Walk) * n_spans, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));  // the one wait of an index
    clk.lap(0, 1, 0), clk.lap(1, 2, 1);
    const auto t0 = std::chrono::steady_clock::now();
    const ix::Walk* w = reinterpret_cast<const ix::Walk*>(c->v_host + rec_at);
    c->x_walks.assign(c->v_host + rec_at, c->v_host + rec_at + sizeof(ix::Walk) * n_spans);
    std::vector<uint64_t> chain;
    ix::ix_link(w, n_spans, [&](uint64_t k) { chain.push_back(k); });
    ix::ix_report(w, chain.data(), chain.size(), acc);
    table.clear();
    for (size_t e = 0; e < chain.size(); e++) {
        const ix::Walk& x = w[chain[e]];
        table.push_back(mi355_block_info{x.btype, e + 1 == chain.size() && x.how == ix::END_FINAL ? 1u : 0u, 0u, 0u, x.count, x.start});
    }
    c->x_ms[2] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return MI355_OK;
}

// the table and the report of an index call handed to the caller
int index_give(mi355_deflate_ctx* c, const std::vector<mi355_block_info>& table, const iw::Rec& acc, mi355_block_info* blocks, size_t cap,
               size_t* n_blocks, mi355_inflate_report* report, std::chrono::steady_clock::time_point t0) {
    uint64_t valid = 0;
    const int rc = inflate_rc(iw::iw_report(acc, ~0ull, *report, &valid));
    report->ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *n_blocks = table.size();
    if (rc == MI355_E_DATA) inflate_say(c, *report, rc, "inflate index");
    if (table.size() > cap) {
        if (cap || blocks) c->err = "inflate index: the table does not fit";
        return MI355_E_OUT_TOO_SMALL;
    }
    for (size_t k = 0; k < table.size(); k++) blocks[k] = table[k];
    return rc;
}

// the index, then the decode it allows, behind the entry's checks: a table of one entry is the one-wave inflate itself
int parallel_one(mi355_deflate_ctx* c, const uint8_t* d_stream, size_t stream_len, int wrapper, uint8_t* d_out, size_t out_cap, size_t* out_len,
                 mi355_inflate_report* report, hipStream_t st, uint64_t* valid) {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<mi355_block_info> table;
    iw::Rec acc;
    int rc = index_run(c, d_stream, stream_len, wrapper, st, table, acc);
    if (rc) return rc;
    if (table.size() < 2) {
        for (int k = 0; k < 4; k++) c->t_ms[k] = 0;
        rc = inflate_one(c, d_stream, stream_len, wrapper, d_out, out_cap, out_len, report, st, valid);
    } else {
        uint64_t total = 0;
        for (const mi355_block_info& b : table) total += b.in_bytes;
        rc = inflate_tabled_one(c, d_stream, stream_len, wrapper, table.data(), table.size(), total, d_out, out_cap, out_len, report, st, valid);
    }
    if (rc == MI355_OK || rc == MI355_E_DATA || rc == MI355_E_OUT_TOO_SMALL)
        report->ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

}  // namespace

extern "C" {

int mi355_inflate_index_device(mi355_deflate_ctx* c, const void* d_stream, size_t stream_len, int wrapper, mi355_block_info* blocks, size_t cap,
                               size_t* n_blocks, mi355_inflate_report* report, void* hip_stream) {
    if (inflate_args_bad(d_stream, stream_len, wrapper, blocks, cap, n_blocks, report)) return tabled_refuse(c, "inflate index: bad argument");
    DefaultGuard dg_;
    if (const int rc = decode_enter(c, dg_)) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<mi355_block_info> table;
    iw::Rec acc;
    if (const int rc = index_run(c, reinterpret_cast<const uint8_t*>(d_stream), stream_len, wrapper, call_stream(c, hip_stream), table, acc))
        return rc;
    return index_give(c, table, acc, blocks, cap, n_blocks, report, t0);
}

// host buffers: the stream staged in; no output buffer and a table to hand back, so stage-out only for an error of index_run's,
// all of which are hard
int mi355_inflate_index(mi355_deflate_ctx* c, const uint8_t* stream, size_t stream_len, int wrapper, mi355_block_info* blocks, size_t cap,
                        size_t* n_blocks, mi355_inflate_report* report) {
    if (inflate_args_bad(stream, stream_len, wrapper, blocks, cap, n_blocks, report)) return tabled_refuse(c, "inflate index: bad argument");
    DefaultGuard dg_;
    if (const int rc = decode_enter(c, dg_)) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    if (const int rc = stage_in(c, stream, stream_len)) return rc;
    std::vector<mi355_block_info> table;
    iw::Rec acc;
    if (const int rc = index_run(c, c->d_in, stream_len, wrapper, c->own_stream, table, acc)) return stage_out(c, rc, nullptr, 0);
    return index_give(c, table, acc, blocks, cap, n_blocks, report, t0);
}

int mi355_inflate_parallel_device(mi355_deflate_ctx* c, const void* d_stream, size_t stream_len, int wrapper, void* d_out, size_t out_cap,
                                  size_t* out_len, mi355_inflate_report* report, void* hip_stream) {
    if (inflate_args_bad(d_stream, stream_len, wrapper, d_out, out_cap, out_len, report)) return tabled_refuse(c, "inflate: bad argument");
    DefaultGuard dg_;
    if (const int rc = decode_enter(c, dg_)) return rc;
    uint64_t valid = 0;
    return parallel_one(c, reinterpret_cast<const uint8_t*>(d_stream), stream_len, wrapper, reinterpret_cast<uint8_t*>(d_out), out_cap, out_len,
                        report, call_stream(c, hip_stream), &valid);
}

// host buffers: staged_call around the index and the decode
int mi355_inflate_parallel(mi355_deflate_ctx* c, const uint8_t* stream, size_t stream_len, int wrapper, uint8_t* out, size_t out_cap,
                           size_t* out_len, mi355_inflate_report* report) {
    if (inflate_args_bad(stream, stream_len, wrapper, out, out_cap, out_len, report)) return tabled_refuse(c, "inflate: bad argument");
    DefaultGuard dg_;
    if (const int rc = decode_enter(c, dg_)) return rc;
    return staged_call(c, stream, stream_len, out, out_cap, [&](const uint8_t* d_stream, uint8_t* d_out, hipStream_t st, uint64_t* valid) {
        return parallel_one(c, d_stream, stream_len, wrapper, d_out, out_cap, out_len, report, st, valid);
    });
}

// HIP-event milliseconds of the context's last index per launch, and the host clock over its link: find, walk, link; the first two
// are zeros unless the stage clocks were on (MI355_CFG_STAGE_CLOCKS)
int mi355_inflate_index_last_stages(mi355_deflate_ctx* c, float ms[3]) {
    if (!c || !ms) return MI355_E_ARG;
    for (int k = 0; k < 3; k++) ms[k] = c->x_ms[k];
    return MI355_OK;
}

// the walkers' records of the context's last index, one per span (a span without a candidate: start == UINT64_MAX, how == 3)
int mi355_inflate_index_last_walks(mi355_deflate_ctx* c, mi355_index_walk* out, size_t cap, size_t* n_spans) {
    if (!c || !n_spans || (!out && cap)) return MI355_E_ARG;
    *n_spans = c->x_walks.size() / sizeof(ix::Walk);
    if (*n_spans > cap) return MI355_E_OUT_TOO_SMALL;
    if (!c->x_walks.empty()) memcpy(out, c->x_walks.data(), c->x_walks.size());
    return MI355_OK;
}

}  // extern "C"
