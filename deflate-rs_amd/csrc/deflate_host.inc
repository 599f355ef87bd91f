// deflate_host.inc -- host side of libmi355deflate.so: workspace, kernel sequencing and the C ABI
// of include/mi355_deflate.h.  Included at the end of deflate_kernels.hip (one translation unit,
// one hipcc invocation).  There is no CPU fallback in here: every encode launches the kernels.
#include <dlfcn.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/mi355_deflate.h"

using namespace mi355;

extern "C" size_t mi355_deflate_bound_ex(size_t n, int wrapper, size_t hdr_len, size_t n_flush);

namespace {

struct Level {
    uint32_t count;   // units on this level
    uint64_t usize;   // positions per unit
    uint16_t* X;      // [count * ZONE]
    uint32_t* E;      // [count]
};

constexpr int MAX_PASSES = 2;
constexpr int N_EV = 7;

}  // namespace

namespace {
struct Arrival;
}
constexpr size_t H_ENDS_CAP = 1024;
constexpr int ARRIVE_MAX = 12;  // pieces a large host input is copied in, at most
constexpr int ARRIVE_MAX_COPY = ARRIVE_MAX;

// ---- the copy engine for finished bytes ----------------------------------------------------------------------------------
// hipMemcpyAsync from the device into page-locked host memory is carried by a copy KERNEL of the runtime when it is queued
// while other copies are in flight (rocprofv3: __amd_rocclr_copyBuffer) -- workgroups that share the chip with the walk of the
// next piece, which loses what the overlap wins (round 4).  The copy engine (SDMA) moves the same bytes at the bus's rate
// without touching a compute unit (tools/probes/d2h_engine.hip: 56 GB/s alone, 45 GB/s beside a host-to-device copy, the
// compute kernel beside it undisturbed), but the runtime does not let a caller pick it.  The HSA runtime underneath does:
// hsa_amd_memory_async_copy between the agent that owns the device buffer and the one that owns the page-locked buffer.
// The library is the one the HIP runtime has loaded already (no new dependency: dlopen with RTLD_NOLOAD); a buffer that is not
// HSA's to copy from (pageable, or locked by hipHostRegister) goes the runtime's way.
struct EngineCopy {
    bool tried = false, ok = false;
    void* lib = nullptr;
    decltype(&hsa_amd_pointer_info) pointer_info = nullptr;
    decltype(&hsa_amd_memory_async_copy) async_copy = nullptr;
    decltype(&hsa_signal_create) signal_create = nullptr;
    decltype(&hsa_signal_destroy) signal_destroy = nullptr;
    decltype(&hsa_signal_store_relaxed) signal_store = nullptr;
    decltype(&hsa_signal_wait_scacquire) signal_wait = nullptr;
    // (optional: the engine of a transfer chosen by the caller.  The runtime spreads transfers that are in flight together over
    // the engines it "prefers" for a direction -- on MI355X engines 1 and 2 for device-to-host, of which engine 1 moves 56 GB/s
    // and engine 2 four (tools/probes/d2h_engine.hip, profiles/r05_d2h_engine_probe.txt): two pieces on their way out at once,
    // or one beside the input's copies, and one of them crawls.  All finished bytes go through the first preferred engine.)
    decltype(&hsa_amd_memory_async_copy_on_engine) async_copy_on_engine = nullptr;
    decltype(&hsa_amd_memory_get_preferred_copy_engine) preferred_engine = nullptr;
    uint32_t d2h_engine = 0;  // engine bit for device-to-host, 0: the runtime chooses
    bool d2h_engine_tried = false;
    hsa_signal_t sig[ARRIVE_MAX_COPY];
    int pending = 0;
    bool load() {
        if (tried) return ok;
        tried = true;
        lib = dlopen("libhsa-runtime64.so.1", RTLD_NOW | RTLD_NOLOAD);
        if (!lib) return false;
        pointer_info = reinterpret_cast<decltype(pointer_info)>(dlsym(lib, "hsa_amd_pointer_info"));
        async_copy = reinterpret_cast<decltype(async_copy)>(dlsym(lib, "hsa_amd_memory_async_copy"));
        signal_create = reinterpret_cast<decltype(signal_create)>(dlsym(lib, "hsa_signal_create"));
        signal_destroy = reinterpret_cast<decltype(signal_destroy)>(dlsym(lib, "hsa_signal_destroy"));
        signal_store = reinterpret_cast<decltype(signal_store)>(dlsym(lib, "hsa_signal_store_relaxed"));
        signal_wait = reinterpret_cast<decltype(signal_wait)>(dlsym(lib, "hsa_signal_wait_scacquire"));
        if (!pointer_info || !async_copy || !signal_create || !signal_destroy || !signal_store || !signal_wait) return false;
        async_copy_on_engine = reinterpret_cast<decltype(async_copy_on_engine)>(dlsym(lib, "hsa_amd_memory_async_copy_on_engine"));
        preferred_engine = reinterpret_cast<decltype(preferred_engine)>(dlsym(lib, "hsa_amd_memory_get_preferred_copy_engine"));
        for (int k = 0; k < ARRIVE_MAX_COPY; k++)
            if (signal_create(1, 0, nullptr, &sig[k]) != HSA_STATUS_SUCCESS) {
                for (int j = 0; j < k; j++) signal_destroy(sig[j]);
                return false;
            }
        ok = true;
        return true;
    }
    // the agents of a device buffer and of a page-locked host buffer the HSA runtime allocated (hipHostMalloc)
    bool agents(const void* dev, const void* host, hsa_agent_t* gpu, hsa_agent_t* cpu) {
        hsa_amd_pointer_info_t pd, ph;
        memset(&pd, 0, sizeof pd);
        memset(&ph, 0, sizeof ph);
        pd.size = sizeof pd;
        ph.size = sizeof ph;
        if (pointer_info(const_cast<void*>(dev), &pd, nullptr, nullptr, nullptr) != HSA_STATUS_SUCCESS) return false;
        if (pointer_info(const_cast<void*>(host), &ph, nullptr, nullptr, nullptr) != HSA_STATUS_SUCCESS) return false;
        if (pd.type != HSA_EXT_POINTER_TYPE_HSA || ph.type != HSA_EXT_POINTER_TYPE_HSA) return false;
        *gpu = pd.agentOwner;
        *cpu = ph.agentOwner;
        return true;
    }
    // one transfer from the device to page-locked host memory, `done` goes below 1 when it has landed
    bool d2h(void* host, hsa_agent_t cpu, const void* dev, hsa_agent_t gpu, size_t bytes, hsa_signal_t done) {
        if (!d2h_engine_tried) {
            d2h_engine_tried = true;
            static const char* const env = getenv("MI355_D2H_ENGINE");  // (development aid: engine number, -1 = the runtime chooses)
            uint32_t mask = 0;
            if (env && *env)
                d2h_engine = atoi(env) >= 0 ? 1u << atoi(env) : 0;
            else if (async_copy_on_engine && preferred_engine && preferred_engine(cpu, gpu, &mask) == HSA_STATUS_SUCCESS && mask)
                d2h_engine = mask & (~mask + 1);  // the first of them
        }
        if (d2h_engine) {
            if (async_copy_on_engine(host, cpu, dev, gpu, bytes, 0, nullptr, done, (hsa_amd_sdma_engine_id_t)d2h_engine, false) == HSA_STATUS_SUCCESS)
                return true;
            d2h_engine = 0;  // (not this way on this box)
        }
        return async_copy(host, cpu, dev, gpu, bytes, 0, nullptr, done) == HSA_STATUS_SUCCESS;
    }
    bool start(void* host, hsa_agent_t cpu, const void* dev, hsa_agent_t gpu, size_t bytes) {
        if (pending >= ARRIVE_MAX_COPY) return false;
        signal_store(sig[pending], 1);
        if (!d2h(host, cpu, dev, gpu, bytes, sig[pending])) return false;
        pending++;
        return true;
    }
    bool wait_all() {
        bool good = true;
        for (int k = 0; k < pending; k++)
            if (signal_wait(sig[k], HSA_SIGNAL_CONDITION_LT, 1, UINT64_MAX, HSA_WAIT_STATE_BLOCKED) != 0) good = false;
        pending = 0;
        return good;
    }
    ~EngineCopy() {
        if (ok)
            for (int k = 0; k < ARRIVE_MAX_COPY; k++) signal_destroy(sig[k]);
    }
};
#include "deflate_bounce.inc"
constexpr size_t HOST_PIECEWISE_FROM = 16u << 20;
constexpr int HOST_PIECES = 8;        // pieces of a host input at most: 1, 2, 3, 3 ... rounds of workgroups, the last takes the rest --
constexpr uint64_t HOST_FIRST_EPOCHS = 64;
constexpr uint64_t HOST_PIECE_ROUNDS = 3;  // the bytes of a piece go back over the bus while the next one is worked on (run_streamed;
                                           // measured: 1,2,3,3,3 / 1,2,4,4,1 18.1 GB/s, 1,3,4,3,1 / 2,3,3,3,1 / 1,2,2,2,2,2,1 17.7, 1,4,6,1 17.1)
struct mi355_deflate_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    std::string err;
    // one big device allocation, carved per encode
    uint8_t* ws = nullptr;
    size_t ws_cap = 0;
    // staging for the host-buffer API
    uint8_t* d_in = nullptr;
    size_t d_in_cap = 0;
    uint8_t* d_out = nullptr;
    size_t d_out_cap = 0;
    uint8_t* d_crc = nullptr;  // mi355_crc32_device: per-chunk CRCs (its own buffer: the workspace may belong to a live shard)
    size_t d_crc_cap = 0;
    DevScalars* d_sc = nullptr;
    DevScalars* h_sc = nullptr;  // pinned
    uint32_t* h_ends = nullptr;  // pinned staging for the segment ends of a call (H_ENDS_CAP entries)
    hipStream_t fill = nullptr;  // the output buffer is cleared here, beside the match stage (run_encode)
    hipEvent_t ev_fill[2] = {nullptr, nullptr};
    hipStream_t copy_stream = nullptr;  // host-buffer calls: the input arrives in pieces while the first ones are worked on
    hipStream_t out_stream = nullptr;   // ... and the output leaves in pieces while the later ones are worked on (run_streamed)
    EngineCopy engine;                  // ... on the copy engine, when the caller's buffer allows
    int host_streaming = 1;             // MI355_CFG_HOST_STREAMING
    Bounce* bounce = nullptr;           // pageable caller buffers: host threads and page-locked slots (deflate_bounce.inc), made when
                                        // the first such call of 4 MiB or more comes
    int host_bounce = 1;                // MI355_CFG_HOST_BOUNCE
    int host_threads = 0;               // MI355_CFG_HOST_THREADS (0: by the host's core count)
    bool bounce_on = false;             // a session of the bounce threads is open (closed by bounce_close before the call returns)
    uint32_t host_path = 0;             // how the last host-buffer call moved its bytes (mi355_deflate_info.host_path)
    int multi_stitch = 0;               // MI355_CFG_MULTI_STITCH (of rank 0's context of a mi355_multi)
    int steps_in_emit = 1;              // MI355_CFG_STEPS_IN_EMIT
    const Arrival* next_arrival = nullptr;  // the next mi355_shard_begin's input is still arriving (deflate_multi.inc); taken once
    hipStream_t blk_stream = nullptr;   // ... a piece's parse, block and pack stages run here, beside the walk of the next piece
    hipEvent_t ev_plan[ARRIVE_MAX], ev_pack[ARRIVE_MAX], ev_walk[ARRIVE_MAX];
    bool out_ok = false;
    uint8_t* h_piece = nullptr;         // pinned: the device scalars as they stand behind every piece's block plan
    hipEvent_t arrive[ARRIVE_MAX];
    bool arrive_ok = false;
    hipEvent_t ev[MAX_PASSES][N_EV];
    bool ev_ok = false;
    mi355_deflate_info info;
    // the stage clocks of the last run_encode are read off its events when somebody asks (mi355_deflate_last_info), not at the
    // end of every call
    int pend_passes = 0;
    bool pend_clocks = true;  // the events between the stages were recorded (else: the first and the last only)
    int stage_clocks = 0;      // MI355_CFG_STAGE_CLOCKS: 0 never (default), 1 always, 2 from STAGE_CLOCKS_FROM bytes on
    int pend_last[MAX_PASSES] = {0, 0};
    // where the last encode left its block plan (diagnostics)
    const BlockPlan* last_plan = nullptr;
    const uint32_t* last_nt = nullptr;
    const uint32_t* last_bstart = nullptr;
    uint32_t last_nb = 0;
    uint64_t last_T = 0;
    uint64_t last_bit_base = 0;
    uint32_t last_crc = 0;
    uint32_t n_cu = 0;  // compute units of the device (k_match tile size)
    int sort_mode = 0;  // k_sort<MODE>: 1 once the device has passed k_lds_order_test -- ranks from returning LDS atomics -- else 0
    bool lds_order_ok = false;  // the answer of k_lds_order_test
    int sort_break = 0;         // (MI355_DEBUG_HOOKS builds: k_sort<1> mis-ranks on purpose)
#ifdef MI355_DEBUG_HOOKS
    int force_swz = 0;                  // mi355_debug_force_swz: 0 product, 1 every epoch with J >= 1024 marked, 2 none
    const uint16_t* dbg_sorted = nullptr;   // the tables the last single-pass call left in the workspace (mi355_debug_sort_tables)
    const uint16_t* dbg_buckets = nullptr;
    uint64_t dbg_epochs = 0;
#endif
    uint32_t last_spec_bad = 0;
    bool reuse_tables = false;  // the encode that follows is the second attempt at an input whose match table and restart steps
                                // are still in the workspace (run_encode after a failed speculative parse)
    uint32_t q1_last_on = 0;    // the last single-pass encode re-warmed two hashes (Q1) ...
    uint64_t q1_last_pos = 0;   // ... at this position (the streaming handle latches it for the ranges behind an early flush)
    int spec_pause = 0;         // encodes left that parse the exact way: the speculative segment entries (k_emit<true>) failed
                                // on this context's last input -- long periodic data -- and would probably fail again
    uint64_t long_range = 512ull << 20;     // deflate_long.inc: bytes per range
    uint64_t long_from = (1ull << 30) + 1;  // one-shot inputs of at least this many bytes go through ranges
    struct mi355_shard* shard_cache = nullptr;  // deflate_shard.inc: the shard object of the last sharded encode
    struct mi355_shard* live_shard = nullptr;   // a shard between _begin and _end: its tokens and tables live in the workspace,
                                                // so no other encode may run on this context meanwhile (MI355_E_STATE)
    // deflate_batch.inc: the descriptors and running sums of a launch set and the items' scalars (device; page-locked staging)
    uint8_t* b_dev = nullptr;
    size_t b_dev_cap = 0;
    uint8_t* b_host = nullptr;
    size_t b_host_cap = 0;
    uint64_t batch_bytes = 256ull << 20;  // MI355_CFG_BATCH_BYTES: input bytes of one launch set
    mi355_batch_info batch = {};          // mi355_deflate_last_batch_info
    // deflate_verify.inc: the items, entries and records of a verify call (device; page-locked staging)
    uint8_t* v_dev = nullptr;
    size_t v_dev_cap = 0;
    uint8_t* v_host = nullptr;
    size_t v_host_cap = 0;
    // deflate_table_inflate.inc: the symbols and the resolved windows of a group of entries
    uint8_t* t_dev = nullptr;
    size_t t_dev_cap = 0;
    uint64_t inflate_group_bytes = 256ull << 20;  // MI355_CFG_INFLATE_GROUP_BYTES: output bytes of one group of entries
    hipEvent_t t_ev[4] = {};                      // between the launch kinds of a tabled inflate, when the stage clocks are on
    bool t_ev_ok = false;
    float t_ms[4] = {};                           // mi355_inflate_tabled_last_stages: decode, windows, resolve, checksums
    uint64_t seek_cut_bytes = 0;  // MI355_CFG_INFLATE_SEEK_CUT_BYTES: output bytes between the cuts of a seek handle's entries; 0: none
    uint64_t seek_cut_walker = 0; // MI355_CFG_INFLATE_SEEK_CUT_WALKER: 1 = the build finds the cuts in a launch of its own (measuring aid)
    hipEvent_t sk_ev[5] = {};     // around the launches of a seek read's set, when the stage clocks are on
    bool sk_ev_ok = false;
    float sk_ms[4] = {};          // mi355_inflate_seek_last_read_stages: pass 1, flatten, windows, resolve
    // deflate_index_inflate.inc: the block table of a stream nobody kept one for
    uint64_t index_span = 16384;  // MI355_CFG_INFLATE_INDEX_SPAN_BYTES: compressed bytes of one span (ix::SPAN_DEFAULT)
    hipEvent_t x_ev[3] = {};      // around the two launches of an index, when the stage clocks are on
    bool x_ev_ok = false;
    float x_ms[3] = {};           // mi355_inflate_index_last_stages: find, walk, host link
    std::vector<uint8_t> x_walks; // mi355_inflate_index_last_walks: the last index's records, 80 bytes a span
    // deflate_members_inflate.inc: the members of a gzip file
    uint64_t member_span = 65536;  // MI355_CFG_INFLATE_MEMBER_SPAN_BYTES: compressed bytes of one span (im::SPAN_DEFAULT)
    uint8_t* m_dev = nullptr;      // the candidates, the walkers' records and the chain's walkers of a call
    size_t m_dev_cap = 0;
    uint8_t* m_rows = nullptr;     // the rows of a fill, or the rows and records of a chain launch
    size_t m_rows_cap = 0;
    hipEvent_t m_ev[2] = {};       // around a launch of a members call, when the stage clocks are on
    bool m_ev_ok = false;
    float m_ms[6] = {};            // mi355_inflate_members_last_stages: find, walk, fill, member decode, chain decode, checksums
    std::vector<uint64_t> m_cands; // mi355_inflate_members_last_walks: the last call's candidates and the records of its first
    std::vector<uint8_t> m_walks;  // walk, 40 bytes a span
    // deflate_bigmembers_inflate.inc: the large plain members of a gzip file
    uint64_t member_parallel = 65536;  // MI355_CFG_INFLATE_MEMBER_PARALLEL_BYTES: bytes left for a discovery (ib::PAR_DEFAULT); 0: off
    uint8_t* mp_dev = nullptr;         // the head, the carried window, the candidates and the walkers' records of a discovery
    size_t mp_dev_cap = 0;
    hipEvent_t mp_ev[4] = {};          // between the launches of a discovery round and of a group, when the stage clocks are on
    bool mp_ev_ok = false;
    float mp_ms[5] = {};               // mi355_inflate_members_last_parallel_stages: find, walk, decode, windows, resolve
    uint64_t mp_stats[6] = {};         // mi355_inflate_members_last_parallel
    // deflate_bgzf.inc: the arena the members of a BGZF encode are packed into, the table, offsets and rows behind them (device;
    // page-locked staging of the one copy back), and the file of a host-buffer call
    uint8_t* bz_arena = nullptr;
    size_t bz_arena_cap = 0;
    uint8_t* bz_tab = nullptr;
    size_t bz_tab_cap = 0;
    uint8_t* bz_host = nullptr;
    size_t bz_host_cap = 0;
    uint8_t* bz_out = nullptr;
    size_t bz_out_cap = 0;
    hipEvent_t bz_ev[4] = {};          // around the packed encode and the two launches, when the stage clocks are on
    bool bz_ev_ok = false;
    float bz_ms[3] = {};               // mi355_bgzf_last_stages: packed encode, place, gather
    // deflate_bgzf_read.inc: BGZF reads (their scratch slots live in t_dev, their descriptors in v_dev)
    hipEvent_t br_ev[5] = {};          // around the launches of a read's set, when the stage clocks are on
    bool br_ev_ok = false;
    float br_ms[3] = {};               // mi355_bgzf_last_read_stages: decode and clip, checksums, trailers
    uint64_t br_stats[6] = {};         // mi355_bgzf_last_read
};
void shard_destroy(struct mi355_shard* s);
// deflate_long.inc: inputs of any length and never-flushed streams, walked in ranges
struct mi355_deflate_stream;
struct LongEnc;
static int stream_pump(mi355_deflate_stream* s);
static int stream_long_end(mi355_deflate_stream* s, int mode);
static bool stream_long_eligible(const mi355_deflate_stream* s);
static void long_free(LongEnc* L);
static int encode_long(mi355_deflate_ctx* c, const uint8_t* d_in, const uint8_t* h_in, uint64_t n, const mi355_deflate_opts* o,
                       uint8_t* d_out, uint8_t* h_out, size_t out_cap, size_t* out_len, const uint8_t* gz_hdr, size_t gz_len);
static uint64_t long_from(const mi355_deflate_ctx* c);
// a call goes through ranges when it is long (a sync-flush chunk too: its last range ends in the sync marker)
static bool goes_long(const mi355_deflate_ctx* c, uint64_t n, const mi355_deflate_opts* o) {
    (void)o;
    return n >= long_from(c);
}

namespace {

// GzBuilder::new().into_header() of crate gzip-header 1.0 (not in the tree; RFC 1952 member header with
// no flags, mtime 0, XFL 0, OS 255 = unknown).  Callers that have the real crate pass its bytes instead.
const uint8_t kBlankGzipHeader[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff};

int fail_hip(mi355_deflate_ctx* c, const char* what, hipError_t e) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    if (c) c->err = buf;
    return MI355_E_HIP;
}
#define HIPCHK(c, x)                                        \
    do {                                                    \
        hipError_t e__ = (x);                               \
        if (e__ != hipSuccess) return fail_hip(c, #x, e__); \
    } while (0)

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct Carver {
    uint8_t* base;
    size_t off = 0;
    template <class T>
    T* take(size_t count) {
        off = align_up(off, 256);
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += count * sizeof(T);
        return p;
    }
};

struct Workspace {
    uint16_t* sorted;    // k_sort: positions of every epoch by (hash, position), one epoch of pad in front
    uint16_t* buckets;   // k_sort: bucket starts per epoch (BSTRIDE entries each)
    uint16_t* link;
    uint32_t* M;
    uint32_t* Mq;
    uint16_t* adv;
    std::vector<Level> levels;
    uint32_t* tokbuf;
    uint32_t* cnt;
    uint32_t* base;
    uint32_t* dtok;
    uint32_t* bstart;
    uint32_t* q13;
    uint32_t* ll_freq;
    uint32_t* d_freq;
    BlockHeader* hdr;
    BlockPlan* plan;
    BlockTab tab;        // per block: token range, sync flag
    uint32_t* seg_ends;  // segment ends (device copy), m entries
    uint32_t* tend;      // tokens before each segment end, m entries
    uint32_t* pb;        // blocks before each segment, m + 1 entries
    uint32_t* rewarm;    // hash re-warm points of the streaming API (stages.h HashOverride), <= m entries
    uint32_t* quirks;    // skew points, then holes (stages.h HashOverride)
    uint32_t* scan_part; // token count of every 1024 segments (k_scan_a -> k_scan_b)
    uint32_t* xs;        // speculative parse: where every segment was left (K0 entries)
    uint32_t* badmap;    // speculative parse: a bit per segment whose entry did not check out, and the list of them
    uint32_t* fixlist;
    uint32_t* crc_part;  // CRC-32 of every 512-byte chunk (gzip)
    uint8_t* gz_hdr;     // device copy of the caller's gzip header
    uint32_t K0, nb_max;
    size_t bytes;
};

// Lay out (or just size, when base == nullptr) the workspace for n input bytes.
Workspace carve(uint8_t* base, uint64_t n, bool need_q, size_t m = 1, size_t gz_len = 0, size_t n_quirks = 0) {
    Workspace w;
    Carver c{base};
    uint64_t np = n + 64;
    const uint64_t n_ep = (n + WINDOW_SIZE - 1) / WINDOW_SIZE;
    w.sorted = c.take<uint16_t>((n_ep + 1) * WINDOW_SIZE + 64);
    w.buckets = c.take<uint16_t>(n_ep * BSTRIDE + 64);
    w.link = c.take<uint16_t>(np + LINKS_PAD);
    w.M = c.take<uint32_t>(np);
    w.Mq = need_q ? c.take<uint32_t>(np) : nullptr;
    w.adv = c.take<uint16_t>(np + LINKS_PAD);  // doubles as hl (hash + publish flag) of k_links
    w.K0 = (uint32_t)((n + SEG - 1) / SEG);
    uint32_t cnt = w.K0;
    uint64_t usize = SEG;
    while (cnt > 0) {
        Level L;
        L.count = cnt;
        L.usize = usize;
        L.X = c.take<uint16_t>((size_t)cnt * ZONE);
        L.E = c.take<uint32_t>(cnt);
        w.levels.push_back(L);
        if (cnt == 1) break;
        cnt = (cnt + FAN - 1) / FAN;
        usize *= FAN;
    }
    w.tokbuf = c.take<uint32_t>((size_t)w.K0 * TOK_SLOT + 64);
    w.cnt = c.take<uint32_t>((size_t)w.K0 + 64);
    w.base = c.take<uint32_t>((size_t)w.K0 + 64);
    w.scan_part = c.take<uint32_t>((size_t)w.K0 / 1024 + 2 + 2 * PIECES_MAX);
    w.xs = c.take<uint32_t>((size_t)w.K0 + 64);
    w.badmap = c.take<uint32_t>((size_t)w.K0 / 32 + 16);
    w.fixlist = c.take<uint32_t>((size_t)2 * FIX_MAX * PIECES_MAX);
    w.dtok = c.take<uint32_t>(np);
    w.nb_max = (uint32_t)(n / MAX_BUFFER_LENGTH + m);  // every segment ends with a block of its own
    size_t nbx = (size_t)w.nb_max + 2;
    w.tab.t0 = c.take<uint32_t>(nbx);
    w.tab.nt = c.take<uint32_t>(nbx);
    w.tab.sync = c.take<uint32_t>(nbx);
    w.seg_ends = c.take<uint32_t>(m + 1);
    w.tend = c.take<uint32_t>(m + 1);
    w.pb = c.take<uint32_t>(m + 2);
    w.rewarm = c.take<uint32_t>(m + 1);
    w.quirks = c.take<uint32_t>(n_quirks + 8);  // (sized from the lists themselves: a trim of the stream's history
                                                 // drops flush points but keeps every later skew point and hole)
    w.bstart = c.take<uint32_t>(nbx);
    w.q13 = c.take<uint32_t>(nbx);
    w.ll_freq = c.take<uint32_t>(nbx * 288 * PSPLIT);
    w.d_freq = c.take<uint32_t>(nbx * 32 * PSPLIT);
    w.hdr = c.take<BlockHeader>(nbx);
    w.plan = c.take<BlockPlan>(nbx);
    w.crc_part = gz_len ? c.take<uint32_t>((size_t)(n / CRC_CHUNK) + 2) : nullptr;
    w.gz_hdr = gz_len ? c.take<uint8_t>(gz_len + 16) : nullptr;
    w.bytes = align_up(c.off, 256);
    return w;
}

int ensure_ws(mi355_deflate_ctx* c, size_t bytes) {
    if (bytes <= c->ws_cap) return MI355_OK;
    c->last_plan = nullptr;
    c->last_nb = 0;
#ifdef MI355_DEBUG_HOOKS
    c->dbg_epochs = 0;  // (the tables' memory goes away below)
#endif
    if (c->ws) {
        (void)hipFree(c->ws);
        c->ws = nullptr;
        c->ws_cap = 0;
    }
    size_t want = bytes + bytes / 8;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&c->ws), want);
    if (e != hipSuccess) {
        want = bytes;
        e = hipMalloc(reinterpret_cast<void**>(&c->ws), want);
    }
    if (e != hipSuccess) return fail_hip(c, "hipMalloc(workspace)", e);
    c->ws_cap = want;
    return MI355_OK;
}

int ensure_buf(mi355_deflate_ctx* c, uint8_t** p, size_t* cap, size_t bytes) {
    if (bytes <= *cap) return MI355_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(p), bytes));
    *cap = bytes;
    return MI355_OK;
}

#ifndef MI355_FORCE_IDENT
#ifndef MI355_IDENT_EPOCHS
#define MI355_IDENT_EPOCHS 3  // (2: the state before tests/golden/identity_hop.bin existed -- that test then fails, which is its point)
#endif
#define MI355_FORCE_IDENT 0  // test builds: always walk the identity hops (must not change any output)
#endif

// Tile size of a k_match launch: as large as the LDS allows, then shrunk so that the tiles come in whole
// rounds over the CUs (a last round that fills a fifth of the chip costs a whole round), and for
// small inputs so that every CU gets a tile.
uint32_t match_tile(uint64_t n, uint32_t n_cu) {
    if (n_cu == 0) n_cu = 256;
    const uint64_t per_round = (uint64_t)n_cu * MT;
    const uint64_t rounds = n ? (n + per_round - 1) / per_round : 1;
    uint64_t mt = (n + rounds * n_cu - 1) / (rounds * n_cu);
    mt = (mt + 63) / 64 * 64;
    if (mt < 2048) mt = 2048;
    if (mt > MT) mt = MT;
    return (uint32_t)mt;
}

uint32_t cdiv(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

// A host input on its way to the device in pieces: ev[k] fires when the bytes of the first upto[k] epochs (and the
// look-ahead behind them) are there; the last piece is the whole input.  n = 0: nothing to wait for.
struct Arrival {
    const hipEvent_t* ev = nullptr;
    int n = 0;
    uint32_t upto[ARRIVE_MAX] = {};
    Bounce* gate = nullptr;  // pageable input: the events are recorded by the bounce threads as they get there (arrival_wait)
};

Bounce* bounce_for(mi355_deflate_ctx* c, const void* host, uint64_t bytes);
void bounce_open(mi355_deflate_ctx* c);

// `st` waits for piece k of an arriving input.  A pageable input's events are recorded by other threads as the chunks get
// queued: a wait on an event that nobody has recorded yet would be no wait at all, so the calling thread first waits (and
// copies chunks itself) until that has happened.
int arrival_wait(mi355_deflate_ctx* c, hipStream_t st, const Arrival& ar, int k) {
    if (ar.gate && !ar.gate->in_wait_recorded(k)) {
        c->err = "host threads: a copy of the input failed";
        return MI355_E_HIP;
    }
    HIPCHK(c, hipStreamWaitEvent(st, ar.ev[k], 0));
    return MI355_OK;
}

// k_match3 runs one workgroup per CU, and a workgroup costs a fixed part (the window staged in LDS, the first dependent loads
// of a batch: F) besides its batches (16 dual batches per wave for a whole epoch, t each; F = 1.35 t measured at the default
// level: pg11.txt 357 / 129 / 83 us with 1 / 4 / 16 parts per epoch).  The epochs of a small input are cut in parts so that the
// rounds of workgroups times what one of them takes is least -- more than sixteen parts leave waves without a batch.
// (Before: parts until there were four rounds of workgroups.  2 MB: 16 parts, 148 us -> 4 parts, 97 us; 16 MB: 3 parts,
// 649 us -> whole epochs, 584 us.  The model's unit comes out at 16-17 us for every size and part count measured, 0.17 to
// 32 MB: the rounds are real -- 306 epochs in whole take two of them, 568 us, in four parts each five short ones, 438 us.)
#ifndef MI355_M3_SPLIT_MAX
#define MI355_M3_SPLIT_MAX 16
#endif
uint32_t match3_split(uint64_t n_ep, uint32_t n_cu) {
    if (n_cu == 0) n_cu = 256;
    if (n_ep == 0) return 1;
    double best = 0;
    uint32_t best_s = 1;
    for (uint32_t s = 1; s <= MI355_M3_SPLIT_MAX; s++) {
        const uint64_t rounds = (n_ep * s + n_cu - 1) / n_cu;
        const double cost = (double)rounds * (1.35 + 16.0 / s);
        if (s == 1 || cost < best - 1e-9) {
            best = cost;
            best_s = s;
        }
    }
    return best_s;
}

uint32_t* sort_bad_flag(mi355_deflate_ctx* c) { return &reinterpret_cast<DevState*>(c->d_sc)->sort_bad; }
// Did the walk meet a bucket out of order (k_match3)?  Call after a wait that brought *c->h_sc (a DevState) up to date.  Yes:
// the context sorts with ballot ranks from now on and the caller runs its tables again.
// Did a segment's speculative entry turn out wrong (k_emit<true>, k_scan_a)?  Same protocol.  Yes: the caller parses again with
// exit tables and the table tree, and so do this context's next encodes (data of that kind comes in runs).
constexpr int SPEC_PAUSE = 16;
bool spec_entries_failed(mi355_deflate_ctx* c) {
    DevState* h = reinterpret_cast<DevState*>(c->h_sc);
    if (!h->spec_bad) return false;
    c->last_spec_bad = h->spec_bad;
    c->spec_pause = SPEC_PAUSE + 1;
    (void)hipMemsetAsync(&reinterpret_cast<DevState*>(c->d_sc)->spec_bad, 0, sizeof(uint32_t), c->own_stream);
    (void)hipStreamSynchronize(c->own_stream);
    h->spec_bad = 0;
    return true;
}

// (the state change alone: the batched call keeps the flag per item and finds it cleared with the items' states)
void sort_fell_back(mi355_deflate_ctx* c) {
    c->sort_mode = 0;
    c->lds_order_ok = false;
    c->sort_break = 0;
}
bool sort_order_failed(mi355_deflate_ctx* c) {
    if (!reinterpret_cast<const DevState*>(c->h_sc)->sort_bad) return false;
    sort_fell_back(c);
    (void)hipMemsetAsync(sort_bad_flag(c), 0, sizeof(uint32_t), c->own_stream);
    (void)hipStreamSynchronize(c->own_stream);
    reinterpret_cast<DevState*>(c->h_sc)->sort_bad = 0;
    return true;
}

// The clocks of the stages (mi355_deflate_info::stage_ms) are events between the kernels of a call -- five of them, 29 us of idle
// queue: a tenth of a 167 KB call, 0.7 % of a 100 MB one -- and a call takes them only when asked (MI355_CFG_STAGE_CLOCKS).
constexpr uint64_t STAGE_CLOCKS_FROM = 32ull << 20;
#ifndef MI355_STATE_KERNEL
#define MI355_STATE_KERNEL 1
#endif
bool stage_clocks_on(const mi355_deflate_ctx* c, uint64_t n) { return c->stage_clocks == 1 || (c->stage_clocks == 2 && n >= STAGE_CLOCKS_FROM); }

// ---- what the drivers share: the single pass, the streamed host call, the shard phases, the batched call -----------------------
// Each of the launch_* functions queues launches on the stream it is given and decides nothing about the call.

// The parse settings of a call's options.  Quirk Q3 (lazy_if_less_than < 3 with Lazy matching) is refused.
int parse_cfg(mi355_deflate_ctx* c, const mi355_deflate_opts* o, ParseCfg* cfg) {
    cfg->checks = o->max_hash_checks;
    cfg->lazy_lt = o->lazy_if_less_than < 32768 ? o->lazy_if_less_than : 32768;  // deflate_state.rs:105
    cfg->mode = o->matching_type == 0 ? MODE_GREEDY : (o->max_hash_checks == 0 ? MODE_RLE : MODE_LAZY);  // lz77.rs:211-231
    cfg->use_quarter = (cfg->mode == MODE_LAZY && cfg->lazy_lt > 32) ? 1 : 0;
    if (cfg->mode == MODE_LAZY && cfg->lazy_lt < 3) {
        c->err = "lazy_if_less_than < 3 with Lazy matching is not supported (SURVEY A.4 Q3)";
        return MI355_E_UNSUPPORTED;
    }
    return MI355_OK;
}
// (the level builds chains and walks them; the budget of the quarter table; whether that table is walked at all)
inline bool cfg_hashing(const ParseCfg& cfg) { return cfg.mode != MODE_RLE && cfg.checks > 0; }
inline uint32_t cfg_cq(const ParseCfg& cfg) { return cfg.use_quarter ? (cfg.checks >> 2) : 0; }
inline bool cfg_has_q(const ParseCfg& cfg) { return cfg.use_quarter && cfg_cq(cfg); }

// no re-warm, no flush points, no write-pattern quirks: every call but a stream's and a second pass
constexpr HashOverride NO_HASH_OVERRIDE = {0, 0, 0, 0, 0, nullptr, 0, nullptr, 0, nullptr};

// ---- after the wait ----
void info_from_scalars(mi355_deflate_info* info, const DevScalars& s) {
    info->n_tokens = s.T;
    info->n_blocks = s.nb;
    info->n_stored = s.n_stored;
    info->n_fixed = s.n_fixed;
    info->n_dynamic = s.n_dynamic;
    info->q13_hits = s.q13_hits;
    info->spec_repaired = 0;
    for (uint32_t k = 0; k < PIECES_MAX; k++) info->spec_repaired += s.n_fix[k];
}
// (bytes of the stream with its frame: stages.h stream_bytes, shared with kb_place)

// the `dbl` argument of k_sort / kb_sort: bit 0 = entries as 2 * position; the further bits are read by the test build only
// (bit 1: mi355_debug_break_sort, ranks from atomics only; bits 2 and 3: mi355_debug_force_swz)
inline uint32_t sort_dbl(const mi355_deflate_ctx* c, int mode) {
#ifdef MI355_DEBUG_HOOKS
    return 1u | ((mode == 1 && c->sort_break) ? 2u : 0u) | (c->force_swz == 1 ? 4u : 0u) | (c->force_swz == 2 ? 8u : 0u);
#else
    return 1u | ((mode == 1 && c->sort_break) ? 2u : 0u);
#endif
}
void launch_sort(mi355_deflate_ctx* c, hipStream_t st, uint32_t epochs, const uint8_t* d_in, uint32_t n32, const HashOverride& ov,
                 uint16_t* S, uint16_t* B, uint32_t e0, const SortInit* init = nullptr) {
    if (epochs == 0) return;
    const SortInit in0 = init ? *init : SortInit{nullptr, 0u, nullptr, 0u};
    if (c->sort_mode == 1)
        hipLaunchKernelGGL(k_sort<1>, dim3(epochs), dim3(1024), 0, st, d_in, n32, ov, S, B, e0, sort_dbl(c, 1), in0);
    else
        hipLaunchKernelGGL(k_sort<0>, dim3(epochs), dim3(1024), 0, st, d_in, n32, ov, S, B, e0, sort_dbl(c, 0), in0);
}

// The walk's plan for `n_ep` epochs: `split` workgroups per epoch (match3_split), and `single` for the launch that walks both
// tables at once (a small call, the batched call): twice the parts and ONE batch a wave instead of a pair where that still is one
// round of workgroups.  A small call's walk
// is the latency of its slowest lane's chain of step blocks, and a wave with one fibre steps through it at twice the
// rate (pg11.txt 0.213 -> 0.202 ms; MI355_M3_SINGLE=0: the pair, a measuring aid)
struct WalkPlan {
    uint32_t split;
    bool single;
};
WalkPlan walk_plan(uint64_t n_ep, uint32_t n_cu) {
    static const bool single_env = !(getenv("MI355_M3_SINGLE") && getenv("MI355_M3_SINGLE")[0] == '0');
    const uint32_t cus = n_cu ? n_cu : 256u;
    const uint32_t split = match3_split(n_ep, n_cu);
    return WalkPlan{split, single_env && split >= MI355_M3_SPLIT_MAX && n_ep * split * 2 <= cus};
}

// the walk over `ne` sorted epochs from e_first on (split: workgroups per epoch; the results go out in the order of the sorted
// arrays and are turned round at the end of an epoch when an epoch is one workgroup's)
void launch_walk(mi355_deflate_ctx* c, hipStream_t st, const uint8_t* d_in, uint32_t n32, const uint16_t* S, Workspace& w, const ParseCfg& cfg,
                 int aligned16, SegEnds sg, const HashOverride& ov, uint32_t e_first, uint32_t ne) {
    const WalkPlan plan = walk_plan(ne, c->n_cu);
    const uint32_t split = plan.split, cq = cfg_cq(cfg);
    const bool has_q = cfg_has_q(cfg);
    // (k_match3 borrows the token arrays, which nothing has written yet, for the results in sorted order: 4 B per position each)
    uint32_t* const borrowed = walk_borrows(w.tokbuf, w.K0);
    uint32_t* const ms = split == 1 ? borrowed : nullptr;
    uint32_t* const mqs = split == 1 ? w.dtok : nullptr;
    if (MI355_SWZ_BANKS && ne * split <= M3_BOTH_UNITS) {  // small: both tables in one launch
        const bool single = plan.single;
        const uint32_t sp = single ? split * 2 : split;
        uint32_t* const ms1 = sp == 1 ? borrowed : nullptr;
        uint32_t* const mqs1 = sp == 1 ? w.dtok : nullptr;
#define MI355_BOTH(Q, SNG, mq, mqs, cqv)                                                                                       \
    hipLaunchKernelGGL((k_match3_both<Q, SNG>), dim3(ne * sp), dim3(M3T), 0, st, d_in, n32, S, w.buckets, w.M, mq, cfg.checks, cqv, \
                       aligned16, sg, ov, e_first, sp, ms1, mqs, sort_bad_flag(c))
        if (has_q && single)
            MI355_BOTH(true, true, w.Mq, mqs1, cq);
        else if (has_q)
            MI355_BOTH(true, false, w.Mq, mqs1, cq);
        else if (single)
            MI355_BOTH(false, true, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u);
        else
            MI355_BOTH(false, false, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u);
#undef MI355_BOTH
        return;
    }
    if (has_q)
        hipLaunchKernelGGL(k_match3<true>, dim3(ne * split), dim3(M3T), 0, st, d_in, n32, S, w.buckets, w.M, w.Mq, cfg.checks, cq,
                           aligned16, sg, ov, e_first, split, ms, mqs, sort_bad_flag(c));
    else
        hipLaunchKernelGGL(k_match3<false>, dim3(ne * split), dim3(M3T), 0, st, d_in, n32, S, w.buckets, w.M, (uint32_t*)nullptr,
                           cfg.checks, 0u, aligned16, sg, ov, e_first, split, ms, (uint32_t*)nullptr, sort_bad_flag(c));
    // the epochs k_sort marked for the permuted pair table (rows of records: their lanes meet on a few LDS banks), a workgroup per
    // compute unit
    if (MI355_SWZ_BANKS) {
        const uint32_t units = ne * split, cus = c->n_cu ? c->n_cu : 256u;
        const uint32_t grid = (MI355_SWZ_PERSISTENT && units > cus) ? cus : units;
        if (has_q)
            hipLaunchKernelGGL(k_match3_swz<true>, dim3(grid), dim3(M3T), 0, st, d_in, n32, S, w.buckets, w.M, w.Mq, cfg.checks, cq,
                               aligned16, sg, ov, e_first, units, split, ms, mqs, sort_bad_flag(c));
        else
            hipLaunchKernelGGL(k_match3_swz<false>, dim3(grid), dim3(M3T), 0, st, d_in, n32, S, w.buckets, w.M, (uint32_t*)nullptr,
                               cfg.checks, 0u, aligned16, sg, ov, e_first, units, split, ms, (uint32_t*)nullptr, sort_bad_flag(c));
    }
}

// A range of segments to parse, as plain data: all segments of a single pass, a piece of the streamed call, a shard's range.
struct SegRange {
    uint32_t seg_hi;        // the segments [piece.seg_lo, seg_hi)
    Piece piece;
    const uint8_t* d_in;    // the buffer, and the parse range in it: n positions from pos0 on, of n_total
    uint32_t n, pos0, n_total;
    uint32_t runup0;        // 1: the range's first segment has history in front of it to run up through
    SegEnds sg;
    const uint16_t* steps;  // the restart steps (k_adv, k_rle), or nullptr: k_emit works them out itself
    uint32_t* E0;           // where the segments are entered ...
    uint32_t* xs;           // ... and where they were left
    uint32_t* fixlist;      // the entries to repair, and how many
    uint32_t* n_fix;
    uint32_t* scan_part;
    uint32_t* tend;         // (k_scan_b: the totals of a call with one segment end, or nullptr)
    uint32_t* pb;
};

// Every segment of the range finds its entry itself (a run-up of SPEC_W positions in front of it) and says where it was left.
void launch_spec_emit(hipStream_t st, const Workspace& w, const ParseCfg& cfg, const SegRange& r) {
    const SpecFix fx{r.fixlist, w.badmap, r.n_fix};
    MI355_LAUNCH_EMIT(1, r.steps, dim3(cdiv(r.seg_hi - r.piece.seg_lo, 4)), st, r.d_in, r.n, r.seg_hi, w.M, cfg.use_quarter ? w.Mq : nullptr, cfg,
                       r.steps, r.E0, w.tokbuf, w.cnt, r.pos0, r.n_total, r.sg, r.xs, fx, r.runup0, r.piece.seg_lo);
}
// The speculative entries of the range: k_emit<1>; then a handful of entries that did not check out (seams of pieces of different
// kinds, a short periodic stretch) are parsed again from where the segment before them was left; what is still wrong then
// fails k_scan_a's check of the chain of entries and exits (DevState::spec_bad).
void launch_spec_entries(mi355_deflate_ctx* c, hipStream_t st, const Workspace& w, const ParseCfg& cfg, const SegRange& r) {
    const uint32_t lo = r.piece.seg_lo, ns = r.seg_hi - lo;
    const SpecFix fx{r.fixlist, w.badmap, r.n_fix};
    launch_spec_emit(st, w, cfg, r);
    hipLaunchKernelGGL(k_spec_check, dim3(cdiv(ns, 256)), dim3(256), 0, st, r.seg_hi, (const uint32_t*)r.E0, (const uint32_t*)r.xs, w.badmap,
                       r.fixlist, r.n_fix, lo);
    MI355_LAUNCH_EMIT(2, r.steps, dim3(FIX_MAX / 4), st, r.d_in, r.n, r.seg_hi, w.M, cfg.use_quarter ? w.Mq : nullptr, cfg, r.steps, r.E0,
                       w.tokbuf, w.cnt, r.pos0, r.n_total, r.sg, r.xs, fx, 0u, 0u);
    hipLaunchKernelGGL(k_scan_a, dim3(cdiv(ns, 1024)), dim3(1024), 0, st, r.seg_hi, w.cnt, r.scan_part, (const uint32_t*)r.E0,
                       (const uint32_t*)r.xs, &reinterpret_cast<DevState*>(c->d_sc)->spec_bad, lo);
}
// The token scan of the range: where every segment's tokens go in the stream, and the tokens there.  `exact`: the entries came from
// the exit tables, there is no chain to check and k_scan_a has not run yet.
void launch_token_scan(mi355_deflate_ctx* c, hipStream_t st, const Workspace& w, const SegRange& r, bool exact) {
    const uint32_t lo = r.piece.seg_lo, ns = r.seg_hi - lo;
    if (exact)
        hipLaunchKernelGGL(k_scan_a, dim3(cdiv(ns, 1024)), dim3(1024), 0, st, r.seg_hi, w.cnt, r.scan_part, (const uint32_t*)nullptr,
                           (const uint32_t*)nullptr, (uint32_t*)nullptr, lo);
    hipLaunchKernelGGL(k_scan_b, dim3(cdiv(ns, 1024)), dim3(1024), 0, st, r.seg_hi, w.cnt, r.scan_part, w.base, c->d_sc, r.tend, r.pb, r.piece);
    hipLaunchKernelGGL(k_compact, dim3(cdiv(ns, 4)), dim3(256), 0, st, r.seg_hi, w.tokbuf, w.cnt, w.base, w.dtok, c->d_sc, lo);
}

// Adler-32 / CRC-32 of d_in[0..n) into the scalars (`part`: a word per CRC_CHUNK bytes)
void launch_adler(mi355_deflate_ctx* c, hipStream_t st, const uint8_t* d_in, uint64_t n) {
    const uint32_t nch = cdiv(n, ADLER_CHUNK);
    if (nch) hipLaunchKernelGGL(k_adler_part, dim3(nch), dim3(256), 0, st, d_in, (uint32_t)n, c->d_sc);
    hipLaunchKernelGGL(k_adler_fold, dim3(1), dim3(64), 0, st, (uint32_t)n, c->d_sc);
}
void launch_crc(mi355_deflate_ctx* c, hipStream_t st, const uint8_t* d_in, uint64_t n, uint32_t* part) {
    const uint32_t nch = cdiv(n, CRC_CHUNK);
    if (nch) {
        hipLaunchKernelGGL(k_crc_part, dim3(cdiv(nch, 256)), dim3(256), 0, st, d_in, (uint32_t)n, part);
        hipLaunchKernelGGL(k_crc_fold, dim3(cdiv(nch, 256)), dim3(256), 0, st, (uint32_t)n, nch, part, c->d_sc);
    }
}
// One run of bytes outside an encode, wrapper 1: Adler-32, 2: CRC-32, into the cleared scalars; the CRC's words in the context's own
// d_crc (the checksum entries below and the decode side, decode_host.inc: the workspace may belong to a live shard)
int launch_sums_one(mi355_deflate_ctx* c, hipStream_t st, int wrapper, const uint8_t* d_in, uint64_t n) {
    if (wrapper == 2)
        if (const int rc = ensure_buf(c, &c->d_crc, &c->d_crc_cap, ((size_t)cdiv(n, CRC_CHUNK) + 2) * 4 + 512)) return rc;
    HIPCHK(c, hipMemsetAsync(c->d_sc, 0, sizeof(DevScalars), st));
    if (wrapper == 1) launch_adler(c, st, d_in, n);
    if (wrapper == 2) launch_crc(c, st, d_in, n, reinterpret_cast<uint32_t*>(c->d_crc));
    return MI355_OK;
}
// The checksum of the input and the frame around the stream (wrapper 1: zlib, 2: gzip with the caller's header; `final`: with the trailer).
int launch_frame_tail(mi355_deflate_ctx* c, hipStream_t st, const uint8_t* d_in, uint64_t n, uint32_t wrapper, const Workspace& w,
                      const uint8_t* gz_hdr, size_t gz_len, uint8_t* d_out, bool final) {
    if (wrapper == 1) {
        launch_adler(c, st, d_in, n);
        hipLaunchKernelGGL(k_zlib_frame, dim3(1), dim3(64), 0, st, c->d_sc, d_out, final ? 1u : 0u);
    }
    if (wrapper == 2) {
        HIPCHK(c, hipMemcpyAsync(w.gz_hdr, gz_hdr, gz_len, hipMemcpyHostToDevice, st));
        launch_crc(c, st, d_in, n, w.crc_part);
        hipLaunchKernelGGL(k_gzip_frame, dim3(1), dim3(64), 0, st, c->d_sc, d_out, w.gz_hdr, (uint32_t)gz_len, (uint32_t)n, final ? 1u : 0u);
    }
    return MI355_OK;
}

// links + match table (chained_hash_table.rs, matching.rs) of d_in[0..n): M, and Mq for a quarter budget.
// Events: ev_mid is recorded between the chain structure (k_links / k_sort) and the walk.
// The hash-sorted path does not represent the identity entries of the head table (head[h] = h at the start and for every
// bucket that slides out), which only matter after a hash re-warm and only for the positions that can see a re-filed
// position: with `ident` the first three epochs go through k_links + k_match (over a prefix of the input; what it
// computes beyond them is overwritten).  Streams with positions that are filed late or not at all (ov.ns, ov.nh: write patterns around a
// flush) take k_links + k_match throughout.
// `redo_head`: a second pass after a hash re-warm (Q1) -- only the positions that can see the two re-filed
// ones (the first two epochs and the first two positions of the third: three epochs through k_links + k_match) are computed again.
int launch_match_tables(mi355_deflate_ctx* c, hipStream_t st, const uint8_t* d_in, uint64_t n, Workspace& w,
                        const ParseCfg& cfg, const HashOverride& ov, bool ident, SegEnds sg, hipEvent_t ev_mid,
                        bool redo_head = false, const Arrival* arr = nullptr, uint64_t quirk_end = 0, const SortInit* init = nullptr) {
    const uint32_t n32 = (uint32_t)n;
    const int aligned16 = ((reinterpret_cast<uintptr_t>(d_in) & 15) == 0) ? 1 : 0;
    const uint32_t cq = cfg_cq(cfg);
    const bool has_q = cfg_has_q(cfg);
    if (cfg.use_quarter && cq == 0) HIPCHK(c, hipMemsetAsync(w.Mq, 0, (n + 64) * 4, st));
    // Positions that a write pattern around a sync flush left out of the chains or filed a byte late (ov.ns | ov.nh) are
    // candidates -- or missing ones -- for as long as they are inside the window: the epochs up to the one behind the last
    // of them (quirk_end = the position behind it; 0 = not known: everything) go through k_links + k_match, which know
    // them, like the first two epochs after a hash re-warm (`ident`); the sorted path takes over two epochs on.
    const bool quirks = (ov.ns | ov.nh) != 0;
    uint32_t n_ep = (uint32_t)((n + WINDOW_SIZE - 1) / WINDOW_SIZE);
    // (ident: THREE epochs.  A re-warm at the very end of the first window -- the first block fills exactly there, or a flush point
    // lies there -- files positions 32768 / 32769 under foreign hashes; after the first slide the identity entries of buckets 0 and 1
    // point at exactly those two, and positions 65536 / 65537 reach them at the far end of their window: tests/golden/identity_hop.bin.
    // Nothing further on can see a re-filed position, through a bucket or through an identity entry.)
    uint32_t e_first = ident ? MI355_IDENT_EPOCHS : 0;  // first epoch of the sorted path
    if (quirks) {
        const uint64_t eq = quirk_end ? (quirk_end - 1) / WINDOW_SIZE + 2 : (uint64_t)n_ep;
        e_first = eq < n_ep ? (uint32_t)(eq > e_first ? eq : e_first) : n_ep;
    }
    const bool sorted_path = e_first < n_ep || n_ep == 0;
    uint64_t n_old = 0;  // what k_links + k_match cover
    if (e_first) {
        n_old = (uint64_t)e_first * WINDOW_SIZE + 4096;
        if (n_old > n || !sorted_path) n_old = n;
    }
    // (the epoch behind the link kernels' part is walked again as well: their last 4096 positions saw the input end early)
    if (redo_head && sorted_path && !quirks && n_ep > e_first + 1) n_ep = e_first + 1;
    // An input that is still arriving (host-buffer call): the plain sorted path sorts and walks the epochs of a piece as
    // soon as their bytes are there; every other path waits for all of it.
    const bool piecewise = arr && arr->n > 1 && sorted_path && e_first == 0 && !redo_head;
    if (arr && arr->n > 0 && !piecewise) {
        const int rc = arrival_wait(c, st, *arr, arr->n - 1);
        if (rc) return rc;
    }
    if (n_old) {
        const uint32_t no = (uint32_t)n_old;
        const uint32_t mt = match_tile(n_old, c->n_cu);
        // hl (hash + publish flag per position) borrows the adv array, which is written later
        hipLaunchKernelGGL(k_links_a, dim3(cdiv(n_old, 256)), dim3(256), 0, st, d_in, no, w.link, w.adv, ov);
        hipLaunchKernelGGL(k_links_b, dim3(cdiv(n_old, WINDOW_SIZE)), dim3(64), 0, st, no, w.link, w.adv,
                           (ov.ns || ident || MI355_FORCE_IDENT) ? 2u : 0u);
        if (ev_mid && (!sorted_path || e_first >= n_ep)) HIPCHK(c, hipEventRecord(ev_mid, st));
        if (has_q)
            hipLaunchKernelGGL(k_match<true>, dim3(cdiv(n_old, mt)), dim3(MTHREADS), 0, st, d_in, no, w.link, w.M, w.Mq,
                               cfg.checks, cq, aligned16, sg, mt);
        else
            hipLaunchKernelGGL(k_match<false>, dim3(cdiv(n_old, mt)), dim3(MTHREADS), 0, st, d_in, no, w.link, w.M,
                               (uint32_t*)nullptr, cfg.checks, 0u, aligned16, sg, mt);
    }
    if (sorted_path && e_first < n_ep) {
        uint16_t* S = w.sorted + WINDOW_SIZE;  // one epoch of pad in front
        if (piecewise) {
            uint32_t e_lo = 0;
            for (int k = 0; k < arr->n; k++) {
                const uint32_t e_hi = k + 1 == arr->n ? n_ep : (arr->upto[k] < n_ep ? arr->upto[k] : n_ep);
                if (e_lo >= e_hi) continue;
                {
                    const int rc = arrival_wait(c, st, *arr, k);
                    if (rc) return rc;
                }
                launch_sort(c, st, e_hi - e_lo, d_in, n32, ov, S, w.buckets, e_lo, e_lo == 0 ? init : nullptr);
                if (e_lo == 0 && ev_mid) HIPCHK(c, hipEventRecord(ev_mid, st));  // (the stage clocks of such a call split at the first piece's sort)
                launch_walk(c, st, d_in, n32, S, w, cfg, aligned16, sg, ov, e_lo, e_hi - e_lo);
                e_lo = e_hi;
            }
            return MI355_OK;
        }
        // (the first sorted epoch reads the buckets of the one before it)
        const uint32_t e_sort = e_first ? e_first - 1 : 0;
        launch_sort(c, st, n_ep - e_sort, d_in, n32, ov, S, w.buckets, e_sort, e_first == 0 ? init : nullptr);
        if (ev_mid) HIPCHK(c, hipEventRecord(ev_mid, st));
        const uint32_t ne = n_ep - e_first;
        launch_walk(c, st, d_in, n32, S, w, cfg, aligned16, sg, ov, e_first, ne);
    }
    return MI355_OK;
}

// The whole kernel sequence for one input resident on the device.
// `ends`: the input as it arrived -- sync flush points in ascending order, then n (one entry = one shot)
// What the streaming handle asks for on top of a plain encode: the buffer starts deep inside a stream at a
// sync-flush point's 32 KiB-aligned history (`mid_stream`: nothing that belongs to the start of a stream
// -- Q1, hash re-warm, identity hops -- may fire), and the output of the first `skip_segments` segments has
// been handed out already (*skip_bytes = where the rest starts; a sync flush leaves the stream byte aligned).
constexpr size_t FILL_ASIDE_FROM = 8u << 20;  // output bounds from which the clearing of the output leaves the call's stream --
                                              // where the call's own kernels do not clear it (small_inits)
#ifndef MI355_FILL_ASIDE_MB
#define MI355_FILL_ASIDE_MB 0x7fffffff
#endif
constexpr size_t FILL_INSIDE_BELOW = (size_t)MI355_FILL_ASIDE_MB << 20;
// the position behind the last one whose filing a skew / hole list changes (a skew at F files F and F + 1 a byte late)
uint64_t quirk_reach(const std::vector<uint32_t>* skew, const std::vector<uint32_t>* holes) {
    uint64_t e = 0;
    if (skew && !skew->empty()) e = (uint64_t)skew->back() + 2;
    if (holes && !holes->empty() && (uint64_t)holes->back() + 1 > e) e = (uint64_t)holes->back() + 1;
    return e;
}
struct EncodeExtra {
    bool mid_stream = false;
    Arrival arrival;
    size_t skip_segments = 0;
    size_t skip_bytes = 0;
    const std::vector<uint32_t>* skew = nullptr;   // stages.h HashOverride::skw (buffer positions, ascending)
    const std::vector<uint32_t>* holes = nullptr;  // HashOverride::hol
};

// k_emit works the restart steps out itself (its adv argument nullptr) and k_adv is not launched: the lazy / greedy levels with the
// full-budget table only and one end of the data (deflate_kernels.hip, k_emit)
static inline bool steps_in_emit(const mi355_deflate_ctx* c, const ParseCfg& cfg, uint32_t m) {
    return MI355_STEPS_IN_EMIT && c->steps_in_emit && cfg.mode != MODE_RLE && !cfg.use_quarter && m == 1;
}
int run_encode(mi355_deflate_ctx* c, const uint8_t* d_in, uint64_t n, const mi355_deflate_opts* o, uint8_t* d_out,
               size_t out_cap, size_t* out_len, hipStream_t st, const std::vector<uint32_t>* ends_in = nullptr,
               const std::vector<uint32_t>* rewarm = nullptr, const uint8_t* gz_hdr = nullptr, size_t gz_len = 0,
               EncodeExtra* extra = nullptr) {
    if (c->live_shard) {
        c->err = "this context holds a sharded encode between mi355_shard_begin and mi355_shard_end";
        return MI355_E_STATE;
    }
    c->last_plan = nullptr;  // (they point into the workspace, which may move or be reused below)
    c->last_nb = 0;
    c->q1_last_on = 0;
#ifdef MI355_DEBUG_HOOKS
    c->dbg_epochs = 0;
#endif
    if (c->spec_pause > 0) c->spec_pause--;
    const bool spec = c->spec_pause == 0;  // segment entries by speculation + check (k_emit<1>) instead of exit tables and tree
    const bool reuse = c->reuse_tables;    // (the match table and the restart steps of this very input are in the workspace)
    c->reuse_tables = false;
    std::vector<uint32_t> ends_default(1, (uint32_t)n);
    const std::vector<uint32_t>& ends = ends_in ? *ends_in : ends_default;
    const size_t m = ends.size();
    if (m == 0 || ends.back() != (uint32_t)n) return MI355_E_ARG;
    if (rewarm && rewarm->size() > m) return MI355_E_ARG;
    if (n >= 0xFFFF0000ull) {
        c->err = "input of 4 GiB - 64 KiB or more in one call is not supported; shard it";
        return MI355_E_UNSUPPORTED;
    }
    ParseCfg cfg;
    if (const int rc = parse_cfg(c, o, &cfg)) return rc;
    const bool hashing = cfg_hashing(cfg);
    const bool zlib = o->wrapper == 1;
    const bool gzip = o->wrapper == 2;
    if (o->wrapper > 2 || (gzip && (!gz_hdr || gz_len == 0 || gz_len > 0xFFFF))) return MI355_E_ARG;
    if (!gzip) gz_len = 0;
    const bool sync_tail = o->flush == MI355_FLUSH_SYNC;
    if (o->flush > MI355_FLUSH_SYNC) return MI355_E_ARG;
    const size_t need_out = mi355_deflate_bound_ex(n, o->wrapper, gz_len, m - 1);
    if (out_cap < need_out) {
        *out_len = need_out;
        c->err = "device output buffer smaller than mi355_deflate_bound_ex(in_len, wrapper, hdr_len, flushes)";
        return MI355_E_OUT_TOO_SMALL;
    }
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n_skew = (extra && extra->skew) ? extra->skew->size() : 0, n_holes = (extra && extra->holes) ? extra->holes->size() : 0;
    Workspace sz = carve(nullptr, n, cfg.use_quarter, m, gz_len, n_skew + n_holes);
    int rc = ensure_ws(c, sz.bytes);
    if (rc) return rc;
    Workspace w = carve(c->ws, n, cfg.use_quarter, m, gz_len, n_skew + n_holes);
#ifdef MI355_DEBUG_HOOKS
    c->dbg_sorted = w.sorted + WINDOW_SIZE;
    c->dbg_buckets = w.buckets;
    c->dbg_epochs = (n + WINDOW_SIZE - 1) / WINDOW_SIZE;
#endif
    // A small plain call (no flush points, no quirks, the sorted path from its first epoch: k_sort is its first kernel) has that
    // kernel clear the scalars and set the one segment end, and k_block_hist clear the output buffer: the runtime's fills were four
    // launches on the way of a call of seventeen (pg11.txt: 22 of 285 us).
    // (Every size: with the output of a 100 MB call cleared by fills on a stream of their own, beside k_sort -- the way of rounds
    // 3 to 5 -- k_sort ran 15 us longer, the wait for them was a bubble in front of the parse, and k_block_hist clearing
    // 100 MB on its way costs 5 us: 4.272 -> 4.242 ms.  MI355_FILL_ASIDE_MB sets a size from which the fills come back.)
    const bool small_inits = m == 1 && n > 0 && hashing && need_out < FILL_INSIDE_BELOW && !rewarm && !extra && !MI355_FORCE_IDENT && !reuse;
    if (m == 1 && small_inits) {
    } else if (m == 1) {  // one segment: its end is a fill of one word (no trip over the bus in front of the first kernel)
        HIPCHK(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(w.seg_ends), (int)(uint32_t)n, 1, st));
    } else if (m <= H_ENDS_CAP) {  // through the context's pinned staging: no wait (it is free again after this call's last sync)
        memcpy(c->h_ends, ends.data(), m * sizeof(uint32_t));
        HIPCHK(c, hipMemcpyAsync(w.seg_ends, c->h_ends, m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    } else {
        HIPCHK(c, hipMemcpyAsync(w.seg_ends, ends.data(), m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipStreamSynchronize(st));  // `ends` may be a temporary of the caller
    }
    const SegEnds sg{w.seg_ends, (uint32_t)m};
    mi355_deflate_info& info = c->info;
    memset(&info, 0, sizeof info);
    c->pend_passes = 0;
    info.in_len = n;

    const uint32_t n32 = (uint32_t)n;
    HashOverride ov = NO_HASH_OVERRIDE;
    uint64_t quirk_end = 0;  // (launch_match_tables)
    if (rewarm && !rewarm->empty() && hashing && n >= 2) {  // flush points that re-warm the hash (stages.h)
        uint8_t b01[2];
        HIPCHK(c, hipMemcpyAsync(w.rewarm, rewarm->data(), rewarm->size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(b01, d_in, 2, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        ov.m = (uint32_t)rewarm->size();
        ov.pts = w.rewarm;
        ov.b0 = b01[0];
        ov.b1 = b01[1];
        info.q1_rewarm = 1;
    }
    if (extra && hashing && ((extra->skew && !extra->skew->empty()) || (extra->holes && !extra->holes->empty()))) {
        const size_t ns = n_skew, nh = n_holes;
        if (ns) HIPCHK(c, hipMemcpyAsync(w.quirks, extra->skew->data(), ns * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        if (nh) HIPCHK(c, hipMemcpyAsync(w.quirks + ns, extra->holes->data(), nh * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipStreamSynchronize(st));
        ov.ns = (uint32_t)ns;
        ov.skw = w.quirks;
        ov.nh = (uint32_t)nh;
        ov.hol = w.quirks + ns;
        quirk_end = quirk_reach(extra->skew, extra->holes);
    }
    // Quirk Q1 (lz77.rs:628-638) needs one look at block 0: did the first block end inside the first window?
    // Then two hashes are re-warmed and the tables change.  The call queues everything and looks at the answer after its
    // one sync; the kernel that makes the block table knows it as well (q1_rewarm, the host's own predicate) and a yes
    // stops the pass's block stages on the device -- the call is run again with the two hashes re-warmed.  (Before: large
    // inputs had the scalars copied to the host between parse and block stages and waited for them before k_pack was
    // queued -- an event, a copy kernel and an event in the queue of every call, 16 us of it idle.)
    const bool q1_possible = hashing && n >= MAX_BUFFER_LENGTH && n >= 2 && !(extra && extra->mid_stream);
    const bool speculate = q1_possible;  // (every size: the device stops the pass's block stages itself -- DevScalars::q1_cancel)
    auto q1_fires = [&](const DevScalars* hs, bool* fires) -> int {  // (after a wait that brought *hs up to date)
        *fires = false;
        if (!hs->b0_full) return MI355_OK;
        uint64_t wpos = 0;
        if (q1_rewarm(hs->b0_last_tok, hs->b0_last_pos, cfg.mode, n, &wpos)) {
            uint8_t b01[2];
            HIPCHK(c, hipMemcpyAsync(b01, d_in, 2, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            ov.on = 1;
            ov.pos = wpos;
            ov.b0 = b01[0];
            ov.b1 = b01[1];
            info.q1_rewarm = 1;
            c->q1_last_on = 1;
            c->q1_last_pos = wpos;
            *fires = true;
        }
        return MI355_OK;
    };
    const uint64_t bit_base = zlib ? 16 : (gzip ? 8 * (uint64_t)gz_len : 0);
    int passes = 0;
    // (one segment end, at most 1 MiB: the stages between the parse and the block histograms are one launch)
    const bool small_tail = MI355_SMALL_TAIL && m == 1 && n > 0 && w.K0 <= SMALL_TAIL_SEGS;
    const bool clocks = stage_clocks_on(c, n);
    const auto host_t0 = std::chrono::steady_clock::now();  // (without the events: the host's clock from here to the return of the last wait)
    float host_ms = 0;
    int ev_last[MAX_PASSES];
    for (int pass = 0; pass < MAX_PASSES; pass++) {
        passes = pass + 1;
        hipEvent_t* ev = c->ev[pass];
        // (the clocks of the stages: an event between two kernels is 5.7 us of idle queue -- five of them were a tenth of a 167 KB call)
        auto mark = [&](int i) -> hipError_t { return clocks ? hipEventRecord(ev[i], st) : hipSuccess; };
        // k_pack ORs its bits into a cleared buffer.  A plain one-shot call has k_sort clear the scalars and k_block_hist the
        // output (small_inits).  The calls that cannot (flush points, quirks, the levels without a hash) clear a large output
        // on a stream of its own, behind whatever used the buffer before, together with the two small clears of the call (the
        // scalars, the root's entry), and the first kernel that needs any of them waits.
        const bool fill_aside = need_out >= FILL_ASIDE_FROM && n > 0 && !small_inits;
        if (fill_aside)
            HIPCHK(c, hipEventRecord(c->ev_fill[0], st));  // (what used the buffers before; the clears themselves are queued once the
                                                           // match stage is on its way: nothing stands between the call and its first kernel)
        else if (!(small_inits && pass == 0))
            HIPCHK(c, hipMemsetAsync(c->d_sc, 0, sizeof(DevScalars), st));
        HIPCHK(c, mark(0));
        const SortInit sort_init{reinterpret_cast<uint32_t*>(c->d_sc), (uint32_t)(sizeof(DevScalars) / 4), w.seg_ends, (uint32_t)n};
        // ---- links + match table -------------------------------------------------------------
        if (n > 0 && reuse && pass == 0) {
            HIPCHK(c, mark(1));
        } else if (n > 0) {
            if (hashing) {
                rc = launch_match_tables(c, st, d_in, n, w, cfg, ov, (ov.on | ov.m | MI355_FORCE_IDENT) != 0, sg, clocks ? ev[1] : nullptr, pass == 1,
                                         extra ? &extra->arrival : nullptr, quirk_end, (small_inits && pass == 0) ? &sort_init : nullptr);
                if (rc) return rc;
            } else {
                if (extra && extra->arrival.n > 0) {
                    rc = arrival_wait(c, st, extra->arrival, extra->arrival.n - 1);
                    if (rc) return rc;
                }
                HIPCHK(c, mark(1));
                if (cfg.mode == MODE_RLE)
                    hipLaunchKernelGGL(k_rle, dim3(cdiv(n, RT)), dim3(256), 0, st, d_in, n32, w.M, w.adv, sg);
                else
                    HIPCHK(c, hipMemsetAsync(w.M, 0, (n + 64) * 4, st));
            }
        } else {
            HIPCHK(c, mark(1));
        }
        HIPCHK(c, mark(2));
        if (fill_aside) {
            HIPCHK(c, hipStreamWaitEvent(c->fill, c->ev_fill[0], 0));
            HIPCHK(c, hipMemsetAsync(c->d_sc, 0, sizeof(DevScalars), c->fill));
            HIPCHK(c, hipMemsetAsync(w.levels.back().E, 0, sizeof(uint32_t), c->fill));
            HIPCHK(c, hipMemsetAsync(d_out, 0, need_out, c->fill));
            HIPCHK(c, hipEventRecord(c->ev_fill[1], c->fill));
        }
        // ---- restart path -> tokens ----------------------------------------------------------
        if (n > 0) {
            const uint32_t* Mq = cfg.use_quarter ? w.Mq : nullptr;
            // (k_rle has written the steps of that level; a second attempt finds the first one's -- if that one made any)
            const bool in_emit = steps_in_emit(c, cfg, m);
            if (cfg.mode != MODE_RLE && !(reuse && pass == 0 && !in_emit) && !(spec && in_emit))
                hipLaunchKernelGGL(k_adv, dim3(cdiv(n, 1024)), dim3(256), 0, st, n32, w.M, Mq, cfg, w.adv, sg, 0u);
            const uint16_t* const steps = in_emit ? nullptr : w.adv;
            const SegRange all{w.K0, Piece{0u, 0u, 1u}, d_in, n32, 0u, n32, 0u, sg, steps, w.levels[0].E, w.xs, w.fixlist, &c->d_sc->n_fix[0],
                               w.scan_part, m == 1 ? w.tend : nullptr, m == 1 ? w.pb : nullptr};
            if (!spec) {
                hipLaunchKernelGGL(k_seg_exit, dim3(cdiv(w.K0, 4)), dim3(256), 0, st, n32, w.K0, w.adv, w.levels[0].X, 0u);
                // the table tree: wide levels as launches of their own, the levels of at most TOP_UNITS units -- up and down -- in one
                size_t lt = 0;
                while (w.levels[lt].count > TOP_UNITS) lt++;
                for (size_t l = 0; l < lt; l++) {
                    const Level& ch = w.levels[l];
                    const Level& pa = w.levels[l + 1];
                    hipLaunchKernelGGL(k_level_up, dim3(pa.count), dim3(ZONE), 0, st, n32, ch.count, ch.usize, ch.X, pa.count, pa.X);
                }
                // the root unit is entered at position 0
                if (fill_aside)
                    HIPCHK(c, hipStreamWaitEvent(st, c->ev_fill[1], 0));
                else
                    HIPCHK(c, hipMemsetAsync(w.levels.back().E, 0, sizeof(uint32_t), st));
                {
                    TopLevels t;
                    memset(&t, 0, sizeof t);
                    t.nl = (uint32_t)(w.levels.size() - lt);
                    if (t.nl > TOP_LEVELS) return MI355_E_ARG;  // (64 * 16^7 segments: beyond any 32-bit input)
                    for (uint32_t k = 0; k < t.nl; k++) {
                        const Level& L = w.levels[lt + k];
                        t.count[k] = L.count;
                        t.usize[k] = L.usize;
                        t.X[k] = L.X;
                        t.E[k] = L.E;
                    }
                    if (lt > 0) {
                        const Level& L = w.levels[lt - 1];
                        t.count_below = L.count;
                        t.usize_below = L.usize;
                        t.X_below = L.X;
                        t.E_below = L.E;
                    }
                    hipLaunchKernelGGL(k_tree_top, dim3(1), dim3(1024), 0, st, n32, t);
                }
                for (size_t l = lt > 0 ? lt - 1 : 0; l-- > 0;) {
                    const Level& ch = w.levels[l];
                    const Level& pa = w.levels[l + 1];
                    hipLaunchKernelGGL(k_level_down, dim3(cdiv(pa.count, 64)), dim3(64), 0, st, n32, ch.count, ch.usize,
                                       ch.X, pa.count, pa.E, ch.E);
                }
                hipLaunchKernelGGL((k_emit<0, false>), dim3(cdiv(w.K0, 4)), dim3(256), 0, st, d_in, n32, w.K0, w.M, Mq, cfg, w.adv,
                                   w.levels[0].E, w.tokbuf, w.cnt, 0u, n32, sg, (uint32_t*)nullptr, SpecFix{nullptr, nullptr, nullptr}, 0u, 0u);
            } else {
                // Every segment finds its entry itself and says where it was left; k_scan_a checks the chain of entries and exits.
                if (fill_aside) HIPCHK(c, hipStreamWaitEvent(st, c->ev_fill[1], 0));
                // (a small one-shot call: check, repair, the final check, the scan and the block table are k_small_fix below)
                if (small_tail)
                    launch_spec_emit(st, w, cfg, all);
                else
                    launch_spec_entries(c, st, w, cfg, all);
            }
            if (small_tail) {
                // a small one-shot call: the check of the chain, the repair, the scan and the block table in one workgroup
                uint32_t* const xs = spec ? w.xs : nullptr;
                if (spec && !steps)
                    hipLaunchKernelGGL((k_small_fix<true>), dim3(1), dim3(SMALL_FIX_T), 0, st, d_in, n32, w.K0, w.M, Mq, cfg, steps,
                                       w.levels[0].E, w.tokbuf, w.cnt, sg, xs, w.badmap, w.fixlist, w.nb_max, sync_tail ? 1u : 0u,
                                       &reinterpret_cast<DevState*>(c->d_sc)->spec_bad, w.base, c->d_sc, w.tend, w.pb, w.bstart, w.q13, w.tab,
                                       (pass == 0 && speculate) ? 1u : 0u);
                else
                    hipLaunchKernelGGL((k_small_fix<false>), dim3(1), dim3(SMALL_FIX_T), 0, st, d_in, n32, w.K0, w.M, Mq, cfg, steps,
                                       w.levels[0].E, w.tokbuf, w.cnt, sg, xs, w.badmap, w.fixlist, w.nb_max, sync_tail ? 1u : 0u,
                                       &reinterpret_cast<DevState*>(c->d_sc)->spec_bad, w.base, c->d_sc, w.tend, w.pb, w.bstart, w.q13, w.tab,
                                       (pass == 0 && speculate) ? 1u : 0u);
                hipLaunchKernelGGL(k_compact, dim3(cdiv(w.K0, 4)), dim3(256), 0, st, w.K0, w.tokbuf, w.cnt, w.base, w.dtok, c->d_sc, 0u);
            } else {
                launch_token_scan(c, st, w, all, !spec);
            }
        } else {
            hipLaunchKernelGGL(k_scan_zero, dim3(1), dim3(64), 0, st, c->d_sc);
        }
        if (!(m == 1 && n > 0)) {  // (one segment: k_scan_b has written its totals)
            hipLaunchKernelGGL(k_seg_tokens, dim3(cdiv(m, 64)), dim3(64), 0, st, sg, w.K0, w.base,
                               w.levels.empty() ? nullptr : w.levels[0].E, w.tokbuf, w.cnt, c->d_sc, w.tend);
            hipLaunchKernelGGL(k_block_count, dim3(1), dim3(64), 0, st, sg, w.tend, w.pb, c->d_sc);
        }
        if (!small_tail)
            hipLaunchKernelGGL(k_block_bounds, dim3(cdiv((uint64_t)w.nb_max + 1, 4)), dim3(256), 0, st, n32, w.K0,
                               w.nb_max, cfg.mode, sg, sync_tail ? 1u : 0u, w.tend, w.pb, w.base,
                               w.levels.empty() ? nullptr : w.levels[0].E, w.tokbuf, w.dtok, c->d_sc, w.bstart, w.q13, w.tab, Piece{0u, 0u, 1u},
                               (const uint32_t*)nullptr, (pass == 0 && speculate) ? 1u : 0u);
        HIPCHK(c, mark(3));
        ev_last[pass] = 3;
        // ---- blocks: histogram, Huffman, plan --------------------------------------------------------
        const uint32_t nbg = w.nb_max;
        const bool hist_clears = !fill_aside && small_inits;  // (need_out is a multiple of 8, d_out 4-byte aligned)
        MI355_LAUNCH_HIST(nbg * PSPLIT, c->n_cu, st, w.dtok, c->d_sc, w.ll_freq, w.d_freq, w.tab, 0u,
                           hist_clears ? reinterpret_cast<uint32_t*>(d_out) : nullptr, (uint32_t)(need_out / 4));
        hipLaunchKernelGGL(k_block_header, dim3(nbg), dim3(128), 0, st, c->d_sc, w.ll_freq, w.d_freq, w.hdr, 0u);
        if (!fill_aside && !hist_clears) HIPCHK(c, hipMemsetAsync(d_out, 0, need_out, st));
        // (raw deflate: nothing behind the plan writes a scalar, and they leave for the host from there)
        const bool state_with_plan = MI355_STATE_KERNEL && !zlib && !gzip;
        hipLaunchKernelGGL(k_plan, dim3(1), dim3(1024), 0, st, c->d_sc, w.hdr, w.bstart, w.q13, w.plan, bit_base,
                           (uint32_t)o->compat, w.tab.sync, reinterpret_cast<uint32_t*>(d_out), Piece{0u, 0u, 1u},
                           state_with_plan ? reinterpret_cast<uint32_t*>(c->h_sc) : (uint32_t*)nullptr);
        HIPCHK(c, mark(4));
        // ---- pack ---------------------------------------------------------------------------------------
        MI355_LAUNCH_PACK(nbg * PSPLIT, c->n_cu, st, d_in, n32, w.dtok, c->d_sc, w.hdr, w.plan, w.bstart,
                           w.q13, (uint32_t)o->compat, reinterpret_cast<uint32_t*>(d_out), w.tab, w.ll_freq, w.d_freq, 0u);
        HIPCHK(c, mark(5));
        rc = launch_frame_tail(c, st, d_in, n, o->wrapper, w, gz_hdr, gz_len, d_out, !sync_tail);
        if (rc) return rc;
        HIPCHK(c, mark(6));
        // (the scalars reach the host by a kernel that writes them into its page-locked memory)
        if (state_with_plan)
            ;
        else if (MI355_STATE_KERNEL)
            hipLaunchKernelGGL(k_state_out, dim3(1), dim3(64), 0, st, reinterpret_cast<const uint32_t*>(c->d_sc),
                               reinterpret_cast<uint32_t*>(c->h_sc), (uint32_t)(sizeof(DevState) / 4));
        else
            HIPCHK(c, hipMemcpyAsync(c->h_sc, c->d_sc, sizeof(DevState), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        if (!clocks) host_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - host_t0).count();
        HIPCHK(c, hipGetLastError());
        if (sort_order_failed(c))  // (never seen on MI355X; the call is done again from the top with ballot ranks)
            return run_encode(c, d_in, n, o, d_out, out_cap, out_len, st, ends_in, rewarm, gz_hdr, gz_len, extra);
        if (spec_entries_failed(c)) {  // (long periodic data: again, with exit tables and the table tree)
            // (what the match stage left -- table and restart steps -- is still there, unless a second pass re-warmed hashes)
            c->reuse_tables = passes == 1;
            const int rc2 = run_encode(c, d_in, n, o, d_out, out_cap, out_len, st, ends_in, rewarm, gz_hdr, gz_len, extra);
            c->info.spec_fallback = c->last_spec_bad;
            return rc2;
        }

        ev_last[pass] = 6;
        if (pass == 0 && speculate) {
            bool fires;
            rc = q1_fires(c->h_sc, &fires);
            if (rc) return rc;
            if (fires) continue;
        }
        break;
    }
    const DevScalars& s = *c->h_sc;
    info.passes = passes;
    info_from_scalars(&info, s);
    c->pend_passes = passes;
    c->pend_clocks = clocks;
    if (!clocks) info.total_ms = host_ms;
    for (int p = 0; p < passes; p++) c->pend_last[p] = ev_last[p];
    if (s.ref_panic) {
        c->err = "the reference panics on this input (stored block after a buffer slide, SURVEY A.4 Q13)";
        return MI355_E_REF_PANIC;
    }
    c->last_plan = w.plan;
    c->last_nt = w.tab.nt;
    c->last_bstart = w.bstart;
    c->last_nb = s.nb;
    c->last_T = s.T;
    c->last_bit_base = bit_base;
    const size_t total = stream_bytes(s.total_bits, o->wrapper, gz_len, sync_tail);
    c->last_crc = s.crc;
    *out_len = total;
    info.out_len = total;
    if (extra && extra->skip_segments) {
        // the first block of segment k starts where the output of segments 0..k-1 ends
        if (extra->skip_segments >= m) return MI355_E_ARG;
        uint32_t b0 = 0;
        BlockPlan bp;
        HIPCHK(c, hipMemcpy(&b0, w.pb + extra->skip_segments, sizeof b0, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(&bp, w.plan + b0, sizeof bp, hipMemcpyDeviceToHost));
        extra->skip_bytes = (size_t)(bp.bit_start / 8);
    }
    return MI355_OK;
}

// ---- a host call whose input is still arriving, worked on -- and delivered -- piece by piece --------------------------------
// mi355_deflate_encode of a large input (encode_host): the input goes over the bus in a few pieces of whole rounds of
// workgroups, and with the segment entries found by speculation (k_emit<1>) nothing in the pipeline needs the whole input
// any more: every piece is sorted, walked, parsed, its tokens appended to the stream's, the blocks that became complete with it
// are costed, planned behind the bits planned so far and packed -- and their bytes go back over the bus while the next piece
// is worked on.  What a piece hands to the next lives on the device (DevScalars::Tcum, nbcum, total_bits; the token array and
// the block tables are the stream's), the host only learns how many bytes are final (a small copy behind every plan) to
// start their copy-out.  The bytes are those of the single pass.  Anything out of the ordinary -- a failed speculation, a
// hash re-warm (Q1: the first block fills inside the first window), a sort that fails its order check -- ends in `*redo`: the
// caller runs the single pass on the input, which is on the device by then.
constexpr int STREAMED_MIN_PIECES = 2;
static_assert(ARRIVE_MAX == (int)PIECES_MAX, "a piece of the arrival is a piece of the stream");

int run_streamed_body(mi355_deflate_ctx* c, const uint8_t* d_in, uint64_t n, const mi355_deflate_opts* o, uint8_t* d_out, size_t d_out_cap,
                      uint8_t* h_out, size_t out_cap, size_t* out_len, const uint8_t* gz_hdr, size_t gz_len, const Arrival& ar, bool* redo);

// (every error exit of the body leaves nothing in flight: copies into the caller's buffer on the out stream or the copy
// engine, block stages that still use the workspace the next call will carve again)
int run_streamed(mi355_deflate_ctx* c, const uint8_t* d_in, uint64_t n, const mi355_deflate_opts* o, uint8_t* d_out, size_t d_out_cap,
                 uint8_t* h_out, size_t out_cap, size_t* out_len, const uint8_t* gz_hdr, size_t gz_len, const Arrival& ar, bool* redo) {
    const int rc = run_streamed_body(c, d_in, n, o, d_out, d_out_cap, h_out, out_cap, out_len, gz_hdr, gz_len, ar, redo);
    if (rc != MI355_OK) {
        if (c->out_stream) (void)hipStreamSynchronize(c->out_stream);
        if (c->blk_stream) (void)hipStreamSynchronize(c->blk_stream);
        (void)hipStreamSynchronize(c->own_stream);
        (void)c->engine.wait_all();
        if (c->bounce && c->bounce_on) (void)c->bounce->out_wait();
    }
    return rc;
}

int run_streamed_body(mi355_deflate_ctx* c, const uint8_t* d_in, uint64_t n, const mi355_deflate_opts* o, uint8_t* d_out, size_t d_out_cap,
                      uint8_t* h_out, size_t out_cap, size_t* out_len, const uint8_t* gz_hdr, size_t gz_len, const Arrival& ar, bool* redo) {
    *redo = true;
    hipStream_t st = c->own_stream;
    // (MI355_HOST_TRACE=1: the calling thread's timeline of a streamed call on stderr -- a development aid)
    static const bool host_trace = getenv("MI355_HOST_TRACE") != nullptr;
    const double ht0 = host_trace ? Bounce::now_ms() : 0;
    std::string htl;
    auto ht = [&](const char* what, int k) {
        if (!host_trace) return;
        char b[64];
        snprintf(b, sizeof b, " %s%d %.3f", what, k, Bounce::now_ms() - ht0);
        htl += b;
    };
    const bool two = c->host_streaming != 2;  // (2: the stages of a piece behind each other on one stream -- a measuring aid)
    ParseCfg cfg;
    if (parse_cfg(c, o, &cfg) != MI355_OK || !cfg_hashing(cfg) || o->wrapper > 2 || o->flush != MI355_FLUSH_FINISH || c->live_shard ||
        c->spec_pause > 0 || ar.n < STREAMED_MIN_PIECES || n >= 0xFFFF0000ull)
        return MI355_OK;  // (not this way: *redo)
    const bool zlib = o->wrapper == 1, gzip = o->wrapper == 2;
    if (gzip && (!gz_hdr || gz_len == 0 || gz_len > 0xFFFF)) return MI355_OK;
    if (!gzip) gz_len = 0;
    const size_t need_out = mi355_deflate_bound_ex(n, o->wrapper, gz_len, 0);
    if (d_out_cap < need_out) return MI355_OK;
    if (!c->out_ok) {
        if (!c->out_stream && hipStreamCreateWithFlags(&c->out_stream, hipStreamNonBlocking) != hipSuccess) return fail_hip(c, "hipStreamCreate", hipGetLastError());
        if (!c->blk_stream && hipStreamCreateWithFlags(&c->blk_stream, hipStreamNonBlocking) != hipSuccess)
            return fail_hip(c, "hipStreamCreate", hipGetLastError());
        for (int k = 0; k < ARRIVE_MAX; k++)
            if (hipEventCreateWithFlags(&c->ev_plan[k], hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&c->ev_walk[k], hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&c->ev_pack[k], hipEventDisableTiming) != hipSuccess)
                return fail_hip(c, "hipEventCreate", hipGetLastError());
        if (hipHostMalloc(reinterpret_cast<void**>(&c->h_piece), ARRIVE_MAX * sizeof(DevState), hipHostMallocDefault) != hipSuccess)
            return fail_hip(c, "hipHostMalloc", hipGetLastError());
        c->out_ok = true;
    }
    c->last_plan = nullptr;
    c->last_nb = 0;
    Workspace sz = carve(nullptr, n, cfg.use_quarter, 1, gz_len, 0);
    int rc = ensure_ws(c, sz.bytes);
    if (rc) return rc;
    Workspace w = carve(c->ws, n, cfg.use_quarter, 1, gz_len, 0);
#ifdef MI355_DEBUG_HOOKS
    c->dbg_sorted = w.sorted + WINDOW_SIZE;
    c->dbg_buckets = w.buckets;
    c->dbg_epochs = (n + WINDOW_SIZE - 1) / WINDOW_SIZE;
#endif
    HIPCHK(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(w.seg_ends), (int)(uint32_t)n, 1, st));
    const SegEnds sg{w.seg_ends, 1u};
    mi355_deflate_info& info = c->info;
    memset(&info, 0, sizeof info);
    c->pend_passes = 0;
    info.in_len = n;
    const uint32_t n32 = (uint32_t)n;
    const HashOverride& ov = NO_HASH_OVERRIDE;
    const int aligned16 = ((reinterpret_cast<uintptr_t>(d_in) & 15) == 0) ? 1 : 0;
    const uint64_t bit_base = zlib ? 16 : (gzip ? 8 * (uint64_t)gz_len : 0);
    const uint32_t* Mq = cfg.use_quarter ? w.Mq : nullptr;
    // the clears of the call beside the first piece's match stage (run_encode)
    HIPCHK(c, hipEventRecord(c->ev_fill[0], st));
    HIPCHK(c, hipEventRecord(c->ev[0][0], st));
    if (cfg.use_quarter && cfg_cq(cfg) == 0) HIPCHK(c, hipMemsetAsync(w.Mq, 0, (n + 64) * 4, st));
    uint16_t* S = w.sorted + WINDOW_SIZE;
    const uint32_t n_ep = (uint32_t)((n + WINDOW_SIZE - 1) / WINDOW_SIZE);
    const uint32_t spe = WINDOW_SIZE / SEG;  // segments per epoch
    uint32_t e_lo = 0, seg_lo = 0;
    hipStream_t sb = two ? c->blk_stream : st;
    int np = 0;  // pieces of the stream (a piece of the arrival that completes no segment is worked on with the next)
    for (int k = 0; k < ar.n; k++) {
        const bool last = k + 1 == ar.n;
        const uint32_t e_hi = last ? n_ep : (ar.upto[k] < n_ep ? ar.upto[k] : n_ep);
        // (the sort of a piece on a stream of its own, beside the walk of the piece before, was measured and lost: 4.98 -> 5.3 ms
        // per call -- its workgroups take compute units the walk's next workgroups were about to get)
        {
            const int rc = arrival_wait(c, st, ar, k);
            if (rc) return rc;
        }
        ht("arrived", k);
        if (e_hi > e_lo) {
            launch_sort(c, st, e_hi - e_lo, d_in, n32, ov, S, w.buckets, e_lo);
            if (e_lo == 0) HIPCHK(c, hipEventRecord(c->ev[0][1], st));
            launch_walk(c, st, d_in, n32, S, w, cfg, aligned16, sg, ov, e_lo, e_hi - e_lo);
            if (last) HIPCHK(c, hipEventRecord(c->ev[0][2], st));
        }
        e_lo = e_hi;
        if (k == 0) {  // (queued behind the first match launches: nothing stands between the call and its first kernel)
            HIPCHK(c, hipStreamWaitEvent(c->fill, c->ev_fill[0], 0));
            HIPCHK(c, hipMemsetAsync(c->d_sc, 0, sizeof(DevScalars), c->fill));
            HIPCHK(c, hipMemsetAsync(d_out, 0, need_out, c->fill));
            HIPCHK(c, hipEventRecord(c->ev_fill[1], c->fill));
            HIPCHK(c, hipStreamWaitEvent(sb, c->ev_fill[1], 0));
        }
        // the segments whose restart steps can be taken: a step looks 260 positions ahead, and the ranges the check kernels
        // look at begin at multiples of 64 segments
        const uint32_t seg_hi = last ? w.K0 : (e_hi * spe > 64 ? (e_hi * spe - 64) / 64 * 64 : 0u);
        if (seg_hi <= seg_lo && !last) continue;
        const uint32_t p = (uint32_t)np++;
        if (sb != st) {  // the piece's match table is there when its walk is done
            HIPCHK(c, hipEventRecord(c->ev_walk[p], st));
            HIPCHK(c, hipStreamWaitEvent(sb, c->ev_walk[p], 0));
        }
        const Piece pc{seg_lo, p, last ? 1u : 0u};
        const uint32_t ns = seg_hi - seg_lo;
        if (ns) {
            const uint16_t* const steps = steps_in_emit(c, cfg, 1u) ? nullptr : w.adv;
            if (steps) hipLaunchKernelGGL(k_adv, dim3(ns), dim3(256), 0, sb, n32, w.M, Mq, cfg, w.adv, sg, seg_lo);
            const SegRange r{seg_hi, pc, d_in, n32, 0u, n32, 0u, sg, steps, w.levels[0].E, w.xs, w.fixlist + (size_t)2 * p * FIX_MAX,
                             &c->d_sc->n_fix[p], w.scan_part + seg_lo / 1024 + 2 * p, w.tend, w.pb};
            launch_spec_entries(c, sb, w, cfg, r);
            launch_token_scan(c, sb, w, r, false);
        } else {  // (an empty last piece cannot be: the last piece holds at least the 64 segments the one before it left)
            return MI355_OK;
        }
        // the blocks that became complete with this piece (at most one per 31744 bytes of it, the one that was open, the last)
        const uint32_t maxb = (uint32_t)((uint64_t)ns * SEG / MAX_BUFFER_LENGTH) + 3;
        hipLaunchKernelGGL(k_block_bounds, dim3(cdiv((uint64_t)maxb + 1, 4)), dim3(256), 0, sb, n32, seg_hi, w.nb_max, cfg.mode, sg, 0u,
                           w.tend, w.pb, w.base, w.levels[0].E, w.tokbuf, w.dtok, c->d_sc, w.bstart, w.q13, w.tab, pc,
                           (const uint32_t*)(w.xs + (seg_hi - 1)), 0u);
        MI355_LAUNCH_HIST(maxb * PSPLIT, c->n_cu, sb, w.dtok, c->d_sc, w.ll_freq, w.d_freq, w.tab, p,
                           (uint32_t*)nullptr, 0u);
        hipLaunchKernelGGL(k_block_header, dim3(maxb), dim3(128), 0, sb, c->d_sc, w.ll_freq, w.d_freq, w.hdr, p);
        hipLaunchKernelGGL(k_plan, dim3(1), dim3(1024), 0, sb, c->d_sc, w.hdr, w.bstart, w.q13, w.plan, bit_base, (uint32_t)o->compat,
                           w.tab.sync, reinterpret_cast<uint32_t*>(d_out), pc, (uint32_t*)nullptr);
        HIPCHK(c, hipMemcpyAsync(c->h_piece + (size_t)p * sizeof(DevState), c->d_sc, sizeof(DevState), hipMemcpyDeviceToHost, sb));
        HIPCHK(c, hipEventRecord(c->ev_plan[p], sb));
        MI355_LAUNCH_PACK(maxb * PSPLIT, c->n_cu, sb, d_in, n32, w.dtok, c->d_sc, w.hdr, w.plan, w.bstart, w.q13,
                           (uint32_t)o->compat, reinterpret_cast<uint32_t*>(d_out), w.tab, w.ll_freq, w.d_freq, p);
        HIPCHK(c, hipEventRecord(c->ev_pack[p], sb));
        seg_lo = seg_hi;
    }
    rc = launch_frame_tail(c, sb, d_in, n, o->wrapper, w, gz_hdr, gz_len, d_out, true);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->h_sc, c->d_sc, sizeof(DevState), hipMemcpyDeviceToHost, sb));
    // everything is queued; now hand the finished bytes over as the plans come in
    bool bad = false, q1 = false;
    uint64_t sent = 0;
    hsa_agent_t a_gpu, a_cpu;
    const bool by_engine = c->engine.load() && c->engine.agents(d_out, h_out, &a_gpu, &a_cpu);
    // (a pageable buffer: the pieces leave through the host threads' slots -- the copy engine into a slot, a thread on to the caller)
    Bounce* const by_threads = by_engine ? nullptr : bounce_for(c, h_out, out_cap);
    if (by_threads) {
        bounce_open(c);
        c->host_path |= MI355_HOST_PATH_OUT_THREADS;
    }
    ht("queued", np);
    for (int p = 0; p < np && !bad; p++) {
        HIPCHK(c, hipEventSynchronize(c->ev_plan[p]));
        ht("plan", p);
        const DevState* hs = reinterpret_cast<const DevState*>(c->h_piece + (size_t)p * sizeof(DevState));
        if (hs->spec_bad || hs->sort_bad || hs->sc.ref_panic) bad = true;
        uint64_t wpos = 0;
        // quirk Q1 (run_encode q1_fires): the single pass deals with it
        if (p == 0 && hs->sc.b0_full && q1_rewarm(hs->sc.b0_last_tok, hs->sc.b0_last_pos, cfg.mode, n, &wpos)) bad = q1 = true;
        if (bad || p + 1 == np) break;  // (the last piece's bytes go with the trailer, below)
        // whole bytes that are final: the byte the next block starts in is not
        uint64_t upto = (bit_base + hs->sc.total_bits) / 8;
        upto &= ~(uint64_t)4095;  // (whole pages: the engine's descriptors and the runtime's copies both like them)
        if (upto > sent && upto <= out_cap) {
            if (by_threads) {
                HIPCHK(c, hipEventSynchronize(c->ev_pack[p]));
                ht("pack", p);
                by_threads->out_push(h_out + sent, d_out + sent, (size_t)(upto - sent));
                c->host_path |= MI355_HOST_PATH_OUT_THREADS;
            } else if (by_engine) {
                HIPCHK(c, hipEventSynchronize(c->ev_pack[p]));
                ht("pack", p);
                if (!c->engine.start(h_out + sent, a_cpu, d_out + sent, a_gpu, (size_t)(upto - sent))) {
                    c->err = "hsa_amd_memory_async_copy failed";
                    (void)c->engine.wait_all();
                    (void)hipStreamSynchronize(st);
                    return MI355_E_HIP;
                }
            } else {
                HIPCHK(c, hipStreamWaitEvent(c->out_stream, c->ev_pack[p], 0));
                HIPCHK(c, hipMemcpyAsync(h_out + sent, d_out + sent, (size_t)(upto - sent), hipMemcpyDeviceToHost, c->out_stream));
            }
            sent = upto;
        }
    }
    HIPCHK(c, hipStreamSynchronize(st));
    if (sb != st) HIPCHK(c, hipStreamSynchronize(sb));
    ht("kernels done", 0);
    HIPCHK(c, hipGetLastError());
    const bool spec_off = spec_entries_failed(c);  // (both look at *c->h_sc and put the context right)
    const bool sort_off = sort_order_failed(c);
    const DevScalars& s = *c->h_sc;
    if (bad || spec_off || sort_off || s.ref_panic) {
        (void)hipStreamSynchronize(c->out_stream);
        (void)c->engine.wait_all();
        if (by_threads) (void)by_threads->out_wait();
        // (the single pass that follows parses the exact way; after a failed speculation and nothing else it finds the match
        // table and the restart steps of the whole input in the workspace)
        c->reuse_tables = spec_off && !sort_off && !q1 && !s.ref_panic;
        return MI355_OK;  // *redo stays set
    }
    const size_t total = stream_bytes(s.total_bits, o->wrapper, gz_len, false);
    *out_len = total;
    if (total > out_cap) {
        (void)hipStreamSynchronize(c->out_stream);
        (void)c->engine.wait_all();
        if (by_threads) (void)by_threads->out_wait();
        *redo = false;
        return MI355_E_OUT_TOO_SMALL;
    }
    const size_t hl = zlib ? 2 : gz_len;
    if (by_threads) {
        if (total > sent) by_threads->out_push(h_out + sent, d_out + sent, total - sent, true);
        if (!by_threads->out_wait()) {
            c->err = "host threads: a copy of the output failed";
            return MI355_E_HIP;
        }
        // (the frame kernels wrote the header bytes at the end, the first piece went out without them: the same bytes from here)
        const uint8_t zhead[2] = {0x78, 0x9C};  // zlib.rs:59-62 with the level the reference always passes (k_zlib_frame)
        if (hl && sent) memcpy(h_out, zlib ? zhead : gz_hdr, hl < sent ? hl : (size_t)sent);
    } else {
        if (total > sent) HIPCHK(c, hipMemcpyAsync(h_out + sent, d_out + sent, total - sent, hipMemcpyDeviceToHost, st));  // (both streams are idle)
        // (the frame kernels wrote the header bytes at the end: the first piece went out without them)
        if (hl && sent) HIPCHK(c, hipMemcpyAsync(h_out, d_out, hl < sent ? hl : (size_t)sent, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(c, hipStreamSynchronize(c->out_stream));
    HIPCHK(c, hipStreamSynchronize(st));
    if (!c->engine.wait_all()) {
        c->err = "copy engine: a device-to-host copy failed";
        return MI355_E_HIP;
    }
    c->host_path |= MI355_HOST_PATH_PIECES;
    ht("out", 0);
    if (host_trace) fprintf(stderr, "[host]%s ms (%s)\n", htl.c_str(), by_threads ? "host threads" : (by_engine ? "copy engine" : "runtime"));
    info.passes = 1;
    info_from_scalars(&info, s);
    info.out_len = total;
    c->last_crc = s.crc;
    c->last_plan = w.plan;  // (the block trace of mi355_deflate_last_blocks: the tables are the stream's, as in the single pass)
    c->last_nt = w.tab.nt;
    c->last_bstart = w.bstart;
    c->last_nb = s.nb;
    c->pend_passes = 0;
    *redo = false;
    return MI355_OK;
}

// The context's bounce threads, if this host buffer is one for them: pageable, large enough, not switched off.
Bounce* bounce_for(mi355_deflate_ctx* c, const void* host, uint64_t bytes) {
    if (!c->host_bounce || bytes < BOUNCE_FROM || !host_pageable(host)) return nullptr;
    if (!c->bounce) {
        if (!c->copy_stream && hipStreamCreate(&c->copy_stream) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        (void)c->engine.load();
        c->bounce = new Bounce;
        if (!c->bounce->start(c->device, &c->engine, c->copy_stream, c->host_threads > 0 ? c->host_threads : Bounce::default_threads())) {
            delete c->bounce;  // (no page-locked memory for the rings: the runtime's copies from here on)
            c->bounce = nullptr;
            c->host_bounce = 0;
            return nullptr;
        }
    }
    return c->bounce;
}
void bounce_open(mi355_deflate_ctx* c) {
    if (c->bounce && !c->bounce_on) {
        c->bounce->begin_session();
        c->bounce_on = true;
    }
}
// Before a host-buffer call returns: no thread touches the caller's buffers or the call's state any more.  `cancel`: the call
// failed, what is not yet copied is dropped.  false: a copy of the threads failed.
bool bounce_close(mi355_deflate_ctx* c, bool cancel) {
    if (!c->bounce || !c->bounce_on) return true;
    Bounce* b = c->bounce;
    b->in_finish(cancel);
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);  // (chunks on their way from the ring to the staging buffer)
    const bool good = b->out_wait() && b->err.load() == 0;
    b->end_session();
    c->bounce_on = false;
    return good;
}
// finished bytes from the device to a pageable host buffer through the threads; false: not this way (the caller copies)
bool bounce_out(mi355_deflate_ctx* c, uint8_t* h_dst, const uint8_t* d_src, size_t bytes) {
    Bounce* b = bounce_for(c, h_dst, bytes);
    if (!b) return false;
    bounce_open(c);
    b->out_push(h_dst, d_src, bytes, true);
    c->host_path |= MI355_HOST_PATH_OUT_THREADS;
    return true;
}

// A host buffer on its way to the device in pieces of whole rounds of k_match3 workgroups (one per CU) on the context's copy
// stream: the first is one round (8 MiB: the first kernel starts after 0.16 ms), the next ones `grow_to` at most -- the bus brings
// ~55 GB/s, sort + walk take ~20 GB/s at Default, so each has arrived before the one before it is done -- and piece
// `max_pieces` takes the rest.  ar.ev[k] fires when the bytes of the first ar.upto[k] epochs and the look-ahead behind them
// are there (launch_match_tables, run_streamed).
int arrive_in_pieces(mi355_deflate_ctx* c, uint8_t* d_dst, const uint8_t* h_src, uint64_t n, Arrival& ar, uint64_t grow_to, int max_pieces,
                     bool doubling) {
    if (!c->copy_stream && hipStreamCreate(&c->copy_stream) != hipSuccess) return fail_hip(c, "hipStreamCreate", hipGetLastError());
    if (!c->arrive_ok) {
        for (int k = 0; k < ARRIVE_MAX; k++)
            if (hipEventCreateWithFlags(&c->arrive[k], hipEventDisableTiming) != hipSuccess)
                return fail_hip(c, "hipEventCreate", hipGetLastError());
        c->arrive_ok = true;
    }
    const uint64_t n_ep = (n + WINDOW_SIZE - 1) / WINDOW_SIZE;
    const uint64_t round = c->n_cu ? c->n_cu : 256;
    ar.ev = c->arrive;
    ar.n = 0;
    uint64_t upto = 0, grow = 1;
    // (development aid: MI355_HOST_PLAN="1,2,3,3" gives the rounds of the pieces one by one; the last piece takes the rest)
    static const char* const plan_env = getenv("MI355_HOST_PLAN");
    const char* pe = doubling ? nullptr : plan_env;
    // (the first piece of a host input is a quarter of a round, walked in four parts per epoch: the first kernel starts 0.1 ms
    // earlier than behind a whole round's bytes, and the round that follows is there when that piece is done)
    static const char* const first_env = getenv("MI355_HOST_FIRST");
    const uint64_t first = doubling ? 0 : (first_env ? strtoull(first_env, nullptr, 10) : HOST_FIRST_EPOCHS);
    if (first && n_ep > first + 2 * round && max_pieces > 2) {
        upto = first;
        ar.upto[ar.n++] = (uint32_t)upto;
    }
    while (upto < n_ep && ar.n < ARRIVE_MAX) {
        if (pe && *pe) {
            grow = strtoull(pe, const_cast<char**>(&pe), 10);
            if (*pe == ',') pe++;
            if (grow == 0) grow = 1;
            if (!*pe) max_pieces = ar.n + 2;
        }
        upto += grow * round;
        if (ar.n + 1 == ARRIVE_MAX || ar.n + 1 == max_pieces || upto + round > n_ep) upto = n_ep;
        ar.upto[ar.n++] = (uint32_t)upto;
        if (doubling)
            grow *= 2;
        else if (grow < grow_to)
            grow++;
    }
    uint64_t sent = 0;
    ar.gate = nullptr;
    if (Bounce* b = bounce_for(c, h_src, n)) {  // pageable memory: the context's host threads carry it (deflate_bounce.inc)
        uint64_t ends[ARRIVE_MAX];
        for (int k = 0; k < ar.n; k++) {
            const uint64_t want = ((uint64_t)ar.upto[k] + 1) * WINDOW_SIZE;
            ends[k] = (k + 1 == ar.n || want > n) ? n : want;
        }
        bounce_open(c);
        b->in_begin(h_src, d_dst, n, ar.n, ends, c->arrive);
        ar.gate = b;
        c->host_path |= MI355_HOST_PATH_IN_THREADS;
        return MI355_OK;
    }
    for (int k = 0; k < ar.n; k++) {
        // (+ one epoch: the look-ahead of the piece's last positions and the 258 bytes behind its last epoch)
        const uint64_t want = ((uint64_t)ar.upto[k] + 1) * WINDOW_SIZE;
        const uint64_t end = (k + 1 == ar.n || want > n) ? n : want;
        if (end > sent) {
            if (hipMemcpyAsync(d_dst + sent, h_src + sent, end - sent, hipMemcpyHostToDevice, c->copy_stream) != hipSuccess) {
                const int rc = fail_hip(c, "hipMemcpyAsync(piece)", hipGetLastError());
                (void)hipStreamSynchronize(c->copy_stream);  // the caller's buffer is no longer read when we return
                return rc;
            }
            sent = end;
        }
        HIPCHK(c, hipEventRecord(c->arrive[k], c->copy_stream));
    }
    return MI355_OK;
}

std::mutex g_default_mu;
mi355_deflate_ctx* g_default_ctx = nullptr;
// Calls that run on the process-wide default context (ctx == NULL) hold this lock from entry to return:
// the context's workspace, staging buffers, events and error string are single-owner state.
std::recursive_mutex g_default_call_mu;
struct DefaultGuard {
    std::unique_lock<std::recursive_mutex> lk;
};

}  // namespace

extern "C" {

int mi355_deflate_version(void) { return MI355_DEFLATE_VERSION; }

// Every block is at most its stored form (huffman_lengths.rs:269-286 picks the cheapest): its bytes, 5 per
// stored piece, a pad.  Blocks end every 31744 tokens and at every sync flush, which adds its marker
// (3 bits, pad, 00 00 FF FF).
size_t mi355_deflate_bound_ex(size_t n, int wrapper, size_t hdr_len, size_t n_flush) {
    size_t b = n + 5 * (n / MAX_BUFFER_LENGTH + n / MAX_STORED_BLOCK_LENGTH + 2) + 16 + 12 * n_flush;
    if (wrapper == 1) b += 6;
    if (wrapper == 2) b += hdr_len + 8;
    return align_up(b, 8) + 8;
}
size_t mi355_deflate_bound(size_t n) { return mi355_deflate_bound_ex(n, 2, 10, 0); }

int mi355_deflate_preset(int level, mi355_deflate_opts* out) {
    if (!out) return MI355_E_ARG;
    mi355_deflate_opts o;
    memset(&o, 0, sizeof o);
    switch (level) {  // compression_options.rs:126-196
    case MI355_LEVEL_FAST: o.max_hash_checks = 1; o.lazy_if_less_than = 0; o.matching_type = 0; break;
    case MI355_LEVEL_DEFAULT: o.max_hash_checks = 128; o.lazy_if_less_than = 32; o.matching_type = 1; break;
    case MI355_LEVEL_BEST: o.max_hash_checks = 1768; o.lazy_if_less_than = 128; o.matching_type = 1; break;
    case MI355_LEVEL_RLE: o.max_hash_checks = 0; o.lazy_if_less_than = 0; o.matching_type = 1; break;
    case MI355_LEVEL_HUFFMAN_ONLY: o.max_hash_checks = 0; o.lazy_if_less_than = 0; o.matching_type = 0; break;
    default: return MI355_E_ARG;
    }
    *out = o;
    return MI355_OK;
}

int mi355_deflate_ctx_create(int device, mi355_deflate_ctx** out) {
    if (!out) return MI355_E_ARG;
    *out = nullptr;
    mi355_deflate_ctx* c = new mi355_deflate_ctx();
    c->device = device;
    memset(&c->info, 0, sizeof c->info);
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= device) {
        // no silent fallback: without a usable HIP device the library refuses to work
        fprintf(stderr, "mi355_deflate: no usable HIP device %d (%s)\n", device,
                e != hipSuccess ? hipGetErrorString(e) : "device index out of range");
        delete c;
        return MI355_E_HIP;
    }
    if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&c->own_stream) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&c->d_sc), sizeof(DevState)) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(&c->h_sc), sizeof(DevState), hipHostMallocDefault) != hipSuccess ||
        hipStreamCreateWithFlags(&c->fill, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_fill[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_fill[1], hipEventDisableTiming) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(&c->h_ends), H_ENDS_CAP * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess) {
        fprintf(stderr, "mi355_deflate: HIP context setup failed on device %d\n", device);
        delete c;
        return MI355_E_HIP;
    }
    for (int p = 0; p < MAX_PASSES; p++)
        for (int i = 0; i < N_EV; i++)
            if (hipEventCreate(&c->ev[p][i]) != hipSuccess) {
                delete c;
                return MI355_E_HIP;
            }
    c->ev_ok = true;
    if (const char* e = getenv("MI355_STAGE_CLOCKS"))  // (measuring aid: the default of MI355_CFG_STAGE_CLOCKS)
        if (e[0] >= '0' && e[0] <= '2' && !e[1]) c->stage_clocks = e[0] - '0';
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
        c->n_cu = (uint32_t)cus;
    {   // k_sort's ranks from returning LDS atomics need the LDS to serve one address in lane order: checked here, once per
        // context, on every CU a few times over (0.1 ms of kernel).  mi355_deflate_ctx_config(MI355_CFG_SORT_RANKS) overrides.
        uint32_t* bad = reinterpret_cast<uint32_t*>(c->d_sc);
        uint32_t h_bad = 1;
        if (hipMemsetAsync(c->d_sc, 0, sizeof(DevState), c->own_stream) == hipSuccess) {
            hipLaunchKernelGGL(k_lds_order_test, dim3(2 * (c->n_cu ? c->n_cu : 256u)), dim3(1024), 0, c->own_stream, 96u, bad);
            if (hipMemcpyAsync(&h_bad, bad, sizeof(uint32_t), hipMemcpyDeviceToHost, c->own_stream) != hipSuccess ||
                hipStreamSynchronize(c->own_stream) != hipSuccess)
                h_bad = 1;
        }
        (void)hipGetLastError();
        c->lds_order_ok = h_bad == 0;
        c->sort_mode = c->lds_order_ok ? 1 : 0;
    }
    *out = c;
    return MI355_OK;
}

void mi355_deflate_ctx_destroy(mi355_deflate_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);  // nothing of this context may still be in flight
    if (c->fill) (void)hipStreamSynchronize(c->fill);
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    delete c->bounce;  // (joins the host threads; their slots go with them)
    c->bounce = nullptr;
    if (c->ev_ok)
        for (int p = 0; p < MAX_PASSES; p++)
            for (int i = 0; i < N_EV; i++) (void)hipEventDestroy(c->ev[p][i]);
    if (c->shard_cache) shard_destroy(c->shard_cache);
    c->shard_cache = nullptr;
    if (c->ws) (void)hipFree(c->ws);
    if (c->d_in) (void)hipFree(c->d_in);
    if (c->d_out) (void)hipFree(c->d_out);
    if (c->d_crc) (void)hipFree(c->d_crc);
    if (c->d_sc) (void)hipFree(c->d_sc);
    if (c->h_sc) (void)hipHostFree(c->h_sc);
    for (int k = 0; k < 2; k++)
        if (c->ev_fill[k]) (void)hipEventDestroy(c->ev_fill[k]);
    if (c->fill) (void)hipStreamDestroy(c->fill);
    if (c->h_ends) (void)hipHostFree(c->h_ends);
    if (c->arrive_ok)
        for (int k = 0; k < ARRIVE_MAX; k++) (void)hipEventDestroy(c->arrive[k]);
    if (c->out_ok)
        for (int k = 0; k < ARRIVE_MAX; k++) {
            (void)hipEventDestroy(c->ev_plan[k]);
            (void)hipEventDestroy(c->ev_pack[k]);
            (void)hipEventDestroy(c->ev_walk[k]);
        }
    if (c->out_stream) (void)hipStreamDestroy(c->out_stream);
    if (c->blk_stream) (void)hipStreamDestroy(c->blk_stream);
    if (c->h_piece) (void)hipHostFree(c->h_piece);
    if (c->b_dev) (void)hipFree(c->b_dev);
    if (c->b_host) (void)hipHostFree(c->b_host);
    if (c->v_dev) (void)hipFree(c->v_dev);
    if (c->v_host) (void)hipHostFree(c->v_host);
    if (c->t_dev) (void)hipFree(c->t_dev);
    if (c->t_ev_ok)
        for (int k = 0; k < 4; k++) (void)hipEventDestroy(c->t_ev[k]);
    if (c->sk_ev_ok)
        for (int k = 0; k < 5; k++) (void)hipEventDestroy(c->sk_ev[k]);
    if (c->x_ev_ok)
        for (int k = 0; k < 3; k++) (void)hipEventDestroy(c->x_ev[k]);
    if (c->m_dev) (void)hipFree(c->m_dev);
    if (c->m_rows) (void)hipFree(c->m_rows);
    if (c->mp_dev) (void)hipFree(c->mp_dev);
    if (c->m_ev_ok)
        for (int k = 0; k < 2; k++) (void)hipEventDestroy(c->m_ev[k]);
    if (c->mp_ev_ok)
        for (int k = 0; k < 4; k++) (void)hipEventDestroy(c->mp_ev[k]);
    if (c->bz_arena) (void)hipFree(c->bz_arena);
    if (c->bz_tab) (void)hipFree(c->bz_tab);
    if (c->bz_host) (void)hipHostFree(c->bz_host);
    if (c->bz_out) (void)hipFree(c->bz_out);
    if (c->bz_ev_ok)
        for (int k = 0; k < 4; k++) (void)hipEventDestroy(c->bz_ev[k]);
    if (c->br_ev_ok)
        for (int k = 0; k < 5; k++) (void)hipEventDestroy(c->br_ev[k]);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

const char* mi355_deflate_last_error(mi355_deflate_ctx* c) { return c ? c->err.c_str() : "no context"; }

int mi355_deflate_last_info(mi355_deflate_ctx* c, mi355_deflate_info* info) {
    if (!c || !info) return MI355_E_ARG;
    if (c->pend_passes) {
        (void)hipSetDevice(c->device);
        for (int p = 0; p < c->pend_passes; p++) {
            hipEvent_t* e = c->ev[p];
            float ms = 0;
            const int stage_of[6] = {MI355_STAGE_LINKS, MI355_STAGE_MATCH, MI355_STAGE_PARSE, MI355_STAGE_BLOCKS,
                                     MI355_STAGE_PACK, MI355_STAGE_OTHER};
            if (!c->pend_clocks) continue;  // (a small call: no events; total_ms is the host's clock)
            for (int i = 0; i < c->pend_last[p]; i++) {
                if (hipEventElapsedTime(&ms, e[i], e[i + 1]) == hipSuccess) {
                    c->info.stage_ms[stage_of[i]] += ms;
                    c->info.total_ms += ms;
                    if (i == 1) {
                        c->info.match_ms += ms;
                        c->info.match_launches += 1;
                    }
                }
            }
        }
        c->pend_passes = 0;
    }
    *info = c->info;
    return MI355_OK;
}

int mi355_deflate_last_blocks(mi355_deflate_ctx* c, mi355_block_info* out, size_t cap, size_t* n_blocks) {
    if (!c || !n_blocks) return MI355_E_ARG;
    *n_blocks = c->last_nb;
    if (!out || !c->last_plan || c->last_nb == 0) return MI355_OK;
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<BlockPlan> plan(c->last_nb);
    std::vector<uint32_t> bs(c->last_nb + 1), nts(c->last_nb);
    HIPCHK(c, hipMemcpy(plan.data(), c->last_plan, sizeof(BlockPlan) * c->last_nb, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(nts.data(), c->last_nt, sizeof(uint32_t) * c->last_nb, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(bs.data(), c->last_bstart, sizeof(uint32_t) * (c->last_nb + 1), hipMemcpyDeviceToHost));
    for (size_t b = 0; b < c->last_nb && b < cap; b++) {
        out[b].btype = plan[b].btype;
        out[b].bfinal = plan[b].bfinal;
        out[b].n_tokens = nts[b];
        out[b].reserved = 0;
        out[b].in_bytes = (uint64_t)bs[b + 1] - bs[b];
        out[b].bit_start = plan[b].bit_start - c->last_bit_base;
    }
    return MI355_OK;
}

static mi355_deflate_ctx* default_ctx() {
    std::lock_guard<std::mutex> g(g_default_mu);
    if (!g_default_ctx) mi355_deflate_ctx_create(0, &g_default_ctx);
    return g_default_ctx;
}
// the context a call works on; the default one comes with its lock
static mi355_deflate_ctx* use_ctx(mi355_deflate_ctx* c, DefaultGuard& g) {
    if (c && c != g_default_ctx) return c;
    g.lk = std::unique_lock<std::recursive_mutex>(g_default_call_mu);
    return c ? c : default_ctx();
}

// Grow the workspace (and the staging buffers of the host-buffer API when `host_api` is set) for inputs of
// up to in_len bytes now, so that the first encode does not pay for hipMalloc.
int mi355_deflate_ctx_reserve(mi355_deflate_ctx* c, size_t in_len, int host_api) {
    DefaultGuard dg_;
    c = use_ctx(c, dg_);
    if (!c) return MI355_E_HIP;
    if (in_len >= 0xFFFF0000ull) return MI355_E_UNSUPPORTED;
    HIPCHK(c, hipSetDevice(c->device));
    Workspace sz = carve(nullptr, in_len, true, 1, 0);
    int rc = ensure_ws(c, sz.bytes);
    if (rc) return rc;
    if (host_api) {
        rc = ensure_buf(c, &c->d_in, &c->d_in_cap, in_len + 64);
        if (rc) return rc;
        rc = ensure_buf(c, &c->d_out, &c->d_out_cap, mi355_deflate_bound_ex(in_len, 2, 64, 4) + 64);
        if (rc) return rc;
    }
    return MI355_OK;
}

int mi355_deflate_encode_device(mi355_deflate_ctx* c, const void* d_in, size_t in_len, const mi355_deflate_opts* opts,
                                void* d_out, size_t out_cap, size_t* out_len, void* hip_stream) {
    DefaultGuard dg_;
    c = use_ctx(c, dg_);
    if (!c) return MI355_E_HIP;
    if (!opts || !out_len || !d_out || (!d_in && in_len)) return MI355_E_ARG;
    if (reinterpret_cast<uintptr_t>(d_out) & 3) {
        c->err = "d_out must be 4-byte aligned";
        return MI355_E_ARG;
    }
    hipStream_t st = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : c->own_stream;
    if (goes_long(c, in_len, opts)) {  // any length, in ranges (deflate_long.inc); the work runs on the context's own stream
        if (hip_stream) HIPCHK(c, hipStreamSynchronize(st));
        return encode_long(c, reinterpret_cast<const uint8_t*>(d_in), nullptr, in_len, opts, reinterpret_cast<uint8_t*>(d_out), nullptr,
                           out_cap, out_len, kBlankGzipHeader, 10);
    }
    if (opts->wrapper == 2)
        return run_encode(c, reinterpret_cast<const uint8_t*>(d_in), in_len, opts, reinterpret_cast<uint8_t*>(d_out),
                          out_cap, out_len, st, nullptr, nullptr, kBlankGzipHeader, 10);
    return run_encode(c, reinterpret_cast<const uint8_t*>(d_in), in_len, opts, reinterpret_cast<uint8_t*>(d_out),
                      out_cap, out_len, st);
}

static int encode_host(mi355_deflate_ctx* c, const uint8_t* in, size_t in_len, const mi355_deflate_opts* opts,
                       uint8_t* out, size_t out_cap, size_t* out_len, const std::vector<uint32_t>* ends,
                       const std::vector<uint32_t>* rewarm = nullptr, const uint8_t* gz_hdr = nullptr, size_t gz_len = 0,
                       EncodeExtra* extra = nullptr);


int mi355_deflate_encode(mi355_deflate_ctx* c, const uint8_t* in, size_t in_len, const mi355_deflate_opts* opts,
                         uint8_t* out, size_t out_cap, size_t* out_len) {
    if (opts && opts->wrapper == 2)
        return encode_host(c, in, in_len, opts, out, out_cap, out_len, nullptr, nullptr, kBlankGzipHeader, 10);
    return encode_host(c, in, in_len, opts, out, out_cap, out_len, nullptr);
}

int mi355_deflate_encode_gzip(mi355_deflate_ctx* c, const uint8_t* in, size_t in_len, const mi355_deflate_opts* opts,
                              const uint8_t* hdr, size_t hdr_len, uint8_t* out, size_t out_cap, size_t* out_len) {
    if (!opts || !hdr || hdr_len == 0) return MI355_E_ARG;
    mi355_deflate_opts o = *opts;
    o.wrapper = 2;
    return encode_host(c, in, in_len, &o, out, out_cap, out_len, nullptr, nullptr, hdr, hdr_len);
}

int mi355_deflate_encode_device_gzip(mi355_deflate_ctx* c, const void* d_in, size_t in_len,
                                     const mi355_deflate_opts* opts, const uint8_t* hdr, size_t hdr_len, void* d_out,
                                     size_t out_cap, size_t* out_len, void* hip_stream) {
    DefaultGuard dg_;
    c = use_ctx(c, dg_);
    if (!c) return MI355_E_HIP;
    if (!opts || !out_len || !d_out || (!d_in && in_len) || !hdr || hdr_len == 0) return MI355_E_ARG;
    if (reinterpret_cast<uintptr_t>(d_out) & 3) {
        c->err = "d_out must be 4-byte aligned";
        return MI355_E_ARG;
    }
    mi355_deflate_opts o = *opts;
    o.wrapper = 2;
    hipStream_t st = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : c->own_stream;
    if (goes_long(c, in_len, &o)) {
        if (hip_stream) HIPCHK(c, hipStreamSynchronize(st));
        return encode_long(c, reinterpret_cast<const uint8_t*>(d_in), nullptr, in_len, &o, reinterpret_cast<uint8_t*>(d_out), nullptr,
                           out_cap, out_len, hdr, hdr_len);
    }
    return run_encode(c, reinterpret_cast<const uint8_t*>(d_in), in_len, &o, reinterpret_cast<uint8_t*>(d_out),
                      out_cap, out_len, st, nullptr, nullptr, hdr, hdr_len);
}

static int encode_host_body(mi355_deflate_ctx* c, const uint8_t* in, size_t in_len, const mi355_deflate_opts* opts,
                            uint8_t* out, size_t out_cap, size_t* out_len, const std::vector<uint32_t>* ends,
                            const std::vector<uint32_t>* rewarm, const uint8_t* gz_hdr, size_t gz_len, EncodeExtra* extra);

static int encode_host(mi355_deflate_ctx* c, const uint8_t* in, size_t in_len, const mi355_deflate_opts* opts,
                       uint8_t* out, size_t out_cap, size_t* out_len, const std::vector<uint32_t>* ends,
                       const std::vector<uint32_t>* rewarm, const uint8_t* gz_hdr, size_t gz_len, EncodeExtra* extra) {
    DefaultGuard dg_;
    c = use_ctx(c, dg_);
    if (!c) return MI355_E_HIP;
    if (!opts || !out_len || (!in && in_len) || (!out && out_cap)) return MI355_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    c->host_path = 0;
    int rc = encode_host_body(c, in, in_len, opts, out, out_cap, out_len, ends, rewarm, gz_hdr, gz_len, extra);
    // (pageable buffers: the host threads are done with the caller's memory, whatever way the call ended)
    if (!bounce_close(c, rc != MI355_OK) && rc == MI355_OK) {
        c->err = "host threads: a copy failed";
        rc = MI355_E_HIP;
    }
    c->info.host_path = c->host_path;
    return rc;
}

static int encode_host_body(mi355_deflate_ctx* c, const uint8_t* in, size_t in_len, const mi355_deflate_opts* opts,
                            uint8_t* out, size_t out_cap, size_t* out_len, const std::vector<uint32_t>* ends,
                            const std::vector<uint32_t>* rewarm, const uint8_t* gz_hdr, size_t gz_len, EncodeExtra* extra) {
    if (goes_long(c, in_len, opts) && !ends && !rewarm && !extra)  // any length, in ranges (deflate_long.inc)
        return encode_long(c, nullptr, in, in_len, opts, nullptr, out, out_cap, out_len, gz_hdr, gz_len);
    size_t ob = mi355_deflate_bound_ex(in_len, opts->wrapper, gz_len, ends ? ends->size() : 0) + 8;
    int rc = ensure_buf(c, &c->d_in, &c->d_in_cap, in_len + 64);
    if (rc) return rc;
    rc = ensure_buf(c, &c->d_out, &c->d_out_cap, ob);
    if (rc) return rc;
    hipStream_t st = c->own_stream;
    // A large plain one-shot input goes over in pieces on a stream of its own, and the match stage works on a piece
    // while the next ones are still on the bus (arrive_in_pieces; run_encode / launch_match_tables / run_streamed): 1, 2, 3, 3 ...
    // rounds of workgroups -- pieces stay small towards the end because the OUTPUT leaves piece by piece as well.
    EncodeExtra local_extra;
    // (a pageable input from 4 MiB on travels through the host threads as well: below 16 MiB as one piece)
    const bool piecewise = (in_len >= HOST_PIECEWISE_FROM || bounce_for(c, in, in_len)) && !ends && !rewarm && !extra;
    if (piecewise) {
        rc = arrive_in_pieces(c, c->d_in, in, in_len, local_extra.arrival, HOST_PIECE_ROUNDS, HOST_PIECES, false);
        if (rc) return rc;
        extra = &local_extra;
    } else if (in_len) {
        HIPCHK(c, hipMemcpyAsync(c->d_in, in, in_len, hipMemcpyHostToDevice, st));
    }
    size_t n = 0;
    if (piecewise && c->host_streaming) {  // worked on and delivered piece by piece, when nothing is out of the ordinary (run_streamed)
        bool redo = true;
        rc = out_cap >= mi355_deflate_bound_ex(in_len, opts->wrapper, gz_len, 0)
                 ? run_streamed(c, c->d_in, in_len, opts, c->d_out, ob, out, out_cap, out_len, gz_hdr, gz_len, local_extra.arrival, &redo)
                 : MI355_OK;
        if (rc || !redo) {
            (void)hipStreamSynchronize(c->copy_stream);
            if (rc) (void)hipStreamSynchronize(st);
            return rc;
        }
    }
    rc = run_encode(c, c->d_in, in_len, opts, c->d_out, ob, &n, st, ends, rewarm, gz_hdr, gz_len, extra);
    if (piecewise) {
        (void)hipStreamSynchronize(c->copy_stream);
        extra = nullptr;
    }
    if (rc) {
        (void)hipStreamSynchronize(st);  // (an early error return may have left the copy of the caller's buffer in flight)
        return rc;
    }
    const size_t skip = extra ? extra->skip_bytes : 0;
    if (skip > n) return MI355_E_ARG;
    *out_len = n - skip;
    if (n - skip > out_cap) return MI355_E_OUT_TOO_SMALL;
    if (n - skip) {
        // (run_encode has waited for its last kernel: the bytes are final.  Pageable memory: through the host threads)
        if (!bounce_out(c, out, c->d_out + skip, n - skip))
            HIPCHK(c, hipMemcpyAsync(out, c->d_out + skip, n - skip, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(c, hipStreamSynchronize(st));
    return MI355_OK;
}

int mi355_adler32_device(mi355_deflate_ctx* c, const void* d_in, size_t n, uint32_t* adler, void* hip_stream) {
    DefaultGuard dg_;
    c = use_ctx(c, dg_);
    if (!c) return MI355_E_HIP;
    if (!adler || (!d_in && n) || n >= 0xFFFF0000ull) return MI355_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : c->own_stream;
    if (const int rc = launch_sums_one(c, st, 1, reinterpret_cast<const uint8_t*>(d_in), n)) return rc;
    HIPCHK(c, hipMemcpyAsync(c->h_sc, c->d_sc, sizeof(DevScalars), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    *adler = c->h_sc->adler;
    return MI355_OK;
}

int mi355_crc32_device(mi355_deflate_ctx* c, const void* d_in, size_t n, uint32_t* crc, void* hip_stream) {
    DefaultGuard dg_;
    c = use_ctx(c, dg_);
    if (!c) return MI355_E_HIP;
    if (!crc || (!d_in && n) || n >= 0xFFFF0000ull) return MI355_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : c->own_stream;
    if (const int rc = launch_sums_one(c, st, 2, reinterpret_cast<const uint8_t*>(d_in), n)) return rc;
    HIPCHK(c, hipMemcpyAsync(c->h_sc, c->d_sc, sizeof(DevScalars), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    *crc = c->h_sc->crc;
    return MI355_OK;
}

}  // extern "C"

#ifdef MI355_MATCH_STATS
extern "C" int mi355_debug_match_stats(unsigned long long* out16, int reset) {
    if (out16 && hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_mstats), sizeof(g_mstats)) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[16] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_mstats), z, sizeof z) != hipSuccess) return -1;
    }
    return 0;
}
extern "C" int mi355_debug_sort_stats(unsigned long long* out16, int reset) {
    if (out16 && hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_sstats), sizeof(g_sstats)) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[16] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_sstats), z, sizeof z) != hipSuccess) return -1;
    }
    return 0;
}
#endif

// ---- streaming encoder (writer.rs:89-290) ---------------------------------------------------
// write() gathers bytes; flush() (Flush::Sync) and finish() encode what has arrived since the last flush
// on the GPU and hand the bytes out at once.  What a later segment can see of the stream behind it is the
// last 32768 bytes (hash chains and window are a pure function of them) and nothing else -- a sync flush
// ends the block, empties the token buffer and leaves the output byte aligned (compress.rs:256-261,
// lz77.rs:728-740) -- so a segment is encoded from a buffer that starts at a 32 KiB-aligned point at least
// one window before it, as a stream whose first segment (the history) is thrown away.  The first three
// windows of a stream are different: Q1, the hash re-warm at early flush points and the first-window
// geometry depend on absolute positions, so until the flushed part has passed them the buffer starts at
// position 0 and carries every flush point so far.
struct mi355_deflate_stream {
    mi355_deflate_ctx* ctx;
    mi355_deflate_opts opts;
    std::vector<uint8_t> win;            // the stream from `base` on
    uint64_t base = 0;                   // stream position of win[0] (a multiple of 32768)
    uint64_t total = 0;                  // bytes written
    uint64_t emitted = 0;                // the last flush point: everything before it has been handed out
    std::vector<uint64_t> flush_points;  // flush points at or after `base`, ascending (stream positions)
    std::vector<uint32_t> rewarm;        // flush points at which the reference re-warms its hash (see write)
    std::vector<uint64_t> skew, holes;   // stages.h HashOverride: one-byte writes after a flush, flushes after 1-2 bytes
    bool after_flush = false;            // the next write is the first one after a flush
    bool header_out = false;             // zlib / gzip header handed out (at the first write, else at finish)
    uint32_t adler = 1;                  // zlib: Adler-32, gzip: CRC-32 of what has been encoded so far
    uint64_t summed = 0;                 // bytes the checksum covers
    std::vector<uint8_t> gz_hdr;         // gzip: GzBuilder::into_header() as given by the caller
    std::vector<uint8_t> output;         // bytes produced and not yet taken
    size_t taken = 0;
    std::vector<uint8_t> handed_out;     // what reset() returned
    bool finished = false;
    bool q1_on = false;                  // a flush call of this stream, encoded from the stream's start, re-warmed two hashes (Q1) ...
    uint64_t q1_pos = 0;                 // ... at this position: the ranges behind a flush in the first windows start from that
    bool failed = false;                 // a range of a never-flushed stream could not be encoded: the handle's position in the
                                         // stream is lost, every later call answers MI355_E_STATE
    LongEnc* L = nullptr;                // deflate_long.inc: a stream that was never flushed hands its ranges over as they fill
};

namespace {

// zlib's adler32_combine / crc32_combine: the checksum of A || B from those of A and B and |B|
uint32_t adler_combine(uint32_t a1, uint32_t a2, uint64_t len2) {
    const uint32_t BASE = 65521u;
    const uint32_t rem = (uint32_t)(len2 % BASE);
    uint32_t sum1 = a1 & 0xffff, sum2 = (uint32_t)(((uint64_t)rem * sum1) % BASE);
    sum1 += (a2 & 0xffff) + BASE - 1;
    sum2 += ((a1 >> 16) & 0xffff) + ((a2 >> 16) & 0xffff) + BASE - rem;
    if (sum1 >= BASE) sum1 -= BASE;
    if (sum1 >= BASE) sum1 -= BASE;
    if (sum2 >= (BASE << 1)) sum2 -= (BASE << 1);
    if (sum2 >= BASE) sum2 -= BASE;
    return sum1 | (sum2 << 16);
}
uint32_t crc_mulmod_host(uint32_t a, uint32_t b) {  // a(x) * b(x) mod P, reflected (bit 31 = x^0)
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) {
        if (a & 0x80000000u) p ^= b;
        a <<= 1;
        b = (b >> 1) ^ ((b & 1u) ? 0xEDB88320u : 0u);
    }
    return p;
}
uint32_t crc_combine(uint32_t c1, uint32_t c2, uint64_t len2) {  // crc(A || B) = x^(8|B|) crc(A) + crc(B)
    uint32_t r = 0x80000000u, sq = 0x00800000u;
    for (uint64_t k = len2; k; k >>= 1) {
        if (k & 1) r = crc_mulmod_host(sq, r);
        sq = crc_mulmod_host(sq, sq);
    }
    return crc_mulmod_host(r, c1) ^ c2;
}

void stream_put(mi355_deflate_stream* s, const uint8_t* p, size_t n) { s->output.insert(s->output.end(), p, p + n); }

void stream_header(mi355_deflate_stream* s) {  // writer.rs:226-232 / :360-368
    if (s->header_out) return;
    s->header_out = true;
    if (s->opts.wrapper == 1) {
        const uint8_t h[2] = {0x78, 0x9C};  // zlib.rs:59-62 with the level the reference always passes (Q9)
        stream_put(s, h, 2);
    } else if (s->opts.wrapper == 2) {
        if (s->gz_hdr.empty()) s->gz_hdr.assign(kBlankGzipHeader, kBlankGzipHeader + 10);
        stream_put(s, s->gz_hdr.data(), s->gz_hdr.size());
    }
}

// flush() / finish(): encode [emitted, total) with the history it can see, hand the bytes out
int stream_encode(mi355_deflate_stream* s, bool finish) {
    mi355_deflate_ctx* c = s->ctx;
    const size_t n = (size_t)(s->total - s->base);
    if (n >= 0xFFFF0000ull) return MI355_E_UNSUPPORTED;
    std::vector<uint32_t> ends;
    for (uint64_t f : s->flush_points) ends.push_back((uint32_t)(f - s->base));
    EncodeExtra ex;
    ex.mid_stream = s->base != 0;
    std::vector<uint32_t> skew, holes;
    for (uint64_t f : s->skew)
        if (f >= s->base) skew.push_back((uint32_t)(f - s->base));
    for (uint64_t f : s->holes)
        if (f >= s->base) holes.push_back((uint32_t)(f - s->base));
    ex.skew = &skew;
    ex.holes = &holes;
    if (finish) {
        ex.skip_segments = ends.size();
        ends.push_back((uint32_t)n);
    } else {
        ex.skip_segments = ends.size() - 1;  // (flush() has just pushed the point this call is for)
    }
    mi355_deflate_opts o = s->opts;
    o.wrapper = 0;  // framing is done here: header at the first write, trailer at finish
    o.flush = finish ? MI355_FLUSH_FINISH : MI355_FLUSH_SYNC;
    const size_t cap = mi355_deflate_bound_ex(n, 0, 0, ends.size()) + 16;
    const size_t at = s->output.size();
    s->output.resize(at + cap);
    size_t got = 0;
    int rc = encode_host(c, s->win.data(), n, &o, s->output.data() + at, cap, &got, &ends,
                         s->base == 0 ? &s->rewarm : nullptr, nullptr, 0, &ex);
    if (rc) {
        s->output.resize(at);
        return rc;
    }
    s->output.resize(at + got);
    if (s->base == 0) {  // (Q1 is decided by the first window of the stream: every such call finds the same answer)
        s->q1_on = c->q1_last_on != 0;
        s->q1_pos = c->q1_last_pos;
    }
    // checksum of the new bytes, from the copy the encode left on the device
    const uint64_t fresh = s->total - s->emitted;
    if (s->opts.wrapper != 0 && fresh) {
        uint32_t part = 0;
        const uint8_t* d = c->d_in + (s->emitted - s->base);
        rc = s->opts.wrapper == 2 ? mi355_crc32_device(c, d, (size_t)fresh, &part, nullptr)
                                  : mi355_adler32_device(c, d, (size_t)fresh, &part, nullptr);
        if (rc) {
            s->output.resize(at);  // nothing of this call stays behind: a retry emits the segment once
            return rc;
        }
        s->adler = s->opts.wrapper == 2 ? crc_combine(s->adler, part, fresh) : adler_combine(s->adler, part, fresh);
        s->summed += fresh;
    }
    s->emitted = s->total;
    if (finish) return MI355_OK;
    // let go of what no later segment can see
    uint64_t want = (s->emitted >= 3ull * WINDOW_SIZE) ? (s->emitted - WINDOW_SIZE) / WINDOW_SIZE * WINDOW_SIZE : 0;
    // A skew point at want - 1 or at want files position `want` a byte late, under d[want - 1] (stages.h skewed_ab), and `want`
    // is a candidate of the position 32768 behind it.  A buffer that began at `want` would have neither the point (want - 1) nor
    // the byte in front of it (the kernels read 0 in front of the buffer): one more window stays
    // (tests/flush_cases.py trim_skew_at_base_minus_1_F65535_q65536, trim_skew_at_base_own_hash_F65536_q65536).
    // This is the one way to a base of 32768.  Nothing of the stream's first window can show from there: the re-warm points
    // are cleared below, and every position still to be encoded lies at 98304 or behind, out of reach of 32768 and 32769.
    auto skewed = [&](uint64_t f) { return std::find(s->skew.begin(), s->skew.end(), f) != s->skew.end(); };
    if (want && (skewed(want - 1) || skewed(want))) want -= WINDOW_SIZE;
    if (want > s->base) {
        s->win.erase(s->win.begin(), s->win.begin() + (size_t)(want - s->base));
        s->base = want;
        s->flush_points.assign(1, s->emitted);
        s->rewarm.clear();
        auto gone = [&](uint64_t f) { return f < s->base; };
        s->skew.erase(std::remove_if(s->skew.begin(), s->skew.end(), gone), s->skew.end());
        s->holes.erase(std::remove_if(s->holes.begin(), s->holes.end(), gone), s->holes.end());
    }
    return MI355_OK;
}
}  // namespace

extern "C" {

int mi355_deflate_stream_new(mi355_deflate_ctx* c, const mi355_deflate_opts* opts, mi355_deflate_stream** out) {
    if (!opts || !out) return MI355_E_ARG;
    if (opts->wrapper > 2) return MI355_E_ARG;
    DefaultGuard dg_;
    c = use_ctx(c, dg_);
    if (!c) return MI355_E_HIP;
    mi355_deflate_stream* s = new mi355_deflate_stream();
    s->ctx = c;
    s->opts = *opts;
    s->adler = opts->wrapper == 1 ? 1u : 0u;
    *out = s;
    return MI355_OK;
}

int mi355_deflate_stream_write(mi355_deflate_stream* s, const uint8_t* data, size_t n) {
    if (!s || (!data && n)) return MI355_E_ARG;
    if (s->finished || s->failed) return MI355_E_STATE;
    if (n == 0) return MI355_OK;  // write_all semantics: an empty buffer never reaches write()
    stream_header(s);
    const uint64_t f = s->total;
    if (s->after_flush && f > 2) {
        // After a sync flush the reference files the last two positions with the first two bytes of the
        // next write (lz77.rs:605-614): F-2, and F-1 if the write has a second byte.  Whatever had left them
        // out before (a flush after the stream's first one or two bytes, a one-byte write after the flush
        // before this one) is undone for the positions that are re-added now.
        auto erase = [](auto& v, uint64_t x) {
            for (size_t i = 0; i < v.size(); i++)
                if ((uint64_t)v[i] == x) {
                    v.erase(v.begin() + i);
                    return;
                }
        };
        auto insert = [](auto& v, uint64_t x) {  // (the lists stay ascending: the kernels search them)
            size_t i = 0;
            while (i < v.size() && (uint64_t)v[i] < x) i++;
            if (i == v.size() || (uint64_t)v[i] != x) v.insert(v.begin() + i, (typename std::remove_reference<decltype(v)>::type::value_type)x);
        };
        erase(s->holes, f - 2);
        if (n >= 2) erase(s->holes, f - 1);
        // (a one-byte write before an adjacent flush had announced a late rolling hash for F-1: F-1 is re-added
        // now, or left out below, and never fed by the parser)
        if (!s->skew.empty() && s->skew.back() == f - 1) s->skew.pop_back();
        // Inside the first window a flush is a processing call that re-warms the rolling hash with data[0],
        // data[1] (the block has no input so far, lz77.rs:628-638).  When it comes one or two bytes after the
        // flush before it, it feeds no position at all (none of them has its hash byte yet), and the
        // re-warmed state meets this call's re-adds: the re-warm lands at F-2, not at the flush point before.
        uint64_t pprev = 0;
        for (uint64_t q : s->flush_points)
            if (q < f && q > pprev) pprev = q;
        if (pprev > 0 && pprev <= WINDOW_SIZE && f - pprev <= 2) {  // (first-window mode lasts until a call has processed past 32768)
            erase(s->rewarm, pprev);
            insert(s->rewarm, f - 2);
        }
        // A 1-byte write leaves F-1 out for good and the rolling hash one byte behind for F and F+1
        // (stages.h HashOverride).
        if (n == 1) {
            insert(s->holes, f - 1);
            insert(s->skew, f);
        }
        // That same call keeps add_initial = false (lz77.rs:601-612).  Inside the first window, if it
        // does not fill the input buffer (2 * 32768 + 258 bytes, input_buffer.rs:9) nothing is processed
        // yet, and the call that does process re-warms the rolling hash with data[0], data[1] at the
        // flush point, because the block has no input so far (lz77.rs:628-638).
        if (f <= WINDOW_SIZE && f + n < 2 * WINDOW_SIZE + MAX_MATCH) insert(s->rewarm, f);
    } else if (s->after_flush && f > 0) {
        // A flush after one or two bytes: nothing is re-added (lz77.rs:606), the positions before F stay
        // out of the chains, and the next processing call re-warms at F (add_initial is still set).
        s->holes.clear();
        for (uint64_t q = 0; q < f; q++) s->holes.push_back(q);
        s->rewarm.assign(1, (uint32_t)f);
    }
    const bool eligible = stream_long_eligible(s);
    s->after_flush = false;
    if (!eligible && s->total + n - s->base >= 0xFFFF0000ull) {
        // (a stream that has been flushed is bounded by its flushes: what has gathered since the last one is encoded
        // in one call, which takes less than 4 GiB - 64 KiB; say so now rather than at the flush)
        s->ctx->err = "more than 4 GiB - 64 KiB written since the last flush() of a stream that has been flushed before";
        return MI355_E_UNSUPPORTED;
    }
    s->win.insert(s->win.end(), data, data + n);
    s->total += n;
    if (eligible) {
        DefaultGuard dg_;
        (void)use_ctx(s->ctx, dg_);
        const int rc = stream_pump(s);
        if (rc) s->failed = true;
        return rc;
    }
    return MI355_OK;
}

// io::Write::flush of the encoders (writer.rs:134-137, 274-277): Flush::Sync -- everything written so
// far is parsed and emitted in non-final blocks followed by the empty stored block 00 00 FF FF; the
// window is kept, so later data may match across the flush point.  The bytes are in _output /
// _take_output when the call returns.
int mi355_deflate_stream_flush(mi355_deflate_stream* s) {
    if (!s) return MI355_E_ARG;
    if (s->finished || s->failed) return MI355_E_STATE;
    DefaultGuard dg_;
    (void)use_ctx(s->ctx, dg_);
    if (s->L) {  // the stream has handed ranges over: the rest is its last range, ended by the sync marker
        int rc = stream_long_end(s, 2);
        if (rc) {
            s->failed = true;
            return rc;
        }
        // from here on the stream is one that has been flushed (window-bounded history, the hash quirks of write calls)
        const uint64_t f0 = s->total;
        s->flush_points.assign(1, f0);
        s->after_flush = true;
        const uint64_t want = (f0 >= 3ull * WINDOW_SIZE) ? (f0 - WINDOW_SIZE) / WINDOW_SIZE * WINDOW_SIZE : 0;
        if (want > s->base) {
            s->win.erase(s->win.begin(), s->win.begin() + (size_t)(want - s->base));
            s->base = want;
        }
        return MI355_OK;
    }
    const uint64_t f = s->total;
    // (Two flushes one or two bytes apart need no rule of their own: the write after the second one re-adds at
    // F-2 / F-1 -- see mi355_deflate_stream_write -- and a one-byte gap moves the re-warm point with it.)
    const bool was_after_flush = s->after_flush;
    s->flush_points.push_back(f);
    s->after_flush = true;
    int rc = stream_encode(s, false);
    if (rc) {  // as if the call had not happened
        s->flush_points.pop_back();
        s->after_flush = was_after_flush;
    }
    return rc;
}

int mi355_deflate_stream_finish(mi355_deflate_stream* s) {
    if (!s) return MI355_E_ARG;
    if (s->finished || s->failed) return MI355_E_STATE;
    DefaultGuard dg_;
    (void)use_ctx(s->ctx, dg_);
    stream_header(s);  // finish() writes the header if no write() did (writer.rs:201-214, :370-381)
    const bool ranges = s->L != nullptr;
    int rc = ranges ? stream_long_end(s, 1) : stream_encode(s, true);
    if (rc) {
        if (ranges) s->failed = true;
        return rc;
    }
    if (s->opts.wrapper == 1) {  // lib.rs:192-196, writer.rs:235-245: Adler-32 big endian
        const uint8_t t[4] = {(uint8_t)(s->adler >> 24), (uint8_t)(s->adler >> 16), (uint8_t)(s->adler >> 8), (uint8_t)s->adler};
        stream_put(s, t, 4);
    } else if (s->opts.wrapper == 2) {  // lib.rs:258-266: CRC-32 and the length mod 2^32, little endian
        uint8_t t[8];
        for (int k = 0; k < 4; k++) t[k] = (uint8_t)(s->adler >> (8 * k));
        for (int k = 0; k < 4; k++) t[4 + k] = (uint8_t)((uint32_t)s->summed >> (8 * k));
        stream_put(s, t, 8);
    }
    s->finished = true;
    std::vector<uint8_t>().swap(s->win);
    return MI355_OK;
}

// write::gzip::GzEncoder::from_builder (writer.rs:346-358): the header of a wrapper-2 stream, i.e. what
// GzBuilder::into_header() returned (crate gzip-header, not in the tree -- the shim passes the bytes);
// without this call the blank header of GzBuilder::new() is used.
int mi355_deflate_stream_gzip_header(mi355_deflate_stream* s, const uint8_t* hdr, size_t hdr_len) {
    if (!s || !hdr || hdr_len == 0 || hdr_len > 0xFFFF) return MI355_E_ARG;
    if (s->opts.wrapper != 2 || s->finished || s->total || s->header_out) return MI355_E_STATE;
    s->gz_hdr.assign(hdr, hdr + hdr_len);
    return MI355_OK;
}

// reset(&mut self, W) -> io::Result<W> (writer.rs:110-117, 216-223, 383-402; deflate_state.rs:133-152):
// the stream so far is finished and what has not been taken of it is handed out (valid until the next
// reset/free), and the handle starts a new stream with the same options.  A gzip stream goes back to the
// blank header (GzEncoder::reset); call _gzip_header again for reset_with_builder.
int mi355_deflate_stream_reset(mi355_deflate_stream* s, const uint8_t** data, size_t* n) {
    if (!s) return MI355_E_ARG;
    if (s->finished || s->failed) return MI355_E_STATE;
    int rc = mi355_deflate_stream_finish(s);
    if (rc) return rc;
    s->handed_out.assign(s->output.begin() + s->taken, s->output.end());
    if (s->L) long_free(s->L);
    s->L = nullptr;
    s->output.clear();
    s->taken = 0;
    s->win.clear();
    s->base = s->total = s->emitted = s->summed = 0;
    s->flush_points.clear();
    s->rewarm.clear();
    s->skew.clear();
    s->holes.clear();
    s->gz_hdr.clear();
    s->after_flush = false;
    s->header_out = false;
    s->finished = false;
    s->q1_on = false;
    s->q1_pos = 0;
    s->adler = s->opts.wrapper == 1 ? 1u : 0u;
    if (data) *data = s->handed_out.data();
    if (n) *n = s->handed_out.size();
    return MI355_OK;
}

// the bytes produced so far that have not been taken (what the inner writer W would have been given)
int mi355_deflate_stream_output(mi355_deflate_stream* s, const uint8_t** data, size_t* n) {
    if (!s || !data || !n) return MI355_E_ARG;
    *data = s->output.data() + s->taken;
    *n = s->output.size() - s->taken;
    return MI355_OK;
}

// Take up to `cap` of those bytes (W::write accepting fewer bytes than offered, compress.rs:96-124,
// 280-299: the shim calls this in a loop for a short-write sink); *n = bytes copied, 0 when none are left.
int mi355_deflate_stream_take_output(mi355_deflate_stream* s, uint8_t* dst, size_t cap, size_t* n) {
    if (!s || !n || (!dst && cap)) return MI355_E_ARG;
    size_t k = s->output.size() - s->taken;
    if (k > cap) k = cap;
    if (k) memcpy(dst, s->output.data() + s->taken, k);
    s->taken += k;
    if (s->taken == s->output.size()) {
        s->output.clear();
        s->taken = 0;
    }
    *n = k;
    return MI355_OK;
}

int mi355_deflate_stream_checksum(mi355_deflate_stream* s, uint32_t* adler) {
    if (!s || !adler) return MI355_E_ARG;
    *adler = s->adler;
    if (s->finished || s->opts.wrapper == 0) return MI355_OK;
    // {Zlib,Gz}Encoder::checksum() mid-stream (writer.rs:248-250, :428-430): of what was written so far --
    // the encoded part is summed already, only the bytes since the last flush are new
    const uint64_t fresh = s->total - s->summed;  // (summed == the last flush point, or the ranges handed over so far)
    if (!fresh) return MI355_OK;
    DefaultGuard dg_;
    mi355_deflate_ctx* c = use_ctx(s->ctx, dg_);
    const bool gz = s->opts.wrapper == 2;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure_buf(c, &c->d_in, &c->d_in_cap, (size_t)fresh + 64);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_in, s->win.data() + (s->summed - s->base), (size_t)fresh, hipMemcpyHostToDevice, c->own_stream));
    uint32_t part = 0;
    rc = gz ? mi355_crc32_device(c, c->d_in, (size_t)fresh, &part, nullptr) : mi355_adler32_device(c, c->d_in, (size_t)fresh, &part, nullptr);
    if (rc) return rc;
    *adler = gz ? crc_combine(s->adler, part, fresh) : adler_combine(s->adler, part, fresh);
    return MI355_OK;
}

void mi355_deflate_stream_free(mi355_deflate_stream* s) {
    if (!s) return;
    if (s->L) long_free(s->L);
    delete s;
}

}  // extern "C"

