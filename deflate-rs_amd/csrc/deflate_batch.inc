// Batched encode (include/mi355_deflate.h mi355_deflate_encode_batch[_device]): many independent inputs, one launch per stage.
// The stages are those of a small one-shot call of run_encode (small_inits && small_tail, the speculative parse): k_sort, the walk
// (k_match3_both), k_adv for the levels that need it, k_emit<1>, k_small_fix, k_compact, k_block_hist, k_block_header, k_plan, k_pack
// and the zlib frame.  Every batched kernel below runs the body of its single-call kernel; the arguments come from the item's
// descriptor (BatchItem) instead of the launch.  A launch's grid is the items' workgroups back to back, and a workgroup finds its item
// by a search over the stage's running sums (stages.h batch_item_of).  The stages that are one workgroup per call (k_small_fix,
// k_plan, the zlib tail, the gzip tail) are one workgroup per item.  A gzip batch (mi355_deflate_encode_batch[_device]_gzip) adds
// kb_crc, the CRC-32 of every item in one flat grid, and kb_gzip_tail, which writes the item's header and trailer with byte stores
// after the pack (a header has any length, so an item's stream starts on any byte of a word).  At the levels without a hash (RLE,
// Huffman only) kb_nohash stands where kb_sort and kb_walk stand: k_rle over the items' tiles, or the items' M slices cleared.
// A packed batch (mi355_deflate_encode_batch_packed[_device]) adds kb_place between kb_plan and kb_pack: the items' exact lengths
// are known there, and a scan over them gives every item its place in the caller's one arena (BatchItem::out, written on the device).
// DESIGN.md section 10.
namespace mi355 {

struct BatchItem {
    const uint8_t* in;
    uint32_t n, K0, nb_max;
    uint32_t q1_check;   // the item's first pass may fire Q1: k_small_fix stops its block stages (run_encode `speculate`)
    uint32_t out_words;  // mi355_deflate_bound_ex(n, wrapper, 0, 0) / 4: cleared by kb_block_hist (k_pack ORs its bits in)
    uint32_t bit_base;   // bits of the frame in front of the item's stream: 0 (raw), 16 (zlib), 8 * the header's bytes (gzip)
    uint32_t gz_off, gz_len;  // gzip: the item's header in the set's header bytes (kb_gzip_tail)
    uint32_t *M, *Mq;
    uint16_t *adv, *S, *B;  // S: the sorted positions behind their pad epoch
    uint32_t *E0, *tokbuf, *cnt, *xs, *badmap, *fixlist, *base, *tend, *pb, *bstart, *q13, *dtok, *ll_freq, *d_freq, *seg_ends;
    BlockTab tab;
    BlockHeader* hdr;
    BlockPlan* plan;
    DevState* st;  // the item's scalars and flags
    uint8_t* out;  // a packed set: written by kb_place; nullptr = not placed (kb_pack, kb_zlib_tail_placed and kb_gzip_tail return at once)
};
// the stages with a grid of their own per item (a row of running sums each)
enum : uint32_t { BS_SORT, BS_WALK, BS_RLE, BS_ADV, BS_EMIT, BS_COMPACT, BS_HIST, BS_HEADER, BS_PACK, BS_ADLER, BS_CRC, BS_N };
struct BatchArgs {
    const BatchItem* it;
    const uint32_t* pre;  // BS_N rows of n_items + 1 running sums of workgroups
    uint32_t n_items;
};
// the item of this workgroup, its index inside the item and the item's workgroup count in this stage
__device__ __forceinline__ uint32_t batch_locate(const BatchArgs& a, uint32_t stage, uint32_t& local, uint32_t& count) {
    const uint32_t* pre = a.pre + (size_t)stage * (a.n_items + 1);
    const uint32_t i = __builtin_amdgcn_readfirstlane(batch_item_of(pre, a.n_items, blockIdx.x));
    local = blockIdx.x - pre[i];
    count = pre[i + 1] - pre[i];
    return i;
}
__device__ __forceinline__ HashOverride batch_no_override() { return HashOverride{0, 0, 0, 0, 0, nullptr, 0, nullptr, 0, nullptr}; }

template <int MODE>
__global__ __launch_bounds__(1024) void kb_sort(BatchArgs bat_, uint32_t dbl) {
    uint32_t local, count;
    const BatchItem& it = bat_.it[batch_locate(bat_, BS_SORT, local, count)];
    // (workgroup 0 of an item clears its scalars and sets its one segment end, as a small call's k_sort does)
    k_sort_body<MODE>(local, it.in, it.n, batch_no_override(), it.S, it.B, 0u, dbl,
                      SortInit{reinterpret_cast<uint32_t*>(it.st), (uint32_t)(sizeof(DevScalars) / 4), it.seg_ends, it.n});
}

// the walk of k_match3_both (both tables in one launch) at every batch size
template <bool HAS_Q, bool SINGLE>
__global__ __launch_bounds__(M3T) __attribute__((amdgpu_waves_per_eu(4, 4))) void kb_walk(BatchArgs bat_, uint32_t checks, uint32_t checks_q,
                                                                                       uint32_t split) {
    __shared__ __attribute__((aligned(256))) uint4 s_T[M3_TABLE_U4];
    __shared__ uint32_t s_next;
    uint32_t local, count;
    const BatchItem& it = bat_.it[batch_locate(bat_, BS_WALK, local, count)];
    const uint32_t e = local / split, part = local % split;
    const SegEnds sg{it.seg_ends, 1u};
    const int aligned16 = (reinterpret_cast<uintptr_t>(it.in) & 15) == 0 ? 1 : 0;
    uint32_t* const ms = split == 1 ? walk_borrows(it.tokbuf, it.K0) : nullptr;  // (as launch_walk)
    uint32_t* const mqs = (HAS_Q && split == 1) ? it.dtok : nullptr;
    uint32_t* const Mq = HAS_Q ? it.Mq : nullptr;
    if (MI355_SWZ_BANKS && __builtin_amdgcn_readfirstlane((int)it.B[(size_t)e * BSTRIDE + WINDOW_SIZE + 2]))
        m3_epoch<HAS_Q, true, SINGLE>(s_T, s_next, e, part, it.in, it.n, it.S, it.B, it.M, Mq, checks, checks_q, aligned16, sg,
                                      batch_no_override(), split, ms, mqs, &it.st->sort_bad);
    else
        m3_epoch<HAS_Q, false, SINGLE>(s_T, s_next, e, part, it.in, it.n, it.S, it.B, it.M, Mq, checks, checks_q, aligned16, sg,
                                       batch_no_override(), split, ms, mqs, &it.st->sort_bad);
}

// The match stage of a set at a level without a hash, one workgroup per tile of RT positions (the grid run_encode gives k_rle).
// RLE: k_rle of the item -- its run table into M, its restart steps into adv; a run ends with the item (k_rle bounds every read and
// every run by n), wherever the item lies and whatever follows it.  Huffman only: the item's M slice cleared (n + 64 entries, the
// fill of run_encode), as whole 16-byte lines: M is 256-byte aligned and its slice is padded to the next 256 bytes (carve).
// Workgroup 0 of an item does what kb_sort does on the side: the item's scalars cleared, its one segment end set.  Nothing in this
// kernel reads either (one segment end: k_rle does not look at it).
template <bool RLE>
__global__ __launch_bounds__(256) void kb_nohash(BatchArgs bat_) {
    uint32_t local, count;
    const BatchItem& it = bat_.it[batch_locate(bat_, BS_RLE, local, count)];
    if (local == 0) {
        uint32_t* const sc = reinterpret_cast<uint32_t*>(it.st);
        for (uint32_t i = threadIdx.x; i < (uint32_t)(sizeof(DevScalars) / 4); i += 256) sc[i] = 0;
        if (threadIdx.x == 0) *it.seg_ends = it.n;
    }
    if (RLE) {
        k_rle_body(local, it.in, it.n, it.M, it.adv, SegEnds{it.seg_ends, 1u});
    } else {
        const uint32_t lo = local * RT, hi = local + 1 == count ? ((it.n + 64 + 3) & ~3u) : lo + RT;
        for (uint32_t i = lo + threadIdx.x * 4; i < hi; i += 256 * 4) *reinterpret_cast<uint4*>(it.M + i) = make_uint4(0, 0, 0, 0);
    }
}

__global__ __launch_bounds__(256) void kb_adv(BatchArgs bat_, ParseCfg cfg) {
    uint32_t local, count;
    const BatchItem& it = bat_.it[batch_locate(bat_, BS_ADV, local, count)];
    k_adv_body(local, it.n, it.M, cfg.use_quarter ? it.Mq : nullptr, cfg, it.adv, SegEnds{it.seg_ends, 1u}, 0u);
}

// k_emit<1, STEPS>: the names the body reads, from the descriptor
template <bool STEPS>
__global__ __launch_bounds__(256) void kb_emit(BatchArgs bat_, ParseCfg cfg) {
    constexpr int MODE = 1;
    uint32_t local, count;
    const BatchItem& it = bat_.it[batch_locate(bat_, BS_EMIT, local, count)];
    const uint8_t* in = it.in;
    uint32_t n = it.n, K = it.K0;
    const uint32_t* M = it.M;
    const uint32_t* Mq = cfg.use_quarter ? it.Mq : nullptr;
    const uint16_t* adv = STEPS ? nullptr : it.adv;
    uint32_t *E0 = it.E0, *tokbuf = it.tokbuf, *cnt = it.cnt, *Xs = it.xs;
    uint32_t pos0 = 0, n_total = it.n, runup0 = 0, seg0 = 0;
    SegEnds sg{it.seg_ends, 1u};
    SpecFix fix{it.fixlist, it.badmap, &it.st->sc.n_fix[0]};
#define BX_ local
#include "body_k_emit.inc"
#undef BX_
}

template <bool STEPS>
__global__ __launch_bounds__(SMALL_FIX_T) void kb_small_fix(BatchArgs bat_, ParseCfg cfg) {
    const BatchItem& it = bat_.it[blockIdx.x];
    k_small_fix_body<STEPS>(0u, it.in, it.n, it.K0, it.M, cfg.use_quarter ? it.Mq : nullptr, cfg, STEPS ? nullptr : it.adv, it.E0,
                            it.tokbuf, it.cnt, SegEnds{it.seg_ends, 1u}, it.xs, it.badmap, it.fixlist, it.nb_max, 0u, &it.st->spec_bad,
                            it.base, &it.st->sc, it.tend, it.pb, it.bstart, it.q13, it.tab, it.q1_check);
}

__global__ __launch_bounds__(256) void kb_compact(BatchArgs bat_) {
    uint32_t local, count;
    const BatchItem& it = bat_.it[batch_locate(bat_, BS_COMPACT, local, count)];
    k_compact_body(local, it.K0, it.tokbuf, it.cnt, it.base, it.dtok, &it.st->sc, 0u);
}

template <uint32_t HT>
__global__ __launch_bounds__(HT) void kb_block_hist(BatchArgs bat_) {
    uint32_t local, count;
    const BatchItem& it = bat_.it[batch_locate(bat_, BS_HIST, local, count)];
    k_block_hist_body<HT>(local, count, it.dtok, &it.st->sc, it.ll_freq, it.d_freq, it.tab, 0u, reinterpret_cast<uint32_t*>(it.out),
                          it.out_words);
}

__global__ __launch_bounds__(128) void kb_block_header(BatchArgs bat_) {
    uint32_t local, count;
    const BatchItem& it = bat_.it[batch_locate(bat_, BS_HEADER, local, count)];
    k_block_header_body(local, &it.st->sc, it.ll_freq, it.d_freq, it.hdr, 0u);
}

__global__ __launch_bounds__(1024) void kb_plan(BatchArgs bat_, uint32_t compat) {
    __shared__ uint32_t s_red[16], s_flag[3];
    const BatchItem& it = bat_.it[blockIdx.x];
    plan_blocks(s_red, s_flag, &it.st->sc, it.hdr, it.bstart, it.q13, it.plan, (uint64_t)it.bit_base, compat, it.tab.sync,
                reinterpret_cast<uint32_t*>(it.out), Piece{0u, 0u, 1u});
}

template <uint32_t PKT>
__global__ __launch_bounds__(PKT) void kb_pack(BatchArgs bat_, uint32_t compat) {
    uint32_t local, count;
    const BatchItem& it = bat_.it[batch_locate(bat_, BS_PACK, local, count)];
    if (!it.out) return;  // (a packed set: the item takes no bytes -- kb_place)
    const uint8_t* in = it.in;
    uint32_t n = it.n, piece = 0;
    const uint32_t* dtok = it.dtok;
    const DevScalars* sc = &it.st->sc;
    const BlockHeader* hdr = it.hdr;
    const BlockPlan* plan = it.plan;
    const uint32_t *bstart = it.bstart, *q13 = it.q13, *ll_freq = it.ll_freq, *d_freq = it.d_freq;
    uint32_t* out32 = reinterpret_cast<uint32_t*>(it.out);
    BlockTab tab = it.tab;
#define BX_ local
#include "body_k_pack.inc"
#undef BX_
}

__global__ __launch_bounds__(256) void kb_adler_part(BatchArgs bat_) {
    uint32_t local, count;
    const BatchItem& it = bat_.it[batch_locate(bat_, BS_ADLER, local, count)];
    const uint8_t* in = it.in;
    uint32_t n = it.n;
    DevScalars* sc = &it.st->sc;
#define BX_ local
#include "body_k_adler_part.inc"
#undef BX_
}

// k_adler_fold and k_zlib_frame of an item, one after the other in one lane
__global__ __launch_bounds__(64) void kb_zlib_tail(BatchArgs bat_) {
    const BatchItem& it = bat_.it[blockIdx.x];
    k_adler_fold_body(0u, it.n, &it.st->sc);
    k_zlib_frame_body(0u, &it.st->sc, it.out, 1u);
}
// ... of a packed set: nothing for an item that kb_place did not place.  (A kernel of its own: with the test inside it,
// kb_zlib_tail came out with one scalar register less, and the kernels of the plain batch stay as they are.)
__global__ __launch_bounds__(64) void kb_zlib_tail_placed(BatchArgs bat_) {
    const BatchItem& it = bat_.it[blockIdx.x];
    if (!it.out) return;
    k_adler_fold_body(0u, it.n, &it.st->sc);
    k_zlib_frame_body(0u, &it.st->sc, it.out, 1u);
}

// k_crc_part and k_crc_fold of an item in one kernel: a thread runs the table CRC over its CRC_CHUNK bytes (the body of k_crc_part),
// multiplies it by x^(8 * bytes of the item behind the chunk) and the products are XOR-ed: over the wave by shuffles, over the
// workgroup through LDS, then one atomicXor into the item's scalar (cleared by the item's kb_sort / kb_nohash).  No per-chunk words in memory.
__global__ __launch_bounds__(256) void kb_crc(BatchArgs bat_) {
    __shared__ uint32_t s_wave[4];
    uint32_t local, count;
    const BatchItem& it = bat_.it[batch_locate(bat_, BS_CRC, local, count)];
    const uint8_t* in = it.in;
    const uint32_t n = it.n;
#define BX_ local
#include "body_k_crc_part.inc"
#undef BX_
    uint32_t v = 0;
    if (mylen) {
        const uint64_t after = n - (my0 + mylen);
        v = ~crc;
        if (after) v = crc_mulmod(crc_xpow8(after), v);
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) v ^= __shfl_xor(v, off, 64);
    if ((tid & 63) == 0) s_wave[tid >> 6] = v;
    __syncthreads();
    if (tid) return;
    v = s_wave[0] ^ s_wave[1] ^ s_wave[2] ^ s_wave[3];
    if (v) atomicXor(&it.st->sc.crc, v);
}

// k_gzip_frame of an item: its header from the set's header bytes, CRC-32 and length behind the stream
__global__ __launch_bounds__(64) void kb_gzip_tail(BatchArgs bat_, const uint8_t* __restrict__ gz) {
    const BatchItem& it = bat_.it[blockIdx.x];
    if (!it.out) return;
    DevScalars* sc = &it.st->sc;
    uint8_t* out = it.out;
    const uint8_t* hdr = gz + it.gz_off;
    const uint32_t hdr_len = it.gz_len, in_len = it.n, trailer = 1u;
#define BX_ 0u
#include "body_k_gzip_frame.inc"
#undef BX_
}

// The placement of a packed set, one workgroup of PLACE_T threads behind kb_plan: an item's stream takes len = stream_bytes(its
// total_bits) bytes -- none where its speculative parse failed or Q1 fired (the one-input path encodes it after the sets) or where
// the reference panics -- and owns align_up(len, align) bytes of the arena.  A 64-bit exclusive scan of those, PLACE_T items a
// round (shuffles inside a wave, the waves' sums through LDS, the running end carried from round to round), started at the end the
// launch sets before this one left, gives every item its offset as if the arena had no end.  An item whose region ends at or
// below `cap` gets its pointer; one that would cross it -- and one without bytes -- gets nullptr and is left alone by kb_pack and
// the tails.  The item's table entry goes to the caller's table (if there is one), the set's end to *tail_out, behind the items'
// DevStates, where the set's one copy back picks it up.
constexpr uint32_t PLACE_T = 1024;
struct PlaceArgs {
    uint8_t* base;        // the address of arena offset tail0
    uint64_t tail0, cap;  // where the set starts; the arena's capacity
    uint32_t align, wrapper;
    const uint32_t* idx;        // the items' places in the caller's array (the table's order)
    mi355_packed_entry* table;  // or nullptr
    uint64_t* tail_out;
};
__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t v, int off) {
    const uint32_t lo = __shfl_up((uint32_t)v, off, 64), hi = __shfl_up((uint32_t)(v >> 32), off, 64);
    return ((uint64_t)hi << 32) | lo;
}
__global__ __launch_bounds__(PLACE_T) void kb_place(BatchArgs bat_, PlaceArgs p) {
    __shared__ uint64_t s_wave[PLACE_T / 64];
    BatchItem* const items = const_cast<BatchItem*>(bat_.it);  // (the descriptors are the context's device memory)
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint64_t amask = (uint64_t)p.align - 1;
    uint64_t end = p.tail0;
    for (uint32_t i0 = 0; i0 < bat_.n_items; i0 += PLACE_T) {
        const uint32_t i = i0 + tid;
        uint64_t len = 0;
        int32_t status = MI355_OK;
        if (i < bat_.n_items) {
            const DevScalars* sc = &items[i].st->sc;
            if (spec_failed(sc))
                len = 0;
            else if (sc->ref_panic)
                status = MI355_E_REF_PANIC;
            else
                len = stream_bytes(sc->total_bits, p.wrapper, items[i].gz_len, false);
        }
        const uint64_t need = (len + amask) & ~amask;
        uint64_t incl = need;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint64_t y = shfl_up_u64(incl, off);
            if (lane >= (uint32_t)off) incl += y;
        }
        if (lane == 63) s_wave[wv] = incl;
        __syncthreads();
        uint64_t wbase = 0, total = 0;
#pragma unroll
        for (uint32_t k = 0; k < PLACE_T / 64; k++) {
            const uint64_t y = s_wave[k];
            if (k < wv) wbase += y;
            total += y;
        }
        const uint64_t off = end + wbase + (incl - need);
        if (i < bat_.n_items) {
            const bool fits = off + need <= p.cap;
            if (len && !fits) status = MI355_E_OUT_TOO_SMALL;
            items[i].out = (len && fits) ? p.base + (off - p.tail0) : nullptr;
            if (p.table) p.table[p.idx[i]] = mi355_packed_entry{off, len, status, 0u};
        }
        end += total;
        __syncthreads();  // (the next round's sums behind this round's reads of them)
    }
    if (tid == 0) *p.tail_out = end;
}

// The clear of a packed set's range (kb_pack ORs its bits in), behind kb_place and sized from its scan: the words from the set's
// start to its end, or to the arena's if that comes first (regions are whole words, so every region that fits ends at or before
// the last whole word below cap).  The pad bytes of the regions are zero because of it.  (One runtime fill in front of the set
// over all the set could reach -- the sum of the items' bounds -- measured the same or worse: DESIGN.md section 10.)
__global__ __launch_bounds__(256) void kb_clear(uint32_t* __restrict__ base, uint64_t tail0, uint64_t cap, const uint64_t* __restrict__ end) {
    const uint64_t stop = *end < cap ? *end : cap;
    const uint64_t words = stop > tail0 ? (stop - tail0) / 4 : 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (uint64_t)gridDim.x * 256) base[i] = 0;
}

}  // namespace mi355

namespace {

constexpr uint32_t BATCH_ITEMS_MAX = 65536;  // items of one launch set (the descriptors and running sums: 38 MiB at most)

// one item of a batch as the launch sets see it: device buffers
struct BatchView {
    const uint8_t* d_in;
    uint64_t n;
    uint8_t* d_out;
    size_t need;
    size_t idx;  // in the caller's array
};

// The gzip headers of a batch (wrapper 2; n as n_hdrs of mi355_deflate_encode_batch_gzip): none for raw and zlib.
struct BatchHeaders {
    const mi355_gzip_header* h = nullptr;
    size_t n = 0;
    bool gzip = false;
    mi355_gzip_header of(size_t i) const {  // the header of item i of the caller's array
        if (!gzip) return mi355_gzip_header{nullptr, 0};
        if (n == 0) return mi355_gzip_header{kBlankGzipHeader, sizeof kBlankGzipHeader};
        return h[n == 1 ? 0 : i];
    }
};

// Can the batched kernels take this item?  (Else: the one-input path, after the launch sets.)
// (Every level but Lazy with a quarter budget of 0 checks; the levels without a hash -- RLE, Huffman only -- have kb_nohash.)
bool batch_takes(const ParseCfg& cfg, uint64_t n) {
    const bool level = !cfg_hashing(cfg) || !(cfg.use_quarter && cfg_cq(cfg) == 0);
    return MI355_SMALL_TAIL && level && n > 0 && (n + SEG - 1) / SEG <= SMALL_TAIL_SEGS;
}

enum BatchOutcome { BO_OK, BO_Q1, BO_SPEC, BO_PANIC };

// The arena of a packed batch (mi355_deflate_encode_batch_packed[_device]) as the launch sets see it.
struct PackedOut {
    uint8_t* d_arena;  // the caller's device arena (_device), or nullptr: every set goes through the context's staging (host)
    uint8_t* h_arena;  // the caller's host arena, or nullptr
    uint64_t cap;
    uint32_t align;
    mi355_packed_entry* d_table;  // or nullptr
    uint64_t tail;                // the end of the regions so far, as if the arena had no end
    // of the set under way: the device address of offset `tail`, and the items' offsets (written by batch_launch_set)
    uint8_t* set_base;
    std::vector<uint64_t> off;
    uint64_t up(uint64_t len) const { return (len + align - 1) & ~(uint64_t)(align - 1); }
};

// One launch set over v[0..k): the kernels, one copy of the items' scalars back, one wait.  out_len / outcome per item.
int batch_launch_set(mi355_deflate_ctx* c, const BatchView* v, uint32_t k, const mi355_deflate_opts* o, const ParseCfg& cfg,
                     hipStream_t st, const BatchHeaders& gz, size_t* out_len, BatchOutcome* outcome, DevScalars* sums,
                     PackedOut* pk = nullptr) {
    const bool zlib = o->wrapper == 1, gzip = o->wrapper == 2;
    const bool hashing = cfg_hashing(cfg);  // (else: no sort, no walk, no Q1 -- kb_nohash is the match stage)
    const uint32_t cq = cfg_cq(cfg);
    const bool has_q = cfg_has_q(cfg);
    // the items' workspaces, one behind the other in the context's one workspace
    std::vector<uint64_t> ws_off(k + 1, 0);
    for (uint32_t i = 0; i < k; i++) ws_off[i + 1] = ws_off[i] + carve(nullptr, v[i].n, cfg.use_quarter).bytes;
    int rc = ensure_ws(c, ws_off[k]);
    if (rc) return rc;
    const size_t pre_words = (size_t)BS_N * (k + 1);
    // the set's header bytes behind the running sums, in the same copy: a header shared by neighbours (the blank one, one for all) once
    const size_t gz_at = sizeof(BatchItem) * k + sizeof(uint32_t) * pre_words;
    std::vector<uint32_t> gz_off(gzip ? k : 0, 0);
    size_t gz_bytes = 0;
    for (uint32_t i = 0; i < k && gzip; i++) {
        const mi355_gzip_header h = gz.of(v[i].idx), prev = i ? gz.of(v[i - 1].idx) : mi355_gzip_header{nullptr, 0};
        if (i && h.hdr == prev.hdr && h.hdr_len == prev.hdr_len) {
            gz_off[i] = gz_off[i - 1];
        } else {
            gz_off[i] = (uint32_t)gz_bytes;
            gz_bytes += h.hdr_len;
        }
    }
    // a packed set: the items' places in the caller's array behind the header bytes (kb_place writes the table in that order), and
    // one more DevState's room behind the items' for the set's end
    const size_t idx_at = align_up(gz_at + gz_bytes, 4);
    const size_t up_bytes = pk ? idx_at + sizeof(uint32_t) * k : gz_at + gz_bytes;
    const size_t desc_bytes = align_up(up_bytes, 256);
    const size_t state_bytes = sizeof(DevState) * (pk ? k + 1 : k);
    rc = ensure_buf(c, &c->b_dev, &c->b_dev_cap, desc_bytes + state_bytes);
    if (rc) return rc;
    if (desc_bytes + state_bytes > c->b_host_cap) {
        if (c->b_host) (void)hipHostFree(c->b_host);
        c->b_host = nullptr;
        c->b_host_cap = 0;
        HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&c->b_host), desc_bytes + state_bytes, 0));
        c->b_host_cap = desc_bytes + state_bytes;
    }
    BatchItem* hit = reinterpret_cast<BatchItem*>(c->b_host);
    uint32_t* hpre = reinterpret_cast<uint32_t*>(c->b_host + sizeof(BatchItem) * k);
    uint8_t* hgz = c->b_host + gz_at;
    DevState* hst = reinterpret_cast<DevState*>(c->b_host + desc_bytes);
    DevState* dst = reinterpret_cast<DevState*>(c->b_dev + desc_bytes);
    // the walk's parts per epoch: as launch_walk cuts the epochs of one call, for all epochs of the set
    uint64_t epochs = 0;
    for (uint32_t i = 0; i < k; i++) epochs += (v[i].n + WINDOW_SIZE - 1) / WINDOW_SIZE;
    const uint32_t cus = c->n_cu ? c->n_cu : 256u;
    const WalkPlan plan = hashing ? walk_plan(epochs, c->n_cu) : WalkPlan{};
    const bool single = plan.single;
    const uint32_t split = single ? plan.split * 2 : plan.split;
    for (uint32_t s = 0; s < BS_N; s++) hpre[(size_t)s * (k + 1)] = 0;
    for (uint32_t i = 0; i < k; i++) {
        const Workspace w = carve(c->ws + ws_off[i], v[i].n, cfg.use_quarter);
        BatchItem& d = hit[i];
        memset(&d, 0, sizeof d);
        d.in = v[i].d_in;
        d.n = (uint32_t)v[i].n;
        d.K0 = w.K0;
        d.nb_max = w.nb_max;
        d.q1_check = (hashing && v[i].n >= MAX_BUFFER_LENGTH) ? 1u : 0u;
        d.out_words = pk ? 0u : (uint32_t)(v[i].need / 4);  // (a packed set's range is cleared as a whole: kb_clear)
        if (pk) reinterpret_cast<uint32_t*>(c->b_host + idx_at)[i] = (uint32_t)v[i].idx;
        d.bit_base = zlib ? 16u : 0u;
        if (gzip) {
            const mi355_gzip_header h = gz.of(v[i].idx);
            d.bit_base = 8u * (uint32_t)h.hdr_len;
            d.gz_off = gz_off[i];
            d.gz_len = (uint32_t)h.hdr_len;
            if (i == 0 || gz_off[i] != gz_off[i - 1]) memcpy(hgz + gz_off[i], h.hdr, h.hdr_len);
        }
        d.M = w.M;
        d.Mq = w.Mq;
        d.adv = w.adv;
        d.S = w.sorted + WINDOW_SIZE;
        d.B = w.buckets;
        d.E0 = w.levels[0].E;
        d.tokbuf = w.tokbuf;
        d.cnt = w.cnt;
        d.xs = w.xs;
        d.badmap = w.badmap;
        d.fixlist = w.fixlist;
        d.base = w.base;
        d.tend = w.tend;
        d.pb = w.pb;
        d.bstart = w.bstart;
        d.q13 = w.q13;
        d.dtok = w.dtok;
        d.ll_freq = w.ll_freq;
        d.d_freq = w.d_freq;
        d.seg_ends = w.seg_ends;
        d.tab = w.tab;
        d.hdr = w.hdr;
        d.plan = w.plan;
        d.st = dst + i;
        d.out = v[i].d_out;
        const uint64_t n_ep = (v[i].n + WINDOW_SIZE - 1) / WINDOW_SIZE;
        const uint64_t wg[BS_N] = {hashing ? n_ep : 0u, hashing ? n_ep * split : 0u, hashing ? 0u : cdiv(v[i].n, RT), cdiv(v[i].n, ADV_TILE),
                                   cdiv(w.K0, 4), cdiv(w.K0, 4), (uint64_t)w.nb_max * PSPLIT, w.nb_max, (uint64_t)w.nb_max * PSPLIT,
                                   cdiv(v[i].n, ADLER_CHUNK), gzip ? cdiv(v[i].n, 256 * CRC_CHUNK) : 0u};
        for (uint32_t s = 0; s < BS_N; s++) {
            const uint64_t t = (uint64_t)hpre[(size_t)s * (k + 1) + i] + wg[s];
            if (t > 0x7fffffffull) return MI355_E_ARG;  // (a launch set of at most 256 MiB of input is far below this)
            hpre[(size_t)s * (k + 1) + i + 1] = (uint32_t)t;
        }
    }
    auto total = [&](uint32_t s) { return hpre[(size_t)s * (k + 1) + k]; };
    const BatchArgs a{reinterpret_cast<const BatchItem*>(c->b_dev), reinterpret_cast<const uint32_t*>(c->b_dev + sizeof(BatchItem) * k), k};
    HIPCHK(c, hipMemcpyAsync(c->b_dev, c->b_host, up_bytes, hipMemcpyHostToDevice, st));
    uint64_t pk_reach = 0;
    HIPCHK(c, hipMemsetAsync(dst, 0, state_bytes, st));  // (the flags behind the scalars: kb_sort / kb_nohash clear the scalars themselves)
    if (pk) {  // as far as the set can reach and the arena goes: the grid of kb_clear
        uint64_t reach = 0;
        for (uint32_t i = 0; i < k; i++) reach += pk->up(v[i].need);
        pk_reach = std::min(reach, pk->cap > pk->tail ? pk->cap - pk->tail : 0);
    }
    // ---- match table (the levels without a hash: kb_nohash, and neither sort nor walk) ----
#define MI355_BWALK(Q, SNG) hipLaunchKernelGGL((kb_walk<Q, SNG>), dim3(total(BS_WALK)), dim3(M3T), 0, st, a, cfg.checks, Q ? cq : 0u, split)
    if (!hashing) {
        if (cfg.mode == MODE_RLE)
            hipLaunchKernelGGL(kb_nohash<true>, dim3(total(BS_RLE)), dim3(256), 0, st, a);
        else
            hipLaunchKernelGGL(kb_nohash<false>, dim3(total(BS_RLE)), dim3(256), 0, st, a);
    } else {
        if (c->sort_mode == 1)
            hipLaunchKernelGGL(kb_sort<1>, dim3(total(BS_SORT)), dim3(1024), 0, st, a, sort_dbl(c, 1));
        else
            hipLaunchKernelGGL(kb_sort<0>, dim3(total(BS_SORT)), dim3(1024), 0, st, a, sort_dbl(c, 0));
        if (has_q && single)
            MI355_BWALK(true, true);
        else if (has_q)
            MI355_BWALK(true, false);
        else if (single)
            MI355_BWALK(false, true);
        else
            MI355_BWALK(false, false);
    }
#undef MI355_BWALK
    // ---- parse: speculative segment entries, the check and repair, the block table (k_small_fix), compaction ----
    // (RLE: k_rle has written the steps of that level, as in run_encode)
    const bool in_emit = steps_in_emit(c, cfg, 1);
    if (!in_emit && cfg.mode != MODE_RLE) hipLaunchKernelGGL(kb_adv, dim3(total(BS_ADV)), dim3(256), 0, st, a, cfg);
    if (in_emit) {
        hipLaunchKernelGGL(kb_emit<true>, dim3(total(BS_EMIT)), dim3(256), 0, st, a, cfg);
        hipLaunchKernelGGL(kb_small_fix<true>, dim3(k), dim3(SMALL_FIX_T), 0, st, a, cfg);
    } else {
        hipLaunchKernelGGL(kb_emit<false>, dim3(total(BS_EMIT)), dim3(256), 0, st, a, cfg);
        hipLaunchKernelGGL(kb_small_fix<false>, dim3(k), dim3(SMALL_FIX_T), 0, st, a, cfg);
    }
    hipLaunchKernelGGL(kb_compact, dim3(total(BS_COMPACT)), dim3(256), 0, st, a);
    // ---- blocks ----
    if (total(BS_HIST) <= cus)
        hipLaunchKernelGGL(kb_block_hist<1024>, dim3(total(BS_HIST)), dim3(1024), 0, st, a);
    else
        hipLaunchKernelGGL(kb_block_hist<256>, dim3(total(BS_HIST)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(kb_block_header, dim3(total(BS_HEADER)), dim3(128), 0, st, a);
    hipLaunchKernelGGL(kb_plan, dim3(k), dim3(1024), 0, st, a, (uint32_t)o->compat);
    if (pk)
        hipLaunchKernelGGL(kb_place, dim3(1), dim3(PLACE_T), 0, st, a,
                           PlaceArgs{pk->set_base, pk->tail, pk->cap, pk->align, (uint32_t)o->wrapper,
                                     reinterpret_cast<const uint32_t*>(c->b_dev + idx_at), pk->d_table, reinterpret_cast<uint64_t*>(dst + k)});
    if (pk && pk_reach)
        hipLaunchKernelGGL(kb_clear, dim3((uint32_t)std::min<uint64_t>(cdiv(pk_reach, 256 * 4 * 8), 2048)), dim3(256), 0, st,
                           reinterpret_cast<uint32_t*>(pk->set_base), pk->tail, pk->cap, reinterpret_cast<const uint64_t*>(dst + k));
    if (total(BS_PACK) <= cus)
        hipLaunchKernelGGL(kb_pack<PKT_SMALL>, dim3(total(BS_PACK)), dim3(PKT_SMALL), 0, st, a, (uint32_t)o->compat);
    else
        hipLaunchKernelGGL(kb_pack<PKT_LARGE>, dim3(total(BS_PACK)), dim3(PKT_LARGE), 0, st, a, (uint32_t)o->compat);
    if (zlib) {
        hipLaunchKernelGGL(kb_adler_part, dim3(total(BS_ADLER)), dim3(256), 0, st, a);
        if (pk)
            hipLaunchKernelGGL(kb_zlib_tail_placed, dim3(k), dim3(64), 0, st, a);
        else
            hipLaunchKernelGGL(kb_zlib_tail, dim3(k), dim3(64), 0, st, a);
    }
    if (gzip) {
        hipLaunchKernelGGL(kb_crc, dim3(total(BS_CRC)), dim3(256), 0, st, a);
        hipLaunchKernelGGL(kb_gzip_tail, dim3(k), dim3(64), 0, st, a, static_cast<const uint8_t*>(c->b_dev + gz_at));
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(hst, dst, state_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    bool sort_bad = false;  // (only the walk sets it)
    for (uint32_t i = 0; i < k && hashing; i++) sort_bad |= hst[i].sort_bad != 0;
    if (sort_bad) {  // (never seen on MI355X; the set is done again with ballot ranks, as run_encode does)
        if (c->sort_mode == 0) {
            c->err = "batched walk: a bucket out of order with ballot ranks";
            return MI355_E_HIP;
        }
        sort_fell_back(c);
        return batch_launch_set(c, v, k, o, cfg, st, gz, out_len, outcome, sums, pk);  // (a packed set places again from the same end)
    }
    uint64_t end = pk ? pk->tail : 0;
    if (pk) pk->off.assign(k, 0);
    for (uint32_t i = 0; i < k; i++) {
        const DevScalars& s = hst[i].sc;
        uint64_t wpos = 0;
        out_len[i] = 0;
        if (hst[i].spec_bad)
            outcome[i] = BO_SPEC;
        else if (hit[i].q1_check && s.b0_full && q1_rewarm(s.b0_last_tok, s.b0_last_pos, cfg.mode, v[i].n, &wpos))
            outcome[i] = BO_Q1;
        else if (s.ref_panic)
            outcome[i] = BO_PANIC;
        else {
            outcome[i] = BO_OK;
            out_len[i] = stream_bytes(s.total_bits, o->wrapper, gz.of(v[i].idx).hdr_len, false);
            sums->T += s.T;
            sums->nb += s.nb;
            sums->n_stored += s.n_stored;
            sums->n_fixed += s.n_fixed;
            sums->n_dynamic += s.n_dynamic;
            sums->q13_hits += s.q13_hits;
        }
        if (pk) {  // the scan of kb_place once more: the items' offsets
            pk->off[i] = end;
            end += pk->up(out_len[i]);
        }
    }
    if (pk) {
        uint64_t dev_end;
        memcpy(&dev_end, hst + k, sizeof dev_end);
        if (dev_end != end) {
            c->err = "packed batch: the device placed the set's items differently from the host's scan of their lengths";
            return MI355_E_HIP;
        }
        pk->tail = end;
    }
    return MI355_OK;
}

// The whole batch: launch sets over the items the batched kernels take, then the others one by one through the one-input path.
// host: the items' buffers are the caller's host memory (gathered into the context's device staging per launch set).
// gz: the items' gzip headers when o->wrapper is 2 (the _gzip entries), else none.
int run_batch(mi355_deflate_ctx* c, mi355_batch_item* items, size_t n_items, const mi355_deflate_opts* o, hipStream_t st, bool host,
              void* hip_stream, const BatchHeaders& gz, PackedOut* pk = nullptr) {
    const auto t0 = std::chrono::steady_clock::now();
    if (c->live_shard) {
        c->err = "this context holds a sharded encode between mi355_shard_begin and mi355_shard_end";
        return MI355_E_STATE;
    }
    ParseCfg cfg;
    if (const int rc = parse_cfg(c, o, &cfg)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    c->last_plan = nullptr;  // (the workspace is carved again below)
    c->last_nb = 0;
    mi355_batch_info bi;
    memset(&bi, 0, sizeof bi);
    bi.n_items = n_items;
    DevScalars sums;
    memset(&sums, 0, sizeof sums);
    uint64_t sum_out = 0;
    std::vector<size_t> singles;
    std::vector<uint8_t> single_q1(n_items, 0), single_spec(n_items, 0);
    std::vector<BatchView> v;
    for (size_t i = 0; i < n_items; i++) {
        mi355_batch_item& it = items[i];
        bi.in_len += it.in_len;
        const size_t need = mi355_deflate_bound_ex(it.in_len, o->wrapper, gz.of(i).hdr_len, 0);
        it.out_len = 0;
        it.status = MI355_OK;
        if (pk) it.out = nullptr;  // (its address in the arena, once it has one)
        if (!pk && it.out_cap < need) {
            it.out_len = need;
            it.status = MI355_E_OUT_TOO_SMALL;
        } else if (batch_takes(cfg, it.in_len)) {
            v.push_back(BatchView{reinterpret_cast<const uint8_t*>(it.in), it.in_len, reinterpret_cast<uint8_t*>(it.out), need, i});
        } else {
            singles.push_back(i);
        }
    }
    // ---- launch sets: consecutive items up to c->batch_bytes of input (at least one) ----
    std::vector<size_t> out_len;
    std::vector<BatchOutcome> outcome;
    for (size_t s0 = 0; s0 < v.size();) {
        size_t s1 = s0 + 1;
        // (a gzip item counts with its header, which travels with the set's descriptors)
        auto set_bytes = [&](const BatchView& b) { return b.n + gz.of(b.idx).hdr_len; };
        uint64_t bytes = set_bytes(v[s0]);
        while (s1 < v.size() && s1 - s0 < BATCH_ITEMS_MAX && bytes + set_bytes(v[s1]) <= c->batch_bytes) bytes += set_bytes(v[s1++]);
        const uint32_t k = (uint32_t)(s1 - s0);
        BatchView* sv = v.data() + s0;
        std::vector<BatchView> staged;
        if (host) {  // the inputs into the device staging, 256-byte aligned each; the outputs behind them the same way
            std::vector<size_t> in_off(k + 1, 0), out_off(k + 1, 0);
            for (uint32_t i = 0; i < k; i++) {
                in_off[i + 1] = in_off[i] + align_up(sv[i].n + 64, 256);
                out_off[i + 1] = out_off[i] + align_up(sv[i].need, 256);
            }
            int rc = ensure_buf(c, &c->d_in, &c->d_in_cap, in_off[k]);
            if (rc) return rc;
            if (pk) {  // the set's part of the arena: as far as the set can reach and the arena goes
                uint64_t reach = 0;
                for (uint32_t i = 0; i < k; i++) reach += pk->up(sv[i].need);
                out_off[k] = (size_t)std::min<uint64_t>(reach, pk->cap > pk->tail ? pk->cap - pk->tail : 0);
            }
            rc = ensure_buf(c, &c->d_out, &c->d_out_cap, out_off[k]);
            if (rc) return rc;
            staged.assign(sv, sv + k);
            for (uint32_t i = 0; i < k; i++) {
                HIPCHK(c, hipMemcpyAsync(c->d_in + in_off[i], sv[i].d_in, sv[i].n, hipMemcpyHostToDevice, st));
                staged[i].d_in = c->d_in + in_off[i];
                staged[i].d_out = pk ? nullptr : c->d_out + out_off[i];
            }
            sv = staged.data();
        }
        out_len.assign(k, 0);
        outcome.assign(k, BO_OK);
        const uint64_t tail0 = pk ? pk->tail : 0;
        if (pk) pk->set_base = host ? c->d_out : pk->d_arena + tail0;  // (beyond the arena's end nothing is placed: never used)
        const int rc = batch_launch_set(c, sv, k, o, cfg, st, gz, out_len.data(), outcome.data(), &sums, pk);
        if (rc) return rc;
        bi.sub_batches++;
        uint64_t fit_end = tail0;  // the end of the last region of the set that lies inside the arena
        for (uint32_t i = 0; i < k; i++) {
            mi355_batch_item& it = items[sv[i].idx];
            switch (outcome[i]) {
            case BO_OK:
                it.out_len = out_len[i];
                bi.n_batched++;
                if (pk) {
                    const uint64_t off = pk->off[i], region_end = off + pk->up(out_len[i]);
                    if (region_end > pk->cap) {  // (kb_place has left it out)
                        it.status = MI355_E_OUT_TOO_SMALL;
                        break;
                    }
                    it.out = (host ? pk->h_arena : pk->d_arena) + off;
                    fit_end = region_end;
                    sum_out += out_len[i];
                    break;
                }
                sum_out += out_len[i];
                if (host) HIPCHK(c, hipMemcpyAsync(it.out, sv[i].d_out, out_len[i], hipMemcpyDeviceToHost, st));
                break;
            case BO_PANIC:
                it.status = MI355_E_REF_PANIC;
                bi.n_batched++;
                break;
            case BO_Q1:
                single_q1[sv[i].idx] = 1;
                singles.push_back(sv[i].idx);
                break;
            case BO_SPEC:
                single_spec[sv[i].idx] = 1;
                singles.push_back(sv[i].idx);
                break;
            }
        }
        // a packed set's bytes: one copy of its placed range, pad bytes and all
        if (host && pk && fit_end > tail0) HIPCHK(c, hipMemcpyAsync(pk->h_arena + tail0, c->d_out, fit_end - tail0, hipMemcpyDeviceToHost, st));
        if (host) HIPCHK(c, hipStreamSynchronize(st));
        s0 = s1;
    }
    // ---- the rest, one by one, exactly as the one-input entries do it ----
    std::sort(singles.begin(), singles.end());
    uint32_t q1_any = 0, spec_any = 0;
    // (a packed batch: into a buffer of the context -- the device staging output, or host memory -- and from there to the arena's
    // end, once the length is known like everyone else's; the table entries by a small copy each)
    std::vector<uint8_t> h_tmp;
    std::vector<mi355_packed_entry> entries;
    entries.reserve(pk ? singles.size() : 0);
    for (size_t i : singles) {
        mi355_batch_item& it = items[i];
        size_t len = 0;
        int rc;
        const mi355_gzip_header h = gz.of(i);
        if (pk) {
            const size_t need = mi355_deflate_bound_ex(it.in_len, o->wrapper, h.hdr_len, 0);
            if (host) {
                if (h_tmp.size() < need) h_tmp.resize(need);
            } else if (const int e = ensure_buf(c, &c->d_out, &c->d_out_cap, need)) {
                return e;
            }
            it.out = host ? static_cast<void*>(h_tmp.data()) : static_cast<void*>(c->d_out);
            it.out_cap = need;
        }
        if (gz.gzip && host)
            rc = mi355_deflate_encode_gzip(c, reinterpret_cast<const uint8_t*>(it.in), it.in_len, o, h.hdr, h.hdr_len,
                                           reinterpret_cast<uint8_t*>(it.out), it.out_cap, &len);
        else if (gz.gzip)
            rc = mi355_deflate_encode_device_gzip(c, it.in, it.in_len, o, h.hdr, h.hdr_len, it.out, it.out_cap, &len, hip_stream);
        else if (host)
            rc = mi355_deflate_encode(c, reinterpret_cast<const uint8_t*>(it.in), it.in_len, o, reinterpret_cast<uint8_t*>(it.out),
                                      it.out_cap, &len);
        else
            rc = mi355_deflate_encode_device(c, it.in, it.in_len, o, it.out, it.out_cap, &len, hip_stream);
        if (rc == MI355_E_HIP) return rc;  // (the device or the runtime failed: nothing else is trustworthy)
        bi.n_single++;
        bi.n_q1_single += single_q1[i];
        bi.n_spec_single += single_spec[i];
        it.status = rc;
        it.out_len = (rc == MI355_OK || rc == MI355_E_OUT_TOO_SMALL) ? len : 0;
        if (pk) {
            const void* const src = it.out;
            const uint64_t off = pk->tail, region = rc == MI355_OK ? pk->up(len) : 0;
            it.out = nullptr;
            it.out_cap = 0;
            if (rc == MI355_OK && off + region > pk->cap) {
                it.status = MI355_E_OUT_TOO_SMALL;
            } else if (rc == MI355_OK && host) {
                memcpy(pk->h_arena + off, src, len);
                memset(pk->h_arena + off + len, 0, region - len);
                it.out = pk->h_arena + off;
            } else if (rc == MI355_OK) {
                if (len) HIPCHK(c, hipMemcpyAsync(pk->d_arena + off, src, len, hipMemcpyDeviceToDevice, st));
                if (region > len) HIPCHK(c, hipMemsetAsync(pk->d_arena + off + len, 0, region - len, st));
                it.out = pk->d_arena + off;
            }
            pk->tail += region;
            if (pk->d_table) {
                entries.push_back(mi355_packed_entry{off, it.out_len, it.status, 0u});
                HIPCHK(c, hipMemcpyAsync(pk->d_table + i, &entries.back(), sizeof(mi355_packed_entry), hipMemcpyHostToDevice, st));
            }
        }
        if (rc == MI355_OK && it.status == MI355_OK) sum_out += len;
        if (rc == MI355_OK) {
            const mi355_deflate_info& in1 = c->info;
            sums.T += (uint32_t)in1.n_tokens;
            sums.nb += in1.n_blocks;
            sums.n_stored += in1.n_stored;
            sums.n_fixed += in1.n_fixed;
            sums.n_dynamic += in1.n_dynamic;
            sums.q13_hits += in1.q13_hits;
            q1_any |= in1.q1_rewarm;
            spec_any |= in1.spec_fallback;
        }
    }
    if (!host) HIPCHK(c, hipStreamSynchronize(st));
    bi.out_len = sum_out;
    bi.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    c->batch = bi;
    // mi355_deflate_last_info: the batch as a whole; mi355_deflate_last_blocks: none
    mi355_deflate_info& info = c->info;
    memset(&info, 0, sizeof info);
    info.in_len = bi.in_len;
    info.out_len = bi.out_len;
    info_from_scalars(&info, sums);
    info.q1_rewarm = q1_any ? 1u : 0u;
    info.spec_fallback = spec_any;
    info.passes = 1;
    info.total_ms = bi.total_ms;
    c->pend_passes = 0;
    c->last_plan = nullptr;
    c->last_nb = 0;
    for (size_t i = 0; i < n_items; i++)
        if (items[i].status != MI355_OK) return items[i].status;
    return MI355_OK;
}

// the checks of the call itself (nothing is written to an item when one fails)
int batch_args_ok(mi355_deflate_ctx* c, const mi355_batch_item* items, size_t n_items, const mi355_deflate_opts* o, bool device,
                  const BatchHeaders& gz) {
    if (!o || (!items && n_items)) return MI355_E_ARG;
    if (o->wrapper > 1 && !gz.gzip) {
        c->err = "batched encode: wrapper 0 (raw) or 1 (zlib) only; gzip has the _gzip entries";
        return MI355_E_ARG;
    }
    if (gz.gzip) {  // (the rule of the single gzip call, run_encode)
        if ((gz.n && !gz.h) || (gz.n > 1 && gz.n != n_items)) {
            c->err = "batched gzip encode: n_hdrs is 0 (blank header), 1 (one for all) or n_items";
            return MI355_E_ARG;
        }
        for (size_t i = 0; i < gz.n; i++)
            if (!gz.h[i].hdr || gz.h[i].hdr_len == 0 || gz.h[i].hdr_len > 0xFFFF) {
                c->err = "batched gzip encode: a header of 1 .. 65535 bytes per entry";
                return MI355_E_ARG;
            }
    }
    if (o->flush != MI355_FLUSH_FINISH) {
        c->err = "batched encode: MI355_FLUSH_FINISH only";
        return MI355_E_ARG;
    }
    for (size_t i = 0; i < n_items; i++) {
        if ((!items[i].in && items[i].in_len) || !items[i].out) return MI355_E_ARG;
        if (device && (reinterpret_cast<uintptr_t>(items[i].out) & 3)) {
            c->err = "batched encode: every item's device output must be 4-byte aligned";
            return MI355_E_ARG;
        }
    }
    return MI355_OK;
}

// the checks of a packed call (nothing is written when one fails); *align: 0 becomes 4
int packed_args_ok(mi355_deflate_ctx* c, const mi355_batch_item* items, size_t n_items, const mi355_deflate_opts* o, const BatchHeaders& gz,
                   const void* arena, size_t* align, bool device) {
    if (!o || (!items && n_items)) return MI355_E_ARG;
    if (o->wrapper < 0 || o->wrapper > 2) {
        c->err = "packed batch: wrapper 0 (raw), 1 (zlib) or 2 (gzip)";
        return MI355_E_ARG;
    }
    if (*align == 0) *align = 4;
    if (*align < 4 || *align > 4096 || (*align & (*align - 1))) {
        c->err = "packed batch: align is a power of two from 4 to 4096 (0: 4)";
        return MI355_E_ARG;
    }
    if (!arena && n_items) {
        c->err = "packed batch: no arena";
        return MI355_E_ARG;
    }
    if (device && (reinterpret_cast<uintptr_t>(arena) & (*align - 1))) {
        c->err = "packed batch: the device arena must be aligned to align";
        return MI355_E_ARG;
    }
    if (gz.gzip) {  // (the rule of the _gzip entries)
        if ((gz.n && !gz.h) || (gz.n > 1 && gz.n != n_items)) {
            c->err = "batched gzip encode: n_hdrs is 0 (blank header), 1 (one for all) or n_items";
            return MI355_E_ARG;
        }
        for (size_t i = 0; i < gz.n; i++)
            if (!gz.h[i].hdr || gz.h[i].hdr_len == 0 || gz.h[i].hdr_len > 0xFFFF) {
                c->err = "batched gzip encode: a header of 1 .. 65535 bytes per entry";
                return MI355_E_ARG;
            }
    }
    if (o->flush != MI355_FLUSH_FINISH) {
        c->err = "batched encode: MI355_FLUSH_FINISH only";
        return MI355_E_ARG;
    }
    for (size_t i = 0; i < n_items; i++)
        if (!items[i].in && items[i].in_len) return MI355_E_ARG;
    return MI355_OK;
}

int run_packed(mi355_deflate_ctx* c, mi355_batch_item* items, size_t n_items, const mi355_deflate_opts* opts, const mi355_gzip_header* hdrs,
               size_t n_hdrs, uint8_t* d_arena, uint8_t* h_arena, size_t arena_cap, size_t align, mi355_packed_entry* d_table,
               size_t* arena_used, void* hip_stream) {
    const bool device = d_arena != nullptr || !h_arena;
    const BatchHeaders gz = (opts && opts->wrapper == 2) ? BatchHeaders{hdrs, n_hdrs, true} : BatchHeaders{};
    int rc = packed_args_ok(c, items, n_items, opts, gz, device ? static_cast<const void*>(d_arena) : h_arena, &align, device);
    if (rc) return rc;
    hipStream_t st = (device && hip_stream) ? reinterpret_cast<hipStream_t>(hip_stream) : c->own_stream;
    PackedOut pk{d_arena, h_arena, arena_cap, (uint32_t)align, d_table, 0, nullptr, {}};
    rc = run_batch(c, items, n_items, opts, st, !device, device ? hip_stream : nullptr, gz, &pk);
    // (the checks inside run_batch -- the options, a live shard -- fail before the first item is written)
    if (rc == MI355_E_HIP || rc == MI355_E_UNSUPPORTED || rc == MI355_E_STATE || rc == MI355_E_ARG) return rc;
    if (arena_used) *arena_used = (size_t)pk.tail;
    return rc;
}

}  // namespace

extern "C" {

size_t mi355_deflate_batch_packed_bound(const mi355_batch_item* items, size_t n_items, int wrapper, const mi355_gzip_header* hdrs,
                                        size_t n_hdrs, size_t align) {
    if (align == 0) align = 4;
    if ((!items && n_items) || align < 4 || align > 4096 || (align & (align - 1))) return 0;
    const BatchHeaders gz = wrapper == 2 ? BatchHeaders{hdrs, n_hdrs, true} : BatchHeaders{};
    if (gz.gzip && ((gz.n && !gz.h) || (gz.n > 1 && gz.n != n_items))) return 0;
    size_t sum = 0;
    for (size_t i = 0; i < n_items; i++) sum += align_up(mi355_deflate_bound_ex(items[i].in_len, wrapper, gz.of(i).hdr_len, 0), align);
    return sum;
}

int mi355_deflate_encode_batch_packed(mi355_deflate_ctx* c, mi355_batch_item* items, size_t n_items, const mi355_deflate_opts* opts,
                                      const mi355_gzip_header* hdrs, size_t n_hdrs, uint8_t* arena, size_t arena_cap, size_t align,
                                      size_t* arena_used) {
    DefaultGuard dg_;
    c = use_ctx(c, dg_);
    if (!c) return MI355_E_HIP;
    if (!arena && n_items) {
        c->err = "packed batch: no arena";
        return MI355_E_ARG;
    }
    static uint8_t none;  // (an empty batch may come without an arena)
    return run_packed(c, items, n_items, opts, hdrs, n_hdrs, nullptr, arena ? arena : &none, arena ? arena_cap : 0, align, nullptr,
                      arena_used, nullptr);
}

int mi355_deflate_encode_batch_packed_device(mi355_deflate_ctx* c, mi355_batch_item* items, size_t n_items, const mi355_deflate_opts* opts,
                                             const mi355_gzip_header* hdrs, size_t n_hdrs, void* d_arena, size_t arena_cap, size_t align,
                                             mi355_packed_entry* d_table, size_t* arena_used, void* hip_stream) {
    DefaultGuard dg_;
    c = use_ctx(c, dg_);
    if (!c) return MI355_E_HIP;
    return run_packed(c, items, n_items, opts, hdrs, n_hdrs, static_cast<uint8_t*>(d_arena), nullptr, arena_cap, align, d_table, arena_used,
                      hip_stream);
}

int mi355_deflate_encode_batch(mi355_deflate_ctx* c, mi355_batch_item* items, size_t n_items, const mi355_deflate_opts* opts) {
    DefaultGuard dg_;
    c = use_ctx(c, dg_);
    if (!c) return MI355_E_HIP;
    int rc = batch_args_ok(c, items, n_items, opts, false, BatchHeaders{});
    if (rc) return rc;
    return run_batch(c, items, n_items, opts, c->own_stream, true, nullptr, BatchHeaders{});
}

int mi355_deflate_encode_batch_device(mi355_deflate_ctx* c, mi355_batch_item* items, size_t n_items, const mi355_deflate_opts* opts,
                                      void* hip_stream) {
    DefaultGuard dg_;
    c = use_ctx(c, dg_);
    if (!c) return MI355_E_HIP;
    int rc = batch_args_ok(c, items, n_items, opts, true, BatchHeaders{});
    if (rc) return rc;
    hipStream_t st = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : c->own_stream;
    return run_batch(c, items, n_items, opts, st, false, hip_stream, BatchHeaders{});
}

int mi355_deflate_encode_batch_gzip(mi355_deflate_ctx* c, mi355_batch_item* items, size_t n_items, const mi355_deflate_opts* opts,
                                    const mi355_gzip_header* hdrs, size_t n_hdrs) {
    DefaultGuard dg_;
    c = use_ctx(c, dg_);
    if (!c) return MI355_E_HIP;
    if (!opts) return MI355_E_ARG;
    mi355_deflate_opts o = *opts;
    o.wrapper = 2;
    const BatchHeaders gz{hdrs, n_hdrs, true};
    int rc = batch_args_ok(c, items, n_items, &o, false, gz);
    if (rc) return rc;
    return run_batch(c, items, n_items, &o, c->own_stream, true, nullptr, gz);
}

int mi355_deflate_encode_batch_device_gzip(mi355_deflate_ctx* c, mi355_batch_item* items, size_t n_items, const mi355_deflate_opts* opts,
                                           const mi355_gzip_header* hdrs, size_t n_hdrs, void* hip_stream) {
    DefaultGuard dg_;
    c = use_ctx(c, dg_);
    if (!c) return MI355_E_HIP;
    if (!opts) return MI355_E_ARG;
    mi355_deflate_opts o = *opts;
    o.wrapper = 2;
    const BatchHeaders gz{hdrs, n_hdrs, true};
    int rc = batch_args_ok(c, items, n_items, &o, true, gz);
    if (rc) return rc;
    hipStream_t st = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : c->own_stream;
    return run_batch(c, items, n_items, &o, st, false, hip_stream, gz);
}

int mi355_deflate_last_batch_info(mi355_deflate_ctx* c, mi355_batch_info* info) {
    if (!c || !info) return MI355_E_ARG;
    *info = c->batch;
    return MI355_OK;
}

}  // extern "C"
