// BGZF encode (include/mi355_deflate.h mi355_bgzf_encode[_device]): one input in device memory, one blocked gzip file in device memory.
// Phase 1 is the packed batch as it stands (deflate_batch.inc run_packed): the input's slices of block_size bytes are its items,
// wrapper 2, the one shared header kBgzfHeader, align 4, into an arena of the context's; the mi355_packed_entry table stays on the
// device.  Phase 2 reads only that table: k_bgzf_place scans the members' lengths in slice order -- whatever order the packed batch
// gave their regions -- into dense file offsets, the member rows, the file's length and the verdict; k_bgzf_gather moves every member
// from its 4-byte aligned region to its byte offset in the file, puts BSIZE = len - 1 into bytes 16..17 on the way and appends the
// end-of-file marker.  Two launches, no host round trip between them, one copy back and one wait behind them.  DESIGN.md section 18.
namespace mi355 {

constexpr uint32_t BGZF_PLACE_T = 1024;   // members per round of k_bgzf_place's scan
constexpr uint32_t BGZF_GATHER_T = 256;   // granules of 16 output bytes per workgroup of k_bgzf_gather
constexpr uint32_t BGZF_EOF_LEN = 28;     // the end-of-file marker: the reference's gzip member of the empty input under kBgzfHeader
constexpr uint64_t BGZF_MEMBER_MAX = 65536;  // what BSIZE (16 bits holding len - 1) can express

struct BgzfHead {       // what the one copy back begins with; the member rows follow
    uint64_t file_len;  // the scan's end + the marker
    uint32_t bad;       // the first slice whose status is not OK or whose member is longer than BGZF_MEMBER_MAX; 0xffffffff: none
    int32_t code;       // ... that slice's status, or MI355_E_UNSUPPORTED for the length
    uint64_t reserved[2];
};  // 32 bytes, so that the rows behind it stay 8-byte aligned
struct BgzfArgs {
    const uint8_t* scratch;           // the arena of the packed batch
    const mi355_packed_entry* table;  // n entries in slice order
    uint64_t* file_off;               // n + 1: the members' first bytes in the file, then the marker's
    BgzfHead* head;
    mi355_member_info* rows;  // n + 1, the marker's last
    uint32_t n;
    uint64_t in_len, block;
};

// byte r of the end-of-file marker: 1f 8b 08 04 | 00 00 00 00 | 00 ff 06 00 | 42 43 02 00 | 1b 00 03 00 | 00 ... (28 bytes)
__device__ __forceinline__ uint32_t bgzf_eof_byte(uint32_t r) {
    const uint32_t w = r < 4 ? 0x04088b1fu : r < 8 ? 0u : r < 12 ? 0x0006ff00u : r < 16 ? 0x00024342u : r < 20 ? 0x0003001bu : 0u;
    return (w >> (8 * (r & 3))) & 0xffu;
}

// One workgroup: the 64-bit exclusive scan of table[k].len in slice order, BGZF_PLACE_T members a round as kb_place does it (shuffles
// inside a wave, the waves' sums through LDS, the running end carried from round to round).
__global__ __launch_bounds__(BGZF_PLACE_T) void k_bgzf_place(BgzfArgs a) {
    __shared__ uint64_t s_wave[BGZF_PLACE_T / 64];
    __shared__ uint32_t s_bad;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) s_bad = 0xffffffffu;
    __syncthreads();
    uint64_t end = 0;
    for (uint32_t i0 = 0; i0 < a.n; i0 += BGZF_PLACE_T) {
        const uint32_t i = i0 + tid;
        uint64_t len = 0;
        if (i < a.n) {
            len = a.table[i].len;
            if (a.table[i].status != MI355_OK || len > BGZF_MEMBER_MAX) atomicMin(&s_bad, i);
        }
        uint64_t incl = len;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint64_t y = shfl_up_u64(incl, off);
            if (lane >= (uint32_t)off) incl += y;
        }
        if (lane == 63) s_wave[wv] = incl;
        __syncthreads();
        uint64_t wbase = 0, total = 0;
#pragma unroll
        for (uint32_t k = 0; k < BGZF_PLACE_T / 64; k++) {
            const uint64_t y = s_wave[k];
            if (k < wv) wbase += y;
            total += y;
        }
        if (i < a.n) {
            const uint64_t off = end + wbase + (incl - len), in0 = (uint64_t)i * a.block;
            a.file_off[i] = off;
            a.rows[i] = mi355_member_info{off, len, in0, a.in_len - in0 < a.block ? a.in_len - in0 : a.block, MI355_MEMBER_HINTED, 0u};
        }
        end += total;
        __syncthreads();  // (the next round's sums behind this round's reads of them; s_bad behind its last atomic)
    }
    if (tid) return;
    const uint32_t bad = s_bad;
    a.file_off[a.n] = end;
    a.rows[a.n] = mi355_member_info{end, BGZF_EOF_LEN, a.in_len, 0, MI355_MEMBER_HINTED, 0u};
    int32_t code = MI355_OK;
    if (bad != 0xffffffffu) code = a.table[bad].status != MI355_OK ? a.table[bad].status : MI355_E_UNSUPPORTED;
    *a.head = BgzfHead{end + BGZF_EOF_LEN, bad, code, {0, 0}};
}

// byte p of the file, p inside member m or the one behind it (m: the last member that begins at or below the granule's first byte)
__device__ __forceinline__ uint32_t bgzf_file_byte(const BgzfArgs& a, uint64_t p, uint32_t m) {
    if (m < a.n && p >= a.file_off[m + 1]) m++;
    const uint32_t r = (uint32_t)(p - a.file_off[m]);
    if (m == a.n) return bgzf_eof_byte(r);
    const mi355_packed_entry e = a.table[m];
    if (r == 16) return (uint32_t)(e.len - 1) & 0xffu;
    if (r == 17) return (uint32_t)((e.len - 1) >> 8) & 0xffu;
    return a.scratch[e.off + r];
}

// The only kernel that writes the caller's buffer, and below min(file length, out_cap) only.  Destination-centric: a thread owns the
// aligned 16-byte granule g of the output, finds the member that covers its first byte by a search over the file offsets (a second
// one may begin inside the granule, never a third: no member is shorter than 28 bytes) and stores the granule with one 16-byte
// store; a granule that the file or the room ends in gets byte stores.  No granule is written by two threads.  A granule inside one
// member and clear of its BSIZE bytes -- all but two a member -- is put together from five aligned source words with funnel shifts
// (a member's region begins on a word, its place in the file on any byte); the others byte by byte.
__global__ __launch_bounds__(BGZF_GATHER_T) void k_bgzf_gather(BgzfArgs a, uint8_t* __restrict__ out, uint64_t out_cap) {
    if (a.head->bad != 0xffffffffu) return;  // (no valid file is promised)
    const uint64_t file_len = a.head->file_len, limit = file_len < out_cap ? file_len : out_cap;
    const uint64_t p0 = ((uint64_t)blockIdx.x * BGZF_GATHER_T + threadIdx.x) * 16;
    if (p0 >= limit) return;
    uint32_t lo = 0, hi = a.n;  // the last m in [0, n] with file_off[m] <= p0 (file_off[0] = 0)
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (a.file_off[mid] <= p0)
            lo = mid;
        else
            hi = mid - 1;
    }
    const uint32_t m = lo;
    const uint64_t r = p0 - a.file_off[m];
    uint32_t v[4];
    if (m < a.n && p0 + 16 <= a.file_off[m + 1] && (r >= 18 || r == 0)) {
        const uint64_t s = a.table[m].off + r;
        const uint32_t* const w = reinterpret_cast<const uint32_t*>(a.scratch + (s & ~(uint64_t)3));  // (the arena is 4-byte aligned)
        const uint32_t sh = 8 * (uint32_t)(s & 3);
        uint32_t x[5];
#pragma unroll
        for (int k = 0; k < 5; k++) x[k] = (k < 4 || sh) ? w[k] : 0u;  // (the fifth word only where a shift needs it)
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = (uint32_t)(((((uint64_t)x[k + 1]) << 32) | x[k]) >> sh);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            v[k] = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const uint64_t p = p0 + 4 * k + b;
                if (p < file_len) v[k] |= bgzf_file_byte(a, p, m) << (8 * b);
            }
        }
    }
    if (p0 + 16 <= limit) {
        *reinterpret_cast<uint4*>(out + p0) = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
        for (uint32_t b = 0; p0 + b < limit; b++) out[p0 + b] = (uint8_t)(v[b >> 2] >> (8 * (b & 3)));
    }
}

}  // namespace mi355

namespace {

// BGZF's member header (the SAM specification, section 4.1): FEXTRA, MTIME 0, XFL 0, OS 255, XLEN 6, subfield 'B','C' of length 2,
// BSIZE zero -- the gather writes the true one
const uint8_t kBgzfHeader[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0, 0};
constexpr size_t BGZF_BLOCK_MAX = 65280;  // bgzip's 0xff00

size_t bgzf_members(size_t in_len, size_t block) { return in_len / block + (in_len % block ? 1 : 0); }

// the argument errors of both entries, decided before the context or the device is touched
bool bgzf_args_bad(const mi355_deflate_ctx* c, const void* in, size_t in_len, const mi355_deflate_opts* o, size_t block, const void* out,
                   size_t out_cap, const size_t* out_len, const mi355_member_info* members, size_t members_cap, bool device) {
    if (!c || !o || !out_len || block > BGZF_BLOCK_MAX || (!in && in_len) || (!out && out_cap) || (!members && members_cap)) return true;
    return device && (reinterpret_cast<uintptr_t>(out) & 15) != 0;
}

// the device worker of both entries
int bgzf_run(mi355_deflate_ctx* c, const uint8_t* d_in, size_t in_len, const mi355_deflate_opts* opts, size_t block, uint8_t* d_out,
             size_t out_cap, size_t* out_len, mi355_member_info* members, size_t members_cap, size_t* n_members, void* hip_stream) {
    if (block == 0) block = BGZF_BLOCK_MAX;
    const size_t n = bgzf_members(in_len, block);
    if (n >= 0x7fffffffull) {
        c->err = "bgzf encode: too many members";
        return MI355_E_UNSUPPORTED;
    }
    mi355_deflate_opts o = *opts;
    o.wrapper = 2;
    if (o.flush != MI355_FLUSH_FINISH) {
        c->err = "bgzf encode: MI355_FLUSH_FINISH only";
        return MI355_E_ARG;
    }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = call_stream(c, hip_stream);
    StageClocks<3, 4> clk{c->bz_ev, c->bz_ev_ok, c->bz_ms, st, stage_clocks_on(c, in_len)};
    int rc = clk.begin(c);
    if (rc) return rc;
    // ---- phase 1: the slices through the packed batch, into the context's arena ----
    std::vector<mi355_batch_item> items(n);
    for (size_t k = 0; k < n; k++) {
        memset(&items[k], 0, sizeof items[k]);
        items[k].in = d_in + k * block;
        items[k].in_len = std::min(block, in_len - k * block);
    }
    const mi355_gzip_header hdr{kBgzfHeader, sizeof kBgzfHeader};
    const size_t arena_cap = mi355_deflate_batch_packed_bound(items.data(), n, 2, &hdr, 1, 4);
    rc = ensure_buf(c, &c->bz_arena, &c->bz_arena_cap, arena_cap + 64);  // (the gather reads whole words: up to 7 bytes behind a member)
    if (rc) return rc;
    // [table n] | [file offsets n + 1] | [head][rows n + 1]
    const size_t off_at = align_up(sizeof(mi355_packed_entry) * n, 256), head_at = align_up(off_at + sizeof(uint64_t) * (n + 1), 256);
    const size_t rows_give = members ? std::min(members_cap, n + 1) : 0, back_bytes = sizeof(mi355::BgzfHead) + sizeof(mi355_member_info) * rows_give;
    rc = ensure_buf(c, &c->bz_tab, &c->bz_tab_cap, head_at + sizeof(mi355::BgzfHead) + sizeof(mi355_member_info) * (n + 1));
    if (rc) return rc;
    if (back_bytes > c->bz_host_cap) {
        if (c->bz_host) (void)hipHostFree(c->bz_host);
        c->bz_host = nullptr;
        c->bz_host_cap = 0;
        HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&c->bz_host), back_bytes, 0));
        c->bz_host_cap = back_bytes;
    }
    mi355_packed_entry* const d_table = reinterpret_cast<mi355_packed_entry*>(c->bz_tab);
    HIPCHK(c, clk.mark(0));
    size_t used = 0;
    // (the internal driver: its checks of the options and of a live shard come before the first launch)
    rc = run_packed(c, items.data(), n, &o, &hdr, 1, c->bz_arena, nullptr, arena_cap, 4, d_table, &used, hip_stream);
    if (rc == MI355_E_HIP || rc == MI355_E_UNSUPPORTED || rc == MI355_E_STATE || rc == MI355_E_ARG) return rc;
    // (an item's own status -- MI355_E_REF_PANIC -- is in the table: the verdict is k_bgzf_place's)
    HIPCHK(c, clk.mark(1));
    // ---- phase 2: place and gather ----
    mi355::BgzfHead* const d_head = reinterpret_cast<mi355::BgzfHead*>(c->bz_tab + head_at);
    const mi355::BgzfArgs a{c->bz_arena, d_table, reinterpret_cast<uint64_t*>(c->bz_tab + off_at), d_head,
                            reinterpret_cast<mi355_member_info*>(c->bz_tab + head_at + sizeof(mi355::BgzfHead)), (uint32_t)n, in_len, block};
    hipLaunchKernelGGL(mi355::k_bgzf_place, dim3(1), dim3(mi355::BGZF_PLACE_T), 0, st, a);
    HIPCHK(c, clk.mark(2));
    // the gather's grid: the room, or what the file can be at most (the regions of the arena are the members rounded up)
    const uint64_t reach = std::min<uint64_t>(out_cap, (uint64_t)used + mi355::BGZF_EOF_LEN);
    const uint64_t wgs = cdiv(reach, 16 * mi355::BGZF_GATHER_T);
    if (wgs > 0x7fffffffull) {
        c->err = "bgzf encode: the file is too long for one launch";
        return MI355_E_UNSUPPORTED;
    }
    if (wgs) hipLaunchKernelGGL(mi355::k_bgzf_gather, dim3((uint32_t)wgs), dim3(mi355::BGZF_GATHER_T), 0, st, a, d_out, (uint64_t)out_cap);
    HIPCHK(c, clk.mark(3));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->bz_host, d_head, back_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    clk.lap(0, 1, 0);
    clk.lap(1, 2, 1);
    clk.lap(2, 3, 2);
    mi355::BgzfHead head;
    memcpy(&head, c->bz_host, sizeof head);
    if (n_members) *n_members = n + 1;
    if (rows_give) memcpy(members, c->bz_host + sizeof head, sizeof(mi355_member_info) * rows_give);
    if (head.bad != 0xffffffffu) {
        char buf[128];
        snprintf(buf, sizeof buf, head.code == MI355_E_UNSUPPORTED ? "bgzf encode: member %u is longer than 65536 bytes" : "bgzf encode: member %u failed",
                 head.bad);
        c->err = buf;
        *out_len = 0;
        return head.code;
    }
    *out_len = (size_t)head.file_len;
    if (head.file_len > out_cap) return MI355_E_OUT_TOO_SMALL;
    return MI355_OK;
}

}  // namespace

extern "C" {

size_t mi355_bgzf_bound(size_t in_len, size_t block_size) {
    if (block_size > BGZF_BLOCK_MAX) return 0;
    if (block_size == 0) block_size = BGZF_BLOCK_MAX;
    const size_t rest = in_len % block_size;
    return in_len / block_size * mi355_deflate_bound_ex(block_size, 2, sizeof kBgzfHeader, 0) +
           (rest ? mi355_deflate_bound_ex(rest, 2, sizeof kBgzfHeader, 0) : 0) + mi355::BGZF_EOF_LEN;
}

int mi355_bgzf_encode_device(mi355_deflate_ctx* c, const void* d_in, size_t in_len, const mi355_deflate_opts* opts, size_t block_size,
                             void* d_out, size_t out_cap, size_t* out_len, mi355_member_info* members, size_t members_cap,
                             size_t* n_members, void* hip_stream) {
    if (bgzf_args_bad(c, d_in, in_len, opts, block_size, d_out, out_cap, out_len, members, members_cap, true)) return MI355_E_ARG;
    DefaultGuard dg_;
    c = use_ctx(c, dg_);
    return bgzf_run(c, static_cast<const uint8_t*>(d_in), in_len, opts, block_size, static_cast<uint8_t*>(d_out), out_cap, out_len, members,
                    members_cap, n_members, hip_stream);
}

// host buffers: plain copies around the device worker
int mi355_bgzf_encode(mi355_deflate_ctx* c, const uint8_t* in, size_t in_len, const mi355_deflate_opts* opts, size_t block_size, uint8_t* out,
                      size_t out_cap, size_t* out_len, mi355_member_info* members, size_t members_cap, size_t* n_members) {
    if (bgzf_args_bad(c, in, in_len, opts, block_size, out, out_cap, out_len, members, members_cap, false)) return MI355_E_ARG;
    DefaultGuard dg_;
    c = use_ctx(c, dg_);
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure_buf(c, &c->d_in, &c->d_in_cap, in_len + 64);
    if (rc) return rc;
    // (the file in a buffer of its own: the one-input path of the packed batch works in the context's output staging)
    const size_t room = std::min(out_cap, mi355_bgzf_bound(in_len, block_size));
    rc = ensure_buf(c, &c->bz_out, &c->bz_out_cap, room + 16);
    if (rc) return rc;
    hipStream_t st = c->own_stream;
    if (in_len) HIPCHK(c, hipMemcpyAsync(c->d_in, in, in_len, hipMemcpyHostToDevice, st));
    rc = bgzf_run(c, c->d_in, in_len, opts, block_size, room ? c->bz_out : nullptr, room, out_len, members, members_cap, n_members, nullptr);
    if (rc != MI355_OK) {
        (void)hipStreamSynchronize(st);  // (the copy of the caller's buffer may be in flight)
        return rc;
    }
    if (*out_len) HIPCHK(c, hipMemcpy(out, c->bz_out, *out_len, hipMemcpyDeviceToHost));
    return MI355_OK;
}

// HIP-event milliseconds of the context's last BGZF encode: the packed encode, the place, the gather; zeros unless the stage clocks
// were on (MI355_CFG_STAGE_CLOCKS)
int mi355_bgzf_last_stages(mi355_deflate_ctx* c, float ms[3]) {
    if (!c || !ms) return MI355_E_ARG;
    for (int k = 0; k < 3; k++) ms[k] = c->bz_ms[k];
    return MI355_OK;
}

}  // extern "C"
