// Large plain members (include/mi355_deflate.h mi355_inflate_members[_device], MI355_CFG_INFLATE_MEMBER_PARALLEL_BYTES): the kernels
// behind inflate_bigmembers.h, which has the rules and the control flow (ib_chain) that tests/inflbig/ runs on the host too.
//   k_bigmember_find        one workgroup of one wave per span of a member's extent: the span's candidate (k_index_find's text on the
//                           member's grid); span 0's workgroup leaves the member's head as well
//   k_bigmember_walk        one workgroup of one wave per walker: k_index_walk's text with the extent's edge
//   k_inflate_mtab          one workgroup of one wave per entry of a group: k_inflate_tab with the entry's part in hand
//   k_inflate_mtab_window   one workgroup per PART: the window walk (it_window_walk.inc) over the part's entries
//   k_inflate_mtab_resolve  flat over the group's symbols -- the only kernel that writes `out`
// Nothing waits inside a kernel.  The host side is MemberDev's (deflate_members_inflate.inc).  DESIGN.md section 15.
#include "inflate_bigmembers.h"

namespace mi355 {

// the index finder's ballot, the walker's sink, and a hinted member's extent for the head
struct BigOps : IndexOps {
    static __host__ __device__ uint64_t total(uint32_t bsize) { return im::Rules::total(bsize); }
};

struct DItem {
    const uint8_t* s;
    uint64_t n, o, S;
    uint64_t rewalk, k_lo, k_hi;  // the walkers: span `rewalk` and [k_lo, k_hi); the extent's edge is k_hi
    uint32_t first, pad;          // the finder begins at span 0 (the head) and not at k_lo
};

__global__ __launch_bounds__(64) void k_bigmember_find(const DItem d, uint64_t* __restrict__ cand, ib::Head* __restrict__ head) {
    __shared__ ic::Tables s_t;
    const uint64_t k = (d.first ? 0 : d.k_lo) + blockIdx.x;
    if (k >= d.k_hi) return;
    const uint64_t c = ib::ib_find_span<BigOps>(s_t, d.s, d.n, d.o, k, d.S);
    if (threadIdx.x == 0) cand[k] = c;
    if (k == 0) {
        ib::Head h;
        ib::ib_head<BigOps>(d.s, d.n, d.o, h);
        if (threadIdx.x == 0) *head = h;
    }
}

__global__ __launch_bounds__(64) void k_bigmember_walk(const DItem d, const uint64_t* __restrict__ cand, ix::Walk* __restrict__ recs) {
    __shared__ ic::Tables s_t;
    const uint64_t k = blockIdx.x == 0 ? d.rewalk : d.k_lo + blockIdx.x - 1;
    if (k >= d.k_hi) return;
    ix::Walk r;
    ib::ib_walk_span<BigOps>(s_t, d.s, d.n, d.o, cand, d.S, k, d.k_hi, r);
    if (threadIdx.x == 0) recs[k] = r;
}

// pass 1
__global__ __launch_bounds__(64) void k_inflate_mtab(const ib::Part* __restrict__ parts, const ic::Entry* __restrict__ ents, uint16_t* sym,
                                                     ic::Rec* __restrict__ recs) {
    __shared__ ic::Tables s_t;
    const ic::Entry e = ents[blockIdx.x];
    const ib::Part pt = parts[e.item];
    ic::Rec r;
    ib::ib_decode_entry<TabSink>(s_t, sym, pt, e, r);
    if (threadIdx.x == 0) recs[blockIdx.x] = r;
}

// pass 2: the workgroup of part blockIdx.x walks the part's entries in order (it_window_walk.inc), two windows ping-ponged in LDS, from
// zeros -- a member begins -- or from the window the group before left in slot 0.  Slot e + 1 gets the window behind entry e when the
// part's next entry or the next group reads it.  It stops at the part's first failing entry and leaves the position up to which pass
// 3 may write.
__global__ __launch_bounds__(1024) void k_inflate_mtab_window(const ib::Part* __restrict__ parts, const ic::Entry* __restrict__ ents,
                                                              const ic::Rec* __restrict__ recs, const uint16_t* __restrict__ sym, uint8_t* win,
                                                              uint32_t n_group, uint64_t* __restrict__ limits) {
    __shared__ __attribute__((aligned(16))) uint8_t s_w[2][it::WIN];
    const ib::Part pt = parts[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = 0; i < it::WIN / 4096; i++) {
        const uint32_t j = (tid + 1024 * i) * 4;
        *reinterpret_cast<uint32_t*>(&s_w[0][j]) = pt.carried ? *reinterpret_cast<const uint32_t*>(win + (uint64_t)pt.e0 * it::WIN + j) : 0u;
    }
    __syncthreads();
    // (the window behind the part's last entry is always made, and stored only where the next group reads it)
    const it::Walk wk{sym + pt.sym_off, ents + pt.e0, recs + pt.e0, pt.n, pt.base, pt.cap, win, pt.e0, n_group, true};
    const WgWalk wp{tid};
#include "it_window_walk.inc"
    if (tid == 0) limits[blockIdx.x] = limit;
}

// pass 3: flat over the group's symbol elements, 16 a thread
__global__ __launch_bounds__(256) void k_inflate_mtab_resolve(const ib::Part* __restrict__ parts, uint32_t n_parts, const ic::Entry* __restrict__ ents,
                                                              const uint64_t* __restrict__ limits, const uint16_t* __restrict__ sym,
                                                              const uint8_t* __restrict__ win, uint64_t syms) {
    const uint64_t f0 = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * it::RESOLVE_RUN;
    if (f0 >= syms) return;
    ib::ib_resolve_run(sym, win, ents, parts, n_parts, limits, f0);
}

}  // namespace mi355

namespace {
static_assert(ib::PAR_DEFAULT == 65536 && ib::PAR_MIN == 1024 && ib::PAR_MAX == (1ull << 30), "the setting's default and range");
static_assert(sizeof(ib::Part) == 72 && sizeof(ib::Head) == 16, "what the kernels read and leave");
}  // namespace
