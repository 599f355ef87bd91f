// Cuts of a seek handle (include/mi355_deflate.h MI355_CFG_INFLATE_SEEK_CUT_BYTES, mi355_inflate_seek_cuts): the kernels.  inflate_cut.h
// has the cut rule, the walk of one cut and the flatten step; tests/inflcut/ builds the same text for the host; the driver is
// deflate_seek_inflate.inc's.  Nothing waits inside a kernel:
//   k_inflate_tab_cut      build, in k_inflate_tab's place: one workgroup of one wave per entry stores the entry's symbols and
//                          records its cuts into the entry's slots (a prefix sum of the table: no counter is shared)
//   k_inflate_cut          read, pass 1 over cuts: one workgroup of one wave per cut, k_inflate_seek's shape
//   k_inflate_cut_flatten  read, between pass 1 and pass 2: one workgroup per entry walks the entry's cuts in order, rewrites the
//                          markers of every cut behind the first and folds the cuts' records into the entry's
// Build-side choice: the cuts are recorded by the pass that stores the symbols, not by a walker launch of its own -- a walker would
// run the scalar chain of every entry a second time, and that chain is what the build's time is made of.  DESIGN.md section 17.
#include "inflate_cut.h"

namespace mi355 {

// build, pass 1 with cuts.  slot0[k] .. slot0[k + 1]: the slots of the group's entry k; n_cut[k]: how many it filled
__global__ __launch_bounds__(64) void k_inflate_tab_cut(const TItem it, const ic::Entry* __restrict__ ents, ic::Rec* __restrict__ recs,
                                                        const uint64_t* __restrict__ slot0, icut::Cut* __restrict__ slots,
                                                        uint32_t* __restrict__ n_cut, uint64_t cut_bytes) {
    __shared__ ic::Tables s_t;
    const ic::Entry e = ents[blockIdx.x];
    const uint64_t a = slot0[blockIdx.x];
    const uint32_t n_slots = (uint32_t)(slot0[blockIdx.x + 1] - a);
    it::Sink o{it.sym, nullptr, it.base, e.pos, it.cap, e.pos};
    icut::Rec r;
    icut::ict_build_entry<TabSink, icut::Rules>(s_t, it.stream, it.stream_len, it.wrapper, o, e, it.total, cut_bytes, slots + a, n_slots, r);
    if (threadIdx.x == 0) {
        recs[blockIdx.x] = r;  // (the entry's record: ic::Rec's fields)
        n_cut[blockIdx.x] = r.n_cuts < n_slots ? r.n_cuts : n_slots;
    }
}

// read, pass 1: the cut's entry and part in hand
__global__ __launch_bounds__(64) void k_inflate_cut(const is::Part* __restrict__ parts, const ic::Entry* __restrict__ ents,
                                                    const icut::Item* __restrict__ items, uint16_t* sym, icut::Rec* __restrict__ crecs) {
    __shared__ ic::Tables s_t;
    const icut::Item ci = items[blockIdx.x];
    const ic::Entry e = ents[ci.ent];
    const is::Part pt = parts[e.item];
    icut::Rec r;
    icut::ict_decode_cut<TabSink, icut::Rules>(s_t, sym, pt, e, ci, r);
    if (threadIdx.x == 0) crecs[blockIdx.x] = r;
}

// read, flatten: the workgroup of the set's entry blockIdx.x.  Cut k's step loads symbols of the entry in front of the cut -- the
// cuts 0 .. k - 1, which this workgroup has rewritten -- and stores the cut's own: one barrier and a workgroup fence stand between
// two steps, and sym is read and written here.  Every thread folds the same records, so the loop's branches are the workgroup's.
__global__ __launch_bounds__(1024) void k_inflate_cut_flatten(const is::Part* __restrict__ parts, const ic::Entry* __restrict__ ents,
                                                              const icut::Item* __restrict__ items, const uint32_t* __restrict__ first,
                                                              const icut::Rec* __restrict__ crecs, uint16_t* sym, ic::Rec* __restrict__ recs) {
    const ic::Entry e = ents[blockIdx.x];
    const is::Part pt = parts[e.item];
    const uint32_t i0 = first[blockIdx.x], n = first[blockIdx.x + 1] - i0;
    uint16_t* psym = sym + pt.sym_off;
    ic::Rec acc{ic::V_OK, 0, 0, 0, 0, 0, e.bit, e.pos, 0};
    bool more = true;
    for (uint32_t k = 0; k < n && more; k++) {
        const uint64_t c_pos = items[i0 + k].c.pos;
        uint64_t upto = icut::ict_fold(acc, crecs + i0, items + i0, k, more);
        if (upto > pt.cap) upto = pt.cap;
        if (!k) continue;  // (the first cut is the entry's start: its markers are the entry's)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the fence's own wait, spelled out as in TabSink::fence: DESIGN.md section 12)
        __syncthreads();
        for (uint64_t q = c_pos + threadIdx.x; q < upto; q += 1024) psym[q - pt.base] = icut::ict_flat<icut::Rules>(psym, pt.base, e.pos, c_pos, q);
    }
    if (threadIdx.x == 0) recs[blockIdx.x] = acc;
}

}  // namespace mi355
