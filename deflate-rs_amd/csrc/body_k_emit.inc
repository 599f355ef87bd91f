// The body of k_emit, included by the kernel itself (BX_ = blockIdx.x) and by its batched form in deflate_batch.inc
// (BX_ = the workgroup's index inside its item).  One text, two places: as a function inlined into the kernel it came
// out with other registers (the callee is optimised before it is inlined, without the kernel's launch bounds).
    constexpr uint32_t ROW = EmitRows<MODE, STEPS>::ROW;
    __shared__ __attribute__((aligned(8))) uint16_t s_adv[4][ROW];
    __shared__ __attribute__((aligned(8))) uint16_t s_pp[4][ROW];
    __shared__ uint32_t s_np[4], s_exit[4];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint64_t k = (uint64_t)BX_ * 4 + wv + seg0;  // (seg0: a launch may cover a range of segments)
    uint32_t given = 0;  // MODE 2: the entry the segment is parsed from
    if (MODE == 2) {
        const uint32_t nf = *fix.n;
        if (nf > FIX_MAX || k >= nf) return;
        // (the exit of the segment before it as k_spec_check saw it -- not Xs[k - 1] as it is now, which a wave that repairs the
        // segments before this one may be rewriting: what a repair is based on must not depend on which wave runs first)
        given = fix.list[2 * k + 1];
        k = fix.list[2 * k];
    }
    if (k >= K) return;  // whole wave; no workgroup barrier is used below
    constexpr bool SPEC = MODE == 1;
    constexpr uint32_t REG = EmitRows<MODE, STEPS>::REG;
    uint16_t* A = s_adv[wv];
    uint16_t* P = s_pp[wv];
#define EMIT_NP s_np[wv]
#define EMIT_EXIT s_exit[wv]
#define EMIT_BADMAP fix.badmap
#include "emit_body.inc"
#undef EMIT_NP
#undef EMIT_EXIT
#undef EMIT_BADMAP
