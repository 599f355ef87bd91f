// The body of k_adler_part, included by the kernel itself (BX_ = blockIdx.x) and by its batched form in deflate_batch.inc
// (BX_ = the workgroup's index inside its item).  One text, two places: as a function inlined into the kernel it came
// out with other registers (the callee is optimised before it is inlined, without the kernel's launch bounds).
    __shared__ uint32_t sa[4], sb[4];
    const uint32_t tid = threadIdx.x;
    const uint64_t c0 = (uint64_t)BX_ * ADLER_CHUNK;
    const uint32_t len = n - c0 < ADLER_CHUNK ? (uint32_t)(n - c0) : ADLER_CHUNK;
    const bool aligned = (reinterpret_cast<uintptr_t>(in) & 15) == 0;
    uint32_t a = 0, b = 0;
#pragma unroll
    for (uint32_t i = 0; i < ADLER_CHUNK / (256 * 16); i++) {
        const uint32_t o = (i * 256 + tid) * 16;
        if (o >= len) break;
        uint32_t v[4] = {0, 0, 0, 0};
        if (o + 16 <= len && aligned) {
            const uint4 q = *reinterpret_cast<const uint4*>(in + c0 + o);
            v[0] = q.x;
            v[1] = q.y;
            v[2] = q.z;
            v[3] = q.w;
        } else {
            for (uint32_t k = 0; k < 16; k++)
                if (o + k < len) v[k >> 2] |= (uint32_t)in[c0 + o + k] << (8 * (k & 3));
        }
        uint32_t s = 0, w = 0;
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) {
            const uint32_t d = (v[k >> 2] >> (8 * (k & 3))) & 0xff;  // (bytes past the end are 0)
            s += d;
            w += k * d;
        }
        a += s;
        b += (len - o) * s - w;  // <= 4 * 16384 * 4080 < 2^32
    }
    b %= 65521u;
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        a += __shfl_xor(a, off, 64);
        b += __shfl_xor(b, off, 64);
    }
    if ((tid & 63) == 0) {
        sa[tid >> 6] = a;
        sb[tid >> 6] = b;
    }
    __syncthreads();
    if (tid == 0) {
        const uint64_t A = ((uint64_t)sa[0] + sa[1] + sa[2] + sa[3]) % 65521u;
        const uint64_t B = ((uint64_t)sb[0] + sb[1] + sb[2] + sb[3]) % 65521u;
        const uint64_t after = (uint64_t)n - c0 - len;
        atomicAdd(reinterpret_cast<unsigned long long*>(&sc->adler_a), (unsigned long long)A);
        atomicAdd(reinterpret_cast<unsigned long long*>(&sc->adler_b), (unsigned long long)((B + (after % 65521u) * A) % 65521u));
    }
