// The body of k_crc_part (deflate_kernels.hip) up to a thread's CRC: the names in, n are the kernel's; BX_ is the workgroup's
// index in the grid of the call (k_crc_part) or of the item (kb_crc, deflate_batch.inc).  It leaves tid, mylen (the bytes of this
// thread's chunk) and crc (the chunk's CRC-32 register, before the final complement).
    __shared__ uint32_t T[4][256];
    __shared__ uint32_t stage[256 * 33];
    const uint32_t tid = threadIdx.x;
    {
        uint32_t c = tid;
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1u) ? CRC_POLY : 0u);
        T[0][tid] = c;
    }
    __syncthreads();
    for (int t = 1; t < 4; t++) {
        uint32_t v = T[t - 1][tid];
        T[t][tid] = (v >> 8) ^ T[0][v & 0xff];
        __syncthreads();
    }
    const uint64_t tile = (uint64_t)(BX_) * 256 * CRC_CHUNK;
    const uint64_t my0 = tile + (uint64_t)tid * CRC_CHUNK;
    const uint32_t mylen = my0 >= n ? 0u : (n - my0 < CRC_CHUNK ? (uint32_t)(n - my0) : CRC_CHUNK);
    const bool aligned = (reinterpret_cast<uintptr_t>(in) & 15) == 0;
    uint32_t crc = 0xFFFFFFFFu;
    for (uint32_t piece = 0; piece < CRC_CHUNK / CRC_PIECE; piece++) {
        // stage: lane j of round r loads 16 bytes of chunk (r * 32 + j / 8), part j % 8
        for (uint32_t r = 0; r < 8; r++) {
            const uint32_t c = r * 32 + tid / 8, part16 = tid % 8;
            const uint64_t g = tile + (uint64_t)c * CRC_CHUNK + piece * CRC_PIECE + part16 * 16;
            uint32_t v[4] = {0, 0, 0, 0};
            if (g + 16 <= n && aligned) {
                const uint4 q = *reinterpret_cast<const uint4*>(in + g);
                v[0] = q.x;
                v[1] = q.y;
                v[2] = q.z;
                v[3] = q.w;
            } else {
                for (uint32_t b = 0; b < 16; b++)
                    if (g + b < n) v[b >> 2] |= (uint32_t)in[g + b] << (8 * (b & 3));
            }
            uint32_t* dst = stage + c * 33 + part16 * 4;
            dst[0] = v[0];
            dst[1] = v[1];
            dst[2] = v[2];
            dst[3] = v[3];
        }
        __syncthreads();
        const uint32_t done = piece * CRC_PIECE;
        const uint32_t here = mylen > done ? (mylen - done < CRC_PIECE ? mylen - done : CRC_PIECE) : 0u;
        const uint32_t* src = stage + tid * 33;
        uint32_t w = 0;
        for (; w * 4 + 4 <= here; w++) {
            crc ^= src[w];
            crc = T[3][crc & 0xff] ^ T[2][(crc >> 8) & 0xff] ^ T[1][(crc >> 16) & 0xff] ^ T[0][crc >> 24];
        }
        for (uint32_t b = w * 4; b < here; b++) {
            const uint32_t d = (src[b >> 2] >> (8 * (b & 3))) & 0xff;
            crc = T[0][(crc ^ d) & 0xff] ^ (crc >> 8);
        }
        __syncthreads();
    }
