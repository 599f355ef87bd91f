// The body of k_gzip_frame (deflate_kernels.hip): the names sc, out, hdr, hdr_len, in_len, trailer are the kernel's; BX_ is the
// workgroup's index in the grid of the call (k_gzip_frame) or of the item (kb_gzip_tail, deflate_batch.inc).
    if (BX_) return;
    for (uint32_t i = threadIdx.x; i < hdr_len; i += blockDim.x) out[i] = hdr[i];
    if (threadIdx.x || !trailer) return;
    uint64_t nbytes = (sc->total_bits + 7) / 8;
    uint8_t* t = out + hdr_len + nbytes;
    uint32_t c = sc->crc;
    for (int k = 0; k < 4; k++) t[k] = (uint8_t)(c >> (8 * k));
    for (int k = 0; k < 4; k++) t[4 + k] = (uint8_t)(in_len >> (8 * k));
