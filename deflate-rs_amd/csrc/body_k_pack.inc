// The body of k_pack, included by the kernel itself (BX_ = blockIdx.x) and by its batched form in deflate_batch.inc
// (BX_ = the workgroup's index inside its item).  One text, two places: as a function inlined into the kernel it came
// out with other registers (the callee is optimised before it is inlined, without the kernel's launch bounds).
    constexpr uint32_t PKW = PKT / 64;
    __shared__ PackLds<PKW> s;
    const uint32_t b = sc->nbcum[piece] + BX_ / PSPLIT, part = BX_ % PSPLIT, tid = threadIdx.x;
    if (b >= sc->nb || spec_failed(sc)) return;
    const uint32_t gtid = part * PKT + tid;  // a stored block's bytes are spread over all parts' threads
    constexpr uint32_t GT = PKT * PSPLIT;
    const BlockPlan pl = plan[b];
    const BlockHeader* h = hdr + b;
    uint64_t bp = pl.bit_start;
    if (pl.btype == BT_STORED) {
        // compress.rs:59-77, stored_block.rs:13-40
        uint64_t src = bstart[b];
        if (q13[b] && (compat & 1)) src += WINDOW_SIZE;  // bug-for-bug (A.4 Q13)
        uint64_t left = (uint64_t)bstart[b + 1] - bstart[b];
        do {
            uint64_t piece = left < (uint64_t)MAX_STORED_BLOCK_LENGTH ? left : (uint64_t)MAX_STORED_BLOCK_LENGTH;
            bool last_piece = piece == left;
            uint64_t hb = (bp + 3 + 7) & ~7ull;  // header bits then pad to a byte
            if (gtid == 0) {
                put_bits(out32, bp, (pl.bfinal && last_piece) ? 1u : 0u, 3);
                put_bits(out32, hb, (piece & 0xffff) | (((~piece) & 0xffff) << 16), 32);
            }
            uint64_t ob = (hb >> 3) + 4;  // first payload byte
            // The output words that lie wholly inside the payload belong to this piece alone: plain
            // 4-byte stores (the source is read byte-wise, it has no alignment to speak of).  The up
            // to three bytes before the first and after the last whole word share their words with
            // the header or with the next block: OR.
            const uint64_t w0 = (ob + 3) >> 2, w1 = (ob + piece) >> 2;  // whole words [w0, w1)
            if (w1 > w0) {
                for (uint64_t w = w0 + gtid; w < w1; w += GT) {
                    const uint64_t i = (w << 2) - ob;  // payload offset of the word's first byte
                    uint32_t v = 0;
#pragma unroll
                    for (int k = 0; k < 4; k++) v |= ((src + i + k < n) ? (uint32_t)in[src + i + k] : 0u) << (8 * k);
                    out32[w] = v;
                }
                const uint64_t headn = (w0 << 2) - ob, tail0 = (w1 << 2) - ob;
                for (uint64_t i = gtid; i < headn + (piece - tail0); i += GT) {
                    const uint64_t j = i < headn ? i : tail0 + (i - headn);
                    const uint64_t o = ob + j;
                    uint32_t v = (src + j < n) ? in[src + j] : 0u;
                    if (v) atomicOr(out32 + (o >> 2), v << (8 * (o & 3)));
                }
            } else {
                for (uint64_t i = gtid; i < piece; i += GT) {
                    uint64_t o = ob + i;
                    uint32_t v = (src + i < n) ? in[src + i] : 0u;
                    if (v) atomicOr(out32 + (o >> 2), v << (8 * (o & 3)));
                }
            }
            bp = (ob + piece) * 8;
            src += piece;
            left -= piece;
        } while (left > 0);
        return;
    }
    const uint32_t nt = tab.nt[b];
    if (part > 0 && part * PQ >= nt) return;  // (an empty block is part 0's)
    // code tables
    if (pl.btype == BT_FIXED) {
        for (uint32_t i = tid; i < 288; i += PKT) s.lll[i] = (uint8_t)fixed_ll_length(i);
        if (tid < 32) s.dl[tid] = 5;
    } else {
        for (uint32_t i = tid; i < 288; i += PKT) s.lll[i] = h->ll_len[i];
        if (tid < 32) s.dl[tid] = h->d_len[tid];
    }
    if (tid < 20) s.cll[tid] = (pl.btype == BT_DYNAMIC && tid < 19) ? h->cl_len[tid] : 0;
    if (tid < 48) s.cnt[tid] = 0;
    for (uint32_t i = tid; i < PKW * PACK_WORDS; i += PKT) (&s.wbuf[0][0])[i] = 0;
    __syncthreads();
    // Canonical codes (huffman_table.rs:253-278; stages.h canonical_codes is the serial form) for the three
    // tables at once: symbols per length by LDS atomics, first code of every length by one thread per table,
    // then symbol i takes the first code of its length plus the number of symbols before it with that length.
    for (uint32_t i = tid; i < 288; i += PKT)
        if (s.lll[i]) atomicAdd(&s.cnt[s.lll[i]], 1u);
    if (tid < 32 && s.dl[tid]) atomicAdd(&s.cnt[16 + s.dl[tid]], 1u);
    if (tid < 19 && s.cll[tid]) atomicAdd(&s.cnt[32 + s.cll[tid]], 1u);
    __syncthreads();
    if (tid < 3) {
        uint32_t* c = s.cnt + 16 * tid;
        uint32_t code = 0, before = 0;  // (no symbol is counted under length 0)
        for (uint32_t bits = 1; bits < 16; bits++) {
            code = ((code + before) << 1) & 0xffff;
            before = c[bits];
            c[bits] = code;
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < 288 + 32 + 20; i += PKT) {
        const uint8_t* len = i < 288 ? s.lll : (i < 320 ? s.dl : s.cll);
        uint16_t* codes = i < 288 ? s.llc : (i < 320 ? s.dc : s.clc);
        const uint32_t* first = s.cnt + (i < 288 ? 0 : (i < 320 ? 16 : 32));
        const uint32_t k = i < 288 ? i : (i < 320 ? i - 288 : i - 320);
        const uint32_t l = len[k];
        uint32_t r = 0;
        if (l) {
            // (the symbols before k with its length, four lengths a read: byte by byte this loop was up to 287 dependent LDS
            // reads a thread, a third of the kernel's table building; the three arrays are 4-byte aligned)
            const uint32_t* lw = reinterpret_cast<const uint32_t*>(len);
            const uint32_t pat = l * 0x01010101u, whole = k >> 2, rem = k & 3u;
#pragma unroll 4
            for (uint32_t w = 0; w < whole; w++) {
                const uint32_t z = lw[w] ^ pat;
                r += (uint32_t)__builtin_popcount(~(((z & 0x7f7f7f7fu) + 0x7f7f7f7fu) | z) & 0x80808080u);  // its zero bytes
            }
            if (rem) {
                const uint32_t z = lw[whole] ^ pat;
                r += (uint32_t)__builtin_popcount(~(((z & 0x7f7f7f7fu) + 0x7f7f7f7fu) | z) & 0x80808080u & ((1u << (8 * rem)) - 1u));
            }
        }
        codes[k] = l ? (uint16_t)reverse_bits16((first[l] + r) & 0xffff, l) : (uint16_t)0;
    }
    __syncthreads();
    // block header
    uint32_t hdr_bits = 3;
    if (part > 0) {
        // Where this part's bits begin: behind the header and the tokens of the parts before it, whose sizes
        // follow from their histograms (code length + extra bits per symbol).  A dynamic header is what is
        // left of dyn_bits (stages.h block_costs) after all the symbols.
        uint32_t pre = 0, all = 0;
        for (uint32_t i = tid; i < 320; i += PKT) {
            uint32_t len = 0;
            if (i < NUM_LL) len = s.lll[i] + (i >= 257 ? length_extra_bits_of_code(i - 257) : 0u);
            if (i >= 288 && i - 288 < NUM_DIST) len = s.dl[i - 288] + distance_extra_bits_of_code(i - 288);
            for (uint32_t k = 0; k < PSPLIT; k++) {
                const uint64_t slot = (uint64_t)b * PSPLIT + k;
                const uint32_t f = i < 288 ? ll_freq[slot * 288 + i] : d_freq[slot * 32 + (i - 288)];
                all += f * len;
                if (k < part) pre += f * len;
            }
        }
#pragma unroll
        for (int off = 32; off; off >>= 1) {
            pre += __shfl_xor(pre, off);
            all += __shfl_xor(all, off);
        }
        if ((tid & 63) == 0) {
            s.scan[tid >> 6] = pre;
            s.scan[PKW + (tid >> 6)] = all;
        }
        __syncthreads();
        pre = 0;
        all = 0;
        for (uint32_t k = 0; k < PKW; k++) {
            pre += s.scan[k];
            all += s.scan[PKW + k];
        }
        __syncthreads();
        hdr_bits = 3 + pre;
        if (pl.btype == BT_DYNAMIC) hdr_bits += (uint32_t)(h->dyn_bits - all - s.lll[END_OF_BLOCK]);
    } else if (pl.btype == BT_DYNAMIC) {
        // 3 + 14 bits, the code-length code lengths (huffman_lengths.rs:329-331), then the run-length
        // coded lengths (:338-368), one symbol per thread: bit strings, a scan of their lengths over
        // the workgroup, OR into the output.  (One lane walking the list would wait for two dependent
        // loads from the header in global memory per symbol.)
        const uint32_t used = h->used_hclens, n_enc = h->n_enc;
        if (tid == 0) {
            uint64_t p = bp;
            put_bits(out32, p, pl.bfinal ? 5u : 4u, 3);  // encoder_state.rs:12-13
            p += 3;
            put_bits(out32, p, (h->n_ll - 257) | ((h->n_d - 1) << 5) | ((used >= 4 ? used - 4 : 0) << 10), 14);
            p += 14;
            for (uint32_t i = 0; i < used; i++) {
                put_bits(out32, p, s.cll[hclen_order(i)], 3);
                p += 3;
            }
        }
        uint64_t hp = bp + 17 + 3ull * used;
        const uint32_t lane0 = tid & 63, wv0 = tid >> 6;
        for (uint32_t i0 = 0; i0 < n_enc; i0 += PKT) {
            const uint32_t i = i0 + tid;
            uint64_t bits = 0;
            uint32_t nb2 = 0;
            if (i < n_enc) {
                const uint32_t e = h->enc[i], kind = e >> 8, v = e & 0xff;
                const uint32_t sym = el_symbol_index(e);
                nb2 = s.cll[sym];
                bits = s.clc[sym];
                if (kind == 1) {
                    bits |= (uint64_t)(v - 3) << nb2;
                    nb2 += 2;
                } else if (kind == 2) {
                    bits |= (uint64_t)(v - 3) << nb2;
                    nb2 += 3;
                } else if (kind == 3) {
                    bits |= (uint64_t)(v - 11) << nb2;
                    nb2 += 7;
                }
            }
            uint32_t incl = nb2;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                uint32_t y = __shfl_up(incl, off);
                if (lane0 >= (uint32_t)off) incl += y;
            }
            if (lane0 == 63) s.scan[wv0] = incl;
            __syncthreads();
            uint32_t wbase = 0, total = 0;
#pragma unroll
            for (uint32_t k = 0; k < PKW; k++) {
                uint32_t y = s.scan[k];
                if (k < wv0) wbase += y;
                total += y;
            }
            put_bits(out32, hp + wbase + (incl - nb2), bits, nb2);
            hp += total;
            __syncthreads();
        }
        hdr_bits = (uint32_t)(hp - bp);
    } else if (tid == 0) {
        put_bits(out32, bp, pl.bfinal ? 3u : 2u, 3);  // encoder_state.rs:10-11
    }
    bp += hdr_bits;
    // tokens: 4 consecutive tokens per lane and round; lengths are scanned inside the wave with
    // shuffles and across the 4 waves through LDS (two barriers per 1024 tokens)
    const uint64_t t0 = (uint64_t)tab.t0[b] + (uint64_t)part * PQ;
    const uint64_t t1 = (uint64_t)tab.t0[b] + ((part + 1) * PQ < nt ? (part + 1) * PQ : nt);
    const uint32_t lane = tid & 63, wv = tid >> 6;
    // (a round's four tokens are fetched a round ahead, as one 16-byte load where all four exist: at the head of the round
    // they were a memory latency per round, between two barriers)
    auto fetch4 = [&](uint64_t tq, uint32_t* tk) {
        if (tq + 4 <= t1) {
            const uint4 v = *reinterpret_cast<const uint4*>(dtok + tq);  // (dword aligned is all a global load asks for)
            tk[0] = v.x;
            tk[1] = v.y;
            tk[2] = v.z;
            tk[3] = v.w;
        } else {
#pragma unroll
            for (int q = 0; q < 4; q++) tk[q] = tq + q < t1 ? dtok[tq + q] : 0u;
        }
    };
    uint32_t nxt[4];
    fetch4(t0 + 4ull * tid, nxt);
    uint32_t* const buf = &s.wbuf[0][0];
    bool first_shared = true;
    for (uint64_t tb = t0; tb < t1; tb += 4 * PKT) {
        uint64_t tq = tb + 4ull * tid;
        uint32_t nb4[4];
        uint64_t bits4[4];
        uint32_t mine = 0;
        const uint32_t cur[4] = {nxt[0], nxt[1], nxt[2], nxt[3]};
        if (tb + 4 * PKT < t1) fetch4(tq + 4 * PKT, nxt);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            nb4[q] = 0;
            bits4[q] = 0;
            if (tq + q < t1) bits4[q] = token_bits(cur[q], s.llc, s.lll, s.dc, s.dl, &nb4[q]);
            mine += nb4[q];
        }
        uint32_t incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            uint32_t v = __shfl_up(incl, off);
            if (lane >= (uint32_t)off) incl += v;
        }
        if (lane == 63) s.scan[wv] = incl;
        __syncthreads();
        uint32_t wbase = 0, total = 0;
#pragma unroll
        for (uint32_t k = 0; k < PKW; k++) {
            uint32_t v = s.scan[k];
            if (k < wv) wbase += v;
            total += v;
        }
        // The round's bits go into ONE buffer of the workgroup, word 0 = the output word the round begins in: the seams between
        // the four waves close in LDS, the round's whole words leave by plain stores, and the word it ends in stays behind as word 0
        // of the next round.  Only the first word of the part (shared with the header or the part before) and its last one
        // (behind the loop) are OR-ed into the output.  (Before: a buffer per wave, its first and last word OR-ed into the output
        // every round -- sixty-four atomics a part among the plain stores to the same lines: 101 -> 80 us without them.)
        const uint32_t rel0 = (uint32_t)(bp & 31);
        uint32_t rel = rel0 + wbase + (incl - mine);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            put_bits_lds(buf, rel, bits4[q], nb4[q]);
            rel += nb4[q];
        }
        __syncthreads();
        const uint64_t word0 = bp >> 5;
        const uint32_t endbit = rel0 + total, nfull = endbit >> 5;  // whole words of the round
        for (uint32_t w = tid; w < nfull; w += PKT) {
            const uint32_t v = buf[w];
            buf[w] = 0;
            if (w == 0 && first_shared) {
                if (v) atomicOr(out32 + word0, v);
            } else {
                out32[word0 + w] = v;
            }
        }
        if (tid == 0 && nfull) {  // (thread 0 has done word 0 above; nobody else touches word nfull)
            buf[0] = buf[nfull];
            buf[nfull] = 0;
        }
        if (nfull) first_shared = false;
        bp += total;
        // (the next round writes its sums behind this round's reads of them, and into the buffer behind its own first barrier)
    }
    if (tid == 0 && (bp & 31)) {  // the word the part ends in: the next part's, the next block's or the end-of-block code's as well
        const uint32_t v = buf[0];
        if (v) atomicOr(out32 + (bp >> 5), v);
    }
    if (tid == 0 && (part + 1) * PQ >= nt) put_bits(out32, bp, s.llc[END_OF_BLOCK], s.lll[END_OF_BLOCK]);  // encoder_state.rs:102-105
