// ic_match_token.inc -- a match token, from its length symbol to a checked (len, dist).  TEXT of inflate_check.h, the one copy:
// ic_huffman_block, iw_huffman_block and it_huffman_block include it inside their symbol loops, and ic_match_token wraps it as a
// function for the host test.  (Text and not a call, like emit_body.inc: as an inline function the same arithmetic compiled to other
// code in the five decode kernels and measured slower -- DESIGN.md section 12.)
//   reads     t (Tables), w (the bits from the token's first on), s (257..285), avail (bits of w inside the stream), at, p
//   updates   used: in, the bits of s's code; out, the bits of the whole token
//   declares  len, dist
//   a failure is reported at (at, p): it sets f and leaves the enclosing loop with `break`
        // a length: 257..264 = 3..10, then four codes per extra bit, 285 = 258
        const uint32_t lc = s - 257;
        uint32_t len = 3 + lc, eb = 0;
        if (lc == 28) {
            len = 258;
        } else if (lc >= 8) {
            eb = (lc >> 2) - 1;
            len = 3 + ((4 + (lc & 3)) << eb) + ((uint32_t)(w >> used) & ((1u << eb) - 1));
        }
        used += eb;
        uint32_t dused;
        const uint32_t ds = ic_decode<P>(t.prim_d, D_BITS, t.sym_d, 31, t.cnt_d, w >> used, dused);
        if (ds == NOCODE) {
            const uint64_t davail = used < avail ? avail - used : 0;
            f = ic_fail(davail < 15 && ic_longer_code_exists(t.cnt_d, davail) ? V_TRUNCATED : V_CODE, at, p);
            break;
        }
        if (ds >= 30) {
            f = ic_fail(used + dused > avail ? V_TRUNCATED : V_CODE, at, p);
            break;
        }
        used += dused;
        // a distance: 0..3 = 1..4, then two codes per extra bit
        uint32_t dist = 1 + ds, de = 0;
        if (ds >= 4) {
            de = (ds >> 1) - 1;
            dist = 1 + ((2 + (ds & 1)) << de) + ((uint32_t)(w >> used) & ((1u << de) - 1));
        }
        used += de;  // (15 + 5 + 15 + 13 = 48 bits at most: inside the 57 of ic_peek)
        if (used > avail) {
            f = ic_fail(V_TRUNCATED, at, p);
            break;
        }
        if (dist > 32768 || dist > p) {
            f = ic_fail(V_DISTANCE, at, p);
            break;
        }
