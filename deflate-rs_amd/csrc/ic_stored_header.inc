// ic_stored_header.inc -- the header of a stored piece: pad to the byte, LEN, NLEN.  TEXT of inflate_check.h, the one copy: the first
// lines of ic_stored_block, iw_stored_block and it_stored_block (text and not a call, for the reason given in ic_match_token.inc).
//   reads     b (Bits), p
//   declares  at (the piece's first bit behind the pad), len, byte0 (where its LEN bytes begin in the stream, all of them inside it)
//   a failure is returned at (at, p); behind the text the reader stands behind NLEN
    b.pos = (b.pos + 7) & ~7ull;  // (the pad bits are ignored, as zlib's inflate does)
    const uint64_t at = b.pos;
    const uint32_t len = ic_take(b, 16), nlen = ic_take(b, 16);
    if (b.over) return ic_fail(V_TRUNCATED, at, p);
    if ((len ^ nlen) != 0xFFFFu) return ic_fail(V_STORED, at, p);
    const uint64_t byte0 = b.pos >> 3;
    if (len > b.nbytes - byte0) return ic_fail(V_TRUNCATED, at, p);  // (byte0 <= nbytes: not over)
