// it_window_walk.inc -- pass 2 over ONE chain of entries: the window behind each from the window in front of it and the entry's symbols,
// and the position up to which pass 3 may write.  TEXT of inflate_table.h, the one copy: k_inflate_tab_window, k_inflate_mtab_window and
// k_inflate_seek_window include it behind their own load of window 0, and it_window_walk wraps it as a function for the host builds
// of tests/.  (Text and not a call, like ic_match_token.inc: DESIGN.md sections 12 and 13.)
//   reads     wk (it::Walk): the chain's symbols, entries and records, n, base, cap; s_w[2]: two windows of WIN bytes, s_w[0] the
//             window in front of entry 0, filled and visible to every caller
//   supplied  by wk: the slot of the window behind entry k (win, slot wk.slot0 + k + 1), whether the last entry is stepped at all beyond
//             start < cap (wk.last_made; the others always are) and whether its window goes to its slot (where that is wk.last_slot;
//             the others' always do).  A window that is made and not stored is still made: a step's cost does not depend on its slot.
//             by wp: the caller's share of a window's 8192 words -- word wp.word(i) for i < wp.turns -- and wp.step_done(k), which
//             returns once every caller's words of the step are written: the workgroup's barrier
//   declares  limit: the end of the last good entry, or the first failing entry's out_pos (it_limit states the rule on its own); and,
//             left in the includer's scope without a meaning behind the walk: cur, status, in_pos, end_pos, start
    uint32_t cur = 0;
    uint64_t limit = wk.base;
    // what a step needs of its entry -- status, out_pos, end, start: the same in every caller, so the branches below are the
    // workgroup's -- is loaded a step ahead, off the chain
    uint32_t status = wk.n ? wk.recs[0].status : 0;
    uint64_t in_pos = wk.n ? wk.recs[0].in_pos : 0, end_pos = wk.n ? wk.recs[0].end_pos : 0, start = wk.n ? wk.ents[0].pos : 0;
    for (uint32_t k = 0; k < wk.n; k++) {
        const uint32_t kn = k + 1 < wk.n ? k + 1 : k;
        const uint32_t status_n = wk.recs[kn].status;
        const uint64_t in_pos_n = wk.recs[kn].in_pos, end_pos_n = wk.recs[kn].end_pos, start_n = wk.ents[kn].pos;
        if (status) {
            limit = in_pos;
            break;
        }
        limit = end_pos;
        if ((k + 1 < wk.n || wk.last_made) && start < wk.cap) {  // (beyond cap it and everything behind it only counted)
            const uint64_t len = end_pos - start;
            const uint8_t* prev = s_w[cur];
            uint8_t* next = s_w[cur ^ 1];
            const bool kept = k + 1 < wk.n || wk.slot0 + wk.n == wk.last_slot;
            uint8_t* slot = wk.win + (uint64_t)(wk.slot0 + k + 1) * it::WIN;
            for (uint32_t i = 0; i < wp.turns; i++) {
                const uint32_t j = wp.word(i);
                uint32_t v = 0;
                for (uint32_t b = 0; b < 4; b++) v |= (uint32_t)it::it_window_byte(wk.sym, wk.base, start, len, wk.cap, prev, j + b) << (8 * b);
                *reinterpret_cast<uint32_t*>(next + j) = v;
                if (kept) *reinterpret_cast<uint32_t*>(slot + j) = v;
            }
            wp.step_done(k);  // (once a step: the window written in this step is not written again before the step after next)
            cur ^= 1;
        }
        status = status_n, in_pos = in_pos_n, end_pos = end_pos_n, start = start_n;
    }
