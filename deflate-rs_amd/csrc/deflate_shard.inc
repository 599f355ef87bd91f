// deflate_shard.inc -- stream-exact (P1) sharding of ONE input over several GPUs: the per-rank
// phases between which the ranks exchange a 576-entry exit table, their token counts, at most
// 31743 straddling tokens and the per-block cost records (include/mi355_deflate.h, "sharded
// encode").  Orchestrated by deflate-rs_amd/shard.py over torch.distributed (RCCL / gloo).
struct mi355_shard {
    mi355_deflate_ctx* c = nullptr;
    hipStream_t st = nullptr;
    mi355_deflate_opts opts;
    ParseCfg cfg;
    const uint8_t* d_ext = nullptr;
    uint64_t n_ext = 0, lo = 0, hi = 0, global_lo = 0, n_global = 0;
    bool last_rank = false;
    Workspace w;
    SegEnds sg{nullptr, 1};
    std::vector<Level> lv;  // level tree over [lo, hi)
    uint64_t entry = 0, T_r = 0, skip = 0, T2 = 0;
    uint32_t nb2 = 0;
    uint64_t* d_cover = nullptr;  // carved from the tail of tokbuf-free space: separate small allocation
    uint32_t* d_lasttok = nullptr;
    ShardCost* d_costs = nullptr;
    size_t small_cap = 0;
    // pinned host staging for the per-block records that cross the bus every step (cost records and block starts back,
    // the plan over): from pageable memory a copy of this size makes the runtime pin and unpin the pages -- 1.5 ms in some runs
    ShardCost* h_costs = nullptr;
    uint32_t* h_bst = nullptr;
    BlockPlan* h_plan = nullptr;
    uint32_t q1 = 0;
    // the range parsed by speculation (k_emit<1>: every segment, the first one included, finds its entry by a run-up into the
    // history in front of the range): whether the chain of entries and exits inside the range checked out, where the range
    // was entered and left.  The driver compares every rank's exit with the next rank's entry: if the whole chain holds, the
    // tokens are there and no exit table was needed.
    bool spec_ok = false;
    uint64_t spec_entry = 0, spec_exit = 0;  // buffer coordinates
    bool steps_done = false;                 // w.adv holds the restart steps (k_adv / k_rle)
    bool tables_done = false;                // exit tables of the range (the exact way: made when somebody asks)
    bool from_flush = false;                 // the range begins at a sync-flush point of a stream (the parse enters AT parse_lo)
    // a range that begins at a sync-flush point of a stream (deflate_long.inc): the positions the write calls around the flush
    // left out of the chains or filed a byte late (stages.h HashOverride; buffer coordinates, ascending)
    std::vector<uint32_t> skew, holes;
    uint64_t quirk_end = 0;
    // ... and, for a flush point inside the first windows of the stream, what belongs to a stream's start: the flush points
    // that re-warm the hash (HashOverride::pts) and the Q1 re-warm an earlier call of the stream found (on / pos)
    std::vector<uint32_t> rewarm;
    bool q1_given = false;
    uint64_t q1_given_pos = 0;
    std::vector<uint32_t> h_bstart;  // block start positions (buffer coordinates), nb2 + 1 entries
};

void shard_destroy(mi355_shard* s) {
    if (!s) return;
    if (s->c) (void)hipSetDevice(s->c->device);
    if (s->d_cover) (void)hipFree(s->d_cover);
    if (s->d_lasttok) (void)hipFree(s->d_lasttok);
    if (s->d_costs) (void)hipFree(s->d_costs);
    if (s->h_costs) (void)hipHostFree(s->h_costs);
    if (s->h_bst) (void)hipHostFree(s->h_bst);
    if (s->h_plan) (void)hipHostFree(s->h_plan);
    delete s;
}

namespace {

int shard_ensure_small(mi355_shard* s, size_t nb) {
    if (nb + 2 <= s->small_cap) return MI355_OK;
    mi355_deflate_ctx* c = s->c;
    if (s->d_cover) (void)hipFree(s->d_cover);
    if (s->d_lasttok) (void)hipFree(s->d_lasttok);
    if (s->d_costs) (void)hipFree(s->d_costs);
    if (s->h_costs) (void)hipHostFree(s->h_costs);
    if (s->h_bst) (void)hipHostFree(s->h_bst);
    if (s->h_plan) (void)hipHostFree(s->h_plan);
    s->d_cover = nullptr;
    s->d_lasttok = nullptr;
    s->d_costs = nullptr;
    s->h_costs = nullptr;
    s->h_bst = nullptr;
    s->h_plan = nullptr;
    s->small_cap = 0;
    size_t cap = nb + 64;
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&s->d_cover), cap * sizeof(uint64_t)));
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&s->d_lasttok), cap * sizeof(uint32_t)));
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&s->d_costs), cap * sizeof(ShardCost)));
    HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&s->h_costs), cap * sizeof(ShardCost), hipHostMallocDefault));
    HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&s->h_bst), cap * sizeof(uint32_t), hipHostMallocDefault));
    HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&s->h_plan), cap * sizeof(BlockPlan), hipHostMallocDefault));
    s->small_cap = cap;
    return MI355_OK;
}

// links + match + adv over the whole buffer
int shard_tables(mi355_shard* s, const HashOverride& ov, bool redo_head = false) {
    mi355_deflate_ctx* c = s->c;
    hipStream_t st = s->st;
    Workspace& w = s->w;
    const ParseCfg& cfg = s->cfg;
    const uint64_t n = s->n_ext;
    const uint32_t n32 = (uint32_t)n;
    const bool hashing = cfg_hashing(cfg);
    s->tables_done = false;
    s->spec_ok = false;
    // (a range whose bytes are still arriving from the host on the copy stream: mi355_deflate_encode_multi; the second pass
    // after a re-warm finds everything there).  Every branch takes the arrival: the levels that do not hash read the
    // whole buffer at once, so they wait for its last piece (run_encode does the same for its non-hashing levels)
    const Arrival* arr = redo_head ? nullptr : c->next_arrival;
    c->next_arrival = nullptr;
    if (!hashing && arr && arr->n > 0) {
        const int rc = arrival_wait(c, st, *arr, arr->n - 1);
        if (rc) return rc;
    }
    if (hashing) {
        int rc = launch_match_tables(c, st, s->d_ext, n, w, cfg, ov, (ov.on | ov.m) != 0, s->sg, c->ev[0][1], redo_head, arr,
                                     s->quirk_end);
        if (rc) return rc;
        HIPCHK(c, hipEventRecord(c->ev[0][2], st));
    } else if (cfg.mode == MODE_RLE) {
        HIPCHK(c, hipEventRecord(c->ev[0][1], st));
        hipLaunchKernelGGL(k_rle, dim3(cdiv(n, RT)), dim3(256), 0, st, s->d_ext, n32, w.M, w.adv, s->sg);
        HIPCHK(c, hipEventRecord(c->ev[0][2], st));
    } else {
        HIPCHK(c, hipEventRecord(c->ev[0][1], st));
        HIPCHK(c, hipMemsetAsync(w.M, 0, (n + 64) * 4, st));
        HIPCHK(c, hipEventRecord(c->ev[0][2], st));
    }
    const uint32_t* Mq = cfg.use_quarter ? w.Mq : nullptr;
    // (k_rle has written the steps of that level; where k_emit works them out itself, k_adv waits for somebody to ask for the exit tables)
    s->steps_done = cfg.mode == MODE_RLE || !steps_in_emit(c, cfg, s->sg.m);
    if (cfg.mode != MODE_RLE && s->steps_done)
        hipLaunchKernelGGL(k_adv, dim3(cdiv(n, 1024)), dim3(256), 0, st, n32, w.M, Mq, cfg, w.adv, s->sg, 0u);
    // level tree over the parse range, in coordinates relative to lo
    const uint32_t nr = (uint32_t)(s->hi - s->lo);
    s->lv.clear();
    uint32_t cnt = cdiv(nr, SEG);
    uint64_t usize = SEG;
    for (size_t l = 0; cnt > 0; l++) {
        Level L = w.levels[l];  // arrays are large enough: cnt <= w.levels[l].count
        L.count = cnt;
        L.usize = usize;
        s->lv.push_back(L);
        if (cnt == 1) break;
        cnt = (cnt + FAN - 1) / FAN;
        usize *= FAN;
    }
    return MI355_OK;
}

// the exit tables of the range, level by level (the exact way to an entry; only made when the speculation did not hold)
int shard_exit_tables(mi355_shard* s) {
    if (s->tables_done) return MI355_OK;
    mi355_deflate_ctx* c = s->c;
    hipStream_t st = s->st;
    Workspace& w = s->w;
    const uint32_t nr = (uint32_t)(s->hi - s->lo);
    if (!s->steps_done) {
        hipLaunchKernelGGL(k_adv, dim3(cdiv(s->n_ext, 1024)), dim3(256), 0, st, (uint32_t)s->n_ext, w.M,
                           s->cfg.use_quarter ? w.Mq : nullptr, s->cfg, w.adv, s->sg, 0u);
        s->steps_done = true;
    }
    hipLaunchKernelGGL(k_seg_exit, dim3(cdiv(s->lv[0].count, 4)), dim3(256), 0, st, nr, s->lv[0].count, w.adv + s->lo,
                       s->lv[0].X, 0u);
    for (size_t l = 0; l + 1 < s->lv.size(); l++)
        hipLaunchKernelGGL(k_level_up, dim3(s->lv[l + 1].count), dim3(ZONE), 0, st, nr,
                           s->lv[l].count, s->lv[l].usize, s->lv[l].X, s->lv[l + 1].count, s->lv[l + 1].X);
    HIPCHK(c, hipGetLastError());
    s->tables_done = true;
    return MI355_OK;
}

// The segments of the range as the parse helpers see them: positions relative to lo, the exits where k_scan_b writes next.
SegRange shard_range(const mi355_shard* s) {
    const Workspace& w = s->w;
    // (the first segment has the range's history in front of it, unless the range begins the stream)
    const uint32_t runup0 = s->lo >= SPEC_W ? 1u : 0u;
    return SegRange{s->lv[0].count, Piece{0u, 0u, 1u}, s->d_ext, (uint32_t)(s->hi - s->lo), (uint32_t)s->lo, (uint32_t)s->n_ext, runup0, s->sg,
                    s->steps_done ? w.adv : nullptr, s->lv[0].E, w.base, w.fixlist, &s->c->d_sc->n_fix[0], w.scan_part, nullptr, nullptr};
}

// The range parsed by speculation: tokens, their count, entry and exit -- and whether the chain inside the range held.
int shard_spec(mi355_shard* s) {
    mi355_deflate_ctx* c = s->c;
    hipStream_t st = s->st;
    Workspace& w = s->w;
    const uint32_t K = s->lv[0].count;
    s->spec_ok = false;
    if (K == 0) return MI355_OK;
    HIPCHK(c, hipMemsetAsync(c->d_sc, 0, sizeof(DevScalars), st));
    const SegRange r = shard_range(s);
    launch_spec_entries(c, st, w, s->cfg, r);
    // (entry of the first segment and exit of the last one travel with the scalars; the exits lie where k_scan_b writes next)
    DevState* const dst = reinterpret_cast<DevState*>(c->d_sc);
    HIPCHK(c, hipMemcpyAsync(&dst->pad[0], s->lv[0].E, sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    HIPCHK(c, hipMemcpyAsync(&dst->pad[1], w.base + (K - 1), sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    launch_token_scan(c, st, w, r, false);
    HIPCHK(c, hipMemcpyAsync(c->h_sc, c->d_sc, sizeof(DevState), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    DevState* h = reinterpret_cast<DevState*>(c->h_sc);
    if (h->spec_bad) {  // (periodic data: this range is parsed the exact way; the flag is the context's, put it back)
        HIPCHK(c, hipMemsetAsync(&reinterpret_cast<DevState*>(c->d_sc)->spec_bad, 0, sizeof(uint32_t), st));
        HIPCHK(c, hipStreamSynchronize(st));
        h->spec_bad = 0;
        return MI355_OK;
    }
    s->spec_ok = true;
    s->spec_entry = s->lo + h->pad[0];
    s->spec_exit = s->lo + h->pad[1];
    s->entry = s->spec_entry;
    s->T_r = c->h_sc->T;
    return MI355_OK;
}

// tokens of the path positions in [entry, hi)
int shard_emit(mi355_shard* s, uint64_t entry) {
    mi355_deflate_ctx* c = s->c;
    hipStream_t st = s->st;
    Workspace& w = s->w;
    if (s->spec_ok && entry == s->spec_entry) return MI355_OK;  // (the speculation entered the range right there: the tokens are there)
    s->spec_ok = false;
    {
        int rc = shard_exit_tables(s);
        if (rc) return rc;
    }
    const uint32_t nr = (uint32_t)(s->hi - s->lo);
    uint32_t e_rel = (uint32_t)(entry - s->lo);
    HIPCHK(c, hipMemcpyAsync(s->lv.back().E, &e_rel, sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipStreamSynchronize(st));  // e_rel is a stack variable
    for (size_t l = s->lv.size() - 1; l-- > 0;)
        hipLaunchKernelGGL(k_level_down, dim3(cdiv(s->lv[l + 1].count, 64)), dim3(64), 0, st, nr, s->lv[l].count,
                           s->lv[l].usize, s->lv[l].X, s->lv[l + 1].count, s->lv[l + 1].E, s->lv[l].E);
    const uint32_t* Mq = s->cfg.use_quarter ? w.Mq : nullptr;
    const uint32_t K = s->lv[0].count;
    HIPCHK(c, hipMemsetAsync(c->d_sc, 0, sizeof(DevScalars), st));
    hipLaunchKernelGGL((k_emit<0, false>), dim3(cdiv(K, 4)), dim3(256), 0, st, s->d_ext, nr, K, w.M, Mq, s->cfg, w.adv, s->lv[0].E,
                       w.tokbuf, w.cnt, (uint32_t)s->lo, (uint32_t)s->n_ext, s->sg, (uint32_t*)nullptr, SpecFix{nullptr, nullptr, nullptr}, 0u, 0u);
    launch_token_scan(c, st, w, shard_range(s), true);  // (K > 0: a range is not empty, shard_begin_at)
    HIPCHK(c, hipMemcpyAsync(c->h_sc, c->d_sc, sizeof(DevScalars), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    s->entry = entry;
    s->T_r = c->h_sc->T;
    return MI355_OK;
}

// the device work of mi355_shard_begin; any failure is cleaned up by the caller
int shard_begin_body(mi355_shard* s, const void* d_ext) {
    mi355_deflate_ctx* c = s->c;
    const ParseCfg& cfg = s->cfg;
    const uint64_t n_ext = s->n_ext, parse_lo = s->lo, global_lo = s->global_lo, n_global = s->n_global;
    const size_t n_quirks = s->skew.size() + s->holes.size() + s->rewarm.size();
    Workspace sz = carve(nullptr, n_ext, cfg.use_quarter, 1, 0, n_quirks);
    int rc = ensure_ws(c, sz.bytes);
    if (rc) return rc;
    s->w = carve(c->ws, n_ext, cfg.use_quarter, 1, 0, n_quirks);
    {   // one segment: the whole buffer (a rank never sees a sync flush)
        // (a fill of one word on the shard's stream: no trip over the bus, no wait for the device's other streams)
        HIPCHK(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(s->w.seg_ends), (int)(uint32_t)n_ext, 1, s->st));
        s->sg = SegEnds{s->w.seg_ends, 1};
    }
    HashOverride ov = NO_HASH_OVERRIDE;
    s->quirk_end = 0;
    if (n_quirks && cfg_hashing(cfg)) {
        const size_t ns = s->skew.size(), nh = s->holes.size();
        if (ns) HIPCHK(c, hipMemcpyAsync(s->w.quirks, s->skew.data(), ns * sizeof(uint32_t), hipMemcpyHostToDevice, s->st));
        if (nh) HIPCHK(c, hipMemcpyAsync(s->w.quirks + ns, s->holes.data(), nh * sizeof(uint32_t), hipMemcpyHostToDevice, s->st));
        HIPCHK(c, hipStreamSynchronize(s->st));
        ov.ns = (uint32_t)ns;
        ov.skw = s->w.quirks;
        ov.nh = (uint32_t)nh;
        ov.hol = s->w.quirks + ns;
        s->quirk_end = quirk_reach(&s->skew, &s->holes);
    }
    if ((!s->rewarm.empty() || s->q1_given) && cfg_hashing(cfg) && n_ext >= 2) {
        // (run_encode does the same for a stream's flush calls: the re-warmed hashes take the stream's first two bytes)
        const size_t at = s->skew.size() + s->holes.size(), nr = s->rewarm.size();
        uint8_t b01[2];
        if (nr) HIPCHK(c, hipMemcpyAsync(s->w.quirks + at, s->rewarm.data(), nr * sizeof(uint32_t), hipMemcpyHostToDevice, s->st));
        HIPCHK(c, hipMemcpyAsync(b01, d_ext, 2, hipMemcpyDeviceToHost, s->st));
        HIPCHK(c, hipStreamSynchronize(s->st));
        ov.m = (uint32_t)nr;
        ov.pts = nr ? s->w.quirks + at : nullptr;
        ov.b0 = b01[0];
        ov.b1 = b01[1];
        if (s->q1_given) {
            ov.on = 1;
            ov.pos = s->q1_given_pos;
            s->q1 = 1;
        }
    }
    rc = shard_tables(s, ov);
    if (!rc) {  // (k_match3's check of the sorted arrays: deflate_host.inc sort_order_failed)
        HIPCHK(c, hipMemcpyAsync(&reinterpret_cast<DevState*>(c->h_sc)->sort_bad, sort_bad_flag(c), sizeof(uint32_t), hipMemcpyDeviceToHost, s->st));
        HIPCHK(c, hipStreamSynchronize(s->st));
        if (sort_order_failed(c)) rc = shard_tables(s, ov);
    }
    if (!rc) rc = shard_spec(s);
    // quirk Q1 (lz77.rs:628-638) lives in the first window of the whole input: the rank that owns
    // position 0 looks at its block 0 before anybody uses its exit table.  (A range that begins at a flush point inside the
    // first window does the same with the block that begins there -- only one block of a stream can fill inside the first
    // window, and if it lay before the flush point the stream's flush call has found it: q1_given.)
    const bool hashing = cfg_hashing(cfg);
    if (!rc && global_lo == 0 && (parse_lo == 0 || (s->from_flush && parse_lo < WINDOW_SIZE)) && !s->q1_given && hashing &&
        n_ext >= MAX_BUFFER_LENGTH) {
        rc = shard_emit(s, parse_lo);  // (nothing to do if the speculation held and entered the range right there)
        if (!rc && s->T_r >= MAX_BUFFER_LENGTH) {
            uint32_t t = 0;
            HIPCHK(c, hipMemcpy(&t, s->w.dtok + (MAX_BUFFER_LENGTH - 1), 4, hipMemcpyDeviceToHost));
            // start of that token = sum of the covers before it: one k_cover launch over the head
            rc = shard_ensure_small(s, 4);
            if (!rc) {
                hipLaunchKernelGGL(k_cover, dim3(1), dim3(256), 0, s->st, s->w.dtok, (uint64_t)(MAX_BUFFER_LENGTH - 1),
                                   (uint64_t)0, 0u, s->d_cover, s->d_lasttok);
                uint64_t tp = 0;
                HIPCHK(c, hipMemcpyAsync(&tp, s->d_cover, 8, hipMemcpyDeviceToHost, s->st));
                HIPCHK(c, hipStreamSynchronize(s->st));
                uint64_t wpos = 0;
                if (q1_rewarm(t, tp + parse_lo, cfg.mode, n_global, &wpos)) {
                    uint8_t b01[2];
                    HIPCHK(c, hipMemcpy(b01, d_ext, 2, hipMemcpyDeviceToHost));
                    ov.on = 1;
                    ov.pos = wpos;
                    ov.b0 = b01[0];
                    ov.b1 = b01[1];
                    s->q1 = 1;
                    rc = shard_tables(s, ov, true);
                    if (!rc) rc = shard_spec(s);
                }
            }
        }
    }
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(s->st));
    HIPCHK(c, hipGetLastError());
    {   // what mi355_deflate_last_info reports for a sharded encode: the dominant kernel's launch time
        memset(&c->info, 0, sizeof c->info);
        c->pend_passes = 0;
        c->info.in_len = n_ext;
        c->info.q1_rewarm = s->q1;
        c->info.passes = 1 + s->q1;
        float ms = 0;
        if (hipEventElapsedTime(&ms, c->ev[0][1], c->ev[0][2]) == hipSuccess) {
            c->info.match_ms = ms;
            c->info.match_launches = 1;
            c->info.stage_ms[MI355_STAGE_MATCH] = ms;
        }
    }
    return MI355_OK;
}

}  // namespace

// what a range that begins at a sync-flush point of a stream inherits from the write calls before it (deflate_long.inc)
struct ShardQuirks {
    const std::vector<uint32_t>* skew = nullptr;    // buffer positions, ascending (stages.h HashOverride::skw)
    const std::vector<uint32_t>* holes = nullptr;   // HashOverride::hol
    const std::vector<uint32_t>* rewarm = nullptr;  // HashOverride::pts (a buffer that begins the stream only)
    bool q1_on = false;                             // HashOverride::on / pos, found by a flush call of the stream
    uint64_t q1_pos = 0;
};
static int shard_begin_at(mi355_deflate_ctx* c, const void* d_ext, size_t n_ext, size_t parse_lo, size_t parse_hi,
                          uint64_t global_lo, uint64_t n_global, const mi355_deflate_opts* o, void* hip_stream,
                          mi355_shard** out, const ShardQuirks* quirks);

extern "C" {

int mi355_shard_begin(mi355_deflate_ctx* c, const void* d_ext, size_t n_ext, size_t parse_lo, size_t parse_hi,
                      uint64_t global_lo, uint64_t n_global, const mi355_deflate_opts* o, void* hip_stream,
                      mi355_shard** out) {
    if ((parse_lo % SEG) != 0) return MI355_E_ARG;
    return shard_begin_at(c, d_ext, n_ext, parse_lo, parse_hi, global_lo, n_global, o, hip_stream, out, nullptr);
}

}  // extern "C"

// (parse_lo need not be a multiple of anything: deflate_long.inc begins a range at a stream's sync-flush point, with the
// lists of positions the write calls around the flush filed differently)
static int shard_begin_at(mi355_deflate_ctx* c, const void* d_ext, size_t n_ext, size_t parse_lo, size_t parse_hi,
                          uint64_t global_lo, uint64_t n_global, const mi355_deflate_opts* o, void* hip_stream,
                          mi355_shard** out, const ShardQuirks* quirks) {
    if (!c || !out || !o || !d_ext || parse_lo >= parse_hi || parse_hi > n_ext) return MI355_E_ARG;
    if (n_ext >= 0xFFFF0000ull) return MI355_E_UNSUPPORTED;
    if ((global_lo % WINDOW_SIZE) != 0) return MI355_E_ARG;  // window geometry must line up
    if (o->wrapper != 0 || o->flush != 0) return MI355_E_UNSUPPORTED;
    ParseCfg cfg;
    if (const int rc = parse_cfg(c, o, &cfg)) return rc;
    if (c->live_shard) {
        c->err = "this context already holds a sharded encode between mi355_shard_begin and mi355_shard_end";
        return MI355_E_STATE;
    }
    HIPCHK(c, hipSetDevice(c->device));
    // one shard object per context, kept (with its small device arrays) between encodes: a step of the
    // sharded encode allocates nothing
    mi355_shard* s = c->shard_cache ? c->shard_cache : new mi355_shard();
    c->shard_cache = nullptr;
    s->lv.clear();
    s->h_bstart.clear();
    s->entry = s->T_r = s->skip = s->T2 = 0;
    s->nb2 = 0;
    s->q1 = 0;
    s->skew.clear();
    s->holes.clear();
    s->rewarm.clear();
    s->q1_given = false;
    s->q1_given_pos = 0;
    s->from_flush = quirks != nullptr;
    if (quirks) {
        if (quirks->skew) s->skew = *quirks->skew;
        if (quirks->holes) s->holes = *quirks->holes;
        if (quirks->rewarm && global_lo == 0) s->rewarm = *quirks->rewarm;
        s->q1_given = quirks->q1_on && global_lo == 0;
        s->q1_given_pos = quirks->q1_pos;
    }
    s->c = c;
    s->st = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : c->own_stream;
    s->opts = *o;
    s->cfg = cfg;
    s->d_ext = reinterpret_cast<const uint8_t*>(d_ext);
    s->n_ext = n_ext;
    s->lo = parse_lo;
    s->hi = parse_hi;
    s->global_lo = global_lo;
    s->n_global = n_global;
    s->last_rank = global_lo + parse_hi >= n_global;
    int rc = shard_begin_body(s, d_ext);
    if (rc) {
        mi355_shard_end(s);  // every failure path gives the object (and its device arrays) back
        return rc;
    }
    c->live_shard = s;
    *out = s;
    return MI355_OK;
}

extern "C" {

int mi355_shard_exit_table(mi355_shard* s, uint32_t* table576) {
    if (!s || !table576) return MI355_E_ARG;
    mi355_deflate_ctx* c = s->c;
    HIPCHK(c, hipSetDevice(c->device));
    {
        int rc = shard_exit_tables(s);
        if (rc) return rc;
    }
    uint16_t t16[ZONE];
    HIPCHK(c, hipMemcpy(t16, s->lv.back().X, ZONE * sizeof(uint16_t), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < ZONE; i++) table576[i] = t16[i];
    return MI355_OK;
}

int mi355_shard_spec(mi355_shard* s, int* held, uint64_t* entry, uint64_t* exit_pos) {
    if (!s || !held || !entry || !exit_pos) return MI355_E_ARG;
    *held = s->spec_ok ? 1 : 0;
    *entry = s->spec_ok ? s->spec_entry : 0;
    *exit_pos = s->spec_ok ? s->spec_exit : 0;
    return MI355_OK;
}

int mi355_shard_emit(mi355_shard* s, uint64_t entry, uint64_t* n_tokens, const void** d_tokens) {
    if (!s || !n_tokens || entry < s->lo) return MI355_E_ARG;
    HIPCHK(s->c, hipSetDevice(s->c->device));
    if (entry >= s->hi) {  // the path jumps over this rank's whole range: it owns no token
        s->entry = entry;
        s->T_r = 0;
    } else {
        int rc = shard_emit(s, entry);
        if (rc) return rc;
    }
    *n_tokens = s->T_r;
    if (d_tokens) *d_tokens = s->w.dtok;
    return MI355_OK;
}

int mi355_shard_blocks(mi355_shard* s, uint64_t skip_tokens, const void* d_tail_tokens, uint64_t n_tail,
                       uint64_t* n_blocks, mi355_block_cost* costs, size_t costs_cap) {
    if (!s) return MI355_E_ARG;
    return mi355_shard_blocks_ex(s, skip_tokens, d_tail_tokens, n_tail, s->last_rank ? 1 : 0, n_blocks, costs, costs_cap);
}

int mi355_shard_blocks_ex(mi355_shard* s, uint64_t skip_tokens, const void* d_tail_tokens, uint64_t n_tail,
                          int owns_final, uint64_t* n_blocks, mi355_block_cost* costs, size_t costs_cap) {
    if (!s || !n_blocks || skip_tokens > s->T_r || (n_tail && !d_tail_tokens)) return MI355_E_ARG;
    mi355_deflate_ctx* c = s->c;
    hipStream_t st = s->st;
    Workspace& w = s->w;
    HIPCHK(c, hipSetDevice(c->device));
    if (s->T_r + n_tail + 64 > s->n_ext + 64) return MI355_E_ARG;
    if (n_tail)
        HIPCHK(c, hipMemcpyAsync(w.dtok + s->T_r, d_tail_tokens, n_tail * 4, hipMemcpyDeviceToDevice, st));
    s->skip = skip_tokens;
    s->T2 = s->T_r - skip_tokens + n_tail;
    if (owns_final) {
        s->nb2 = (uint32_t)(s->T2 / MAX_BUFFER_LENGTH + 1);
    } else {
        if (s->T2 % MAX_BUFFER_LENGTH) {
            c->err = "a rank that does not own the last block must own whole 31744-token blocks";
            return MI355_E_ARG;
        }
        s->nb2 = (uint32_t)(s->T2 / MAX_BUFFER_LENGTH);
    }
    *n_blocks = s->nb2;
    if (s->nb2 > w.nb_max + 1) return MI355_E_ARG;
    int rc = shard_ensure_small(s, s->nb2);
    if (rc) return rc;
    if (s->nb2 == 0) return MI355_OK;
    DevScalars hs;
    memset(&hs, 0, sizeof hs);
    hs.T = (uint32_t)s->T2;
    hs.nb = s->nb2;
    *c->h_sc = hs;
    HIPCHK(c, hipMemcpyAsync(c->d_sc, c->h_sc, sizeof(DevScalars), hipMemcpyHostToDevice, st));
    const uint32_t* tok = w.dtok + s->skip;
    hipLaunchKernelGGL(k_cover, dim3(s->nb2 + 1), dim3(256), 0, st, w.dtok, s->skip, s->T2, s->nb2, s->d_cover,
                       s->d_lasttok);
    hipLaunchKernelGGL(k_shard_bounds, dim3(1), dim3(64), 0, st, s->entry, s->d_cover, s->d_lasttok, s->nb2, s->T2,
                       s->cfg.mode, s->global_lo, s->n_global, w.bstart, w.q13);
    hipLaunchKernelGGL(k_block_table_uniform, dim3(cdiv(s->nb2, 256)), dim3(256), 0, st, s->T2, s->nb2, w.tab);
    MI355_LAUNCH_HIST(s->nb2 * PSPLIT, c->n_cu, st, tok, c->d_sc, w.ll_freq, w.d_freq, w.tab, 0u,
                       (uint32_t*)nullptr, 0u);
    hipLaunchKernelGGL(k_block_header, dim3(s->nb2), dim3(128), 0, st, c->d_sc, w.ll_freq, w.d_freq, w.hdr, 0u);
    hipLaunchKernelGGL(k_shard_costs, dim3(cdiv(s->nb2, 256)), dim3(256), 0, st, w.hdr, w.bstart, w.q13, s->nb2,
                       s->d_costs);
    const ShardCost* hc = s->h_costs;
    HIPCHK(c, hipMemcpyAsync(s->h_costs, s->d_costs, sizeof(ShardCost) * s->nb2, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(s->h_bst, w.bstart, 4 * (s->nb2 + 1), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    s->h_bstart.assign(s->h_bst, s->h_bst + s->nb2 + 1);
    for (size_t b = 0; b < s->nb2 && b < costs_cap; b++) {
        costs[b].dyn_bits = hc[b].dyn_bits;
        costs[b].dyn_est = hc[b].dyn_est;
        costs[b].static_est = hc[b].static_est;
        costs[b].fixed_bits = hc[b].fixed_bits;
        costs[b].in_bytes = hc[b].in_bytes;
        costs[b].q13 = hc[b].q13;
        costs[b].reserved = 0;
    }
    return MI355_OK;
}

// The serial step, run identically by every rank over the costs of ALL blocks of the stream
// (compress.rs:157-246, huffman_lengths.rs:269-286).
int mi355_plan_blocks(const mi355_block_cost* costs, size_t n, uint32_t compat, mi355_block_info* plans,
                      uint64_t* total_bits) {
    if ((!costs || !plans) && n) return MI355_E_ARG;
    uint64_t bitpos = 0;
    for (size_t b = 0; b < n; b++) {
        BlockPlan p;
        plan_block(costs[b].dyn_bits, costs[b].dyn_est, costs[b].static_est, costs[b].fixed_bits, costs[b].in_bytes,
                   b + 1 == n, bitpos, &p);
        if (p.btype == BT_STORED && costs[b].q13 == 2 && (compat & MI355_COMPAT_Q13)) return MI355_E_REF_PANIC;
        plans[b].btype = p.btype;
        plans[b].bfinal = p.bfinal;
        plans[b].n_tokens = 0;
        plans[b].reserved = 0;
        plans[b].in_bytes = costs[b].in_bytes;
        plans[b].bit_start = p.bit_start;
        bitpos += p.bit_len;
    }
    if (total_bits) *total_bits = bitpos;
    return MI355_OK;
}

// Pack this rank's blocks.  plans[i].bit_start are global bit offsets; the rank's bytes start at
// byte *first_byte (a multiple of 4) of the stream and *n_bytes of them are valid; the first and the
// last byte may be shared with the neighbours and must be OR-ed when the stream is stitched.
int mi355_shard_pack(mi355_shard* s, const mi355_block_info* plans, uint64_t end_bit, void* d_out, size_t out_cap,
                     uint64_t* first_byte, size_t* n_bytes) {
    if (!s || !first_byte || !n_bytes || (!plans && s->nb2) || !d_out) return MI355_E_ARG;
    mi355_deflate_ctx* c = s->c;
    hipStream_t st = s->st;
    Workspace& w = s->w;
    HIPCHK(c, hipSetDevice(c->device));
    *n_bytes = 0;
    *first_byte = 0;
    if (s->nb2 == 0) return MI355_OK;
    const uint64_t base_bit = plans[0].bit_start / 32 * 32;
    const uint64_t nbytes = (end_bit - base_bit + 7) / 8;
    if (nbytes + 8 > out_cap) {
        *n_bytes = (size_t)nbytes + 8;
        return MI355_E_OUT_TOO_SMALL;
    }
    BlockPlan* const hp = s->h_plan;  // (free again: every call of this function ends in a wait for the stream)
    for (uint32_t b = 0; b < s->nb2; b++) {
        // only a Stored block needs its raw bytes; those of a straddling block lie in the look-ahead -- a window further on where
        // the reference's bytes are asked for (A.4 Q13: body_k_pack.inc reads them there; the flags are those mi355_shard_blocks_ex
        // left in h_costs)
        const uint64_t ahead = (s->h_costs[b].q13 && (s->opts.compat & MI355_COMPAT_Q13)) ? WINDOW_SIZE : 0;
        if (plans[b].btype == BT_STORED && (uint64_t)s->h_bstart[b + 1] + ahead > s->n_ext) {
            c->err = "a stored block of this rank reaches past the look-ahead it was given";
            return MI355_E_ARG;
        }
        hp[b].btype = plans[b].btype;
        hp[b].bfinal = plans[b].bfinal;
        hp[b].bit_start = plans[b].bit_start - base_bit;
        hp[b].bit_len = 0;
    }
    HIPCHK(c, hipMemcpyAsync(w.plan, hp, sizeof(BlockPlan) * s->nb2, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(d_out, 0, align_up(nbytes + 8, 4), st));
    MI355_LAUNCH_PACK(s->nb2 * PSPLIT, c->n_cu, st, s->d_ext, (uint32_t)s->n_ext, w.dtok + s->skip, c->d_sc,
                       w.hdr, w.plan, w.bstart, w.q13, (uint32_t)s->opts.compat, reinterpret_cast<uint32_t*>(d_out), w.tab,
                       w.ll_freq, w.d_freq, 0u);
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    *first_byte = base_bit / 8;
    *n_bytes = (size_t)nbytes;
    return MI355_OK;
}

void mi355_shard_end(mi355_shard* s) {
    if (!s) return;
    mi355_deflate_ctx* c = s->c;
    if (c && c->live_shard == s) c->live_shard = nullptr;
    if (c && !c->shard_cache) {  // back to the context, device arrays and all
        c->shard_cache = s;
        return;
    }
    shard_destroy(s);
}

// zlib's adler32_combine / crc32_combine: the checksum of A || B from those of A and B and |B| -- what the
// driver of a sharded zlib / gzip encode folds the ranks' checksums with (kind 1 = Adler-32, 2 = CRC-32)
uint32_t mi355_checksum_combine(int kind, uint32_t sum_a, uint32_t sum_b, uint64_t len_b) {
    return kind == 2 ? crc_combine(sum_a, sum_b, len_b) : adler_combine(sum_a, sum_b, len_b);
}

}  // extern "C"
