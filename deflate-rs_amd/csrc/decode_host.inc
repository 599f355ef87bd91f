// What the host drivers of the decode side share (deflate_verify.inc, deflate_inflate.inc, deflate_table_inflate.inc,
// deflate_index_inflate.inc, deflate_members_inflate.inc with deflate_bigmembers_inflate.inc, deflate_seek_inflate.inc with
// deflate_cut_inflate.inc, deflate_bgzf_read.inc): the head of an entry -- the context, its device, the refusal of a context that is
// busy with a shard --, the stream of a call, the two halves of the staging of a host-buffer call, the descriptor room, the plan of
// a batch's checksum launches, the stage clocks, and the bookkeeping of a batch of items and of a batch of ranges.  The decode launch
// and the checksum half that the IItem drivers share are deflate_inflate.inc's (decode_half, sums_half, framed_tail).  Host code
// only: the kernels and what they decide are in those files and their headers.
namespace {

constexpr uint64_t VERIFY_MAX_IN = 0xFFFF0000ull;  // 4 GiB - 64 KiB: what one pass encodes, and what the checksum kernels take

// every decode entry asks this once, behind its argument checks and in front of its work
int shard_refusal(mi355_deflate_ctx* c) {
    if (!c->live_shard) return MI355_OK;
    c->err = "the context holds a sharded encode";
    return MI355_E_STATE;
}

// The head of a decode entry: the caller's context (a seek read: its handle's) or the default one, which dg keeps for the call; its
// device selected; shard_refusal.  An entry that refuses its arguments before a context exists calls this behind its checks;
// args_bad is for the one that looks at them with the context in hand (mi355_inflate), between the device and the shard.
int decode_enter(mi355_deflate_ctx*& c, DefaultGuard& dg, bool args_bad = false) {
    c = use_ctx(c, dg);
    if (!c) return MI355_E_HIP;
    HIPCHK(c, hipSetDevice(c->device));
    if (args_bad) return MI355_E_ARG;
    return shard_refusal(c);
}

// the caller's stream, or the context's own
hipStream_t call_stream(const mi355_deflate_ctx* c, void* hip_stream) { return hip_stream ? (hipStream_t)hip_stream : c->own_stream; }

// the device and the page-locked side of a call's descriptors and records
int verify_room(mi355_deflate_ctx* c, size_t bytes) {
    int rc = ensure_buf(c, &c->v_dev, &c->v_dev_cap, bytes);
    if (rc) return rc;
    if (bytes > c->v_host_cap) {
        if (c->v_host) (void)hipHostFree(c->v_host);
        c->v_host = nullptr;
        c->v_host_cap = 0;
        HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&c->v_host), bytes, 0));
        c->v_host_cap = bytes;
    }
    return MI355_OK;
}

// The staging of a call on host buffers, on the context's own stream, in two halves.  Stage-in: the caller's n bytes on their way
// into `to` with a plain asynchronous copy; nullptr: into the context's d_in, grown to hold them.
int stage_in(mi355_deflate_ctx* c, const uint8_t* src, size_t n, uint8_t* to = nullptr) {
    if (!to) {
        if (const int rc = ensure_buf(c, &c->d_in, &c->d_in_cap, n + 64)) return rc;
        to = c->d_in;
    }
    if (n) HIPCHK(c, hipMemcpyAsync(to, src, n, hipMemcpyHostToDevice, c->own_stream));
    return MI355_OK;
}
// a call that leaves without having waited on its stream waits here, before the caller may touch the buffer it staged in
void stage_settle(mi355_deflate_ctx* c) { (void)hipStreamSynchronize(c->own_stream); }  // (the copy of the caller's buffer may be in flight)
// Stage-out, with the worker's rc: a hard error -- anything but MI355_OK, MI355_E_DATA and MI355_E_OUT_TOO_SMALL, behind which the
// worker has waited -- settles; else the `valid` bytes of d_out that hold data come back with a plain copy.
int stage_out(mi355_deflate_ctx* c, int rc, uint8_t* out, uint64_t valid) {
    if (rc != MI355_OK && rc != MI355_E_DATA && rc != MI355_E_OUT_TOO_SMALL) {
        stage_settle(c);
        return rc;
    }
    if (valid) HIPCHK(c, hipMemcpy(out, c->d_out, (size_t)valid, hipMemcpyDeviceToHost));
    return rc;
}

// A call on host buffers around its device worker, behind decode_enter: room for the output, stage-in, the worker, stage-out.
// work(d_stream, d_out, st, &valid): MI355_OK, MI355_E_DATA or MI355_E_OUT_TOO_SMALL and the bytes of d_out that hold data; d_out
// is nullptr when the caller gave no room.
template <class Work>
int staged_call(mi355_deflate_ctx* c, const uint8_t* stream, size_t stream_len, uint8_t* out, size_t out_cap, Work work) {
    if (const int rc = ensure_buf(c, &c->d_out, &c->d_out_cap, out_cap + 64)) return rc;
    if (const int rc = stage_in(c, stream, stream_len)) return rc;
    uint64_t valid = 0;
    const int rc = work(c->d_in, out_cap ? c->d_out : nullptr, c->own_stream, &valid);
    return stage_out(c, rc, out, valid);
}

// Where a batched call keeps its checksum plan in the descriptor room, behind `front` bytes of its own descriptors and in front of
// its k records: [front] | [BatchItem k][running workgroup sums BS_N x (k + 1)] | [DevState k] | [record k]; without sums the three
// middle parts are empty.  The host side up to st_at is what goes to the device.
struct BatchSums {
    size_t k, bat_at, pre_at, st_at, rec_at, bytes;
    BatchSums(size_t front, size_t k_, bool sums, size_t rec_size) : k(k_) {
        bat_at = align_up(front, 256);
        pre_at = bat_at + (sums ? sizeof(BatchItem) * k : 0);
        st_at = align_up(pre_at + (sums ? sizeof(uint32_t) * BS_N * (k + 1) : 0), 256);
        rec_at = align_up(st_at + (sums ? sizeof(DevState) * k : 0), 256);
        bytes = rec_at + rec_size * k;
    }
    DevState* states(const mi355_deflate_ctx* c) const { return reinterpret_cast<DevState*>(c->v_dev + st_at); }

    // the host side of the plan: item(j, &bytes, &n) names the j-th run of bytes; the rows count the workgroups kb_adler_part and
    // kb_crc give each item.  The caller uploads it.
    template <class Item>
    int fill(mi355_deflate_ctx* c, Item item) const {
        BatchItem* hb = reinterpret_cast<BatchItem*>(c->v_host + bat_at);
        uint32_t* hpre = reinterpret_cast<uint32_t*>(c->v_host + pre_at);
        memset(c->v_host + bat_at, 0, st_at - bat_at);
        for (size_t j = 0; j < k; j++) {
            uint64_t n = 0;
            item(j, &hb[j].in, &n);
            hb[j].n = (uint32_t)n;
            hb[j].st = states(c) + j;
            const uint64_t wg[2] = {cdiv(n, ADLER_CHUNK), cdiv(n, 256 * CRC_CHUNK)};
            for (uint32_t s = 0; s < 2; s++) {
                const size_t row = (size_t)(s ? BS_CRC : BS_ADLER) * (k + 1);
                const uint64_t t = (uint64_t)hpre[row + j] + wg[s];
                if (t > 0x7fffffffull) return MI355_E_ARG;
                hpre[row + j + 1] = (uint32_t)t;
            }
        }
        return MI355_OK;
    }
    // behind the upload: the items' sums cleared, one flat launch over the row's total
    int launch(mi355_deflate_ctx* c, int wrapper, hipStream_t st) const {
        HIPCHK(c, hipMemsetAsync(states(c), 0, sizeof(DevState) * k, st));
        const BatchArgs a{reinterpret_cast<const BatchItem*>(c->v_dev + bat_at), reinterpret_cast<const uint32_t*>(c->v_dev + pre_at), (uint32_t)k};
        const uint32_t grid = reinterpret_cast<const uint32_t*>(c->v_host + pre_at)[(size_t)(wrapper == 1 ? BS_ADLER : BS_CRC) * (k + 1) + k];
        if (grid && wrapper == 1) hipLaunchKernelGGL(kb_adler_part, dim3(grid), dim3(256), 0, st, a);
        if (grid && wrapper == 2) hipLaunchKernelGGL(kb_crc, dim3(grid), dim3(256), 0, st, a);
        return MI355_OK;
    }
};

// HIP-event time between the launches of a call, only when asked (MI355_CFG_STAGE_CLOCKS): an event is idle queue between two
// kernels.  The events, their flag and the milliseconds are the context's: N slots of milliseconds, E events (N, unless the caller
// brackets every launch with the same pair and laps it into the launch kind's slot).
template <int N, int E = N>
struct StageClocks {
    hipEvent_t (&ev)[E];
    bool& ev_ok;
    float (&ms)[N];
    hipStream_t st;
    bool on;  // (the call's stage_clocks_on)
    // the slots cleared; the events made on first use, all of them or none: what was made before a failure is destroyed again
    int begin(mi355_deflate_ctx* c) {
        for (int k = 0; k < N; k++) ms[k] = 0;
        if (!on || ev_ok) return MI355_OK;
        hipEvent_t made[E];
        for (int k = 0; k < E; k++) {
            const hipError_t e = hipEventCreate(&made[k]);
            if (e == hipSuccess) continue;
            for (int j = 0; j < k; j++) (void)hipEventDestroy(made[j]);
            HIPCHK(c, e);
        }
        for (int k = 0; k < E; k++) ev[k] = made[k];
        ev_ok = true;
        return MI355_OK;
    }
    hipError_t mark(int k) const { return on ? hipEventRecord(ev[k], st) : hipSuccess; }
    // after a wait behind both marks
    void lap(int from, int to, int slot) const {
        float t = 0;
        if (on && hipEventElapsedTime(&t, ev[from], ev[to]) == hipSuccess) ms[slot] += t;
    }
};

// The head of a batch entry: the items that are not skipped (a status on entry: left alone) in `act`.  check(item): MI355_OK, or
// the entry's own refusal of an active item.  Argument errors, then the entry's refusals, then the context's state.
template <class Check>
int batch_active(mi355_deflate_ctx* c, const mi355_batch_item* items, size_t n_items, int wrapper, std::vector<uint32_t>& act, Check check) {
    if ((!items && n_items) || wrapper < 0 || wrapper > 2 || n_items > 0x7fffffffull) return MI355_E_ARG;
    for (size_t i = 0; i < n_items; i++) {
        if (items[i].status != MI355_OK) continue;  // skipped, left alone
        if (!items[i].in && items[i].in_len) return MI355_E_ARG;
        const int rc = check(items[i]);
        if (rc) return rc;
        act.push_back((uint32_t)i);
    }
    return shard_refusal(c);
}

// The tail of a batch entry: judge(j, item, report) turns the j-th record into the item's report and status (and what else the entry
// leaves in the item); every report gets the call's time; the first failure is the call's return code and, through say(report,
// status, what) with what = "<name>: item <index in the caller's array>", its text.
template <class Report, class Judge, class Say>
int batch_give(mi355_batch_item* items, const std::vector<uint32_t>& act, Report* reports, float ms, const char* name, Judge judge, Say say) {
    int first = MI355_OK;
    for (size_t j = 0; j < act.size(); j++) {
        Report r;
        const int s = judge(j, items[act[j]], r);
        r.ms = ms;
        if (reports) reports[act[j]] = r;
        items[act[j]].status = s;
        if (s != MI355_OK && first == MI355_OK) {
            first = s;
            char what[48];
            snprintf(what, sizeof what, "%s: item %u", name, act[j]);
            say(r, s, what);
        }
    }
    return first;
}

// The tail of a batch of ranges, which skips none: judge(i, report, &got) turns what the call knows of range i into its report, the
// bytes it got and its status; every report gets the call's time; the first failure is the call's return code and, through
// say(report, status, what) with what = "<name>: range <index in the caller's array>", its text.
template <class Judge, class Say>
int ranges_give(mi355_seek_range* r, size_t n, mi355_inflate_report* reports, float ms, const char* name, Judge judge, Say say) {
    int first = MI355_OK;
    for (size_t i = 0; i < n; i++) {
        mi355_inflate_report rep{};
        uint64_t got = 0;
        const int s = judge(i, rep, &got);
        rep.ms = ms;
        r[i].got = got, r[i].status = s, r[i].reserved = 0;
        if (reports) reports[i] = rep;
        if (s != MI355_OK && first == MI355_OK) {
            first = s;
            char what[48];
            snprintf(what, sizeof what, "%s: range %zu", name, i);
            say(rep, s, what);
        }
    }
    return first;
}

}  // namespace
