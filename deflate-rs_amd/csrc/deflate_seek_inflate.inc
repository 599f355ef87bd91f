// Seek points (include/mi355_deflate.h mi355_inflate_seek_*): a handle that keeps the table of ONE large stream and the resolved 32 KiB
// window in front of some of its entries, and byte ranges decoded from the nearest of them.  inflate_seek.h has the point rule, the
// range plan and the passes' rules; tests/inflseek/ builds the same text for the host.  Nothing waits inside a kernel:
//   k_seek_keep             build, behind a group's window pass: one workgroup per kept point copies the window in front of its entry
//                           from the group's workspace into the handle's store
//   k_inflate_seek          pass 1, one workgroup of one wave per (range, entry): k_inflate_mtab's shape, the entry's part in hand
//   k_inflate_seek_window   pass 2, one workgroup per part: the window of its point from the store (or zeros), then
//                           the window walk (it_window_walk.inc) over the part's entries
//   k_inflate_seek_resolve  pass 3, flat over the set's symbols -- the only kernel that writes `out`, and only [lo, min(limit, cap))
// The build is the tabled inflate's passes 1 and 2 (k_inflate_tab, k_inflate_tab_window) group by group without an output buffer; a
// framed stream's groups are resolved into a scratch region for the checksum launches.  The host driver's shared steps are in
// decode_host.inc: the entries' head (a read takes its context from the handle), the stage-in of a host build into the buffer the
// handle keeps, the stage-out of a host read, and the tail of a batch of ranges.  DESIGN.md section 16.
// With MI355_CFG_INFLATE_SEEK_CUT_BYTES set at the build, the handle also keeps CUTS inside its entries (inflate_cut.h; the kernels are
// deflate_cut_inflate.inc's): the build's pass 1 is k_inflate_tab_cut, and a read's pass 1 is k_inflate_cut over cuts with
// k_inflate_cut_flatten behind it -- four launches a set -- in front of the same passes 2 and 3.  DESIGN.md section 17.
#include <memory>

#include "inflate_seek.h"

namespace mi355 {

struct KeepItem {
    uint32_t slot, index;  // the group's window slot, the store's window
};

// build: window `slot` of the group's workspace is the window in front of a point: into the store, 16 bytes a lane a step
__global__ __launch_bounds__(256) void k_seek_keep(const KeepItem* __restrict__ keep, const uint8_t* __restrict__ win, uint8_t* __restrict__ store) {
    const KeepItem k = keep[blockIdx.x];
    const uint4* src = reinterpret_cast<const uint4*>(win + (uint64_t)k.slot * it::WIN);
    uint4* dst = reinterpret_cast<uint4*>(store + (uint64_t)k.index * it::WIN);
    for (uint32_t i = 0; i < it::WIN / 16 / 256; i++) dst[threadIdx.x + 256 * i] = src[threadIdx.x + 256 * i];
}

// pass 1
__global__ __launch_bounds__(64) void k_inflate_seek(const is::Part* __restrict__ parts, const ic::Entry* __restrict__ ents, uint16_t* sym,
                                                     ic::Rec* __restrict__ recs) {
    __shared__ ic::Tables s_t;
    const ic::Entry e = ents[blockIdx.x];
    const is::Part pt = parts[e.item];
    ic::Rec r;
    is::is_decode_entry<TabSink>(s_t, sym, pt, e, r);
    if (threadIdx.x == 0) recs[blockIdx.x] = r;
}

// pass 2: the workgroup of part blockIdx.x loads the window in front of its point -- kept by the build, or zeros in front of the
// stream --, leaves it in the part's slot 0 for pass 3, and walks the part's entries in order (it_window_walk.inc), two windows in LDS.
// Slot k + 1 gets the window behind entry k when the part has an entry k + 1 to read it.  It stops at the part's first failing entry and
// leaves the position up to which pass 3 may write.
__global__ __launch_bounds__(1024) void k_inflate_seek_window(const is::Part* __restrict__ parts, const ic::Entry* __restrict__ ents,
                                                              const ic::Rec* __restrict__ recs, const uint16_t* __restrict__ sym,
                                                              const uint8_t* __restrict__ store, uint8_t* win, uint64_t* __restrict__ limits) {
    __shared__ __attribute__((aligned(16))) uint8_t s_w[2][it::WIN];
    const is::Part pt = parts[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    {
        const bool zeros = pt.wslot == is::WSLOT_ZEROS;
        const uint4* src = reinterpret_cast<const uint4*>(store + (zeros ? 0ull : (uint64_t)pt.wslot * it::WIN));
        uint4* slot = reinterpret_cast<uint4*>(win + (uint64_t)pt.w0 * it::WIN);
        for (uint32_t i = 0; i < it::WIN / 16 / 1024; i++) {
            const uint32_t j = tid + 1024 * i;
            const uint4 v = zeros ? make_uint4(0, 0, 0, 0) : src[j];
            *reinterpret_cast<uint4*>(&s_w[0][16 * j]) = v;
            slot[j] = v;
        }
    }
    __syncthreads();
    // (the window behind the part's last entry is nobody's: it is not made)
    const it::Walk wk{sym + pt.sym_off, ents + pt.e0, recs + pt.e0, pt.n, pt.base, pt.cap, win, pt.w0, pt.w0 + pt.n, false};
    const WgWalk wp{tid};
#include "it_window_walk.inc"
    if (tid == 0) limits[blockIdx.x] = limit;
}

// pass 3: flat over the set's symbol elements, 16 a thread
__global__ __launch_bounds__(256) void k_inflate_seek_resolve(const is::Part* __restrict__ parts, uint32_t n_parts, const ic::Entry* __restrict__ ents,
                                                              const uint64_t* __restrict__ limits, const uint16_t* __restrict__ sym,
                                                              const uint8_t* __restrict__ win, uint64_t syms) {
    const uint64_t f0 = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * it::RESOLVE_RUN;
    if (f0 >= syms) return;
    is::is_resolve_set<is::Rules>(sym, win, ents, parts, n_parts, limits, f0);
}

}  // namespace mi355

#include "deflate_cut_inflate.inc"

// what a seek handle owns: the table on the host, the windows of its points on the device, and -- the host form -- the stream
struct mi355_inflate_seek {
    mi355_deflate_ctx* c = nullptr;
    std::vector<ic::Entry> ents;
    std::vector<uint32_t> pts;
    uint64_t total = 0, spacing = 0, stream_len = 0;
    uint32_t wrapper = 0;
    uint8_t* store = nullptr;   // pts.size() - 1 windows
    size_t store_bytes = 0;
    uint8_t* d_stream = nullptr;  // mi355_inflate_seek_build: the handle's own copy
    is::Counts last{0, 0, 0, 0};
    // cuts (inflate_cut.h): entry g's are cuts[cut0[g], cut0[g + 1]); none when the handle was built with the key at 0
    uint64_t cut_bytes = 0, cut_span = 0;  // (cut_span: the output bytes of the largest cut)
    std::vector<icut::Cut> cuts;
    std::vector<uint64_t> cut0;
    icut::Counts last_cuts{0, 0, 0, 0};
};

namespace {

static_assert(sizeof(is::Part) == 88 && sizeof(KeepItem) == 8, "what the kernels read");
static_assert(sizeof(icut::Cut) == 24 && sizeof(mi355_seek_cut) == 24 && sizeof(icut::Item) == 56 && sizeof(icut::Rec) == 72, "the cuts' records");
static_assert(icut::CUT_MIN == 64 && icut::CUT_MAX == (1ull << 30), "the range of MI355_CFG_INFLATE_SEEK_CUT_BYTES");
static_assert(sizeof(mi355_seek_info) == 56 && sizeof(mi355_seek_point) == 16 && sizeof(mi355_seek_range) == 40, "the seek calls' records");
static_assert(is::SPACING_DEFAULT == (1ull << 20) && is::SPACING_MIN == 32768 && is::SPACING_MAX == (1ull << 30), "the spacing's default and range");

// the device room of a build's cuts, freed when the build leaves
struct CutRoom {
    uint8_t* p = nullptr;
    ~CutRoom() {
        if (p) (void)hipFree(p);
    }
};

void seek_release(mi355_inflate_seek* h) {
    if (!h) return;
    if (h->store) (void)hipFree(h->store);
    if (h->d_stream) (void)hipFree(h->d_stream);
    delete h;
}

// what is wrong with a build's arguments, or nullptr: decided before a context or the device is touched (the tabled calls' rule)
const char* seek_build_args(const void* stream, size_t stream_len, int wrapper, const mi355_block_info* blocks, size_t n_blocks, uint64_t spacing,
                            mi355_inflate_seek* const* seek, const mi355_inflate_report* report, uint64_t* total) {
    uint64_t sp;
    size_t len = 0;
    if (!seek) return "inflate seek: bad argument";
    if (!is::is_spacing(spacing, sp)) return "inflate seek: the spacing is 0 or 32 KiB to 1 GiB";
    *total = 0;
    if (!blocks || !n_blocks) return inflate_args_bad(stream, stream_len, wrapper, nullptr, 0, &len, report) ? "inflate seek: bad argument" : nullptr;
    return tabled_args(stream, stream_len, wrapper, blocks, n_blocks, nullptr, 0, &len, report, total);
}

// The build, device resident stream (the entry has checked the arguments and asked shard_refusal): the table, then the tabled decode
// group by group with cap = total, the points' windows kept.  MI355_OK: *out is the handle.
int seek_build_one(mi355_deflate_ctx* c, const uint8_t* d_stream, size_t stream_len, int wrapper, const mi355_block_info* blocks, size_t n_blocks,
                   uint64_t total, uint64_t spacing, mi355_inflate_seek** out, mi355_inflate_report* report, hipStream_t st) {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<mi355_block_info> table;
    if (!blocks || !n_blocks) {
        iw::Rec found;
        if (const int rc = index_run(c, d_stream, stream_len, wrapper, st, table, found)) return rc;
        if (table.empty()) table.push_back(mi355_block_info{0u, 0u, 0u, 0u, 0ull, 0ull});  // (the decode reports what is wrong at bit 0)
        total = 0;
        for (const mi355_block_info& b : table) total += b.in_bytes;
        blocks = table.data(), n_blocks = table.size();
    }
    std::unique_ptr<mi355_inflate_seek, void (*)(mi355_inflate_seek*)> h(new mi355_inflate_seek, seek_release);
    h->c = c, h->total = total, h->stream_len = stream_len, h->wrapper = (uint32_t)wrapper;
    (void)is::is_spacing(spacing, h->spacing);
    h->ents.resize(n_blocks);
    ic::ic_make_entries([&](uint64_t k) { return blocks[k].bit_start; }, [&](uint64_t k) { return blocks[k].in_bytes; }, n_blocks, 0u, h->ents.data());
    is::is_points<is::Rules>(h->ents.data(), n_blocks, h->spacing, h->pts);
    h->store_bytes = (h->pts.size() - 1) * (size_t)it::WIN;
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&h->store), h->store_bytes ? h->store_bytes : (size_t)it::WIN));  // (never a null store)
    const std::vector<ic::Entry>& ents = h->ents;
    // the groups, the tabled driver's; a framed group is resolved into `scratch` behind its symbols
    const auto group = [&](uint64_t k0, uint64_t& k1, uint64_t& base, uint64_t& stored) {
        k1 = it::it_group_end([&](uint64_t k) { return blocks[k].in_bytes; }, n_blocks, k0, c->inflate_group_bytes);
        base = ents[k0].pos;
        stored = (k1 < n_blocks ? ents[k1].pos : total) - base;
    };
    // with cuts: a group's slots -- [slot0 n + 1] [n_cut n] [Cut slots] in a room of the build's own -- are a prefix sum of the table
    const uint64_t cb = c->seek_cut_bytes;
    h->cut_bytes = cb;
    const auto slots_of = [&](uint64_t k0, uint64_t k1) {
        uint64_t sum = 0;
        for (uint64_t k = k0; k < k1; k++) sum += icut::ict_slots(blocks[k].in_bytes, cb);
        return sum;
    };
    uint64_t slots_max = 0;
    size_t ws = 0, n_max = 0;
    for (uint64_t k0 = 0, k1, base, stored; k0 < n_blocks; k0 = k1) {
        group(k0, k1, base, stored);
        if (cb) {
            const uint64_t sl = slots_of(k0, k1);
            if (sl > 0xffffffffull) {
                c->err = "inflate seek: a group has more cuts than a launch takes";
                return MI355_E_UNSUPPORTED;
            }
            slots_max = sl > slots_max ? sl : slots_max;
        }
        if (wrapper && stored > VERIFY_MAX_IN) {
            c->err = "inflate seek: a group of a framed stream is larger than the checksum kernels take";
            return MI355_E_UNSUPPORTED;
        }
        const size_t need = (size_t)(k1 - k0 + 1) * it::WIN + align_up(2 * (size_t)stored, 256) + (wrapper ? (size_t)stored : 0) + 256;
        ws = need > ws ? need : ws;
        n_max = k1 - k0 > n_max ? k1 - k0 : n_max;
    }
    int rc = ensure_buf(c, &c->t_dev, &c->t_dev_cap, ws);
    if (rc) return rc;
    // descriptors: [Entry n] | [limit] [Rec n] | [Part] | [KeepItem n]
    const size_t lim_at = align_up(sizeof(ic::Entry) * n_max, 256), rec_at = lim_at + 256;
    const size_t part_at = align_up(rec_at + sizeof(ic::Rec) * n_max, 256), keep_at = part_at + 256;
    rc = verify_room(c, align_up(keep_at + sizeof(KeepItem) * n_max, 256) + 512);
    if (rc) return rc;
    CutRoom room;
    const size_t ncut_at = align_up(sizeof(uint64_t) * (n_max + 1), 256), slot_at = align_up(ncut_at + sizeof(uint32_t) * n_max, 256);
    std::vector<uint8_t> cut_host;
    if (cb) {
        HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&room.p), slot_at + sizeof(icut::Cut) * slots_max + 256));
        cut_host.resize(slot_at + sizeof(icut::Cut) * slots_max);
        h->cut0.assign(1, 0);
    }
    iw::Rec acc = iw::Rec{ic::V_OK, 0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t adler = 1, crc = 0;
    size_t next_pt = 1;  // (point 0 has no window to keep)
    bool first = true;
    for (uint64_t k0 = 0, k1, base, stored; k0 < n_blocks; k0 = k1) {
        group(k0, k1, base, stored);
        const uint32_t n = (uint32_t)(k1 - k0);
        const size_t sym_at = (size_t)(n + 1) * it::WIN, out_at = sym_at + align_up(2 * (size_t)stored, 256);
        uint8_t* scratch = c->t_dev + out_at;
        memcpy(c->v_host, ents.data() + k0, sizeof(ic::Entry) * n);
        *reinterpret_cast<is::Part*>(c->v_host + part_at) =
            is::Part{d_stream, stream_len, scratch, base, base + stored, total, base, 0, 0u, n, 0u, is::WSLOT_ZEROS, (uint32_t)wrapper, 0u};
        KeepItem* keep = reinterpret_cast<KeepItem*>(c->v_host + keep_at);
        uint32_t n_keep = 0;
        for (; next_pt < h->pts.size() && h->pts[next_pt] < k1; next_pt++)
            keep[n_keep++] = KeepItem{(uint32_t)(h->pts[next_pt] - k0), (uint32_t)(next_pt - 1)};
        const TItem item{d_stream, stream_len, reinterpret_cast<uint16_t*>(c->t_dev + sym_at), c->t_dev, base, total, total, (uint32_t)wrapper, n};
        const ic::Entry* d_ents = reinterpret_cast<const ic::Entry*>(c->v_dev);
        uint64_t* d_lim = reinterpret_cast<uint64_t*>(c->v_dev + lim_at);
        ic::Rec* d_recs = reinterpret_cast<ic::Rec*>(c->v_dev + rec_at);
        HIPCHK(c, hipMemcpyAsync(c->v_dev, c->v_host, sizeof(ic::Entry) * n, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(c->v_dev + part_at, c->v_host + part_at, keep_at + sizeof(KeepItem) * n_keep - part_at, hipMemcpyHostToDevice, st));
        if (first) HIPCHK(c, hipMemsetAsync(c->t_dev, 0, it::WIN, st));  // (nothing refers to the window in front of the stream)
        first = false;
        uint64_t n_slots = 0;
        if (cb) {
            uint64_t* slot0 = reinterpret_cast<uint64_t*>(cut_host.data());
            for (uint32_t k = 0; k < n; k++) slot0[k] = n_slots, n_slots += icut::ict_slots(blocks[k0 + k].in_bytes, cb);
            slot0[n] = n_slots;
            HIPCHK(c, hipMemcpyAsync(room.p, slot0, sizeof(uint64_t) * (n + 1), hipMemcpyHostToDevice, st));
            TItem walk = item;
            if (c->seek_cut_walker) {  // (the alternative the bench measures: pass 1 as without cuts, then a walk that stores no symbol)
                hipLaunchKernelGGL(k_inflate_tab, dim3(n), dim3(64), 0, st, item, d_ents, d_recs);
                HIPCHK(c, hipGetLastError());
                walk.cap = walk.base;
            }
            hipLaunchKernelGGL(k_inflate_tab_cut, dim3(n), dim3(64), 0, st, walk, d_ents, d_recs, reinterpret_cast<const uint64_t*>(room.p),
                               reinterpret_cast<icut::Cut*>(room.p + slot_at), reinterpret_cast<uint32_t*>(room.p + ncut_at), cb);
        } else {
            hipLaunchKernelGGL(k_inflate_tab, dim3(n), dim3(64), 0, st, item, d_ents, d_recs);
        }
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(k_inflate_tab_window, dim3(1), dim3(1024), 0, st, item, d_ents, d_recs, d_lim);
        HIPCHK(c, hipGetLastError());
        if (n_keep) {
            hipLaunchKernelGGL(k_seek_keep, dim3(n_keep), dim3(256), 0, st, reinterpret_cast<const KeepItem*>(c->v_dev + keep_at), c->t_dev, h->store);
            HIPCHK(c, hipGetLastError());
        }
        if (wrapper && stored) {
            hipLaunchKernelGGL(k_inflate_seek_resolve, dim3(cdiv(stored, 256 * it::RESOLVE_RUN)), dim3(256), 0, st,
                               reinterpret_cast<const is::Part*>(c->v_dev + part_at), 1u, d_ents, d_lim, item.sym, c->t_dev, it::it_align(stored));
            HIPCHK(c, hipGetLastError());
            // (a group that holds a failure: the sums of what lies in the scratch region are never used)
            rc = launch_sums_one(c, st, wrapper, scratch, stored);
            if (rc) return rc;
            HIPCHK(c, hipMemcpyAsync(c->h_sc, c->d_sc, sizeof(DevScalars), hipMemcpyDeviceToHost, st));
        }
        // the group's last window stays on the device as the window in front of the next group
        if (k1 < n_blocks) HIPCHK(c, hipMemcpyAsync(c->t_dev, c->t_dev + (size_t)n * it::WIN, it::WIN, hipMemcpyDeviceToDevice, st));
        HIPCHK(c, hipMemcpyAsync(c->v_host + rec_at, c->v_dev + rec_at, sizeof(ic::Rec) * n, hipMemcpyDeviceToHost, st));
        if (cb)
            HIPCHK(c, hipMemcpyAsync(cut_host.data() + ncut_at, room.p + ncut_at, slot_at - ncut_at + sizeof(icut::Cut) * n_slots, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));  // the one wait of a group
        if (!it::it_report(reinterpret_cast<const ic::Rec*>(c->v_host + rec_at), n, acc)) break;
        if (cb) {  // the slots an entry filled, packed behind those of the entries in front of it
            const uint64_t* slot0 = reinterpret_cast<const uint64_t*>(cut_host.data());
            const uint32_t* n_cut = reinterpret_cast<const uint32_t*>(cut_host.data() + ncut_at);
            const icut::Cut* slots = reinterpret_cast<const icut::Cut*>(cut_host.data() + slot_at);
            for (uint32_t k = 0; k < n; k++) {
                h->cuts.insert(h->cuts.end(), slots + slot0[k], slots + slot0[k] + n_cut[k]);
                h->cut0.push_back(h->cuts.size());
            }
        }
        if (wrapper && stored) {
            adler = mi355_checksum_combine(1, adler, c->h_sc->adler, stored);
            crc = mi355_checksum_combine(2, crc, c->h_sc->crc, stored);
        }
    }
    if (!acc.status && wrapper) {
        uint8_t t[8] = {0};
        const size_t tn = wrapper == 1 ? 4 : 8;  // (the last entry's TRAILER test has found the frame whole)
        if (stream_len < tn) return MI355_E_ARG;
        HIPCHK(c, hipMemcpyAsync(t, d_stream + stream_len - tn, tn, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        if (!is::is_trailer_ok((uint32_t)wrapper, t, adler, crc, total)) is::is_checksum_failed(acc);
    }
    uint64_t valid = 0;
    rc = inflate_rc(iw::iw_report(acc, ~0ull, *report, &valid));
    report->ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rc != MI355_OK) {
        inflate_say(c, *report, rc, "inflate seek");
        return rc;
    }
    for (size_t g = 0; g + 1 < h->cut0.size(); g++)
        for (uint64_t i = h->cut0[g]; i < h->cut0[g + 1]; i++) {
            const uint64_t end = i + 1 < h->cut0[g + 1] ? h->cuts[i + 1].pos : (g + 1 < n_blocks ? ents[g + 1].pos : total);
            h->cut_span = end - h->cuts[i].pos > h->cut_span ? end - h->cuts[i].pos : h->cut_span;
        }
    *out = h.release();
    return MI355_OK;
}

// A batch of ranges, device resident stream and buffers (the entry has checked the arguments): the plan, then pass 1, 2 and 3 per
// launch set, one wait a set.  A handle with cuts differs in its descriptors, in the kernel of pass 1 and in the flatten launch
// behind it; everything else of a set is the same text.
int seek_read_ranges(mi355_inflate_seek* h, mi355_deflate_ctx* c, const uint8_t* d_stream, mi355_seek_range* r, size_t n,
                     mi355_inflate_report* reports, hipStream_t st) {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<is::Range> ranges(n);
    for (size_t i = 0; i < n; i++) ranges[i] = is::Range{r[i].off, r[i].len, reinterpret_cast<uint8_t*>(r[i].out)};
    std::vector<is::Set> sets;
    is::is_plan(h->ents.data(), h->ents.size(), h->total, h->pts, ranges.data(), n, c->inflate_group_bytes, d_stream, h->stream_len, h->wrapper, sets,
                h->last);
    std::vector<iw::Rec> acc(n, iw::Rec{ic::V_OK, 0, 0, 0, 0, 0, 0, 0, 0});
    std::vector<uint8_t> failed(n, 0);
    const bool cut = h->cut_bytes != 0;
    h->last_cuts = icut::Counts{0, h->last.symbols, 0, 0};
    std::vector<icut::Item> items;
    std::vector<uint32_t> item0;
    std::vector<uint64_t> ent0;
    // (a measuring aid, only when asked: the time per launch kind -- pass 1, flatten, windows, resolve -- summed over the sets)
    StageClocks<4, 5> clk{c->sk_ev, c->sk_ev_ok, c->sk_ms, st, stage_clocks_on(c, h->last.symbols)};
    if (const int rc = clk.begin(c)) return rc;
    for (is::Set& s : sets) {
        is::is_drop(s, failed);
        const size_t np = s.parts.size(), ne = s.ents.size();
        if (ne > 0x7fffffffull) return MI355_E_UNSUPPORTED;
        if (cut) {  // the set's cuts: pass 1 runs over them, and flatten stands between it and pass 2
            ent0.resize(np);
            for (size_t j = 0; j < np; j++) ent0[j] = h->pts[is::is_point_of(h->ents.data(), h->pts, s.parts[j].lo)];
            icut::ict_items(s, ent0, h->cut0, h->cuts, items, item0);
            if (items.size() > 0x7fffffffull) return MI355_E_UNSUPPORTED;
            h->last_cuts.cuts += items.size(), h->last_cuts.steps += items.size() - ne;
        }
        const size_t ni = cut ? items.size() : 0;
        h->last_cuts.launches += cut ? 4 : 3;
        // workspace: [window slots] [symbols]; descriptors: [Part np] [Entry ne] ([Item ni] [first ne + 1]) | [limit np] [Rec ne] ([cut Rec ni])
        const size_t sym_at = (size_t)s.slots * it::WIN;
        int rc = ensure_buf(c, &c->t_dev, &c->t_dev_cap, sym_at + 2 * (size_t)s.syms + 256);
        if (rc) return rc;
        const size_t ent_at = align_up(sizeof(is::Part) * np, 256), item_at = align_up(ent_at + sizeof(ic::Entry) * ne, 256);
        const size_t first_at = align_up(item_at + sizeof(icut::Item) * ni, 256);
        const size_t front = cut ? first_at + sizeof(uint32_t) * (ne + 1) : ent_at + sizeof(ic::Entry) * ne;  // what goes to the device
        const size_t lim_at = align_up(front, 256), rec_at = align_up(lim_at + sizeof(uint64_t) * np, 256);
        const size_t crec_at = align_up(rec_at + sizeof(ic::Rec) * ne, 256);
        rc = verify_room(c, crec_at + sizeof(icut::Rec) * ni + 256);
        if (rc) return rc;
        memcpy(c->v_host, s.parts.data(), sizeof(is::Part) * np);
        memcpy(c->v_host + ent_at, s.ents.data(), sizeof(ic::Entry) * ne);
        if (cut) {
            memcpy(c->v_host + item_at, items.data(), sizeof(icut::Item) * ni);
            memcpy(c->v_host + first_at, item0.data(), sizeof(uint32_t) * (ne + 1));
        }
        const is::Part* d_parts = reinterpret_cast<const is::Part*>(c->v_dev);
        const ic::Entry* d_ents = reinterpret_cast<const ic::Entry*>(c->v_dev + ent_at);
        uint64_t* d_lim = reinterpret_cast<uint64_t*>(c->v_dev + lim_at);
        ic::Rec* d_recs = reinterpret_cast<ic::Rec*>(c->v_dev + rec_at);
        uint16_t* d_sym = reinterpret_cast<uint16_t*>(c->t_dev + sym_at);
        HIPCHK(c, hipMemcpyAsync(c->v_dev, c->v_host, front, hipMemcpyHostToDevice, st));
        HIPCHK(c, clk.mark(0));
        if (cut) {
            const icut::Item* d_items = reinterpret_cast<const icut::Item*>(c->v_dev + item_at);
            icut::Rec* d_crecs = reinterpret_cast<icut::Rec*>(c->v_dev + crec_at);
            hipLaunchKernelGGL(k_inflate_cut, dim3((uint32_t)ni), dim3(64), 0, st, d_parts, d_ents, d_items, d_sym, d_crecs);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, clk.mark(1));
            hipLaunchKernelGGL(k_inflate_cut_flatten, dim3((uint32_t)ne), dim3(1024), 0, st, d_parts, d_ents, d_items,
                               reinterpret_cast<const uint32_t*>(c->v_dev + first_at), d_crecs, d_sym, d_recs);
        } else {
            hipLaunchKernelGGL(k_inflate_seek, dim3((uint32_t)ne), dim3(64), 0, st, d_parts, d_ents, d_sym, d_recs);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, clk.mark(1));
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, clk.mark(2));
        hipLaunchKernelGGL(k_inflate_seek_window, dim3((uint32_t)np), dim3(1024), 0, st, d_parts, d_ents, d_recs, d_sym, h->store, c->t_dev, d_lim);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, clk.mark(3));
        hipLaunchKernelGGL(k_inflate_seek_resolve, dim3(cdiv(s.syms, 256 * it::RESOLVE_RUN)), dim3(256), 0, st, d_parts, (uint32_t)np, d_ents, d_lim,
                           d_sym, c->t_dev, s.syms);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, clk.mark(4));
        HIPCHK(c, hipMemcpyAsync(c->v_host + rec_at, c->v_dev + rec_at, sizeof(ic::Rec) * ne, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));  // the one wait of a set
        clk.lap(0, 1, 0), clk.lap(2, 3, 2), clk.lap(3, 4, 3);
        if (cut) clk.lap(1, 2, 1);  // (without cuts the two marks stand back to back: no launch kind's time)
        const ic::Rec* recs = reinterpret_cast<const ic::Rec*>(c->v_host + rec_at);
        for (const is::Part& pt : s.parts)
            if (!failed[pt.range] && !is::is_report(recs, pt, acc[pt.range])) failed[pt.range] = 1;
    }
    const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return ranges_give(
        r, n, reports, ms, "inflate seek",
        [&](size_t i, mi355_inflate_report& rep, uint64_t* got) {
            *got = is::is_give(acc[i], r[i].off, r[i].len, h->total);
            uint64_t valid = 0;
            return inflate_rc(iw::iw_report(acc[i], ~0ull, rep, &valid));
        },
        [&](const mi355_inflate_report& rep, int rc, const char* what) { inflate_say(c, rep, rc, what); });
}

bool seek_ranges_bad(const mi355_inflate_seek* h, const mi355_seek_range* r, size_t n) {
    if (!h || (!r && n) || n > 0x7fffffffull) return true;
    for (size_t i = 0; i < n; i++)
        if (!r[i].out && r[i].len) return true;
    return false;
}

}  // namespace

extern "C" {

int mi355_inflate_seek_build_device(mi355_deflate_ctx* c, const void* d_stream, size_t stream_len, int wrapper, const mi355_block_info* blocks,
                                    size_t n_blocks, uint64_t spacing, mi355_inflate_seek** seek, mi355_inflate_report* report, void* hip_stream) {
    uint64_t total = 0;
    if (const char* why = seek_build_args(d_stream, stream_len, wrapper, blocks, n_blocks, spacing, seek, report, &total)) return tabled_refuse(c, why);
    *seek = nullptr;
    DefaultGuard dg_;
    if (const int rc = decode_enter(c, dg_)) return rc;
    return seek_build_one(c, reinterpret_cast<const uint8_t*>(d_stream), stream_len, wrapper, blocks, n_blocks, total, spacing, seek, report,
                          call_stream(c, hip_stream));
}

// host bytes: the handle keeps a device copy of the stream, which every read decodes from
int mi355_inflate_seek_build(mi355_deflate_ctx* c, const uint8_t* stream, size_t stream_len, int wrapper, const mi355_block_info* blocks,
                             size_t n_blocks, uint64_t spacing, mi355_inflate_seek** seek, mi355_inflate_report* report) {
    uint64_t total = 0;
    if (const char* why = seek_build_args(stream, stream_len, wrapper, blocks, n_blocks, spacing, seek, report, &total)) return tabled_refuse(c, why);
    *seek = nullptr;
    DefaultGuard dg_;
    if (const int rc = decode_enter(c, dg_)) return rc;
    uint8_t* d = nullptr;
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&d), stream_len + 64));
    int rc = stage_in(c, stream, stream_len, d);  // into a buffer the handle will own
    if (rc == MI355_OK) rc = seek_build_one(c, d, stream_len, wrapper, blocks, n_blocks, total, spacing, seek, report, c->own_stream);
    if (rc != MI355_OK) {  // (no handle for any failure, MI355_E_DATA among them)
        stage_settle(c);
        (void)hipFree(d);
        return rc;
    }
    (*seek)->d_stream = d;
    return MI355_OK;
}

void mi355_inflate_seek_free(mi355_inflate_seek* seek) { seek_release(seek); }

int mi355_inflate_seek_info(mi355_inflate_seek* h, mi355_seek_info* info) {
    if (!h || !info) return MI355_E_ARG;
    *info = mi355_seek_info{h->total, h->ents.size(), h->pts.size(), h->spacing, h->store_bytes + (h->d_stream ? h->stream_len + 64 : 0), h->stream_len,
                            h->wrapper, 0u};
    return MI355_OK;
}

int mi355_inflate_seek_points(mi355_inflate_seek* h, mi355_seek_point* out, size_t cap, size_t* n) {
    if (!h || !n || (!out && cap)) return MI355_E_ARG;
    *n = h->pts.size();
    if (*n > cap) return MI355_E_OUT_TOO_SMALL;
    for (size_t i = 0; i < h->pts.size(); i++) out[i] = mi355_seek_point{h->ents[h->pts[i]].bit, h->ents[h->pts[i]].pos};
    return MI355_OK;
}

int mi355_inflate_seek_read_batch_device(mi355_inflate_seek* h, const void* d_stream, mi355_seek_range* r, size_t n, mi355_inflate_report* reports,
                                         void* hip_stream) {
    if (seek_ranges_bad(h, r, n)) return MI355_E_ARG;
    const uint8_t* s = d_stream ? reinterpret_cast<const uint8_t*>(d_stream) : h->d_stream;
    if (!s && h->stream_len) return MI355_E_ARG;
    DefaultGuard dg_;
    mi355_deflate_ctx* c = h->c;
    if (const int rc = decode_enter(c, dg_)) return rc;
    return seek_read_ranges(h, c, s, r, n, reports, call_stream(c, hip_stream));
}

int mi355_inflate_seek_read_device(mi355_inflate_seek* h, const void* d_stream, uint64_t off, uint64_t len, void* d_out, uint64_t* got,
                                   mi355_inflate_report* report, void* hip_stream) {
    if (!got || !report) return MI355_E_ARG;
    mi355_seek_range r{off, len, d_out, 0, MI355_OK, 0u};
    const int rc = mi355_inflate_seek_read_batch_device(h, d_stream, &r, 1, report, hip_stream);
    if (rc == MI355_OK || rc == MI355_E_DATA) *got = r.got;
    return rc;
}

// host buffer, a handle of mi355_inflate_seek_build: the range into the context's staging, the bytes that hold data copied back
int mi355_inflate_seek_read(mi355_inflate_seek* h, uint64_t off, uint64_t len, uint8_t* out, uint64_t* got, mi355_inflate_report* report) {
    if (!h || !got || !report || (!out && len) || (!h->d_stream && h->stream_len)) return MI355_E_ARG;
    DefaultGuard dg_;
    mi355_deflate_ctx* c = h->c;
    if (const int rc = decode_enter(c, dg_)) return rc;
    const uint64_t room = is::is_got(off, len, h->total);
    if (const int rc = ensure_buf(c, &c->d_out, &c->d_out_cap, (size_t)room + 64)) return rc;
    mi355_seek_range r{off, len, c->d_out, 0, MI355_OK, 0u};
    int rc = seek_read_ranges(h, c, h->d_stream, &r, 1, report, c->own_stream);
    rc = stage_out(c, rc, out, r.got);  // (nothing was staged in: the wait behind a hard error finds the stream idle)
    if (rc == MI355_OK || rc == MI355_E_DATA) *got = r.got;
    return rc;
}

int mi355_inflate_seek_cuts(mi355_inflate_seek* h, mi355_seek_cut* out, size_t cap, size_t* n) {
    if (!h || !n || (!out && cap)) return MI355_E_ARG;
    *n = h->cuts.size();
    if (*n > cap) return MI355_E_OUT_TOO_SMALL;
    for (size_t i = 0; i < h->cuts.size(); i++) out[i] = mi355_seek_cut{h->cuts[i].bit, h->cuts[i].pos, h->cuts[i].hdr_bit};
    return MI355_OK;
}

// the cut_bytes in force, the cuts, the host bytes they take, the output bytes of the largest cut
int mi355_inflate_seek_cut_info(mi355_inflate_seek* h, uint64_t v[4]) {
    if (!h || !v) return MI355_E_ARG;
    v[0] = h->cut_bytes, v[1] = h->cuts.size(), v[2] = sizeof(icut::Cut) * h->cuts.size() + sizeof(uint64_t) * h->cut0.size(), v[3] = h->cut_span;
    return MI355_OK;
}

// what the handle's last read did: cuts decoded, symbols stored, cuts flatten rewrote, launches
int mi355_inflate_seek_last_read_cuts(mi355_inflate_seek* h, uint64_t v[4]) {
    if (!h || !v) return MI355_E_ARG;
    v[0] = h->last_cuts.cuts, v[1] = h->last_cuts.symbols, v[2] = h->last_cuts.steps, v[3] = h->last_cuts.launches;
    return MI355_OK;
}

// HIP-event time per launch kind of the context's last seek read, summed over its sets: pass 1 (entries or cuts), flatten, windows,
// resolve; zeros unless the stage clocks were on (MI355_CFG_STAGE_CLOCKS)
int mi355_inflate_seek_last_read_stages(mi355_deflate_ctx* c, float ms[4]) {
    if (!ms) return MI355_E_ARG;
    DefaultGuard dg_;
    c = use_ctx(c, dg_);
    if (!c) return MI355_E_HIP;
    for (int k = 0; k < 4; k++) ms[k] = c->sk_ms[k];
    return MI355_OK;
}

// what the handle's last read did, from its plan: entries decoded, symbols stored, window steps, launch sets
int mi355_inflate_seek_last_read(mi355_inflate_seek* h, uint64_t v[4]) {
    if (!h || !v) return MI355_E_ARG;
    v[0] = h->last.entries, v[1] = h->last.symbols, v[2] = h->last.steps, v[3] = h->last.sets;
    return MI355_OK;
}

}  // extern "C"
