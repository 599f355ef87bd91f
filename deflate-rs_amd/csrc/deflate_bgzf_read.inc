// BGZF reads (include/mi355_deflate.h mi355_bgzf_index_*, mi355_bgzf_read*): byte ranges of the uncompressed data of a blocked gzip
// file, decoding only the members that hold them.  bgzf_read.h has the index, the plan, the clip and the verdict, which the host
// build of tests/bgzfread/ runs too; here are the one kernel and the device side of a call:
//   k_bgzf_read   one workgroup of one wave per DISTINCT member of a launch set: iw_inflate into the member's slot -- the range's own
//                 buffer for a member in place, else a scratch slot of the workspace --, then the member's pieces from the slot to
//                 the ranges that asked for them, then the record
// The index is built by the find, walk and fill kernels of deflate_members_inflate.inc as they stand, and the members' checksums are
// judged by the batch plan and k_inflate_trailer of deflate_inflate.inc: a launch set is that file's decode_half with k_bgzf_read
// and sums_half, so it has two waits: the records, then the trailers.  Nothing waits inside a kernel.  The entries' head, the
// staging of the host forms and the ranges' tail are decode_host.inc's.  DESIGN.md section 19.
#include "bgzf_read.h"

namespace mi355 {

__global__ __launch_bounds__(64) void k_bgzf_read(const IItem* __restrict__ items, const br::Ref* __restrict__ refs,
                                                  const br::Piece* __restrict__ pieces, iw::Rec* __restrict__ recs) {
    __shared__ ic::Tables s_t;
    const IItem it = items[blockIdx.x];
    iw::Rec r;
    iw::iw_inflate<WaveSink>(s_t, it.stream, it.stream_len, it.wrapper, it.out, it.cap, r);
    const br::Ref ref = refs[blockIdx.x];
    const uint64_t valid = br::br_valid<br::Rules>(r, it.cap);
    if (ref.n_pieces && valid) {
        WaveSink::fence(valid);  // the lanes load what other lanes of this wave stored
        for (uint32_t j = 0; j < ref.n_pieces; j++) {
            const br::Piece pc = pieces[ref.piece0 + j];
            br::br_lane_piece<br::Rules>(it.out, pc.lo, pc.hi, pc.dst, valid, WaveSink::lane());
        }
    }
    if (threadIdx.x == 0) recs[blockIdx.x] = r;
}

}  // namespace mi355

struct mi355_bgzf_index {
    mi355::br::Index ix;
};

namespace {

static_assert(sizeof(br::Piece) == 24 && sizeof(br::Ref) == 8, "what k_bgzf_read reads");
static_assert(br::SET_MEMBERS == MEMBER_GROUP, "a launch set is a members call's group");
static_assert(br::MEMBER_MAX == VERIFY_MAX_IN, "what the checksum kernels take");
static_assert(br::RC_ARG == MI355_E_ARG && br::RC_UNSUPPORTED == MI355_E_UNSUPPORTED && br::RC_DATA == MI355_E_DATA, "the header's values");
static_assert(sizeof(mi355_bgzf_info) == 40, "mi355_bgzf_info is 40 bytes");

// Path A from byte 0 on the device: the steps of a members call, with clocks of its own that are never on and the members call's
// kept walk put back behind it
int bgzf_index_one(mi355_deflate_ctx* c, const uint8_t* d_file, size_t file_len, mi355_bgzf_index** idx, mi355_inflate_report* report,
                   hipStream_t st) {
    const auto t0 = std::chrono::steady_clock::now();
    *report = mi355_inflate_report{};
    const uint64_t S = c->member_span, n_spans = im::im_n_spans(file_len, S);
    if (n_spans > 0x7fffffffull) {
        c->err = "bgzf index: the file has too many spans";
        return MI355_E_UNSUPPORTED;
    }
    std::unique_ptr<mi355_bgzf_index> h(new mi355_bgzf_index);
    uint64_t pos = 0;
    int rc = MI355_E_DATA;
    if (file_len) {
        hipEvent_t ev2[2] = {}, ev4[4] = {};
        bool ok2 = false, ok4 = false;
        float ms6[6], ms5[5];
        StageClocks<6, 2> clk{ev2, ok2, ms6, st, false};
        StageClocks<5, 4> pclk{ev4, ok4, ms5, st, false};
        const size_t walk_at = align_up(sizeof(uint64_t) * n_spans, 256), seg_at = align_up(walk_at + sizeof(im::Walk) * n_spans, 256);
        rc = ensure_buf(c, &c->m_dev, &c->m_dev_cap, seg_at + sizeof(im::Seg) * n_spans);
        if (rc) return rc;
        MemberDev be{c, d_file, file_len, nullptr, 0, S, n_spans, st, clk, pclk};
        be.d_cand = reinterpret_cast<uint64_t*>(c->m_dev);
        be.d_walk = reinterpret_cast<im::Walk*>(c->m_dev + walk_at);
        be.d_seg = reinterpret_cast<im::Seg*>(c->m_dev + seg_at);
        std::vector<uint64_t> kept(1, 0);  // (not empty: MemberDev::walk keeps nothing of this walk)
        kept.swap(c->m_cands);
        rc = br::br_build(be, file_len, S, h->ix, &pos);
        kept.swap(c->m_cands);
    }
    report->ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rc == MI355_E_DATA) {
        report->status = MI355_VERIFY_FRAME, report->out_pos = pos;
        inflate_say(c, *report, rc, "bgzf index");
        return rc;
    }
    if (rc) return rc;
    report->out_len = report->out_pos = h->ix.total;
    *idx = h.release();
    return MI355_OK;
}

// A batch of ranges, device resident file and buffers (the entry has checked the arguments).  The file's byte `bias` stands at
// d_file: a host read stages the touched extent only.  copied: the compressed bytes a host read copied, for mi355_bgzf_last_read.
int bgzf_read_ranges(mi355_deflate_ctx* c, const br::Index& ix, const uint8_t* d_file, uint64_t bias, mi355_seek_range* r, size_t n,
                     mi355_inflate_report* reports, hipStream_t st, uint64_t copied) {
    const auto t0 = std::chrono::steady_clock::now();
    for (int k = 0; k < 6; k++) c->br_stats[k] = 0;
    std::vector<br::Range> ranges(n);
    for (size_t i = 0; i < n; i++) ranges[i] = br::Range{r[i].off, r[i].len, reinterpret_cast<uint8_t*>(r[i].out)};
    std::vector<br::Set> sets;
    std::vector<uint8_t> unsupported;
    br::Counts cnt;
    br::br_plan<br::Rules>(ix, ranges.data(), n, c->inflate_group_bytes, sets, unsupported, cnt);
    StageClocks<3, 5> clk{c->br_ev, c->br_ev_ok, c->br_ms, st, stage_clocks_on(c, cnt.distinct * 65536)};
    if (const int rc = clk.begin(c)) return rc;
    std::vector<uint64_t> ids;  // the members decoded, in file order, and their records
    std::vector<iw::Rec> recs;
    ids.reserve(cnt.distinct), recs.reserve(cnt.distinct);
    for (const br::Set& s : sets) {
        const size_t k = s.decs.size(), np = s.pieces.size();
        // descriptors: [IItem k] [Ref k] [Piece np] | the checksum plan | [Rec k]; workspace: the scratch slots
        const size_t ref_at = align_up(sizeof(IItem) * k, 256), piece_at = align_up(ref_at + sizeof(br::Ref) * k, 256);
        const size_t front = piece_at + sizeof(br::Piece) * np;
        const BatchSums plan(front, k, true, sizeof(iw::Rec));
        int rc = verify_room(c, plan.bytes);
        if (rc) return rc;
        if (s.scratch) {
            rc = ensure_buf(c, &c->t_dev, &c->t_dev_cap, (size_t)s.scratch + 256);
            if (rc) return rc;
        }
        IItem* hit = reinterpret_cast<IItem*>(c->v_host);
        br::Ref* href = reinterpret_cast<br::Ref*>(c->v_host + ref_at);
        for (size_t j = 0; j < k; j++) {
            const br::Dec& d = s.decs[j];
            const im::Member& m = ix.mem[d.member];
            hit[j] = IItem{d_file + (m.in_off - bias), m.in_len, d.slot == br::NONE ? d.dst : c->t_dev + d.slot, m.out_len, nullptr, 2u, 0u};
            href[j] = d.ref;
        }
        if (np) memcpy(c->v_host + piece_at, s.pieces.data(), sizeof(br::Piece) * np);
        const iw::Rec* hrec = reinterpret_cast<const iw::Rec*>(c->v_host + plan.rec_at);
        // the first half and wait of a set: inflate_run's (decode_half of deflate_inflate.inc), with this file's kernel and its two arrays
        rc = decode_half(
            c, st, k, front, plan.rec_at,
            [&](const IItem* items, iw::Rec* d_recs) {
                hipLaunchKernelGGL(k_bgzf_read, dim3((uint32_t)k), dim3(64), 0, st, items, reinterpret_cast<const br::Ref*>(c->v_dev + ref_at),
                                   reinterpret_cast<const br::Piece*>(c->v_dev + piece_at), d_recs);
            },
            [&](int e) { return clk.mark(e); });
        if (rc) return rc;
        clk.lap(0, 1, 0);
        // the second half and wait (sums_half): the members that are clean and fit get their sums, the items go up again with the plan
        size_t summed = 0;
        for (size_t j = 0; j < k; j++)
            if (br::br_summed<br::Rules>(hrec[j], hit[j].cap)) hit[j].sc = &plan.states(c)[j].sc, summed++;
        if (summed) {
            rc = sums_half(
                c, st, plan, 2, false, 0, false, [&](size_t j, uint64_t* len) { return *len = hit[j].cap, hit[j].sc != nullptr; },
                [&](int e) { return clk.mark(e == 0 ? 2 : e == 2 ? 3 : 4); });  // (events 2 to 4: the checksums, the trailers)
            if (rc) return rc;
            clk.lap(2, 3, 1), clk.lap(3, 4, 2);
        }
        for (size_t j = 0; j < k; j++) ids.push_back(s.decs[j].member), recs.push_back(hrec[j]);
    }
    const uint64_t v[6] = {cnt.distinct, cnt.in_place, cnt.scratch, cnt.pieces, cnt.sets, copied};
    for (int k = 0; k < 6; k++) c->br_stats[k] = v[k];
    const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return ranges_give(
        r, n, reports, ms, "bgzf read",
        [&](size_t i, mi355_inflate_report& rep, uint64_t* got) -> int {
            if (unsupported[i]) return MI355_E_UNSUPPORTED;
            return br::br_give(ix, ranges[i],
                               [&](uint64_t member, const iw::Rec*& rec, br::Verdict& vd) {
                                   const size_t at = std::lower_bound(ids.begin(), ids.end(), member) - ids.begin();
                                   rec = &recs[at];  // (there: the plan decoded every member a supported range touches)
                                   vd = br::br_judge<br::Rules>(recs[at], ix.mem[member].out_len);
                               },
                               rep, got);
        },
        [&](const mi355_inflate_report& rep, int rc, const char* what) {
            if (rc == MI355_E_DATA)
                inflate_say(c, rep, rc, what);
            else
                c->err = std::string(what) + ": a member's claim exceeds what one launch set takes";
        });
}

bool bgzf_ranges_bad(const mi355_bgzf_index* h, const void* file, const mi355_seek_range* r, size_t n) {
    if (!h || (!r && n) || n > 0x7fffffffull || (!file && h->ix.file_len)) return true;
    for (size_t i = 0; i < n; i++)
        if (!r[i].out && r[i].len) return true;
    return false;
}

}  // namespace

extern "C" {

int mi355_bgzf_index_build_device(mi355_deflate_ctx* c, const void* d_file, size_t file_len, mi355_bgzf_index** idx, mi355_inflate_report* report,
                                  void* hip_stream) {
    if (!idx || !report || (!d_file && file_len)) return tabled_refuse(c, "bgzf index: bad argument");
    *idx = nullptr;
    DefaultGuard dg_;
    if (const int rc = decode_enter(c, dg_)) return rc;
    return bgzf_index_one(c, reinterpret_cast<const uint8_t*>(d_file), file_len, idx, report, call_stream(c, hip_stream));
}

// host bytes: the file into the context's staging, as mi355_inflate_members stages it; nothing of it is kept
int mi355_bgzf_index_build(mi355_deflate_ctx* c, const uint8_t* file, size_t file_len, mi355_bgzf_index** idx, mi355_inflate_report* report) {
    if (!idx || !report || (!file && file_len)) return tabled_refuse(c, "bgzf index: bad argument");
    *idx = nullptr;
    DefaultGuard dg_;
    if (const int rc = decode_enter(c, dg_)) return rc;
    if (const int rc = stage_in(c, file, file_len)) return rc;
    const int rc = bgzf_index_one(c, c->d_in, file_len, idx, report, c->own_stream);
    stage_settle(c);  // (on every path: behind a worker that has waited it finds the stream idle)
    return rc;
}

int mi355_bgzf_index_from_members(const mi355_member_info* members, size_t n, size_t file_len, mi355_bgzf_index** idx) {
    if (!idx) return MI355_E_ARG;
    *idx = nullptr;
    std::unique_ptr<mi355_bgzf_index> h(new mi355_bgzf_index);
    if (!br::br_from_members(members, n, file_len, h->ix)) return MI355_E_ARG;
    *idx = h.release();
    return MI355_OK;
}

void mi355_bgzf_index_free(mi355_bgzf_index* idx) { delete idx; }

int mi355_bgzf_index_info(const mi355_bgzf_index* h, mi355_bgzf_info* info) {
    if (!h || !info) return MI355_E_ARG;
    *info = mi355_bgzf_info{h->ix.total, h->ix.mem.size(), h->ix.file_len, sizeof(*h) + sizeof(im::Member) * h->ix.mem.capacity(), h->ix.max_out};
    return MI355_OK;
}

int mi355_bgzf_index_members(const mi355_bgzf_index* h, mi355_member_info* out, size_t cap, size_t* n) {
    if (!h || !n || (!out && cap)) return MI355_E_ARG;
    *n = h->ix.mem.size();
    if (*n > cap) return MI355_E_OUT_TOO_SMALL;
    memcpy(out, h->ix.mem.data(), sizeof(im::Member) * *n);
    return MI355_OK;
}

int mi355_bgzf_voffset(const mi355_bgzf_index* h, uint64_t uoff, uint64_t* voff) {
    if (!h || !voff) return MI355_E_ARG;
    return br::br_voffset(h->ix, uoff, voff);
}

int mi355_bgzf_uoffset(const mi355_bgzf_index* h, uint64_t voff, uint64_t* uoff) {
    if (!h || !uoff) return MI355_E_ARG;
    return br::br_uoffset(h->ix, voff, uoff);
}

int mi355_bgzf_read_batch_device(mi355_deflate_ctx* c, const mi355_bgzf_index* h, const void* d_file, mi355_seek_range* r, size_t n,
                                 mi355_inflate_report* reports, void* hip_stream) {
    if (bgzf_ranges_bad(h, d_file, r, n)) return tabled_refuse(c, "bgzf read: bad argument");
    DefaultGuard dg_;
    if (const int rc = decode_enter(c, dg_)) return rc;
    return bgzf_read_ranges(c, h->ix, reinterpret_cast<const uint8_t*>(d_file), 0, r, n, reports, call_stream(c, hip_stream), 0);
}

int mi355_bgzf_read_device(mi355_deflate_ctx* c, const mi355_bgzf_index* h, const void* d_file, uint64_t off, uint64_t len, void* d_out,
                           uint64_t* got, mi355_inflate_report* report, void* hip_stream) {
    if (!got || !report) return tabled_refuse(c, "bgzf read: bad argument");
    mi355_seek_range r{off, len, d_out, 0, MI355_OK, 0u};
    const int rc = mi355_bgzf_read_batch_device(c, h, d_file, &r, 1, report, hip_stream);
    if (rc == MI355_OK || rc == MI355_E_DATA) *got = r.got;
    return rc;
}

// host pointers: the compressed extent from the first through the last touched member goes to the device, `got` bytes come back
int mi355_bgzf_read(mi355_deflate_ctx* c, const mi355_bgzf_index* h, const uint8_t* file, uint64_t off, uint64_t len, uint8_t* out,
                    uint64_t* got, mi355_inflate_report* report) {
    if (!h || !got || !report || (!out && len) || (!file && h->ix.file_len)) return tabled_refuse(c, "bgzf read: bad argument");
    DefaultGuard dg_;
    if (const int rc = decode_enter(c, dg_)) return rc;
    const br::Index& ix = h->ix;
    const uint64_t room = br::br_got(off, len, ix.total);
    uint64_t lo = 0, hi = 0;
    if (room) {
        uint64_t k0, k1;
        br::br_touched(ix, off, room, k0, k1);
        lo = ix.mem[k0].in_off, hi = ix.mem[k1].in_off + ix.mem[k1].in_len;
    }
    if (const int rc = ensure_buf(c, &c->d_out, &c->d_out_cap, (size_t)room + 64)) return rc;
    if (const int rc = stage_in(c, file + lo, (size_t)(hi - lo))) return rc;
    mi355_seek_range r{off, room, c->d_out, 0, MI355_OK, 0u};
    int rc = bgzf_read_ranges(c, ix, c->d_in, lo, &r, 1, report, c->own_stream, hi - lo);
    rc = stage_out(c, rc, out, r.got);
    if (rc == MI355_OK || rc == MI355_E_DATA) *got = r.got;
    return rc;
}

// A measuring aid: what the context's last BGZF read did -- distinct members decoded, members in place, members to scratch, pieces
// copied, launch sets, compressed bytes a host read copied
int mi355_bgzf_last_read(mi355_deflate_ctx* c, uint64_t v[6]) {
    if (!c || !v) return MI355_E_ARG;
    for (int k = 0; k < 6; k++) v[k] = c->br_stats[k];
    return MI355_OK;
}

// ... and its HIP-event milliseconds per launch kind, summed over its sets: decode and clip, checksums, trailers; zeros unless the
// stage clocks were on (MI355_CFG_STAGE_CLOCKS)
int mi355_bgzf_last_read_stages(mi355_deflate_ctx* c, float ms[3]) {
    if (!c || !ms) return MI355_E_ARG;
    for (int k = 0; k < 3; k++) ms[k] = c->br_ms[k];
    return MI355_OK;
}

}  // extern "C"
