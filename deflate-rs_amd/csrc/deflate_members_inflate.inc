// Members (include/mi355_deflate.h mi355_inflate_members[_device]): a gzip file of any number of members decoded to its bytes, the
// runs of members that state their own size (BGZF) in parallel.  inflate_members.h has the rules and the call's control flow
// (im_run), which the host build of tests/inflmembers/ runs too; here are its four kernels and the device side of its steps:
//   k_member_find    one workgroup of one wave per span: the span's candidate, the first hinted byte offset in it
//   k_member_walk    one LANE per span: hops from header to header, counting members and ISIZEs, until it links, ends or opens
//   k_member_fill    one lane per walker on the chain: the (offset, size, ISIZE) rows of its members
//   k_inflate_chain  one workgroup of one wave: member after member, open ended (Path B)
// The hinted members themselves are decoded by k_inflate as it stands, and the members' checksums by the batch plan and
// k_inflate_trailer of deflate_inflate.inc, through that file's decode_half and sums_half.  A large member that states no size is found and decoded in parallel by the kernels of
// deflate_bigmembers_inflate.inc, which MemberDev::chain drives (inflate_bigmembers.h).  Nothing waits inside a kernel.  The host
// driver's shared steps are in decode_host.inc.  DESIGN.md section 15.
#include "inflate_members.h"

namespace mi355 {

// the finder's ballot on top of the chain's sink
struct MemberOps : WaveSink, im::Rules {
    static __host__ __device__ uint64_t survivors(const uint8_t* s, uint64_t n, uint64_t base, uint64_t end) {
#if defined(__HIP_DEVICE_COMPILE__)
        const uint64_t o = base + lane();
        return __ballot(o < end && im::im_fixed4(s, n, o));
#else
        return 0;
#endif
    }
};

__global__ __launch_bounds__(64) void k_member_find(const uint8_t* __restrict__ s, uint64_t n, uint64_t S, uint64_t* __restrict__ cand) {
    const uint64_t c = im::im_find<MemberOps>(s, n, blockIdx.x, S);
    if (threadIdx.x == 0) cand[blockIdx.x] = c;
}

__global__ __launch_bounds__(64) void k_member_walk(const uint8_t* __restrict__ s, uint64_t n, uint64_t S, uint64_t n_spans, uint64_t o,
                                                    const uint64_t* __restrict__ cand, im::Walk* __restrict__ recs) {
    const uint64_t k = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (k >= n_spans) return;
    im::Walk r;
    im::im_walk_span<MemberOps>(s, n, cand, n_spans, S, o, k, r);
    recs[k] = r;
}

__global__ __launch_bounds__(64) void k_member_fill(const uint8_t* __restrict__ s, uint64_t n, const im::Seg* __restrict__ segs, uint64_t n_segs,
                                                    im::Hint* __restrict__ rows, uint64_t n_rows) {
    const uint64_t k = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (k >= n_segs) return;
    im::im_fill<MemberOps>(s, n, segs[k], rows, n_rows);
}

struct ChainArgs {
    const uint8_t* s;
    uint64_t n, o, p;
    uint8_t* out;
    uint64_t out_cap;
    uint32_t ignore_hints, room;
    uint32_t behind, pad;  // members the launch set has walked in front of o (inflate_bigmembers.h)
};
__global__ __launch_bounds__(64) void k_inflate_chain(const ChainArgs a, im::Member* __restrict__ rows, iw::Rec* __restrict__ recs,
                                                      im::ChainEnd* __restrict__ end) {
    __shared__ ic::Tables s_t;
    im::ChainEnd e;
    im::im_chain_behind<MemberOps>(s_t, a.s, a.n, a.o, a.p, a.out, a.out_cap, a.ignore_hints != 0, a.behind, rows, recs, a.room, e);
    if (threadIdx.x == 0) *end = e;
}

}  // namespace mi355

namespace {

static_assert(sizeof(im::Member) == 40 && sizeof(mi355_member_info) == 40, "mi355_member_info mirrors im::Member");
static_assert(im::SPAN_DEFAULT == 65536 && im::SPAN_MIN == 16 && im::SPAN_MAX == (1ull << 30), "the setting's default and range");
static_assert(im::HINTED == MI355_MEMBER_HINTED, "the flag");
static_assert(sizeof(im::Walk) == 40 && sizeof(mi355_member_walk) == 40, "mi355_member_walk mirrors im::Walk");

constexpr uint32_t MEMBER_GROUP = 16384;  // members of one decode launch and of one checksum pass: what the descriptor room is grown to
constexpr uint32_t CHAIN_ROOM = 1024;     // members of one launch of Path B

// the device side of im_run's steps for one call
struct MemberDev {
    mi355_deflate_ctx* c;
    const uint8_t* s;
    uint64_t n;
    uint8_t* out;
    uint64_t out_cap, S, n_spans;
    hipStream_t st;
    StageClocks<6, 2>& clk;
    StageClocks<5, 4>& pclk;  // the launch kinds of the large plain members: discovery find and walk, tabled decode, window chains, resolve
    ib::Stats stats = {};
    uint64_t* d_cand = nullptr;
    im::Walk* d_walk = nullptr;
    im::Seg* d_seg = nullptr;

    static uint64_t group() { return MEMBER_GROUP; }
    // the wait behind a launch between marks 0 and 1, its time into `slot`
    int wait(int slot) {
        HIPCHK(c, hipStreamSynchronize(st));
        clk.lap(0, 1, slot);
        return MI355_OK;
    }
    int find(uint64_t) {
        HIPCHK(c, clk.mark(0));
        hipLaunchKernelGGL(k_member_find, dim3((uint32_t)n_spans), dim3(64), 0, st, s, n, S, d_cand);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, clk.mark(1));
        return wait(0);
    }
    int walk(uint64_t o, std::vector<im::Walk>& w) {
        w.resize(n_spans);
        HIPCHK(c, clk.mark(0));
        hipLaunchKernelGGL(k_member_walk, dim3(cdiv(n_spans, 64)), dim3(64), 0, st, s, n, S, n_spans, o, d_cand, d_walk);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, clk.mark(1));
        HIPCHK(c, hipMemcpyAsync(w.data(), d_walk, sizeof(im::Walk) * n_spans, hipMemcpyDeviceToHost, st));
        const bool keep = c->m_cands.empty();  // the call's first walk: kept with the candidates for mi355_inflate_members_last_walks
        if (keep) {
            c->m_cands.resize(n_spans);
            HIPCHK(c, hipMemcpyAsync(c->m_cands.data(), d_cand, sizeof(uint64_t) * n_spans, hipMemcpyDeviceToHost, st));
        }
        if (const int rc = wait(1)) return rc;
        if (keep) c->m_walks.assign(reinterpret_cast<const uint8_t*>(w.data()), reinterpret_cast<const uint8_t*>(w.data() + n_spans));
        return MI355_OK;
    }
    int fill(const std::vector<im::Seg>& segs, uint64_t n_rows, std::vector<im::Hint>& rows) {
        rows.resize(n_rows);
        if (n_rows > n / im::HOP_MIN + 1 || segs.size() > n_spans) return MI355_E_HIP;  // (never: the walkers' counts are bounded so)
        if (const int rc = ensure_buf(c, &c->m_rows, &c->m_rows_cap, sizeof(im::Hint) * n_rows)) return rc;
        im::Hint* d_rows = reinterpret_cast<im::Hint*>(c->m_rows);
        HIPCHK(c, hipMemcpyAsync(d_seg, segs.data(), sizeof(im::Seg) * segs.size(), hipMemcpyHostToDevice, st));
        HIPCHK(c, clk.mark(0));
        hipLaunchKernelGGL(k_member_fill, dim3(cdiv(segs.size(), 64)), dim3(64), 0, st, s, n, d_seg, (uint64_t)segs.size(), d_rows, n_rows);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, clk.mark(1));
        HIPCHK(c, hipMemcpyAsync(rows.data(), d_rows, sizeof(im::Hint) * n_rows, hipMemcpyDeviceToHost, st));
        return wait(2);
    }
    // k members as their rows claim them, the first at output position p: inflate_run's first half (decode_half of
    // deflate_inflate.inc) with k_inflate, wrapper 2, no sums yet.  Its second half is sums() below: the two are apart here because
    // the checksums of a members call are judged once over the whole table, after Path B has had its say, and not per launch.
    int decode(const im::Hint* rows, uint64_t k, uint64_t p, std::vector<iw::Rec>& got) {
        const size_t rec_at = align_up(sizeof(IItem) * k, 256);
        if (const int rc = verify_room(c, rec_at + sizeof(iw::Rec) * k)) return rc;
        IItem* hit = reinterpret_cast<IItem*>(c->v_host);
        for (uint64_t j = 0; j < k; j++) {
            const im::Hint& h = rows[j];
            const bool inside = h.in_off <= n && h.in_len <= n - h.in_off;  // (always: im_hint tested the extent)
            const uint64_t room = im::im_room_at(out_cap, p);
            hit[j] = IItem{s + (inside ? h.in_off : 0), inside ? h.in_len : 0, im::im_out_at(out, out_cap, p), room < h.isize ? room : h.isize,
                           nullptr, 2u, 0u};
            p += h.isize;
        }
        if (const int rc = decode_half(c, st, k, sizeof(IItem) * k, rec_at, inflate_launch(k, st), [&](int e) { return clk.mark(e); })) return rc;
        clk.lap(0, 1, 3);
        const iw::Rec* recs = reinterpret_cast<const iw::Rec*>(c->v_host + rec_at);
        got.assign(recs, recs + k);
        return MI355_OK;
    }
    // Path B from (o, p): by discovery and the joint tabled launch sets when enough of the file is left, else -- and for what those
    // leave -- by the one wave
    int chain(uint64_t o, uint64_t p, bool ignore_hints, std::vector<im::Member>& rows, std::vector<iw::Rec>& got, im::ChainEnd& e) {
        if (c->member_parallel && o < n && n - o >= c->member_parallel && ix::ix_n_spans(n, c->index_span) <= 0x7fffffffull)
            return ib::ib_chain<ib::Rules>(*this, s, n, o, p, out, out_cap, ignore_hints, CHAIN_ROOM, rows, got, e, stats);
        return serial(o, p, ignore_hints, 0u, CHAIN_ROOM, rows, got, e);
    }
    uint64_t threshold() const { return c->member_parallel; }
    uint64_t span() const { return c->index_span; }
    uint64_t group_bytes() const { return c->inflate_group_bytes; }
    // the head of the member at o: the finder's workgroup of span 0 alone (its candidate is o's first deflate bit, whatever stands there)
    int head(uint64_t o, ib::Head& h) {
        const uint64_t n_all = ix::ix_n_spans(n, c->index_span);
        const size_t cand_at = 256 + it::WIN, walk_at = align_up(cand_at + sizeof(uint64_t) * n_all, 256);
        if (const int rc = ensure_buf(c, &c->mp_dev, &c->mp_dev_cap, walk_at + sizeof(ix::Walk) * n_all)) return rc;
        const DItem d{s, n, o, c->index_span, 0, 1, 1, 1u, 0u};
        HIPCHK(c, pclk.mark(0));
        hipLaunchKernelGGL(k_bigmember_find, dim3(1), dim3(64), 0, st, d, reinterpret_cast<uint64_t*>(c->mp_dev + cand_at),
                           reinterpret_cast<ib::Head*>(c->mp_dev));
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, pclk.mark(1));
        HIPCHK(c, hipMemcpyAsync(&h, c->mp_dev, sizeof h, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        pclk.lap(0, 1, 0);
        return MI355_OK;
    }
    // one round of a discovery (ib_discover): [Head] | [carried window] | [candidate n_all] | [Walk n_all], sized once for the file
    int round(uint64_t o, bool first, uint64_t rewalk, uint64_t k_lo, uint64_t k_hi, ib::Head& head, std::vector<ix::Walk>& w) {
        const uint64_t n_all = ix::ix_n_spans(n, c->index_span);
        if (k_hi > n_all || k_lo > k_hi || rewalk >= k_hi || w.size() < k_hi) return MI355_E_HIP;  // (never)
        const size_t cand_at = 256 + it::WIN, walk_at = align_up(cand_at + sizeof(uint64_t) * n_all, 256);
        if (const int rc = ensure_buf(c, &c->mp_dev, &c->mp_dev_cap, walk_at + sizeof(ix::Walk) * n_all)) return rc;
        ib::Head* d_head = reinterpret_cast<ib::Head*>(c->mp_dev);
        uint64_t* d_c = reinterpret_cast<uint64_t*>(c->mp_dev + cand_at);
        ix::Walk* d_w = reinterpret_cast<ix::Walk*>(c->mp_dev + walk_at);
        const DItem d{s, n, o, c->index_span, rewalk, k_lo, k_hi, first ? 1u : 0u, 0u};
        const uint64_t n_find = first ? k_hi : k_hi - k_lo;
        HIPCHK(c, pclk.mark(0));
        if (n_find) hipLaunchKernelGGL(k_bigmember_find, dim3((uint32_t)n_find), dim3(64), 0, st, d, d_c, d_head);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, pclk.mark(1));
        hipLaunchKernelGGL(k_bigmember_walk, dim3((uint32_t)(k_hi - k_lo + 1)), dim3(64), 0, st, d, d_c, d_w);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, pclk.mark(2));
        if (first) HIPCHK(c, hipMemcpyAsync(&head, d_head, sizeof head, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(w.data() + rewalk, d_w + rewalk, sizeof(ix::Walk), hipMemcpyDeviceToHost, st));
        if (k_hi > k_lo) HIPCHK(c, hipMemcpyAsync(w.data() + k_lo, d_w + k_lo, sizeof(ix::Walk) * (k_hi - k_lo), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        pclk.lap(0, 1, 0), pclk.lap(1, 2, 1);
        return MI355_OK;
    }
    // the three passes over one group of parts: descriptors [Entry n] | [Part np] | [limit np] | [Rec n], workspace [window n + 1]
    // [symbols]; the window a group leaves for the next one waits in the discovery room (the workspace may move when it grows)
    int decode(const ib::Plan& g, bool first, std::vector<ic::Rec>& got) {
        const size_t k = g.ents.size(), np = g.parts.size();
        got.resize(k);
        if (!k || !np || k > it::GROUP_ENTRIES) return MI355_E_HIP;  // (never)
        const size_t parts_at = align_up(sizeof(ic::Entry) * k, 256), lim_at = align_up(parts_at + sizeof(ib::Part) * np, 256);
        const size_t rec_at = align_up(lim_at + sizeof(uint64_t) * np, 256), sym_at = (k + 1) * it::WIN;
        if (const int rc = verify_room(c, rec_at + sizeof(ic::Rec) * k)) return rc;
        if (const int rc = ensure_buf(c, &c->t_dev, &c->t_dev_cap, sym_at + 2 * (size_t)g.syms + 256)) return rc;
        if (const int rc = ensure_buf(c, &c->mp_dev, &c->mp_dev_cap, 256 + it::WIN)) return rc;
        memcpy(c->v_host, g.ents.data(), sizeof(ic::Entry) * k);
        memcpy(c->v_host + parts_at, g.parts.data(), sizeof(ib::Part) * np);
        const ic::Entry* d_ents = reinterpret_cast<const ic::Entry*>(c->v_dev);
        const ib::Part* d_parts = reinterpret_cast<const ib::Part*>(c->v_dev + parts_at);
        uint64_t* d_lim = reinterpret_cast<uint64_t*>(c->v_dev + lim_at);
        ic::Rec* d_recs = reinterpret_cast<ic::Rec*>(c->v_dev + rec_at);
        uint16_t* d_sym = reinterpret_cast<uint16_t*>(c->t_dev + sym_at);
        HIPCHK(c, hipMemcpyAsync(c->v_dev, c->v_host, parts_at + sizeof(ib::Part) * np, hipMemcpyHostToDevice, st));
        if (g.parts[0].carried) {
            if (first) return MI355_E_HIP;  // (never: a set's first group begins with a member)
            HIPCHK(c, hipMemcpyAsync(c->t_dev, c->mp_dev + 256, it::WIN, hipMemcpyDeviceToDevice, st));
        }
        HIPCHK(c, pclk.mark(0));
        hipLaunchKernelGGL(k_inflate_mtab, dim3((uint32_t)k), dim3(64), 0, st, d_parts, d_ents, d_sym, d_recs);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, pclk.mark(1));
        hipLaunchKernelGGL(k_inflate_mtab_window, dim3((uint32_t)np), dim3(1024), 0, st, d_parts, d_ents, d_recs, d_sym, c->t_dev, (uint32_t)k, d_lim);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, pclk.mark(2));
        if (g.syms) {
            hipLaunchKernelGGL(k_inflate_mtab_resolve, dim3(cdiv(g.syms, 256 * it::RESOLVE_RUN)), dim3(256), 0, st, d_parts, (uint32_t)np, d_ents, d_lim,
                               d_sym, c->t_dev, g.syms);
            HIPCHK(c, hipGetLastError());
        }
        HIPCHK(c, pclk.mark(3));
        if (g.carry_out) HIPCHK(c, hipMemcpyAsync(c->mp_dev + 256, c->t_dev + k * it::WIN, it::WIN, hipMemcpyDeviceToDevice, st));
        HIPCHK(c, hipMemcpyAsync(c->v_host + rec_at, c->v_dev + rec_at, sizeof(ic::Rec) * k, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));  // the one wait of a group
        pclk.lap(0, 1, 2), pclk.lap(1, 2, 3), pclk.lap(2, 3, 4);
        memcpy(got.data(), c->v_host + rec_at, sizeof(ic::Rec) * k);
        return MI355_OK;
    }
    // one launch of k_inflate_chain: the one wave, member after member
    int serial(uint64_t o, uint64_t p, bool ignore_hints, uint32_t behind, uint32_t room, std::vector<im::Member>& rows, std::vector<iw::Rec>& got,
               im::ChainEnd& e) {
        if (!room || room > CHAIN_ROOM) return MI355_E_HIP;  // (never)
        const size_t rec_at = align_up(sizeof(im::Member) * CHAIN_ROOM, 256), end_at = align_up(rec_at + sizeof(iw::Rec) * CHAIN_ROOM, 256);
        if (const int rc = ensure_buf(c, &c->m_rows, &c->m_rows_cap, end_at + sizeof(im::ChainEnd))) return rc;
        const ChainArgs a{s, n, o, p, out, out_cap, ignore_hints ? 1u : 0u, room, behind, 0u};
        HIPCHK(c, clk.mark(0));
        hipLaunchKernelGGL(k_inflate_chain, dim3(1), dim3(64), 0, st, a, reinterpret_cast<im::Member*>(c->m_rows),
                           reinterpret_cast<iw::Rec*>(c->m_rows + rec_at), reinterpret_cast<im::ChainEnd*>(c->m_rows + end_at));
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, clk.mark(1));
        HIPCHK(c, hipMemcpyAsync(&e, c->m_rows + end_at, sizeof e, hipMemcpyDeviceToHost, st));
        if (const int rc = wait(4)) return rc;
        if (e.count > CHAIN_ROOM) return MI355_E_HIP;  // (never)
        rows.resize(e.count), got.resize(e.count);
        if (e.count) {
            HIPCHK(c, hipMemcpyAsync(rows.data(), c->m_rows, sizeof(im::Member) * e.count, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipMemcpyAsync(got.data(), c->m_rows + rec_at, sizeof(iw::Rec) * e.count, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
        }
        return MI355_OK;
    }
    // The checksum pass over the member table: the batch plan's flat CRC launch over the outputs of the judged members, then
    // k_inflate_trailer against their trailers, MEMBER_GROUP members a turn; it stops behind the first turn that holds a failure.
    // (inflate_run's second half, sums_half, a turn: the items here carry no decode, sc == nullptr marks a member that is not judged,
    // and the records go up with the plan.)
    int sums(const std::vector<im::Member>& mem, std::vector<iw::Rec>& recs) {
        for (size_t lo = 0; lo < mem.size(); lo += MEMBER_GROUP) {
            const size_t k = mem.size() - lo < MEMBER_GROUP ? mem.size() - lo : MEMBER_GROUP;
            if (std::none_of(mem.begin() + lo, mem.begin() + lo + k, [&](const im::Member& m) { return im::im_judged(m, out_cap); })) continue;
            const BatchSums plan(sizeof(IItem) * k, k, true, sizeof(iw::Rec));
            if (const int rc = verify_room(c, plan.bytes)) return rc;
            IItem* hit = reinterpret_cast<IItem*>(c->v_host);
            for (size_t j = 0; j < k; j++) {
                const im::Member& m = mem[lo + j];
                const bool on = im::im_judged(m, out_cap);
                hit[j] = IItem{s + (on ? m.in_off : 0), on ? m.in_len : 0, im::im_out_at(out, out_cap, m.out_off), on ? m.out_len : 0,
                               on ? &plan.states(c)[j].sc : nullptr, 2u, 0u};
            }
            memcpy(c->v_host + plan.rec_at, recs.data() + lo, sizeof(iw::Rec) * k);
            const int rc = sums_half(
                c, st, plan, 2, false, 0, true, [&](size_t j, uint64_t* n) { return *n = hit[j].cap, hit[j].sc != nullptr; },
                [&](int e) { return e < 2 ? clk.mark(e) : hipSuccess; });  // (one slot for the checksums and the trailers)
            if (rc == MI355_E_UNSUPPORTED) c->err = "inflate members: a member inflates to more than 4 GiB - 64 KiB";
            if (rc) return rc;
            clk.lap(0, 1, 5);
            memcpy(recs.data() + lo, c->v_host + plan.rec_at, sizeof(iw::Rec) * k);
            for (size_t j = 0; j < k; j++)
                if (recs[lo + j].status) return MI355_OK;
        }
        return MI355_OK;
    }
};

bool members_args_bad(const void* stream, size_t stream_len, const void* out, size_t out_cap, const size_t* out_len, const void* members,
                      size_t members_cap, const mi355_inflate_report* report) {
    return !report || !out_len || (!stream && stream_len) || (!out && out_cap) || (!members && members_cap);
}

// a members call refused for its arguments: no other call's counters stay behind it
int members_refuse(mi355_deflate_ctx* c) {
    if (c)
        for (int k = 0; k < 6; k++) c->mp_stats[k] = 0;
    return tabled_refuse(c, "inflate members: bad argument");
}

// one file, device resident, its arguments checked by the entry; *valid: the bytes of d_out that hold data
int members_one(mi355_deflate_ctx* c, const uint8_t* d_stream, size_t stream_len, uint8_t* d_out, size_t out_cap, size_t* out_len,
                mi355_member_info* members, size_t members_cap, size_t* n_members, mi355_inflate_report* report, hipStream_t st,
                uint64_t* valid) {
    const auto t0 = std::chrono::steady_clock::now();
    c->m_cands.clear(), c->m_walks.clear();
    for (int k = 0; k < 6; k++) c->mp_stats[k] = 0;  // (first: a call that fails leaves no other call's counters)
    const uint64_t S = c->member_span, n_spans = im::im_n_spans(stream_len, S);
    if (n_spans > 0x7fffffffull) {
        c->err = "inflate members: the file has too many spans";
        return MI355_E_UNSUPPORTED;
    }
    StageClocks<6, 2> clk{c->m_ev, c->m_ev_ok, c->m_ms, st, stage_clocks_on(c, stream_len)};
    int rc = clk.begin(c);
    if (rc) return rc;
    StageClocks<5, 4> pclk{c->mp_ev, c->mp_ev_ok, c->mp_ms, st, stage_clocks_on(c, stream_len)};
    rc = pclk.begin(c);
    if (rc) return rc;
    // [candidate n] | [Walk n] | [Seg n]
    const size_t walk_at = align_up(sizeof(uint64_t) * n_spans, 256), seg_at = align_up(walk_at + sizeof(im::Walk) * n_spans, 256);
    rc = ensure_buf(c, &c->m_dev, &c->m_dev_cap, seg_at + sizeof(im::Seg) * n_spans);
    if (rc) return rc;
    MemberDev be{c, d_stream, stream_len, d_out, out_cap, S, n_spans, st, clk, pclk};
    be.d_cand = reinterpret_cast<uint64_t*>(c->m_dev);
    be.d_walk = reinterpret_cast<im::Walk*>(c->m_dev + walk_at);
    be.d_seg = reinterpret_cast<im::Seg*>(c->m_dev + seg_at);
    std::vector<im::Member> mem;
    std::vector<iw::Rec> recs;
    rc = im::im_run(be, stream_len, S, mem, recs);
    const uint64_t par[6] = {be.stats.parallel, be.stats.handed, be.stats.spans, be.stats.walkers, be.stats.entries, be.stats.sets};
    for (int k = 0; k < 6; k++) c->mp_stats[k] = par[k];
    if (rc) return rc;
    uint64_t total = 0;
    if (!(im::im_total(mem, total) && total > out_cap)) {  // (longer than the room: no checksum is judged, as in mi355_inflate)
        rc = be.sums(mem, recs);
        if (rc) return rc;
    }
    rc = inflate_rc(im::im_report(mem, recs, out_cap, *report, valid));
    report->ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *out_len = rc == MI355_E_DATA ? (size_t)*valid : (size_t)report->out_len;
    if (n_members) *n_members = mem.size();
    for (size_t j = 0; j < mem.size() && j < members_cap; j++)
        members[j] = mi355_member_info{mem[j].in_off, mem[j].in_len, mem[j].out_off, mem[j].out_len, mem[j].flags, mem[j].status};
    if (rc != MI355_OK) inflate_say(c, *report, rc, "inflate members");
    return rc;
}

}  // namespace

extern "C" {

int mi355_inflate_members_device(mi355_deflate_ctx* c, const void* d_stream, size_t stream_len, void* d_out, size_t out_cap, size_t* out_len,
                                 mi355_member_info* members, size_t members_cap, size_t* n_members, mi355_inflate_report* report,
                                 void* hip_stream) {
    if (members_args_bad(d_stream, stream_len, d_out, out_cap, out_len, members, members_cap, report))
        return members_refuse(c);
    DefaultGuard dg_;
    if (const int rc = decode_enter(c, dg_)) return rc;
    uint64_t valid = 0;
    return members_one(c, reinterpret_cast<const uint8_t*>(d_stream), stream_len, reinterpret_cast<uint8_t*>(d_out), out_cap, out_len, members,
                       members_cap, n_members, report, call_stream(c, hip_stream), &valid);
}

// host buffers: staged_call around the device worker
int mi355_inflate_members(mi355_deflate_ctx* c, const uint8_t* stream, size_t stream_len, uint8_t* out, size_t out_cap, size_t* out_len,
                          mi355_member_info* members, size_t members_cap, size_t* n_members, mi355_inflate_report* report) {
    if (members_args_bad(stream, stream_len, out, out_cap, out_len, members, members_cap, report))
        return members_refuse(c);
    DefaultGuard dg_;
    if (const int rc = decode_enter(c, dg_)) return rc;
    return staged_call(c, stream, stream_len, out, out_cap, [&](const uint8_t* d_stream, uint8_t* d_out, hipStream_t st, uint64_t* valid) {
        return members_one(c, d_stream, stream_len, d_out, out_cap, out_len, members, members_cap, n_members, report, st, valid);
    });
}

// HIP-event milliseconds of the context's last members call per launch kind, summed over its launches: find, walk, fill, member
// decode, chain decode, checksums; zeros unless the stage clocks were on (MI355_CFG_STAGE_CLOCKS)
int mi355_inflate_members_last_stages(mi355_deflate_ctx* c, float ms[6]) {
    if (!c || !ms) return MI355_E_ARG;
    for (int k = 0; k < 6; k++) ms[k] = c->m_ms[k];
    return MI355_OK;
}

// The large plain members of the context's last members call (MI355_CFG_INFLATE_MEMBER_PARALLEL_BYTES): members decoded by the
// parallel path, members handed back to the one-wave chain, index spans searched, walkers launched, table entries decoded, launch sets
int mi355_inflate_members_last_parallel(mi355_deflate_ctx* c, uint64_t v[6]) {
    if (!c || !v) return MI355_E_ARG;
    for (int k = 0; k < 6; k++) v[k] = c->mp_stats[k];
    return MI355_OK;
}

// ... and their HIP-event milliseconds per launch kind, summed over the call's launches: discovery find, discovery walk, tabled
// decode, window chains, resolve; zeros unless the stage clocks were on (MI355_CFG_STAGE_CLOCKS)
int mi355_inflate_members_last_parallel_stages(mi355_deflate_ctx* c, float ms[5]) {
    if (!c || !ms) return MI355_E_ARG;
    for (int k = 0; k < 5; k++) ms[k] = c->mp_ms[k];
    return MI355_OK;
}

// the candidates and the walkers' records of the first walk (the run from byte 0) of the context's last members call, one of each
// per span; none for an empty file or a call that failed in front of its walk
int mi355_inflate_members_last_walks(mi355_deflate_ctx* c, uint64_t* cand, mi355_member_walk* walks, size_t cap, size_t* n_spans) {
    if (!c || !n_spans || ((!cand || !walks) && cap)) return MI355_E_ARG;
    const size_t n = c->m_walks.size() / sizeof(im::Walk);
    *n_spans = n;
    if (n > cap) return MI355_E_OUT_TOO_SMALL;
    if (n && c->m_cands.size() >= n) {
        memcpy(cand, c->m_cands.data(), sizeof(uint64_t) * n);
        memcpy(walks, c->m_walks.data(), sizeof(im::Walk) * n);
    }
    return MI355_OK;
}

}  // extern "C"
