// Stand-alone sanitizer run of the large plain members (TEST INFRASTRUCTURE): reads a corpus file of cases and runs the host build of
// inflate_bigmembers.h over each, built with -fsanitize=address,undefined.  The file, the output buffers, the member tables, the
// candidates, the symbols and the windows are exact-size heap allocations: a read one byte outside the file, a store at or beyond
// out_cap, a candidate read beyond an extent's edge or a symbol outside its group is reported.  Per case: the serial walk, then the call
// as the device runs it with the parallel path on; return value, length, report, member count, the rows (all but the HINTED flag) and
// the bytes that hold data must be equal.  Exit status 0: every case ran clean and agreed.
//
// Corpus file: "IBC1", u32 count, then per case u64 stream_len, u64 out_cap, u64 member span, u64 threshold, u64 index span, u64 group
// bytes, the file; all little endian.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/mi355_deflate.h"

extern "C" int inflmembers_serial(const uint8_t* stream, uint64_t stream_len, uint8_t* out, uint64_t out_cap, uint64_t* out_len,
                                  mi355_member_info* members, uint64_t members_cap, uint64_t* n_members, mi355_inflate_report* report);
extern "C" int inflbig_run(int mutant, uint64_t S, const uint8_t* stream, uint64_t stream_len, uint8_t* out, uint64_t out_cap, uint64_t* out_len,
                           mi355_member_info* members, uint64_t members_cap, uint64_t* n_members, mi355_inflate_report* report);
extern "C" int inflbig_set(uint64_t threshold, uint64_t index_span, uint64_t group_bytes);
extern "C" void inflbig_stats(uint64_t v[6]);

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s corpus-file\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    char magic[4];
    uint32_t count = 0;
    if (!rd(f, magic, 4) || memcmp(magic, "IBC1", 4) != 0 || !rd(f, &count, 4)) {
        fprintf(stderr, "not a corpus file\n");
        return 2;
    }
    unsigned long long by_status[13] = {0}, small = 0, walked = 0;
    for (uint32_t i = 0; i < count; i++) {
        uint64_t h[6];
        if (!rd(f, h, sizeof h) || h[0] > (1ull << 31) || h[1] > (1ull << 31) || h[2] < 16 || inflbig_set(h[3], h[4], h[5]) != MI355_OK) {
            fprintf(stderr, "case %u: bad record\n", i);
            return 2;
        }
        const uint64_t sl = h[0], cap = h[1], S = h[2];
        const uint64_t room = sl / 18 + 2;  // (a member is 18 bytes at least)
        uint8_t* s = (uint8_t*)malloc(sl ? sl : 1);
        uint8_t* out[2];
        mi355_member_info* tab[2];
        for (int k = 0; k < 2; k++) {
            out[k] = (uint8_t*)malloc(cap ? cap : 1);
            tab[k] = (mi355_member_info*)malloc(room * sizeof(mi355_member_info));
            if (!out[k] || !tab[k]) return 2;
            memset(out[k], 0xA5, cap ? cap : 1);
            memset(tab[k], 0, room * sizeof(mi355_member_info));
        }
        if (!s || !rd(f, s, sl)) {
            fprintf(stderr, "case %u: short file\n", i);
            return 2;
        }
        mi355_inflate_report r[2];
        uint64_t n[2] = {0, 0}, m[2] = {0, 0};
        int rc[2];
        memset(r, 0, sizeof r);
        rc[0] = inflmembers_serial(sl ? s : NULL, sl, cap ? out[0] : NULL, cap, &n[0], tab[0], room, &m[0], &r[0]);
        rc[1] = inflbig_run(0, S, sl ? s : NULL, sl, cap ? out[1] : NULL, cap, &n[1], tab[1], room, &m[1], &r[1]);
        if (rc[0] != MI355_OK && rc[0] != MI355_E_DATA && rc[0] != MI355_E_OUT_TOO_SMALL) {
            fprintf(stderr, "case %u: unexpected return %d\n", i, rc[0]);
            return 1;
        }
        const uint64_t held = n[0] < cap ? n[0] : cap;
        bool same = rc[1] == rc[0] && n[1] == n[0] && m[1] == m[0] && m[0] <= room && memcmp(&r[1], &r[0], sizeof r[0]) == 0 &&
                    memcmp(out[1], out[0], held) == 0;
        for (uint64_t j = 0; same && j < m[0]; j++) {
            mi355_member_info a = tab[1][j], b = tab[0][j];
            a.flags = b.flags = 0;
            same = memcmp(&a, &b, sizeof a) == 0;
        }
        if (!same) {
            fprintf(stderr, "case %u: the call differs from the serial walk (rc %d / %d, status %u / %u, out_pos %llu / %llu, members %llu / %llu)\n", i,
                    rc[0], rc[1], r[0].status, r[1].status, (unsigned long long)r[0].out_pos, (unsigned long long)r[1].out_pos,
                    (unsigned long long)m[0], (unsigned long long)m[1]);
            return 1;
        }
        walked += m[0];
        if (r[0].status < 13) by_status[r[0].status]++;
        if (rc[0] == MI355_E_OUT_TOO_SMALL) small++;
        free(s);
        for (int k = 0; k < 2; k++) free(out[k]), free(tab[k]);
    }
    fclose(f);
    uint64_t v[6];
    inflbig_stats(v);
    printf("%u cases:", count);
    for (int k = 0; k < 13; k++) printf(" %llu", by_status[k]);
    printf("; %llu too small; %llu members, %llu parallel, %llu handed back\n", small, walked, (unsigned long long)v[0], (unsigned long long)v[1]);
    return 0;
}
