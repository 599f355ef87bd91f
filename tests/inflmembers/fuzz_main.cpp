// Stand-alone sanitizer run of the members inflate (TEST INFRASTRUCTURE): reads a corpus file of (file, span size, out_cap) cases and
// runs the host build of inflate_members.h over each, built with -fsanitize=address,undefined.  The file, the output buffers and the
// member tables are exact-size heap allocations: a read one byte outside the file, a store at or beyond out_cap, or a row one element
// outside its table is reported.  Per case: the serial walk, then the call as the device runs it with the finder lane by lane and as
// the plain predicate; return value, length, report, member count, the rows (all but the HINTED flag) and the bytes that hold data
// must be equal.  Exit status 0: every case ran clean and agreed.
//
// Corpus file: "IMC1", u32 count, then per case u64 stream_len, u64 out_cap, u64 span_bytes, the file; all little endian.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/mi355_deflate.h"

extern "C" int inflmembers_serial(const uint8_t* stream, uint64_t stream_len, uint8_t* out, uint64_t out_cap, uint64_t* out_len,
                                  mi355_member_info* members, uint64_t members_cap, uint64_t* n_members, mi355_inflate_report* report);
extern "C" int inflmembers_run(int mutant, int lanes, uint64_t S, const uint8_t* stream, uint64_t stream_len, uint8_t* out, uint64_t out_cap,
                               uint64_t* out_len, mi355_member_info* members, uint64_t members_cap, uint64_t* n_members,
                               mi355_inflate_report* report, uint64_t* cand);

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
    if (!rd(f, magic, 4) || memcmp(magic, "IMC1", 4) != 0 || !rd(f, &count, 4)) {
        fprintf(stderr, "not a corpus file\n");
        return 2;
    }
    unsigned long long by_status[13] = {0}, small = 0, hinted = 0, walked = 0;
    for (uint32_t i = 0; i < count; i++) {
        uint64_t sl, cap, S;
        if (!rd(f, &sl, 8) || !rd(f, &cap, 8) || !rd(f, &S, 8) || sl > (1ull << 31) || cap > (1ull << 31) || S < 16) {
            fprintf(stderr, "case %u: bad record\n", i);
            return 2;
        }
        const uint64_t room = sl / 18 + 2;  // (a member is 18 bytes at least)
        uint8_t* s = (uint8_t*)malloc(sl ? sl : 1);
        uint8_t* out[3];
        mi355_member_info* tab[3];
        for (int k = 0; k < 3; k++) {
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
        mi355_inflate_report r[3];
        uint64_t n[3] = {0, 0, 0}, m[3] = {0, 0, 0};
        int rc[3];
        memset(r, 0, sizeof r);
        rc[0] = inflmembers_serial(sl ? s : NULL, sl, cap ? out[0] : NULL, cap, &n[0], tab[0], room, &m[0], &r[0]);
        rc[1] = inflmembers_run(0, 1, S, sl ? s : NULL, sl, cap ? out[1] : NULL, cap, &n[1], tab[1], room, &m[1], &r[1], NULL);
        rc[2] = inflmembers_run(0, 0, S, sl ? s : NULL, sl, cap ? out[2] : NULL, cap, &n[2], tab[2], room, &m[2], &r[2], NULL);
        if (rc[0] != MI355_OK && rc[0] != MI355_E_DATA && rc[0] != MI355_E_OUT_TOO_SMALL) {
            fprintf(stderr, "case %u: unexpected return %d\n", i, rc[0]);
            return 1;
        }
        const uint64_t held = n[0] < cap ? n[0] : cap;
        for (int k = 1; k < 3; k++) {
            bool same = rc[k] == rc[0] && n[k] == n[0] && m[k] == m[0] && m[0] <= room && memcmp(&r[k], &r[0], sizeof r[0]) == 0 &&
                        memcmp(out[k], out[0], held) == 0;
            for (uint64_t j = 0; same && j < m[0]; j++) {
                mi355_member_info a = tab[k][j], b = tab[0][j];
                hinted += k == 1 && (a.flags & MI355_MEMBER_HINTED);
                a.flags = b.flags = 0;
                same = memcmp(&a, &b, sizeof a) == 0;
            }
            if (!same) {
                fprintf(stderr, "case %u: the call (%s finder) differs from the serial walk (rc %d / %d, status %u / %u, out_pos %llu / %llu, members %llu / %llu)\n",
                        i, k == 1 ? "lanes" : "plain", rc[0], rc[k], r[0].status, r[k].status, (unsigned long long)r[0].out_pos,
                        (unsigned long long)r[k].out_pos, (unsigned long long)m[0], (unsigned long long)m[k]);
                return 1;
            }
        }
        walked += m[0];
        if (r[0].status < 13) by_status[r[0].status]++;
        if (rc[0] == MI355_E_OUT_TOO_SMALL) small++;
        free(s);
        for (int k = 0; k < 3; k++) free(out[k]), free(tab[k]);
    }
    fclose(f);
    printf("%u cases:", count);
    for (int k = 0; k < 13; k++) printf(" %llu", by_status[k]);
    printf("; %llu too small; %llu members, %llu hinted\n", small, walked, hinted);
    return 0;
}
