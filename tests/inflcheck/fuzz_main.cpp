// Stand-alone sanitizer run of the verify decisions (TEST INFRASTRUCTURE): reads a corpus file of (stream, input, wrapper) cases and
// runs the host build of inflate_check.h over each, built with -fsanitize=address,undefined.  Every buffer is an exact-size heap
// allocation, so a read one byte outside the stream or the input is reported.  Exit status 0: every case ran clean.
//
// Corpus file: "IFC1", u32 count, then per case u32 wrapper, u64 stream_len, u64 in_len, u64 n_table, the stream, the input,
// n_table x (u64 bit_start, u64 in_bytes); all little endian.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/mi355_deflate.h"

extern "C" int inflcheck_verify(const uint8_t* stream, uint64_t stream_len, const uint8_t* in, uint64_t in_len, int wrapper,
                                const uint64_t* bit_start, const uint64_t* in_bytes, uint64_t n, mi355_verify_report* report);

extern "C" int inflcheck_verify_lanes(const uint8_t* stream, uint64_t stream_len, const uint8_t* in, uint64_t in_len, int wrapper,
                                      const uint64_t* bit_start, const uint64_t* in_bytes, uint64_t n, mi355_verify_report* report);

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
    if (!rd(f, magic, 4) || memcmp(magic, "IFC1", 4) != 0 || !rd(f, &count, 4)) {
        fprintf(stderr, "not a corpus file\n");
        return 2;
    }
    unsigned long long by_status[13] = {0};
    for (uint32_t i = 0; i < count; i++) {
        uint32_t wrapper;
        uint64_t sl, il, nt;
        if (!rd(f, &wrapper, 4) || !rd(f, &sl, 8) || !rd(f, &il, 8) || !rd(f, &nt, 8) || sl > (1ull << 31) || il > (1ull << 31) ||
            nt > (1ull << 24)) {
            fprintf(stderr, "case %u: bad record\n", i);
            return 2;
        }
        // exact-size allocations (malloc(0) may be null: one byte then, never read by a correct decoder)
        uint8_t* s = (uint8_t*)malloc(sl ? sl : 1);
        uint8_t* in = (uint8_t*)malloc(il ? il : 1);
        uint64_t* tab = (uint64_t*)malloc(nt ? nt * 16 : 1);
        if (!s || !in || !tab || !rd(f, s, sl) || !rd(f, in, il) || !rd(f, tab, nt * 16)) {
            fprintf(stderr, "case %u: short file\n", i);
            return 2;
        }
        uint64_t* bs = (uint64_t*)malloc(nt ? nt * 8 : 1);
        uint64_t* ib = (uint64_t*)malloc(nt ? nt * 8 : 1);
        for (uint64_t k = 0; k < nt; k++) bs[k] = tab[2 * k], ib[k] = tab[2 * k + 1];
        mi355_verify_report r;
        memset(&r, 0, sizeof r);
        const int rc = inflcheck_verify(sl ? s : NULL, sl, il ? in : NULL, il, (int)wrapper, bs, ib, nt, &r);
        if (rc != MI355_OK && rc != MI355_E_VERIFY && rc != MI355_E_ARG) {
            fprintf(stderr, "case %u: unexpected return %d\n", i, rc);
            return 1;
        }
        // the same case with the compares done lane by lane, the kernel's way: the same report
        mi355_verify_report q;
        memset(&q, 0, sizeof q);
        const int rc2 = inflcheck_verify_lanes(sl ? s : NULL, sl, il ? in : NULL, il, (int)wrapper, bs, ib, nt, &q);
        if (rc2 != rc || memcmp(&q, &r, sizeof r) != 0) {
            fprintf(stderr, "case %u: lane by lane the report differs (status %u / %u, in_pos %llu / %llu)\n", i, r.status, q.status,
                    (unsigned long long)r.in_pos, (unsigned long long)q.in_pos);
            return 1;
        }
        if (r.status < 13) by_status[r.status]++;
        free(s), free(in), free(tab), free(bs), free(ib);
    }
    fclose(f);
    printf("%u cases:", count);
    for (int k = 0; k < 13; k++) printf(" %llu", by_status[k]);
    printf("\n");
    return 0;
}
