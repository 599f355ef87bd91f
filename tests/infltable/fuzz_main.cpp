// Stand-alone sanitizer run of the tabled inflate (TEST INFRASTRUCTURE): reads a corpus file of (stream, wrapper, table, group size,
// out_cap) cases and runs the host builds of inflate_table.h over each -- the serial model and the three passes -- built with
// -fsanitize=address,undefined.  The stream, the table and the output are exact-size heap allocations, and so are the symbols and
// the windows of every group inside the three-pass build: a read one byte outside the stream, or a store or a load one element
// outside what a group holds, is reported.  Exit status 0: every case ran clean and both builds agree.
//
// Corpus file: "ITC1", u32 count, then per case u32 wrapper, u64 stream_len, u64 out_cap, u64 group_bytes, u64 n, n x (u64 bit_start,
// u64 in_bytes), the stream; all little endian.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/mi355_deflate.h"

extern "C" int infltable_inflate(int mode, const uint8_t* stream, uint64_t stream_len, int wrapper, const uint64_t* bit_start,
                                 const uint64_t* in_bytes, uint64_t n, uint64_t group_bytes, uint8_t* out, uint64_t out_cap, uint64_t* out_len,
                                 mi355_inflate_report* report);
extern "C" uint64_t infltable_unfenced_loads(void);

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
    if (!rd(f, magic, 4) || memcmp(magic, "ITC1", 4) != 0 || !rd(f, &count, 4)) {
        fprintf(stderr, "not a corpus file\n");
        return 2;
    }
    unsigned long long by_status[13] = {0}, small = 0;
    for (uint32_t i = 0; i < count; i++) {
        uint32_t wrapper;
        uint64_t sl, cap, group, n;
        if (!rd(f, &wrapper, 4) || !rd(f, &sl, 8) || !rd(f, &cap, 8) || !rd(f, &group, 8) || !rd(f, &n, 8) || sl > (1ull << 31) ||
            cap > (1ull << 31) || n > (1ull << 24)) {
            fprintf(stderr, "case %u: bad record\n", i);
            return 2;
        }
        // exact-size allocations (malloc(0) may be null: one byte then, never touched by a correct decoder -- the pointer handed over is NULL)
        uint64_t* bits = (uint64_t*)malloc(n ? n * 8 : 1);
        uint64_t* bytes = (uint64_t*)malloc(n ? n * 8 : 1);
        uint8_t* s = (uint8_t*)malloc(sl ? sl : 1);
        uint8_t* a = (uint8_t*)malloc(cap ? cap : 1);
        uint8_t* b = (uint8_t*)malloc(cap ? cap : 1);
        bool ok = bits && bytes && s && a && b;
        for (uint64_t k = 0; ok && k < n; k++) ok = rd(f, bits + k, 8) && rd(f, bytes + k, 8);
        if (!ok || !rd(f, s, sl)) {
            fprintf(stderr, "case %u: short file\n", i);
            return 2;
        }
        memset(a, 0xA5, cap ? cap : 1), memset(b, 0xA5, cap ? cap : 1);
        mi355_inflate_report r, q;
        memset(&r, 0, sizeof r), memset(&q, 0, sizeof q);
        uint64_t n1 = 0, n2 = 0;
        const int rc = infltable_inflate(0, sl ? s : NULL, sl, (int)wrapper, bits, bytes, n, group, cap ? a : NULL, cap, &n1, &r);
        if (rc != MI355_OK && rc != MI355_E_DATA && rc != MI355_E_OUT_TOO_SMALL) {
            fprintf(stderr, "case %u: unexpected return %d\n", i, rc);
            return 1;
        }
        const int rc2 = infltable_inflate(1, sl ? s : NULL, sl, (int)wrapper, bits, bytes, n, group, cap ? b : NULL, cap, &n2, &q);
        if (rc2 != rc || n1 != n2 || memcmp(&q, &r, sizeof r) != 0 || memcmp(a, b, cap) != 0) {
            fprintf(stderr, "case %u: the three passes differ from the serial model (rc %d / %d, status %u / %u, out_pos %llu / %llu)\n", i, rc,
                    rc2, r.status, q.status, (unsigned long long)r.out_pos, (unsigned long long)q.out_pos);
            return 1;
        }
        if (r.status < 13) by_status[r.status]++;
        if (rc == MI355_E_OUT_TOO_SMALL) small++;
        free(bits), free(bytes), free(s), free(a), free(b);
    }
    fclose(f);
    if (infltable_unfenced_loads()) {
        fprintf(stderr, "%llu symbol loads in front of a fence\n", (unsigned long long)infltable_unfenced_loads());
        return 1;
    }
    printf("%u cases:", count);
    for (int k = 0; k < 13; k++) printf(" %llu", by_status[k]);
    printf("; %llu too small\n", small);
    return 0;
}
