// Stand-alone sanitizer run of the inflate decisions (TEST INFRASTRUCTURE): reads a corpus file of (stream, wrapper, out_cap) cases and
// runs the host build of inflate_write.h over each, scalar and lane by lane, built with -fsanitize=address,undefined.  The stream and
// the output are exact-size heap allocations -- out_cap bytes for the output --, so a read one byte outside the stream, or a store or
// a load one byte outside out[0, out_cap), is reported.  Exit status 0: every case ran clean and both sinks agree.
//
// Corpus file: "IWC1", u32 count, then per case u32 wrapper, u64 stream_len, u64 out_cap, the stream; all little endian.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/mi355_deflate.h"

extern "C" int inflwrite_inflate(const uint8_t* stream, uint64_t stream_len, int wrapper, uint8_t* out, uint64_t out_cap, uint64_t* out_len,
                                 mi355_inflate_report* report);
extern "C" int inflwrite_inflate_lanes(const uint8_t* stream, uint64_t stream_len, int wrapper, uint8_t* out, uint64_t out_cap,
                                       uint64_t* out_len, mi355_inflate_report* report);
extern "C" uint64_t inflwrite_unfenced_loads(void);

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
    if (!rd(f, magic, 4) || memcmp(magic, "IWC1", 4) != 0 || !rd(f, &count, 4)) {
        fprintf(stderr, "not a corpus file\n");
        return 2;
    }
    unsigned long long by_status[13] = {0}, small = 0;
    for (uint32_t i = 0; i < count; i++) {
        uint32_t wrapper;
        uint64_t sl, cap;
        if (!rd(f, &wrapper, 4) || !rd(f, &sl, 8) || !rd(f, &cap, 8) || sl > (1ull << 31) || cap > (1ull << 31)) {
            fprintf(stderr, "case %u: bad record\n", i);
            return 2;
        }
        // exact-size allocations (malloc(0) may be null: one byte then, never touched by a correct decoder -- the pointer handed over is NULL)
        uint8_t* s = (uint8_t*)malloc(sl ? sl : 1);
        uint8_t* a = (uint8_t*)malloc(cap ? cap : 1);
        uint8_t* b = (uint8_t*)malloc(cap ? cap : 1);
        if (!s || !a || !b || !rd(f, s, sl)) {
            fprintf(stderr, "case %u: short file\n", i);
            return 2;
        }
        memset(a, 0xA5, cap ? cap : 1), memset(b, 0xA5, cap ? cap : 1);
        mi355_inflate_report r, q;
        memset(&r, 0, sizeof r), memset(&q, 0, sizeof q);
        uint64_t n1 = 0, n2 = 0;
        const int rc = inflwrite_inflate(sl ? s : NULL, sl, (int)wrapper, cap ? a : NULL, cap, &n1, &r);
        if (rc != MI355_OK && rc != MI355_E_DATA && rc != MI355_E_OUT_TOO_SMALL) {
            fprintf(stderr, "case %u: unexpected return %d\n", i, rc);
            return 1;
        }
        const int rc2 = inflwrite_inflate_lanes(sl ? s : NULL, sl, (int)wrapper, cap ? b : NULL, cap, &n2, &q);
        if (rc2 != rc || n1 != n2 || memcmp(&q, &r, sizeof r) != 0 || memcmp(a, b, cap) != 0) {
            fprintf(stderr, "case %u: lane by lane the result differs (rc %d / %d, status %u / %u, out_pos %llu / %llu)\n", i, rc, rc2, r.status,
                    q.status, (unsigned long long)r.out_pos, (unsigned long long)q.out_pos);
            return 1;
        }
        if (r.status < 13) by_status[r.status]++;
        if (rc == MI355_E_OUT_TOO_SMALL) small++;
        free(s), free(a), free(b);
    }
    fclose(f);
    if (inflwrite_unfenced_loads()) {
        fprintf(stderr, "%llu loads of the output in front of a fence\n", (unsigned long long)inflwrite_unfenced_loads());
        return 1;
    }
    printf("%u cases:", count);
    for (int k = 0; k < 13; k++) printf(" %llu", by_status[k]);
    printf("; %llu too small\n", small);
    return 0;
}
