// Stand-alone sanitizer run of the inflate index (TEST INFRASTRUCTURE): reads a corpus file of (stream, wrapper, span size, group
// size, out_cap) cases and runs the host build of inflate_index.h over each, built with -fsanitize=address,undefined.  The stream,
// the candidates and the walkers' records are exact-size heap allocations: a read one byte outside the stream, or a candidate or a
// record one element outside its array, is reported.  Per case: the finder with its prefilter against the plain predicate
// (candidates and records must be equal), then the combined call against the table-less inflate (return value, length, report and
// bytes must be equal).  Exit status 0: every case ran clean and agreed.
//
// Corpus file: "IXC1", u32 count, then per case u32 wrapper, u64 stream_len, u64 out_cap, u64 span_bytes, u64 group_bytes, the stream;
// all little endian.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/mi355_deflate.h"

extern "C" uint64_t inflindex_n_spans(uint64_t stream_len, uint64_t S);
extern "C" int inflindex_scan(int mutant, int lanes, const uint8_t* stream, uint64_t stream_len, int wrapper, uint64_t S, uint64_t* cand,
                              mi355_index_walk* recs);
extern "C" int inflindex_parallel(int mutant, const uint8_t* stream, uint64_t stream_len, int wrapper, uint64_t S, uint64_t group_bytes,
                                  uint8_t* out, uint64_t out_cap, uint64_t* out_len, mi355_inflate_report* report);
extern "C" int infltable_inflate(int mode, const uint8_t* stream, uint64_t stream_len, int wrapper, const uint64_t* bit_start,
                                 const uint64_t* in_bytes, uint64_t n, uint64_t group_bytes, uint8_t* out, uint64_t out_cap, uint64_t* out_len,
                                 mi355_inflate_report* report);

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
    if (!rd(f, magic, 4) || memcmp(magic, "IXC1", 4) != 0 || !rd(f, &count, 4)) {
        fprintf(stderr, "not a corpus file\n");
        return 2;
    }
    unsigned long long by_status[13] = {0}, small = 0, walkers = 0;
    for (uint32_t i = 0; i < count; i++) {
        uint32_t wrapper;
        uint64_t sl, cap, S, group;
        if (!rd(f, &wrapper, 4) || !rd(f, &sl, 8) || !rd(f, &cap, 8) || !rd(f, &S, 8) || !rd(f, &group, 8) || sl > (1ull << 31) ||
            cap > (1ull << 31) || S < 256) {
            fprintf(stderr, "case %u: bad record\n", i);
            return 2;
        }
        const uint64_t n = inflindex_n_spans(sl, S);
        // exact-size allocations (malloc(0) may be null: one byte then, never touched by a correct decoder -- the pointer handed over is NULL)
        uint8_t* s = (uint8_t*)malloc(sl ? sl : 1);
        uint8_t* a = (uint8_t*)malloc(cap ? cap : 1);
        uint8_t* b = (uint8_t*)malloc(cap ? cap : 1);
        uint64_t* c0 = (uint64_t*)malloc(n * 8);
        uint64_t* c1 = (uint64_t*)malloc(n * 8);
        mi355_index_walk* w0 = (mi355_index_walk*)malloc(n * sizeof(mi355_index_walk));
        mi355_index_walk* w1 = (mi355_index_walk*)malloc(n * sizeof(mi355_index_walk));
        if (!s || !a || !b || !c0 || !c1 || !w0 || !w1 || !rd(f, s, sl)) {
            fprintf(stderr, "case %u: short file\n", i);
            return 2;
        }
        memset(w0, 0, n * sizeof(mi355_index_walk)), memset(w1, 0, n * sizeof(mi355_index_walk));
        if (inflindex_scan(0, 0, sl ? s : NULL, sl, (int)wrapper, S, c0, w0) != MI355_OK ||
            inflindex_scan(0, 1, sl ? s : NULL, sl, (int)wrapper, S, c1, w1) != MI355_OK) {
            fprintf(stderr, "case %u: the scan was refused\n", i);
            return 1;
        }
        if (memcmp(c0, c1, n * 8) != 0 || memcmp(w0, w1, n * sizeof(mi355_index_walk)) != 0) {
            fprintf(stderr, "case %u: the prefiltered finder differs from the plain predicate\n", i);
            return 1;
        }
        for (uint64_t k = 0; k < n; k++) walkers += c0[k] != UINT64_MAX;
        memset(a, 0xA5, cap ? cap : 1), memset(b, 0xA5, cap ? cap : 1);
        mi355_inflate_report r, q;
        memset(&r, 0, sizeof r), memset(&q, 0, sizeof q);
        uint64_t n1 = 0, n2 = 0;
        const int rc = infltable_inflate(1, sl ? s : NULL, sl, (int)wrapper, NULL, NULL, 0, group, cap ? a : NULL, cap, &n1, &r);
        if (rc != MI355_OK && rc != MI355_E_DATA && rc != MI355_E_OUT_TOO_SMALL) {
            fprintf(stderr, "case %u: unexpected return %d\n", i, rc);
            return 1;
        }
        const int rc2 = inflindex_parallel(0, sl ? s : NULL, sl, (int)wrapper, S, group, cap ? b : NULL, cap, &n2, &q);
        if (rc2 != rc || n1 != n2 || memcmp(&q, &r, sizeof r) != 0 || memcmp(a, b, cap) != 0) {
            fprintf(stderr, "case %u: the parallel inflate differs from the inflate (rc %d / %d, status %u / %u, out_pos %llu / %llu)\n", i, rc,
                    rc2, r.status, q.status, (unsigned long long)r.out_pos, (unsigned long long)q.out_pos);
            return 1;
        }
        if (r.status < 13) by_status[r.status]++;
        if (rc == MI355_E_OUT_TOO_SMALL) small++;
        free(s), free(a), free(b), free(c0), free(c1), free(w0), free(w1);
    }
    fclose(f);
    printf("%u cases:", count);
    for (int k = 0; k < 13; k++) printf(" %llu", by_status[k]);
    printf("; %llu too small; %llu walkers\n", small, walkers);
    return 0;
}
