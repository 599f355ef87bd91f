// Stand-alone sanitizer run of the cuts of a seek handle (TEST INFRASTRUCTURE): reads a corpus file of (stream, wrapper, table,
// spacing, group size, cut_bytes, damaged stream, ranges) cases, builds the handle with the host build of inflate_cut.h -- lane by
// lane and by the serial model -- and reads every range, one by one and as one batch, built with -fsanitize=address,undefined.  The
// stream, the table, every range's buffer, the slots of every group's cuts and the symbols and windows of every launch set are
// exact-size heap allocations: a cut stored outside its entry's slots, a flatten load or store outside the set's symbols, a store
// in front of or behind a range's buffer is reported.  The bytes read from an undamaged stream are compared with `want`.  Exit
// status 0: every case ran clean.
//
// Corpus file: "ICC1", u32 count, then per case u32 wrapper, u64 stream_len, u64 spacing, u64 group_bytes, u64 cut_bytes, u64 n,
// u64 want_len, u64 n_ranges, u32 damaged, n x (u64 bit_start, u64 in_bytes), the stream, [the damaged stream, stream_len bytes],
// want_len bytes, n_ranges x (u64 off, u64 len); all little endian.  The build runs on the stream, the reads on the damaged one.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/mi355_deflate.h"

extern "C" void* inflcut_build(int mutant, int serial, const uint8_t* stream, uint64_t stream_len, int wrapper, const uint64_t* bit_start,
                               const uint64_t* in_bytes, uint64_t n, uint64_t spacing, uint64_t group_bytes, uint64_t cut_bytes, int* rc,
                               mi355_inflate_report* report);
extern "C" void inflcut_free(void* h);
extern "C" int inflcut_read(void* hv, const uint8_t* stream, uint64_t stream_len, const uint64_t* off, const uint64_t* len, const uint64_t* out_at,
                            uint64_t n, uint64_t budget, uint8_t* out, uint64_t* got, mi355_inflate_report* reports, uint64_t counts[4],
                            uint64_t cut_counts[4]);
extern "C" uint64_t inflcut_bad_loads(void);

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
    if (!rd(f, magic, 4) || memcmp(magic, "ICC1", 4) != 0 || !rd(f, &count, 4)) {
        fprintf(stderr, "not a corpus file\n");
        return 2;
    }
    unsigned long long built = 0, refused = 0, reads = 0, bad_reads = 0;
    for (uint32_t i = 0; i < count; i++) {
        uint32_t wrapper, damaged;
        uint64_t sl, spacing, group, cb, n, wl, nr;
        if (!rd(f, &wrapper, 4) || !rd(f, &sl, 8) || !rd(f, &spacing, 8) || !rd(f, &group, 8) || !rd(f, &cb, 8) || !rd(f, &n, 8) || !rd(f, &wl, 8) ||
            !rd(f, &nr, 8) || !rd(f, &damaged, 4) || sl > (1ull << 31) || wl > (1ull << 31) || n > (1ull << 24) || nr > (1ull << 20)) {
            fprintf(stderr, "case %u: bad record\n", i);
            return 2;
        }
        uint64_t* bits = (uint64_t*)malloc(n ? n * 8 : 1);
        uint64_t* bytes = (uint64_t*)malloc(n ? n * 8 : 1);
        uint8_t* s = (uint8_t*)malloc(sl ? sl : 1);
        uint8_t* d = (uint8_t*)malloc(sl ? sl : 1);
        uint8_t* want = (uint8_t*)malloc(wl ? wl : 1);
        uint64_t* off = (uint64_t*)malloc(nr ? nr * 8 : 1);
        uint64_t* len = (uint64_t*)malloc(nr ? nr * 8 : 1);
        bool ok = bits && bytes && s && d && want && off && len;
        for (uint64_t k = 0; ok && k < n; k++) ok = rd(f, bits + k, 8) && rd(f, bytes + k, 8);
        ok = ok && rd(f, s, sl) && (!damaged || rd(f, d, sl)) && rd(f, want, wl);
        for (uint64_t k = 0; ok && k < nr; k++) ok = rd(f, off + k, 8) && rd(f, len + k, 8) && len[k] <= (1ull << 31);
        if (!ok) {
            fprintf(stderr, "case %u: short file\n", i);
            return 2;
        }
        if (!damaged) memcpy(d, s, sl);
        for (int serial = 0; serial < 2; serial++) {
            mi355_inflate_report r;
            memset(&r, 0, sizeof r);
            int rc = 0;
            void* h = inflcut_build(0, serial, sl ? s : NULL, sl, (int)wrapper, bits, bytes, n, spacing, group, cb, &rc, &r);
            if (!h) {
                if (rc != MI355_E_DATA && rc != MI355_E_ARG) {
                    fprintf(stderr, "case %u: unexpected return %d of the build\n", i, rc);
                    return 1;
                }
                refused++;
                continue;
            }
            built++;
            // one by one, each range into a buffer of its own exact size ...
            for (uint64_t k = 0; k < nr; k++) {
                uint8_t* out = (uint8_t*)malloc(len[k] ? len[k] : 1);
                const uint64_t at = 0;
                uint64_t got = 0, counts[4], cc[4];
                mi355_inflate_report q;
                if (!out) return 2;
                memset(out, 0xA5, len[k] ? len[k] : 1);
                rc = inflcut_read(h, sl ? d : NULL, sl, off + k, len + k, &at, 1, group, len[k] ? out : NULL, &got, &q, counts, cc);
                reads++;
                if (rc != MI355_OK && rc != MI355_E_DATA) {
                    fprintf(stderr, "case %u range %llu: unexpected return %d\n", i, (unsigned long long)k, rc);
                    return 1;
                }
                if (rc == MI355_E_DATA) bad_reads++;
                const uint64_t full = off[k] >= wl ? 0 : (len[k] < wl - off[k] ? len[k] : wl - off[k]);
                if (got > full || (rc == MI355_OK && got != full) || (!damaged && (rc != MI355_OK || memcmp(out, want + (got ? off[k] : 0), got) != 0))) {
                    fprintf(stderr, "case %u range %llu: rc %d, %llu bytes of %llu, or other bytes than the stream's\n", i, (unsigned long long)k, rc,
                            (unsigned long long)got, (unsigned long long)full);
                    return 1;
                }
                for (uint64_t b = got; b < len[k]; b++)
                    if (out[b] != 0xA5) {
                        fprintf(stderr, "case %u range %llu: a store behind the bytes that hold data\n", i, (unsigned long long)k);
                        return 1;
                    }
                free(out);
            }
            // ... and all of them as one batch, back to back in one buffer
            uint64_t sum = 0;
            uint64_t* at = (uint64_t*)malloc(nr ? nr * 8 : 1);
            uint64_t* got = (uint64_t*)malloc(nr ? nr * 8 : 1);
            mi355_inflate_report* q = (mi355_inflate_report*)malloc(nr ? nr * sizeof(mi355_inflate_report) : 1);
            if (!at || !got || !q) return 2;
            for (uint64_t k = 0; k < nr; k++) at[k] = sum, sum += len[k];
            uint8_t* out = (uint8_t*)malloc(sum ? sum : 1);
            uint64_t counts[4], cc[4];
            if (!out) return 2;
            rc = inflcut_read(h, sl ? d : NULL, sl, off, len, at, nr, group, out, got, q, counts, cc);
            if (rc != MI355_OK && rc != MI355_E_DATA) {
                fprintf(stderr, "case %u: unexpected return %d of the batch\n", i, rc);
                return 1;
            }
            for (uint64_t k = 0; k < nr; k++)
                if (!damaged && memcmp(out + at[k], want + (got[k] ? off[k] : 0), got[k]) != 0) {
                    fprintf(stderr, "case %u range %llu: the batch gives other bytes than the stream's\n", i, (unsigned long long)k);
                    return 1;
                }
            free(at), free(got), free(q), free(out);
            inflcut_free(h);
        }
        free(bits), free(bytes), free(s), free(d), free(want), free(off), free(len);
    }
    fclose(f);
    if (inflcut_bad_loads()) {
        fprintf(stderr, "%llu symbol loads in front of a fence\n", (unsigned long long)inflcut_bad_loads());
        return 1;
    }
    printf("%u cases: %llu built, %llu refused, %llu reads, %llu of them failed\n", count, built, refused, reads, bad_reads);
    return 0;
}
