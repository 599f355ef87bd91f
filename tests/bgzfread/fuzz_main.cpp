// Stand-alone sanitizer run of the BGZF reads (TEST INFRASTRUCTURE): reads a corpus file of (file, damaged file, scratch budget,
// ranges) cases, builds the index with the host build of bgzf_read.h from the file's own claims and reads every range from the
// damaged file (or the file itself) -- one by one and as one batch --, built with -fsanitize=address,undefined.  The file and every
// range's buffer are exact-size heap allocations, and so are the scratch slots of every launch set inside the host build: a read one
// byte outside the file, a store in front of or behind a range's buffer, or a load outside a set's padded slots, is reported.  The
// bytes read from an undamaged file are compared with `want`, the file's whole output as the corpus file states it.  Exit status 0:
// every case ran clean.
//
// Corpus file: "BRC1", u32 count, then per case u64 file_len, u64 budget, u64 want_len, u64 n_ranges, u32 damaged, the file, [the
// damaged file, file_len bytes], want_len bytes, n_ranges x (u64 off, u64 len); all little endian.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/mi355_deflate.h"

extern "C" void* bgzfread_build(const uint8_t* file, uint64_t file_len, uint64_t S, int* rc, mi355_inflate_report* report);
extern "C" void bgzfread_free(void* h);
extern "C" int bgzfread_read(void* hv, int mutant, const uint8_t* file, uint64_t file_len, const uint64_t* off, const uint64_t* len,
                             const uint64_t* out_at, uint64_t n, uint64_t budget, uint8_t* out, uint64_t* got, int32_t* status,
                             mi355_inflate_report* reports, uint64_t counts[5]);
extern "C" uint64_t bgzfread_unfenced_loads(void);

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
    if (!rd(f, magic, 4) || memcmp(magic, "BRC1", 4) != 0 || !rd(f, &count, 4)) {
        fprintf(stderr, "not a corpus file\n");
        return 2;
    }
    unsigned long long built = 0, refused = 0, reads = 0, bad_reads = 0;
    for (uint32_t i = 0; i < count; i++) {
        uint32_t damaged;
        uint64_t fl, budget, wl, nr;
        if (!rd(f, &fl, 8) || !rd(f, &budget, 8) || !rd(f, &wl, 8) || !rd(f, &nr, 8) || !rd(f, &damaged, 4) || fl > (1ull << 31) || wl > (1ull << 31) ||
            nr > (1ull << 20)) {
            fprintf(stderr, "case %u: bad record\n", i);
            return 2;
        }
        uint8_t* s = (uint8_t*)malloc(fl ? fl : 1);
        uint8_t* d = (uint8_t*)malloc(fl ? fl : 1);
        uint8_t* want = (uint8_t*)malloc(wl ? wl : 1);
        uint64_t* off = (uint64_t*)malloc(nr ? nr * 8 : 1);
        uint64_t* len = (uint64_t*)malloc(nr ? nr * 8 : 1);
        bool ok = s && d && want && off && len;
        ok = ok && rd(f, s, fl) && (!damaged || rd(f, d, fl)) && rd(f, want, wl);
        for (uint64_t k = 0; ok && k < nr; k++) ok = rd(f, off + k, 8) && rd(f, len + k, 8) && len[k] <= (1ull << 31);
        if (!ok) {
            fprintf(stderr, "case %u: short file\n", i);
            return 2;
        }
        if (!damaged) memcpy(d, s, fl);
        mi355_inflate_report r;
        int rc = 0;
        void* h = bgzfread_build(fl ? s : NULL, fl, 65536, &rc, &r);
        if (!h) {
            if (rc != MI355_E_DATA) {
                fprintf(stderr, "case %u: unexpected return %d of the build\n", i, rc);
                return 1;
            }
            refused++;
        } else {
            built++;
            // one by one, each range into a buffer of its own exact size ...
            for (uint64_t k = 0; k < nr; k++) {
                uint8_t* out = (uint8_t*)malloc(len[k] ? len[k] : 1);
                const uint64_t at = 0;
                uint64_t got = 0, counts[5];
                int32_t st = 0;
                mi355_inflate_report q;
                if (!out) return 2;
                memset(out, 0xA5, len[k] ? len[k] : 1);
                rc = bgzfread_read(h, 0, d, fl, off + k, len + k, &at, 1, budget, len[k] ? out : NULL, &got, &st, &q, counts);
                reads++;
                if ((rc != MI355_OK && rc != MI355_E_DATA) || rc != st) {
                    fprintf(stderr, "case %u range %llu: unexpected return %d\n", i, (unsigned long long)k, rc);
                    return 1;
                }
                if (rc == MI355_E_DATA) bad_reads++;
                const uint64_t full = off[k] >= wl ? 0 : (len[k] < wl - off[k] ? len[k] : wl - off[k]);
                if (got > len[k] || (rc == MI355_OK && got != full) || (!damaged && (rc != MI355_OK || memcmp(out, want + (got ? off[k] : 0), got) != 0))) {
                    fprintf(stderr, "case %u range %llu: rc %d, %llu bytes of %llu, or other bytes than the file's\n", i, (unsigned long long)k, rc,
                            (unsigned long long)got, (unsigned long long)full);
                    return 1;
                }
                free(out);
            }
            // ... and all of them as one batch, back to back in one buffer
            uint64_t sum = 0;
            uint64_t* at = (uint64_t*)malloc(nr ? nr * 8 : 1);
            uint64_t* got = (uint64_t*)malloc(nr ? nr * 8 : 1);
            int32_t* st = (int32_t*)malloc(nr ? nr * 4 : 1);
            mi355_inflate_report* q = (mi355_inflate_report*)malloc(nr ? nr * sizeof(mi355_inflate_report) : 1);
            if (!at || !got || !st || !q) return 2;
            for (uint64_t k = 0; k < nr; k++) at[k] = sum, sum += len[k];
            uint8_t* out = (uint8_t*)malloc(sum ? sum : 1);
            uint64_t counts[5];
            if (!out) return 2;
            rc = bgzfread_read(h, 0, d, fl, off, len, at, nr, budget, out, got, st, q, counts);
            if (rc != MI355_OK && rc != MI355_E_DATA) {
                fprintf(stderr, "case %u: unexpected return %d of the batch\n", i, rc);
                return 1;
            }
            for (uint64_t k = 0; k < nr; k++)
                if (!damaged && (st[k] != MI355_OK || memcmp(out + at[k], want + (got[k] ? off[k] : 0), got[k]) != 0)) {
                    fprintf(stderr, "case %u range %llu: the batch gives other bytes than the file's\n", i, (unsigned long long)k);
                    return 1;
                }
            free(at), free(got), free(st), free(q), free(out);
            bgzfread_free(h);
        }
        free(s), free(d), free(want), free(off), free(len);
    }
    fclose(f);
    if (bgzfread_unfenced_loads()) {
        fprintf(stderr, "%llu loads in front of a fence\n", (unsigned long long)bgzfread_unfenced_loads());
        return 1;
    }
    printf("%u cases: %llu built, %llu refused, %llu reads, %llu of them failed\n", count, built, refused, reads, bad_reads);
    return 0;
}
