// Stand-alone sanitizer run of the stream-inflate decisions (TEST INFRASTRUCTURE): reads a corpus file of (stream, wrapper, dict, split,
// caps) cases and drives the handle model of inflstream.cpp over each, scalar and lane by lane, built with
// -fsanitize=address,undefined.  Every piece and every output buffer is an exact-size heap allocation, and so are the model's pending
// bytes and histories, so a read one byte outside the pending bytes or a history, or a store or a load one byte outside out[0, cap),
// is reported.  A write that finds its room too small is repeated once with the room the state names.  Exit status 0: every case ran
// clean and both sinks agree.
//
// Corpus file: "ISC1", u32 count, then per case u32 wrapper, u32 n_pieces, u64 stream_len, u64 dict_len, the stream, the dictionary,
// and per piece u64 length, u64 cap; all little endian.  The pieces' lengths sum to stream_len.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/mi355_deflate.h"

extern "C" void* ism_new(int wrapper, const uint8_t* dict, uint64_t dict_len, int lanes);
extern "C" int ism_write(void* p, const uint8_t* in, uint64_t in_len, uint8_t* out, uint64_t cap, uint64_t* out_len, mi355_inflate_report* rep);
extern "C" int ism_finish(void* p, mi355_inflate_report* rep);
extern "C" void ism_state(void* p, mi355_inflate_stream_state* st);
extern "C" void ism_free(void* p);
extern "C" uint64_t ism_unfenced_loads(void);

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

struct Trace {
    std::vector<int> rcs;
    std::vector<uint8_t> bytes;
    mi355_inflate_report last;
};

static bool drive(int lanes, uint32_t wrapper, const uint8_t* s, const uint8_t* dict, uint64_t dict_len, const std::vector<uint64_t>& pieces,
                  Trace& t) {
    void* m = ism_new((int)wrapper, dict_len ? dict : NULL, dict_len, lanes);
    if (!m) return false;
    uint64_t at = 0;
    memset(&t.last, 0, sizeof t.last);
    for (size_t k = 0; k + 1 < pieces.size(); k += 2) {
        const uint64_t n = pieces[k];
        uint64_t cap = pieces[k + 1];
        uint8_t* in = (uint8_t*)malloc(n ? n : 1);
        memcpy(in, s + at, n);
        at += n;
        for (int turn = 0; turn < 2; turn++) {
            uint8_t* out = (uint8_t*)malloc(cap ? cap : 1);
            memset(out, 0xA5, cap ? cap : 1);
            uint64_t got = 0;
            const int rc = ism_write(m, turn || !n ? NULL : in, turn ? 0 : n, cap ? out : NULL, cap, &got, &t.last);
            t.rcs.push_back(rc);
            if (got > cap) {
                fprintf(stderr, "out_len %llu beyond cap %llu\n", (unsigned long long)got, (unsigned long long)cap);
                return false;
            }
            t.bytes.insert(t.bytes.end(), out, out + got);
            free(out);
            if (rc != MI355_E_OUT_TOO_SMALL) break;
            mi355_inflate_stream_state st;
            ism_state(m, &st);
            cap = st.need_out;
        }
        free(in);
    }
    t.rcs.push_back(ism_finish(m, &t.last));
    ism_free(m);
    return true;
}

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
    if (!rd(f, magic, 4) || memcmp(magic, "ISC1", 4) != 0 || !rd(f, &count, 4)) {
        fprintf(stderr, "not a corpus file\n");
        return 2;
    }
    unsigned long long done = 0, dead = 0;
    for (uint32_t i = 0; i < count; i++) {
        uint32_t wrapper, np;
        uint64_t sl, dl;
        if (!rd(f, &wrapper, 4) || !rd(f, &np, 4) || !rd(f, &sl, 8) || !rd(f, &dl, 8) || sl > (1ull << 28) || dl > (1ull << 28) || np > (1u << 20)) {
            fprintf(stderr, "case %u: bad record\n", i);
            return 2;
        }
        uint8_t* s = (uint8_t*)malloc(sl ? sl : 1);
        uint8_t* d = (uint8_t*)malloc(dl ? dl : 1);
        std::vector<uint64_t> pieces(2 * (size_t)np);
        if (!s || !d || !rd(f, s, sl) || !rd(f, d, dl) || !rd(f, pieces.data(), 16 * (size_t)np)) {
            fprintf(stderr, "case %u: short file\n", i);
            return 2;
        }
        uint64_t sum = 0;
        for (uint32_t k = 0; k < np; k++) sum += pieces[2 * k];
        if (sum != sl) {
            fprintf(stderr, "case %u: the pieces are not the stream\n", i);
            return 2;
        }
        Trace a, b;
        if (!drive(0, wrapper, s, d, dl, pieces, a) || !drive(1, wrapper, s, d, dl, pieces, b)) {
            fprintf(stderr, "case %u: the model refused it\n", i);
            return 1;
        }
        if (a.rcs != b.rcs || a.bytes != b.bytes || memcmp(&a.last, &b.last, sizeof a.last) != 0) {
            fprintf(stderr, "case %u: lane by lane the result differs\n", i);
            return 1;
        }
        if (a.rcs.back() == MI355_OK) done++;
        else dead++;
        free(s), free(d);
    }
    fclose(f);
    if (ism_unfenced_loads()) {
        fprintf(stderr, "%llu loads of the output in front of a fence\n", (unsigned long long)ism_unfenced_loads());
        return 1;
    }
    printf("%u cases: %llu done, %llu not\n", count, done, dead);
    return 0;
}
