/* A plain C program over the C ABI of include/mi355_deflate.h (what the Rust shim of INTEGRATION.md
 * binds): compresses a file on the GPU, or with -d decompresses one.
 *   mi355_deflate_cli [-raw|-zlib|-gzip] [-fast|-default|-best] [-chunk N] [--verify] IN OUT
 *   mi355_deflate_cli --bgzf [--block N] [-fast|-default|-best] [--verify] IN OUT
 *   mi355_deflate_cli -d [--parallel | --chunk N] [-raw|-zlib|-gzip] IN OUT
 *   mi355_deflate_cli -d --members [-gzip] IN OUT
 *   mi355_deflate_cli -d --members --range OFF:LEN [-gzip] IN OUT
 *   mi355_deflate_cli -d --range OFF:LEN [--cut BYTES] [-raw|-zlib|-gzip] IN OUT
 * -chunk N drives the streaming handle (write N bytes at a time) instead of the one-shot call.
 * --verify checks the stream against the input on the GPU before it is written (mi355_deflate_last_blocks +
 * mi355_deflate_verify: what `gzip -t` answers), prints the report and exits with status 3 if it does not inflate to the input.
 * --bgzf writes a BGZF file (mi355_bgzf_encode: what bgzip writes and htslib, `gzip -d` and -d --members read): IN in slices of N bytes
 * (--block N: 1 to 65280, the default), a gzip member that states its size per slice, the end-of-file marker last.  Not together with a
 * format switch, -chunk or -d.  With --verify the file is inflated again on the GPU (mi355_inflate_members) and compared with IN
 * before it is written; exit status 3 if it differs.
 * -d / --decompress inflates IN (a raw, zlib or gzip stream by the format switch) to OUT on the GPU: mi355_inflate once without a
 * buffer for the size, once more for the bytes; exits with status 3 and the report if the stream is not valid.  With --parallel the
 * two calls are mi355_inflate_parallel: the block table of the stream is found on the GPU and every entry decoded by a wave of its own
 * (the way for one large file from anywhere); the result is the same.  With --chunk N the file goes N bytes at a time through a stream
 * handle (mi355_inflate_stream_write: what a receiver of a connection does), every write's bytes straight to OUT; the result is the
 * same, and --chunk does not go with --parallel, --members or --range.  With --members IN is a gzip FILE of any number of members --
 * BGZF, `cat a.gz b.gz` -- and the two calls are mi355_inflate_members (plain -d -gzip takes exactly one member); --members with -raw or -zlib is refused with the usage text.
 * With --range OFF:LEN only the bytes [OFF, OFF + LEN) of what IN inflates to are written (fewer at its end, like pread): a seek index
 * is built (mi355_inflate_seek_build: the table found on the GPU, a window kept every MiB of output) and the range is decoded from the
 * nearest point (mi355_inflate_seek_read); not together with --parallel.  With --members --range IN is a BGZF file: its member index
 * is built from the file's own size fields without decoding anything (mi355_bgzf_index_build) and only the members that hold the
 * range are decoded and verified (mi355_bgzf_read); --cut does not go with it.  With --cut BYTES the index also remembers
 * a cut every BYTES of output inside its table entries (MI355_CFG_INFLATE_SEEK_CUT_BYTES: 64 bytes to 1 GiB) and the read decodes a
 * wave per cut; only together with --range.
 * Build:  gcc -O2 -Iinclude examples/mi355_deflate_cli.c -Ldeflate-rs_amd -lmi355deflate \
 *             -Wl,-rpath,$PWD/deflate-rs_amd -o /tmp/mi355_deflate_cli */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mi355_deflate.h"

static int fail(const char* what, int rc, mi355_deflate_ctx* ctx) {
    fprintf(stderr, "%s: error %d (%s)\n", what, rc, ctx ? mi355_deflate_last_error(ctx) : "");
    return 1;
}

int main(int argc, char** argv) {
    int wrapper = 0, level = 1;
    size_t chunk = 0;
    int verify = 0, decompress = 0, parallel = 0, members = 0, format_given = 0, ranged = 0;
    unsigned long long r_off = 0, r_len = 0, cut = 0;
    int cut_given = 0, bgzf = 0, block_given = 0;
    unsigned long long block = 0;
    int a = 1;
    for (; a < argc && argv[a][0] == '-'; a++) {
        if (!strcmp(argv[a], "-raw")) wrapper = 0, format_given = 1;
        else if (!strcmp(argv[a], "-zlib")) wrapper = 1, format_given = 1;
        else if (!strcmp(argv[a], "-gzip")) wrapper = 2, format_given = 1;
        else if (!strcmp(argv[a], "-fast")) level = 0;
        else if (!strcmp(argv[a], "-default")) level = 1;
        else if (!strcmp(argv[a], "-best")) level = 2;
        else if (!strcmp(argv[a], "--verify") || !strcmp(argv[a], "-verify")) verify = 1;
        else if (!strcmp(argv[a], "-d") || !strcmp(argv[a], "--decompress")) decompress = 1;
        else if (!strcmp(argv[a], "--parallel") || !strcmp(argv[a], "-parallel")) parallel = 1;
        else if (!strcmp(argv[a], "--members") || !strcmp(argv[a], "-members")) members = 1;
        else if ((!strcmp(argv[a], "--range") || !strcmp(argv[a], "-range")) && a + 1 < argc) {
            char* end = NULL;
            r_off = strtoull(argv[++a], &end, 10);
            ranged = end && *end == ':' && end != argv[a] && end[1] ? 1 : -1;
            if (ranged == 1) {
                const char* tail = end + 1;
                r_len = strtoull(tail, &end, 10);
                if (*end) ranged = -1;
            }
        } else if ((!strcmp(argv[a], "--cut") || !strcmp(argv[a], "-cut")) && a + 1 < argc) {
            char* end = NULL;
            cut = strtoull(argv[++a], &end, 10);
            cut_given = end && end != argv[a] && !*end ? 1 : -1;
        } else if (!strcmp(argv[a], "--bgzf") || !strcmp(argv[a], "-bgzf")) bgzf = 1;
        else if ((!strcmp(argv[a], "--block") || !strcmp(argv[a], "-block")) && a + 1 < argc) {
            char* end = NULL;
            block = strtoull(argv[++a], &end, 10);
            block_given = end && end != argv[a] && !*end && block >= 1 && block <= 65280 ? 1 : -1;
        } else if ((!strcmp(argv[a], "-chunk") || !strcmp(argv[a], "--chunk")) && a + 1 < argc) chunk = strtoull(argv[++a], NULL, 10);
        else break;
    }
    /* --members is gzip by definition: another format switch beside it is refused, not ignored */
    if (argc - a != 2 || ((parallel || members || ranged) && !decompress) || (parallel && members) || (members && format_given && wrapper != 2) ||
        ranged < 0 || (ranged && parallel) || cut_given < 0 || (cut_given && (!ranged || members)) || block_given < 0 || (block_given && !bgzf) ||
        (bgzf && (decompress || format_given || chunk)) || (decompress && chunk && (parallel || members || ranged))) {
        fprintf(stderr, "usage: %s [-raw|-zlib|-gzip] [-fast|-default|-best] [-chunk N] [--verify] IN OUT\n       %s --bgzf [--block N] [-fast|-default|-best] [--verify] IN OUT\n       %s -d [--parallel | --chunk N] [-raw|-zlib|-gzip] IN OUT\n       %s -d --members [-gzip] IN OUT\n       %s -d --members --range OFF:LEN [-gzip] IN OUT\n       %s -d --range OFF:LEN [--cut BYTES] [-raw|-zlib|-gzip] IN OUT\n",
                argv[0], argv[0], argv[0], argv[0], argv[0], argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[a], "rb");
    if (!f) return fail("open input", -1, NULL);
    fseek(f, 0, SEEK_END);
    size_t n = (size_t)ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t* in = (uint8_t*)malloc(n ? n : 1);
    if (fread(in, 1, n, f) != n) return fail("read input", -1, NULL);
    fclose(f);

    mi355_deflate_ctx* ctx = NULL;
    int rc = mi355_deflate_ctx_create(0, &ctx);
    if (rc) return fail("mi355_deflate_ctx_create (no GPU? there is no CPU fallback)", rc, NULL);
    if (decompress && chunk) { /* a stream handle, fed N bytes at a time; a block that waits for room gets the room the state names */
        mi355_inflate_stream* is = NULL;
        mi355_inflate_stream_state st;
        mi355_inflate_report r;
        size_t cap = 8 * chunk > 65536 ? 8 * chunk : 65536, total = 0, writes = 0;
        uint8_t* data = (uint8_t*)malloc(cap);
        if (!data) return fail("malloc", -1, NULL);
        rc = mi355_inflate_stream_new(ctx, wrapper, NULL, 0, &is);
        if (rc) return fail("mi355_inflate_stream_new", rc, ctx);
        f = fopen(argv[a + 1], "wb");
        if (!f) return fail("write output", -1, NULL);
        for (size_t i = 0; rc == MI355_OK && (i < n || i == 0); i += chunk) {
            size_t k = n - i < chunk ? n - i : chunk, fed = 0;
            do { /* again without input while a complete block waits for room */
                size_t got = 0;
                rc = mi355_inflate_stream_write(is, fed ? NULL : in + i, fed ? 0 : k, data, cap, &got, &r);
                fed = 1, writes++;
                if (rc != MI355_OK && rc != MI355_E_OUT_TOO_SMALL && rc != MI355_E_DATA) return fail("mi355_inflate_stream_write", rc, ctx);
                if (fwrite(data, 1, got, f) != got) return fail("write output", -1, NULL);
                total += got;
                mi355_inflate_stream_state_get(is, &st);
                if (rc != MI355_E_DATA && st.need_out) {
                    if (st.need_out > cap) {
                        free(data);
                        cap = (size_t)st.need_out;
                        data = (uint8_t*)malloc(cap);
                        if (!data) return fail("malloc", -1, NULL);
                    }
                    rc = MI355_OK;
                }
            } while (rc == MI355_OK && st.need_out);
        }
        if (rc == MI355_OK) rc = mi355_inflate_stream_finish(is, &r);
        fclose(f);
        if (rc == MI355_E_DATA) {
            fprintf(stderr, "inflate: status %u at bit %llu, output byte %llu\n%s\n", r.status, (unsigned long long)r.bit,
                    (unsigned long long)r.out_pos, mi355_deflate_last_error(ctx));
            return 3;
        }
        if (rc) return fail("mi355_inflate_stream_finish", rc, ctx);
        mi355_inflate_stream_state_get(is, &st);
        fprintf(stderr, "%lu -> %lu bytes in %lu writes of %lu bytes, checksum %08x\n", (unsigned long)n, (unsigned long)total, (unsigned long)writes,
                (unsigned long)chunk, st.adler_or_crc);
        mi355_inflate_stream_free(is);
        free(data);
        free(in);
        mi355_deflate_ctx_destroy(ctx);
        return 0;
    }
    if (decompress && members && ranged) { /* a BGZF file: its member index from its own claims, then the members that hold the range */
        mi355_inflate_report r;
        mi355_bgzf_index* idx = NULL;
        mi355_bgzf_info info;
        uint64_t got = 0, v[6];
        rc = mi355_bgzf_index_build(ctx, in, n, &idx, &r);
        if (rc == MI355_E_DATA) {
            fprintf(stderr, "index: no BGZF member behind output byte %llu\n%s\n", (unsigned long long)r.out_pos, mi355_deflate_last_error(ctx));
            return 3;
        }
        if (rc) return fail("mi355_bgzf_index_build", rc, ctx);
        mi355_bgzf_index_info(idx, &info);
        const uint64_t room = r_off >= info.total ? 0 : (r_len < info.total - r_off ? r_len : info.total - r_off);
        uint8_t* data = (uint8_t*)malloc(room ? (size_t)room : 1);
        if (!data) return fail("malloc", -1, NULL);
        rc = mi355_bgzf_read(ctx, idx, in, r_off, room, data, &got, &r);
        if (rc == MI355_E_DATA) {
            fprintf(stderr, "read: status %u at bit %llu, output byte %llu\n%s\n", r.status, (unsigned long long)r.bit,
                    (unsigned long long)r.out_pos, mi355_deflate_last_error(ctx));
            return 3;
        }
        if (rc) return fail("mi355_bgzf_read", rc, ctx);
        mi355_bgzf_last_read(ctx, v);
        f = fopen(argv[a + 1], "wb");
        if (!f || fwrite(data, 1, (size_t)got, f) != got) return fail("write output", -1, NULL);
        fclose(f);
        fprintf(stderr, "%llu bytes at %llu of %llu; %llu members of %llu decoded, %llu of %lu compressed bytes copied, %llu blocks, %.3f ms\n",
                (unsigned long long)got, r_off, (unsigned long long)info.total, (unsigned long long)v[0], (unsigned long long)info.n_members,
                (unsigned long long)v[5], (unsigned long)n, (unsigned long long)r.n_blocks, r.ms);
        free(data);
        free(in);
        mi355_bgzf_index_free(idx);
        mi355_deflate_ctx_destroy(ctx);
        return 0;
    }
    if (decompress && members) { /* a gzip file of any number of members: the size first, then the bytes */
        mi355_inflate_report r;
        size_t need = 0, got = 0, n_members = 0;
        uint8_t* data = NULL;
        rc = mi355_inflate_members(ctx, in, n, NULL, 0, &need, NULL, 0, &n_members, &r);
        if (rc == MI355_E_OUT_TOO_SMALL) {
            data = (uint8_t*)malloc(need);
            if (!data) return fail("malloc", -1, NULL);
            rc = mi355_inflate_members(ctx, in, n, data, need, &got, NULL, 0, &n_members, &r);
        }
        if (rc == MI355_E_DATA) {
            fprintf(stderr, "inflate: member %lu: status %u at bit %llu, output byte %llu\n%s\n", (unsigned long)(n_members - 1), r.status,
                    (unsigned long long)r.bit, (unsigned long long)r.out_pos, mi355_deflate_last_error(ctx));
            return 3;
        }
        if (rc) return fail("mi355_inflate_members", rc, ctx);
        f = fopen(argv[a + 1], "wb");
        if (!f || fwrite(data, 1, got, f) != got) return fail("write output", -1, NULL);
        fclose(f);
        fprintf(stderr, "%lu -> %lu bytes, %lu members, %llu blocks (%u stored, %u fixed, %u dynamic), %.3f ms\n", (unsigned long)n,
                (unsigned long)got, (unsigned long)n_members, (unsigned long long)r.n_blocks, r.n_stored, r.n_fixed, r.n_dynamic, r.ms);
        free(data);
        free(in);
        mi355_deflate_ctx_destroy(ctx);
        return 0;
    }
    if (decompress && ranged) { /* a seek index of the stream, then the one range from its nearest point */
        mi355_inflate_report r;
        mi355_inflate_seek* seek = NULL;
        mi355_seek_info si;
        uint64_t got = 0, cv[4] = {0, 0, 0, 0};
        if (cut_given) {
            rc = mi355_deflate_ctx_config(ctx, MI355_CFG_INFLATE_SEEK_CUT_BYTES, cut);
            if (rc) return fail("--cut: 0, or 64 bytes to 1 GiB", rc, NULL);
        }
        rc = mi355_inflate_seek_build(ctx, in, n, wrapper, NULL, 0, 0, &seek, &r);
        const float build_ms = r.ms;
        if (rc == MI355_OK) rc = mi355_inflate_seek_info(seek, &si);
        if (rc == MI355_OK) rc = mi355_inflate_seek_cut_info(seek, cv);
        uint8_t* data = NULL;
        if (rc == MI355_OK) {
            if (r_off > si.total) r_off = si.total;
            if (r_len > si.total - r_off) r_len = si.total - r_off;
            data = (uint8_t*)malloc(r_len ? (size_t)r_len : 1);
            if (!data) return fail("malloc", -1, NULL);
            rc = mi355_inflate_seek_read(seek, r_off, r_len, data, &got, &r);
        }
        if (rc == MI355_E_DATA) {
            fprintf(stderr, "inflate: status %u at bit %llu, output byte %llu\n%s\n", r.status, (unsigned long long)r.bit,
                    (unsigned long long)r.out_pos, mi355_deflate_last_error(ctx));
            return 3;
        }
        if (rc) return fail("mi355_inflate_seek", rc, ctx);
        f = fopen(argv[a + 1], "wb");
        if (!f || fwrite(data, 1, (size_t)got, f) != (size_t)got) return fail("write output", -1, NULL);
        fclose(f);
        fprintf(stderr, "%lu -> bytes [%llu, %llu) of %llu, %llu entries, %llu points, %llu cuts, index %.3f ms, read %.3f ms\n", (unsigned long)n,
                r_off, r_off + (unsigned long long)got, (unsigned long long)si.total, (unsigned long long)si.n_entries,
                (unsigned long long)si.n_points, (unsigned long long)cv[1], build_ms, r.ms);
        free(data);
        free(in);
        mi355_inflate_seek_free(seek);
        mi355_deflate_ctx_destroy(ctx);
        return 0;
    }
    if (decompress) { /* the size first (no buffer: the decode counts), then the bytes */
        mi355_inflate_report r;
        size_t need = 0, got = 0;
        uint8_t* data = NULL;
        int (*inflate)(mi355_deflate_ctx*, const uint8_t*, size_t, int, uint8_t*, size_t, size_t*, mi355_inflate_report*) =
            parallel ? mi355_inflate_parallel : mi355_inflate;
        rc = inflate(ctx, in, n, wrapper, NULL, 0, &need, &r);
        if (rc == MI355_E_OUT_TOO_SMALL) {
            data = (uint8_t*)malloc(need);
            if (!data) return fail("malloc", -1, NULL);
            rc = inflate(ctx, in, n, wrapper, data, need, &got, &r);
        }
        if (rc == MI355_E_DATA) {
            fprintf(stderr, "inflate: status %u at bit %llu, output byte %llu\n%s\n", r.status, (unsigned long long)r.bit,
                    (unsigned long long)r.out_pos, mi355_deflate_last_error(ctx));
            return 3;
        }
        if (rc) return fail(parallel ? "mi355_inflate_parallel" : "mi355_inflate", rc, ctx);
        f = fopen(argv[a + 1], "wb");
        if (!f || fwrite(data, 1, got, f) != got) return fail("write output", -1, NULL);
        fclose(f);
        fprintf(stderr, "%lu -> %lu bytes, %llu blocks (%u stored, %u fixed, %u dynamic), %.3f ms\n", (unsigned long)n, (unsigned long)got,
                (unsigned long long)r.n_blocks, r.n_stored, r.n_fixed, r.n_dynamic, r.ms);
        free(data);
        free(in);
        mi355_deflate_ctx_destroy(ctx);
        return 0;
    }
    mi355_deflate_opts o;
    mi355_deflate_preset(level, &o); /* Compression::{Fast,Default,Best} */
    o.wrapper = (uint8_t)wrapper;

    if (bgzf) { /* one blocked gzip file; --verify: inflated again member by member and compared with the input */
        size_t cap = mi355_bgzf_bound(n, (size_t)block), file_len = 0, n_members = 0;
        uint8_t* file = (uint8_t*)malloc(cap);
        if (!file) return fail("malloc", -1, NULL);
        rc = mi355_bgzf_encode(ctx, in, n, &o, (size_t)block, file, cap, &file_len, NULL, 0, &n_members);
        if (rc) return fail("mi355_bgzf_encode", rc, ctx);
        mi355_deflate_info binfo;
        mi355_deflate_last_info(ctx, &binfo);
        if (verify) {
            mi355_inflate_report r;
            size_t got = 0, walked = 0;
            uint8_t* back = (uint8_t*)malloc(n ? n : 1);
            if (!back) return fail("malloc", -1, NULL);
            rc = mi355_inflate_members(ctx, file, file_len, back, n, &got, NULL, 0, &walked, &r);
            if (rc != MI355_OK && rc != MI355_E_DATA && rc != MI355_E_OUT_TOO_SMALL) return fail("mi355_inflate_members", rc, ctx);
            const int same = rc == MI355_OK && got == n && walked == n_members && !memcmp(back, in, n);
            fprintf(stderr, "verify: %s; %lu members, status %u, %llu blocks (%u stored, %u fixed, %u dynamic), %.3f ms\n",
                    same ? "the file inflates to the input" : "the file does NOT inflate to the input", (unsigned long)walked, r.status,
                    (unsigned long long)r.n_blocks, r.n_stored, r.n_fixed, r.n_dynamic, r.ms);
            free(back);
            if (!same) return 3;
        }
        f = fopen(argv[a + 1], "wb");
        if (!f || fwrite(file, 1, file_len, f) != file_len) return fail("write output", -1, NULL);
        fclose(f);
        fprintf(stderr, "%lu -> %lu bytes, %lu members (the end-of-file marker among them), %u blocks\n", (unsigned long)n, (unsigned long)file_len,
                (unsigned long)n_members, binfo.n_blocks);
        free(file);
        free(in);
        mi355_deflate_ctx_destroy(ctx);
        return 0;
    }
    const uint8_t* out = NULL;
    uint8_t* owned = NULL;
    size_t out_len = 0;
    mi355_deflate_stream* s = NULL;
    if (chunk) { /* write::{Deflate,Zlib,Gz}Encoder: new, write_all ..., finish */
        rc = mi355_deflate_stream_new(ctx, &o, &s);
        if (rc) return fail("stream_new", rc, ctx);
        for (size_t i = 0; i < n; i += chunk) {
            size_t k = n - i < chunk ? n - i : chunk;
            if ((rc = mi355_deflate_stream_write(s, in + i, k))) return fail("stream_write", rc, ctx);
        }
        if ((rc = mi355_deflate_stream_finish(s))) return fail("stream_finish", rc, ctx);
        mi355_deflate_stream_output(s, &out, &out_len);
    } else { /* deflate_bytes_conf / deflate_bytes_zlib_conf / deflate_bytes_gzip */
        size_t cap = mi355_deflate_bound(n) + 64;
        owned = (uint8_t*)malloc(cap);
        rc = mi355_deflate_encode(ctx, in, n, &o, owned, cap, &out_len);
        if (rc) return fail("mi355_deflate_encode", rc, ctx);
        out = owned;
    }
    if (verify) { /* with the block table of a one-shot encode: one wave per block; a stream's output: one wave, no table */
        mi355_block_info* blocks = NULL;
        size_t n_blocks = 0;
        mi355_verify_report r;
        if (!chunk) {
            if ((rc = mi355_deflate_last_blocks(ctx, NULL, 0, &n_blocks))) return fail("mi355_deflate_last_blocks", rc, ctx);
            blocks = (mi355_block_info*)malloc((n_blocks ? n_blocks : 1) * sizeof *blocks);
            if ((rc = mi355_deflate_last_blocks(ctx, blocks, n_blocks, &n_blocks))) return fail("mi355_deflate_last_blocks", rc, ctx);
        }
        rc = mi355_deflate_verify(ctx, out, out_len, in, n, wrapper, n_blocks ? blocks : NULL, n_blocks, &r);
        free(blocks);
        if (rc != MI355_OK && rc != MI355_E_VERIFY) return fail("mi355_deflate_verify", rc, ctx);
        fprintf(stderr, "verify: status %u, entry %u, bit %llu, input byte %llu; %llu blocks (%u stored, %u fixed, %u dynamic), %.3f ms\n",
                r.status, r.entry, (unsigned long long)r.bit, (unsigned long long)r.in_pos, (unsigned long long)r.n_blocks, r.n_stored,
                r.n_fixed, r.n_dynamic, r.ms);
        if (rc == MI355_E_VERIFY) {
            fprintf(stderr, "%s\n", mi355_deflate_last_error(ctx));
            return 3;
        }
    }
    f = fopen(argv[a + 1], "wb");
    if (!f || fwrite(out, 1, out_len, f) != out_len) return fail("write output", -1, NULL);
    fclose(f);
    mi355_deflate_info info;
    mi355_deflate_last_info(ctx, &info);
    fprintf(stderr, "%zu -> %zu bytes, %u blocks, %.3f ms on the GPU\n", n, out_len, info.n_blocks, info.total_ms);
    if (s) mi355_deflate_stream_free(s);
    free(owned);
    free(in);
    mi355_deflate_ctx_destroy(ctx);
    return 0;
}
