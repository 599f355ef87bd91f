/*
 * mi355_deflate.h -- C ABI of the MI355X-native DEFLATE encode path (libmi355deflate.so).
 *
 * Drop-in boundary for the hot path of image-rs/deflate-rs v1.0.0.  The reference has no FFI
 * seam (src/lib.rs:50 forbids unsafe code); the natural seam is its block driver
 *     compress_data_dynamic_n(input, &mut DeflateState<W>, Flush)      src/compress.rs:80-84
 * as called by compress_until_done (src/writer.rs:15-23) from compress_data_dynamic
 * (src/lib.rs:110-122) and by the Write impls (src/writer.rs:124-127, 254-267).  Each entry
 * point below names the reference item it replaces.  INTEGRATION.md shows the Rust shim a
 * maintainer would add on the reference side.
 *
 * All functions are extern "C", take plain pointers and sizes, never throw, never abort, and
 * return 0 on success or a negative MI355_E_* code.  There is NO CPU fallback: every encode
 * runs the HIP kernels and fails with MI355_E_HIP if no gfx950 device is usable.
 */
#ifndef MI355_DEFLATE_H
#define MI355_DEFLATE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355_DEFLATE_VERSION 101 /* 0.1.1: the packed batch */

#define MI355_OK 0
#define MI355_E_ARG (-1)           /* null pointer / bad option */
#define MI355_E_OUT_TOO_SMALL (-2) /* *out_len holds the size needed */
#define MI355_E_HIP (-3)           /* HIP runtime error; see mi355_deflate_last_error */
#define MI355_E_UNSUPPORTED (-4)   /* lazy_if_less_than < 3 with Lazy matching -- nothing else: one-shot
                                      calls, sync-flush chunks and streams, flushed anywhere or not at all, take any length
                                      in ranges, in bounded memory */
#define MI355_E_REF_PANIC (-5)     /* the reference itself panics on this input (A.4 Q13, slice out
                                      of range) and MI355_COMPAT_Q13 was requested */
#define MI355_E_STATE (-6)         /* stream used after finish, or after a range of it failed; context busy with a shard */
#define MI355_E_VERIFY (-7)        /* the stream is not a valid raw / zlib / gzip deflate stream of this input; see the report */
#define MI355_E_DATA (-8)          /* inflate: the stream is not a valid raw / zlib / gzip deflate stream; see the report */

/* CompressionOptions (src/compression_options.rs:78-120) + MatchingType (src/lz77.rs:27-37).
 * `special` has only the Normal variant reachable from the public API and is omitted. */
typedef struct {
    uint16_t max_hash_checks;   /* compression_options.rs:84 */
    uint16_t lazy_if_less_than; /* :101; clamped to 32768 like deflate_state.rs:105 */
    uint8_t matching_type;      /* 0 = MatchingType::Greedy, 1 = MatchingType::Lazy */
    uint8_t wrapper;            /* 0 = raw deflate (deflate_bytes_conf, DeflateEncoder),
                                   1 = zlib: 78 9C + Adler-32 BE (deflate_bytes_zlib_conf,
                                   ZlibEncoder; src/lib.rs:182-198, src/zlib.rs:59-62),
                                   2 = gzip: header + CRC-32 LE + length mod 2^32 LE (feature "gzip":
                                   deflate_bytes_gzip_conf src/lib.rs:242-267, GzEncoder
                                   src/writer.rs:293-467); the header is GzBuilder::new()'s unless
                                   one of the _gzip entry points supplies it */
    uint8_t compat;             /* MI355_COMPAT_* bits */
    uint8_t flush;              /* MI355_FLUSH_FINISH (0) or MI355_FLUSH_SYNC (1) */
} mi355_deflate_opts;

/* How the stream ends (src/compress.rs:18-30 Flush).  FINISH: the last block carries BFINAL
 * (compress_until_done(.., Flush::Finish), what deflate_bytes_conf and finish() do).  SYNC: what a
 * fresh encoder has written after write_all(input) + flush() (src/writer.rs:134-137): every block
 * non-final, then the empty stored block 00 00 FF FF (src/compress.rs:256-261).  The output is byte
 * aligned, so SYNC chunks followed by one FINISH chunk concatenate into one valid deflate stream --
 * the chunk-exact ("P2") stitch used to shard one input over several GPUs.  With wrapper = 1 the
 * zlib trailer is only written for FINISH. */
#define MI355_FLUSH_FINISH 0
#define MI355_FLUSH_SYNC 1

/* Bug-for-bug mode for SURVEY A.4 Q13: when a Stored block ends on a match that crosses the
 * end of a non-first window, the reference reads the stored bytes 32768 too far ahead
 * (src/lz77.rs:679-695 + src/compress.rs:230-245) and emits a stream that does NOT inflate to
 * the input.  Default (bit clear): emit the block's real bytes (valid stream; differs from the
 * reference only inside that block).  Bit set: reproduce the reference's bytes exactly. */
#define MI355_COMPAT_Q13 1u

/* Compression::{Fast, Default, Best} -> CompressionOptions (compression_options.rs:188-196)
 * and the two named profiles rle() :171-178, huffman_only() :155-162. */
#define MI355_LEVEL_FAST 0
#define MI355_LEVEL_DEFAULT 1
#define MI355_LEVEL_BEST 2
#define MI355_LEVEL_RLE 3
#define MI355_LEVEL_HUFFMAN_ONLY 4
int mi355_deflate_preset(int level, mi355_deflate_opts* out);

int mi355_deflate_version(void);

/* Upper bound of the output size for in_len input bytes: every block is at most its stored form
 * (src/huffman_lengths.rs:269-286 picks the cheapest, src/stored_block.rs:13-40), plus the framing of any
 * wrapper with the blank gzip header.  mi355_deflate_bound_ex is the exact requirement of the encode
 * entry points for a given wrapper (0 raw, 1 zlib, 2 gzip with hdr_len header bytes) and number of sync
 * flush points (each can add a block header and the marker 00 00 FF FF, src/compress.rs:256-261); a
 * buffer of mi355_deflate_bound(in_len) bytes is always enough for a one-shot call. */
size_t mi355_deflate_bound(size_t in_len);
size_t mi355_deflate_bound_ex(size_t in_len, int wrapper, size_t hdr_len, size_t n_flush);

/* A context owns one HIP device, its workspace and timing events.  Not thread safe; use one
 * context per thread (the reference's encoders are likewise single-owner: DeflateState,
 * src/deflate_state.rs:66-97).  Where an entry point accepts ctx == NULL it works on a process-wide
 * default context on device 0 and holds that context's lock for the whole call, so NULL-context calls
 * from several threads are safe (and serialised).
 * Creating a context runs one short self-test kernel on the device (about 0.1 ms): the hash sort takes its ranks
 * from returning LDS atomics when -- and only when -- the device serves the lanes that hit one LDS address in lane
 * order (MI355X does); otherwise it ranks with ballots.  The output is the same either way, and every encode
 * checks the order of the sorted buckets it walks (MI355_CFG_SORT_RANKS below).
 * A context that holds a sharded encode (between mi355_shard_begin and mi355_shard_end) refuses other encodes
 * with MI355_E_STATE: the shard's tokens and tables live in the context's workspace. */
typedef struct mi355_deflate_ctx mi355_deflate_ctx;
int mi355_deflate_ctx_create(int device, mi355_deflate_ctx** out);
void mi355_deflate_ctx_destroy(mi355_deflate_ctx* ctx);
const char* mi355_deflate_last_error(mi355_deflate_ctx* ctx);

/* Tuning of one context (ctx may be NULL: the default context).  No reference item: the reference has no tunables
 * beyond CompressionOptions; these set the memory / throughput trade of the GPU path, never the bytes it produces.
 *   MI355_CFG_RANGE_BYTES  bytes per range of a long input or a stream (default 512 MiB; at least 16 MiB,
 *                          at most 3 GiB, rounded down to a multiple of 32768).  Device memory of a long encode is two
 *                          workspaces of about 20 B per byte of a range, host memory of a stream one range + 16 MiB.
 *   MI355_CFG_LONG_FROM    one-shot inputs of at least this many bytes are walked in ranges (default 1 GiB + 1; at most
 *                          4 GiB - 64 KiB, what a single pass takes)
 *   MI355_CFG_SORT_RANKS   where the hash sort takes its ranks from: 1 = returning LDS atomics (the default on a device
 *                          that passed the self-test of mi355_deflate_ctx_create; MI355_E_UNSUPPORTED on one that did
 *                          not), 0 = ballots (any device; about 40 % more time in the sort).  Whatever the setting, the
 *                          match kernel checks every hash bucket's order on the data it walks and an encode that finds
 *                          one out of order is done again with ballot ranks, which the context then keeps.
 *   MI355_CFG_HOST_STREAMING  how a host-buffer call of 16 MiB or more (mi355_deflate_encode and its zlib / gzip
 *                          forms) hands its bytes back: 1 (default) = piece by piece -- the input arrives in pieces, each
 *                          is encoded as it arrives (its parse, block and pack stages beside the match stage of the next
 *                          one) and the finished bytes leave on the copy engine while the later pieces are worked on;
 *                          0 = one copy-out after the last kernel; 2 = pieces with their stages behind each other
 *                          (a measuring aid).  Same bytes every way; data the piecewise form does not take (a hash re-warm
 *                          in the first window, long periodic data) is encoded the other way without the caller noticing.
 *                          (Measuring aids, read once per process: the environment variables MI355_HOST_PLAN="1,2,3,3" -- rounds of
 *                          256 windows per piece -- and MI355_HOST_FIRST=<windows of the first piece, 0 = a whole round>.)
 *   MI355_CFG_HOST_BOUNCE  what a host-buffer call does with PAGEABLE caller memory (a plain &[u8] / Vec<u8>: what
 *                          deflate_bytes hands over, src/lib.rs:137-147) of 4 MiB or more: 1 (default) = the context's host
 *                          threads copy it through two page-locked rings of 64 MiB -- the input's pieces arrive while the
 *                          first ones are worked on, the finished bytes leave piece by piece, as for a caller that page-locked
 *                          its buffers; 0 = the runtime's own copies (one thread, in series with the kernels).
 *                          Page-locked buffers (hipHostMalloc / hipHostRegister) never take the threads.  The same threads
 *                          carry the ranges of a call of more than 1 GiB and of mi355_deflate_encode_multi.
 *   MI355_CFG_HOST_THREADS  how many such threads the context starts when the first pageable call comes (1..16; default 8 on
 *                          a host of 32 hardware threads or more, else 4 or 2; the environment variable MI355_HOST_THREADS
 *                          sets the default).  They stay on the memory node of the thread that made them, poll for a
 *                          millisecond after a call and sleep between calls.  MI355_E_STATE once they run.
 *   MI355_CFG_MULTI_STITCH  (of rank 0's context of a mi355_multi handle: mi355_multi_ctx(m, 0)) how the packed ranges of
 *                          mi355_deflate_encode_multi_device reach rank 0's device: 0 (default) = peer copies
 *                          (hipMemcpyPeerAsync: xGMI between the GPUs of a node), 1 = RCCL -- one ncclSend per rank, the
 *                          matching ncclRecv posted by rank 0's thread straight into the caller's buffer; librccl.so is
 *                          looked up when the first such call is made (MI355_E_UNSUPPORTED if it is not there).
 *   MI355_CFG_STEPS_IN_EMIT  where the parser's restart steps (lz77.rs:305-547 seen from a position) are worked out: 1 (default) =
 *                          by the kernel that writes the tokens, from the match table, where that is possible (the lazy and
 *                          greedy levels without a quarter-budget table, input without flush points); 0 = always by a kernel
 *                          of their own that leaves them in device memory (what the exact path search, `Best` and flushed
 *                          streams use anyway).  Same bytes either way: a testing and measuring aid.
 *   MI355_CFG_STAGE_CLOCKS  the per-stage clocks in mi355_deflate_info -- stage_ms, match_ms --: 0 (default) = never, 1 = for every
 *                          call, 2 = for calls of 32 MiB or more.  They are events between the kernels of a call, each 5.7 us of
 *                          idle queue -- a tenth of a 167 KB call, 0.7 % of a 100 MB one; without them stage_ms and match_ms read 0
 *                          and total_ms is the host's clock from the call's first launch to the return of its last wait.
 *                          (The environment variable MI355_STAGE_CLOCKS sets the default: a measuring aid.)
 *   MI355_CFG_BATCH_BYTES  input bytes of one launch set of mi355_deflate_encode_batch[_device] (default 256 MiB; 1 MiB .. 1 GiB):
 *                          a batch with more is cut into consecutive sub-batches.  Same bytes either way.
 *   MI355_CFG_INFLATE_GROUP_BYTES  output bytes of one group of table entries of mi355_inflate_tabled[_device] (default 256 MiB;
 *                          at least 64 KiB): a group's workspace is two bytes per output byte plus 32 KiB per entry, so a longer
 *                          stream is decoded group after group.  An entry larger than this is a group of its own.  Same bytes
 *                          either way.
 *   MI355_CFG_INFLATE_INDEX_SPAN_BYTES  compressed bytes of one span of mi355_inflate_index[_device] / mi355_inflate_parallel[_device]
 *                          (default 16 KiB; 256 bytes .. 1 GiB): one wave searches a span for a block start and one walks on from
 *                          it, so a table has one entry per span at most.  Same bytes either way.  The default is the best of a
 *                          sweep over 16 / 32 / 64 / 128 KiB on 100 MB of text deflated by zlib at level 6: 55.5 / 70.4 / 83.1 /
 *                          140.1 ms for the whole mi355_inflate_parallel_device call (profiles/inflate_index_bench.json).
 *   MI355_CFG_INFLATE_MEMBER_SPAN_BYTES  compressed bytes of one span of mi355_inflate_members[_device] (default 64 KiB; 16 bytes ..
 *                          1 GiB): one wave searches a span for a member that states its own size and one lane hops on from it.
 *                          Same results either way.  The default is derived, not measured: a BGZF member is 64 KiB at most, so at
 *                          that size every interior span of a BGZF file holds a member start.
 *   MI355_CFG_INFLATE_MEMBER_PARALLEL_BYTES  how many compressed bytes must be left in the file from the start of a member that states
 *                          no size for mi355_inflate_members[_device] to look for its end and its block table on the device and to
 *                          decode it in parallel (default 64 KiB; 1 KiB .. 1 GiB; 0 switches the path off: every such member is
 *                          walked by one wave).  Same results either way.  The default is derived, not measured -- four spans of
 *                          MI355_CFG_INFLATE_INDEX_SPAN_BYTES at its default, so that a table of two entries at least is likely --
 *                          and no measured optimum.  What tools/inflate_members_bench.py has measured (profiles/
 *                          inflate_members_bench.json; 100 MB of text as 64 members): finding a member costs about 29 ms whatever
 *                          its size, so the path wins where one wave would need longer for the member -- deflated text: 2354 ms
 *                          on, 17 285 ms off -- and LOSES where one wave is fast -- the same members as stored blocks: 1450 ms on,
 *                          72.7 ms off.  Set 0 for files of stored or hardly compressed members.
 *   MI355_CFG_INFLATE_SEEK_CUT_BYTES  output bytes between the CUTS a seek handle remembers inside its table entries (default 0: no
 *                          cuts, every seek call does what it did without the key; else 64 bytes .. 1 GiB, anything else is
 *                          MI355_E_ARG).  Read when a handle is built (mi355_inflate_seek_build[_device]): the handle keeps the value
 *                          in force.  With cuts a read decodes one wave per cut instead of one per entry.  Same bytes either way.
 *                          The sweep of tools/inflate_cut_bench.py (profiles/inflate_cut_bench.json) favours 4 KiB on deflated text; the
 *                          default stays 0 until turning it on is a change of its own.
 *   MI355_CFG_INFLATE_SEEK_CUT_WALKER  a measuring aid and no part of the stable interface (default 0; 0 or 1): 1 = a build with
 *                          cuts runs its pass 1 as without cuts and finds the cuts in a second launch that stores no symbol -- the
 *                          alternative tools/inflate_cut_bench.py times against recording them in pass 1.  Same handle either way. */
#define MI355_CFG_RANGE_BYTES 1
#define MI355_CFG_LONG_FROM 2
#define MI355_CFG_SORT_RANKS 3
#define MI355_CFG_HOST_STREAMING 4
#define MI355_CFG_MULTI_STITCH 5
#define MI355_CFG_STEPS_IN_EMIT 6
#define MI355_CFG_HOST_BOUNCE 7
#define MI355_CFG_HOST_THREADS 8
#define MI355_CFG_STAGE_CLOCKS 9
#define MI355_CFG_BATCH_BYTES 10
#define MI355_CFG_INFLATE_GROUP_BYTES 11
#define MI355_CFG_INFLATE_INDEX_SPAN_BYTES 12
#define MI355_CFG_INFLATE_MEMBER_SPAN_BYTES 13
#define MI355_CFG_INFLATE_MEMBER_PARALLEL_BYTES 14
#define MI355_CFG_INFLATE_SEEK_CUT_BYTES 15
#define MI355_CFG_INFLATE_SEEK_CUT_WALKER 16
int mi355_deflate_ctx_config(mi355_deflate_ctx* ctx, int key, uint64_t value);
/* What a key of the decode side (11 to 16) is set to; any other key is MI355_E_ARG. */
int mi355_deflate_ctx_config_get(mi355_deflate_ctx* ctx, int key, uint64_t* value);

/* deflate_bytes_conf / deflate_bytes_zlib_conf (src/lib.rs:137-147, 182-198): host buffers
 * in, host buffer out.  ctx may be NULL (the default context, see above).  An input of 16 MiB or more is
 * copied in pieces and worked on while the later ones are still on the bus, and its finished bytes leave piece by piece:
 * for page-locked buffers (hipHostMalloc / hipHostRegister) on the copy engines directly, for pageable memory -- what a
 * drop-in caller has -- through the context's host threads and their page-locked slots (MI355_CFG_HOST_BOUNCE).
 * Any in_len is taken, like src/lib.rs:137-147: an input of more than 1 GiB is walked as consecutive ranges of
 * 512 MiB (csrc/deflate_long.inc -- the phases of the sharded encode below, one range after the other on this
 * GPU; the same bytes as a single pass), which also bounds the device memory of a call: two workspaces of
 * about 20 B per byte of a range. */
int mi355_deflate_encode(mi355_deflate_ctx* ctx, const uint8_t* in, size_t in_len, const mi355_deflate_opts* opts,
                         uint8_t* out, size_t out_cap, size_t* out_len);

/* Allocate now what encodes of up to in_len bytes need (the workspace is about 20 bytes per input byte
 * and only ever grows; with host_api != 0 also the device staging buffers of mi355_deflate_encode), so
 * that the first call does not pay for it.  No reference item: the reference's encoders allocate their
 * 330 KiB in ::new (src/deflate_state.rs:82-119). */
int mi355_deflate_ctx_reserve(mi355_deflate_ctx* ctx, size_t in_len, int host_api);

/* Same computation with input and output resident in device memory (no PCIe in the path):
 * compress_data_dynamic + compress_until_done(.., Flush::Finish) (src/lib.rs:110-122,
 * src/writer.rs:15-58) over d_in[0..in_len).  d_out must be 4-byte aligned and hold
 * mi355_deflate_bound(in_len) bytes (exactly: mi355_deflate_bound_ex(in_len, opts->wrapper, 10, 0); a
 * smaller buffer is refused with MI355_E_OUT_TOO_SMALL and the size in *out_len).  `hip_stream` is a
 * hipStream_t (NULL = the context's own stream); the
 * call returns after the stream has drained, with *out_len set.  Always raw deflate unless
 * opts->wrapper == 1, in which case the 2-byte header and 4-byte trailer are written too.
 * Any in_len (more than 1 GiB: in ranges, see mi355_deflate_encode; the work then runs on the context's streams). */
int mi355_deflate_encode_device(mi355_deflate_ctx* ctx, const void* d_in, size_t in_len, const mi355_deflate_opts* opts,
                                void* d_out, size_t out_cap, size_t* out_len, void* hip_stream);

/* What the last encode on this context did (also the hook bench.py reads its HIP-event timings
 * from). */
#define MI355_STAGE_LINKS 0   /* k_links        (chained_hash_table.rs) */
#define MI355_STAGE_MATCH 1   /* k_match/k_rle  (matching.rs, rle.rs) */
#define MI355_STAGE_PARSE 2   /* k_adv .. k_compact (lz77.rs parsers as a restart path) */
#define MI355_STAGE_BLOCKS 3  /* bounds, histogram, header, plan (output_writer.rs, huffman_lengths.rs) */
#define MI355_STAGE_PACK 4    /* k_pack         (encoder_state.rs, bitstream.rs, stored_block.rs) */
#define MI355_STAGE_OTHER 5   /* memset, adler, copies */
#define MI355_N_STAGES 6
typedef struct {
    uint64_t in_len, out_len;
    uint64_t n_tokens;
    uint32_t n_blocks, n_stored, n_fixed, n_dynamic;
    uint32_t q1_rewarm;       /* 1 if the hash re-warm quirk (A.4 Q1) fired and was reproduced */
    uint32_t q13_hits;        /* stored blocks hit by A.4 Q13 */
    uint32_t passes;          /* 1, or 2 when Q1 forced a second pass */
    uint32_t spec_fallback;   /* 1: the speculative segment entries of the parse did not check out (long periodic data) and
                                 the call was parsed again the exact way -- same bytes, about a millisecond per 100 MB more */
    float stage_ms[MI355_N_STAGES]; /* HIP-event time per stage, summed over passes (0 without the stage clocks: MI355_CFG_STAGE_CLOCKS) */
    float total_ms;                 /* first kernel enqueued .. last kernel done (without the stage clocks: the host's clock over the same) */
    uint32_t match_launches;        /* launches of the dominant kernel in this encode */
    float match_ms;                 /* their summed duration */
    uint32_t spec_repaired;         /* segments whose speculative entry was wrong and that were parsed again in place */
    uint32_t host_path;             /* how the last host-buffer call (mi355_deflate_encode and its forms) moved its bytes:
                                       MI355_HOST_PATH_* bits; 0 after a device-buffer call */
} mi355_deflate_info;
#define MI355_HOST_PATH_PIECES 1u      /* worked on and handed back piece by piece (MI355_CFG_HOST_STREAMING) */
#define MI355_HOST_PATH_IN_THREADS 2u  /* pageable input: carried to the device by the context's host threads */
#define MI355_HOST_PATH_OUT_THREADS 4u /* pageable output: carried back by them */
int mi355_deflate_last_info(mi355_deflate_ctx* ctx, mi355_deflate_info* info);

/* Diagnostics: the block layout of the last encode (type, BFINAL, tokens, input bytes, bit offset
 * of the first header bit inside the raw deflate stream) -- the per-block facts of
 * compress_data_dynamic_n's loop (src/compress.rs:157-246), for diffing against an oracle. */
typedef struct {
    uint32_t btype; /* 0 stored, 1 fixed, 2 dynamic */
    uint32_t bfinal;
    uint32_t n_tokens;
    uint32_t reserved;
    uint64_t in_bytes;
    uint64_t bit_start;
} mi355_block_info;
int mi355_deflate_last_blocks(mi355_deflate_ctx* ctx, mi355_block_info* out, size_t cap, size_t* n_blocks);

/* ---- batched encode: many independent inputs, one set of launches -----------------------------
 * Item i's output is byte for byte what mi355_deflate_encode gives for that item alone with the same opts (whatever the
 * other items, their order or their number).  One opts for the whole batch: every level, wrapper 0 (raw) or 1 (zlib),
 * MI355_FLUSH_FINISH; wrapper 2 or a sync flush is MI355_E_ARG, lazy_if_less_than < 3 with Lazy MI355_E_UNSUPPORTED.
 * Items of up to 2 MiB are encoded together by the batched kernels, at the levels with a hash table and at those without
 * one (RLE, Huffman-only); longer items, empty items and the items whose first block fires the hash re-warm (A.4 Q1; the
 * levels with a hash only) or whose speculative parse fails (at RLE: runs too long to re-join, zero fill first of all) go
 * through the one-input path after them.
 * An item with out_cap < mi355_deflate_bound_ex(in_len, opts->wrapper, 0, 0) gets MI355_E_OUT_TOO_SMALL and the size needed in
 * out_len; an item may get MI355_E_REF_PANIC under MI355_COMPAT_Q13.  Neither disturbs the other items.  The call returns
 * MI355_OK when every item is OK, else the status of the first failing item; errors of the call itself (NULL items with
 * n_items > 0, NULL opts, an item without buffers, bad options) are MI355_E_ARG and write no item.
 * _device: in / out are device pointers (out 4-byte aligned); hip_stream NULL = the context's stream; the call returns
 * after the stream has drained.  Without _device they are host pointers.
 * After a batch, mi355_deflate_last_info describes the batch as a whole (sums) and mi355_deflate_last_blocks reports 0 blocks. */
typedef struct {
    const void* in;    /* host pointer (mi355_deflate_encode_batch) or device pointer (_device) */
    size_t in_len;
    void* out;         /* host / device; on the device entry 4-byte aligned */
    size_t out_cap;    /* >= mi355_deflate_bound_ex(in_len, opts->wrapper, 0, 0) */
    size_t out_len;    /* written: bytes produced, or the size needed after MI355_E_OUT_TOO_SMALL */
    int status;        /* written: MI355_OK or this item's MI355_E_* */
} mi355_batch_item;

typedef struct {
    uint64_t n_items, in_len, out_len;   /* sums over the items */
    uint32_t n_batched;                  /* items encoded by the batched kernels */
    uint32_t n_single;                   /* items sent through the one-input path */
    uint32_t n_q1_single, n_spec_single; /* of n_single: Q1 re-warm fired / speculative entries failed */
    uint32_t sub_batches;                /* launch sets the batch was cut into */
    float total_ms;                      /* host clock over the call */
} mi355_batch_info;

int mi355_deflate_encode_batch(mi355_deflate_ctx* ctx, mi355_batch_item* items, size_t n_items,
                               const mi355_deflate_opts* opts);
int mi355_deflate_encode_batch_device(mi355_deflate_ctx* ctx, mi355_batch_item* items, size_t n_items,
                                      const mi355_deflate_opts* opts, void* hip_stream);
int mi355_deflate_last_batch_info(mi355_deflate_ctx* ctx, mi355_batch_info* info);

/* The gzip forms of the batch (cargo feature "gzip"): every item is one gzip member with a header of its own, i.e.
 *   item i = deflate_bytes_gzip_conf(input_i, options, builder_i)   src/lib.rs:242-267
 * and byte for byte what mi355_deflate_encode_gzip gives for that item alone with the same opts and its header (whatever
 * the other items, their order, their number or the way the batch is cut into launch sets).  opts->wrapper is taken as 2
 * whatever it holds, as the single _gzip entries do; mi355_deflate_encode_batch[_device] itself keeps answering
 * MI355_E_ARG to wrapper 2.
 * hdrs[i].hdr = the bytes GzBuilder::into_header() returned for item i (host memory for both entries):
 *   n_hdrs == 0        every item gets the blank header, GzBuilder::new() (hdrs is not read)
 *   n_hdrs == 1        all items share hdrs[0]
 *   n_hdrs == n_items  item i gets hdrs[i]
 * Any other n_hdrs, a NULL hdrs with n_hdrs > 0, or an entry with a NULL pointer, length 0 or a length above 0xFFFF is
 * MI355_E_ARG and writes no item; the other errors of the call are those of mi355_deflate_encode_batch.
 * An item needs out_cap >= mi355_deflate_bound_ex(in_len, 2, hdr_len_i, 0); a shorter one gets MI355_E_OUT_TOO_SMALL and
 * that size in out_len, the other items undisturbed.  The items the batched kernels take are those of the raw / zlib
 * batch: CRC-32, header and trailer are written by the launches of the set (one more kernel for the CRC-32, one for the
 * frame); the others go through mi355_deflate_encode_gzip / _device_gzip with their own header.
 * Return value, mi355_deflate_last_batch_info, mi355_deflate_last_info and mi355_deflate_last_blocks: as after
 * mi355_deflate_encode_batch[_device]. */
typedef struct {
    const uint8_t* hdr; /* host memory */
    size_t hdr_len;     /* 1 .. 0xFFFF */
} mi355_gzip_header;

int mi355_deflate_encode_batch_gzip(mi355_deflate_ctx* ctx, mi355_batch_item* items, size_t n_items,
                                    const mi355_deflate_opts* opts, const mi355_gzip_header* hdrs, size_t n_hdrs);
int mi355_deflate_encode_batch_device_gzip(mi355_deflate_ctx* ctx, mi355_batch_item* items, size_t n_items,
                                           const mi355_deflate_opts* opts, const mi355_gzip_header* hdrs, size_t n_hdrs,
                                           void* hip_stream);

/* ---- batched encode into one packed arena ---------------------------------------------------------
 * The batch above with another way of handing the bytes back: all streams back to back in ONE caller-supplied arena, at
 * offsets worked out on the device from the streams' exact lengths, so that the arena needs to be only as large as the
 * output is.  The items are mi355_batch_item: `in` and `in_len` are read, `out` and `out_cap` are ignored on entry; on
 * return `out` is the item's address inside the arena (NULL for an item that is not MI355_OK), `out_len` its exact
 * length and `status` its status.
 * Wrapper and headers: opts->wrapper is 0 (raw), 1 (zlib) or 2 (gzip); hdrs / n_hdrs are read for wrapper 2 only, with the
 *   0 / 1 / n_items rule of the _gzip entries above.  The other checks of the call are those of mi355_deflate_encode_batch
 *   (MI355_FLUSH_FINISH only; lazy_if_less_than < 3 with Lazy is MI355_E_UNSUPPORTED; a live shard is MI355_E_STATE).  A
 *   call that fails its checks writes no item, no arena byte and leaves *arena_used alone.
 * align: a power of two from 4 to 4096; 0 means 4; anything else is MI355_E_ARG.  The device arena must be aligned to
 *   `align`; the host arena may have any address.
 * Bytes: item i's out_len bytes at out are byte for byte what mi355_deflate_encode / mi355_deflate_encode_gzip gives for
 *   that item alone -- whatever the other items, their order or number, the way the batch is cut into launch sets, and
 *   whatever align is.
 * Layout: every OK item owns the region [off, off + align_up(len, align)) of the arena, off a multiple of align; the
 *   regions are disjoint and dense, pad bytes inside a region are zero, and *arena_used is the sum of align_up(len, align)
 *   over the OK items = the end of the last region.  No order of the regions is promised (today: the items of the
 *   batched kernels in item order, then those of the one-input path in item order); the table tells.  Arena contents at or
 *   beyond *arena_used are unspecified; nothing is ever written at or beyond arena_cap.
 * Capacity: arena_cap >= mi355_deflate_batch_packed_bound(...) always succeeds; the bound is the sum of
 *   align_up(mi355_deflate_bound_ex(in_len_i, wrapper, hdr_len_i, 0), align), computed on the host without a GPU (hdr_len_i:
 *   0 unless wrapper is 2; 10, the blank header, with n_hdrs 0).  A smaller arena is legal: offsets are assigned as if it
 *   were unbounded, and an item whose region would end beyond arena_cap is not written -- it gets MI355_E_OUT_TOO_SMALL
 *   and its exact out_len; the call then returns MI355_E_OUT_TOO_SMALL and *arena_used holds the bytes the whole batch
 *   needs.  The items that fit are complete and valid, and a second call with arena_cap = *arena_used succeeds.
 * Failing items: MI355_E_REF_PANIC under MI355_COMPAT_Q13 takes no bytes, like the overflow above, and does not disturb
 *   its neighbours.  The call returns the status of the first failing item, as mi355_deflate_encode_batch does.
 * d_table (device memory, n_items entries, may be NULL): entry i = {off, len, status} of items[i], for a caller whose
 *   next kernel reads the arena; off = out - arena for an OK item, and the offset the item was assigned (nothing is
 *   written there) for one that is not.  It is complete when the call returns, which is after the stream has drained.
 * mi355_deflate_last_batch_info, mi355_deflate_last_info, mi355_deflate_last_blocks and the routing of the items
 * (the batched kernels or the one-input path, MI355_CFG_BATCH_BYTES): as with mi355_deflate_encode_batch. */
typedef struct {
    uint64_t off, len; /* the item's first byte in the arena; its exact length */
    int32_t status;    /* MI355_OK or the item's MI355_E_* */
    uint32_t reserved; /* 0 */
} mi355_packed_entry;  /* 24 bytes */

size_t mi355_deflate_batch_packed_bound(const mi355_batch_item* items, size_t n_items, int wrapper,
                                        const mi355_gzip_header* hdrs, size_t n_hdrs, size_t align);
int mi355_deflate_encode_batch_packed(mi355_deflate_ctx* ctx, mi355_batch_item* items, size_t n_items,
                                      const mi355_deflate_opts* opts, const mi355_gzip_header* hdrs, size_t n_hdrs,
                                      uint8_t* arena, size_t arena_cap, size_t align, size_t* arena_used);
int mi355_deflate_encode_batch_packed_device(mi355_deflate_ctx* ctx, mi355_batch_item* items, size_t n_items,
                                             const mi355_deflate_opts* opts, const mi355_gzip_header* hdrs, size_t n_hdrs,
                                             void* d_arena, size_t arena_cap, size_t align, mi355_packed_entry* d_table,
                                             size_t* arena_used, void* hip_stream);

/* ---- verify: does this stream inflate to this input? ------------------------------------------------
 * What `gzip -t` and `zstd --check` answer, on the device and without writing a byte: the expected output is the input, so a
 * literal is right when it equals in[p] and a match (len, dist) at p when in[p + i] == in[p + i - dist] for i < len.  No reference
 * item: the reference has no decoder.  FINISH streams only (the last block carries BFINAL); pad bits behind the BFINAL block and
 * in front of a stored LEN are ignored, as zlib's inflate does; in_len at most 4 GiB - 64 KiB (more: MI355_E_UNSUPPORTED), 0 is legal.
 * blocks / n_blocks (host memory): what mi355_deflate_last_blocks returned for the encode that made the stream; only bit_start and
 *   in_bytes are read.  The table is a set of restart points, checked by one wave each: entry e starts at bit bit_start[e] of the
 *   raw stream and its first output byte is in[sum of in_bytes[k], k < e].  An entry may hold several deflate blocks (an encoder
 *   "stored block" is a run of stored pieces; empty blocks are legal): after each one a non-last entry is done when it stands
 *   exactly at the next entry's bit and input offset, and passing either is MI355_VERIFY_TABLE.  blocks == NULL: one entry at
 *   (0, 0) -- one wave walks the whole stream: for small streams and for streams made elsewhere.  bit_start values that do not
 *   ascend, or in_bytes that do not sum to in_len, are MI355_E_ARG.
 * wrapper: as in mi355_deflate_opts.  1: CM = 8, CINFO <= 7, FCHECK, no FDICT, Adler-32 big endian behind the data.  2: the RFC 1952
 *   header (ID1, ID2, CM, reserved FLG bits clear; FEXTRA, FNAME, FCOMMENT and FHCRC are skipped; it must end within 64 KiB + 32
 *   bytes), then CRC-32 and ISIZE little endian.  Anything else is MI355_E_ARG.
 * Returns MI355_OK when the stream verifies and MI355_E_VERIFY when it does not; the report is filled either way and
 *   mi355_deflate_last_error gives one line.  FRAME is reported first, then the failing entry with the smallest index and inside it
 *   the first failure in stream order; TRAILER / CHECKSUM only when every entry is clean.  The result is a function of the
 *   arguments alone.  MI355_E_ARG, MI355_E_HIP and MI355_E_STATE (live shard) as elsewhere.  A verify call does not disturb
 *   mi355_deflate_last_info / _last_blocks / _last_batch_info of the encode before it.
 * A dynamic header is judged by zlib's rules (MI355_VERIFY_LENGTHS): more than 286 literal/length or 30 distance codes; a
 *   code-length code that is not complete; repeat code 16 with nothing before it; a repeat that runs past HLIT + HDIST; no code
 *   for symbol 256; a set that is over-subscribed, or incomplete unless it is exactly one code of length 1.  All distance lengths
 *   zero is legal (a length symbol then fails as MI355_VERIFY_CODE).
 * _device: d_stream / d_in are device pointers of any alignment; hip_stream NULL = the context's stream; the call returns after the
 *   stream has drained.  Without _device they are host pointers, copied into the context's staging buffers.
 * _batch_device: item i is verified without a table -- in / in_len is the input, out / out_len the stream, as a batch encode left
 *   them (the packed entries' out pointers into the arena work too).  Items whose status on entry is not MI355_OK are skipped and
 *   left alone; for the others status becomes MI355_OK or MI355_E_VERIFY and reports[i] (if reports is not NULL) is filled.  The
 *   call returns the first failing item's status.  One launch for all items, one workgroup per item. */
#define MI355_VERIFY_OK        0
#define MI355_VERIFY_FRAME     1  /* zlib / gzip header malformed, or the stream is shorter than its frame */
#define MI355_VERIFY_BTYPE     2  /* BTYPE 3 */
#define MI355_VERIFY_STORED    3  /* LEN != ~NLEN */
#define MI355_VERIFY_LENGTHS   4  /* dynamic header: see the rules above */
#define MI355_VERIFY_CODE      5  /* bits that are no code of the set; ll symbol 286/287; distance symbol 30/31 */
#define MI355_VERIFY_DISTANCE  6  /* distance > 32768 or > the bytes produced so far (counted from input position 0) */
#define MI355_VERIFY_MISMATCH  7  /* a literal, a match or a stored byte differs from the input */
#define MI355_VERIFY_LENGTH    8  /* last entry / no table: a token runs past in_len, or the BFINAL block ends before in_len */
#define MI355_VERIFY_TABLE     9  /* with a table: an entry's blocks do not end exactly at the next entry's bit_start and input
                                     offset, or BFINAL is met before the last entry */
#define MI355_VERIFY_TRUNCATED 10 /* bits needed beyond the end of the deflate data (incl. no BFINAL block before it) */
#define MI355_VERIFY_TRAILER   11 /* bytes between the end of the BFINAL block and the trailer, or after it */
#define MI355_VERIFY_CHECKSUM  12 /* Adler-32 (zlib) / CRC-32 or ISIZE (gzip) in the trailer is not the input's */

typedef struct {
    uint32_t status;    /* MI355_VERIFY_* */
    uint32_t entry;     /* index into blocks[] of the failing entry (0 without a table) */
    uint64_t bit;       /* raw-deflate bit offset (frame header excluded) where the failing element begins:
                           the block header, the code-length section, the code, the LEN field */
    uint64_t in_pos;    /* MISMATCH: the first input byte that differs; else the bytes produced before the element */
    uint64_t n_blocks;  /* OK only: deflate blocks decoded (a stored piece counts as one) */
    uint32_t n_stored, n_fixed, n_dynamic;
    float ms;           /* host clock over the call */
} mi355_verify_report;  /* 48 bytes */

int mi355_deflate_verify_device(mi355_deflate_ctx* ctx, const void* d_stream, size_t stream_len, const void* d_in, size_t in_len,
                                int wrapper, const mi355_block_info* blocks, size_t n_blocks, mi355_verify_report* report,
                                void* hip_stream);
int mi355_deflate_verify(mi355_deflate_ctx* ctx, const uint8_t* stream, size_t stream_len, const uint8_t* in, size_t in_len,
                         int wrapper, const mi355_block_info* blocks, size_t n_blocks, mi355_verify_report* report);
int mi355_deflate_verify_batch_device(mi355_deflate_ctx* ctx, mi355_batch_item* items, size_t n_items, int wrapper,
                                      mi355_verify_report* reports /* n_items entries, or NULL */, void* hip_stream);

/* ---- inflate: decode one stream, or a batch of streams, to its bytes on the device -----------------------
 * The other half of the batch entry points: what the library wrote into device memory -- one stream, the items of a batch, the
 * regions of a packed arena -- is decoded where it lies.  No reference item: the reference has no decoder.  Streams made by anyone
 * are accepted, not only ones this library encoded; pointers of any alignment.
 * wrapper: 0 / 1 / 2 as in verify, and the framing rules are verify's: zlib with FDICT is MI355_VERIFY_FRAME; ONE gzip member
 *   only (a file of several: mi355_inflate_members below), bytes after the trailer are MI355_VERIFY_TRAILER (so are bytes behind
 *   the BFINAL block of a raw stream); pad bits are ignored, as zlib does; a dynamic header is judged by zlib's rules (see verify).  Anything else is MI355_E_ARG.
 * Return value, for one stream and for each item of a batch:
 *   MI355_OK               out[0, out_len) is the data; report.out_pos == report.out_len.
 *   MI355_E_DATA           the report names the first failure in stream order (status, bit, out_pos); out[0, min(out_pos, out_cap))
 *                          holds the bytes decoded in front of it -- literals gathered in front of the failing element are written
 *                          before it is reported -- and nothing is written at or beyond out_pos.  *out_len = the bytes that hold data.
 *   MI355_E_OUT_TOO_SMALL  the stream is structurally valid but longer than out_cap: the decode went on COUNTING without storing, so
 *                          *out_len / report.out_len is the exact size needed and out[0, out_cap) holds the first out_cap bytes.  The
 *                          checksum is not judged.  out_cap == 0 with out == NULL is a legal size query.
 *   No store ever lands at an index >= out_cap, and no load of the output happens at an index >= min(p, out_cap), p being the
 *   bytes produced so far.  A framed stream that inflates to more than 4 GiB - 64 KiB is MI355_E_UNSUPPORTED (the checksum kernels).
 * ctx == NULL (the default context), a live shard (MI355_E_STATE), MI355_E_ARG and MI355_E_HIP: as in verify.  _device: device
 *   pointers; hip_stream NULL = the context's stream; the call returns after the stream has drained.  Without _device they are host
 *   pointers: the stream is copied into the context's staging and the bytes that hold data are copied back.  An inflate call leaves
 *   mi355_deflate_last_info / _last_blocks / _last_batch_info alone; mi355_deflate_last_error gives one line.
 * Checksums (wrapper 1 / 2): the output's length exists only after the decode, so a framed call waits twice: the decode and its
 *   records, then the encode's checksum kernels over the outputs that are structurally valid and fit, and a small kernel that
 *   compares them (and ISIZE) with the trailers: MI355_VERIFY_CHECKSUM.  A raw call waits once.
 * _batch_device: the direction is the natural one for a decoder and the REVERSE of mi355_deflate_verify_batch_device: in / in_len
 *   is the stream (the out pointers of a packed arena's items go here), out / out_cap the buffer; out_len and status are written,
 *   and reports[i] if reports is not NULL.  Items whose status on entry is not MI355_OK are skipped and left alone.  A failing item
 *   disturbs no neighbour; the call returns the first failing item's status.  One decode launch for all items, one workgroup per item.
 * Speed: ONE wave walks a whole stream, symbol after symbol, so a large single stream is slow; the entry points are
 *   made for many streams at once -- pages, tiles, the items of a batch.  For one large stream whose block table was kept:
 *   mi355_inflate_tabled[_device] below; for one large stream from anywhere: mi355_inflate_parallel[_device] below. */
typedef struct {
    uint32_t status;    /* MI355_VERIFY_OK, _FRAME, _BTYPE, _STORED, _LENGTHS, _CODE, _DISTANCE, _TRUNCATED, _TRAILER, _CHECKSUM
                           (never _MISMATCH, _LENGTH: there is no input), and _TABLE from mi355_inflate_tabled* */
    uint32_t reserved;  /* 0 */
    uint64_t bit;       /* raw-deflate bit offset where the failing element begins (verify's rule) */
    uint64_t out_pos;   /* bytes produced before the failing element; == out_len when OK */
    uint64_t out_len;   /* bytes the stream inflates to (OK, and OUT_TOO_SMALL: the exact size needed); 0 after a failure */
    uint64_t n_blocks;  /* not after a failure: deflate blocks decoded (a stored piece counts as one) */
    uint32_t n_stored, n_fixed, n_dynamic;
    float ms;           /* host clock over the call */
} mi355_inflate_report; /* 56 bytes */

int mi355_inflate_device(mi355_deflate_ctx* ctx, const void* d_stream, size_t stream_len, int wrapper, void* d_out, size_t out_cap,
                         size_t* out_len, mi355_inflate_report* report, void* hip_stream);
int mi355_inflate(mi355_deflate_ctx* ctx, const uint8_t* stream, size_t stream_len, int wrapper, uint8_t* out, size_t out_cap,
                  size_t* out_len, mi355_inflate_report* report);
int mi355_inflate_batch_device(mi355_deflate_ctx* ctx, mi355_batch_item* items, size_t n_items, int wrapper,
                               mi355_inflate_report* reports /* n_items entries, or NULL */, void* hip_stream);

/* ---- tabled inflate: ONE large stream decoded in parallel from its encoder block table ---------------------
 * The way back for a stream this library encoded and whose block table the caller kept (mi355_deflate_last_blocks): entry e of the
 * table starts at bit bit_start[e] and at output position sum of in_bytes[k], k < e, so every entry is decoded by a wave of its own
 * -- into 16-bit symbols, a byte or "byte j of the 32 KiB in front of this entry" --, one workgroup then makes the resolved 32 KiB
 * window behind every entry, one entry after the other, and a flat launch turns symbols into bytes.  Nothing waits inside a kernel.
 * The contract is mi355_inflate[_device]'s: wrappers and framing rules, MI355_OK / MI355_E_DATA / MI355_E_OUT_TOO_SMALL with the
 *   exact size (the table's sum, once every entry has been found to end where the next begins), the size query, out[0, min(out_pos,
 *   out_cap)) = the data decoded in front of the first failure and nothing at or beyond it, the trailer's checksum judged over the
 *   output, MI355_E_STATE / _ARG / _HIP / _UNSUPPORTED as there.
 * The table's rules are verify's: only bit_start and in_bytes are read; blocks in HOST memory; bit_start values that do not ascend
 *   are MI355_E_ARG, and so is a first entry that does not begin at bit 0 (like every argument error of a tabled call, decided
 *   before a context or the device is touched; mi355_deflate_last_error of the context given has the reason); n_blocks == 0 or
 *   blocks == NULL means no table and the call IS mi355_inflate[_device].
 * MI355_VERIFY_TABLE is a status a tabled inflate reports: an entry's last block does not end exactly at the next entry's bit and
 *   output position, a token would pass that position, BFINAL before the last entry, or the BFINAL block ends at a position other
 *   than the sum of in_bytes.  Because entry 0 must begin at bit 0 and every entry must end exactly where the next begins, a table
 *   that passes describes the one serial walk of the stream: a wrong table never yields wrong bytes with MI355_OK.  The report is the first failing entry's in
 *   stream order; on success the block counts are the sums over the entries.
 * Entries are worked on in groups of consecutive entries -- MI355_CFG_INFLATE_GROUP_BYTES output bytes or 4096 entries, whichever
 *   comes first -- with a workspace of two bytes per output byte of the group plus 32 KiB per entry; one wait per group, and one
 *   more for the checksum of a framed stream. */
int mi355_inflate_tabled_device(mi355_deflate_ctx* ctx, const void* d_stream, size_t stream_len, int wrapper,
                                const mi355_block_info* blocks, size_t n_blocks, void* d_out, size_t out_cap, size_t* out_len,
                                mi355_inflate_report* report, void* hip_stream);
int mi355_inflate_tabled(mi355_deflate_ctx* ctx, const uint8_t* stream, size_t stream_len, int wrapper,
                         const mi355_block_info* blocks, size_t n_blocks, uint8_t* out, size_t out_cap, size_t* out_len,
                         mi355_inflate_report* report);
/* Diagnostics, for tools/inflate_table_bench.py -- a measuring aid, not part of the stable interface, and it may change with the
 * kernels it times: HIP-event milliseconds of the context's last tabled call per launch kind, summed over its groups -- ms[0] the decode
 * (a wave per entry), ms[1] the window chain, ms[2] the resolve, ms[3] the checksum half of a framed call.  Zeros unless the stage
 * clocks were on for the call (MI355_CFG_STAGE_CLOCKS = 1, or 2 for tables of 32 MiB or more). */
int mi355_inflate_tabled_last_stages(mi355_deflate_ctx* ctx, float ms[4]);

/* ---- index and parallel inflate: the block table of ANY large stream, found on the device -------------------
 * A stream that this library did not encode, or whose table was not kept -- a .gz from disk, a zlib stream from anywhere -- gets its
 * table here.  The deflate data behind the frame header is cut into spans of MI355_CFG_INFLATE_INDEX_SPAN_BYTES compressed bytes.
 * One wave per span finds the span's candidate: the smallest bit offset in it at which a NON-FINAL DYNAMIC block with a valid header
 * (the rules of MI355_VERIFY_LENGTHS) begins, the header wholly inside the stream; span 0's candidate is the first deflate bit.  One
 * wave per candidate then decodes from it on, counting and storing nothing, until it stands on the candidate of a later span, behind
 * the BFINAL block or at a failure.  The host follows the links from span 0: that chain is the stream's one serial walk, and its
 * walkers are the table's entries.  Stored and fixed blocks are not searched for, so a stretch without a non-final dynamic block
 * start (fixed only, stored only, one Huffman-only block) is ONE entry walked by one wave and costs what mi355_inflate costs.
 * mi355_inflate_index[_device]: the table, in HOST memory, as mi355_inflate_tabled and mi355_deflate_verify take it: bit_start,
 *   in_bytes, btype of the entry's first block, bfinal = 1 on the last entry of a chain that reached the BFINAL block, the other
 *   fields 0.  *n_blocks = the count, never more than the number of spans; cap too small: MI355_E_OUT_TOO_SMALL and the count needed
 *   (cap == 0 with blocks == NULL is the query).  A stream whose chain fails: MI355_E_DATA, the entries up to and including the failing
 *   link (its in_bytes = the bytes counted in front of the failure) and the failure in the report, out_pos = the bytes in front of
 *   it.  What the index cannot see -- a distance that reaches in front of the stream, bytes behind the BFINAL block, the checksum --
 *   the decode judges.  Wrappers and frame rules, MI355_E_ARG (decided before a context or the device is touched) / _STATE / _HIP:
 *   the tabled call's; more than 2^31 - 1 spans are MI355_E_UNSUPPORTED.  last_info / last_blocks / last_batch_info are left alone.
 * mi355_inflate_parallel[_device]: the index, then the tabled inflate from its table (a table of one entry: mi355_inflate itself).
 *   The contract is mi355_inflate[_device]'s on every stream, valid or not: return value, *out_len, every report field but ms, the
 *   bytes of out, nothing at or beyond out_pos or out_cap.  The tabled pass refuses a table that is not the serial walk, so a wrong
 *   candidate costs time and never a byte. */
int mi355_inflate_index_device(mi355_deflate_ctx* ctx, const void* d_stream, size_t stream_len, int wrapper, mi355_block_info* blocks,
                               size_t cap, size_t* n_blocks, mi355_inflate_report* report, void* hip_stream);
int mi355_inflate_index(mi355_deflate_ctx* ctx, const uint8_t* stream, size_t stream_len, int wrapper, mi355_block_info* blocks, size_t cap,
                        size_t* n_blocks, mi355_inflate_report* report);
int mi355_inflate_parallel_device(mi355_deflate_ctx* ctx, const void* d_stream, size_t stream_len, int wrapper, void* d_out, size_t out_cap,
                                  size_t* out_len, mi355_inflate_report* report, void* hip_stream);
int mi355_inflate_parallel(mi355_deflate_ctx* ctx, const uint8_t* stream, size_t stream_len, int wrapper, uint8_t* out, size_t out_cap,
                           size_t* out_len, mi355_inflate_report* report);
/* Diagnostics, measuring aids like mi355_inflate_tabled_last_stages and no part of the stable interface.  _last_stages: milliseconds of
 * the context's last index: ms[0] the find launch, ms[1] the walk launch (HIP events; zeros unless the stage clocks were on), ms[2]
 * the host's link.  _last_walks: the walkers' records of the last index, one per span of the whole stream's length. */
typedef struct {
    uint64_t start;    /* the span's candidate, a raw-deflate bit offset; UINT64_MAX: none */
    uint64_t end_bit;  /* where the walk stopped */
    uint64_t count;    /* output bytes counted */
    uint32_t how;      /* 0 linked to span `link`, 1 behind the BFINAL block, 2 failed, 3 no candidate */
    uint32_t link;
    uint32_t btype;    /* of the first block */
    uint32_t status;   /* the failure: MI355_VERIFY_* */
    uint32_t n_stored, n_fixed, n_dynamic, reserved;
    uint64_t n_blocks;
    uint64_t bit;      /* the failure's bit */
    uint64_t in_pos;   /* ... and the bytes counted in front of it */
} mi355_index_walk; /* 80 bytes */
int mi355_inflate_index_last_stages(mi355_deflate_ctx* ctx, float ms[3]);
int mi355_inflate_index_last_walks(mi355_deflate_ctx* ctx, mi355_index_walk* out, size_t cap, size_t* n_spans);

/* ---- members: a gzip FILE, any number of members, BGZF members in parallel ------------------------------------
 * RFC 1952 defines a gzip file as a sequence of members; mi355_inflate (wrapper 2) takes exactly one.  These calls take the
 * sequence: BGZF (bgzip: BAM, tabix-indexed VCF), `cat a.gz b.gz`, and an arena of mi355_deflate_encode_batch_packed_device with gzip
 * members whose regions lie back to back (pad bytes between regions would be the next member's FRAME).  No reference item: the reference has no decoder.
 * The contract is the SERIAL WALK, whatever path produced a result:
 *     o = 0, p = 0, m = 0
 *     do:  member m begins at byte o.  Its header is mi355_inflate's gzip header (same rules), parsed on stream[o, stream_len);
 *          failure, or fewer than 18 bytes left: MI355_VERIFY_FRAME (bit 0, out_pos p).
 *          Its deflate blocks run through the BFINAL block, by mi355_inflate's rules and statuses; `bit` is counted from the member's
 *          first deflate bit, and a distance is limited by the bytes THIS member has produced.
 *          The 8 trailer bytes follow the byte in which the BFINAL block ends: bits needed from the file's last 8 bytes on are
 *          MI355_VERIFY_TRUNCATED.  CRC-32 and ISIZE are of this member's output alone: MI355_VERIFY_CHECKSUM.
 *          o = end of trailer, p += the member's output, m += 1
 *     while o < stream_len
 *   An empty file is FRAME.  Bytes behind a member that do not begin another member are that next member's FRAME: there is no
 *   special case for zero padding (Python and GNU gzip skip it; these calls stay strict, as mi355_inflate is about trailing bytes).
 *   Empty members (BGZF's 28-byte end-of-file marker) are legal anywhere.
 * Return value, over the whole file, as mi355_inflate's:
 *   MI355_OK               the file decoded and fits.
 *   MI355_E_DATA           the first failure in file order (a CHECKSUM failure of member j comes before a structural failure of a
 *                          member k > j); report.out_pos = the bytes produced in front of the failing element over all members, *out_len
 *                          = min(out_pos, out_cap), the leading bytes of out that hold data.  A member's checksum is judged when
 *                          all of its output was stored (it ends at or below out_cap).  DIFFERENT from mi355_inflate: the bytes of
 *                          out[*out_len, out_cap) are unspecified -- members behind the failure may have been written already.
 *   MI355_E_OUT_TOO_SMALL  every member is structurally valid and the total is larger than out_cap: *out_len is the exact total,
 *                          out[0, out_cap) holds the first out_cap bytes, no checksum or ISIZE is judged.  out == NULL with out_cap
 *                          == 0 is the size query.
 *   MI355_E_UNSUPPORTED    a member that inflates to more than 4 GiB - 64 KiB (the checksum kernels' limit).
 *   In every outcome nothing at or beyond out_cap is ever stored.  MI355_E_ARG (decided before a context or the device is touched)
 *   / _STATE / _HIP, ctx == NULL, _device and host pointers, hip_stream: as in the inflate family.
 * members (HOST memory, may be NULL with members_cap 0): one entry per member walked; *n_members (may be NULL) = their count -- after
 *   MI355_E_DATA the failing member's index + 1, that entry carrying the status, in_len 0 unless the failure is CHECKSUM, and in out_len
 *   the bytes counted in front of the failure.  The table is cut at members_cap without an error; the count is still the full one.
 * report: mi355_inflate_report; on success the block counts are the sums over the members; reserved stays 0.  For a file of ONE
 *   member the return value, *out_len, every report field but ms, and the bytes equal mi355_inflate(..., wrapper 2, ...), with one
 *   exception: bytes behind the trailer are the next member's FRAME here and TRAILER there.
 * How: a member that states its own size -- FEXTRA with a subfield 'B','C' of length 2 holding BSIZE = size - 1, as BGZF's -- is
 *   HINTED.  The file is cut into spans of MI355_CFG_INFLATE_MEMBER_SPAN_BYTES; a wave per span finds the first hinted offset in it,
 *   a lane per span hops from header to header, the host links the hops into the run of members from the current position, and the run
 *   is decoded by the batched one-wave inflate, member k at the sum of the ISIZEs in front of it.  A hint is a claim and never
 *   trusted for a byte: the run is accepted up to the first member that is not both structurally clean and exactly ISIZE bytes
 *   long, and from there one wave walks member after member, open ended, until a hinted header follows again (at most 8 such
 *   returns a call, which bounds the launches an adversarial file can cost and changes no result).  The checksums: one pass of the
 *   batch's checksum launches over the member table.
 *   The third path, for members that state no size (`cat a.gz b.gz`, rotated logs, this library's packed gzip arena): where at
 *   least MI355_CFG_INFLATE_MEMBER_PARALLEL_BYTES are left in the file, the member's end is DISCOVERED -- the finder and the walkers
 *   of mi355_inflate_index over a bounded extent of MI355_CFG_INFLATE_INDEX_SPAN_BYTES spans behind its header, the extent doubling
 *   while the chain of walkers runs into its edge -- and with it the member's size, its block table and the next member's start.
 *   The tables of all members so found are decoded together by the three passes of mi355_inflate_tabled, in groups of
 *   MI355_CFG_INFLATE_GROUP_BYTES that may hold many members: a wave per table entry, a window chain per member, one resolve.  A
 *   member found is never trusted for a byte either: the first one that is not clean, in discovery or in decode, and everything
 *   behind it go back to the one wave, whose results are the call's.  A member shorter than the setting ends discovery, so a file of
 *   many small plain members costs one discovery a launch of the one wave and not one a member. */
#define MI355_MEMBER_HINTED 1u   /* the member's size was taken from its BC subfield and found true */
typedef struct {
    uint64_t in_off, in_len;     /* the member in the file, header through trailer */
    uint64_t out_off, out_len;   /* its data in the output */
    uint32_t flags, status;      /* MI355_MEMBER_*; MI355_VERIFY_* of this member */
} mi355_member_info;             /* 40 bytes */
int mi355_inflate_members_device(mi355_deflate_ctx* ctx, const void* d_stream, size_t stream_len, void* d_out, size_t out_cap,
                                 size_t* out_len, mi355_member_info* members, size_t members_cap, size_t* n_members,
                                 mi355_inflate_report* report, void* hip_stream);
int mi355_inflate_members(mi355_deflate_ctx* ctx, const uint8_t* stream, size_t stream_len, uint8_t* out, size_t out_cap, size_t* out_len,
                          mi355_member_info* members, size_t members_cap, size_t* n_members, mi355_inflate_report* report);
/* A measuring aid like mi355_inflate_index_last_stages: HIP-event milliseconds of the context's last members call per launch kind,
 * summed over its launches -- find, walk, fill, member decode, chain decode, checksums; zeros unless the stage clocks were on. */
int mi355_inflate_members_last_stages(mi355_deflate_ctx* ctx, float ms[6]);
/* Measuring aids and no part of the stable interface: the third path in the context's last members call.  v: members decoded by the
 * parallel path, members handed back to the one-wave chain, index spans searched, walkers launched, table entries decoded, launch
 * sets (groups).  ms: HIP-event milliseconds per launch kind, summed over the call's launches -- discovery find, discovery walk,
 * tabled decode, window chains, resolve; zeros unless the stage clocks were on.  (The one wave's time stays in slot 4 of
 * mi355_inflate_members_last_stages.) */
int mi355_inflate_members_last_parallel(mi355_deflate_ctx* ctx, uint64_t v[6]);
int mi355_inflate_members_last_parallel_stages(mi355_deflate_ctx* ctx, float ms[5]);
/* A measuring aid like mi355_inflate_index_last_walks and no part of the stable interface: what the find and the first walk of the
 * context's last members call (the run from byte 0) left on the device, one of each per span of the file -- cand[k], the span's
 * candidate (UINT64_MAX: none), and walks[k], its walker's record.  *n_spans = their count (0 behind an empty file or a call that
 * failed in front of its walk); more than cap: MI355_E_OUT_TOO_SMALL and nothing is written. */
typedef struct {
    uint64_t start;      /* where the walker began: byte 0 in span 0, else the span's candidate; UINT64_MAX: none */
    uint64_t end;        /* where it stopped */
    uint64_t n_members;  /* members hopped over */
    uint64_t out_bytes;  /* the sum of their ISIZEs */
    uint32_t how;        /* 0 linked to span `link`, 1 the end of the file, 2 a byte that is not hinted, 3 no candidate */
    uint32_t link;
} mi355_member_walk; /* 40 bytes */
int mi355_inflate_members_last_walks(mi355_deflate_ctx* ctx, uint64_t* cand, mi355_member_walk* walks, size_t cap, size_t* n_spans);

/* ---- BGZF encode: one input, one blocked gzip file (the write side of the members calls above) ---------------
 * The file bgzip writes and htslib, `gzip -d` and mi355_inflate_members read: the input cut into slices of block_size bytes, every
 * slice a gzip member that states its own size, the members back to back without a byte between them, the 28-byte end-of-file
 * marker last.  With H = 1f 8b 08 04 00 00 00 00 00 ff 06 00 42 43 02 00 00 00 (FEXTRA, MTIME 0, XFL 0, OS 255, XLEN 6, subfield
 * 'B','C' of length 2):
 *     member k = mi355_deflate_encode_gzip(in[k * B, min((k + 1) * B, in_len)), opts, hdr = H)     deflate_bytes_gzip_conf, src/lib.rs:242-267
 *     with bytes 16..17 replaced by the little-endian 16-bit value len(member k) - 1 (BSIZE)
 *     marker   = 1f 8b 08 04 00 00 00 00 00 ff 06 00 42 43 02 00 1b 00 03 00 00 00 00 00 00 00 00 00   (the same call on the empty input)
 * block_size B: 1 to 65280; 0 means 65280 (bgzip's 0xff00).  in_len == 0 gives the marker alone.  A member of at most 65280 input
 *   bytes is at most 65321 bytes long, which BSIZE can express; the device still checks, and a member longer than 65536 bytes makes
 *   the call return MI355_E_UNSUPPORTED with no valid file promised.
 * opts: every level, MI355_FLUSH_FINISH only; opts->wrapper is taken as 2 whatever it holds, as the _gzip entries do.  The other
 *   checks are the packed batch's: lazy_if_less_than < 3 with Lazy is MI355_E_UNSUPPORTED, a live shard is MI355_E_STATE.
 *   MI355_E_ARG is decided before the device is touched: a NULL ctx (these calls take no default context), opts or out_len,
 *   block_size > 65280, a NULL input with in_len > 0, a NULL buffer with out_cap > 0 or a NULL table with members_cap > 0, and
 *   (_device) a d_out that is not 16-byte aligned.
 * Capacity: *out_len is always the exact size of the file.  out_cap >= mi355_bgzf_bound(in_len, block_size) always succeeds -- the
 *   sum of the members' mi355_deflate_bound_ex(len_k, 2, 18, 0) plus 28, computed without a GPU; 0 for a bad block_size -- and so does
 *   a smaller one that still holds the file.  One that does not: MI355_E_OUT_TOO_SMALL, out[0, out_cap) unspecified, and nothing at
 *   or beyond out_cap is ever stored.  out == NULL with out_cap == 0 is the size query: it runs the encode and answers
 *   MI355_E_OUT_TOO_SMALL with the size (a file is never empty: the marker alone is 28 bytes).
 * members (HOST memory, may be NULL with members_cap 0): mi355_member_info, one entry per member in file order, the marker last with
 *   out_len 0; flags MI355_MEMBER_HINTED and status 0 in every entry: after a successful call the table mi355_inflate_members
 *   returns for the file.  Cut at members_cap without an error; *n_members (may be NULL) is the full count.
 * A member on which the reference panics under MI355_COMPAT_Q13 fails the whole call with MI355_E_REF_PANIC (*out_len 0).
 * How: the slices are the items of the packed batch above (wrapper 2, the one header H, align 4) in an arena the context owns; one
 *   workgroup then scans the members' exact lengths in slice order into file offsets, and one launch moves every member from its
 *   aligned region to its byte offset, writes BSIZE on the way and appends the marker.  Routing of the slices (the batched kernels
 *   or the one-input path, MI355_CFG_BATCH_BYTES) is the packed batch's and is not visible in the result;
 *   mi355_deflate_last_info, _last_batch_info and _last_blocks read as after that packed batch.
 * _device: d_in / d_out are device pointers, hip_stream NULL = the context's stream; the call returns after the stream has drained.
 * mi355_bgzf_encode: host pointers, staged with plain copies. */
size_t mi355_bgzf_bound(size_t in_len, size_t block_size);
int mi355_bgzf_encode_device(mi355_deflate_ctx* ctx, const void* d_in, size_t in_len, const mi355_deflate_opts* opts, size_t block_size,
                             void* d_out, size_t out_cap, size_t* out_len, mi355_member_info* members, size_t members_cap,
                             size_t* n_members, void* hip_stream);
int mi355_bgzf_encode(mi355_deflate_ctx* ctx, const uint8_t* in, size_t in_len, const mi355_deflate_opts* opts, size_t block_size,
                      uint8_t* out, size_t out_cap, size_t* out_len, mi355_member_info* members, size_t members_cap, size_t* n_members);
/* A measuring aid like mi355_inflate_members_last_stages: HIP-event milliseconds of the context's last BGZF encode -- the packed
 * encode, the place, the gather; zeros unless the stage clocks were on (MI355_CFG_STAGE_CLOCKS). */
int mi355_bgzf_last_stages(mi355_deflate_ctx* ctx, float ms[3]);

/* ---- seek points: any byte range of ONE large stream, decoded from the nearest restart point ---------------
 * mi355_inflate_parallel gives back a whole stream; these calls give back PART of one without an output buffer for the rest and
 * without decoding the rest.  A handle keeps the stream's table (the caller's, or the one mi355_inflate_index finds) and, for some
 * of its entries -- the POINTS --, the resolved 32 KiB of output in front of them: decoding from a point needs nothing before it.
 * Point rule: entry 0 is a point (its window is zeros and is not stored); entry k > 0 is a point iff its output position lies
 *   `spacing` bytes or more behind the last point's.  spacing: output bytes, 0 = 1 MiB (zran's convention; derived, not measured),
 *   else 32 KiB to 1 GiB; anything else is MI355_E_ARG.  A handle holds 16 bytes per entry on the host and 32 KiB per point on the
 *   device (mi355_inflate_seek_info).
 * _build[_device]: the tabled decode of the whole stream, group by group (MI355_CFG_INFLATE_GROUP_BYTES), without an output buffer.
 *   blocks == NULL (or n_blocks == 0): the table is found as mi355_inflate_index finds it; else the caller's table under
 *   mi355_inflate_tabled's rules.  Every structural status of mi355_inflate_tabled (MI355_VERIFY_TABLE included) is the build's, and
 *   for wrapper 1 / 2 every group is resolved into a scratch region, summed by the checksum kernels, and the sums are folded
 *   (mi355_checksum_combine) and compared with the trailer and ISIZE: MI355_VERIFY_CHECKSUM.  Because the sums are per group a framed
 *   stream may inflate to more than 4 GiB - 64 KiB; a single GROUP above that is MI355_E_UNSUPPORTED.  A stream that fails:
 *   MI355_E_DATA, the report, *seek = NULL.  MI355_OK: report.out_len = the stream's size and *seek is the handle, to be freed with
 *   mi355_inflate_seek_free before its context is destroyed.  Argument errors are decided before a context or the device is touched;
 *   a live shard is MI355_E_STATE; build and reads leave mi355_deflate_last_info / _last_blocks / _last_batch_info alone.
 *   _device never keeps the stream: the caller passes it again at each read.  The host form keeps a device copy in the handle
 *   (d_stream = NULL at a _device read means that copy), and mi355_inflate_seek_read copies the bytes back.
 * _read*: pread.  *got = min(len, total - off), 0 when off >= total -- which is MI355_OK, as is len == 0.  MI355_OK: out[0, got) are
 *   the stream's bytes [off, off + got); report.out_len = got, report.out_pos = the stream position reached, the block counts are
 *   those of the entries decoded.  The range decodes the entries from the last point at or before `off` through the entry that holds
 *   its last byte; a range of more than MI355_CFG_INFLATE_GROUP_BYTES symbols is cut at points into pieces, each from its own point.
 *   If the stream passed no longer decodes as it did at the build: MI355_E_DATA, the report is the first failing entry's among those
 *   decoded (out_pos a position of the stream), *got = the bytes that hold data, out[0, max(out_pos, off) - off) clipped to len, and
 *   nothing is stored at or beyond that.  No store ever lands at or beyond out + len.  NO CHECKSUM IS JUDGED ON A READ: damage that
 *   leaves every decoded entry structurally valid and ending where the table says is not noticed.
 * _read_batch_device: n ranges through ONE launch set -- three launches and one wait; more sets only when their symbols exceed the
 *   group budget.  got and status are written per range, reports[i] if reports is not NULL; a failing range disturbs no neighbour; the
 *   call returns the first failing status.  Overlapping out buffers are undefined. */
typedef struct mi355_inflate_seek mi355_inflate_seek; /* owns: the table (host), one 32 KiB window per point (device) */
typedef struct {
    uint64_t total;        /* bytes the stream inflates to */
    uint64_t n_entries;    /* of the table */
    uint64_t n_points;     /* entry 0 included */
    uint64_t spacing;      /* the one in force */
    uint64_t device_bytes; /* held on the device: the windows, and the host form's copy of the stream */
    uint64_t stream_len;
    uint32_t wrapper, reserved;
} mi355_seek_info; /* 56 bytes */
typedef struct {
    uint64_t bit; /* raw-deflate bit offset of the point's entry */
    uint64_t pos; /* its output position */
} mi355_seek_point; /* 16 bytes */
typedef struct {
    uint64_t off, len;
    void* out;        /* device memory, len bytes */
    uint64_t got;     /* written */
    int32_t status;   /* written: MI355_OK or MI355_E_DATA */
    uint32_t reserved;
} mi355_seek_range; /* 40 bytes */
int mi355_inflate_seek_build_device(mi355_deflate_ctx* ctx, const void* d_stream, size_t stream_len, int wrapper,
                                    const mi355_block_info* blocks, size_t n_blocks, uint64_t spacing, mi355_inflate_seek** seek,
                                    mi355_inflate_report* report, void* hip_stream);
int mi355_inflate_seek_build(mi355_deflate_ctx* ctx, const uint8_t* stream, size_t stream_len, int wrapper,
                             const mi355_block_info* blocks, size_t n_blocks, uint64_t spacing, mi355_inflate_seek** seek,
                             mi355_inflate_report* report);
void mi355_inflate_seek_free(mi355_inflate_seek* seek);
int mi355_inflate_seek_info(mi355_inflate_seek* seek, mi355_seek_info* info);
int mi355_inflate_seek_points(mi355_inflate_seek* seek, mi355_seek_point* out, size_t cap, size_t* n); /* cap too small: MI355_E_OUT_TOO_SMALL and *n */
int mi355_inflate_seek_read_device(mi355_inflate_seek* seek, const void* d_stream, uint64_t off, uint64_t len, void* d_out, uint64_t* got,
                                   mi355_inflate_report* report, void* hip_stream);
int mi355_inflate_seek_read(mi355_inflate_seek* seek, uint64_t off, uint64_t len, uint8_t* out, uint64_t* got, mi355_inflate_report* report);
int mi355_inflate_seek_read_batch_device(mi355_inflate_seek* seek, const void* d_stream, mi355_seek_range* ranges, size_t n,
                                         mi355_inflate_report* reports /* n entries, or NULL */, void* hip_stream);
/* A measuring aid and no part of the stable interface: what the handle's last read did, from its plan -- v[0] entries decoded, v[1]
 * symbols stored (lead-ins included), v[2] window steps, v[3] launch sets. */
int mi355_inflate_seek_last_read(mi355_inflate_seek* seek, uint64_t v[4]);
/* CUTS (MI355_CFG_INFLATE_SEEK_CUT_BYTES at the build).  A table entry begins at a block header, so a read costs
 * what one wave needs for the blocks of the entries it touches, and a stream of fixed or stored blocks is ONE entry.  With the key set
 * the build's walk remembers places INSIDE the entries where a wave may begin: a cut is (bit, pos, hdr_bit) -- where decoding resumes,
 * the output position there, and the bit of the 3-bit header of the block it lies in; bit == hdr_bit: the cut stands at a block
 * header, otherwise at a token start of a fixed or dynamic block, whose header the wave parses again for its tables.  Rule: the first
 * cut of an entry is its start; the walk records a cut at every block header and token start whose output position lies cut_bytes
 * or more behind the entry's last cut.  The handle keeps 24 bytes per cut on the host.  Points stay entries.
 * A read of such a handle is four launches and one wait a set: a wave per cut from the point's entry through the cut that holds the
 * range's last byte, a pass that makes every entry's symbols what one wave would have left and checks that each cut ended where and
 * in the block its successor begins, then the window and resolve passes as without cuts.  Bytes, got and status of a stream that
 * decodes as it did at the build are those of a handle without cuts; the report's block counts are those of the cuts decoded.
 * Otherwise: MI355_E_DATA, the report is the first failing cut's in stream order (a cut that does not meet its successor:
 * MI355_VERIFY_TABLE), nothing is stored at or beyond it, and nothing ever at or beyond out + len.  The build's status, report and
 * points do not depend on the key.
 * _cuts: the cuts in stream order (cap too small: MI355_E_OUT_TOO_SMALL and *n); none when the handle was built with the key at 0.
 * _cut_info: v[0] the cut_bytes in force, v[1] cuts, v[2] host bytes they take, v[3] the output bytes of the largest cut.
 * _last_read_cuts, a measuring aid like _last_read: v[0] cuts decoded, v[1] symbols stored, v[2] cuts the flatten pass rewrote (those
 * behind their entry's first), v[3] kernel launches. */
typedef struct {
    uint64_t bit;     /* raw-deflate bit offset where decoding resumes */
    uint64_t pos;     /* the output position there */
    uint64_t hdr_bit; /* the header bit of the block it lies in; == bit: at a block header */
} mi355_seek_cut; /* 24 bytes */
int mi355_inflate_seek_cuts(mi355_inflate_seek* seek, mi355_seek_cut* out, size_t cap, size_t* n);
int mi355_inflate_seek_cut_info(mi355_inflate_seek* seek, uint64_t v[4]);
int mi355_inflate_seek_last_read_cuts(mi355_inflate_seek* seek, uint64_t v[4]);
/* A measuring aid: HIP-event milliseconds per launch kind of the context's last seek read, summed over its sets -- pass 1 (entries, or
 * cuts), flatten (0 without cuts), windows, resolve; zeros unless the stage clocks were on for the call (MI355_CFG_STAGE_CLOCKS). */
int mi355_inflate_seek_last_read_stages(mi355_deflate_ctx* ctx, float ms[4]);

/* ---- BGZF reads: byte ranges of a blocked gzip file from a member index ------------------------------------------
 * What BGZF exists for, and what htslib's bgzf_useek / bgzf_seek + bgzf_read do: a byte range of the UNCOMPRESSED data, decoding
 * only the members that hold it, with no output buffer for the rest of the file and -- in the host form -- no copy of the rest.
 * THE INDEX (mi355_bgzf_index) is an opaque handle that holds the member table -- in_off, in_len, out_off, out_len per member -- in
 *   HOST memory and nothing on the device.  It is bound to no context: one index serves several contexts or GPUs.
 *   _index_build[_device]: Path A of the members calls from byte 0 -- find, walk, link on the host, fill, with the kernels and the
 *     span setting (MI355_CFG_INFLATE_MEMBER_SPAN_BYTES) of mi355_inflate_members -- and NOTHING is decoded.  The run must reach the
 *     end of the file: a byte that begins no hinted member, or an empty file, is MI355_E_DATA with MI355_VERIFY_FRAME, *idx = NULL and
 *     report.out_pos = the sum of the ISIZEs in front of it.  MI355_OK: report.out_len = report.out_pos = the total; the report's
 *     block counts are 0 either way.  The host form stages the file as mi355_inflate_members does and keeps nothing of it.
 *   _index_from_members: the table mi355_bgzf_encode or a successful mi355_inflate_members returned; no GPU and no context.  The
 *     table may describe any gzip file of members (MI355_MEMBER_HINTED is not required).  MI355_E_ARG unless n >= 1, every status
 *     is 0, in_off[0] == 0, in_off[k + 1] == in_off[k] + in_len[k], the last member ends at file_len, out_off[0] == 0,
 *     out_off[k + 1] == out_off[k] + out_len[k] and every in_len >= 18.
 *   _index_info: the total, the members, file_len, the host bytes held, the largest out_len.  _index_members: the table (a cap that
 *     is too small: MI355_E_OUT_TOO_SMALL and *n).  _index_free before nothing in particular: the index owns host memory only.
 *   WHAT AN INDEX IS: a built index holds the FILE'S OWN CLAIMS -- BSIZE, and ISIZE from the trailers --, as a .gzi does.  A read
 *     verifies every member it touches and NOTHING about members it does not touch: a lying ISIZE in an untouched member in front
 *     of a range shifts the range without notice.  An index made from the table of a completed mi355_inflate_members call holds
 *     verified offsets.
 *   Virtual offsets (host only; htslib's convention, coffset << 16 | offset inside the member).  _voffset(uoff): for uoff < total
 *     the member is the one with out_off <= uoff < out_off + out_len (never an empty one); uoff == total gives file_len << 16;
 *     uoff > total is MI355_E_ARG; a member with out_len > 65536 or in_off >= 2^48 is MI355_E_UNSUPPORTED.  _uoffset(voff): coffset
 *     must be a member's in_off with the low 16 bits below its out_len (0 is also taken for an empty member); coffset == file_len
 *     with low bits 0 gives the total; anything else is MI355_E_ARG.  A read at a virtual offset is a read at uoffset(voff).
 * READS are pread over the uncompressed bytes.  *got = min(len, total - off), 0 when off >= total -- which is MI355_OK, as is
 *   len == 0.  A range touches member k iff their byte intervals intersect; empty members are never touched.  Every touched member
 *   is decoded WHOLE by one wave, as a wrapper-2 stream on file[in_off, in_off + in_len) under the cap out_len the index claims, and
 *   is accepted only if it is structurally clean, exactly out_len bytes long and its CRC-32 and ISIZE match: unlike a seek read the
 *   checksum IS judged, because members are decoded whole.  Every touched member accepted: MI355_OK, out[0, got) are the bytes; the
 *   report's block counts are the sums over the touched members, out_len = got, out_pos = off + got.  Otherwise MI355_E_DATA and the
 *   report is the first failing touched member's in file order: its own status and bit with out_pos = out_off[k] + its out_pos for
 *   a structural failure inside its claim; MI355_VERIFY_TABLE with out_pos = out_off[k] for a member that is clean but not as long as
 *   claimed or that inflates beyond its claim; MI355_VERIFY_CHECKSUM with out_pos = out_off[k].  *got = max(out_pos, off) - off
 *   clipped to len, and out[*got, len) is unspecified.  In every outcome nothing is stored outside [out, out + len).
 *   A member wanted by exactly one range that covers all of it is decoded in place, straight into out; every other member is decoded
 *   into a scratch slot of the context's workspace and the wave that decoded it copies the slices asked for.  A member is decoded once
 *   per call however many ranges want it.  Launch sets hold at most 16384 members and MI355_CFG_INFLATE_GROUP_BYTES of scratch; a
 *   range that wants a scratch member whose claim exceeds that budget, or any member above 4 GiB - 64 KiB, is MI355_E_UNSUPPORTED
 *   (status of the range, got 0) -- BGZF never gets there.
 *   _read_batch_device: got and status are written per range, reports[i] if reports is not NULL; a failing range disturbs no
 *   neighbour; the call returns the first failing status.  Overlapping out buffers are undefined.  MI355_E_ARG is decided before the
 *   device is touched (a NULL index, got or report, a NULL out with len > 0, a NULL file of a file_len > 0); a live shard is
 *   MI355_E_STATE; mi355_deflate_last_info / _last_blocks / _last_batch_info are left alone.  ctx NULL is the default context.
 *   mi355_bgzf_read (host pointers) copies to the device only the compressed extent from the first through the last touched member,
 *   and copies back got bytes. */
typedef struct mi355_bgzf_index mi355_bgzf_index; /* owns: the member table (host) */
typedef struct {
    uint64_t total;       /* bytes the file inflates to, as the table claims */
    uint64_t n_members;
    uint64_t file_len;
    uint64_t host_bytes;  /* held by the index */
    uint64_t max_out_len; /* the largest member's out_len */
} mi355_bgzf_info; /* 40 bytes */
int mi355_bgzf_index_build_device(mi355_deflate_ctx* ctx, const void* d_file, size_t file_len, mi355_bgzf_index** idx,
                                  mi355_inflate_report* report, void* hip_stream);
int mi355_bgzf_index_build(mi355_deflate_ctx* ctx, const uint8_t* file, size_t file_len, mi355_bgzf_index** idx, mi355_inflate_report* report);
int mi355_bgzf_index_from_members(const mi355_member_info* members, size_t n, size_t file_len, mi355_bgzf_index** idx);
void mi355_bgzf_index_free(mi355_bgzf_index* idx);
int mi355_bgzf_index_info(const mi355_bgzf_index* idx, mi355_bgzf_info* info);
int mi355_bgzf_index_members(const mi355_bgzf_index* idx, mi355_member_info* out, size_t cap, size_t* n);
int mi355_bgzf_voffset(const mi355_bgzf_index* idx, uint64_t uoff, uint64_t* voff);
int mi355_bgzf_uoffset(const mi355_bgzf_index* idx, uint64_t voff, uint64_t* uoff);
int mi355_bgzf_read_device(mi355_deflate_ctx* ctx, const mi355_bgzf_index* idx, const void* d_file, uint64_t off, uint64_t len, void* d_out,
                           uint64_t* got, mi355_inflate_report* report, void* hip_stream);
int mi355_bgzf_read(mi355_deflate_ctx* ctx, const mi355_bgzf_index* idx, const uint8_t* file, uint64_t off, uint64_t len, uint8_t* out,
                    uint64_t* got, mi355_inflate_report* report);
int mi355_bgzf_read_batch_device(mi355_deflate_ctx* ctx, const mi355_bgzf_index* idx, const void* d_file, mi355_seek_range* ranges, size_t n,
                                 mi355_inflate_report* reports /* n entries, or NULL */, void* hip_stream);
/* Measuring aids and no part of the stable interface.  _last_read: what the context's last BGZF read did -- v[0] distinct members
 * decoded, v[1] of them in place, v[2] to scratch, v[3] pieces copied, v[4] launch sets, v[5] compressed bytes a host read copied.
 * _last_read_stages: its HIP-event milliseconds per launch kind summed over the sets -- decode and clip, checksums, trailers; zeros
 * unless the stage clocks were on (MI355_CFG_STAGE_CLOCKS). */
int mi355_bgzf_last_read(mi355_deflate_ctx* ctx, uint64_t v[6]);
int mi355_bgzf_last_read_stages(mi355_deflate_ctx* ctx, float ms[3]);

/* ---- streaming inflate: decode a stream as it arrives, piece by piece ---------------------------------------------------
 * zlib's inflate() with Z_SYNC_FLUSH: the receiving end of mi355_deflate_stream_flush, of a MI355_FLUSH_SYNC chunk, of a long-lived
 * compressed connection.  A handle (mi355_inflate_stream) belongs to a context and holds, in DEVICE memory, the compressed bytes it
 * could not use yet -- everything from the byte that holds the COMMIT POINT, the end of the last block it handed over -- and a pair of
 * 32 KiB history buffers; on the host the totals, the running Adler-32 / CRC-32 and its state.
 * _new: wrapper 0 / 1 / 2 as everywhere, anything else MI355_E_ARG.  dict (host memory, may be NULL with dict_len 0): a preset
 *   dictionary for a RAW stream, the last 32768 bytes of which are the history in front of the first byte; dict_len > 0 with wrapper
 *   1 or 2 is MI355_E_ARG (a zlib stream with FDICT stays MI355_VERIFY_FRAME).  ONE gzip member.
 * A WRITE appends in[0, in_len) to the pending bytes, decodes from the commit point and hands over the bytes of every block that has
 *   become complete and fits:
 *   MI355_OK               out[0, *out_len) are the stream's next bytes; *out_len may be 0 (more input is needed); report.out_pos =
 *                          the bytes handed over since the stream began (state.total_out), report.out_len = *out_len.  If the write
 *                          committed some blocks and found the next complete one too large, state.need_out says what room suffices.
 *   MI355_E_OUT_TOO_SMALL  the next complete block does not fit and nothing could be committed: *out_len = 0, state.need_out = the
 *                          room that suffices (exact: the decode went on counting).  The input WAS taken: write(NULL, 0, a bigger
 *                          buffer) goes on.  out_cap == 0 with out == NULL is the query form.
 *   MI355_E_DATA           the report is mi355_inflate's: status, the ABSOLUTE raw-deflate bit and the absolute out_pos of the first
 *                          failing element; out[0, *out_len) holds the bytes in front of it that were not handed over before (the
 *                          prefix that fits out_cap).  The handle is dead: every later write and _finish is MI355_E_STATE until
 *                          _reset.  The checksum of a framed stream (MI355_VERIFY_CHECKSUM, Adler-32 / CRC-32 / ISIZE mod 2^32) is
 *                          judged at the write that completes the trailer, whose bytes are handed over all the same.
 *   After the stream's end (state.done) a write of 0 bytes is MI355_OK and bytes behind the end are MI355_E_DATA with
 *   MI355_VERIFY_TRAILER -- the one-shot's single-member rule; so are bytes behind the trailer in the write that completes it.
 *   No store lands in out at an index >= out_cap.  What runs out of input is never an error of a write: a header, a code, extra
 *   bits, a stored piece that is not all there yet leaves the handle waiting at its commit point.
 * GRANULARITY is the deflate block: a partial block is decoded again by the next write from its first bit, and none of its bytes is
 *   handed over before it is complete (the BFINAL block: before its trailer is).  The FLUSH GUARANTEE follows: after a write whose
 *   input ends at or behind a complete empty stored block (00 00 FF FF), or behind any block end, every byte the encoder had taken
 *   before that point has been handed over, given the room.  One wave walks a handle's bytes, so this is made for MANY handles with
 *   a small message each (_write_batch_device); one large stream belongs to mi355_inflate_parallel.
 * _finish: no more input will come.  MI355_OK if the stream is done; else MI355_E_DATA with MI355_VERIFY_FRAME (the header never
 *   completed) or MI355_VERIFY_TRUNCATED at the first element that could not be completed -- the deflate data is taken to be
 *   everything behind the header --, and the handle is dead.
 * _state_get: total_in (bytes written), total_out (bytes handed over), pending_in (compressed bytes held), need_out, done, failed
 *   (the MI355_VERIFY_* the handle died of), adler_or_crc (of the bytes handed over: Adler-32 for wrapper 1, CRC-32 for 2, 0 for 0).
 * _reset: same context, wrapper and dictionary, a new stream; revives a dead handle.  _free: NULL is fine.
 * _write_device: device pointers for in and out; hip_stream NULL = the context's stream; the call returns after it has drained.  A
 *   write of a raw stream is one launch and one wait: the wave also leaves the next history.  A framed write waits a second time when
 *   bytes were handed over: the encode's checksum kernels over them, folded on the host with mi355_checksum_combine.
 * _write_batch_device: items[i].in / in_len is the chunk for s[i], out / out_cap its room (device pointers); out_len and status are
 *   written, and reports[i] if reports is not NULL.  Items whose status on entry is not MI355_OK are skipped and left alone.  The
 *   handles must be distinct, not NULL and belong to ctx (ctx NULL: to the default context), else MI355_E_ARG before anything is
 *   touched.  One decode launch for all, one workgroup per handle; a failing or starved handle disturbs no neighbour; a dead handle's
 *   item gets MI355_E_STATE; the call returns the first failing item's status.
 * MI355_E_ARG is decided before the device is touched: a NULL handle, report or out_len, in == NULL with in_len > 0, out == NULL with
 *   out_cap > 0, a bad wrapper in _new.  A live shard on the handle's context is MI355_E_STATE.  More than 4 GiB - 64 KiB pending is
 *   MI355_E_UNSUPPORTED.  A stream write leaves mi355_deflate_last_info / _last_blocks / _last_batch_info alone;
 *   mi355_deflate_last_error of the handle's context gives one line.  A handle must be freed before its context is destroyed. */
typedef struct mi355_inflate_stream mi355_inflate_stream; /* owns: pending bytes and two 32 KiB histories (device) */
typedef struct {
    uint64_t total_in, total_out, pending_in, need_out;
    uint32_t done, failed, adler_or_crc, reserved;
} mi355_inflate_stream_state; /* 48 bytes */
int mi355_inflate_stream_new(mi355_deflate_ctx* ctx, int wrapper, const uint8_t* dict, size_t dict_len, mi355_inflate_stream** out);
int mi355_inflate_stream_write(mi355_inflate_stream* s, const uint8_t* in, size_t in_len, uint8_t* out, size_t out_cap, size_t* out_len,
                               mi355_inflate_report* report);
int mi355_inflate_stream_write_device(mi355_inflate_stream* s, const void* d_in, size_t in_len, void* d_out, size_t out_cap,
                                      size_t* out_len, mi355_inflate_report* report, void* hip_stream);
int mi355_inflate_stream_write_batch_device(mi355_deflate_ctx* ctx, mi355_inflate_stream* const* s, mi355_batch_item* items, size_t n,
                                            mi355_inflate_report* reports /* n entries, or NULL */, void* hip_stream);
int mi355_inflate_stream_finish(mi355_inflate_stream* s, mi355_inflate_report* report); /* no more input will come */
int mi355_inflate_stream_state_get(mi355_inflate_stream* s, mi355_inflate_stream_state* state);
int mi355_inflate_stream_reset(mi355_inflate_stream* s); /* same wrapper and dictionary, a new stream */
void mi355_inflate_stream_free(mi355_inflate_stream* s);

/* ---- sharded encode: ONE input over several GPUs, stream-exact (P1) ---------------------------
 * Rank r holds in device memory the bytes [global_lo, global_lo + n_ext) of the input: its own range
 * [parse_lo, parse_hi) (buffer coordinates; parse_lo = 32768 of history except on the first rank,
 * global_lo a multiple of 32768) plus >= 128 KiB of look-ahead except on the last rank (258 bytes of match
 * look-ahead, and a Stored block that begins in the range -- never more than ~110 KB -- must end inside it).  What the
 * reference's single loop threads through the stream (src/lz77.rs parse state, the 31744-value block
 * counter src/output_writer.rs:19, the bit position src/compress.rs:167) is exchanged between the
 * phases: a 576-entry exit table, token counts, <= 31743 straddling tokens, per-block costs.
 *   1. begin      links, match table, restart steps of the buffer; the range is parsed by speculation (its first
 *                 segment, like every other, finds its entry by a run-up of 128 positions into the history)
 *   2. spec       did the chain of segment entries and exits inside the range hold, where was the range entered and
 *                 left?  all-gather: if every rank's entry is the exit of the rank before it (rank 0: position 0),
 *                 every entry is the true one, the tokens of step 3 are there already and step 2b is not needed
 *   2b. exit_table X[e] = where the parse leaves the range (offset beyond parse_hi) if it enters at
 *                 parse_lo + e (made when asked for: the exact way, for periodic data);  all-gather, then every
 *                 rank knows its entry position
 *   3. emit       tokens of the path positions in [entry, parse_hi) (returns at once with the speculation's tokens
 *                 if entry is where that entered); all-gather the counts;
 *                 rank r sends the first (-first_token_index mod 31744) of its tokens to rank r-1
 *   4. blocks     histogram + Huffman per owned block -> cost records; all-gather
 *   5. mi355_plan_blocks (host, every rank, identical result) -> block types and global bit offsets
 *   6. pack       the rank's blocks at their global bit offsets; byte ranges are OR-stitched on rank 0
 * deflate-rs_amd/shard.py drives this over torch.distributed (one process per GPU); mi355_deflate_encode_multi
 * below drives it inside the library (one process, one thread per GPU). */
typedef struct mi355_shard mi355_shard;
typedef struct {
    uint64_t dyn_bits, dyn_est, static_est, fixed_bits, in_bytes;
    uint32_t q13, reserved;
} mi355_block_cost;
int mi355_shard_begin(mi355_deflate_ctx* ctx, const void* d_ext, size_t n_ext, size_t parse_lo, size_t parse_hi,
                      uint64_t global_lo, uint64_t n_global, const mi355_deflate_opts* opts, void* hip_stream,
                      mi355_shard** out);
/* held != 0: the range was parsed from *entry to *exit_pos (buffer coordinates, *exit_pos >= parse_hi), consistently
 * inside; 0: the caller takes the exact way (exit_table, emit). */
int mi355_shard_spec(mi355_shard* s, int* held, uint64_t* entry, uint64_t* exit_pos);
int mi355_shard_exit_table(mi355_shard* s, uint32_t* table576);
int mi355_shard_emit(mi355_shard* s, uint64_t entry, uint64_t* n_tokens, const void** d_tokens);
int mi355_shard_blocks(mi355_shard* s, uint64_t skip_tokens, const void* d_tail_tokens, uint64_t n_tail,
                       uint64_t* n_blocks, mi355_block_cost* costs, size_t costs_cap);
/* The same with the owner of the stream's last block named by the caller (owns_final != 0: this rank's tokens
 * end in the last, possibly partial or empty, block; 0: it owns whole blocks only, possibly none).
 * mi355_shard_blocks decides that by "is the last rank", which holds whenever every rank's range reaches the
 * next block boundary; a range with fewer tokens than that belongs to a block that began several ranks to its
 * left, and the tail a rank needs is then made of the heads of several ranks to its right. */
int mi355_shard_blocks_ex(mi355_shard* s, uint64_t skip_tokens, const void* d_tail_tokens, uint64_t n_tail,
                          int owns_final, uint64_t* n_blocks, mi355_block_cost* costs, size_t costs_cap);
int mi355_plan_blocks(const mi355_block_cost* costs, size_t n, uint32_t compat, mi355_block_info* plans,
                      uint64_t* total_bits);
/* MI355_E_ARG if a Stored block of the rank ends behind the bytes the rank holds -- or, under MI355_COMPAT_Q13, a Stored block
 * flagged q13 less than 32768 bytes in front of their end: the reference's bytes for it lie that much further on. */
int mi355_shard_pack(mi355_shard* s, const mi355_block_info* plans, uint64_t end_bit, void* d_out, size_t out_cap,
                     uint64_t* first_byte, size_t* n_bytes);
void mi355_shard_end(mi355_shard* s);
/* A sharded zlib / gzip stream (deflate_bytes_zlib_conf, ZlibEncoder: src/lib.rs:182-198, src/checksum.rs:33-57):
 * every rank sums its own byte range (mi355_adler32_device / mi355_crc32_device), rank 0 folds the sums in
 * rank order with this and frames the stitched raw stream.  kind 1 = Adler-32, 2 = CRC-32;
 * returns checksum(A || B) from checksum(A), checksum(B) and |B|. */
uint32_t mi355_checksum_combine(int kind, uint32_t sum_a, uint32_t sum_b, uint64_t len_b);

/* ---- ONE input over the GPUs of a node in ONE call (stream-exact) -----------------------------------------
 * deflate_bytes_conf / deflate_bytes_zlib_conf / deflate_bytes_gzip_conf (src/lib.rs:137-147, 182-198, 242-267) with
 * several devices behind them: one process, one context and one host thread per device.  The input is cut into
 * contiguous ranges of whole 32 KiB windows, one per device (each device also holds 32 KiB of history and 128 KiB of
 * look-ahead: read from the host buffer, no GPU-to-GPU traffic); every device runs the phases of the sharded encode
 * above on its range, what they exchange -- exit tables, token counts and head tokens, block costs: kilobytes --
 * goes through host memory, and the packed byte ranges land at their offsets in `out`, the word two neighbours share
 * OR-ed in.  The bytes are those of ONE encoder over the whole input, i.e. the reference's.
 *   _create    devices[i] = HIP device of rank i (a device may be named more than once: ranks then share it --
 *              how a one-GPU box tests the N-rank path); n_devices <= 64; devices == NULL with n_devices == 0: every
 *              device of the node (mi355_device_count of them, in HIP's order)
 * A handle serves ONE call at a time: the encode calls hold its lock from entry to return, calls from several threads
 * are safe and serialised, and the calling thread's current HIP device is what it was when the call returns.
 * Size: a rank is one pass of the pipeline (32-bit positions, about 20 B of device memory per byte of its range), so an
 * input of more than 2 x MI355_CFG_RANGE_BYTES of rank 0's context per device (default: 1 GiB per device) is cut into
 * MORE ranks than devices -- rank r lives on device r % n_devices, the ranks of a device run one after the other in
 * every phase, each with a context of its own -- up to 64 ranks (64 GiB with the default).  Beyond that the host-buffer
 * call goes through the single-device call of rank 0, which walks any length in ranges; the device-resident call,
 * whose shards the caller lays out, returns MI355_E_UNSUPPORTED (raise MI355_CFG_RANGE_BYTES: a rank is clamped to what one
 * pass addresses, just under 4 GiB -- reached at 2 GiB of MI355_CFG_RANGE_BYTES -- so 64 ranks take about 255 GiB).
 *   _encode_multi         host buffers in and out (ctx-less: the handle owns its contexts); wrapper 0 / 1 / 2 as in
 *              mi355_deflate_opts, `gz_hdr` = GzBuilder::into_header() for wrapper 2 (NULL: the blank header);
 *              out_cap >= mi355_deflate_bound_ex(in_len, wrapper, gz_len, 0); an input of less than 1 MiB per
 *              device uses fewer devices (down to the plain single-device call)
 *   _layout    which bytes rank `rank` holds for an input of in_len bytes: [g_lo, g_hi) of the input, of which
 *              [lo, hi) is its own range; *n_ranks = the ranks that take part (rank >= *n_ranks: nothing) -- fewer than
 *              the devices for a short input, more for a long one (rank r on device r % n_devices)
 *   _encode_multi_device  the same with the input already resident: d_ext[r] = device pointer, on rank r's device
 *              (device r % n_devices), to the bytes [g_lo, g_hi) of _layout (+ 64 readable bytes behind them); d_out = device buffer on
 *              rank 0's device (4-byte aligned).  The packed ranges reach it by peer copies (hipMemcpyPeer: xGMI
 *              between the GPUs of a node) -- the only GPU-to-GPU traffic of the call
 *   _ctx       rank r's context (mi355_deflate_last_info of it: that rank's match-kernel time ...; NULL for a rank no
 *              call has needed yet)
 *   _last_trace  rank 0's wall clock of the last call in ms: [0] bytes + tables, [1] wait, [2] entry + tokens,
 *              [3] wait, [4] block costs, [5] wait, [6] plan + pack + copy-out, [7] wait, [8] seams + framing,
 *              [9] host work of the exchanges (entries, token plan, tails, block plan, seams), [10] the whole call
 *   _stitch_info  how the packed ranges of the last call reached rank 0: *by_rccl = 1 over ncclSend / ncclRecv
 *              (MI355_CFG_MULTI_STITCH = 1, resident output), 0 by copies; *rccl_ranks = the ranks the communicator of rank 0's
 *              device reports (one per distinct device of the handle), 0 when the handle holds none.  A stitch that fails on
 *              one device ends the call with an error inside a bounded wait, aborts the communicators, and later calls of
 *              the handle take the peer copies */
typedef struct mi355_multi mi355_multi;
int mi355_device_count(void); /* HIP devices this process sees (0: none, or no HIP runtime); for callers that do not link HIP */
int mi355_multi_create(const int* devices, int n_devices, mi355_multi** out);
void mi355_multi_destroy(mi355_multi* m);
int mi355_multi_devices(const mi355_multi* m);
mi355_deflate_ctx* mi355_multi_ctx(mi355_multi* m, int rank);
const char* mi355_multi_last_error(mi355_multi* m);
int mi355_multi_layout(const mi355_multi* m, size_t in_len, int rank, int* n_ranks, uint64_t* g_lo, uint64_t* g_hi,
                       uint64_t* lo, uint64_t* hi);
int mi355_deflate_encode_multi(mi355_multi* m, const uint8_t* in, size_t in_len, const mi355_deflate_opts* opts,
                               const uint8_t* gz_hdr, size_t gz_len, uint8_t* out, size_t out_cap, size_t* out_len);
int mi355_deflate_encode_multi_device(mi355_multi* m, const void* const* d_ext, size_t in_len,
                                      const mi355_deflate_opts* opts, const uint8_t* gz_hdr, size_t gz_len, void* d_out,
                                      size_t out_cap, size_t* out_len);
int mi355_multi_last_trace(const mi355_multi* m, double* ms, size_t cap);
int mi355_multi_stitch_info(const mi355_multi* m, int* by_rccl, int* rccl_ranks);

/* The gzip forms (cargo feature "gzip").  `hdr` = the bytes GzBuilder::into_header() returned: the
 * header comes from the crate gzip-header 1.0, which is not part of the reference tree, so the shim
 * builds it with the real crate and passes it through.  Written after the stream: Crc::sum() and
 * Crc::amt_as_u32() little endian (src/lib.rs:258-266), both computed on the GPU.
 *   mi355_deflate_encode_gzip        = deflate_bytes_gzip_conf(input, options, builder)  :242-267
 *   mi355_deflate_encode with wrapper 2 = deflate_bytes_gzip(input) (blank header)        :283-285 */
int mi355_deflate_encode_gzip(mi355_deflate_ctx* ctx, const uint8_t* in, size_t in_len, const mi355_deflate_opts* opts,
                              const uint8_t* hdr, size_t hdr_len, uint8_t* out, size_t out_cap, size_t* out_len);
int mi355_deflate_encode_device_gzip(mi355_deflate_ctx* ctx, const void* d_in, size_t in_len,
                                     const mi355_deflate_opts* opts, const uint8_t* hdr, size_t hdr_len, void* d_out,
                                     size_t out_cap, size_t* out_len, void* hip_stream);
/* CRC-32 (RFC 1952 section 8) of a device buffer: gzip_header::Crc::update + sum as used by
 * src/lib.rs:258-259 and src/writer.rs:436-444, computed on the GPU. */
int mi355_crc32_device(mi355_deflate_ctx* ctx, const void* d_in, size_t in_len, uint32_t* crc, void* hip_stream);

/* Adler-32 of a device buffer (crate adler32's RollingAdler32::update_buffer as used by
 * src/checksum.rs:33-57), computed on the GPU. */
int mi355_adler32_device(mi355_deflate_ctx* ctx, const void* d_in, size_t in_len, uint32_t* adler, void* hip_stream);

/* Streaming encoder mirroring write::{DeflateEncoder, ZlibEncoder, gzip::GzEncoder}<W> (src/writer.rs:89-467):
 *   _new         = ::new(W, options)                    :93-99 / :189-199
 *   _write       = io::Write::write_all                 :124-127 / :254-267
 *   _flush       = io::Write::flush (Flush::Sync)       :134-137 / :274-277
 *   _finish      = finish(self) -> W                    :103-108 / :209-214
 *   _output      = the bytes produced and not yet taken (what the inner writer W is owed)
 *   _take_output = hand over up to `cap` of them: the shim's loop over W::write, which may accept fewer
 *                  bytes than offered (src/compress.rs:96-124, 280-299; tests/test.rs:163-200 issue_47)
 *   _checksum    = {Zlib,Gz}Encoder::checksum()         :248-250 / :428-430
 * write() gathers (the reference likewise does nothing until its 64 KiB + 258 buffer is full,
 * src/lz77.rs:627, and its output does not depend on how the input is split: src/lib.rs:408-433); the GPU
 * encodes at flush() and finish(), and the bytes of a flush -- ending in 00 00 FF FF, as
 * src/writer.rs:570-595 asserts -- are available when flush() returns.  Between flushes the handle keeps
 * the bytes since the last flush plus the 32 KiB window before it (the whole stream while the flushed part
 * is shorter than three windows).  What gathers is bounded all the same (the reference's O(window) streaming,
 * src/compress.rs:96-124): whenever 512 MiB and a margin of 16 MiB have gathered -- since the start of a stream that
 * has not been flushed yet, or since the last flush point -- write() encodes that range and makes its bytes available
 * (_output / _take_output), keeping the rest, one window of history and the bytes not yet taken: a stream of any
 * length, e.g. 8 GiB into a ZlibEncoder with or without a flush() in the middle, holds about 0.55 GiB of host memory.
 * The first range behind a flush point begins AT it, with the hash side effects of the write calls around the flush;
 * the next flush() / finish() ends the last range (with the sync marker / the final block).  Behind a flush() within the
 * first 96 KiB of a stream -- where a stream's start has hash rules of its own, src/lz77.rs:601-638 -- the first range
 * holds the stream from its start and takes over what the flush calls found: the flush points that re-warm the hash and
 * the re-warm behind a block that fills inside the first window (Q1).  One _write call stands for one write_all call (n == 0: no call at all);
 * the size of the first write after a flush is remembered, because the reference's hash re-warm at a
 * flush point inside the first window depends on it (src/lz77.rs:601-638).  The shim's Drop calls _finish
 * and drains the output like the reference's (src/writer.rs:139-152). */
typedef struct mi355_deflate_stream mi355_deflate_stream;
int mi355_deflate_stream_new(mi355_deflate_ctx* ctx, const mi355_deflate_opts* opts, mi355_deflate_stream** out);
int mi355_deflate_stream_write(mi355_deflate_stream* s, const uint8_t* data, size_t n);
/* io::Write::flush (Flush::Sync, src/writer.rs:134-137, 274-277; src/compress.rs:256-261; src/lz77.rs:
 * 605-614, 728-740): what was written so far is emitted in non-final blocks + 00 00 FF FF, the window
 * is kept.  The hash-table side effects the reference has for writes of one or two bytes around a flush
 * (positions filed late, under a stale rolling hash, or not at all; the re-warm of the first window) are
 * reproduced for every pattern; no write / flush sequence is refused. */
int mi355_deflate_stream_flush(mi355_deflate_stream* s);
int mi355_deflate_stream_finish(mi355_deflate_stream* s);
/* GzEncoder::from_builder (src/writer.rs:346-358): header bytes of a wrapper-2 stream, before the first
 * write; _checksum of such a stream is GzEncoder::checksum() (:428-430), the CRC-32. */
int mi355_deflate_stream_gzip_header(mi355_deflate_stream* s, const uint8_t* hdr, size_t hdr_len);
/* reset(&mut self, W) -> io::Result<W> (src/writer.rs:110-117, 216-223, 383-402): finishes the stream,
 * hands its untaken bytes out (valid until the next reset / free) and starts a new one with the same options
 * (gzip: with the blank header again, as GzEncoder::reset does). */
int mi355_deflate_stream_reset(mi355_deflate_stream* s, const uint8_t** data, size_t* n);
int mi355_deflate_stream_output(mi355_deflate_stream* s, const uint8_t** data, size_t* n);
int mi355_deflate_stream_take_output(mi355_deflate_stream* s, uint8_t* dst, size_t cap, size_t* n);
int mi355_deflate_stream_checksum(mi355_deflate_stream* s, uint32_t* adler);
/* Host memory the handle holds right now: gathered input, the window, bytes produced and not yet taken (what the
 * reference bounds at about 330 KiB, src/deflate_state.rs:82-119; here one range for a stream that is never flushed). */
uint64_t mi355_deflate_stream_held_bytes(mi355_deflate_stream* s);
void mi355_deflate_stream_free(mi355_deflate_stream* s);

#ifdef MI355_DEBUG_HOOKS
/* Test build only (libmi355deflate_dbg.so, `make debug`; never part of the product library): make the hash sort of this
 * context hand out a wrong order, as a device would whose LDS did not serve same-address lanes in lane order, so that
 * a test can watch the match kernel's order check catch it.  _sort_ranks reports what the context sorts with now. */
int mi355_debug_break_sort(mi355_deflate_ctx* ctx, int on);
int mi355_debug_sort_ranks(mi355_deflate_ctx* ctx);
/* The sort's tables as the context's last single-pass call left them in its workspace, copied to host memory after a wait for
 * the context's stream: for `ne` epochs from `e0` on, 32 768 entries of S (positions by (hash, position), stored x 2; those
 * from the epoch's J on are unspecified) and 32 776 entries of B (bucket starts, [32768] = J, [32769] = run flag, [32770] =
 * the mark for the permuted pair table).  MI355_E_ARG if the workspace holds fewer epochs. */
int mi355_debug_sort_tables(mi355_deflate_ctx* ctx, uint32_t e0, uint32_t ne, uint16_t* S_out, uint16_t* B_out);
/* mode 0: the product's behaviour.  1: every epoch with J >= 1024 carries the mark, whatever its samples say (only states that
 * input data could produce).  2: no epoch carries it. */
int mi355_debug_force_swz(mi355_deflate_ctx* ctx, int mode);
#endif

#ifdef __cplusplus
}
#endif
#endif
