"""Python host side of the MI355X DEFLATE encode path: a ctypes binding of libmi355deflate.so
(include/mi355_deflate.h) shaped like the reference's public API so that tests read like the
reference's own (src/lib.rs:137-216, src/writer.rs:89-290, src/compression_options.rs).

There is no CPU fallback here.  Importing works anywhere (so the symbol check can run on a
machine without a GPU); every encode call goes through the HIP kernels and raises if the library
or a gfx950 device is missing.
"""
import ctypes as C
import enum
import os
import struct

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MI355_DEFLATE_LIB", os.path.join(_HERE, "libmi355deflate.so"))

FLUSH_FINISH, FLUSH_SYNC = 0, 1
OK, E_ARG, E_OUT_TOO_SMALL, E_HIP, E_UNSUPPORTED, E_REF_PANIC, E_STATE = 0, -1, -2, -3, -4, -5, -6
E_VERIFY = -7
E_DATA = -8
COMPAT_Q13 = 1

STAGES = ["links", "match", "parse", "blocks", "pack", "other"]


class Opts(C.Structure):
    _fields_ = [("max_hash_checks", C.c_uint16), ("lazy_if_less_than", C.c_uint16),
                ("matching_type", C.c_uint8), ("wrapper", C.c_uint8), ("compat", C.c_uint8),
                ("flush", C.c_uint8)]


class Info(C.Structure):
    _fields_ = [("in_len", C.c_uint64), ("out_len", C.c_uint64), ("n_tokens", C.c_uint64),
                ("n_blocks", C.c_uint32), ("n_stored", C.c_uint32), ("n_fixed", C.c_uint32),
                ("n_dynamic", C.c_uint32), ("q1_rewarm", C.c_uint32), ("q13_hits", C.c_uint32),
                ("passes", C.c_uint32), ("spec_fallback", C.c_uint32), ("stage_ms", C.c_float * 6),
                ("total_ms", C.c_float), ("match_launches", C.c_uint32), ("match_ms", C.c_float),
                ("spec_repaired", C.c_uint32), ("host_path", C.c_uint32)]


class BlockInfo(C.Structure):
    _fields_ = [("btype", C.c_uint32), ("bfinal", C.c_uint32), ("n_tokens", C.c_uint32), ("reserved", C.c_uint32),
                ("in_bytes", C.c_uint64), ("bit_start", C.c_uint64)]


class BlockCost(C.Structure):
    _fields_ = [("dyn_bits", C.c_uint64), ("dyn_est", C.c_uint64), ("static_est", C.c_uint64),
                ("fixed_bits", C.c_uint64), ("in_bytes", C.c_uint64), ("q13", C.c_uint32), ("reserved", C.c_uint32)]


class MatchingType(enum.IntEnum):
    """src/lz77.rs:27-37"""
    Greedy = 0
    Lazy = 1


class Compression(enum.IntEnum):
    """src/compression_options.rs:31-42"""
    Fast = 0
    Default = 1
    Best = 2


class CompressionOptions:
    """src/compression_options.rs:78-120; profiles :126-178."""

    def __init__(self, max_hash_checks=128, lazy_if_less_than=32, matching_type=MatchingType.Lazy):
        self.max_hash_checks = max_hash_checks
        self.lazy_if_less_than = lazy_if_less_than
        self.matching_type = MatchingType(matching_type)

    @staticmethod
    def default():
        return CompressionOptions(128, 32, MatchingType.Lazy)

    @staticmethod
    def high():
        return CompressionOptions(1768, 128, MatchingType.Lazy)

    @staticmethod
    def fast():
        return CompressionOptions(1, 0, MatchingType.Greedy)

    @staticmethod
    def huffman_only():
        return CompressionOptions(0, 0, MatchingType.Greedy)

    @staticmethod
    def rle():
        return CompressionOptions(0, 0, MatchingType.Lazy)

    @staticmethod
    def from_(o):
        """impl From<Compression> for CompressionOptions (:188-196)"""
        if isinstance(o, CompressionOptions):
            return o
        o = Compression(o)
        return {Compression.Fast: CompressionOptions.fast, Compression.Default: CompressionOptions.default,
                Compression.Best: CompressionOptions.high}[o]()

    def to_c(self, wrapper=0, compat=0, flush=0):
        return Opts(self.max_hash_checks, self.lazy_if_less_than, int(self.matching_type), wrapper, compat, flush)


class BatchItem(C.Structure):
    """mi355_batch_item"""
    _fields_ = [("in_", C.c_void_p), ("in_len", C.c_size_t), ("out", C.c_void_p), ("out_cap", C.c_size_t),
                ("out_len", C.c_size_t), ("status", C.c_int)]


class GzipHeader(C.Structure):
    """mi355_gzip_header"""
    _fields_ = [("hdr", C.c_char_p), ("hdr_len", C.c_size_t)]


class PackedEntry(C.Structure):
    """mi355_packed_entry: an item's place in the arena of a packed batch"""
    _fields_ = [("off", C.c_uint64), ("len", C.c_uint64), ("status", C.c_int32), ("reserved", C.c_uint32)]


class PackedResult:
    """What a packed batch call left: the arena, entries[i] = (off, len) of item i (off None for an item that is not OK; len is
    exact either way), the items' statuses, the call's arena_used and its return code."""

    def __init__(self, arena, entries, statuses, used, rc):
        self.arena, self.entries, self.statuses, self.used, self.rc = arena, entries, statuses, used, rc


class BatchInfo(C.Structure):
    """mi355_batch_info"""
    _fields_ = [("n_items", C.c_uint64), ("in_len", C.c_uint64), ("out_len", C.c_uint64), ("n_batched", C.c_uint32),
                ("n_single", C.c_uint32), ("n_q1_single", C.c_uint32), ("n_spec_single", C.c_uint32),
                ("sub_batches", C.c_uint32), ("total_ms", C.c_float)]


VERIFY_STATUS = ["OK", "FRAME", "BTYPE", "STORED", "LENGTHS", "CODE", "DISTANCE", "MISMATCH", "LENGTH", "TABLE", "TRUNCATED",
                 "TRAILER", "CHECKSUM"]  # MI355_VERIFY_*


class VerifyReport(C.Structure):
    """mi355_verify_report (48 bytes)"""
    _fields_ = [("status", C.c_uint32), ("entry", C.c_uint32), ("bit", C.c_uint64), ("in_pos", C.c_uint64),
                ("n_blocks", C.c_uint64), ("n_stored", C.c_uint32), ("n_fixed", C.c_uint32), ("n_dynamic", C.c_uint32),
                ("ms", C.c_float)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in VerifyReport._fields_}
        d["status"] = VERIFY_STATUS[self.status] if self.status < len(VERIFY_STATUS) else self.status
        return d


class InflateReport(C.Structure):
    """mi355_inflate_report (56 bytes)"""
    _fields_ = [("status", C.c_uint32), ("reserved", C.c_uint32), ("bit", C.c_uint64), ("out_pos", C.c_uint64),
                ("out_len", C.c_uint64), ("n_blocks", C.c_uint64), ("n_stored", C.c_uint32), ("n_fixed", C.c_uint32),
                ("n_dynamic", C.c_uint32), ("ms", C.c_float)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in InflateReport._fields_ if k != "reserved"}
        d["status"] = VERIFY_STATUS[self.status] if self.status < len(VERIFY_STATUS) else self.status
        return d


class IndexWalk(C.Structure):
    """mi355_index_walk (80 bytes): what the walker of one span of mi355_inflate_index left"""
    _fields_ = [("start", C.c_uint64), ("end_bit", C.c_uint64), ("count", C.c_uint64), ("how", C.c_uint32), ("link", C.c_uint32),
                ("btype", C.c_uint32), ("status", C.c_uint32), ("n_stored", C.c_uint32), ("n_fixed", C.c_uint32),
                ("n_dynamic", C.c_uint32), ("reserved", C.c_uint32), ("n_blocks", C.c_uint64), ("bit", C.c_uint64),
                ("in_pos", C.c_uint64)]


MEMBER_HINTED = 1  # MI355_MEMBER_HINTED


class MemberInfo(C.Structure):
    """mi355_member_info (40 bytes): one member of a gzip file, as mi355_inflate_members walked it"""
    _fields_ = [("in_off", C.c_uint64), ("in_len", C.c_uint64), ("out_off", C.c_uint64), ("out_len", C.c_uint64),
                ("flags", C.c_uint32), ("status", C.c_uint32)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in MemberInfo._fields_}
        d["status"] = VERIFY_STATUS[self.status] if self.status < len(VERIFY_STATUS) else self.status
        return d


class MemberWalk(C.Structure):
    """mi355_member_walk (40 bytes): what the walker of one span of mi355_inflate_members left on its first walk"""
    _fields_ = [("start", C.c_uint64), ("end", C.c_uint64), ("n_members", C.c_uint64), ("out_bytes", C.c_uint64),
                ("how", C.c_uint32), ("link", C.c_uint32)]


class SeekInfo(C.Structure):
    """mi355_seek_info (56 bytes)"""
    _fields_ = [("total", C.c_uint64), ("n_entries", C.c_uint64), ("n_points", C.c_uint64), ("spacing", C.c_uint64),
                ("device_bytes", C.c_uint64), ("stream_len", C.c_uint64), ("wrapper", C.c_uint32), ("reserved", C.c_uint32)]


class SeekPoint(C.Structure):
    """mi355_seek_point (16 bytes): a point's raw-deflate bit offset and output position"""
    _fields_ = [("bit", C.c_uint64), ("pos", C.c_uint64)]


class SeekCut(C.Structure):
    """mi355_seek_cut (24 bytes): where decoding resumes, the output position there, the header bit of the block it lies in"""
    _fields_ = [("bit", C.c_uint64), ("pos", C.c_uint64), ("hdr_bit", C.c_uint64)]


class SeekRange(C.Structure):
    """mi355_seek_range (40 bytes): one range of mi355_inflate_seek_read_batch_device"""
    _fields_ = [("off", C.c_uint64), ("len", C.c_uint64), ("out", C.c_void_p), ("got", C.c_uint64), ("status", C.c_int32),
                ("reserved", C.c_uint32)]


class BgzfInfo(C.Structure):
    """mi355_bgzf_info (40 bytes)"""
    _fields_ = [("total", C.c_uint64), ("n_members", C.c_uint64), ("file_len", C.c_uint64), ("host_bytes", C.c_uint64),
                ("max_out_len", C.c_uint64)]


class InflateStreamState(C.Structure):
    """mi355_inflate_stream_state (48 bytes)"""
    _fields_ = [("total_in", C.c_uint64), ("total_out", C.c_uint64), ("pending_in", C.c_uint64), ("need_out", C.c_uint64),
                ("done", C.c_uint32), ("failed", C.c_uint32), ("adler_or_crc", C.c_uint32), ("reserved", C.c_uint32)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in InflateStreamState._fields_ if k != "reserved"}
        d["failed"] = VERIFY_STATUS[self.failed] if self.failed < len(VERIFY_STATUS) else self.failed
        return d


class DeflateError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("mi355_deflate error %d: %s" % (code, msg))
        self.code = code


_lib = None


def load():
    """Load libmi355deflate.so.  Raises (loudly) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libmi355deflate.so is missing (%s); run __graft_entry__.build() or "
                          "`make -C deflate-rs_amd` -- there is no CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    u8p = C.POINTER(C.c_uint8)
    L.mi355_deflate_version.restype = C.c_int
    L.mi355_deflate_bound.argtypes = [C.c_size_t]
    L.mi355_deflate_bound.restype = C.c_size_t
    L.mi355_deflate_preset.argtypes = [C.c_int, C.POINTER(Opts)]
    L.mi355_deflate_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.mi355_deflate_ctx_destroy.argtypes = [C.c_void_p]
    L.mi355_deflate_ctx_destroy.restype = None
    L.mi355_deflate_last_error.argtypes = [C.c_void_p]
    L.mi355_deflate_last_error.restype = C.c_char_p
    L.mi355_deflate_encode.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(Opts), u8p, C.c_size_t,
                                       C.POINTER(C.c_size_t)]
    L.mi355_deflate_encode_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(Opts), C.c_void_p,
                                              C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]
    L.mi355_deflate_last_info.argtypes = [C.c_void_p, C.POINTER(Info)]
    L.mi355_deflate_last_blocks.argtypes = [C.c_void_p, C.POINTER(BlockInfo), C.c_size_t, C.POINTER(C.c_size_t)]
    L.mi355_shard_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint64,
                                    C.c_uint64, C.POINTER(Opts), C.c_void_p, C.POINTER(C.c_void_p)]
    L.mi355_shard_exit_table.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    L.mi355_shard_spec.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.mi355_shard_emit.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_void_p)]
    L.mi355_shard_blocks.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                     C.POINTER(BlockCost), C.c_size_t]
    L.mi355_shard_blocks_ex.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_uint64),
                                        C.POINTER(BlockCost), C.c_size_t]
    L.mi355_plan_blocks.argtypes = [C.POINTER(BlockCost), C.c_size_t, C.c_uint32, C.POINTER(BlockInfo),
                                    C.POINTER(C.c_uint64)]
    L.mi355_shard_pack.argtypes = [C.c_void_p, C.POINTER(BlockInfo), C.c_uint64, C.c_void_p, C.c_size_t,
                                   C.POINTER(C.c_uint64), C.POINTER(C.c_size_t)]
    L.mi355_shard_end.argtypes = [C.c_void_p]
    L.mi355_shard_end.restype = None
    L.mi355_adler32_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.c_void_p]
    L.mi355_deflate_ctx_reserve.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
    L.mi355_crc32_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.c_void_p]
    L.mi355_deflate_encode_gzip.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(Opts), C.c_char_p, C.c_size_t,
                                            u8p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.mi355_deflate_encode_device_gzip.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(Opts), C.c_char_p,
                                                   C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                                   C.c_void_p]
    L.mi355_deflate_stream_gzip_header.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.mi355_deflate_stream_reset.argtypes = [C.c_void_p, C.POINTER(u8p), C.POINTER(C.c_size_t)]
    L.mi355_deflate_stream_new.argtypes = [C.c_void_p, C.POINTER(Opts), C.POINTER(C.c_void_p)]
    L.mi355_deflate_stream_write.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.mi355_deflate_stream_flush.argtypes = [C.c_void_p]
    L.mi355_deflate_stream_finish.argtypes = [C.c_void_p]
    L.mi355_deflate_stream_output.argtypes = [C.c_void_p, C.POINTER(u8p), C.POINTER(C.c_size_t)]
    L.mi355_deflate_stream_take_output.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.mi355_deflate_bound_ex.argtypes = [C.c_size_t, C.c_int, C.c_size_t, C.c_size_t]
    L.mi355_deflate_bound_ex.restype = C.c_size_t
    L.mi355_checksum_combine.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint64]
    L.mi355_checksum_combine.restype = C.c_uint32
    L.mi355_deflate_stream_checksum.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    L.mi355_deflate_stream_free.argtypes = [C.c_void_p]
    L.mi355_device_count.restype = C.c_int
    L.mi355_multi_create.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]
    L.mi355_multi_destroy.argtypes = [C.c_void_p]
    L.mi355_multi_destroy.restype = None
    L.mi355_multi_devices.argtypes = [C.c_void_p]
    L.mi355_multi_ctx.argtypes = [C.c_void_p, C.c_int]
    L.mi355_multi_ctx.restype = C.c_void_p
    L.mi355_multi_last_error.argtypes = [C.c_void_p]
    L.mi355_multi_last_error.restype = C.c_char_p
    L.mi355_multi_layout.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_int)] + [C.POINTER(C.c_uint64)] * 4
    L.mi355_deflate_encode_multi.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(Opts), C.c_char_p, C.c_size_t, u8p,
                                             C.c_size_t, C.POINTER(C.c_size_t)]
    L.mi355_deflate_encode_multi_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(Opts), C.c_char_p,
                                                    C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.mi355_multi_last_trace.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_size_t]
    L.mi355_multi_stitch_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.mi355_deflate_ctx_config.argtypes = [C.c_void_p, C.c_int, C.c_uint64]
    L.mi355_deflate_stream_held_bytes.argtypes = [C.c_void_p]
    L.mi355_deflate_stream_held_bytes.restype = C.c_uint64
    L.mi355_deflate_stream_free.restype = None
    L.mi355_deflate_encode_batch.argtypes = [C.c_void_p, C.POINTER(BatchItem), C.c_size_t, C.POINTER(Opts)]
    L.mi355_deflate_encode_batch_device.argtypes = [C.c_void_p, C.POINTER(BatchItem), C.c_size_t, C.POINTER(Opts), C.c_void_p]
    L.mi355_deflate_last_batch_info.argtypes = [C.c_void_p, C.POINTER(BatchInfo)]
    L.mi355_deflate_encode_batch_gzip.argtypes = [C.c_void_p, C.POINTER(BatchItem), C.c_size_t, C.POINTER(Opts),
                                                  C.POINTER(GzipHeader), C.c_size_t]
    L.mi355_deflate_encode_batch_device_gzip.argtypes = [C.c_void_p, C.POINTER(BatchItem), C.c_size_t, C.POINTER(Opts),
                                                         C.POINTER(GzipHeader), C.c_size_t, C.c_void_p]
    L.mi355_deflate_batch_packed_bound.argtypes = [C.POINTER(BatchItem), C.c_size_t, C.c_int, C.POINTER(GzipHeader), C.c_size_t,
                                                   C.c_size_t]
    L.mi355_deflate_batch_packed_bound.restype = C.c_size_t
    L.mi355_deflate_encode_batch_packed.argtypes = [C.c_void_p, C.POINTER(BatchItem), C.c_size_t, C.POINTER(Opts),
                                                    C.POINTER(GzipHeader), C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                                                    C.POINTER(C.c_size_t)]
    L.mi355_deflate_encode_batch_packed_device.argtypes = [C.c_void_p, C.POINTER(BatchItem), C.c_size_t, C.POINTER(Opts),
                                                           C.POINTER(GzipHeader), C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                                                           C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p]
    L.mi355_deflate_verify_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int,
                                              C.POINTER(BlockInfo), C.c_size_t, C.POINTER(VerifyReport), C.c_void_p]
    L.mi355_deflate_verify.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_int, C.POINTER(BlockInfo),
                                       C.c_size_t, C.POINTER(VerifyReport)]
    L.mi355_deflate_verify_batch_device.argtypes = [C.c_void_p, C.POINTER(BatchItem), C.c_size_t, C.c_int, C.POINTER(VerifyReport),
                                                    C.c_void_p]
    L.mi355_inflate_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                       C.POINTER(InflateReport), C.c_void_p]
    L.mi355_inflate.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                C.POINTER(InflateReport)]
    L.mi355_inflate_batch_device.argtypes = [C.c_void_p, C.POINTER(BatchItem), C.c_size_t, C.c_int, C.POINTER(InflateReport),
                                             C.c_void_p]
    L.mi355_inflate_tabled_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(BlockInfo), C.c_size_t, C.c_void_p,
                                              C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(InflateReport), C.c_void_p]
    L.mi355_inflate_tabled.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_int, C.POINTER(BlockInfo), C.c_size_t, C.c_void_p,
                                       C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(InflateReport)]
    L.mi355_inflate_tabled_last_stages.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.mi355_inflate_index_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(BlockInfo), C.c_size_t,
                                             C.POINTER(C.c_size_t), C.POINTER(InflateReport), C.c_void_p]
    L.mi355_inflate_index.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_int, C.POINTER(BlockInfo), C.c_size_t,
                                      C.POINTER(C.c_size_t), C.POINTER(InflateReport)]
    L.mi355_inflate_parallel_device.argtypes = L.mi355_inflate_device.argtypes
    L.mi355_inflate_parallel.argtypes = L.mi355_inflate.argtypes
    L.mi355_inflate_index_last_stages.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.mi355_inflate_index_last_walks.argtypes = [C.c_void_p, C.POINTER(IndexWalk), C.c_size_t, C.POINTER(C.c_size_t)]
    L.mi355_inflate_members_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                               C.POINTER(MemberInfo), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(InflateReport), C.c_void_p]
    L.mi355_inflate_members.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                        C.POINTER(MemberInfo), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(InflateReport)]
    L.mi355_inflate_members_last_stages.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.mi355_inflate_members_last_parallel.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.mi355_inflate_members_last_parallel_stages.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.mi355_inflate_members_last_walks.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(MemberWalk), C.c_size_t, C.POINTER(C.c_size_t)]
    L.mi355_inflate_seek_build_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(BlockInfo), C.c_size_t, C.c_uint64,
                                                  C.POINTER(C.c_void_p), C.POINTER(InflateReport), C.c_void_p]
    L.mi355_inflate_seek_build.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_int, C.POINTER(BlockInfo), C.c_size_t, C.c_uint64,
                                           C.POINTER(C.c_void_p), C.POINTER(InflateReport)]
    L.mi355_inflate_seek_free.argtypes = [C.c_void_p]
    L.mi355_inflate_seek_free.restype = None
    L.mi355_inflate_seek_info.argtypes = [C.c_void_p, C.POINTER(SeekInfo)]
    L.mi355_inflate_seek_points.argtypes = [C.c_void_p, C.POINTER(SeekPoint), C.c_size_t, C.POINTER(C.c_size_t)]
    L.mi355_inflate_seek_read_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64),
                                                 C.POINTER(InflateReport), C.c_void_p]
    L.mi355_inflate_seek_read.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(InflateReport)]
    L.mi355_inflate_seek_read_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(SeekRange), C.c_size_t, C.POINTER(InflateReport),
                                                       C.c_void_p]
    L.mi355_inflate_seek_last_read.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.mi355_inflate_seek_cuts.argtypes = [C.c_void_p, C.POINTER(SeekCut), C.c_size_t, C.POINTER(C.c_size_t)]
    L.mi355_inflate_seek_cut_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.mi355_inflate_seek_last_read_cuts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.mi355_inflate_seek_last_read_stages.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.mi355_deflate_ctx_config_get.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]
    L.mi355_bgzf_bound.argtypes = [C.c_size_t, C.c_size_t]
    L.mi355_bgzf_bound.restype = C.c_size_t
    L.mi355_bgzf_encode_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(Opts), C.c_size_t, C.c_void_p, C.c_size_t,
                                           C.POINTER(C.c_size_t), C.POINTER(MemberInfo), C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]
    L.mi355_bgzf_encode.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(Opts), C.c_size_t, C.c_void_p, C.c_size_t,
                                    C.POINTER(C.c_size_t), C.POINTER(MemberInfo), C.c_size_t, C.POINTER(C.c_size_t)]
    L.mi355_bgzf_last_stages.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.mi355_bgzf_index_build_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(InflateReport), C.c_void_p]
    L.mi355_bgzf_index_build.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(InflateReport)]
    L.mi355_bgzf_index_from_members.argtypes = [C.POINTER(MemberInfo), C.c_size_t, C.c_size_t, C.POINTER(C.c_void_p)]
    L.mi355_bgzf_index_free.argtypes = [C.c_void_p]
    L.mi355_bgzf_index_free.restype = None
    L.mi355_bgzf_index_info.argtypes = [C.c_void_p, C.POINTER(BgzfInfo)]
    L.mi355_bgzf_index_members.argtypes = [C.c_void_p, C.POINTER(MemberInfo), C.c_size_t, C.POINTER(C.c_size_t)]
    L.mi355_bgzf_voffset.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.mi355_bgzf_uoffset.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.mi355_bgzf_read_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64),
                                         C.POINTER(InflateReport), C.c_void_p]
    L.mi355_bgzf_read.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint64, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64),
                                  C.POINTER(InflateReport)]
    L.mi355_bgzf_read_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SeekRange), C.c_size_t, C.POINTER(InflateReport),
                                               C.c_void_p]
    L.mi355_bgzf_last_read.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.mi355_bgzf_last_read_stages.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.mi355_inflate_stream_new.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p)]
    L.mi355_inflate_stream_write.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                             C.POINTER(InflateReport)]
    L.mi355_inflate_stream_write_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                                    C.POINTER(InflateReport), C.c_void_p]
    L.mi355_inflate_stream_write_batch_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(BatchItem), C.c_size_t,
                                                          C.POINTER(InflateReport), C.c_void_p]
    L.mi355_inflate_stream_finish.argtypes = [C.c_void_p, C.POINTER(InflateReport)]
    L.mi355_inflate_stream_state_get.argtypes = [C.c_void_p, C.POINTER(InflateStreamState)]
    L.mi355_inflate_stream_reset.argtypes = [C.c_void_p]
    L.mi355_inflate_stream_free.argtypes = [C.c_void_p]
    L.mi355_inflate_stream_free.restype = None
    _lib = L
    return L


EXPORTED = [
    "mi355_deflate_version", "mi355_deflate_bound", "mi355_deflate_bound_ex", "mi355_deflate_preset", "mi355_deflate_ctx_create",
    "mi355_deflate_ctx_destroy", "mi355_deflate_last_error", "mi355_deflate_encode",
    "mi355_deflate_encode_device", "mi355_deflate_last_info", "mi355_deflate_last_blocks", "mi355_adler32_device",
    "mi355_deflate_stream_new", "mi355_deflate_stream_write", "mi355_deflate_stream_flush",
    "mi355_deflate_stream_finish",
    "mi355_deflate_stream_output", "mi355_deflate_stream_take_output", "mi355_deflate_stream_checksum",
    "mi355_deflate_stream_free",
    "mi355_deflate_ctx_reserve", "mi355_deflate_stream_gzip_header", "mi355_deflate_stream_reset",
    "mi355_deflate_encode_gzip",
    "mi355_deflate_encode_device_gzip", "mi355_crc32_device",
    "mi355_shard_begin", "mi355_shard_spec", "mi355_shard_exit_table", "mi355_shard_emit", "mi355_shard_blocks", "mi355_shard_blocks_ex",
    "mi355_plan_blocks",
    "mi355_shard_pack", "mi355_shard_end", "mi355_checksum_combine",
    "mi355_deflate_ctx_config", "mi355_deflate_stream_held_bytes",
    "mi355_device_count", "mi355_multi_create", "mi355_multi_destroy", "mi355_multi_devices", "mi355_multi_ctx", "mi355_multi_last_error",
    "mi355_multi_layout", "mi355_deflate_encode_multi", "mi355_deflate_encode_multi_device", "mi355_multi_last_trace",
    "mi355_multi_stitch_info",
    "mi355_deflate_encode_batch", "mi355_deflate_encode_batch_device", "mi355_deflate_last_batch_info",
    "mi355_deflate_encode_batch_gzip", "mi355_deflate_encode_batch_device_gzip",
    "mi355_deflate_batch_packed_bound", "mi355_deflate_encode_batch_packed", "mi355_deflate_encode_batch_packed_device",
    "mi355_deflate_verify", "mi355_deflate_verify_device", "mi355_deflate_verify_batch_device",
    "mi355_inflate", "mi355_inflate_device", "mi355_inflate_batch_device",
    "mi355_inflate_tabled", "mi355_inflate_tabled_device", "mi355_inflate_tabled_last_stages",
    "mi355_inflate_index", "mi355_inflate_index_device", "mi355_inflate_parallel", "mi355_inflate_parallel_device",
    "mi355_inflate_index_last_stages", "mi355_inflate_index_last_walks",
    "mi355_inflate_members", "mi355_inflate_members_device", "mi355_inflate_members_last_stages",
    "mi355_inflate_members_last_walks", "mi355_inflate_members_last_parallel", "mi355_inflate_members_last_parallel_stages",
    "mi355_inflate_seek_build", "mi355_inflate_seek_build_device", "mi355_inflate_seek_free", "mi355_inflate_seek_info",
    "mi355_inflate_seek_points", "mi355_inflate_seek_read", "mi355_inflate_seek_read_device", "mi355_inflate_seek_read_batch_device",
    "mi355_inflate_seek_last_read", "mi355_inflate_seek_cuts", "mi355_inflate_seek_cut_info", "mi355_inflate_seek_last_read_cuts",
    "mi355_inflate_seek_last_read_stages", "mi355_deflate_ctx_config_get",
    "mi355_bgzf_bound", "mi355_bgzf_encode", "mi355_bgzf_encode_device", "mi355_bgzf_last_stages",
    "mi355_bgzf_index_build", "mi355_bgzf_index_build_device", "mi355_bgzf_index_from_members", "mi355_bgzf_index_free",
    "mi355_bgzf_index_info", "mi355_bgzf_index_members", "mi355_bgzf_voffset", "mi355_bgzf_uoffset",
    "mi355_bgzf_read", "mi355_bgzf_read_device", "mi355_bgzf_read_batch_device", "mi355_bgzf_last_read", "mi355_bgzf_last_read_stages",
    "mi355_inflate_stream_new", "mi355_inflate_stream_write", "mi355_inflate_stream_write_device",
    "mi355_inflate_stream_write_batch_device", "mi355_inflate_stream_finish", "mi355_inflate_stream_state_get",
    "mi355_inflate_stream_reset", "mi355_inflate_stream_free",
]


class InflateStream:
    """A streaming inflate handle (mi355_inflate_stream): zlib's decompressobj on the device.  Made by Context.inflate_stream.  The
    granularity is the deflate block: write() returns the bytes of every block that has become complete."""

    def __init__(self, ctx, handle):
        self._ctx, self._h = ctx, handle

    def close(self):
        if getattr(self, "_h", None):
            load().mi355_inflate_stream_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def write_raw(self, chunk, room):
        """mi355_inflate_stream_write on host bytes: (rc, the bytes handed over, report dict); rc is OK, E_DATA, E_OUT_TOO_SMALL or
        E_STATE, anything else raises.  room 0 hands the decoder a NULL buffer (the query form)."""
        chunk = bytes(chunk)
        buf = C.create_string_buffer(room) if room else None
        n = C.c_size_t(0)
        r = InflateReport()
        rc = load().mi355_inflate_stream_write(self._h, chunk if chunk else None, len(chunk), C.cast(buf, C.c_void_p) if room else None, room,
                                               C.byref(n), C.byref(r))
        if rc not in (OK, E_DATA, E_OUT_TOO_SMALL, E_STATE):
            self._ctx._err(rc)
        return rc, (buf.raw[: n.value] if room else b""), r.as_dict()

    def write(self, chunk, room=None):
        """The stream's next bytes after `chunk` (possibly none: more input is needed).  room None: the buffer starts at eight times
        the chunk and the write is repeated with state()["need_out"] for as long as a complete block waits for room; a given room
        is used as it is, and DeflateError(E_OUT_TOO_SMALL, ...) says that the next block does not fit.  Raises DeflateError(E_DATA,
        ...) for a stream that is not valid -- the bytes in front of the failure are the exception's `partial` -- and
        DeflateError(E_STATE, ...) for a dead handle."""
        out, cap = [], (max(8 * len(chunk), 4096) if room is None else room)
        while True:
            rc, data, _rep = self.write_raw(chunk, cap)
            chunk = b""
            out.append(data)
            need = self.state()["need_out"]
            if rc in (OK, E_OUT_TOO_SMALL) and room is None and need:
                cap = need
                continue
            if rc != OK:
                try:
                    self._ctx._err(rc)
                except DeflateError as e:
                    e.partial = b"".join(out)
                    raise
            return b"".join(out)

    def write_device(self, d_in_ptr, in_len, d_out_ptr, out_cap, stream=0):
        """mi355_inflate_stream_write_device: device pointers.  Returns (rc, out_len, report dict); rc as in write_raw."""
        n = C.c_size_t(0)
        r = InflateReport()
        rc = load().mi355_inflate_stream_write_device(self._h, C.c_void_p(d_in_ptr), in_len, C.c_void_p(d_out_ptr), out_cap, C.byref(n),
                                                      C.byref(r), C.c_void_p(stream))
        if rc not in (OK, E_DATA, E_OUT_TOO_SMALL, E_STATE):
            self._ctx._err(rc)
        return rc, n.value, r.as_dict()

    def finish_raw(self):
        """mi355_inflate_stream_finish: (rc, report dict); OK, E_DATA (FRAME / TRUNCATED) or E_STATE"""
        r = InflateReport()
        rc = load().mi355_inflate_stream_finish(self._h, C.byref(r))
        if rc not in (OK, E_DATA, E_STATE):
            self._ctx._err(rc)
        return rc, r.as_dict()

    def finish(self):
        """No more input will come: raises DeflateError(E_DATA, ...) unless the stream is done"""
        rc, _rep = self.finish_raw()
        if rc != OK:
            self._ctx._err(rc)

    def state(self):
        """mi355_inflate_stream_state_get as a dict"""
        s = InflateStreamState()
        rc = load().mi355_inflate_stream_state_get(self._h, C.byref(s))
        if rc != OK:
            self._ctx._err(rc)
        return s.as_dict()

    @property
    def done(self):
        return bool(self.state()["done"])

    def reset(self):
        """Same wrapper and dictionary, a new stream; revives a dead handle"""
        rc = load().mi355_inflate_stream_reset(self._h)
        if rc != OK:
            self._ctx._err(rc)


class SeekIndex:
    """A seek index of one stream (mi355_inflate_seek): its table and the 32 KiB window in front of some of its entries, for reads of
    byte ranges.  Made by Context.inflate_seek (host bytes: the handle keeps a device copy of the stream) or
    Context.inflate_seek_device (the caller passes the stream's device pointer again at every read)."""

    def __init__(self, ctx, handle, report):
        self._ctx, self._h, self.report = ctx, handle, report

    def close(self):
        if getattr(self, "_h", None):
            load().mi355_inflate_seek_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def info(self):
        """mi355_inflate_seek_info"""
        i = SeekInfo()
        rc = load().mi355_inflate_seek_info(self._h, C.byref(i))
        if rc != OK:
            raise DeflateError(rc, "inflate seek: bad handle")
        return {k: getattr(i, k) for k, _ in SeekInfo._fields_ if k != "reserved"}

    def points(self):
        """mi355_inflate_seek_points: [(bit, pos)] of the points, entry 0 first"""
        n = C.c_size_t(0)
        load().mi355_inflate_seek_points(self._h, None, 0, C.byref(n))
        arr = (SeekPoint * max(n.value, 1))()
        rc = load().mi355_inflate_seek_points(self._h, arr, n.value, C.byref(n))
        if rc != OK:
            raise DeflateError(rc, "inflate seek: bad handle")
        return [(arr[k].bit, arr[k].pos) for k in range(n.value)]

    def last_read(self):
        """mi355_inflate_seek_last_read: what the last read did, from its plan"""
        v = (C.c_uint64 * 4)()
        rc = load().mi355_inflate_seek_last_read(self._h, v)
        if rc != OK:
            raise DeflateError(rc, "inflate seek: bad handle")
        return dict(zip(("entries", "symbols", "steps", "sets"), v))

    def cuts(self):
        """mi355_inflate_seek_cuts: [(bit, pos, hdr_bit)] in stream order; none when the handle was built without cuts"""
        n = C.c_size_t(0)
        load().mi355_inflate_seek_cuts(self._h, None, 0, C.byref(n))
        arr = (SeekCut * max(n.value, 1))()
        rc = load().mi355_inflate_seek_cuts(self._h, arr, n.value, C.byref(n))
        if rc != OK:
            raise DeflateError(rc, "inflate seek: bad handle")
        return [(arr[k].bit, arr[k].pos, arr[k].hdr_bit) for k in range(n.value)]

    def cut_info(self):
        """mi355_inflate_seek_cut_info"""
        v = (C.c_uint64 * 4)()
        rc = load().mi355_inflate_seek_cut_info(self._h, v)
        if rc != OK:
            raise DeflateError(rc, "inflate seek: bad handle")
        return dict(zip(("cut_bytes", "n_cuts", "host_bytes", "largest_cut"), v))

    def last_read_cuts(self):
        """mi355_inflate_seek_last_read_cuts: what the last read did"""
        v = (C.c_uint64 * 4)()
        rc = load().mi355_inflate_seek_last_read_cuts(self._h, v)
        if rc != OK:
            raise DeflateError(rc, "inflate seek: bad handle")
        return dict(zip(("cuts", "symbols", "steps", "launches"), v))

    def read_raw(self, off, length):
        """mi355_inflate_seek_read on a handle of Context.inflate_seek: (rc, report dict, the bytes that hold data); rc is OK or E_DATA"""
        out = C.create_string_buffer(max(length, 1))
        got, r = C.c_uint64(0), InflateReport()
        rc = load().mi355_inflate_seek_read(self._h, off, length, C.cast(out, C.c_void_p) if length else None, C.byref(got), C.byref(r))
        if rc not in (OK, E_DATA):
            self._ctx._err(rc)
        return rc, r.as_dict(), out.raw[:got.value]

    def read(self, off, length):
        """pread: the stream's bytes [off, off + length), fewer at its end; DeflateError(E_DATA, ...) if the stream no longer decodes"""
        rc, _rep, data = self.read_raw(off, length)
        if rc != OK:
            self._ctx._err(rc)
        return data

    def read_device(self, off, length, d_out_ptr, d_stream_ptr=0, stream=0, check=False):
        """mi355_inflate_seek_read_device: (rc, got, report dict).  d_stream_ptr 0: the handle's own copy of the stream."""
        got, r = C.c_uint64(0), InflateReport()
        rc = load().mi355_inflate_seek_read_device(self._h, C.c_void_p(d_stream_ptr), off, length, C.c_void_p(d_out_ptr), C.byref(got),
                                                   C.byref(r), C.c_void_p(stream))
        if rc not in (OK, E_DATA) or (check and rc != OK):
            self._ctx._err(rc)
        return rc, got.value, r.as_dict()

    def read_batch_device(self, ranges, d_stream_ptr=0, stream=0, check=False):
        """mi355_inflate_seek_read_batch_device: ranges = [(off, len, d_out_ptr)], all through one launch set.  Returns (rc, [(status,
        got, report dict)])."""
        n = len(ranges)
        arr = (SeekRange * max(n, 1))()
        for k, (off, length, ptr) in enumerate(ranges):
            arr[k].off, arr[k].len, arr[k].out = off, length, ptr
        reps = (InflateReport * max(n, 1))()
        rc = load().mi355_inflate_seek_read_batch_device(self._h, C.c_void_p(d_stream_ptr), arr, n, reps, C.c_void_p(stream))
        if rc not in (OK, E_DATA) or (check and rc != OK):
            self._ctx._err(rc)
        return rc, [(arr[k].status, arr[k].got, reps[k].as_dict()) for k in range(n)]

    def read_batch(self, ranges):
        """[(off, len), ...] -> [bytes, ...]: one launch set for all of them, through a device buffer of this call"""
        import torch

        total = sum(length for _off, length in ranges)
        buf = torch.empty(max(total, 1), dtype=torch.uint8, device="cuda:%d" % self._ctx.device)
        at, items = 0, []
        for off, length in ranges:
            items.append((off, length, buf.data_ptr() + at if length else 0))
            at += length
        _rc, res = self.read_batch_device(items, check=True)
        host = buf.cpu().numpy().tobytes()
        out, at = [], 0
        for (_off, length), (_st, got, _rep) in zip(ranges, res):
            out.append(host[at:at + got])
            at += length
        return out


class BgzfIndex:
    """The member table of a BGZF file (mi355_bgzf_index), for reads of byte ranges of its uncompressed data.  It holds host memory
    only and is bound to no context.  Made by Context.bgzf_index / Context.bgzf_index_device, which keep the context and the file for
    the reads, or by bgzf_index_from_members, whose reads take ctx= and file= (or d_file_ptr=)."""

    def __init__(self, handle, report=None, ctx=None, file=None, d_file_ptr=0):
        self._h, self.report, self._ctx, self._file, self._d_file = handle, report, ctx, file, d_file_ptr

    def close(self):
        if getattr(self, "_h", None):
            load().mi355_bgzf_index_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @staticmethod
    def _check(rc, what):
        if rc != OK:
            raise DeflateError(rc, "bgzf index: " + what)

    def info(self):
        """mi355_bgzf_index_info"""
        i = BgzfInfo()
        self._check(load().mi355_bgzf_index_info(self._h, C.byref(i)), "bad handle")
        return {k: getattr(i, k) for k, _ in BgzfInfo._fields_}

    def members(self):
        """mi355_bgzf_index_members: the table, one dict per member"""
        n = C.c_size_t(0)
        load().mi355_bgzf_index_members(self._h, None, 0, C.byref(n))
        arr = (MemberInfo * max(n.value, 1))()
        self._check(load().mi355_bgzf_index_members(self._h, arr, n.value, C.byref(n)), "bad handle")
        return [arr[k].as_dict() for k in range(n.value)]

    def voffset(self, uoff):
        """mi355_bgzf_voffset: htslib's virtual offset of an uncompressed offset"""
        v = C.c_uint64(0)
        self._check(load().mi355_bgzf_voffset(self._h, uoff, C.byref(v)), "no virtual offset for %d" % uoff)
        return v.value

    def uoffset(self, voff):
        """mi355_bgzf_uoffset: the uncompressed offset of a virtual offset"""
        u = C.c_uint64(0)
        self._check(load().mi355_bgzf_uoffset(self._h, voff, C.byref(u)), "no such virtual offset: %#x" % voff)
        return u.value

    def _context(self, ctx):
        ctx = ctx or self._ctx
        if ctx is None:
            raise ValueError("this index was made from a member table: pass ctx=")
        return ctx

    def last_read(self, ctx=None):
        """mi355_bgzf_last_read of the context the reads ran on"""
        ctx = self._context(ctx)
        v = (C.c_uint64 * 6)()
        rc = load().mi355_bgzf_last_read(ctx._h, v)
        if rc != OK:
            ctx._err(rc)
        return dict(zip(("distinct", "in_place", "scratch", "pieces", "sets", "copied"), v))

    def read_raw(self, off, length, ctx=None, file=None):
        """mi355_bgzf_read on host bytes: (rc, got, report dict, the bytes that hold data); rc is OK or E_DATA"""
        ctx = self._context(ctx)
        file = self._file if file is None else bytes(file)
        if file is None:
            raise ValueError("this index keeps no file: pass file=")
        room = min(length, self.info()["total"])
        out = C.create_string_buffer(max(room, 1))
        got, r = C.c_uint64(0), InflateReport()
        rc = load().mi355_bgzf_read(ctx._h, self._h, file, off, min(length, room), C.cast(out, C.c_void_p) if room else None, C.byref(got),
                                    C.byref(r))
        if rc not in (OK, E_DATA):
            ctx._err(rc)
        return rc, got.value, r.as_dict(), out.raw[:got.value]

    def read(self, off, length, ctx=None, file=None):
        """pread over the uncompressed bytes: [off, off + length), fewer at the end; DeflateError(E_DATA, ...) if a touched member
        is not what the index claims"""
        ctx = self._context(ctx)
        rc, _got, _rep, data = self.read_raw(off, length, ctx, file)
        if rc != OK:
            ctx._err(rc)
        return data

    def read_device(self, off, length, d_out_ptr, d_file_ptr=0, ctx=None, stream=0, check=False):
        """mi355_bgzf_read_device: (rc, got, report dict).  d_file_ptr 0: the pointer Context.bgzf_index_device was given."""
        ctx = self._context(ctx)
        got, r = C.c_uint64(0), InflateReport()
        rc = load().mi355_bgzf_read_device(ctx._h, self._h, C.c_void_p(d_file_ptr or self._d_file), off, length, C.c_void_p(d_out_ptr),
                                           C.byref(got), C.byref(r), C.c_void_p(stream))
        if rc not in (OK, E_DATA) or (check and rc != OK):
            ctx._err(rc)
        return rc, got.value, r.as_dict()

    def read_batch_device(self, ranges, d_file_ptr=0, ctx=None, stream=0, check=False):
        """mi355_bgzf_read_batch_device: ranges = [(off, len, d_out_ptr)]; every touched member is decoded once.  Returns (rc,
        [(status, got, report dict)])."""
        ctx = self._context(ctx)
        n = len(ranges)
        arr = (SeekRange * max(n, 1))()
        for k, (off, length, ptr) in enumerate(ranges):
            arr[k].off, arr[k].len, arr[k].out = off, length, ptr
        reps = (InflateReport * max(n, 1))()
        rc = load().mi355_bgzf_read_batch_device(ctx._h, self._h, C.c_void_p(d_file_ptr or self._d_file), arr, n, reps, C.c_void_p(stream))
        if rc not in (OK, E_DATA, E_UNSUPPORTED) or (check and rc != OK):
            ctx._err(rc)
        return rc, [(arr[k].status, arr[k].got, reps[k].as_dict()) for k in range(n)]

    def read_batch(self, ranges, ctx=None, file=None):
        """[(off, len), ...] -> [bytes, ...] from host bytes: the file goes to the device once, the ranges through one call"""
        import torch

        ctx = self._context(ctx)
        file = self._file if file is None else bytes(file)
        if file is None:
            raise ValueError("this index keeps no file: pass file=")
        dev = "cuda:%d" % ctx.device
        d_file = torch.frombuffer(bytearray(file) or bytearray(1), dtype=torch.uint8).to(dev)
        total = self.info()["total"]
        rooms = [min(length, max(total - off, 0)) for off, length in ranges]
        buf = torch.empty(max(sum(rooms), 1), dtype=torch.uint8, device=dev)
        at, items = 0, []
        for (off, _length), room in zip(ranges, rooms):
            items.append((off, room, buf.data_ptr() + at if room else 0))
            at += room
        _rc, res = self.read_batch_device(items, d_file.data_ptr(), ctx, check=True)
        host = buf.cpu().numpy().tobytes()
        out, at = [], 0
        for room, (_st, got, _rep) in zip(rooms, res):
            out.append(host[at:at + got])
            at += room
        return out


def bgzf_index_from_members(members, file_len):
    """mi355_bgzf_index_from_members: a BgzfIndex from the table mi355_bgzf_encode or a successful mi355_inflate_members returned
    ([MemberInfo], or dicts as MemberInfo.as_dict gives them).  No GPU and no context."""
    arr = (MemberInfo * max(len(members), 1))()
    for k, m in enumerate(members):
        if isinstance(m, dict):
            st = m.get("status", 0)
            st = VERIFY_STATUS.index(st) if isinstance(st, str) else st
            arr[k] = MemberInfo(m["in_off"], m["in_len"], m["out_off"], m["out_len"], m.get("flags", 0), st)
        else:
            arr[k] = MemberInfo(m.in_off, m.in_len, m.out_off, m.out_len, m.flags, m.status)
    h = C.c_void_p()
    rc = load().mi355_bgzf_index_from_members(arr if len(members) else None, len(members), file_len, C.byref(h))
    if rc != OK:
        raise DeflateError(rc, "bgzf index: the member table does not describe a file of %d bytes" % file_len)
    return BgzfIndex(h)


class Context:
    """One HIP device + workspace (mi355_deflate_ctx)."""

    def __init__(self, device=0):
        L = load()
        h = C.c_void_p()
        rc = L.mi355_deflate_ctx_create(device, C.byref(h))
        if rc != OK:
            raise DeflateError(rc, "cannot create a context on HIP device %d (no GPU? no CPU fallback exists)"
                               % device)
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            load().mi355_deflate_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _err(self, rc):
        raise DeflateError(rc, load().mi355_deflate_last_error(self._h).decode())

    CFG_RANGE_BYTES, CFG_LONG_FROM, CFG_SORT_RANKS, CFG_HOST_STREAMING, CFG_MULTI_STITCH, CFG_STEPS_IN_EMIT = 1, 2, 3, 4, 5, 6
    CFG_HOST_BOUNCE, CFG_HOST_THREADS, CFG_STAGE_CLOCKS, CFG_BATCH_BYTES = 7, 8, 9, 10
    CFG_INFLATE_GROUP_BYTES = 11
    CFG_INFLATE_INDEX_SPAN_BYTES = 12
    CFG_INFLATE_MEMBER_SPAN_BYTES = 13
    CFG_INFLATE_MEMBER_PARALLEL_BYTES = 14
    CFG_INFLATE_SEEK_CUT_BYTES = 15
    CFG_INFLATE_SEEK_CUT_WALKER = 16
    HOST_PATH_PIECES, HOST_PATH_IN_THREADS, HOST_PATH_OUT_THREADS = 1, 2, 4

    def config(self, key, value):
        """mi355_deflate_ctx_config: range size / long-input threshold / where the sort takes its ranks from"""
        rc = load().mi355_deflate_ctx_config(self._h, int(key), int(value))
        if rc != OK:
            self._err(rc)

    def config_get(self, key):
        """mi355_deflate_ctx_config_get: what a key of the decode side (11 to 16) is set to"""
        v = C.c_uint64(0)
        rc = load().mi355_deflate_ctx_config_get(self._h, int(key), C.byref(v))
        if rc != OK:
            self._err(rc)
        return v.value

    def reserve(self, in_len, host_api=False):
        """mi355_deflate_ctx_reserve: allocate for inputs of up to in_len bytes now"""
        rc = load().mi355_deflate_ctx_reserve(self._h, in_len, 1 if host_api else 0)
        if rc != OK:
            self._err(rc)

    def encode(self, data, options=Compression.Default, wrapper=0, compat=0, flush=0, verify=False):
        """Host bytes in, host bytes out (mi355_deflate_encode).  verify: check the stream against the input on the device, with
        the encode's block table (mi355_deflate_verify), and raise DeflateError(E_VERIFY, ...) if it does not inflate to it."""
        L = load()
        o = CompressionOptions.from_(options).to_c(wrapper, compat, flush)
        data = bytes(data)
        cap = L.mi355_deflate_bound(len(data)) + 16
        out = (C.c_uint8 * cap)()
        n = C.c_size_t(0)
        rc = L.mi355_deflate_encode(self._h, data, len(data), C.byref(o), out, cap, C.byref(n))
        if rc != OK:
            self._err(rc)
        res = bytes(memoryview(out)[: n.value])
        if verify:
            self._verify_last(res, data, wrapper)
        return res

    def encode_host_ptr(self, in_ptr, in_len, out_ptr, out_cap, options=Compression.Default, wrapper=0):
        """mi355_deflate_encode on raw host pointers (e.g. pinned buffers): H2D, encode, D2H; returns the length"""
        L = load()
        o = CompressionOptions.from_(options).to_c(wrapper, 0, 0)
        n = C.c_size_t(0)
        rc = L.mi355_deflate_encode(self._h, C.cast(C.c_void_p(in_ptr), C.c_char_p), in_len, C.byref(o),
                                    C.cast(C.c_void_p(out_ptr), C.POINTER(C.c_uint8)), out_cap, C.byref(n))
        if rc != OK:
            self._err(rc)
        return n.value

    def encode_gzip(self, data, options=Compression.Default, header=None, compat=0, verify=False):
        """mi355_deflate_encode_gzip; header = GzBuilder::into_header() bytes (None: the blank one).  verify: as in encode."""
        L = load()
        o = CompressionOptions.from_(options).to_c(2, compat, 0)
        data = bytes(data)
        header = BLANK_GZIP_HEADER if header is None else bytes(header)
        cap = L.mi355_deflate_bound(len(data)) + 32 + len(header)
        out = (C.c_uint8 * cap)()
        n = C.c_size_t(0)
        rc = L.mi355_deflate_encode_gzip(self._h, data, len(data), C.byref(o), header, len(header), out, cap,
                                         C.byref(n))
        if rc != OK:
            self._err(rc)
        res = bytes(memoryview(out)[: n.value])
        if verify:
            self._verify_last(res, data, 2)
        return res

    def crc32_device(self, d_ptr, n, stream=0):
        a = C.c_uint32(0)
        rc = load().mi355_crc32_device(self._h, C.c_void_p(d_ptr), n, C.byref(a), C.c_void_p(stream))
        if rc != OK:
            self._err(rc)
        return a.value

    def encode_device(self, d_in_ptr, in_len, d_out_ptr, out_cap, options=Compression.Default, wrapper=0,
                      compat=0, stream=0, flush=0):
        """Device pointers in/out (mi355_deflate_encode_device); returns the output length."""
        L = load()
        o = CompressionOptions.from_(options).to_c(wrapper, compat, flush)
        n = C.c_size_t(0)
        rc = L.mi355_deflate_encode_device(self._h, C.c_void_p(d_in_ptr), in_len, C.byref(o), C.c_void_p(d_out_ptr),
                                           out_cap, C.byref(n), C.c_void_p(stream))
        if rc != OK:
            self._err(rc)
        return n.value

    def _batch_error(self, rc, items):
        bad = [k for k in range(len(items)) if items[k].status != OK]
        if not bad:
            self._err(rc)
        raise DeflateError(rc, "batch item %d failed (status %d): %s" % (bad[0], items[bad[0]].status,
                                                                        load().mi355_deflate_last_error(self._h).decode()))

    def encode_batch(self, datas, options=Compression.Default, wrapper=0, compat=0):
        """Many host inputs in one batched call (mi355_deflate_encode_batch); a list of bytes, item i's exactly what
        encode(datas[i]) gives.  Raises DeflateError naming the first failing index."""
        L = load()
        o = CompressionOptions.from_(options).to_c(wrapper, compat, 0)
        datas = [bytes(d) for d in datas]
        items = (BatchItem * max(len(datas), 1))()
        outs = []
        for k, d in enumerate(datas):
            cap = L.mi355_deflate_bound_ex(len(d), wrapper, 0, 0)
            out = (C.c_uint8 * max(cap, 1))()
            outs.append(out)
            items[k].in_ = C.cast(C.c_char_p(d), C.c_void_p) if d else C.c_void_p(0)
            items[k].in_len = len(d)
            items[k].out = C.cast(out, C.c_void_p)
            items[k].out_cap = cap
        rc = L.mi355_deflate_encode_batch(self._h, items, len(datas), C.byref(o))
        if rc != OK:
            self._batch_error(rc, items[: len(datas)])
        return [bytes(memoryview(outs[k])[: items[k].out_len]) for k in range(len(datas))]

    def encode_batch_device(self, ins, outs=None, options=Compression.Default, wrapper=0, compat=0, stream=0, check=True):
        """Device inputs in one batched call (mi355_deflate_encode_batch_device).  ins: torch tensors on this context's device
        or (pointer, length) pairs; outs: the same for the outputs (None: uint8 tensors of mi355_deflate_bound_ex bytes, made
        here).  Returns (outs, lengths, statuses).  check: raise DeflateError naming the first failing index."""
        L = load()
        o = CompressionOptions.from_(options).to_c(wrapper, compat, 0)

        def ptr_len(x):
            if isinstance(x, tuple):
                return int(x[0]), int(x[1])
            return int(x.data_ptr()), int(x.numel() * x.element_size())
        ins_pl = [ptr_len(x) for x in ins]
        if outs is None:
            import torch
            dev = ins[0].device if ins and not isinstance(ins[0], tuple) else torch.device("cuda", 0)
            outs = [torch.empty(L.mi355_deflate_bound_ex(n, wrapper, 0, 0), dtype=torch.uint8, device=dev) for _, n in ins_pl]
        outs_pl = [ptr_len(x) for x in outs]
        items = (BatchItem * max(len(ins_pl), 1))()
        for k, ((ip, n), (op, cap)) in enumerate(zip(ins_pl, outs_pl)):
            items[k].in_ = C.c_void_p(ip if n else 0)
            items[k].in_len = n
            items[k].out = C.c_void_p(op)
            items[k].out_cap = cap
        rc = L.mi355_deflate_encode_batch_device(self._h, items, len(ins_pl), C.byref(o), C.c_void_p(stream))
        if rc != OK and check:
            self._batch_error(rc, items[: len(ins_pl)])
        return outs, [items[k].out_len for k in range(len(ins_pl))], [items[k].status for k in range(len(ins_pl))]

    @staticmethod
    def _gzip_headers(headers, n_items):
        """headers (None, one bytes, or a list as long as the batch) as (the GzipHeader array or None, n_hdrs, the bytes kept alive,
        item i's header length)"""
        if headers is None:
            return None, 0, [], [len(BLANK_GZIP_HEADER)] * n_items
        one = isinstance(headers, (bytes, bytearray, memoryview))
        hs = [bytes(headers)] if one else [bytes(h) for h in headers]
        if not one and len(hs) != n_items:
            raise ValueError("headers: None, one bytes, or one per item (%d for %d items)" % (len(hs), n_items))
        arr = (GzipHeader * max(len(hs), 1))()
        for k, h in enumerate(hs):
            arr[k].hdr = h
            arr[k].hdr_len = len(h)
        return arr, len(hs), hs, [len(hs[0 if one else k]) for k in range(n_items)]

    def encode_batch_gzip(self, datas, options=Compression.Default, headers=None, compat=0):
        """Many host inputs in one batched call, each a gzip member (mi355_deflate_encode_batch_gzip); a list of bytes, item i's
        exactly what encode_gzip(datas[i], options, header_i) gives.  headers: None (the blank header), one bytes for all, or a
        list as long as the batch (GzBuilder::into_header() bytes, e.g. gzip_header()).  Raises DeflateError naming the first
        failing index."""
        L = load()
        o = CompressionOptions.from_(options).to_c(2, compat, 0)
        datas = [bytes(d) for d in datas]
        arr, n_hdrs, keep, hlen = self._gzip_headers(headers, len(datas))
        items = (BatchItem * max(len(datas), 1))()
        outs = []
        for k, d in enumerate(datas):
            cap = L.mi355_deflate_bound_ex(len(d), 2, hlen[k], 0)
            out = (C.c_uint8 * max(cap, 1))()
            outs.append(out)
            items[k].in_ = C.cast(C.c_char_p(d), C.c_void_p) if d else C.c_void_p(0)
            items[k].in_len = len(d)
            items[k].out = C.cast(out, C.c_void_p)
            items[k].out_cap = cap
        rc = L.mi355_deflate_encode_batch_gzip(self._h, items, len(datas), C.byref(o), arr, n_hdrs)
        if rc != OK:
            self._batch_error(rc, items[: len(datas)])
        return [bytes(memoryview(outs[k])[: items[k].out_len]) for k in range(len(datas))]

    def encode_batch_device_gzip(self, ins, outs=None, options=Compression.Default, headers=None, compat=0, stream=0, check=True):
        """Device inputs in one batched call, each a gzip member (mi355_deflate_encode_batch_device_gzip).  ins / outs / the
        return value as encode_batch_device (outs None: uint8 tensors of mi355_deflate_bound_ex(n, 2, len(header_i), 0) bytes);
        headers as encode_batch_gzip (host bytes)."""
        L = load()
        o = CompressionOptions.from_(options).to_c(2, compat, 0)

        def ptr_len(x):
            if isinstance(x, tuple):
                return int(x[0]), int(x[1])
            return int(x.data_ptr()), int(x.numel() * x.element_size())
        ins_pl = [ptr_len(x) for x in ins]
        arr, n_hdrs, keep, hlen = self._gzip_headers(headers, len(ins_pl))
        if outs is None:
            import torch
            dev = ins[0].device if ins and not isinstance(ins[0], tuple) else torch.device("cuda", 0)
            outs = [torch.empty(L.mi355_deflate_bound_ex(n, 2, hlen[k], 0), dtype=torch.uint8, device=dev)
                    for k, (_, n) in enumerate(ins_pl)]
        outs_pl = [ptr_len(x) for x in outs]
        items = (BatchItem * max(len(ins_pl), 1))()
        for k, ((ip, n), (op, cap)) in enumerate(zip(ins_pl, outs_pl)):
            items[k].in_ = C.c_void_p(ip if n else 0)
            items[k].in_len = n
            items[k].out = C.c_void_p(op)
            items[k].out_cap = cap
        rc = L.mi355_deflate_encode_batch_device_gzip(self._h, items, len(ins_pl), C.byref(o), arr, n_hdrs, C.c_void_p(stream))
        if rc != OK and check:
            self._batch_error(rc, items[: len(ins_pl)])
        return outs, [items[k].out_len for k in range(len(ins_pl))], [items[k].status for k in range(len(ins_pl))]

    def _packed_result(self, arena, base, items, n, used, rc, check):
        if rc != OK and check:
            self._batch_error(rc, items[:n])
        entries = [((items[k].out - base) if items[k].status == OK and items[k].out else None, items[k].out_len) for k in range(n)]
        return PackedResult(arena, entries, [items[k].status for k in range(n)], used, rc)

    def encode_batch_packed(self, datas, options=Compression.Default, wrapper=0, headers=None, align=4, compat=0, arena_cap=None,
                            arena=None, check=True):
        """Many host inputs in one batched call, all streams in ONE arena (mi355_deflate_encode_batch_packed).  Returns
        (arena, [(off, len), ...]): item i's bytes are arena[off : off + len], exactly what encode(datas[i]) / encode_gzip gives;
        off is a multiple of align and the regions are dense.  wrapper 2: headers as encode_batch_gzip.  arena_cap None: the
        bound of packed_bound(); a smaller one is legal (mi355_deflate.h).  arena: a writable ctypes array to use instead of one
        made here (then arena_cap defaults to its size); otherwise the arena comes back as a bytearray of the bytes used.
        check False: no exception for a failing item, and the return value is the PackedResult."""
        L = load()
        o = CompressionOptions.from_(options).to_c(wrapper, compat, 0)
        datas = [bytes(d) for d in datas]
        n = len(datas)
        arr, n_hdrs, keep, _ = self._gzip_headers(headers if wrapper == 2 else None, n)
        items = (BatchItem * max(n, 1))()
        for k, d in enumerate(datas):
            items[k].in_ = C.cast(C.c_char_p(d), C.c_void_p) if d else C.c_void_p(0)
            items[k].in_len = len(d)
        own = arena is None
        if own:
            if arena_cap is None:
                arena_cap = L.mi355_deflate_batch_packed_bound(items, n, wrapper, arr, n_hdrs, align)
            arena = (C.c_uint8 * max(arena_cap, 1))()
        elif arena_cap is None:
            arena_cap = C.sizeof(arena)
        used = C.c_size_t(0)
        rc = L.mi355_deflate_encode_batch_packed(self._h, items, n, C.byref(o), arr, n_hdrs, C.cast(arena, C.c_void_p), arena_cap,
                                                 align, C.byref(used))
        res = self._packed_result(arena, C.addressof(arena), items, n, used.value, rc, check)
        if own:
            res.arena = bytearray(memoryview(arena)[: min(used.value, arena_cap)])
        return (res.arena, res.entries) if check else res

    def encode_batch_packed_device(self, ins, arena=None, options=Compression.Default, wrapper=0, headers=None, align=4, compat=0,
                                   arena_cap=None, table=None, stream=0, check=True):
        """Device inputs in one batched call, all streams in ONE device arena (mi355_deflate_encode_batch_packed_device).  ins: torch
        tensors on this context's device or (pointer, length) pairs; arena: a uint8 tensor or such a pair, aligned to align (None:
        a tensor of packed_bound() bytes, made here); table: None, or a device buffer of 24 bytes per item (tensor or pair) that
        receives the items' mi355_packed_entry.  Returns a PackedResult (arena = the tensor or pair).  check: raise DeflateError
        naming the first failing index."""
        L = load()
        o = CompressionOptions.from_(options).to_c(wrapper, compat, 0)

        def ptr_len(x):
            if isinstance(x, tuple):
                return int(x[0]), int(x[1])
            return int(x.data_ptr()), int(x.numel() * x.element_size())
        ins_pl = [ptr_len(x) for x in ins]
        n = len(ins_pl)
        arr, n_hdrs, keep, _ = self._gzip_headers(headers if wrapper == 2 else None, n)
        items = (BatchItem * max(n, 1))()
        for k, (ip, ln) in enumerate(ins_pl):
            items[k].in_ = C.c_void_p(ip if ln else 0)
            items[k].in_len = ln
        if arena is None:
            import torch
            dev = ins[0].device if ins and not isinstance(ins[0], tuple) else torch.device("cuda", 0)
            cap = arena_cap if arena_cap is not None else L.mi355_deflate_batch_packed_bound(items, n, wrapper, arr, n_hdrs, align)
            arena = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
            arena_cap = cap
        ap, alen = ptr_len(arena)
        if arena_cap is None:
            arena_cap = alen
        if table is not None and ptr_len(table)[1] < C.sizeof(PackedEntry) * n:
            raise ValueError("table: %d bytes per item" % C.sizeof(PackedEntry))
        used = C.c_size_t(0)
        rc = L.mi355_deflate_encode_batch_packed_device(self._h, items, n, C.byref(o), arr, n_hdrs, C.c_void_p(ap), arena_cap, align,
                                                        C.c_void_p(ptr_len(table)[0] if table is not None else 0), C.byref(used),
                                                        C.c_void_p(stream))
        return self._packed_result(arena, ap, items, n, used.value, rc, check)

    # ---- seek points: byte ranges of one large stream (mi355_inflate_seek_*) ----
    def _seek(self, call, cut):
        h, r = C.c_void_p(), InflateReport()
        if cut is not None:
            before = self.config_get(self.CFG_INFLATE_SEEK_CUT_BYTES)
            self.config(self.CFG_INFLATE_SEEK_CUT_BYTES, cut)  # the key is read at the build: set for it, the value before put back
        try:
            rc = call(C.byref(h), C.byref(r))
        finally:
            if cut is not None:
                self.config(self.CFG_INFLATE_SEEK_CUT_BYTES, before)
        if rc != OK:
            self._err(rc)
        return SeekIndex(self, h, r.as_dict())

    def inflate_seek(self, stream, wrapper=0, spacing=0, blocks=None, cut=0):
        """mi355_inflate_seek_build on host bytes -> SeekIndex.  spacing: output bytes between points, 0 = 1 MiB; blocks: the stream's
        table (Context.blocks()), else the device finds one.  cut: CFG_INFLATE_SEEK_CUT_BYTES for this build, the context's value put
        back behind it (0: no cuts; None: the key is left as the context has it).  A stream that does not decode raises DeflateError(E_DATA, ...)."""
        arr, nb = self._block_table(blocks)
        stream = bytes(stream)
        return self._seek(lambda h, r: load().mi355_inflate_seek_build(self._h, stream, len(stream), wrapper, arr, nb, spacing, h, r), cut)

    def inflate_seek_last_read_stages(self):
        """mi355_inflate_seek_last_read_stages: ms per launch kind of the last seek read (zeros unless CFG_STAGE_CLOCKS was on)"""
        v = (C.c_float * 4)()
        rc = load().mi355_inflate_seek_last_read_stages(self._h, v)
        if rc != OK:
            self._err(rc)
        return dict(zip(("pass1", "flatten", "windows", "resolve"), v))

    def inflate_seek_device(self, d_stream_ptr, stream_len, wrapper=0, spacing=0, blocks=None, stream=0, cut=0):
        """mi355_inflate_seek_build_device: the same for a stream in device memory, which the handle does not keep"""
        arr, nb = self._block_table(blocks)
        return self._seek(lambda h, r: load().mi355_inflate_seek_build_device(self._h, C.c_void_p(d_stream_ptr), stream_len, wrapper, arr, nb,
                                                                             spacing, h, r, C.c_void_p(stream)), cut)

    # ---- BGZF reads: byte ranges of a blocked gzip file from its member index (mi355_bgzf_index_*, mi355_bgzf_read*) ----
    def bgzf_index(self, file):
        """mi355_bgzf_index_build on host bytes -> BgzfIndex, which keeps this context and the file for its reads.  A file that is
        not BGZF members from its first to its last byte raises DeflateError(E_DATA, ...)."""
        file = bytes(file)
        h, r = C.c_void_p(), InflateReport()
        rc = load().mi355_bgzf_index_build(self._h, file, len(file), C.byref(h), C.byref(r))
        if rc != OK:
            self._err(rc)
        return BgzfIndex(h, r.as_dict(), self, file)

    def bgzf_index_device(self, d_file_ptr, file_len, stream=0):
        """mi355_bgzf_index_build_device: the same for a file in device memory, whose pointer the index remembers for read_device"""
        h, r = C.c_void_p(), InflateReport()
        rc = load().mi355_bgzf_index_build_device(self._h, C.c_void_p(d_file_ptr), file_len, C.byref(h), C.byref(r), C.c_void_p(stream))
        if rc != OK:
            self._err(rc)
        return BgzfIndex(h, r.as_dict(), self, None, d_file_ptr)

    def bgzf_last_read_stages(self):
        """mi355_bgzf_last_read_stages: ms per launch kind of the last BGZF read (zeros unless CFG_STAGE_CLOCKS was on)"""
        v = (C.c_float * 3)()
        rc = load().mi355_bgzf_last_read_stages(self._h, v)
        if rc != OK:
            self._err(rc)
        return dict(zip(("decode", "checksums", "trailers"), v))

    # ---- verify: does the stream inflate to the input? (mi355_deflate_verify*) ----
    @staticmethod
    def _block_table(blocks):
        """None, a BlockInfo array, or a list of dicts (Context.blocks()) / (bit_start, in_bytes) pairs -> (array or None, n)"""
        if blocks is None:
            return None, 0
        if isinstance(blocks, C.Array):
            return blocks, len(blocks)
        arr = (BlockInfo * max(len(blocks), 1))()
        for k, b in enumerate(blocks):
            arr[k].bit_start, arr[k].in_bytes = (b["bit_start"], b["in_bytes"]) if isinstance(b, dict) else (b[0], b[1])
        return arr, len(blocks)

    def verify(self, stream, data, wrapper=0, blocks=None, check=False):
        """mi355_deflate_verify: host bytes.  blocks: the table of the encode that made the stream (Context.blocks()) or None.
        Returns (rc, report dict); rc is OK or E_VERIFY.  Other return codes raise, and so does E_VERIFY with check=True."""
        arr, n = self._block_table(blocks)
        stream, data = bytes(stream), bytes(data)
        r = VerifyReport()
        rc = load().mi355_deflate_verify(self._h, stream, len(stream), data, len(data), wrapper, arr, n, C.byref(r))
        if rc not in (OK, E_VERIFY) or (rc != OK and check):
            self._err(rc)
        return rc, r.as_dict()

    def verify_device(self, d_stream_ptr, stream_len, d_in_ptr, in_len, wrapper=0, blocks=None, stream=0, check=False):
        """mi355_deflate_verify_device: device pointers; otherwise as verify"""
        arr, n = self._block_table(blocks)
        r = VerifyReport()
        rc = load().mi355_deflate_verify_device(self._h, C.c_void_p(d_stream_ptr), stream_len, C.c_void_p(d_in_ptr), in_len, wrapper,
                                                arr, n, C.byref(r), C.c_void_p(stream))
        if rc not in (OK, E_VERIFY) or (rc != OK and check):
            self._err(rc)
        return rc, r.as_dict()

    def verify_batch_device(self, items, wrapper=0, stream=0):
        """mi355_deflate_verify_batch_device.  items: a BatchItem array as a batch encode left it, or a list of
        (stream pointer, stream length, input pointer, input length) with an optional fifth element, the status on entry.
        Returns (rc, statuses, report dicts); the statuses of a BatchItem array are also written in place."""
        if not isinstance(items, C.Array):
            arr = (BatchItem * max(len(items), 1))()
            for k, it in enumerate(items):
                arr[k].out, arr[k].out_len, arr[k].in_, arr[k].in_len = C.c_void_p(it[0]), it[1], C.c_void_p(it[2]), it[3]
                arr[k].out_cap = it[1]
                arr[k].status = it[4] if len(it) > 4 else OK
            n, items = len(items), arr
        else:
            n = len(items)
        reps = (VerifyReport * max(n, 1))()
        rc = load().mi355_deflate_verify_batch_device(self._h, items, n, wrapper, reps, C.c_void_p(stream))
        if rc not in (OK, E_VERIFY):
            self._err(rc)
        return rc, [items[k].status for k in range(n)], [reps[k].as_dict() for k in range(n)]

    def _verify_last(self, stream, data, wrapper):
        """the stream of the encode this context has just done against its input, with that encode's block table"""
        L = load()
        nb = C.c_size_t(0)
        L.mi355_deflate_last_blocks(self._h, None, 0, C.byref(nb))
        arr = (BlockInfo * max(nb.value, 1))()
        rc = L.mi355_deflate_last_blocks(self._h, arr, nb.value, C.byref(nb))
        if rc != OK:
            self._err(rc)
        r = VerifyReport()
        rc = L.mi355_deflate_verify(self._h, stream, len(stream), data, len(data), wrapper, arr if nb.value else None, nb.value,
                                    C.byref(r))
        if rc != OK:
            self._err(rc)

    # ---- inflate: the stream's bytes (mi355_inflate*) ----
    def inflate_raw(self, stream, wrapper=0, out_cap=0, blocks=None, parallel=False):
        """mi355_inflate on host bytes, nothing raised for the three outcomes of a decode: (rc, out_len, report dict, the bytes
        of the buffer that hold data).  rc is OK, E_DATA or E_OUT_TOO_SMALL; out_cap 0 hands over no buffer (the size query).
        blocks: the table of the encode that made the stream (Context.blocks()): mi355_inflate_tabled, every entry decoded on its own.
        parallel: no table is at hand, the device finds one (mi355_inflate_parallel); an error together with blocks."""
        stream = bytes(stream)
        out = (C.c_uint8 * out_cap)() if out_cap else None
        n = C.c_size_t(0)
        r = InflateReport()
        if parallel:
            if blocks is not None:
                raise ValueError("parallel=True finds the table itself: give blocks or parallel, not both")
            rc = load().mi355_inflate_parallel(self._h, stream, len(stream), wrapper, C.cast(out, C.c_void_p) if out_cap else None,
                                               out_cap, C.byref(n), C.byref(r))
        elif blocks is None:
            rc = load().mi355_inflate(self._h, stream, len(stream), wrapper, C.cast(out, C.c_void_p) if out_cap else None, out_cap,
                                      C.byref(n), C.byref(r))
        else:
            arr, nb = self._block_table(blocks)
            rc = load().mi355_inflate_tabled(self._h, stream, len(stream), wrapper, arr, nb, C.cast(out, C.c_void_p) if out_cap else None,
                                             out_cap, C.byref(n), C.byref(r))
        if rc not in (OK, E_DATA, E_OUT_TOO_SMALL):
            self._err(rc)
        held = min(n.value, out_cap)
        return rc, n.value, r.as_dict(), bytes(memoryview(out)[:held]) if held else b""

    def inflate(self, stream, wrapper=0, out_cap=None, blocks=None, parallel=False):
        """Host bytes in, the bytes the stream (raw / zlib / gzip by wrapper) inflates to out.  out_cap None: the size is queried
        first (one decode that stores nothing), then the stream is decoded.  Raises DeflateError(E_DATA, ...) for a stream that
        is not valid and DeflateError(E_OUT_TOO_SMALL, ...) for one longer than a given out_cap.  blocks, parallel: as in inflate_raw."""
        if out_cap is None:
            rc, out_cap, _rep, _ = self.inflate_raw(stream, wrapper, 0, blocks, parallel)
            if rc == E_DATA:
                self._err(rc)
        rc, _n, _rep, data = self.inflate_raw(stream, wrapper, out_cap, blocks, parallel)
        if rc != OK:
            self._err(rc)
        return data

    def inflate_device(self, d_stream_ptr, stream_len, d_out_ptr, out_cap, wrapper=0, stream=0, check=False, blocks=None, parallel=False):
        """mi355_inflate_device: device pointers.  Returns (rc, out_len, report dict); rc is OK, E_DATA or E_OUT_TOO_SMALL.
        Other return codes raise, and so do those two with check=True.  blocks: the table of the encode that made the stream
        (Context.blocks()): mi355_inflate_tabled_device.  parallel: mi355_inflate_parallel_device, the table found on the device; an
        error together with blocks."""
        n = C.c_size_t(0)
        r = InflateReport()
        if parallel:
            if blocks is not None:
                raise ValueError("parallel=True finds the table itself: give blocks or parallel, not both")
            rc = load().mi355_inflate_parallel_device(self._h, C.c_void_p(d_stream_ptr), stream_len, wrapper, C.c_void_p(d_out_ptr), out_cap,
                                                      C.byref(n), C.byref(r), C.c_void_p(stream))
        elif blocks is None:
            rc = load().mi355_inflate_device(self._h, C.c_void_p(d_stream_ptr), stream_len, wrapper, C.c_void_p(d_out_ptr), out_cap,
                                             C.byref(n), C.byref(r), C.c_void_p(stream))
        else:
            arr, nb = self._block_table(blocks)
            rc = load().mi355_inflate_tabled_device(self._h, C.c_void_p(d_stream_ptr), stream_len, wrapper, arr, nb, C.c_void_p(d_out_ptr),
                                                    out_cap, C.byref(n), C.byref(r), C.c_void_p(stream))
        if rc not in (OK, E_DATA, E_OUT_TOO_SMALL) or (rc != OK and check):
            self._err(rc)
        return rc, n.value, r.as_dict()

    def inflate_tabled_stages(self):
        """mi355_inflate_tabled_last_stages: HIP-event ms of the last tabled inflate per launch kind (zeros without CFG_STAGE_CLOCKS)"""
        ms = (C.c_float * 4)()
        rc = load().mi355_inflate_tabled_last_stages(self._h, ms)
        if rc != OK:
            self._err(rc)
        return dict(zip(("decode_ms", "windows_ms", "resolve_ms", "checksums_ms"), ms))

    # ---- the table of a stream that came without one (mi355_inflate_index*) ----
    def _index(self, call):
        n = C.c_size_t(0)
        r = InflateReport()
        rc = call(None, 0, C.byref(n), C.byref(r))  # the query
        arr = (BlockInfo * max(n.value, 1))()
        if rc == E_OUT_TOO_SMALL:
            rc = call(arr, n.value, C.byref(n), C.byref(r))
        if rc != OK:
            self._err(rc)
        return [dict(btype=a.btype, bfinal=a.bfinal, n_lz=a.n_tokens, in_bytes=a.in_bytes, bit_start=a.bit_start) for a in arr[: n.value]]

    def inflate_index(self, stream, wrapper=0):
        """mi355_inflate_index on host bytes: the stream's block table, found on the device, in the form Context.blocks() returns --
        what blocks= of inflate and verify takes.  Raises DeflateError(E_DATA, ...) for a stream whose walk fails."""
        stream = bytes(stream)
        return self._index(lambda arr, cap, n, r: load().mi355_inflate_index(self._h, stream, len(stream), wrapper, arr, cap, n, r))

    def inflate_index_device(self, d_stream_ptr, stream_len, wrapper=0, stream=0):
        """mi355_inflate_index_device: the same for a stream in device memory"""
        return self._index(lambda arr, cap, n, r: load().mi355_inflate_index_device(self._h, C.c_void_p(d_stream_ptr), stream_len, wrapper,
                                                                                   arr, cap, n, r, C.c_void_p(stream)))

    def inflate_index_stages(self):
        """mi355_inflate_index_last_stages: ms of the last index -- the find and the walk launch (HIP events; zeros without
        CFG_STAGE_CLOCKS) and the host's link"""
        ms = (C.c_float * 3)()
        rc = load().mi355_inflate_index_last_stages(self._h, ms)
        if rc != OK:
            self._err(rc)
        return dict(zip(("find_ms", "walk_ms", "link_ms"), ms))

    def inflate_index_walks(self):
        """mi355_inflate_index_last_walks: the walkers' records of the last index, one tuple per span in IndexWalk's field order"""
        n = C.c_size_t(0)
        load().mi355_inflate_index_last_walks(self._h, None, 0, C.byref(n))
        arr = (IndexWalk * max(n.value, 1))()
        rc = load().mi355_inflate_index_last_walks(self._h, arr, n.value, C.byref(n))
        if rc != OK:
            self._err(rc)
        return [tuple(getattr(a, f) for f, _t in IndexWalk._fields_) for a in arr[: n.value]]

    # ---- a gzip file of any number of members (mi355_inflate_members*) ----
    def _members(self, call, room, table=True):
        """the call with a table of `room` entries, again with the count it names if that was too few (table False: whatever fits)"""
        n, nm, r = C.c_size_t(0), C.c_size_t(0), InflateReport()
        arr = (MemberInfo * max(room, 1))()
        rc = call(arr, room, C.byref(n), C.byref(nm), C.byref(r))
        if table and rc in (OK, E_DATA, E_OUT_TOO_SMALL) and nm.value > room:
            room = nm.value
            arr = (MemberInfo * room)()
            rc = call(arr, room, C.byref(n), C.byref(nm), C.byref(r))
        if rc not in (OK, E_DATA, E_OUT_TOO_SMALL):
            self._err(rc)
        return rc, n.value, r.as_dict(), [arr[k].as_dict() for k in range(min(nm.value, room))]

    def inflate_members_raw(self, stream, out_cap=0, room=None):
        """mi355_inflate_members on host bytes, nothing raised for the three outcomes of a decode: (rc, out_len, report dict, member
        dicts, the bytes of the buffer that hold data).  out_cap 0 hands over no buffer (the size query).  room: entries of the
        member table handed over -- None: a guess from the file's length, and the call again if the file has more; a number: that
        many and no second call, the list is cut there (0: no table at all)."""
        stream = bytes(stream)
        out = (C.c_uint8 * out_cap)() if out_cap else None
        rc, n, rep, members = self._members(
            lambda arr, room, pn, pm, pr: load().mi355_inflate_members(self._h, stream, len(stream), C.cast(out, C.c_void_p) if out_cap else None,
                                                                       out_cap, pn, arr if room else None, room, pm, pr),
            max(64, len(stream) // 4096) if room is None else room, room is None)
        held = min(n, out_cap)
        return rc, n, rep, members, bytes(memoryview(out)[:held]) if held else b""

    def _members_count(self, stream):
        """(rc, out_len, members walked) of the size query: no buffer and no table"""
        stream = bytes(stream)
        n, nm, r = C.c_size_t(0), C.c_size_t(0), InflateReport()
        rc = load().mi355_inflate_members(self._h, stream, len(stream), None, 0, C.byref(n), None, 0, C.byref(nm), C.byref(r))
        if rc not in (OK, E_DATA, E_OUT_TOO_SMALL):
            self._err(rc)
        return rc, n.value, nm.value

    def inflate_members(self, stream, out_cap=None):
        """A gzip file of any number of members (BGZF, `cat a.gz b.gz`, a packed gzip arena) in host bytes -> (data, members).
        out_cap None: the size is queried first.  Raises DeflateError(E_DATA, ...) for a file that is not valid and
        DeflateError(E_OUT_TOO_SMALL, ...) for one longer than a given out_cap."""
        room = None
        if out_cap is None:  # the size query needs no table, and its member count is the room of the decode: two decodes in all
            rc, out_cap, room = self._members_count(stream)
            if rc == E_DATA:
                self._err(rc)
        rc, _n, _rep, members, data = self.inflate_members_raw(stream, out_cap, room)
        if rc != OK:
            self._err(rc)
        return data, members

    def inflate_members_device(self, d_stream_ptr, stream_len, d_out_ptr, out_cap, stream=0, check=False):
        """mi355_inflate_members_device: device pointers.  Returns (rc, out_len, report dict, member dicts); rc is OK, E_DATA or
        E_OUT_TOO_SMALL.  Other return codes raise, and so do those two with check=True."""
        rc, n, rep, members = self._members(
            lambda arr, room, pn, pm, pr: load().mi355_inflate_members_device(self._h, C.c_void_p(d_stream_ptr), stream_len, C.c_void_p(d_out_ptr),
                                                                              out_cap, pn, arr, room, pm, pr, C.c_void_p(stream)),
            max(64, stream_len // 16384))
        if rc != OK and check:
            self._err(rc)
        return rc, n, rep, members

    # ---- BGZF encode: one input, one blocked gzip file (mi355_bgzf_*) ----
    def encode_bgzf_raw(self, data, options=Compression.Default, block_size=0, compat=0, out_cap=None, room=None):
        """mi355_bgzf_encode on host bytes, nothing raised: (rc, out_len, n_members, member dicts, the buffer's bytes).  out_cap None:
        the bound; 0 hands over no buffer (the size query).  room: entries of the member table handed over (None: all)."""
        L = load()
        o = CompressionOptions.from_(options).to_c(2, compat, 0)
        data = bytes(data)
        if out_cap is None:
            out_cap = L.mi355_bgzf_bound(len(data), block_size)
        if room is None:
            room = len(data) // (block_size or BGZF_BLOCK_MAX) + 2
        out = (C.c_uint8 * out_cap)() if out_cap else None
        arr = (MemberInfo * max(room, 1))()
        n, nm = C.c_size_t(0), C.c_size_t(0)
        rc = L.mi355_bgzf_encode(self._h, data, len(data), C.byref(o), block_size, C.cast(out, C.c_void_p) if out_cap else None, out_cap,
                                 C.byref(n), arr if room else None, room, C.byref(nm))
        return rc, n.value, nm.value, [arr[k].as_dict() for k in range(min(nm.value, room))], bytes(out) if out_cap else b""

    def encode_bgzf(self, data, options=Compression.Default, block_size=0, compat=0):
        """Host bytes -> (the BGZF file, its members): the input in slices of block_size bytes (0: 65280), a gzip member that states
        its size per slice, the end-of-file marker last (mi355_bgzf_encode).  members: dicts of mi355_member_info in file order."""
        rc, n, _nm, members, buf = self.encode_bgzf_raw(data, options, block_size, compat)
        if rc != OK:
            self._err(rc)
        return buf[:n], members

    def encode_bgzf_device(self, d_in_ptr, in_len, d_out_ptr, out_cap, options=Compression.Default, block_size=0, compat=0, stream=0,
                           room=None, check=True):
        """mi355_bgzf_encode_device on device pointers (d_out 16-byte aligned): (rc, out_len, n_members, member dicts); rc is OK or
        E_OUT_TOO_SMALL with check=False, else anything but OK raises."""
        L = load()
        o = CompressionOptions.from_(options).to_c(2, compat, 0)
        if room is None:
            room = in_len // (block_size or BGZF_BLOCK_MAX) + 2
        arr = (MemberInfo * max(room, 1))()
        n, nm = C.c_size_t(0), C.c_size_t(0)
        rc = L.mi355_bgzf_encode_device(self._h, C.c_void_p(d_in_ptr), in_len, C.byref(o), block_size, C.c_void_p(d_out_ptr), out_cap,
                                        C.byref(n), arr if room else None, room, C.byref(nm), C.c_void_p(stream))
        if rc != OK and (check or rc != E_OUT_TOO_SMALL):
            self._err(rc)
        return rc, n.value, nm.value, [arr[k].as_dict() for k in range(min(nm.value, room))]

    def bgzf_stages(self):
        """mi355_bgzf_last_stages: HIP-event ms of the last BGZF encode per stage (zeros without CFG_STAGE_CLOCKS)"""
        ms = (C.c_float * 3)()
        rc = load().mi355_bgzf_last_stages(self._h, ms)
        if rc != OK:
            self._err(rc)
        return dict(zip(("packed_encode_ms", "place_ms", "gather_ms"), ms))

    def inflate_members_stages(self):
        """mi355_inflate_members_last_stages: HIP-event ms of the last members call per launch kind (zeros without CFG_STAGE_CLOCKS)"""
        ms = (C.c_float * 6)()
        rc = load().mi355_inflate_members_last_stages(self._h, ms)
        if rc != OK:
            self._err(rc)
        return dict(zip(("find_ms", "walk_ms", "fill_ms", "member_decode_ms", "chain_decode_ms", "checksums_ms"), ms))

    def inflate_members_last_parallel(self):
        """mi355_inflate_members_last_parallel: what the parallel path of the last members call did (CFG_INFLATE_MEMBER_PARALLEL_BYTES)
        -- members it decoded, members handed back to the one-wave chain, index spans searched, walkers launched, table entries
        decoded, launch sets"""
        v = (C.c_uint64 * 6)()
        rc = load().mi355_inflate_members_last_parallel(self._h, v)
        if rc != OK:
            self._err(rc)
        return dict(zip(("parallel", "handed", "spans", "walkers", "entries", "sets"), v))

    def inflate_members_parallel_stages(self):
        """mi355_inflate_members_last_parallel_stages: HIP-event ms of the parallel path's launch kinds in the last members call
        (zeros without CFG_STAGE_CLOCKS)"""
        ms = (C.c_float * 5)()
        rc = load().mi355_inflate_members_last_parallel_stages(self._h, ms)
        if rc != OK:
            self._err(rc)
        return dict(zip(("discover_find_ms", "discover_walk_ms", "tabled_decode_ms", "windows_ms", "resolve_ms"), ms))

    def inflate_members_walks(self):
        """mi355_inflate_members_last_walks: (candidates, walkers' records as tuples in MemberWalk's field order) of the find and
        the first walk of the last members call, one of each per span; two empty lists behind an empty file"""
        n = C.c_size_t(0)
        load().mi355_inflate_members_last_walks(self._h, None, None, 0, C.byref(n))
        cand, arr = (C.c_uint64 * max(n.value, 1))(), (MemberWalk * max(n.value, 1))()
        rc = load().mi355_inflate_members_last_walks(self._h, cand, arr, n.value, C.byref(n))
        if rc != OK:
            self._err(rc)
        return list(cand[: n.value]), [tuple(getattr(a, f) for f, _t in MemberWalk._fields_) for a in arr[: n.value]]

    def inflate_batch_device(self, items, wrapper=0, stream=0):
        """mi355_inflate_batch_device.  items: a BatchItem array (in_ / in_len the stream, out / out_cap the buffer, e.g. the out
        pointers of a packed arena moved to in_), or a list of (stream pointer, stream length, buffer pointer, buffer size) with an
        optional fifth element, the status on entry.  Returns (rc, report dicts); out_len and status are written into the array,
        which is the second element's `items` attribute when a list was given."""
        if not isinstance(items, C.Array):
            arr = (BatchItem * max(len(items), 1))()
            for k, it in enumerate(items):
                arr[k].in_, arr[k].in_len, arr[k].out, arr[k].out_cap = C.c_void_p(it[0]), it[1], C.c_void_p(it[2]), it[3]
                arr[k].status = it[4] if len(it) > 4 else OK
            n, items = len(items), arr
        else:
            n = len(items)
        reps = (InflateReport * max(n, 1))()
        rc = load().mi355_inflate_batch_device(self._h, items, n, wrapper, reps, C.c_void_p(stream))
        if rc not in (OK, E_DATA, E_OUT_TOO_SMALL):
            self._err(rc)
        out = InflateReports(reps[k].as_dict() for k in range(n))
        out.items = items
        return rc, out

    # ---- streaming inflate (mi355_inflate_stream_*) ----
    def inflate_stream(self, wrapper=0, zdict=None):
        """A streaming inflate handle on this context.  zdict: a preset dictionary (raw streams only)."""
        h = C.c_void_p()
        zdict = bytes(zdict) if zdict else None
        rc = load().mi355_inflate_stream_new(self._h, wrapper, zdict, len(zdict) if zdict else 0, C.byref(h))
        if rc != OK:
            if rc == E_ARG:
                raise DeflateError(rc, "inflate stream: wrapper must be 0, 1 or 2, and a dictionary goes with wrapper 0 only")
            self._err(rc)
        return InflateStream(self, h)

    def inflate_stream_write_batch_device(self, streams, items, stream=0):
        """mi355_inflate_stream_write_batch_device.  streams: InflateStream handles; items: a BatchItem array, or a list of (chunk
        pointer, chunk length, buffer pointer, buffer size) with an optional fifth element, the status on entry.  Returns (rc, report
        dicts); out_len and status are written into the array, the second element's `items` attribute."""
        n = len(streams)
        if not isinstance(items, C.Array):
            arr = (BatchItem * max(n, 1))()
            for k, it in enumerate(items):
                arr[k].in_, arr[k].in_len, arr[k].out, arr[k].out_cap = C.c_void_p(it[0]), it[1], C.c_void_p(it[2]), it[3]
                arr[k].status = it[4] if len(it) > 4 else OK
            items = arr
        hs = (C.c_void_p * max(n, 1))(*[s._h for s in streams])
        reps = (InflateReport * max(n, 1))()
        rc = load().mi355_inflate_stream_write_batch_device(self._h, hs, items, n, reps, C.c_void_p(stream))
        if rc not in (OK, E_DATA, E_OUT_TOO_SMALL, E_STATE):
            self._err(rc)
        out = InflateReports(reps[k].as_dict() for k in range(n))
        out.items = items
        return rc, out

    def inflate_stream_write_batch(self, streams, chunks, room=None):
        """One chunk of host bytes for each handle, all through one call: [bytes], the next bytes of every stream.  room None:
        eight times the chunk (4096 at least) each; handles whose next block waits for room are written again, alone, with what
        their state asks for.  Raises DeflateError at the first handle that fails."""
        import torch

        dev = "cuda:%d" % self.device
        chunks = [bytes(c) for c in chunks]
        rooms = [max(8 * len(c), 4096) if room is None else room for c in chunks]
        d_in = torch.frombuffer(bytearray(b"".join(chunks)) or bytearray(1), dtype=torch.uint8).to(dev)
        d_out = torch.empty(max(sum(rooms), 1), dtype=torch.uint8, device=dev)
        items, a, b = [], 0, 0
        for c, r in zip(chunks, rooms):
            items.append((d_in.data_ptr() + a if c else 0, len(c), d_out.data_ptr() + b if r else 0, r))
            a, b = a + len(c), b + r
        rc, reps = self.inflate_stream_write_batch_device(streams, items)
        host = d_out.cpu().numpy().tobytes()
        out, b = [], 0
        for k, r in enumerate(rooms):
            out.append(host[b:b + reps.items[k].out_len])
            b += r
        for k, s in enumerate(streams):
            st = reps.items[k].status
            if st in (OK, E_OUT_TOO_SMALL) and room is None and s.state()["need_out"]:
                out[k] += s.write(b"")
            elif st != OK:
                raise DeflateError(st, "inflate stream: item %d: %s" % (k, reps[k]["status"]))
        return out

    def batch_info(self):
        """mi355_deflate_last_batch_info as a dict"""
        i = BatchInfo()
        load().mi355_deflate_last_batch_info(self._h, C.byref(i))
        return {k: getattr(i, k) for k, _ in BatchInfo._fields_}

    def info(self):
        i = Info()
        load().mi355_deflate_last_info(self._h, C.byref(i))
        d = {k: getattr(i, k) for k, _ in Info._fields_ if k not in ("stage_ms", "reserved")}
        d["stage_ms"] = {STAGES[k]: i.stage_ms[k] for k in range(6)}
        return d

    def blocks(self):
        """Block layout of the last encode, same dict shape as the oracle's trace."""
        L = load()
        n = C.c_size_t(0)
        L.mi355_deflate_last_blocks(self._h, None, 0, C.byref(n))
        arr = (BlockInfo * max(n.value, 1))()
        rc = L.mi355_deflate_last_blocks(self._h, arr, n.value, C.byref(n))
        if rc != OK:
            self._err(rc)
        return [dict(btype=a.btype, bfinal=a.bfinal, n_lz=a.n_tokens, in_bytes=a.in_bytes, bit_start=a.bit_start)
                for a in arr[: n.value]]

    def adler32_device(self, d_ptr, n, stream=0):
        a = C.c_uint32(0)
        rc = load().mi355_adler32_device(self._h, C.c_void_p(d_ptr), n, C.byref(a), C.c_void_p(stream))
        if rc != OK:
            self._err(rc)
        return a.value


_default = None


def default_context():
    global _default
    if _default is None:
        _default = Context(0)
    return _default


def bound(n):
    return load().mi355_deflate_bound(n)


class InflateReports(list):
    """the report dicts of an inflate batch; .items is the BatchItem array the call wrote out_len and status into"""
    items = None


def inflate_bytes(stream, wrapper=0, ctx=None, blocks=None, parallel=False, members=False):
    """The bytes `stream` (raw / zlib / gzip by wrapper) inflates to, decoded on the GPU; DeflateError(E_DATA, ...) if it is not valid.
    blocks: the block table of the encode that made the stream, for a parallel decode (Context.inflate); parallel: a parallel decode
    of a stream from anywhere, the table found on the device.  members: the stream is a gzip FILE of any number of members
    (Context.inflate_members); wrapper 2 only, and neither blocks nor parallel."""
    if members:
        if wrapper != 2 or blocks is not None or parallel:
            raise ValueError("members=True takes a gzip file: wrapper=2, and neither blocks nor parallel")
        return (ctx or default_context()).inflate_members(stream)[0]
    return (ctx or default_context()).inflate(stream, wrapper, blocks=blocks, parallel=parallel)


def verify_bytes(stream, data, wrapper=0, ctx=None):
    """Does `stream` (raw / zlib / gzip by wrapper) inflate to `data`?  (True, report) or (False, report); on the GPU, no table."""
    rc, rep = (ctx or default_context()).verify(stream, data, wrapper)
    return rc == OK, rep


# ---- the reference's one-shot functions (src/lib.rs) -------------------------------------------
def deflate_bytes_conf(data, options, ctx=None):
    """src/lib.rs:137-147"""
    return (ctx or default_context()).encode(data, options, wrapper=0)


def deflate_bytes(data, ctx=None):
    """src/lib.rs:163-165"""
    return deflate_bytes_conf(data, Compression.Default, ctx)


def deflate_bytes_zlib_conf(data, options, ctx=None):
    """src/lib.rs:182-198"""
    return (ctx or default_context()).encode(data, options, wrapper=1)


def deflate_bytes_zlib(data, ctx=None):
    """src/lib.rs:216-218"""
    return deflate_bytes_zlib_conf(data, Compression.Default, ctx)


# ---- the same, many inputs in one batched call (mi355_deflate_encode_batch) --------------------
def deflate_bytes_batch_conf(datas, options, ctx=None):
    """deflate_bytes_conf of every input, in one batch"""
    return (ctx or default_context()).encode_batch(datas, options, wrapper=0)


def deflate_bytes_batch(datas, ctx=None):
    return deflate_bytes_batch_conf(datas, Compression.Default, ctx)


def deflate_bytes_zlib_batch_conf(datas, options, ctx=None):
    """deflate_bytes_zlib_conf of every input, in one batch"""
    return (ctx or default_context()).encode_batch(datas, options, wrapper=1)


def deflate_bytes_zlib_batch(datas, ctx=None):
    return deflate_bytes_zlib_batch_conf(datas, Compression.Default, ctx)


# GzBuilder::new().into_header() of crate gzip-header 1.0 (the crate is not in the reference tree)
BLANK_GZIP_HEADER = bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff])


def gzip_header(filename=None, comment=None, extra=None, mtime=0, xfl=0, os_code=255):
    """RFC 1952 member header as GzBuilder builds it (fields in the order FEXTRA, FNAME, FCOMMENT)."""
    flg = (4 if extra is not None else 0) | (8 if filename is not None else 0) | (16 if comment is not None else 0)
    h = bytearray([0x1f, 0x8b, 8, flg]) + int(mtime).to_bytes(4, "little") + bytes([xfl, os_code])
    if extra is not None:
        h += len(extra).to_bytes(2, "little") + bytes(extra)
    if filename is not None:
        h += bytes(filename) + b"\0"
    if comment is not None:
        h += bytes(comment) + b"\0"
    return bytes(h)


def deflate_bytes_gzip_conf(data, options, header=None, ctx=None):
    """src/lib.rs:242-267 (feature "gzip"); header = GzBuilder::into_header() bytes"""
    return (ctx or default_context()).encode_gzip(data, options, header)


def deflate_bytes_gzip(data, ctx=None):
    """src/lib.rs:283-285"""
    return deflate_bytes_gzip_conf(data, Compression.Default, None, ctx)


def deflate_bytes_gzip_batch_conf(datas, options, headers=None, ctx=None):
    """deflate_bytes_gzip_conf of every input (src/lib.rs:242-267), in one batch; headers: None, one bytes, or one per input"""
    return (ctx or default_context()).encode_batch_gzip(datas, options, headers)


def deflate_bytes_gzip_batch(datas, ctx=None):
    return deflate_bytes_gzip_batch_conf(datas, Compression.Default, None, ctx)


# ---- ... with all outputs in one arena (mi355_deflate_encode_batch_packed) ------------------------
def packed_bound(lens, wrapper=0, headers=None, align=4):
    """mi355_deflate_batch_packed_bound: the arena that always suffices for inputs of these lengths (no GPU involved).
    headers (wrapper 2): None, one bytes, or one per input."""
    lens = [int(x) for x in lens]
    arr, n_hdrs, keep, _ = Context._gzip_headers(headers if wrapper == 2 else None, len(lens))
    items = (BatchItem * max(len(lens), 1))()
    for k, ln in enumerate(lens):
        items[k].in_len = ln
    return load().mi355_deflate_batch_packed_bound(items, len(lens), wrapper, arr, n_hdrs, align)


def deflate_bytes_batch_packed_conf(datas, options, wrapper=0, headers=None, align=4, ctx=None):
    """deflate_bytes_conf / _zlib_conf / _gzip_conf (wrapper 0 / 1 / 2) of every input, in one batch and one arena:
    (arena, [(off, len), ...])"""
    return (ctx or default_context()).encode_batch_packed(datas, options, wrapper=wrapper, headers=headers, align=align)


def deflate_bytes_batch_packed(datas, ctx=None):
    return deflate_bytes_batch_packed_conf(datas, Compression.Default, ctx=ctx)


# ---- the reference's Write encoders (src/writer.rs) ---------------------------------------------
BGZF_BLOCK_MAX = 65280  # bgzip's 0xff00: the largest (and the default) block_size of a BGZF encode
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_bound(n, block_size=0):
    """mi355_bgzf_bound: the output room that always suffices for a BGZF encode of n bytes (no GPU needed; 0 for a bad block_size)"""
    return load().mi355_bgzf_bound(n, block_size)


def bgzf_bytes(data, options=Compression.Default, block_size=0, ctx=None):
    """The BGZF file of `data` (Context.encode_bgzf without the member table)"""
    return (ctx or default_context()).encode_bgzf(data, options, block_size)[0]


def bgzf_gzi(members):
    """The .gzi index of `bgzip -i` for a member table (dicts or MemberInfo, the end-of-file marker included or not): a little-endian
    u64 count, then (compressed offset, uncompressed offset) u64 pairs for every data member but the first."""
    get = (lambda m, k: m[k]) if members and isinstance(members[0], dict) else getattr
    data = [m for m in members if get(m, "out_len")]
    pairs = [(get(m, "in_off"), get(m, "out_off")) for m in data[1:]]
    return struct.pack("<Q", len(pairs)) + b"".join(struct.pack("<QQ", a, b) for a, b in pairs)


class _Encoder:
    _wrapper = 0

    def __init__(self, writer, options=Compression.Default, ctx=None):
        """::new(writer, options) (writer.rs:93-99, 189-199); `writer` needs a .write(bytes)."""
        self._ctx = ctx or default_context()
        self._w = writer
        o = CompressionOptions.from_(options).to_c(self._wrapper, 0)
        h = C.c_void_p()
        rc = load().mi355_deflate_stream_new(self._ctx._h, C.byref(o), C.byref(h))
        if rc != OK:
            raise DeflateError(rc, "stream_new")
        self._s = h

    def _drain(self):
        """Hand what the encoder has produced to the inner writer, the way the reference does
        (compress.rs:96-124, 280-299; writer.rs:40-47): `W.write` may accept fewer bytes than offered
        (tests/test.rs:163-200 SmallWriter); a writer that returns None took everything."""
        L = load()
        p = C.POINTER(C.c_uint8)()
        n = C.c_size_t(0)
        while True:
            L.mi355_deflate_stream_output(self._s, C.byref(p), C.byref(n))
            if not n.value:
                return
            chunk = C.string_at(p, n.value)
            took = self._w.write(chunk)
            took = len(chunk) if took is None else int(took)
            if took <= 0:
                raise IOError("inner writer accepted no bytes (io::ErrorKind::WriteZero)")
            k = C.c_size_t(0)
            buf = (C.c_uint8 * took)()
            L.mi355_deflate_stream_take_output(self._s, buf, took, C.byref(k))

    def write(self, buf):
        """io::Write::write (always consumes everything, like write_all)"""
        buf = bytes(buf)
        rc = load().mi355_deflate_stream_write(self._s, buf, len(buf))
        if rc != OK:
            raise DeflateError(rc, "stream_write")
        self._drain()
        return len(buf)

    write_all = write

    def flush(self):
        """io::Write::flush = Flush::Sync (writer.rs:134-137): sync marker, window kept; the inner writer
        holds the bytes -- ending in 00 00 FF FF -- when this returns (writer.rs:570-595)"""
        L = load()
        rc = L.mi355_deflate_stream_flush(self._s)
        if rc != OK:
            raise DeflateError(rc, L.mi355_deflate_last_error(self._ctx._h).decode())
        self._drain()

    def finish(self):
        """finish(self) -> W (writer.rs:103-108, 209-214)"""
        L = load()
        rc = L.mi355_deflate_stream_finish(self._s)
        if rc != OK:
            raise DeflateError(rc, L.mi355_deflate_last_error(self._ctx._h).decode())
        self._drain()
        self._done = True
        return self._w

    def reset(self, writer):
        """reset(&mut self, W) -> W (writer.rs:110-117, 216-223, 383-402): the finished stream goes to the
        old writer, which is returned; the encoder starts over on `writer` with the same options"""
        L = load()
        p = C.POINTER(C.c_uint8)()
        n = C.c_size_t(0)
        rc = L.mi355_deflate_stream_reset(self._s, C.byref(p), C.byref(n))
        if rc != OK:
            raise DeflateError(rc, L.mi355_deflate_last_error(self._ctx._h).decode())
        rest = C.string_at(p, n.value) if n.value else b""
        while rest:
            took = self._w.write(rest)
            took = len(rest) if took is None else int(took)
            if took <= 0:
                raise IOError("inner writer accepted no bytes (io::ErrorKind::WriteZero)")
            rest = rest[took:]
        old, self._w = self._w, writer
        return old

    def close(self):
        """Drop (writer.rs:139-152): an encoder that goes away unfinished finishes its stream; errors are
        swallowed, as Drop must"""
        if getattr(self, "_s", None) and not getattr(self, "_done", False):
            try:
                self.finish()
            except Exception:
                pass

    def checksum(self):
        """{Zlib,Gz}Encoder::checksum() (writer.rs:248-250, :428-430)"""
        a = C.c_uint32(0)
        rc = load().mi355_deflate_stream_checksum(self._s, C.byref(a))
        if rc != OK:
            raise DeflateError(rc, "stream_checksum")
        return a.value

    def __del__(self):
        if getattr(self, "_s", None):
            try:
                self.close()
                load().mi355_deflate_stream_free(self._s)
            except Exception:
                pass
            self._s = None


class DeflateEncoder(_Encoder):
    """write::DeflateEncoder (src/writer.rs:89-152)"""
    _wrapper = 0


class ZlibEncoder(_Encoder):
    """write::ZlibEncoder (src/writer.rs:183-290)"""
    _wrapper = 1


class GzEncoder(_Encoder):
    """write::gzip::GzEncoder (src/writer.rs:293-467, feature "gzip")"""
    _wrapper = 2

    @classmethod
    def from_builder(cls, header, writer, options=Compression.Default, ctx=None):
        """from_builder(builder, writer, options) (:346-358); header = builder.into_header() bytes"""
        e = cls(writer, options, ctx)
        e.set_header(header)
        return e

    def set_header(self, header):
        header = bytes(header)
        rc = load().mi355_deflate_stream_gzip_header(self._s, header, len(header))
        if rc != OK:
            raise DeflateError(rc, "stream_gzip_header")

    def reset_with_builder(self, writer, header):
        """reset_with_builder (:393-402)"""
        old = self.reset(writer)
        self.set_header(header)
        return old


# ---- sharded, stream-exact encode: the per-rank phases (mi355_shard_*) -------------------------------
ZONE = 576
BLOCK_TOKENS = 31744


class MultiGpu:
    """mi355_multi: one input over several GPUs of this node in one call (one process, a thread per device); the
    stream is the one a single encoder produces for the whole input.  devices: HIP device per rank (a device may be
    named more than once: the ranks then share it)."""
    TRACE = ["tables", "wait1", "tokens", "wait2", "block costs", "wait3", "plan+pack+copy", "wait4", "seams+framing",
             "host work of the exchanges", "call"]

    def __init__(self, devices=None):
        """devices=None: every device of the node"""
        h = C.c_void_p()
        if devices is None:
            rc = load().mi355_multi_create(None, 0, C.byref(h))
            devices = list(range(load().mi355_device_count()))
        else:
            arr = (C.c_int * len(devices))(*devices)
            rc = load().mi355_multi_create(arr, len(devices), C.byref(h))
        if rc != OK:
            raise DeflateError(rc, "cannot create contexts on HIP devices %r" % (list(devices),))
        self._h = h
        self.devices = list(devices)

    def close(self):
        if getattr(self, "_h", None):
            load().mi355_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _err(self, rc):
        raise DeflateError(rc, load().mi355_multi_last_error(self._h).decode())

    def config(self, key, value):
        """mi355_deflate_ctx_config of rank 0's context (CFG_RANGE_BYTES: twice that is the most one rank takes)"""
        rc = load().mi355_deflate_ctx_config(C.c_void_p(load().mi355_multi_ctx(self._h, 0)), key, value)
        if rc != OK:
            self._err(rc)

    def layout(self, in_len, rank):
        """-> dict(n_ranks, g_lo, g_hi, lo, hi): the bytes rank `rank` holds and owns"""
        n = C.c_int(0)
        v = [C.c_uint64(0) for _ in range(4)]
        rc = load().mi355_multi_layout(self._h, in_len, rank, C.byref(n), *[C.byref(x) for x in v])
        if rc != OK:
            self._err(rc)
        return dict(n_ranks=n.value, g_lo=v[0].value, g_hi=v[1].value, lo=v[2].value, hi=v[3].value)

    def encode(self, data, options=Compression.Default, wrapper=0, compat=0, gzip_header=None):
        """deflate_bytes_conf / _zlib_conf / _gzip_conf over all devices: bytes in, bytes out"""
        data = bytes(data) if not isinstance(data, bytes) else data
        o = CompressionOptions.from_(options).to_c(wrapper, compat, FLUSH_FINISH)
        hdr = bytes(gzip_header) if gzip_header is not None else None
        cap = load().mi355_deflate_bound_ex(len(data), wrapper, len(hdr) if hdr else 10, 0) + 8
        out = (C.c_uint8 * cap)()
        n = C.c_size_t(0)
        rc = load().mi355_deflate_encode_multi(self._h, data, len(data), C.byref(o), hdr, len(hdr) if hdr else 0, out, cap, C.byref(n))
        if rc != OK:
            self._err(rc)
        return bytes(memoryview(out)[: n.value])

    def encode_host_ptr(self, in_ptr, n, out_ptr, out_cap, options=Compression.Default, wrapper=0):
        o = CompressionOptions.from_(options).to_c(wrapper, 0, FLUSH_FINISH)
        got = C.c_size_t(0)
        rc = load().mi355_deflate_encode_multi(self._h, C.cast(C.c_void_p(in_ptr), C.c_char_p), n, C.byref(o), None, 0,
                                               C.cast(C.c_void_p(out_ptr), C.POINTER(C.c_uint8)), out_cap, C.byref(got))
        if rc != OK:
            self._err(rc)
        return got.value

    def encode_device(self, d_ext_ptrs, in_len, d_out_ptr, out_cap, options=Compression.Default, wrapper=0, compat=0,
                      gzip_header=None):
        """d_ext_ptrs[r] = device pointer (on rank r's device) to the bytes layout(in_len, r) names; d_out on rank 0's"""
        o = CompressionOptions.from_(options).to_c(wrapper, compat, FLUSH_FINISH)
        hdr = bytes(gzip_header) if gzip_header is not None else None
        arr = (C.c_void_p * len(d_ext_ptrs))(*[C.c_void_p(p) for p in d_ext_ptrs])
        n = C.c_size_t(0)
        rc = load().mi355_deflate_encode_multi_device(self._h, arr, in_len, C.byref(o), hdr, len(hdr) if hdr else 0,
                                                      C.c_void_p(d_out_ptr), out_cap, C.byref(n))
        if rc != OK:
            self._err(rc)
        return n.value

    def stitch_info(self):
        """how the packed ranges of the last call reached rank 0 ("rccl" / "peer"), and the ranks RCCL reports (0: no communicator)"""
        a, b = C.c_int(0), C.c_int(0)
        load().mi355_multi_stitch_info(self._h, C.byref(a), C.byref(b))
        return {"stitch": "rccl" if a.value else "peer", "rccl_ranks": b.value}

    def trace(self):
        t = (C.c_double * 11)()
        load().mi355_multi_last_trace(self._h, t, 11)
        return dict(zip(self.TRACE, [round(x, 4) for x in t]))

    def rank_info(self, rank):
        info = Info()
        load().mi355_deflate_last_info(C.c_void_p(load().mi355_multi_ctx(self._h, rank)), C.byref(info))
        return {"match_ms": info.match_ms, "match_launches": info.match_launches}


class Shard:
    """One rank's session of the sharded (P1) encode; see include/mi355_deflate.h."""

    def __init__(self, ctx, d_ext_ptr, n_ext, parse_lo, parse_hi, global_lo, n_global, options=Compression.Default,
                 compat=0, stream=0):
        self.ctx = ctx
        o = CompressionOptions.from_(options).to_c(0, compat, 0)
        h = C.c_void_p()
        rc = load().mi355_shard_begin(ctx._h, C.c_void_p(d_ext_ptr), n_ext, parse_lo, parse_hi, global_lo, n_global,
                                      C.byref(o), C.c_void_p(stream), C.byref(h))
        if rc != OK:
            ctx._err(rc)
        self._h = h
        self.compat = compat
        self.nb = 0

    def spec(self):
        """-> (held, entry, exit) of the range's speculative parse (buffer coordinates)"""
        h, e, x = C.c_int(0), C.c_uint64(0), C.c_uint64(0)
        rc = load().mi355_shard_spec(self._h, C.byref(h), C.byref(e), C.byref(x))
        if rc != OK:
            self.ctx._err(rc)
        return bool(h.value), e.value, x.value

    def exit_table(self):
        t = (C.c_uint32 * ZONE)()
        rc = load().mi355_shard_exit_table(self._h, t)
        if rc != OK:
            self.ctx._err(rc)
        return list(t)

    def emit(self, entry):
        """-> (token count, device pointer of the dense token array)"""
        n = C.c_uint64(0)
        p = C.c_void_p()
        rc = load().mi355_shard_emit(self._h, entry, C.byref(n), C.byref(p))
        if rc != OK:
            self.ctx._err(rc)
        return n.value, (p.value or 0)

    def _blocks_call(self, skip, d_tail_ptr, n_tail, owns_final, nb, costs, cap):
        if owns_final is None:  # "the last rank owns the last block" (every range reaches its next block boundary)
            return load().mi355_shard_blocks(self._h, skip, C.c_void_p(d_tail_ptr), n_tail, C.byref(nb), costs, cap)
        return load().mi355_shard_blocks_ex(self._h, skip, C.c_void_p(d_tail_ptr), n_tail, 1 if owns_final else 0,
                                            C.byref(nb), costs, cap)

    def blocks(self, skip, d_tail_ptr, n_tail, owns_final=None):
        """-> list of cost tuples (dyn_bits, dyn_est, static_est, fixed_bits, in_bytes, q13)"""
        n, costs = self.blocks_raw(skip, d_tail_ptr, n_tail, owns_final)
        return [(c.dyn_bits, c.dyn_est, c.static_est, c.fixed_bits, c.in_bytes, c.q13) for c in costs[:n]]

    def blocks_raw(self, skip, d_tail_ptr, n_tail, owns_final=None):
        """-> (number of blocks, ctypes array of BlockCost): no per-block Python work (the distributed driver)"""
        nb = C.c_uint64(0)
        cap = 1 << 14
        costs = (BlockCost * cap)()
        rc = self._blocks_call(skip, d_tail_ptr, n_tail, owns_final, nb, costs, cap)
        if rc != OK:
            self.ctx._err(rc)
        if nb.value > cap:
            costs = (BlockCost * nb.value)()
            rc = self._blocks_call(skip, d_tail_ptr, n_tail, owns_final, nb, costs, nb.value)
            if rc != OK:
                self.ctx._err(rc)
        self.nb = nb.value
        return nb.value, costs

    def pack_raw(self, plans_arr, first, end_bit, d_out_ptr, out_cap):
        """plans_arr: ctypes array of BlockInfo for the whole stream, `first` = index of this rank's first block"""
        fb = C.c_uint64(0)
        nbts = C.c_size_t(0)
        ptr = C.cast(C.byref(plans_arr, first * C.sizeof(BlockInfo)), C.POINTER(BlockInfo))
        rc = load().mi355_shard_pack(self._h, ptr, end_bit, C.c_void_p(d_out_ptr), out_cap, C.byref(fb), C.byref(nbts))
        if rc != OK:
            self.ctx._err(rc)
        return fb.value, nbts.value

    def pack(self, plans, end_bit, d_out_ptr, out_cap):
        """plans: list of (btype, bfinal, bit_start) of this rank's blocks -> (first_byte, n_bytes)"""
        arr = (BlockInfo * max(1, len(plans)))()
        for i, (bt, bf, bs) in enumerate(plans):
            arr[i].btype, arr[i].bfinal, arr[i].bit_start = bt, bf, bs
        fb = C.c_uint64(0)
        nbts = C.c_size_t(0)
        rc = load().mi355_shard_pack(self._h, arr, end_bit, C.c_void_p(d_out_ptr), out_cap, C.byref(fb), C.byref(nbts))
        if rc != OK:
            self.ctx._err(rc)
        return fb.value, nbts.value

    def close(self):
        if getattr(self, "_h", None):
            load().mi355_shard_end(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def plan_blocks_raw(costs_arr, n, compat=0):
    """plan_blocks over a ctypes array of BlockCost -> (ctypes array of BlockInfo, total_bits)"""
    out = (BlockInfo * max(1, n))()
    tot = C.c_uint64(0)
    rc = load().mi355_plan_blocks(costs_arr, n, compat, out, C.byref(tot))
    if rc != OK:
        raise DeflateError(rc, "mi355_plan_blocks")
    return out, tot.value


def plan_blocks(costs, compat=0):
    """The serial block plan over the costs of ALL blocks of the stream (host; identical on every rank).
    -> (list of (btype, bfinal, bit_start), total_bits)"""
    n = len(costs)
    arr = (BlockCost * max(1, n))()
    for i, c in enumerate(costs):
        (arr[i].dyn_bits, arr[i].dyn_est, arr[i].static_est, arr[i].fixed_bits, arr[i].in_bytes, arr[i].q13) = c
    out = (BlockInfo * max(1, n))()
    tot = C.c_uint64(0)
    rc = load().mi355_plan_blocks(arr, n, compat, out, C.byref(tot))
    if rc != OK:
        raise DeflateError(rc, "mi355_plan_blocks")
    return [(o.btype, o.bfinal, o.bit_start) for o in out[:n]], tot.value
