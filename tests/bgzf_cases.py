"""Cases for the BGZF encode (include/mi355_deflate.h mi355_bgzf_encode[_device]): the model of the file and the inputs, shared by the
CPU test of the model (test_bgzf_cases.py) and the GPU test (test_bgzf_gpu.py).  TEST INFRASTRUCTURE.

The model is the header's definition run on the oracle: member k = oracle_binding.encode_gzip(slice k, H) with bytes 16..17 replaced
by len - 1, the members in slice order with no byte between them, the end-of-file marker last.  model(data, level, B) gives (file,
members), members = the rows of mi355_member_info as dicts.

A case is Case(name, data, level, block, batch_bytes): block as the call takes it (0 = 65280); batch_bytes = MI355_CFG_BATCH_BYTES for
the call, None = the default.

  edge()        in_len 0, 1, B - 1, B, B + 1 at B = 65280 (in_len 1: one slice of one byte, a member of 29 bytes, a file of 57)
  three()       3 * 65280 + 1 bytes of text at B = 0, every preset
  small()       100 000 bytes of text at B = 64: 1563 members of 60 to 91 bytes, more than one round of the scan
  interleaved() eight slices of 65280 bytes: text, noise, zeros, text, twice -- the one-input path (noise fires Q1, zeros fail the
                speculative parse) between slices of the batched kernels: the case that catches order
  sets()        3 MiB of text with MI355_CFG_BATCH_BYTES at 1 MiB: the packed batch cuts its launch sets (four: an item counts with
                its header, so sixteen slices fit the MiB and the forty-ninth is a set of its own)
  noise()       two slices of noise at B = 65280, every preset: the longest members there are
"""
import collections
import functools
import struct
import zlib

import datagen
import oracle_binding as ob

Case = collections.namedtuple("Case", "name data level block batch_bytes")

H = bytes.fromhex("1f8b08040000000000ff0600424302000000")
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
BLOCK_MAX = 65280
MEMBER_MAX = 65536  # what BSIZE can express
HINTED = 1
# name -> (the oracle's preset, (max_hash_checks, lazy_if_less_than, matching_type))
LEVELS = collections.OrderedDict([("fast", (ob.FAST, (1, 0, 0))), ("default", (ob.DEFAULT, (128, 32, 1))), ("best", (ob.BEST, (1768, 128, 1))),
                                  ("rle", (ob.RLE, (0, 0, 1))), ("huffman_only", (ob.HUFFMAN_ONLY, (0, 0, 0)))])


def slices(data, block):
    b = block or BLOCK_MAX
    return [data[o: o + b] for o in range(0, len(data), b)]


def patch(member):
    """the member with BSIZE = its length - 1 in bytes 16..17"""
    assert member[:16] == H[:16] and len(member) <= MEMBER_MAX
    return member[:16] + struct.pack("<H", len(member) - 1) + member[18:]


def rows_of(parts, lens):
    """the member table of a file of `parts`, the marker last; lens = the slices' lengths"""
    rows, o, p = [], 0, 0
    for m, n in zip(parts, list(lens) + [0]):
        rows.append(dict(in_off=o, in_len=len(m), out_off=p, out_len=n, flags=HINTED, status="OK"))
        o += len(m)
        p += n
    return rows


@functools.lru_cache(maxsize=None)
def model_parts(data, level, block):
    """the members of the file, patched, the marker last"""
    return tuple(patch(ob.encode_gzip(s, H, level=LEVELS[level][0])) for s in slices(data, block)) + (EOF,)


def model(data, level, block):
    """(file, members) as the header defines them, from the oracle"""
    parts = model_parts(bytes(data), level, block)
    return b"".join(parts), rows_of(parts, [len(s) for s in slices(data, block)])


@functools.lru_cache(maxsize=None)
def _text(n, seed):
    return datagen.text_like(n, seed)


@functools.lru_cache(maxsize=None)
def _noise(n, seed):
    return datagen.rng_bytes(n, seed)


def edge():
    t = _text(BLOCK_MAX + 1, 41)
    return [Case("edge-%d" % n, t[:n], "default", 0, None) for n in (0, 1, BLOCK_MAX - 1, BLOCK_MAX, BLOCK_MAX + 1)]


def three():
    t = _text(3 * BLOCK_MAX + 1, 42)
    return [Case("three-%s" % lv, t, lv, 0, None) for lv in LEVELS]


def small():
    return [Case("small-64", _text(100000, 43), "default", 64, None)]


def interleaved():
    kinds = [_text(BLOCK_MAX, 44), _noise(BLOCK_MAX, 45), bytes(BLOCK_MAX), _text(BLOCK_MAX, 46)]
    return [Case("interleaved", b"".join(kinds + kinds), "default", BLOCK_MAX, None)]


def sets():
    return [Case("sets-3MiB", _text(3 << 20, 47), "default", 0, 1 << 20)]


def noise():
    d = _noise(2 * BLOCK_MAX, 48)
    return [Case("noise-%s" % lv, d, lv, BLOCK_MAX, None) for lv in LEVELS]


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(edge() + three() + small() + interleaved() + sets() + noise())


def walk(file):
    """The file walked by its BSIZEs: [(offset, length)] of its members.  Raises AssertionError where a member does not begin with BGZF's
    header, runs past the file, or is not exactly one gzip member."""
    out, o = [], 0
    assert len(file) >= len(EOF)
    while o < len(file):
        assert file[o: o + 16] == H[:16], "no BGZF header at %d" % o
        n = struct.unpack_from("<H", file, o + 16)[0] + 1
        assert o + n <= len(file), "the member at %d runs past the file" % o
        d = zlib.decompressobj(31)
        try:
            d.decompress(file[o: o + n])
        except zlib.error as e:
            raise AssertionError("the member at %d: %s" % (o, e))
        assert d.eof and not d.unused_data, "BSIZE at %d is not the member's size" % o
        out.append((o, n))
        o += n
    return out


def check_file(file, members, data, block):
    """What a BGZF file of `data` must satisfy, whoever made it: gzip reads it, every BSIZE is true, the marker is last, the members are
    the slices in order and the table says so"""
    import gzip
    assert gzip.decompress(file) == data
    got = walk(file)
    assert file[got[-1][0]:] == EOF
    sl = slices(data, block)
    assert len(got) == len(sl) + 1 == len(members)
    p = 0
    for (o, n), s, row in zip(got, sl + [b""], members):
        assert zlib.decompress(file[o: o + n], 31) == s
        assert row == dict(in_off=o, in_len=n, out_off=p, out_len=len(s), flags=HINTED, status="OK")
        p += len(s)


def gzi(members):
    """the .gzi index of `bgzip -i`: a count, then (compressed offset, uncompressed offset) of every data member but the first"""
    rows = [m for m in members if m["out_len"]][1:]
    return struct.pack("<Q", len(rows)) + b"".join(struct.pack("<QQ", m["in_off"], m["out_off"]) for m in rows)


def coverage(cases=None):
    """(member start residues mod 16, member length residues mod 16, the interior positions 1..15 at which some 16-byte granule of a
    file holds the last byte of one member and the first of the next) over the models of the cases"""
    starts, lens, seams = set(), set(), set()
    for c in cases or all_cases():
        _file, members = model(c.data, c.level, c.block)
        for m in members:
            starts.add(m["in_off"] % 16)
            lens.add(m["in_len"] % 16)
            if m["in_off"] and m["in_off"] % 16:
                seams.add(m["in_off"] % 16)
    return starts, lens, seams
