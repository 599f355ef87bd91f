"""ic_match_token (deflate-rs_amd/csrc/inflate_check.h), the one copy of the arithmetic from a length symbol to a checked
(len, dist) that verify, inflate and the tabled inflate share, called directly through the host build of tests/inflcheck.  The
expected values come from the tables of RFC 1951 3.2.5 as written out below: nothing is taken from zlib or from the code under
test.  CPU only."""
import inflcheck_binding as ib

# RFC 1951 3.2.5: (extra bits, first length) of the length symbols 257..285; (extra bits, first distance) of the distance symbols 0..29
LENGTHS = [(0, 3), (0, 4), (0, 5), (0, 6), (0, 7), (0, 8), (0, 9), (0, 10), (1, 11), (1, 13), (1, 15), (1, 17), (2, 19), (2, 23),
           (2, 27), (2, 31), (3, 35), (3, 43), (3, 51), (3, 59), (4, 67), (4, 83), (4, 99), (4, 115), (5, 131), (5, 163), (5, 195),
           (5, 227), (0, 258)]
DISTS = [(0, 1), (0, 2), (0, 3), (0, 4), (1, 5), (1, 7), (2, 9), (2, 13), (3, 17), (3, 25), (4, 33), (4, 49), (5, 65), (5, 97),
         (6, 129), (6, 193), (7, 257), (7, 385), (8, 513), (8, 769), (9, 1025), (9, 1537), (10, 2049), (10, 3073), (11, 4097),
         (11, 6145), (12, 8193), (12, 12289), (13, 16385), (13, 24577)]
assert len(LENGTHS) == 29 and len(DISTS) == 30

FIXED = [5] * 32               # the fixed distance code: symbol d is the 5-bit code d
ONE = [1] + [0] * 31           # one code, '0' = symbol 0; the bit 1 is no code and no longer code exists
ONE_AND_15 = [1, 15] + [0] * 30  # incomplete: '0' = symbol 0, '1' + 14 zeros = symbol 1; 11... is no code
WIDEST = [1] + [0] * 28 + [15, 0, 0]  # '0' = symbol 0, '1' + 14 zeros = symbol 29 (13 extra bits)
LCODE = 7                      # the bits of the length symbol's own code in these tokens (any value 1..15 does)
FAR = 32768                    # an output position no distance is larger than


def token(fields, fill=1, lcode=LCODE):
    """fields: (value, bits, msb_first) in stream order behind the length symbol's code.  A Huffman code is packed most
    significant bit first, extra bits least significant first (RFC 1951 3.1.1).  Returns (w, bits of the whole token); the bits
    of the length code and everything behind the token are `fill`, which the function must not look at."""
    bits = [fill] * lcode
    for value, n, msb_first in fields:
        assert 0 <= value < (1 << n) or n == 0 and value == 0
        order = range(n - 1, -1, -1) if msb_first else range(n)
        bits += [(value >> i) & 1 for i in order]
    n = len(bits)
    bits += [fill] * (64 - n)
    return sum(b << i for i, b in enumerate(bits)), n


def fixed_token(ls, lx, ds, dx, fill=1):
    """length symbol ls with extra value lx, the fixed 5-bit code of distance symbol ds, extra value dx"""
    return token([(lx, LENGTHS[ls - 257][0], False), (ds, 5, True), (dx, DISTS[ds][0] if ds < 30 else 0, False)], fill)


def test_every_length_with_every_distance_under_the_fixed_code():
    n = 0
    for ls in range(257, 286):
        eb, l0 = LENGTHS[ls - 257]
        for lx in (0, (1 << eb) - 1):
            for ds in range(30):
                de, d0 = DISTS[ds]
                for dx in (0, (1 << de) - 1):
                    w, bits = fixed_token(ls, lx, ds, dx, fill=(n & 1))
                    assert bits == LCODE + eb + 5 + de
                    got = ib.match_token(FIXED, w, ls, LCODE, bits, FAR)  # (avail: not a bit more than the token)
                    assert got == ("OK", l0 + lx, d0 + dx, bits), (ls, lx, ds, dx, got)
                    n += 1
    assert n == 3480


def test_distance_symbols_30_and_31_are_no_symbols():
    for ds in (30, 31):
        for ls in (257, 265, 284):  # 0, 1 and 5 extra bits in front of the distance code
            w, bits = fixed_token(ls, 0, ds, 0)
            assert bits == LCODE + LENGTHS[ls - 257][0] + 5
            for avail in (bits, bits + 1, 64, 1 << 40):
                assert ib.match_token(FIXED, w, ls, LCODE, avail, FAR)[0] == "CODE", (ds, ls, avail)
            for avail in range(bits):  # the stream ends inside the code, or in front of it
                assert ib.match_token(FIXED, w, ls, LCODE, avail, FAR)[0] == "TRUNCATED", (ds, ls, avail)


def test_a_token_that_ends_behind_the_stream_is_truncated():
    """one token of each extra-bit width: every avail below its bit count is TRUNCATED, the count itself is OK"""
    tokens = [(257 + k, 0) for k in (0, 8, 12, 16, 20, 24)] + [(257, ds) for ds in range(2, 30, 2)]
    assert sorted(LENGTHS[ls - 257][0] for ls, ds in tokens if ds == 0) == [0, 1, 2, 3, 4, 5]
    assert sorted(DISTS[ds][0] for ls, ds in tokens if ls == 257)[1:] == list(range(14))
    for ls, ds in tokens:
        for ones in (0, 1):
            eb, de = LENGTHS[ls - 257][0], DISTS[ds][0]
            lx, dx = ones * ((1 << eb) - 1), ones * ((1 << de) - 1)
            w, bits = fixed_token(ls, lx, ds, dx, fill=ones)
            for avail in range(bits):
                assert ib.match_token(FIXED, w, ls, LCODE, avail, FAR)[0] == "TRUNCATED", (ls, ds, avail)
            assert ib.match_token(FIXED, w, ls, LCODE, bits, FAR) == ("OK", LENGTHS[ls - 257][1] + lx, DISTS[ds][1] + dx, bits)


def test_a_distance_reaches_the_first_byte_and_no_further():
    for ds in range(30):
        de, d0 = DISTS[ds]
        for dx in (0, (1 << de) - 1):
            dist = d0 + dx
            w, bits = fixed_token(258, 0, ds, dx)
            assert ib.match_token(FIXED, w, 258, LCODE, 64, dist - 1)[0] == "DISTANCE", dist
            assert ib.match_token(FIXED, w, 258, LCODE, 64, dist) == ("OK", 4, dist, bits), dist
            assert ib.match_token(FIXED, w, 258, LCODE, 64, 1 << 40) == ("OK", 4, dist, bits), dist


def test_the_window_edge():
    w, bits = fixed_token(285, 0, 29, 8191)
    assert DISTS[29][1] + 8191 == 32768
    assert ib.match_token(FIXED, w, 285, LCODE, 64, 32768) == ("OK", 258, 32768, bits)
    assert ib.match_token(FIXED, w, 285, LCODE, 64, 32767)[0] == "DISTANCE"


def test_the_widest_token_is_48_bits():
    """a 15-bit length code, 5 extra bits, a 15-bit distance code, 13 extra bits"""
    w, bits = token([(31, 5, False), (1 << 14, 15, True), (8191, 13, False)], fill=0, lcode=15)
    assert bits == 48
    assert ib.match_token(WIDEST, w, 284, 15, 48, FAR) == ("OK", 258, 32768, 48)
    assert ib.match_token(WIDEST, w, 284, 15, 47, FAR)[0] == "TRUNCATED"


def test_no_code_under_a_one_code_distance_set():
    """the bit 1 is no code.  With a bit or more of it inside the stream no longer code exists (the set's only code has one bit):
    CODE, whether 15 bits are left behind the length or not.  With no bit left, a code of one bit is a longer one: TRUNCATED."""
    for ls in (257, 273):
        eb = LENGTHS[ls - 257][0]
        w, _ = token([(0, eb, False), (1, 1, True)], fill=1)
        for left in list(range(1, 15)) + [15, 16, 40]:
            assert ib.match_token(ONE, w, ls, LCODE, LCODE + eb + left, FAR)[0] == "CODE", (ls, left)
        for avail in range(LCODE + eb + 1):
            assert ib.match_token(ONE, w, ls, LCODE, avail, FAR)[0] == "TRUNCATED", (ls, avail)
        w, bits = token([(0, eb, False), (0, 1, True)], fill=1)  # (the set's code itself)
        assert ib.match_token(ONE, w, ls, LCODE, bits, FAR) == ("OK", LENGTHS[ls - 257][1], 1, bits)


def test_no_code_where_a_longer_code_exists():
    """'0' and a 15-bit code: 11... is no code, and with fewer than 15 bits left more bits could have made one"""
    for ls in (257, 273):
        eb = LENGTHS[ls - 257][0]
        w, _ = token([(0, eb, False), (3, 2, True)], fill=1)
        for left in range(15):
            assert ib.match_token(ONE_AND_15, w, ls, LCODE, LCODE + eb + left, FAR)[0] == "TRUNCATED", (ls, left)
        for left in (15, 16, 40):
            assert ib.match_token(ONE_AND_15, w, ls, LCODE, LCODE + eb + left, FAR)[0] == "CODE", (ls, left)
        w, bits = token([(0, eb, False), (1 << 14, 15, True)], fill=1)  # (the 15-bit code itself: symbol 1, distance 2)
        assert ib.match_token(ONE_AND_15, w, ls, LCODE, bits, FAR) == ("OK", LENGTHS[ls - 257][1], 2, bits)
