"""What hdlz_compress_batch_bits + hdlz_join_batch_ws must answer (a helper module like checked_ref.py, not a conftest): the joined
stream of include/hdlz_join.h built from the CPU oracle's per-block streams and stock zlib only -- never from device output.

The end bit of a block is found by walking the fixed-Huffman codes of the oracle's stream (RFC 1951 3.2.6) up to the end-of-block
code; the sync marker follows from the pad bits, and the marker that the rule does NOT pick is shown not to decode."""
import zlib

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
MARKERS = {4: b"\x00\x00\xff\xff", 5: b"\x00\x00\x00\xff\xff"}
_cache = {}


def end_bit(z):
    """z: a zlib stream of ONE final fixed-Huffman block -> the bit index, from the stream's first bit, of the first bit of its
    end-of-block code"""
    assert z[:2] == b"\x78\x9c"
    assert z[2] & 7 == 3, "BFINAL = 1, BTYPE = 01"
    pos = 19

    def code(n):                 # Huffman codes are packed most significant bit first
        nonlocal pos
        c = 0
        for _ in range(n):
            c = (c << 1) | ((z[pos >> 3] >> (pos & 7)) & 1)
            pos += 1
        return c

    while True:
        start = pos
        c = code(7)
        if c <= 0b0010111:
            sym = 256 + c
        else:
            c = (c << 1) | code(1)
            if 0b00110000 <= c <= 0b10111111:
                sym = c - 0b00110000
            elif 0b11000000 <= c <= 0b11000111:
                sym = 280 + c - 0b11000000
            else:
                c = (c << 1) | code(1)
                assert 0b110010000 <= c <= 0b111111111
                sym = 144 + c - 0b110010000
        if sym == 256:
            return start
        if sym > 256:
            assert sym <= 285
            pos += LEN_EXTRA[sym - 257]
            d = code(5)
            assert d < 30
            pos += DIST_EXTRA[d]
        assert pos <= 8 * (len(z) - 4)


def member_of(blk, cwindow, maxmatch):
    """-> (the oracle's stream R, E, p, the member M) of one block"""
    key = (blk, cwindow, maxmatch)
    if key in _cache:
        return _cache[key]
    from oracle import oracle as O
    rc, z = O.compress(blk, cwindow, maxmatch)
    assert rc == 0, rc
    E = end_bit(z)
    nbytes = len(z) - 4
    assert E >= 19 and nbytes == (E + 14) >> 3
    p = 8 * nbytes - E - 7
    assert 0 <= p <= 7
    body = bytes([z[2] & 0xFE]) + z[3:nbytes]
    pick = 4 if p >= 3 else 5

    def decodes(marker):
        d = zlib.decompressobj(-15)
        try:
            return d.decompress(body + marker + b"\x03\x00") == blk and d.eof and d.unused_data == b""
        except zlib.error:
            return False
    assert decodes(MARKERS[pick]) and not decodes(MARKERS[9 - pick]), (len(blk), p)
    _cache[key] = (z, E, p, body + MARKERS[pick])
    return _cache[key]


class Joined(object):
    """stream: the contract's bytes; rows / end_bits / pads / members per block; offsets[b] = where member b starts, offsets[B] = where
    03 00 starts; adler = zlib.adler32 of the concatenated input"""


def expected_joined(blocks, cwindow, maxmatch):
    j = Joined()
    parts = [member_of(bytes(b), cwindow, maxmatch) for b in blocks]
    j.rows = [q[0] for q in parts]
    j.end_bits = [q[1] for q in parts]
    j.pads = [q[2] for q in parts]
    j.members = [q[3] for q in parts]
    j.offsets = [2]
    for m in j.members:
        j.offsets.append(j.offsets[-1] + len(m))
    j.data = b"".join(bytes(b) for b in blocks)
    j.adler = zlib.adler32(j.data)
    j.stream = b"\x78\x9c" + b"".join(j.members) + b"\x03\x00" + j.adler.to_bytes(4, "big")
    assert len(j.stream) == j.offsets[-1] + 6
    return j
