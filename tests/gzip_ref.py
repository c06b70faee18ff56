"""What the gzip form of the joined stream must answer (include/hdlz_gzip.h; a helper module like joined_ref.py, not a conftest):
the stream built from joined_ref.expected_joined by swapping header and trailer, and the CRC-32 combination rule of
hdl_deflate_amd/csrc/hdlz_crc32.h stated in pure Python -- never from device output."""
import zlib

import joined_ref

GZIP_HEADER = bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 0xFF])
POLY = 0xEDB88320
ONE = 0x80000000                  # x^0: bit 31 of a word is x^0, bit 0 is x^31
INIT = 0xFFFFFFFF
TILE = 32768
FIN_THREADS = 1024


class Gzip(object):
    """stream: the contract's bytes; offsets[b] = where member b starts (offsets[0] = 10), offsets[B] = where 03 00 starts; members,
    rows, end_bits, data as in joined_ref.Joined; crc = zlib.crc32 of the concatenated input; zlib_form: the Joined it was made from"""


def expected_gzip(blocks, cwindow, maxmatch):
    j = joined_ref.expected_joined(blocks, cwindow, maxmatch)
    g = Gzip()
    g.zlib_form = j
    g.rows, g.end_bits, g.pads, g.members, g.data = j.rows, j.end_bits, j.pads, j.members, j.data
    g.offsets = [o + 8 for o in j.offsets]
    g.crc = zlib.crc32(j.data)
    assert j.stream[:2] == b"\x78\x9c" and j.stream[-6:-4] == b"\x03\x00"
    g.stream = GZIP_HEADER + j.stream[2:-4] + g.crc.to_bytes(4, "little") + (len(j.data) & 0xFFFFFFFF).to_bytes(4, "little")
    assert len(g.stream) == len(j.stream) + 12 == g.offsets[-1] + 10
    return g


# ---- the arithmetic of hdlz_crc32.h
def mul(a, b):
    """a * b mod P (zlib's multmodp)"""
    p = 0
    for i in range(31, -1, -1):
        if (a >> i) & 1:
            p ^= b
        b = (b >> 1) ^ (POLY if b & 1 else 0)
    return p


XP2 = [ONE >> 1]
for _k in range(31):
    XP2.append(mul(XP2[-1], XP2[-1]))


def xpow(e):
    r, k = ONE, 0
    while e:
        if e & 1:
            r = mul(r, XP2[k & 31])
        e >>= 1
        k += 1
    return r


def raw(data):
    """the register after `data` from a register of 0, no final xor"""
    return zlib.crc32(data, 0xFFFFFFFF) ^ 0xFFFFFFFF


def tree(vals, first_level):
    """vals[i] for i = 0 .. 2^m - 1 -> xor_i vals[i] * x^(2^first_level * i), level k multiplying the FARTHER neighbour by XP2[first_level + k]"""
    vals = list(vals)
    k = 0
    while (1 << k) < len(vals):
        for i in range(0, len(vals), 2 << k):
            vals[i] ^= mul(vals[i + (1 << k)], XP2[(first_level + k) & 31])
        k += 1
    return vals[0]


def tile_word(tile):
    """a tile of up to 32768 bytes -> its word, as a workgroup computes it: 256 strips of 128 bytes, zeros behind a short tile;
    the EARLIER neighbour is multiplied (in a tile the strips are numbered from the front), so the tree runs over the reversed list"""
    tile = tile + bytes(TILE - len(tile))
    strips = [raw(tile[128 * t:128 * t + 128]) for t in range(256)]
    waves = [tree(strips[64 * w:64 * w + 64][::-1], 10) for w in range(4)]
    return tree(waves[::-1], 16)


def crc32_from_words(words, n):
    """the finishing workgroup: the words numbered from the END, the initial register as one more word in front, 1024 Horner chains with
    a stride of 1024 words, the tree over the chains, the padding of the last tile taken back"""
    ntiles = len(words)
    assert ntiles == (n + TILE - 1) // TILE
    w = list(reversed(words)) + [INIT]                    # w[j], j = 0 .. ntiles
    chains = []
    for i in range(FIN_THREADS):
        v = 0
        for j in range(i + (ntiles - i) // FIN_THREADS * FIN_THREADS, -1, -FIN_THREADS) if i <= ntiles else ():
            v = mul(v, XP2[28]) ^ w[j]
        chains.append(v)
    R = tree(chains, 18)
    pad = ntiles * TILE - n
    return mul(R, xpow(0xFFFFFFFF - 8 * pad)) ^ INIT


def crc32_by_rule(data, word_of=tile_word):
    return crc32_from_words([word_of(data[o:o + TILE]) for o in range(0, len(data), TILE)], len(data))
