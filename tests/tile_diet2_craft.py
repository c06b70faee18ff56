"""Crafted inputs for the second diet of the one-tile compress kernel (k_compress<1, ., true, .>, hdlz_compress_common.h): the literal
emitter of match-free tiles (literal_codes), the distance planes updated per group of four distances (match_search_bits) and the plain
Adler sums of a one-tile block.  No GPU and no torch here: tests/test_tile_diet2_cpu.py holds every case against the oracle's tokens (an
input that does not show its token is a bug of this file), tests/test_gpu_tile_diet2.py compares the kernels with the oracle's bytes.

Cases, expectations and routes are those of tests/tile_diet_craft.py (Case, check); everything here takes the route "tile".  Fillers
hold no pair of neighbouring bytes twice, so no trigram repeats and nothing in them matches: a block cut from one is match-free at
every length -- the positions behind a short block's end are zero bytes, but the end cap of the search sets their mismatch bits, and the
oracle (which has no padding at all) gives literals only.  Whether the KERNEL takes its match-free arm for a short block cannot be read
from the oracle; the lengths below are right for either answer, and 2046 .. 2048 reach the arm whatever the cap does."""
import functools
import random

from tile_diet_craft import RUN, TILE, Case, filler, plant

LIT_SIZES = (5, 6, 31, 32, 33, 2046, 2047, 2048)
EDGE_BYTES = (143, 144, 0, 255)           # the last 8-bit literal, the first 9-bit one, and the two ends of the byte range
PAIRS_APART = ((4, 7), (28, 31))          # two candidates whose copies of the trigram do not overlap
PAIRS_NEXT = ((7, 8), (31, 32))           # neighbours: the sources overlap, a run of four of one byte
LENGTH_DISTS = (1, 2, 16, 31, 32)


def _tile(label, data, expect, cw=32, mm=10):
    return Case(label, bytes(data), cw, mm, "tile", tuple(expect))


# ------------------------------------------------------------------------------------------------ A: match-free tiles
def _mixed(r, n):
    """a filler over all bytes in which every byte lane m = 0 .. 3 (position mod 4) holds 143, 144, 0 and 255 somewhere -- as far as n
    allows; neighbours stay distinct and no pair of neighbours occurs twice"""
    b = filler(r, n, 1, 255)              # (0 and 255 occur only where they are put: no pair with them can repeat by accident)
    spots = [(8 * k + m + 16 * (k % 2), v) for k, v in enumerate(EDGE_BYTES) for m in range(4)]
    seen = set()
    for q, v in spots:
        q = q % n if n < 64 else q + 40
        while q in seen or q - 1 in seen or q + 1 in seen:
            q = (q + 4) % n
        if n >= 64 or len(seen) < n // 3:
            b[q] = v
            seen.add(q)
    return b


def _no_trigram_twice(b, reach=48):
    last = {}
    for p in range(len(b) - 2):
        g = bytes(b[p:p + 3])
        if g in last and p - last[g] <= reach:
            return False
        last[g] = p
    return True


@functools.lru_cache(maxsize=None)
def literal_tiles():
    """blocks without a 3-byte repeat: bytes all < 144 (8-bit codes), all >= 144 (288 bits per lane: the most a lane sums), both kinds
    mixed with 143, 144, 0 and 255 in every byte lane; every length of LIT_SIZES"""
    out = []
    for n in LIT_SIZES:
        r = random.Random(41000 + n)
        for name, b in (("low", filler(r, n, 0, 144)), ("high", filler(r, n, 144, 256)), ("mixed", _mixed(r, n))):
            assert _no_trigram_twice(b), (name, n)
            out.append(_tile("free %s n=%d" % (name, n), b, [("all_lit",)]))
    return out


@functools.lru_cache(maxsize=None)
def literal_tile_neighbours():
    """blocks one candidate away from a match-free tile: (a) the only "candidate" is the false history lane 0 takes from lane 63 -- the
    block's last bytes repeat its first three, d behind the end -- which the normal path must reject; (b) exactly one real candidate at
    the last eligible position n - 5 (and the same block with it one position later, where nothing is eligible)"""
    out = []
    for d in (3, 17, 32):
        r = random.Random(42000 + d)
        b = filler(r, TILE)
        b[TILE - d:TILE - d + 3] = b[0:3][:min(3, d)]
        out.append(_tile("false history d=%d" % d, b[:TILE], [("all_lit",)]))
    for n in (2048, 2047, 33):
        for d in (1, 5, 28):
            r = random.Random(43000 + 50 * n + d)
            b = filler(r, n)
            plant(b, n - 5, 3, d)
            out.append(_tile("last eligible n=%d d=%d" % (n, d), b, [("tok", n - 5, 3, d), ("nomatch", 0, n - 5)]))
            b = filler(r, n)
            if d >= 3:                                               # (d < 3 would be a run that starts a position earlier)
                plant(b, n - 4, 3, d)
                out.append(_tile("behind the last n=%d d=%d" % (n, d), b, [("all_lit",)]))
    return out


def alternating(G, rows=2, extra=7, every=509):
    """-> (blocks, kinds, long_ones) for a batch whose grid is G waves: wave w takes block k G + (w + k) mod G of row k (the moving
    column of the one-tile bit-search kernels).  The block of wave w in row k is match-free iff k + w is even (kinds[b] = True) and
    4-symbol text otherwise; short blocks of 48 .. 96 bytes, and for every `every`-th wave blocks of 2046 .. 2048 bytes.  The match-free
    ones come from a filler over bytes >= 128, so 8- and 9-bit codes mix"""
    r = random.Random(44000)
    free = bytes(filler(r, 8192, 128, 256))
    text = bytes(r.choice(b"acgt") for _ in range(8192))
    blocks, kinds, long_ones = [], [], []
    for b in range(rows * G + extra):
        k = b // G
        w = (b % G - k) % G
        lit = (k + w) % 2 == 0
        if w % every == 3:
            n = 2048 - (k + w // every) % 3
            long_ones.append(b)
        else:
            n = 48 + b % 49
        src = free if lit else text
        o = (b * 131) % (len(src) - n)
        blocks.append(src[o:o + n])
        kinds.append(lit)
    return blocks, kinds, long_ones


# ------------------------------------------------------------------------------------------------ B: distance planes by groups
def _planted_distance(d, cw):
    """one block, one distance: a three-byte match inside a lane (lane 5, local 10), on the lane seams (lane 9 local 30, lane 13 local
    31), in lane 0 at i = d (its source is the block's first bytes) and in lane 63 (local 5).  Lane 0 at i = d - 1 would need the byte
    in front of the block: what the search sees there is lane 63's last byte, so the trigram (last byte, b[0], b[1]) is put at i = d - 1
    in a block of its own (false_history_at) -- it must not match"""
    r = random.Random(45000 + d)
    b, exp = filler(r, TILE), []
    for p in (d, RUN * 5 + 10, RUN * 9 + 30, RUN * 13 + 31, RUN * 63 + 5):
        plant(b, p, 3, d)
        exp.append(("tok", p, 3, d) if d <= cw else ("nomatch", p, p + 3))
    return _tile("planted d=%d cw=%d" % (d, cw), b, exp, cw=cw)


def false_history_at(d):
    """lane 0, i = d - 1: position i holds (b[2047], b[0], b[1]) -- at distance d the search compares it with lane 63's last byte and
    the block's first two, a match in the rotated history that does not exist in the block"""
    r = random.Random(46000 + d)
    b = filler(r, TILE)
    i = d - 1
    if i < 2:
        return None                                                  # (the trigram would overlap its own source)
    b[i], b[i + 1], b[i + 2] = b[TILE - 1], b[0], b[1]
    if b[i + 3] == b[2]:
        b[i + 3] ^= 0x55
    return _tile("lane 0 i=d-1 d=%d" % d, b, [("nomatch", i, i + 1)])


@functools.lru_cache(maxsize=None)
def distance_groups():
    """every distance 1 .. 32 planted alone (window 32, and window 20, which refuses 21 .. 32), lane 0's false history one position in
    front of i = d, and positions with TWO candidates whose distances share an aligned group of four or straddle one: the nearer wins.
    4 / 7 and 28 / 31: three copies of one trigram.  7 / 8 and 31 / 32: neighbouring distances mean overlapping sources, a run of four
    of one byte, and the trigram of that byte at p.  1 / 3 and 3 / 4 exist only inside a run of one byte, where distance 1 is a
    candidate as well: a run of 14 -- the first match takes ten, the next token starts where every distance 1 .. 10 is a candidate,
    and takes 1"""
    out = [_planted_distance(d, cw) for cw in (32, 20) for d in range(1, 33)]
    out += [c for c in (false_history_at(d) for d in range(1, 33)) if c is not None]
    for near, far in PAIRS_APART:
        for p in (RUN * 7 + 12, RUN * 20 + 31, 40, RUN * 63 + 3):
            r = random.Random(47000 + 100 * far + p)
            b = filler(r, TILE, 0, 200)
            t = [200 + r.randrange(18) * 3 + k for k in range(3)]    # (bytes the filler does not hold)
            for q in (p - far, p - near, p):
                b[q:q + 3] = t
            out.append(_tile("pair %d/%d p=%d" % (near, far, p), b, [("tok", p - near, 3, far - near), ("tok", p, 3, near)]))
    for near, far in PAIRS_NEXT:
        for p in (RUN * 7 + 12, RUN * 20 + 31, 40, RUN * 63 + 3):
            r = random.Random(48000 + 100 * far + p)
            b = filler(r, TILE, 0, 200)
            x = 200 + r.randrange(56)
            b[p - far:p - far + 4] = [x] * 4
            b[p:p + 3] = [x] * 3
            out.append(_tile("pair %d/%d p=%d" % (near, far, p), b, [("tok", p - far + 1, 3, 1), ("tok", p, 3, near)]))
    for s in (RUN * 7 + 12, RUN * 20 + 25, 0, RUN * 63 + 8):
        r = random.Random(49000 + s)
        b = filler(r, TILE, 0, 200)
        b[s:s + 14] = [200 + r.randrange(56)] * 14
        out.append(_tile("run of 14 s=%d" % s, b, [("tok", s + 1, 10, 1), ("tok", s + 11, 3, 1)]))
    return out


# ------------------------------------------------------------------------------------------------ C: lengths next to edge literals
@functools.lru_cache(maxsize=None)
def lengths_and_literals():
    """a match of every length 3 .. 10 at the distances 1, 2, 16, 31, 32 (the ends of the match LUT's rows), each right behind a
    literal 0, 143, 144 or 255 that sits in every byte lane in turn; MAXMATCH 10 and 5 (which cuts the longer ones)"""
    out = []
    for mm in (10, 5):
        for d in LENGTH_DISTS:
            r = random.Random(50000 + 40 * mm + d)
            b, exp = filler(r, TILE, 1, 143), []
            for k, L in enumerate(range(3, 11)):
                for j, v in enumerate(EDGE_BYTES):
                    p = 64 + 48 * (4 * k + j) + (k + j) % 4 + 1          # the literal at p - 1: every byte lane for every value
                    plant(b, p, L, d, 1, 143)
                    if d == 1:                                       # (the source IS the literal: a run of it)
                        for q in range(p - 1, p + L):
                            b[q] = v
                    elif d == 2:
                        for q in range(p - 1, p + L, 2):
                            b[q] = v
                    else:
                        b[p - 1] = v
                    exp += [("lit", p - 1), ("tok", p, min(L, mm), d)]
            out.append(_tile("lengths d=%d mm=%d" % (d, mm), b, exp, mm=mm))
    return out


# ------------------------------------------------------------------------------------------------ D: the plain Adler sums
@functools.lru_cache(maxsize=None)
def adler_extremes():
    """2048 and 2047 bytes of 0xFF: every lane's sum and every weight at its maximum (the wave's sum of weights is the largest there
    is); five bytes: one lane with five terms, 63 with none; a period of three high bytes"""
    out = [_tile("ff n=%d" % n, b"\xff" * n, [("tok", 1, 10, 1)]) for n in (2048, 2047)]
    out.append(_tile("ff n=5", b"\xff" * 5, [("all_lit",)]))
    out.append(_tile("five", bytes([1, 200, 0, 255, 144]), [("all_lit",)]))
    out.append(_tile("fe ff ff n=2048", bytes(255 - (k % 3 == 0) for k in range(TILE)), [("tail", 3, 3)]))      # (period 3: no distance 1)
    return out


FAMILIES = (literal_tiles, literal_tile_neighbours, distance_groups, lengths_and_literals, adler_extremes)


def all_cases():
    return [c for f in FAMILIES for c in f()]
