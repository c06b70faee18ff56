"""Crafted inputs for the tile body of the compress kernels (hdlz_compress_common.h): the next lane's mismatch word at the lane seams of
the bit-sliced search, lane 63's missing neighbour, the bit counts and code widths of the LUT entries, the start flags of token_codes and
the cap of the extension.  No GPU and no torch here: tests/test_tile_diet_cpu.py holds every case against the oracle's tokens (an input
that does not show its token is a bug of this file), tests/test_gpu_tile_diet.py compares the kernels with the oracle's bytes.

A case is a Case: the bytes, (cwindow, maxmatch), the route that compresses it and what the oracle's token stream must hold:
  ("tok", p, L, d)      a match of length L at distance d starts at position p
  ("lit", p)            a literal starts at p
  ("nomatch", p, q)     no match starts in [p, q)
  ("all_lit",)          every token is a literal
  ("tail", p, d)        some match at distance d starts at or behind p
Routes: "tile" (a ragged batch with the bound 2048: k_compress<1, ., true>), "small" (a ragged batch with a bound <= 1024:
k_compress_small), "wide" (a ragged batch with the bound 4096: k_compress<8, ., false>), "stream" (Engine.compress_stream), "session"
(the chunked session path).  Everything is seeded.  A lane owns 32 consecutive positions of the block; "local" is the position in it.
Fillers hold no pair of neighbouring bytes twice, so no trigram repeats and nothing in them matches."""
import collections
import functools
import random

RUN, TILE = 32, 2048
Case = collections.namedtuple("Case", "label data cw mm route expect")
SEAM_SIZES = (2048, 2047, 2046, 2045, 1056, 37)
SENTINEL_CONFIGS = ((32, 10), (32, 5), (20, 10), (20, 5))       # FULLWIN true / false, MAXMATCH 10 / 5


def filler(r, n, lo=0, hi=256):
    """n bytes of [lo, hi), no pair of neighbours twice"""
    out = [r.randrange(lo, hi)]
    seen = set()
    while len(out) < n:
        for _ in range(10000):
            x = r.randrange(lo, hi)
            if x != out[-1] and (out[-1], x) not in seen:
                break
        else:
            raise AssertionError("alphabet too small for %d bytes" % n)
        seen.add((out[-1], x))
        out.append(x)
    return bytearray(out)


def _other(b, q, bad, lo, hi):
    """a byte of [lo, hi) for position q that is none of `bad` and neither neighbour"""
    bad = set(bad) | {b[q - 1] if q else -1, b[q + 1] if q + 1 < len(b) else -1}
    x = b[q]
    while x in bad:
        x = lo + (x - lo + 37) % (hi - lo)
    return x


def plant(b, p, L, d, lo=0, hi=256):
    """b[p:p+L] becomes the copy of b[p-d:p-d+L] (byte by byte), exactly L long and starting at p; what is changed stays in [lo, hi)"""
    assert p - d >= 0 and p + L <= len(b)
    if p - 1 - d >= 0 and b[p - 1] == b[p - 1 - d]:
        b[p - 1] = _other(b, p - 1, (b[p - 1 - d],), lo, hi)         # (before the copy: for d <= 2 this byte is part of the source)
    for k in range(L):
        b[p + k] = b[p - d + k]
    if p + L < len(b) and b[p + L] == b[p + L - d]:
        b[p + L] = _other(b, p + L, (b[p + L - d],), lo, hi)


def fresh(b, r, q, lo=0, hi=256, back=44, ahead=44):
    """a byte of [lo, hi) that does not occur within `back` bytes in front of position q nor `ahead` behind it"""
    near = set(b[max(0, q - back):q + ahead + 1])
    while True:
        x = r.randrange(lo, hi)
        if x not in near:
            return x


def _lanes(n):
    last = (n - 1) // RUN
    return sorted(l for l in {0, 1, 31, 62, 63, last - 1, last} if 0 <= l <= last)


def _expect_plant(n, p, L, d, mm):
    """what the oracle makes of a copy of L bytes planted at p: a match needs p <= n - 5 and ends at n - 2 at the latest"""
    got = min(L, mm, n - 2 - p)
    if p <= n - 5 and got >= 3:
        return ("tok", p, got, d)
    return ("nomatch", p, min(p + L, n))


# ------------------------------------------------------------------------------------------------ A: the next lane's word
@functools.lru_cache(maxsize=None)
def lane_seams():
    """every distance 1 .. 32, a three-byte match that starts at local 29, 30, 31 of lanes 0, 1, 31, 62, 63 (and of the block's last two
    lanes): its second or third byte lies in the next lane's word.  Then lengths 4 .. 10 from local 20 .. 31: the extension reads both"""
    out = []
    for n in SEAM_SIZES:
        for d in range(1, 33):
            for i in (29, 30, 31):
                r = random.Random(n * 100003 + d * 101 + i)
                b, exp = filler(r, n), []
                for l in _lanes(n):
                    p = RUN * l + i
                    if p - d < 0 or p + 3 > n:
                        continue
                    plant(b, p, 3, d)
                    exp.append(_expect_plant(n, p, 3, d, 10))
                if exp:
                    out.append(Case("seam n=%d d=%d i=%d" % (n, d, i), bytes(b), 32, 10, "tile", tuple(exp)))
    for n in (2048, 1056):
        for i in range(20, 32):
            for L in range(4, 11):
                d = 1 + (7 * i + 5 * L) % 32
                r = random.Random(n * 7919 + i * 131 + L)
                b, exp = filler(r, n), []
                for l in _lanes(n):
                    p = RUN * l + i
                    if p - d < 0 or p + L > n:
                        continue
                    plant(b, p, L, d)
                    exp.append(_expect_plant(n, p, L, d, 10))
                out.append(Case("long n=%d i=%d L=%d d=%d" % (n, i, L, d), bytes(b), 32, 10, "tile", tuple(exp)))
    return out


@functools.lru_cache(maxsize=None)
def lane63():
    """blocks of 2043 .. 2048 bytes that end in 40 bytes of period 1, 2, 3 or 32: nothing at or behind n - 4 may start a match"""
    out = []
    for n in range(2043, 2049):
        for per in (1, 2, 3, 32):
            r = random.Random(n * 31 + per)
            b = filler(r, n)
            pat = r.sample(range(256), per)
            for k in range(40):
                b[n - 40 + k] = pat[k % per]
            if b[n - 41] == pat[per - 1]:
                b[n - 41] ^= 0x55
            exp = [("nomatch", n - 4, n), ("tail", n - 40, per)]
            if per == 32:
                exp.append(("tok", n - 8, 6, 32))                    # cut by the end of the block: p + 6 = n - 2
            out.append(Case("lane63 n=%d per=%d" % (n, per), bytes(b), 32, 10, "tile", tuple(exp)))
    return out


# ------------------------------------------------------------------------------------------------ B: bit sums and code widths
def _nearest_is(b, p, d):
    t = bytes(b[p:p + 3])
    return all(bytes(b[p - dd:p - dd + 3]) != t for dd in range(1, d))


def _copy(b, L, d):
    for _ in range(L):
        b.append(b[len(b) - d])


@functools.lru_cache(maxsize=None)
def bit_sums():
    """2048 nine-bit literals (every lane sums 288 bits, the most there is); blocks that alternate a nine-bit literal with a match of
    the full length"""
    out = [Case("nine n=2048", bytes(filler(random.Random(9), 2048, 144, 256)), 32, 10, "tile", (("all_lit",),))]
    for seed in range(4):
        r = random.Random(1000 + seed)
        b, exp = filler(r, 40 + seed, 144, 256), []
        while len(b) + 11 + 4 <= TILE:
            q = len(b)
            b.append(fresh(b, r, q, 144, 256, ahead=0))
            for d in r.sample(range(3, 33), 30):
                _copy(b, 10, d)
                if _nearest_is(b, q + 1, d):
                    exp += [("lit", q), ("tok", q + 1, 10, d)]
                    break
                del b[q + 1:]
        while len(b) < TILE:
            b.append(fresh(b, r, len(b), 144, 256, ahead=0))
        out.append(Case("alternate seed=%d" % seed, bytes(b), 32, 10, "tile", tuple(exp)))
    return out


def _wide_piece(r, n, first, dists):
    """n bytes >= 144 (nine-bit literals); from `first` on, every 26 bytes a literal and right behind it a match of length 10 at a
    distance of `dists` (129 .. 256: 18 bits, the widest code), the literal at even and odd positions in turn"""
    b, exp = filler(r, n, 144, 256), []
    k, srcs, left = 0, [], list(dists)
    while first + 26 * k + 12 + 4 <= n and left:
        q = first + 26 * k + (k & 1)
        # a source that is no earlier copy's source: else that copy, which is nearer, holds the same bytes
        d = next((d for d in left if all(abs(q + 1 - d - s) >= 12 for s in srcs)), None)
        k += 1
        if d is None:
            continue
        left.remove(d)
        srcs.append(q + 1 - d)
        plant(b, q + 1, 10, d, 144, 256)
        exp += [("lit", q), ("tok", q + 1, 10, d)]
    return b, exp


WIDE_DISTS = tuple(range(129, 257))
WIDE_DISTS_SHORT = (129, 256, 130, 255, 160, 192, 193, 224, 225, 250, 131, 254, 144, 176, 208, 240)


@functools.lru_cache(maxsize=None)
def wide_codes():
    """CWINDOW 256: the widest pair, a nine-bit literal and an 18-bit match, through every kernel that emits codes"""
    out = []
    b, exp = _wide_piece(random.Random(256), 4096, 300, WIDE_DISTS)
    assert len(exp) == 2 * 128
    out.append(Case("wide n=4096", bytes(b), 256, 10, "wide", tuple(exp)))
    out.append(Case("wide session n=4096", bytes(b), 256, 10, "session", tuple(exp)))
    s, sexp = _wide_piece(random.Random(257), 1024, 260, WIDE_DISTS_SHORT)
    out.append(Case("wide small n=1024", bytes(s), 256, 10, "small", tuple(sexp)))
    big, bexp = bytearray(), []
    for k in range(4):                                               # (sources stay inside their piece: first >= 256 + 10)
        pb, pexp = _wide_piece(random.Random(300 + k), 4096, 300, WIDE_DISTS[32 * k:] + WIDE_DISTS[:32 * k])
        bexp += [(e[0], e[1] + 4096 * k) + e[2:] for e in pexp]
        big += pb
    out.append(Case("wide stream n=16384", bytes(big), 256, 10, "stream", tuple(bexp)))
    return out


# ------------------------------------------------------------------------------------------------ C: start flags
@functools.lru_cache(maxsize=None)
def start_flags():
    out = []
    # matches back to back at every length (a lane then starts as few tokens as it can: four for length 10)
    for L in range(3, 11):
        r = random.Random(500 + L)
        b, exp = filler(r, 40), []
        prev = None                                                  # distance of the match that ends at len(b), if it could go on
        while len(b) + L + 4 <= TILE:
            p = len(b)
            for d in r.sample(range(1, 33), 32):
                if prev is not None and b[p - d] == b[p - prev]:
                    continue                                         # (the match in front would go on)
                _copy(b, L, d)
                if _nearest_is(b, p, d):
                    exp.append(("tok", p, L, d))
                    prev = d if L < 10 else None
                    break
                del b[p:]
            else:
                b.append(fresh(b, r, p, ahead=0))
                prev = None
        while len(b) < TILE:
            b.append(fresh(b, r, len(b), ahead=0))
        assert len(exp) >= (TILE - 200) // L // 2, (L, len(exp))
        out.append(Case("back to back L=%d" % L, bytes(b), 32, 10, "tile", tuple(exp)))
    # a match that ends exactly at a lane's last position, every length
    r = random.Random(600)
    b, exp = filler(r, TILE), []
    for L in range(3, 11):
        for l in (2 * L, 2 * L + 21, 63 if L == 3 else 2 * L + 40):
            p, d = RUN * l + RUN - L, 1 + (5 * L + l) % 32
            if p + L > TILE - 2:
                continue
            plant(b, p, L, d)
            exp.append(("tok", p, L, d))
    out.append(Case("lane end", bytes(b), 32, 10, "tile", tuple(exp)))
    # a match that ends exactly at the last position a match may cover (n - 3): planted so, and cut there by the end of the block
    for n in (2048, 2047, 1056):
        for L in range(3, 11):
            for more in (0, 2):
                r = random.Random(n * 13 + L * 3 + more)
                b = filler(r, n)
                p, d = n - 2 - L, 1 + (3 * L + n) % 32
                plant(b, p, L + more, d)
                out.append(Case("tile end n=%d L=%d more=%d" % (n, L, more), bytes(b), 32, 10, "tile", (("tok", p, L, d), ("nomatch", n - 4, n))))
    # LIMIT: small blocks that end inside a lane
    for n in (5, 33, 100):
        for v in range(6):
            r = random.Random(n * 17 + v)
            b, exp = filler(r, n), []
            if n == 5:
                exp.append(("all_lit",))
            else:
                p, L, d = (8 + v, 3 + v, 2 + v) if n == 33 else (29 + v, 5 + v, 7 + 3 * v)
                plant(b, p, L, d)
                exp.append(("tok", p, L, d))
                x = fresh(b, r, n - 9, back=40, ahead=9)
                for k in range(n - 9, n):                            # a run to the end of the block: cut at n - 2
                    b[k] = x
                exp += [("tok", n - 8, 6, 1), ("nomatch", n - 4, n)]
            out.append(Case("limit n=%d v=%d" % (n, v), bytes(b), 32, 10, "small", tuple(exp)))
    return out


# ------------------------------------------------------------------------------------------------ D: the cap of the extension
@functools.lru_cache(maxsize=None)
def sentinel_runs():
    """runs of one byte, 3 .. 13 long, from local 0 and 20 .. 31: a match at distance 1 of every length up to the cap and beyond"""
    spots = [(i, R) for i in (0,) + tuple(range(20, 32)) for R in range(3, 14)]
    out = []
    for cw, mm in SENTINEL_CONFIGS:
        for blk in range(0, len(spots), 30):
            r = random.Random(cw * 1009 + mm * 17 + blk)
            b, exp = filler(r, TILE), []
            for k, (i, R) in enumerate(spots[blk:blk + 30]):
                p = RUN * (2 + 2 * k) + i
                x = fresh(b, r, p, back=44, ahead=60)
                for j in range(R):
                    b[p + j] = x
                if R >= 4:
                    exp.append(("tok", p + 1, min(R - 1, mm), 1))
                else:
                    exp.append(("nomatch", p, p + R))
            out.append(Case("runs cw=%d mm=%d blk=%d" % (cw, mm, blk), bytes(b), cw, mm, "tile", tuple(exp)))
    return out


def all_cases():
    return lane_seams() + lane63() + bit_sums() + wide_codes() + start_flags() + sentinel_runs()


def check(case, pos, ln, ds):
    """the case's expectations against the oracle's token arrays (compress_craft.token_arrays) -> list of the ones that fail"""
    import numpy as np
    bad = []
    for e in case.expect:
        if e[0] in ("tok", "lit"):
            k = int(np.searchsorted(pos, e[1]))
            got = (int(ln[k]), int(ds[k])) if k < len(pos) and pos[k] == e[1] else None
            ok = got is not None and (got == (e[2], e[3]) if e[0] == "tok" else got[0] == 0)
        elif e[0] == "nomatch":
            ok = not ((pos >= e[1]) & (pos < e[2]) & (ln > 0)).any()
        elif e[0] == "all_lit":
            ok = not (ln > 0).any() and len(pos) == len(case.data)
        elif e[0] == "tail":
            ok = bool(((pos >= e[1]) & (ln > 0) & (ds == e[2])).any())
        else:
            raise AssertionError(e)
        if not ok:
            bad.append(e)
    return bad
