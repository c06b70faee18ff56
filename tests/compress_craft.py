"""Crafted inputs for the compress kernels that walk a block in several 2048-position tiles (k_compress<., ., false>, the stream passes of
hdlz_compress_stream.hip, k_compress_chunk): lone matches over a tile seam, the block's neighbours in memory, every carried parse phase,
block ends at a seam and chains of tiles long enough for the two-level scans.  No GPU and no torch here: tests/test_compress_seams_cpu.py
holds the premises against the oracle's tokens, tests/test_gpu_compress_seams.py compares the kernels with the oracle's bytes.

A case is (label, bytes); the label is "F key=value ..." (fields() reads it back).  Everything is seeded: the same (cwindow, maxmatch)
gives the same bytes in every process.  Background bytes are noise; a chance match in it is harmless, the oracle decides what is right."""
import functools
import random

import numpy as np

TILE = 2048
SEAMS = (TILE, 2 * TILE)
N0, N7 = 3 * TILE, 3 * TILE + 7                   # three tiles; three tiles and a fourth of 7 bytes
WINDOWS = [(32, 10), (32, 5), (31, 10), (20, 10), (33, 10), (48, 5), (64, 10), (65, 10), (200, 10), (255, 5), (256, 10), (256, 5)]
SESSION_WINDOWS = [(32, 10), (64, 10), (256, 10)]
CHAIN_WINDOWS = [(32, 10), (64, 10), (256, 5)]
OFFSETS_A = tuple(range(-12, 4))                  # start of the planted match relative to the seam
LENGTHS_A = (3, 4, 9, 10, 12)                     # 12: comes out as maxmatch
DEFECTS_C = (-45, -33, -32, -31, -20, -11, -10, -9, -3, -1, 0, 1, 9, 10, 11)
TILES_E = (255, 256, 257, 512, 514)
BIG_TILES_E = 64 * 256 + 1                        # 65 chunks of 256 tiles: K = 2 in k_stream_skips_top / k_stream_offsets_top


def label(family, **kw):
    return family + "".join(" %s=%s" % kv for kv in kw.items())


def fields(lab):
    """the label's key=value pairs, numbers as int; "family" is its first word"""
    words = lab.split()
    out = {"family": words[0]}
    for w in words[1:]:
        k, v = w.split("=")
        out[k] = int(v) if v.lstrip("-").isdigit() else v
    return out


def _seed(family, cw, mm, extra=0):
    return (ord(family) * 1000003 + cw * 1009 + mm * 17 + extra) & 0x7FFFFFFF


def _pattern(r, per):
    """`per` bytes none of whose cyclic 3-grams repeats: the periodic body built from it has no match nearer than `per`"""
    syms = list(range(256))
    r.shuffle(syms)
    pat = syms[:min(per, 256)]
    if per > 256:                                 # 257: one byte twice, with different neighbours
        assert per == 257
        pat.append(pat[100])
    return bytes(pat)


def _periodic(pat, n, phase=0):
    per = len(pat)
    rep = (pat * ((n + phase) // per + 2))
    return rep[phase:phase + n]


def distances_a(cw):
    return sorted(d for d in {1, 2, 3, 31, 32, 33, cw - 1, cw, cw + 1} if 1 <= d <= 257)


# ------------------------------------------------------------------------------------------------ A: lone matches over a seam
def _plant(b, p, L, d):
    """b[p:p+L] becomes the copy of b[p-d:p-d+L] (byte by byte: d < L gives a run of period d), exactly L long and starting at p"""
    if p - 1 - d >= 0 and b[p - 1] == b[p - 1 - d]:
        b[p - 1] ^= 0x81                          # (before the copy: for d <= 2 this byte is part of the source)
    for k in range(L):
        b[p + k] = b[p - d + k]
    if b[p + L] == b[p + L - d]:
        b[p + L] ^= 0x42


@functools.lru_cache(maxsize=None)
def family_a(cw, mm):
    """-> {n: [(label, bytes)]}.  Every (seam, offset, distance) once, the length cycling so that every (offset, length) and every
    (distance, length) pair occurs at either seam; at N0 each case has its twin (byte 2 of the copy flipped: no match at that distance;
    a twin whose copy does not overlap its source and leaves room gets an exact copy at distance cw instead); N7 has the exact cases
    with the lengths shifted by two"""
    r = random.Random(_seed("A", cw, mm))
    out = {N0: [], N7: []}
    for n in (N0, N7):
        for si, S in enumerate(SEAMS):
            for oi, o in enumerate(OFFSETS_A):
                for di, d in enumerate(distances_a(cw)):
                    p = S + o
                    if p - d < 0:
                        continue
                    L = LENGTHS_A[(oi + di + si + (2 if n == N7 else 0)) % 5]
                    b = bytearray(r.randbytes(n))
                    _plant(b, p, L, d)
                    out[n].append((label("A", n=n, S=S, o=o, L=L, d=d, twin=0, far=0), bytes(b)))
                    if n != N0:
                        continue
                    b[p + 2] ^= 0x55
                    far = int(L <= d <= cw - L and p - cw >= 1)         # (d >= L: the copy does not repeat in itself)
                    if far:
                        b[p - cw:p - cw + L] = b[p:p + L]
                    out[n].append((label("A", n=n, S=S, o=o, L=L, d=d, twin=1, far=far), bytes(b)))
    return out


# ------------------------------------------------------------------------------------------------ B: the block's neighbours in memory
def distances_b(cw):
    return sorted({1, 2, 3, 9, min(cw, 31), cw})


LAYOUTS_B = ((N0, N0), (N7, N7), (N7, (N7 + 15) // 16 * 16))        # (n, pitch): back to back twice, and padded to 16 with 9 pad bytes


@functools.lru_cache(maxsize=None)
def family_b(cw, mm):
    """-> [(label, n, pitch, nblocks, mem)]: block k is mem[k * pitch:k * pitch + n].  From 5 .. 13 bytes (b_run) in front of the end of block k - 1,
    through the pad bytes, to j bytes into block k the memory is ONE run copied from distance d <= cw: block k - 1 ends in a match that
    the bytes behind it would extend, block k begins with bytes whose candidate lies in front of it.  j = 3 .. 12 for every distance"""
    out = []
    for li, (n, pitch) in enumerate(LAYOUTS_B):
        r = random.Random(_seed("B", cw, mm, li))
        dists = distances_b(cw)
        nb = 1 + 10 * len(dists)
        mem = bytearray(r.randbytes((nb - 1) * pitch + n + 64))
        for k in range(1, nb + 1):                # (k == nb: the bytes behind the last block continue its last match, too)
            d = dists[((k - 1) // 10) % len(dists)]
            j = 3 + (k - 1) % 10
            end = (k - 1) * pitch + n
            stop = min(k * pitch + j, len(mem))
            for i in range(end - b_run(k), stop):
                mem[i] = mem[i - d]
        out.append((label("B", n=n, pitch=pitch), n, pitch, nb, bytes(mem)))
    return out


def b_run(k):
    """bytes of the run in front of the end of block k - 1: most of them so few that the end of the block cuts the match, not maxmatch"""
    return (5, 6, 8, 11, 5, 6, 13, 7)[k % 8]


def b_fields(k, cw):
    """(d, j) of block k's front (k >= 1) and of block k - 1's end"""
    dists = distances_b(cw)
    return dists[((k - 1) // 10) % len(dists)], 3 + (k - 1) % 10


# ------------------------------------------------------------------------------------------------ C: parse phases
def periods_c(cw):
    return sorted({1, 2, 3, 7, cw - 1, cw, cw + 1})


def _block_c(r, n, h, per):
    return bytearray(r.randbytes(h) + _periodic(_pattern(r, per), n - h))


@functools.lru_cache(maxsize=None)
def family_c(cw, mm):
    """-> {n: [(label, bytes)]}.  h = 0 .. 9 bytes of noise, then a periodic body (every period of periods_c): the back-to-back maximal
    matches carry every phase over the seams.  At N0 the same blocks with ONE byte changed at S + o: every (period, o) at both seams with
    two prefixes each, so that every (h, o) and (h, period) pair occurs"""
    r = random.Random(_seed("C", cw, mm))
    out = {N0: [], N7: []}
    pers = periods_c(cw)
    for n in (N0, N7):
        for h in range(10):
            for per in pers:
                out[n].append((label("C", n=n, h=h, per=per, S=0, o=0, defect=0), bytes(_block_c(r, n, h, per))))
    for pi, per in enumerate(pers):
        for oi, o in enumerate(DEFECTS_C):
            for k, S in enumerate(SEAMS):
                for rep in (0, 1):
                    h = (pi + oi + 3 * k + 5 * rep) % 10
                    b = _block_c(r, N0, h, per)
                    b[S + o] ^= 0xA5
                    out[N0].append((label("C", n=N0, h=h, per=per, S=S, o=o, defect=1), bytes(b)))
    return out


# ------------------------------------------------------------------------------------------------ D: block ends at a seam
def sizes_d():
    s = set()
    for k in (1, 2, 3):
        s.update(TILE * k + r for r in (0, 1, 2, 3, 4, 5, 9, 10, 11, 12))
        s.update(TILE * k - r for r in (1, 9, 10, 11))
    return sorted(s)


def bodies_d(cw):
    return (1, 3, cw)


@functools.lru_cache(maxsize=None)
def family_d(cw, mm):
    """-> {n: [(label, bytes)]}, one block per (size, body).  The blocks of one body are cut one behind the other from ONE periodic
    string, in the order of sizes_d(): laid out in that order (d_flat) each block is followed by the continuation of its period, and
    tail_d gives that continuation for a block that stands alone"""
    r = random.Random(_seed("D", cw, mm))
    out = {n: [] for n in sizes_d()}
    for per in bodies_d(cw):
        pat = bytes(1) if per == 1 else _pattern(r, per)
        at = 0
        for n in sizes_d():
            out[n].append((label("D", n=n, per=per), _periodic(pat, n, at % per)))
            at += n
    return out


def tail_d(data, per, k):
    """the k bytes that continue a periodic block"""
    n = len(data)
    return bytes(data[n - per + i % per] for i in range(k))


def d_flat(cw, mm, per):
    """the blocks of one body in the order of sizes_d() -> (blocks, flat): back to back, the continuation behind the last one"""
    blocks = [b for n in sizes_d() for lab, b in family_d(cw, mm)[n] if fields(lab)["per"] == per]
    return blocks, b"".join(blocks) + tail_d(blocks[-1], per, 64)


# ------------------------------------------------------------------------------------------------ E: long chains
VARIANTS_E = ((1, 3), (7, 6))                     # (period, prefix)


@functools.lru_cache(maxsize=4)
def chain_e(tiles, variant):
    """-> (label, bytes): tiles * 2048 + 5 bytes, a prefix of h noise bytes and a body of period 1 or 7 (back-to-back maximal matches:
    every tile's transfer function is a permutation of the skip) with one byte changed about every 37 tiles (the parse re-synchronises
    there: a constant function among the permutations).  The phase that reaches a chunk seam (tile 256, 512, ...) comes through 30 and
    more permutation tiles"""
    per, h = VARIANTS_E[variant]
    n = tiles * TILE + 5
    r = random.Random(_seed("E", tiles & 0xFFFF, per, variant))
    b = bytearray(r.randbytes(h) + _periodic(_pattern(r, per), n - h))
    i = 1
    while True:
        q = 37 * TILE * i - 900 + (i * 613 + 7 * variant + 4) % 1500
        if q >= n - 16:
            break
        b[q] ^= 0x5A
        i += 1
    return label("E", tiles=tiles, per=per, h=h), bytes(b)


# ------------------------------------------------------------------------------------------------ the oracle, once per process
_streams, _tokens = {}, {}


def expect(oracle, data, cw, mm):
    """oracle.compress(data) -> (status, stream), computed once per (data, cwindow, maxmatch) and process"""
    key = (data, cw, mm)
    if key not in _streams:
        _streams[key] = oracle.compress(data, cwindow=cw, maxmatch=mm)
    return _streams[key]


def token_arrays(oracle, data, cw, mm):
    """oracle.tokens as three numpy arrays (pos, len, dist): the same call, without a Python tuple per token"""
    import ctypes
    n = len(data)
    pos, ln, ds = np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint16), np.zeros(n + 1, np.uint16)
    nt = ctypes.c_size_t(0)
    rc = oracle.lib().hdlz_oracle_tokens(data, n, cw, mm, pos.ctypes.data, ln.ctypes.data, ds.ctypes.data, n + 1, ctypes.byref(nt))
    assert rc == 0
    k = nt.value
    return pos[:k].astype(np.int64), ln[:k].astype(np.int64), ds[:k].astype(np.int64)


def entry_skips(pos, ln, seams):
    """how far the token that covers S - 1 reaches beyond S, for every S of `seams` (token arrays of token_arrays)"""
    seams = np.asarray(seams, np.int64)
    i = np.searchsorted(pos, seams - 1, side="right") - 1
    return pos[i] + np.maximum(ln[i], 1) - seams


def token_bits(tok):
    """bits of one oracle token in the fixed-Huffman stream"""
    _, ln, v = tok
    if ln == 0:
        return 8 if v < 144 else 9
    return 7 + 5 + max(0, (v - 1).bit_length() - 2)              # lengths 3 .. 10: seven bits, no extra bits


def first_wrong_token(oracle, data, cw, mm, ref, got):
    """the oracle's token in whose bits `got` first differs from `ref` (or a note that the difference lies in the frame)"""
    k = next((i for i in range(min(len(ref), len(got))) if ref[i] != got[i]), min(len(ref), len(got)))
    toks = oracle.tokens(data, cw, mm)
    bit = 16 + 3
    for i, t in enumerate(toks):
        bit += token_bits(t)
        if bit > 8 * k:
            return "byte %d of %d / %d: token %d of %d, %r after %r" % (k, len(ref), len(got), i, len(toks), t, toks[max(0, i - 3):i])
    return "byte %d of %d / %d: behind the last token (end of block, padding, Adler-32)" % (k, len(ref), len(got))
