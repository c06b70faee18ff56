"""What hdlz_png_filter_ws, hdlz_png_write_ws, Engine.encode_png and save_png must answer (a helper module like zip_write_ref.py, not a
conftest): THE FILTER RULE and THE FILE RULE of include/hdlz_png_write.h as serial texts in Python, built from png_ref.filter_rows,
joined_ref.expected_joined (the CPU oracle's rows, the end bit and the marker), chain.plan_blocks and zlib.crc32 / adler32 -- never from
device output --, and the case lists the CPU and the GPU tests share.  tests/test_png_write_cabi.py holds the rules against Pillow and
against the reader's rule of png_ref.py."""
import functools
import os
import re
import struct
import zlib

import numpy as np

import joined_ref as J
import png_ref as P

OK, E_OUT_CAPACITY, E_BAD_PARAM, E_BAD_HEADER = P.OK, P.E_OUT_CAPACITY, P.E_BAD_PARAM, P.E_BAD_HEADER
ADAPTIVE = 5
PAIRS = [(0, 8), (0, 16), (2, 8), (2, 16), (4, 8), (4, 16), (6, 8), (6, 16)]
NONE64 = 2 ** 64 - 1


def kernel_constants():
    """the constants of include/hdlz_png_write.h the filter kernel's paths hang on, read out of the header's text"""
    from types import SimpleNamespace
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hdlz_png_write.h")).read()
    found = {}
    for name in ("BAND", "STEP", "ROW_REG_MAX"):
        m = re.findall(r"#define\s+HDLZ_PNGW_%s\s+(\d+)u" % name, text)
        assert len(m) == 1, (name, m)
        found[name] = int(m[0])
    assert found["ROW_REG_MAX"] % found["STEP"] == 0 and found["STEP"] == 64 * 16
    return SimpleNamespace(**found)


def scanlines(pixels):
    """a numpy array (H, W) or (H, W, C) of uint8 or uint16 -> (the scanline bytes, width, height, colour, depth): 16-bit samples big-endian"""
    a = np.asarray(pixels)
    assert a.dtype in (np.uint8, np.uint16) and a.ndim in (2, 3)
    h, w, c = a.shape[0], a.shape[1], (a.shape[2] if a.ndim == 3 else 1)
    depth = 16 if a.dtype == np.uint16 else 8
    return (a.astype(">u2") if depth == 16 else a).tobytes(), w, h, {1: 0, 2: 4, 3: 2, 4: 6}[c], depth


def _residuals(raw, r, rb, bpp):
    """the five filtered rows of row r, int32 [5, rb] (values 0 .. 255)"""
    x = np.frombuffer(raw, np.uint8, rb, r * rb).astype(np.int32)
    b = np.frombuffer(raw, np.uint8, rb, (r - 1) * rb).astype(np.int32) if r else np.zeros(rb, np.int32)
    z = np.zeros(min(bpp, rb), np.int32)
    a = np.concatenate([z, x[:-bpp]]) if rb > bpp else np.zeros(rb, np.int32)
    c = np.concatenate([z, b[:-bpp]]) if rb > bpp else np.zeros(rb, np.int32)
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]) & 255


def row_sums(raw, height, rb, bpp):
    """S_f of every row: Python ints [height][5]"""
    out = []
    for r in range(height):
        y = _residuals(raw, r, rb, bpp).astype(np.int64)
        out.append([int(v) for v in np.where(y < 128, y, 256 - y).sum(axis=1)])
    return out


def choose_filters(raw, height, rb, bpp, mode):
    """THE FILTER RULE's choice: mode for every row, or per row the f with the smallest S_f, the lowest f on a tie"""
    if mode != ADAPTIVE:
        return [mode] * height
    return [s.index(min(s)) for s in row_sums(raw, height, rb, bpp)]


def filtered(raw, width, height, colour, depth, mode):
    """-> (the filtered stream, the filter of every row)"""
    rb, bpp = P.row_bytes_of(width, colour, depth), P.bpp_of(colour, depth)
    fl = choose_filters(raw, height, rb, bpp, mode)
    return P.filter_rows(raw, height, rb, bpp, fl), fl


def zstream(stream, block, cwindow=32, maxmatch=10):
    """THE FILE RULE's Z over a filtered stream"""
    from hdl_deflate_amd.chain import plan_blocks
    if len(stream) < 5:
        n = len(stream)
        return b"\x78\x9c\x01" + struct.pack("<HH", n, n ^ 0xFFFF) + stream + struct.pack(">I", zlib.adler32(stream))
    return J.expected_joined([stream[a:a + ln] for a, ln in plan_blocks(len(stream), block)], cwindow, maxmatch).stream


def frame(width, height, colour, depth, z, idat):
    """signature, IHDR, Z in IDAT chunks of idat bytes (the last shorter, never empty), IEND"""
    out = [P.SIG, P.chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, depth, colour, 0, 0, 0))]
    out += [P.chunk(b"IDAT", z[k:k + idat]) for k in range(0, len(z), idat)]
    out.append(P.chunk(b"IEND", b""))
    f = b"".join(out)
    assert len(f) == 33 + len(z) + 12 * -(-len(z) // idat) + 12
    return f


class Written(object):
    """file: the rule's bytes; stream: the filtered stream; filters: per row; z: the zlib stream"""


@functools.lru_cache(maxsize=None)
def _expected(raw, width, height, colour, depth, mode, block, idat, cwindow, maxmatch):
    w = Written()
    w.stream, w.filters = filtered(raw, width, height, colour, depth, mode)
    w.z = zstream(w.stream, block, cwindow, maxmatch)
    w.file = frame(width, height, colour, depth, w.z, idat)
    return w


def expected(pixels, mode=ADAPTIVE, block=1 << 16, idat=1 << 16, cwindow=32, maxmatch=10):
    """pixels: a numpy array as scanlines() takes it -> Written"""
    raw, w, h, colour, depth = scanlines(pixels)
    return _expected(raw, w, h, colour, depth, mode, block, idat, cwindow, maxmatch)


def bound(n, nblocks, block_len, idat_len):
    from hdl_deflate_amd.constants import out_bound
    Z = 15 * n + nblocks * (out_bound(block_len) - 1)
    return Z + 12 * (Z // idat_len) + 57 * n


def filter_work_bytes(n):
    r = lambda x: (x + 255) // 256 * 256
    return 2 * r(8 * (n + 1))


def write_work_bytes(n, nblocks):
    r = lambda x: (x + 255) // 256 * 256
    return 5 * r(8 * (nblocks + 1)) + 2 * r(8 * (n + 1)) + 2 * r(4 * n) + 256


# ---- pixels
def noise(shape, dtype, seed):
    return np.random.default_rng(seed).integers(0, 256 if dtype == np.uint8 else 65536, shape, dtype=dtype)


def smooth(shape, dtype, seed):
    """a ramp plus a little noise: every filter has something to predict and no row is trivially tied"""
    h, w = shape[0], shape[1]
    c = shape[2] if len(shape) == 3 else 1
    yy, xx, cc = np.mgrid[0:h, 0:w, 0:c]
    v = xx * 3 + yy * 5 + cc * 17 + np.random.default_rng(seed).integers(0, 4, (h, w, c))
    if dtype == np.uint16:
        v = v * 37
    return (v & (255 if dtype == np.uint8 else 65535)).astype(dtype).reshape(shape)


def ramp():
    """the noise-free ramp of the ratio condition: (3 x + 5 y) & 255 over the 768 bytes x of a row, 256 x 64 RGB"""
    yy, xx = np.mgrid[0:64, 0:768]
    return ((3 * xx + 5 * yy) & 255).astype(np.uint8).reshape(64, 256, 3)


def shape_for(colour, depth, width, height):
    c = P.CHANNELS[colour]
    return ((height, width) if c == 1 else (height, width, c)), (np.uint16 if depth == 16 else np.uint8)


# ---- crafted rows: 8-bit grey images of width 8 (bpp 1): (label, rows, the row in question, the filters that tie at its minimum)
CRAFTED = [
    ("0 wins", [[10, 200, 30, 180, 50, 160, 70, 140], [1, 255, 2, 254, 1, 255, 2, 254]], 1, [0]),
    ("1 wins", [[10, 200, 30, 180, 50, 160, 70, 140], [100, 101, 102, 103, 104, 105, 106, 107]], 1, [1]),
    ("2 wins", [[10, 200, 30, 180, 50, 160, 70, 140], [11, 201, 31, 181, 51, 161, 71, 141]], 1, [2, 4]),
    ("2 wins strictly", [[175, 176, 175, 175, 160, 161, 160, 161], [175, 175, 161, 161, 176, 161, 176, 161]], 1, [2]),
    ("3 wins", [[0, 100, 0, 100, 0, 100, 0, 100], [60, 80, 40, 70, 35, 68, 34, 67]], 1, [3]),
    ("4 wins", [[180, 160, 180, 180, 159, 180, 159, 159], [179, 179, 180, 179, 179, 159, 160, 180]], 1, [4]),
    ("0 and 1 tie", [[185, 167, 107, 120, 156, 190, 199, 121], [254, 0, 0, 0, 255, 255, 254, 255]], 1, [0, 1]),
    ("1 and 2 tie", [[221, 184, 222, 221, 221, 184, 221, 222], [183, 222, 184, 221, 183, 184, 183, 184]], 1, [1, 2]),
    ("2 and 3 tie", [[171, 171, 171, 128, 170, 129, 129, 129], [129, 170, 170, 170, 171, 171, 128, 129]], 1, [2, 3]),
    ("3 and 4 tie", [[255, 255, 255, 255, 169, 169, 174, 255], [169, 255, 169, 169, 174, 255, 255, 255]], 1, [3, 4]),
    ("1 to 4 tie", [[0, 4, 4, 4, 4, 4, 4, 4], [4, 4, 4, 4, 4, 4, 4, 4]], 1, [1, 2, 3, 4]),
    ("all five tie: a zero row under a zero row", [[0] * 8, [0] * 8], 1, [0, 1, 2, 3, 4]),
    ("all five tie: a first zero row", [[0] * 8], 0, [0, 1, 2, 3, 4]),
    ("a first row: b = c = 0, so 0 and 2 agree, and 1 and 4", [[5, 250, 3, 252, 7, 249, 2, 251]], 0, [0, 2]),
]


def crafted_properties():
    """the case list asserts what it claims of itself (CPU): who ties at the minimum of the row in question, and that between them the
    cases hold a strict winner for every f, a tie at the minimum between every adjacent pair, the all-zero rows and a first row"""
    strict, ties = set(), set()
    for label, rows, r, who in CRAFTED:
        a = np.array(rows, np.uint8)
        s = row_sums(a.tobytes(), a.shape[0], 8, 1)[r]
        got = [f for f in range(5) if s[f] == min(s)]
        assert got == who, (label, s, got)
        assert choose_filters(a.tobytes(), a.shape[0], 8, 1, ADAPTIVE)[r] == who[0], label
        if len(who) == 1:
            strict.add(who[0])
        ties |= {(f, f + 1) for f in who if f + 1 in who}
        if r == 0:                                           # a first row: nothing above it
            assert s[0] == s[2] and s[1] == s[4], label
    assert strict == {0, 1, 2, 3, 4} and ties >= {(0, 1), (1, 2), (2, 3), (3, 4)}
    assert any(len(who) == 5 for _, _, _, who in CRAFTED) and any(r == 0 for _, _, r, _ in CRAFTED)
    return strict, ties


def crafted_images():
    """[(label, pixels uint8 (H, 8))]"""
    return [(label, np.array(rows, np.uint8)) for label, rows, _, _ in CRAFTED]
