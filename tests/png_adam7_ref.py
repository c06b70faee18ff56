"""The rule of include/hdlz_png.h for Adam7 interlaced images, in Python and numpy (a helper module, not a test): tests/png_ref.py
extended by the pass geometry, an encoder of interlaced files (make_adam7) and, under flags & ADAM7, the sizes of step 4 and the pixels
of an interlaced image: every pass unfiltered by png_ref.unfilter as an image of its own, scattered, then png_ref.expand.  Everything
else is png_ref's.  tests/test_png_adam7_cpu.py holds it against Pillow; the GPU tests hold the library against it."""
import zlib

import numpy as np

import png_ref as P
from png_ref import OK, E_BAD_BTYPE, E_BAD_HEADER, E_OUT_CAPACITY, E_NO_EOF, E_BAD_CHECKSUM, E_BAD_SYMBOL, E_BAD_PARAM     # noqa: F401

ADAM7 = 4
# pass p = 1 .. 7: (x0, y0, dx, dy)
PASSES = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))


def passes_of(width, height, colour, depth):
    """-> [(x0, y0, dx, dy, pw, ph, prb)] of the PRESENT passes, in stream order"""
    got = []
    for x0, y0, dx, dy in PASSES:
        pw = -(-(width - x0) // dx) if width > x0 else 0
        ph = -(-(height - y0) // dy) if height > y0 else 0
        if pw and ph:
            got.append((x0, y0, dx, dy, pw, ph, (pw * depth * P.CHANNELS[colour] + 7) // 8))
    return got


def raw_len_of(width, height, colour, depth):
    return sum(ph * (prb + 1) for _, _, _, _, _, ph, prb in passes_of(width, height, colour, depth))


def _pixels(rows, width, height, colour, depth):
    """packed scanlines -> an array (height, width, k) of the pixels' pieces: bits below 8 bits a pixel, else bytes"""
    rb = P.row_bytes_of(width, colour, depth)
    a = np.frombuffer(rows, np.uint8).reshape(height, rb)
    bits = depth * P.CHANNELS[colour]
    if bits < 8:
        return np.unpackbits(a, axis=1)[:, :width * bits].reshape(height, width, bits)
    return a.reshape(height, width, bits // 8)


def _packed(px, colour, depth):
    """the inverse of _pixels for one (sub-)image: (h, w, k) -> packed scanlines, pad bits 0"""
    h, w, _ = px.shape
    if depth * P.CHANNELS[colour] < 8:
        return np.packbits(px.reshape(h, -1), axis=1).tobytes()
    return np.ascontiguousarray(px).tobytes()


def interlace_rows(rows, w, h, colour, depth):
    """the unfiltered scanlines of an image -> [the unfiltered scanlines of each present pass]"""
    px = _pixels(rows, w, h, colour, depth)
    return [_packed(px[y0::dy, x0::dx], colour, depth) for x0, y0, dx, dy, _, _, _ in passes_of(w, h, colour, depth)]


def deinterlace(subs, w, h, colour, depth):
    """the inverse of interlace_rows"""
    px = None
    for sub, (x0, y0, dx, dy, pw, ph, _) in zip(subs, passes_of(w, h, colour, depth)):
        s = _pixels(sub, pw, ph, colour, depth)
        if px is None:
            px = np.zeros((h, w, s.shape[2]), np.uint8)
        px[y0::dy, x0::dx] = s
    return _packed(px, colour, depth)


def adam7_stream(w, h, colour, depth, rows, filters=0):
    """the bytes an interlaced PNG deflates.  filters: one type for all rows, a list per row of the STREAM (the passes' rows, one behind
    the other), or a function (pass number 1 .. 7, rows of the pass) -> a list"""
    bpp = P.bpp_of(colour, depth)
    out, at = [], 0
    geo = passes_of(w, h, colour, depth)
    for sub, (x0, y0, dx, dy, pw, ph, prb) in zip(interlace_rows(rows, w, h, colour, depth), geo):
        if callable(filters):
            fl = list(filters(PASSES.index((x0, y0, dx, dy)) + 1, ph))
        else:
            fl = [filters] * ph if isinstance(filters, int) else list(filters[at:at + ph])
        assert len(fl) == ph
        out.append(P.filter_rows(sub, ph, prb, bpp, fl))
        at += ph
    return b"".join(out)


def make_adam7(w, h, colour, depth, rows=None, filters=0, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, seed=0, **kw):
    """-> the bytes of an interlaced PNG of the scanlines `rows` (default: noise from `seed`): every pass filtered by
    png_ref.filter_rows, the passes compressed as one stream, framed by png_ref.make_png (whose idat, palette, trns, extra and ihdr
    arguments pass through)"""
    if rows is None:
        rows = P.random_rows(w, h, colour, depth, seed)
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    stream = co.compress(adam7_stream(w, h, colour, depth, rows, filters)) + co.flush()
    return P.make_png(w, h, colour, depth, rows=rows, seed=seed, interlace=1, stream=stream, **kw)


def total_rows(w, h):
    """the rows of an interlaced image's stream"""
    return sum(g[5] for g in passes_of(w, h, 0, 8))


# ---- THE RULE
_image, _index = P.image, P.index          # (png_ref's own, whatever a test has put in their place)


def image(f, flags):
    """png_ref.image; with flags & ADAM7 a file whose interlace byte is 1 goes through every other line of the rule as it stands and
    gets, in step 4, the raw_len of its passes"""
    if not (flags & ADAM7) or len(f) < 29 or f[28] != 1:
        return _image(f, flags & P.EXPAND)
    g = bytearray(f)
    g[28] = 0                                                  # (the rule reads no CRC)
    keep = P.sizes_of

    def sizes(width, height, depth, colour, trns, fl):
        rb, _, out_len, co, sb = keep(width, height, depth, colour, trns, fl)
        return rb, raw_len_of(width, height, colour, depth), out_len, co, sb
    P.sizes_of = sizes
    try:
        rec = _image(bytes(g), flags & P.EXPAND)
    finally:
        P.sizes_of = keep
    if rec["status"] == OK:
        rec["interlace"] = 1
    return rec


def index(files, flags=P.EXPAND | ADAM7, out_align=64, image_cap=None, offsets=None, files_len=None):
    """png_ref.index with `image` above"""
    keep = P.image
    P.image = image
    try:
        return _index(files, flags, out_align, image_cap, offsets, files_len)
    finally:
        P.image = keep


def decode(f, rec, flags=P.EXPAND | ADAM7):
    """png_ref.decode; an interlaced record is judged on its raw_len, unfiltered pass by pass and scattered.  A record with
    interlace set and flags without ADAM7 is refused as the decode refuses it"""
    if rec["status"] != OK or not rec["interlace"]:
        return P.decode(f, rec, flags & P.EXPAND)
    if not flags & ADAM7:
        return E_BAD_PARAM, None
    w, h, colour, depth = rec["width"], rec["height"], rec["colour"], rec["depth"]
    if rec["raw_len"] != raw_len_of(w, h, colour, depth):
        return E_BAD_PARAM, None
    st, stream = _judged(f, rec)
    if st != OK:
        return st, None
    subs, at, bad = [], 0, False
    for x0, y0, dx, dy, pw, ph, prb in passes_of(w, h, colour, depth):
        sub, b = P.unfilter(stream[at:at + ph * (prb + 1)], ph, prb, P.bpp_of(colour, depth))
        subs.append(sub)
        bad |= b
        at += ph * (prb + 1)
    if bad:
        return E_BAD_SYMBOL, None
    raw = deinterlace(subs, w, h, colour, depth)
    return OK, P.expand(raw, rec, f) if flags & P.EXPAND else raw


def _judged(f, rec):
    """the lines of png_ref.decode in front of the unfilter -> (status, the decoded stream)"""
    if rec["zlen"] < 6:
        return E_NO_EOF, None
    got, z = P.chunks_of(f, rec)
    for at, L in got:
        if zlib.crc32(f[at:at + 4 + L]) != P._be32(f, at + 4 + L):
            return E_BAD_CHECKSUM, None
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(z[2:])
    except zlib.error:
        return P.DECODER, None
    if not d.eof:
        return P.DECODER, None
    end = len(z) - len(d.unused_data)
    if z[0] & 15 != 8 or z[0] >> 4 > 7 or (z[0] * 256 + z[1]) % 31 or z[1] & 0x20:
        return E_BAD_HEADER, None
    if len(out) > rec["raw_len"]:
        return E_OUT_CAPACITY, None
    if len(out) < rec["raw_len"]:
        return E_BAD_CHECKSUM, None
    if end + 4 != rec["zlen"]:
        return E_NO_EOF, None
    if zlib.adler32(out) != P._be32(z, end):
        return E_BAD_CHECKSUM, None
    return OK, out


def read(files, flags=P.EXPAND | ADAM7, out_align=64):
    """index and decode -> (the index, [status], [slot bytes or None])"""
    ix = index(files, flags, out_align)
    res = [decode(f, rec, flags) for f, rec in zip(files, ix["images"])]
    return ix, [s for s, _ in res], [o for _, o in res]
