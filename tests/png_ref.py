"""The rule of include/hdlz_png.h in Python and numpy (a helper module, not a test): the chunk walk and the record of every image
(index), the judgement and the pixels of a decode (decode), and an encoder that takes the filter of every row, the zlib level, the IDAT
split and extra chunks as arguments (make_png).  tests/test_png_cabi.py holds it against Pillow; the GPU tests hold the library against
it."""
import struct
import zlib

import numpy as np

from hdl_deflate_amd.constants import (OK, E_OUT_CAPACITY, E_BAD_BTYPE, E_NO_EOF, E_BAD_SYMBOL, E_BAD_PARAM, E_BAD_HEADER,      # noqa: F401
                                       E_BAD_CHECKSUM)

SIG = b"\x89PNG\r\n\x1a\n"
RAW, EXPAND, LARGE_MIN = 0, 1, 16384
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
PAIRS = [(0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16), (6, 8), (6, 16)]
RAW_MAX, Z_MAX = 2 ** 32 - 512, 2 ** 28 - 7
FIELDS = ("file_off", "file_len", "idat_off", "zlen", "plte_off", "trns_off", "used", "row_bytes", "raw_len", "out_len", "z_off",
          "raw_off", "out_off", "width", "height", "nidat", "plte_n", "trns_n", "status", "depth", "colour", "interlace", "channels_out",
          "sample_bytes")


def r16(x):
    return (x + 15) & ~15


def bpp_of(colour, depth):
    return max(1, depth * CHANNELS[colour] // 8)


def row_bytes_of(width, colour, depth):
    return (width * depth * CHANNELS[colour] + 7) // 8


# ---- the encoder
def chunk(ctype, data, crc=None):
    return struct.pack(">I", len(data)) + ctype + data + struct.pack(">I", zlib.crc32(ctype + data) if crc is None else crc)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def filter_rows(raw, height, rb, bpp, filters):
    """the unfiltered scanlines -> the stream a PNG deflates: a filter byte and the filtered bytes per row (a filter byte above 4 is
    written as it is, over unfiltered bytes)"""
    out = bytearray()
    prev = bytes(rb)
    for r in range(height):
        f = filters[r]
        cur = raw[r * rb:(r + 1) * rb]
        x = np.frombuffer(cur, np.uint8).astype(np.int32)
        a = np.concatenate([np.zeros(bpp, np.int32), x[:-bpp]]) if rb > bpp else np.zeros(rb, np.int32)
        b = np.frombuffer(prev, np.uint8).astype(np.int32)
        c = np.concatenate([np.zeros(bpp, np.int32), b[:-bpp]]) if rb > bpp else np.zeros(rb, np.int32)
        if f == 1:
            y = x - a
        elif f == 2:
            y = x - b
        elif f == 3:
            y = x - ((a + b) >> 1)
        elif f == 4:
            p = a + b - c
            pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
            y = x - np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        else:
            y = x
        out.append(f)
        out += (y & 255).astype(np.uint8).tobytes()
        prev = cur
    return bytes(out)


def random_rows(width, height, colour, depth, seed, smooth=False):
    """unfiltered scanlines: noise, or (smooth) a ramp plus a little noise so that filters 1 to 4 have something to predict; pad bits 0"""
    rng = np.random.default_rng(seed)
    rb = row_bytes_of(width, colour, depth)
    if smooth:
        yy, xx = np.mgrid[0:height, 0:rb]
        a = ((xx * 3 + yy * 5) & 255).astype(np.int64) + rng.integers(0, 4, (height, rb))
        a = (a & 255).astype(np.uint8)
    else:
        a = rng.integers(0, 256, (height, rb), dtype=np.uint8)
    pad = rb * 8 - width * depth * CHANNELS[colour]
    if pad:
        a[:, -1] &= (0xFF << pad) & 0xFF
    return a.tobytes()


def make_png(width, height, colour, depth, rows=None, filters=0, level=6, idat=None, palette=None, trns=None, extra=(), seed=0,
             interlace=0, strategy=zlib.Z_DEFAULT_STRATEGY, stream=None, ihdr=None):
    """-> the bytes of a PNG.  rows: the unfiltered scanlines (default: noise from `seed`); filters: one type for all rows or a list per
    row; idat: the split size (None: one chunk) or a list of sizes (the rest in a last chunk); palette: bytes of RGB triples (default for
    colour 3: 2^depth random ones); trns: bytes; extra: (where, type, data) chunks, where in "front" (behind IHDR), "mid" (between PLTE
    and IDAT), "split" (between two IDATs), "back" (behind the IDATs); stream: the zlib stream to store instead of the encoded one;
    ihdr: the 13 bytes to store instead of the true ones"""
    rb, bpp = row_bytes_of(width, colour, depth), bpp_of(colour, depth)
    if rows is None:
        rows = random_rows(width, height, colour, depth, seed)
    fl = [filters] * height if isinstance(filters, int) else list(filters)
    if stream is None:
        co = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
        stream = co.compress(filter_rows(rows, height, rb, bpp, fl)) + co.flush()
    out = [SIG, chunk(b"IHDR", ihdr if ihdr is not None else struct.pack(">IIBBBBB", width, height, depth, colour, 0, 0, interlace))]
    out += [chunk(t, d) for w, t, d in extra if w == "front"]
    if colour == 3 and palette is None:
        palette = np.random.default_rng(seed + 1).integers(0, 256, 3 << depth, dtype=np.uint8).tobytes()
    if palette is not None:
        out.append(chunk(b"PLTE", palette))
    if trns is not None:
        out.append(chunk(b"tRNS", trns))
    out += [chunk(t, d) for w, t, d in extra if w == "mid"]
    sizes = [len(stream)] if idat is None else idat if isinstance(idat, (list, tuple)) else [idat] * (len(stream) // idat + 1)
    at, pieces = 0, []
    for s in sizes:
        if at >= len(stream):
            break
        pieces.append(stream[at:at + s])
        at += s
    if at < len(stream):
        pieces.append(stream[at:])
    for k, pc in enumerate(pieces or [b""]):
        out.append(chunk(b"IDAT", pc))
        if k == 0:
            out += [chunk(t, d) for w, t, d in extra if w == "split"]
    out += [chunk(t, d) for w, t, d in extra if w == "back"]
    out.append(chunk(b"IEND", b""))
    return b"".join(out)


# ---- THE RULE
def _be32(f, p):
    return struct.unpack_from(">I", f, p)[0]


def sizes_of(width, height, depth, colour, trns, flags):
    ch = CHANNELS[colour]
    rb = row_bytes_of(width, colour, depth)
    sb = 2 if depth == 16 else 1
    co = (4 if trns else 3) if (flags & EXPAND) and colour == 3 else ch
    raw_len = height * (rb + 1)
    out_len = height * width * co * sb if flags & EXPAND else height * rb
    return rb, raw_len, out_len, co, sb


def image(f, flags):
    """steps 1 to 4 for one file -> the record's fields but file_off and the offsets (a failed image: status only)"""
    n = len(f)
    if n < 8 or f[:8] != SIG:
        return dict(status=E_BAD_HEADER)
    if n >= 16 and f[8:16] != b"\x00\x00\x00\x0dIHDR":
        return dict(status=E_BAD_HEADER)
    p, seen, gap, plte, trns = 8, False, False, None, None
    idat_off = nidat = zlen = 0
    while True:
        if p + 12 > n:
            return dict(status=E_NO_EOF)
        L = _be32(f, p)
        if L >= 2 ** 31:
            return dict(status=E_BAD_HEADER)
        if p + 12 + L > n:
            return dict(status=E_NO_EOF)
        t = f[p + 4:p + 8]
        if t == b"IEND":
            used = p + 12 + L
            break
        if t == b"IHDR":
            if p != 8:
                return dict(status=E_BAD_HEADER)
        elif t == b"IDAT":
            if gap:
                return dict(status=E_BAD_HEADER)
            if not seen:
                idat_off = p
            nidat, zlen, seen = nidat + 1, zlen + L, True
        else:
            if seen:
                gap = True
            if not t[0] & 0x20 and t != b"PLTE":
                return dict(status=E_BAD_BTYPE)
            if t == b"PLTE" and not seen and plte is None:
                if L == 0 or L > 768 or L % 3:
                    return dict(status=E_BAD_HEADER)
                plte = (p + 8, L // 3)
            elif t == b"tRNS" and not seen and trns is None and f[25] == 3:
                if L > 256:
                    return dict(status=E_BAD_HEADER)
                trns = (p + 8, L)
        p += 12 + L
    if not seen or (f[25] == 3 and plte is None):
        return dict(status=E_BAD_HEADER)
    width, height, depth, colour, comp, filt, lace = struct.unpack_from(">IIBBBBB", f, 16)
    if width == 0 or height == 0 or width >= 2 ** 31 or height >= 2 ** 31:
        return dict(status=E_BAD_HEADER)
    if (colour, depth) not in PAIRS or comp or filt:
        return dict(status=E_BAD_HEADER)
    if lace == 1:
        return dict(status=E_BAD_BTYPE)
    if lace > 1:
        return dict(status=E_BAD_HEADER)
    rb, raw_len, out_len, co, sb = sizes_of(width, height, depth, colour, trns is not None, flags)
    if raw_len > RAW_MAX or zlen > Z_MAX:
        return dict(status=E_OUT_CAPACITY)
    return dict(status=OK, idat_off=idat_off, zlen=zlen, plte_off=plte[0] if plte else 0, plte_n=plte[1] if plte else 0,
                trns_off=trns[0] if trns else 0, trns_n=trns[1] if trns else 0, used=used, row_bytes=rb, raw_len=raw_len, out_len=out_len,
                width=width, height=height, nidat=nidat, depth=depth, colour=colour, interlace=0, channels_out=co, sample_bytes=sb)


def index(files, flags=EXPAND, out_align=64, image_cap=None, offsets=None, files_len=None):
    """files: a list of bytes -> {"images": the records (dicts of FIELDS), "nimages", "total_z", "total_raw", "total_out", "status"}.
    offsets: where the caller says the files lie in a buffer of files_len bytes (default: packed, in order)"""
    recs = []
    z = raw = out = end = at = 0
    for i, f in enumerate(files):
        off = at if offsets is None else offsets[i]
        at += len(f)
        rec = dict.fromkeys(FIELDS, 0)
        if files_len is not None and off + len(f) > files_len:
            rec.update(status=E_BAD_PARAM)
        else:
            rec.update(image(f, flags))
        rec.update(file_off=off, file_len=len(f), z_off=z, raw_off=raw, out_off=out)
        ok = rec["status"] == OK
        end = out + (rec["out_len"] if ok else 0)
        if ok:
            z += r16(rec["zlen"] + 8)
            raw += r16(rec["raw_len"])
            out += (rec["out_len"] + out_align - 1) & -out_align
        recs.append(rec)
    cap = len(files) if image_cap is None else image_cap
    return dict(images=recs[:cap], nimages=len(files), total_z=z, total_raw=raw, total_out=end if files else 0,
                status=E_OUT_CAPACITY if len(files) > cap else OK)


# ---- THE PIXELS
def unfilter(stream, height, rb, bpp):
    """-> (the unfiltered scanlines, was a filter byte above 4).  Filters 0 to 2 in numpy, 3 and 4 byte by byte as the text has them"""
    out = bytearray(height * rb)
    prev = bytes(rb)
    bad = False
    for r in range(height):
        f = stream[r * (rb + 1)]
        x = stream[r * (rb + 1) + 1:(r + 1) * (rb + 1)]
        if f > 4:
            bad, f = True, 0
        if f == 0:
            cur = bytearray(x)
        elif f == 2:
            cur = bytearray(((np.frombuffer(x, np.uint8).astype(np.int32) + np.frombuffer(prev, np.uint8)) & 255).astype(np.uint8).tobytes())
        elif f == 1:
            a = np.frombuffer(x, np.uint8).astype(np.int64)
            for k in range(bpp):                                # each of the bpp byte chains is a running sum
                a[k::bpp] = np.cumsum(a[k::bpp])
            cur = bytearray((a & 255).astype(np.uint8).tobytes())
        else:
            cur = bytearray(rb)
            for i in range(rb):
                a = cur[i - bpp] if i >= bpp else 0
                b = prev[i]
                c = prev[i - bpp] if i >= bpp else 0
                cur[i] = (x[i] + ((a + b) >> 1 if f == 3 else _paeth(a, b, c))) & 255
        out[r * rb:(r + 1) * rb] = cur
        prev = bytes(cur)
    return bytes(out), bad


def expand(raw, rec, f):
    """the unfiltered scanlines of an image -> the bytes HDLZ_PNG_EXPAND delivers (f: the file, for PLTE and tRNS)"""
    h, w, d, colour, rb = rec["height"], rec["width"], rec["depth"], rec["colour"], rec["row_bytes"]
    a = np.frombuffer(raw, np.uint8).reshape(h, rb)
    if d == 16:
        return a.reshape(h, rb // 2, 2)[:, :, ::-1].tobytes()
    if d == 8 and colour != 3:
        return raw
    if d < 8:
        bits = np.unpackbits(a, axis=1)[:, :w * d].reshape(h, w, d)
        v = np.zeros((h, w), np.int64)
        for k in range(d):
            v = (v << 1) | bits[:, :, k]
    else:
        v = a.astype(np.int64)
    if colour != 3:
        return (v * (255 // ((1 << d) - 1))).astype(np.uint8).tobytes()
    n, co = rec["plte_n"], rec["channels_out"]
    table = np.zeros((256, co), np.uint8)
    table[:n, :3] = np.frombuffer(f[rec["plte_off"]:rec["plte_off"] + 3 * n], np.uint8).reshape(n, 3)
    if co == 4:
        table[:, 3] = 255
        table[:rec["trns_n"], 3] = np.frombuffer(f[rec["trns_off"]:rec["trns_off"] + rec["trns_n"]], np.uint8)
    return table[v].tobytes()


def chunks_of(f, rec):
    """the chunks the decode checks: IHDR, the PLTE and tRNS taken, every IDAT, IEND -> [(type offset, data length)]; and the IDAT data"""
    got = [(12, 13)]
    if rec["plte_off"]:
        got.append((rec["plte_off"] - 4, 3 * rec["plte_n"]))
    if rec["trns_off"]:
        got.append((rec["trns_off"] - 4, rec["trns_n"]))
    p, z = rec["idat_off"], []
    for _ in range(rec["nidat"]):
        L = _be32(f, p)
        got.append((p + 4, L))
        z.append(f[p + 8:p + 8 + L])
        p += 12 + L
    while f[p + 4:p + 8] != b"IEND":
        p += 12 + _be32(f, p)
    got.append((p + 4, _be32(f, p)))
    return got, b"".join(z)


DECODER = "the decoder's own status"     # what decode answers where the deflate data itself is broken: the rule leaves the word to the decoder


def decode(f, rec, flags=EXPAND):
    """the judgement of one image whose record is `rec` -> (status, the slot's bytes or None)"""
    if rec["status"] != OK:
        return rec["status"], None
    if rec["zlen"] < 6:
        return E_NO_EOF, None
    got, z = chunks_of(f, rec)
    for at, L in got:
        if zlib.crc32(f[at:at + 4 + L]) != _be32(f, at + 4 + L):
            return E_BAD_CHECKSUM, None
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(z[2:])
    except zlib.error:
        return DECODER, None
    if not d.eof:
        return DECODER, None
    end = len(z) - len(d.unused_data)
    if z[0] & 15 != 8 or z[0] >> 4 > 7 or (z[0] * 256 + z[1]) % 31 or z[1] & 0x20:
        return E_BAD_HEADER, None
    if len(out) > rec["raw_len"]:
        return E_OUT_CAPACITY, None
    if len(out) < rec["raw_len"]:
        return E_BAD_CHECKSUM, None
    if end + 4 != rec["zlen"]:
        return E_NO_EOF, None
    if zlib.adler32(out) != _be32(z, end):
        return E_BAD_CHECKSUM, None
    raw, bad = unfilter(out, rec["height"], rec["row_bytes"], bpp_of(rec["colour"], rec["depth"]))
    if bad:
        return E_BAD_SYMBOL, None
    return OK, expand(raw, rec, f) if flags & EXPAND else raw


def read(files, flags=EXPAND, out_align=64):
    """index and decode -> (the index, [status], [slot bytes or None])"""
    ix = index(files, flags, out_align)
    res = [decode(f, rec, flags) for f, rec in zip(files, ix["images"])]
    return ix, [s for s, _ in res], [o for _, o in res]


def shape_of(rec, flags=EXPAND):
    if not flags & EXPAND:
        return (rec["height"], rec["row_bytes"])
    return (rec["height"], rec["width"]) if rec["channels_out"] == 1 else (rec["height"], rec["width"], rec["channels_out"])
