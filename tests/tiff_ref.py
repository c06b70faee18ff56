"""The rule of include/hdlz_tiff.h in Python and numpy (a helper module, not a test): the hops, the tags and the record of every image
(index), the judgement of every chunk and the pixels of a decode (decode), and a small TIFF writer for the tests (make_tiff): either
byte order, strips or tiles, SHORT or LONG arrays, inline or out-of-line values, unsorted and duplicate tags, padded chunks, predictor
1 / 2 / 3, compression 1 / 8 / 32946, several pages, and tag overrides for the crafted files.  tests/test_tiff_cpu.py holds it against
Pillow; the GPU tests hold the library against it."""
import struct
import zlib

import numpy as np

from hdl_deflate_amd.constants import (OK, E_OUT_CAPACITY, E_BAD_BTYPE, E_NO_EOF, E_BAD_PARAM, E_BAD_HEADER, E_BAD_CHECKSUM)      # noqa: F401

LARGE_MIN = 16384
RAW_MAX, Z_MAX, OUT_MAX, PAGE_MAX = 2 ** 32 - 512, 2 ** 28 - 7, 2 ** 62, 65535
PHOTO_NONE = 0xFFFFFFFF
SHORT, LONG = 3, 4
TAGS = (256, 257, 258, 259, 262, 273, 277, 278, 279, 284, 317, 322, 323, 324, 325, 339)
ARRAYS = (258, 339, 273, 279, 324, 325)
KNOWN_COMPRESSIONS = (2, 3, 4, 5, 6, 7, 32773, 34712, 34925, 50000, 50001)
FIELDS = ("file_off", "file_len", "ifd_off", "next_ifd", "off_arr", "cnt_arr", "raw_len", "out_len", "chunk_off", "raw_off", "out_off",
          "width", "height", "tile_w", "tile_h", "nchunks", "compression", "photometric", "status", "off_type", "cnt_type", "bits", "samples",
          "format", "predictor", "big_endian", "tiled")
DECODER = "the decoder's own status"     # what decode answers where the deflate data itself is broken: the rule leaves the word to the decoder


def r16(x):
    return (x + 15) & ~15


def r256(x):
    return (x + 255) & ~255


# ---- THE RULE, steps 1 to 6
def geometry(width, height, tile_w, tile_h, tiled, samples, bits):
    """step 6 -> a dict, or None past a limit"""
    px = samples * bits // 8
    across, down = -(-width // tile_w), -(-height // tile_h)
    nchunks = across * down
    if nchunks >= 2 ** 31 or tile_w * tile_h * px > RAW_MAX or width * height * px > OUT_MAX:
        return None
    full = tile_w * tile_h * px
    last = full if tiled else (height - (down - 1) * tile_h) * tile_w * px
    return dict(px=px, across=across, nchunks=nchunks, full=full, last=last, raw_len=(nchunks - 1) * full + last,
                raw16=(nchunks - 1) * r16(full) + r16(last), out_len=width * height * px)


def image(f, page=0):
    """steps 1 to 6 for one file -> the fields of its record that the steps set (status alone when it fails)"""
    n = len(f)
    if n < 4:
        return dict(status=E_BAD_HEADER)
    if f[:4] in (b"II+\0", b"MM\0+"):
        return dict(status=E_BAD_BTYPE)
    if f[:4] not in (b"II*\0", b"MM\0*") or n < 8:
        return dict(status=E_BAD_HEADER)
    be = f[:2] == b"MM"
    e = ">" if be else "<"
    u16 = lambda p: struct.unpack_from(e + "H", f, p)[0]
    u32 = lambda p: struct.unpack_from(e + "I", f, p)[0]
    o = u32(4)
    for k in range(page + 1):
        if o == 0:
            return dict(status=E_NO_EOF)
        if o & 1 or o < 8:
            return dict(status=E_BAD_HEADER)
        if o + 2 > n:
            return dict(status=E_NO_EOF)
        nent = u16(o)
        if nent == 0:
            return dict(status=E_BAD_HEADER)
        if o + 2 + 12 * nent + 4 > n:
            return dict(status=E_NO_EOF)
        nxt = u32(o + 2 + 12 * nent)
        if k < page:
            o = nxt
    taken = {}
    for k in range(nent):
        at = o + 2 + 12 * k
        tag = u16(at)
        if tag not in TAGS or tag in taken:
            continue
        typ, cnt = u16(at + 2), u32(at + 4)
        if typ not in (SHORT, LONG) or cnt == 0:
            return dict(status=E_BAD_HEADER)
        nbytes = cnt * (2 if typ == SHORT else 4)
        where = at + 8
        if nbytes > 4:
            where = u32(at + 8)
            if where + nbytes > n:
                return dict(status=E_NO_EOF)
        if tag not in ARRAYS and cnt != 1:
            return dict(status=E_BAD_HEADER)
        taken[tag] = (where, typ, cnt)

    def value(tag, k=0, default=None):
        if tag not in taken:
            return default
        where, typ, _ = taken[tag]
        return u16(where + 2 * k) if typ == SHORT else u32(where + 4 * k)

    width, height = value(256, default=0), value(257, default=0)
    if not 0 < width < 2 ** 31 or not 0 < height < 2 ** 31:
        return dict(status=E_BAD_HEADER)
    samples = value(277, default=1)
    if samples == 0:
        return dict(status=E_BAD_HEADER)
    if samples > 8:
        return dict(status=E_BAD_BTYPE)
    for tag in (258, 339):
        if tag in taken and taken[tag][2] != samples:
            return dict(status=E_BAD_HEADER)
    bits, fmt = value(258, default=1), value(339, default=1)
    unequal = any(value(t, k) != value(t) for t in (258, 339) if t in taken for k in range(samples))
    if bits == 0 or bits > 64:
        return dict(status=E_BAD_HEADER)
    if unequal or bits not in (8, 16, 32, 64):
        return dict(status=E_BAD_BTYPE)
    if fmt == 0 or fmt > 6:
        return dict(status=E_BAD_HEADER)
    if fmt > 3 or (fmt == 3 and bits < 32):
        return dict(status=E_BAD_BTYPE)
    comp = value(259, default=1)
    if comp not in (1, 8, 32946):
        return dict(status=E_BAD_BTYPE if comp in KNOWN_COMPRESSIONS else E_BAD_HEADER)
    photo = value(262, default=PHOTO_NONE)
    if photo == 6:
        return dict(status=E_BAD_BTYPE)
    planar = value(284, default=1)
    if planar != 1:
        return dict(status=E_BAD_BTYPE if planar == 2 else E_BAD_HEADER)
    pred = value(317, default=1)
    if pred not in (1, 2, 3):
        return dict(status=E_BAD_HEADER)
    if pred == 3 and fmt != 3:
        return dict(status=E_BAD_BTYPE)
    tiled = 322 in taken
    if tiled:
        if not all(t in taken for t in (323, 324, 325)) or 273 in taken or 279 in taken:
            return dict(status=E_BAD_HEADER)
        tile_w, tile_h = value(322), value(323)
        if not 0 < tile_w < 2 ** 31 or not 0 < tile_h < 2 ** 31:
            return dict(status=E_BAD_HEADER)
        ao, ac = taken[324], taken[325]
    else:
        if 273 not in taken or 279 not in taken or any(t in taken for t in (323, 324, 325)):
            return dict(status=E_BAD_HEADER)
        rps = value(278, default=height)
        if rps == 0:
            return dict(status=E_BAD_HEADER)
        tile_w, tile_h = width, min(rps, height)
        ao, ac = taken[273], taken[279]
    g = geometry(width, height, tile_w, tile_h, tiled, samples, bits)
    if g is None:
        return dict(status=E_OUT_CAPACITY)
    if ao[2] != g["nchunks"] or ac[2] != g["nchunks"]:
        return dict(status=E_BAD_HEADER)
    return dict(status=OK, ifd_off=o, next_ifd=nxt, off_arr=ao[0], cnt_arr=ac[0], raw_len=g["raw_len"], out_len=g["out_len"], width=width,
                height=height, tile_w=tile_w, tile_h=tile_h, nchunks=g["nchunks"], compression=comp, photometric=photo, off_type=ao[1],
                cnt_type=ac[1], bits=bits, samples=samples, format=fmt, predictor=pred, big_endian=int(be), tiled=int(tiled))


def raw16_of(rec):
    return geometry(rec["width"], rec["height"], rec["tile_w"], rec["tile_h"], rec["tiled"], rec["samples"], rec["bits"])["raw16"]


def index(files, pages=None, out_align=64, image_cap=None, offsets=None, files_len=None):
    """files: a list of bytes -> {"images": the records (dicts of FIELDS), "nimages", "total_chunks", "total_raw", "total_out", "status"}.
    pages: per image its page (default 0); offsets: where the caller says the files lie in a buffer of files_len bytes (default:
    packed, in order)"""
    recs = []
    chunks = raw = out = end = at = 0
    for i, f in enumerate(files):
        off = at if offsets is None else offsets[i]
        at += len(f)
        page = 0 if pages is None else pages[i]
        rec = dict.fromkeys(FIELDS, 0)
        if (files_len is not None and off + len(f) > files_len) or page > PAGE_MAX:
            rec.update(status=E_BAD_PARAM)
        else:
            rec.update(image(f, page))
        rec.update(file_off=off, file_len=len(f), chunk_off=chunks, raw_off=raw, out_off=out)
        ok = rec["status"] == OK
        end = out + (rec["out_len"] if ok else 0)
        if ok:
            chunks += rec["nchunks"]
            raw += raw16_of(rec)
            out += (rec["out_len"] + out_align - 1) & -out_align
        recs.append(rec)
    cap = len(files) if image_cap is None else image_cap
    return dict(images=recs[:cap], nimages=len(files), total_chunks=chunks, total_raw=raw, total_out=end if files else 0,
                status=E_OUT_CAPACITY if len(files) > cap else OK)


def index_work_bytes(n):
    return 0 if n == 0 or n >= 2 ** 31 else 256 + r256(24 * n)


# ---- THE PIXELS
def np_dtype(fmt, bits, order="<"):
    return np.dtype(order + {1: "u", 2: "i", 3: "f"}[fmt] + str(bits // 8))


def unpredict(data, rows, rec):
    """the decoded bytes of one chunk (rows x tile_w pixels) -> a little-endian array (rows, tile_w, samples) of the unsigned words"""
    B, S, tw = rec["bits"] // 8, rec["samples"], rec["tile_w"]
    order = ">" if rec["big_endian"] else "<"
    if rec["predictor"] == 3:
        by = np.frombuffer(data, np.uint8).reshape(rows, tw * S * B).astype(np.uint64)
        for s in range(S):                                  # byte i += byte i - samples, over the whole row
            by[:, s::S] = np.cumsum(by[:, s::S], axis=1)
        planes = (by & 0xFF).astype(np.uint8).reshape(rows, B, tw * S)       # the most significant plane first
        words = np.zeros((rows, tw * S), np.uint64)
        for p in range(B):
            words |= planes[:, p, :].astype(np.uint64) << np.uint64(8 * (B - 1 - p))
        return words.astype("<u%d" % B).reshape(rows, tw, S)
    words = np.frombuffer(data, order + "u%d" % B).reshape(rows, tw, S).astype("<u%d" % B)
    if rec["predictor"] == 2:
        with np.errstate(over="ignore"):
            words = np.cumsum(words, axis=1, dtype="<u%d" % B)
    return words


def chunk_words(f, rec, k):
    e = ">" if rec["big_endian"] else "<"
    get = lambda arr, typ: struct.unpack_from(e + ("H" if typ == SHORT else "I"), f, arr + k * (2 if typ == SHORT else 4))[0]
    return get(rec["off_arr"], rec["off_type"]), get(rec["cnt_arr"], rec["cnt_type"])


def chunk_status(f, rec, k, raw_c):
    """steps (a) and (e) for chunk k -> (status, its decoded bytes or None)"""
    o, n = chunk_words(f, rec, k)
    if o + n > len(f):
        return E_NO_EOF, None
    if rec["compression"] == 1:
        return (E_NO_EOF, None) if n < raw_c else (OK, f[o:o + raw_c])
    if n < 6:
        return E_NO_EOF, None
    if n > Z_MAX:
        return E_OUT_CAPACITY, None
    z = f[o:o + n]
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(z[2:], raw_c + 1)
    except zlib.error:
        return DECODER, None
    if not d.eof and len(out) <= raw_c:
        return DECODER, None
    if z[0] & 15 != 8 or z[0] >> 4 > 7 or (z[0] * 256 + z[1]) % 31 or z[1] & 0x20:
        return E_BAD_HEADER, None
    if len(out) > raw_c:
        return E_OUT_CAPACITY, None
    if len(out) < raw_c:
        return E_BAD_CHECKSUM, None
    end = n - len(d.unused_data)
    if end + 4 > n:
        return E_NO_EOF, None
    if zlib.adler32(out) != struct.unpack_from(">I", z, end)[0]:
        return E_BAD_CHECKSUM, None
    return OK, out


def decode(f, rec):
    """the judgement of one image whose record is `rec` -> (status, the slot's bytes or None)"""
    if rec["status"] != OK:
        return rec["status"], None
    g = geometry(rec["width"], rec["height"], rec["tile_w"], rec["tile_h"], rec["tiled"], rec["samples"], rec["bits"])
    W, H, tw, th, S, B = rec["width"], rec["height"], rec["tile_w"], rec["tile_h"], rec["samples"], rec["bits"] // 8
    out = np.zeros((H, W, S), "<u%d" % B)
    for k in range(g["nchunks"]):
        raw_c = g["last"] if k == g["nchunks"] - 1 else g["full"]
        st, data = chunk_status(f, rec, k, raw_c)
        if st != OK:
            return st, None                                 # the lowest failed chunk
        rows = raw_c // (tw * g["px"])
        words = unpredict(data, rows, rec)
        tx, ty = k % g["across"], k // g["across"]
        x0, y0 = tx * tw, ty * th
        vw, vh = min(tw, W - x0), min(rows, H - y0)
        out[y0:y0 + vh, x0:x0 + vw] = words[:vh, :vw]
    return OK, out.tobytes()


def read(files, pages=None, out_align=64):
    """index and decode -> (the index, [status], [slot bytes or None])"""
    ix = index(files, pages, out_align)
    res = [decode(f, rec) for f, rec in zip(files, ix["images"])]
    return ix, [s for s, _ in res], [o for _, o in res]


def shape_of(rec):
    return (rec["height"], rec["width"]) if rec["samples"] == 1 else (rec["height"], rec["width"], rec["samples"])


def array_of(rec, data):
    return np.frombuffer(data, np_dtype(rec["format"], rec["bits"])).reshape(shape_of(rec))


def decode_work_bytes(L, count, chunk_cap, raw_bytes):
    """the closed form of hdlz_tiff_decode_work_bytes (L: the library, for the one-chunk route's share)"""
    if count == 0 or count >= 2 ** 31 or chunk_cap >= 2 ** 31 or raw_bytes >= 2 ** 40:
        return 0
    d = 0
    if count == 1 and chunk_cap == 1:
        d = r256(L.hdlz_inflate_work_bytes(1, min(2 * raw_bytes + 64, 2 ** 28 - 1), min(raw_bytes & ~3, 2 ** 32 - 512), 0, 1))
    return r256(8 * count) + r256(16 * count + 272) + r256(24 * chunk_cap) + r256(20 * chunk_cap) + r256(8 * (raw_bytes // 32768 + chunk_cap)) + \
        r256(raw_bytes) + d


# ---- a writer for the tests
def random_pixels(height, width, samples, fmt, bits, seed, smooth=False):
    """full-range random words of any bit pattern (sums wrap; floats include NaNs: compare bytes), or a smooth ramp that compresses"""
    shape = (height, width) if samples == 1 else (height, width, samples)
    dt = np_dtype(fmt, bits)
    if smooth:
        ramp = np.add.outer(np.arange(height), 3 * np.arange(width))[:, :, None] + 7 * np.arange(samples)
        return (ramp % 251).astype(dt).reshape(shape)
    return np.random.default_rng(seed).integers(0, 256, shape + (bits // 8,), dtype=np.uint8).view(dt).reshape(shape)


def predict(block, predictor, be):
    """a chunk's pixels (rows, tile_w, samples) of unsigned little-endian words -> its bytes as the file stores them, undecoded"""
    rows, tw, S = block.shape
    B = block.dtype.itemsize
    if predictor == 3:
        by = block.astype(">u%d" % B).view(np.uint8).reshape(rows, tw * S, B)
        planes = by.transpose(0, 2, 1).reshape(rows, tw * S * B).astype(np.int64)
        d = planes.copy()
        d[:, S:] -= planes[:, :-S]
        return (d & 0xFF).astype(np.uint8).tobytes()
    w = block
    if predictor == 2:
        w = block.copy()
        with np.errstate(over="ignore"):
            w[:, 1:] = block[:, 1:] - block[:, :-1]
    return w.astype((">" if be else "<") + "u%d" % B).tobytes()


def make_tiff(pages, big=False):
    """pages: a list of dicts -> the bytes of a TIFF file with one directory each.  A page:
      pix          numpy (H, W) or (H, W, S) of an unsigned, signed or float dtype (the SampleFormat and BitsPerSample follow it)
      compression  1, 8 (default) or 32946; level: zlib's
      predictor    1 (default), 2, 3
      tile         (tile_w, tile_h): tiles; else strips of `rps` rows (default: the whole image; rps_tag False: no tag 278)
      arrays       SHORT or LONG (default): the type of the two chunk arrays (SHORT offsets need a file below 64 KiB)
      pad          bytes appended to every chunk and counted in its byte count
      fill         the value of tile pixels outside the image (default 0xA5 bytes)
      unsorted     a seed: the entries are shuffled
      photometric  (default: 1, or 2 for 3 samples)
      override     {tag: (type, count, packed value bytes) or None (the tag is dropped)}: applied last, for crafted files
      extra        [(tag, type, count, packed value bytes)]: further entries, duplicates allowed; `extra_first`: put in front
      damage       f(k, chunk bytes) -> chunk bytes, applied to every stored chunk behind the compression
    Out-of-line values and chunks stand in front of their directory; every directory starts at an even offset."""
    e = ">" if big else "<"
    out = bytearray((b"MM\0*" if big else b"II*\0") + b"\0\0\0\0")
    link = 4                                                # where the offset of the next directory goes
    for pg in pages:
        pix = np.asarray(pg["pix"])
        if pix.ndim == 2:
            pix = pix[:, :, None]
        H, W, S = pix.shape
        B = pix.dtype.itemsize
        fmt = {"u": 1, "i": 2, "f": 3}[pix.dtype.kind]
        words = np.ascontiguousarray(pix.astype(pix.dtype.newbyteorder("<"))).view("<u%d" % B).reshape(H, W, S)
        comp, pred = pg.get("compression", 8), pg.get("predictor", 1)
        tile = pg.get("tile")
        tw, th = tile if tile else (W, min(pg.get("rps", H), H))
        across, down = -(-W // tw), -(-H // th)
        offs, cnts = [], []
        for k in range(across * down):
            tx, ty = k % across, k // across
            rows = th if tile else min(th, H - ty * th)
            block = np.frombuffer(bytes([pg.get("fill", 0xA5)]) * (rows * tw * S * B), "<u%d" % B).reshape(rows, tw, S).copy()
            part = words[ty * th:ty * th + rows, tx * tw:tx * tw + tw]
            block[:part.shape[0], :part.shape[1]] = part
            data = predict(block, pred, big)
            if comp != 1:
                data = zlib.compress(data, pg.get("level", 6))
            data += bytes(pg.get("pad", 0))
            if "damage" in pg:
                data = pg["damage"](k, data)
            offs.append(len(out))
            cnts.append(len(data))
            out += data
            if len(out) & 1:
                out += b"\0"
        at = pg.get("arrays", LONG)
        pack = lambda typ, vals: struct.pack(e + "%d%s" % (len(vals), "H" if typ == SHORT else "I"), *vals)
        ents = {256: (LONG, 1, pack(LONG, [W])), 257: (SHORT if H < 65536 else LONG, 1, pack(SHORT if H < 65536 else LONG, [H])),
                258: (SHORT, S, pack(SHORT, [8 * B] * S)), 259: (SHORT, 1, pack(SHORT, [comp])),
                262: (SHORT, 1, pack(SHORT, [pg.get("photometric", 2 if S == 3 else 1)])), 277: (SHORT, 1, pack(SHORT, [S])),
                284: (SHORT, 1, pack(SHORT, [1])), 339: (SHORT, S, pack(SHORT, [fmt] * S))}
        if pred != 1:
            ents[317] = (SHORT, 1, pack(SHORT, [pred]))
        if tile:
            ents.update({322: (SHORT, 1, pack(SHORT, [tw])), 323: (LONG, 1, pack(LONG, [th])), 324: (at, len(offs), pack(at, offs)),
                         325: (at, len(cnts), pack(at, cnts))})
        else:
            ents.update({273: (at, len(offs), pack(at, offs)), 279: (at, len(cnts), pack(at, cnts))})
            if pg.get("rps_tag", True):
                ents[278] = (LONG, 1, pack(LONG, [pg.get("rps", H)]))
        for tag, v in pg.get("override", {}).items():
            if v is None:
                ents.pop(tag, None)
            else:
                ents[tag] = v
        order = [(t,) + ents[t] for t in sorted(ents)]
        if pg.get("unsorted") is not None:
            np.random.default_rng(pg["unsorted"]).shuffle(order)
        extra = [tuple(x) for x in pg.get("extra", [])]
        order = extra + order if pg.get("extra_first") else order + extra
        fields = []
        for tag, typ, cnt, val in order:                    # the values that do not fit the entry, in front of the directory
            if len(val) > 4:
                fields.append(struct.pack(e + "I", len(out)))
                out += val
                if len(out) & 1:
                    out += b"\0"
            else:
                fields.append(val + b"\0" * (4 - len(val)))
        ifd = len(out)
        struct.pack_into(e + "I", out, link, ifd)
        out += struct.pack(e + "H", len(order))
        for (tag, typ, cnt, _), field in zip(order, fields):
            out += struct.pack(e + "HHI", tag, typ, cnt) + field
        link = len(out)
        out += b"\0\0\0\0"
    return bytes(out)
