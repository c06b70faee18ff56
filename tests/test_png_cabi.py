"""CPU: the extension header include/hdlz_png.h -- every declaration exported and bound with its arity, the tables in front of it and
the version as they were, both work-bytes queries equal to their closed forms, every parameter refusal in the header's order and in front
of the device, the mirrors of the three structs; and the rule and the pixels as tests/png_ref.py states them held against Pillow (where
it is installed) for every colour type and depth, on 1x1, 5x3 and 67x66 images with random filters and 7-byte IDATs."""
import ctypes
import io
import re

import numpy as np
import pytest

import png_ref as P
from cabi_common import declarations, header, host_buffer as _host_buffer, no_device as _no_device, r256

E_BAD_PARAM, E_HIP = 8, 9


def test_every_declaration_is_exported_and_bound():
    from hdl_deflate_amd import _lib
    text = header("hdlz_png.h")
    params = declarations(text)
    assert params == {"hdlz_png_index_work_bytes": 2, "hdlz_png_index_ws": 13, "hdlz_png_decode_work_bytes": 4, "hdlz_png_decode_ws": 16}
    assert sorted(params) == sorted(_lib.PNG_EXPORTS) == sorted(_lib.PNG_CALLS)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    L = _lib.load()
    for name, n in params.items():
        assert hasattr(raw, name), name
        restype, argtypes = _lib.PNG_CALLS[name]
        assert len(argtypes) == n, name
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert '#include "hdlz_zip.h"' in text and "Not there" in text
    assert int(re.search(r"#define\s+HDLZ_PNG_LARGE_MIN\s+(\d+)u", text).group(1)) == _lib.PNG_LARGE_MIN == P.LARGE_MIN
    assert (int(re.search(r"#define\s+HDLZ_PNG_RAW\s+(\d+)u", text).group(1)), int(re.search(r"#define\s+HDLZ_PNG_EXPAND\s+(\d+)u", text).group(1))) == \
        (_lib.PNG_RAW, _lib.PNG_EXPAND) == (P.RAW, P.EXPAND)
    import hdl_deflate_amd
    assert callable(hdl_deflate_amd.load_png) and hdl_deflate_amd.PngIndex is not None


def test_the_tables_in_front_of_it_are_as_they_were():
    from hdl_deflate_amd import _lib
    older = (_lib.EXPORTS, _lib.JOIN_EXPORTS, _lib.UNJOIN_EXPORTS, _lib.GZIP_EXPORTS, _lib.BGZF_EXPORTS, _lib.BGZF_RANGE_EXPORTS, _lib.BGZF_STORED_EXPORTS,
             _lib.GUNZIP_EXPORTS, _lib.ZIP_EXPORTS, _lib.ZIP_WRITE_EXPORTS, _lib.ZIP64_EXPORTS, _lib.GZIP_MEMBERS_EXPORTS, _lib.SEEK_EXPORTS)
    assert [len(t) for t in older] == [22, 4, 2, 7, 8, 2, 3, 2, 4, 3, 7, 4, 4]
    assert len(_lib.PNG_EXPORTS) == 4 and not set(_lib.PNG_EXPORTS) & set().union(*older)
    assert not [n for n in dir(_lib) if n.endswith("SIGNATURES") and "PNG" in n]
    assert _lib.load().hdlz_version() == 0x000600
    assert "PNG" not in header("hdlz_zip.h")                 # its "out of scope" sentence is as it was: the pointer stands in the new header


def test_the_struct_mirrors_match_the_header():
    from hdl_deflate_amd import _lib
    from hdl_deflate_amd.png import IMAGE_DTYPE
    text = header("hdlz_png.h")
    size = {"uint64_t": 8, "uint32_t": 4, "uint8_t": 1}

    def members(struct):
        body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (struct, struct), text, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        got = []
        for t, names in re.findall(r"(uint64_t|uint32_t|uint8_t)\s+([\w,\s\[\]]+);", body):
            for n in names.split(","):
                m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", n)
                got.append((t, m.group(1), size[t] * int(m.group(2) or 1)))
        return got
    for struct, mirror, total in (("hdlz_png_image", _lib.PngImage, 136), ("hdlz_png_index_result", _lib.PngIndexResult, 40),
                                  ("hdlz_png_decode_result", _lib.PngDecodeResult, 24)):
        m = members(struct)
        assert [n for _, n, _ in m] == [f[0] for f in mirror._fields_], struct
        assert [s for _, _, s in m] == [ctypes.sizeof(f[1]) for f in mirror._fields_], struct
        o = 0
        for t, n, s in m:                                   # (every member is naturally aligned where it stands: no padding)
            assert getattr(mirror, n).offset == o and o % size[t] == 0, (struct, n)
            o += s
        assert ctypes.sizeof(mirror) == o == total and total % 8 == 0, struct
    assert [(n, IMAGE_DTYPE.fields[n][1], IMAGE_DTYPE.fields[n][0].itemsize) for n in IMAGE_DTYPE.names] == \
        [(f[0], getattr(_lib.PngImage, f[0]).offset, ctypes.sizeof(f[1])) for f in _lib.PngImage._fields_]
    assert tuple(n for n in IMAGE_DTYPE.names if n != "reserved") == P.FIELDS


def test_the_queries_are_their_closed_forms():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    for n in (1, 2, 200, 4096, (1 << 31) - 1):
        for cap in (0, 1, n):
            assert L.hdlz_png_index_work_bytes(n, cap) == 256 + r256(24 * n)
    assert L.hdlz_png_index_work_bytes(0, 0) == 0 and L.hdlz_png_index_work_bytes(1 << 31, 0) == 0
    for count in (1, 2, 3, 200, 4096):
        for idat in (count, 7 * count, 300000):
            for zb in (16, 4096, 270016, (1 << 28) + 5):
                for rb in (16, 100, 32768, 270304, 1 << 26, (1 << 32) + 48):
                    d = r256(L.hdlz_inflate_work_bytes(1, min(zb, (1 << 28) - 1), min(rb & ~3, (1 << 32) - 512), 0, 1)) if count == 1 else 0
                    want = r256(32 * count) + r256(56 * count + 288) + r256(24 * (idat + 4 * count)) + r256(8 * (rb // 32768 + count)) + \
                        r256(zb) + r256(rb) + d
                    assert L.hdlz_png_decode_work_bytes(count, idat, zb, rb) == want, (count, idat, zb, rb)
    assert L.hdlz_png_decode_work_bytes(0, 0, 0, 0) == 0 and L.hdlz_png_decode_work_bytes(1 << 31, 1, 16, 16) == 0
    assert L.hdlz_png_decode_work_bytes(2, 1 << 40, 16, 16) == 0
    assert L.hdlz_png_decode_work_bytes(1, 1, 1 << 20, 1 << 22) > L.hdlz_png_decode_work_bytes(2, 1, 1 << 20, 1 << 22)      # the whole-GPU path's share


def _pairs(L, call, faults):
    for kw, word in faults:
        assert call(**kw) == E_BAD_PARAM and word in L.hdlz_last_error(), (kw, L.hdlz_last_error())
    for i, (kw_i, word_i) in enumerate(faults):              # ... and every pair: the earlier one answers
        for kw_j, _ in faults[i + 1:]:
            if set(kw_i) & set(kw_j):
                continue
            assert call(**dict(kw_j, **kw_i)) == E_BAD_PARAM and word_i in L.hdlz_last_error(), (kw_i, kw_j, L.hdlz_last_error())


def test_index_parameter_errors_come_before_the_device_in_their_order():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    keep, base = _host_buffer(1 << 16)
    wb = L.hdlz_png_index_work_bytes(3, 3)
    good = dict(files=base, files_len=1000, off=base + 2048, len=base + 2304, n=3, flags=1, align=64, cap=3, images=base + 4096, result=base + 8192,
                work=base + 16384, work_bytes=wb)

    def call(**kw):
        a = dict(good, **kw)
        return L.hdlz_png_index_ws(a["files"], a["files_len"], a["off"], a["len"], a["n"], a["flags"], a["align"], a["cap"], a["images"], a["result"],
                                   a["work"], a["work_bytes"], None)

    faults = [(dict(result=None), b"null device pointer"), (dict(images=None), b"d_images is null"), (dict(n=1 << 31), b"n too large"),
              (dict(cap=1 << 31), b"image_cap too large"), (dict(flags=2), b"flags must be"), (dict(align=3), b"out_align"),
              (dict(work_bytes=wb - 1), b"hdlz_png_index_work_bytes"), (dict(work=base + 16384 + 4), b"8-byte")]
    _pairs(L, call, faults)
    for kw in (dict(files=None), dict(off=None), dict(len=None)):
        assert call(**kw) == E_BAD_PARAM and b"null device pointer" in L.hdlz_last_error()
    for align in (0, 6, 512, 1 << 31):
        assert call(align=align) == E_BAD_PARAM and b"out_align" in L.hdlz_last_error()
    assert call(work=None) == E_BAD_PARAM and b"hdlz_png_index_work_bytes" in L.hdlz_last_error()
    for kw in (dict(off=base + 2052), dict(len=base + 2308), dict(images=base + 4100), dict(result=base + 8196)):
        assert call(**kw) == E_BAD_PARAM and b"8-byte" in L.hdlz_last_error()
    if _no_device():
        assert call() == E_HIP
        assert call(flags=0) == E_HIP and call(align=1) == E_HIP and call(align=256) == E_HIP
        assert call(cap=0, images=None) == E_HIP               # the sizing call
        assert call(n=0, files=None, off=None, len=None, work=None, work_bytes=0) == E_HIP
        assert call(files=base + 1) == E_HIP


def test_decode_parameter_errors_come_before_the_device_in_their_order():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    keep, base = _host_buffer(1 << 18)
    wb = L.hdlz_png_decode_work_bytes(2, 4, 4096, 8192)
    good = dict(files=base, files_len=1000, images=base + 4096, first=0, count=2, flags=1, idat=4, zb=4096, rb=8192, out=base + 8192, out_cap=4096,
                st=base + 16384, result=base + 16640, work=base + 20480, work_bytes=wb)

    def call(**kw):
        a = dict(good, **kw)
        return L.hdlz_png_decode_ws(a["files"], a["files_len"], a["images"], a["first"], a["count"], a["flags"], a["idat"], a["zb"], a["rb"], a["out"],
                                    a["out_cap"], a["st"], a["result"], a["work"], a["work_bytes"], None)

    faults = [(dict(result=None), b"d_result is required"), (dict(files=None), b"null device pointer"), (dict(out=None), b"d_out is null"),
              (dict(first=(1 << 31) - 1), b"first + count too large"), (dict(flags=7), b"flags must be"), (dict(idat=1 << 40), b"too large (below 2^40)"),
              (dict(images=base + 4100), b"d_images / d_result"), (dict(st=base + 16386), b"d_image_status"),
              (dict(work=base + 20480 + 128), b"256-byte"), (dict(work_bytes=wb - 1), b"hdlz_png_decode_work_bytes")]
    _pairs(L, call, faults)
    assert call(images=None) == E_BAD_PARAM and b"null device pointer" in L.hdlz_last_error()
    assert call(count=1 << 31) == E_BAD_PARAM and b"first + count too large" in L.hdlz_last_error()
    for kw in (dict(zb=1 << 40), dict(rb=1 << 40)):
        assert call(**kw) == E_BAD_PARAM and b"too large (below 2^40)" in L.hdlz_last_error()
    assert call(result=base + 16644) == E_BAD_PARAM and b"8-byte" in L.hdlz_last_error()
    assert call(work=None) == E_BAD_PARAM and b"hdlz_png_decode_work_bytes" in L.hdlz_last_error()
    assert call(result=None, count=0, work=None, work_bytes=0) == E_BAD_PARAM                 # required, always
    if _no_device():
        assert call() == E_HIP
        assert call(st=None) == E_HIP and call(flags=0) == E_HIP                              # nullable; RAW
        assert call(out=None, out_cap=0) == E_HIP and call(out=base + 8193) == E_HIP          # slots at any alignment
        assert call(count=0, files=None, images=None, work=None, work_bytes=0) == E_HIP
        one = L.hdlz_png_decode_work_bytes(1, 4, 4096, 8192)
        assert one > wb and call(count=1, work_bytes=one) == E_HIP and call(count=1, work_bytes=wb) == E_BAD_PARAM
        assert call(first=7, count=1, work_bytes=one) == E_HIP


# ---- the rule and the pixels against Pillow
GRID = [(c, d, w, h) for c, d in P.PAIRS for w, h in ((1, 1), (5, 3), (67, 66))]


@pytest.mark.parametrize("colour,depth,width,height", GRID)
def test_png_ref_reads_images_as_pillow_does(colour, depth, width, height):
    """random filters, 7-byte IDATs; palette images with a tRNS shorter than the palette.  Pillow reduces 16-bit RGB and RGBA to 8 bits:
    those are held against the encoder's own pixels only"""
    Image = pytest.importorskip("PIL.Image")
    seed = colour * 1000 + depth * 10 + width
    rng = np.random.default_rng(seed)
    rows = P.random_rows(width, height, colour, depth, seed)
    trns = bytes(rng.integers(0, 256, min(3, 1 << depth), dtype=np.uint8)) if colour == 3 and width > 1 else None
    f = P.make_png(width, height, colour, depth, rows=rows, filters=list(rng.integers(0, 5, height)), idat=7, trns=trns, seed=seed)
    ix, sts, outs = P.read([f])
    rec = ix["images"][0]
    assert sts == [P.OK] and rec["nidat"] == -(-rec["zlen"] // 7) and rec["used"] == len(f)
    assert P.read([f], P.RAW)[2][0] == rows                   # the unfilter undoes the encoder's filter
    got = np.frombuffer(outs[0], np.uint16 if depth == 16 else np.uint8).reshape(P.shape_of(rec))
    if depth == 16 and colour != 0:
        want = np.frombuffer(rows, ">u2").reshape(got.shape)
        assert (got == want).all()
        return
    im = Image.open(io.BytesIO(f))
    im.load()
    if colour == 3:
        im = im.convert("RGBA" if trns is not None else "RGB")
    want = np.asarray(im)
    if colour == 0 and depth < 8 and im.mode == "1":
        want = want.astype(np.uint8) * 255
    elif colour == 0 and depth < 8 and want.max(initial=0) < (1 << depth) and im.mode != "L":
        want = want.astype(np.uint8) * (255 // ((1 << depth) - 1))
    assert got.shape == want.shape and (got == want.astype(got.dtype)).all(), (im.mode, got.ravel()[:8], want.ravel()[:8])


def test_pillow_renders_an_out_of_range_palette_index_black():
    Image = pytest.importorskip("PIL.Image")
    rows = bytes([0, 1, 2, 3, 7, 200])
    f = P.make_png(6, 1, 3, 8, rows=rows, palette=bytes(range(30, 39)))       # three entries
    _, sts, outs = P.read([f])
    got = np.frombuffer(outs[0], np.uint8).reshape(1, 6, 3)
    assert sts == [P.OK] and (got[0, 3:] == 0).all() and got[0, 1].tolist() == [33, 34, 35]
    assert (np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) == got).all()


def test_the_rule_on_crafted_files_and_the_capacity_call():
    good = P.make_png(5, 3, 2, 8, seed=1)
    assert P.index([good])["images"][0]["status"] == P.OK
    assert P.index([good[:20]])["images"][0]["status"] == P.E_NO_EOF and P.index([b"x" + good[1:]])["images"][0]["status"] == P.E_BAD_HEADER
    assert P.index([P.make_png(5, 3, 2, 8, interlace=1)])["images"][0]["status"] == P.E_BAD_BTYPE
    assert P.index([P.make_png(5, 3, 2, 8, extra=[("front", b"ABCD", b"")])])["images"][0]["status"] == P.E_BAD_BTYPE
    assert P.index([P.make_png(5, 3, 2, 8, extra=[("front", b"abCD", b"xyz"), ("back", b"tEXt", b"k\0v")])])["images"][0]["status"] == P.OK
    files = [good, good[:30], P.make_png(9, 9, 0, 1, seed=2)]
    full = P.index(files)
    assert [r["status"] for r in full["images"]] == [P.OK, P.E_NO_EOF, P.OK] and full["images"][1]["out_off"] == full["images"][2]["out_off"] == 64
    for cap in (0, 2):
        ix = P.index(files, image_cap=cap)
        assert ix["status"] == P.E_OUT_CAPACITY and len(ix["images"]) == cap and ix["total_out"] == full["total_out"] == 64 + 81
