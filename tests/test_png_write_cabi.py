"""CPU: the extension header include/hdlz_png_write.h -- every declaration exported and bound with its arity, the tables in front of it
and the version as they were, the mirrors of the two structs, the size queries equal to their closed forms, every parameter refusal in
the header's order and in front of the device; and the two rules as tests/png_write_ref.py states them: the crafted rows hold what they
claim, the files are read by Pillow (where it is installed) and by the reader's rule of tests/png_ref.py, for the 8 pairs on 1x1, 5x3
and 67x66 images."""
import ctypes
import io
import re

import numpy as np
import pytest

import png_ref as P
import png_write_ref as W
from cabi_common import declarations, header, host_buffer as _host_buffer, no_device as _no_device
from test_png_cabi import _pairs

E_BAD_PARAM, E_HIP = 8, 9


def test_every_declaration_is_exported_and_bound():
    from hdl_deflate_amd import _lib
    text = header("hdlz_png_write.h")
    params = declarations(text)
    assert params == {"hdlz_png_filter_work_bytes": 1, "hdlz_png_filter_ws": 14, "hdlz_png_write_bound": 5, "hdlz_png_write_work_bytes": 2,
                      "hdlz_png_write_ws": 26}
    assert sorted(params) == sorted(_lib.PNG_WRITE_EXPORTS) == sorted(_lib.PNG_WRITE_CALLS)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    L = _lib.load()
    for name, n in params.items():
        assert hasattr(raw, name), name
        restype, argtypes = _lib.PNG_WRITE_CALLS[name]
        assert len(argtypes) == n, name
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert '#include "hdlz_png.h"' in text and '#include "hdlz_join.h"' in text and "Not there" in text
    k = W.kernel_constants()
    assert (int(re.search(r"#define\s+HDLZ_PNG_FILTER_ADAPTIVE\s+(\d+)u", text).group(1)), k.BAND, k.STEP, k.ROW_REG_MAX) == \
        (_lib.PNG_FILTER_ADAPTIVE, _lib.PNGW_BAND, _lib.PNGW_STEP, _lib.PNGW_ROW_REG_MAX) and _lib.PNG_FILTER_ADAPTIVE == W.ADAPTIVE
    import hdl_deflate_amd
    from hdl_deflate_amd.engine import Engine
    assert callable(hdl_deflate_amd.save_png) and callable(Engine.encode_png)


def test_the_tables_in_front_of_it_are_as_they_were():
    from hdl_deflate_amd import _lib
    older = (_lib.EXPORTS, _lib.JOIN_EXPORTS, _lib.UNJOIN_EXPORTS, _lib.GZIP_EXPORTS, _lib.BGZF_EXPORTS, _lib.BGZF_RANGE_EXPORTS, _lib.BGZF_STORED_EXPORTS,
             _lib.GUNZIP_EXPORTS, _lib.ZIP_EXPORTS, _lib.ZIP_WRITE_EXPORTS, _lib.ZIP64_EXPORTS, _lib.GZIP_MEMBERS_EXPORTS, _lib.SEEK_EXPORTS, _lib.PNG_EXPORTS)
    assert [len(t) for t in older] == [22, 4, 2, 7, 8, 2, 3, 2, 4, 3, 7, 4, 4, 4]
    assert len(_lib.PNG_WRITE_EXPORTS) == 5 and not set(_lib.PNG_WRITE_EXPORTS) & set().union(*older)
    assert not [n for n in dir(_lib) if n.endswith("SIGNATURES") and "PNG" in n]
    assert _lib.load().hdlz_version() == 0x000600
    assert declarations(header("hdlz_png.h")) == {"hdlz_png_index_work_bytes": 2, "hdlz_png_index_ws": 13, "hdlz_png_decode_work_bytes": 4,
                                                  "hdlz_png_decode_ws": 16}


def test_the_struct_mirrors_match_the_header():
    from hdl_deflate_amd import _lib
    from hdl_deflate_amd.png import SPEC_DTYPE
    text = header("hdlz_png_write.h")
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
    for struct, mirror, total in (("hdlz_png_spec", _lib.PngSpec, 24), ("hdlz_png_write_result", _lib.PngWriteResult, 24)):
        m = members(struct)
        assert [n for _, n, _ in m] == [f[0] for f in mirror._fields_], struct
        assert [s for _, _, s in m] == [ctypes.sizeof(f[1]) for f in mirror._fields_], struct
        o = 0
        for t, n, s in m:                                   # (every member is naturally aligned where it stands: no padding)
            assert getattr(mirror, n).offset == o and o % size[t] == 0, (struct, n)
            o += s
        assert ctypes.sizeof(mirror) == o == total, struct
    assert [(n, SPEC_DTYPE.fields[n][1], SPEC_DTYPE.fields[n][0].itemsize) for n in SPEC_DTYPE.names] == \
        [(f[0], getattr(_lib.PngSpec, f[0]).offset, ctypes.sizeof(f[1])) for f in _lib.PngSpec._fields_]


def test_the_queries_are_their_closed_forms():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    for n in (1, 2, 31, 32, 200, 4096, (1 << 31) - 1):
        assert L.hdlz_png_filter_work_bytes(n) == W.filter_work_bytes(n)
        for B in (0, 1, 31, 255, 256, 70000, (1 << 31) - 1):
            assert L.hdlz_png_write_work_bytes(n, B) == W.write_work_bytes(n, B), (n, B)
    assert L.hdlz_png_filter_work_bytes(0) == 0 and L.hdlz_png_filter_work_bytes(1 << 31) == 0
    assert L.hdlz_png_write_work_bytes(0, 0) == 0 and L.hdlz_png_write_work_bytes(1 << 31, 0) == 0 and L.hdlz_png_write_work_bytes(1, 1 << 31) == 0
    for n, B, block, idat in ((0, 0, 65536, 65536), (1, 0, 32, 1), (1, 1, 64, 7), (3, 40, 65536, 65536), (4096, 4096, 65536, 8192), (1, 1024, 65536, 1 << 30)):
        assert L.hdlz_png_write_bound(n, 12345, B, block, idat) == W.bound(n, B, block, idat), (n, B, block, idat)
    assert L.hdlz_png_write_bound(1, 5, 1, 64, 0) == 0


def test_filter_parameter_errors_come_before_the_device_in_their_order():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    keep, base = _host_buffer(1 << 16)
    wb = L.hdlz_png_filter_work_bytes(3)
    good = dict(pix=base, pix_len=1000, specs=base + 2048, n=3, mode=5, rows=30, raw=base + 4096, raw_cap=2000, rf=base + 8192, st=base + 8448,
                raw_off=base + 8704, work=base + 16384, work_bytes=wb)

    def call(**kw):
        a = dict(good, **kw)
        return L.hdlz_png_filter_ws(a["pix"], a["pix_len"], a["specs"], a["n"], a["mode"], a["rows"], a["raw"], a["raw_cap"], a["rf"], a["st"],
                                    a["raw_off"], a["work"], a["work_bytes"], None)

    faults = [(dict(specs=None), b"null device pointer"), (dict(pix=None), b"d_pix is null"), (dict(raw=None), b"d_raw is null"),
              (dict(n=1 << 31), b"n too large"), (dict(mode=6), b"mode must be"), (dict(rows=1 << 40), b"total_rows too large"),
              (dict(work_bytes=wb - 1), b"hdlz_png_filter_work_bytes"), (dict(raw_off=base + 8708), b"8-byte"), (dict(st=base + 8450), b"4-byte")]
    _pairs(L, call, faults)
    for kw in (dict(st=None), dict(raw_off=None)):
        assert call(**kw) == E_BAD_PARAM and b"null device pointer" in L.hdlz_last_error()
    assert call(work=None) == E_BAD_PARAM and b"hdlz_png_filter_work_bytes" in L.hdlz_last_error()
    for kw in (dict(specs=base + 2052), dict(work=base + 16388)):
        assert call(**kw) == E_BAD_PARAM and b"8-byte" in L.hdlz_last_error()
    if _no_device():
        assert call() == E_HIP
        assert call(rf=None) == E_HIP and call(mode=0) == E_HIP and call(rows=0) == E_HIP           # nullable; a fixed filter; any total_rows
        assert call(raw=None, raw_cap=0) == E_HIP                                                  # the sizing call
        assert call(pix=base + 1, raw=base + 4097) == E_HIP                                        # bytes at any alignment
        assert call(n=0, specs=None, st=None, raw_off=None, work=None, work_bytes=0) == E_HIP


def test_write_parameter_errors_come_before_the_device_in_their_order():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    keep, base = _host_buffer(1 << 17)
    wb = L.hdlz_png_write_work_bytes(3, 5)
    good = dict(specs=base, n=3, raw=base + 256, raw_off=base + 1024, fst=base + 1280, in_off=base + 1536, rows=base + 2048, pitch=100, len=base + 4096,
                end_bits=base + 4352, st=base + 4608, B=5, blk_first=base + 4864, idat=65536, flags=1, align=64, file=base + 8192, cap=4096,
                file_off=base + 12544, file_len=base + 12800, ist=base + 13056, images=base + 13312, result=base + 16384, work=base + 32768, work_bytes=wb)

    def call(**kw):
        a = dict(good, **kw)
        return L.hdlz_png_write_ws(a["specs"], a["n"], a["raw"], a["raw_off"], a["fst"], a["in_off"], a["rows"], a["pitch"], a["len"], a["end_bits"],
                                   a["st"], a["B"], a["blk_first"], a["idat"], a["flags"], a["align"], a["file"], a["cap"], a["file_off"], a["file_len"],
                                   a["ist"], a["images"], a["result"], a["work"], a["work_bytes"], None)

    faults = [(dict(result=None), b"d_result is required"), (dict(n=1 << 31), b"n too large"), (dict(B=1 << 31), b"nblocks too large"),
              (dict(specs=None), b"(the images)"), (dict(rows=None), b"(the rows)"), (dict(file=None), b"d_file is null"),
              (dict(idat=0), b"idat_len"), (dict(flags=2), b"flags must be"), (dict(align=3), b"out_align"),
              (dict(work_bytes=wb - 1), b"hdlz_png_write_work_bytes"), (dict(images=base + 13316), b"8-byte"), (dict(ist=base + 13058), b"4-byte")]
    _pairs(L, call, faults)
    assert call(n=0) == E_BAD_PARAM and b"rows without images" in L.hdlz_last_error()
    for kw in (dict(raw_off=None), dict(blk_first=None), dict(file_off=None), dict(file_len=None)):
        assert call(**kw) == E_BAD_PARAM and b"(the images)" in L.hdlz_last_error()
    for kw in (dict(in_off=None), dict(len=None), dict(end_bits=None), dict(st=None)):
        assert call(**kw) == E_BAD_PARAM and b"(the rows)" in L.hdlz_last_error()
    assert call(idat=1 << 31) == E_BAD_PARAM and b"idat_len" in L.hdlz_last_error()
    for align in (0, 6, 512):
        assert call(align=align) == E_BAD_PARAM and b"out_align" in L.hdlz_last_error()
    assert call(work=None) == E_BAD_PARAM and b"hdlz_png_write_work_bytes" in L.hdlz_last_error()
    for kw in (dict(specs=base + 4), dict(raw_off=base + 1028), dict(in_off=base + 1540), dict(end_bits=base + 4356), dict(blk_first=base + 4868),
               dict(file_off=base + 12548), dict(file_len=base + 12804), dict(result=base + 16388), dict(work=base + 32772)):
        assert call(**kw) == E_BAD_PARAM and b"8-byte" in L.hdlz_last_error(), kw
    for kw in (dict(len=base + 4098), dict(st=base + 4610), dict(fst=base + 1282)):
        assert call(**kw) == E_BAD_PARAM and b"4-byte" in L.hdlz_last_error(), kw
    if _no_device():
        assert call() == E_HIP
        assert call(fst=None) == E_HIP and call(ist=None) == E_HIP and call(images=None) == E_HIP and call(raw=None) == E_HIP      # the nullable ones
        assert call(file=None, cap=0) == E_HIP                                                       # the sizing call
        assert call(flags=0, align=1, idat=1) == E_HIP and call(idat=(1 << 31) - 1, align=256) == E_HIP
        assert call(file=base + 8193, rows=base + 2049, raw=base + 257) == E_HIP                     # bytes at any alignment
        none = dict(B=0, in_off=None, rows=None, len=None, end_bits=None, st=None)
        assert call(work_bytes=L.hdlz_png_write_work_bytes(3, 0), **none) == E_HIP
        assert call(n=0, specs=None, raw_off=None, blk_first=None, file_off=None, file_len=None, work=None, work_bytes=0, **none) == E_HIP


# ---- the rules
def test_the_crafted_rows_hold_what_they_claim():
    strict, ties = W.crafted_properties()
    assert strict == {0, 1, 2, 3, 4} and {(0, 1), (1, 2), (2, 3), (3, 4)} <= ties


def test_the_sums_are_python_integers_and_the_stored_form_is_zlib():
    import zlib
    wide = np.full((1, 70000), 128, np.uint8)                    # S_0 = 70000 * 128: past 2^23, summed without a width
    assert W.row_sums(wide.tobytes(), 1, 70000, 1)[0][0] == 70000 * 128
    for n in (2, 3, 4):
        s = bytes(range(n))
        assert zlib.decompress(W.zstream(s, 64)) == s and len(W.zstream(s, 64)) == 11 + n
    s = bytes(range(5))
    assert zlib.decompress(W.zstream(s, 64)) == s and W.zstream(s, 64)[:2] == b"\x78\x9c" and W.zstream(s, 64)[2] & 7 == 2      # a fixed block, not final


GRID = [(c, d, w, h) for c, d in W.PAIRS for w, h in ((1, 1), (5, 3), (67, 66))]


def _pixels(colour, depth, width, height):
    shape, dtype = W.shape_for(colour, depth, width, height)
    seed = colour * 1000 + depth * 10 + width
    return W.smooth(shape, dtype, seed) if width > 1 else W.noise(shape, dtype, seed)


@pytest.mark.parametrize("colour,depth,width,height", GRID)
def test_the_reference_files_are_read_back_by_png_ref(colour, depth, width, height):
    pix = _pixels(colour, depth, width, height)
    for mode, idat in ((W.ADAPTIVE, 1 << 16), (4, 7)):
        w = W.expected(pix, mode=mode, block=64, idat=idat)
        ix, sts, outs = P.read([w.file])
        rec = ix["images"][0]
        assert sts == [P.OK] and rec["nidat"] == -(-len(w.z) // idat) and rec["used"] == len(w.file) and rec["idat_off"] == 33
        assert outs[0] == pix.tobytes() and P.shape_of(rec) == pix.shape
        assert P.read([w.file], P.RAW)[2][0] == W.scanlines(pix)[0]
        assert [w.stream[r * (rec["row_bytes"] + 1)] for r in range(height)] == w.filters


@pytest.mark.parametrize("colour,depth,width,height", GRID)
def test_the_reference_files_are_read_by_pillow(colour, depth, width, height):
    """Pillow reduces 16-bit RGB, RGBA and grey + alpha to 8 bits: those are held to the high bytes"""
    Image = pytest.importorskip("PIL.Image")
    pix = _pixels(colour, depth, width, height)
    w = W.expected(pix, block=64, idat=7)
    im = Image.open(io.BytesIO(w.file))
    im.load()
    if depth == 16 and colour != 0:
        got = np.asarray(im.convert({2: "RGB", 4: "LA", 6: "RGBA"}[colour]))
        assert got.shape == pix.shape and (got == (pix >> 8)).all(), (im.mode, got.ravel()[:8], pix.ravel()[:8])
        return
    got = np.asarray(im)
    assert got.shape == pix.shape and (got.astype(pix.dtype) == pix).all(), (im.mode, got.ravel()[:8], pix.ravel()[:8])


def test_the_ratio_condition_of_the_ramp():
    a, z = W.expected(W.ramp()), W.expected(W.ramp(), mode=0)
    assert (len(a.z), len(z.z)) == (7570, 51918) and 2 * len(a.file) < len(z.file)
