"""CPU: the extension header include/hdlz_tiff.h -- every declaration exported and bound with its arity, the tables in front of it and
the version as they were, the mirrors of the three structs, both work-bytes queries equal to their closed forms, every parameter refusal
in the header's order and in front of the device."""
import ctypes
import re

import tiff_ref as T
from cabi_common import declarations, header, host_buffer as _host_buffer, no_device as _no_device, r256
from test_png_cabi import _pairs

E_BAD_PARAM, E_HIP = 8, 9


def test_every_declaration_is_exported_and_bound():
    from hdl_deflate_amd import _lib
    text = header("hdlz_tiff.h")
    params = declarations(text)
    assert params == {"hdlz_tiff_index_work_bytes": 2, "hdlz_tiff_index_ws": 13, "hdlz_tiff_decode_work_bytes": 3, "hdlz_tiff_decode_ws": 14}
    assert sorted(params) == sorted(_lib.TIFF_EXPORTS) == sorted(_lib.TIFF_CALLS)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    L = _lib.load()
    for name, n in params.items():
        assert hasattr(raw, name), name
        restype, argtypes = _lib.TIFF_CALLS[name]
        assert len(argtypes) == n, name
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert '#include "hdlz_png.h"' in text and "Not there" in text
    assert int(re.search(r"#define\s+HDLZ_TIFF_LARGE_MIN\s+(\d+)u", text).group(1)) == _lib.TIFF_LARGE_MIN == _lib.PNG_LARGE_MIN == T.LARGE_MIN
    import hdl_deflate_amd
    from hdl_deflate_amd.engine import Engine
    assert callable(hdl_deflate_amd.load_tiff) and hdl_deflate_amd.TiffIndex is not None and callable(Engine.tiff_index) and callable(Engine.decode_tiff)


def test_the_tables_in_front_of_it_are_as_they_were():
    from hdl_deflate_amd import _lib
    older = (_lib.EXPORTS, _lib.JOIN_EXPORTS, _lib.UNJOIN_EXPORTS, _lib.GZIP_EXPORTS, _lib.BGZF_EXPORTS, _lib.BGZF_RANGE_EXPORTS, _lib.BGZF_STORED_EXPORTS,
             _lib.GUNZIP_EXPORTS, _lib.ZIP_EXPORTS, _lib.ZIP_WRITE_EXPORTS, _lib.ZIP64_EXPORTS, _lib.GZIP_MEMBERS_EXPORTS, _lib.SEEK_EXPORTS, _lib.PNG_EXPORTS,
             _lib.PNG_WRITE_EXPORTS)
    assert [len(t) for t in older] == [22, 4, 2, 7, 8, 2, 3, 2, 4, 3, 7, 4, 4, 4, 5]
    assert len(_lib.TIFF_EXPORTS) == 4 and not set(_lib.TIFF_EXPORTS) & set().union(*older)
    assert not [n for n in dir(_lib) if n.endswith("SIGNATURES") and "TIFF" in n]
    assert _lib.load().hdlz_version() == 0x000600
    assert "TIFF" not in header("hdlz_png.h") and "TIFF" not in header("hdlz_zip.h")      # additive: the pointer stands in the new header
    assert declarations(header("hdlz_png.h")) == {"hdlz_png_index_work_bytes": 2, "hdlz_png_index_ws": 13, "hdlz_png_decode_work_bytes": 4,
                                                  "hdlz_png_decode_ws": 16}


def test_the_struct_mirrors_match_the_header():
    from hdl_deflate_amd import _lib
    from hdl_deflate_amd.tiff import IMAGE_DTYPE
    text = header("hdlz_tiff.h")
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
    for struct, mirror, total in (("hdlz_tiff_image", _lib.TiffImage, 136), ("hdlz_tiff_index_result", _lib.TiffIndexResult, 40),
                                  ("hdlz_tiff_decode_result", _lib.TiffDecodeResult, 24)):
        m = members(struct)
        assert [n for _, n, _ in m] == [f[0] for f in mirror._fields_], struct
        assert [s for _, _, s in m] == [ctypes.sizeof(f[1]) for f in mirror._fields_], struct
        o = 0
        for t, n, s in m:                                   # (every member is naturally aligned where it stands: no padding)
            assert getattr(mirror, n).offset == o and o % size[t] == 0, (struct, n)
            o += s
        assert ctypes.sizeof(mirror) == o == total and total % 8 == 0, struct
        assert sorted((size[t] for t, _, _ in m), reverse=True) == [size[t] for t, _, _ in m], struct      # the 8-byte fields first
    assert [(n, IMAGE_DTYPE.fields[n][1], IMAGE_DTYPE.fields[n][0].itemsize) for n in IMAGE_DTYPE.names] == \
        [(f[0], getattr(_lib.TiffImage, f[0]).offset, ctypes.sizeof(f[1])) for f in _lib.TiffImage._fields_]
    assert tuple(n for n in IMAGE_DTYPE.names if n != "reserved") == T.FIELDS


def test_the_queries_are_their_closed_forms():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    for n in (1, 2, 200, 4096, (1 << 31) - 1):
        for cap in (0, 1, n):
            assert L.hdlz_tiff_index_work_bytes(n, cap) == 256 + r256(24 * n) == T.index_work_bytes(n)
    assert L.hdlz_tiff_index_work_bytes(0, 0) == 0 and L.hdlz_tiff_index_work_bytes(1 << 31, 0) == 0
    for count in (1, 2, 3, 200, 4096):
        for chunks in (0, 1, count, 16 * count, 300000, (1 << 31) - 1):
            for rb in (0, 16, 100, 32768, 270304, 1 << 26, (1 << 32) + 48):
                assert L.hdlz_tiff_decode_work_bytes(count, chunks, rb) == T.decode_work_bytes(L, count, chunks, rb), (count, chunks, rb)
    assert L.hdlz_tiff_decode_work_bytes(0, 0, 0) == 0 and L.hdlz_tiff_decode_work_bytes(1 << 31, 1, 16) == 0
    assert L.hdlz_tiff_decode_work_bytes(2, 1 << 31, 16) == 0 and L.hdlz_tiff_decode_work_bytes(2, 2, 1 << 40) == 0
    assert L.hdlz_tiff_decode_work_bytes(1, 1, 1 << 22) > L.hdlz_tiff_decode_work_bytes(1, 2, 1 << 22)      # the whole-GPU path's share


def test_index_parameter_errors_come_before_the_device_in_their_order():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    keep, base = _host_buffer(1 << 16)
    wb = L.hdlz_tiff_index_work_bytes(3, 3)
    good = dict(files=base, files_len=1000, off=base + 2048, len=base + 2304, page=base + 2560, n=3, align=64, cap=3, images=base + 4096, result=base + 8192,
                work=base + 16384, work_bytes=wb)

    def call(**kw):
        a = dict(good, **kw)
        return L.hdlz_tiff_index_ws(a["files"], a["files_len"], a["off"], a["len"], a["page"], a["n"], a["align"], a["cap"], a["images"], a["result"],
                                    a["work"], a["work_bytes"], None)

    faults = [(dict(result=None), b"null device pointer"), (dict(images=None), b"d_images is null"), (dict(n=1 << 31), b"n too large"),
              (dict(cap=1 << 31), b"image_cap too large"), (dict(align=3), b"out_align"),
              (dict(work_bytes=wb - 1), b"hdlz_tiff_index_work_bytes"), (dict(work=base + 16384 + 4), b"8-byte"), (dict(page=base + 2562), b"d_page")]
    _pairs(L, call, faults)
    for kw in (dict(files=None), dict(off=None), dict(len=None)):
        assert call(**kw) == E_BAD_PARAM and b"null device pointer" in L.hdlz_last_error()
    for align in (0, 6, 512, 1 << 31):
        assert call(align=align) == E_BAD_PARAM and b"out_align" in L.hdlz_last_error()
    assert call(work=None) == E_BAD_PARAM and b"hdlz_tiff_index_work_bytes" in L.hdlz_last_error()
    for kw in (dict(off=base + 2052), dict(len=base + 2308), dict(images=base + 4100), dict(result=base + 8196)):
        assert call(**kw) == E_BAD_PARAM and b"8-byte" in L.hdlz_last_error()
    if _no_device():
        assert call() == E_HIP
        assert call(page=None) == E_HIP and call(align=1) == E_HIP and call(align=256) == E_HIP      # nullable: page 0 of every file
        assert call(cap=0, images=None) == E_HIP               # the sizing call
        assert call(n=0, files=None, off=None, len=None, page=None, work=None, work_bytes=0) == E_HIP
        assert call(files=base + 1) == E_HIP


def test_decode_parameter_errors_come_before_the_device_in_their_order():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    keep, base = _host_buffer(1 << 18)
    wb = L.hdlz_tiff_decode_work_bytes(2, 4, 8192)
    good = dict(files=base, files_len=1000, images=base + 4096, first=0, count=2, chunks=4, rb=8192, out=base + 8192, out_cap=4096,
                st=base + 16384, result=base + 16640, work=base + 20480, work_bytes=wb)

    def call(**kw):
        a = dict(good, **kw)
        return L.hdlz_tiff_decode_ws(a["files"], a["files_len"], a["images"], a["first"], a["count"], a["chunks"], a["rb"], a["out"],
                                     a["out_cap"], a["st"], a["result"], a["work"], a["work_bytes"], None)

    faults = [(dict(result=None), b"d_result is required"), (dict(files=None), b"null device pointer"), (dict(out=None), b"d_out is null"),
              (dict(first=(1 << 31) - 1), b"first + count too large"), (dict(chunks=1 << 31), b"chunk_cap (below 2^31)"),
              (dict(images=base + 4100), b"d_images / d_result"), (dict(st=base + 16386), b"d_image_status"),
              (dict(work=base + 20480 + 128), b"256-byte"), (dict(work_bytes=wb - 1), b"hdlz_tiff_decode_work_bytes")]
    _pairs(L, call, faults)
    assert call(images=None) == E_BAD_PARAM and b"null device pointer" in L.hdlz_last_error()
    assert call(count=1 << 31) == E_BAD_PARAM and b"first + count too large" in L.hdlz_last_error()
    assert call(rb=1 << 40) == E_BAD_PARAM and b"raw_bytes (below 2^40)" in L.hdlz_last_error()
    assert call(result=base + 16644) == E_BAD_PARAM and b"8-byte" in L.hdlz_last_error()
    assert call(work=None) == E_BAD_PARAM and b"hdlz_tiff_decode_work_bytes" in L.hdlz_last_error()
    assert call(result=None, count=0, work=None, work_bytes=0) == E_BAD_PARAM                 # required, always
    if _no_device():
        assert call() == E_HIP
        assert call(st=None) == E_HIP                                                         # nullable
        assert call(out=None, out_cap=0) == E_HIP and call(out=base + 8193) == E_HIP          # slots at any alignment
        assert call(count=0, files=None, images=None, work=None, work_bytes=0) == E_HIP
        one = L.hdlz_tiff_decode_work_bytes(1, 1, 8192)
        assert one > L.hdlz_tiff_decode_work_bytes(1, 2, 8192) and call(count=1, chunks=1, work_bytes=one) == E_HIP
        assert call(count=1, chunks=1, work_bytes=L.hdlz_tiff_decode_work_bytes(1, 2, 8192)) == E_BAD_PARAM
        assert call(first=7, count=1, chunks=1, work_bytes=one) == E_HIP
