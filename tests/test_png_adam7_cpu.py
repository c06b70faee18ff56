"""CPU: HDLZ_PNG_ADAM7 of include/hdlz_png.h.  The reference for interlaced images (tests/png_adam7_ref.py: the pass geometry, the encoder
make_adam7, the sizes and the pixels under flags & 4) held against Pillow for every (colour, depth) pair at the sizes where passes vanish;
and, without a device, the flag in the header, in _lib and in the parameter checks of both calls: 4 and 5 pass them as 0 and 1 do, every
other value is refused."""
import io
import re

import numpy as np
import pytest

import png_ref as P
import png_adam7_ref as A
from cabi_common import header, host_buffer as _host_buffer, no_device as _no_device

E_BAD_PARAM, E_HIP = 8, 9
SIZES = [(1, 1), (2, 3), (3, 2), (4, 5), (5, 4), (8, 8), (9, 9), (13, 11), (33, 17)]


def test_the_pass_geometry():
    """every pixel lies in exactly one pass, at the place the pass's origin and step give; the sums the header states"""
    for w, h in SIZES + [(1, 9), (9, 1), (5, 1), (1, 5)]:
        seen = np.zeros((h, w), int)
        for x0, y0, dx, dy, pw, ph, prb in A.passes_of(w, h, 2, 8):
            assert pw == len(range(x0, w, dx)) and ph == len(range(y0, h, dy)) and prb == 3 * pw
            seen[y0::dy, x0::dx] += 1
        assert (seen == 1).all()
    assert [g[:4] for g in A.passes_of(1, 1, 0, 8)] == [A.PASSES[0]] and A.raw_len_of(1, 1, 0, 1) == 2
    assert A.raw_len_of(8, 8, 0, 8) == 2 + 2 + 3 + 2 * 3 + 2 * 5 + 4 * 5 + 4 * 9 and A.total_rows(8, 8) == 15
    assert A.raw_len_of(8, 8, 0, 1) == 15 * 2 and P.sizes_of(8, 8, 1, 0, False, 0)[1] == 16      # the two lengths differ


@pytest.mark.parametrize("width,height", SIZES)
@pytest.mark.parametrize("colour,depth", P.PAIRS)
def test_the_reference_reads_interlaced_images_as_pillow_does(colour, depth, width, height):
    """random filters per row of every pass, 7-byte IDATs, a tRNS shorter than the palette: Pillow sees an interlaced file with the
    pixels of the plain file of the same scanlines, and the reference's decode equals png_ref's of that file in both modes.  (Pillow
    reduces 16-bit RGB and RGBA to 8 bits: the two Pillow images are compared with each other.)"""
    Image = pytest.importorskip("PIL.Image")
    seed = colour * 1000 + depth * 10 + width
    rng = np.random.default_rng(seed)
    rows = P.random_rows(width, height, colour, depth, seed)
    trns = bytes(rng.integers(0, 256, min(3, 1 << depth), dtype=np.uint8)) if colour == 3 and width > 1 else None
    kw = dict(rows=rows, idat=7, trns=trns, seed=seed)
    plain = P.make_png(width, height, colour, depth, filters=list(rng.integers(0, 5, height)), **kw)
    laced = A.make_adam7(width, height, colour, depth, filters=list(rng.integers(0, 5, A.total_rows(width, height))), **kw)
    a, b = Image.open(io.BytesIO(laced)), Image.open(io.BytesIO(plain))
    a.load()
    b.load()
    assert a.info["interlace"] == 1 and not b.info.get("interlace")
    assert a.mode == b.mode and a.size == b.size and (np.asarray(a) == np.asarray(b)).all()
    for flags in (P.EXPAND, P.RAW):
        ix, sts, outs = A.read([laced], flags | A.ADAM7)
        rec, ref = ix["images"][0], P.read([plain], flags)
        assert sts == [P.OK] and outs[0] == ref[2][0] and (outs[0] == rows or flags == P.EXPAND)
        want = dict(ref[0]["images"][0], interlace=1, raw_len=A.raw_len_of(width, height, colour, depth), zlen=rec["zlen"], nidat=rec["nidat"],
                    used=rec["used"], file_len=len(laced))
        assert rec == want, {n: (rec[n], want[n]) for n in rec if rec[n] != want[n]}
        assert A.read([laced], flags)[1] == [P.E_BAD_BTYPE]                       # without the flag: the old refusal
        assert A.decode(laced, rec, flags) == (P.E_BAD_PARAM, None)


def test_the_reference_on_crafted_interlaced_files():
    """interlace 2; a stream one row short; a plain stream under an interlaced IHDR; filter byte 5 in a row of pass 4; the limit"""
    import struct
    import zlib
    assert A.index([P.make_png(5, 3, 2, 8, interlace=2)])["images"][0]["status"] == P.E_BAD_HEADER
    rows = P.random_rows(9, 9, 2, 8, 1)
    stream = A.adam7_stream(9, 9, 2, 8, rows, 1)
    last = 1 + 3 * 9                                              # pass 7's row
    short = P.make_png(9, 9, 2, 8, interlace=1, stream=zlib.compress(stream[:-last]))
    assert A.read([short])[1] == [P.E_BAD_CHECKSUM]
    plain = P.make_png(9, 9, 2, 8, rows=rows, ihdr=struct.pack(">IIBBBBB", 9, 9, 8, 2, 0, 0, 1))
    assert A.raw_len_of(9, 9, 2, 8) > 9 * 28 and A.read([plain])[1] == [P.E_BAD_CHECKSUM]
    at = sum(ph * (prb + 1) for _, _, _, _, _, ph, prb in A.passes_of(9, 9, 2, 8)[:3]) + (1 + 3 * 2)     # pass 4, its second row
    five = P.make_png(9, 9, 2, 8, interlace=1, stream=zlib.compress(stream[:at] + b"\x05" + stream[at + 1:]))
    assert A.read([five])[1] == [P.E_BAD_SYMBOL]
    huge = P.make_png(5, 3, 2, 8, ihdr=struct.pack(">IIBBBBB", 1 << 20, 1 << 20, 8, 2, 0, 0, 1))
    assert A.index([huge])["images"][0]["status"] == P.E_OUT_CAPACITY
    mixed = A.index([A.make_adam7(5, 3, 2, 8), P.make_png(5, 3, 2, 8), short[:40]])
    assert [(r["status"], r["interlace"]) for r in mixed["images"]] == [(P.OK, 1), (P.OK, 0), (P.E_NO_EOF, 0)]


def test_the_flag_in_the_header_and_in_the_bindings():
    from hdl_deflate_amd import _lib
    import hdl_deflate_amd
    import inspect
    text = header("hdlz_png.h")
    assert int(re.search(r"#define\s+HDLZ_PNG_ADAM7\s+(\d+)u", text).group(1)) == _lib.PNG_ADAM7 == A.ADAM7 == 4
    not_there = text[text.index("Not there"):text.index("#ifndef HDLZ_PNG_H")]
    assert "Adam7" not in not_there and "Adam7" in text
    assert inspect.signature(hdl_deflate_amd.load_png).parameters["interlaced"].default is True
    from hdl_deflate_amd.engine import Engine
    assert inspect.signature(Engine.png_index).parameters["interlaced"].default is False
    assert _lib.load().hdlz_version() == 0x000600


def test_flags_4_and_5_pass_the_parameter_checks_of_both_calls():
    """in front of the device, in the way of tests/test_png_cabi.py: 0, 1, 4 and 5 get past the checks (without a device: HDLZ_E_HIP, as
    0 and 1 do), everything else is refused by name"""
    from hdl_deflate_amd import _lib
    L = _lib.load()
    keep, base = _host_buffer(1 << 18)
    iw = L.hdlz_png_index_work_bytes(3, 3)
    dw = L.hdlz_png_decode_work_bytes(2, 4, 4096, 8192)

    def index(flags, **kw):
        a = dict(dict(work_bytes=iw), **kw)
        return L.hdlz_png_index_ws(base, 1000, base + 2048, base + 2304, 3, flags, 64, 3, base + 4096, base + 8192, base + 16384, a["work_bytes"], None)

    def decode(flags, **kw):
        a = dict(dict(work_bytes=dw), **kw)
        return L.hdlz_png_decode_ws(base, 1000, base + 4096, 0, 2, flags, 4, 4096, 8192, base + 8192, 4096, base + 16384, base + 16640, base + 20480,
                                    a["work_bytes"], None)

    for call in (index, decode):
        for flags in (2, 3, 6, 7, 8, 12, 1 << 31):
            assert call(flags) == E_BAD_PARAM and b"flags must be" in L.hdlz_last_error(), (call.__name__, flags, L.hdlz_last_error())
        for flags in (0, 1, 4, 5):                                # the check behind the flags' still answers: they were accepted
            assert call(flags, work_bytes=1) == E_BAD_PARAM and b"work_bytes" in L.hdlz_last_error() and b"flags" not in L.hdlz_last_error(), \
                (call.__name__, flags, L.hdlz_last_error())
        if _no_device():
            assert [call(flags) for flags in (0, 1, 4, 5)] == [E_HIP] * 4
