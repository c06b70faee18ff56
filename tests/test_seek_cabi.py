"""CPU: the extension header include/hdlz_seek.h -- every declaration exported and bound with its arity, the struct mirror, both work
queries equal to their closed forms, parameter errors in front of the device; the index file of hdl_deflate_amd/seek.py against
hand-written bytes; and seek_ref, the reference of the GPU tests, held against stock zlib -- every reference segment is decoded again by
zlib.decompressobj(wbits=-15, zdict=window) from its bits moved to a byte boundary (block by block: a stored block rests on the byte
alignment that moving the bits breaks) -- with the coverage the GPU tests rely on asserted from the reference index alone."""
import ctypes
import re
import struct
import zlib

import pytest

import seek_ref as ref
from cabi_common import check_struct_mirror, declarations, header, host_buffer, no_device as _no_device, r256

OK, E_BAD_PARAM, E_HIP = 0, 8, 9


def _header():
    return header("hdlz_seek.h")


def test_every_declaration_is_exported_and_bound():
    from hdl_deflate_amd import _lib
    params = declarations(_header())
    assert params == {"hdlz_seek_index_work_bytes": 4, "hdlz_seek_index_ws": 15, "hdlz_seek_ranges_work_bytes": 4, "hdlz_seek_read_ranges_ws": 20}
    assert sorted(params) == sorted(_lib.SEEK_EXPORTS) == sorted(_lib.SEEK_CALLS)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    L = _lib.load()
    for name, n in params.items():
        assert hasattr(raw, name), name
        restype, argtypes = _lib.SEEK_CALLS[name]
        assert len(argtypes) == n, name
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert '#include "hdlz_bgzf_range.h"' in _header()
    for name, v in (("ZLIB", _lib.SEEK_ZLIB), ("GZIP", _lib.SEEK_GZIP), ("WINDOW", _lib.SEEK_WINDOW)):
        assert re.search(r"#define\s+HDLZ_SEEK_%s\s+%du" % (name, v), _header()), name
    older = set().union(*(getattr(_lib, n) for n in dir(_lib) if n.endswith("_EXPORTS") and n != "SEEK_EXPORTS"), _lib.EXPORTS)
    assert not set(_lib.SEEK_EXPORTS) & older and L.hdlz_version() == 0x000600            # additive: the ABI word stays
    assert "Not there" in _header() and "chain route" in _header().lower()


def test_the_struct_mirrors_match_the_header():
    from hdl_deflate_amd import _lib
    check_struct_mirror(_header(), "hdlz_seek_result", _lib.SeekResult,
                        [("uint64_t", "npoints"), ("uint64_t", "total_out"), ("uint64_t", "end_bit"), ("uint64_t", "max_seg"),
                         ("uint32_t", "status"), ("uint32_t", "route")])
    assert ctypes.sizeof(_lib.SeekResult) == 40
    assert re.search(r"typedef\s+hdlz_bgzf_ranges_result\s+hdlz_seek_ranges_result\s*;", _header()) and _lib.SeekRangesResult is _lib.BgzfRangesResult


def index_form(L, file_len, flags, out_cap, P):
    row = min(out_cap & ~3, (1 << 32) - 512)
    return 768 + 2 * r256(8 * P) + r256(8 * ((row + 32767) // 32768)) + r256(L.hdlz_inflate_work_bytes(1, file_len, row, 0, 1 if flags == 2 else 0))


def ranges_form(R, T, seg_cap):
    return 256 + 4 * r256(8 * (R + 1)) + 3 * r256(4 * R) + 3 * r256(8 * T) + 9 * r256(4 * T) + 2 * r256(seg_cap) * R if R else 0


SIZES = (0, 1, 255, 256, 257, 1 << 20)


def test_the_work_queries_are_their_closed_forms():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    for P in SIZES:
        for out_cap in (0, 3, 4, 32768, 32769, 65536, 1 << 24, (1 << 32) - 512, (1 << 32) + 5, 1 << 36):
            for flags in (1, 2):
                for file_len in (0, 1000, 5000, 1 << 24):
                    assert L.hdlz_seek_index_work_bytes(file_len, flags, out_cap, P) == index_form(L, file_len, flags, out_cap, P), (P, out_cap, flags, file_len)
    for file_len, flags, P in ((1 << 28, 1, 5), (10, 0, 5), (10, 3, 5), (10, 4, 5), (10, 1, 1 << 31)):
        assert L.hdlz_seek_index_work_bytes(file_len, flags, 100, P) == 0
    for R in SIZES:
        for T in SIZES:
            for seg in (0, 1, 256, 257, 65536, 300000):
                assert L.hdlz_seek_ranges_work_bytes(R, T, seg, 0) == ranges_form(R, T, seg), (R, T, seg)
    # with the slot of a BGZF member, and without the three words a task has here, it is that call's scratch
    assert L.hdlz_seek_ranges_work_bytes(7, 9, 65536, 0) - 3 * r256(4 * 9) == L.hdlz_bgzf_ranges_work_bytes(7, 9, 0)
    for R, T, seg, flags in ((1 << 31, 1, 5, 0), (1, 1 << 31, 5, 0), (5, 5, (1 << 32) - 511, 0), (5, 5, 5, 1)):
        assert L.hdlz_seek_ranges_work_bytes(R, T, seg, flags) == 0


def test_parameter_errors_come_before_the_device():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    keep, base = host_buffer(1 << 20)
    wb = L.hdlz_seek_index_work_bytes(100, 2, 4096, 3)
    assert wb == index_form(L, 100, 2, 4096, 3)

    def index(file=base, file_len=100, flags=2, span=1024, out=base + 1024, out_cap=4096, bit=base + 8192, pos=base + 8448, crc=base + 8704,
              win=base + 16384, point_cap=3, result=base + 9216, work=base + (1 << 18), work_bytes=wb):
        return L.hdlz_seek_index_ws(file, file_len, flags, span, out, out_cap, bit, pos, crc, win, point_cap, result, work, work_bytes, None)
    for k in ("file", "out", "bit", "pos", "crc", "win", "result", "work"):
        assert index(**{k: None}) == E_BAD_PARAM, k
    for flags in (0, 3, 4, 1 << 31):
        assert index(flags=flags) == E_BAD_PARAM and b"flags" in L.hdlz_last_error(), flags
    assert index(span=0) == E_BAD_PARAM and b"span" in L.hdlz_last_error()
    assert index(file_len=1 << 28) == E_BAD_PARAM and b"file_len" in L.hdlz_last_error()
    assert index(point_cap=1 << 31) == E_BAD_PARAM and b"2^31" in L.hdlz_last_error()
    for k in ("bit", "pos", "result"):
        assert index(**{k: base + 8196}) == E_BAD_PARAM and b"8-byte" in L.hdlz_last_error(), k
    for k in ("crc", "out"):
        assert index(**{k: base + 8706}) == E_BAD_PARAM and b"4-byte" in L.hdlz_last_error(), k
    assert index(win=base + 16392) == E_BAD_PARAM and b"16-byte" in L.hdlz_last_error()
    assert index(work=base + (1 << 18) + 128) == E_BAD_PARAM and b"256-byte" in L.hdlz_last_error()
    assert index(work_bytes=wb - 1) == E_BAD_PARAM and b"hdlz_seek_index_work_bytes" in L.hdlz_last_error()
    rb = L.hdlz_seek_ranges_work_bytes(2, 4, 3000, 0)
    assert rb == ranges_form(2, 4, 3000)

    def read(file=base, file_len=100, bit=base + 8192, pos=base + 8448, crc=base + 8704, win=base + 16384, npoints=3, ranges=base + 3072, nranges=2,
             flags=0, seg_cap=3000, out=base + 4096, out_cap=64, range_off=base + 5120, status=None, task_cap=4, result=base + 6144,
             work=base + (1 << 18), work_bytes=rb):
        return L.hdlz_seek_read_ranges_ws(file, file_len, bit, pos, crc, win, npoints, ranges, nranges, flags, seg_cap, out, out_cap, range_off,
                                          status, task_cap, result, work, work_bytes, None)
    for k in ("file", "bit", "pos", "crc", "win", "ranges", "out", "range_off", "result", "work"):
        assert read(**{k: None}) == E_BAD_PARAM, k
    for k in ("nranges", "npoints", "task_cap"):
        assert read(**{k: 1 << 31}) == E_BAD_PARAM and b"2^31" in L.hdlz_last_error(), k
    assert read(npoints=0) == E_BAD_PARAM and b"npoints" in L.hdlz_last_error()
    assert read(file_len=1 << 28) == E_BAD_PARAM and b"file_len" in L.hdlz_last_error()
    assert read(seg_cap=(1 << 32) - 511) == E_BAD_PARAM and b"seg_cap" in L.hdlz_last_error()
    for flags in (1, 2, 1 << 31):
        assert read(flags=flags) == E_BAD_PARAM and b"flags" in L.hdlz_last_error(), flags
    for k in ("bit", "pos", "ranges", "range_off", "result"):
        assert read(**{k: base + 1028}) == E_BAD_PARAM and b"8-byte" in L.hdlz_last_error(), k
    for k in ("crc", "status"):
        assert read(**{k: base + 7170}) == E_BAD_PARAM and b"4-byte" in L.hdlz_last_error(), k
    assert read(work=base + (1 << 18) + 128) == E_BAD_PARAM and b"256-byte" in L.hdlz_last_error()
    assert read(work_bytes=rb - 1) == E_BAD_PARAM and b"hdlz_seek_ranges_work_bytes" in L.hdlz_last_error()
    assert read(nranges=0, range_off=None) == E_BAD_PARAM and read(nranges=0, result=None) == E_BAD_PARAM
    if _no_device():                                     # good parameters: no CPU path behind them
        assert index() == E_HIP and index(flags=1) == E_HIP
        assert index(point_cap=0, bit=None, pos=None, crc=None, win=None, work_bytes=L.hdlz_seek_index_work_bytes(100, 2, 4096, 0)) == E_HIP   # the sizing call
        assert read() == E_HIP and read(status=base + 7168) == E_HIP and read(file=base + 1, out=base + 4097, win=base + 16385) == E_HIP
        assert read(out=None, out_cap=0, task_cap=0, work_bytes=L.hdlz_seek_ranges_work_bytes(2, 0, 3000, 0)) == E_HIP
        assert read(nranges=0, file=None, bit=None, pos=None, crc=None, win=None, ranges=None, out=None, out_cap=0, work=None, work_bytes=0) == E_HIP


# ---- hdl_deflate_amd/seek.py
def _small_index():
    import torch
    from hdl_deflate_amd.seek import SeekIndex
    win = torch.zeros((2, 32768), dtype=torch.uint8)
    win[1, -3:] = torch.tensor([7, 8, 9], dtype=torch.uint8)
    return SeekIndex(torch.tensor([16, 83, 200]), torch.tensor([0, 3, 10]), torch.tensor([0x11223344, -2], dtype=torch.int32), win,
                     span=2, file_len=30, total=10, end_bit=200, max_seg=7, container="zlib")


def test_dumps_is_the_stated_layout():
    import hdl_deflate_amd
    from hdl_deflate_amd import seek
    ix = _small_index()
    want = b"HDLZSEEK" + struct.pack("<IIQQQQ", 1, 1, 2, 30, 2, 7) + struct.pack("<3Q", 16, 83, 200) + struct.pack("<3Q", 0, 3, 10) + \
        bytes.fromhex("44332211" "feffffff") + bytes(32768) + bytes(32765) + b"\x07\x08\x09"
    z = ix.dumps()
    assert z == want and len(z) == seek.file_bytes(2) == 48 + 48 + 8 + 65536
    back = seek.loads(z)
    assert (back.span, back.file_len, back.total, back.end_bit, back.max_seg, back.container, back.npoints) == (2, 30, 10, 200, 7, "zlib", 2)
    assert back.bit.tolist() == [16, 83, 200] and back.pos.tolist() == [0, 3, 10] and back.crc.tolist() == [0x11223344, -2]
    assert bytes(back.win.numpy().tobytes()) == bytes(ix.win.numpy().tobytes()) and back.dumps() == z
    assert hdl_deflate_amd.SeekIndex is seek.SeekIndex and hdl_deflate_amd.seek is seek
    assert "HDLZSEEK" in seek.__doc__ and "max_seg" in seek.__doc__


def test_loads_rejects_what_is_not_an_index():
    from hdl_deflate_amd import seek
    good = _small_index().dumps()
    for cut in (b"", good[:7], good[:47], good[:48], good[:100], good[:-1]):                                   # truncated
        with pytest.raises(ValueError):
            seek.loads(cut)

    def patched(at, fmt, v):
        return good[:at] + struct.pack(fmt, v) + good[at + struct.calcsize(fmt):]
    bad = [b"HDLZSEEX" + good[8:], good + b"\0", patched(8, "<I", 2), patched(12, "<I", 3), patched(12, "<I", 0), patched(16, "<Q", 0),
           patched(32, "<Q", 1), patched(32, "<Q", 3), patched(32, "<Q", 0), patched(40, "<Q", 6),
           patched(48 + 8, "<Q", 16), patched(48 + 8, "<Q", 201), patched(48 + 16, "<Q", 241),       # bits: not ascending; behind the file
           patched(72 + 8, "<Q", 0), patched(72 + 8, "<Q", 11), patched(72, "<Q", 1)]                # positions: not ascending; not from 0
    for b in bad:
        with pytest.raises(ValueError):
            seek.loads(b)


# ---- the reference against stock zlib, and the coverage of its streams
def _indexes():
    for name, (container, z, data, spans) in ref.streams().items():
        w = ref.walk(z, container)
        for span in spans:
            yield name, container, z, data, w, span, ref.index(w, span)


def test_the_walker_finds_what_zlib_decodes():
    for name, (container, z, data, spans) in ref.streams().items():
        w = ref.walk(z, container)
        assert w.data == data and w.total == len(data) and 64 << 10 <= len(data) <= 300 << 10 or name == "ONE", name
        assert w.boundaries[0].bit == 8 * w.payload and w.boundaries[0].pos == 0
        trailer = 8 if container == "gzip" else 4
        end = (w.end_bit + 7) // 8
        assert end + trailer <= len(z) and (container == "gzip" or end + trailer == len(z)), name
        check = zlib.crc32(data).to_bytes(4, "little") if container == "gzip" else zlib.adler32(data).to_bytes(4, "big")
        assert z[end:end + 4] == check, name


def test_every_reference_segment_decodes_with_stock_zlib():
    n = 0
    for name, container, z, data, w, span, ix in _indexes():
        assert ix.bit[0] == 8 * w.payload and ix.pos[0] == 0 and ix.pos[-1] == len(data) and ix.bit[-1] == w.end_bit
        assert all(ix.pos[k] < ix.pos[k + 1] for k in range(len(ix.crc) - 1)) and all(ix.bit[k] < ix.bit[k + 1] for k in range(len(ix.crc)))
        assert all(ix.pos[k] // span > ix.pos[k - 1] // span for k in range(1, len(ix.crc)))
        for k in range(len(ix.crc)):
            seg = data[ix.pos[k]:ix.pos[k + 1]]
            assert ref.decode_segment(z, w, ix, k) == seg, (name, span, k)
            assert ix.crc[k] == zlib.crc32(seg) and len(ix.win[k]) == 32768
            h = min(32768, ix.pos[k])
            assert ix.win[k] == bytes(32768 - h) + data[ix.pos[k] - h:ix.pos[k]]
            n += 1
    assert n > 500


def test_the_streams_cover_what_the_gpu_tests_rely_on():
    residues, types, low, shared, skipped, single = set(), set(), 0, 0, 0, 0
    for name, container, z, data, w, span, ix in _indexes():
        at = {b.bit: b for b in w.boundaries}
        n = len(ix.crc)
        single += n == 1 and len(w.boundaries) == 1
        for k in range(n):
            b = at[ix.bit[k]]                                   # every point is a true boundary
            assert b.pos == ix.pos[k]
            residues.add(b.bit & 7)
            types.add(b.btype)
            low += 0 < b.pos < 32768
            same = [c for c in w.boundaries if c.pos == b.pos]
            assert same[0] == b                                 # of the boundaries that share a position, the first
            shared += len(same) > 1 and k > 0
            skipped += k > 0 and ix.pos[k] // span > ix.pos[k - 1] // span + 1
    assert residues == set(range(8))
    assert types == {0, 1, 2}                                   # points in front of stored, fixed and dynamic blocks
    assert low > 10 and shared > 10 and skipped > 3 and single >= 1
    assert any(ix.max_seg > 65536 for *_, ix in _indexes())     # a segment longer than a BGZF member: the slots are the call's own size


def test_points_is_the_rule():
    bd = [(16, 0), (100, 5), (200, 5), (300, 9), (400, 10), (500, 10), (600, 31), (700, 39), (800, 40)]
    assert ref.points(bd, 10) == [(16, 0), (400, 10), (600, 31), (800, 40)]
    assert ref.points(bd, 1) == [(16, 0), (100, 5), (300, 9), (400, 10), (600, 31), (700, 39), (800, 40)]
    assert ref.points(bd, 1000) == [(16, 0)]
    # a subset S that holds the first header selects by its own predecessors
    assert ref.points([bd[0], bd[3], bd[5], bd[8]], 10) == [(16, 0), (500, 10), (800, 40)]


def test_expected_is_slices_of_the_data():
    pos, d = [0, 10, 25, 25 + 7], bytes(range(32))
    ranges = [(0, 1), (9, 11), (0, 1 << 40), (31, 32), (10, 10), (9, 3), (32, 60), (10, 25), (24, 26)]
    e = ref.expected(d, pos, ranges)
    assert e.status == [0, 0, 0, 0, 0, E_BAD_PARAM, 0, 0, 0] and (e.record_status, e.first_bad) == (E_BAD_PARAM, 5)
    assert [p for p in e.pieces if p is not None] == [d[x:y] for x, y in ranges if x <= y]
    assert e.ntasks == 1 + 2 + 3 + 1 + 0 + 0 + 0 + 1 + 2 and e.total_out == e.range_off[-1] == 1 + 2 + 32 + 1 + 15 + 2
    short = ref.expected(d, pos, ranges, out_cap=e.total_out - 1)
    assert short.status == [2, 2, 2, 2, 2, E_BAD_PARAM, 2, 2, 2] and (short.record_status, short.first_bad) == (2, ref.NOBODY)
    hit = ref.expected(d, pos, ranges, segment_status=[0, 12, 0])
    assert hit.status == [0, 12, 12, 0, 0, E_BAD_PARAM, 0, 12, 12] and (hit.record_status, hit.first_bad) == (12, 1)
