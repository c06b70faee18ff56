"""CPU: the extension header include/hdlz_bgzf_range.h -- every declaration exported and bound with its arity, the struct mirror, the
work query equal to its closed form, parameter errors in front of the device, no CPU path behind good parameters; bgzf_range_ref, the
reference of the GPU tests, held against a brute-force per-byte map; and the host module hdl_deflate_amd/bgzf.py (virtual offsets, the
.gzi file) against hand-written bytes."""
import ctypes
import re
import struct

import pytest

import bgzf_ref
from cabi_common import check_struct_mirror, declarations, header, host_buffer, no_device as _no_device, r256
import bgzf_range_ref as ref
from bgzf_ref import OK, E_BAD_PARAM

E_HIP = 9


def _header():
    return header("hdlz_bgzf_range.h")


def _declarations():
    return declarations(_header())


def test_every_declaration_is_exported_and_bound():
    from hdl_deflate_amd import _lib
    params = _declarations()
    assert params == {"hdlz_bgzf_ranges_work_bytes": 3, "hdlz_bgzf_read_ranges_ws": 17}
    assert sorted(params) == sorted(_lib.BGZF_RANGE_EXPORTS) == sorted(_lib.BGZF_RANGE_SIGNATURES)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    L = _lib.load()
    for name, n in params.items():
        assert hasattr(raw, name), name
        restype, argtypes = _lib.BGZF_RANGE_SIGNATURES[name]
        assert len(argtypes) == n, name
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert '#include "hdlz_bgzf.h"' in _header()
    assert re.search(r"#define\s+HDLZ_BGZF_RANGE_VIRTUAL\s+1u", _header()) and _lib.BGZF_RANGE_VIRTUAL == 1


def test_the_tables_in_front_of_it_are_as_they_were():
    from hdl_deflate_amd import _lib
    assert [len(t) for t in (_lib.EXPORTS, _lib.JOIN_EXPORTS, _lib.UNJOIN_EXPORTS, _lib.GZIP_EXPORTS, _lib.BGZF_EXPORTS)] == [22, 4, 2, 7, 8]
    older = set(_lib.EXPORTS) | set(_lib.JOIN_EXPORTS) | set(_lib.UNJOIN_EXPORTS) | set(_lib.GZIP_EXPORTS) | set(_lib.BGZF_EXPORTS)
    assert len(_lib.BGZF_RANGE_EXPORTS) == 2 and not set(_lib.BGZF_RANGE_EXPORTS) & older
    assert _lib.load().hdlz_version() == 0x000600


def test_the_struct_mirror_matches_the_header():
    from hdl_deflate_amd import _lib
    R = _lib.BgzfRangesResult
    check_struct_mirror(_header(), "hdlz_bgzf_ranges_result", R,
                        [("uint64_t", "total_out"), ("uint64_t", "ntasks"), ("uint64_t", "first_bad"), ("uint32_t", "status"), ("uint32_t", "reserved")])
    assert ctypes.sizeof(R) == 32


def closed_form(R, T):
    return 256 + 4 * r256(8 * (R + 1)) + 3 * r256(4 * R) + 3 * r256(8 * T) + 6 * r256(4 * T) + 131072 * R if R else 0


SIZES = (0, 1, 255, 256, 257, 1 << 20)


def test_the_work_query_is_its_closed_form():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    for R in SIZES:
        for T in SIZES:
            for flags in (0, 1):
                assert L.hdlz_bgzf_ranges_work_bytes(R, T, flags) == closed_form(R, T), (R, T, flags)
            if R:                                                         # what the issue bounds: slots, words per range and per task
                got = L.hdlz_bgzf_ranges_work_bytes(R, T, 0)
                assert got - 131072 * R <= 64 * R + 64 * T + 8192
        assert L.hdlz_bgzf_ranges_work_bytes(0, R, 0) == 0
    for R, T, flags in ((1 << 31, 1, 0), (1, 1 << 31, 0), (5, 5, 2), (5, 5, 3), (5, 5, 128)):
        assert L.hdlz_bgzf_ranges_work_bytes(R, T, flags) == 0


def _host_buffer():
    return host_buffer(1 << 19)


def test_parameter_errors_come_before_the_device():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    keep, base = _host_buffer()
    wb = L.hdlz_bgzf_ranges_work_bytes(2, 4, 0)
    assert wb == closed_form(2, 4) and wb + 16384 <= 1 << 19

    def read(file=base, off=base + 1024, out_off=base + 2048, nmembers=3, ranges=base + 3072, nranges=2, flags=0, out=base + 4096, out_cap=64,
             range_off=base + 5120, status=None, task_cap=4, result=base + 6144, work=base + 16384, work_bytes=wb):
        return L.hdlz_bgzf_read_ranges_ws(file, 100, off, out_off, nmembers, ranges, nranges, flags, out, out_cap, range_off, status, task_cap,
                                          result, work, work_bytes, None)
    for k in ("file", "off", "out_off", "ranges", "out", "range_off", "result", "work"):
        assert read(**{k: None}) == E_BAD_PARAM, k
    for k in ("nranges", "nmembers", "task_cap"):
        assert read(**{k: 1 << 31}) == E_BAD_PARAM and b"2^31" in L.hdlz_last_error(), k
    for flags in (2, 3, 4, 64, 1 << 31):
        assert read(flags=flags) == E_BAD_PARAM and b"flags" in L.hdlz_last_error(), flags
    for k in ("off", "out_off", "ranges", "range_off", "result"):
        assert read(**{k: base + 1028}) == E_BAD_PARAM and b"8-byte" in L.hdlz_last_error(), k
    assert read(status=base + 7170) == E_BAD_PARAM and b"4-byte" in L.hdlz_last_error()
    assert read(work=base + 16384 + 128) == E_BAD_PARAM and b"256-byte" in L.hdlz_last_error()
    assert read(work_bytes=wb - 1) == E_BAD_PARAM and b"hdlz_bgzf_ranges_work_bytes" in L.hdlz_last_error()
    # an empty batch still wants its two outputs
    assert read(nranges=0, range_off=None) == E_BAD_PARAM and read(nranges=0, result=None) == E_BAD_PARAM
    if _no_device():
        assert read() == E_HIP and read(flags=1) == E_HIP and read(status=base + 7168) == E_HIP
        assert read(file=base + 1, out=base + 4097) == E_HIP                                   # file and output need no alignment
        assert read(out=None, out_cap=0, task_cap=0, work_bytes=L.hdlz_bgzf_ranges_work_bytes(2, 0, 0)) == E_HIP      # the sizing call
        assert read(nranges=0, file=None, off=None, out_off=None, ranges=None, out=None, out_cap=0, work=None, work_bytes=0) == E_HIP


# ---- bgzf_range_ref against a per-byte map
def _files():
    """(off, out_off) of files from bgzf_ref.member with empty members in front, inside and behind"""
    for lens in ((0, 0, 5, 0, 0, 7, 1, 0), (3,), (0,), (), (4, 4, 4), (0, 9, 0, 0, 2)):
        ms = [bgzf_ref.member(bgzf_ref.data(n, n + 1), 6) for n in lens] + [bgzf_ref.EOF]
        w = bgzf_ref.walk(b"".join(ms))
        assert w.status == OK and w.nmembers == len(lens) + 1
        yield w.off, w.out_off


def _byte_map(out_off):
    """owner[p] = the member that holds byte p of the data"""
    owner = []
    for b in range(len(out_off) - 1):
        owner += [b] * (out_off[b + 1] - out_off[b])
    return owner


@pytest.mark.parametrize("index", list(_files()), ids=lambda ix: "M%d" % (len(ix[0]) - 1))
def test_resolve_is_the_per_byte_map(index):
    off, out_off = index
    M, total = len(off) - 1, out_off[-1]
    owner = _byte_map(out_off)
    ranges = [(x, y) for x in range(total + 3) for y in range(total + 3)]
    for (x, y), (st, p0, p1, lo, hi) in zip(ranges, ref.resolve(off, out_off, ranges)):
        if x > y:
            assert (st, p0, p1, lo, hi) == (E_BAD_PARAM, 0, 0, 0, 0)
            continue
        assert (st, p0, p1) == (OK, min(x, total), min(y, total))
        touched = owner[p0:p1]
        if not touched:
            assert lo == hi == 0
        else:                                # every member from the first byte's to the last byte's, the empty ones between them too
            assert (lo, hi) == (touched[0], touched[-1] + 1)
            assert out_off[lo + 1] > out_off[lo] and out_off[hi] > out_off[hi - 1]              # the edges are never empty
    # virtual mode: every (member, u) names the position O[b] + u; both aliases of a boundary; what names nothing
    names = [(b, u) for b in range(M) for u in range(out_off[b + 1] - out_off[b] + 1)] + [(M, 0)]
    pos = {(b, u): out_off[b] + u for b, u in names}
    vr = [(ref.virtual(off[b0], u0), ref.virtual(off[b1], u1)) for b0, u0 in names for b1, u1 in names]
    plain = ref.resolve(off, out_off, [(pos[n0], pos[n1]) for n0 in names for n1 in names])
    for got, want in zip(ref.resolve(off, out_off, vr, virtual=True), plain):
        assert got == want
    bad = [ref.virtual(off[M], 1), ref.virtual(off[M] + 1, 0), ref.virtual(off[0] + 5, 0)]
    bad += [ref.virtual(off[b], out_off[b + 1] - out_off[b] + 1) for b in range(M)]
    for v in bad:
        assert ref.resolve(off, out_off, [(v, ref.virtual(off[M], 0)), (ref.virtual(off[0], 0), v)], virtual=True) == [(E_BAD_PARAM, 0, 0, 0, 0)] * 2


def test_expected_is_slices_of_the_data():
    parts = [bgzf_ref.data(n, n) for n in (0, 300, 0, 0, 5000, 12, 0)]
    f = b"".join(bgzf_ref.member(p, 6) for p in parts) + bgzf_ref.EOF
    data = b"".join(parts)
    ranges = [(0, 1), (299, 301), (0, 1 << 40), (5311, 5312), (300, 300), (9, 3), (5312, 6000), (250, 5305)]
    e = ref.expected(f, ranges)
    assert e.status == [0, 0, 0, 0, 0, E_BAD_PARAM, 0, 0] and (e.record_status, e.first_bad) == (E_BAD_PARAM, 5)
    assert [p for p in e.pieces if p is not None] == [data[x:y] for x, y in ranges if x <= y]
    assert e.range_off == [0, 1, 3, 5315, 5316, 5316, 5316, 5316, 5316 + 5055] and e.total_out == e.range_off[-1]
    assert e.ntasks == 1 + 4 + 5 + 1 + 0 + 0 + 0 + 5
    short = ref.expected(f, ranges, out_cap=e.total_out - 1)
    assert short.status == [2, 2, 2, 2, 2, E_BAD_PARAM, 2, 2] and (short.record_status, short.first_bad) == (2, ref.NOBODY)
    assert (short.total_out, short.ntasks, short.range_off) == (e.total_out, e.ntasks, e.range_off)
    assert ref.expected(f, ranges, task_cap=e.ntasks - 1).status == short.status
    hit = ref.expected(f, ranges, member_status=[0, 0, 0, 0, 12, 0, 0, 0])
    assert hit.status == [0, 12, 12, 0, 0, E_BAD_PARAM, 0, 12] and (hit.record_status, hit.first_bad) == (12, 1)


# ---- hdl_deflate_amd/bgzf.py
def test_gzi_dumps_is_the_stated_layout():
    from hdl_deflate_amd import bgzf
    # five members -- 100 bytes, 0 bytes, 7 bytes, 65536 bytes, 1 byte -- and the EOF member
    off = [0, 90, 118, 150, 40150, 40180, 40208]
    out_off = [0, 100, 100, 107, 65643, 65644, 65644]
    want = bytes.fromhex("0300000000000000"                       # three entries: members 2, 3 and 4
                         "7600000000000000" "6400000000000000"     # (118, 100)
                         "9600000000000000" "6b00000000000000"     # (150, 107)
                         "d69c000000000000" "6b00010000000000")    # (40150, 65643)
    assert bgzf.gzi_dumps(off, out_off) == want == ref.gzi(off, out_off)
    assert bgzf.gzi_loads(want) == ([118, 150, 40150], [100, 107, 65643])
    assert bgzf.gzi_dumps([0, 28], [0, 0]) == bytes(8) == bgzf.gzi_dumps([0], [0])           # the EOF member alone; no member
    assert bgzf.gzi_loads(bytes(8)) == ([], [])
    for index in _files():
        z = bgzf.gzi_dumps(*index)
        assert z == ref.gzi(*index)
        c, u = bgzf.gzi_loads(z)
        assert z == struct.pack("<Q", len(c)) + b"".join(struct.pack("<QQ", a, b) for a, b in zip(c, u))
        assert c == [index[0][b] for b in range(1, len(index[0]) - 1) if index[1][b + 1] > index[1][b]]
    import hdl_deflate_amd
    assert hdl_deflate_amd.gzi_dumps is bgzf.gzi_dumps and hdl_deflate_amd.gzi_loads is bgzf.gzi_loads and hdl_deflate_amd.bgzf is bgzf


def test_gzi_loads_rejects_what_is_not_an_index():
    from hdl_deflate_amd import bgzf
    good = bgzf.gzi_dumps([0, 90, 118, 150, 178], [0, 100, 100, 107, 107])
    assert bgzf.gzi_loads(good) == ([118], [100])
    two = struct.pack("<QQQQQ", 2, 90, 100, 150, 107)
    assert bgzf.gzi_loads(two) == ([90, 150], [100, 107])
    for cut in (b"", good[:7], good[:8], good[:-1], two[:24]):                                # truncated
        with pytest.raises(ValueError):
            bgzf.gzi_loads(cut)
    for wrong in (good + b"\0", two + bytes(16), struct.pack("<QQQ", 0, 1, 2)):               # the count does not match the length
        with pytest.raises(ValueError):
            bgzf.gzi_loads(wrong)
    for a, b, c, d in ((150, 100, 90, 107), (90, 107, 150, 100), (90, 100, 90, 107), (90, 100, 150, 100), (0, 0, 150, 100)):   # not ascending
        with pytest.raises(ValueError):
            bgzf.gzi_loads(struct.pack("<QQQQQ", 2, a, b, c, d))


def test_virtual_offsets():
    from hdl_deflate_amd import bgzf
    import hdl_deflate_amd
    assert bgzf.virtual_offset(0, 0) == 0 and bgzf.split_virtual(0) == (0, 0)
    top = bgzf.virtual_offset((1 << 48) - 1, 65535)
    assert top == (1 << 64) - 1 and bgzf.split_virtual(top) == ((1 << 48) - 1, 65535)
    assert bgzf.virtual_offset(0x1234, 0x00FF) == 0x123400FF and bgzf.split_virtual(0x123400FF) == (0x1234, 0xFF)
    for c, u in ((-1, 0), (1 << 48, 0), (0, -1), (0, 65536)):
        with pytest.raises(ValueError):
            bgzf.virtual_offset(c, u)
    for v in (-1, 1 << 64):
        with pytest.raises(ValueError):
            bgzf.split_virtual(v)
    assert hdl_deflate_amd.virtual_offset is bgzf.virtual_offset and hdl_deflate_amd.split_virtual is bgzf.split_virtual
