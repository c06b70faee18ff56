"""CPU: the extension header include/hdlz_bgzf.h -- every declaration exported and bound with its arity, the struct mirrors, the queries
equal to their closed forms, parameter errors in front of the device, no CPU path behind good parameters; and bgzf_ref, the reference
of the GPU tests (members from stock zlib, the serial walk of the index call), held against gzip.decompress before any kernel is
trusted to it."""
import ctypes
import gzip
import zlib

import numpy as np
import pytest

import bgzf_ref
from cabi_common import check_struct_mirror, declarations, header, host_buffer as _host_buffer, no_device as _no_device, r256
from bgzf_ref import OK, E_NO_EOF, E_BAD_PARAM, E_BAD_HEADER

E_HIP = 9
LEVELS = (0, 1, 6, 9)


def _header():
    return header("hdlz_bgzf.h")


def _declarations():
    return declarations(_header())


def test_every_declaration_is_exported_and_bound():
    from hdl_deflate_amd import _lib
    params = _declarations()
    assert params == {"hdlz_crc32_batch_ws": 7, "hdlz_bgzf_bound": 2, "hdlz_bgzf_join_work_bytes": 1, "hdlz_bgzf_join_ws": 15,
                      "hdlz_bgzf_index_work_bytes": 1, "hdlz_bgzf_index_ws": 9, "hdlz_bgzf_inflate_work_bytes": 2, "hdlz_bgzf_inflate_ws": 13}
    assert sorted(params) == sorted(_lib.BGZF_EXPORTS) == sorted(_lib.BGZF_SIGNATURES)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    L = _lib.load()
    for name, n in params.items():
        assert hasattr(raw, name), name
        restype, argtypes = _lib.BGZF_SIGNATURES[name]
        assert len(argtypes) == n, name
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert '#include "hdlz_gzip.h"' in _header()


def test_the_tables_in_front_of_it_are_as_they_were():
    from hdl_deflate_amd import _lib
    assert len(_lib.EXPORTS) == 22 and len(_lib.JOIN_EXPORTS) == 4 and len(_lib.UNJOIN_EXPORTS) == 2 and len(_lib.GZIP_EXPORTS) == 7
    assert len(_lib.BGZF_EXPORTS) == 8
    assert not set(_lib.BGZF_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.JOIN_EXPORTS) | set(_lib.UNJOIN_EXPORTS) | set(_lib.GZIP_EXPORTS))
    assert _lib.load().hdlz_version() == 0x000600


@pytest.mark.parametrize("struct, mirror, want", [
    ("hdlz_bgzf_join_result", "BgzfJoinResult", [("uint64_t", "file_len"), ("uint32_t", "status"), ("uint32_t", "first_bad")]),
    ("hdlz_bgzf_index_result", "BgzfIndexResult", [("uint64_t", "nmembers"), ("uint64_t", "total_out"), ("uint64_t", "file_used"),
                                                   ("uint32_t", "status"), ("uint32_t", "eof_marker")]),
    ("hdlz_bgzf_inflate_result", "BgzfInflateResult", [("uint64_t", "out_len"), ("uint64_t", "first_bad"), ("uint32_t", "status"),
                                                       ("uint32_t", "reserved")]),
])
def test_struct_mirrors_match_the_header(struct, mirror, want):
    from hdl_deflate_amd import _lib
    check_struct_mirror(_header(), struct, getattr(_lib, mirror), want)


def test_the_queries_are_their_closed_forms():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    for nb in (0, 1, 255, 256, 257, 1 << 20, (1 << 31) - 1, 1 << 31):
        assert L.hdlz_bgzf_join_work_bytes(nb) == L.hdlz_join_work_bytes(nb), nb
        for in_len in (5, 2048, 57344, 58230, 65536):
            assert L.hdlz_bgzf_bound(nb, in_len) == 28 + nb * (L.hdlz_out_bound(in_len) + 20)
    for x in (0, 5, 65536):
        assert L.hdlz_bgzf_bound(0, x) == 28 == len(bgzf_ref.EOF)
    for n in (0, 1, 17, 65535, 65536, 65537, 10 * 65536, (1 << 33) + 1):
        W = (n + 65535) // 65536
        assert L.hdlz_bgzf_index_work_bytes(n) == (r256(64 + 48 * W) if W else 0), n
    for n in (1, 21, 22, 255, 256, 257, 1 << 20, (1 << 31) - 1):
        assert L.hdlz_bgzf_inflate_work_bytes(n, 0) == r256(12 * n) + r256(16 * (n + 1)) + r256(4 * n), n
    for n, flags in ((0, 0), (1 << 31, 0), (5, 2), (5, 4), (5, 64), (5, 1)):
        assert L.hdlz_bgzf_inflate_work_bytes(n, flags) == 0


def test_blocks_of_58230_bytes_always_fit_a_member():
    """a member is its row without the six bytes of the zlib frame, between 18 and 8 bytes: d_len + 20 <= 65536"""
    from hdl_deflate_amd import _lib
    L = _lib.load()
    assert L.hdlz_out_bound(58230) == 6 + ((9 * 58230 + 17) >> 3) == 65516
    assert L.hdlz_out_bound(58230) + 20 <= 65536 < L.hdlz_out_bound(58231) + 20


def test_crc32_batch_parameter_errors_come_before_the_device():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    keep, base = _host_buffer()

    def crc(data=base, off=None, pitch=64, length=64, nblocks=2, out=base + 1024):
        return L.hdlz_crc32_batch_ws(data, off, pitch, length, nblocks, out, None)
    assert crc(out=None) == E_BAD_PARAM and crc(data=None) == E_BAD_PARAM and crc(data=None, off=base) == E_BAD_PARAM
    assert crc(nblocks=1 << 31) == E_BAD_PARAM and b"2^31" in L.hdlz_last_error()
    assert crc(out=base + 1026) == E_BAD_PARAM and b"4-byte" in L.hdlz_last_error()
    assert crc(off=base + 4) == E_BAD_PARAM and b"8-byte" in L.hdlz_last_error()
    if _no_device():
        assert crc() == E_HIP and crc(off=base + 512) == E_HIP and crc(data=base + 3, pitch=7, length=5) == E_HIP
        assert crc(data=None, length=0) == E_HIP and crc(nblocks=0, data=None, out=None) == E_HIP


def test_join_parameter_errors_come_before_the_device():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    keep, base = _host_buffer()
    wb = L.hdlz_bgzf_join_work_bytes(1)
    assert 0 < wb <= 4096

    def join(rows=base, length=base, status=base, in_off=None, crc=base, file=base, off=base, result=base, work=base, work_bytes=wb, nblocks=1):
        return L.hdlz_bgzf_join_ws(rows, 64, length, status, in_off, 64, nblocks, crc, file, 4096, off, result, work, work_bytes, None)
    for k in ("rows", "length", "status", "crc", "file", "off", "result", "work"):
        assert join(**{k: None}) == E_BAD_PARAM, k
    assert join(nblocks=1 << 31) == E_BAD_PARAM and b"2^31" in L.hdlz_last_error()
    assert join(work_bytes=wb - 1) == E_BAD_PARAM and b"hdlz_bgzf_join_work_bytes" in L.hdlz_last_error()
    for k in ("off", "result", "work", "in_off"):
        assert join(**{k: base + 4}) == E_BAD_PARAM and b"8-byte" in L.hdlz_last_error(), k
    assert join(crc=base + 2) == E_BAD_PARAM and b"4-byte" in L.hdlz_last_error()
    if _no_device():
        assert join() == E_HIP and join(in_off=base) == E_HIP
        assert join(nblocks=0, rows=None, length=None, status=None, crc=None, work=None, work_bytes=0) == E_HIP


def test_index_parameter_errors_come_before_the_device():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    keep, base = _host_buffer()
    wb = L.hdlz_bgzf_index_work_bytes(100)
    assert wb == 256

    def index(file=base, file_len=100, cap=4, off=base + 1024, out_off=base + 2048, result=base + 3072, work=base + 4096, work_bytes=wb):
        return L.hdlz_bgzf_index_ws(file, file_len, cap, off, out_off, result, work, work_bytes, None)
    for k in ("file", "off", "out_off", "result", "work"):
        assert index(**{k: None}) == E_BAD_PARAM, k
    assert index(work_bytes=wb - 1) == E_BAD_PARAM and b"hdlz_bgzf_index_work_bytes" in L.hdlz_last_error()
    assert index(cap=1 << 40) == E_BAD_PARAM
    for k in ("off", "out_off", "result", "work"):
        assert index(**{k: base + 1028}) == E_BAD_PARAM and b"8-byte" in L.hdlz_last_error(), k
    if _no_device():
        assert index() == E_HIP and index(file=base + 1) == E_HIP and index(cap=0) == E_HIP
        assert index(file=None, file_len=0, work=None, work_bytes=0) == E_HIP


def test_inflate_parameter_errors_come_before_the_device():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    keep, base = _host_buffer()
    wb = L.hdlz_bgzf_inflate_work_bytes(1, 0)
    assert wb == 768

    def inflate(file=base, off=base + 1024, out_off=base + 2048, out=base + 3072, out_cap=64, status=None, result=base + 4096, work=base + 8192,
                work_bytes=wb, nmembers=1, flags=0):
        return L.hdlz_bgzf_inflate_ws(file, 100, off, out_off, nmembers, flags, out, out_cap, status, result, work, work_bytes, None)
    for k in ("file", "off", "out_off", "out", "result", "work"):
        assert inflate(**{k: None}) == E_BAD_PARAM, k
    assert inflate(nmembers=1 << 31) == E_BAD_PARAM and b"2^31" in L.hdlz_last_error()
    for flags in (1, 2, 4, 8, 64, 128):                                # the mapping hints do not apply here
        assert inflate(flags=flags) == E_BAD_PARAM and b"flags" in L.hdlz_last_error(), flags
    for k in ("off", "out_off", "result"):
        assert inflate(**{k: base + 1028}) == E_BAD_PARAM and b"8-byte" in L.hdlz_last_error(), k
    assert inflate(work=base + 8192 + 128) == E_BAD_PARAM and b"256-byte" in L.hdlz_last_error()
    assert inflate(work_bytes=wb - 1) == E_BAD_PARAM and b"hdlz_bgzf_inflate_work_bytes" in L.hdlz_last_error()
    if _no_device():
        assert inflate() == E_HIP and inflate(status=base + 5120) == E_HIP and inflate(out=base + 3073) == E_HIP      # slots need no alignment
        assert inflate(nmembers=0, file=None, off=None, out_off=None, out=None, out_cap=0, work=None, work_bytes=0) == E_HIP


# ---- bgzf_ref against stock readers
_data = bgzf_ref.data


def test_the_eof_member_is_the_standard_one():
    assert len(bgzf_ref.EOF) == 28
    for level in LEVELS[1:]:
        assert bgzf_ref.member(b"", level) == bgzf_ref.EOF
    assert gzip.decompress(bgzf_ref.EOF) == b""
    assert bgzf_ref.is_header(bgzf_ref.EOF[:18]) and bgzf_ref.header(28) == bgzf_ref.EOF[:18]


@pytest.mark.parametrize("level", LEVELS)
def test_files_built_from_members_round_trip(level):
    parts = [_data(n, n + level) for n in (0, 1, 100, 65280, 40000, 0, 7)]
    parts.append(bytes(65536) if level else _data(65536 - 100, 3))      # (stored: 64 KiB of payload do not fit a member)
    f = b"".join(bgzf_ref.member(p, level) for p in parts)
    for tail in (b"", bgzf_ref.EOF):
        assert gzip.decompress(f + tail) == b"".join(parts)
        w = bgzf_ref.walk(f + tail)
        assert w.record() == (len(parts) + (1 if tail else 0), sum(map(len, parts)), len(f + tail), OK, 1 if tail else 0)
        assert [(f + tail)[a:b] for a, b in zip(w.off, w.off[1:])] == [bgzf_ref.member(p, level) for p in parts] + ([tail] if tail else [])
        assert w.out_off == [0] + list(np.cumsum([len(p) for p in parts] + ([0] if tail else [])))
    if level == 0:                                                       # stored: the payload is in the member verbatim
        assert parts[3] in bgzf_ref.member(parts[3], 0)


def test_the_framing_of_rows_is_read_by_stock_readers():
    blocks = [_data(n, n) for n in (5, 31, 2048, 700)]
    rows = []
    for b in blocks:                                                     # a zlib stream of one final block: what a row looks like
        c = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_FIXED)
        rows.append(c.compress(b) + c.flush())
    f, offs = bgzf_ref.framed_rows(rows, blocks)
    assert gzip.decompress(f) == b"".join(blocks) and f.endswith(bgzf_ref.EOF)
    w = bgzf_ref.walk(f)
    assert w.off[:-1] == offs and w.record() == (5, sum(map(len, blocks)), len(f), OK, 1)
    assert all(offs[b + 1] - offs[b] == len(rows[b]) + 20 for b in range(4))
    assert bgzf_ref.framed_rows([], []) == (bgzf_ref.EOF, [0])


@pytest.mark.parametrize("label, f, want", list(bgzf_ref.damaged_files()), ids=[c[0] for c in bgzf_ref.damaged_files()])
def test_the_walk_gives_the_statuses_of_the_contract(label, f, want):
    w = bgzf_ref.walk(f)
    assert w.record() == want
    assert len(w.off) == len(w.out_off) == w.nmembers + 1 and w.off[-1] == w.file_used and w.out_off[-1] == w.total_out
    if w.nmembers:                                                       # the members in front of a failure stay valid
        sound = f[:w.file_used]
        assert "ISIZE" in label or len(gzip.decompress(sound)) == w.total_out
