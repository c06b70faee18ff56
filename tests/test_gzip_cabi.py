"""CPU: the extension header include/hdlz_gzip.h -- every declaration exported and bound with its arity, the struct mirrors, the
queries equal to their closed forms, parameter errors in front of the device, no CPU path behind good parameters; the gzip stream of
gzip_ref read back by stock readers; and the CRC-32 tile / tree combination rule of hdlz_crc32.h stated in Python (gzip_ref) and
held against zlib.crc32 before any kernel sees it."""
import ctypes
import gzip
import zlib

import numpy as np
import pytest

import gzip_ref
from cabi_common import check_struct_mirror, declarations, header, host_buffer as _host_buffer, no_device as _no_device, r256

E_BAD_PARAM, E_HIP = 8, 9
LANE, WAVE, GROUP = 2, 4, 64


def _header():
    return header("hdlz_gzip.h")


def _declarations():
    return declarations(_header())


def test_every_declaration_is_exported_and_bound():
    from hdl_deflate_amd import _lib
    params = _declarations()
    assert params == {"hdlz_crc32_work_bytes": 1, "hdlz_crc32_ws": 6, "hdlz_join_gzip_bound": 2, "hdlz_join_gzip_work_bytes": 1,
                      "hdlz_join_gzip_ws": 16, "hdlz_unjoin_gzip_work_bytes": 3, "hdlz_unjoin_gzip_ws": 14}
    assert sorted(params) == sorted(_lib.GZIP_EXPORTS) == sorted(_lib.GZIP_SIGNATURES)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    L = _lib.load()
    for name, n in params.items():
        assert hasattr(raw, name), name
        restype, argtypes = _lib.GZIP_SIGNATURES[name]
        assert len(argtypes) == n, name
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert '#include "hdlz_unjoin.h"' in _header()
    # the two calls that mirror an older one take that one's parameters (the join: d_crc behind the first eight)
    j = list(_lib.JOIN_SIGNATURES["hdlz_join_batch_ws"][1])
    assert _lib.GZIP_SIGNATURES["hdlz_join_gzip_ws"][1] == j[:8] + [ctypes.c_void_p] + j[8:]
    assert _lib.GZIP_SIGNATURES["hdlz_unjoin_gzip_ws"][1] == _lib.UNJOIN_SIGNATURES["hdlz_unjoin_ws"][1]


def test_the_tables_in_front_of_it_are_as_they_were():
    from hdl_deflate_amd import _lib
    assert len(_lib.EXPORTS) == 22 and len(_lib.JOIN_EXPORTS) == 4 and len(_lib.UNJOIN_EXPORTS) == 2 and len(_lib.GZIP_EXPORTS) == 7
    assert not set(_lib.GZIP_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.JOIN_EXPORTS) | set(_lib.UNJOIN_EXPORTS))
    assert _lib.load().hdlz_version() == 0x000600


@pytest.mark.parametrize("struct, mirror, want", [
    ("hdlz_join_gzip_result", "JoinGzipResult", [("uint64_t", "stream_len"), ("uint32_t", "status"), ("uint32_t", "crc")]),
    ("hdlz_unjoin_gzip_result", "UnjoinGzipResult", [("uint64_t", "out_len"), ("uint64_t", "first_bad"), ("uint32_t", "status"), ("uint32_t", "crc")]),
])
def test_struct_mirrors_match_the_header(struct, mirror, want):
    from hdl_deflate_amd import _lib
    check_struct_mirror(_header(), struct, getattr(_lib, mirror), want)


def test_the_queries_are_their_closed_forms():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    for n in (0, 1, 32767, 32768, 32769, 64 * 32768, 64 * 32768 + 1, 1 << 31, 1 << 40):
        assert L.hdlz_crc32_work_bytes(n) == r256(4 * ((n + 32767) // 32768)), n
    assert L.hdlz_crc32_work_bytes(0) == 0
    for nb in (0, 1, 255, 256, 257, 1 << 20, (1 << 31) - 1, 1 << 31):
        assert L.hdlz_join_gzip_work_bytes(nb) == L.hdlz_join_work_bytes(nb), nb
        for in_len in (5, 2048, 65536):
            assert L.hdlz_join_gzip_bound(nb, in_len) == L.hdlz_join_bound(nb, in_len) + 12 == 20 + nb * (L.hdlz_out_bound(in_len) - 1)
    for n in (0, 1, 255, 256, 257, 1 << 20, (1 << 31) - 1):
        lists = 0 if n == 0 else max(256, r256(4 * (2 + 130 + n + (n if n > 64 else 0))))
        for flags in (0, LANE, WAVE, GROUP):
            for total in (0, 1, 32767, 32768, 32769, 1 << 40):
                want = r256(12 * n) + r256(4 * ((total + 32767) // 32768)) + r256(lists)
                assert L.hdlz_unjoin_gzip_work_bytes(n, total, flags) == want, (n, total, flags)
    for total in (0, 1, 32768, 1 << 40):
        assert L.hdlz_unjoin_gzip_work_bytes(1 << 31, total, 0) == 0


def test_crc32_parameter_errors_come_before_the_device():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    keep, base = _host_buffer()
    wb = L.hdlz_crc32_work_bytes(64)
    assert wb == 256

    def crc(data=base, n=64, out=base + 1024, work=base + 2048, work_bytes=wb):
        return L.hdlz_crc32_ws(data, n, out, work, work_bytes, None)
    assert crc(out=None) == E_BAD_PARAM
    assert crc(data=None) == E_BAD_PARAM
    assert crc(work=None) == E_BAD_PARAM and b"hdlz_crc32_work_bytes" in L.hdlz_last_error()
    assert crc(work_bytes=wb - 1) == E_BAD_PARAM and b"hdlz_crc32_work_bytes" in L.hdlz_last_error()
    assert crc(out=base + 1026) == E_BAD_PARAM and b"4-byte" in L.hdlz_last_error()
    assert crc(out=None, n=0, data=None, work=None, work_bytes=0) == E_BAD_PARAM
    if _no_device():
        assert crc() == E_HIP
        assert crc(data=base + 1) == E_HIP and crc(data=base + 15, n=3) == E_HIP        # any alignment
        assert crc(data=None, n=0, work=None, work_bytes=0) == E_HIP                      # nothing to read, no scratch


def test_join_parameter_errors_come_before_the_device():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    keep, base = _host_buffer()
    wb = L.hdlz_join_gzip_work_bytes(1)
    assert 0 < wb <= 4096

    def join(rows=base, length=base, end_bits=base, status=base, in_off=None, crc=base, stream=base, off=base, result=base, work=base,
             work_bytes=wb, nblocks=1):
        return L.hdlz_join_gzip_ws(rows, 64, length, end_bits, status, in_off, 64, nblocks, crc, stream, 4096, off, result, work, work_bytes, None)
    for k in ("rows", "length", "end_bits", "status", "crc", "stream", "off", "result", "work"):
        assert join(**{k: None}) == E_BAD_PARAM, k
    assert join(crc=None, nblocks=0, work=None, work_bytes=0) == E_BAD_PARAM and b"d_crc" in L.hdlz_last_error()     # required, always
    assert join(nblocks=1 << 31) == E_BAD_PARAM and b"2^31" in L.hdlz_last_error()
    assert join(work_bytes=wb - 1) == E_BAD_PARAM and b"hdlz_join_gzip_work_bytes" in L.hdlz_last_error()
    for k in ("off", "result", "work"):
        assert join(**{k: base + 4}) == E_BAD_PARAM and b"8-byte" in L.hdlz_last_error(), k
    assert join(crc=base + 2) == E_BAD_PARAM and b"4-byte" in L.hdlz_last_error()
    if _no_device():
        assert join() == E_HIP
        assert join(in_off=base) == E_HIP
        assert join(nblocks=0, rows=None, length=None, end_bits=None, status=None, work=None, work_bytes=0) == E_HIP


def test_unjoin_parameter_errors_come_before_the_device():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    keep, base = _host_buffer()
    wb = L.hdlz_unjoin_gzip_work_bytes(1, 64, 0)
    assert 0 < wb <= 8192

    def unjoin(stream=base, off=base, out_off=None, out=base, out_cap=64, status=None, result=base, work=base, work_bytes=wb, nmembers=1, flags=0):
        return L.hdlz_unjoin_gzip_ws(stream, 64, off, out_off, 64, nmembers, flags, out, out_cap, status, result, work, work_bytes, None)
    for k in ("stream", "off", "out", "result", "work"):
        assert unjoin(**{k: None}) == E_BAD_PARAM, k
    assert unjoin(nmembers=1 << 31) == E_BAD_PARAM and b"2^31" in L.hdlz_last_error()
    assert unjoin(out=base + 2) == E_BAD_PARAM and b"4-byte" in L.hdlz_last_error()
    for k in ("off", "out_off", "result"):
        assert unjoin(**{k: base + 4}) == E_BAD_PARAM and b"8-byte" in L.hdlz_last_error(), k
    assert unjoin(work=base + 128) == E_BAD_PARAM and b"256-byte" in L.hdlz_last_error()
    assert unjoin(work_bytes=wb - 1) == E_BAD_PARAM and b"hdlz_unjoin_gzip_work_bytes" in L.hdlz_last_error()
    for flags in (1, 8, 128, 256, LANE | WAVE, LANE | GROUP, WAVE | GROUP, LANE | 1):
        assert unjoin(flags=flags) == E_BAD_PARAM, flags
    if _no_device():
        assert unjoin() == E_HIP
        assert unjoin(status=base, out_off=base) == E_HIP
        for flags in (LANE, WAVE, GROUP):
            assert unjoin(flags=flags) == E_HIP
        assert unjoin(nmembers=0, work=None, work_bytes=0, out=None, out_cap=0) == E_HIP


def test_other_container_names_are_refused_before_anything_runs():
    from hdl_deflate_amd import engine
    assert engine._container_is_gzip("gzip") and not engine._container_is_gzip("zlib")
    for name in ("gz", "GZIP", "raw", "", None, 31):
        with pytest.raises(ValueError):
            engine._container_is_gzip(name)


def _batches():
    r = np.random.default_rng(20261018)
    text = bytes(r.choice(np.frombuffer(b"abcdefgh \n", np.uint8), 4000))
    rand = bytes(r.integers(0, 256, 2000, dtype=np.uint8))
    yield 32, 10, []
    yield 32, 10, [text[:5]]
    yield 256, 10, [text[a:a + n] for a, n in ((0, 37), (100, 5), (300, 2048), (2500, 300))] + [rand[:64], bytes(50), rand[64:1300]]
    yield 20, 5, [text[k * 11:k * 11 + 5 + k] for k in range(40)] + [rand[k * 7:k * 7 + 5 + (k * 13) % 60] for k in range(40)]


@pytest.mark.parametrize("cw, mm, blocks", list(_batches()), ids=lambda v: str(len(v)) if isinstance(v, list) else str(v))
def test_stock_readers_read_the_reference_stream(cw, mm, blocks):
    g = gzip_ref.expected_gzip(blocks, cw, mm)
    z = g.zlib_form
    assert g.stream[:10] == bytes.fromhex("1f8b0800" "00000000" "00ff") and g.offsets[0] == 10
    assert len(g.stream) == len(z.stream) + 12 and g.stream[10:g.offsets[-1]] == z.stream[2:z.offsets[-1]]
    assert g.stream[g.offsets[-1]:] == b"\x03\x00" + zlib.crc32(g.data).to_bytes(4, "little") + (len(g.data) & 0xFFFFFFFF).to_bytes(4, "little")
    assert gzip.decompress(g.stream) == g.data
    d = zlib.decompressobj(31)
    assert d.decompress(g.stream + b"behind") == g.data and d.eof and d.unused_data == b"behind"
    if not blocks:
        assert g.stream == bytes.fromhex("1f8b0800" "00000000" "00ff" "0300" "00000000" "00000000") and len(g.stream) == 20
    for at in (-8, -5, -4, -1):                                     # a flipped CRC byte, a flipped ISIZE byte
        bad = bytearray(g.stream)
        bad[at] ^= 0x10
        with pytest.raises(zlib.error):
            zlib.decompressobj(31).decompress(bytes(bad))


def test_the_arithmetic_identities():
    r = np.random.default_rng(7)
    a, b = bytes(r.integers(0, 256, 300, dtype=np.uint8)), bytes(r.integers(0, 256, 77, dtype=np.uint8))
    raw, mul, xpow = gzip_ref.raw, gzip_ref.mul, gzip_ref.xpow
    assert raw(bytes(19) + a) == raw(a)
    assert raw(a + b) == raw(a + bytes(len(b))) ^ raw(b) == mul(raw(a), xpow(8 * len(b))) ^ raw(b)
    for x in (a, b, a + b, b"abcd"):
        assert zlib.crc32(x) == raw(x) ^ raw(b"\xff\xff\xff\xff" + bytes(len(x) - 4)) ^ 0xFFFFFFFF
        assert zlib.crc32(x) == raw(x) ^ mul(0xFFFFFFFF, xpow(8 * len(x))) ^ 0xFFFFFFFF      # ... as a word in front, any length
    assert zlib.crc32(b"") == mul(0xFFFFFFFF, xpow(0)) ^ 0xFFFFFFFF == 0
    assert xpow(0xFFFFFFFF) == gzip_ref.ONE and mul(xpow(8 * 1000), xpow(0xFFFFFFFF - 8 * 1000)) == gzip_ref.ONE      # x^-e
    assert gzip_ref.XP2[10] == xpow(8 * 128) and gzip_ref.XP2[18] == xpow(8 * 32768) and gzip_ref.XP2[28] == xpow(8 * 32768 * 1024)
    assert mul(gzip_ref.XP2[31], gzip_ref.XP2[31]) == gzip_ref.XP2[0]                        # x^(2^k): k counts mod 32


PINNED = [(b"123456789", 0xCBF43926), (bytes(32768), 0x011FFCA6), (b"\xff" * 65536, 0xDEAB7E4E),
          (bytes((7 * p + 3) & 255 for p in range(70001)), 0x5C5C297A), (b"", 0)]


@pytest.mark.parametrize("k", range(len(PINNED)))
def test_the_rule_gives_the_pinned_values(k):
    data, want = PINNED[k]
    assert zlib.crc32(data) == want == gzip_ref.crc32_by_rule(data)


def test_the_tile_word_is_the_raw_register_of_the_padded_tile():
    r = np.random.default_rng(11)
    for n in (1, 127, 128, 129, 8191, 8192, 8193, 32767, 32768):
        for tile in (bytes(r.integers(0, 256, n, dtype=np.uint8)), bytes(n), b"\xff" * n):
            assert gzip_ref.tile_word(tile) == gzip_ref.raw(tile + bytes(32768 - n)), n


@pytest.mark.parametrize("ntiles", [1, 2, 3, 255, 256, 257, 1023, 1024, 1025])
@pytest.mark.parametrize("tail", [0, 7, 32767])
def test_the_finishing_rule_for_tile_counts(ntiles, tail):
    """the tile words taken as given (zlib's register of the padded tile), the tree and the unpadding held against zlib.crc32"""
    r = np.random.default_rng(ntiles * 3 + tail)
    n = ntiles * 32768 - (32768 - tail if tail else 0)
    for data in (bytes(r.integers(0, 256, n, dtype=np.uint8)), bytes(n)):
        words = [gzip_ref.raw(data[o:o + 32768] + bytes(max(0, o + 32768 - n))) for o in range(0, n, 32768)]
        assert len(words) == (n + 32767) // 32768
        assert gzip_ref.crc32_from_words(words, n) == zlib.crc32(data), (ntiles, tail)
