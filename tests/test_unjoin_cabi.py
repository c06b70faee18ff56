"""CPU: the extension header include/hdlz_unjoin.h -- every declaration exported and bound with its arity, the struct mirror, the
scratch query equal to its closed form, parameter errors in front of the device, no CPU path behind good parameters; and the judge's
member rule (end bit -> three zero bits -> 00 00 FF FF -> the next offset) stated in Python and held against joined_ref before any
kernel sees it."""
import ctypes

import numpy as np

import joined_ref
from cabi_common import check_struct_mirror, declarations, header, r256

E_BAD_PARAM, E_HIP = 8, 9
LANE, WAVE, GROUP = 2, 4, 64


def _header():
    return header("hdlz_unjoin.h")


def _declarations():
    return declarations(_header())


def test_every_declaration_is_exported_and_bound():
    from hdl_deflate_amd import _lib
    params = _declarations()
    assert params == {"hdlz_unjoin_work_bytes": 3, "hdlz_unjoin_ws": 14}
    assert sorted(params) == sorted(_lib.UNJOIN_EXPORTS) == sorted(_lib.UNJOIN_SIGNATURES)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    L = _lib.load()
    for name, n in params.items():
        assert hasattr(raw, name), name
        restype, argtypes = _lib.UNJOIN_SIGNATURES[name]
        assert len(argtypes) == n, name
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert '#include "hdlz_join.h"' in _header()


def test_the_tables_in_front_of_it_are_as_they_were():
    from hdl_deflate_amd import _lib
    assert len(_lib.EXPORTS) == 22 and len(_lib.JOIN_EXPORTS) == 4 and len(_lib.UNJOIN_EXPORTS) == 2
    assert not set(_lib.UNJOIN_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.JOIN_EXPORTS))
    assert _lib.load().hdlz_version() == 0x000600


def test_struct_mirror_matches_the_header():
    from hdl_deflate_amd import _lib
    R = _lib.UnjoinResult
    check_struct_mirror(_header(), "hdlz_unjoin_result", R, [("uint64_t", "out_len"), ("uint64_t", "first_bad"), ("uint32_t", "status"), ("uint32_t", "adler")])
    assert ctypes.sizeof(R) == 24 and (R.out_len.offset, R.first_bad.offset, R.status.offset, R.adler.offset) == (0, 8, 16, 20)


def test_the_work_size_is_its_closed_form():
    import hdl_deflate_amd
    from hdl_deflate_amd import _lib
    L = _lib.load()
    for n in (0, 1, 255, 256, 257, 1 << 20, (1 << 31) - 1):
        # the batch decode's share, a ragged batch of n streams (include/hdlz.h): the lists of the lane mapping, 256 bytes at least
        lists = 0 if n == 0 else max(256, r256(4 * (2 + 130 + n + (n if n > 64 else 0))))
        for flags in (0, LANE, WAVE, GROUP):
            assert L.hdlz_inflate_work_bytes(n, 0, 0, flags, 1) == lists, (n, flags)
            for total in (0, 1, 32767, 32768, 32769, 1 << 40):
                want = r256(12 * n) + r256(8 * ((total + 32767) // 32768)) + r256(lists)
                assert L.hdlz_unjoin_work_bytes(n, total, flags) == want == hdl_deflate_amd.unjoin_work_bytes(n, total, flags), (n, total, flags)
    for total in (0, 1, 32768, 1 << 40):
        assert L.hdlz_unjoin_work_bytes(1 << 31, total, 0) == 0


def test_parameter_errors_come_before_the_device():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    buf = (ctypes.c_uint8 * 16384)()
    base = ctypes.addressof(buf)
    base += -base % 256
    wb = L.hdlz_unjoin_work_bytes(1, 64, 0)
    assert 0 < wb <= 8192

    def unjoin(stream=base, off=base, out_off=None, out=base, out_cap=64, status=None, result=base, work=base, work_bytes=wb, nmembers=1, flags=0):
        return L.hdlz_unjoin_ws(stream, 64, off, out_off, 64, nmembers, flags, out, out_cap, status, result, work, work_bytes, None)
    for k in ("stream", "off", "out", "result", "work"):
        assert unjoin(**{k: None}) == E_BAD_PARAM, k
    assert unjoin(nmembers=1 << 31) == E_BAD_PARAM and b"2^31" in L.hdlz_last_error()
    assert unjoin(out=base + 2) == E_BAD_PARAM and b"4-byte" in L.hdlz_last_error()
    for k in ("off", "out_off", "result"):
        assert unjoin(**{k: base + 4}) == E_BAD_PARAM and b"8-byte" in L.hdlz_last_error(), k
    assert unjoin(work=base + 8) == E_BAD_PARAM and b"256-byte" in L.hdlz_last_error()
    assert unjoin(work=base + 128) == E_BAD_PARAM and b"256-byte" in L.hdlz_last_error()
    assert unjoin(work_bytes=wb - 1) == E_BAD_PARAM and b"hdlz_unjoin_work_bytes" in L.hdlz_last_error()
    for flags in (1, 8, 128, 256, LANE | WAVE, LANE | GROUP, WAVE | GROUP, LANE | 1):
        assert unjoin(flags=flags) == E_BAD_PARAM, flags
    import torch
    if torch.cuda.is_available():
        return                       # (with a device the good calls below would run kernels on these host buffers)
    assert unjoin() == E_HIP
    assert unjoin(status=base, out_off=base) == E_HIP
    assert unjoin(out=None, out_cap=0) == E_HIP                      # d_out is only required when there is room for output
    for flags in (LANE, WAVE, GROUP):
        assert unjoin(flags=flags) == E_HIP
    assert unjoin(nmembers=0, work=None, work_bytes=0, out=None, out_cap=0) == E_HIP


def _batches():
    r = np.random.default_rng(20261018)
    text = bytes(r.choice(np.frombuffer(b"abcdefgh \n", np.uint8), 4000))
    rand = bytes(r.integers(0, 256, 2000, dtype=np.uint8))
    yield [text[:5]]
    yield [text[a:a + n] for a, n in ((0, 37), (100, 5), (300, 2048), (2500, 300))] + [rand[:64], bytes(50), rand[64:1300]]
    yield [text[k * 11:k * 11 + 5 + k] for k in range(40)] + [rand[k * 7:k * 7 + 5 + (k * 13) % 60] for k in range(40)]


def member_ends_where_the_index_says(stream, lo, hi, e):
    """the judge's rule (include/hdlz_unjoin.h, check 4): e = the first bit behind the end-of-block code, counted from byte lo - 2"""
    base = lo - 2
    bit = lambda p: (stream[base + (p >> 3)] >> (p & 7)) & 1
    if bit(e) or bit(e + 1) or bit(e + 2):
        return False
    q = (e + 3 + 7) >> 3
    return stream[base + q:base + q + 4] == b"\x00\x00\xff\xff" and base + q + 4 == hi


def test_the_member_rule_holds_for_every_member_of_the_reference():
    marker = set()
    for cw, mm, blocks in zip((32, 256, 20), (10, 10, 5), _batches()):
        j = joined_ref.expected_joined(blocks, cw, mm)
        for b, E in enumerate(j.end_bits):
            lo, hi = j.offsets[b], j.offsets[b + 1]
            e = E + 7                                    # the row's first bit is the bit of byte lo - 2: the 2 header bytes are the same 16 bits
            assert (j.stream[lo] >> 1) & 3 == 1 and j.stream[lo] & 1 == 0
            assert member_ends_where_the_index_says(j.stream, lo, hi, e), (cw, mm, b)
            # ... and for no other end bit nearby that a decoder could report by mistake, nor for a neighbour's offset
            assert not member_ends_where_the_index_says(j.stream, lo, hi + 1, e) and not member_ends_where_the_index_says(j.stream, lo, hi - 1, e)
            assert not member_ends_where_the_index_says(j.stream, lo, hi, e + 8) and not member_ends_where_the_index_says(j.stream, lo, hi, e - 8)
            marker.add(hi - lo - (len(j.rows[b]) - 6))
            assert hi - lo >= 5
        assert j.stream[j.offsets[-1]:j.offsets[-1] + 2] == b"\x03\x00"
    assert marker == {4, 5}
