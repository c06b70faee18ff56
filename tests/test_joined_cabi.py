"""CPU: the extension header include/hdlz_join.h -- every declaration exported and bound with its arity, the two size queries equal to
their closed forms, parameter errors in front of the device, no CPU path behind good parameters; and the reference side of the GPU
tests (joined_ref.expected_joined) against stock zlib."""
import ctypes
import zlib

import numpy as np

import joined_ref
from cabi_common import check_struct_mirror, declarations, header

E_BAD_PARAM, E_HIP = 8, 9


def _declarations():
    return declarations(header("hdlz_join.h"))


def test_every_declaration_is_exported_and_bound():
    from hdl_deflate_amd import _lib
    params = _declarations()
    assert params == {"hdlz_join_bound": 2, "hdlz_join_work_bytes": 1, "hdlz_compress_batch_bits": 13, "hdlz_join_batch_ws": 15}
    assert sorted(params) == sorted(_lib.JOIN_EXPORTS) == sorted(_lib.JOIN_SIGNATURES)
    assert not set(_lib.JOIN_EXPORTS) & set(_lib.EXPORTS) and len(_lib.EXPORTS) == 22          # additive: hdlz.h's table is as it was
    raw = ctypes.CDLL(_lib.LIB_PATH)
    L = _lib.load()
    for name, n in params.items():
        assert hasattr(raw, name), name
        restype, argtypes = _lib.JOIN_SIGNATURES[name]
        assert len(argtypes) == n, name
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert L.hdlz_version() == 0x000600
    assert ctypes.sizeof(_lib.JoinResult) == 16 and _lib.JoinResult.status.offset == 8 and _lib.JoinResult.adler.offset == 12
    check_struct_mirror(header("hdlz_join.h"), "hdlz_join_result", _lib.JoinResult, [("uint64_t", "stream_len"), ("uint32_t", "status"), ("uint32_t", "adler")])
    assert [f[0] for f in _lib.JoinResult._fields_] == ["stream_len", "status", "adler"]


def test_size_queries_are_their_closed_forms():
    import hdl_deflate_amd
    from hdl_deflate_amd import _lib
    L = _lib.load()
    for nblocks in (0, 1, 2, 255, 256, 257, 513, 1 << 20, (1 << 31) - 1):
        for in_len in (5, 64, 2047, 2048, 2049, 65536):
            want = 8 + nblocks * (L.hdlz_out_bound(in_len) - 1)
            assert L.hdlz_join_bound(nblocks, in_len) == want == hdl_deflate_amd.join_bound(nblocks, in_len), (nblocks, in_len)
        ntiles = (nblocks + 255) // 256
        want = (8 + 24 * ntiles + 255) // 256 * 256 if ntiles else 0          # ticket + pad, a look-back word and four sums per tile
        assert L.hdlz_join_work_bytes(nblocks) == want, nblocks
    assert L.hdlz_join_work_bytes(1 << 31) == 0
    # a member is a row without its 2 header and 4 trailer bytes plus at most 5 marker bytes: out_bound - 1
    assert L.hdlz_join_bound(0, 2048) == 8 == len(b"\x78\x9c\x03\x00\x00\x00\x00\x01")


def test_parameter_errors_come_before_the_device():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    buf = (ctypes.c_uint8 * 4096)()
    base = ctypes.addressof(buf)
    base += -base % 16
    wb = L.hdlz_join_work_bytes(1)

    def join(rows=base, length=base, bits=base, status=base, stream=base, off=base, result=base, work=base, work_bytes=wb, nblocks=1):
        return L.hdlz_join_batch_ws(rows, 64, length, bits, status, None, 64, nblocks, stream, 64, off, result, work, work_bytes, None)
    for k in ("rows", "length", "bits", "status", "stream", "off", "result", "work"):
        assert join(**{k: None}) == E_BAD_PARAM, k
    assert join(nblocks=1 << 31) == E_BAD_PARAM and b"2^31" in L.hdlz_last_error()
    assert join(work_bytes=wb - 1) == E_BAD_PARAM and b"hdlz_join_work_bytes" in L.hdlz_last_error()
    assert join(work=base + 4) == E_BAD_PARAM and b"8-byte" in L.hdlz_last_error()
    assert join(nblocks=0, rows=None, length=None, bits=None, status=None, stream=None) == E_BAD_PARAM       # the outputs stay required

    def bits(end_bits=base, cwindow=32, out_pitch=64):
        return L.hdlz_compress_batch_bits(base, None, 64, 64, 1, cwindow, 10, base, out_pitch, base, base, end_bits, None)
    assert bits(end_bits=None) == E_BAD_PARAM and b"d_end_bits" in L.hdlz_last_error()
    assert bits(end_bits=base + 4) == E_BAD_PARAM
    assert bits(cwindow=999) == E_BAD_PARAM and bits(out_pitch=66) == E_BAD_PARAM          # ... and hdlz_compress_batch's own
    import torch
    if torch.cuda.is_available():
        return                       # (with a device the good calls below would run kernels on these host buffers)
    assert join() == E_HIP
    assert join(nblocks=0, rows=None, length=None, bits=None, status=None, work=None, work_bytes=0) == E_HIP
    assert bits() == E_HIP


def _batches():
    r = np.random.default_rng(20261018)
    text = bytes(r.choice(np.frombuffer(b"abcdefgh \n", np.uint8), 4000))
    rand = bytes(r.integers(0, 256, 2000, dtype=np.uint8))
    yield [text[:5]]
    yield [text[a:a + n] for a, n in ((0, 37), (100, 5), (300, 2048), (2500, 300))] + [rand[:64], bytes(50), rand[64:1300]]
    yield [text[k * 11:k * 11 + 5 + k] for k in range(40)] + [rand[k * 7:k * 7 + 5 + (k * 13) % 60] for k in range(40)]


def test_expected_joined_is_a_zlib_stream_of_the_concatenation():
    """the reference of the GPU tests, on three small batches: stock zlib reads it back, its trailer is zlib's checksum, exactly one of
    the two markers decodes behind every block (asserted inside), and both marker lengths occur"""
    lens = set()
    for cw, mm, blocks in zip((32, 256, 20), (10, 10, 5), _batches()):
        j = joined_ref.expected_joined(blocks, cw, mm)
        d = zlib.decompressobj()
        assert d.decompress(j.stream) == b"".join(blocks) and d.eof and d.unused_data == b""
        assert j.stream[-4:] == zlib.adler32(b"".join(blocks)).to_bytes(4, "big") and j.stream[-6:-4] == b"\x03\x00"
        for z, E, p, m in zip(j.rows, j.end_bits, j.pads, j.members):
            assert len(z) == ((E + 14) >> 3) + 4 and len(m) == len(z) - 6 + (4 if p >= 3 else 5)
            lens.add(len(m) - (len(z) - 6))
    assert lens == {4, 5}
    assert joined_ref.expected_joined([], 32, 10).stream == b"\x78\x9c\x03\x00\x00\x00\x00\x01"


def test_the_adler_reduction_of_the_design_note():
    """s1 = 1 + sum A_b, s2 = N + N sum A_b - sum e_b A_b + sum (s2_b - n_b) (mod 65521) is zlib.adler32 of the concatenation"""
    M = 65521
    r = np.random.default_rng(7)
    for _ in range(50):
        blocks = [bytes(r.integers(0, 256, int(n), dtype=np.uint8)) for n in r.integers(5, 70000, int(r.integers(1, 9)))]
        N, e, sa, sea, ss = sum(len(b) for b in blocks), 0, 0, 0, 0
        for b in blocks:
            e += len(b)
            ad = zlib.adler32(b)
            A = ((ad & 0xFFFF) - 1) % M
            sa, sea, ss = sa + A, sea + e * A, ss + (ad >> 16) - len(b)
        s1, s2 = (1 + sa) % M, (N + N * sa - sea + ss) % M
        assert (s2 << 16) | s1 == zlib.adler32(b"".join(blocks))
