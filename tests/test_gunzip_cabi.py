"""CPU: the extension header include/hdlz_gunzip.h -- both declarations exported and bound with their arity, the work-bytes query equal
to its closed form, every parameter refusal in its order and in front of the device, no CPU path behind good parameters; and the
member rule as tests/gunzip_ref.py states it held against stock zlib (zlib.decompressobj(31), gzip.decompress) on every case the GPU
tests run."""
import ctypes
import gzip
import zlib

import pytest

import gunzip_ref as G
from cabi_common import declarations, header, host_buffer as _host_buffer, no_device as _no_device, r256

E_BAD_PARAM, E_HIP = 8, 9


def test_every_declaration_is_exported_and_bound():
    from hdl_deflate_amd import _lib
    text = header("hdlz_gunzip.h")
    params = declarations(text)
    assert params == {"hdlz_gunzip_work_bytes": 4, "hdlz_gunzip_ws": 14}
    assert sorted(params) == sorted(_lib.GUNZIP_EXPORTS) == sorted(_lib.GUNZIP_SIGNATURES)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    L = _lib.load()
    for name, n in params.items():
        assert hasattr(raw, name), name
        restype, argtypes = _lib.GUNZIP_SIGNATURES[name]
        assert len(argtypes) == n, name
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert '#include "hdlz_gzip.h"' in text
    # the call takes the checked call's parameters without flags and obsize; d_crc stands where d_adler stood
    c = list(_lib.SIGNATURES["hdlz_inflate_checked"][1])
    assert _lib.GUNZIP_SIGNATURES["hdlz_gunzip_ws"][1] == c[:5] + c[7:]
    assert _lib.GUNZIP_SIGNATURES["hdlz_gunzip_work_bytes"][1] == [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int]


def test_the_tables_in_front_of_it_are_as_they_were():
    from hdl_deflate_amd import _lib
    older = (_lib.EXPORTS, _lib.JOIN_EXPORTS, _lib.UNJOIN_EXPORTS, _lib.GZIP_EXPORTS, _lib.BGZF_EXPORTS, _lib.BGZF_RANGE_EXPORTS, _lib.BGZF_STORED_EXPORTS)
    assert [len(t) for t in older] == [22, 4, 2, 7, 8, 2, 3]
    assert len(_lib.GUNZIP_EXPORTS) == 2 and not set(_lib.GUNZIP_EXPORTS) & set().union(*older)
    assert _lib.load().hdlz_version() == 0x000600
    assert "hdlz_gunzip.h" in header("hdlz_gzip.h")          # the "out of scope" sentence points here


def test_the_query_is_its_closed_form():
    from hdl_deflate_amd import _lib
    L = _lib.load()

    def tiles(n, pitch):
        t = (min(pitch, (1 << 32) - 1) + 32767) // 32768
        return n * t if pitch >= 65536 and n * t < 1 << 31 else 0

    for n in (1, 2, 21, 22, 64, 65, 4096, (1 << 31) - 1):
        for pitch in (0, 4, 2048, 65532, 65536, 65540, 131072, 1 << 24, (1 << 32) - 4):
            for in_len in (0, 10, 2047, 2048, 1 << 20, (1 << 28) - 1):
                for ragged in (0, 1):
                    d = r256(L.hdlz_inflate_work_bytes(1, in_len, pitch, 0, 1)) if n == 1 else 0
                    want = r256(12 * n) + r256(16 * n) + r256(4 * tiles(n, pitch)) + d
                    assert L.hdlz_gunzip_work_bytes(n, in_len, pitch, ragged) == want, (n, in_len, pitch, ragged)
    assert L.hdlz_gunzip_work_bytes(2, 64, 65536, 0) == 256 + 256 + 256 and L.hdlz_gunzip_work_bytes(2, 64, 65532, 0) == 512
    assert L.hdlz_gunzip_work_bytes(1, 1 << 20, 1 << 22, 0) > L.hdlz_gunzip_work_bytes(1, 2047, 1 << 22, 0)      # the whole-GPU path's share
    # what the call refuses has no size: no streams, 2^31 streams, a row length of 2^28 (a ragged bound of that size is no bound),
    # rows of 2^32 for more than one stream
    assert L.hdlz_gunzip_work_bytes(0, 64, 64, 0) == 0 and L.hdlz_gunzip_work_bytes(1 << 31, 64, 64, 0) == 0
    assert L.hdlz_gunzip_work_bytes(1, 1 << 28, 64, 0) == 0 and L.hdlz_gunzip_work_bytes(1, 1 << 28, 64, 1) == L.hdlz_gunzip_work_bytes(1, 0, 64, 1)
    assert L.hdlz_gunzip_work_bytes(2, 64, 1 << 32, 0) == 0 and L.hdlz_gunzip_work_bytes(1, 64, 1 << 32, 0) != 0


def test_parameter_errors_come_before_the_device_in_their_order():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    keep, base = _host_buffer(1 << 16)
    wb = L.hdlz_gunzip_work_bytes(2, 64, 64, 0)
    assert wb == 512
    good = dict(d_in=base, in_off=None, in_pitch=64, in_len=64, n=2, out=base + 1024, out_pitch=64, out_len=base + 2048, status=base + 2304,
                used=base + 2560, crc=base + 2816, work=base + 4096, work_bytes=wb)

    def call(**kw):
        a = dict(good, **kw)
        return L.hdlz_gunzip_ws(a["d_in"], a["in_off"], a["in_pitch"], a["in_len"], a["n"], a["out"], a["out_pitch"], a["out_len"], a["status"],
                                a["used"], a["crc"], a["work"], a["work_bytes"], None)

    # every refusal alone, in the order of the header's list: (the bad argument, a word of its message)
    faults = [(dict(used=None), b"d_in_used is required"), (dict(n=1 << 31), b"nstreams too large"), (dict(d_in=None), b"null device pointer"),
              (dict(in_len=1 << 28, in_pitch=1 << 28), b"in_len too large"), (dict(in_pitch=63), b"in_pitch < in_len"),
              (dict(out_pitch=1 << 32), b"out_pitch too large"), (dict(out_pitch=66), b"d_out / out_pitch"), (dict(in_off=base + 4), b"d_in_off"),
              (dict(crc=base + 2818), b"d_out_len / d_status / d_in_used / d_crc"), (dict(work=base + 4096 + 128), b"256-byte"),
              (dict(work_bytes=wb - 1), b"hdlz_gunzip_work_bytes")]
    for kw, word in faults:
        assert call(**kw) == E_BAD_PARAM and word in L.hdlz_last_error(), (kw, L.hdlz_last_error())
    # ... and every pair: the earlier one answers
    for i, (kw_i, word_i) in enumerate(faults):
        for kw_j, _ in faults[i + 1:]:
            if set(kw_i) & set(kw_j) or ("in_off" in kw_j and {"in_len", "in_pitch"} & set(kw_i)):      # (a ragged call has no row length)
                continue
            assert call(**dict(kw_j, **kw_i)) == E_BAD_PARAM and word_i in L.hdlz_last_error(), (kw_i, kw_j, L.hdlz_last_error())
    for k in ("out", "out_len", "status"):
        assert call(**{k: None}) == E_BAD_PARAM and b"null device pointer" in L.hdlz_last_error(), k
    for k in ("out_len", "status", "used"):
        assert call(**{k: good[k] + 2}) == E_BAD_PARAM and b"4-byte" in L.hdlz_last_error(), k
    assert call(out=good["out"] + 2) == E_BAD_PARAM and b"4-byte" in L.hdlz_last_error()
    assert call(work=None) == E_BAD_PARAM and b"hdlz_gunzip_work_bytes" in L.hdlz_last_error()
    assert call(used=None, n=0, work=None, work_bytes=0) == E_BAD_PARAM                       # required, always
    if _no_device():
        assert call() == E_HIP
        assert call(crc=None) == E_HIP                                                         # nullable
        assert call(in_off=base + 8, in_len=0) == E_HIP and call(in_off=base, in_len=1 << 28) == E_HIP      # ragged: a bound nobody can use is no bound
        assert call(d_in=base + 1, in_pitch=65) == E_HIP                                       # any alignment of the streams
        assert call(n=0, d_in=None, out=None, out_len=None, status=None, work=None, work_bytes=0) == E_HIP
        one = L.hdlz_gunzip_work_bytes(1, 64, 1 << 32, 0)
        assert call(n=1, out_pitch=1 << 32, work_bytes=one) == E_HIP                           # one stream: rows of any size


def _case_ids():
    return [label for label, _ in G.all_cases()]


@pytest.mark.parametrize("k", range(len(G.all_cases())), ids=_case_ids())
def test_the_rule_accepts_what_zlib_accepts(oracle, k):
    """every case of the GPU tests: the rule answers OK exactly where zlib.decompressobj(31) reaches the member's end without an error,
    with zlib's bytes and zlib's count of consumed bytes; and a refusal names a step"""
    label, z = G.all_cases()[k]
    e = G.member(oracle, z, 65532)
    za = G.zaccepts(z)
    assert (e["status"] == G.OK) == (za is not None), (label, e["status"])
    if za is not None:
        assert (e["data"], e["in_used"]) == za and e["crc"] == zlib.crc32(za[0]) and e["out_len"] == len(za[0])
    else:
        assert e["status"] in (G.E_SHORT_INPUT, G.E_NO_EOF, G.E_BAD_HEADER, G.E_BAD_CHECKSUM, 10) and e["out_len"] == 0
        assert (e["in_used"] != 0) == (e["status"] == G.E_BAD_CHECKSUM)


def test_what_zlib_says_about_the_header_fields():
    """the points of RFC 1952 the rule leans on, as this machine's zlib answers them"""
    d = G.text(300, 1)
    assert G.zaccepts(G.gz(d, extra=b"ab\x02\x00xy", name=b"file.txt", comment=b"a comment", hcrc=True, flg=G.FTEXT))[0] == d
    for bad, word in ((G.gz(d, name=b"x", hcrc=True, hcrc_xor=1), "header crc mismatch"), (G.gz(d, flg=0x20), "unknown header flags"),
                      (G.gz(d, flg=0x80), "unknown header flags"), (G.gz(d, crc_xor=1), "incorrect data check"),
                      (G.gz(d, isize_add=1), "incorrect length check"), (G.gz(d, cm=7), "unknown compression method")):
        with pytest.raises(zlib.error, match=word):
            zlib.decompressobj(31).decompress(bad)
    a, b = G.gz(d, name=b"a"), G.gz(d[:100], hcrc=True)
    dd = zlib.decompressobj(31)
    assert dd.decompress(a + b) == d and dd.eof and dd.unused_data == b
    assert gzip.decompress(a + b + bytes(7)) == d + d[:100] and gzip.decompress(b"") == b""
    with pytest.raises(Exception):
        gzip.decompress(a + b"garbage behind")


def test_capacity_is_the_decoders_status(oracle):
    z = G.gz(G.text(1000, 9), name=b"cap")
    assert G.member(oracle, z, 1000)["status"] == G.OK and G.member(oracle, z, 996)["status"] == G.E_OUT_CAPACITY
    assert G.member(oracle, G.header(name=b"n") + b"\x03", 64)["status"] == G.E_SHORT_INPUT      # a payload of fewer than 3 bytes
