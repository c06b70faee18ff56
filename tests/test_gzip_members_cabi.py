"""CPU: the extension header include/hdlz_gzip_members.h -- its declarations exported and bound with their arity, both work-bytes
queries equal to their closed forms, every parameter refusal in its order and in front of the device, the older tables as they were;
and the rules of tests/gzip_members_ref.py (the index rule, the member verdict, the repair loop) held against gzip.decompress on the
files the GPU tests read, with the number of repairs each of them needs."""
import ctypes
import gzip

import pytest

import gunzip_ref as G
import gzip_members_ref as R
from cabi_common import check_struct_mirror, declarations, header, host_buffer as _host_buffer, no_device as _no_device, r256

E_BAD_PARAM, E_HIP = 8, 9


def test_every_declaration_is_exported_and_bound():
    from hdl_deflate_amd import _lib
    text = header("hdlz_gzip_members.h")
    params = declarations(text)
    assert params == {"hdlz_gzip_members_index_work_bytes": 1, "hdlz_gzip_members_index_ws": 9,
                      "hdlz_gzip_members_inflate_work_bytes": 1, "hdlz_gzip_members_inflate_ws": 12}
    assert sorted(params) == sorted(_lib.GZIP_MEMBERS_EXPORTS) == sorted(_lib.GZIP_MEMBERS_SIGNATURES)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    L = _lib.load()
    for name, n in params.items():
        assert hasattr(raw, name), name
        restype, argtypes = _lib.GZIP_MEMBERS_SIGNATURES[name]
        assert len(argtypes) == n, name
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert '#include "hdlz_gunzip.h"' in text
    # the index takes hdlz_bgzf_index_ws's parameters; the read hdlz_bgzf_inflate_ws's without flags
    assert _lib.GZIP_MEMBERS_SIGNATURES["hdlz_gzip_members_index_ws"][1] == _lib.BGZF_SIGNATURES["hdlz_bgzf_index_ws"][1]
    b = list(_lib.BGZF_SIGNATURES["hdlz_bgzf_inflate_ws"][1])
    assert _lib.GZIP_MEMBERS_SIGNATURES["hdlz_gzip_members_inflate_ws"][1] == b[:5] + b[6:]
    check_struct_mirror(text, "hdlz_gzip_members_index_result", _lib.GzipMembersIndexResult,
                        [("uint64_t", "nmembers"), ("uint64_t", "total_out"), ("uint32_t", "status"), ("uint32_t", "reserved")])
    check_struct_mirror(text, "hdlz_gzip_members_inflate_result", _lib.GzipMembersInflateResult,
                        [("uint64_t", "out_len"), ("uint64_t", "first_bad"), ("uint32_t", "status"), ("uint32_t", "reserved")])


def test_the_tables_in_front_of_it_are_as_they_were():
    from hdl_deflate_amd import _lib
    older = (_lib.EXPORTS, _lib.JOIN_EXPORTS, _lib.UNJOIN_EXPORTS, _lib.GZIP_EXPORTS, _lib.BGZF_EXPORTS, _lib.BGZF_RANGE_EXPORTS, _lib.BGZF_STORED_EXPORTS,
             _lib.GUNZIP_EXPORTS, _lib.ZIP_EXPORTS, _lib.ZIP_WRITE_EXPORTS, _lib.ZIP64_EXPORTS)
    assert [len(t) for t in older] == [22, 4, 2, 7, 8, 2, 3, 2, 4, 3, 7]
    assert len(_lib.GZIP_MEMBERS_EXPORTS) == 4 and not set(_lib.GZIP_MEMBERS_EXPORTS) & set().union(*older)
    assert _lib.load().hdlz_version() == 0x000600
    scope = header("hdlz_gunzip.h")
    assert "hdlz_gzip_members.h" in scope and "hdlz_zip.h" in scope          # the "out of scope" sentence points to both


def test_the_queries_are_their_closed_forms():
    import hdl_deflate_amd
    from hdl_deflate_amd import _lib
    L = _lib.load()
    assert L.hdlz_gzip_members_index_work_bytes(0) == 0
    for n in (1, 3, 4, 32767, 32768, 32769, 1 << 20, (1 << 28) + 5, 1 << 33, (1 << 40) + 1):
        W = (n + 32767) // 32768
        assert L.hdlz_gzip_members_index_work_bytes(n) == r256(64 + 308 * W) == hdl_deflate_amd.gzip_members_index_work_bytes(n), n
    assert L.hdlz_gzip_members_inflate_work_bytes(0) == 0 and L.hdlz_gzip_members_inflate_work_bytes(1 << 31) == 0
    for m in (1, 2, 10, 11, 12, 13, 64, 300, 4096, 50000, (1 << 31) - 1):
        assert L.hdlz_gzip_members_inflate_work_bytes(m) == r256(20 * m) + r256(24 * m + 8) == hdl_deflate_amd.gzip_members_inflate_work_bytes(m), m


def _pairs(call, faults, L, independent=lambda i, j: True):
    for kw, word in faults:
        assert call(**kw) == E_BAD_PARAM and word in L.hdlz_last_error(), (kw, L.hdlz_last_error())
    for i, (kw_i, word_i) in enumerate(faults):                      # ... and every pair: the earlier one answers
        for kw_j, _ in faults[i + 1:]:
            if set(kw_i) & set(kw_j) or not independent(kw_i, kw_j):
                continue
            assert call(**dict(kw_j, **kw_i)) == E_BAD_PARAM and word_i in L.hdlz_last_error(), (kw_i, kw_j, L.hdlz_last_error())


def test_the_index_refuses_in_its_order_before_the_device():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    keep, base = _host_buffer(1 << 16)
    wb = L.hdlz_gzip_members_index_work_bytes(40000)
    assert wb == r256(64 + 616)
    good = dict(f=base, n=40000, cap=8, off=base + 40960, out_off=base + 41216, res=base + 41472, work=base + 41728, work_bytes=wb)

    def call(**kw):
        a = dict(good, **kw)
        return L.hdlz_gzip_members_index_ws(a["f"], a["n"], a["cap"], a["off"], a["out_off"], a["res"], a["work"], a["work_bytes"], None)

    faults = [(dict(off=None), b"null device pointer"), (dict(cap=1 << 40), b"member_cap too large"), (dict(work_bytes=wb - 1), b"hdlz_gzip_members_index_work_bytes"),
              (dict(out_off=good["out_off"] + 4), b"8-byte")]
    _pairs(call, faults, L)
    for k in ("out_off", "res", "f"):
        assert call(**{k: None}) == E_BAD_PARAM and b"null device pointer" in L.hdlz_last_error(), k
    for k in ("off", "res", "work"):
        assert call(**{k: good[k] + 4}) == E_BAD_PARAM and b"8-byte" in L.hdlz_last_error(), k
    assert call(work=None) == E_BAD_PARAM and b"hdlz_gzip_members_index_work_bytes" in L.hdlz_last_error()
    if _no_device():
        assert call() == E_HIP
        assert call(f=base + 1) == E_HIP                                       # any alignment of the file
        assert call(f=None, n=0, work=None, work_bytes=0) == E_HIP             # an empty file needs no scratch
        assert call(cap=0) == E_HIP


def test_the_read_refuses_in_its_order_before_the_device():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    keep, base = _host_buffer(1 << 16)
    wb = L.hdlz_gzip_members_inflate_work_bytes(3)
    assert wb == 512
    good = dict(f=base, n=4096, off=base + 4096, out_off=base + 4352, m=3, out=base + 8192, cap=4096, st=base + 4608, res=base + 4864,
                work=base + 16384, work_bytes=wb)

    def call(**kw):
        a = dict(good, **kw)
        return L.hdlz_gzip_members_inflate_ws(a["f"], a["n"], a["off"], a["out_off"], a["m"], a["out"], a["cap"], a["st"], a["res"], a["work"],
                                              a["work_bytes"], None)

    faults = [(dict(res=None), b"null device pointer"), (dict(m=1 << 31), b"nmembers too large"), (dict(off=good["off"] + 4), b"d_off / d_out_off / d_result"),
              (dict(st=good["st"] + 2), b"d_member_status"), (dict(work=good["work"] + 128), b"256-byte"),
              (dict(work_bytes=wb - 1), b"hdlz_gzip_members_inflate_work_bytes")]
    _pairs(call, faults, L, independent=lambda i, j: not ("m" in i and "work_bytes" in j))      # (2^31 members have no size to fall short of)
    for k in ("f", "off", "out_off", "out"):
        assert call(**{k: None}) == E_BAD_PARAM and b"null device pointer" in L.hdlz_last_error(), k
    assert call(out_off=good["out_off"] + 4) == E_BAD_PARAM and b"8-byte" in L.hdlz_last_error()
    assert call(work=None) == E_BAD_PARAM and b"hdlz_gzip_members_inflate_work_bytes" in L.hdlz_last_error()
    if _no_device():
        assert call() == E_HIP
        assert call(st=None) == E_HIP                                          # nullable
        assert call(f=base + 3, out=base + 8193) == E_HIP                      # any alignment of the file and of the output
        assert call(m=0, f=None, off=None, out_off=None, out=None, cap=0, work=None, work_bytes=0) == E_HIP


def test_the_index_rule_on_small_files():
    assert R.index_rule(b"") == ([0], [0])
    assert R.index_rule(b"\x1f") == ([0, 1], [0, 0]) and R.index_rule(b"abc") == ([0, 3], [0, 0])
    assert R.index_rule(R.MAGIC) == ([0, 4], [0, 0]) and R.index_rule(b"ab" + R.MAGIC) == ([0, 2, 6], [0, 0, 0])
    assert R.index_rule(R.MAGIC + R.MAGIC) == ([0, 4, 8], [0, 0, 0])
    assert R.candidates(b"x" * 10 + b"\x1f\x8b\x08") == [0] and R.candidates(b"x" * 10 + b"\x1f\x8b\x08\x1f") == [0, 10]
    assert R.candidates(b"x" * 10 + b"\x1f\x8b\x08\x20") == [0]               # a reserved flag bit
    z = bytes(14) + (77).to_bytes(4, "little")
    assert R.index_rule(z) == ([0, 18], [0, 77]) and R.index_rule(z[1:]) == ([0, 17], [0, 0])
    z = bytes(14) + b"\xff\xff\xff\xff"
    assert R.index_rule(z) == ([0, 18], [0, 1032 * 18 + 258])                  # the guess is held to deflate's largest expansion
    m = R.stored(b"abc")
    assert len(m) == 26 and gzip.decompress(m) == b"abc" and len(R.stored(bytes(65536))) == 23 + 65536 + 5
    assert len(R.stored_of_length(100000, 1)) == 100000 and gzip.decompress(R.stored_of_length(23, 1)) == b""
    f = R.place([0, 100, 4097, 70000], 140000)
    assert R.candidates(f) == [0, 100, 4097, 70000] and len(f) == 140000 and len(gzip.decompress(f)) == 140000 - 4 * 23 - 2 * 5


def test_the_clean_files_need_no_repair_and_the_crafted_ones_their_count(oracle):
    """the index rule, the member verdicts and the repair loop on the CPU: gzip.decompress's bytes and acceptance on every file, and
    the number of repairs the GPU tests hold the device route to"""
    for label, z, repairs in R.file_cases():
        want = R.gzip_accepts(z)
        got = R.read_with_rules(oracle, z)
        assert got[0] == want, label
        assert got[1] == repairs and got[2] == 0, (label, got[1:])
        assert R.read_rule(z)[0] == want, (label, "the serial reader alone")
        # big_member forced low: spans of 2000 bytes and more take the one-stream route, the bytes do not change
        assert R.read_with_rules(oracle, z, big=2000)[0] == want, label
    ms, datas = R.many_members()
    assert len(ms) == 300 and b"" in datas and gzip.compress(b"", mtime=1) in ms
    v = R.verdicts(oracle, b"".join(ms))
    assert [st for st, _ in v] == [R.OK] * 300 and [d for _, d in v] == datas


def test_the_verdict_on_damaged_members_is_gunzip_refs(oracle):
    """a member alone in its span: the verdict is the member rule's, a slot that is too long or too short is told apart"""
    d = G.text(900, 51)
    z = G.gz(d, name=b"v")
    assert R.verdict(oracle, z, 0, len(z), 900) == (R.OK, d)
    assert R.verdict(oracle, z, 0, len(z), 901)[0] == R.E_BAD_CHECKSUM         # shorter than its slot
    assert R.verdict(oracle, z, 0, len(z), 899)[0] == R.E_OUT_CAPACITY         # longer than its slot: the decoder's status
    assert R.verdict(oracle, z + b"\0", 0, len(z) + 1, 900)[0] == R.E_NO_EOF   # stops in front of the span's end
    assert R.verdict(oracle, z, 0, len(z) - 1, 900)[0] == R.E_NO_EOF           # cut
    assert R.verdict(oracle, z, 0, len(z) + 1, 900)[0] == R.E_BAD_PARAM and R.verdict(oracle, z, 5, 4, 0)[0] == R.E_BAD_PARAM
    assert R.verdict(oracle, z, 0, len(z), 900, out_room=899)[0] == R.E_BAD_PARAM
    for label, case in G.trailer_cases() + G.header_cases():
        if label in ("a second member behind", "garbage behind"):
            continue
        n_slot = int.from_bytes(case[-4:], "little") if len(case) >= 18 else 0
        if n_slot > 70000:
            continue
        got = R.verdict(oracle, case, 0, len(case), n_slot)[0]
        want = G.member(oracle, case, n_slot)["status"]
        if want == R.OK:
            assert got == R.OK and G.zaccepts(case) is not None, label
        else:
            assert got != R.OK and G.zaccepts(case) is None, label
            assert got == want, (label, want, got)
