"""CPU: the extension header include/hdlz_bgzf_stored.h -- every declaration exported and bound with its arity, the struct mirror, both
queries equal to their closed forms, parameter errors in front of the device, no CPU path behind good parameters; and bgzf_stored_ref,
the reference of the GPU tests (the member rule on the CPU oracle's rows), held against gzip.decompress and bgzf_ref's walk and against
the arithmetic of the rule on crafted blocks before any kernel is trusted to it."""
import ctypes
import gzip

import numpy as np

import bgzf_ref
from cabi_common import check_struct_mirror, declarations as _declarations, header, host_buffer as _host_buffer, no_device as _no_device
import bgzf_stored_ref as ref
from bgzf_ref import OK, E_OUT_CAPACITY, E_BAD_PARAM
from bgzf_stored_ref import FIXED, STORED, E_SHORT_INPUT

E_HIP = 9
E_BAD_DISTANCE = 4


def _header():
    return header("hdlz_bgzf_stored.h")


def test_every_declaration_is_exported_and_bound():
    from hdl_deflate_amd import _lib
    params = _declarations(_header())
    assert params == {"hdlz_bgzf_stored_bound": 2, "hdlz_bgzf_join_stored_work_bytes": 1, "hdlz_bgzf_join_stored_ws": 18}
    assert sorted(params) == sorted(_lib.BGZF_STORED_EXPORTS) == sorted(_lib.BGZF_STORED_SIGNATURES)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    L = _lib.load()
    for name, n in params.items():
        assert hasattr(raw, name), name
        restype, argtypes = _lib.BGZF_STORED_SIGNATURES[name]
        assert len(argtypes) == n, name
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert '#include "hdlz_bgzf.h"' in _header()


def test_the_tables_in_front_of_it_are_as_they_were():
    from hdl_deflate_amd import _lib
    older = (_lib.EXPORTS, _lib.JOIN_EXPORTS, _lib.UNJOIN_EXPORTS, _lib.GZIP_EXPORTS, _lib.BGZF_EXPORTS, _lib.BGZF_RANGE_EXPORTS)
    assert [len(t) for t in older] == [22, 4, 2, 7, 8, 2]
    assert len(_lib.BGZF_STORED_EXPORTS) == 3 and not set(_lib.BGZF_STORED_EXPORTS) & set().union(*older)
    assert _lib.load().hdlz_version() == 0x000600
    # the header it extends still declares its eight functions and nothing of this one
    base = _declarations(header("hdlz_bgzf.h"))
    assert len(base) == 8 and not set(base) & set(_lib.BGZF_STORED_EXPORTS)


def test_struct_mirror_matches_the_header():
    from hdl_deflate_amd import _lib
    R = _lib.BgzfStoredResult
    fields = [("uint64_t", "file_len"), ("uint64_t", "nstored"), ("uint32_t", "status"), ("uint32_t", "first_bad")]
    check_struct_mirror(_header(), "hdlz_bgzf_stored_result", R, fields)
    assert [getattr(R, f[1]).offset for f in fields] == [0, 8, 16, 20] and ctypes.sizeof(R) == 24


def test_the_queries_are_their_closed_forms():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    for nb in (0, 1, 257, 1 << 20):
        assert L.hdlz_bgzf_join_stored_work_bytes(nb) == L.hdlz_join_work_bytes(nb), nb
        for in_len in (0, 5, 30, 31, 2048, 58230, 65280, 65505, 65536):
            assert L.hdlz_bgzf_stored_bound(nb, in_len) == 28 + nb * min(L.hdlz_out_bound(in_len) + 20, in_len + 31), (nb, in_len)
    for x in (0, 5, 65536):
        assert L.hdlz_bgzf_stored_bound(0, x) == 28 == len(bgzf_ref.EOF)
    # the bound never exceeds the older writer's
    assert L.hdlz_bgzf_stored_bound(1, 65280) == 28 + 65311 < L.hdlz_bgzf_bound(1, 65280)
    assert all(L.hdlz_bgzf_stored_bound(3, n) <= L.hdlz_bgzf_bound(3, n) for n in range(0, 300))


def test_join_stored_parameter_errors_come_before_the_device():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    keep, base = _host_buffer()
    wb = L.hdlz_bgzf_join_stored_work_bytes(1)
    assert 0 < wb <= 4096

    def join(data=base, in_off=None, rows=base, length=base, status=base, crc=base, file=base, off=base, kind=None, result=base, work=base,
             work_bytes=wb, nblocks=1):
        return L.hdlz_bgzf_join_stored_ws(data, in_off, 64, 64, rows, 64, length, status, nblocks, crc, file, 4096, off, kind, result, work,
                                          work_bytes, None)
    for k in ("data", "rows", "length", "status", "crc", "file", "off", "result", "work"):
        assert join(**{k: None}) == E_BAD_PARAM, k
    assert join(nblocks=1 << 31) == E_BAD_PARAM and b"2^31" in L.hdlz_last_error()
    assert join(work_bytes=wb - 1) == E_BAD_PARAM and b"hdlz_bgzf_join_stored_work_bytes" in L.hdlz_last_error()
    for k in ("off", "result", "work", "in_off"):
        assert join(**{k: base + 4}) == E_BAD_PARAM and b"8-byte" in L.hdlz_last_error(), k
    assert join(crc=base + 2) == E_BAD_PARAM and b"4-byte" in L.hdlz_last_error()
    if _no_device():
        assert join() == E_HIP and join(in_off=base) == E_HIP and join(kind=base + 1) == E_HIP and join(data=base + 3) == E_HIP
        assert join(nblocks=0, data=None, rows=None, length=None, status=None, crc=None, work=None, work_bytes=0) == E_HIP


# ---- bgzf_stored_ref against stock readers and against the arithmetic of the rule
def test_the_reference_files_are_read_by_stock_readers(oracle):
    blocks = [b"", b"a", b"abcd"] + [c[1] for c in ref.CRAFTED] + [bgzf_ref.data(n, n) for n in (5, 31, 700, 2048)] + \
        [bytes(np.random.default_rng(2).integers(0, 256, 2048, dtype=np.uint8))]
    rows, statuses = ref.oracle_rows(oracle, blocks)
    f, offs, kinds = ref.file(rows, blocks, statuses)
    assert gzip.decompress(f) == b"".join(blocks) and f.endswith(bgzf_ref.EOF)
    w = bgzf_ref.walk(f)
    assert w.off[:-1] == offs and w.record() == (len(blocks) + 1, sum(map(len, blocks)), len(f), OK, 1)
    assert kinds[:3] == [STORED] * 3 and kinds[-1] == STORED and FIXED in kinds
    assert ref.record(rows, blocks, statuses) == (len(f), sum(kinds), OK, ref.NONE_BAD)
    for b, (blk, kind) in enumerate(zip(blocks, kinds)):
        size = offs[b + 1] - offs[b]
        assert size <= len(blk) + 31 and size == (len(blk) + 31 if kind == STORED else len(rows[b]) + 20)
        if kind == STORED:                                               # the payload verbatim behind 23 bytes
            assert f[offs[b] + 18] == 1 and f[offs[b] + 23:offs[b] + 23 + len(blk)] == blk
    assert ref.file([], []) == (bgzf_ref.EOF, [0], [])


def test_all_fixed_files_are_the_older_writers(oracle):
    blocks = [bgzf_ref.data(2 * n, n)[:n] for n in (40, 64, 700, 2048)]      # (text: every block compresses)
    rows, statuses = ref.oracle_rows(oracle, blocks)
    f, offs, kinds = ref.file(rows, blocks, statuses)
    assert kinds == [FIXED] * 4 and (f, offs) == bgzf_ref.framed_rows(rows, blocks)


def test_the_arithmetic_of_the_rule(oracle):
    """100 distinct bytes, c of them >= 144: every token is a literal, the row is 6 + ceil((810 + c) / 8) bytes, its member 20 more,
    against the stored member's 131"""
    for label, blk, L, kind in ref.CRAFTED:
        (row,), (st,) = ref.oracle_rows(oracle, [blk])
        assert st == OK and len(row) == L, (label, len(row))            # the row lengths, before they are used
        high = sum(1 for x in blk if x >= 144)
        if label != "5 random":
            assert len(set(blk)) == len(blk) and L == ref.literal_row_len(len(blk), high), label
        got = ref.choose(row, blk, OK)
        assert got[:2] == (OK, kind), label
        assert len(got[2]) == (len(blk) + 31 if kind == STORED else L + 20), label
        assert (L + 20 <= len(blk) + 31) == (kind == FIXED), label
        assert gzip.decompress(got[2]) == blk
    assert [(c[2] + 20, len(c[1]) + 31) for c in ref.CRAFTED] == [(130, 131), (131, 131), (131, 131), (132, 131), (132, 131), (73, 71), (33, 36)]


def test_the_failures_of_the_rule(oracle):
    r = np.random.default_rng(1)
    blk = bgzf_ref.data(600, 3)[:300]                                   # (text: the fixed form is the shorter one)
    (row,), _ = ref.oracle_rows(oracle, [blk])
    assert ref.choose(row, blk, E_BAD_DISTANCE)[:2] == (E_BAD_DISTANCE, FIXED)          # 1.
    assert ref.choose(row[:7], blk, OK)[0] == E_BAD_PARAM and ref.choose(row, blk, OK, row_pitch=len(row) - 1)[0] == E_BAD_PARAM      # 2.
    big = bytes(r.integers(0, 256, 65506, dtype=np.uint8))
    assert ref.choose(b"x" * 100, big, OK)[0] == E_OUT_CAPACITY and ref.choose(b"", big, E_SHORT_INPUT)[0] == E_OUT_CAPACITY      # 3.
    assert ref.choose(b"x" * 65517, big[:65505], OK)[:2] == (OK, STORED)                 # 4.: L + 20 > 65536 is not usable
    assert ref.choose(row, blk, E_SHORT_INPUT)[:2] == (OK, STORED)                       # 5.: SHORT_INPUT is always stored
    assert ref.choose(b"", b"", E_SHORT_INPUT) == (OK, STORED, bgzf_ref.frame(b"\x01\x00\x00\xff\xff", 0, 0))
    # the record: the worst status first, the lowest failed block, a failed block of length 0
    rows, blocks, sts = [row, row, b"", row], [blk, blk, big, blk], [OK, E_BAD_DISTANCE, E_SHORT_INPUT, OK]
    assert ref.record(rows, blocks, sts) == (0, 0, E_BAD_DISTANCE, 1)
    f, offs, kinds = ref.file(rows, blocks, sts)
    assert offs[1] == offs[2] == offs[3] and kinds == [FIXED] * 4
    assert ref.record([row], [blk], cap=10) == (len(row) + 20 + 28, 0, E_OUT_CAPACITY, ref.NONE_BAD)
