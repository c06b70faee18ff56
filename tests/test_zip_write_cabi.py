"""CPU: the extension header include/hdlz_zip_write.h -- every declaration exported and bound with its arity, the tables in front of it
and the version as they were, both queries equal to their closed forms, every parameter refusal in the header's order and in front of
the device, no CPU path behind good parameters, the ctypes mirror of the result record; and THE FILE RULE as tests/zip_write_ref.py
states it held against zipfile, numpy.load and the index rule of tests/zip_ref.py on every case the GPU tests use."""
import io
import zipfile

import numpy as np
import pytest

import zip_ref as Z
import zip_write_ref as W
from cabi_common import check_struct_mirror, declarations, header, host_buffer as _host_buffer, no_device as _no_device

E_BAD_PARAM, E_HIP = 8, 9


def test_every_declaration_is_exported_and_bound():
    import ctypes
    from hdl_deflate_amd import _lib
    text = header("hdlz_zip_write.h")
    params = declarations(text)
    assert params == {"hdlz_zip_write_bound": 5, "hdlz_zip_write_work_bytes": 2, "hdlz_zip_write_ws": 25}
    assert sorted(params) == sorted(_lib.ZIP_WRITE_EXPORTS) == sorted(_lib.ZIP_WRITE_SIGNATURES)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    L = _lib.load()
    for name, n in params.items():
        assert hasattr(raw, name), name
        restype, argtypes = _lib.ZIP_WRITE_SIGNATURES[name]
        assert len(argtypes) == n, name
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert '#include "hdlz_zip.h"' in text and "0x0800u" in text and _lib.ZIP_FLAG_UTF8 == W.FLAG_UTF8 == 0x800
    import hdl_deflate_amd
    assert callable(hdl_deflate_amd.save_npz) and callable(hdl_deflate_amd.load_npz)
    from hdl_deflate_amd.engine import Engine
    assert callable(Engine.compress_zip) and callable(Engine.write_zip_bytes)


def test_the_tables_in_front_of_it_are_as_they_were():
    from hdl_deflate_amd import _lib
    older = (_lib.EXPORTS, _lib.JOIN_EXPORTS, _lib.UNJOIN_EXPORTS, _lib.GZIP_EXPORTS, _lib.BGZF_EXPORTS, _lib.BGZF_RANGE_EXPORTS, _lib.BGZF_STORED_EXPORTS,
             _lib.GUNZIP_EXPORTS, _lib.ZIP_EXPORTS)
    assert [len(t) for t in older] == [22, 4, 2, 7, 8, 2, 3, 2, 4]
    assert len(_lib.ZIP_WRITE_EXPORTS) == 3 and not set(_lib.ZIP_WRITE_EXPORTS) & set().union(*older)
    assert _lib.load().hdlz_version() == 0x000600
    assert declarations(header("hdlz_zip.h")) == {"hdlz_zip_index_work_bytes": 2, "hdlz_zip_index_ws": 9, "hdlz_zip_inflate_work_bytes": 3, "hdlz_zip_inflate_ws": 13}
    assert "hdlz_zip_write.h" in header("hdlz_zip.h")         # the "out of scope" sentence points here


def test_the_struct_mirror_matches_the_header():
    from hdl_deflate_amd import _lib
    import ctypes
    check_struct_mirror(header("hdlz_zip_write.h"), "hdlz_zip_write_result", _lib.ZipWriteResult,
                        [("uint64_t", "file_len"), ("uint64_t", "cd_off"), ("uint64_t", "cd_size"), ("uint64_t", "nstored"), ("uint32_t", "status"),
                         ("uint32_t", "first_bad")])
    assert ctypes.sizeof(_lib.ZipWriteResult) == 40


def test_the_queries_are_their_closed_forms():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    for E in (0, 1, 31, 32, 4096, 65535):
        for B in (0, 1, 255, 256, 257, 16384, 1 << 20, (1 << 31) - 1):
            assert L.hdlz_zip_write_work_bytes(E, B) == W.work_bytes(E, B), (E, B)
            for block_len in (32, 1 << 16):
                for total, names in ((0, 0), (5, 1), (1 << 30, 65535 * 300)):
                    assert L.hdlz_zip_write_bound(E, B, block_len, total, names) == W.bound(E, total, names) == 22 + 76 * E + 2 * names + total
    assert L.hdlz_zip_write_work_bytes(65536, 0) == 0 and L.hdlz_zip_write_work_bytes(1, 1 << 31) == 0
    assert L.hdlz_zip_write_work_bytes(0, 0) == 256 + 2 * 256 + 256 + 6 * 256
    assert L.hdlz_zip_write_bound(0, 0, 0, 0, 0) == 22


def _pairs(L, call, faults):
    for kw, word in faults:
        assert call(**kw) == E_BAD_PARAM and word in L.hdlz_last_error(), (kw, L.hdlz_last_error())
    for i, (kw_i, word_i) in enumerate(faults):              # ... and every pair: the earlier one answers
        for kw_j, _ in faults[i + 1:]:
            if set(kw_i) & set(kw_j):
                continue
            assert call(**dict(kw_j, **kw_i)) == E_BAD_PARAM and word_i in L.hdlz_last_error(), (kw_i, kw_j, L.hdlz_last_error())


def test_parameter_errors_come_before_the_device_in_their_order():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    keep, base = _host_buffer(1 << 17)
    wb = L.hdlz_zip_write_work_bytes(3, 7)
    at = lambda k: base + 4096 * k
    good = dict(d_in=at(0), ent_off=at(1), names=at(2), name_off=at(3), E=3, in_off=at(4), rows=at(5), pitch=64, len=at(6), end_bits=at(7), status=at(8),
                B=7, blk_first=at(9), crc=at(10), flags=0, dt=0x210000, align=1, total=100, file=at(11), cap=4096, entries=at(12), result=at(13),
                work=at(14), work_bytes=wb)
    assert wb <= 4096 * 10

    def call(**kw):
        a = dict(good, **kw)
        return L.hdlz_zip_write_ws(a["d_in"], a["ent_off"], a["names"], a["name_off"], a["E"], a["in_off"], a["rows"], a["pitch"], a["len"], a["end_bits"],
                                   a["status"], a["B"], a["blk_first"], a["crc"], a["flags"], a["dt"], a["align"], a["total"], a["file"], a["cap"],
                                   a["entries"], a["result"], a["work"], a["work_bytes"], None)

    faults = [(dict(result=None), b"d_result is required"), (dict(E=65536), b"nentries too large"), (dict(B=1 << 31), b"nblocks too large"),
              (dict(ent_off=None), b"(the entries)"), (dict(len=None), b"(the rows)"), (dict(file=None), b"d_file is null"),
              (dict(flags=0x808), b"HDLZ_ZIP_FLAG_UTF8"), (dict(align=3), b"out_align"), (dict(work_bytes=wb - 1), b"hdlz_zip_write_work_bytes"),
              (dict(name_off=at(3) + 4), b"8-byte"), (dict(crc=at(10) + 2), b"4-byte")]
    # (E = 65536 and B = 2^31 change what the scratch query answers; they are paired with the faults in front of that check only)
    _pairs(L, call, faults[:8])
    _pairs(L, call, faults[3:])
    for k in ("d_in", "names", "name_off", "blk_first", "crc"):
        assert call(**{k: None}) == E_BAD_PARAM and b"(the entries)" in L.hdlz_last_error(), k
    for k in ("in_off", "rows", "end_bits", "status"):
        assert call(**{k: None}) == E_BAD_PARAM and b"(the rows)" in L.hdlz_last_error(), k
    assert call(E=0) == E_BAD_PARAM and b"rows without entries" in L.hdlz_last_error()
    for flags in (1, 8, 0x801, 1 << 31):
        assert call(flags=flags) == E_BAD_PARAM and b"HDLZ_ZIP_FLAG_UTF8" in L.hdlz_last_error()
    for align in (0, 6, 512, 1 << 31):
        assert call(align=align) == E_BAD_PARAM and b"out_align" in L.hdlz_last_error()
    assert call(work=None) == E_BAD_PARAM and b"hdlz_zip_write_work_bytes" in L.hdlz_last_error()
    for k in ("ent_off", "in_off", "end_bits", "blk_first", "entries", "result", "work"):
        assert call(**{k: good[k] + 4}) == E_BAD_PARAM and b"8-byte" in L.hdlz_last_error(), k
    for k in ("len", "status"):
        assert call(**{k: good[k] + 2}) == E_BAD_PARAM and b"4-byte" in L.hdlz_last_error(), k
    if _no_device():                                         # no CPU path behind good parameters
        assert call() == E_HIP
        assert call(flags=0x800) == E_HIP and call(entries=None) == E_HIP
        assert call(file=None, cap=0) == E_HIP               # the sizing call
        assert call(d_in=at(0) + 1, names=at(2) + 3, rows=at(5) + 1, file=at(11) + 5) == E_HIP       # bytes at any alignment
        assert call(B=0, in_off=None, rows=None, len=None, end_bits=None, status=None) == E_HIP
        w0 = L.hdlz_zip_write_work_bytes(0, 0)
        assert call(E=0, B=0, d_in=None, ent_off=None, names=None, name_off=None, blk_first=None, crc=None, in_off=None, rows=None, len=None,
                    end_bits=None, status=None, entries=None, work_bytes=w0) == E_HIP


# ---- the rule against zipfile and the index rule
LABELS = [c["label"] for c in W.all_cases()]


@pytest.mark.parametrize("label", LABELS + list(W.SHAPE_LABELS))
def test_the_reference_file_reads_as_the_rule_says(label):
    case = {c["label"]: c for c in W.all_cases()}.get(label) or W.shape_case(label)
    w = W.written(label)
    z, items = w.file, case["items"]
    zf = zipfile.ZipFile(io.BytesIO(z))
    infos = zf.infolist()
    assert zf.testzip() is None and len(infos) == len(items)
    step = max(1, len(items) // 50)
    for k in range(0, len(items), step):
        (name, data), info, en = items[k], infos[k], w.entries[k]
        assert info.filename == name and info.date_time == W.DATE_TIME and info.extra == b"" and info.comment == b"" and info.external_attr == 0
        assert (info.compress_type, info.file_size, info.compress_size, info.CRC, info.flag_bits) == (w.methods[k], len(data), en["csize"], en["crc"], en["flags"])
        assert zf.read(info) == bytes(data)
        stored = bool(case["store"] and case["store"][k]) or len(data) < 5
        assert w.methods[k] == (0 if stored or w.diffs[k] >= 0 else 8) and (w.diffs[k] is None) == stored
        assert en["flags"] == (W.FLAG_UTF8 if label == "a name that is not ASCII" else 0)
    from hdl_deflate_amd import _lib
    nblocks = sum(len(W.plan(len(d), case["block"], bool(case["store"] and case["store"][k]))) for k, (_, d) in enumerate(items))
    room = _lib.load().hdlz_zip_write_bound(len(items), nblocks, case["block"], sum(len(d) for _, d in items), sum(en["name_len"] for en in w.entries))
    assert len(z) <= room == W.bound(len(items), sum(len(d) for _, d in items), sum(en["name_len"] for en in w.entries))
    for align in (1, 64):
        ix = Z.index(z, align)
        wa = W.written(label, align)
        assert wa.file == z
        assert (ix["status"], ix["nentries"], ix["cd_off"], ix["cd_size"]) == (Z.OK, len(items), w.record["cd_off"], w.record["cd_size"])
        assert Z.records(ix) == Z.records(dict(entries=wa.entries)), label
        assert all(en["status"] == Z.OK for en in ix["entries"])
    ix, sts, flat = Z.read(z)
    assert sts == [Z.OK] * len(items) and flat == b"".join(bytes(d) for _, d in items)


def test_the_cases_cover_what_they_are_meant_to():
    from hdl_deflate_amd import _lib
    from hdl_deflate_amd.engine import Engine
    assert _lib.ZIP_FLAG_UTF8 == W.FLAG_UTF8 and Engine.ZIP_CRC_TILED_MIN == W.CRC_TILED_MIN
    by = {c["label"]: c for c in W.all_cases()}
    large = by["entries around ZIP_CRC_TILED_MIN"]
    assert [len(d) >= W.CRC_TILED_MIN for _, d in large["items"]] == [False, False, True, False, False, True, True, False]
    assert W.written(large["label"]).methods == [8, 0, 8, 0, 8, 0, 8, 8]
    # both marker lengths, every number of pad bits
    assert set(W.written("pad bits 0 .. 7").pads) == set(range(8))
    # the ties: only -1 is deflated
    ties = W.tie_entries()
    assert sorted(ties) == [-1, 0, 1]
    w = W.written("ties: c - u of -1, 0 and +1")
    assert w.diffs == [-1, 0, 1] and w.methods == [8, 0, 0] and w.record["nstored"] == 2
    # the sizes: 33 bytes is where plan_blocks shortens the block in front of a short tail, 48 two exact blocks
    assert [len(W.plan(n, 32)) for n in (0, 1, 4, 5, 31, 32, 33, 47, 48, 49)] == [0, 0, 0, 1, 1, 1, 2, 2, 2, 2]
    assert W.plan(33, 32) == [(0, 16), (16, 17)] and W.plan(48, 32) == [(0, 32), (32, 16)]
    firsts = np.cumsum([0] + [len(W.plan(len(d), 32)) for _, d in by["1 .. 600 blocks at block 32"]["items"]])
    assert list(firsts) == [0, 1, 256, 512, 515, 772, 1372]
    # incompressible entries with blocks are stored from the input; forced and mixed forms
    w = W.written("incompressible entries with blocks")
    assert w.methods == [0] * 6 and all(d is not None and d >= 0 for d in w.diffs)
    assert W.written("store= entries").methods == [8, 0, 0, 8, 0, 8]
    m = W.written("the forms alternating").methods
    assert 0 in m and 8 in m and any(a != b for a, b in zip(m, m[1:]))
    # payloads start at every residue mod 16
    w = W.written("names of 1 to 16 bytes")
    assert [en["payload_off"] % 16 for en in w.entries] == 2 * list(range(16)) and w.methods == [8] * 16 + [0] * 16
    assert all(1 <= en["name_len"] <= 16 for en in w.entries) and len({en["name_len"] for en in w.entries}) > 8
    assert [en["name_len"] for en in W.written("names of 300 and 65535 bytes").entries] == [5, 300, 65535, 4]
    assert len(W.written("no entry").file) == 22 and W.written("65535 empty entries").record["nstored"] == 65535


# ---- the shape cases: each one proved, from its arrays alone, to reach the branch of hdlz_zip_write.hip it is for.  The model of the
# lookup (zip_write_ref.gather_lookup) judges the CASES; what the device must write is zip_write_ref.expected alone.
def _lookup(label):
    case = W.shape_case(label)
    first, B = W.batch_arrays(case)
    F = np.asarray(first, np.int64)
    g = W.gather_lookup(F, B)
    assert np.array_equal(g.entry, np.searchsorted(F, np.arange(B), side="right") - 1), label      # the lookup as modelled finds every row's entry
    return case, F, B, g


def test_the_model_of_the_wave_search_is_an_upper_bound():
    import bisect
    for n in list(range(1, 300)) + list(range(4095, 4162)) + [5000, 65535, 65536]:
        v = np.sort(np.random.default_rng(n).integers(0, 3 * n, n)).astype(np.int64)
        seen = set()
        for x in (-1, 0, int(v[0]), int(v[n // 3]) - 1, int(v[n // 2]), int(v[-1]) - 1, int(v[-1]), int(v[-1]) + 1):
            got, rounds = W.wave_upper_bound(v, x)
            assert got == bisect.bisect_right(v.tolist(), x), (n, x)
            seen.add(rounds)
        assert seen <= ({1} if n <= 64 else {2} if n <= 4096 and n % 64 == 0 else {2, 3}) and max(seen) == (1 if n <= 64 else 2 if n <= 4096 else 3), (n, seen)


def test_the_shape_cases_reach_the_branches_they_are_for():
    k = W.kernel_constants()
    assert k.ROWS_MAX == 4 * 64 and k.ROWS_FEW == 4 * 4 and k.JT == 256 and k.PLAN_THREADS == 16 * 64
    assert len(W.SHAPE_LABELS) == len(set(W.SHAPE_LABELS)) == 14 and not set(W.SHAPE_LABELS) & {c["label"] for c in W.all_cases()}
    soft, noise = W.alphabet()
    assert len(soft) == 32 and len(noise) == 16 and {len(b) for b in soft + noise} == {32}

    # -- search widths: E + 1 words in one round, in two, and in three where the second round is itself wider than 64
    rounds = {}
    for E in W.MANY:
        case, F, B, g = _lookup("%d entries of 1 to 3 rows" % E)
        w = W.written(case["label"])
        assert len(case["items"]) == E and g.per == 4 and not g.fallback.any()
        rows = np.diff(F)
        assert set(rows.tolist()) == {0, 1, 2, 3} and 0 < np.count_nonzero(rows == 0) < E // 8
        assert 0 in w.methods and 8 in w.methods and any(m == 0 and n for m, n in zip(w.methods, rows))      # stored without and with rows
        rounds[E] = set(g.rounds.tolist())
    assert rounds[63] == {1} and rounds[64] == {2} and rounds[4095] == {2} and rounds[1023] == rounds[1024] == rounds[1025] == rounds[2049] == {2}
    assert rounds[4096] == {2, 3} and rounds[4097] == {2, 3}      # (two rounds: the waves whose first row lies in the partial last chunk)

    # -- the ragged plan: per entries a thread, the threads that take all of them, the entries of the one thread that takes fewer
    claimed = {63: (1, 63, 0), 64: (1, 64, 0), 1023: (1, 1023, 0), 1024: (1, 1024, 0), 1025: (2, 512, 1), 2049: (3, 683, 0), 4095: (4, 1023, 3),
               4096: (4, 1024, 0), 4097: (5, 819, 2), 65535: (64, 1023, 63)}
    for E, claim in claimed.items():
        assert W.plan_share(E) == claim, E
    for E in (1023, 1024, 1025, 2049, 4095, 4096, 4097):
        w = W.written("%d entries of 1 to 3 rows" % E)
        per = claimed[E][0]
        size = np.array([30 + en["name_len"] + en["csize"] for en in w.entries] + [0] * (k.PLAN_THREADS * per - E), np.int64)
        threads = size.reshape(k.PLAN_THREADS, per).sum(axis=1)
        waves = threads.reshape(16, 64).sum(axis=1)
        busy = -(-E // per)                                      # the threads that take an entry; neighbours leave different partial sums
        assert np.count_nonzero(np.diff(threads[:busy])) > 0.8 * busy and busy > 64 and np.diff(waves[:-(-busy // 64)]).all(), E
    # the entries the failure tests fail: with rows, in three waves of the plan, the last one in the ragged last thread
    case, F, B, g = _lookup("4097 entries of 1 to 3 rows")
    assert all(F[e + 1] > F[e] for e in W.FAIL_ENTRIES)
    assert [e // 5 // 64 for e in W.FAIL_ENTRIES] == [1, 2, 12, 12] and W.FAIL_ENTRIES[3] // 5 == claimed[4097][1] and W.FAIL_ENTRIES[3] == 4097 - 1

    # -- rowless runs: the lone search exactly from 63 entries between two rows of a wave on
    case, F, B, g = _lookup("rowless runs of 62 to 200 entries")
    assert g.per == 4
    e, positions = 0, set()
    for R in W.RUNS:
        for n in W.RUN_ROWS:
            front, behind = int(F[e]) + n - 1, int(F[e]) + n      # the rows in front of and behind the run
            assert F[e] % 4 == 0 and F[e + 1] - F[e] == n and (np.diff(F[e + 1:e + R + 2]) == 0).all() and F[e + R + 2] > F[e + R + 1] == behind
            assert {len(d) for _, d in case["items"][e + 1:e + R + 1]} == {0, 3, 40} and set(case["store"][e + 1:e + 4]) == {False, True}
            positions.add(front % 4)
            same_wave = front // 4 == behind // 4
            assert same_wave == (n < 4)
            assert bool(g.fallback[behind]) == (same_wave and R >= 63), (R, n)
            assert g.fallback[behind:int(F[e + R + 2])].all() == bool(g.fallback[behind]) and g.entry[behind] == e + R + 1
            e += R + 2
    assert positions == {0, 1, 2, 3} and e == len(case["items"]) and int(g.fallback.sum()) == 4 * (3 + 2 + 1)
    assert 8 in W.written(case["label"]).methods

    # -- the dispatch seam: the same entries at 65535 rows (16 a workgroup) and at 65536 (256 a workgroup, 64 a wave)
    for n, group in ((65535, k.ROWS_FEW), (65536, k.ROWS_MAX)):
        case, F, B, g = _lookup("%d rows across the seams" % n)
        w = W.written(case["label"])
        assert B == n and g.rows_per_group == group and g.per == group // 4
        assert (n >= k.ROWS_MANY_MIN) == (n == 65536) and B % group == (0 if n == 65536 else 15)      # (65535: a partial last group)
        assert -(-B // k.JT) > 128                               # tiles: the look-backs go on past their first window of 64, twice
        assert [d[:32 * 100] for _, d in case["items"][:12]] == [d[:32 * 100] for _, d in W.shape_case("65535 rows across the seams")["items"][:12]]
        assert set((F % 64).tolist()) >= {0, 1} and set((F % 256).tolist()) >= {0, 1} and any(f // k.JT > 64 for f in F[:-1])
        spans = lambda e, step: (F[e] // step + 1) * step < F[e + 1]
        stored = [e for e in range(len(F) - 1) if w.methods[e] == 0 and F[e + 1] > F[e]]
        assert len(stored) >= 2 and [W.SEAM_FORMS[e] for e in stored] == ["n"] * len(stored)
        assert any(spans(e, k.JT) and spans(e, group) and F[e + 1] - F[e] > 32 * k.JT for e in stored)      # stored with rows, over many tiles and groups
        assert any(W.SEAM_FORMS[e] == "m" and w.methods[e] == 8 and F[e + 1] - F[e] > 64 * k.JT for e in range(len(F) - 1))
        assert {p >= 3 for p in w.pads} == {False, True}         # both marker lengths among the members of deflated entries
    # the rows the failure tests tamper with: in entries of many tiles, away from their ends, behind tile 64 and behind tile 128
    (e1, b1), (e2, b2) = W.SEAM_STATUS, W.SEAM_CONTRADICTION
    assert e1 < e2 and F[e1] + 1024 < b1 < F[e1 + 1] - 1024 and F[e2] + 1024 < b2 < F[e2 + 1] - 1024
    assert b1 // k.JT > 64 and b2 // k.JT > 128 and F[e1] // k.JT < 64 < 128 < F[e2] // k.JT      # cnt[F1] - cnt[F0] across look-back windows
    assert all(F[e + 1] > F[e] for e in (e1 - 1, e1 + 1, e2 - 1, e2 + 1))
    assert w.methods[e1] == 0 and w.methods[e2] == 8

    # -- many entries and many rows at once: three rounds and the lone search with 64 rows a wave, per = 64 in the plan
    case, F, B, g = _lookup("65535 entries and more rows")
    w = W.written(case["label"])
    rows = np.diff(F)
    assert len(case["items"]) == 65535 and B >= k.ROWS_MANY_MIN and g.per == 64 and 3 in set(g.rounds.tolist())
    assert set(rows.tolist()) == {0, 1, 2, 3}
    with_rows = sum(1 for m, n in zip(w.methods, rows) if m == 0 and n)
    assert 65535 // 12 < with_rows < 65535 // 5 and w.methods.count(8) > 30000
    lo, hi = W.MANY_ROWS_RUN[0], sum(W.MANY_ROWS_RUN)
    assert not rows[lo:hi].any() and rows[lo - 1] and rows[hi]
    assert (F[lo] - 1) // 64 == F[hi] // 64 and g.fallback[F[hi]] and g.entry[F[hi]] == hi      # the rows on either side of the run in one wave
    assert {p >= 3 for p in w.pads} == {False, True}

    # -- stored tiles among many entries: the tiles' search runs over a prefix in which most entries have one tile or none
    case, F, B, g = _lookup("stored tiles among 300 entries")
    w = W.written(case["label"])
    tiles = [-(-len(d) // k.STORE_TILE) if F[e + 1] == F[e] else 0 for e, (_, d) in enumerate(case["items"])]
    assert len(tiles) == 300 and tiles.count(0) > 30 and tiles.count(1) > 150 and sorted(t for t in tiles if t > 1) == [2, 4]
    assert sorted(len(d) for (_, d), s in zip(case["items"], case["store"]) if s) == list(W.BIG_STORED)
    assert w.methods.count(8) == 3 and B > 3 and case["block"] == 2048


def test_numpy_loads_the_reference_npz():
    arrays = W.npz_arrays()
    for store in (None, [True] * len(arrays)):
        w = W.expected(W.npz_items(arrays), block=1 << 16, store=store)
        back = np.load(io.BytesIO(w.file))
        assert sorted(back.files) == sorted(arrays)
        for name, a in arrays.items():
            assert back[name].dtype == a.dtype and back[name].shape == a.shape and np.array_equal(back[name], a), name
        assert (8 in w.methods) == (store is None)
    from hdl_deflate_amd import npz
    import torch
    assert [npz._npy_descr(t) for t in (torch.bool, torch.float16, torch.complex128)] == ["|b1", "<f2", "<c16"]
    for name, a in arrays.items():                           # the descr table is the reverse of load_npz's
        assert npz._torch_dtype(np.lib.format.dtype_to_descr(a.dtype))[1] == a.dtype
        assert npz._npy_descr(npz._torch_dtype(np.lib.format.dtype_to_descr(a.dtype))[0]) == np.lib.format.dtype_to_descr(a.dtype), name
    with pytest.raises(npz.Error):
        npz._npy_descr(torch.bfloat16)
