"""CPU: the extension header include/hdlz_zip64.h -- every declaration exported and bound with its arity, the tables in front of it and
the version as they were, the queries equal to their closed forms, every parameter refusal in the header's order and in front of the
device, no CPU path behind good parameters, the ctypes mirrors of the structs; and the rule as tests/zip64_ref.py states it held
against zipfile, unzip and numpy on every archive the GPU tests use -- THE INDEX RULE on the archives read, THE FILE RULE on the files
written, whose index under the first rule is the writer's own records."""
import ctypes
import io
import os
import re
import subprocess
import zipfile

import numpy as np
import pytest

import zip_ref as Z
import zip64_ref as R
from cabi_common import declarations, header, host_buffer as _host_buffer, no_device as _no_device, r256
from test_zip_cabi import _pairs

E_BAD_PARAM, E_HIP = 8, 9
UNZIP = "/usr/bin/unzip"


def test_every_declaration_is_exported_and_bound():
    from hdl_deflate_amd import _lib
    text = header("hdlz_zip64.h")
    params = declarations(text)
    assert params == {"hdlz_zip64_index_work_bytes": 2, "hdlz_zip64_index_ws": 9, "hdlz_zip64_inflate_work_bytes": 3, "hdlz_zip64_inflate_ws": 13,
                      "hdlz_zip64_write_bound": 5, "hdlz_zip64_write_work_bytes": 2, "hdlz_zip64_write_ws": 26}
    assert sorted(params) == sorted(_lib.ZIP64_EXPORTS) == sorted(_lib.ZIP64_SIGNATURES)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    L = _lib.load()
    for name, n in params.items():
        assert hasattr(raw, name), name
        restype, argtypes = _lib.ZIP64_SIGNATURES[name]
        assert len(argtypes) == n, name
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert '#include "hdlz_zip_write.h"' in text
    # the same parameters as the classic calls
    assert _lib.ZIP64_SIGNATURES["hdlz_zip64_index_ws"] == _lib.ZIP_SIGNATURES["hdlz_zip_index_ws"]
    assert _lib.ZIP64_SIGNATURES["hdlz_zip64_inflate_ws"] == _lib.ZIP_SIGNATURES["hdlz_zip_inflate_ws"]
    classic = _lib.ZIP_WRITE_SIGNATURES["hdlz_zip_write_ws"]
    assert _lib.ZIP64_SIGNATURES["hdlz_zip64_write_ws"] == (classic[0], classic[1][:17] + [ctypes.c_uint64] + classic[1][17:])      # zip64_from behind out_align
    assert _lib.ZIP64_SIGNATURES["hdlz_zip64_write_bound"] == _lib.ZIP_WRITE_SIGNATURES["hdlz_zip_write_bound"]


def test_the_tables_in_front_of_it_are_as_they_were():
    from hdl_deflate_amd import _lib
    older = (_lib.EXPORTS, _lib.JOIN_EXPORTS, _lib.UNJOIN_EXPORTS, _lib.GZIP_EXPORTS, _lib.BGZF_EXPORTS, _lib.BGZF_RANGE_EXPORTS, _lib.BGZF_STORED_EXPORTS,
             _lib.GUNZIP_EXPORTS, _lib.ZIP_EXPORTS, _lib.ZIP_WRITE_EXPORTS)
    assert [len(t) for t in older] == [22, 4, 2, 7, 8, 2, 3, 2, 4, 3]
    assert len(_lib.ZIP64_EXPORTS) == 7 and not set(_lib.ZIP64_EXPORTS) & set().union(*older)
    assert _lib.load().hdlz_version() == 0x000600
    assert "hdlz_zip64.h" in header("hdlz_zip.h") and "hdlz_zip64.h" in header("hdlz_zip_write.h")      # the "out of scope" sentences point here


def test_the_struct_mirrors_match_the_header():
    from hdl_deflate_amd import _lib
    from hdl_deflate_amd.zip import ENTRY_DTYPE, ENTRY64_DTYPE
    text = header("hdlz_zip64.h")
    body = re.search(r"typedef\s+struct\s+hdlz_zip64_entry\s*\{(.*?)\}\s*hdlz_zip64_entry\s*;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    m = [(t, n.strip()) for t, names in re.findall(r"(uint64_t|uint32_t|uint16_t)\s+([\w,\s]+);", body) for n in names.split(",")]
    size = {"uint64_t": 8, "uint32_t": 4, "uint16_t": 2}
    mirror = _lib.Zip64Entry
    assert [n for _, n in m] == [f[0] for f in mirror._fields_]
    assert [size[t] for t, _ in m] == [ctypes.sizeof(f[1]) for f in mirror._fields_]
    o = 0
    for t, n in m:                                          # (every member is naturally aligned where it stands: no padding)
        assert getattr(mirror, n).offset == o and o % size[t] == 0, n
        o += size[t]
    assert ctypes.sizeof(mirror) == o == 64 and ctypes.sizeof(_lib.ZipIndexResult) == 40 and ctypes.sizeof(_lib.ZipWriteResult) == 40
    assert [(n, ENTRY64_DTYPE.fields[n][1], ENTRY64_DTYPE.fields[n][0].itemsize) for n in ENTRY64_DTYPE.names] == \
        [(f[0], getattr(mirror, f[0]).offset, ctypes.sizeof(f[1])) for f in mirror._fields_]
    assert set(ENTRY_DTYPE.names) <= set(ENTRY64_DTYPE.names)           # code that reads index.host[...] works on both
    assert ENTRY64_DTYPE.names[:3] == ENTRY_DTYPE.names[:3] == ("cd_off", "payload_off", "out_off")      # (inflate_zip reads column 2)


def test_the_queries_are_their_closed_forms():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    for file_len in (0, 22, 1 << 20, (1 << 32) - 1, 1 << 32, 1 << 40, (1 << 64) - 1):
        for cap in (0, 1, 15, 16, 17, 65535, 65536, 131073, 1 << 20, (1 << 31) - 1):
            assert L.hdlz_zip64_index_work_bytes(file_len, cap) == 256 + r256(16 * cap), (file_len, cap)
        assert L.hdlz_zip64_index_work_bytes(file_len, 1 << 31) == 0
    row = lambda cap: min(cap & ~3, (1 << 32) - 512)
    for count in (1, 2, 10, 11, 4096, (1 << 31) - 1):
        for in_len in (0, 100, 2048, 16390, 1 << 20, (1 << 28) - 1, (1 << 32) - 1):
            for out_cap in (0, 3, 4, 5, 32768, 32769, 1 << 22, (1 << 22) + 2, (1 << 32) - 512, 1 << 32, (1 << 32) + 8, 1 << 36):
                t = r256(4 * ((out_cap + 32767) // 32768)) if count == 1 else 0
                d = r256(L.hdlz_inflate_work_bytes(1, in_len, row(out_cap), 0, 1)) if count == 1 else 0
                assert L.hdlz_zip64_inflate_work_bytes(count, in_len, out_cap) == 2 * r256(24 * count) + t + d, (count, in_len, out_cap)
                if out_cap <= (1 << 32) - 512:
                    assert L.hdlz_zip64_inflate_work_bytes(count, in_len, out_cap) == L.hdlz_zip_inflate_work_bytes(count, in_len, out_cap)
    assert L.hdlz_zip64_inflate_work_bytes(0, 0, 0) == 0 and L.hdlz_zip64_inflate_work_bytes(1 << 31, 0, 0) == 0
    for E in (0, 1, 31, 32, 63, 64, 65535, 65536, 131073, (1 << 31) - 1):
        for B in (0, 1, 255, 256, 257, 65537, (1 << 31) - 1):
            assert L.hdlz_zip64_write_work_bytes(E, B) == R.write_work_bytes(E, B), (E, B)
        for total, names in ((0, 0), (5, 7), (1 << 32, 1 << 20), (1 << 40, 3)):
            assert L.hdlz_zip64_write_bound(E, 9, 32, total, names) == R.write_bound(E, total, names) == 98 + 124 * E + 2 * names + total
    assert L.hdlz_zip64_write_work_bytes(1 << 31, 0) == 0 and L.hdlz_zip64_write_work_bytes(0, 1 << 31) == 0


def test_index_parameter_errors_come_before_the_device_in_their_order():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    keep, base = _host_buffer((1 << 20) + 4096)
    wb = L.hdlz_zip64_index_work_bytes(1000, 4)
    assert wb == 512
    good = dict(file=base, file_len=1000, cap=4, align=1, entries=base + 4096, result=base + 8192, work=base + 16384, work_bytes=wb)

    def call(**kw):
        a = dict(good, **kw)
        return L.hdlz_zip64_index_ws(a["file"], a["file_len"], a["cap"], a["align"], a["entries"], a["result"], a["work"], a["work_bytes"], None)

    faults = [(dict(result=None), b"null device pointer"), (dict(entries=None), b"d_entries is null"), (dict(cap=1 << 31), b"entry_cap too large"),
              (dict(align=3), b"out_align"), (dict(work_bytes=wb - 1), b"hdlz_zip64_index_work_bytes"), (dict(work=base + 16384 + 4), b"8-byte")]
    _pairs(L, call, faults)
    assert call(file=None) == E_BAD_PARAM and b"null device pointer" in L.hdlz_last_error()
    for align in (0, 6, 512, 1 << 31):
        assert call(align=align) == E_BAD_PARAM and b"out_align" in L.hdlz_last_error()
    assert call(work=None) == E_BAD_PARAM and b"hdlz_zip64_index_work_bytes" in L.hdlz_last_error()
    assert call(cap=17) == E_BAD_PARAM and b"hdlz_zip64_index_work_bytes" in L.hdlz_last_error()       # the scratch is sized from entry_cap
    assert call(entries=base + 4100) == E_BAD_PARAM and call(result=base + 8196) == E_BAD_PARAM and b"8-byte" in L.hdlz_last_error()
    if _no_device():
        assert call() == E_HIP
        for file_len in (1 << 32, 1 << 40, (1 << 64) - 1):      # any file_len
            assert call(file_len=file_len) == E_HIP
        assert call(cap=0, entries=None, work_bytes=256) == E_HIP              # the sizing call
        assert call(file=None, file_len=0) == E_HIP and call(file=base + 1) == E_HIP


def test_inflate_parameter_errors_come_before_the_device_in_their_order():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    keep, base = _host_buffer(1 << 16)
    wb = L.hdlz_zip64_inflate_work_bytes(2, 0, 4096)
    assert wb == 512
    good = dict(file=base, file_len=1000, entries=base + 4096, first=0, count=2, in_len=0, out=base + 8192, out_cap=4096, st=base + 16384,
                result=base + 16640, work=base + 20480, work_bytes=wb)

    def call(**kw):
        a = dict(good, **kw)
        return L.hdlz_zip64_inflate_ws(a["file"], a["file_len"], a["entries"], a["first"], a["count"], a["in_len"], a["out"], a["out_cap"], a["st"],
                                       a["result"], a["work"], a["work_bytes"], None)

    faults = [(dict(result=None), b"d_result is required"), (dict(file=None), b"null device pointer"), (dict(out=None), b"d_out is null"),
              (dict(first=(1 << 31) - 1), b"first + count too large"), (dict(entries=base + 4100), b"d_entries / d_result"),
              (dict(st=base + 16386), b"d_entry_status"), (dict(work=base + 20480 + 128), b"256-byte"),
              (dict(work_bytes=wb - 1), b"hdlz_zip64_inflate_work_bytes")]
    _pairs(L, call, faults)
    assert call(count=1 << 31) == E_BAD_PARAM and b"first + count too large" in L.hdlz_last_error()
    assert call(work=None) == E_BAD_PARAM and b"hdlz_zip64_inflate_work_bytes" in L.hdlz_last_error()
    assert call(result=None, count=0, work=None, work_bytes=0) == E_BAD_PARAM
    if _no_device():
        assert call() == E_HIP and call(st=None) == E_HIP
        for file_len in (1 << 32, 1 << 40):                     # any file_len
            assert call(file_len=file_len) == E_HIP
        assert call(out=None, out_cap=0) == E_HIP and call(out=base + 8193) == E_HIP
        assert call(count=0, file=None, entries=None, work=None, work_bytes=0) == E_HIP
        one = L.hdlz_zip64_inflate_work_bytes(1, 1 << 20, 4096)
        assert call(count=1, in_len=1 << 20, work_bytes=one) == E_HIP and call(count=1, in_len=1 << 20, work_bytes=wb) == E_BAD_PARAM


def test_write_parameter_errors_come_before_the_device_in_their_order():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    keep, base = _host_buffer(1 << 16)
    wb = L.hdlz_zip64_write_work_bytes(2, 3)
    at = lambda k: base + 1024 * k
    good = dict(d_in=at(0), ent_off=at(1), names=at(2), name_off=at(3), E=2, in_off=at(4), rows=at(5), pitch=64, len=at(6), end_bits=at(7), status=at(8), B=3,
                blk_first=at(9), crc=at(10), flags=0, dt=0x210000, align=1, z=0xFFFFFFFF, total=100, file=at(11), cap=512, entries=at(12), result=at(13),
                work=at(16), work_bytes=wb)
    order = ("d_in", "ent_off", "names", "name_off", "E", "in_off", "rows", "pitch", "len", "end_bits", "status", "B", "blk_first", "crc", "flags", "dt",
             "align", "z", "total", "file", "cap", "entries", "result", "work", "work_bytes")

    def call(**kw):
        a = dict(good, **kw)
        return L.hdlz_zip64_write_ws(*[a[k] for k in order], None)

    faults = [(dict(result=None), b"d_result is required"), (dict(E=1 << 31), b"nentries too large"), (dict(B=1 << 31), b"nblocks too large"),
              (dict(crc=None), b"(the entries)"), (dict(rows=None), b"(the rows)"), (dict(file=None), b"d_file is null"), (dict(flags=1), b"flags"),
              (dict(align=3), b"out_align"), (dict(z=1 << 32), b"zip64_from"), (dict(work_bytes=wb - 1), b"hdlz_zip64_write_work_bytes"),
              (dict(entries=at(12) + 4), b"8-byte"), (dict(len=at(6) + 2), b"4-byte")]
    _pairs(L, call, faults)
    assert call(E=0) == E_BAD_PARAM and b"rows without entries" in L.hdlz_last_error()
    assert call(work=None) == E_BAD_PARAM and b"hdlz_zip64_write_work_bytes" in L.hdlz_last_error()
    assert call(E=70000) == E_BAD_PARAM and b"hdlz_zip64_write_work_bytes" in L.hdlz_last_error()      # 65536 entries and more are no refusal of their own
    if _no_device():
        assert call() == E_HIP
        for z in (0, 1, 12345, 0xFFFFFFFE):                      # any zip64_from up to FFFFFFFF
            assert call(z=z) == E_HIP
        assert call(E=70000, work_bytes=L.hdlz_zip64_write_work_bytes(70000, 3)) == E_HIP
        assert call(file=None, cap=0) == E_HIP and call(entries=None) == E_HIP
        assert call(E=0, B=0, work_bytes=L.hdlz_zip64_write_work_bytes(0, 0)) == E_HIP


# ---- THE FILE RULE against stock readers and against the index rule
import zip_write_ref as W    # noqa: E402

WRITE_LABELS = [c["label"] for c in W.all_cases()]
FROMS = ("standard", "always", "between")


def _from(label, how):
    return {"standard": 0xFFFFFFFF, "always": 0, "between": R.between(label)}[how]


@pytest.mark.parametrize("how", FROMS)
@pytest.mark.parametrize("label", WRITE_LABELS)
def test_the_file_rule_is_read_by_zipfile_unzip_and_the_index_rule(label, how, tmp_path):
    items = {c["label"]: c for c in W.all_cases()}[label]["items"]
    w = R.written(label, _from(label, how))
    if how == "standard":
        assert w.file == W.written(label).file and not w.end64 and not any(w.central)      # the classic writer's bytes
    if how == "always":
        assert w.end64 and all(c == ("usize", "csize", "L") for c in w.central) and all(w.local)
    zf = zipfile.ZipFile(io.BytesIO(w.file))
    infos = zf.infolist()
    assert len(infos) == len(items) and zf.start_dir == w.record["cd_off"]
    offs = R.local_offsets(w)
    for k, (info, en, (_, data)) in enumerate(zip(infos, w.entries, items)):
        assert (info.file_size, info.compress_size, info.CRC, info.header_offset, info.compress_type) == (len(data), en["csize"], en["crc"], offs[k], en["method"])
        assert info.extract_version == (45 if w.central[k] else 20) and info.orig_filename.encode("utf-8" if en["flags"] & 0x800 else "cp437") == en["name"]
    if len(infos) <= 1000:
        assert zf.testzip() is None
    ix = R.index(w.file)                                          # rule 7: the index rule gives the writer's records
    assert (ix["status"], ix["nentries"], ix["cd_off"], ix["cd_size"]) == (Z.OK, len(items), w.record["cd_off"], w.record["cd_size"])
    assert ix["entries"] == w.entries
    assert len(w.file) <= R.write_bound(len(items), sum(len(d) for _, d in items), sum(en["name_len"] for en in w.entries))
    if os.path.exists(UNZIP) and 0 < len(infos) <= 1000:
        f = tmp_path / "a.zip"
        f.write_bytes(w.file)
        got = subprocess.run([UNZIP, "-tqq", str(f)], capture_output=True)
        # (unzip's own limit on a name's length is a warning, exit 1: every entry still tested sound)
        assert got.returncode == 0 or (got.returncode == 1 and set(got.stdout.splitlines()) == {b"warning:  filename too long--truncating."}), (label, got)


def test_a_zip64_from_between_reaches_every_combination():
    """over all cases at their `between` value: local extras with and without, central extras holding the offset alone, sizes alone and
    both -- the reference's own arrays say so"""
    seen_c, seen_l = set(), set()
    for label in WRITE_LABELS:
        w = R.written(label, R.between(label))
        seen_c |= set(w.central)
        seen_l |= set(bool(x) for x in w.local)
    assert seen_l == {True, False}
    assert {(), ("L",), ("usize", "csize", "L")} <= seen_c and any("L" not in c and c for c in seen_c), seen_c


@pytest.mark.parametrize("E", (65535, 65536, 131073))
def test_the_file_rule_at_many_entries(E):
    w = R.expected(R.many_items(E))
    assert w.end64 == (E > 65535) and not any(w.central)
    zf = zipfile.ZipFile(io.BytesIO(w.file))
    assert len(zf.infolist()) == E and zf.start_dir == w.record["cd_off"]
    ix = R.index(w.file)
    assert ix["status"] == Z.OK and ix["entries"] == w.entries


def test_numpy_reads_the_file_rule_npz():
    arrays = W.npz_arrays()
    for z64 in (0xFFFFFFFF, 0, 300):
        w = R.expected(W.npz_items(arrays), z64, block=1 << 16)
        got = np.load(io.BytesIO(w.file))
        assert sorted(got.files) == sorted(arrays) and all(np.array_equal(got[k], v) for k, v in arrays.items())


# ---- the rule against stock readers
WELL_FORMED = R.crafted_cases() + R.many_cases()


@pytest.mark.parametrize("label", [c[0] for c in WELL_FORMED])
def test_the_rule_reads_well_formed_files_as_zipfile_and_unzip_do(label, tmp_path):
    """names, header_offset, sizes, CRC and the bytes of every entry; unzip -t where it is installed"""
    from hdl_deflate_amd.zip import decode_name
    z = dict(WELL_FORMED)[label]
    ix, sts, flat = R.read(z)
    zf = zipfile.ZipFile(io.BytesIO(z))
    infos = zf.infolist()
    assert ix["status"] == Z.OK and ix["nentries"] == len(infos) and sts == [Z.OK] * len(infos)
    assert ix["cd_off"] == zf.start_dir and ix["total_out"] == sum(i.file_size for i in infos)
    L = {i.orig_filename: i.header_offset for i in infos}
    for en, info in zip(ix["entries"], infos):
        assert decode_name(en["name"], en["flags"]) == info.orig_filename
        assert (en["csize"], en["usize"], en["crc"], en["method"], en["flags"]) == (info.compress_size, info.file_size, info.CRC, info.compress_type, info.flag_bits)
        assert z[L[info.orig_filename]:L[info.orig_filename] + 4] == Z.SIG_LOCAL and en["payload_off"] >= info.header_offset + 30
    step = max(1, len(infos) // 40)
    for en, info in list(zip(ix["entries"], infos))[::step]:
        assert flat[en["out_off"]:en["out_off"] + en["usize"]] == zf.read(info)
    if len(infos) <= 1000:
        assert zf.testzip() is None
    if os.path.exists(UNZIP) and len(infos):
        f = tmp_path / "a.zip"
        f.write_bytes(z)
        assert subprocess.run([UNZIP, "-tqq", str(f)], capture_output=True).returncode == 0, label


@pytest.mark.parametrize("label", [c[0] for c in Z.all_archives()])
def test_a_file_without_zip64_reads_as_under_the_classic_rule(label):
    """no locator and no all-ones word: the new rule is the old one (a file with a locator the old rule refuses and the new one may
    not: that case alone may differ)"""
    z = dict(Z.all_archives())[label]
    for align, cap in ((1, None), (64, None), (1, 10 ** 6)):
        a, b = Z.index(z, align, cap), R.index(z, align, cap)
        assert a == b or label == "a ZIP64 locator", label


@pytest.mark.parametrize("k", range(len(R.bad_cases())), ids=[c[0] for c in R.bad_cases()])
def test_one_edit_away_from_a_good_file(k):
    label, z, want, kept, e = R.bad_cases()[k]
    ix, sts, flat = R.read(z)
    assert (ix["status"], ix["nentries"]) == (want, kept), (label, ix["status"], ix["nentries"])
    assert [s != Z.OK for s in sts] == [j == e for j in range(kept)] and (e is None or ix["entries"][e]["status"] == Z.E_BAD_HEADER), (label, sts)


def test_entry_cap_and_the_sizing_call():
    z = R.make_zip64(R.three_items(), always=True)
    full = R.index(z)
    assert full["total_out"] == 300 + 77 + 5000
    assert (R.index(z, entry_cap=0)["status"], R.index(z, entry_cap=0)["total_out"], R.index(z, entry_cap=0)["nentries"]) == (Z.E_OUT_CAPACITY, 0, 3)
    assert (R.index(z, entry_cap=2)["status"], R.index(z, entry_cap=2)["total_out"]) == (Z.E_OUT_CAPACITY, 377)
    assert R.index(z, entry_cap=3) == R.index(z, entry_cap=4) == full


def test_numpy_reads_an_npz_in_the_always_layout():
    arrays = dict(a=np.arange(500, dtype=np.int64), b=np.linspace(0, 1, 300, dtype=np.float32))
    items = []
    for name, a in arrays.items():
        buf = io.BytesIO()
        np.lib.format.write_array(buf, a)
        items.append(dict(name=name.encode() + b".npy", data=buf.getvalue(), method=0))
    z = R.make_zip64(items, always=True)
    got = np.load(io.BytesIO(z))
    assert all(np.array_equal(got[k], v) for k, v in arrays.items()) and R.index(z)["status"] == Z.OK
