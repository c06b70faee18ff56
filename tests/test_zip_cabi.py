"""CPU: the extension header include/hdlz_zip.h -- every declaration exported and bound with its arity, the tables in front of it and
the version as they were, both work-bytes queries equal to their closed forms, every parameter refusal in the header's order and in front
of the device, no CPU path behind good parameters, the ctypes mirrors of the two structs; and the rule as tests/zip_ref.py states it held
against zipfile on every archive the GPU tests use."""
import ctypes
import io
import re
import zipfile

import numpy as np
import pytest

import zip_ref as Z
from cabi_common import declarations, header, host_buffer as _host_buffer, no_device as _no_device, r256

E_BAD_PARAM, E_HIP = 8, 9


def test_every_declaration_is_exported_and_bound():
    from hdl_deflate_amd import _lib
    text = header("hdlz_zip.h")
    params = declarations(text)
    assert params == {"hdlz_zip_index_work_bytes": 2, "hdlz_zip_index_ws": 9, "hdlz_zip_inflate_work_bytes": 3, "hdlz_zip_inflate_ws": 13}
    assert sorted(params) == sorted(_lib.ZIP_EXPORTS) == sorted(_lib.ZIP_SIGNATURES)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    L = _lib.load()
    for name, n in params.items():
        assert hasattr(raw, name), name
        restype, argtypes = _lib.ZIP_SIGNATURES[name]
        assert len(argtypes) == n, name
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert '#include "hdlz_gzip.h"' in text
    assert int(re.search(r"#define\s+HDLZ_ZIP_LARGE_MIN\s+(\d+)u", text).group(1)) == _lib.ZIP_LARGE_MIN == Z.LARGE_MIN
    import hdl_deflate_amd
    assert callable(hdl_deflate_amd.load_npz) and hdl_deflate_amd.ZipIndex is not None


def test_the_tables_in_front_of_it_are_as_they_were():
    from hdl_deflate_amd import _lib
    older = (_lib.EXPORTS, _lib.JOIN_EXPORTS, _lib.UNJOIN_EXPORTS, _lib.GZIP_EXPORTS, _lib.BGZF_EXPORTS, _lib.BGZF_RANGE_EXPORTS, _lib.BGZF_STORED_EXPORTS,
             _lib.GUNZIP_EXPORTS)
    assert [len(t) for t in older] == [22, 4, 2, 7, 8, 2, 3, 2]
    assert len(_lib.ZIP_EXPORTS) == 4 and not set(_lib.ZIP_EXPORTS) & set().union(*older)
    assert _lib.load().hdlz_version() == 0x000600
    assert "hdlz_zip.h" in header("hdlz_gunzip.h")          # the "out of scope" sentence points here


def test_the_struct_mirrors_match_the_header():
    from hdl_deflate_amd import _lib
    from hdl_deflate_amd.zip import ENTRY_DTYPE
    text = header("hdlz_zip.h")
    # (the header declares several members per line: expand them)
    def members(struct):
        body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (struct, struct), text, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return [(t, n.strip()) for t, names in re.findall(r"(uint64_t|uint32_t|uint16_t)\s+([\w,\s]+);", body) for n in names.split(",")]
    size = {"uint64_t": 8, "uint32_t": 4, "uint16_t": 2}
    for struct, mirror, total in (("hdlz_zip_entry", _lib.ZipEntry, 48), ("hdlz_zip_index_result", _lib.ZipIndexResult, 40),
                                  ("hdlz_zip_inflate_result", _lib.ZipInflateResult, 24)):
        m = members(struct)
        assert [n for _, n in m] == [f[0] for f in mirror._fields_], struct
        assert [size[t] for t, _ in m] == [ctypes.sizeof(f[1]) for f in mirror._fields_], struct
        o = 0
        for t, n in m:                                      # (every member is naturally aligned where it stands: no padding)
            assert getattr(mirror, n).offset == o and o % size[t] == 0, (struct, n)
            o += size[t]
        assert ctypes.sizeof(mirror) == o == total, struct
    assert [(n, ENTRY_DTYPE.fields[n][1], ENTRY_DTYPE.fields[n][0].itemsize) for n in ENTRY_DTYPE.names] == \
        [(f[0], getattr(_lib.ZipEntry, f[0]).offset, ctypes.sizeof(f[1])) for f in _lib.ZipEntry._fields_]


def test_the_queries_are_their_closed_forms():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    for file_len in (0, 21, 22, 1 << 20, (1 << 32) - 1):
        for cap in (0, 1, 65535, 1 << 20):
            assert L.hdlz_zip_index_work_bytes(file_len, cap) == 256 + 2 * 262144 == 524544
    assert L.hdlz_zip_index_work_bytes(1 << 32, 0) == 0
    for count in (1, 2, 10, 11, 21, 22, 4096, 65535, (1 << 31) - 1):
        for in_len in (0, 100, 2047, 2048, 16390, 1 << 20, (1 << 28) - 1):
            for out_cap in (0, 3, 4, 5, 32768, 32769, 70000, 1 << 22, (1 << 22) + 2):
                t = r256(4 * ((out_cap + 32767) // 32768)) if count == 1 else 0
                d = r256(L.hdlz_inflate_work_bytes(1, in_len, out_cap & ~3, 0, 1)) if count == 1 else 0
                assert L.hdlz_zip_inflate_work_bytes(count, in_len, out_cap) == 2 * r256(24 * count) + t + d, (count, in_len, out_cap)
    assert L.hdlz_zip_inflate_work_bytes(0, 0, 0) == 0 and L.hdlz_zip_inflate_work_bytes(1 << 31, 0, 0) == 0
    assert L.hdlz_zip_inflate_work_bytes(2, 0, 1 << 22) == 512
    assert L.hdlz_zip_inflate_work_bytes(1, 1 << 20, 1 << 22) > L.hdlz_zip_inflate_work_bytes(1, 2047, 1 << 22)      # the whole-GPU path's share


def _pairs(L, call, faults, independent=lambda a, b: True):
    for kw, word in faults:
        assert call(**kw) == E_BAD_PARAM and word in L.hdlz_last_error(), (kw, L.hdlz_last_error())
    for i, (kw_i, word_i) in enumerate(faults):              # ... and every pair: the earlier one answers
        for kw_j, _ in faults[i + 1:]:
            if set(kw_i) & set(kw_j) or not independent(kw_i, kw_j):
                continue
            assert call(**dict(kw_j, **kw_i)) == E_BAD_PARAM and word_i in L.hdlz_last_error(), (kw_i, kw_j, L.hdlz_last_error())


def test_index_parameter_errors_come_before_the_device_in_their_order():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    keep, base = _host_buffer((1 << 20) + 4096)
    wb = L.hdlz_zip_index_work_bytes(1000, 4)
    good = dict(file=base, file_len=1000, cap=4, align=1, entries=base + 4096, result=base + 8192, work=base + 16384, work_bytes=wb)

    def call(**kw):
        a = dict(good, **kw)
        return L.hdlz_zip_index_ws(a["file"], a["file_len"], a["cap"], a["align"], a["entries"], a["result"], a["work"], a["work_bytes"], None)

    faults = [(dict(result=None), b"null device pointer"), (dict(entries=None), b"d_entries is null"), (dict(file_len=1 << 32), b"file_len too large"),
              (dict(cap=1 << 32), b"entry_cap too large"), (dict(align=3), b"out_align"), (dict(work_bytes=wb - 1), b"hdlz_zip_index_work_bytes"),
              (dict(work=base + 16384 + 4), b"8-byte")]
    _pairs(L, call, faults)
    assert call(file=None) == E_BAD_PARAM and b"null device pointer" in L.hdlz_last_error()
    for align in (0, 6, 512, 1 << 31):
        assert call(align=align) == E_BAD_PARAM and b"out_align" in L.hdlz_last_error()
    assert call(work=None) == E_BAD_PARAM and b"hdlz_zip_index_work_bytes" in L.hdlz_last_error()
    assert call(entries=base + 4100) == E_BAD_PARAM and call(result=base + 8196) == E_BAD_PARAM and b"8-byte" in L.hdlz_last_error()
    if _no_device():
        assert call() == E_HIP
        for align in (1, 2, 64, 256):
            assert call(align=align) == E_HIP
        assert call(cap=0, entries=None) == E_HIP              # the sizing call
        assert call(file=None, file_len=0) == E_HIP and call(file=base + 1) == E_HIP


def test_inflate_parameter_errors_come_before_the_device_in_their_order():
    from hdl_deflate_amd import _lib
    L = _lib.load()
    keep, base = _host_buffer(1 << 16)
    wb = L.hdlz_zip_inflate_work_bytes(2, 0, 4096)
    assert wb == 512
    good = dict(file=base, file_len=1000, entries=base + 4096, first=0, count=2, in_len=0, out=base + 8192, out_cap=4096, st=base + 16384,
                result=base + 16640, work=base + 20480, work_bytes=wb)

    def call(**kw):
        a = dict(good, **kw)
        return L.hdlz_zip_inflate_ws(a["file"], a["file_len"], a["entries"], a["first"], a["count"], a["in_len"], a["out"], a["out_cap"], a["st"],
                                     a["result"], a["work"], a["work_bytes"], None)

    faults = [(dict(result=None), b"d_result is required"), (dict(file=None), b"null device pointer"), (dict(out=None), b"d_out is null"),
              (dict(first=(1 << 31) - 1), b"first + count too large"), (dict(file_len=1 << 32), b"file_len too large"),
              (dict(entries=base + 4100), b"d_entries / d_result"), (dict(st=base + 16386), b"d_entry_status"),
              (dict(work=base + 20480 + 128), b"256-byte"), (dict(work_bytes=wb - 1), b"hdlz_zip_inflate_work_bytes")]
    _pairs(L, call, faults)
    assert call(entries=None) == E_BAD_PARAM and b"null device pointer" in L.hdlz_last_error()
    assert call(count=1 << 31) == E_BAD_PARAM and b"first + count too large" in L.hdlz_last_error()
    assert call(result=base + 16644) == E_BAD_PARAM and b"8-byte" in L.hdlz_last_error()
    assert call(work=None) == E_BAD_PARAM and b"hdlz_zip_inflate_work_bytes" in L.hdlz_last_error()
    assert call(result=None, count=0, work=None, work_bytes=0) == E_BAD_PARAM                 # required, always
    if _no_device():
        assert call() == E_HIP
        assert call(st=None) == E_HIP                                                          # nullable
        assert call(out=None, out_cap=0) == E_HIP and call(out=base + 8193) == E_HIP           # slots at any alignment
        assert call(count=0, file=None, entries=None, work=None, work_bytes=0) == E_HIP
        one = L.hdlz_zip_inflate_work_bytes(1, 1 << 20, 4096)
        assert call(count=1, in_len=1 << 20, work_bytes=one) == E_HIP and call(count=1, in_len=1 << 20, work_bytes=wb) == E_BAD_PARAM
        assert call(first=7, count=1, work_bytes=one) == E_HIP


# ---- the rule against zipfile
def _zipfile_view(z):
    zf = zipfile.ZipFile(io.BytesIO(z))
    return zf, zf.infolist()


@pytest.mark.parametrize("label", [c[0] for c in Z.writer_cases() + Z.lookalike_cases() + Z.geometry_cases()])
def test_the_rule_reads_well_formed_files_as_zipfile_does(label):
    """names, header_offset, sizes, CRC and the bytes of every entry"""
    from hdl_deflate_amd.zip import decode_name
    z = dict(Z.writer_cases() + Z.lookalike_cases() + Z.geometry_cases())[label]
    ix, sts, flat = Z.read(z)
    try:
        zf, infos = _zipfile_view(z)
    except zipfile.BadZipFile:
        # zipfile takes the LAST end-record signature in the file, also one inside the archive comment, and gives up there; the rule
        # asks that the comment fits.  The same file with that comment blanked reads the same under the rule, and zipfile reads it
        assert label in ("signatures everywhere", "an end record in the comment")
        clen = Z._u16(z, ix["cd_off"] + ix["cd_size"] + 20)
        blank = z[:len(z) - clen] + b"x" * clen
        assert Z.read(blank) == (ix, sts, flat)
        z = blank
        zf, infos = _zipfile_view(z)
    assert ix["status"] == Z.OK and ix["nentries"] == len(infos) and sts == [Z.OK] * len(infos)
    assert ix["cd_off"] == zf.start_dir and ix["total_out"] == sum(i.file_size for i in infos)
    for en, info in zip(ix["entries"], infos):
        assert decode_name(en["name"], en["flags"]) == info.orig_filename
        assert (Z._u32(z, en["cd_off"] + 42), en["csize"], en["usize"], en["crc"], en["method"], en["flags"]) == \
            (info.header_offset, info.compress_size, info.file_size, info.CRC, info.compress_type, info.flag_bits)
    step = max(1, len(infos) // 50)                          # (65535 entries: every 1310th is read)
    for en, info in list(zip(ix["entries"], infos))[::step]:
        assert flat[en["out_off"]:en["out_off"] + en["usize"]] == zf.read(info)
    assert zf.testzip() is None
    if label == "savez_compressed":
        assert all(Z._u16(z, Z._u32(z, en["cd_off"] + 42) + 28) == 20 and Z._u16(z, en["cd_off"] + 30) == 0 for en in ix["entries"])
    for align in (64, 256):
        ia = Z.index(z, align)
        assert all(en["out_off"] % align == 0 for en in ia["entries"]) and ia["total_out"] >= ix["total_out"]
        assert [en["usize"] for en in ia["entries"]] == [en["usize"] for en in ix["entries"]]


@pytest.mark.parametrize("k", range(len(Z.entry_damage_cases())), ids=[c[0] for c in Z.entry_damage_cases()])
def test_zipfile_rejects_the_entry_the_rule_rejects(k):
    """exactly the damaged entry fails under the rule, its neighbours read byte-exact; zipfile fails the same entry wherever it can
    tell (it reads sizes from the directory and cannot see a csize that is too large, and it takes a local offset on trust until the
    signature there is missing)"""
    label, z, e, want = Z.entry_damage_cases()[k]
    ix, sts, flat = Z.read(z)
    good = Z.read(Z.make_zip(Z.base_items()))
    assert ix["status"] == Z.OK and [s != Z.OK for s in sts] == [j == e for j in range(9)], (label, sts)
    assert want is None or sts[e] == want, (label, sts[e], want)
    for j, en in enumerate(ix["entries"]):
        if j != e:
            g = good[0]["entries"][j]
            assert flat[en["out_off"]:en["out_off"] + en["usize"]] == good[2][g["out_off"]:g["out_off"] + g["usize"]], (label, j)
    zf, infos = _zipfile_view(z)
    bad = []
    for j, info in enumerate(infos):
        try:
            if len(zf.read(info)) != info.file_size:         # (zipfile hands out fewer bytes than the directory names without a word)
                bad.append(j)
        except Exception:                                    # (BadZipFile, zlib.error, NotImplementedError, RuntimeError: encrypted)
            bad.append(j)
    if label.startswith(("csize + 1", "csize - 1")):
        assert bad in ([], [e])                              # zlib stops at the end of the final block, wherever csize says it is
    else:
        assert bad == [e], (label, bad)


@pytest.mark.parametrize("k", range(len(Z.file_damage_cases())), ids=[c[0] for c in Z.file_damage_cases()])
def test_zipfile_rejects_the_file_the_rule_rejects(k):
    label, z, want, kept = Z.file_damage_cases()[k]
    ix, sts, flat = Z.read(z)
    assert (ix["status"], ix["nentries"]) == (want, kept) and sts == [Z.OK] * kept, (label, ix["status"], ix["nentries"], sts)
    if kept:                                                 # the entries in front of the stop are those of the sound file
        good = Z.read(Z.make_zip(Z.base_items()[:8]))
        assert Z.records(ix) == Z.records(good[0])[:kept] and flat == good[2][:len(flat)]
    if label in ("an entry count one too few", "an entry count one too many"):
        return                                               # (zipfile walks the directory by its size and does not count)
    try:
        rejected = zipfile.ZipFile(io.BytesIO(z)).testzip() is not None
    except Exception:                                        # (BadZipFile)
        rejected = True
    assert rejected, "zipfile accepts " + label


def test_entry_cap_and_the_sizing_call():
    z = Z.make_zip(Z.base_items())
    full = Z.index(z)
    for cap in (0, 8):
        ix = Z.index(z, entry_cap=cap)
        assert ix["status"] == Z.E_OUT_CAPACITY and (ix["nentries"], ix["total_out"]) == (9, full["total_out"])
    assert Z.index(z, entry_cap=9)["status"] == Z.OK
