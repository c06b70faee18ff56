"""CPU: the C-ABI library loads, exports every symbol include/hdlz.h declares, and refuses to
compute without a GPU (there is no CPU fallback in the product)."""
import ctypes
import os
import re

from conftest import REPO
from cabi_common import declarations, header


def _header():
    return re.sub(r"/\*.*?\*/", "", header("hdlz.h"), flags=re.S)


def _declared():
    return sorted(set(re.findall(r"\b(hdlz_[a-z_0-9]+)\s*\(", _header())))


def test_library_exports_every_declared_symbol():
    from hdl_deflate_amd import _lib
    names = _declared()
    assert set(names) == set(_lib.EXPORTS)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(L, n), n


def test_signature_table_matches_the_header():
    """every entry point has a restype and an argtypes list as long as its declaration's parameter list ((void) = 0), and load()
    puts exactly those on the library's functions"""
    from hdl_deflate_amd import _lib
    params = declarations(_header())
    assert len(params) == 22 and sorted(params) == sorted(_lib.EXPORTS) == sorted(_lib.SIGNATURES)
    assert sorted(set(params.values())) == [0, 1, 2, 5, 7, 8, 10, 11, 12, 13, 14, 16]
    L = _lib.load()
    for name in _lib.EXPORTS:
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is not None and isinstance(argtypes, list) and len(argtypes) == params[name], name
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    for name in ("hdlz_version", "hdlz_last_error", "hdlz_device_count", "hdlz_release_scratch"):
        assert params[name] == 0 and _lib.SIGNATURES[name][1] == []


def _struct_members(name):
    """[(member, array length or None)] and the byte size of `typedef struct <name> { ... }` (uint32_t / uint8_t members; one line
    may declare several: `uint32_t nlen, ndist;`)"""
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), _header(), flags=re.S).group(1)
    members, size = [], 0
    for ctype, decls in re.findall(r"\b(uint32_t|uint8_t)\s+([^;]+);", body):
        for d in decls.split(","):
            m = re.fullmatch(r"\s*(\w+)\s*(?:\[(\d+)\])?\s*", d)
            members.append((m.group(1), int(m.group(2)) if m.group(2) else None))
            size += (4 if ctype == "uint32_t" else 1) * int(m.group(2) or 1)
    return members, size


def test_state_structs_mirror_the_header():
    """CState / IState: the header's member names in the header's order, arrays of the header's lengths, 64 and 384 bytes (the sizes
    the header's comments state) -- the sessions read the state by these names"""
    from hdl_deflate_amd import _lib
    for cls, name, size in ((_lib.CState, "hdlz_cstate", 64), (_lib.IState, "hdlz_istate", 384)):
        members, hsize = _struct_members(name)
        assert [f[0] for f in cls._fields_] == [m[0] for m in members], name
        assert [getattr(f[1], "_length_", None) for f in cls._fields_] == [m[1] for m in members], name
        assert ctypes.sizeof(cls) == hsize == size, name
    assert [m for m in _struct_members("hdlz_cstate")[0] if m[1]] == [("reserved", 5)]
    assert [m for m in _struct_members("hdlz_istate")[0] if m[1]] == [("reserved", 4), ("lengths", 320)]
    assert _lib.IState.status.offset == 40 and _lib.CState.status.offset == 40 and _lib.IState.lengths.offset == 64


def test_version_bound_and_strings():
    from hdl_deflate_amd import _lib, out_bound
    L = _lib.load()
    assert L.hdlz_version() == 0x000600
    for n in (0, 5, 256, 2048, 65536, 1 << 24):
        assert L.hdlz_out_bound(n) == out_bound(n) == 6 + (9 * n + 10 + 7) // 8
    assert L.hdlz_status_string(0) == b"OK" and b"SHORT" in L.hdlz_status_string(1)


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        return
    from hdl_deflate_amd import _lib, E_HIP, E_BAD_PARAM
    import hdl_deflate_amd
    L = _lib.load()
    assert L.hdlz_device_count() == 0
    buf = (ctypes.c_uint8 * 64)()
    rc = L.hdlz_compress_batch(buf, None, 64, 64, 1, 32, 10, buf, 64, buf, buf, None)
    assert rc == E_HIP and b"no CPU path" in L.hdlz_last_error() or rc == E_HIP
    assert L.hdlz_compress_batch(buf, None, 64, 64, 1, 999, 10, buf, 64, buf, buf, None) == E_BAD_PARAM
    assert L.hdlz_inflate_batch(buf, None, 64, 64, 1, 0, 0, buf, 64, buf, buf, None) == E_HIP
    # hdlz_archive_batch: parameter checks come before the device is looked at; with good parameters: no device, no CPU path
    off = (ctypes.c_uint64 * 4)()
    assert L.hdlz_archive_batch(buf, 64, buf, 1 << 31, buf, 64, off, None) == E_BAD_PARAM and b"2^31" in L.hdlz_last_error()
    assert L.hdlz_archive_batch(buf, 64, buf, 1, buf, 64, None, None) == E_BAD_PARAM
    assert L.hdlz_archive_batch(buf, 64, buf, 1, buf, 64, off, None) == E_HIP
    # the entry points with caller-owned scratch: sizes are host arithmetic (no device needed), the calls have no CPU path either
    assert L.hdlz_archive_work_bytes(0) == 0 and L.hdlz_archive_work_bytes(1) >= 16 and L.hdlz_archive_work_bytes(1 << 20) >= 8 * 4096
    assert L.hdlz_archive_batch_ws(buf, 64, buf, 1, buf, 64, off, None, 0, None) == E_BAD_PARAM and b"hdlz_archive_work_bytes" in L.hdlz_last_error()
    assert L.hdlz_archive_batch_ws(buf, 64, buf, 1, buf, 64, off, buf, 4096, None) == E_HIP
    assert L.hdlz_inflate_work_bytes(0, 0, 0, 0, 0) == 0
    lanes = L.hdlz_inflate_work_bytes(1 << 20, 0, 2048, 0, 1)             # ragged lane mapping: the ordered lists, ~8 bytes per stream
    assert 8 << 20 <= lanes <= 9 << 20
    one = L.hdlz_inflate_work_bytes(1, 1 << 24, 1 << 26, 0, 0)            # ONE 16 MiB stream: the whole-GPU path's markers and lists
    assert one >= 1 << 26 and L.hdlz_inflate_work_bytes(1, 1 << 24, 1 << 26, 2, 0) < 1 << 16      # (a mapping hint keeps the batch kernels)
    assert L.hdlz_inflate_work_bytes(4096, 1 << 20, 1 << 22, 0, 0) <= (8 << 30) + (1 << 20)         # a batch: bounded by the 8 GiB budget
    assert L.hdlz_inflate_batch_ws(buf, None, 64, 64, 1, 0, 0, buf, 64, buf, buf, None, 0, None) == E_HIP
    assert L.hdlz_inflate_batch_ws(buf, None, 64, 64, 1, 16, 0, buf, 64, buf, buf, None, 0, None) == E_BAD_PARAM      # flags 16 / 32 left with round 6
    try:
        hdl_deflate_amd.Engine()
    except RuntimeError as e:
        assert "no CPU fallback" in str(e)
    else:
        raise AssertionError("Engine() must fail loudly without a GPU")


def test_product_never_imports_oracle():
    """only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline may touch oracle/"""
    pkg = os.path.join(REPO, "hdl_deflate_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", ".sh")):
                txt = open(os.path.join(root, f), errors="ignore").read()
                assert "oracle" not in txt.lower(), (root, f)


def test_tile_phases_have_one_source():
    """match search / extension / parse / token bits / bit scatter live ONCE, in hdlz_compress_common.h; the three
    compress kernels only call them (round 1 had the text three times, one copy generated)"""
    csrc = os.path.join(REPO, "hdl_deflate_amd", "csrc")
    common = open(os.path.join(csrc, "hdlz_compress_common.h")).read()
    for fn in ("match_search", "make_tokens", "run_transfer", "chain_skips", "token_codes", "scatter_codes", "adler_run"):
        assert common.count("void %s(" % fn) + common.count("uint32_t %s(" % fn) + common.count("uint64_t %s(" % fn) == 1, fn
    for f in ("hdlz_compress.hip", "hdlz_compress_small.hip", "hdlz_compress_stream.hip"):
        txt = open(os.path.join(csrc, f)).read()
        assert "match_search<" in txt and "make_tokens<" in txt and "run_transfer(" in txt, f
        assert "umin3(m[i]" not in txt and "v_lshl_add_u32" not in txt, f      # no pasted phase bodies
    assert not os.path.exists(os.path.join(REPO, "tools", "gen_stream_kernel.py"))
    # what stands around the phases has one source as well: the R1 header, the scratch layout of the stream passes, the window rule
    five = {f: open(os.path.join(csrc, f)).read() for f in ("hdlz_compress.hip", "hdlz_compress_small.hip", "hdlz_compress_stream.hip",
                                                            "hdlz_compress_chunk.hip", "hdlz_compress_common.h")}
    assert sum(t.count("0x9Cu") for t in five.values()) == 1 and common.count("HEADER_WORD = 0x78u | (0x9Cu << 8)") == 1
    body = re.search(r"size_t stream_work_bytes\([^)]*\)\s*\{(.*?)\n?\}", five["hdlz_compress_stream.hip"], flags=re.S).group(1)
    assert "stream_layout(" in body and not re.search(r"[*+]|\d\d", body), body       # no per-array arithmetic of its own
    assert five["hdlz_compress_stream.hip"].count("stream_layout(") == 3              # the definition, the size query, the launcher
    compares = r"cwindow\s*(?:<=|>=|==|!=|<|>)\s*(?:32|64|256)\b"
    helper = re.search(r"inline void window_case\(.*?inline void with_window\(.*?\n\}\n", common, flags=re.S).group(0)
    assert len(re.findall(compares, helper)) == 3                                      # <= 32, <= 64, == 32 * NCH
    for f, t in five.items():
        code = re.sub(r"//[^\n]*", "", t.replace(helper, ""))
        assert not re.search(compares, code), (f, re.search(compares, code).group(0))
        assert f == "hdlz_compress_common.h" or "with_window(" in code, f
    assert "SMALL_LAUNCH" not in five["hdlz_compress_small.hip"] and "SMALL_BY_NCH" not in five["hdlz_compress_small.hip"]


def test_stream_scratch_size_is_the_closed_form():
    """hdlz_streams_work_bytes is host arithmetic (no device needed) and callers size buffers by it: for nt = ceil(n / 2048) * nblocks
    tiles and nc = ceil(nt / 256) chunks it stays nt * 32 + nc * 40 + 64 + nblocks * 8 + nt * 2368 -- the value it had when the formula
    and the carve were two texts -- at the tile counts around a chunk (255, 256, 257), at one tile and at 4097; and it refuses
    (returns 0) no blocks, a block of 2^31 bytes and 2^31 tiles"""
    from hdl_deflate_amd import _lib
    L = _lib.load()

    def closed(n, nblocks):
        nt = (n + 2047) // 2048 * nblocks
        nc = (nt + 255) // 256
        return nt * 32 + nc * 40 + 64 + nblocks * 8 + nt * 2368

    seen = set()
    for tiles in (1, 255, 256, 257, 4097):
        for n in ((tiles - 1) * 2048 + 1, tiles * 2048 - 1, tiles * 2048):
            for nblocks in (1, 3, 37):
                assert L.hdlz_streams_work_bytes(n, nblocks) == closed(n, nblocks), (n, nblocks)
                seen.add((n + 2047) // 2048 * nblocks)
            assert L.hdlz_stream_work_bytes(n) == L.hdlz_streams_work_bytes(n, 1) == closed(n, 1), n
    assert {1, 255, 256, 257, 4097} <= seen
    assert L.hdlz_streams_work_bytes(0, 5) == closed(0, 5) == 64 + 40                # (no tiles: the totals alone)
    assert L.hdlz_streams_work_bytes(2048, 0) == 0 and L.hdlz_streams_work_bytes(2048, 1 << 32) == 0
    assert L.hdlz_streams_work_bytes(1 << 31, 1) == 0 and L.hdlz_stream_work_bytes(1 << 31) == 0
    assert L.hdlz_streams_work_bytes((1 << 31) - 1, 1) == closed((1 << 31) - 1, 1)
    assert L.hdlz_streams_work_bytes((1 << 31) - 1, 2047) == closed((1 << 31) - 1, 2047)      # 2^31 - 2^20 tiles
    assert L.hdlz_streams_work_bytes((1 << 31) - 1, 2048) == 0 and L.hdlz_streams_work_bytes(2048, 1 << 31) == 0      # 2^31 tiles


def test_inflate_group_decode_has_one_source():
    """the fast path's group decode of the lane kernel (up to three literals + the match behind them, fixed blocks) lives ONCE -- the
    TOK_FIXED_GROUP text of hdlz_inflate_tok.hip, used by both decode steps of a round --, the kernel file is not included twice
    anywhere, and it keeps few preprocessor switches"""
    csrc = os.path.join(REPO, "hdl_deflate_amd", "csrc")
    txt = open(os.path.join(csrc, "hdlz_inflate_tok.hip")).read()
    assert txt.count("#define TOK_FIXED_GROUP(") == 1 and txt.count("TOK_FIXED_GROUP(false,") == 1 and txt.count("TOK_FIXED_GROUP(true,") == 1
    # the distance look-up behind a length: the group decode once (the DYN fast path has its own, x_decode), and the serial path once --
    # its text is hdlz_inflate_rules.h's, which asks this kernel's TOK_DIST_CODE step for the look-up
    rules = open(os.path.join(csrc, "hdlz_inflate_rules.h")).read()
    assert txt.count("dst_at((uint32_t)") == 1 and txt.count("dst_at((bits)") == 1 and txt.count("#define TOK_DIST_CODE(") == 1
    assert rules.count("K##_DIST_CODE((uint32_t)bb") == 1 and txt.count("HDLZ_SERIAL_ITEMS(TOK)") == 1
    assert sum(1 for ln in txt.splitlines() if ln.startswith("#if")) <= 5
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".h")):
            assert '#include "hdlz_inflate_tok.hip"' not in open(os.path.join(csrc, f)).read(), f


def test_inflate_rules_have_one_source():
    """the deflate block rules the five inflate decoders apply -- the order of the code-length code, where a stored LEN sits, the mask on
    it, the two end-of-input margins, the input load -- are stated ONCE, in hdlz_inflate_rules.h, which all five include; a decoder that
    pastes one back (the last rule fix had to be made three times) is named here"""
    csrc = os.path.join(REPO, "hdl_deflate_amd", "csrc")
    rules = "hdlz_inflate_rules.h"
    code = {f: re.sub(r"/\*.*?\*/", "", re.sub(r"//[^\n]*", "", open(os.path.join(csrc, f)).read()), flags=re.S)
            for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))}

    def sites(pattern):
        return [f for f, t in code.items() for _ in re.findall(pattern, t)]

    for what, pattern, where in (("the order table's initialiser", r"16,\s*17,\s*18,\s*0,\s*8", [rules]),
                                 ("stored_len_skip", r"skip <= 2u", [rules]),
                                 ("stored_len_mask", r"__builtin_clz\((?:a\.)?obsize\)", [rules]),
                                 ("no_eof_behind_code", r"isize - 3", [rules]), ("copy_hold", r"isize - 2", [rules]),
                                 ("the wave decoder's own load", r"dload32", [])):
        assert sites(pattern) == where, "%s (%s) stands in %s" % (what, pattern, sites(pattern))
    for f in ("hdlz_inflate_tok.hip", "hdlz_inflate_grp.hip", "hdlz_inflate_dyn.hip", "hdlz_inflate_par.hip", "hdlz_inflate_any.hip"):
        assert '#include "%s"' % rules in code[f], f
