"""GPU (-m gpu): the four calls of include/hdlz_bgzf.h inside the guard bands of tests/guards.py, as tests/test_gpu_containment.py runs
the older ones: every buffer carved out of one patterned arena, on the pattern and on its complement -- no byte outside the stated
"writes" changes, the scratch stays inside work_bytes, and the results do not depend on the initial contents of the outputs and the
scratch, nor on the bytes around the inputs."""
import zlib

import numpy as np
import pytest
import torch

import bgzf_ref
import guards
from bgzf_ref import OK, E_OUT_CAPACITY, E_BAD_PARAM, E_BAD_CHECKSUM, EOF, member
from hdl_deflate_amd import _lib
from hdl_deflate_amd.constants import out_bound

pytestmark = pytest.mark.gpu

BAND = 1 << 16
SALTS = (0x3C, 0x3C ^ 0xFF)


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def u8(a, dtype):
    return np.array(a, dtype).view(np.uint8)


def two_runs(specs, fills, call, keep):
    """the call on the pattern and on its complement -> (the last arena, bytes untouched in both runs, the kept regions of each run)"""
    clean, runs = None, []
    for salt in SALTS:
        a = guards.Arena(guards.Arena.size_for(specs), "cuda", salt)
        for s in specs:
            a.carve(*s)
        for name, data in fills.items():
            a.fill(name, data)
        call(a)
        torch.cuda.synchronize()
        u = a.untouched_flat()
        clean = u if clean is None else clean & u
        runs.append({n: a.view(n).cpu().numpy().copy() for n in keep})
    return a, clean, runs


@pytest.mark.parametrize("ragged", [True, False])
def test_crc32_batch_inside_guard_bands(engine, ragged):
    L = engine.lib
    lens = [0, 1, 127, 32769, 5, 70001, 32768] if ragged else [4099] * 5
    pitch = 0 if ragged else 4101
    n = sum(lens) if ragged else pitch * len(lens) - 2                # (the last row ends where its block ends)
    data = np.random.default_rng(3).integers(0, 256, n, dtype=np.uint8)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64) + 77
    B = len(lens)
    specs = [("data", n, 16, BAND, True, 5), ("off", 8 * (B + 1), 8, BAND, True), ("crc", 4 * B, 4, BAND)]

    def call(a):
        rc = L.hdlz_crc32_batch_ws(a.ptr("data"), a.ptr("off") if ragged else None, pitch, 0 if ragged else 4099, B, a.ptr("crc"), stream_ptr())
        assert rc == 0, L.hdlz_last_error()
    a, clean, runs = two_runs(specs, {"data": data, "off": offs.view(np.uint8)}, call, ["crc"])
    hb = data.tobytes()
    want = [zlib.crc32(hb[x - 77:y - 77]) for x, y in zip(offs, offs[1:])] if ragged else [zlib.crc32(hb[b * pitch:b * pitch + 4099]) for b in range(B)]
    for r in runs:
        assert list(r["crc"].view(np.uint32)) == want
    assert guards.violations(a, clean, {"crc": True}) == []
    assert not bool(a.split(clean)["crc"][1].any())


@pytest.mark.parametrize("B, short", [(257, 0), (257, 1), (3, 0), (3, 29)])
def test_join_inside_guard_bands(engine, oracle, B, short):
    L = engine.lib
    r = np.random.default_rng(B)
    pool = bgzf_ref.data(4096, B)
    blocks = [pool[a:a + n] for a, n in zip(r.integers(0, 3800, B), r.integers(5, 201, B))]
    rows = []
    for b in blocks:
        rc, z = oracle.compress(b, 32, 10)
        assert rc == 0
        rows.append(z)
    want, offs = bgzf_ref.framed_rows(rows, blocks)
    pitch = (out_bound(200) + 3) & ~3
    cap = len(want) - short
    wb = L.hdlz_bgzf_join_work_bytes(B)
    specs = [("rows", B * pitch, 4, BAND, True), ("len", 4 * B, 4, BAND, True), ("status", 4 * B, 4, BAND, True), ("in_off", 8 * (B + 1), 8, BAND, True),
             ("crc", 4 * B, 4, BAND, True), ("file", cap, 16, BAND, False, 5), ("off", 8 * (B + 1), 8, BAND), ("result", 16, 8, BAND),
             ("work", wb, 8, BAND)]
    # (the rows' slack keeps the pattern: only what lies below d_len[b] is the call's to read)
    fills = {"len": u8([len(z) for z in rows], np.uint32), "status": u8([0] * B, np.uint32),
             "in_off": u8(np.concatenate([[0], np.cumsum([len(b) for b in blocks])]), np.int64), "crc": u8([zlib.crc32(b) for b in blocks], np.uint32)}

    def call(a):
        for b, z in enumerate(rows):
            a.fill("rows", z, at=b * pitch)
        rc = L.hdlz_bgzf_join_ws(a.ptr("rows"), pitch, a.ptr("len"), a.ptr("status"), a.ptr("in_off"), 200, B, a.ptr("crc"), a.ptr("file"), cap,
                                 a.ptr("off"), a.ptr("result"), a.ptr("work"), wb, stream_ptr())
        assert rc == 0, L.hdlz_last_error()
    a, clean, runs = two_runs(specs, fills, call, ["file", "off", "result"])
    written = np.zeros(cap, bool)                                      # the members that fit; the EOF member if all fits
    for b in range(B):
        if offs[b + 1] <= cap:
            written[offs[b]:offs[b + 1]] = True
    if not short:
        written[:] = True
    for run in runs:
        rec = _lib.BgzfJoinResult.from_buffer_copy(run["result"].tobytes())
        assert (rec.file_len, rec.status, rec.first_bad) == (len(want), E_OUT_CAPACITY if short else OK, 0xFFFFFFFF)
        assert list(run["off"].view(np.int64)) == offs
        assert np.array_equal(run["file"][written], np.frombuffer(want, np.uint8)[:cap][written])
    bad = guards.violations(a, clean, {"file": torch.from_numpy(written), "off": True, "result": True, "work": True})
    assert bad == [], bad
    parts = a.split(clean)
    assert not bool(parts["off"][1].any()) and not bool(parts["result"][1].any())


def some_file():
    """five windows: members of every block type, an empty one, a look-alike header in a stored payload"""
    parts = [bgzf_ref.data(n, n) for n in (65536, 100, 0, 65280, 30000, 65536, 7, 50000, 65536)]
    levels = (6, 1, 6, 0, 9, 1, 6, 0, 6)
    ms = [member(p, lv) for p, lv in zip(parts, levels)]
    fake = bytearray(parts[7])
    fake[20000:20018] = bgzf_ref.header(500)
    ms[7] = member(bytes(fake), 0)
    parts[7] = bytes(fake)
    return b"".join(ms) + EOF, b"".join(parts)


@pytest.mark.parametrize("cap_short", [0, 3])
def test_index_inside_guard_bands(engine, cap_short):
    L = engine.lib
    f, _ = some_file()
    w = bgzf_ref.walk(f)
    assert w.status == OK and len(f) > 3 * 65536
    cap = w.nmembers - cap_short
    wb = L.hdlz_bgzf_index_work_bytes(len(f))
    specs = [("file", len(f), 16, BAND, True, 3), ("off", 8 * (cap + 1), 8, BAND), ("out_off", 8 * (cap + 1), 8, BAND), ("result", 32, 8, BAND),
             ("work", wb, 8, BAND)]

    def call(a):
        rc = L.hdlz_bgzf_index_ws(a.ptr("file"), len(f), cap, a.ptr("off"), a.ptr("out_off"), a.ptr("result"), a.ptr("work"), wb, stream_ptr())
        assert rc == 0, L.hdlz_last_error()
    a, clean, runs = two_runs(specs, {"file": f}, call, ["off", "out_off", "result"])
    for run in runs:
        rec = _lib.BgzfIndexResult.from_buffer_copy(run["result"].tobytes())
        assert (rec.nmembers, rec.total_out, rec.file_used, rec.status, rec.eof_marker) == \
            (w.nmembers, w.total_out, w.file_used, E_OUT_CAPACITY if cap_short else OK, 0 if cap_short else 1)
        assert list(run["off"].view(np.int64)) == w.off[:cap + 1] and list(run["out_off"].view(np.int64)) == w.out_off[:cap + 1]
    assert guards.violations(a, clean, {"off": True, "out_off": True, "result": True, "work": True}) == []
    parts = a.split(clean)
    assert not bool(parts["off"][1].any()) and not bool(parts["out_off"][1].any()) and not bool(parts["result"][1].any())


@pytest.mark.parametrize("case", ["whole", "range", "short", "damaged"])
def test_inflate_inside_guard_bands(engine, case):
    L = engine.lib
    f, data = some_file()
    w = bgzf_ref.walk(f)
    b0, b1 = (2, 8) if case == "range" else (0, w.nmembers)
    off, out_off = w.off[b0:b1 + 1], w.out_off[b0:b1 + 1]
    B = b1 - b0
    total = out_off[-1] - out_off[0]
    cap = total - (1 if case == "short" else 0)
    if case == "damaged":
        f = f[:w.off[5] - 7] + bytes([f[w.off[5] - 7] ^ 0x80]) + f[w.off[5] - 6:]      # member 4's CRC
    wb = L.hdlz_bgzf_inflate_work_bytes(B, 0)
    specs = [("file", len(f), 16, BAND, True, 1), ("off", 8 * (B + 1), 8, BAND, True), ("out_off", 8 * (B + 1), 8, BAND, True),
             ("out", cap, 16, BAND, False, 3), ("member", 4 * B, 4, BAND), ("result", 24, 8, BAND), ("work", wb, 256, BAND)]

    def call(a):
        rc = L.hdlz_bgzf_inflate_ws(a.ptr("file"), len(f), a.ptr("off"), a.ptr("out_off"), B, 0, a.ptr("out"), cap, a.ptr("member"),
                                    a.ptr("result"), a.ptr("work"), wb, stream_ptr())
        assert rc == 0, L.hdlz_last_error()
    a, clean, runs = two_runs(specs, {"file": f, "off": u8(off, np.int64), "out_off": u8(out_off, np.int64)}, call, ["out", "member", "result"])
    for run in runs:
        rec = _lib.BgzfInflateResult.from_buffer_copy(run["result"].tobytes())
        members = list(run["member"].view(np.int32))
        if case == "short":                                           # the last data member's slot and the EOF member's end behind the capacity
            assert (rec.status, rec.first_bad, rec.out_len) == (E_BAD_PARAM, B - 2, 0) and members == [0] * (B - 2) + [E_BAD_PARAM] * 2
            assert run["out"][:out_off[B - 2]].tobytes() == data[:out_off[B - 2]]
        elif case == "damaged":
            assert (rec.status, rec.first_bad, rec.out_len) == (E_BAD_CHECKSUM, 4, 0) and members == [0] * 4 + [E_BAD_CHECKSUM] + [0] * (B - 5)
        else:
            assert (rec.status, rec.first_bad, rec.out_len) == (OK, (1 << 64) - 1, total) and not any(members)
            assert run["out"].tobytes() == data[out_off[0]:out_off[-1]]
    assert runs[0]["result"].tobytes() == runs[1]["result"].tobytes() and runs[0]["member"].tobytes() == runs[1]["member"].tobytes()
    bad = guards.violations(a, clean, {"out": True, "member": True, "result": True, "work": True})
    assert bad == [], bad
    parts = a.split(clean)
    assert not bool(parts["member"][1].any()) and not bool(parts["result"][1].any())
    if case in ("whole", "range"):
        assert not bool(parts["out"][1].any())
