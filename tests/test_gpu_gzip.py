"""GPU (-m gpu): the joined stream as one gzip member (include/hdlz_gzip.h) -- hdlz_crc32_ws against zlib.crc32, hdlz_join_gzip_ws
bit-exact against gzip_ref.expected_gzip (the CPU oracle's per-block streams and stock zlib only) and read by Python's gzip,
hdlz_unjoin_gzip_ws with every kind of damage to the frame, all three inside guard bands and in one HIP graph, and the Engine's
container="gzip"."""
import gzip
import random
import zlib

import numpy as np
import pytest
import torch

import guards
import gzip_ref
from hdl_deflate_amd import _lib
from hdl_deflate_amd.constants import out_bound
from hdl_deflate_amd.data import family_bytes
from gzip_calls import ZlibCall, ragged_blocks, round4, blocks_of, offsets_of, flipped

pytestmark = pytest.mark.gpu

OK, E_SHORT_INPUT, E_OUT_CAPACITY, E_NO_EOF, E_BAD_PARAM, E_BAD_HEADER, E_BAD_CHECKSUM = 0, 1, 2, 5, 8, 11, 12
LANE, WAVE, GROUP = 2, 4, 64
HINTS = (0, LANE, WAVE, GROUP)
NOBODY = (1 << 64) - 1
TILE = 32768


def dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype)).cuda()


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


# ---- hdlz_crc32_ws
SMALL = list(range(81)) + [255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 32767, 32768, 32769,
                           65535, 65536, 65537, 3 * TILE, 5 * TILE + 17]
LARGE = [257 * TILE + 7, 513 * TILE + 7, 1000 * TILE + 7]
_host = {}


def host_data(kind):
    """1000 tiles and a bit of: random bytes, zeros (where length handling goes wrong: only the length speaks), FF"""
    if kind not in _host:
        n = LARGE[-1] + 64
        _host[kind] = (np.random.default_rng(31).integers(0, 256, n, dtype=np.uint8) if kind == "random" else
                       np.full(n, 0 if kind == "zeros" else 255, np.uint8))
    return _host[kind]


def device_crcs(L, d_buf, cases):
    """hdlz_crc32_ws of d_buf[a : a + n] for every (a, n): junk in the result words and in the scratch beforehand, one sync"""
    words = torch.full((len(cases),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    wb = max(L.hdlz_crc32_work_bytes(n) for _, n in cases)
    work = torch.full((max(wb, 4) // 4,), -1, dtype=torch.int32, device="cuda")
    for k, (a, n) in enumerate(cases):
        need = L.hdlz_crc32_work_bytes(n)
        rc = L.hdlz_crc32_ws(d_buf.data_ptr() + a, n, words.data_ptr() + 4 * k, work.data_ptr() if need else None, need, stream_ptr())
        assert rc == 0, L.hdlz_last_error()
    torch.cuda.synchronize()
    return [int(w) & 0xFFFFFFFF for w in words.cpu().numpy()]


@pytest.mark.parametrize("kind", ["random", "zeros", "ff"])
def test_crc32_against_zlib(engine, kind):
    """every length 0 .. 80, the lengths around a strip, a wave's share and a tile, whole tiles, and 257 / 513 / 1000 tiles plus 7 bytes:
    one tile a workgroup and one word a thread of the finishing workgroup (the second tile of a workgroup, from 1025 tiles on, and the
    second Horner step, from 1024 tiles on: tests/test_gpu_second_trips.py); base pointers 0, 1, 4 and 15 bytes off a 16-byte boundary.
    The slices lie inside one larger buffer: a load in front of the data or behind it would change the random case."""
    h = host_data(kind)
    d = dev(h)
    assert d.data_ptr() % 16 == 0
    cases = [(16 + a, n) for a in (0, 1, 4, 15) for n in SMALL] + [(16 + a, n) for a, n in zip((0, 1, 15), LARGE)]
    got = device_crcs(engine.lib, d, cases)
    hb = h.tobytes()
    bad = [(a - 16, n, hex(g)) for (a, n), g in zip(cases, got) if g != zlib.crc32(hb[a:a + n])]
    assert bad == [], bad[:8]


def test_crc32_pinned_values(engine):
    pins = [(b"123456789", 0xCBF43926), (bytes(32768), 0x011FFCA6), (b"\xff" * 65536, 0xDEAB7E4E),
            (bytes((7 * p + 3) & 255 for p in range(70001)), 0x5C5C297A), (b"", 0)]
    for data, want in pins:
        d = dev(np.frombuffer(data + b"x", np.uint8))
        assert device_crcs(engine.lib, d, [(0, len(data))]) == [want] == [zlib.crc32(data)]
        t = engine.crc32(d[:len(data)])
        assert t.dtype == torch.uint32 and t.numel() == 1 and int(t.cpu().numpy()[0]) == want


@pytest.mark.parametrize("n, phase", [(0, 0), (1, 3), (5 * TILE + 17, 5), (64 * TILE, 0)])
def test_crc32_inside_guard_bands(engine, n, phase):
    """data, result word and scratch carved out of one patterned arena, on the pattern and on its complement: nothing but d_crc[0] and
    the scratch is written, and the result is the same -- it depends neither on the bytes around the data nor on what the scratch held"""
    L = engine.lib
    data = np.random.default_rng(n + 1).integers(0, 256, n, dtype=np.uint8)
    wb = L.hdlz_crc32_work_bytes(n)
    band = 1 << 16
    specs = [("data", n, 16, band, True, phase), ("crc", 4, 4, band), ("work", wb, 4, band)]
    clean, got = None, []
    for salt in (0x3C, 0x3C ^ 0xFF):
        a = guards.Arena(guards.Arena.size_for(specs), "cuda", salt)
        for s in specs:
            a.carve(*s)
        a.fill("data", data)
        rc = L.hdlz_crc32_ws(a.ptr("data") if n else None, n, a.ptr("crc"), a.ptr("work") if wb else None, wb, stream_ptr())
        assert rc == 0, L.hdlz_last_error()
        torch.cuda.synchronize()
        u = a.untouched_flat()
        clean = u if clean is None else clean & u
        got.append(int(a.view("crc").cpu().numpy().view(np.uint32)[0]))
    assert got == [zlib.crc32(data.tobytes())] * 2
    assert guards.violations(a, clean, {"crc": True, "work": True}) == []
    assert not bool(a.split(clean)["crc"][1].any())


# ---- hdlz_join_gzip_ws
class Call(ZlibCall):
    """the buffers of one CRC + compress + gzip join (test_gpu_joined.Call with the gzip call's capacity, record and CRC word)"""

    def __init__(self, engine, blocks, cap=None, **kw):
        ZlibCall.__init__(self, engine, blocks, **kw)
        nmax = max([len(b) for b in blocks] + [kw.get("bound", 0), 5])
        self.zcap = self.cap
        self.cap = self.L.hdlz_join_gzip_bound(self.B, nmax) if cap is None else cap
        self.stream = torch.zeros(max(self.cap, 1), dtype=torch.uint8, device="cuda")
        assert self.L.hdlz_join_gzip_work_bytes(self.B) == self.wb
        self.n = sum(len(b) for b in blocks)
        self.crc = torch.full((1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        self.crc_wb = self.L.hdlz_crc32_work_bytes(self.n)
        self.crc_work = torch.zeros(max(self.crc_wb, 4) // 4, dtype=torch.int32, device="cuda")

    def checksum(self):
        """(ragged input only: X is one flat buffer)"""
        assert self.in_off is not None
        rc = self.L.hdlz_crc32_ws(self.d_in.data_ptr(), self.n, self.crc.data_ptr(), self.crc_work.data_ptr() if self.crc_wb else None,
                                  self.crc_wb, stream_ptr())
        assert rc == 0, self.L.hdlz_last_error()

    def join(self):
        rc = self.L.hdlz_join_gzip_ws(self.rows.data_ptr(), self.pitch, self.out_len.data_ptr(), self.end_bits.data_ptr(),
                                      self.status.data_ptr(), self.in_off.data_ptr() if self.in_off is not None else None, self.in_len,
                                      self.B, self.crc.data_ptr(), self.stream.data_ptr(), self.cap, self.off.data_ptr(),
                                      self.result.data_ptr(), self.work.data_ptr() if self.wb else None, self.wb, stream_ptr())
        assert rc == 0, self.L.hdlz_last_error()

    def join_zlib(self):
        """hdlz_join_batch_ws of the same rows -> (stream bytes, offsets)"""
        z = torch.zeros(max(self.zcap, 1), dtype=torch.uint8, device="cuda")
        off, res = torch.zeros_like(self.off), torch.zeros_like(self.result)
        rc = self.L.hdlz_join_batch_ws(self.rows.data_ptr(), self.pitch, self.out_len.data_ptr(), self.end_bits.data_ptr(),
                                       self.status.data_ptr(), self.in_off.data_ptr() if self.in_off is not None else None, self.in_len,
                                       self.B, z.data_ptr(), self.zcap, off.data_ptr(), res.data_ptr(),
                                       self.work.data_ptr() if self.wb else None, self.wb, stream_ptr())
        assert rc == 0, self.L.hdlz_last_error()
        torch.cuda.synchronize()
        r = _lib.JoinResult.from_buffer_copy(res.cpu().numpy().tobytes())
        assert r.status == OK
        return z[:r.stream_len].cpu().numpy().tobytes(), list(off.cpu().numpy())

    def record(self):
        torch.cuda.synchronize()
        r = _lib.JoinGzipResult.from_buffer_copy(self.result.cpu().numpy().tobytes())
        return r.stream_len, r.status, r.crc


def check(label, c, blocks, want=None):
    g = want or gzip_ref.expected_gzip(blocks, c.cw, c.mm)
    slen, st, crc = c.record()
    assert (slen, st, crc) == (len(g.stream), OK, g.crc), (label, slen, st, hex(crc), len(g.stream), hex(g.crc))
    assert list(c.off.cpu().numpy()) == g.offsets, (label, "offsets")
    z = c.stream[:slen].cpu().numpy().tobytes()
    assert z == g.stream, (label, "stream", next(k for k in range(len(z)) if z[k] != g.stream[k]))
    assert gzip.decompress(z) == g.data, label
    d = zlib.decompressobj(31)
    assert d.decompress(z) == g.data and d.eof and d.unused_data == b""
    return g


def run(engine, blocks, **kw):
    c = Call(engine, blocks, **kw)
    if c.in_off is not None:
        c.checksum()
    else:                                                   # a pitched batch: X is not one buffer, the word comes from elsewhere
        c.crc.copy_(dev([zlib.crc32(b"".join(blocks))], np.uint32).view(torch.int32))
    c.compress()
    c.join()
    return c


@pytest.mark.parametrize("B", [0, 1, 2, 255, 256, 257, 513])
def test_block_counts_at_the_tile_edges_of_the_look_back(engine, B):
    blocks = ragged_blocks(B, 5, 64, seed=B)
    c = run(engine, blocks, bound=64)
    g = check(("count", B), c, blocks)
    zs, zoff = c.join_zlib()                                # the members are those of the zlib join of the same rows
    assert zs == g.zlib_form.stream and zoff == g.zlib_form.offsets
    z = c.stream.cpu().numpy().tobytes()
    assert z[10:g.offsets[B]] == zs[2:zoff[B]] and [o - 8 for o in g.offsets] == zoff
    if B == 0:
        assert z[:20] == bytes.fromhex("1f8b0800" "00000000" "00ff" "0300" "00000000" "00000000") and c.record()[0] == 20


def test_sizes_around_the_compress_tile(engine):
    def five(n, seed):
        big = b"".join(family_bytes(1 + (seed + k) % 4, 4200, seed=seed + k) for k in range(5))
        return [big[k * 4200:k * 4200 + n] for k in range(5)]
    for n in (2047, 2048, 2049, 4113):
        blocks = five(n, n)
        check(("fixed", n), run(engine, blocks, fixed=(n, (n + 15) // 16 * 16)), blocks)
    blocks = [five(n, 3 * n)[k] for k, n in enumerate((2049, 2047, 4113, 2048, 2047))]
    for bound in (0, 4113):
        check(("mix", bound), run(engine, blocks, bound=bound), blocks)


@pytest.mark.parametrize("cw,mm", [(32, 10), (33, 10), (256, 10), (32, 5)])
def test_windows(engine, cw, mm):
    blocks = ragged_blocks(70, 5, 300, seed=cw + mm) + ragged_blocks(8, 900, 1024, seed=cw)
    check(("window", cw, mm), run(engine, blocks, cw=cw, mm=mm, bound=1024), blocks)


def test_failed_block_and_short_capacity(engine):
    """as the zlib join behaves (test_gpu_joined): the worst status and an empty record; E_OUT_CAPACITY with the length and the CRC
    still reported, the index whole, the members that end inside the capacity in place"""
    blocks = ragged_blocks(40, 5, 64, seed=77)
    bad = blocks[:20] + [b"abcd"] + blocks[20:]
    c = run(engine, bad, bound=64)
    assert c.record() == (0, E_SHORT_INPUT, 0)
    g = gzip_ref.expected_gzip(blocks, 32, 10)
    for cap in (len(g.stream) - 1, len(g.stream) - 10, 15, 9, 7, 0):
        c = Call(engine, blocks, bound=64, cap=cap)
        c.stream = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        c.checksum()
        c.compress()
        c.join()
        assert c.record() == (len(g.stream), E_OUT_CAPACITY, g.crc), (cap, c.record())
        assert list(c.off.cpu().numpy()) == g.offsets
        z = c.stream.cpu().numpy().tobytes()
        fits = max([o for o in g.offsets if o <= cap] + [10 if cap >= 10 else 0])
        assert z[:fits] == g.stream[:fits], cap
        assert z[cap:] == b"\xa5" * 64, cap                            # never a byte at or behind stream_cap


@pytest.mark.parametrize("B,short", [(257, 0), (257, 1), (3, 0), (3, 11)])
def test_join_inside_guard_bands(engine, B, short):
    """test_gpu_joined's containment test for the gzip call: every buffer carved out of one patterned arena, stream_cap exact and short,
    on the pattern and on its complement -- no byte outside the stated "writes" changes, and the results are identical"""
    L = engine.lib
    blocks = ragged_blocks(B, 5, 200, seed=100 + B)
    g = gzip_ref.expected_gzip(blocks, 32, 10)
    pitch = round4(out_bound(200))
    cap = len(g.stream) - short
    wb = L.hdlz_join_gzip_work_bytes(B)
    off = np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).astype(np.int64)
    band = 1 << 16
    specs = [("rows", B * pitch, 4, band, True), ("len", 4 * B, 4, band, True), ("bits", 8 * B, 8, band, True), ("status", 4 * B, 4, band, True),
             ("in_off", 8 * (B + 1), 8, band, True), ("crc", 4, 4, band, True), ("stream", cap, 16, band, False, 5), ("off", 8 * (B + 1), 8, band),
             ("result", 16, 8, band), ("work", wb, 8, band)]
    clean, runs = None, []
    for salt in (0x3C, 0x3C ^ 0xFF):
        a = guards.Arena(guards.Arena.size_for(specs), "cuda", salt)
        for s in specs:
            a.carve(*s)
        for b, z in enumerate(g.rows):
            a.fill("rows", z, at=b * pitch)
        a.fill("len", np.array([len(z) for z in g.rows], np.uint32).view(np.uint8))
        a.fill("bits", np.array(g.end_bits, np.uint64).view(np.uint8))
        a.fill("status", np.zeros(B, np.uint32).view(np.uint8))
        a.fill("in_off", off.view(np.uint8))
        a.fill("crc", np.array([g.crc], np.uint32).view(np.uint8))
        rc = L.hdlz_join_gzip_ws(a.ptr("rows"), pitch, a.ptr("len"), a.ptr("bits"), a.ptr("status"), a.ptr("in_off"), 200, B, a.ptr("crc"),
                                 a.ptr("stream"), cap, a.ptr("off"), a.ptr("result"), a.ptr("work"), wb, stream_ptr())
        assert rc == 0, L.hdlz_last_error()
        torch.cuda.synchronize()
        u = a.untouched_flat()
        clean = u if clean is None else clean & u
        runs.append({n: a.view(n).cpu().numpy().copy() for n in ("stream", "off", "result")})
    written = np.zeros(cap, bool)                                      # the header, the members that fit, the trailer if all fits
    written[:10] = True
    for b in range(B):
        if g.offsets[b + 1] <= cap:
            written[g.offsets[b]:g.offsets[b + 1]] = True
    if not short:
        written[:] = True
    for r in runs:
        rec = _lib.JoinGzipResult.from_buffer_copy(r["result"].tobytes())
        assert (rec.stream_len, rec.status, rec.crc) == (len(g.stream), E_OUT_CAPACITY if short else OK, g.crc)
        assert list(r["off"].view(np.int64)) == g.offsets
        assert np.array_equal(r["stream"][written], np.frombuffer(g.stream, np.uint8)[:cap][written])
    bad = guards.violations(a, clean, {"stream": torch.from_numpy(written), "off": True, "result": True, "work": True})
    assert bad == [], bad
    parts = a.split(clean)
    assert not bool(parts["off"][1].any()) and not bool(parts["result"][1].any())


# ---- hdlz_unjoin_gzip_ws
class Run(object):
    """one hdlz_unjoin_gzip_ws call: every output pre-filled with junk, then the record, the bytes and the member statuses"""

    def __init__(self, L, stream, off, out_off=None, out_len=0, out_cap=None, flags=0, stream_len=None, fill=0xA5):
        B = len(off) - 1
        if out_cap is None:
            out_cap = out_off[-1] if out_off is not None else B * out_len
        self.d_stream, self.d_off = dev(np.frombuffer(stream + bytes(8), np.uint8)), dev(off, np.int64)
        self.d_out_off = dev(out_off, np.int64) if out_off is not None else None
        self.out = torch.full((out_cap + 64,), fill, dtype=torch.uint8, device="cuda")
        self.member = torch.full((max(B, 1),), -1, dtype=torch.int32, device="cuda")
        self.result = torch.full((3,), -1, dtype=torch.int64, device="cuda")
        wb = L.hdlz_unjoin_gzip_work_bytes(B, out_cap, flags)
        self.work = torch.full((max(wb, 1),), fill ^ 0xFF, dtype=torch.uint8, device="cuda")
        rc = L.hdlz_unjoin_gzip_ws(self.d_stream.data_ptr(), len(stream) if stream_len is None else stream_len, self.d_off.data_ptr(),
                                   self.d_out_off.data_ptr() if out_off is not None else None, out_len, B, flags,
                                   self.out.data_ptr() if out_cap else None, out_cap, self.member.data_ptr(), self.result.data_ptr(),
                                   self.work.data_ptr() if wb else None, wb, stream_ptr())
        assert rc == 0, L.hdlz_last_error()
        torch.cuda.synchronize()
        self.rec = _lib.UnjoinGzipResult.from_buffer_copy(self.result.cpu().numpy().tobytes())
        self.members = list(self.member.cpu().numpy()[:B])
        self.out_cap, self.fill = out_cap, fill

    def bytes(self):
        return self.out[:self.rec.out_len].cpu().numpy().tobytes()

    def slack_untouched(self):
        return bool((self.out[self.out_cap:] == self.fill).all())


_base = {}


def damage_base():
    """72 ragged members, 43 KiB of output: two CRC tiles, the second short"""
    if not _base:
        r = random.Random(99)
        blocks = blocks_of([4 * r.randint(2, 300) for _ in range(71)] + [61], seed=5)
        _base["g"] = gzip_ref.expected_gzip(blocks, 32, 10)
        _base["out_off"] = offsets_of(blocks)
        assert len(_base["g"].data) > TILE
    return _base["g"], list(_base["out_off"])


@pytest.mark.parametrize("flags", HINTS)
def test_round_trip_under_every_mapping(engine, flags):
    g, oo = damage_base()
    r = Run(engine.lib, g.stream, g.offsets, oo, flags=flags)
    assert (r.rec.status, r.rec.first_bad, r.rec.out_len, r.rec.crc) == (OK, NOBODY, len(g.data), g.crc), (r.rec.status, r.rec.first_bad)
    assert r.bytes() == g.data and not any(r.members) and r.slack_untouched()
    blocks = blocks_of([2048] * 65, seed=2, distinct=24)               # uniform members, no offset array; 133120 bytes: five tiles
    u = gzip_ref.expected_gzip(blocks, 32, 10)
    r = Run(engine.lib, u.stream, u.offsets, None, 2048, flags=flags)
    assert (r.rec.status, r.rec.first_bad, r.rec.out_len, r.rec.crc) == (OK, NOBODY, len(u.data), u.crc)
    assert r.bytes() == u.data and r.slack_untouched()
    e = gzip_ref.expected_gzip([], 32, 10)                             # no members: the 20-byte stream
    r = Run(engine.lib, e.stream, e.offsets, [0], flags=flags)
    assert len(e.stream) == 20 and (r.rec.status, r.rec.first_bad, r.rec.out_len, r.rec.crc) == (OK, NOBODY, 0, 0)


_many = {}


@pytest.mark.parametrize("flags", [LANE, WAVE, GROUP])
def test_failed_members_beyond_the_first_wave_and_workgroup(engine, flags):
    """600 members of 5 to 64 bytes: the failing ones sit in other waves and other workgroups of the judge than member 0 -- the lowest
    one is reported"""
    if not _many:
        r = random.Random(600)
        blocks = blocks_of([4 * r.randint(2, 16) for _ in range(599)] + [5], seed=6)
        _many["g"], _many["oo"] = gzip_ref.expected_gzip(blocks, 32, 10), offsets_of(blocks)
    g, oo = _many["g"], _many["oo"]
    for bad in ((300, 570), (570,)):
        z = g.stream
        for k in bad:                                                                       # a member's FF FF -> FF FE
            assert z[g.offsets[k + 1] - 2:g.offsets[k + 1]] == b"\xff\xff"
            z = flipped(z, g.offsets[k + 1] - 1, 0x01)
        r = Run(engine.lib, z, g.offsets, oo, flags=flags)
        assert (r.rec.status, r.rec.first_bad, r.rec.out_len, r.rec.crc) == (E_NO_EOF, bad[0], 0, 0), (bad, r.rec.status, r.rec.first_bad)
        assert [(b, s) for b, s in enumerate(r.members) if s] == [(k, E_NO_EOF) for k in bad]


@pytest.mark.parametrize("flags", HINTS)
def test_damaged_frame(engine, flags):
    g, oo = damage_base()
    B, end, L = len(g.members), g.offsets[-1], engine.lib
    assert g.stream[end:end + 2] == b"\x03\x00" and len(g.stream) == end + 10

    def verdict(**kw):
        r = Run(L, kw.pop("stream", g.stream), kw.pop("off", g.offsets), oo, flags=flags, **kw)
        assert r.rec.out_len == 0 and r.rec.status != OK
        return r.rec.status, r.rec.first_bad
    for at in (0, 1, 2):                                                                    # the magic and CM
        assert verdict(stream=flipped(g.stream, at, 0x01)) == (E_BAD_HEADER, B), at
    for bit in (0x01, 0x02, 0x04, 0x08, 0x10, 0x80):                                        # FLG must be 0
        assert verdict(stream=flipped(g.stream, 3, bit)) == (E_BAD_HEADER, B), bit
    # d_off[0] != 10 with every member whole: one byte slipped in behind the header, the index moved with it
    moved = g.stream[:10] + b"\x00" + g.stream[10:]
    assert verdict(stream=moved, off=[o + 1 for o in g.offsets]) == (E_BAD_HEADER, B)
    r = Run(L, moved, [o + 1 for o in g.offsets], oo, flags=flags)
    assert not any(r.members)                                                               # ... only the frame's rule fired
    off = list(g.offsets)
    off[0] = 2                                                                              # the zlib form's index: member 0 starts in the header
    assert verdict(off=off) == (3, 0)                                                       # HDLZ_E_BAD_BTYPE: byte 2 is 08
    for at in range(4, 10):                                                                 # MTIME, XFL, OS are not looked at
        r = Run(L, flipped(g.stream, at, 0xFF), g.offsets, oo, flags=flags)
        assert (r.rec.status, r.rec.out_len) == (OK, len(g.data)), at
    for k in (0, 33, B - 1):                                                                # a member's marker: FF FF -> FF FE
        r = Run(L, flipped(g.stream, g.offsets[k + 1] - 1, 0x01), g.offsets, oo, flags=flags)
        assert (r.rec.status, r.rec.first_bad, r.rec.out_len, r.rec.crc) == (E_NO_EOF, k, 0, 0), (k, r.rec.status, r.rec.first_bad)
        assert [b for b, s in enumerate(r.members) if s] == [k]
    for at, xor in ((end, 0x01), (end, 0x04), (end + 1, 0x01)):                             # 03 00
        assert verdict(stream=flipped(g.stream, at, xor)) == (E_NO_EOF, B), at
    for at in range(end + 2, end + 10):                                                     # every byte of CRC-32 and ISIZE
        r = Run(L, flipped(g.stream, at, 0x40), g.offsets, oo, flags=flags)
        assert (r.rec.status, r.rec.first_bad, r.rec.out_len, r.rec.crc) == (E_BAD_CHECKSUM, B, 0, g.crc), at
    for cut in (1, 8, 10):                                                                  # the trailer cut
        assert verdict(stream_len=len(g.stream) - cut) == (E_NO_EOF, B), cut
    r = Run(L, g.stream + b"trailing garbage", g.offsets, oo, flags=flags)                  # bytes behind the trailer are no error
    assert (r.rec.status, r.rec.first_bad, r.rec.out_len, r.bytes()) == (OK, NOBODY, len(g.data), g.data)
    bad = flipped(g.stream, g.offsets[40] + 3, 0x20)                                        # a data bit: a member fails, or the CRC does
    r = Run(L, bad, g.offsets, oo, flags=flags)
    assert r.rec.status != OK and r.rec.out_len == 0 and r.rec.first_bad in (40, B)
    assert r.rec.first_bad == 40 or (r.rec.status == E_BAD_CHECKSUM and r.rec.crc != g.crc)


@pytest.mark.parametrize("short", [0, 4])
@pytest.mark.parametrize("flags", HINTS)
def test_unjoin_inside_guard_bands(engine, flags, short):
    """test_gpu_unjoin's containment test for the gzip call: an OK call and one whose last member's slot is a word too small"""
    L = engine.lib
    r = random.Random(3)
    blocks = blocks_of([4 * r.randint(2, 500) for _ in range(69)] + [1003], seed=8)
    g = gzip_ref.expected_gzip(blocks, 32, 10)
    B = len(blocks)
    oo = offsets_of(blocks)
    oo[-1] -= short
    total = oo[-1]
    wb = L.hdlz_unjoin_gzip_work_bytes(B, total, flags)
    band = 1 << 16
    specs = [("stream", len(g.stream), 1, band, True), ("off", 8 * (B + 1), 8, band, True), ("out_off", 8 * (B + 1), 8, band, True),
             ("out", total, 16, band), ("member", 4 * B, 4, band), ("result", 24, 8, band), ("work", wb, 256, band)]
    clean, runs = None, []
    for salt in (0x3C, 0x3C ^ 0xFF):
        a = guards.Arena(guards.Arena.size_for(specs), "cuda", salt)
        for s in specs:
            a.carve(*s)
        a.fill("stream", g.stream)
        a.fill("off", np.array(g.offsets, np.int64).view(np.uint8))
        a.fill("out_off", np.array(oo, np.int64).view(np.uint8))
        rc = L.hdlz_unjoin_gzip_ws(a.ptr("stream"), len(g.stream), a.ptr("off"), a.ptr("out_off"), 0, B, flags, a.ptr("out"), total,
                                   a.ptr("member"), a.ptr("result"), a.ptr("work"), wb, stream_ptr())
        assert rc == 0, L.hdlz_last_error()
        torch.cuda.synchronize()
        u = a.untouched_flat()
        clean = u if clean is None else clean & u
        runs.append({n: a.view(n).cpu().numpy().copy() for n in ("out", "member", "result")})
    for run_ in runs:
        rec = _lib.UnjoinGzipResult.from_buffer_copy(run_["result"].tobytes())
        if short:
            assert (rec.status, rec.first_bad, rec.out_len, rec.crc) == (E_OUT_CAPACITY, B - 1, 0, 0)
            assert list(run_["member"].view(np.int32)) == [0] * (B - 1) + [E_OUT_CAPACITY]
        else:
            assert (rec.status, rec.first_bad, rec.out_len, rec.crc) == (OK, NOBODY, total, g.crc)
            assert run_["out"].tobytes() == g.data and not run_["member"].any()
    assert runs[0]["result"].tobytes() == runs[1]["result"].tobytes() and runs[0]["member"].tobytes() == runs[1]["member"].tobytes()
    bad = guards.violations(a, clean, {"out": True, "member": True, "result": True, "work": True})
    assert bad == [], bad
    parts = a.split(clean)
    assert not bool(parts["member"][1].any()) and not bool(parts["result"][1].any())


# ---- CRC -> compress -> gzip join -> gzip unjoin as one serial chain in one HIP graph
def test_four_calls_in_one_hip_graph(engine):
    L = engine.lib
    blocks = blocks_of([4 * random.Random(k).randint(2, 300) for k in range(300)], seed=9)
    g = gzip_ref.expected_gzip(blocks, 32, 10)
    c = Call(engine, blocks, bound=1200)
    total, B = len(g.data), len(blocks)
    out = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    back = torch.zeros(3, dtype=torch.int64, device="cuda")
    uwb = L.hdlz_unjoin_gzip_work_bytes(B, total, 0)
    uwork = torch.zeros(uwb, dtype=torch.uint8, device="cuda")

    def calls():
        c.checksum()
        c.compress()
        c.join()
        rc = L.hdlz_unjoin_gzip_ws(c.stream.data_ptr(), len(g.stream), c.off.data_ptr(), c.in_off.data_ptr(), 0, B, 0, out.data_ptr(), total,
                                   None, back.data_ptr(), uwork.data_ptr(), uwb, stream_ptr())
        assert rc == 0, L.hdlz_last_error()

    def verify(label):
        check(label, c, blocks, want=g)
        rec = _lib.UnjoinGzipResult.from_buffer_copy(back.cpu().numpy().tobytes())
        assert (rec.status, rec.first_bad, rec.out_len, rec.crc) == (OK, NOBODY, total, g.crc), label
        assert out[:total].cpu().numpy().tobytes() == g.data and bool((out[total:] == 0xA5).all() or label == "eager"), label
    calls()
    verify("eager")
    graph, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            calls()
    for launch in range(3):
        for t in (c.rows, c.stream, out, uwork):
            t.fill_(0xA5)
        for t in (c.work, c.crc_work, c.crc):
            t.fill_(0x5A5A5A5A + launch)
        for t in (c.out_len, c.status, c.end_bits, c.off, c.result, back):
            t.fill_(-1 - launch)
        graph.replay()
        verify(("graph", launch))


# ---- the Engine
@pytest.mark.parametrize("n", [5, 69, 65537])
def test_engine_containers(engine, n):
    from hdl_deflate_amd.chain import plan_blocks
    import joined_ref
    data = (family_bytes(2, 40000, seed=n) + family_bytes(1, 30000, seed=n))[:n]
    plan = plan_blocks(n, 65536)
    blocks = [data[o:o + ln] for o, ln in plan]
    g = gzip_ref.expected_gzip(blocks, 32, 10)
    d = dev(np.frombuffer(data, np.uint8))
    z, offs = engine.compress_joined(d, block=65536, container="gzip")
    torch.cuda.synchronize()
    assert z.cpu().numpy().tobytes() == g.stream and list(offs.cpu().numpy()) == g.offsets
    assert gzip.decompress(g.stream) == data
    back = engine.inflate_joined(z, offs, block=65536, total=n, container="gzip")
    assert back.cpu().numpy().tobytes() == data
    assert engine.compress_bytes(data, block=65536, container="gzip") == (OK, g.stream)
    assert engine.inflate_bytes(g.stream, members=(g.offsets, 65536), container="gzip") == (OK, data)          # the length from ISIZE
    assert engine.inflate_bytes(g.stream, out_cap=n, members=(g.offsets, 65536), container="gzip") == (OK, data)
    assert engine.inflate_bytes(flipped(g.stream, len(g.stream) - 6, 1), out_cap=n, members=(g.offsets, 65536), container="gzip") == (E_BAD_CHECKSUM, b"")
    assert engine.inflate_bytes(g.stream[:-3], members=(g.offsets, 65536), container="gzip") == (E_NO_EOF, b"")
    # ISIZE damaged and no out_cap: the length is read from it before anything is verified.  +1 / +4: the index still fits, the last
    # slot is wrong; a high byte flipped: the index cannot belong to that length
    for delta in (1, 4, 1 << 20, -1):
        isize = ((n + delta) & 0xFFFFFFFF).to_bytes(4, "little")
        assert engine.inflate_bytes(g.stream[:-4] + isize, members=(g.offsets, 65536), container="gzip") == (E_BAD_CHECKSUM, b""), delta
    assert engine.compress_bytes(b"abcd", block=65536, container="gzip") == (E_SHORT_INPUT, b"")
    # the default container is the zlib form, byte for byte what it was
    j = joined_ref.expected_joined(blocks, 32, 10)
    for kw in ({}, {"container": "zlib"}):
        zz, zo = engine.compress_joined(d, block=65536, **kw)
        assert zz.cpu().numpy().tobytes() == j.stream and list(zo.cpu().numpy()) == j.offsets
        assert engine.compress_bytes(data, block=65536, **kw) == (OK, j.stream)
        assert engine.inflate_bytes(j.stream, members=(j.offsets, 65536), **kw) == (OK, data)
        assert engine.inflate_joined(zz, zo, block=65536, total=n, **kw).cpu().numpy().tobytes() == data
    for call in (lambda: engine.compress_joined(d, container="gz"), lambda: engine.inflate_joined(z, offs, block=65536, total=n, container="raw"),
                 lambda: engine.compress_bytes(data, block=65536, container="deflate"),
                 lambda: engine.inflate_bytes(g.stream, members=(g.offsets, 65536), container="GZIP")):
        with pytest.raises(ValueError):
            call()
    assert int(engine.crc32(d).cpu().numpy()[0]) == zlib.crc32(data)
