"""GPU (-m gpu): a batch of blocks as ONE standard zlib stream -- hdlz_compress_batch_bits + hdlz_join_batch_ws (include/hdlz_join.h),
Engine.compress_joined and compress_bytes(block=...).  Every byte is compared with joined_ref.expected_joined, which is built from the
CPU oracle's per-block streams and stock zlib only; the end bits with its walk over the oracle's fixed-Huffman codes."""
import random
import zlib

import numpy as np
import pytest
import torch

import guards
import joined_ref
from hdl_deflate_amd import _lib
from hdl_deflate_amd.constants import out_bound
from hdl_deflate_amd.data import family_bytes

pytestmark = pytest.mark.gpu

OK, E_SHORT_INPUT, E_OUT_CAPACITY = 0, 1, 2


def round4(x):
    return (x + 3) & ~3


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


_pools = {}


def pool(f):
    """4 KiB of data family f (hdl_deflate_amd.data: 1 .. 4), 0 = random bytes"""
    if f not in _pools:
        _pools[f] = family_bytes(f, 4096, seed=11 + f) if f else bytes(random.Random(5).randrange(256) for _ in range(4096))
    return _pools[f]


def ragged_blocks(B, lo, hi, seed):
    r = random.Random(seed)
    out = []
    for k in range(B):
        n = r.randint(lo, hi)
        a = r.randrange(0, 4096 - n)
        out.append(pool(k % 5)[a:a + n])
    return out


class Call(object):
    """the buffers of one compress + join; ragged (in_off, `bound` = the stated in_len) or fixed = (n, in_pitch)"""

    def __init__(self, engine, blocks, cw=32, mm=10, bound=0, fixed=None, cap=None, pitch=None):
        self.L, self.B, self.cw, self.mm = engine.lib, len(blocks), cw, mm
        B = self.B
        nmax = max([len(b) for b in blocks] + [bound, 5])
        self.pitch = pitch or round4(out_bound(nmax))
        if fixed:
            n, in_pitch = fixed
            flat = np.zeros(B * in_pitch + 64, np.uint8)
            for b, blk in enumerate(blocks):
                flat[b * in_pitch:b * in_pitch + n] = np.frombuffer(blk, np.uint8)
            self.in_off, self.in_pitch, self.in_len = None, in_pitch, n
        else:
            flat = np.frombuffer(b"".join(blocks) + bytes(64), np.uint8)
            off = np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).astype(np.int64)
            self.in_off, self.in_pitch, self.in_len = dev(off), 0, bound
        self.d_in = dev(flat)
        self.rows = torch.zeros((max(B, 1), self.pitch), dtype=torch.uint8, device="cuda")
        self.out_len, self.status = (torch.full((max(B, 1),), -1, dtype=torch.int32, device="cuda") for _ in range(2))
        self.end_bits = torch.full((max(B, 1),), -1, dtype=torch.int64, device="cuda")
        self.cap = self.L.hdlz_join_bound(B, nmax) if cap is None else cap
        self.stream = torch.zeros(max(self.cap, 1), dtype=torch.uint8, device="cuda")
        self.off = torch.full((B + 1,), -1, dtype=torch.int64, device="cuda")
        self.result = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        self.wb = self.L.hdlz_join_work_bytes(B)
        self.work = torch.zeros(max(self.wb, 8) // 8, dtype=torch.int64, device="cuda")

    def _in(self):
        return (self.d_in.data_ptr(), self.in_off.data_ptr() if self.in_off is not None else None, self.in_pitch, self.in_len, self.B,
                self.cw, self.mm)

    def compress(self):
        rc = self.L.hdlz_compress_batch_bits(*self._in(), self.rows.data_ptr(), self.pitch, self.out_len.data_ptr(), self.status.data_ptr(),
                                             self.end_bits.data_ptr(), stream_ptr())
        assert rc == 0, self.L.hdlz_last_error()

    def compress_plain(self):
        """hdlz_compress_batch on the same input -> (rows, out_len, status) as numpy"""
        rows = torch.zeros_like(self.rows)
        ol, st = torch.zeros_like(self.out_len), torch.zeros_like(self.status)
        rc = self.L.hdlz_compress_batch(*self._in(), rows.data_ptr(), self.pitch, ol.data_ptr(), st.data_ptr(), stream_ptr())
        assert rc == 0, self.L.hdlz_last_error()
        torch.cuda.synchronize()
        return rows.cpu().numpy(), ol.cpu().numpy(), st.cpu().numpy()

    def join(self):
        rc = self.L.hdlz_join_batch_ws(self.rows.data_ptr(), self.pitch, self.out_len.data_ptr(), self.end_bits.data_ptr(),
                                       self.status.data_ptr(), self.in_off.data_ptr() if self.in_off is not None else None, self.in_len,
                                       self.B, self.stream.data_ptr(), self.cap, self.off.data_ptr(), self.result.data_ptr(),
                                       self.work.data_ptr() if self.wb else None, self.wb, stream_ptr())
        assert rc == 0, self.L.hdlz_last_error()

    def record(self):
        torch.cuda.synchronize()
        r = _lib.JoinResult.from_buffer_copy(self.result.cpu().numpy().tobytes())
        return r.stream_len, r.status, r.adler


def check(label, c, blocks, want=None):
    """the device's rows, end bits, offsets, stream and record against the reference"""
    j = want or joined_ref.expected_joined(blocks, c.cw, c.mm)
    slen, st, ad = c.record()
    B = len(blocks)
    if B:
        ol, bs, eb = c.out_len.cpu().numpy()[:B], c.status.cpu().numpy()[:B], c.end_bits.cpu().numpy()[:B]
        assert not bs.any(), (label, bs)
        assert list(eb) == j.end_bits, (label, "end bits", [k for k in range(B) if eb[k] != j.end_bits[k]][:8])
        assert list(ol) == [((E + 14) >> 3) + 4 for E in j.end_bits] == [len(z) for z in j.rows], (label, "out_len")
        rows = c.rows.cpu().numpy()
        for b in range(B):
            assert rows[b, :ol[b]].tobytes() == j.rows[b], (label, "row", b)
    assert (slen, st, ad) == (len(j.stream), OK, j.adler), (label, slen, st, hex(ad), len(j.stream), hex(j.adler))
    assert list(c.off.cpu().numpy()) == j.offsets, (label, "offsets")
    z = c.stream[:slen].cpu().numpy().tobytes()
    assert z == j.stream, (label, "stream", next(k for k in range(len(z)) if z[k] != j.stream[k]))
    d = zlib.decompressobj()
    assert d.decompress(z) == j.data and d.eof and d.unused_data == b"" and ad == zlib.adler32(j.data), label
    return j


@pytest.mark.parametrize("B", [0, 1, 2, 255, 256, 257, 513])
def test_block_counts_at_the_tile_edges_of_the_look_back(engine, B):
    """ragged blocks of 5 .. 64 bytes from the four data families and random bytes.  From 255 blocks on the batch itself holds (asserted
    on the reference) every number of pad bits, both marker lengths, members that start at and off a 16-byte boundary and members
    shorter than 16 bytes; the batches of 0, 1 and 2 blocks are too small to hold eight values of anything."""
    blocks = ragged_blocks(B, 5, 64, seed=B)
    c = Call(engine, blocks, bound=64)
    c.compress()
    c.join()
    j = check(("count", B), c, blocks)
    if B >= 255:
        assert set(j.pads) == set(range(8)), sorted(set(j.pads))
        assert {len(m) - (len(z) - 6) for m, z in zip(j.members, j.rows)} == {4, 5}
        assert c.stream.data_ptr() % 16 == 0
        starts = {o % 16 for o in j.offsets[:-1]}
        assert 0 in starts and len(starts) > 1, starts
        # ... and BFINAL is cleared on both paths of the copy: in a 16-byte store (an aligned member with 16 row bytes) and singly
        assert any(o % 16 == 0 and len(z) - 6 >= 16 for o, z in zip(j.offsets, j.rows)), "no aligned member with a 16-byte body"
        assert any(o % 16 != 0 for o in j.offsets[:-1])
        assert min(len(m) for m in j.members) < 16 and max(len(m) for m in j.members) >= 32


def test_sizes_around_the_compress_tile(engine):
    """fixed-pitch batches of 2047 / 2048 / 2049 / 4113 bytes (one tile, its edge, two tiles, two tiles and a bit: end bits behind
    flushed words) and a ragged mix of them, five blocks each"""
    def five(n, seed):
        big = b"".join(family_bytes(1 + (seed + k) % 4, 4200, seed=seed + k) for k in range(5))
        return [big[k * 4200:k * 4200 + n] for k in range(5)]
    for n in (2047, 2048, 2049, 4113):
        blocks = five(n, n)
        c = Call(engine, blocks, fixed=(n, (n + 15) // 16 * 16))
        c.compress()
        c.join()
        check(("fixed", n), c, blocks)
    blocks = [five(n, 3 * n)[k] for k, n in enumerate((2049, 2047, 4113, 2048, 2047))]
    for bound in (0, 4113):
        c = Call(engine, blocks, bound=bound)
        c.compress()
        c.join()
        check(("mix", bound), c, blocks)


@pytest.mark.parametrize("cw,mm", [(32, 10), (33, 10), (64, 10), (256, 10), (32, 5)])
def test_windows_and_the_small_block_shape(engine, cw, mm):
    """ragged blocks with a stated bound <= 1024 -- the shape hdlz_compress_batch packs several to a wave: the call with end bits
    keeps them on the wave-per-block kernels, the rows are the same bytes and the end bits the walker's, for every window kernel"""
    blocks = ragged_blocks(70, 5, 300, seed=cw + mm) + ragged_blocks(8, 900, 1024, seed=cw)
    c = Call(engine, blocks, cw=cw, mm=mm, bound=1024)
    c.compress()
    rows, ol, st = c.compress_plain()
    assert not st.any() and np.array_equal(ol, c.out_len.cpu().numpy())
    mine = c.rows.cpu().numpy()
    for b in range(len(blocks)):
        assert np.array_equal(rows[b, :ol[b]], mine[b, :ol[b]]), (cw, mm, b)
    c.join()
    check(("window", cw, mm), c, blocks)


def test_round_trip_through_the_checked_inflate(engine):
    """64 KiB in 4 KiB blocks: the library's own inflate reads the joined stream (fixed blocks and empty stored blocks) and verifies
    its header and Adler-32"""
    data = b"".join(family_bytes(1 + k % 4, 4096, seed=40 + k) for k in range(16))
    blocks = [data[k:k + 4096] for k in range(0, 65536, 4096)]
    c = Call(engine, blocks, fixed=(4096, 4096))
    c.compress()
    c.join()
    j = check("64 KiB", c, blocks)
    st, back = engine.inflate_bytes(j.stream, verify=True)
    assert st == OK and back == data


def test_failed_block_and_short_capacity(engine):
    blocks = ragged_blocks(40, 5, 64, seed=77)
    bad = blocks[:20] + [b"abcd"] + blocks[20:]
    c = Call(engine, bad, bound=64)
    c.compress()
    c.join()
    assert c.record() == (0, E_SHORT_INPUT, 0)
    assert int(c.status[20]) == E_SHORT_INPUT and int(c.end_bits[20]) == 0 and int(c.out_len[20]) == 0
    j = joined_ref.expected_joined(blocks, 32, 10)
    for cap in (len(j.stream) - 1, 7):
        c = Call(engine, blocks, bound=64, cap=cap)
        c.compress()
        c.join()
        assert c.record() == (len(j.stream), E_OUT_CAPACITY, j.adler), (cap, c.record())
        assert list(c.off.cpu().numpy()) == j.offsets
        z = c.stream.cpu().numpy().tobytes()
        fits = max(o for o in j.offsets if o <= cap)                   # the members that end inside the capacity are there
        assert z[:fits] == j.stream[:fits], cap


@pytest.mark.parametrize("B,short", [(257, 0), (257, 1), (3, 0), (3, 9)])
def test_join_inside_guard_bands(engine, B, short):
    """every buffer of hdlz_join_batch_ws carved out of one patterned arena (tests/guards.py), stream_cap exact and short, rows filled
    up to their length only: run on the pattern and on its complement, no byte outside the stated "writes" changes and the results are
    identical -- nothing depends on row slack, on the scratch or on what the outputs held"""
    L = engine.lib
    blocks = ragged_blocks(B, 5, 200, seed=100 + B)
    j = joined_ref.expected_joined(blocks, 32, 10)
    pitch = round4(out_bound(200))
    cap = len(j.stream) - short
    wb = L.hdlz_join_work_bytes(B)
    off = np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).astype(np.int64)
    band = 1 << 16
    specs = [("rows", B * pitch, 4, band, True), ("len", 4 * B, 4, band, True), ("bits", 8 * B, 8, band, True), ("status", 4 * B, 4, band, True),
             ("in_off", 8 * (B + 1), 8, band, True), ("stream", cap, 16, band, False, 5), ("off", 8 * (B + 1), 8, band),
             ("result", 16, 8, band), ("work", wb, 8, band)]
    clean, runs = None, []
    for salt in (0x3C, 0x3C ^ 0xFF):
        a = guards.Arena(guards.Arena.size_for(specs), "cuda", salt)
        for s in specs:
            a.carve(*s)
        for b, z in enumerate(j.rows):
            a.fill("rows", z, at=b * pitch)
        a.fill("len", np.array([len(z) for z in j.rows], np.uint32).view(np.uint8))
        a.fill("bits", np.array(j.end_bits, np.uint64).view(np.uint8))
        a.fill("status", np.zeros(B, np.uint32).view(np.uint8))
        a.fill("in_off", off.view(np.uint8))
        rc = L.hdlz_join_batch_ws(a.ptr("rows"), pitch, a.ptr("len"), a.ptr("bits"), a.ptr("status"), a.ptr("in_off"), 200, B, a.ptr("stream"),
                                  cap, a.ptr("off"), a.ptr("result"), a.ptr("work"), wb, stream_ptr())
        assert rc == 0, L.hdlz_last_error()
        torch.cuda.synchronize()
        u = a.untouched_flat()
        clean = u if clean is None else clean & u
        runs.append({n: a.view(n).cpu().numpy().copy() for n in ("stream", "off", "result")})
    written = np.zeros(cap, bool)                                      # the header, the members that fit, the trailer if all fits
    written[:2] = True
    for b in range(B):
        if j.offsets[b + 1] <= cap:
            written[j.offsets[b]:j.offsets[b + 1]] = True
    if not short:
        written[:] = True
    for r in runs:
        rec = _lib.JoinResult.from_buffer_copy(r["result"].tobytes())
        assert (rec.stream_len, rec.status, rec.adler) == (len(j.stream), E_OUT_CAPACITY if short else OK, j.adler)
        assert list(r["off"].view(np.int64)) == j.offsets
        assert np.array_equal(r["stream"][written], np.frombuffer(j.stream, np.uint8)[:cap][written])
    bad = guards.violations(a, clean, {"stream": torch.from_numpy(written), "off": True, "result": True, "work": True})
    assert bad == [], bad
    parts = a.split(clean)
    assert not bool(parts["off"][1].any()) and not bool(parts["result"][1].any())          # ... and those ARE written


def test_both_calls_in_one_hip_graph(engine):
    blocks = ragged_blocks(300, 5, 300, seed=9)
    c = Call(engine, blocks, bound=300)
    c.compress()
    c.join()
    j = check("eager", c, blocks)
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            c.compress()
            c.join()
    for launch in range(3):
        for t in (c.rows, c.stream, c.work):
            t.fill_(0xA5 if t.dtype == torch.uint8 else 0x5A5A5A5A + launch)
        for t in (c.out_len, c.status, c.end_bits, c.off, c.result):
            t.fill_(-1 - launch)
        g.replay()
        check(("graph", launch), c, blocks, want=j)


@pytest.mark.parametrize("n", [5, 69, 65537])
def test_engine_compress_joined_and_compress_bytes(engine, n):
    """block = 65536; 65537 bytes: the tail of one byte shortens the block before it (chain.plan_blocks)"""
    from hdl_deflate_amd.chain import plan_blocks
    data = (family_bytes(2, 40000, seed=n) + family_bytes(1, 30000, seed=n))[:n]
    plan = plan_blocks(n, 65536)
    assert len(plan) == (2 if n == 65537 else 1) and (n != 65537 or plan[-1][1] >= 5)
    j = joined_ref.expected_joined([data[o:o + ln] for o, ln in plan], 32, 10)
    z, offs = engine.compress_joined(dev(np.frombuffer(data, np.uint8)), block=65536)
    torch.cuda.synchronize()
    assert z.cpu().numpy().tobytes() == j.stream and list(offs.cpu().numpy()) == j.offsets
    assert engine.compress_bytes(data, block=65536) == (OK, j.stream)
    assert zlib.decompress(j.stream) == data
    if len(plan) == 1:
        assert engine.compress_bytes(data) == (OK, j.rows[0])                    # block=None: one block, as before
    assert engine.compress_bytes(b"abcd", block=65536) == (E_SHORT_INPUT, b"")
