"""GPU (-m gpu): a joined stream read back member by member -- hdlz_unjoin_ws (include/hdlz_unjoin.h), Engine.inflate_joined and
inflate_bytes(members=...).  The streams and their indices come from joined_ref.expected_joined (the CPU oracle's per-block streams
and stock zlib), the expected data from the input and zlib.decompress; nothing is compared with device output.  Every case runs
without a mapping hint and under each of the three."""
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
from hdl_deflate_amd.errors import HdlzStatusError

pytestmark = pytest.mark.gpu

OK, E_OUT_CAPACITY, E_NO_EOF, E_BAD_PARAM, E_BAD_HEADER, E_BAD_CHECKSUM = 0, 2, 5, 8, 11, 12
LANE, WAVE, GROUP = 2, 4, 64
HINTS = (0, LANE, WAVE, GROUP)
NOBODY = (1 << 64) - 1


def dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype)).cuda()


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


_pool = {}


def pool(kind):
    """64 KiB of one kind of data: 1 .. 4 the bench families, 0 random bytes, 5 text of ten letters, 6 zeros"""
    if kind not in _pool:
        r = random.Random(17 + kind)
        _pool[kind] = (bytes(r.randrange(256) for _ in range(1 << 16)) if kind == 0 else bytes(1 << 16) if kind == 6 else
                       bytes(r.choice(b"abcdefgh \n") for _ in range(1 << 16)) if kind == 5 else family_bytes(kind, 1 << 16, seed=11 + kind))
    return _pool[kind]


def blocks_of(lengths, seed, distinct=48):
    """one block per length: text, random bytes, zeros, the bench families in turn, every sixth a repeat of the block in front (same
    length) -- drawn from at most `distinct` places of the pools, so that the CPU reference compresses each block once"""
    r = random.Random(seed)
    out = []
    for k, n in enumerate(lengths):
        if k % 6 == 5 and len(out[-1]) == n:
            out.append(out[-1])
            continue
        a = 64 * r.randrange(distinct)
        out.append(pool(k % 7)[a:a + n])
    return out


def offsets_of(blocks):
    return [0] + [int(x) for x in np.cumsum([len(b) for b in blocks])]


class Run(object):
    """one hdlz_unjoin_ws call: every output pre-filled with junk, then the record, the bytes and the member statuses"""

    def __init__(self, L, stream, off, out_off=None, out_len=0, out_cap=None, flags=0, stream_len=None, fill=0xA5):
        B = len(off) - 1
        if out_cap is None:
            out_cap = out_off[-1] if out_off is not None else B * out_len
        self.d_stream, self.d_off = dev(np.frombuffer(stream + bytes(8), np.uint8)), dev(off, np.int64)
        self.d_out_off = dev(out_off, np.int64) if out_off is not None else None
        self.out = torch.full((out_cap + 64,), fill, dtype=torch.uint8, device="cuda")
        self.member = torch.full((max(B, 1),), -1, dtype=torch.int32, device="cuda")
        self.result = torch.full((3,), -1, dtype=torch.int64, device="cuda")
        wb = L.hdlz_unjoin_work_bytes(B, out_cap, flags)
        self.work = torch.full((max(wb, 1),), fill ^ 0xFF, dtype=torch.uint8, device="cuda")
        rc = L.hdlz_unjoin_ws(self.d_stream.data_ptr(), len(stream) if stream_len is None else stream_len, self.d_off.data_ptr(),
                              self.d_out_off.data_ptr() if out_off is not None else None, out_len, B, flags,
                              self.out.data_ptr() if out_cap else None, out_cap, self.member.data_ptr(), self.result.data_ptr(),
                              self.work.data_ptr() if wb else None, wb, stream_ptr())
        assert rc == 0, L.hdlz_last_error()
        torch.cuda.synchronize()
        self.rec = _lib.UnjoinResult.from_buffer_copy(self.result.cpu().numpy().tobytes())
        self.members = list(self.member.cpu().numpy()[:B])
        self.out_cap, self.fill = out_cap, fill

    def bytes(self):
        return self.out[:self.rec.out_len].cpu().numpy().tobytes()

    def slack_untouched(self):
        return bool((self.out[self.out_cap:] == self.fill).all())


def roundtrip(engine, label, blocks, cw=32, mm=10, uniform=False):
    """the reference's stream of `blocks` through the call, with and without every hint -> the reference"""
    j = joined_ref.expected_joined(blocks, cw, mm)
    assert zlib.decompress(j.stream) == j.data
    for flags in HINTS:
        r = Run(engine.lib, j.stream, j.offsets, None if uniform else offsets_of(blocks), len(blocks[0]) if uniform else 0, flags=flags)
        rec = r.rec
        assert (rec.status, rec.first_bad, rec.out_len, rec.adler) == (OK, NOBODY, len(j.data), zlib.adler32(j.data)), \
            (label, flags, rec.status, rec.first_bad, rec.out_len, [k for k, s in enumerate(r.members) if s][:8])
        got = r.bytes()
        assert got == j.data, (label, flags, next(k for k in range(len(got)) if got[k] != j.data[k]))
        assert not any(r.members) and r.slack_untouched(), (label, flags)
    return j


@pytest.mark.parametrize("B", [1, 2, 64, 65, 300])
@pytest.mark.parametrize("n", [32, 2044, 2048, 2052, 4096])
def test_uniform_blocks(engine, n, B):
    """fixed-size members without an offset array (o_b = b * out_len): one ring line, the group kernel's ring and its edge, two rings;
    one member, two, a wave of lanes, one more (the lane mapping's length-ordered lists start above HDLZ_INFLATE_BIN_MIN = 64), several
    workgroups of every mapping"""
    roundtrip(engine, ("uniform", n, B), blocks_of([n] * B, seed=n + B, distinct=24), uniform=True)


@pytest.mark.parametrize("tail", [4996, 5, 7])
def test_ragged_batches(engine, tail):
    """lengths 8 .. 5000, all but the last a multiple of 4 (what chain.plan_blocks cuts with such a block size): text, random bytes,
    zeros, the bench families and repeats of the block in front; the last member 5 and 7 bytes long (the plan's shortest tails)"""
    r = random.Random(tail)
    lengths = [8, 5000, 12, 2048] + [4 * r.randint(2, 1250) for _ in range(90)] + [tail]
    j = roundtrip(engine, ("ragged", tail), blocks_of(lengths, seed=tail))
    assert {len(m) - (len(z) - 6) for m, z in zip(j.members, j.rows)} == {4, 5} and len(set(j.pads)) == 8


@pytest.mark.parametrize("cw,mm", [(32, 10), (256, 10), (32, 5), (256, 5)])
def test_windows_and_match_lengths(engine, cw, mm):
    r = random.Random(cw + mm)
    roundtrip(engine, ("window", cw, mm), blocks_of([4 * r.randint(2, 700) for _ in range(70)] + [333], seed=cw * mm), cw=cw, mm=mm)


def test_three_large_members(engine):
    """300 KiB each: thousands of flushed lines per member, copies that read flushed output back (CWINDOW 256: distances beyond the lane
    kernel's ring), a checksum of 29 tiles"""
    blocks = [family_bytes(1 + k, 300 * 1024, seed=70 + k) for k in range(3)]
    roundtrip(engine, "large", blocks, cw=256)


def test_all_ff_across_tile_edges(engine):
    """the worst case of the checksum's bounds (hdlz_adler.h) through the flat finish: every byte FF, two and three full 32 KiB tiles
    and an odd tail of 3 and 5 bytes, the capacity the total itself"""
    for lengths, total in (([32768, 32764, 7], 65539), ([32768, 32768, 32768, 5], 98309)):
        assert sum(lengths) == total
        roundtrip(engine, ("ff", total), [b"\xff" * n for n in lengths])


def test_no_members(engine):
    for flags in HINTS:
        r = Run(engine.lib, b"\x78\x9c\x03\x00\x00\x00\x00\x01", [2], out_cap=0, flags=flags)
        assert (r.rec.status, r.rec.first_bad, r.rec.out_len, r.rec.adler) == (OK, NOBODY, 0, 1)
        r = Run(engine.lib, b"\x78\x9c\x03\x00\x00\x00\x00\x02", [2], out_cap=0, flags=flags)
        assert (r.rec.status, r.rec.first_bad, r.rec.out_len, r.rec.adler) == (E_BAD_CHECKSUM, 0, 0, 1)


# ---- damaged streams: one reference batch, one change each
_damage = {}


def damage_base():
    if not _damage:
        r = random.Random(99)
        blocks = blocks_of([4 * r.randint(2, 300) for _ in range(71)] + [61], seed=5)
        _damage["j"] = joined_ref.expected_joined(blocks, 32, 10)
        _damage["out_off"] = offsets_of(blocks)
    return _damage["j"], list(_damage["out_off"])


def flipped(z, at, xor):
    z = bytearray(z)
    z[at] ^= xor
    return bytes(z)


def damaged(engine, flags, stream=None, off=None, out_off=None, stream_len=None, out_cap=None):
    j, oo = damage_base()
    return Run(engine.lib, j.stream if stream is None else stream, j.offsets if off is None else off, oo if out_off is None else out_off,
               flags=flags, stream_len=stream_len, out_cap=out_cap)


@pytest.mark.parametrize("flags", HINTS)
def test_damaged_frame(engine, flags):
    j, _ = damage_base()
    B, end = len(j.members), j.offsets[-1]
    r = damaged(engine, flags, stream=flipped(j.stream, len(j.stream) - 1, 0x01))
    assert (r.rec.status, r.rec.first_bad, r.rec.out_len, r.rec.adler) == (E_BAD_CHECKSUM, B, 0, j.adler) and not any(r.members)
    assert j.stream[end:end + 2] == b"\x03\x00"
    r = damaged(engine, flags, stream=flipped(j.stream, end + 1, 0x01))                    # 03 00 -> 03 01
    assert (r.rec.status, r.rec.first_bad, r.rec.out_len) == (E_NO_EOF, B, 0)
    r = damaged(engine, flags, stream=flipped(j.stream, 1, 0x01))                          # 78 9C -> 78 9D
    assert (r.rec.status, r.rec.first_bad, r.rec.out_len) == (E_BAD_HEADER, B, 0)
    r = damaged(engine, flags, stream_len=len(j.stream) - 1)
    assert (r.rec.status, r.rec.first_bad, r.rec.out_len) == (E_NO_EOF, B, 0)
    r = damaged(engine, flags, stream=j.stream + b"trailing garbage")                      # bytes behind the frame are no error
    assert (r.rec.status, r.rec.first_bad, r.rec.out_len, r.bytes()) == (OK, NOBODY, len(j.data), j.data)


@pytest.mark.parametrize("flags", HINTS)
def test_damaged_members(engine, flags):
    j, oo = damage_base()
    B = len(j.members)
    for k in (0, 33, B - 1):                                                                # a member's FF FF -> FF FE
        assert j.stream[j.offsets[k + 1] - 2:j.offsets[k + 1]] == b"\xff\xff"
        r = damaged(engine, flags, stream=flipped(j.stream, j.offsets[k + 1] - 1, 0x01))
        assert (r.rec.status, r.rec.first_bad, r.rec.out_len, r.rec.adler) == (E_NO_EOF, k, 0, 0), (k, r.rec.status, r.rec.first_bad)
        assert [b for b, s in enumerate(r.members) if s] == [k] and r.members[k] == E_NO_EOF
    # the first pad bit behind an end-of-block code (p >= 3: it is the empty stored block's BFINAL) set: zlib ends the stream there
    k = next(b for b in range(2, B) if j.pads[b] >= 3)
    e = j.end_bits[k] + 7                                                                   # counted from byte offsets[k] - 2
    bad = flipped(j.stream, j.offsets[k] - 2 + (e >> 3), 1 << (e & 7))
    with pytest.raises(zlib.error):
        zlib.decompress(bad)
    r = damaged(engine, flags, stream=bad)
    assert (r.rec.status, r.rec.first_bad, r.rec.out_len) == (E_NO_EOF, k, 0)
    # the index moved by one byte at member k: the member in front of it or k itself fails
    for k in (1, 40):
        off = list(j.offsets)
        off[k] += 1
        r = damaged(engine, flags, off=off)
        assert r.rec.status != OK and r.rec.first_bad in (k - 1, k) and r.rec.out_len == 0, (k, r.rec.status, r.rec.first_bad)


@pytest.mark.parametrize("flags", [LANE, WAVE, GROUP])
def test_failed_members_beyond_the_first_wave_and_workgroup(engine, flags):
    """600 members of 5 to 64 bytes: the failing ones sit in other waves and other workgroups of the judge than member 0 -- the lowest
    one is reported"""
    if "many" not in _damage:
        r = random.Random(600)
        blocks = blocks_of([4 * r.randint(2, 16) for _ in range(599)] + [5], seed=6)
        _damage["many"] = (joined_ref.expected_joined(blocks, 32, 10), offsets_of(blocks))
    j, oo = _damage["many"]
    for bad in ((300, 570), (570,)):
        z = j.stream
        for k in bad:                                                                       # a member's FF FF -> FF FE
            assert z[j.offsets[k + 1] - 2:j.offsets[k + 1]] == b"\xff\xff"
            z = flipped(z, j.offsets[k + 1] - 1, 0x01)
        r = Run(engine.lib, z, j.offsets, oo, flags=flags)
        assert (r.rec.status, r.rec.first_bad, r.rec.out_len, r.rec.adler) == (E_NO_EOF, bad[0], 0, 0), (bad, r.rec.status, r.rec.first_bad)
        assert [(b, s) for b, s in enumerate(r.members) if s] == [(k, E_NO_EOF) for k in bad]


@pytest.mark.parametrize("flags", HINTS)
def test_wrong_output_slots(engine, flags):
    j, oo = damage_base()
    B = len(j.members)
    for k in (0, 20, B - 2):
        small = list(oo)
        small[k + 1] -= 4                                                                   # member k: one word too small
        r = damaged(engine, flags, out_off=small)
        assert (r.rec.status, r.rec.first_bad, r.rec.out_len, r.rec.adler) == (E_OUT_CAPACITY, k, 0, 0), (k, r.rec.status, r.rec.first_bad)
        large = list(oo)
        large[k + 1] += 4                                                                   # member k: one word too large
        r = damaged(engine, flags, out_off=large)
        assert (r.rec.status, r.rec.first_bad, r.rec.out_len) == (E_BAD_PARAM, k, 0), (k, r.rec.status, r.rec.first_bad)
        assert r.members[k + 1] == E_OUT_CAPACITY
    odd = list(oo)
    odd[7] += 1                                                                             # o_7 is no multiple of 4
    r = damaged(engine, flags, out_off=odd)
    assert r.rec.status == E_BAD_PARAM and r.rec.first_bad == 6 and r.members[7] == E_BAD_PARAM and r.members[6] == E_BAD_PARAM
    r = damaged(engine, flags, out_cap=oo[-1] - 4)                                          # the last slot ends behind the capacity
    assert (r.rec.status, r.rec.first_bad) == (E_BAD_PARAM, B - 1) and r.slack_untouched()


# ---- containment
@pytest.mark.parametrize("short", [0, 4])
@pytest.mark.parametrize("flags", HINTS)
def test_unjoin_inside_guard_bands(engine, flags, short):
    """every buffer of the call carved out of one patterned arena (tests/guards.py), d_out exactly as long as the index says: an OK call,
    and one whose LAST member's slot is a word too small -- a slot whose length is no multiple of 4, so a dword or 16-byte store of an
    overflowing member would land behind out_cap.  Run on the pattern and on its complement: no band byte changes, and the record (and
    the bytes of the OK call) are the same -- nothing depends on what the outputs or the scratch held"""
    L = engine.lib
    r = random.Random(3)
    blocks = blocks_of([4 * r.randint(2, 500) for _ in range(69)] + [1003], seed=8)
    j = joined_ref.expected_joined(blocks, 32, 10)
    B = len(blocks)
    oo = offsets_of(blocks)
    oo[-1] -= short
    total = oo[-1]
    assert (oo[-1] - oo[-2]) % 4 == 3
    wb = L.hdlz_unjoin_work_bytes(B, total, flags)
    band = 1 << 16
    specs = [("stream", len(j.stream), 1, band, True), ("off", 8 * (B + 1), 8, band, True), ("out_off", 8 * (B + 1), 8, band, True),
             ("out", total, 16, band), ("member", 4 * B, 4, band), ("result", 24, 8, band), ("work", wb, 256, band)]
    clean, runs = None, []
    for salt in (0x3C, 0x3C ^ 0xFF):
        a = guards.Arena(guards.Arena.size_for(specs), "cuda", salt)
        for s in specs:
            a.carve(*s)
        a.fill("stream", j.stream)
        a.fill("off", np.array(j.offsets, np.int64).view(np.uint8))
        a.fill("out_off", np.array(oo, np.int64).view(np.uint8))
        rc = L.hdlz_unjoin_ws(a.ptr("stream"), len(j.stream), a.ptr("off"), a.ptr("out_off"), 0, B, flags, a.ptr("out"), total, a.ptr("member"),
                              a.ptr("result"), a.ptr("work"), wb, stream_ptr())
        assert rc == 0, L.hdlz_last_error()
        torch.cuda.synchronize()
        u = a.untouched_flat()
        clean = u if clean is None else clean & u
        runs.append({n: a.view(n).cpu().numpy().copy() for n in ("out", "member", "result")})
    for run in runs:
        rec = _lib.UnjoinResult.from_buffer_copy(run["result"].tobytes())
        if short:
            assert (rec.status, rec.first_bad, rec.out_len, rec.adler) == (E_OUT_CAPACITY, B - 1, 0, 0)
            assert list(run["member"].view(np.int32)) == [0] * (B - 1) + [E_OUT_CAPACITY]
        else:
            assert (rec.status, rec.first_bad, rec.out_len, rec.adler) == (OK, NOBODY, total, j.adler)
            assert run["out"].tobytes() == j.data and not run["member"].any()
    assert runs[0]["result"].tobytes() == runs[1]["result"].tobytes() and runs[0]["member"].tobytes() == runs[1]["member"].tobytes()
    bad = guards.violations(a, clean, {"out": True, "member": True, "result": True, "work": True})
    assert bad == [], bad
    parts = a.split(clean)
    assert not bool(parts["member"][1].any()) and not bool(parts["result"][1].any())       # ... and those ARE written


# ---- compress + join + unjoin in one HIP graph
def test_three_calls_in_one_hip_graph(engine):
    L = engine.lib
    r = random.Random(12)
    lengths = [4 * r.randint(2, 75) for _ in range(299)] + [297]
    B, bound = len(lengths), 300
    off = offsets_of(lengths_as_blocks(lengths))
    total = off[-1]
    pitch = (out_bound(bound) + 3) & ~3
    d_in = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    in_off = dev(off, np.int64)
    rows = torch.zeros((B, pitch), dtype=torch.uint8, device="cuda")
    out_len, status = (torch.zeros(B, dtype=torch.int32, device="cuda") for _ in range(2))
    bits, joff = torch.zeros(B, dtype=torch.int64, device="cuda"), torch.zeros(B + 1, dtype=torch.int64, device="cuda")
    cap = L.hdlz_join_bound(B, bound)
    z = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    jres, ures = torch.zeros(2, dtype=torch.int64, device="cuda"), torch.zeros(3, dtype=torch.int64, device="cuda")
    jwb, uwb = L.hdlz_join_work_bytes(B), L.hdlz_unjoin_work_bytes(B, total, 0)
    jwork, uwork = torch.zeros(jwb, dtype=torch.uint8, device="cuda"), torch.zeros(uwb, dtype=torch.uint8, device="cuda")
    back = torch.zeros(total, dtype=torch.uint8, device="cuda")

    def calls():
        s = stream_ptr()
        assert L.hdlz_compress_batch_bits(d_in.data_ptr(), in_off.data_ptr(), 0, bound, B, 32, 10, rows.data_ptr(), pitch, out_len.data_ptr(),
                                          status.data_ptr(), bits.data_ptr(), s) == 0, L.hdlz_last_error()
        assert L.hdlz_join_batch_ws(rows.data_ptr(), pitch, out_len.data_ptr(), bits.data_ptr(), status.data_ptr(), in_off.data_ptr(), bound, B,
                                    z.data_ptr(), cap, joff.data_ptr(), jres.data_ptr(), jwork.data_ptr(), jwb, s) == 0, L.hdlz_last_error()
        # (the stream's length is on the device: the capacity is passed, bytes behind the frame are no error)
        assert L.hdlz_unjoin_ws(z.data_ptr(), cap, joff.data_ptr(), in_off.data_ptr(), 0, B, 0, back.data_ptr(), total, None, ures.data_ptr(),
                                uwork.data_ptr(), uwb, s) == 0, L.hdlz_last_error()

    def fresh(seed):
        data = b"".join(blocks_of(lengths, seed=seed, distinct=900))
        d_in[:total] = dev(np.frombuffer(data, np.uint8))
        return data

    def check(label, data):
        torch.cuda.synchronize()
        rec = _lib.UnjoinResult.from_buffer_copy(ures.cpu().numpy().tobytes())
        jr = _lib.JoinResult.from_buffer_copy(jres.cpu().numpy().tobytes())
        assert (rec.status, rec.first_bad, rec.out_len, rec.adler) == (OK, NOBODY, total, zlib.adler32(data)), (label, rec.status, rec.first_bad)
        assert back.cpu().numpy().tobytes() == data, label
        assert jr.status == OK and zlib.decompress(z[:jr.stream_len].cpu().numpy().tobytes()) == data, label

    data = fresh(0)
    calls()
    check("eager", data)
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            calls()
    for launch in range(5):
        data = fresh(100 + launch)
        for t in (rows, z, back, jwork, uwork):
            t.fill_(0xA5 ^ launch)
        for t in (out_len, status, bits, joff, jres, ures):
            t.fill_(-1 - launch)
        g.replay()
        check(("graph", launch), data)


def lengths_as_blocks(lengths):
    return [bytes(n) for n in lengths]


# ---- Engine
def test_engine_round_trip(engine):
    """compress_joined -> inflate_joined(block=...) on 1 MiB + 3 bytes in 4 KiB blocks: 257 members, the tail of 3 bytes shortens the
    block in front of it (chain.plan_blocks), so the output offsets are ragged; inflate_bytes(members=...) on the same stream"""
    n = (1 << 20) + 3
    data = b"".join(family_bytes(1 + k % 4, 1 << 16, seed=30 + k) for k in range(17))[:n]
    d = dev(np.frombuffer(data, np.uint8))
    z, offs = engine.compress_joined(d, block=4096)
    assert offs.numel() == 257 + 1
    for flags in HINTS:
        back = engine.inflate_joined(z, offs, block=4096, total=n, flags=flags)
        assert back.numel() == n and back.cpu().numpy().tobytes() == data, flags
    zb = z.cpu().numpy().tobytes()
    assert zlib.decompress(zb) == data
    assert engine.inflate_bytes(zb, members=(offs, 4096)) == (OK, data)
    assert engine.inflate_bytes(zb, members=(offs.tolist(), 4096), out_cap=n) == (OK, data)
    assert engine.inflate_bytes(flipped(zb, len(zb) - 1, 0x80), members=(offs, 4096)) == (E_BAD_CHECKSUM, b"")
    with pytest.raises(HdlzStatusError) as e:
        engine.inflate_joined(dev(np.frombuffer(flipped(zb, int(offs[100]) - 1, 0x01), np.uint8)), offs, block=4096, total=n)
    assert e.value.status == E_NO_EOF and e.value.first_bad == 99
    # uniform blocks: no offset array at all
    z, offs = engine.compress_joined(d[:1 << 20], block=4096)
    assert engine.inflate_joined(z, offs, block=4096, total=1 << 20).cpu().numpy().tobytes() == data[:1 << 20]
    with pytest.raises(ValueError, match="inflate_bytes"):
        engine.inflate_joined(z, offs, block=1022, total=1 << 20)


def test_it_ran_in_parallel(engine):
    """4 MiB in 2 KiB blocks, 2048 members: inflate_joined against inflate_bytes(z, verify=True) of the same stream, the only way
    back before this call (one serial decoder: the chains for one stream give a joined stream up).  Both timed with HIP events after one
    warm-up.  The factor 5 is the one tests/test_gpu_single_stream.py asserts for the same purpose; expected: hundreds."""
    blocks = blocks_of([2048] * 2048, seed=1, distinct=64)
    j = joined_ref.expected_joined(blocks, 32, 10)
    z, offs = dev(np.frombuffer(j.stream, np.uint8)), dev(j.offsets, np.int64)

    def timed(fn):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), res
    t_new, back = timed(lambda: engine.inflate_joined(z, offs, block=2048, total=len(j.data)))
    assert back.cpu().numpy().tobytes() == j.data
    t_old, (st, old) = timed(lambda: engine.inflate_bytes(j.stream, verify=True))
    assert st == OK and old == j.data
    print("inflate_joined %.3f ms, inflate_bytes(verify=True) %.3f ms: %.1f x" % (t_new, t_old, t_old / t_new))
    assert t_old >= 5 * t_new, (t_old, t_new)
