"""GPU (-m gpu): hdlz_gunzip_ws / Engine.inflate_gzip / Engine.inflate_gzip_bytes -- gzip members of any writer, one per stream.

The cases are those of tests/gunzip_ref.py (built on the CPU with zlib and hand-made headers, fixed seeds); what every stream must
answer is gunzip_ref.member, the rule of include/hdlz_gunzip.h in Python, which tests/test_gunzip_cabi.py holds against stock zlib on
the same cases.  Every case runs through both decode routes: as one of many (the member view of the wave-per-stream decoder) and
alone in its call (the batch call's path)."""
import gzip
import time
import zlib

import numpy as np
import pytest

import gunzip_ref as G

pytestmark = pytest.mark.gpu

P_ROWS, P_TILES = 65532, 131072          # a workgroup per row below 64 KiB of capacity; 32 KiB tiles from there on


def _padded(zs):
    n = max(len(z) for z in zs)
    return [z + b"\xAA" * (n - len(z)) for z in zs]


def _batch(engine, oracle, label, cases, pitch, ragged=True):
    """one call over all the cases, every stream held to the rule -> the five results"""
    zs = [z for _, z in cases]
    res = G.run(engine, zs, pitch, ragged)
    seen = zs if ragged else _padded(zs)          # (rows of one pitch: what stands behind a stream belongs to it)
    for k, (name, _) in enumerate(cases):
        G.check((label, name), G.expect(oracle, seen[k], pitch), res[2][k], res[1][k], res[3][k], res[4][k], res[0][k])
    return res


def _alone(engine, oracle, label, cases, pitch):
    """every case alone in its call (nstreams = 1), pitched: the stream is the row"""
    for name, z in cases:
        if len(z) == 0:
            continue                              # (a row of no bytes has no address)
        rows, ol, st, used, crc = G.run(engine, [z], pitch, ragged=False)
        G.check((label, name, "alone"), G.expect(oracle, z, pitch), st[0], ol[0], used[0], crc[0], rows[0])


def test_header_walk_ragged(engine, oracle):
    """no flags, each flag alone, all four, XLEN 0 and 65535, a 300-byte name, the payload at every alignment mod 16, FHCRC right and
    wrong by a bit, reserved flag bits, CM = 7, wrong magic, a header cut at every byte, an unterminated name, XLEN past the end, the
    20-byte file of gzip.compress(b"")"""
    cases = G.header_cases()
    res = _batch(engine, oracle, "ragged", cases, P_ROWS)
    st = dict(zip([n for n, _ in cases], res[2]))
    assert all(st["payload at %d mod 16" % a] == G.OK for a in range(16)) and st["all four"] == G.OK and st["XLEN 65535 FHCRC"] == G.OK
    assert st["FHCRC wrong by bit 0"] == st["reserved flag 0x20"] == st["CM = 7"] == st["wrong magic"] == G.E_BAD_HEADER
    assert st["unterminated name"] == st["XLEN past the end"] == st["cut at 9"] == st["cut at 27"] == G.E_NO_EOF
    assert st["gzip.compress(b\"\")"] == G.OK


def test_header_walk_pitched(engine, oracle):
    _batch(engine, oracle, "pitched", G.header_cases(), P_ROWS, ragged=False)


def test_payloads_and_trailers(engine, oracle):
    """stored, fixed, dynamic (levels 1, 6, 9), several blocks, a full flush in the middle; the trailer cut at end + 7, + 4, + 3, one
    bit of the CRC word, ISIZE off by 1 and by 2^20, a second member behind the first, and the failed streams' neighbours exact"""
    cases = G.payload_cases() + G.trailer_cases()
    for ragged in (False, True):
        rows, ol, st, used, crc = _batch(engine, oracle, "ragged" if ragged else "pitched", cases, P_ROWS, ragged)
    names = [n for n, _ in cases]
    k = names.index("a second member behind")
    first = G.trailer_cases()[-1][1]
    assert st[k] == G.OK and used[k] == len(first) and cases[k][1][used[k]:used[k] + 3] == b"\x1f\x8b\x08"
    for name in ("cut at end + 7", "cut at end + 4", "cut at end + 3"):
        assert st[names.index(name)] == G.E_NO_EOF and used[names.index(name)] == 0 and crc[names.index(name)] == 0
    for name in ("CRC bit 0", "ISIZE + 1", "ISIZE + 2^20"):
        j = names.index(name)
        assert st[j] == G.E_BAD_CHECKSUM and ol[j] == 0 and used[j] == len(first) and crc[j] == zlib.crc32(G.text(5000, 6))


def _lengths(engine, oracle, lengths, pitch):
    zs = G.lengths_case(lengths + [pitch, pitch + 1])          # exactly at capacity, and a byte over
    cases = [("%d bytes" % n, z) for n, z in zip(lengths + [pitch, pitch + 1], zs)]
    for ragged in (True, False):
        rows, ol, st, used, crc = _batch(engine, oracle, ("lengths", pitch), cases, pitch, ragged)
        assert list(ol) == lengths + [pitch, 0] and list(st) == [G.OK] * (len(lengths) + 1) + [G.E_OUT_CAPACITY]
    _alone(engine, oracle, ("lengths", pitch), cases, pitch)


def test_output_lengths_a_workgroup_per_row(engine, oracle):
    _lengths(engine, oracle, [0, 1, 127, 128, 129, 32767, 32768, 32769, 65531], P_ROWS)


def test_output_lengths_in_tiles(engine, oracle):
    _lengths(engine, oracle, [0, 1, 32768, 32769, 65537, 131071], P_TILES)


def test_every_case_alone_in_its_call(engine, oracle):
    """nstreams = 1 takes the batch call's path: the same cases, the same answers"""
    _alone(engine, oracle, "rows", G.all_cases(), P_ROWS)
    _alone(engine, oracle, "tiles", G.payload_cases() + G.trailer_cases(), P_TILES)


def test_alone_and_as_one_of_65(engine, oracle):
    """the same stream alone in a call and as one of 65 gives the same five result words and the same bytes (the two routes count
    the end of the final block differently: a byte there, a bit here)"""
    hdr, pay, tr = dict(G.header_cases()), dict(G.payload_cases()), dict(G.trailer_cases())
    picks = [hdr["payload at 11 mod 16"], hdr["all four"], pay["level 9"], pay["full flush"], pay["stored"], tr["a second member behind"],
             tr["CRC bit 31"], tr["cut at end + 4"], hdr["FHCRC wrong by bit 15"], hdr["gzip.compress(b\"\")"]]
    filler = [G.gz(G.text(100 + 37 * k, 40 + k), name=b"f" * (k % 7)) for k in range(65)]
    for j, z in enumerate(picks):
        at = (0, 64, 17)[j % 3]
        zs = filler[:at] + [z] + filler[at + 1:]
        many = G.run(engine, zs, P_ROWS)
        one = G.run(engine, [z], P_ROWS)
        five_many, five_one = [int(a[at]) for a in many[1:]], [int(a[0]) for a in one[1:]]
        assert five_many == five_one, (j, five_many, five_one)
        n = five_one[0]
        assert bytes(many[0][at][:n]) == bytes(one[0][0][:n])
        e = G.expect(oracle, z, P_ROWS)
        G.check((j, "one of 65"), e, many[2][at], many[1][at], many[3][at], many[4][at], many[0][at])
        for k in (at - 1, at + 1):                              # the neighbours of a failed stream are exact
            if 0 <= k < 65:
                G.check((j, "neighbour", k), G.expect(oracle, zs[k], P_ROWS), many[2][k], many[1][k], many[3][k], many[4][k], many[0][k])


def test_a_4_mib_member_takes_the_whole_gpu(engine, oracle):
    """one 4 MiB level-6 member with an FNAME header (an odd payload offset), alone in the call: the bytes and the CRC are right, and --
    the whole-GPU chains ran -- it takes at most 1/5 of the time of hdlz_inflate_checked with HDLZ_INFLATE_WAVE_PER_STREAM on the same
    payload in zlib framing (the factor tests/test_gpu_single_stream.py uses for the same purpose)"""
    import torch
    data = G.text(4 << 20, 77)
    raw = G.deflate(data, 6)
    z = G.header(name=b"four.bin") + raw + G.trailer(data)
    assert G.walk(z) == (G.OK, 19)
    zz = b"\x78\x9c" + raw + zlib.adler32(data).to_bytes(4, "big")
    cap = (4 << 20) + 64
    zin = torch.frombuffer(bytearray(z + bytes(64)), dtype=torch.uint8).cuda().reshape(1, -1)
    zzin = torch.frombuffer(bytearray(zz + bytes(64)), dtype=torch.uint8).cuda().reshape(1, -1)
    out, ol, st, used, crc = engine.inflate_gzip(zin, in_len=len(z), out_pitch=cap)
    torch.cuda.synchronize()
    assert (int(st[0]), int(ol[0]), int(used[0]), int(crc[0]) & 0xFFFFFFFF) == (G.OK, len(data), len(z), zlib.crc32(data))
    assert out[0, :len(data)].cpu().numpy().tobytes() == data

    def timed(fn, reps):
        best = None
        for _ in range(reps):                                   # (best of three: a clock tick of the box must not fail the test)
            torch.cuda.synchronize()
            t0 = time.time()
            fn()
            torch.cuda.synchronize()
            best = time.time() - t0 if best is None else min(best, time.time() - t0)
        return best
    t_gz = timed(lambda: engine.inflate_gzip(zin, in_len=len(z), out_pitch=cap), 3)
    res = []
    t_wave = timed(lambda: res.append(engine.inflate_checked(zzin, in_len=len(zz), out_pitch=cap, flags=4)), 1)
    assert int(res[0][2][0]) == G.OK and int(res[0][1][0]) == len(data)
    print("4 MiB member: hdlz_gunzip_ws %.3f ms, hdlz_inflate_checked (wave per stream) %.3f ms" % (t_gz * 1e3, t_wave * 1e3))
    assert t_gz * 5 <= t_wave, (t_gz, t_wave)


def test_inflate_gzip_bytes_reads_files_as_gzip_decompress_does(engine):
    a, b, c = G.text(70000, 50), G.text(300, 51), G.text(2000000, 52)
    one = gzip.compress(a)
    three = G.gz(a, name=b"a.txt") + gzip.compress(b, 1) + G.gz(c, level=1, hcrc=True, comment=b"third")
    for z in (one, three, three + bytes(13), one + bytes(1), gzip.compress(b"") + gzip.compress(b)):
        assert engine.inflate_gzip_bytes(z) == (G.OK, gzip.decompress(z))
    assert engine.inflate_gzip_bytes(b"") == (G.OK, b"") and gzip.decompress(b"") == b""
    for z in (one + b"garbage behind the member", three + b"\x00\x00x", one + b"ab", one + b"\x1f"[:1] + b"\x00"):
        with pytest.raises(Exception):
            gzip.decompress(z)
        assert engine.inflate_gzip_bytes(z) == (G.E_BAD_HEADER, b"")
    assert engine.inflate_gzip_bytes(one[:-1]) == (G.E_NO_EOF, b"")
    bad = bytearray(three); bad[-6] ^= 4
    assert engine.inflate_gzip_bytes(bytes(bad)) == (G.E_BAD_CHECKSUM, b"")
    assert engine.inflate_gzip_bytes(one, out_cap=70000) == (G.OK, a) and engine.inflate_gzip_bytes(one, out_cap=69984) == (G.E_OUT_CAPACITY, b"")


def test_inflate_gzip_with_the_callers_buffers(engine, oracle):
    import torch
    cases = G.payload_cases()[:6]
    zs = [z for _, z in cases]
    L = engine.lib
    for pitch in (P_ROWS, P_TILES):
        need = L.hdlz_gunzip_work_bytes(len(zs), max(len(z) for z in zs), pitch, 1)
        out = torch.full((len(zs), pitch), 0x5A, dtype=torch.uint8, device="cuda")
        work = torch.full((need + 512,), 0xA5, dtype=torch.uint8, device="cuda")
        res = G.run(engine, zs, pitch, out=out, work=work[:need])
        assert bool((work[need:] == 0xA5).all())
        for k, (name, z) in enumerate(cases):
            G.check(name, G.expect(oracle, z, pitch), res[2][k], res[1][k], res[3][k], res[4][k], res[0][k])
            assert bool((out[k, int(res[1][k]):] == 0x5A).all()), (name, "bytes behind out_len were written")
        with pytest.raises(AssertionError):
            engine.inflate_gzip(torch.zeros((2, 64), dtype=torch.uint8, device="cuda"), out_pitch=pitch, work=work[:256])


def test_the_call_is_hip_graph_capturable(engine, oracle):
    """both routes with caller scratch captured into ONE HIP graph (the pattern of test_calls_are_hip_graph_capturable) and launched a
    few times on new data in the same buffers: nothing is allocated, the host reads nothing in between"""
    import torch
    L = engine.lib
    sets = [[G.gz(G.text(3000 + 500 * k, 60 + 10 * s + k), level=(1, 6, 9)[k % 3], name=b"g" * k) for k in range(5)] for s in range(3)]
    bigs = [G.gz(G.text(300000, 90 + s), name=b"big", hcrc=True) for s in range(3)]
    n_small, n_big = max(len(z) for zs in sets for z in zs), max(len(z) for z in bigs)
    rows = torch.zeros((5, n_small), dtype=torch.uint8, device="cuda")
    big = torch.zeros((1, n_big), dtype=torch.uint8, device="cuda")
    out = torch.empty((5, 8192), dtype=torch.uint8, device="cuda")
    bout = torch.empty((1, 300032), dtype=torch.uint8, device="cuda")
    work = torch.empty(L.hdlz_gunzip_work_bytes(5, n_small, 8192, 0), dtype=torch.uint8, device="cuda")
    bwork = torch.empty(L.hdlz_gunzip_work_bytes(1, n_big, 300032, 0), dtype=torch.uint8, device="cuda")

    def load(s):
        host = np.full((5, n_small), 0xAA, np.uint8)
        for k, z in enumerate(sets[s]):
            host[k, :len(z)] = np.frombuffer(z, np.uint8)
        rows.copy_(torch.from_numpy(host))
        hb = np.full((1, n_big), 0xAA, np.uint8)
        hb[0, :len(bigs[s])] = np.frombuffer(bigs[s], np.uint8)
        big.copy_(torch.from_numpy(hb))
    load(0)
    engine.inflate_gzip(rows, out_pitch=8192, out=out, work=work)         # eager once
    engine.inflate_gzip(big, out_pitch=300032, out=bout, work=bwork)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            r1 = engine.inflate_gzip(rows, out_pitch=8192, out=out, work=work)
            r2 = engine.inflate_gzip(big, out_pitch=300032, out=bout, work=bwork)
    for k in (1, 2, 0, 1):
        load(k)
        out.zero_(); bout.zero_()
        g.replay()
        torch.cuda.synchronize()
        pad = lambda z, n: z + b"\xAA" * (n - len(z))
        for j, z in enumerate(sets[k]):
            G.check(("graph", k, j), G.expect(oracle, pad(z, n_small), 8192), r1[2][j].item(), r1[1][j].item(), r1[3][j].item(), r1[4][j].item(),
                    out[j].cpu().numpy())
        G.check(("graph", k, "big"), G.expect(oracle, pad(bigs[k], n_big), 300032), r2[2][0].item(), r2[1][0].item(), r2[3][0].item(), r2[4][0].item(),
                bout[0].cpu().numpy())
        assert int(r2[2][0].item()) == G.OK and int(r2[1][0].item()) == 300000
