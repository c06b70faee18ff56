"""GPU (-m gpu): hdlz_inflate_checked -- the decode of hdlz_inflate_batch_ws plus the judging pass (zlib header, Adler-32 of the output
against the trailer, bytes consumed).  Every expectation comes from stock zlib and, for decoder statuses, the CPU oracle
(tests/checked_ref.py): never from the library's own unchecked call."""
import collections
import time
import zlib

import numpy as np
import pytest

import checked_ref as R

pytestmark = pytest.mark.gpu

OK, E_NO_EOF, E_BAD_HEADER, E_BAD_CHECKSUM = R.OK, R.E_NO_EOF, R.E_BAD_HEADER, R.E_BAD_CHECKSUM
HINTS = (0, 2, 4, 64)           # no hint, HDLZ_INFLATE_LANE_PER_STREAM, _WAVE_PER_STREAM, _GROUP_PER_STREAM


def _zfixed(data, level=6):
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 9, zlib.Z_FIXED)
    return co.compress(data) + co.flush()


def _words(n, seed, vocab=4096, wlen=8):
    """n bytes of pseudo-text with matches at every distance (numpy: 16 MiB in a blink)"""
    rng = np.random.default_rng(seed)
    w = rng.integers(97, 123, (vocab, wlen), dtype=np.uint8)
    w[:, -1] = 32
    return w[rng.integers(0, vocab, (n + wlen - 1) // wlen)].tobytes()[:n]


def _flip(z, byte, bit):
    m = bytearray(z)
    m[byte] ^= 1 << bit
    return bytes(m)


def _rejected_flip(z, start, step=-1):
    """the first single-bit flip from byte `start` on (downwards) that stock zlib does not accept: an output-changing bit"""
    for byte in range(start, 2, step):
        for bit in (0, 3, 6):
            m = _flip(z, byte, bit)
            if R.zjudge(m)[0] != "ok":
                return m
    raise AssertionError("no rejected flip")


# ------------------------------------------------------------------------------------------------------------------ 1. damage sweep
def test_damage_sweep_every_mapping(engine, oracle):
    """27 streams x 200 single-bit flips (+ the 27 intact ones) as ragged batches of pitch 4096, once per mapping: the rules of
    checked_ref.expect per stream, and the four mappings agree word for word in all four result arrays"""
    intact, damaged = R.sweep(oracle)
    # the recipe's self-check, before the GPU is asked anything
    counts = collections.Counter((R.zjudge(z)[0], oracle.inflate(z, out_cap=4096)[0] == 0) for z, _ in damaged)
    assert sorted(counts.items()) == R.SWEEP_COUNTS, sorted(counts.items())
    both = damaged + intact
    zs, payloads = [z for z, _ in both], [d for _, d in both]
    exps = [R.expect(oracle, z, 4096, d) for z, d in both]
    assert sum(1 for e in exps if e["status"] is None) == 2          # the two lenient streams: a changed LEN, changed output
    assert all(e["status"] == OK for e in exps[len(damaged):])
    results = []
    for flags in HINTS:
        rows, ol, st, used, ad = R.check_all(("sweep", flags), oracle, engine, zs, 4096, flags=flags, exps=exps)
        results.append((ol, st, used, ad))
    for k in range(1, len(results)):
        for a, b in zip(results[0], results[k]):
            assert np.array_equal(a, b), ("mappings disagree", HINTS[k])


# ------------------------------------------------------------------------------------------------------------------ 2. trailer and slack
def test_cut_trailers_noise_behind_and_members_back_to_back(engine, oracle):
    intact, _ = R.sweep(oracle)
    kinds = intact[:9]              # the text payload: own CWINDOW 32 / 256, zlib level 6 / 1 / 9, Z_FIXED, stored, Huffman only, RLE
    rng = np.random.default_rng(2)
    zs, exps, labels = [], [], []
    cut1_no_eof = 0
    for k, (z, d) in enumerate(kinds):
        for c in (1, 2, 3, 4):
            zc = z[:-c]
            rc = oracle.inflate(zc, out_cap=4096)[0]
            e = R.expect(oracle, zc, 4096, None)
            assert e["status"] != OK
            if rc == OK:                                          # the reference still says OK: the checked call says the trailer is cut
                e = dict(status=E_NO_EOF, out_len=0, in_used=0, adler=0)
                cut1_no_eof += c == 1
            zs.append(zc); exps.append(e); labels.append(("cut", k, c))
        for extra in list(range(1, 41, 3)) + [40]:
            zn = z + rng.integers(0, 256, extra, dtype=np.uint8).tobytes()
            e = R.expect(oracle, zn, 4096, d)
            assert e["status"] == OK and e["in_used"] == len(z)
            zs.append(zn); exps.append(e); labels.append(("noise", k, extra))
        z2 = z + kinds[(k + 1) % len(kinds)][0]
        e = R.expect(oracle, z2, 4096, d)
        assert e["status"] == OK and e["in_used"] == len(z)
        zs.append(z2); exps.append(e); labels.append(("members", k))
    assert cut1_no_eof >= 5                                        # (7 of these 9: the reference lets a lost trailer byte pass, a stored stream two)
    for z, want in ((zlib.compress(b""), 1), (zlib.compress(b"a"), 0x00620062)):
        e = R.expect(oracle, z, 4096, None)
        assert e["status"] == OK and e["adler"] == want
        zs.append(z); exps.append(e); labels.append(("tiny", want))
    for flags in HINTS:
        R.check_all(("trailer", flags), oracle, engine, zs, 4096, flags=flags, exps=exps)


# ------------------------------------------------------------------------------------------------------------------ 3. rows of one pitch
def test_rows_of_one_pitch_slack_is_ignored_damage_is_found(engine):
    import torch
    from hdl_deflate_amd.data import make_blocks
    B = 4096
    d = make_blocks(B, 2048, "cuda", seed=3)
    z, zl, zs = engine.compress_batch(d, cwindow=32, maxmatch=10)
    assert int((zs != 0).sum()) == 0
    hd, hz, hl = d.cpu().numpy(), z.cpu().numpy().copy(), zl.cpu().numpy()
    pitch = hz.shape[1]
    for b in range(0, B, 257):
        assert zlib.decompress(hz[b, :hl[b]].tobytes()) == hd[b].tobytes()
    want_ad = np.array([zlib.adler32(hd[b].tobytes()) for b in range(B)], np.uint32)

    def run(rows):
        o, ol, st, used, ad = engine.inflate_checked(torch.from_numpy(rows).cuda(), out_pitch=2048)
        torch.cuda.synchronize()
        return o.cpu().numpy(), ol.cpu().numpy(), st.cpu().numpy(), used.cpu().numpy(), ad.cpu().numpy().view(np.uint32)
    o, ol, st, used, ad = run(hz)
    assert not st.any() and np.array_equal(used, hl) and np.array_equal(ad, want_ad) and (ol == 2048).all() and np.array_equal(o, hd)
    # one byte changed in the slack of 64 rows (behind the compressor's out_len): nothing changes
    slack = [b for b in range(5, B, 61) if hl[b] + 1 <= pitch][:64]
    assert len(slack) == 64
    h2 = hz.copy()
    for i, b in enumerate(slack):
        h2[b, hl[b] + (i % (pitch - hl[b]))] ^= 0xA5
    r2 = run(h2)
    for a, b in zip((o, ol, st, used, ad), r2):
        assert np.array_equal(a, b)
    # one bit changed inside 64 other rows: exactly those rows are not OK (each flip is one stock zlib rejects)
    hit = [b for b in range(17, B, 59) if b not in slack][:64]
    assert len(hit) == 64
    h3 = hz.copy()
    for i, b in enumerate(hit):
        zb = hz[b, :hl[b]].tobytes()
        m = _rejected_flip(zb, hl[b] - 1 - (i % 3) * (hl[b] // 3))
        h3[b, :hl[b]] = np.frombuffer(m, np.uint8)
    o3, ol3, st3, used3, ad3 = run(h3)
    bad = np.zeros(B, bool)
    bad[hit] = True
    assert np.array_equal(st3 != 0, bad), (np.nonzero((st3 != 0) != bad)[0][:8])
    assert not ol3[bad].any() and np.array_equal(ol3[~bad], ol[~bad]) and np.array_equal(ad3[~bad], ad[~bad])


# ------------------------------------------------------------------------------------------------------------------ 4. default mappings
@pytest.mark.parametrize("nstreams", [65536, 12288, 2000])
def test_default_mapping_by_batch_size(engine, nstreams):
    """ragged Z_FIXED streams of ~2 KiB: a lane per stream above 22 528 streams, 16 lanes per stream for 8192 .. 16 384, a wave per
    stream below: all OK and equal to zlib; then with every 97th stream damaged in its last trailer byte"""
    K = 251
    rng = np.random.default_rng(nstreams)
    payloads = [_words(int(rng.integers(1900, 2049)), 1000 + k, vocab=256, wlen=int(rng.integers(3, 9))) for k in range(K)]
    kinds = [_zfixed(p) for p in payloads]
    ads = np.array([zlib.adler32(p) for p in payloads], np.uint32)
    idx = np.arange(nstreams) % K
    zs = [kinds[i] for i in idx]
    want_len = np.array([len(p) for p in payloads])[idx]
    want_used = np.array([len(z) for z in kinds])[idx]
    rows, ol, st, used, ad = R.run_ragged(engine, zs, 2048)
    assert not st.any() and np.array_equal(ol, want_len) and np.array_equal(used, want_used) and np.array_equal(ad, ads[idx])
    for k in range(K):
        ref = np.frombuffer(payloads[k], np.uint8)
        assert (rows[k::K, :len(ref)] == ref[None, :]).all(), k
    zd = list(zs)
    for b in range(0, nstreams, 97):
        zd[b] = _flip(zd[b], len(zd[b]) - 1, b % 8)
    rows, ol, st, used, ad = R.run_ragged(engine, zd, 2048)
    bad = np.zeros(nstreams, bool)
    bad[::97] = True
    assert (st[bad] == E_BAD_CHECKSUM).all() and not st[~bad].any()
    assert not ol[bad].any() and np.array_equal(used, want_used) and np.array_equal(ad, ads[idx])


# ------------------------------------------------------------------------------------------------------------------ 5. whole-GPU chains
def _one(engine, z, cap, flags=0):
    import torch
    zin = torch.frombuffer(bytearray(z + bytes(64)), dtype=torch.uint8).cuda().reshape(1, -1)
    o, ol, st, used, ad = engine.inflate_checked(zin, in_len=len(z), out_pitch=cap, flags=flags)
    torch.cuda.synchronize()
    return int(st.item()), int(ol.item()), int(used.item()), int(ad.item()) & 0xFFFFFFFF, o


def _timed_checked(engine, z, cap, flags):
    import torch
    zin = torch.frombuffer(bytearray(z + bytes(64)), dtype=torch.uint8).cuda().reshape(1, -1)
    engine.inflate_checked(zin, in_len=len(z), out_pitch=cap, flags=flags)
    best = None
    for _ in range(3):                                         # (best of three: a clock tick of the box must not fail the test)
        torch.cuda.synchronize()
        t0 = time.time()
        engine.inflate_checked(zin, in_len=len(z), out_pitch=cap, flags=flags)
        torch.cuda.synchronize()
        dt = time.time() - t0
        best = dt if best is None else min(best, dt)
    return best


def _timed_wave(engine, z, cap):
    import torch
    zin = torch.frombuffer(bytearray(z + bytes(64)), dtype=torch.uint8).cuda().reshape(1, -1)
    torch.cuda.synchronize()
    t0 = time.time()
    engine.inflate_batch(zin, in_len=len(z), out_pitch=cap, flags=4)        # the yardstick "one wave", nothing is checked against it
    torch.cuda.synchronize()
    return time.time() - t0


def _single_stream_case(engine, oracle, name, z, want, flags=0, timed=False):
    cap = (len(want) + 64 + 15) // 16 * 16
    assert zlib.decompress(z) == want
    st, ol, used, ad, o = _one(engine, z, cap, flags)
    assert (st, ol, used, ad) == (OK, len(want), len(z), zlib.adler32(want)), (name, st, ol, used, hex(ad))
    assert o[0, :ol].cpu().numpy().tobytes() == want, name
    # three noise bytes behind the stream: still OK, and not consumed
    st, ol, used, ad, o = _one(engine, z + b"\x9d\x00\xe7", cap, flags)
    assert (st, ol, used, ad) == (OK, len(want), len(z), zlib.adler32(want)), (name, "noise", st, ol, used)
    # one output-changing bit near the end of the stream body: by the rules of the sweep
    m = _rejected_flip(z, len(z) - 12)
    e = R.expect(oracle, m, cap, want)
    assert e["status"] != OK
    st, ol, used, ad, o = _one(engine, m, cap, flags)
    R.check((name, "flip"), e, st, ol, used, ad, o[0].cpu().numpy())
    if timed:
        t_par, t_wave = _timed_checked(engine, z, cap, flags), _timed_wave(engine, z, cap)
        assert t_par * 5 < t_wave, (name, len(z), t_par, t_wave)


def test_whole_gpu_single_streams(engine, oracle):
    import torch
    from hdl_deflate_amd.data import make_blocks
    n = 16 << 20
    d = make_blocks(n // 2048 + 1, 2048, "cuda", seed=5).reshape(-1)
    out, ol, st = engine.compress_stream(d, n)
    assert int(st.item()) == 0
    own = out[:int(ol.item())].cpu().numpy().tobytes()
    want = d[:n].cpu().numpy().tobytes()
    del d, out
    _single_stream_case(engine, oracle, "16 MiB own stream", own, want, 0, timed=True)
    _single_stream_case(engine, oracle, "16 MiB own stream, ONE_FIXED_BLOCK", own, want, 128)
    text = _words(n, 51)
    _single_stream_case(engine, oracle, "16 MiB zlib level 6", zlib.compress(text, 6), text, 0, timed=True)
    t4 = text[: 4 << 20]
    zf = _zfixed(t4)
    assert (zf[2] & 7) == 2                                        # BFINAL = 0, BTYPE = 01: several fixed blocks
    _single_stream_case(engine, oracle, "4 MiB Z_FIXED, several blocks", zf, t4)
    # a class the chains give up on: memLevel 1 and a sync flush every few hundred bytes -- right whichever path ends up taking it
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 1)
    t5 = text[:300000]
    parts = []
    for k in range(0, len(t5), 300):
        parts.append(co.compress(t5[k:k + 300]) + co.flush(zlib.Z_SYNC_FLUSH))
    _single_stream_case(engine, oracle, "memLevel 1 + sync flushes", b"".join(parts) + co.flush(), t5)
    torch.cuda.empty_cache()


def test_whole_gpu_batch_256_rows_of_1_mib(engine, oracle):
    import torch
    kinds = [_words(1 << 20, 60 + k) for k in range(8)]
    zk = [zlib.compress(t, 6) for t in kinds]
    B = 256
    pitch = (max(len(z) for z in zk) + 64 + 15) // 16 * 16
    host = np.zeros((B, pitch), np.uint8)
    flipped = {}
    for b in range(B):
        z = zk[b % 8]
        if b % 37 == 5:                                            # a few damaged rows among the good ones
            z = _rejected_flip(z, len(z) - 12 - b)
            flipped[b] = z
        host[b, :len(z)] = np.frombuffer(z, np.uint8)
    cap = (1 << 20) + 64
    o, ol, st, used, ad = engine.inflate_checked(torch.from_numpy(host).cuda(), out_pitch=cap)
    torch.cuda.synchronize()
    ol, st, used, ad = ol.cpu().numpy(), st.cpu().numpy(), used.cpu().numpy(), ad.cpu().numpy().view(np.uint32)
    for b in range(B):
        if b in flipped:
            e = R.expect(oracle, host[b].tobytes(), cap, kinds[b % 8])
            assert e["status"] != OK
            R.check(("256 x 1 MiB", b), e, st[b], ol[b], used[b], ad[b], None)
        else:
            assert (st[b], ol[b], used[b], ad[b]) == (OK, 1 << 20, len(zk[b % 8]), zlib.adler32(kinds[b % 8])), b
    for b in (0, 7, 100, 255):
        assert o[b, : 1 << 20].cpu().numpy().tobytes() == kinds[b % 8]
    del o
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------ 6. odd shapes
def _ff_mix(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, n, dtype=np.uint8)
    a[rng.random(n) < 0.5] = 0xFF
    return a.tobytes()


@pytest.mark.parametrize("pitch,phase", [(16660, 4), (16656, 0), (65556, 4), (65584, 0), (72228, 12)])
def test_unaligned_rows_and_the_lengths_a_lazy_modulo_gets_wrong(engine, pitch, phase):
    """out_pitch % 16 == 4 with a d_out that is 4-byte but not 16-byte aligned (and the aligned twins); output lengths 0, 1, 15, 16, 17,
    5552 k +- 1, 65 521, 65 522, the pitch itself -- rows below 64 KiB (16 lanes per row) and above (tiles)"""
    import torch
    lens = [0, 1, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097]
    for k in (1, 2, 3, 5, 11, 12, 13):
        lens += [5552 * k - 1, 5552 * k, 5552 * k + 1]
    lens += [32767, 32768, 32769, 65519, 65520, 65521, 65522, 65535, 65536, 65537, pitch - 1, pitch]
    lens = sorted(set(n for n in lens if n <= pitch))
    payloads = [bytes([0xFF]) * n if k % 3 == 0 else _ff_mix(n, k) for k, n in enumerate(lens)]
    zs = [zlib.compress(p, 1) for p in payloads]
    B = len(zs)
    raw = torch.full((B * pitch + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    skip = (phase - raw.data_ptr()) % 16
    out = raw[skip:skip + B * pitch].view(B, pitch)
    assert out.data_ptr() % 16 == phase
    for flags in (0, 2):
        rows, ol, st, used, ad = R.run_ragged(engine, zs, pitch, flags=flags, out=out)
        for k, p in enumerate(payloads):
            assert (st[k], ol[k], used[k], ad[k]) == (OK, len(p), len(zs[k]), zlib.adler32(p)), (flags, k, len(p), int(st[k]), hex(int(ad[k])))
            assert rows[k, :len(p)].tobytes() == p


def test_the_largest_sums_16_mib_of_ff(engine):
    n = (1 << 24) - 5
    p = bytes([0xFF]) * n
    z = zlib.compress(p, 6)
    st, ol, used, ad, o = _one(engine, z, 1 << 24)
    assert (st, ol, used, ad) == (OK, n, len(z), zlib.adler32(p)), (st, ol, used, hex(ad))
    zr = zlib.compress(_ff_mix(n, 9), 1)
    st, ol, used, ad, o = _one(engine, zr, 1 << 24)
    assert (st, ol, used, ad) == (OK, n, len(zr), zlib.adler32(_ff_mix(n, 9))), (st, ol, used, hex(ad))


# ------------------------------------------------------------------------------------------------------------------ 7. graph
def test_checked_call_inside_a_hip_graph_verdicts_follow_the_inputs(engine):
    import torch
    text = _words(1 << 20, 70)
    z1 = zlib.compress(text, 6)
    z1_bad = _rejected_flip(z1, len(z1) - 12)
    K, B = 64, 4096
    payloads = [_words(2000 + k, 700 + k, vocab=256, wlen=5) for k in range(K)]
    kinds = [_zfixed(p) for p in payloads]
    zs = [kinds[b % K] for b in range(B)]
    zs_bad = list(zs)
    for b in range(3, B, 41):
        zs_bad[b] = _flip(zs_bad[b], len(zs_bad[b]) - 2, b % 8)
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum([len(z) for z in zs])]).astype(np.int64)).cuda()

    def dev(b):
        return torch.from_numpy(np.frombuffer(b + bytes(64), np.uint8).copy()).cuda()
    one_good, one_bad = dev(z1).reshape(1, -1), dev(z1_bad).reshape(1, -1)
    many_good, many_bad = dev(b"".join(zs)), dev(b"".join(zs_bad))
    in1, inb = one_good.clone(), many_good.clone()
    cap1 = (1 << 20) + 64
    out1 = torch.empty((1, cap1), dtype=torch.uint8, device="cuda")
    outb = torch.empty((B, 2112), dtype=torch.uint8, device="cuda")
    L = engine.lib
    w1 = torch.empty(L.hdlz_inflate_checked_work_bytes(1, len(z1), cap1, 0, 0), dtype=torch.uint8, device="cuda")
    wb = torch.empty(L.hdlz_inflate_checked_work_bytes(B, 0, 2112, 0, 1), dtype=torch.uint8, device="cuda")
    engine.inflate_checked(in1, in_len=len(z1), out_pitch=cap1, out=out1, work=w1)
    engine.inflate_checked(inb, in_off=offs, out_pitch=2112, out=outb, work=wb)
    torch.cuda.synchronize()
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            r1 = engine.inflate_checked(in1, in_len=len(z1), out_pitch=cap1, out=out1, work=w1)
            rb = engine.inflate_checked(inb, in_off=offs, out_pitch=2112, out=outb, work=wb)
    want_ad = np.array([zlib.adler32(payloads[b % K]) for b in range(B)], np.uint32)
    bad_rows = np.zeros(B, bool)
    bad_rows[3::41] = True
    for launch in range(10):
        bad1, badb = launch % 2 == 1, launch % 3 == 1
        in1.copy_(one_bad if bad1 else one_good)
        inb.copy_(many_bad if badb else many_good)
        out1.zero_(); outb.zero_(); w1.fill_(0x5A); wb.fill_(0x5A)
        g.replay()
        torch.cuda.synchronize()
        st1, ol1, used1, ad1 = int(r1[2].item()), int(r1[1].item()), int(r1[3].item()), int(r1[4].item()) & 0xFFFFFFFF
        if bad1:
            assert st1 != OK and ol1 == 0, (launch, st1)
        else:
            assert (st1, ol1, used1, ad1) == (OK, 1 << 20, len(z1), zlib.adler32(text)), (launch, st1, ol1, used1)
            assert out1[0, : 1 << 20].cpu().numpy().tobytes() == text
        st, ol, ad = rb[2].cpu().numpy(), rb[1].cpu().numpy(), rb[4].cpu().numpy().view(np.uint32)
        if badb:
            assert (st[bad_rows] == E_BAD_CHECKSUM).all() and not st[~bad_rows].any() and not ol[bad_rows].any(), launch
        else:
            assert not st.any(), launch
        assert np.array_equal(ad, want_ad), launch
