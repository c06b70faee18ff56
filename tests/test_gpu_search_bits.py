"""GPU (-m gpu): the bit-sliced match search of the one-tile kernel (match_search_bits, hdlz_compress_common.h) against the oracle.

The search keeps a lane's 32 bytes as 8 bit planes, takes the previous lane's planes by a DPP rotate (lane 0 gets lane 63's: whatever
they "match" lies in front of the block and must be rejected), the next lane's byte-equality bits for the 3-byte strings that straddle
the end of a run, and walks the distances 1..32 nearest first.  Every block below goes through k_compress<1, ., true> (a ragged batch
with a stated bound of 2048 bytes: the one-tile kernel whatever the lengths) and is compared with the oracle, at CWINDOW 32, 16 and 31,
with MATCH10 on and off.  The same file runs against lib/libhdlz_keys.so (the key-difference search, -DHDLZ_SEARCH_KEYS) in a
subprocess: both searches give the oracle's streams."""
import os
import random
import subprocess
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = os.path.join(REPO, "hdl_deflate_amd", "lib", "libhdlz_keys.so")
WINDOWS = [(32, 10), (32, 5), (16, 10), (16, 5), (31, 10), (31, 5)]


def _one_tile(torch, engine, blocks, cw, mm):
    """the blocks as ONE ragged batch whose stated bound (2048) sends it through the one-tile kernel"""
    flat = b"".join(blocks) + bytes(64)
    off = np.cumsum([0] + [len(b) for b in blocks]).astype(np.int64)
    d_in = torch.frombuffer(bytearray(flat), dtype=torch.uint8).cuda()
    out, ol, st = engine.compress_batch(d_in, in_off=torch.from_numpy(off).cuda(), cwindow=cw, maxmatch=mm, max_len=2048)
    torch.cuda.synchronize()
    out, ol, st = out.cpu().numpy(), ol.cpu().numpy(), st.cpu().numpy()
    return [bytes(out[b, :ol[b]].tobytes()) for b in range(len(blocks))], st


def _check(engine, oracle, blocks):
    import torch
    assert all(5 <= len(b) <= 2048 for b in blocks)
    for cw, mm in WINDOWS:
        got, st = _one_tile(torch, engine, blocks, cw, mm)
        for k, b in enumerate(blocks):
            rc, ref = oracle.compress(b, cwindow=cw, maxmatch=mm)
            assert st[k] == rc == 0 and got[k] == ref, (cw, mm, k, len(b))
        assert zlib.decompress(got[0]) == blocks[0]


def _noise(r, n):
    """random bytes: a chance 3-byte repeat within 32 positions is about one in 2^19 per position"""
    return bytearray(r.getrandbits(8) for _ in range(n))


def test_search_bits_periodic_blocks(engine, oracle):
    """every period 1..40 (33..40: no match inside the window but chance ones), whole tiles and shorter blocks behind a random head"""
    r = random.Random(701)
    blocks = []
    for per in range(1, 41):
        pat = bytes(r.getrandbits(8) for _ in range(per))
        blocks.append((pat * (2048 // per + 1))[:2048])
        n = 1000 + 25 * per
        blocks.append((bytes(r.getrandbits(8) for _ in range(per + 5)) + pat * (n // per + 1))[:n])
    _check(engine, oracle, blocks)


def test_search_bits_lone_repeats_at_the_window_edge(engine, oracle):
    """one repeat of 3..12 bytes at distance exactly 32 (inside a 32-byte window) and 33 (never), and a few near ones, at many places"""
    r = random.Random(702)
    blocks = []
    for dist in (32, 33, 31, 1, 2, 3):
        for ln in (3, 4, 10, 12):
            for p in (33, 63, 64, 95, 100, 1023, 1024, 2015, 2030, 2040):
                b = _noise(r, 2048)
                if p + ln <= 2048:
                    b[p:p + ln] = b[p - dist:p - dist + ln]
                blocks.append(bytes(b))
    _check(engine, oracle, blocks)


def test_search_bits_candidates_in_the_previous_run(engine, oracle):
    """a match at own position i (0..31) of a run whose candidate lies in the PREVIOUS lane's run (d > i), for every i and the nearest,
    a middle and the farthest such distance; lanes 1, 31 and 63 -- and lane 0, whose "previous run" is lane 63's (what the rotate feeds
    it): its bytes made equal to the string, a match in front of the block that must be rejected"""
    r = random.Random(703)
    blocks = []
    for lane in (0, 1, 31, 63):
        for i in range(32):
            p = 32 * lane + i
            if p + 4 > 2048:
                continue
            for d in sorted({i + 1, min(i + 7, 32), 32}):
                b = _noise(r, 2048)
                if p - d >= 0:
                    b[p:p + 4] = b[p - d:p - d + 4]
                elif 2048 + p - d + 4 <= 2048:
                    b[2048 + p - d:2048 + p - d + 4] = b[p:p + 4]
                blocks.append(bytes(b))
    _check(engine, oracle, blocks)


def test_search_bits_strings_across_a_run_boundary(engine, oracle):
    """3-byte strings at own positions 29..31 (the last bytes belong to the next lane's run), candidates inside the run and in the
    previous one; then the byte in the next run changed (no match there) and an exact copy at distance 32"""
    r = random.Random(704)
    blocks = []
    for lane in (0, 5, 62, 63):
        for i in (29, 30, 31):
            p = 32 * lane + i
            if p + 3 > 2048:
                continue
            for d in (1, 2, 3, 5, 17, 29, 30, 31, 32):
                if p - d < 0:
                    continue
                b = _noise(r, 2048)
                b[p:p + 3] = b[p - d:p - d + 3]
                blocks.append(bytes(b))
                b[p + 2] ^= 0x40
                if p >= 32:
                    b[p - 32:p - 29] = b[p:p + 3]
                blocks.append(bytes(b))
    _check(engine, oracle, blocks)


def test_search_bits_one_bit_plane_differs(engine, oracle):
    """candidates that differ from the own string in ONE bit of ONE byte (bit plane b = 0..7, byte 0..2 of the string): no match there,
    a farther exact one wins; and blocks of zeros with one bit plane set in every third byte"""
    r = random.Random(705)
    blocks = []
    for bit in range(8):
        for which in range(3):
            b = _noise(r, 2048)
            for p in range(40 + bit, 2000, 97):
                near, far = 3 + (p % 11), 20 + (p % 13)
                b[p:p + 3] = b[p - far:p - far + 3]
                b[p - near:p - near + 3] = b[p:p + 3]
                b[p - near + which] ^= 1 << bit
            blocks.append(bytes(b))
            blocks.append(bytes((1 << bit) if k % 3 == which else 0 for k in range(2048)))
    _check(engine, oracle, blocks)


def test_search_bits_constant_blocks_and_lengths(engine, oracle):
    """all-0x00 and all-0xFF blocks, and block lengths 5..2048 -- many of them ending inside a lane's run -- of small-alphabet text,
    a period of 13 and noise"""
    r = random.Random(706)
    text = bytes(r.choice(b"etaoin shrdlu") for _ in range(2048))
    per = (bytes(r.getrandbits(8) for _ in range(13)) * 160)[:2048]
    noise = bytes(_noise(r, 2048))
    blocks = []
    for n in (2048, 2047, 1025, 64, 33, 32, 31, 5):
        blocks.append(bytes(n))
        blocks.append(bytes([0xFF]) * n)
    lens = sorted(set(list(range(5, 80)) + list(range(80, 2049, 29)) + [2016 + k for k in range(33)] + [1022, 1023, 1024, 1025, 1026]))
    for n in lens:
        blocks.append(text[:n])
        blocks.append(per[2048 - n:])
        blocks.append(noise[:n])
    _check(engine, oracle, blocks)


def test_search_bits_agrees_with_the_key_search():
    """the tests above against lib/libhdlz_keys.so (the key-difference search, built with -DHDLZ_SEARCH_KEYS), in a subprocess"""
    assert os.path.exists(KEYS), "lib/libhdlz_keys.so is not built: hdl_deflate_amd/csrc/build.sh keys"
    env = dict(os.environ, HDLZ_LIB=KEYS)
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_search_bits.py", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "not agrees_with_the_key_search"], cwd=REPO, env=env, capture_output=True, text=True, timeout=1200)
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    assert r.returncode == 0, tail
    assert "6 passed" in r.stdout and " failed" not in r.stdout, tail
