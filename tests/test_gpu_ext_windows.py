"""GPU (-m gpu): the lane-private candidate windows of the one-tile kernel (copy_windows / WaveLdsWin, hdlz_compress_common.h).

k_compress<1, ., true> copies, per lane, the 19 dwords [32 l - 32, 32 l + 44) of the staged tile into a window of its own at a 19-dword
stride; the extension gathers from there, the search and the Adler sums take the own bytes from the copy's registers, and the bit buffer
overlays the windows once the extension is through.  What can go wrong is a window that is off by a dword, a lane edge (lane 0's zero
halo, lane 63's look-ahead, the lane a short block ends in), a gather that leaves its window, and a bit buffer that is zeroed too early
or too late.  Every block below goes through the one-tile kernel (a ragged batch with a stated bound of 2048, or fixed pitch above 1024
bytes) and is compared with the C oracle on bytes, length and status, at CWINDOW 32, 31 and 20 (both instantiations) and MAXMATCH 10 and
5; the same file runs against lib/libhdlz_keys.so (the key search, which keeps the shared layout and its masked gather) in a subprocess.
The oracle's stream of a (block, cwindow, maxmatch) is computed once per process."""
import os
import random
import subprocess
import sys
import zlib

import numpy as np
import pytest

import test_gpu_containment as containment      # the guarded hdlz_compress_batch call (tests/guards.py) -- helpers only

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = os.path.join(REPO, "hdl_deflate_amd", "lib", "libhdlz_keys.so")
PARAMS = [(32, 10), (32, 5), (31, 10), (31, 5), (20, 10), (20, 5)]
# lane edges (32, 64), the 12 look-ahead bytes of the lane a block ends in (33 .. 45: 32 + 1 .. 32 + 13; 76, 77: the window's own size),
# the smallest blocks (5, 6), the first size that is not packed (1025), the last lane's edges and its look-ahead (2015 .. 2048)
SIZES = [5, 6, 33, 34, 44, 45, 63, 64, 65, 76, 77, 1025, 2015, 2016, 2017, 2047, 2048]
DEFECTS = list(range(12)) + [29, 30, 31]
_ref = {}


def _expect(oracle, blk, cw, mm):
    key = (blk, cw, mm)
    if key not in _ref:
        _ref[key] = oracle.compress(blk, cwindow=cw, maxmatch=mm)
    return _ref[key]


def _compare(oracle, blocks, cw, mm, out, ol, st, label):
    out, ol, st = out.cpu().numpy(), ol.cpu().numpy(), st.cpu().numpy()
    for k, b in enumerate(blocks):
        rc, ref = _expect(oracle, b, cw, mm)
        assert rc == 0 and st[k] == 0 and ol[k] == len(ref) and out[k, :ol[k]].tobytes() == ref, (label, cw, mm, k, len(b))
    assert zlib.decompress(out[0, :ol[0]].tobytes()) == blocks[0]


def _check_ragged(engine, oracle, blocks, label, params=PARAMS):
    """the blocks as ONE ragged batch whose stated bound (2048 > 1024) sends every size through the one-tile kernel"""
    import torch
    assert len(blocks) <= 4096 and all(5 <= len(b) <= 2048 for b in blocks)
    flat = b"".join(blocks) + bytes(64)
    off = np.cumsum([0] + [len(b) for b in blocks]).astype(np.int64)
    d_in = torch.frombuffer(bytearray(flat), dtype=torch.uint8).cuda()
    d_off = torch.from_numpy(off).cuda()
    for cw, mm in params:
        out, ol, st = engine.compress_batch(d_in, in_off=d_off, cwindow=cw, maxmatch=mm, max_len=2048)
        torch.cuda.synchronize()
        _compare(oracle, blocks, cw, mm, out, ol, st, label)


def _periodic(r, per, n):
    pat = bytes(r.getrandbits(8) for _ in range(per))
    return bytearray((pat * (n // per + 1))[:n])


def _alphabet(r, k, n):
    return bytes(r.randrange(k) if k < 256 else r.getrandbits(8) for _ in range(n))


def test_ext_windows_periodic_with_one_defect(engine, oracle):
    """periods 1 .. 32 (a candidate at every distance, the same in every lane: the conflict-free gather) and 33, 40 (none inside the
    window), one byte changed at 32 k + j, j = 0 .. 11 (inside the look-ahead of lane k - 1's last positions) and 29 .. 31: the matches in
    front of it are cut to every length 3 .. 10 across the lane boundary, the ones behind it start with their candidate in lane k - 1"""
    r = random.Random(811)
    blocks = []
    for per in list(range(1, 33)) + [33, 40]:
        for j in DEFECTS:
            b = _periodic(r, per, 2048)
            k = 1 + (7 * per + 5 * j) % 63             # lanes 1 .. 63
            b[32 * k + j] ^= 0x5A
            blocks.append(bytes(b))
    for j in DEFECTS:                                   # the first and the last lane boundary, every period class once more
        for k in (1, 63):
            b = _periodic(r, 1 + (j + k) % 32, 2048)
            b[32 * k + j] ^= 0xA5
            blocks.append(bytes(b))
    _check_ragged(engine, oracle, blocks, "periodic")


def test_ext_windows_block_sizes(engine, oracle):
    """every size of SIZES as periodic text (periods 1, 3, 7, 32), small-alphabet text, noise and zeros, in one mixed ragged batch
    (blocks start at every alignment), and the same blocks in descending order"""
    r = random.Random(812)
    blocks = []
    for n in SIZES:
        for per in (1, 3, 7, 32):
            blocks.append(bytes(_periodic(r, per, n)))
        blocks.append(_alphabet(r, 4, n))
        blocks.append(_alphabet(r, 256, n))
        blocks.append(bytes(n))
        b = _periodic(r, 5, n)                          # a defect in the last five bytes: the tail rules of R3 / R5 next to a match
        b[n - 1 - (n % 5)] ^= 1
        blocks.append(bytes(b))
    _check_ragged(engine, oracle, blocks, "sizes")
    _check_ragged(engine, oracle, blocks[::-1], "sizes reversed", params=[(32, 10), (20, 5)])


def test_ext_windows_random_alphabets(engine, oracle):
    """alphabets of 2 and 4 symbols (a candidate almost everywhere, distances that differ from lane to lane: the scattered gather) and
    of 256 (almost every position "none": the gather at distance 63 into the pad and the previous lane's window)"""
    r = random.Random(813)
    blocks = []
    for k in (2, 4, 256):
        for n in (2048, 2048, 2048, 2047, 2017, 1025, 77, 45):
            blocks.append(_alphabet(r, k, n))
    _check_ragged(engine, oracle, blocks, "alphabets")


def test_ext_windows_fixed_pitch_at_every_source_alignment(engine, oracle):
    """fixed-pitch batches (pitch = block size: 2048 keeps the alignment of the first block, 2017 walks through all of them) whose first
    byte sits at 0 .. 15 modulo 16: the tile comes in by 16-byte requests of any alignment plus the masked chunk the block ends in"""
    import torch
    r = random.Random(814)
    for n in (2048, 2017):
        blocks = [bytes(_periodic(r, 9, n)), _alphabet(r, 4, n), _alphabet(r, 256, n), bytes(_periodic(r, 32, n)), _alphabet(r, 2, n)]
        flat = b"".join(blocks)
        for a in range(16):
            buf = torch.zeros(a + len(flat) + 64, dtype=torch.uint8, device="cuda")
            assert buf.data_ptr() % 16 == 0
            buf[a:a + len(flat)] = torch.frombuffer(bytearray(flat), dtype=torch.uint8).cuda()
            for cw, mm in ((32, 10), (20, 5)):
                out, ol, st = engine.compress_batch(buf[a:a + len(flat)], in_len=n, nblocks=len(blocks), cwindow=cw, maxmatch=mm)
                torch.cuda.synchronize()
                _compare(oracle, blocks, cw, mm, out, ol, st, ("fixed", n, a))


def test_ext_windows_writes_stay_inside(engine, oracle):
    """guard bands (tests/guards.py) around every buffer of one ragged and one fixed-pitch call of either instantiation: rows at the
    minimal pitch, nothing written outside out[:out_len rounded up to 4], out_len and status -- and nothing into the rows of the
    short blocks between them"""
    r = random.Random(815)
    for cw in (32, 20):
        path = "k_compress<1,%s,true> windows" % ("true" if cw == 32 else "false")
        rows, silent = [], []
        for n in (2048, 2047, 1025, 77, 45, 5):
            b = _periodic(r, 6, n)
            b[n // 2] ^= 0x11
            rows += [bytes(b), containment.incompressible(oracle, n)]
            silent.append(len(rows))
            rows.append(containment.SHORT_BLOCKS[len(silent) % len(containment.SHORT_BLOCKS)])
        pitch = containment.round4(oracle.out_bound(2048))
        containment.compress_batch_call(engine, oracle, (path, "ragged"), path, rows, cw, 10, pitch, bound=2048, mis=7, silent=silent)
        n = 2017
        rows = [bytes(_periodic(r, 11, n)), containment.incompressible(oracle, n), bytes(n), _alphabet(r, 4, n)]
        containment.compress_batch_call(engine, oracle, (path, "fixed"), path, rows, cw, 10, containment.round4(oracle.out_bound(n)),
                                        mis=5, fixed=(n, 2032))


def test_ext_windows_agrees_with_the_shared_layout():
    """the tests above against lib/libhdlz_keys.so -- the one-tile kernel with the shared tile layout and the masked gather -- in a
    subprocess: both layouts give the oracle's streams"""
    assert os.path.exists(KEYS), "lib/libhdlz_keys.so is not built: hdl_deflate_amd/csrc/build.sh keys"
    env = dict(os.environ, HDLZ_LIB=KEYS)
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_ext_windows.py", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "not agrees_with_the_shared_layout"], cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    assert r.returncode == 0, tail
    assert "5 passed" in r.stdout and " failed" not in r.stdout, tail
