"""GPU (-m gpu): the extension of the one-tile kernels from the search's mismatch bits (make_tokens_bits / WaveLdsBits,
hdlz_compress_common.h).

k_compress<1, ., true, .> keeps, for every distance d, the word neq_d of match_search_bits in LDS (NEQ[d & 31][lane]) and takes the
match length of position i from the zero bits of (neq_d of the next lane : neq_d) from bit i + 3 on, instead of comparing bytes
again; NEQ is the wave's whole LDS, so the staged tile in front of it and the bit buffer + the constant LUT (fetched per tile) behind
it share its memory.  What can go wrong: a row that is off by one (d = 32 aliases row 0, "none" reads row 31), the switch from the
single-word shift (i <= 22) to the two-word v_alignbit (i >= 23), lane 63 without a successor, lane 0's false history, a cap that is
off by one (Kmax - 3, N - 5 - p), a LUT that is read before it has landed or a bit buffer zeroed over it.  Every block below goes
through the one-tile kernel (a ragged batch with a stated bound of 2048, or fixed pitch above 1024 bytes) and is compared with the C
oracle on bytes, length and status; the same file runs against lib/libhdlz_keys.so (the key search with the byte-gather extension)
in a subprocess.  The oracle's stream of a (block, cwindow, maxmatch) is computed once per process."""
import os
import random
import subprocess
import sys
import zlib

import numpy as np
import pytest

import joined_ref                               # end_bit(): the end-of-block position of an oracle stream -- helper only
import test_gpu_containment as containment      # the guarded hdlz_compress_batch call (tests/guards.py) -- helpers only

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = os.path.join(REPO, "hdl_deflate_amd", "lib", "libhdlz_keys.so")
PARAMS = [(32, 10), (32, 5), (31, 10), (31, 5), (16, 10), (16, 5)]      # FULLWIN and the non-FULLWIN instantiation
SIZES = [5, 6, 7, 12, 13] + list(range(31, 46)) + [63, 64, 65, 66] + list(range(2015, 2049))
STARTS = list(range(20, 32))                    # match starts inside a run: the single-word / two-word switch at 22 / 23
LANES = (0, 1, 62, 63)
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
    assert len(blocks) <= 800 and all(5 <= len(b) <= 2048 for b in blocks)
    flat = b"".join(blocks) + bytes(64)
    off = np.cumsum([0] + [len(b) for b in blocks]).astype(np.int64)
    d_in = torch.frombuffer(bytearray(flat), dtype=torch.uint8).cuda()
    d_off = torch.from_numpy(off).cuda()
    for cw, mm in params:
        out, ol, st = engine.compress_batch(d_in, in_off=d_off, cwindow=cw, maxmatch=mm, max_len=2048)
        torch.cuda.synchronize()
        _compare(oracle, blocks, cw, mm, out, ol, st, label)


def _periodic(r, per, n):
    pat = bytes(r.sample(range(256), per))       # distinct bytes: the period is exactly `per`
    return bytearray((pat * (n // per + 1))[:n])


def _alphabet(r, k, n):
    return bytes(r.randrange(k) if k < 256 else r.getrandbits(8) for _ in range(n))


def _flip(b, q):
    if 0 <= q < len(b):
        b[q] ^= 0x5A


def test_ext_bits_periodic_first_mismatch_behind_the_start(engine, oracle):
    """one period d = 1 .. 32 per block; at every site (lane, i) a defect at p - 1 lets a match start at p = 32 lane + i, a second one
    at p + L puts the first mismatch L = 3 .. 10 bytes behind it.  Starts i = 20 .. 31 in lanes 0, 1, 62, 63, L rotating so that every
    (i, L) and (d, L) pair occurs; lane 63's sites end within the block's last bytes (the N - 5 - p cap)"""
    r = random.Random(911)
    blocks = []
    for d in range(1, 33):
        for i in STARTS:
            b = _periodic(r, d, 2048)
            for k, lane in enumerate(LANES):
                p = 32 * lane + i
                L = 3 + (d + i + 3 * k) % 8
                _flip(b, p - 1)
                _flip(b, p + L)
            blocks.append(bytes(b))
    assert len(blocks) == 384
    _check_ragged(engine, oracle, blocks[:192], "periodic a")
    _check_ragged(engine, oracle, blocks[192:], "periodic b")


def test_ext_bits_planted_matches_every_distance_start_and_length(engine, oracle):
    """noise (no candidate anywhere) with planted copies: x[p .. p + L) = x[p - d .. p - d + L) and x[p + L] different, so position p =
    32 lane + i holds exactly one candidate, at distance d, of length exactly L.  Per block one d and one i; lanes 0, 1, 62, 63 with a
    rotating L and lanes 8, 12, .. 36 with L = 3 .. 10 each: every (d, i, L) occurs, at MAXMATCH 10 and 5 (the Kmax - 3 cap)"""
    r = random.Random(912)
    blocks = []
    for d in range(1, 33):
        for i in STARTS:
            b = bytearray(containment.incompressible(oracle, 2048, seed=(d * 32 + i) % 7))
            sites = [(lane, 3 + (d + i + 3 * k) % 8) for k, lane in enumerate(LANES)] + [(8 + 4 * k, 3 + k) for k in range(8)]
            for lane, L in sites:
                p = 32 * lane + i
                if p - d < 0 or p + L + 2 >= 2048:
                    L = min(L, 2048 - 3 - p)             # (lane 63: the copy ends where a match may end at most; lane 0: d > p plants nothing)
                    if p - d < 0 or L < 3:
                        continue
                for k in range(L):
                    b[p + k] = b[p + k - d]
                if p + L < 2048 and b[p + L] == b[p + L - d]:
                    b[p + L] = 144 + (b[p + L] - 144 + 1) % 112
            blocks.append(bytes(b))
    for part in range(2):
        _check_ragged(engine, oracle, blocks[192 * part:192 * (part + 1)], ("planted", part), params=[(32, 10), (32, 5), (16, 10), (31, 5)])


def test_ext_bits_block_sizes(engine, oracle):
    """every size of SIZES as periodic text (periods 1, 3, 32), two-symbol noise, noise and a period with a defect in the last bytes, in
    one mixed ragged batch (blocks start at every alignment)"""
    r = random.Random(913)
    blocks = []
    for n in SIZES:
        for per in (1, 3, 32):
            blocks.append(bytes(_periodic(r, per, n)))
        blocks.append(_alphabet(r, 2, n))
        blocks.append(_alphabet(r, 256, n))
        b = _periodic(r, 5, n)                          # a defect in the last five bytes: the tail rules of R3 / R5 next to a match
        b[n - 1 - (n % 5)] ^= 1
        blocks.append(bytes(b))
    _check_ragged(engine, oracle, blocks[:180], "sizes a")
    _check_ragged(engine, oracle, blocks[180:], "sizes b")
    _check_ragged(engine, oracle, blocks[::-3], "sizes reversed", params=[(32, 10), (16, 5)])


def test_ext_bits_lane_0_false_history(engine, oracle):
    """2048-byte blocks whose last 32 bytes equal their first 32: the search hands lane 0 lane 63's bytes as history (a rotate), so
    every position of lane 0 finds a "match" 32 + i - j back, in front of the block -- all rejected by d <= p; with a short period
    inside the first run the real candidates (d <= p) must win"""
    r = random.Random(914)
    blocks = []
    for k in range(24):
        b = bytearray(_alphabet(r, 256 if k < 8 else 4, 2048)) if k < 16 else _periodic(r, 1 + k % 7, 2048)
        if k >= 16:
            b[40 + k] ^= 0x33
        b[2016:2048] = b[0:32]
        blocks.append(bytes(b))
    _check_ragged(engine, oracle, blocks, "false history")


def test_ext_bits_no_candidates_two_symbols_and_zeros(engine, oracle):
    """random bytes (almost every position "none": row 31, discarded), two-symbol noise (a candidate almost everywhere, distances that
    differ from lane to lane: rows scattered over NEQ) and zeros (distance 1 everywhere, every match capped by Kmax)"""
    r = random.Random(915)
    blocks = []
    for n in (2048, 2048, 2047, 2017, 1025, 66, 45):
        blocks += [_alphabet(r, 256, n), _alphabet(r, 2, n), _alphabet(r, 3, n), bytes(n), containment.incompressible(oracle, n)]
    _check_ragged(engine, oracle, blocks, "alphabets")


def test_ext_bits_fixed_pitch_at_every_source_alignment(engine, oracle):
    """fixed-pitch batches (pitch = block size: 2048 keeps the alignment of the first block, 2017 walks through all of them) whose first
    byte sits at 0 .. 15 modulo 16, and the same blocks as a ragged batch at each of those alignments"""
    import torch
    r = random.Random(916)
    for n in (2048, 2017):
        blocks = [bytes(_periodic(r, 9, n)), _alphabet(r, 4, n), _alphabet(r, 256, n), bytes(_periodic(r, 32, n)), _alphabet(r, 2, n)]
        flat = b"".join(blocks)
        off = torch.from_numpy(np.cumsum([0] + [len(b) for b in blocks]).astype(np.int64)).cuda()
        for a in range(16):
            buf = torch.zeros(a + len(flat) + 64, dtype=torch.uint8, device="cuda")
            assert buf.data_ptr() % 16 == 0
            buf[a:a + len(flat)] = torch.frombuffer(bytearray(flat), dtype=torch.uint8).cuda()
            for cw, mm in ((32, 10), (16, 5)):
                out, ol, st = engine.compress_batch(buf[a:a + len(flat)], in_len=n, nblocks=len(blocks), cwindow=cw, maxmatch=mm)
                torch.cuda.synchronize()
                _compare(oracle, blocks, cw, mm, out, ol, st, ("fixed", n, a))
            out, ol, st = engine.compress_batch(buf[a:a + len(flat)], in_off=off, cwindow=32, maxmatch=10, max_len=2048)
            torch.cuda.synchronize()
            _compare(oracle, blocks, 32, 10, out, ol, st, ("ragged", n, a))


def test_ext_bits_end_bits_twin(engine, oracle):
    """hdlz_compress_batch_bits (the ENDBITS instantiations): the same rows as the oracle and, per block, the bit its end-of-block code
    starts at"""
    import torch
    r = random.Random(917)
    blocks = []
    for n in (2048, 2047, 2016, 1025, 77, 45, 13, 5):
        blocks += [bytes(_periodic(r, 1 + n % 31, n)), _alphabet(r, 2, n), _alphabet(r, 256, n), bytes(n)]
    b = _periodic(r, 32, 2048)
    b[32 * 63 + 27] ^= 1
    blocks.append(bytes(b))
    B = len(blocks)
    flat = b"".join(blocks) + bytes(64)
    d_in = torch.frombuffer(bytearray(flat), dtype=torch.uint8).cuda()
    d_off = torch.from_numpy(np.cumsum([0] + [len(x) for x in blocks]).astype(np.int64)).cuda()
    pitch = containment.round4(oracle.out_bound(2048))
    for cw, mm in ((32, 10), (16, 5)):
        rows = torch.zeros((B, pitch), dtype=torch.uint8, device="cuda")
        ol, st = (torch.full((B,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
        eb = torch.full((B,), -1, dtype=torch.int64, device="cuda")
        rc = engine.lib.hdlz_compress_batch_bits(d_in.data_ptr(), d_off.data_ptr(), 0, 2048, B, cw, mm, rows.data_ptr(), pitch, ol.data_ptr(),
                                                 st.data_ptr(), eb.data_ptr(), containment.stream_ptr())
        assert rc == 0, engine.lib.hdlz_last_error()
        torch.cuda.synchronize()
        _compare(oracle, blocks, cw, mm, rows, ol, st, "end bits")
        assert eb.cpu().tolist() == [joined_ref.end_bit(_expect(oracle, x, cw, mm)[1]) for x in blocks], ("end bits", cw, mm)


def test_ext_bits_writes_stay_inside(engine, oracle):
    """guard bands (tests/guards.py) around every buffer of one ragged call of either instantiation: rows at the minimal pitch, nothing
    written outside out[:out_len rounded up to 4], out_len and status -- and nothing into the rows of the short blocks between them"""
    r = random.Random(918)
    for cw in (32, 16):
        path = "k_compress<1,%s,true> mismatch bits" % ("true" if cw == 32 else "false")
        rows, silent = [], []
        for n in (2048, 2047, 1025, 66, 45, 5):
            b = _periodic(r, 6, n)
            b[n // 2] ^= 0x11
            rows += [bytes(b), containment.incompressible(oracle, n)]
            silent.append(len(rows))
            rows.append(containment.SHORT_BLOCKS[len(silent) % len(containment.SHORT_BLOCKS)])
        pitch = containment.round4(oracle.out_bound(2048))
        containment.compress_batch_call(engine, oracle, (path, "ragged"), path, rows, cw, 10, pitch, bound=2048, mis=7, silent=silent)


def test_ext_bits_agrees_with_the_keys_build():
    """the tests above against lib/libhdlz_keys.so -- the one-tile kernel with the key search, the shared tile layout and the byte-gather
    extension -- in a subprocess: both give the oracle's streams"""
    assert os.path.exists(KEYS), "lib/libhdlz_keys.so is not built: hdl_deflate_amd/csrc/build.sh keys"
    env = dict(os.environ, HDLZ_LIB=KEYS)
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_ext_bits.py", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "not agrees_with_the_keys_build"], cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    assert r.returncode == 0, tail
    assert "8 passed" in r.stdout and " failed" not in r.stdout, tail
