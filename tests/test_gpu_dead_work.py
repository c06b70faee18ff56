"""GPU (-m gpu): the work the one-tile kernels skip because the data does not need it (match_search_bits, hdlz_compress_common.h, and
the BITS branch of k_compress, hdlz_compress.hip).

1. A bit plane that is the same word 0 or 0xFFFFFFFF in all 64 lanes adds nothing to any mismatch word: its 63 instructions are jumped
   over by one wave-uniform branch.  What can go wrong: a plane taken for dead that is constant in every lane but not ACROSS the lanes, or
   constant in 63 lanes, or constant in the data but not in the zero padding behind a short block; a plane taken for dead at a constant
   that is neither 0 nor all ones.
2. A tile in which no position has a 3-byte candidate at any distance 1..32 is all literals: the result is not transposed, the extension,
   the parse and the skip chain do not run.  What can go wrong: one candidate in one lane that does not switch the whole tile back, a
   candidate that exists but is not eligible (it must still give literals, through the normal path), a row store of the search that lands
   on the LUT or the zeroed bit buffer (the match-free path reads nothing from NEQ: it orders the two itself), and the LDS timeline
   when a wave runs a tile of one kind directly behind one of the other kind.

Every block goes through the one-tile kernel (a ragged batch with a stated bound of 2048) and is compared with the C oracle on bytes,
length and status at (CWINDOW, MAXMATCH) = (32, 10), (32, 5), (31, 10), (16, 10): both FULLWIN instantiations.  The same file runs
against lib/libhdlz_alllive.so (no plane skipped, no literal tile: -DHDLZ_PLANES_ALL_LIVE -DHDLZ_NO_LITERAL_TILE) in a subprocess.

(Positions behind the end of a block are zero bytes, and zeros repeat at distance 1: a block shorter than 2046 bytes always has a
candidate in its padding and takes the normal path.  The match-free path is reached by blocks of 2046 .. 2048 bytes only -- the
alternation test therefore plants full-size blocks into some waves' sequences, beside the short ones.)"""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import joined_ref                               # end_bit(): the end-of-block position of an oracle stream -- helper only
import test_gpu_containment as containment      # stream_ptr(), round4() -- helpers only
import test_gpu_ext_bits as ext                 # _check_ragged(), _expect(), _compare() -- helpers only

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALLLIVE = os.path.join(REPO, "hdl_deflate_amd", "lib", "libhdlz_alllive.so")
PARAMS = [(32, 10), (32, 5), (31, 10), (16, 10)]
_pool = {}


def _check(engine, oracle, blocks, label):
    for k in range(0, len(blocks), 800):
        ext._check_ragged(engine, oracle, blocks[k:k + 800], (label, k), params=PARAMS)


# ------------------------------------------------------------------------------------------------------------------ plane skip
def _plane_alphabet(r, planes, k):
    """k symbols (2 .. 4) whose bits outside `planes` are clear and in which every plane of `planes` varies"""
    mask = sum(1 << b for b in planes)
    syms = [0, mask]
    while len(syms) < min(k, 1 << len(planes)):
        s = r.getrandbits(8) & mask
        if s not in syms:
            syms.append(s)
    return syms


def _over(r, syms, n, const=0):
    return bytes(r.choice(syms) ^ const for _ in range(n))


def test_dead_work_chosen_plane_sets(engine, oracle):
    """alphabets of 2 .. 4 symbols in which exactly a chosen set of planes varies -- each plane alone, each plane dead, {0..6}, {0..3},
    {0} -- with the other planes at constant 0 and at constant 1; 2048 bytes, and 2047 / 777 (the padding makes a constant-1 plane vary)"""
    r = random.Random(1201)
    sets = [(b,) for b in range(8)] + [tuple(x for x in range(8) if x != b) for b in range(8)] + [tuple(range(7)), tuple(range(4)), (0,)]
    blocks = []
    for planes in sets:
        mask = sum(1 << b for b in planes)
        for const in (0, 0xFF & ~mask):
            for n, k in ((2048, 4), (2048, 2), (2047, 3), (777, 4)):
                blocks.append(_over(r, _plane_alphabet(r, planes, k), n, const))
    _check(engine, oracle, blocks, "plane sets")


def test_dead_work_plane_constant_in_every_lane_not_across(engine, oracle):
    """periodic text whose plane b is clear in the bytes of lanes 0 .. k and set in lanes k + 1 .. 63 (and the other way round), k = 0,
    31, 62: every lane's word of the plane is 0 or all ones, the wave's is not -- a wrong skip finds matches across the seam"""
    r = random.Random(1202)
    blocks = []
    for per in (1, 3, 7, 32):
        pat = bytes(r.sample(range(0x20, 0x60), per))
        base = (pat * (2048 // per + 1))[:2048]
        for b in (7, 6, 0):
            clear = bytes(x & ~(1 << b) & 0xFF for x in base)
            for k in (0, 31, 62):
                cut = 32 * (k + 1)
                blocks.append(clear[:cut] + bytes(x | (1 << b) for x in clear[cut:]))
                blocks.append(bytes(x | (1 << b) for x in clear[:cut]) + clear[cut:])
    _check(engine, oracle, blocks, "seam")


def test_dead_work_one_exception_lane(engine, oracle):
    """a plane constant (0 or 1) in 63 lanes that differs in ONE byte -- the first or the last of the run -- of lane 0, 1, 33 or 63"""
    r = random.Random(1203)
    blocks = []
    for b in (7, 5, 1):
        syms = _plane_alphabet(r, tuple(x for x in (0, 2, 4) if x != b), 4)
        for const in (0, 1 << b):
            for lane in (0, 1, 33, 63):
                for i in (0, 31):
                    blk = bytearray(_over(r, syms, 2048, const))
                    blk[32 * lane + i] ^= 1 << b
                    blocks.append(bytes(blk))
    _check(engine, oracle, blocks, "exception lane")


def test_dead_work_padded_blocks(engine, oracle):
    """short blocks whose data holds a plane at constant 1 (bytes >= 0x80 only, all-0xFF): the zero padding behind N makes it vary; one
    byte value repeated (every plane dead in the data) at N = 2048 and below"""
    r = random.Random(1204)
    blocks = []
    for n in (5, 33, 100, 2047):
        blocks.append(bytes([0xFF]) * n)
        blocks.append(_over(r, [0x80, 0x81, 0xC3, 0xFF], n))
        blocks.append(bytes(r.randrange(0x80, 0x100) for _ in range(n)))
        blocks.append(_over(r, [0xF0, 0xF1], n))
    for v in (0x00, 0xFF, 0x41, 0x80, 0x7F):
        for n in (2048, 2047, 2016, 100, 33, 5):
            blocks.append(bytes([v]) * n)
    _check(engine, oracle, blocks, "padded")


# ------------------------------------------------------------------------------------------------------------ match-free tiles
def _no_repeat(b, reach=48):
    """no 3-byte string of b occurs twice within `reach` positions"""
    last = {}
    for p in range(len(b) - 2):
        g = bytes(b[p:p + 3])
        if g in last and p - last[g] <= reach:
            return False
        last[g] = p
    return True


def _match_free(seed, n=2048):
    """n random bytes (every plane varies) without a 3-byte repeat within 48 positions"""
    if (seed, n) not in _pool:
        r = random.Random(77000 + seed)
        while True:
            b = bytes(r.getrandbits(8) for _ in range(n))
            if _no_repeat(b):
                break
        _pool[(seed, n)] = b
    return _pool[(seed, n)]


def _plant(b, p, d):
    """x[p .. p + 3) = x[p - d .. p - d + 3), if it fits: a 3-byte candidate at position p and distance d"""
    b = bytearray(b)
    if p - d < 0 or p + 3 > len(b):
        return None
    for k in range(3):
        b[p + k] = b[p + k - d]
    return bytes(b)


def _match_free_batch():
    blocks = []
    for s, n in enumerate((5, 37, 2046, 2047, 2048, 2048)):                 # no candidate
        blocks.append(_match_free(s, 2048)[:n])
    base = _match_free(10)
    for d in (1, 3, 31, 32):                                                # one candidate in one lane: the whole tile takes the normal path
        for lane in (0, 1, 63):
            for i in (0, 3, 29, 31):
                b = _plant(base, 32 * lane + i, d)
                if b is not None:
                    blocks.append(b)
    for d in (33, 40):                                                      # just outside the window: stays match-free
        for p in (40, 64, 1000, 2045):
            blocks.append(_plant(base, p, d))
    assert all(_no_repeat(b, 32) for b in blocks[-8:])
    for d in (3, 10, 22, 32):                                               # lane 0's false history: its first bytes among lane 63's
        b = bytearray(_match_free(11))
        b[2048 - d:2048 - d + 3] = b[0:3]
        blocks.append(bytes(b))
    for p in (20, 700, 2040):                                               # distance 20: no candidate at CWINDOW 16
        blocks.append(_plant(_match_free(12), p, 20))
    for n, p in ((2048, 2044), (2048, 2045), (2047, 2043), (37, 33)):       # a repeat that starts in the last four positions
        blocks.append(_plant(_match_free(13)[:n], p, 7))
    assert all(b is not None for b in blocks)
    return blocks


def test_dead_work_match_free_tiles(engine, oracle):
    """no candidate (sizes 5 .. 2048), exactly one planted candidate at distance 1, 3, 31, 32 and sites (lane 0, 1, 63) x (i = 0, 3,
    29, 31), a repeat at distance 33 / 40 only, and candidates that are not eligible: lane 0's false history, distance 20 at CWINDOW 16,
    a start in the last four positions"""
    _check(engine, oracle, _match_free_batch(), "match-free")


def test_dead_work_end_bits(engine, oracle):
    """the match-free batch through hdlz_compress_batch_bits (the ENDBITS instantiations): rows and, per block, the end-of-block bit"""
    import torch
    blocks = _match_free_batch()
    B = len(blocks)
    flat = b"".join(blocks) + bytes(64)
    d_in = torch.frombuffer(bytearray(flat), dtype=torch.uint8).cuda()
    d_off = torch.from_numpy(np.cumsum([0] + [len(x) for x in blocks]).astype(np.int64)).cuda()
    pitch = containment.round4(oracle.out_bound(2048))
    for cw, mm in PARAMS:
        rows = torch.zeros((B, pitch), dtype=torch.uint8, device="cuda")
        ol, st = (torch.full((B,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
        eb = torch.full((B,), -1, dtype=torch.int64, device="cuda")
        rc = engine.lib.hdlz_compress_batch_bits(d_in.data_ptr(), d_off.data_ptr(), 0, 2048, B, cw, mm, rows.data_ptr(), pitch, ol.data_ptr(),
                                                 st.data_ptr(), eb.data_ptr(), containment.stream_ptr())
        assert rc == 0, engine.lib.hdlz_last_error()
        torch.cuda.synchronize()
        ext._compare(oracle, blocks, cw, mm, rows, ol, st, "end bits")
        assert eb.cpu().tolist() == [joined_ref.end_bit(ext._expect(oracle, x, cw, mm)[1]) for x in blocks], ("end bits", cw, mm)


def test_dead_work_alternation_within_a_wave(engine, oracle):
    """a wave runs a block of one kind directly behind one of the other kind (the LDS timeline across iterations: NEQ rows, LUT, bit
    buffer).  With G = min(256 CUs, nblocks) wave w takes block k G + (w + k) mod G of row k (k_compress, BITS: the moving column): 2 G + 7
    short blocks (48 .. 96 bytes), the block of wave w in row k without a 3-byte repeat iff k + w is even, 4-symbol text otherwise; for
    every 509th wave the three blocks are 2046 .. 2048 bytes long instead -- those reach the match-free path itself (see the module
    text).  All lengths and statuses against the oracle; bytes of the first and last 200 blocks, every 97th and every long one"""
    import torch
    G = 256 * torch.cuda.get_device_properties(0).multi_processor_count
    B = 2 * G + 7
    r = random.Random(1206)
    free = _match_free(20, 1 << 16)
    text = bytes(r.choice(b"acgt") for _ in range(1 << 16))
    blocks, long_ones = [], []
    for b in range(B):
        k = b // G
        w = (b % G - k) % G                             # the wave that takes block b
        src = free if (k + w) % 2 == 0 else text
        if w % 509 == 3:
            n = 2048 - (k + w // 509) % 3
            long_ones.append(b)
        else:
            n = 48 + b % 49
        o = (b * 131) % (len(src) - n)
        blocks.append(src[o:o + n])
    flat = np.frombuffer(b"".join(blocks) + bytes(64), dtype=np.uint8)
    off = np.cumsum([0] + [len(x) for x in blocks]).astype(np.int64)
    _, ref_len, ref_st = oracle.compress_batch(flat[:off[-1]], off.astype(np.uint64), 32, 10, nthreads=8)
    d_in = torch.from_numpy(flat.copy()).cuda()
    out, ol, st = engine.compress_batch(d_in, in_off=torch.from_numpy(off).cuda(), cwindow=32, maxmatch=10, max_len=2048)
    torch.cuda.synchronize()
    ol_h, st_h = ol.cpu().numpy(), st.cpu().numpy()
    assert not ref_st.any() and not st_h.any()
    bad = np.nonzero(ol_h.astype(np.int64) != ref_len.astype(np.int64))[0]
    assert bad.size == 0, ("lengths", bad[:10].tolist())
    pick = sorted(set(list(range(200)) + list(range(B - 200, B)) + list(range(0, B, 97)) + long_ones))
    rows = out[torch.tensor(pick, device="cuda")].cpu().numpy()
    for k, b in enumerate(pick):
        rc, ref = oracle.compress(blocks[b], 32, 10)
        assert rc == 0 and rows[k, :ol_h[b]].tobytes() == ref, ("bytes", b, len(blocks[b]))


# -------------------------------------------------------------------------------------------------------------------- both forms
def test_dead_work_agrees_with_the_all_live_build():
    """the tests above against lib/libhdlz_alllive.so -- every plane computed, every tile through the extension, the parse and the
    chain -- in a subprocess: both forms give the oracle's streams"""
    if not os.path.exists(ALLLIVE):
        pytest.skip("lib/libhdlz_alllive.so is not built: hdl_deflate_amd/csrc/build.sh alllive")
    env = dict(os.environ, HDLZ_LIB=ALLLIVE)
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_dead_work.py", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "not agrees_with_the_all_live_build"], cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    assert r.returncode == 0, tail
    assert "7 passed" in r.stdout and " failed" not in r.stdout, tail
