"""GPU (-m gpu): the window dispatch and the block framing that the four compress drivers share (with_window, HEADER_WORD / HEADER_BITS,
block_nbytes, put_adler / adler_byte, adler_finish, wipe_behind, zero_tail16 -- hdlz_compress_common.h) and the single-sourced scratch
layout of the stream passes (stream_layout, hdlz_compress_stream.hip).

What these can break is WHICH kernel a window gets (the edges 32 | 33, 64 | 65 and "cwindow == 32 * NCH": FULLWIN) and WHERE a block's
trailer lands, so every CWINDOW of WINDOWS at MAXMATCH 5 and 10 compresses the same inputs through all four drivers -- the packed
small-block kernel (ragged and fixed pitch), the one-tile and the multi-tile kernel, the stream passes and a compress session -- and
every output byte, length and status is compared with the C oracle.  The inputs: one block of every length 5 .. 68 over the full byte
alphabet (literals of 8 and 9 bits mix, so a block ends at any bit), the same lengths over two symbols (match-dense: the end moves
differently), and the lengths around one and two tiles; their streams end at every byte alignment of an output word (asserted).
The oracle's stream of an (input, cwindow, maxmatch) is computed once per process."""
import random

import numpy as np
import pytest
import torch

import test_gpu_containment as containment      # the guarded hdlz_compress_streams call (tests/guards.py) -- helpers only

pytestmark = pytest.mark.gpu

WINDOWS = (1, 31, 32, 33, 63, 64, 65, 255, 256)
MAXMATCH = (5, 10)
SHORT = list(range(5, 69))                                       # 64 lengths
LONG = [2047, 2048, 2049, 4096, 4097, 4101]
FIXED = [32, 33, 256, 1024]                                      # the packed kernel's uniform path
PIECES = (32, 64, 2048)                                          # positions per call of a session
SUBSET = [5, 8, 32, 33, 64, 68] + LONG                           # the dozen lengths of the stream passes and the sessions


def _full(r, n):
    return bytes(r.getrandbits(8) for _ in range(n))


def _two(r, n):
    return bytes(b"ab"[r.getrandbits(1)] for _ in range(n))


def _inputs():
    r = random.Random(20261018)
    short = [_full(r, n) for n in SHORT] + [_two(r, n) for n in SHORT]
    long_ = [_full(r, n) for n in LONG] + [_two(r, n) for n in LONG]
    fixed = {n: [(_full, _two)[k % 2](r, n) for k in range(7)] for n in FIXED}
    return short, long_, fixed


SHORT_BLOCKS, LONG_BLOCKS, FIXED_BLOCKS = _inputs()
_ref = {}


def _expect(oracle, blk, cw, mm):
    key = (blk, cw, mm)
    if key not in _ref:
        rc, z = oracle.compress(blk, cwindow=cw, maxmatch=mm)
        assert rc == 0
        _ref[key] = z
    return _ref[key]


def subset_blocks():
    """SUBSET's lengths, the alphabets alternating (short and long blocks hold the full alphabet first, the two symbols behind it)"""
    by_len = {}
    for b in SHORT_BLOCKS + LONG_BLOCKS:
        by_len.setdefault(len(b), []).append(b)
    return [by_len[n][k % 2] for k, n in enumerate(SUBSET)]


def _dev(data):
    """host bytes -> a device buffer readable up to len(data) rounded up to 16, zeros behind the data"""
    buf = torch.zeros((len(data) + 15) // 16 * 16 + 16, dtype=torch.uint8)
    buf[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    return buf.cuda()


def _compare_rows(oracle, blocks, cw, mm, out, ol, st, label):
    out, ol, st = out.cpu().numpy(), ol.cpu().numpy(), st.cpu().numpy()
    for k, b in enumerate(blocks):
        ref = _expect(oracle, b, cw, mm)
        assert st[k] == 0 and ol[k] == len(ref) and out[k, :ol[k]].tobytes() == ref, (label, cw, mm, k, len(b), int(st[k]), int(ol[k]), len(ref))


def _ragged(engine, oracle, blocks, cw, mm, max_len, label):
    flat = b"".join(blocks) + bytes(64)
    off = np.cumsum([0] + [len(b) for b in blocks]).astype(np.int64)
    d_in, d_off = torch.frombuffer(bytearray(flat), dtype=torch.uint8).cuda(), torch.from_numpy(off).cuda()
    out, ol, st = engine.compress_batch(d_in, in_off=d_off, cwindow=cw, maxmatch=mm, max_len=max_len)
    _compare_rows(oracle, blocks, cw, mm, out, ol, st, label)


@pytest.mark.parametrize("cw", WINDOWS)
def test_trailers_end_at_every_byte_of_a_word(oracle, cw):
    """the premise of the tests below: over the inputs of one window the zlib streams have every length modulo 4, in the whole set and
    in the dozen that go through the stream passes and the sessions"""
    for mm in MAXMATCH:
        assert {len(_expect(oracle, b, cw, mm)) % 4 for b in SHORT_BLOCKS + LONG_BLOCKS} == {0, 1, 2, 3}, (cw, mm)
        assert {len(_expect(oracle, b, cw, mm)) % 4 for b in subset_blocks()} == {0, 1, 2, 3}, (cw, mm)


@pytest.mark.parametrize("cw", WINDOWS)
def test_compress_batch_ragged_three_kernels(engine, oracle, cw):
    """the short blocks with a stated bound of 68 (<= 1024: k_compress_small, ragged), the blocks of up to one tile with a bound of 2048
    (k_compress<., ., true> for windows up to 32, the multi-tile form above) and the longer ones (k_compress<., ., false>)"""
    for mm in MAXMATCH:
        _ragged(engine, oracle, SHORT_BLOCKS, cw, mm, max(SHORT), "small")
        _ragged(engine, oracle, [b for b in LONG_BLOCKS if len(b) <= 2048], cw, mm, 2048, "one tile")
        _ragged(engine, oracle, [b for b in LONG_BLOCKS if len(b) > 2048], cw, mm, max(LONG), "tiles")


@pytest.mark.parametrize("cw", WINDOWS)
def test_compress_batch_fixed_pitch_packed(engine, oracle, cw):
    """k_compress_small's uniform path: seven blocks (a partial group) of 32, 33, 256 and 1024 bytes at a 16-byte aligned pitch"""
    for n in FIXED:
        pitch = (n + 15) // 16 * 16
        rows = torch.zeros((len(FIXED_BLOCKS[n]), pitch), dtype=torch.uint8)
        for k, b in enumerate(FIXED_BLOCKS[n]):
            rows[k, :n] = torch.frombuffer(bytearray(b), dtype=torch.uint8)
        d_in = rows.cuda()
        assert d_in.data_ptr() % 16 == 0
        for mm in MAXMATCH:
            out, ol, st = engine.compress_batch(d_in, in_len=n, cwindow=cw, maxmatch=mm)
            _compare_rows(oracle, FIXED_BLOCKS[n], cw, mm, out, ol, st, ("fixed", n))


@pytest.mark.parametrize("cw", WINDOWS)
def test_compress_stream_passes(engine, oracle, cw):
    """hdlz_compress_stream (k_stream_*; k_stream_place composes the trailer in registers) for a dozen lengths: one to three tiles"""
    for blk in subset_blocks():
        d = _dev(blk)
        for mm in MAXMATCH:
            out, ol, st = engine.compress_stream(d, len(blk), cwindow=cw, maxmatch=mm)
            ref = _expect(oracle, blk, cw, mm)
            n = int(ol.item())
            assert int(st.item()) == 0 and n == len(ref) and out[:n].cpu().numpy().tobytes() == ref, (cw, mm, len(blk), n, len(ref))


@pytest.mark.parametrize("cw", WINDOWS)
def test_compress_session_in_pieces(engine, oracle, cw):
    """a compress session (k_compress_chunk) fed 32, 64 and 2048 bytes at a time, a step after every piece"""
    for blk in subset_blocks():
        for mm in MAXMATCH:
            ref = _expect(oracle, blk, cw, mm)
            for piece in PIECES:
                ses = engine.compress_session(cwindow=cw, maxmatch=mm)
                for k in range(0, len(blk), piece):
                    ses.write(blk[k:k + piece])
                    assert ses.step(max_positions=piece) == 0
                assert ses.step(final=True) == 0 and ses.done
                assert ses.out_len == len(ref) and ses.output(0, ses.out_len) == ref, (cw, mm, len(blk), piece, ses.out_len, len(ref))


@pytest.mark.parametrize("cw,nblocks", [(33, 3), (256, 1)])
def test_stream_scratch_layout_inside_guard_bands(engine, oracle, cw, nblocks):
    """the single-sourced scratch layout fenced at windows the containment suite does not run: exactly hdlz_streams_work_bytes bytes of
    scratch between guard bands, three tiles per block"""
    blocks = [b for b in LONG_BLOCKS if len(b) == 4101][:1] + [containment.incompressible(oracle, 4101), bytes(4101)]
    containment.compress_streams_call(engine, oracle, ("framing", cw, nblocks), blocks[:nblocks], cw=cw)
