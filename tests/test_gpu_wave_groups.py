"""GPU (-m gpu): the one-tile kernels with the bit search, k_compress<1, ., true, .> -- which blocks a wave takes, and the end of the
block as a bit of the search's mismatch words (end_cap_word / make_tokens_bits_packed, hdlz_compress_common.h).

What can go wrong.  Mapping: a batch smaller than, equal to or a little larger than a handful of waves; a batch of ncu * 256 + 7 blocks,
where the moving column wraps and the last row leaves most waves without a block; short blocks (status E_SHORT_INPUT, nothing written)
between blocks that compress.  End cap: the match length at position p is the run of zero mismatch bits from bit i + 3 on, and the
block's end is a forced bit at N - 2 -- off by one it lets a match run into the last two bytes or cuts it a byte short; the bit sits
in the lane the block ends in, in the next lane (N - 2 = 32 k) or in none (a full tile's lane 63 holds it at bit 30).  So: every
length 5 .. 70 and 1984 .. 2048 (every N mod 32, the end at 32 k + {0 .. 5}) with data of period 1, 2, 3, 31 and 32, whose matches
run to the block's end so that only the cap limits them, and one block without any candidate per length, which takes the literal arm
now that the zero bytes behind a short block's end no longer match each other.  Result bytes read in place (sub-dword operands):
distances 1, 31, 32 in lane 0 at positions below the distance (lane 63's bytes as false history) and in lane 63.
Every case is compared with the C oracle on bytes, lengths and statuses; the oracle's stream of a (block, cwindow, maxmatch) is computed
once per process (the cache of test_gpu_ext_bits).  The same cases run against lib/libhdlz_dword.so, the build without the sub-dword
operands (-DHDLZ_EXT_SDWA=0), in a subprocess."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import joined_ref                               # end_bit(): helper only
import test_gpu_containment as containment      # incompressible(), round4(), stream_ptr(): helpers only
import test_gpu_ext_bits as ext                 # the ragged helper, the oracle cache, the data makers: helpers only

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DWORD = os.path.join(REPO, "hdl_deflate_amd", "lib", "libhdlz_dword.so")
E_SHORT_INPUT = 1
SMALL = (1, 4, 5, 6, 9, 11)
MAPPING_PARAMS = [(32, 10), (31, 10)]           # <1, true, true> and <1, false, true>
CAP_PARAMS = [(cw, mm) for cw in (32, 31, 5) for mm in (10, 5)]
CAP_LENGTHS = list(range(5, 71)) + list(range(1984, 2049))


def _mixed(oracle, r, count, size=None):
    """blocks of the kinds whose tiles cost differently (text-like, two symbols, a short period, no candidate at all), lengths that end
    in every part of a run (or all of one size)"""
    out = []
    for k in range(count):
        n = size or (2048, 2047, 1999, 1025, 333, 70, 37, 2048, 1030, 5, 2046)[k % 11]
        kind = k % 4
        if kind == 0:
            out.append(ext._alphabet(r, 20, n))
        elif kind == 1:
            out.append(ext._alphabet(r, 2, n))
        elif kind == 2:
            out.append(bytes(ext._periodic(r, 1 + k % 32, n)))
        else:
            out.append(containment.incompressible(oracle, n, seed=k % 3))
    return out


def test_mapping_small_batches(engine, oracle):
    """batches of 1, 4, 5, 6, 9 and 11 blocks, both window instantiations"""
    r = random.Random(3301)
    for count in SMALL:
        ext._check_ragged(engine, oracle, _mixed(oracle, r, count), ("small", count), params=MAPPING_PARAMS)


def test_mapping_small_batches_end_bits(engine, oracle):
    """hdlz_compress_batch_bits (the ENDBITS instantiations) on the same small batches: rows, lengths, statuses and the end bit"""
    import torch
    r = random.Random(3301)
    pitch = containment.round4(oracle.out_bound(2048))
    for count in SMALL:
        blocks = _mixed(oracle, r, count)
        flat = b"".join(blocks) + bytes(64)
        d_in = torch.frombuffer(bytearray(flat), dtype=torch.uint8).cuda()
        d_off = torch.from_numpy(np.cumsum([0] + [len(x) for x in blocks]).astype(np.int64)).cuda()
        for cw, mm in MAPPING_PARAMS:
            rows = torch.zeros((count, pitch), dtype=torch.uint8, device="cuda")
            ol, st = (torch.full((count,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
            eb = torch.full((count,), -1, dtype=torch.int64, device="cuda")
            rc = engine.lib.hdlz_compress_batch_bits(d_in.data_ptr(), d_off.data_ptr(), 0, 2048, count, cw, mm, rows.data_ptr(), pitch,
                                                     ol.data_ptr(), st.data_ptr(), eb.data_ptr(), containment.stream_ptr())
            assert rc == 0, engine.lib.hdlz_last_error()
            torch.cuda.synchronize()
            ext._compare(oracle, blocks, cw, mm, rows, ol, st, ("small end bits", count))
            assert eb.cpu().tolist() == [joined_ref.end_bit(ext._expect(oracle, x, cw, mm)[1]) for x in blocks], ("end bits", count, cw)


def test_mapping_column_wraps_and_last_row_is_short(engine, oracle):
    """ncu * 256 + 7 blocks of 2048 bytes: one full row of the moving column and a second row of seven blocks.  61 distinct blocks
    (a prime: every wave meets every kind) repeated; lengths and statuses of ALL blocks, bytes of the first and last 200 and of
    every 97th"""
    import torch
    r = random.Random(3302)
    kinds = _mixed(oracle, r, 61, size=2048)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    B = ncu * 256 + 7
    idx = torch.arange(B, device="cuda") % 61
    table = torch.frombuffer(bytearray(b"".join(kinds)), dtype=torch.uint8).cuda().view(61, 2048)
    d = table[idx].contiguous()
    out, ol, st = engine.compress_batch(d, cwindow=32, maxmatch=10)
    torch.cuda.synchronize()
    refs = [ext._expect(oracle, b, 32, 10) for b in kinds]
    assert all(rc == 0 for rc, _ in refs)
    want_len = torch.tensor([len(z) for _, z in refs], dtype=ol.dtype, device="cuda")[idx]
    assert int((st != 0).sum()) == 0
    assert torch.equal(ol, want_len)
    rows = sorted(set(range(200)) | set(range(B - 200, B)) | set(range(0, B, 97)))
    got = out[torch.tensor(rows, device="cuda")].cpu().numpy()
    for j, k in enumerate(rows):
        z = refs[k % 61][1]
        assert got[j, :len(z)].tobytes() == z, ("wrap", k)


def test_mapping_short_blocks_between_compressing_ones(engine, oracle):
    """a ragged batch in which blocks of 0 .. 4 bytes (E_SHORT_INPUT, length 0) sit between blocks that compress"""
    import torch
    r = random.Random(3303)
    blocks = []
    for k, b in enumerate(_mixed(oracle, r, 22)):
        blocks.append(b)
        if k % 3 != 1:
            blocks.append(containment.SHORT_BLOCKS[k % 5])
        if k % 5 == 0:
            blocks.append(containment.SHORT_BLOCKS[(k + 2) % 5])
    flat = b"".join(blocks) + bytes(64)
    d_in = torch.frombuffer(bytearray(flat), dtype=torch.uint8).cuda()
    d_off = torch.from_numpy(np.cumsum([0] + [len(x) for x in blocks]).astype(np.int64)).cuda()
    for cw, mm in MAPPING_PARAMS:
        out, ol, st = engine.compress_batch(d_in, in_off=d_off, cwindow=cw, maxmatch=mm, max_len=2048)
        torch.cuda.synchronize()
        out, ol, st = out.cpu().numpy(), ol.cpu().numpy(), st.cpu().numpy()
        for k, b in enumerate(blocks):
            if len(b) < 5:
                assert st[k] == E_SHORT_INPUT and ol[k] == 0, ("short", cw, k)
            else:
                rc, ref = ext._expect(oracle, b, cw, mm)
                assert rc == 0 and st[k] == 0 and ol[k] == len(ref) and out[k, :ol[k]].tobytes() == ref, ("between short", cw, k, len(b))


def _cap_blocks(oracle, lengths):
    r = random.Random(3304)
    blocks = []
    for n in lengths:
        for per in (1, 2, 3, 31, 32):
            blocks.append(bytes(ext._periodic(r, per, n)))          # a match that runs to the block's end: only the cap stops it
        blocks.append(containment.incompressible(oracle, n, seed=n % 3))     # no candidate: the literal arm
    return blocks


@pytest.mark.parametrize("part", ["len5to70", "len1984to2016", "len2017to2048"])
def test_end_cap_every_length(engine, oracle, part):
    """every length of the part, periods 1, 2, 3, 31, 32 and one block without a candidate, MAXMATCH 5 and 10, CWINDOW 5, 31 and 32"""
    lo, hi = (int(x) for x in part[3:].split("to"))
    blocks = _cap_blocks(oracle, [n for n in CAP_LENGTHS if lo <= n <= hi])
    ext._check_ragged(engine, oracle, blocks, ("end cap", part), params=CAP_PARAMS)


def test_result_bytes_distances_1_31_32_in_lanes_0_and_63(engine, oracle):
    """noise with copies planted at distance 1, 31 and 32: in lane 0 at positions below the distance (the candidate lies in front of
    the block -- lane 63's bytes are made to look like it -- and must be rejected) and at and above it, and in lane 63 up to the
    last position a match may start at"""
    blocks = []
    for d in (1, 31, 32):
        for i in (0, 1, 7, 8, 15, 16, 24, 30, 31):
            b = bytearray(containment.incompressible(oracle, 2048, seed=(d + i) % 3))
            b[2048 - 32:2048] = b[0:32]                              # lane 63's run = lane 0's: the rotate's false history matches
            for p in (i, 32 * 63 + i):                               # the same site in lane 0 and in lane 63
                L = min(3 + (d + i) % 8, 2048 - 2 - p)
                if p - d < 0 or L < 3:
                    continue
                for k in range(L):
                    b[p + k] = b[p + k - d]
            blocks.append(bytes(b))
    ext._check_ragged(engine, oracle, blocks, "distances", params=[(32, 10), (32, 5), (31, 10)])


def test_agrees_with_the_build_without_sub_dword_operands():
    """the end-cap cases of the shortest part, the small batches and the distance sites against lib/libhdlz_dword.so
    (-DHDLZ_EXT_SDWA=0: result bytes extracted into registers, plain operands) in a subprocess: both builds give the oracle's streams"""
    assert os.path.exists(DWORD), "lib/libhdlz_dword.so is not built: hdl_deflate_amd/csrc/build.sh dword"
    env = dict(os.environ, HDLZ_LIB=DWORD)
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_wave_groups.py", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "len5to70 or small_batches or distances"], cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    assert r.returncode == 0, tail
    assert "4 passed" in r.stdout and " failed" not in r.stdout, tail
