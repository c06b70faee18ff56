"""GPU (-m gpu): the one-tile compress kernel (k_compress<1, ., true, .>) on the crafted inputs of tests/tile_diet2_craft.py.

What is under test: the literal emitter of a match-free tile (literal_codes: codes straight from the own bytes, no token words, no start
flags; 8- and 9-bit literals, 288 bits in a lane, the padding literals behind a short block's end and their removal, the LUT fetch and
the zeroed bit buffer after a tile of either kind), the tiles one candidate away from it (lane 0's false history, one match at the
last eligible position), the distance planes updated once per aligned group of four distances (every distance alone, at lane seams, in
lane 0 and lane 63, pairs of candidates inside a group and across two, window 20), the extension's lengths next to the edge literals,
and the plain Adler sums of a one-tile block at their largest.  Every stream is compared with the C oracle on status, length and every
byte and read back by zlib.  tests/test_tile_diet2_cpu.py holds the premises without a GPU."""
import numpy as np
import pytest

import test_gpu_tile_diet as gpu_diet           # _run(), _judge() -- helpers only
import tile_diet2_craft as diet2

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("family", diet2.FAMILIES, ids=lambda f: f.__name__)
def test_crafted_tiles_against_the_oracle(engine, oracle, family):
    cases = family()
    gpu_diet._judge(oracle, cases, gpu_diet._run(engine, cases))


def test_literal_tiles_as_a_fixed_pitch_batch(engine, oracle):
    """the full-size match-free blocks (and one ordinary block between them) as ONE fixed-pitch batch -- the call the benchmark makes"""
    import torch
    blocks = [c.data for c in diet2.literal_tiles() if len(c.data) == 2048]
    blocks.insert(2, next(c.data for c in diet2.distance_groups() if c.label == "planted d=32 cw=32"))
    d = torch.frombuffer(bytearray(b"".join(blocks)), dtype=torch.uint8).cuda().view(len(blocks), 2048)
    out, ol, st = engine.compress_batch(d, cwindow=32, maxmatch=10)
    torch.cuda.synchronize()
    out, ol, st = out.cpu().numpy(), ol.cpu().numpy(), st.cpu().numpy()
    for k, b in enumerate(blocks):
        rc, ref = oracle.compress(b, 32, 10)
        assert rc == 0 and st[k] == 0 and out[k, :ol[k]].tobytes() == ref, k


def test_alternation_within_a_wave(engine, oracle):
    """a wave runs a match-free block directly behind an ordinary one and the other way round (tile_diet2_craft.alternating, placed by
    (row, wave) for the grid of this device): the LUT and the zeroed bit buffer are right after either kind.  All lengths and statuses
    against the oracle; bytes of the first and last 200 blocks, every 97th and every long one"""
    import torch
    G = 256 * torch.cuda.get_device_properties(0).multi_processor_count
    blocks, kinds, long_ones = diet2.alternating(G)
    B = len(blocks)
    flat = np.frombuffer(b"".join(blocks) + bytes(64), dtype=np.uint8)
    off = np.cumsum([0] + [len(x) for x in blocks]).astype(np.int64)
    _, ref_len, ref_st = oracle.compress_batch(flat[:off[-1]], off.astype(np.uint64), 32, 10, nthreads=8)
    out, ol, st = engine.compress_batch(torch.from_numpy(flat.copy()).cuda(), in_off=torch.from_numpy(off).cuda(), cwindow=32, maxmatch=10,
                                        max_len=2048)
    torch.cuda.synchronize()
    ol_h, st_h = ol.cpu().numpy(), st.cpu().numpy()
    assert not ref_st.any() and not st_h.any()
    bad = np.nonzero(ol_h.astype(np.int64) != ref_len.astype(np.int64))[0]
    assert bad.size == 0, ("lengths", bad[:10].tolist())
    pick = sorted(set(list(range(200)) + list(range(B - 200, B)) + list(range(0, B, 97)) + long_ones))
    rows = out[torch.tensor(pick, device="cuda")].cpu().numpy()
    for k, b in enumerate(pick):
        rc, ref = oracle.compress(blocks[b], 32, 10)
        assert rc == 0 and rows[k, :ol_h[b]].tobytes() == ref, ("bytes", b, len(blocks[b]), kinds[b])
