"""GPU (-m gpu): the compress kernels that walk a block in several 2048-position tiles, on the crafted inputs of tests/compress_craft.py.

What is under test: the halo and the look-ahead of a staged tile (a candidate in the previous tile at cw - 1, cw, cw + 1; a match whose
3 .. 10 bytes straddle the seam at every offset), the start and the end of a block that has other blocks' bytes around it in memory, the
parse phase carried from tile to tile (k_stream_tails' last-32 functions, constant or marked for k_stream_xfer, composed by the two-level
scans), block ends at a seam, and chains of tiles across the chunk seams of the scans up to K = 2 chunks per lane.  Every stream is
compared with the C oracle on status, length and every byte and is read back by zlib, on four routes:
  one wave     engine.compress_batch, ragged with a bound above 2048 (or fixed pitch): k_compress<., ., false>, one wave per block
  streams      hdlz_compress_streams called directly, all cases of one length in ONE call, in_pitch == in_len where the layout says so
  one stream   engine.compress_stream: every case of family C, every eighth of the others
  session      engine.compress_session (k_compress_chunk), steps that end at S - 32, S, S + 32 and S + 1024, then the block in one call
tests/test_compress_seams_cpu.py holds the premises (that the inputs reach these edges) without a GPU.  The oracle's stream of a
(block, cwindow, maxmatch) is computed once per process (compress_craft.expect)."""
import zlib

import numpy as np
import pytest

import compress_craft as craft
from compress_craft import TILE, SEAMS, N0, N7, WINDOWS, fields

pytestmark = pytest.mark.gpu
SESSION_ENDS = sorted(S + k for S in SEAMS for k in (-32, 0, 32, 1024))          # all <= N0 - 11


def _judge(oracle, family, route, cw, mm, cases, results):
    """cases [(label, bytes)] against results [(status, stream)]: the oracle's status, length and bytes, and zlib reads it back"""
    assert len(cases) == len(results)
    wrong = []
    for (lab, b), (st, got) in zip(cases, results):
        rc, ref = craft.expect(oracle, b, cw, mm)
        if not (rc == 0 and st == 0 and got == ref):
            wrong.append((lab, b, st, ref, got))
            continue
        assert zlib.decompress(got) == b, (family, lab, cw, mm, route)
    if wrong:
        lab, b, st, ref, got = wrong[0]
        raise AssertionError("%d of %d streams differ from the oracle; first: %r status %d, %s" % (
            len(wrong), len(cases), (family, lab, cw, mm, route), st, craft.first_wrong_token(oracle, b, cw, mm, ref, got)))


def _rows(out, ol, st):
    out, ol, st = out.cpu().numpy(), ol.cpu().numpy(), st.cpu().numpy()
    return [(int(st[k]), out[k, :ol[k]].tobytes()) for k in range(len(ol))]


def _device(data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def _one_wave_ragged(engine, blocks, flat, cw, mm):
    """the blocks, back to back in `flat`, as ONE ragged batch whose stated bound is above 2048: one wave per block, tile by tile"""
    import torch
    off = np.cumsum([0] + [len(b) for b in blocks]).astype(np.int64)
    assert len(flat) >= off[-1] + 64 and max(len(b) for b in blocks) > TILE
    out, ol, st = engine.compress_batch(_device(flat), in_off=torch.from_numpy(off).cuda(), cwindow=cw, maxmatch=mm,
                                        max_len=max(len(b) for b in blocks))
    torch.cuda.synchronize()
    return _rows(out, ol, st)


def _one_wave_pitched(engine, mem, n, pitch, nb, cw, mm):
    import torch
    assert pitch % 16 == 0 and TILE < n < engine.LARGE_BLOCK
    d = _device(mem[:nb * pitch].ljust(nb * pitch + 64, b"\0"))
    out, ol, st = engine.compress_batch(d[:nb * pitch].view(nb, pitch), in_len=n, cwindow=cw, maxmatch=mm)
    torch.cuda.synchronize()
    return _rows(out, ol, st)


def _streams(engine, mem, n, pitch, nb, cw, mm):
    """hdlz_compress_streams itself: nb blocks of n bytes, block k at mem + k * pitch (any pitch; 64 readable bytes behind the last)"""
    import torch
    L = engine.lib
    assert len(mem) >= (nb - 1) * pitch + n + 64
    d_in = _device(mem)
    opitch = (L.hdlz_out_bound(n) + 3) // 4 * 4
    out = torch.zeros((nb, opitch), dtype=torch.uint8, device="cuda")
    ol = torch.full((nb,), -1, dtype=torch.int32, device="cuda")
    st = torch.full((nb,), -1, dtype=torch.int32, device="cuda")
    wb = L.hdlz_streams_work_bytes(n, nb)
    assert wb > 0
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    rc = L.hdlz_compress_streams(d_in.data_ptr(), pitch, n, nb, cw, mm, out.data_ptr(), opitch, ol.data_ptr(), st.data_ptr(),
                                 work.data_ptr(), wb, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.hdlz_last_error()
    torch.cuda.synchronize()
    return _rows(out, ol, st)


def _one_stream(engine, d_in, n, cw, mm):
    out, ol, st = engine.compress_stream(d_in, n, cwindow=cw, maxmatch=mm)
    k = int(ol.cpu()[0])
    return int(st.cpu()[0]), out[:max(k, 0)].cpu().numpy().tobytes()


def _padded(b, tail=b""):
    """a block alone in a buffer of its own: readable up to its size rounded up to 16 and 16 more, `tail` then zeros behind it"""
    return _device((b + tail).ljust((len(b) + 15) // 16 * 16 + 16, b"\0"))


def _session(engine, b, cw, mm, ends):
    """a compress session whose calls end at `ends` (each time with no more known than the eleven bytes the call needs), then the rest"""
    ses = engine.compress_session(cwindow=cw, maxmatch=mm)
    known = 0
    for q in ends:
        assert q % 32 == 0 and q <= len(b) - 11
        ses.write(b[known:q + 11])
        known = q + 11
        assert ses.step(max_positions=q - ses.pos) == 0 and ses.pos == q and not ses.done
    ses.write(b[known:])
    st = ses.step(final=True)
    assert ses.done
    return st, ses.output(0, ses.out_len)


def _flat(cases):
    return b"".join(b for _, b in cases)


def _every_eighth(cases):
    return cases[::8]


# ------------------------------------------------------------------------------------------------ A: lone matches over a seam
@pytest.mark.parametrize("cw,mm", WINDOWS)
def test_lone_matches_one_wave(engine, oracle, cw, mm):
    """both lengths in one ragged batch: the blocks start at every alignment"""
    fam = craft.family_a(cw, mm)
    cases = []
    for i, c in enumerate(fam[N0]):                          # case, twin, a case of the other length, ...
        cases.append(c)
        if i % 2 and i // 2 < len(fam[N7]):
            cases.append(fam[N7][i // 2])
    assert len(cases) == len(fam[N0]) + len(fam[N7])
    _judge(oracle, "A", "one wave", cw, mm, cases, _one_wave_ragged(engine, [b for _, b in cases], _flat(cases) + bytes(64), cw, mm))


@pytest.mark.parametrize("cw,mm", WINDOWS)
def test_lone_matches_streams(engine, oracle, cw, mm):
    for n, cases in craft.family_a(cw, mm).items():
        _judge(oracle, "A", "streams", cw, mm, cases, _streams(engine, _flat(cases) + bytes(64), n, n, len(cases), cw, mm))


# ------------------------------------------------------------------------------------------------ B: the block's neighbours in memory
def _blocks_b(lay):
    lab, n, pitch, nb, mem = lay
    return [("%s k=%d" % (lab, k), mem[k * pitch:k * pitch + n]) for k in range(nb)]


@pytest.mark.parametrize("cw,mm", WINDOWS)
def test_neighbours_one_wave(engine, oracle, cw, mm):
    for lay in craft.family_b(cw, mm):
        lab, n, pitch, nb, mem = lay
        cases = _blocks_b(lay)
        if pitch == n:
            got = _one_wave_ragged(engine, [b for _, b in cases], mem, cw, mm)
        else:
            got = _one_wave_pitched(engine, mem, n, pitch, nb, cw, mm)
        _judge(oracle, "B", "one wave", cw, mm, cases, got)


@pytest.mark.parametrize("cw,mm", WINDOWS)
def test_neighbours_streams(engine, oracle, cw, mm):
    for lay in craft.family_b(cw, mm):
        lab, n, pitch, nb, mem = lay
        _judge(oracle, "B", "streams", cw, mm, _blocks_b(lay), _streams(engine, mem, n, pitch, nb, cw, mm))


# ------------------------------------------------------------------------------------------------ C: parse phases
@pytest.mark.parametrize("cw,mm", WINDOWS)
def test_parse_phases_one_wave(engine, oracle, cw, mm):
    fam = craft.family_c(cw, mm)
    cases = fam[N7] + fam[N0]
    _judge(oracle, "C", "one wave", cw, mm, cases, _one_wave_ragged(engine, [b for _, b in cases], _flat(cases) + bytes(64), cw, mm))


@pytest.mark.parametrize("cw,mm", WINDOWS)
def test_parse_phases_streams(engine, oracle, cw, mm):
    for n, cases in craft.family_c(cw, mm).items():
        _judge(oracle, "C", "streams", cw, mm, cases, _streams(engine, _flat(cases) + bytes(64), n, n, len(cases), cw, mm))


# ------------------------------------------------------------------------------------------------ D: block ends at a seam
@pytest.mark.parametrize("cw,mm", WINDOWS)
def test_block_ends_one_wave(engine, oracle, cw, mm):
    """the blocks of one body back to back: behind each block's end its period goes on"""
    fam = craft.family_d(cw, mm)
    for per in craft.bodies_d(cw):
        blocks, flat = craft.d_flat(cw, mm, per)
        cases = [c for n in craft.sizes_d() for c in fam[n] if fields(c[0])["per"] == per]
        assert [b for _, b in cases] == blocks
        _judge(oracle, "D", "one wave", cw, mm, cases, _one_wave_ragged(engine, blocks, flat, cw, mm))


@pytest.mark.parametrize("cw,mm", WINDOWS)
def test_block_ends_streams(engine, oracle, cw, mm):
    """one call per size, the three bodies at a pitch of the size rounded up to 16 and 16 more, the continuation in the gap"""
    for n, cases in craft.family_d(cw, mm).items():
        pitch = (n + 15) // 16 * 16 + 16
        mem = b"".join(b + craft.tail_d(b, fields(lab)["per"], pitch - n) for lab, b in cases) + bytes(64)
        _judge(oracle, "D", "streams", cw, mm, cases, _streams(engine, mem, n, pitch, len(cases), cw, mm))


# ------------------------------------------------------------------------------------------------ one stream at a time
@pytest.mark.parametrize("cw,mm", WINDOWS)
def test_one_stream_every_phase_case_and_every_eighth_of_the_others(engine, oracle, cw, mm):
    for fam, name in ((craft.family_c(cw, mm), "C"), (craft.family_a(cw, mm), "A")):
        cases = [c for n in fam for c in fam[n]]
        cases = cases if name == "C" else _every_eighth(cases)
        _judge(oracle, name, "one stream", cw, mm, cases, [_one_stream(engine, _padded(b), len(b), cw, mm) for _, b in cases])
    for lay in craft.family_b(cw, mm):                       # inside the layout's buffer: the neighbours on both sides, any alignment
        lab, n, pitch, nb, mem = lay
        d_mem = _device(mem)
        ks = list(range(nb))[::8]
        cases = [_blocks_b(lay)[k] for k in ks]
        _judge(oracle, "B", "one stream", cw, mm, cases, [_one_stream(engine, d_mem[k * pitch:], n, cw, mm) for k in ks])
    fam = craft.family_d(cw, mm)
    cases = _every_eighth([c for n in fam for c in fam[n]])
    got = [_one_stream(engine, _padded(b, craft.tail_d(b, fields(lab)["per"], 24)), len(b), cw, mm) for lab, b in cases]
    _judge(oracle, "D", "one stream", cw, mm, cases, got)


# ------------------------------------------------------------------------------------------------ sessions
def _sessions(engine, oracle, family, cases, cw, mm):
    _judge(oracle, family, "session, calls end around the seams", cw, mm, cases,
           [_session(engine, b, cw, mm, SESSION_ENDS) for _, b in cases])
    _judge(oracle, family, "session, one call", cw, mm, cases, [_session(engine, b, cw, mm, []) for _, b in cases])


@pytest.mark.parametrize("cw,mm", craft.SESSION_WINDOWS)
def test_lone_matches_session(engine, oracle, cw, mm):
    _sessions(engine, oracle, "A", craft.family_a(cw, mm)[N0], cw, mm)


@pytest.mark.parametrize("cw,mm", craft.SESSION_WINDOWS)
def test_parse_phases_session(engine, oracle, cw, mm):
    _sessions(engine, oracle, "C", craft.family_c(cw, mm)[N0], cw, mm)


# ------------------------------------------------------------------------------------------------ E: long chains
@pytest.mark.parametrize("cw,mm", craft.CHAIN_WINDOWS)
def test_chains_across_the_chunk_seams(engine, oracle, cw, mm):
    cases = [craft.chain_e(t, v) for t in craft.TILES_E for v in range(len(craft.VARIANTS_E))]
    _judge(oracle, "E", "one stream", cw, mm, cases, [_one_stream(engine, _padded(b), len(b), cw, mm) for _, b in cases])


@pytest.mark.parametrize("variant", range(len(craft.VARIANTS_E)))
def test_chain_of_two_chunks_per_lane(engine, oracle, variant):
    """64 * 256 + 1 tiles and 5 bytes (33.6 MB): 65 chunks, the first stream in the suite with K = 2 in the top scans"""
    case = craft.chain_e(craft.BIG_TILES_E, variant)
    _judge(oracle, "E", "one stream", 32, 10, [case], [_one_stream(engine, _padded(case[1]), len(case[1]), 32, 10)])


def test_chain_of_257_tiles_on_one_wave(engine, oracle):
    """MANY_WAVES = 0 keeps a one-row batch of a large block on hdlz_compress_batch: one wave carries the phase through 257 tiles"""
    import torch
    saved = engine.MANY_WAVES
    engine.MANY_WAVES = 0
    try:
        for cw, mm in craft.CHAIN_WINDOWS:
            for v in range(len(craft.VARIANTS_E)):
                lab, b = craft.chain_e(257, v)
                d = _padded(b)
                pitch = d.numel() - 16
                out, ol, st = engine.compress_batch(d[:pitch].view(1, pitch), in_len=len(b), cwindow=cw, maxmatch=mm)
                torch.cuda.synchronize()
                _judge(oracle, "E", "one wave", cw, mm, [(lab, b)], _rows(out, ol, st))
    finally:
        engine.MANY_WAVES = saved
