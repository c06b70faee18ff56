"""GPU (-m gpu): the tile body of the compress kernels on the crafted inputs of tests/tile_diet_craft.py.

What is under test: the mismatch word of the NEXT lane in the bit-sliced search and its extension (three-byte matches whose second or
third byte lies behind a lane seam, at every distance; longer ones that read both words), lane 63, which has no next lane (nothing at or
behind n - 4 may match), the LUT entries -- the bit count a lane sums (288 bits at most) and the widest pair of codes (a nine-bit
literal and an 18-bit match) through every kernel that emits codes --, the start flags of token_codes (matches back to back at every
length, a match that ends at a lane's or the tile's last position, small blocks that end inside a lane) and the cap of the extension
(runs up to and beyond MAXMATCH 10 and 5, windows 32 and 20).  Every stream is compared with the C oracle on status, length and every
byte and read back by zlib.  tests/test_tile_diet_cpu.py holds the premises -- that every input shows its token -- without a GPU.

With lengths of at most 10 a lane of 32 positions always starts at least three tokens: "a lane that starts no token" exists only as the
idle lanes of a packed small batch (sizes 5, 33, 100 below), not in a one-tile block; the fewest starts are those of the length-10 chain."""
import zlib

import numpy as np
import pytest

import compress_craft as craft
import tile_diet_craft as diet

pytestmark = pytest.mark.gpu
BOUND = {"tile": 2048, "small": None, "wide": 4096}


def _device(data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def _ragged(engine, blocks, cw, mm, bound):
    """the blocks back to back as ONE ragged batch with the stated bound on their lengths -> [(status, stream)]"""
    import torch
    off = np.cumsum([0] + [len(b) for b in blocks]).astype(np.int64)
    out, ol, st = engine.compress_batch(_device(b"".join(blocks) + bytes(64)), in_off=torch.from_numpy(off).cuda(), cwindow=cw,
                                        maxmatch=mm, max_len=bound)
    torch.cuda.synchronize()
    out, ol, st = out.cpu().numpy(), ol.cpu().numpy(), st.cpu().numpy()
    return [(int(st[k]), out[k, :ol[k]].tobytes()) for k in range(len(ol))]


def _padded(b):
    return _device(b.ljust((len(b) + 15) // 16 * 16 + 16, b"\0"))


def _stream(engine, b, cw, mm):
    out, ol, st = engine.compress_stream(_padded(b), len(b), cwindow=cw, maxmatch=mm)
    k = int(ol.cpu()[0])
    return int(st.cpu()[0]), out[:max(k, 0)].cpu().numpy().tobytes()


def _session(engine, b, cw, mm, ends):
    ses = engine.compress_session(cwindow=cw, maxmatch=mm)
    known = 0
    for q in ends:
        ses.write(b[known:q + 11])
        known = q + 11
        assert ses.step(max_positions=q - ses.pos) == 0 and ses.pos == q and not ses.done
    ses.write(b[known:])
    st = ses.step(final=True)
    assert ses.done
    return st, ses.output(0, ses.out_len)


def _run(engine, cases):
    """every case on its route, the batch routes one call per (route, cwindow, maxmatch) -> results in the order of `cases`"""
    res = [None] * len(cases)
    groups = {}
    for k, c in enumerate(cases):
        if c.route == "stream":
            res[k] = _stream(engine, c.data, c.cw, c.mm)
        elif c.route == "session":
            res[k] = _session(engine, c.data, c.cw, c.mm, [2048])
        else:
            groups.setdefault((c.route, c.cw, c.mm), []).append(k)
    for (route, cw, mm), ks in groups.items():
        blocks = [cases[k].data for k in ks]
        bound = BOUND[route] or max(len(b) for b in blocks)
        assert max(len(b) for b in blocks) <= bound and (route != "small" or bound <= 1024) and (route != "tile" or bound > 1024)
        for k, r in zip(ks, _ragged(engine, blocks, cw, mm, bound)):
            res[k] = r
    return res


def _judge(oracle, cases, results):
    wrong = []
    for c, (st, got) in zip(cases, results):
        rc, ref = craft.expect(oracle, c.data, c.cw, c.mm)
        if not (rc == 0 and st == 0 and got == ref):
            wrong.append((c, st, ref, got))
            continue
        assert zlib.decompress(got) == c.data, c.label
    if wrong:
        c, st, ref, got = wrong[0]
        raise AssertionError("%d of %d streams differ from the oracle; first: %r (%s, cwindow %d, maxmatch %d) status %d, %s" % (
            len(wrong), len(cases), c.label, c.route, c.cw, c.mm, st, craft.first_wrong_token(oracle, c.data, c.cw, c.mm, ref, got)))


@pytest.mark.parametrize("family", [diet.lane_seams, diet.lane63, diet.bit_sums, diet.wide_codes, diet.start_flags, diet.sentinel_runs],
                         ids=lambda f: f.__name__)
def test_crafted_tiles_against_the_oracle(engine, oracle, family):
    cases = family()
    _judge(oracle, cases, _run(engine, cases))


def test_nine_bit_lanes_through_the_other_kernels(engine, oracle):
    """the 288-bit lanes (2048 nine-bit literals, then the same twice and eight times) through the small, the multi-tile, the stream
    and the session kernels: their bit counts come from the same entries"""
    nine = diet.bit_sums()[0].data
    mk = lambda lab, data, route: diet.Case(lab, data, 32, 10, route, (("all_lit",),))
    cases = [mk("nine small", nine[:1024], "small"), mk("nine small odd", nine[:1001], "small"), mk("nine wide", nine + nine[::-1], "wide"),
             mk("nine stream", (nine + nine[::-1]) * 4, "stream"), mk("nine session", nine + nine[::-1], "session")]
    _judge(oracle, cases, _run(engine, cases))
