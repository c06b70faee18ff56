"""GPU (-m gpu): the crafted dynamic-tree headers of tests/deflate_craft.py on every inflate decoder.

Three hand-written table builders read a dynamic block header -- k_inflate_tok<true, CAP_SMALL / CAP_FULL> (the lane mapping's second
pass: flags = 2), k_inflate_dyn (one wave per stream: the default of a small batch, flags = 4, the sessions, the checked call's serial
pass, the BGZF readers' member view) and k_any_* (the whole-GPU path of large streams) -- and stock zlib's encoder feeds them a small
corner of what they must accept and nothing of what they must reject.  Here they get 15-bit codes, a 7-bit code-length code, 143 / 144 /
145 / 286 coded symbols (the CAP_SMALL boundary), one-code and empty distance sets, repeats that run from the literal/length lengths
into the distance lengths, trees that alternate between 286 symbols and two (a table row left over from the block before), headers at
every bit offset, every rejected header of the catalogue, streams cut at every byte and bits flipped INSIDE headers.  The expectation is
the C oracle's status, length and bytes -- which tests/test_crafted_trees_cpu.py holds against stock zlib on the same streams -- and,
for the valid ones, the plain bytes the generator computed from its own tokens."""
import gzip
import random
import zlib

import numpy as np
import pytest

import bgzf_ref
import checked_ref as R
import deflate_craft as C

pytestmark = pytest.mark.gpu
MAPPINGS = (0, 2, 4, 64)      # the default and the three hints of test_gpu_parity.py
_ref = {}


def _oracle(oracle, z, cap):
    """the oracle's (status, bytes) of a stream at an output capacity, computed once per process"""
    key = (z, cap)
    if key not in _ref:
        _ref[key] = oracle.inflate(z, out_cap=cap)
    return _ref[key]


def _small_streams():
    """-> (labels, streams): the catalogue, the cut streams, the 300 random streams and the header flips"""
    S = C.suite()
    labels = [c.name for c in S["catalogue"]] + ["cut %d" % k for k in range(len(S["cuts"]))] + [c.name for c in S["random"]] + \
             ["flip %d" % k for k in range(len(S["flips"]))]
    return labels, [c.z for c in S["catalogue"]] + S["cuts"] + [c.z for c in S["random"]] + S["flips"]


def _ragged(engine, zs, pitch, flags, in_len=None):
    import torch
    flat = torch.from_numpy(np.frombuffer(b"".join(zs) + bytes(64), np.uint8).copy()).cuda()
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum([len(z) for z in zs])]).astype(np.int64)).cuda()
    out, ol, st = engine.inflate_batch(flat, in_off=offs, in_len=in_len, out_pitch=pitch, flags=flags)
    torch.cuda.synchronize()
    return out.cpu().numpy(), ol.cpu().numpy(), st.cpu().numpy()


def _compare(oracle, labels, zs, pitch, out, ol, st, what):
    wrong = []
    for k, z in enumerate(zs):
        rc, ref = _oracle(oracle, z, pitch)
        if (int(st[k]), int(ol[k])) != (rc, len(ref)) or out[k, :len(ref)].tobytes() != ref:
            wrong.append((labels[k], "status %d length %d" % (st[k], ol[k]), "oracle: status %d length %d" % (rc, len(ref))))
    assert not wrong, (what, len(wrong), wrong[:12])


# ------------------------------------------------------------------------------------------------------ small streams, all mappings
@pytest.mark.parametrize("flags", MAPPINGS)
def test_small_streams_every_mapping(engine, oracle, flags):
    """one ragged batch of every small stream, at a capacity of 64 KiB and at 16 bytes (rounded to the 4 the call asks for) below the
    largest output: status, length and bytes are the oracle's"""
    labels, zs = _small_streams()
    S = C.suite()
    for c in S["catalogue"] + S["random"]:                        # the oracle's word is the generator's own
        assert _oracle(oracle, c.z, 65536) == (c.status, c.plain or b""), c.name
    largest = max(len(c.plain) for c in S["catalogue"] + S["random"] if c.status == 0)
    assert 32768 < largest <= 65536 - 16
    for pitch in (65536, (largest - 16) // 4 * 4):
        out, ol, st = _ragged(engine, zs, pitch, flags)
        _compare(oracle, labels, zs, pitch, out, ol, st, ("flags", flags, "pitch", pitch))
    short = [k for k, z in enumerate(zs) if _oracle(oracle, z, (largest - 16) // 4 * 4)[0] == 2]
    assert len(short) >= 2                                        # (the two all-symbols streams ran out of room)


# ------------------------------------------------------------------------------------------------------ the whole-GPU path
def _large_cap():
    return (max(len(p) for _, _, p in C.large() if p is not None) + 4096 + 15) // 16 * 16


@pytest.mark.parametrize("flags", (0, 4))
def test_large_streams_one_at_a_time(engine, oracle, flags):
    """six streams of 40 crafted blocks (60 .. 80 KB, 0.4 .. 0.6 MB plain), the all-symbols stream, eight header flips of each and three
    streams with a header in the middle that must be rejected although its block could be decoded, each as one call: by default the
    chain that searches every bit position for a header (k_any_*), or whatever it falls back to; flags = 4: one wave.  No timing is
    asserted: headers this unlike zlib's may make the chain give a stream up, and the serial decoder's answer is as good"""
    cap = _large_cap()
    wrong = []
    for label, z, plain in C.large():
        rc, ref = _oracle(oracle, z, cap)
        if plain is not None:
            assert (rc, ref) == (0, plain) and zlib.decompress(z) == plain, label
        st, got = engine.inflate_bytes(z, out_cap=cap, flags=flags)
        if (st, got) != (rc, ref):
            wrong.append((label, st, len(got), rc, len(ref)))
    assert not wrong, wrong


@pytest.mark.parametrize("flags", (0, 4))
def test_large_streams_in_batches(engine, oracle, flags):
    """the same streams together: one fixed-pitch batch and one ragged batch with a stated bound (the shapes that take the whole-GPU path
    stream by stream)"""
    import torch
    cap = _large_cap()
    L = C.large()
    labels, zs = [l for l, _, _ in L], [z for _, z, _ in L]
    pitch = (max(len(z) for z in zs) + 64 + 15) // 16 * 16
    assert min(len(z) for z in zs) >= 16384                        # (HDLZ_INFLATE_PAR_LONG: up to 4096 such streams take that path)
    host = np.zeros((len(zs), pitch), np.uint8)
    for k, z in enumerate(zs):
        host[k, :len(z)] = np.frombuffer(z, np.uint8)
    # fixed pitch: every stream is followed by zero padding, and in_len = the pitch.  The oracle reads the same padded rows
    out, ol, st = engine.inflate_batch(torch.from_numpy(host).cuda(), in_len=pitch, out_pitch=cap, flags=flags)
    torch.cuda.synchronize()
    out, ol, st = out.cpu().numpy(), ol.cpu().numpy(), st.cpu().numpy()
    rows = [host[k].tobytes() for k in range(len(zs))]
    _compare(oracle, labels, rows, cap, out, ol, st, ("fixed pitch", flags))
    for k, (_, _, plain) in enumerate(L):
        if plain is not None:
            assert st[k] == 0 and out[k, :ol[k]].tobytes() == plain
    out, ol, st = _ragged(engine, zs, cap, flags, in_len=pitch)
    _compare(oracle, labels, zs, cap, out, ol, st, ("ragged with a bound", flags))


# ------------------------------------------------------------------------------------------------------ sessions
def _feed(engine, z, r, pieces, window=4096):
    """the stream in the given pieces, the output limit growing by random amounts as in test_gpu_sessions._feed_inflate"""
    s = engine.inflate_session()
    i, limit, guard, k = 0, window, 0, 0
    while not s.done:
        guard += 1
        assert guard < 200000
        if i < len(z):
            n = pieces[k] if k < len(pieces) else len(z) - i
            k += 1
            s.write(z[i:i + n])
            i += n
        st = s.step(final=(i >= len(z)), out_limit=limit)
        if st != 0:
            return st, b""
        assert s.out_pos <= limit
        if s.need == 2 or r.random() < 0.3:
            limit += r.randint(1, window)
    return 0, s.output(0, s.out_pos)


def _session_cases():
    cat = C.suite()["catalogue"]
    rejected = [c for c in cat if c.status != 0]
    names = ("first_op_is_16", "repeat_overruns", "no_end_of_block", "literals_oversubscribed", "distances_incomplete_two_codes",
             "single_distance_code_of_length_5", "end_of_block_only_length_3", "code_length_code_incomplete", "hlit_287",
             "unused_code_of_one_distance_code", "distance_before_the_start")
    return [c for c in cat if c.status == 0] + [c for c in rejected if c.name in names]


@pytest.mark.parametrize("how", ("bytes", "pieces"))
def test_sessions(engine, oracle, how):
    """every valid catalogue stream and eleven rejected ones through engine.inflate_session, a byte per call and in random pieces of up
    to 50 bytes.  A byte per call: up to 800 bytes behind the end of every header -- a session parses a dynamic header once 700 bytes
    behind its start are there (or the stream has ended), so it is looked at again after every one of those bytes --; what lies further
    behind a header, which only the three streams with kilobytes of literals have, comes in pieces of up to 4096"""
    r = random.Random(81)
    for c in _session_cases():
        rc, ref = oracle.inflate(c.z)
        assert rc == c.status
        if how == "pieces":
            pieces = []
            while sum(pieces) < len(c.z):
                pieces.append(r.randint(1, 50))
        else:
            near = np.zeros(len(c.z), bool)
            for a, b in c.spans:
                near[max(0, (a >> 3) - 2):(b >> 3) + 800] = True
            pieces, i = [], 0
            while i < len(c.z):
                n = 1 if near[i] else min(4096, len(c.z) - i, int(np.argmax(near[i:])) or len(c.z))
                pieces.append(n)
                i += n
        st, got = _feed(engine, c.z, r, pieces)
        assert (st, got) == (rc, ref if rc == 0 else b""), (c.name, how, st, len(got))


# ------------------------------------------------------------------------------------------------------ the checked call
@pytest.mark.parametrize("flags", MAPPINGS)
def test_checked_call(engine, oracle, flags):
    """the valid catalogue and random streams: status 0, every byte consumed, the checksum of the plain bytes; the rejected ones: the
    decoder's status, the two newly rejected single-code headers among them"""
    S = C.suite()
    cases = S["catalogue"] + S["random"]
    zs = [c.z for c in cases]
    rows, ol, st, used, ad = R.run_ragged(engine, zs, 65536, flags=flags)
    for k, c in enumerate(cases):
        if c.status == 0:
            assert (st[k], ol[k], used[k], ad[k]) == (0, len(c.plain), len(c.z), zlib.adler32(c.plain)), (c.name, st[k], ol[k], used[k])
            assert rows[k, :ol[k]].tobytes() == c.plain, c.name
        else:
            assert (st[k], ol[k], used[k], ad[k]) == (c.status, 0, 0, 0), (c.name, st[k])
    by_name = dict((c.name, k) for k, c in enumerate(cases))
    for name in ("single_distance_code_of_length_5", "end_of_block_only_length_3"):
        assert st[by_name[name]] == C.E_BAD_TREE


# ------------------------------------------------------------------------------------------------------ BGZF
def test_bgzf_members_with_crafted_trees(engine):
    """22 raw crafted streams, each a BGZF member (at most 64 KiB either way): inflate_bgzf returns the data, read_bgzf the slices of
    three ranges that straddle member seams -- the empty member and the two 40 KB ones among them"""
    import torch
    S = C.suite()
    valid = [c for c in S["catalogue"] if c.status == 0]
    chosen = valid[:15] + valid[16::2] + S["random"][:3]
    assert len(chosen) == 22 and all(len(c.raw) + 26 <= 65536 and len(c.plain) <= 65536 for c in chosen)
    f = b"".join(bgzf_ref.frame(c.raw, zlib.crc32(c.plain), len(c.plain)) for c in chosen) + bgzf_ref.EOF
    data = b"".join(c.plain for c in chosen)
    assert gzip.decompress(f) == data
    w = bgzf_ref.walk(f)
    assert (w.status, w.nmembers, w.total_out) == (0, 23, len(data))
    d_file = torch.from_numpy(np.frombuffer(f, np.uint8).copy()).cuda()
    assert engine.inflate_bgzf(d_file).cpu().numpy().tobytes() == data
    seams = w.out_off
    assert seams[2] == seams[3]                                    # (member 2 is the block that is only an end-of-block code)
    ranges = [(seams[1] - 100, seams[1] + 100), (seams[2] - 7, seams[4] + 9), (seams[5] - 3000, seams[9] + 1)]
    out, roff = engine.read_bgzf(d_file, ranges)
    assert roff.cpu().tolist() == np.cumsum([0] + [b - a for a, b in ranges]).tolist()
    assert out.cpu().numpy().tobytes() == b"".join(data[a:b] for a, b in ranges)
