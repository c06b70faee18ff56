"""GPU (-m gpu): the crafted match geometry of tests/deflate_craft.py on every inflate decoder.

Every decoder keeps its recent output in a small LDS ring and serves a match from the ring, from its own flushed output or from a marker
that is resolved later; which, is decided by comparisons of the distance and the length with constants of the kernel: k_inflate_tok
(a lane per stream; flags = 2) NEAR = RINGB - 16 and the far load whose safety rests on URGENT and the 19 bytes of a round; k_inflate_grp
(16 lanes per stream; flags = 64) NEAR = RB - 32 and FLUSH; k_inflate_dyn (a wave per stream; flags = 4, the sessions, the checked
call's serial pass, the BGZF member view) D + len <= DRING - 512, the parallel copy against the serial `i % D` loop, the decode window
cut at WCAP; k_par_emit / k_any_* (the whole GPU) HREACH = HRING - 128, SPAN and the chains through a batch's own bytes.  What stock
encoders write meets those comparisons by accident.  Here every decoder gets, for each of 116 distances on and next to the thresholds
(tests/test_match_geometry_cpu.py recomputes them from the kernels' sources), a stream of 39 matches of every interesting length behind
random literals, in a fixed and in a dynamic block -- the dynamic code from the frequencies, so that three matches fall into one 64-bit
window --, matches that reach byte 0 and one byte before it, and 1 MiB of all distances and lengths mixed.  The expectation is the C
oracle's status, length and bytes at the same capacity and flags -- the CPU file holds the oracle against stock zlib on the same
streams -- and, for the valid ones, the plain bytes the generator computed from its own tokens."""
import gzip
import time
import zlib

import numpy as np
import pytest

import bgzf_ref
import checked_ref as R
import deflate_craft as C

pytestmark = pytest.mark.gpu
MAPPINGS = (0, 2, 4, 64)      # the default and the three hints of test_gpu_parity.py
ONE_FIXED_BLOCK = 128         # HDLZ_INFLATE_ONE_FIXED_BLOCK
_ref = {}


def _oracle(oracle, z, cap, flags=0, obsize=0):
    """the oracle's (status, bytes) of a stream at an output capacity, flags and obsize, computed once per process"""
    key = (z, cap, flags, obsize)
    if key not in _ref:
        _ref[key] = oracle.inflate(z, out_cap=cap, flags=flags, obsize=obsize)
    return _ref[key]


def _ragged(engine, zs, pitch, flags, in_len=None, obsize=0):
    import torch
    flat = torch.from_numpy(np.frombuffer(b"".join(zs) + bytes(64), np.uint8).copy()).cuda()
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum([len(z) for z in zs])]).astype(np.int64)).cuda()
    out, ol, st = engine.inflate_batch(flat, in_off=offs, in_len=in_len, out_pitch=pitch, flags=flags, obsize=obsize)
    torch.cuda.synchronize()
    return out.cpu().numpy(), ol.cpu().numpy(), st.cpu().numpy()


def _compare(oracle, labels, zs, pitch, out, ol, st, what, flags=0, obsize=0):
    wrong = []
    for k, z in enumerate(zs):
        rc, ref = _oracle(oracle, z, pitch, flags, obsize)
        if (int(st[k]), int(ol[k])) != (rc, len(ref)) or out[k, :len(ref)].tobytes() != ref:
            wrong.append((labels[k], "status %d length %d" % (st[k], ol[k]), "oracle: status %d length %d" % (rc, len(ref))))
    assert not wrong, (what, len(wrong), wrong[:12])


def _batch_cases():
    G = C.geometry()
    return G["short"] + G["reach"] + G["short_by_one"] + G["obsize"]


# ------------------------------------------------------------------------------------------------------ the batch kernels
@pytest.mark.parametrize("flags", MAPPINGS)
def test_batch_every_mapping(engine, oracle, flags):
    """the 232 short-preamble streams and the streams that reach byte 0 or one byte before it, as one ragged batch, at a capacity that
    holds everything and at three that cut rows inside matches and inside preambles (E_OUT_CAPACITY has to come from the right token):
    status, length and bytes are the oracle's.  Every stream's 39 matches alone are 2787 bytes behind at least 64 literals, so 1000 and
    2304 cut all 232 of them (what fits there are the short streams that reach byte 0); 3072 lies in the middle of the lengths of the
    streams with D <= 131 (2908 .. 3100 bytes) and has both arms"""
    cases = _batch_cases()
    assert len(cases) == 232 + 12 + 10 + 4
    labels, zs = [c.name for c in cases], [c.z for c in cases]
    for c in cases:                                               # the oracle's word is the generator's own
        assert _oracle(oracle, c.z, 65536) == (c.status, c.plain or b""), c.name
    for pitch in (65536, 3072, 2304, 1000):
        out, ol, st = _ragged(engine, zs, pitch, flags)
        _compare(oracle, labels, zs, pitch, out, ol, st, ("flags", flags, "pitch", pitch), flags)
    for pitch in (1000, 2304, 3072):                                                 # neither arm is empty
        assert sum(1 for z in zs if _oracle(oracle, z, pitch, flags)[0] == 2) >= 100, pitch
    assert sum(1 for z in zs if _oracle(oracle, z, 3072, flags)[0] == 0) >= 100


@pytest.mark.parametrize("flags", MAPPINGS)
def test_obsize_at_the_distance(engine, oracle, flags):
    """streams whose only matches are (10, D) and (10, D + 1), decoded with an OBSIZE of D - 1, D, D + 1 and 0: E_BAD_DISTANCE exactly
    for a non-zero obsize below D + 1.  The four streams as one batch under every obsize, and each alone through inflate_bytes"""
    obs = C.geometry()["obsize"]
    assert [c.D for c in obs] == list(C.OBSIZE_D)
    labels, zs = [c.name for c in obs], [c.z for c in obs]
    for c in obs:
        for obsize in (c.D - 1, c.D, c.D + 1, 0):
            rc, ref = _oracle(oracle, c.z, 4096, flags, obsize)
            assert rc == (C.E_BAD_DISTANCE if obsize and obsize < c.D + 1 else 0) and ref == (c.plain if rc == 0 else b"")
            out, ol, st = _ragged(engine, zs, 4096, flags, obsize=obsize)
            _compare(oracle, labels, zs, 4096, out, ol, st, ("flags", flags, "obsize", obsize), flags, obsize)
            assert engine.inflate_bytes(c.z, out_cap=4096, flags=flags, obsize=obsize) == (rc, ref), (c.name, flags, obsize)


# ------------------------------------------------------------------------------------------------------ the whole-GPU path, stream by stream
def _long():
    G = C.geometry()["long"]
    assert len(G) == 232 and min(len(c.z) for c in G) >= 4400              # above HDLZ_INFLATE_PAR_MIN (2048) and ANY_MIN (4096)
    return G


@pytest.mark.parametrize("flags", (0, 4, ONE_FIXED_BLOCK))
def test_long_preamble_one_at_a_time(engine, oracle, flags):
    """the 232 streams with a preamble of 4400 literals or more, each as one call: by default the fixed-block chain (k_par_*: inflate_bytes
    sees a single fixed block and sets the hint) or the chain for any block types (k_any_*), flags = 4: one wave; the fixed ones also
    with the hint given by the caller"""
    wrong = []
    for c in _long():
        if flags == ONE_FIXED_BLOCK and c.kind != "fixed":
            continue
        assert _oracle(oracle, c.z, 65536, flags) == (0, c.plain), c.name
        st, got = engine.inflate_bytes(c.z, out_cap=65536, flags=flags)
        if (st, got) != (0, c.plain):
            wrong.append((c.name, st, len(got), len(c.plain)))
    assert not wrong, (len(wrong), wrong[:12])


@pytest.mark.parametrize("flags", (0, 4))
def test_long_preamble_in_batches(engine, oracle, flags):
    """the same streams together: one fixed-pitch batch with in_len = the pitch -- zero padding stands behind every stream, and the
    oracle reads the same padded rows -- and one ragged batch with the stated bound"""
    import torch
    L = _long()
    labels, zs = [c.name for c in L], [c.z for c in L]
    cap = 65536
    pitch = (max(len(z) for z in zs) + 64 + 15) // 16 * 16
    host = np.zeros((len(zs), pitch), np.uint8)
    for k, z in enumerate(zs):
        host[k, :len(z)] = np.frombuffer(z, np.uint8)
    out, ol, st = engine.inflate_batch(torch.from_numpy(host).cuda(), in_len=pitch, out_pitch=cap, flags=flags)
    torch.cuda.synchronize()
    out, ol, st = out.cpu().numpy(), ol.cpu().numpy(), st.cpu().numpy()
    rows = [host[k].tobytes() for k in range(len(zs))]
    _compare(oracle, labels, rows, cap, out, ol, st, ("fixed pitch", flags), flags)
    for k, c in enumerate(L):
        assert st[k] == 0 and out[k, :ol[k]].tobytes() == c.plain, c.name
    out, ol, st = _ragged(engine, zs, cap, flags, in_len=pitch)
    _compare(oracle, labels, zs, cap, out, ol, st, ("ragged with a bound", flags), flags)
    for k, c in enumerate(L):
        assert st[k] == 0 and out[k, :ol[k]].tobytes() == c.plain, c.name


# ------------------------------------------------------------------------------------------------------ the whole-GPU path, large
def _timed(engine, z, cap, flags):
    import torch
    zin = torch.frombuffer(bytearray(z + bytes(64)), dtype=torch.uint8).cuda().reshape(1, -1)
    engine.inflate_batch(zin, in_len=len(z), out_pitch=cap, flags=flags)
    torch.cuda.synchronize()
    best = None
    for _ in range(1 if flags & 4 else 3):               # (best of three: a clock tick of the box must not fail the test)
        t0 = time.time()
        engine.inflate_batch(zin, in_len=len(z), out_pitch=cap, flags=flags)
        torch.cuda.synchronize()
        dt = time.time() - t0
        best = dt if best is None else min(best, dt)
    return best


def test_mixed_geometry_one_mib(engine, oracle):
    """1 MiB of random (length, distance) pairs from the two grids behind 33000 literals, as one fixed block and as three dynamic
    blocks: status and bytes under the default mapping, on one wave and, the fixed one, with the one-fixed-block hint.  The fixed stream
    must have been taken by the parallel chain -- the bar of test_far_history_and_deep_marker_chains: at least 5x faster than one wave
    --; the chain for any block types may hand blocks of the dynamic one to the serial pass, so its times are only printed"""
    fixed, dyn = C.geometry_large()
    cap = (1 << 20) + 4096
    for c in (fixed, dyn):
        assert zlib.decompress(c.z) == c.plain
        for flags in (0, 4) + ((ONE_FIXED_BLOCK,) if c is fixed else ()):
            assert _oracle(oracle, c.z, cap, flags) == (0, c.plain), (c.name, flags)
            st, got = engine.inflate_bytes(c.z, out_cap=cap, flags=flags)
            assert st == 0 and got == c.plain, (c.name, flags, st, len(got))
    t_par, t_wave = _timed(engine, fixed.z, cap, 0), _timed(engine, fixed.z, cap, 4)
    print("mixed geometry, fixed: whole GPU %.2f ms, one wave %.2f ms" % (t_par * 1e3, t_wave * 1e3))
    d_par, d_wave = _timed(engine, dyn.z, cap, 0), _timed(engine, dyn.z, cap, 4)
    print("mixed geometry, dynamic: whole GPU %.2f ms, one wave %.2f ms" % (d_par * 1e3, d_wave * 1e3))
    assert t_par * 5 < t_wave, (len(fixed.z), t_par, t_wave)


# ------------------------------------------------------------------------------------------------------ sessions
def _by_distance(kind):
    return dict((c.D, c) for c in C.geometry()["short"] if c.kind == kind)


@pytest.mark.parametrize("grow", ("by 1 then 449", "by 61"))
def test_sessions_output_side(engine, grow):
    """all input written, final = True, and the output limit growing from the preamble's length by 1 per step for 700 steps and then by
    449 (WCAP + 1), or by 61 throughout: the decoder is parked between every pair of tokens and inside them, and resumes with a ring
    that has to be rebuilt from its output.  After every step the output is a prefix of the plain bytes"""
    dyn = _by_distance("dynamic")
    for D in (1, 3, 113, 1535, 1537, 2049):
        c = dyn[D]
        s = engine.inflate_session()
        s.write(c.z)
        limit, steps = c.first_match, 0
        while True:
            st = s.step(final=True, out_limit=limit)
            assert st == 0 and s.out_pos <= limit, (D, steps, st, s.out_pos, limit)
            assert s.output(0, s.out_pos) == c.plain[:s.out_pos], (D, steps, limit, s.out_pos)
            if s.done:
                break
            assert s.need == 2 and limit <= len(c.plain) + 449, (D, steps, s.need, limit)
            steps += 1
            limit += 61 if grow == "by 61" else 1 if steps <= 700 else 449
        assert s.out_pos == len(c.plain) and s.output(0, s.out_pos) == c.plain, D
        assert steps >= (40 if grow == "by 61" else 700), (D, steps)


@pytest.mark.parametrize("kind", C.GEO_KINDS)
def test_sessions_input_side(engine, kind):
    """the stream in two pieces, cut at every byte from the one in which the first match begins to the end and at every 97th byte of the
    preamble: write, step, write the rest, step(final): status 0, the plain bytes, and the first step produced a prefix of them"""
    by_d = _by_distance(kind)
    for D in (1, 113, 1537):
        c = by_d[D]
        first = 2 + (c.token_pos[c.first_match] >> 3)                  # (.z: two header bytes in front of .raw)
        assert c.first_match * 6 // 8 < first < len(c.z) - 40
        cuts = list(range(97, first, 97)) + list(range(first, len(c.z)))
        for n in cuts:
            s = engine.inflate_session()
            s.write(c.z[:n])
            assert s.step() == 0, (D, n)
            p = s.out_pos
            assert p <= len(c.plain) and s.output(0, p) == c.plain[:p], (D, n, p)
            s.write(c.z[n:])
            assert s.step(final=True) == 0 and s.done, (D, n)
            assert s.out_pos == len(c.plain) and s.output(0, s.out_pos) == c.plain, (D, n)


# ------------------------------------------------------------------------------------------------------ the checked call, the member view
@pytest.mark.parametrize("flags", MAPPINGS)
def test_checked_call(engine, flags):
    """hdlz_inflate_checked over the 232 short-preamble streams: status 0, every byte consumed, the Adler-32 of the plain bytes"""
    cases = C.geometry()["short"]
    rows, ol, st, used, ad = R.run_ragged(engine, [c.z for c in cases], 65536, flags=flags)
    for k, c in enumerate(cases):
        assert (st[k], ol[k], used[k], ad[k]) == (0, len(c.plain), len(c.z), zlib.adler32(c.plain)), (c.name, st[k], ol[k], used[k])
        assert rows[k, :ol[k]].tobytes() == c.plain, c.name


def test_bgzf_members(engine):
    """the 232 raw streams as BGZF members (all fit 64 KiB both ways): inflate_bgzf returns the data, read_bgzf six ranges that begin
    and end inside matches of the members with D = 113, 1537 and 2049"""
    import torch
    cases = C.geometry()["short"]
    assert all(len(c.raw) + 26 <= 65536 and len(c.plain) <= 65536 for c in cases)
    f = b"".join(bgzf_ref.frame(c.raw, zlib.crc32(c.plain), len(c.plain)) for c in cases) + bgzf_ref.EOF
    data = b"".join(c.plain for c in cases)
    assert gzip.decompress(f) == data
    w = bgzf_ref.walk(f)
    assert (w.status, w.nmembers, w.total_out) == (0, 233, len(data))
    d_file = torch.from_numpy(np.frombuffer(f, np.uint8).copy()).cuda()
    assert engine.inflate_bgzf(d_file).cpu().numpy().tobytes() == data
    ranges = []
    for k, c in enumerate(cases):
        if c.D in (113, 1537, 2049):
            # the output offsets at which the matches begin: a range from the middle of the third match to the middle of the last
            # but one (fixed), from one byte into the first match to one byte before the end of the last (dynamic)
            starts, o = [], 0
            for t in c.tokens:
                if not isinstance(t, int):
                    starts.append((o, t[0]))
                o += 1 if isinstance(t, int) else t[0]
            a, b = (starts[2], starts[-2]) if c.kind == "fixed" else (starts[0], starts[-1])
            lo, hi = (a[0] + a[1] // 2, b[0] + b[1] // 2) if c.kind == "fixed" else (a[0] + 1, b[0] + b[1] - 1)
            assert a[0] < lo < a[0] + a[1] and b[0] < hi < b[0] + b[1] and lo < hi
            ranges.append((w.out_off[k] + lo, w.out_off[k] + hi))
    assert len(ranges) == 6
    out, roff = engine.read_bgzf(d_file, ranges)
    assert roff.cpu().tolist() == np.cumsum([0] + [b - a for a, b in ranges]).tolist()
    assert out.cpu().numpy().tobytes() == b"".join(data[a:b] for a, b in ranges)
