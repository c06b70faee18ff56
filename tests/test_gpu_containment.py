"""GPU (-m gpu): where ELSE did a call write?  Every buffer of every C-ABI call here is carved out of a guard-band arena
(tests/guards.py): exact sizes, a band of pattern bytes on each side, every case run on the pattern and on its complement.

  H1  every band is untouched (d_out, d_out_len, d_status, d_work, d_archive, d_off, d_state)
  H2  the read-only regions are untouched (the input and its slack, d_in_off, d_len / d_rows of the archive call)
  H3  status, out_len and out[:out_len] equal the oracle's and are identical in both runs -- the runs differ in every byte the call
      was not given (input slack, scratch, unused output), so the results do not depend on those
  H4  interior rows: rows that fail before their first byte ("silent" rows) stay untouched between loud neighbours, and every row
      kind is the first row of one call and the last row of another (rotations), where H1's bands sit right against it
  H5  how far behind out_len a row is written -- the statements of include/hdlz.h, asserted per path (the EXTENT_* constants)
  H6  the checker, told an extent that is too short, reports the bytes the kernel really wrote there

The direct C-ABI is used (engine.lib), with the _ws variants, so that out_len / status / scratch are the arena's.

Measured on an MI355X when the file was written (each test prints its "H5" lines; run with -s): every compress path (k_compress<*>,
k_compress_small, k_stream_*, k_compress_chunk) writes at most 3 bytes behind out_len -- the word the stream ends in -- and nothing into
the row of a failed block; every inflate path (k_inflate_tok / _grp / _dyn, the whole-GPU chains) writes exactly out_len bytes of an OK
row, up to the whole row of a failed one (status 2: 2048 of 2048, 16777152 of 16777212) and nothing into the row of a stream that fails
before its first byte -- the silent-row check holds for every kernel, none had to be left to the rotations alone.  The scratch of the
whole-GPU path is written up to 132 bytes in front of its end (H6).  With store_words changed to round its word count up to 4 (a copy of
the tree, not kept) test_compress_batch_ragged_rows_at_minimal_pitch fails at its first call: 20 bytes written into the silent rows
behind the loud ones.  The file takes 26 s, the rest of the GPU suite 104 s."""
import random
import zlib

import numpy as np
import pytest
import torch

import guards
from hdl_deflate_amd._lib import CState, IState

pytestmark = pytest.mark.gpu

SALT = 0x3C
WORK_BAND = 1 << 20                       # around scratch: where a caller's arena would hold its next sub-allocation


def row_band(pitch):                      # around rows, out_len, status, states: the nearest neighbours of a caller's own data
    return max(1 << 16, 2 * pitch)


def round4(x):
    return (x + 3) & ~3


# ---- H5: the write extents include/hdlz.h states, per path (what an OK row / a failed row may write of its own row)
EXTENT_WORD = round4                      # compress paths: store_words / the packed flush / k_stream_* store whole 32-bit words
EXTENT_EXACT = int                        # inflate, OK rows: the flushes of k_inflate_tok / _grp / _dyn and k_par_emit end at out_len
FAILED_COMPRESS = 0                       # a compress row that fails is decided before its first store
# a failed inflate row may hold a prefix of what was decoded before the failure: anything inside the row (its pitch)

MEASURED = {}                             # path -> [max (last written byte + 1 - out_len) over OK rows, max last written + 1 over failed rows]


def note(path, ok_excess, fail_tail):
    m = MEASURED.setdefault(path, [None, None])
    if ok_excess is not None:
        m[0] = ok_excess if m[0] is None else max(m[0], ok_excess)
    if fail_tail is not None:
        m[1] = fail_tail if m[1] is None else max(m[1], fail_tail)


def report(prefix):
    for path in sorted(MEASURED):
        if path.startswith(prefix):
            print("H5 %-34s OK rows: last written - out_len <= %s   failed rows: last written + 1 <= %s" %
                  (path, MEASURED[path][0], MEASURED[path][1]))


def two_runs(specs, setup, call, reads):
    """-> (arena of the second run, bytes unwritten in BOTH runs, the regions `reads` of either run as numpy)"""
    clean, runs = None, []
    for salt in (SALT, SALT ^ 0xFF):
        a = guards.Arena(guards.Arena.size_for(specs), "cuda", salt)
        for s in specs:
            a.carve(*s)
        setup(a)
        call(a)
        torch.cuda.synchronize()
        u = a.untouched_flat()
        clean = u if clean is None else clean & u
        runs.append({n: a.view(n).cpu().numpy().copy() for n in reads})
    return a, clean, runs


def judge_rows(label, path, a, clean, runs, B, pitch, exp_st, exp_len, ref, extent, fail_extent, silent=(), extra=None, told=None):
    """H1 .. H5 of one call whose output is B rows of `pitch` bytes.  ref: uint8 [B, pitch] (compared where k < exp_len[b]);
    told: {row: extent} overrides (H6 only) -> the violations instead of asserting that there are none"""
    exp_st, exp_len = np.asarray(exp_st, np.uint32), np.asarray(exp_len, np.uint32)
    mask = np.arange(pitch)[None, :] < exp_len[:, None]
    for k, r in enumerate(runs):                                                        # H3
        st, ol = r["status"].view(np.uint32), r["out_len"].view(np.uint32)
        assert np.array_equal(st, exp_st), (label, k, np.nonzero(st != exp_st)[0][:8], st[st != exp_st][:8], exp_st[st != exp_st][:8])
        assert np.array_equal(ol, exp_len), (label, k, np.nonzero(ol != exp_len)[0][:8], ol[ol != exp_len][:8], exp_len[ol != exp_len][:8])
        out = r["out"].reshape(B, pitch)
        assert np.array_equal(out[mask], ref[mask]), (label, k, np.nonzero(((out != ref) & mask).any(axis=1))[0][:8])
    for n in ("status", "out_len"):
        assert np.array_equal(runs[0][n], runs[1][n]), (label, n)
    silent = set(silent)
    ext = [extent(int(exp_len[b])) if exp_st[b] == 0 else (0 if b in silent else fail_extent) for b in range(B)]
    assert all(e <= pitch for e in ext), label                                          # "inside the row" is the floor
    for b, e in (told or {}).items():
        ext[b] = e
    allowed = {"out": guards.row_mask(B, pitch, ext, "cuda"), "out_len": True, "status": True}
    allowed.update(extra or {})
    bad = guards.violations(a, clean, allowed)                                          # H1, H2, H4, H5
    if told is not None:
        return bad
    assert bad == [], (label, bad)
    tails = guards.row_tails(a.split(clean)["out"][1], B, pitch).cpu().numpy()
    ok = exp_st == 0
    note(path, int((tails[ok] - exp_len[ok]).max()) if ok.any() else None, int(tails[~ok].max()) if (~ok).any() else None)
    return bad


def rotations(kinds, silents):
    """kinds: [(name, payload)] -> one batch per kind i: k_i, S, k_i+1, S, ..., S, k_i-1 as [(name, payload, is silent)].  Every kind
    is the first row once and the last row once; in the other batches a silent row directly precedes and directly follows it."""
    K = len(kinds)
    assert K >= 2
    for i in range(K):
        rows = []
        for j in range(K):
            if j:
                rows.append(("silent", silents[(i + j) % len(silents)], True))
            rows.append((kinds[(i + j) % K][0], kinds[(i + j) % K][1], False))
        yield rows


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


# =================================================================================================== compress: hdlz_compress_batch
_inc_cache = {}


def incompressible(oracle, n, seed=0):
    """n bytes in 144 .. 255 (9 bits per literal) without a 3-byte match in a window of 256, hence in any smaller one: the output of
    every path is exactly hdlz_out_bound(n) bytes.  Positions where the oracle finds a match are redrawn until it finds none."""
    if (n, seed) in _inc_cache:
        return _inc_cache[(n, seed)]
    rng = np.random.default_rng(1000 + 7 * n + seed)
    d = rng.integers(144, 256, size=n, dtype=np.uint8)
    for _ in range(200):
        if n < 5:
            break
        hit = [p for p, ln, _ in oracle.tokens(d.tobytes(), 256, 10) if ln]
        if not hit:
            break
        for p in hit:
            d[p:p + 3] = rng.integers(144, 256, size=len(d[p:p + 3]), dtype=np.uint8)
    data = d.tobytes()
    if n >= 5:
        for cw in (20, 32, 256):
            rc, z = oracle.compress(data, cw, 10)
            assert rc == 0 and len(z) == oracle.out_bound(n), (n, cw, len(z))
    _inc_cache[(n, seed)] = data
    return data


_ref_cache = {}


def compress_expect(oracle, blk, cw, mm, pitch, bound):
    n = len(blk)
    if n < 5:
        return 1, b""
    if bound and n > bound:
        return 8, b""
    if oracle.out_bound(n) > pitch:
        return 2, b""
    key = (blk, cw, mm)
    if key not in _ref_cache:
        rc, z = oracle.compress(blk, cw, mm)
        assert rc == 0
        _ref_cache[key] = z
    return 0, _ref_cache[key]


def compress_batch_call(engine, oracle, label, path, blocks, cw, mm, pitch, bound=0, mis=0, fixed=None, silent=(), told=None):
    """one guarded hdlz_compress_batch: ragged (in_off; `bound` = the stated in_len) or fixed = (n, in_pitch)"""
    L, B, band = engine.lib, len(blocks), row_band(pitch)
    if fixed:
        n, in_pitch = fixed
        nin = (B - 1) * in_pitch + n
        specs = [("in", nin, 16, band, True, mis)]
    else:
        off = np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).astype(np.int64)
        specs = [("in", int(off[-1]), 16, band, True, mis), ("in_off", 8 * (B + 1), 8, band, True)]
    specs += [("out", B * pitch, 4, band), ("out_len", 4 * B, 4, band), ("status", 4 * B, 4, band)]

    def setup(a):
        if fixed:
            for b, blk in enumerate(blocks):
                a.fill("in", blk, at=b * fixed[1])
        else:
            a.fill("in", b"".join(blocks))
            a.fill("in_off", off.view(np.uint8))

    def call(a):
        rc = L.hdlz_compress_batch(a.ptr("in"), None if fixed else a.ptr("in_off"), fixed[1] if fixed else 0, fixed[0] if fixed else bound,
                                   B, cw, mm, a.ptr("out"), pitch, a.ptr("out_len"), a.ptr("status"), stream_ptr())
        assert rc == 0, (label, L.hdlz_last_error())

    a, clean, runs = two_runs(specs, setup, call, ("out", "out_len", "status"))
    exp = [compress_expect(oracle, blk, cw, mm, pitch, bound) for blk in blocks]
    ref = np.zeros((B, pitch), np.uint8)
    for b, (_, z) in enumerate(exp):
        ref[b, :len(z)] = np.frombuffer(z, np.uint8)
    return judge_rows(label, path, a, clean, runs, B, pitch, [e[0] for e in exp], [len(e[1]) for e in exp], ref, EXTENT_WORD,
                      FAILED_COMPRESS, silent=silent, told=told)


SHORT_BLOCKS = [b"", b"a", b"ab", b"abc", b"abcd"]          # ragged blocks of 0 .. 4 bytes: status 1, nothing written

# (kernel the rows are meant to reach, stated bound, cwindow, block sizes) -- ragged batches, one per size, out_pitch = out_bound(n)
# rounded up to 4, three row kinds per size (incompressible = maximal output, zeros and "abab.." = short outputs) rotated with short blocks
COMPRESS_RAGGED = [
    ("k_compress<1,true,true>", 2048, 32, (1025, 1026, 1500, 2045, 2047, 2048)),
    ("k_compress<1,false,true>", 2048, 20, (1025, 1026, 1500, 2045, 2047, 2048)),
    ("k_compress<1,true,false>", 0, 32, (2049, 2050, 2052, 5000, 70001)),
    ("k_compress<1,false,false>", 0, 20, (2049, 2050, 2052, 5000, 70001)),
    ("k_compress<2,true,false>", 0, 64, (2049, 2050, 2052, 5000, 70001)),
    ("k_compress<2,false,false>", 0, 48, (2049, 2050, 2052, 5000, 70001)),
    ("k_compress<8,true,false>", 0, 256, (2049, 2050, 2052, 5000, 70001)),
    ("k_compress<8,false,false>", 0, 100, (2049, 2050, 2052, 5000, 70001)),
    ("k_compress_small ragged", None, 32, (5, 6, 7, 8, 10, 33, 256, 1024)),        # bound = the size itself
    ("k_compress_small ragged", None, 256, (5, 6, 7, 8, 10, 33, 256, 1024)),
]


def kinds_of_size(oracle, n):
    return [("incompressible", incompressible(oracle, n)), ("zeros", bytes(n)), ("abab", (b"ab" * n)[:n])]


def test_compress_batch_ragged_rows_at_minimal_pitch(engine, oracle):
    for path, bound, cw, sizes in COMPRESS_RAGGED:
        assert {oracle.out_bound(n) % 4 for n in sizes} == {0, 1, 2, 3}, path
        for n in sizes:
            pitch = round4(oracle.out_bound(n))
            for i, rows in enumerate(rotations(kinds_of_size(oracle, n), SHORT_BLOCKS)):
                silent = [b for b, r in enumerate(rows) if r[2]]
                compress_batch_call(engine, oracle, (path, n, i), path, [r[1] for r in rows], cw, 10 if i != 1 else 5, pitch,
                                    bound=n if bound is None else bound, mis=(0, 3, 9)[i], silent=silent)
    report("k_compress")


def test_compress_batch_small_blocks_fixed_pitch_and_bound_violation(engine, oracle):
    """k_compress_small: fixed-pitch batches whose block counts leave a partial group; a ragged batch with a leading misalignment in
    which ONE block violates the stated bound (status 8, nothing written)"""
    path = "k_compress_small fixed pitch"
    for n, B in ((5, 67), (33, 131), (256, 67), (1024, 19)):
        pitch, in_pitch = round4(oracle.out_bound(n)), (n + 15) // 16 * 16
        for first in (0, 1):                                  # B is odd: either kind is the first AND the last row of one call
            blocks = [incompressible(oracle, n, seed=b) if (b + first) % 2 == 0 else (b"ab" * n)[:n] for b in range(B)]
            for cw in (32, 256):
                compress_batch_call(engine, oracle, (path, n, B, first, cw), path, blocks, cw, 10, pitch, fixed=(n, in_pitch))
    path = "k_compress_small ragged"
    kinds = [("incompressible", incompressible(oracle, 100)), ("violator", incompressible(oracle, 101)), ("zeros", bytes(100)),
             ("short", incompressible(oracle, 37)), ("abab", b"ab" * 25)]
    pitch = round4(oracle.out_bound(101))
    for i, rows in enumerate(rotations(kinds, SHORT_BLOCKS)):
        silent = [b for b, r in enumerate(rows) if r[2] or r[0] == "violator"]
        compress_batch_call(engine, oracle, (path, "bound", i), path, [r[1] for r in rows], 32, 10, pitch, bound=100, mis=(3, 7, 1, 13, 2)[i],
                            silent=silent)
    report("k_compress_small")


def test_compress_batch_capacity(engine, oracle):
    """out_pitch < hdlz_out_bound(n): every status is 2, every out_len 0 and the whole of d_out untouched"""
    for n, B, fixed, cw in ((2048, 5, True, 32), (256, 67, True, 32), (5000, 3, True, 64), (1500, 4, False, 32), (300, 70, False, 256)):
        pitch = round4(oracle.out_bound(n)) - 4
        blocks = [incompressible(oracle, n, seed=b % 3) if b % 2 else bytes(n) for b in range(B)]
        compress_batch_call(engine, oracle, ("capacity", n, B, fixed), "capacity", blocks, cw, 10, pitch,
                            bound=0 if fixed else (n if n <= 2048 else 0), fixed=(n, (n + 15) // 16 * 16) if fixed else None)
    assert MEASURED["capacity"] == [None, 0]


# ================================================================================ compress: hdlz_compress_streams / hdlz_compress_stream
def compress_streams_call(engine, oracle, label, blocks, cw=32, mm=10):
    L, B, n = engine.lib, len(blocks), len(blocks[0])
    pitch, in_pitch = round4(oracle.out_bound(n)), (n + 15) // 16 * 16
    wb = L.hdlz_streams_work_bytes(n, B)
    assert wb > 0
    band = row_band(pitch)
    specs = [("in", (B - 1) * in_pitch + n, 16, band, True), ("out", B * pitch, 4, band), ("out_len", 4 * B, 4, band),
             ("status", 4 * B, 4, band), ("work", wb, 8, WORK_BAND)]

    def setup(a):
        for b, blk in enumerate(blocks):
            a.fill("in", blk, at=b * in_pitch)

    def call(a):
        if B == 1:
            rc = L.hdlz_compress_stream(a.ptr("in"), n, cw, mm, a.ptr("out"), pitch, a.ptr("out_len"), a.ptr("status"), a.ptr("work"), wb,
                                        stream_ptr())
        else:
            rc = L.hdlz_compress_streams(a.ptr("in"), in_pitch, n, B, cw, mm, a.ptr("out"), pitch, a.ptr("out_len"), a.ptr("status"),
                                         a.ptr("work"), wb, stream_ptr())
        assert rc == 0, (label, L.hdlz_last_error())

    a, clean, runs = two_runs(specs, setup, call, ("out", "out_len", "status"))
    exp = [compress_expect(oracle, blk, cw, mm, pitch, 0) for blk in blocks]
    ref = np.zeros((B, pitch), np.uint8)
    for b, (_, z) in enumerate(exp):
        ref[b, :len(z)] = np.frombuffer(z, np.uint8)
    judge_rows(label, "k_stream_*", a, clean, runs, B, pitch, [e[0] for e in exp], [len(e[1]) for e in exp], ref, EXTENT_WORD,
               FAILED_COMPRESS, extra={"work": True})


def incompressible32(oracle, n, seed):
    """as incompressible(), for the window of 32 the stream cases use (a megabyte without a match in 256 bytes takes too many draws)"""
    rng = np.random.default_rng(5000 + seed)
    d = rng.integers(144, 256, size=n, dtype=np.uint8)
    for _ in range(200):
        hit = [p for p, ln, _ in oracle.tokens(d.tobytes(), 32, 10) if ln]
        if not hit:
            break
        for p in hit:
            d[p:p + 3] = rng.integers(144, 256, size=len(d[p:p + 3]), dtype=np.uint8)
    data = d.tobytes()
    assert len(oracle.compress(data, 32, 10)[1]) == oracle.out_bound(n)
    return data


def test_compress_streams_exact_capacity_and_scratch(engine, oracle):
    from hdl_deflate_amd.data import family_bytes
    for n in (1 << 14, 100001, (1 << 20) + 7):
        inc = incompressible32(oracle, n, n % 97)
        txt = family_bytes(2, n, seed=n % 89)
        compress_streams_call(engine, oracle, ("stream", n, "incompressible"), [inc])
        compress_streams_call(engine, oracle, ("stream", n, "text"), [txt])
        compress_streams_call(engine, oracle, ("streams", n, 0), [inc, txt, inc])
        compress_streams_call(engine, oracle, ("streams", n, 1), [txt, inc, txt])
    report("k_stream")


# ====================================================================================================== compress: hdlz_compress_chunk
def test_compress_chunk_state_and_output_slack(engine, oracle):
    """out_cap exactly hdlz_out_bound(n) + 2400, the 64-byte hdlz_cstate in bands of its own, the input known only as far as each call
    is told (the bytes behind in_len still hold the pattern); pieces of 32, 320 and 2048 positions and one piece"""
    from hdl_deflate_amd.data import family_bytes
    L = engine.lib
    for data, cw in ((family_bytes(1, 7001), 32), (incompressible(oracle, 5000), 32), (family_bytes(2, 9000, seed=3), 256), (b"hello", 32)):
        n = len(data)
        rc, ref = oracle.compress(data, cw, 10)
        cap = oracle.out_bound(n) + 2400
        for step in (32, 320, 2048, None):
            band = row_band(cap)
            specs = [("in", n, 16, band, True, 5), ("out", cap, 4, band), ("state", 64, 4, band)]
            states = []

            def setup(a):
                a.fill("state", bytes(64))

            def call(a):
                pos, known = 0, 0
                while step is not None and pos + step <= n - 11:
                    q = pos + step
                    a.fill("in", data[known:q + 11], at=known)                     # the reference's stall margin: ten bytes of look-ahead
                    known = q + 11
                    assert L.hdlz_compress_chunk(a.ptr("in"), known, q, 0, cw, 10, a.ptr("out"), cap, a.ptr("state"), stream_ptr()) == 0
                    pos = q
                a.fill("in", data[known:], at=known)
                assert L.hdlz_compress_chunk(a.ptr("in"), n, n, 1, cw, 10, a.ptr("out"), cap, a.ptr("state"), stream_ptr()) == 0

            a, clean, runs = two_runs(specs, setup, call, ("out", "state"))
            for r in runs:
                st = CState.from_buffer_copy(r["state"])
                assert (st.pos, st.done, st.out_len, st.status) == (n, 1, len(ref), 0), (n, step, r["state"].view(np.uint32)[:11])
                assert r["out"][:len(ref)].tobytes() == ref, (n, step)
            assert np.array_equal(runs[0]["state"], runs[1]["state"]), (n, step)
            assert guards.violations(a, clean, {"out": EXTENT_WORD(len(ref)), "state": True}) == [], (n, step)
            note("k_compress_chunk", int(guards.row_tails(a.split(clean)["out"][1], 1, cap)[0]) - len(ref), None)
    report("k_compress_chunk")


# ======================================================================================================= inflate: hdlz_inflate_batch_ws
SILENT_STREAMS = [b"\x78\x9c\x07\x00\x00\x00\x00\x00", b"\x78\x9c\x03", b""]       # oracle: status 3, 1, 1; length 0, no byte
ORACLE_FLAGS = 1 | 8                                                               # the semantic flags; the others are mapping hints


def inflate_call(engine, oracle, label, path, streams, pitch, flags, work_bytes, bound=0, mis=0, fixed=None, silent=(), told=None,
                 told_work=None, fail_extent=None):
    """one guarded hdlz_inflate_batch_ws: ragged (in_off; `bound` = the stated in_len) or fixed = (in_len, in_pitch): a stream per row,
    the rest of the row keeps the pattern.  work_bytes: the size of d_work (0: none is passed)"""
    L, B, band = engine.lib, len(streams), row_band(pitch)
    off = np.concatenate([[0], np.cumsum([len(z) for z in streams])]).astype(np.int64)
    if fixed:
        specs = [("in", (B - 1) * fixed[1] + fixed[0], 16, band, True, mis)]
    else:
        specs = [("in", int(off[-1]), 16, band, True, mis), ("in_off", 8 * (B + 1), 8, band, True)]
    specs += [("out", B * pitch, 4, band), ("out_len", 4 * B, 4, band), ("status", 4 * B, 4, band), ("work", work_bytes, 256, WORK_BAND)]

    def setup(a):
        if fixed:
            for b, z in enumerate(streams):
                a.fill("in", z, at=b * fixed[1])
        else:
            a.fill("in", b"".join(streams))
            a.fill("in_off", off.view(np.uint8))

    def call(a):
        rc = L.hdlz_inflate_batch_ws(a.ptr("in"), None if fixed else a.ptr("in_off"), fixed[1] if fixed else 0, fixed[0] if fixed else bound,
                                     B, flags, 0, a.ptr("out"), pitch, a.ptr("out_len"), a.ptr("status"),
                                     a.ptr("work") if work_bytes else None, work_bytes, stream_ptr())
        assert rc == 0, (label, L.hdlz_last_error())

    a, clean, runs = two_runs(specs, setup, call, ("out", "out_len", "status"))
    flat = np.frombuffer(b"".join(streams) + bytes(8), np.uint8)
    ref, rl, rs = oracle.inflate_batch(flat, off.astype(np.uint64), pitch, flags=flags & ORACLE_FLAGS, nthreads=8)
    if told_work:                                            # (H6: the caller judges the scratch itself)
        return a, clean
    return judge_rows(label, path, a, clean, runs, B, pitch, rs, rl, ref, EXTENT_EXACT, pitch if fail_extent is None else fail_extent,
                      silent=silent, extra={"work": True} if work_bytes else None, told=told)


def fixed_stream(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 9, zlib.Z_FIXED)
    return c.compress(data) + c.flush()


def inflate_kinds(oracle, P):
    """the stream kinds of one pitch P: plain lengths of exactly P (capacity = the output length), P + 1 (one byte less) and 3 P + 7"""
    from hdl_deflate_amd.data import family_bytes
    text = family_bytes(2, P + 8, seed=P)
    r = random.Random(P)
    words = bytes(r.choice(b"eeeeeeeeetttttttaaaaaooooiiinnn  shrdlucmfwypvbgkqjxz") for _ in range(3 * P + 7))
    dyn = zlib.compress(words[:P], 6)
    c = zlib.compressobj(9)
    multi = c.compress(words[:P // 2]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(words[P // 2:P]) + c.flush()
    damaged = bytearray(dyn)
    damaged[len(dyn) // 2] ^= 0x10
    kinds = [("Z_FIXED", fixed_stream(text[:P])), ("default strategy", dyn), ("stored", zlib.compress(text[:P], 0)), ("Z_FULL_FLUSH", multi),
             ("distance-1 run", fixed_stream(b"z" * P, 9)), ("damaged", bytes(damaged)), ("cut", fixed_stream(text[:P])[:-(5 + P // 16)]),
             ("one byte over", fixed_stream(text[:P + 1])), ("far over", zlib.compress(words, 6))]
    if P >= 5:
        kinds.append(("STARTC", oracle.compress(text[:P], 32, 10)[1]))
    for name, z in kinds[:5] + kinds[9:]:
        assert zlib.decompress(z) == (b"z" * P if name == "distance-1 run" else words[:P] if name in ("default strategy", "Z_FULL_FLUSH") else text[:P])
    return kinds


MAPPING_PATH = {2: "k_inflate_tok (lane per stream)", 4: "k_inflate_dyn (wave per stream)", 64: "k_inflate_grp (16 lanes per stream)",
                0: "k_inflate_dyn (auto, small batch)"}


def work_sizes(L, B, bound, pitch, flags, ragged):
    full = L.hdlz_inflate_work_bytes(B, bound, pitch, flags, ragged)
    return [full, full // 2, 1024, 0]


def test_inflate_every_mapping_pitch_and_kind(engine, oracle):
    """small ragged batches without a stated bound (so: the batch kernels), every stream kind first once and last once with silent rows
    between the others; pitches 4 .. 2052; scratch of the asked size, half of it, 1024 bytes and none (cycling with the rotation)"""
    L = engine.lib
    for P in (4, 64, 516, 2048, 2052):
        kinds = inflate_kinds(oracle, P)
        for flags in (2, 4, 64, 0):
            for i, rows in enumerate(rotations(kinds, SILENT_STREAMS)):
                silent = [b for b, r in enumerate(rows) if r[2]]
                wb = work_sizes(L, len(rows), 0, P, flags, 1)[i % 4]
                inflate_call(engine, oracle, (P, flags, i, wb), MAPPING_PATH[flags], [r[1] for r in rows], P, flags, wb, mis=i % 16,
                             silent=silent)
    report("k_inflate")


def test_inflate_last_token_is_a_258_byte_match_at_the_capacity(engine, oracle):
    """streams whose LAST token is a 258-byte match that ends exactly at the capacity (520) and one byte behind it (521 > 520)"""
    fits, over = fixed_stream(b"abc" + b"q" * 517, 9), fixed_stream(b"abcd" + b"q" * 517, 9)
    assert len(fits) == 15 and len(over) == 16                     # 4 / 5 literals, two matches of 258, the end-of-block code
    assert oracle.inflate(fits, out_cap=520)[0] == 0 and oracle.inflate(over, out_cap=520)[0] == 2
    kinds = [("ends at the capacity", fits), ("ends one byte behind", over), ("Z_FIXED", fixed_stream(bytes(range(256)) * 2 + bytes(8)))]
    for flags in (2, 4, 64, 0):
        for i, rows in enumerate(rotations(kinds, SILENT_STREAMS)):
            silent = [b for b, r in enumerate(rows) if r[2]]
            inflate_call(engine, oracle, ("258", flags, i), MAPPING_PATH[flags], [r[1] for r in rows], 520, flags,
                         L_full(engine, len(rows), 520, flags), silent=silent)
    # the whole-GPU path meets the same edge with longer streams: 2 KiB of stream is ~1 MiB of 258-byte matches
    n = 4 + 258 * 4100
    big_fits, big_over = fixed_stream(b"abc" + b"q" * (n - 3), 9), fixed_stream(b"abcd" + b"q" * (n - 3), 9)
    assert len(big_fits) >= 2048 and n % 4 == 0
    for z, name in ((big_fits, "fits"), (big_over, "over")):
        wb = engine.lib.hdlz_inflate_work_bytes(1, len(z), n, 0, 0)
        inflate_call(engine, oracle, ("258 whole-GPU", name), "whole-GPU, one stream", [z], n, 0, wb, fixed=(len(z), len(z)))
    report("k_inflate")


def L_full(engine, B, pitch, flags):
    return engine.lib.hdlz_inflate_work_bytes(B, 0, pitch, flags, 1)


def cycled_batch(kinds, B):
    """B rows: the kinds in turn, a silent row in front of every second one"""
    rows, silent, k = [], [], 0
    while len(rows) < B:
        if k % 2 == 1 and len(rows) < B - 1:
            silent.append(len(rows))
            rows.append(SILENT_STREAMS[(k // 2) % 3])
        rows.append(kinds[k % len(kinds)][1])
        k += 1
    return rows, silent


def test_inflate_length_binned_lists_and_second_pass_in_guarded_scratch(engine, oracle):
    """batches of 300 ragged streams (more than HDLZ_INFLATE_BIN_MIN: the lane mapping orders them by length class in its lists) through
    the lane and the 16-lane mapping at every scratch size; then the automatic choices: 8192 streams (16 lanes) and 23000 (a lane)"""
    L = engine.lib
    for P in (516, 2048):
        rows, silent = cycled_batch(inflate_kinds(oracle, P), 300)
        for flags in (2, 64):
            for wb in work_sizes(L, 300, 0, P, flags, 1):
                inflate_call(engine, oracle, ("300", P, flags, wb), MAPPING_PATH[flags], rows, P, flags, wb, mis=11, silent=silent)
    kinds = inflate_kinds(oracle, 64)
    for B, path in ((8192, "k_inflate_grp (auto, 8192 streams)"), (23000, "k_inflate_tok (auto, 23000 streams)")):
        rows, silent = cycled_batch(kinds, B)
        inflate_call(engine, oracle, ("auto", B), path, rows, 64, 0, L.hdlz_inflate_work_bytes(B, 0, 64, 0, 1), silent=silent)
    report("k_inflate")


# ---------------------------------------------------------------------------------------------- the whole-GPU path (k_par_*, k_any_*)
def plain_bytes(n, seed):
    from hdl_deflate_amd.data import make_blocks
    rows = (n + 2047) // 2048
    return make_blocks(rows, 2048, "cuda", seed=seed, families=(1, 2, 4)).reshape(-1)[:n].cpu().numpy().tobytes()


def par_sizes(full):
    return [full, full // 2, full // 5, full // 48 + 4096, 70000, 256, 0]


def one_large_stream(engine, oracle, name, z, n, flags=0, sizes=None, short_pitch=True):
    L = engine.lib
    pitch = round4(n)
    full = L.hdlz_inflate_work_bytes(1, len(z), pitch, flags, 0)
    assert len(z) >= 2048 and full > 4096, (name, len(z), full)
    for wb in (par_sizes(full) if sizes is None else [s(full) for s in sizes]):
        inflate_call(engine, oracle, (name, flags, wb), "whole-GPU, one stream", [z], pitch, flags, wb, fixed=(len(z), len(z)))
    if short_pitch and pitch - 4 > 0:           # one word less: the chain gives up, the serial pass reports status 2
        inflate_call(engine, oracle, (name, flags, "pitch - 4"), "whole-GPU, one stream", [z], pitch - 4, flags,
                     L.hdlz_inflate_work_bytes(1, len(z), pitch - 4, flags, 0), fixed=(len(z), len(z)))


def test_inflate_whole_gpu_single_streams(engine, oracle):
    few = [lambda f: f, lambda f: f // 2, lambda f: 70000]
    own = {}
    for n, seed in ((1 << 16, 31), ((1 << 20) + 5, 32), (1 << 24, 33)):
        data = plain_bytes(n, seed)
        st, z = engine.compress_bytes(data)
        assert st == 0 and zlib.decompress(z) == data
        own[n] = z
        for flags in (0, 128):                                   # 128: HDLZ_INFLATE_ONE_FIXED_BLOCK
            one_large_stream(engine, oracle, "STARTC %d" % n, z, n, flags=flags, sizes=few if n == 1 << 24 or flags else None,
                             short_pitch=flags == 0)
    small = 1 << 14                                              # a level-6 stream of about 4 KiB
    while len(zlib.compress(plain_bytes(small, 41), 6)) < 4096:
        small += 1 << 13
    for n, level, seed in ((small, 6, 41), (1 << 20, 6, 42), (1 << 24, 6, 43), (1 << 19, 1, 44), (1 << 18, 0, 45)):
        data = plain_bytes(n, seed)
        z = zlib.compress(data, level)
        assert len(z) >= 2048
        one_large_stream(engine, oracle, "zlib -%d %d" % (level, n), z, n, sizes=few if n == 1 << 24 else None)
    # a damaged large stream: the serial decoder writes the same row
    z = bytearray(own[(1 << 20) + 5])
    z[len(z) // 2] ^= 0x04
    one_large_stream(engine, oracle, "damaged STARTC", bytes(z), (1 << 20) + 5, sizes=few, short_pitch=False)
    z = bytearray(zlib.compress(plain_bytes(1 << 20, 42), 6))
    z[len(z) // 3] ^= 0x40
    one_large_stream(engine, oracle, "damaged zlib -6", bytes(z), 1 << 20, sizes=few, short_pitch=False)
    report("whole-GPU")


def test_inflate_whole_gpu_batches(engine, oracle):
    L = engine.lib
    # 48 x 64 KiB at a fixed pitch (own streams; a row's bytes behind its stream keep the pattern -- so no damaged row here: the bytes
    # behind it would be part of what it decodes), two BTYPE-3 rows among them
    plains = [plain_bytes(1 << 16, 100 + b) for b in range(48)]
    zs = [oracle.compress(p, 32, 10)[1] for p in plains]
    zs[7], zs[20] = SILENT_STREAMS[0], SILENT_STREAMS[0]
    in_len = (max(len(z) for z in zs) + 15) // 16 * 16
    for flags in (0, 128):
        full = L.hdlz_inflate_work_bytes(48, in_len, 1 << 16, flags, 0)
        assert full > 48 * 65536 * 2
        for wb in (par_sizes(full) if flags == 0 else [full, full // 5]):
            inflate_call(engine, oracle, ("48 x 64 KiB", flags, wb), "whole-GPU, batch", zs, 1 << 16, flags, wb, fixed=(in_len, in_len),
                         silent=(7, 20))
        for first in (zs[8:] + zs[:8], zs[7:] + zs[:7]):          # the silent row last / first
            sil = [b for b, z in enumerate(first) if z == SILENT_STREAMS[0]]
            inflate_call(engine, oracle, ("48 x 64 KiB rotated", flags), "whole-GPU, batch", first, 1 << 16, flags, full,
                         fixed=(in_len, in_len), silent=sil)
    # one word less than the output: the chain gives up on every stream, the serial pass reports status 2
    inflate_call(engine, oracle, ("48 x 64 KiB", "pitch - 4"), "whole-GPU, batch", zs, (1 << 16) - 4, 0,
                 L.hdlz_inflate_work_bytes(48, in_len, (1 << 16) - 4, 0, 0), fixed=(in_len, in_len), silent=(7, 20))
    # 200 ragged streams with a stated bound, real lengths from a tenth of the bound to the bound; every kind of silent row between them
    r = random.Random(5)
    big = plain_bytes(200 * 3000 + 70000, 77)
    zs, silent = [], []
    for k in range(200):
        n = 6000 + (k * 7919) % 54001 if k else 60000
        p = big[k * 3000:k * 3000 + n]
        if k % 10 == 5:
            silent.append(len(zs))
            zs.append(SILENT_STREAMS[(k // 10) % 3])
        zs.append(oracle.compress(p, 32, 10)[1] if k % 2 else zlib.compress(p, 6 if k % 4 else 1))
        if k in (50, 51):                                        # a damaged zlib stream and a damaged own stream: the serial decoder's rows
            z = bytearray(zs[-1])
            z[len(z) // 2] ^= 0x08
            zs[-1] = bytes(z)
    bound = max(len(z) for z in zs)
    assert min(len(z) for z in zs if len(z) > 8) < bound // 4 and bound >= 2048
    assert silent[0] == 5
    for rot in (0, 1, 5, 6):                                     # (rotated: a zlib stream / an own stream / a silent row first, a silent row last)
        rows = zs[rot:] + zs[:rot]
        sil = [(b - rot) % len(zs) for b in silent]
        full = L.hdlz_inflate_work_bytes(len(rows), bound, 60000, 0, 1)
        for wb in ((full, full // 5) if rot == 0 else (full,)):
            inflate_call(engine, oracle, ("200 ragged", rot, wb), "whole-GPU, ragged batch", rows, 60000, 0, wb, bound=bound, mis=rot % 16,
                         silent=sil)
    report("whole-GPU")


# ================================================================================================================ hdlz_inflate_chunk
def test_inflate_chunk_exact_capacity_and_state(engine, oracle):
    """out_cap exactly the output length, out_limit advancing in steps of 1, 257 and 4096, the hdlz_istate (16 words + lengths[320] =
    384 bytes) in bands of its own; a stream with dynamic blocks, and the same stream cut"""
    L = engine.lib
    r = random.Random(3)
    data = bytes(r.choice(b"hello world, said the fox ") for _ in range(9001))
    z = zlib.compress(data, 6)
    for name, zz in (("dynamic", z), ("cut", z[:len(z) * 2 // 3])):
        rc, ref = oracle.inflate(zz, out_cap=len(data))
        assert (rc == 0) == (name == "dynamic")
        for step in (1, 257, 4096):
            if step == 1 and name == "cut":
                continue
            cap = len(data)
            band = row_band(cap)
            specs = [("in", len(zz), 16, band, True, 7), ("out", cap, 4, band), ("state", 384, 4, band)]
            seen = []

            def setup(a):
                a.fill("in", zz)
                a.fill("state", bytes(384))

            def call(a):
                limit = 0
                for _ in range(cap + 8):
                    limit = min(cap, limit + step)
                    assert L.hdlz_inflate_chunk(a.ptr("in"), len(zz), 1, 0, 0, a.ptr("out"), cap, limit, a.ptr("state"), stream_ptr()) == 0
                    if step > 1 or limit == cap:
                        st = IState.from_buffer_copy(a.view("state").cpu().numpy())
                        assert st.out_pos <= limit
                        if st.done or st.status:
                            break
                seen.append(limit)

            a, clean, runs = two_runs(specs, setup, call, ("out", "state"))
            for k in runs:
                st, words = IState.from_buffer_copy(k["state"]), k["state"].view(np.uint32)[:12]
                if rc == 0:
                    assert (st.out_pos, st.done, st.status) == (len(data), 1, 0), (name, step, words)
                    assert k["out"].tobytes() == data
                else:
                    assert st.status == rc and st.done == 0, (name, step, words)
                    assert k["out"][:st.out_pos].tobytes() == data[:st.out_pos]
            assert np.array_equal(runs[0]["state"][:48], runs[1]["state"][:48]) and seen[0] == seen[1], (name, step)
            assert guards.violations(a, clean, {"out": True, "state": True}) == [], (name, step)


# ============================================================================================================= hdlz_archive_batch_ws
def test_archive_scratch_offsets_and_capacity(engine):
    """d_work exactly hdlz_archive_work_bytes(B), d_off exactly B + 1 words, archive_cap exactly the total and one byte less (the rows
    that would end beyond it are not copied)"""
    L = engine.lib
    pitch = 64
    for B in (1, 255, 256, 257, 5000):
        rng = np.random.default_rng(B)
        rows = rng.integers(0, 256, size=(B, pitch), dtype=np.uint8)
        lens = rng.integers(0, pitch + 1, size=B).astype(np.int32)
        lens[-1] = max(lens[-1], 1)
        off = np.concatenate([[0], np.cumsum(lens.astype(np.int64))]).astype(np.int64)
        total = int(off[-1])
        wb = L.hdlz_archive_work_bytes(B)
        for cap in (total, total - 1):
            specs = [("rows", B * pitch, 4, 1 << 16, True), ("len", 4 * B, 4, 1 << 16, True), ("archive", cap, 1, 1 << 16),
                     ("off", 8 * (B + 1), 8, 1 << 16), ("work", wb, 8, WORK_BAND)]

            def setup(a):
                a.fill("rows", rows)
                a.fill("len", lens.view(np.uint8))

            def call(a):
                rc = L.hdlz_archive_batch_ws(a.ptr("rows"), pitch, a.ptr("len"), B, a.ptr("archive"), cap, a.ptr("off"), a.ptr("work"), wb,
                                             stream_ptr())
                assert rc == 0, (B, cap, L.hdlz_last_error())

            a, clean, runs = two_runs(specs, setup, call, ("archive", "off"))
            may = np.zeros(cap, bool)
            for k in runs:
                assert np.array_equal(k["off"].view(np.int64), off), (B, cap)
                for b in range(B):
                    if off[b + 1] <= cap:
                        may[off[b]:off[b + 1]] = True
                        assert np.array_equal(k["archive"][off[b]:off[b + 1]], rows[b, :lens[b]]), (B, cap, b)
            assert guards.violations(a, clean, {"archive": torch.from_numpy(may), "off": True, "work": True}) == [], (B, cap)


# ==================================================================================================================================== H6
def test_the_checker_reports_real_stores_when_told_a_shorter_extent(engine, oracle):
    """sensitivity without a faulty kernel: the CHECKER (not the library) is told that the last row is 4 bytes shorter and the scratch
    256 bytes shorter than what was passed; it must report the bytes the kernels really wrote there"""
    # compress: the last row is incompressible, its output ends in the last word of its minimal pitch
    n = 2048
    pitch = round4(oracle.out_bound(n))
    blocks = [bytes(n), b"abc", incompressible(oracle, n)]
    bad = compress_batch_call(engine, oracle, "H6 compress", "H6", blocks, 32, 10, pitch, bound=2048, silent=[1], told={2: pitch - 4})
    assert bad == [("out", "region", 3 * pitch - 4, 3 * pitch - 1, 4)], bad
    # whole-GPU inflate, an own stream whose output fills the capacity: the last array of its scratch layout (with the hint that leaves
    # the chain for any block types out: nfail, a word per sub-piece) is written up to its end, which lies in the scratch's last 256 bytes
    data = plain_bytes(1 << 16, 31)
    st, z = engine.compress_bytes(data)
    wb = engine.lib.hdlz_inflate_work_bytes(1, len(z), 1 << 16, 128, 0)
    a, clean = inflate_call(engine, oracle, "H6 scratch", "H6", [z], 1 << 16, 128, wb, fixed=(len(z), len(z)), told_work=True)
    last = int(guards.row_tails(a.split(clean)["work"][1], 1, wb)[0])
    print("H6 scratch: hdlz_inflate_work_bytes = %d, last written byte + 1 = %d" % (wb, last))
    assert guards.violations(a, clean, {"out": True, "out_len": True, "status": True, "work": True}) == []
    bad = guards.violations(a, clean, {"out": True, "out_len": True, "status": True, "work": wb - 256})
    assert len(bad) == 1 and bad[0][:2] == ("work", "region") and wb - 256 <= bad[0][2] <= bad[0][3] == last - 1 < wb, (bad, wb, last)
    bad = inflate_call(engine, oracle, "H6 out", "H6", [z], 1 << 16, 128, wb, fixed=(len(z), len(z)), told={0: (1 << 16) - 4})
    assert bad == [("out", "region", (1 << 16) - 4, (1 << 16) - 1, 4)], bad
