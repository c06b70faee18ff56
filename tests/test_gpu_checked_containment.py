"""GPU (-m gpu): hdlz_inflate_checked inside guard bands (tests/guards.py), in the manner of tests/test_gpu_containment.py: every
buffer of the call carved out of one patterned arena, each case run on the pattern and on its complement.

  bands and read-only regions (d_in and its slack, d_in_off) untouched;
  d_in_used / d_adler written for [0, nstreams) only, d_work only inside what was passed, rows as hdlz_inflate_batch_ws writes them;
  all four result arrays identical in both runs -- the runs differ in every byte behind out_len, every slack byte of d_in and the
  initial content of every output, so none of those reaches a verdict -- and equal to what zlib / the oracle say (checked_ref)."""
import zlib

import numpy as np
import pytest

import checked_ref as R
import guards
import test_gpu_containment as C

pytestmark = pytest.mark.gpu


def checked_call(engine, oracle, label, streams, pitch, flags, bound=0, fixed=None, work_cut=0, adler=True, mis=0):
    """one guarded hdlz_inflate_checked: ragged (bound = the stated in_len) or fixed = (in_len, in_pitch).  work_cut: bytes less than
    the query's answer are passed (never below the judging pass's share)"""
    L, B, band = engine.lib, len(streams), C.row_band(pitch)
    off = np.concatenate([[0], np.cumsum([len(z) for z in streams])]).astype(np.int64)
    ilen = fixed[0] if fixed else bound
    full = L.hdlz_inflate_checked_work_bytes(B, ilen, pitch, flags, 0 if fixed else 1)
    share = full - L.hdlz_inflate_work_bytes(B, ilen, pitch, flags, 0 if fixed else 1)
    work_bytes = max(share, full - work_cut)
    if fixed:
        specs = [("in", (B - 1) * fixed[1] + fixed[0], 16, band, True, mis)]
    else:
        specs = [("in", int(off[-1]), 16, band, True, mis), ("in_off", 8 * (B + 1), 8, band, True)]
    specs += [("out", B * pitch, 4, band), ("out_len", 4 * B, 4, band), ("status", 4 * B, 4, band), ("in_used", 4 * B, 4, band),
              ("adler", 4 * B, 4, band), ("work", work_bytes, 256, C.WORK_BAND)]

    def setup(a):
        if fixed:
            for b, z in enumerate(streams):
                a.fill("in", z, at=b * fixed[1])
        else:
            a.fill("in", b"".join(streams))
            a.fill("in_off", off.view(np.uint8))

    def call(a):
        rc = L.hdlz_inflate_checked(a.ptr("in"), None if fixed else a.ptr("in_off"), fixed[1] if fixed else 0, ilen, B, flags, 0,
                                    a.ptr("out"), pitch, a.ptr("out_len"), a.ptr("status"), a.ptr("in_used"),
                                    a.ptr("adler") if adler else None, a.ptr("work") if work_bytes else None, work_bytes, C.stream_ptr())
        assert rc == 0, (label, L.hdlz_last_error())

    a, clean, runs = C.two_runs(specs, setup, call, ("out", "out_len", "status", "in_used", "adler"))
    for n in ("out_len", "status", "in_used") + (("adler",) if adler else ()):
        assert np.array_equal(runs[0][n], runs[1][n]), (label, n, "depends on bytes the call was not given")
    assert not fixed or all(len(z) == fixed[0] for z in streams)      # (fixed pitch here: rows without slack, so zlib sees what the call sees)
    exps = [R.expect(oracle, z, pitch) for z in streams]
    for k, r in enumerate(runs):
        st, ol, used, ad = (r[n].view(np.uint32) for n in ("status", "out_len", "in_used", "adler"))
        out = r["out"].reshape(B, pitch)
        for b in range(B):
            R.check((label, k, b), exps[b], st[b], ol[b], used[b], ad[b] if adler else exps[b].get("adler", 0), out[b])
    st, ol = runs[1]["status"].view(np.uint32), runs[1]["out_len"].view(np.uint32)
    ext = [int(ol[b]) if st[b] == 0 else pitch for b in range(B)]       # an OK row: exactly out_len bytes; a failed one: anything inside the row
    allowed = {"out": guards.row_mask(B, pitch, ext, "cuda"), "out_len": True, "status": True, "in_used": True}
    if adler:
        allowed["adler"] = True
    if work_bytes:
        allowed["work"] = True
    bad = guards.violations(a, clean, allowed)
    assert bad == [], (label, bad)
    # ... and the arrays ARE written for [0, nstreams): no word of them keeps the pattern in both runs
    parts = a.split(clean)
    for n in ("in_used",) + (("adler",) if adler else ()):
        assert not bool(parts[n][1].any()), (label, n, "not written")
    if not adler:
        assert bool(parts["adler"][1].all()), (label, "d_adler = NULL: nothing of that region may be written")
    return runs


def test_batch_mappings_in_guard_bands(engine, oracle):
    """one ragged batch per mapping (lane, wave, 16 lanes per stream, default), every stream kind of test_gpu_containment with silent
    rows between them, rotated so that every kind is first once and last once; pitch 2052 (not a multiple of 16) and 2048"""
    for P, flags in ((2052, 2), (2052, 4), (2048, 64), (2052, 0)):
        kinds = C.inflate_kinds(oracle, P)
        for i, rows in enumerate(C.rotations(kinds, C.SILENT_STREAMS)):
            if i % 3:
                continue
            checked_call(engine, oracle, (P, flags, i), [r[1] for r in rows], P, flags, work_cut=(0, 1 << 30)[i % 2], adler=i % 4 != 3,
                         mis=i % 16)


def test_rows_of_64_kib_take_the_tiles_in_guarded_scratch(engine, oracle):
    """rows of 64 KiB + 4 under a mapping hint: the batch kernels decode, the judging pass cuts the rows into tiles -- its per-tile sums
    are the FRONT of d_work, and with nothing but its own share passed the call still answers the same"""
    P = 65540
    r = np.random.default_rng(4)
    plain = [bytes(r.integers(97, 105, n, dtype=np.uint8)) for n in (65540, 65521, 32768, 1, 40000)]
    streams = [zlib.compress(p, 6) for p in plain] + [b"\x78\x9c\x03", zlib.compress(b"")]
    bad = bytearray(streams[1]); bad[-1] ^= 0x40; streams.append(bytes(bad))
    hdr = bytearray(streams[2]); hdr[1] ^= 0x01; streams.append(bytes(hdr))
    for flags, cut in ((4, 0), (2, 1 << 30), (4, 1 << 30)):
        runs = checked_call(engine, oracle, ("tiles", flags, cut), streams, P, flags, work_cut=cut)
        st = runs[0]["status"].view(np.uint32)
        assert list(st) == [0, 0, 0, 0, 0, 1, 0, R.E_BAD_CHECKSUM, R.E_BAD_HEADER], list(st)


def test_whole_gpu_shape_in_guard_bands(engine, oracle):
    """ONE large stream (the whole-GPU chains, their scratch behind the judging pass's share) and a batch of large streams
    given ragged with a bound: intact and damaged in the trailer"""
    text = C.plain_bytes(3 << 20, 7)
    z = zlib.compress(text, 6)
    cap = (3 << 20) + 64
    for zz in (z, C.fixed_stream(text[: 1 << 20]), z[:-1] + bytes([z[-1] ^ 1])):
        runs = checked_call(engine, oracle, ("one stream", len(zz)), [zz], cap, 0, fixed=(len(zz), len(zz)))
    assert int(runs[0]["status"].view(np.uint32)[0]) == R.E_BAD_CHECKSUM
    zs = [zlib.compress(C.plain_bytes(200000 + 5000 * k, 20 + k), 6) for k in range(5)] + [C.fixed_stream(C.plain_bytes(150000, 30))]
    zs[3] = zs[3][:-2] + bytes([zs[3][-2] ^ 0x10]) + zs[3][-1:]
    runs = checked_call(engine, oracle, "ragged batch of large streams", zs, 230000, 0, bound=int(max(len(x) for x in zs)))
    st = runs[0]["status"].view(np.uint32)
    assert list(st) == [0, 0, 0, R.E_BAD_CHECKSUM, 0, 0], list(st)
