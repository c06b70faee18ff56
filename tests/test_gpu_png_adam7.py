"""GPU (-m gpu): HDLZ_PNG_ADAM7 -- Adam7 interlaced images through hdlz_png_index_ws / hdlz_png_decode_ws / Engine.png_index(interlaced=True) /
Engine.decode_png / load_png.

The files are those of tests/png_adam7_ref.py's encoder (fixed seeds); what every record, status and slot must hold is that module's
index and decode, the rule of include/hdlz_png.h under flags & 4, which tests/test_png_adam7_cpu.py holds against Pillow.  Where the
encoder was given the scanlines, the expected slot is made of them directly (png_ref.expand), not of the reference's own unfilter.
Every set is decoded in ONE call over all images and as Engine.decode_png routes it.

The seams, named as in tests/test_gpu_png.py, apply inside a PASS: a BAND is 64 rows of one pass; a TILE is S = 128 // bpp steps of the
diagonal wavefront over a pass's row; a SEGMENT starts at a pass's row 0 and at the first row with filter 0 or 1 of every further band
of the pass."""
import struct
import zlib

import numpy as np
import pytest

import png_ref as P
import png_adam7_ref as A
import test_gpu_png as T

pytestmark = pytest.mark.gpu
EX, RAW = P.EXPAND | A.ADAM7, P.RAW | A.ADAM7
MODES = pytest.mark.parametrize("flags", [EX, RAW], ids=["expand", "raw"])


def png_index(engine, d, off, ln, flags, out_align=64):
    return engine.png_index(d, off, ln, out_align=out_align, expand=bool(flags & P.EXPAND), interlaced=bool(flags & A.ADAM7))


def run_decode(engine, d, pi, first, count, flags, out_fill=0):
    """ONE hdlz_png_decode_ws call over images [first, first + count) under `flags` -> (out, status, record)"""
    import torch
    from hdl_deflate_amd import _lib
    L, h = engine.lib, pi.host
    last = first + count - 1
    ok = int(h["status"][last] == 0)
    zb = int(h["z_off"][last] - h["z_off"][first]) + P.r16(int(h["zlen"][last]) + 8) * ok
    rb = int(h["raw_off"][last] - h["raw_off"][first]) + P.r16(int(h["raw_len"][last])) * ok
    total = int(h["out_off"][last] - h["out_off"][first]) + int(h["out_len"][last]) * ok
    idat = int(h["nidat"][first:first + count].sum())
    out = torch.full((total,), out_fill, dtype=torch.uint8, device="cuda")
    status = torch.full((count,), 77, dtype=torch.int32, device="cuda")
    work = torch.empty(L.hdlz_png_decode_work_bytes(count, idat, zb, rb), dtype=torch.uint8, device="cuda")
    rec = engine._record("hdlz_png_decode_ws", _lib.PngDecodeResult, (work, work.data_ptr(), work.numel()), d.data_ptr(), d.numel(),
                         pi.images.data_ptr(), first, count, flags, idat, zb, rb, out.data_ptr() if total else None, total, status.data_ptr())
    return out, status, rec


def check(engine, label, files, expect=None, flags=EX, routed=True):
    """index the files and decode them -- ONE call over all of them and as Engine.decode_png routes them -- against the rule.
    expect: [(status, slot bytes)] (default: the reference's decode of every file)"""
    d, off, ln = T.stage(files)
    pi = png_index(engine, d, off, ln, flags)
    assert pi.interlaced == bool(flags & A.ADAM7) and pi.expand == bool(flags & P.EXPAND)
    ix = A.index(files, flags, 64)
    for i, rec in enumerate(ix["images"]):
        got = {n: int(pi.host[n][i]) for n in P.FIELDS}
        assert got == rec, (label, i, {n: (got[n], rec[n]) for n in P.FIELDS if got[n] != rec[n]})
    assert (pi.host["reserved"] == 0).all()
    r = pi.record
    assert (r.nimages, r.total_z, r.total_raw, r.total_out, r.status, r.reserved) == \
        (len(files), ix["total_z"], ix["total_raw"], ix["total_out"], P.OK, 0), label
    if expect is None:
        expect = [A.decode(f, rec, flags) for f, rec in zip(files, ix["images"])]
    n = len(files)
    out, status, rec = run_decode(engine, d, pi, 0, n, flags)
    T.check_slots((label, "one call"), pi, 0, n, expect, out, status)
    bad = [k for k, (s, _) in enumerate(expect) if s != P.OK]
    assert (rec.status, rec.first_bad) == ((P.OK, 2 ** 64 - 1) if not bad else (expect[bad[0]][0], bad[0])), (label, rec.status, rec.first_bad)
    assert rec.out_len == (ix["total_out"] if not bad else 0) and rec.reserved == 0
    if routed:
        out, status = engine.decode_png(d, pi)
        T.check_slots((label, "routed"), pi, 0, n, expect, out, status)
    return d, pi, ix, expect


def made(w, h, colour, depth, seed, flags=EX, filters=None, **kw):
    """an interlaced image of known scanlines, random filters per row of every pass -> (file, (OK, the slot's bytes))"""
    rows = kw.pop("rows", None) or P.random_rows(w, h, colour, depth, seed, smooth=kw.pop("smooth", False))
    if filters is None:
        filters = [int(x) for x in np.random.default_rng(seed + 99).integers(0, 5, A.total_rows(w, h))]
    f = A.make_adam7(w, h, colour, depth, rows=rows, filters=filters, seed=seed, **kw)
    rec = A.index([f], flags)["images"][0]
    assert rec["status"] == P.OK and rec["interlace"] == 1
    return f, (P.OK, P.expand(rows, rec, f) if flags & P.EXPAND else rows)


def both(items):
    return [f for f, _ in items], [e for _, e in items]


@MODES
@pytest.mark.parametrize("colour,depth", [(2, 8), (0, 1)], ids=["rgb8", "grey1"])
def test_every_geometry_up_to_9_by_9(engine, colour, depth, flags):
    """every (w, h) in 1 .. 9 x 1 .. 9 in one call: the sizes at which passes vanish, one by one, in x and in y"""
    items = [made(w, h, colour, depth, seed=10 * w + h, flags=flags, smooth=(w + h) % 2 == 0) for w in range(1, 10) for h in range(1, 10)]
    d, pi, ix, _ = check(engine, ("grid", colour, depth, flags), *both(items), flags=flags)
    assert ix["images"][0]["raw_len"] == 1 + P.row_bytes_of(1, colour, depth) and len({r["raw_len"] for r in ix["images"]}) > 20
    assert A.decode(items[40][0], ix["images"][40], flags) == items[40][1]           # (the reference agrees with the scanlines it was made of)


@MODES
def test_every_type_and_the_palette(engine, flags):
    """all 15 pairs at 13 x 11 and 33 x 17 with per-row random filters; palette images with and without a tRNS, a palette of fewer than
    2^depth entries whose images hold indices past plte_n (black, opaque)"""
    items = [made(w, h, colour, depth, seed=colour * 100 + depth + w, flags=flags, idat=None if depth == 8 else 11,
                  trns=bytes([7, 130, 0]) if colour == 3 and w == 33 else None)
             for colour, depth in P.PAIRS for w, h in ((13, 11), (33, 17))]
    for depth, npal, trns in ((8, 200, None), (8, 3, bytes([1, 2, 3, 4])), (4, 5, None), (2, 1, bytes([77])), (1, 1, None)):
        pal = bytes(np.random.default_rng(depth + npal).integers(0, 256, 3 * npal, dtype=np.uint8))
        items.append(made(21, 10, 3, depth, seed=depth, flags=flags, palette=pal, trns=trns))
    d, pi, ix, expect = check(engine, ("types", flags), *both(items), flags=flags)
    if flags & P.EXPAND:
        assert set(pi.host["channels_out"]) == {1, 2, 3, 4}
        a = np.frombuffer(expect[-2][1], np.uint8).reshape(10, 21, 4)           # depth 2, one entry, one tRNS byte
        assert (a[..., 3] == 255).any() and (a[..., 3] == 77).any() and (a[a[..., 3] == 255][:, :3] == 0).all()
    assert A.decode(items[3][0], ix["images"][3], flags) == items[3][1] and A.decode(items[-2][0], ix["images"][-2], flags) == items[-2][1]


@MODES
def test_band_seams_inside_a_pass(engine, flags):
    """9 x 130: passes 6 and 7 have 65 rows; 3 x 520: pass 1 has 65; 5 x 1032: pass 1 has 129, three bands"""
    geo = {(9, 130): {6: 65, 7: 65}, (3, 520): {1: 65}, (5, 1032): {1: 129}}
    items = []
    for (w, h), want in geo.items():
        ph = {A.PASSES.index(g[:4]) + 1: g[5] for g in A.passes_of(w, h, 0, 8)}
        assert all(ph[p] == n for p, n in want.items()), (w, h, ph)
        for k, (colour, depth) in enumerate(((2, 8), (0, 1), (6, 16), (3, 4))):
            items.append(made(w, h, colour, depth, seed=w + k, flags=flags, smooth=k % 2 == 0, level=1))
    check(engine, ("band seams", flags), *both(items), flags=flags)


def test_segment_starts_inside_a_pass(engine):
    """one 8 x 1600 RGBA image: pass 7 has 800 rows of 8 pixels, 13 bands.  Its band 1 has no row with filter 0 or 1 (the segment of
    band 0 runs on through it), band 2 has its first such row mid-band (row 150), band 3 starts with one (row 192); the other passes'
    rows and the rest of pass 7 look up at random"""
    rng = np.random.default_rng(8)

    def filters(p, ph):
        fl = [int(x) for x in rng.integers(0, 5, ph)]
        if p == 7:
            fl[64:192] = [int(x) for x in rng.integers(2, 5, 128)]
            fl[150], fl[192] = 1, 0
        if p == 6:                                            # 800 rows too: no quiet row at all behind row 0
            fl = [int(x) for x in rng.integers(2, 5, ph)]
        return fl
    f, e = made(8, 1600, 6, 8, seed=4, filters=filters, smooth=True, level=1)
    assert [g[5] for g in A.passes_of(8, 1600, 6, 8)] == [200, 200, 200, 400, 400, 800, 800]
    d, pi, ix, _ = check(engine, "segments", [f], [e])
    assert A.decode(f, ix["images"][0]) == e
    small = made(3, 3, 6, 8, seed=1)
    check(engine, "segments, in a batch", [small[0], f, small[0]], [small[1], e, small[1]])


@MODES
def test_tile_seams_of_the_wavefront(engine, flags):
    """1040 x 9 grey 8: pass 1 is 130 pixels wide, past a tile of S = 128; 300 x 4 grey 1; 140 x 70 RGBA 16 (bpp 8, S = 16): a pass both
    wider than a tile and taller than a band"""
    items = [made(1040, 9, 0, 8, seed=1, flags=flags, smooth=True), made(300, 4, 0, 1, seed=2, flags=flags), made(140, 70, 6, 16, seed=3, flags=flags, level=1)]
    assert A.passes_of(1040, 9, 0, 8)[0][4] == 130 and A.passes_of(140, 70, 6, 16)[6][4:6] == (140, 35) and A.passes_of(140, 70, 6, 16)[5][5] == 35
    items.append(made(140, 140, 6, 16, seed=5, flags=flags, level=1))      # passes 6 and 7: 70 rows of 70 and 140 pixels
    check(engine, ("tile seams", flags), *both(items), flags=flags)


def _noise():
    """256 x 256 RGBA noise, interlaced: zlen is past PNG_LARGE_MIN (filters 0 to 2: the reference is not asked to undo it)"""
    return made(256, 256, 6, 8, seed=12, filters=[r % 3 for r in range(A.total_rows(256, 256))], level=1)


def test_a_mixed_batch_and_its_ranges(engine):
    """interlaced, plain and broken files in one call; sub-ranges; count == 1; a large interlaced image that decode_png sends alone on the
    whole-GPU route, with the same answer as in the batch"""
    from hdl_deflate_amd import _lib
    big = _noise()
    broken = A.make_adam7(20, 10, 2, 8, seed=9)
    items = []
    for k in range(24):
        colour, depth = P.PAIRS[(2 * k) % len(P.PAIRS)]
        w, h = 3 + 4 * k, 40 - k
        if k % 3 == 1:
            items.append(T.made(w, h, colour, depth, [r % 5 for r in range(h)], seed=k))
        elif k % 8 == 3:
            items.append((broken[:len(broken) - 20 - k], None))
        else:
            items.append(made(w, h, colour, depth, seed=k, idat=None if k % 2 else 13))
    items[5] = big
    files = [f for f, _ in items]
    ix = A.index(files, EX)
    expect = [e if e is not None else A.decode(f, rec, EX) for (f, e), rec in zip(items, ix["images"])]
    assert sorted({s for s, _ in expect}) == [P.OK, P.E_NO_EOF] and {r["interlace"] for r in ix["images"]} == {0, 1}
    assert ix["images"][5]["zlen"] >= _lib.PNG_LARGE_MIN > max(r["zlen"] for k, r in enumerate(ix["images"]) if k != 5)
    d, pi, _, _ = check(engine, "mixed", files, expect)
    for first, count in ((0, 1), (2, 1), (3, 1), (5, 1), (1, 4), (4, 3), (6, 18), (23, 1)):
        out, status, rec = run_decode(engine, d, pi, first, count, EX, out_fill=first + 1)
        T.check_slots(("range", first, count), pi, first, count, expect, out, status)
        bad = [k for k in range(count) if expect[first + k][0] != P.OK]
        assert rec.first_bad == (bad[0] if bad else 2 ** 64 - 1) and rec.status == (expect[first + bad[0]][0] if bad else P.OK)
        out2, status2 = engine.decode_png(d, pi, first, count)
        T.check_slots(("routed range", first, count), pi, first, count, expect, out2, status2)
    check(engine, "the large image alone", [big[0]], [big[1]])
    check(engine, "the large image alone, raw", [big[0]], [(P.OK, P.random_rows(256, 256, 6, 8, 12))], flags=RAW)


def test_refusals(engine):
    """a stream one row short; a plain stream under an interlaced IHDR; filter byte 5 in pass 4; interlace 2; interlace 1 without the
    flag; an interlaced record decoded without the flag; a record whose raw_len is the plain image's"""
    import torch
    from hdl_deflate_amd.png import PngIndex
    rows = P.random_rows(9, 9, 2, 8, 1)
    stream = A.adam7_stream(9, 9, 2, 8, rows, [r % 5 for r in range(A.total_rows(9, 9))])
    good = made(9, 9, 2, 8, seed=1, rows=rows)
    short = P.make_png(9, 9, 2, 8, interlace=1, stream=zlib.compress(stream[:-28]))
    plain = P.make_png(9, 9, 2, 8, rows=rows, ihdr=struct.pack(">IIBBBBB", 9, 9, 8, 2, 0, 0, 1))
    at = sum(g[5] * (g[6] + 1) for g in A.passes_of(9, 9, 2, 8)[:3]) + 7                   # pass 4, its second row
    five = P.make_png(9, 9, 2, 8, interlace=1, stream=zlib.compress(stream[:at] + b"\x05" + stream[at + 1:]))
    two = P.make_png(9, 9, 2, 8, rows=rows, interlace=2)
    files = [good[0], short, good[0], plain, five, two, good[0]]
    want = [P.OK, P.E_BAD_CHECKSUM, P.OK, P.E_BAD_CHECKSUM, P.E_BAD_SYMBOL, P.E_BAD_HEADER, P.OK]
    assert A.raw_len_of(9, 9, 2, 8) != 9 * 28
    for flags in (EX, RAW):
        ix = A.index(files, flags)
        expect = [A.decode(f, rec, flags) for f, rec in zip(files, ix["images"])]
        assert [s for s, _ in expect] == want and expect[0][1] == (good[1][1] if flags == EX else rows)
        d, pi, _, _ = check(engine, ("refusals", flags), files, expect, flags=flags)
        for k in range(len(files)):                              # ... and alone in a call: the one-stream route judges alike
            out, status, rec = run_decode(engine, d, pi, k, 1, flags)
            assert (int(status[0]), rec.status, rec.first_bad) == (want[k], want[k], 2 ** 64 - 1 if want[k] == P.OK else 0), (k, int(status[0]), rec.status)
    # without the flag: the index refuses what it refused, and bit for bit
    check(engine, "no flag", files, [(P.E_BAD_BTYPE, None)] * 5 + [(P.E_BAD_HEADER, None), (P.E_BAD_BTYPE, None)], flags=P.EXPAND)
    # the records of the flag, decoded without it
    d, off, ln = T.stage(files)
    pi = png_index(engine, d, off, ln, EX)
    for first, count in ((0, len(files)), (0, 1)):
        out, status, rec = run_decode(engine, d, pi, first, count, P.EXPAND, out_fill=0x5A)
        assert [int(s) for s in status] == [P.E_BAD_PARAM if pi.host["status"][first + k] == P.OK else int(pi.host["status"][first + k]) for k in range(count)]
        assert (rec.status, rec.first_bad, rec.out_len) == (P.E_BAD_PARAM, 0, 0) and bool((out == 0x5A).all())
    # a record with the plain image's raw_len
    host = pi.host.copy()
    host["raw_len"][2] = 9 * 28
    forged = PngIndex(torch.from_numpy(np.frombuffer(host.tobytes(), np.int64).reshape(len(files), 17).copy()).cuda(), pi.record, host, 64, True, True)
    out, status, rec = run_decode(engine, d, forged, 0, len(files), EX)
    assert [int(s) for s in status] == want[:2] + [P.E_BAD_PARAM] + want[3:]
    o = int(host["out_off"][6])
    assert out[:len(good[1][1])].cpu().numpy().tobytes() == out[o:o + len(good[1][1])].cpu().numpy().tobytes() == good[1][1]
    out, status, rec = run_decode(engine, d, forged, 2, 1, EX)
    assert (int(status[0]), rec.status, rec.first_bad) == (P.E_BAD_PARAM, P.E_BAD_PARAM, 0)


def test_load_png_reads_both_kinds(engine):
    """load_png on a list mixing interlaced and plain files of the same scanlines: equal tensors; interlaced=False is the old refusal"""
    import torch
    from hdl_deflate_amd import load_png, HdlzStatusError
    laced, plain, shapes = [], [], []
    for k, (colour, depth) in enumerate(((6, 8), (0, 16), (3, 2), (2, 16), (0, 1), (2, 8))):
        w, h = 33 - 4 * k, 17 + 3 * k
        rows = P.random_rows(w, h, colour, depth, k)
        trns = bytes([5]) if colour == 3 else None
        laced.append(made(w, h, colour, depth, seed=k, rows=rows, trns=trns)[0])
        plain.append(P.make_png(w, h, colour, depth, rows=rows, filters=[r % 5 for r in range(h)], seed=k, trns=trns))
        shapes.append((h, w))
    want = load_png(engine, plain, interlaced=False)
    mixed = [laced[k] if k % 2 == 0 else plain[k] for k in range(6)]
    for files in (laced, mixed):
        got = load_png(engine, files)
        for t, g, (h, w) in zip(got, want, shapes):
            assert t.is_cuda and t.dtype == g.dtype and tuple(t.shape[:2]) == (h, w) and torch.equal(t, g)
    assert torch.equal(load_png(engine, laced[3]), want[3])
    with pytest.raises(HdlzStatusError) as ei:
        load_png(engine, [plain[0], plain[1], laced[2], laced[3]], interlaced=False)
    assert ei.value.first_bad == 2 and ei.value.status == P.E_BAD_BTYPE
