"""GPU (-m gpu): hdlz_png_index_ws / hdlz_png_decode_ws / Engine.png_index / Engine.decode_png / load_png.

The files are those of tests/png_ref.py's encoder (fixed seeds); what every record, status and slot must hold is png_ref.index,
png_ref.decode and png_ref.expand, the rule of include/hdlz_png.h in Python, which tests/test_png_cabi.py holds against Pillow.  Where the
encoder was given the scanlines, they are the expected RAW bytes as they stand (test_png_cabi.py shows that png_ref.unfilter undoes the
encoder).  Images are decoded on both routes: many in a call (a wave each) and alone in a call (the batch call's path).

The seams of the unfilter kernel, named: a BAND is 64 rows (a wave's lanes); a TILE is S = 128 // bpp steps of the diagonal wavefront
(pixel x of lane l is taken at step x + l), staged as 16-byte PIECES of a row; a SEGMENT starts at the first row with filter 0 or 1 of
every band of 64 rows counted from row 0."""
import io
import struct
import zipfile
import zlib

import numpy as np
import pytest

import png_ref as P

pytestmark = pytest.mark.gpu


def stage(files):
    import torch
    blob = b"".join(files)
    d = torch.frombuffer(bytearray(blob + bytes(16)), dtype=torch.uint8).cuda()[:len(blob)]
    lens = np.array([len(f) for f in files], np.int64)
    return d, torch.from_numpy(np.cumsum(lens) - lens).cuda(), torch.from_numpy(lens).cuda()


def run_decode(engine, d, pi, first, count, out_fill=0, flags=None):
    """ONE hdlz_png_decode_ws call over images [first, first + count) -> (out, status, record).  flags: default, the index's expand"""
    import torch
    from hdl_deflate_amd import _lib
    L, h = engine.lib, pi.host
    if flags is None:
        flags = _lib.PNG_EXPAND if pi.expand else _lib.PNG_RAW
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


def check_slots(label, pi, first, count, expect, out, status):
    st = [int(s) for s in status.cpu()]
    host = out.cpu().numpy().tobytes()
    base = int(pi.host["out_off"][first]) if count else 0
    for k in range(count):
        want_st, want = expect[first + k]
        assert st[k] == want_st, (label, first + k, st[k], want_st)
        if want_st == P.OK:
            o = int(pi.host["out_off"][first + k]) - base
            got = host[o:o + len(want)]
            if got != want:
                bad = next(i for i in range(len(want)) if got[i] != want[i])
                raise AssertionError((label, first + k, "byte", bad, "of", len(want), got[bad:bad + 8], want[bad:bad + 8]))


def check(engine, label, files, expect=None, flags=P.EXPAND, routed=True):
    """index the files and decode them -- ONE call over all of them and as Engine.decode_png routes them -- against the rule.
    expect: [(status, slot bytes)] (default: png_ref.decode of every file)"""
    d, off, ln = stage(files)
    pi = engine.png_index(d, off, ln, out_align=64, expand=bool(flags))
    ix = P.index(files, flags, 64)
    for i, rec in enumerate(ix["images"]):
        got = {n: int(pi.host[n][i]) for n in P.FIELDS}
        assert got == rec, (label, i, {n: (got[n], rec[n]) for n in P.FIELDS if got[n] != rec[n]})
    assert (pi.host["reserved"] == 0).all()
    r = pi.record
    assert (r.nimages, r.total_z, r.total_raw, r.total_out, r.status, r.reserved) == \
        (len(files), ix["total_z"], ix["total_raw"], ix["total_out"], P.OK, 0), label
    if expect is None:
        expect = [P.decode(f, rec, flags) for f, rec in zip(files, ix["images"])]
    n = len(files)
    out, status, rec = run_decode(engine, d, pi, 0, n)
    check_slots((label, "one call"), pi, 0, n, expect, out, status)
    bad = [k for k, (s, _) in enumerate(expect) if s != P.OK]
    assert (rec.status, rec.first_bad) == ((P.OK, 2 ** 64 - 1) if not bad else (expect[bad[0]][0], bad[0])), (label, rec.status, rec.first_bad)
    assert rec.out_len == (ix["total_out"] if not bad else 0) and rec.reserved == 0
    if routed:
        out, status = engine.decode_png(d, pi)
        check_slots((label, "routed"), pi, 0, n, expect, out, status)
    return d, pi, ix, expect


def made(width, height, colour, depth, filters, seed, flags=P.EXPAND, **kw):
    """an image of the encoder with known scanlines -> (file, (OK, the slot's bytes))"""
    rows = kw.pop("rows", None) or P.random_rows(width, height, colour, depth, seed, smooth=kw.pop("smooth", False))
    f = P.make_png(width, height, colour, depth, rows=rows, filters=filters, seed=seed, **kw)
    rec = P.index([f], flags)["images"][0]
    assert rec["status"] == P.OK
    return f, (P.OK, P.expand(rows, rec, f) if flags & P.EXPAND else rows)


def filter_modes(height, seed):
    rng = np.random.default_rng(seed)
    return [0, 1, 2, 3, 4, [r % 5 for r in range(height)], [int(x) for x in rng.integers(0, 5, height)]]


@pytest.mark.parametrize("flags", [P.EXPAND, P.RAW], ids=["expand", "raw"])
@pytest.mark.parametrize("colour,depth", P.PAIRS)
def test_filter_geometry_and_type_grid(engine, colour, depth, flags):
    """every (colour, depth) pair x every filter alone, a cycling filter, random filters x the geometry seams: widths 1, 2, 3 and one each
    side of the TILE seam (S - 1, S, S + 1 pixels; 2 S + 1: a third tile) and of the 16-byte PIECE seam of a row (15, 16, 17 bytes);
    heights 1, 2, 63, 64, 65, 129: one each side of the BAND seam, and a third band"""
    bpp = P.bpp_of(colour, depth)
    per_byte = 8 // depth if depth < 8 else 1                 # pixels a byte holds below 8 bits
    S = 128 // bpp * per_byte                                 # a tile's steps, in pixels
    piece = 16 * per_byte // bpp if depth >= 8 else 16 * per_byte
    widths = sorted({1, 2, 3, max(1, piece - 1), max(1, piece), piece + 1, S - 1, S, S + 1, 2 * S + 1})
    heights = [1, 2, 63, 64, 65, 129]
    geo = sorted({(w, h) for w in widths for h in (1, 65)} | {(w, h) for w in (3, S + 1) for h in heights})
    files, expect = [], []
    for gi, (w, h) in enumerate(geo):
        for mi, fl in enumerate(filter_modes(h, gi)):
            f, e = made(w, h, colour, depth, fl, seed=gi * 7 + mi, flags=flags, smooth=mi % 2 == 0, level=1)
            files.append(f)
            expect.append(e)
    check(engine, (colour, depth, flags), files, expect, flags, routed=flags == P.EXPAND)


def test_crafted_filter_rows(engine):
    """rows that hit each Paeth tie (bytes drawn from {0, 1, 2, 254, 255}: pa == pb, pb == pc and all equal occur in every row); the 9-bit
    Average sum (a = b = 255); filters 2, 3 and 4 on the first row; a row of filter 0 or 1 directly on each side of a BAND and SEGMENT
    seam (rows 63, 64, 65, 127, 128, 129) among Paeth, Average and Up rows"""
    rng = np.random.default_rng(5)
    files, expect = [], []
    for colour, depth in ((0, 8), (2, 8), (6, 8), (6, 16), (4, 8), (0, 2)):
        rb = P.row_bytes_of(37, colour, depth)
        ties = rng.choice(np.array([0, 1, 2, 254, 255], np.uint8), (200, rb))
        if depth < 8:
            ties[:, -1] &= 0xFF << (rb * 8 - 37 * depth * P.CHANNELS[colour]) & 0xFF
        for first in (2, 3, 4):
            for quiet in ((), (63,), (64,), (65,), (63, 64, 65), (127, 129), (128,), (1, 64, 199)):
                fl = [[4, 3, 2][(r + first) % 3] for r in range(200)]
                fl[0] = first
                for q in quiet:
                    fl[q] = (q + first) & 1
                f, e = made(37, 200, colour, depth, fl, seed=first, rows=ties.tobytes(), level=1)
                files.append(f)
                expect.append(e)
        full = bytes([255]) * (rb * 70)
        for fl in (3, 4, [3, 4] * 35):
            f, e = made(37, 70, colour, depth, fl, seed=0, rows=full if depth >= 8 else None, level=1)
            files.append(f)
            expect.append(e)
    d, pi, ix, expect = check(engine, "crafted", files, expect)
    assert P.decode(files[0], ix["images"][0])[1] == expect[0][1] and P.decode(files[-1], ix["images"][-1])[1] == expect[-1][1]


def _noise(level=6, strategy=zlib.Z_DEFAULT_STRATEGY, **kw):
    return made(300, 300, 2, 8, [r % 5 for r in range(300)], seed=11, level=level, strategy=strategy, **kw)


def test_idat_splits(engine):
    """one chunk; 1-byte chunks; a split inside the zlib header and inside the Adler-32; 8 KiB and 64 KiB chunks; ancillary chunks in
    front, between PLTE and IDAT, and behind"""
    files, expect = [], []
    zlen = P.index([made(40, 30, 2, 8, [r % 5 for r in range(30)], seed=3)[0]])["images"][0]["zlen"]
    anc = [("front", b"gAMA", struct.pack(">I", 45455)), ("front", b"pHYs", bytes(9)), ("mid", b"bKGD", bytes(6)), ("mid", b"tEXt", b"a\0b" * 50),
           ("back", b"tIME", bytes(7)), ("back", b"zTXt", b"k\0\0" + zlib.compress(b"v" * 100))]
    for kw in (dict(), dict(idat=1), dict(idat=[1]), dict(idat=[zlen - 2]), dict(idat=[1, 1, zlen - 5, 1]), dict(idat=7), dict(extra=anc),
               dict(idat=100, extra=anc)):
        f, e = made(40, 30, 2, 8, [r % 5 for r in range(30)], seed=3, **kw)
        files.append(f)
        expect.append(e)
    f, e = made(9, 9, 3, 4, 1, seed=4, extra=anc, trns=bytes([1, 2, 3]))
    files.append(f)
    expect.append(e)
    for idat in (8192, 65536):
        f, e = _noise(idat=idat)
        files.append(f)
        expect.append(e)
    d, pi, ix, _ = check(engine, "splits", files, expect)
    assert [int(x) for x in pi.host["nidat"][:6]] == [1, zlen, 2, 2, 5, -(-zlen // 7)]
    assert pi.host["zlen"][-1] >= 200000 and pi.host["nidat"][-2] > 25 > pi.host["nidat"][-1] > 3


@pytest.mark.parametrize("variant", ["level 6", "stored", "fixed"])
def test_a_large_image_takes_the_one_stream_route(engine, variant):
    """300 x 300 RGB noise (zlen >= HDLZ_PNG_LARGE_MIN): decoded alone (count == 1: the batch call's path) and as one of a batch of 3 (a
    wave), the answers identical; a stored-block and a Z_FIXED variant of the same image"""
    f, e = _noise(**{"level 6": dict(), "stored": dict(level=0), "fixed": dict(strategy=zlib.Z_FIXED)}[variant])
    small = made(5, 3, 6, 8, 4, seed=1)
    d, pi, ix, _ = check(engine, variant, [f], [e])
    assert ix["images"][0]["zlen"] >= P.LARGE_MIN
    alone = run_decode(engine, d, pi, 0, 1)
    files = [small[0], f, small[0]]
    d3, pi3, _, _ = check(engine, (variant, "batch"), files, [small[1], e, small[1]])
    batch = run_decode(engine, d3, pi3, 0, 3)
    o = int(pi3.host["out_off"][1])
    assert alone[0].cpu().numpy().tobytes() == batch[0][o:o + len(e[1])].cpu().numpy().tobytes() == e[1]
    assert int(alone[1][0]) == int(batch[1][1]) == P.OK and alone[2].out_len == len(e[1])


def _damaged():
    """one crafted file per status of the rule and of the judgement -> [(label, file, status)]"""
    good = P.make_png(20, 10, 2, 8, filters=[r % 5 for r in range(10)], seed=9, idat=50)
    rec = P.index([good])["images"][0]
    idat, zlen, used = rec["idat_off"], rec["zlen"], rec["used"]
    stream = P.chunks_of(good, rec)[1]
    rows = P.random_rows(20, 10, 2, 8, 9)
    plain = P.filter_rows(rows, 10, 60, 3, [r % 5 for r in range(10)])

    def flip(f, at, bit=1):
        b = bytearray(f)
        b[at] ^= bit
        return bytes(b)

    def restream(data, adler=None, tail=b""):
        z = zlib.compress(data, 6)
        if adler is not None:
            z = z[:-4] + struct.pack(">I", adler)
        return P.make_png(20, 10, 2, 8, stream=z + tail)
    pal = P.make_png(8, 8, 3, 4, seed=2)
    prec = P.index([pal])["images"][0]
    cases = [
        ("sound", good, P.OK),
        ("bad signature", flip(good, 1), P.E_BAD_HEADER),
        ("the first chunk is not IHDR", good[:12] + b"IHDS" + good[16:], P.E_BAD_HEADER),
        ("truncated in a length word", good[:idat + 2], P.E_NO_EOF),
        ("truncated in data", good[:idat + 30], P.E_NO_EOF),
        ("truncated before IEND", good[:used - 12], P.E_NO_EOF),
        ("7 bytes", good[:7], P.E_BAD_HEADER),
        ("a length word of 2^31", good[:idat] + b"\x80\0\0\0" + good[idat + 4:], P.E_BAD_HEADER),
        ("unknown critical chunk", P.make_png(20, 10, 2, 8, seed=9, extra=[("mid", b"CgBI", b"1234")]), P.E_BAD_BTYPE),
        ("a second IHDR", P.make_png(20, 10, 2, 8, seed=9, extra=[("mid", b"IHDR", bytes(13))]), P.E_BAD_HEADER),
        ("split IDAT run", P.make_png(20, 10, 2, 8, seed=9, idat=50, extra=[("split", b"tEXt", b"x\0y")]), P.E_BAD_HEADER),
        ("no IDAT", good[:idat] + P.chunk(b"IEND", b""), P.E_BAD_HEADER),
        ("bad PLTE length", P.make_png(8, 8, 3, 4, seed=2, palette=bytes(10)), P.E_BAD_HEADER),
        ("empty PLTE", P.make_png(8, 8, 3, 4, seed=2, palette=b""), P.E_BAD_HEADER),
        ("palette image without PLTE", pal[:33] + pal[prec["plte_off"] + 3 * prec["plte_n"] + 4:], P.E_BAD_HEADER),
        ("tRNS of 257 bytes", P.make_png(8, 8, 3, 8, seed=2, trns=bytes(257)), P.E_BAD_HEADER),
        ("bad (colour, depth) pair", P.make_png(20, 10, 2, 8, seed=9, ihdr=struct.pack(">IIBBBBB", 20, 10, 4, 2, 0, 0, 0)), P.E_BAD_HEADER),
        ("width 0", P.make_png(20, 10, 2, 8, seed=9, ihdr=struct.pack(">IIBBBBB", 0, 10, 8, 2, 0, 0, 0)), P.E_BAD_HEADER),
        ("filter method 1", P.make_png(20, 10, 2, 8, seed=9, ihdr=struct.pack(">IIBBBBB", 20, 10, 8, 2, 0, 1, 0)), P.E_BAD_HEADER),
        ("interlace 1", P.make_png(20, 10, 2, 8, seed=9, interlace=1), P.E_BAD_BTYPE),
        ("interlace 2", P.make_png(20, 10, 2, 8, seed=9, interlace=2), P.E_BAD_HEADER),
        ("past the decoders' limit", P.make_png(20, 10, 2, 8, seed=9, ihdr=struct.pack(">IIBBBBB", 1 << 20, 1 << 20, 8, 2, 0, 0, 0)), P.E_OUT_CAPACITY),
        ("IHDR CRC", flip(good, 29), P.E_BAD_CHECKSUM), ("IHDR data", flip(good, 19), P.E_BAD_CHECKSUM),
        ("IDAT CRC", flip(good, idat + 8 + 50 + 3), P.E_BAD_CHECKSUM), ("IDAT data", flip(good, idat + 8 + 20, 0x10), P.E_BAD_CHECKSUM),
        ("the last IDAT's data", flip(good, used - 12 - 4 - 2, 0x40), P.E_BAD_CHECKSUM),
        ("IEND CRC", flip(good, used - 1), P.E_BAD_CHECKSUM),
        ("PLTE CRC", flip(pal, prec["plte_off"] + 3 * prec["plte_n"]), P.E_BAD_CHECKSUM), ("PLTE data", flip(pal, prec["plte_off"] + 5), P.E_BAD_CHECKSUM),
        ("Adler-32 off by one", restream(plain, zlib.adler32(plain) ^ 1), P.E_BAD_CHECKSUM),
        ("one row short", restream(plain[:-61]), P.E_BAD_CHECKSUM),
        ("one byte long", restream(plain + b"\0"), P.E_OUT_CAPACITY),
        ("garbage behind the zlib stream", restream(plain, tail=b"\x55\xAA\x01"), P.E_NO_EOF),
        ("a zlib stream of 5 bytes", P.make_png(20, 10, 2, 8, stream=b"\x78\x9c\x03\x00\x00"), P.E_NO_EOF),
        ("FDICT in the zlib header", P.make_png(20, 10, 2, 8, stream=b"\x78\xbb" + zlib.compress(plain, 6)[2:]), P.E_BAD_HEADER),
        ("filter byte 5", restream(plain[:61 * 4] + b"\x05" + plain[61 * 4 + 1:]), P.E_BAD_SYMBOL),
    ]
    tr = P.make_png(8, 8, 3, 4, seed=2, trns=bytes([9, 8, 7]))
    trec = P.index([tr])["images"][0]
    cases += [("tRNS CRC", flip(tr, trec["trns_off"] + 3), P.E_BAD_CHECKSUM), ("tRNS data", flip(tr, trec["trns_off"] + 1), P.E_BAD_CHECKSUM)]
    return cases


def test_every_status_of_the_rule(engine):
    """one crafted file each; every file stands between two sound ones, which decode as if it were not there"""
    cases = _damaged()
    small = made(7, 5, 4, 8, 4, seed=6)
    files, expect = [small[0]], [small[1]]
    for label, f, want in cases:
        rec = P.index([f])["images"][0]
        st, out = P.decode(f, rec)
        assert st == want, (label, st, want)
        files += [f, small[0]]
        expect += [(st, out), small[1]]
    d, pi, ix, _ = check(engine, "statuses", files, expect)
    for k, (label, f, want) in enumerate(cases):              # ... and alone in a call: the one-stream route judges alike
        out, status, rec = run_decode(engine, d, pi, 1 + 2 * k, 1)
        assert (int(status[0]), rec.status) == (want, want), (label, int(status[0]), rec.status, want)
        assert rec.first_bad == (2 ** 64 - 1 if want == P.OK else 0)


def test_a_batch_of_200_mixed_small_images(engine):
    """every type, sizes 1 to 40, all filters, failed images among them that leave their neighbours intact; sub-ranges decode without the
    rest"""
    rng = np.random.default_rng(21)
    damaged = _damaged()
    files, expect = [], []
    for k in range(200):
        if k % 13 == 5:
            label, f, want = damaged[(k // 13 * 5 + 1) % len(damaged)]
            files.append(f)
            expect.append(P.decode(f, P.index([f])["images"][0]))
            continue
        colour, depth = P.PAIRS[k % len(P.PAIRS)]
        w, h = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        f, e = made(w, h, colour, depth, [int(x) for x in rng.integers(0, 5, h)], seed=k, level=int(rng.integers(0, 10)),
                    idat=None if k % 3 else int(rng.integers(1, 60)), trns=bytes([k & 255, 7]) if colour == 3 and k % 2 else None, smooth=k % 4 == 0)
        files.append(f)
        expect.append(e)
    assert sum(1 for s, _ in expect if s != P.OK) >= 10
    d, pi, ix, _ = check(engine, "batch of 200", files, expect)
    for first, count in ((0, 1), (3, 4), (5, 1), (5, 2), (17, 60), (150, 50), (199, 1)):
        out, status, rec = run_decode(engine, d, pi, first, count, out_fill=first & 255)
        check_slots(("range", first, count), pi, first, count, expect, out, status)
        bad = [k for k in range(count) if expect[first + k][0] != P.OK]
        assert rec.first_bad == (bad[0] if bad else 2 ** 64 - 1) and rec.status == (expect[first + bad[0]][0] if bad else P.OK)
        out2, status2 = engine.decode_png(d, pi, first, count)
        check_slots(("routed range", first, count), pi, first, count, expect, out2, status2)


def _tiny_batch(n, flags):
    """n images of 1 .. 5 x 1 .. 5 pixels: every pair of P.PAIRS in turn, a filter a row at random, every eleventh image interlaced; a
    damaged file at every 97th image, at 191 and 192 and at the last -> (files, png_adam7_ref's index at out_align 64, its decode of each)"""
    import png_adam7_ref as A
    rng = np.random.default_rng(97)
    damaged = [c for c in _damaged() if c[2] != P.OK and not c[0].startswith("interlace")]      # (under ADAM7 interlace 1 is no damage)
    files = []
    for k in range(n):
        if k % 97 == 50 or k in (191, 192, n - 1):
            files.append(damaged[(k // 97 + k) % len(damaged)][1])
            continue
        colour, depth = P.PAIRS[k % len(P.PAIRS)]
        w, h = int(rng.integers(1, 6)), int(rng.integers(1, 6))
        kw = dict(seed=k, level=1, trns=bytes([k & 255, 7]) if colour == 3 and k % 2 else None)
        if k % 11 == 7:
            files.append(A.make_adam7(w, h, colour, depth, filters=[int(x) for x in rng.integers(0, 5, A.total_rows(w, h))], **kw))
        else:
            files.append(P.make_png(w, h, colour, depth, filters=[int(x) for x in rng.integers(0, 5, h)], idat=None if k % 3 else 3, **kw))
    ix = A.index(files, flags, 64)
    return files, ix, [A.decode(f, rec, flags) for f, rec in zip(files, ix["images"])]


def test_a_batch_of_2051_tiny_images_three_a_thread_of_the_planners(engine):
    """2051 images: k_png_offsets and k_png_plan take them three a thread (1024 threads), so a thread's strip holds images of several
    kinds, eleven waves have work, wave 10 a partial strip and the threads behind it none; failed images on both sides of a wave
    seam (191 | 192 at three a thread), in many waves and at the very end.  Records and totals for out_align 64 and 1, every slot and
    status, first_bad, sub-ranges that start and end inside strips, and an index call with room for 1500 records"""
    import torch
    import png_adam7_ref as A
    from hdl_deflate_amd import _lib
    n, flags = 2051, P.EXPAND | A.ADAM7
    files, ix, expect = _tiny_batch(n, flags)
    bad = [k for k, (s, _) in enumerate(expect) if s != P.OK]
    assert {191, 192, n - 1} <= set(bad) and len(bad) >= 24 and sum(r["interlace"] for r in ix["images"]) > 150
    assert {r["colour"] * 100 + r["depth"] for r in ix["images"] if r["status"] == P.OK} == {c * 100 + d for c, d in P.PAIRS}
    d, off, ln = stage(files)
    for align in (64, 1):
        pi = engine.png_index(d, off, ln, out_align=align, expand=True, interlaced=True)
        want = ix if align == 64 else A.index(files, flags, align)
        names = list(P.FIELDS)
        got = np.stack([pi.host[f].astype(np.int64) for f in names], 1)
        ref = np.array([[rec[f] for f in names] for rec in want["images"]], np.int64)
        rows = np.nonzero((got != ref).any(1))[0]
        assert rows.size == 0, (align, int(rows[0]), got[rows[0]].tolist(), ref[rows[0]].tolist())
        assert (pi.host["reserved"] == 0).all()
        r = pi.record
        assert (r.nimages, r.total_z, r.total_raw, r.total_out, r.status, r.reserved) == \
            (n, want["total_z"], want["total_raw"], want["total_out"], P.OK, 0), align
    pi = engine.png_index(d, off, ln, out_align=64, expand=True, interlaced=True)
    out, status, rec = run_decode(engine, d, pi, 0, n, flags=flags)
    check_slots("one call", pi, 0, n, expect, out, status)
    assert (rec.status, rec.first_bad, rec.out_len, rec.reserved) == (expect[bad[0]][0], bad[0], 0, 0)
    for first, count in ((3, 2048), (1500, 551), (2050, 1)):
        out, status, rec = run_decode(engine, d, pi, first, count, out_fill=first & 255, flags=flags)
        check_slots(("range", first, count), pi, first, count, expect, out, status)
        fb = [k for k in range(count) if expect[first + k][0] != P.OK]
        assert rec.first_bad == fb[0] and rec.status == expect[first + fb[0]][0], (first, count)
    # room for 1500 records: those are written, no word behind them, and the totals are those of all 2051
    cap, nrec = 1500, pi.images.shape[1]
    images = torch.full((n, nrec), -1, dtype=torch.int64, device="cuda")
    work = torch.empty(engine.lib.hdlz_png_index_work_bytes(n, cap), dtype=torch.uint8, device="cuda")
    r = engine._record("hdlz_png_index_ws", _lib.PngIndexResult, (work, work.data_ptr(), work.numel()), d.data_ptr(), d.numel(), off.data_ptr(),
                       ln.data_ptr(), n, flags, 64, cap, images.data_ptr())
    assert (r.nimages, r.total_z, r.total_raw, r.total_out, r.status) == (n, ix["total_z"], ix["total_raw"], ix["total_out"], P.E_OUT_CAPACITY)
    assert torch.equal(images[:cap], pi.images[:cap]) and bool((images[cap:] == -1).all())


def test_palette_images(engine):
    """out-of-range indices (black, opaque); a tRNS shorter than the palette (alpha 255 behind it); depths 1, 2 and 4 with widths that
    leave pad bits; a PLTE of fewer than 2^depth entries"""
    files, expect = [], []
    for depth, w in ((1, 13), (2, 7), (4, 5), (8, 9), (1, 8), (4, 33)):
        for npal, trns in ((1 << depth, None), (max(1, (1 << depth) // 2), None), (max(1, (1 << depth) - 1), bytes([0, 128])), (1, bytes([77]))):
            pal = bytes(np.random.default_rng(depth * 10 + npal).integers(0, 256, 3 * min(npal, 256), dtype=np.uint8))
            f, e = made(w, 11, 3, depth, [r % 5 for r in range(11)], seed=depth + w, palette=pal, trns=trns)
            files.append(f)
            expect.append(e)
    d, pi, ix, _ = check(engine, "palette", files, expect)
    assert set(pi.host["channels_out"]) == {3, 4}
    k = 1 * 4 + 3                                            # depth 2, one palette entry, one tRNS byte
    a = np.frombuffer(expect[k][1], np.uint8).reshape(11, 7, 4)
    assert (a[..., 3] == 255).any() and (a[..., 3] == 77).any() and (a[a[..., 3] == 255][:, :3] == 0).all()


def test_load_png_and_a_zip_of_pngs(engine):
    """shapes, dtypes and values of load_png; a ZIP of PNGs (stored and deflated entries of zipfile) read with zip_index(out_align=64),
    inflate_zip and load_png((out, out_off, usize)) -- nothing staged in between"""
    import torch
    from hdl_deflate_amd import load_png, HdlzStatusError
    items = [made(33, 17, 6, 8, 4, seed=1), made(9, 4, 0, 16, 3, seed=2), made(12, 5, 3, 2, 1, seed=3, trns=bytes([5])), made(31, 7, 2, 16, 2, seed=4),
             made(6, 6, 0, 1, 0, seed=5), _noise()]
    want = [((17, 33, 4), torch.uint8), ((4, 9), torch.uint16), ((5, 12, 4), torch.uint8), ((7, 31, 3), torch.uint16), ((6, 6), torch.uint8),
            ((300, 300, 3), torch.uint8)]
    got = load_png(engine, [f for f, _ in items])
    one = load_png(engine, items[0][0])
    assert torch.equal(one, got[0])
    for t, (f, (st, e)), (shape, dtype) in zip(got, items, want):
        assert t.is_cuda and tuple(t.shape) == shape and t.dtype == dtype and t.data_ptr() % 64 == 0
        assert t.cpu().numpy().tobytes() == e
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w") as zf:
        for k, (f, _) in enumerate(items):
            zf.writestr(zipfile.ZipInfo("img%d.png" % k), f, zipfile.ZIP_STORED if k % 2 else zipfile.ZIP_DEFLATED)
    z = buf.getvalue()
    dz = torch.frombuffer(bytearray(z + bytes(16)), dtype=torch.uint8).cuda()[:len(z)]
    zi = engine.zip_index(dz, out_align=64)
    out, out_off, status = engine.inflate_zip(dz, zi)
    assert [int(s) for s in status] == [0] * len(items)
    usize = zi.entries[:, 3] >> 32                            # (the record's csize and usize share a word)
    assert [int(u) for u in usize] == [len(f) for f, _ in items]
    via = load_png(engine, (out, out_off, usize))
    for t, g in zip(via, got):
        assert t.dtype == g.dtype and torch.equal(t, g)
    with pytest.raises(HdlzStatusError) as ei:
        load_png(engine, [items[0][0], items[1][0][:40], items[2][0]])
    assert ei.value.first_bad == 1 and ei.value.status == P.E_NO_EOF
    bad = bytearray(items[4][0])
    bad[-1] ^= 1
    with pytest.raises(HdlzStatusError) as ei:
        load_png(engine, [items[0][0], bytes(bad)])
    assert ei.value.first_bad == 1 and ei.value.status == P.E_BAD_CHECKSUM


def test_the_calls_are_hip_graph_capturable(engine):
    """index + a count >= 2 decode + a count == 1 decode with caller scratch captured into ONE HIP graph and replayed twice: nothing is
    allocated, the host reads nothing in between, and the results are identical each time"""
    import torch
    from hdl_deflate_amd import _lib
    L = engine.lib
    items = [made(20 + k, 9 + k, *P.PAIRS[(3 * k) % len(P.PAIRS)], [r % 5 for r in range(9 + k)], seed=k) for k in range(5)] + [_noise()]
    files = [f for f, _ in items]
    ix = P.index(files)
    d, off, ln = stage(files)
    n, total = 6, ix["total_out"]
    big = ix["images"][5]
    images = torch.zeros((n, 17), dtype=torch.int64, device="cuda")
    rec = torch.zeros(16, dtype=torch.int64, device="cuda")     # the three records
    iwork = torch.empty(L.hdlz_png_index_work_bytes(n, n), dtype=torch.uint8, device="cuda")
    out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    args5 = (sum(r["nidat"] for r in ix["images"][:5]), big["z_off"], big["raw_off"])
    args1 = (big["nidat"], P.r16(big["zlen"] + 8), P.r16(big["raw_len"]))
    w5 = torch.empty(L.hdlz_png_decode_work_bytes(5, *args5), dtype=torch.uint8, device="cuda")
    w1 = torch.empty(L.hdlz_png_decode_work_bytes(1, *args1), dtype=torch.uint8, device="cuda")

    def calls():
        s = torch.cuda.current_stream().cuda_stream
        assert L.hdlz_png_index_ws(d.data_ptr(), d.numel(), off.data_ptr(), ln.data_ptr(), n, 1, 64, n, images.data_ptr(), rec.data_ptr(),
                                   iwork.data_ptr(), iwork.numel(), s) == 0
        assert L.hdlz_png_decode_ws(d.data_ptr(), d.numel(), images.data_ptr(), 0, 5, 1, *args5, out.data_ptr(), big["out_off"], status.data_ptr(),
                                    rec[5:].data_ptr(), w5.data_ptr(), w5.numel(), s) == 0
        assert L.hdlz_png_decode_ws(d.data_ptr(), d.numel(), images.data_ptr(), 5, 1, 1, *args1, out.data_ptr() + big["out_off"], big["out_len"],
                                    status[5:].data_ptr(), rec[8:].data_ptr(), w1.data_ptr(), w1.numel(), s) == 0
    calls()                                                      # eager once
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            calls()
    seen = []
    for k in range(2):
        images.fill_(-1 - k); rec.fill_(k); out.fill_(k); status.fill_(7); iwork.fill_(0x11 * k); w5.fill_(0x22 * k); w1.fill_(0x33 * k)
        g.replay()
        torch.cuda.synchronize()
        host = out.cpu().numpy().tobytes()
        slots = [host[r["out_off"]:r["out_off"] + r["out_len"]] for r in ix["images"]]
        seen.append((images.cpu().numpy().tobytes(), rec[:11].cpu().numpy().tobytes(), slots, status.cpu().numpy().tobytes()))
        r = _lib.PngIndexResult.from_buffer_copy(rec[:5].cpu().numpy().tobytes())
        assert (r.status, r.nimages, r.total_out) == (P.OK, 6, total)
        assert [int(x) for x in status] == [0] * 6
        assert slots == [e for _, (_, e) in items]
        gaps = np.ones(total, bool)
        for r in ix["images"]:
            gaps[r["out_off"]:r["out_off"] + r["out_len"]] = False
        assert gaps.any() and (np.frombuffer(host, np.uint8)[gaps] == k).all()           # nothing outside the slots was written
    assert seen[0] == seen[1]
