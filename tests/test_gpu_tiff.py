"""GPU (-m gpu): hdlz_tiff_index_ws and hdlz_tiff_decode_ws through Engine.tiff_index, Engine.decode_tiff and load_tiff, held against
the rule and the pixels as tests/tiff_ref.py states them, byte for byte: the records of every accepted type and of one crafted file per
refusal line; the pixels over byte order x bits x samples x predictor x compression; the geometries at which k_tiff_unpredict takes
another path (rows below a lane's 16 bytes, several rows a wave, exactly one step, a step and a sample, carries across steps, pixels
cut by lane borders at every channel phase, edge tiles on both axes); pages, batches, sub-ranges and the one-chunk route; the verdicts
of damaged chunks; files written by libtiff; TIFFs out of a ZIP."""
import io
import os
import struct
import zipfile
import zlib

import numpy as np
import pytest
import torch

import tiff_ref as T
from conftest import GOLD
from test_tiff_cpu import GOLDEN, crafted

pytestmark = pytest.mark.gpu


def staged(engine, files, gap=0):
    """the files in one device buffer, `gap` bytes of 0xEE between them -> (buffer, offsets, lengths) on the device"""
    blob, offs = bytearray(), []
    for f in files:
        offs.append(len(blob))
        blob += f + b"\xEE" * gap
    d = engine._stage(bytes(blob))[:len(blob)]
    return d, torch.tensor(offs, dtype=torch.int64, device=d.device), torch.tensor([len(f) for f in files], dtype=torch.int64, device=d.device)


def records_equal(index, ix, label=""):
    got = [tuple(int(r[f]) for f in T.FIELDS) for r in index.host]
    want = [tuple(rec[f] for f in T.FIELDS) for rec in ix["images"]]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (label, k, dict((f, (a, b)) for f, a, b in zip(T.FIELDS, g, w) if a != b))
    assert len(got) == len(want) and not index.host["reserved"].any()
    r = index.record
    assert (r.nimages, r.total_chunks, r.total_raw, r.total_out, r.status, r.reserved) == \
        (ix["nimages"], ix["total_chunks"], ix["total_raw"], ix["total_out"], ix["status"], 0), label


def check(engine, files, pages=None, gap=0, label="", first=0, count=None):
    """index and decode `files` on the device and by the rule; every record, status and slot must agree -> (index, out, status, rule's statuses)"""
    d, off, ln = staged(engine, files, gap)
    offs = [int(o) for o in off.cpu()]
    index = engine.tiff_index(d, off, ln, pages=pages)
    ix = T.index(files, pages, offsets=offs, files_len=d.numel())
    records_equal(index, ix, label)
    count = len(files) - first if count is None else count
    out, status = engine.decode_tiff(d, index, first, count)
    st, o = status.cpu().numpy(), out.cpu().numpy()
    base = ix["images"][first]["out_off"] if count else 0
    want_st = []
    for k in range(first, first + count):
        rec = ix["images"][k]
        want, data = T.decode(files[k], rec)
        want_st.append(want)
        if want is T.DECODER:
            assert st[k - first] not in (T.OK, T.E_BAD_PARAM), (label, k, int(st[k - first]))
            continue
        assert st[k - first] == want, (label, k, int(st[k - first]), want)
        if want == T.OK:
            at = rec["out_off"] - base
            got = o[at:at + rec["out_len"]].tobytes()
            if got != data:
                a, b = np.frombuffer(got, np.uint8), np.frombuffer(data, np.uint8)
                bad = np.nonzero(a != b)[0]
                raise AssertionError((label, k, "pixels", len(bad), bad[:8].tolist(), a[bad[:8]].tolist(), b[bad[:8]].tolist()))
    return index, out, status, want_st


def page(fmt, bits, samples, h, w, seed, **kw):
    return dict(pix=T.random_pixels(h, w, samples, fmt, bits, seed), **kw)


# ---- the index
def test_index_records_of_every_accepted_type(engine):
    files, k = [], 0
    for be in (False, True):
        for fmt, bits in ((1, 8), (2, 8), (1, 16), (2, 16), (1, 32), (2, 32), (3, 32), (1, 64), (2, 64), (3, 64)):
            for samples in (1, 3, 8):
                k += 1
                layout = (dict(rps=4), dict(tile=(16, 16)), dict(rps_tag=False), dict(tile=(32, 16), arrays=T.SHORT))[k % 4]
                files.append(T.make_tiff([page(fmt, bits, samples, 9 + k % 5, 11 + k % 7, k, predictor=1 + k % (3 if fmt == 3 else 2),
                                               compression=(1, 8, 32946)[k % 3], unsorted=k if k % 3 == 0 else None, **layout)], big=be))
    index = check(engine, files, gap=3, label="every type")[0]
    assert all(s is not None for s in index.shapes)


def test_index_refusals_one_crafted_file_each(engine):
    cases = crafted()
    files = [f for _, f, _ in cases]
    d, off, ln = staged(engine, files, gap=5)
    index = engine.tiff_index(d, off, ln)
    records_equal(index, T.index(files, offsets=[int(o) for o in off.cpu()], files_len=d.numel()), "crafted")
    for (label, _, want), got in zip(cases, index.host["status"]):
        assert got == want, (label, int(got), want)
    assert {T.OK, T.E_BAD_HEADER, T.E_BAD_BTYPE, T.E_NO_EOF, T.E_OUT_CAPACITY} == set(int(s) for s in index.host["status"])
    check(engine, files, label="crafted, decoded: a failed image between good ones")


def test_a_file_outside_the_buffer_and_the_sizing_call(engine):
    good = T.make_tiff([page(1, 8, 3, 20, 24, 1, rps=6)])
    d, off, ln = staged(engine, [good, good, good])
    ln2 = ln.clone()
    ln2[2] += 1                                               # one byte past the buffer
    index = engine.tiff_index(d, off, ln2)
    assert [int(s) for s in index.host["status"]] == [T.OK, T.OK, T.E_BAD_PARAM] and index.shapes[2] is None
    L, n = engine.lib, 3
    from hdl_deflate_amd import _lib
    work = torch.empty(L.hdlz_tiff_index_work_bytes(n, 0), dtype=torch.uint8, device=d.device)
    res = torch.zeros(5, dtype=torch.int64, device=d.device)
    rc = L.hdlz_tiff_index_ws(d.data_ptr(), d.numel(), off.data_ptr(), ln.data_ptr(), None, n, 64, 0, None, res.data_ptr(), work.data_ptr(), work.numel(),
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    rec = _lib.TiffIndexResult.from_buffer_copy(res.cpu().numpy().tobytes())
    full = T.index([good] * 3)
    assert rc == 0 and (rec.nimages, rec.total_chunks, rec.total_raw, rec.total_out, rec.status) == \
        (3, full["total_chunks"], full["total_raw"], full["total_out"], T.E_OUT_CAPACITY)


# ---- the pixels
@pytest.mark.parametrize("be", [False, True])
def test_pixels_over_types_predictors_and_compressions(engine, be):
    files, k = [], 0
    for bits in (8, 16, 32, 64):
        for samples in (1, 2, 3, 4, 8):
            for pred in (1, 2, 3):
                for comp in (1, 8, 32946):
                    k += 1
                    fmt = 3 if pred == 3 else (1, 2, 3)[k % 3] if bits >= 32 else (1, 2)[k % 2]
                    if fmt == 3 and bits < 32:
                        continue
                    layout = (dict(rps=5), dict(tile=(16, 16)), dict(), dict(tile=(32, 16)))[k % 4]
                    files.append(T.make_tiff([page(fmt, bits, samples, 19, 21, k, predictor=pred, compression=comp, pad=k % 3, **layout)], big=be))
    check(engine, files, label=("the product", be))


def _geometries():
    """(label, page) at the sizes where k_tiff_unpredict takes another path; random full-range words, so that the sums wrap"""
    g = [("1 x 1", page(1, 8, 1, 1, 1, 1, predictor=2)), ("1 x 1, 8 samples of 64 bits", page(2, 64, 8, 1, 1, 2, predictor=2)),
         ("37 x 45 in 16 x 16 tiles", page(1, 8, 3, 45, 37, 3, predictor=2, tile=(16, 16))),
         ("37 x 45 in 32 x 16 tiles", page(1, 16, 3, 45, 37, 4, predictor=2, tile=(32, 16))),
         ("37 x 45 floats in 16 x 16 tiles", page(3, 32, 3, 45, 37, 5, predictor=3, tile=(16, 16))),
         ("37 rows in strips of 5", page(1, 16, 2, 37, 29, 6, predictor=2, rps=5)), ("37 rows in strips of 64", page(1, 16, 2, 37, 29, 7, predictor=2, rps=64)),
         ("a row below one lane's 16 bytes", page(1, 8, 3, 9, 5, 8, predictor=2)), ("a row of 16 bytes", page(1, 16, 1, 70, 8, 9, predictor=2)),
         ("a row of 17 bytes: two lanes", page(1, 8, 1, 70, 17, 10, predictor=2)), ("several rows a wave: 100 bytes", page(1, 8, 4, 131, 25, 11, predictor=2)),
         ("several rows a wave: 512 bytes", page(1, 32, 1, 67, 128, 12, predictor=2)), ("a row of 513 bytes", page(1, 8, 3, 5, 171, 13, predictor=2)),
         ("a row of exactly 1024 bytes", page(1, 16, 2, 6, 256, 14, predictor=2)), ("a row of 1024 bytes and one sample", page(1, 16, 1, 6, 513, 15, predictor=2)),
         ("a row of 1024 bytes and one pixel of three", page(1, 8, 3, 4, 342, 16, predictor=2)),
         ("a 4200-byte row: carries across steps", page(1, 16, 3, 5, 700, 17, predictor=2)),
         ("a 4200-byte row, big-endian words", page(2, 16, 3, 5, 700, 18, predictor=2)),
         ("128 x 128 tiles of 4 samples", page(1, 8, 4, 150, 200, 19, predictor=2, tile=(128, 128))),
         ("128 x 128 tiles of float RGBA", page(3, 32, 4, 130, 140, 20, predictor=3, tile=(128, 128))),
         ("doubles in planes, 5 samples", page(3, 64, 5, 7, 131, 21, predictor=3)), ("floats, a row of one", page(3, 32, 1, 3, 1, 22, predictor=3)),
         ("uncompressed floats in planes", page(3, 32, 2, 9, 77, 23, predictor=3, compression=1, tile=(48, 16)))]
    # 3 samples of 8 bits: a lane's first byte has channel (16 lane) mod 3, so the lane borders fall on every channel phase; and 5, 6, 7
    # samples, whose phases never align with the lanes
    for s, w in ((3, 80), (3, 341), (5, 77), (6, 50), (7, 200), (8, 33)):
        g.append(("%d samples of 8 bits, width %d" % (s, w), page(1, 8, s, 4, w, 30 + s, predictor=2)))
    for b, s in ((32, 3), (32, 8), (64, 3), (64, 5), (16, 7)):
        g.append(("%d samples of %d bits" % (s, b), page(1, b, s, 3, 301, 40 + s + b, predictor=2)))
    return g


def test_the_geometries_where_the_kernel_takes_another_path(engine):
    geo = _geometries()
    for be in (False, True):
        files = [T.make_tiff([dict(pg, compression=(8, 1)[k % 2] if "compression" not in pg else pg["compression"])], big=be) for k, (_, pg) in enumerate(geo)]
        try:
            check(engine, files, label=("geometries", be))
        except AssertionError as e:                           # name the geometry
            k = e.args[0][1] if e.args and isinstance(e.args[0], tuple) else None
            raise AssertionError((geo[k][0] if isinstance(k, int) and k < len(geo) else None,) + tuple(e.args))


# ---- routes and pages
def test_three_pages_read_by_pages(engine):
    a, b, c = page(1, 8, 3, 30, 40, 1), page(1, 16, 1, 17, 23, 2, tile=(16, 16), predictor=2), page(3, 32, 1, 9, 12, 3, predictor=3, compression=1)
    f = T.make_tiff([a, b, c], big=True)
    index = check(engine, [f] * 5, pages=[2, 0, 1, 3, 0], label="pages")[0]
    assert [int(s) for s in index.host["status"]] == [T.OK, T.OK, T.OK, T.E_NO_EOF, T.OK]
    assert index.host["next_ifd"][0] == 0 and index.host["next_ifd"][1] == index.host["ifd_off"][2]
    assert index.shapes[:3] == [(9, 12), (30, 40, 3), (17, 23)] and index.dtypes[:3] == [torch.float32, torch.uint8, torch.uint16]


def _batch64():
    files = []
    bad = {k: f for k, (_, f, want) in enumerate(crafted()) if want != T.OK}
    damaged = lambda k, d: d if k != 0 else d[:len(d) // 2] + bytes([d[len(d) // 2] ^ 1]) + d[len(d) // 2 + 1:]      # (level 0: a payload byte)
    for k in range(64):
        if k % 9 == 4:
            files.append(bad[sorted(bad)[k % len(bad)]])
            continue
        fmt, bits = ((1, 8), (1, 16), (3, 32), (2, 32), (3, 64), (1, 8))[k % 6]
        layout = (dict(rps=3 + k % 11), dict(tile=(16, 16)), dict(), dict(tile=(32, 48)))[k % 4]
        files.append(T.make_tiff([page(fmt, bits, 1 + k % 4, 10 + 3 * (k % 13), 8 + 5 * (k % 7), k, predictor=(3 if fmt == 3 and k % 2 else 1 + k % 2),
                                       compression=(8, 8, 1)[k % 3], pad=k % 2, level=0 if k % 16 == 7 else 6,
                                       **(dict(damage=damaged) if k % 16 == 7 else {}), **layout)], big=bool(k % 2)))
    return files


def test_a_batch_of_64_small_files_some_failing(engine):
    files = _batch64()
    _, _, status, want = check(engine, files, gap=1, label="batch of 64")
    st = status.cpu().numpy()
    assert (st != T.OK).sum() == sum(1 for w in want if w != T.OK) >= 8 and T.E_BAD_CHECKSUM in st


def test_any_sub_range_equals_the_same_slots_of_the_full_decode(engine):
    files = _batch64()[:24]
    d, off, ln = staged(engine, files)
    index = engine.tiff_index(d, off, ln)
    full, fst = engine.decode_tiff(d, index)
    oo, ol, ok = index.host["out_off"], index.host["out_len"], index.host["status"] == T.OK
    for first, count in ((0, 1), (3, 7), (4, 1), (10, 14), (23, 1), (5, 0)):
        out, st = engine.decode_tiff(d, index, first, count)
        assert torch.equal(st, fst[first:first + count]), (first, count)
        for k in range(first, first + count):
            if ok[k] and int(fst[k]) == T.OK:
                a = int(oo[k] - oo[first])
                assert torch.equal(out[a:a + int(ol[k])], full[int(oo[k]):int(oo[k] + ol[k])]), (first, count, k)


def test_a_large_single_strip_takes_the_one_stream_route(engine):
    pix = T.random_pixels(256, 256, 3, 1, 8, 77)
    pix[:, 128:] = pix[:, :128]                               # half of it matches: a stream of both literals and copies
    one = T.make_tiff([dict(pix=pix, predictor=2)])
    strips = T.make_tiff([dict(pix=pix, predictor=2, rps=16)])
    rec = T.index([one])["images"][0]
    assert rec["nchunks"] == 1 and T.chunk_words(one, rec, 0)[1] >= T.LARGE_MIN and len(one) >= T.LARGE_MIN
    small = T.make_tiff([page(1, 8, 1, 5, 5, 1)])
    index, out, status, _ = check(engine, [small, one, strips, small], label="one stream")
    assert status.tolist() == [0, 0, 0, 0]
    o, n = index.host["out_off"], index.host["out_len"]
    assert torch.equal(out[int(o[1]):int(o[1] + n[1])], out[int(o[2]):int(o[2] + n[2])])
    check(engine, [one], label="one stream, alone")
    check(engine, [T.make_tiff([dict(pix=pix, predictor=2, compression=1)])], label="one stored strip, alone")
    # the one-chunk route's own refusal and verdicts
    cut = T.make_tiff([dict(pix=pix, predictor=2, damage=lambda k, d: d[:len(d) // 2])])
    flip = T.make_tiff([dict(pix=pix, level=0, damage=lambda k, d: d[:9000] + bytes([d[9000] ^ 4]) + d[9001:])])
    padded = T.make_tiff([dict(pix=pix, predictor=2, pad=7)])
    for f, want in ((cut, None), (flip, T.E_BAD_CHECKSUM), (padded, T.OK)):
        st = check(engine, [f], label=("one stream", want))[2]
        assert want is None or int(st[0]) == want


# ---- the verdicts
def test_the_verdicts_of_damaged_chunks(engine):
    pix = T.random_pixels(12, 10, 1, 1, 8, 9)
    flip = lambda at, bit=1: (lambda k, d: d if k != 1 else d[:at % len(d)] + bytes([d[at % len(d)] ^ bit]) + d[at % len(d) + 1:])
    mk = lambda **kw: T.make_tiff([dict(dict(pix=pix, rps=4, level=0), **kw)])
    cases = [("sound", mk(), T.OK), ("padded", mk(pad=5), T.OK), ("a payload bit", mk(damage=flip(12)), T.E_BAD_CHECKSUM),
             ("an Adler byte", mk(damage=flip(-1)), T.E_BAD_CHECKSUM), ("a bad zlib header", mk(damage=flip(1, 0x20)), T.E_BAD_HEADER),
             ("a chunk that decodes long", mk(damage=lambda k, d: d if k != 1 else zlib.compress(bytes(41), 0)), T.E_OUT_CAPACITY),
             ("a chunk that decodes short", mk(damage=lambda k, d: d if k != 1 else zlib.compress(bytes(39), 0)), T.E_BAD_CHECKSUM),
             ("a truncated chunk", mk(level=6, damage=lambda k, d: d if k != 1 else d[:len(d) - 6]), T.E_NO_EOF),
             ("a chunk without its Adler-32", mk(damage=lambda k, d: d if k != 1 else d[:-4]), T.E_NO_EOF),
             ("a truncated stored chunk", mk(compression=1, override={279: (T.LONG, 3, struct.pack("<3I", 40, 39, 40))}), T.E_NO_EOF),
             ("five bytes", mk(damage=lambda k, d: d if k != 1 else d[:5]), T.E_NO_EOF),
             ("a chunk behind the file", mk(override={273: (T.LONG, 3, struct.pack("<3I", 8, 1 << 20, 8))}), T.E_NO_EOF)]
    files = [f for _, f, _ in cases]
    st = check(engine, files, gap=2, label="verdicts")[2].cpu().numpy()
    for (label, _, want), got in zip(cases, st):
        assert got == want, (label, int(got), want)
    for k in (2, 5, 7):                                       # ... and alone, a call each
        assert int(check(engine, [files[k]], label=("verdict alone", k))[2][0]) == cases[k][2]


# ---- other writers, round trips
def test_the_golden_libtiff_files(engine):
    import hdl_deflate_amd
    files = [open(os.path.join(GOLD, "tiff", n + ".tif"), "rb").read() for n in GOLDEN]
    got = hdl_deflate_amd.load_tiff(engine, files)
    for n, g in zip(GOLDEN, got):
        want = np.load(os.path.join(GOLD, "tiff", n + ".npy"))
        assert g.is_cuda and tuple(g.shape) == want.shape and g.cpu().numpy().dtype == want.dtype and (g.cpu().numpy() == want).all(), n
    check(engine, files, label="golden")


def test_load_tiff_shapes_dtypes_and_failures(engine):
    import hdl_deflate_amd
    from hdl_deflate_amd.errors import HdlzStatusError
    want = {(1, 8): torch.uint8, (2, 8): torch.int8, (1, 16): torch.uint16, (2, 16): torch.int16, (1, 32): torch.uint32, (2, 32): torch.int32,
            (3, 32): torch.float32, (1, 64): torch.uint64, (2, 64): torch.int64, (3, 64): torch.float64}
    pages = [page(f, b, 1 + k % 3, 6 + k, 9 - k % 4, k, tile=(16, 16) if k % 2 else None, predictor=1 + k % 2) for k, (f, b) in enumerate(want)]
    for pg in pages:
        if pg["tile"] is None:
            del pg["tile"]
    got = hdl_deflate_amd.load_tiff(engine, [T.make_tiff([pg], big=bool(k % 2)) for k, pg in enumerate(pages)])
    for pg, g, dt in zip(pages, got, want.values()):
        assert g.dtype == dt and tuple(g.shape) == pg["pix"].shape and g.cpu().numpy().tobytes() == pg["pix"].tobytes()
        assert g.data_ptr() % 64 == 0
    stack = T.make_tiff(pages[:3])
    one = hdl_deflate_amd.load_tiff(engine, stack, page=2)
    assert one.cpu().numpy().tobytes() == pages[2]["pix"].tobytes()
    both = hdl_deflate_amd.load_tiff(engine, [stack, stack], page=[1, 0])
    assert both[0].cpu().numpy().tobytes() == pages[1]["pix"].tobytes() and both[1].cpu().numpy().tobytes() == pages[0]["pix"].tobytes()
    with pytest.raises(HdlzStatusError) as e:
        hdl_deflate_amd.load_tiff(engine, [stack, stack[:40], stack])
    assert e.value.first_bad == 1
    with pytest.raises(HdlzStatusError) as e:
        hdl_deflate_amd.load_tiff(engine, [stack, T.make_tiff([dict(pages[0], damage=lambda k, d: d[:-1] + bytes([d[-1] ^ 1]))])])
    assert e.value.first_bad == 1 and e.value.status == T.E_BAD_CHECKSUM


def test_tiffs_out_of_a_zip(engine):
    import hdl_deflate_amd
    pages = [page(1, 8, 3, 33, 47, 1, predictor=2, rps=8), page(3, 32, 1, 20, 31, 2, predictor=3, tile=(16, 16)), page(1, 16, 1, 9, 9, 3, compression=1)]
    files = [T.make_tiff([pg], big=k == 1) for k, pg in enumerate(pages)]
    b = io.BytesIO()
    with zipfile.ZipFile(b, "w", zipfile.ZIP_DEFLATED) as z:
        for k, f in enumerate(files):
            z.writestr("image%d.tif" % k, f)
    blob = b.getvalue()
    d = engine._stage(blob)[:len(blob)]
    zi = engine.zip_index(d, out_align=64)
    out, out_off, status = engine.inflate_zip(d, zi)
    assert status.tolist() == [0, 0, 0]
    got = hdl_deflate_amd.load_tiff(engine, (out, out_off, torch.from_numpy(zi.host["usize"].astype(np.int64))))
    for pg, g in zip(pages, got):
        assert g.cpu().numpy().tobytes() == pg["pix"].tobytes() and tuple(g.shape) == pg["pix"].shape
