"""GPU (-m gpu): PNG files written on the device (include/hdlz_png_write.h) -- hdlz_png_filter_ws, the ragged compress batch and
hdlz_png_write_ws through Engine.encode_png and save_png, every file held byte for byte against the two rules of
tests/png_write_ref.py (the CPU oracle's rows, zlib's checksums; never device output), at the shapes the filter kernel branches on:
its wave step, its register-row limit and its band height (png_write_ref.kernel_constants()), rows that start at every alignment,
pixels that straddle the 16-byte lanes, streams under 5 bytes, members that straddle chunk seams."""
import io

import numpy as np
import pytest
import torch

import png_ref as P
import png_write_ref as W

pytestmark = pytest.mark.gpu
K = W.kernel_constants()
MODES = (0, 1, 2, 3, 4, W.ADAPTIVE)


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                 # (a copy: a case's bytes may be read-only)


def encode(engine, arrays, **kw):
    """numpy images -> (the files as bytes, the index) through Engine.encode_png"""
    flat = torch.cat([dev(a).view(torch.uint8).reshape(-1) for a in arrays])
    shapes = [(a.shape[0], a.shape[1], a.shape[2] if a.ndim == 3 else 1, 8 * a.dtype.itemsize) for a in arrays]
    files, index = engine.encode_png(flat, shapes, **kw)
    host = files.cpu().numpy().tobytes()
    return [host[int(r["file_off"]):int(r["file_off"]) + int(r["file_len"])] for r in index.host], index


def pixels(colour, depth, width, height, seed):
    shape, dtype = W.shape_for(colour, depth, width, height)
    return W.smooth(shape, dtype, seed) if seed % 3 else W.noise(shape, dtype, seed)


def shapes_of(colour, depth):
    """(width, height) of one pair: row_bytes of 1 (grey), 15, 16, 17 and the wave step and the register row - 1, + 0, + 1 as nearly
    as the pixel size allows, every height of 1, 2, 3 and the band +- 1 among them; all six heights at a narrow row; streams of 2 .. 5
    bytes"""
    bpp = P.bpp_of(colour, depth)
    heights = (1, 2, 3, K.BAND - 1, K.BAND, K.BAND + 1)
    widths = sorted({max(1, -(-rb // bpp)) for rb in (1, 15, 16, 17, K.STEP - 1, K.STEP, K.STEP + 1, K.ROW_REG_MAX - 1, K.ROW_REG_MAX, K.ROW_REG_MAX + 1)} |
                    {max(1, rb // bpp) for rb in (15, 17, K.STEP - 1, K.STEP + 1, K.ROW_REG_MAX - 1, K.ROW_REG_MAX + 1)})
    got = [(w, heights[k % len(heights)]) for k, w in enumerate(widths)]
    got += [(5, h) for h in heights] + [(2 * K.STEP // bpp + 3, K.BAND + 1)]
    got += [(w, h) for w, h in ((1, 1), (2, 1), (3, 1), (4, 1), (1, 2), (1, 3)) if h * (w * bpp + 1) <= 6]
    return got


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("colour,depth", W.PAIRS)
def test_files_are_the_rules_bytes_at_the_shapes_the_kernel_branches_on(engine, colour, depth, mode):
    arrays = [pixels(colour, depth, w, h, 7 * k + colour + depth) for k, (w, h) in enumerate(shapes_of(colour, depth))]
    files, index = encode(engine, arrays, filter=mode)
    filters = index.row_filters.cpu().numpy()
    for k, a in enumerate(arrays):
        want = W.expected(a, mode=mode)
        assert files[k] == want.file, (k, a.shape, len(files[k]), len(want.file))
        assert filters[index.row_base[k]:index.row_base[k + 1]].tolist() == want.filters, (k, a.shape)
    assert index.write_record.status == W.OK and index.write_record.first_bad == W.NONE64 and index.write_record.total_len == sum(map(len, files))


def test_the_crafted_rows_take_the_filter_the_rule_names(engine):
    """a strict winner for every filter, ties between every adjacent pair (the lower one wins), all-zero rows, a first row"""
    W.crafted_properties()
    cases = W.crafted_images()
    files, index = encode(engine, [a for _, a in cases])
    filters = index.row_filters.cpu().numpy()
    for k, (label, a) in enumerate(cases):
        want = W.expected(a)
        assert filters[index.row_base[k]:index.row_base[k + 1]].tolist() == want.filters, label
        assert files[k] == want.file, label


def test_members_straddle_the_chunk_seams(engine):
    """block = 64: nine members; IDAT chunks of 1 and 7 bytes, of exactly zlen (one chunk) and of zlen - 1 (a last chunk of one byte)"""
    a = W.smooth((9, 20, 3), np.uint8, 4)
    zlen = len(W.expected(a, block=64).z)
    for idat in (1, 7, zlen, zlen - 1):
        want = W.expected(a, block=64, idat=idat)
        files, index = encode(engine, [a], block=64, idat=idat)
        assert files[0] == want.file, idat
        assert int(index.host["nidat"][0]) == -(-zlen // idat) and int(index.host["zlen"][0]) == zlen


def test_a_512_x_512_rgb_image_at_the_defaults(engine):
    a = W.smooth((512, 512, 3), np.uint8, 1)
    files, index = encode(engine, [a])
    want = W.expected(a)
    assert files[0] == want.file
    assert index.row_filters.cpu().numpy().tolist() == want.filters


def test_more_chunks_than_the_crc_grid_holds(engine):
    """idat = 1 over a stream of more than 4096 bytes: the CRC kernel's workgroups make a second trip"""
    a = W.noise((70, 70), np.uint8, 9)
    want = W.expected(a, idat=1)
    assert len(want.z) > 4096
    files, _ = encode(engine, [a], idat=1)
    assert files[0] == want.file


def test_the_filter_waves_stride_when_total_rows_understated_the_rows(engine):
    """total_rows sizes the grid alone: with 1 for 600 rows in 3 images every wave of the few that are launched takes many bands, and
    the files are the same; only the filters of rows behind total_rows are not reported"""
    arrays = [W.smooth((200, 33, 4), np.uint8, 2), W.smooth((300, 5), np.uint16, 3), W.noise((100, 40, 3), np.uint8, 4)]
    flat = torch.cat([dev(a).view(torch.uint8).reshape(-1) for a in arrays])
    shapes = [(a.shape[0], a.shape[1], a.shape[2] if a.ndim == 3 else 1, 8 * a.dtype.itemsize) for a in arrays]
    p = engine._png_plan(flat, shapes, "adaptive", 1 << 16, 1 << 16, 32, 10, None, 64, True)
    assert p.total_rows == 600
    p.total_rows = 1
    p.row_filter.fill_(77)
    engine._png_launch(p)
    off, ln = p.file_off.cpu().numpy(), p.file_len.cpu().numpy()
    host = p.out.cpu().numpy().tobytes()
    for k, a in enumerate(arrays):
        assert host[int(off[k]):int(off[k]) + int(ln[k])] == W.expected(a).file, k
    assert int(p.row_filter[0]) == W.expected(arrays[0]).filters[0]


def _mixed_batch(n, seed, widths=(1, 40), heights=(1, 20), failing=()):
    """n small images of every pair, widths and heights drawn from [lo, hi), every tenth one -- and those of `failing` -- failing in one
    of three ways -> (flat pixels, specs, [pixels or the status])"""
    from hdl_deflate_amd.png import SPEC_DTYPE
    rng = np.random.default_rng(seed)
    sp = np.zeros(n, SPEC_DTYPE)
    arrays, blobs, at = [], [], 0
    for k in range(n):
        colour, depth = W.PAIRS[int(rng.integers(0, 8))]
        w, h = int(rng.integers(*widths)), int(rng.integers(*heights))
        a = pixels(colour, depth, w, h, seed + k)
        sp[k] = (at, w, h, depth, colour, 0)
        blobs.append(a.tobytes())
        at += len(blobs[-1])
        arrays.append(a)
        if k % 10 == 3 or k in failing:
            bad = (k // 10) % 3
            if bad == 0:
                sp[k]["width"] = 0
            elif bad == 1:
                sp[k]["colour"] = 3
            else:
                sp[k]["pix_off"] = 1 << 40
            arrays[-1] = W.E_BAD_PARAM if bad == 2 else W.E_BAD_HEADER
    return dev(np.frombuffer(b"".join(blobs), np.uint8)), sp, arrays


def test_a_batch_of_mixed_images_some_of_them_failing(engine):
    from hdl_deflate_amd import HdlzStatusError
    flat, sp, arrays = _mixed_batch(300, 50)
    files, index = engine.encode_png(flat, sp, check=False)
    host = files.cpu().numpy().tobytes()
    at = 0
    for k, a in enumerate(arrays):
        r = index.host[k]
        if isinstance(a, int):
            assert (int(r["status"]), int(r["file_len"]), int(r["file_off"])) == (a, 0, at), k
            continue
        want = W.expected(a).file
        assert (int(r["status"]), int(r["file_off"]), int(r["file_len"])) == (W.OK, at, len(want)), k
        assert host[at:at + len(want)] == want, k
        at += len(want)
    rec = index.write_record
    assert (rec.status, rec.first_bad, rec.total_len) == (W.E_BAD_HEADER, 3, at) and len(host) == at      # the largest status, the lowest failed image
    with pytest.raises(HdlzStatusError) as e:
        engine.encode_png(flat, sp)
    assert e.value.first_bad == 3


def test_a_batch_of_2051_tiny_images_three_a_thread_of_the_planners(engine):
    """2051 images of 1 .. 5 x 1 .. 5 pixels in blocks of 32 bytes: k_pngw_plan and k_pngw_layout take the images three a thread (1024
    threads), k_pngw_scan the blocks -- more than 2048, asserted -- at least three a thread; failing specs every tenth image, on both
    sides of a wave seam (191 | 192 at three a thread) and at the very end; images under 5 stream bytes, which are stored, among them.
    (Of 2051 such images about 70 are under 5 bytes and a tenth fail, so it is the blocks that are counted, not the images of at
    least 5 bytes: the block size makes most images bring two or more.)"""
    from hdl_deflate_amd.chain import plan_blocks
    n, block = 2051, 32
    flat, sp, arrays = _mixed_batch(n, 70, widths=(1, 6), heights=(1, 6), failing=(191, 192, 2050))
    failed = np.array([isinstance(a, int) for a in arrays])
    raw_len = [0 if isinstance(a, int) else a.nbytes + a.shape[0] for a in arrays]      # the scanlines and a filter byte a row
    assert sum(len(plan_blocks(r, block)) for r in raw_len if r >= 5) > 2048 and sum(1 for r in raw_len if 0 < r < 5) >= 20
    files, index = engine.encode_png(flat, sp, block=block, check=False)
    host = files.cpu().numpy().tobytes()
    off, ln = index.host["file_off"].astype(np.int64), index.host["file_len"].astype(np.int64)
    assert (off == np.cumsum(ln) - ln).all() and (ln[failed] == 0).all() and len(host) == int(ln.sum())
    assert index.host["status"].tolist() == [a if isinstance(a, int) else W.OK for a in arrays]
    near = {k + j for k in np.nonzero(failed)[0] for j in (-1, 1)}
    for k, a in enumerate(arrays):
        if isinstance(a, int):
            continue
        f = host[int(off[k]):int(off[k]) + int(ln[k])]
        if k % 8 == 0 or k in near:
            assert f == W.expected(a, block=block).file, k
        rec = P.index([f])["images"][0]
        st, back = P.decode(f, rec)
        assert (st, rec["used"]) == (P.OK, len(f)) and back == a.tobytes(), (k, st)
    rec = index.write_record
    assert (rec.status, rec.first_bad, rec.total_len) == (max(a for a in arrays if isinstance(a, int)), 3, len(host))
    # the records are the index of the written files, byte for byte; of a refused image -- an empty file -- all but the reason
    again = engine.png_index(files, torch.from_numpy(off).cuda(), torch.from_numpy(ln).cuda(), out_align=64, expand=True)
    theirs = again.host.copy()
    assert (theirs["status"][failed] != W.OK).all()
    theirs["status"][failed] = index.host["status"][failed]
    assert theirs.tobytes() == index.host.tobytes(), [f for f in theirs.dtype.names if (theirs[f] != index.host[f]).any()]
    assert (again.record.total_z, again.record.total_raw, again.record.total_out) == (index.record.total_z, index.record.total_raw, index.record.total_out)


def test_the_sizing_call_and_a_capacity_one_byte_short_write_nothing(engine):
    arrays = [W.smooth((9, 20, 3), np.uint8, 4), W.noise((3, 3), np.uint16, 5)]
    flat = torch.cat([dev(a).view(torch.uint8).reshape(-1) for a in arrays])
    shapes = [(9, 20, 3, 8), (3, 3, 1, 16)]
    want = [W.expected(a).file for a in arrays]
    total = sum(map(len, want))
    for cap in (0, total - 1, total):
        out = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        files, index = engine.encode_png(flat, shapes, out=out[:cap], check=False)
        rec = index.write_record
        assert (rec.status, rec.total_len, rec.first_bad) == (W.OK if cap == total else W.E_OUT_CAPACITY, total, W.NONE64), cap
        assert [int(x) for x in index.host["file_len"]] == [len(w) for w in want] and [int(x) for x in index.host["file_off"]] == [0, len(want[0])]
        got = out.cpu().numpy()
        if cap == total:
            assert got[:total].tobytes() == b"".join(want) and (got[total:] == 0xA5).all()
        else:
            assert (got == 0xA5).all() and files.numel() == 0, cap


def test_the_records_are_the_index_of_the_written_files(engine):
    from hdl_deflate_amd.png import IMAGE_DTYPE
    arrays = [pixels(c, d, w, h, c + d + w) for (c, d), (w, h) in zip(W.PAIRS, ((1, 1), (5, 3), (67, 66), (2, 1), (300, 2), (17, 9), (64, 64), (3, 7)))]
    for expand, align in ((True, 64), (False, 1), (True, 256)):
        flat = torch.cat([dev(a).view(torch.uint8).reshape(-1) for a in arrays])
        shapes = [(a.shape[0], a.shape[1], a.shape[2] if a.ndim == 3 else 1, 8 * a.dtype.itemsize) for a in arrays]
        files, index = engine.encode_png(flat, shapes, idat=100, out_align=align, expand=expand)
        off = torch.from_numpy(index.host["file_off"].astype(np.int64)).cuda()
        ln = torch.from_numpy(index.host["file_len"].astype(np.int64)).cuda()
        again = engine.png_index(files, off, ln, out_align=align, expand=expand)
        assert again.host.tobytes() == index.host.tobytes(), [n for n in IMAGE_DTYPE.names if (again.host[n] != index.host[n]).any()]
        assert (again.record.total_z, again.record.total_raw, again.record.total_out) == (index.record.total_z, index.record.total_raw, index.record.total_out)
        assert index.shapes == again.shapes and index.dtypes == again.dtypes
        out, status = engine.decode_png(files, index)
        assert int((status != 0).sum()) == 0
        for k, a in enumerate(arrays):
            o = int(index.host["out_off"][k])
            want = a.tobytes() if expand else W.scanlines(a)[0]
            assert out[o:o + len(want)].cpu().numpy().tobytes() == want, (k, expand)


@pytest.mark.parametrize("colour,depth", W.PAIRS)
def test_load_png_reads_what_save_png_wrote(engine, colour, depth):
    import hdl_deflate_amd
    xs = [dev(pixels(colour, depth, w, h, 11 * w + h)) for w, h in ((1, 1), (67, 66), (300, 9))]
    files = hdl_deflate_amd.save_png(engine, xs)
    assert isinstance(files, list) and all(isinstance(f, bytes) for f in files)
    back = hdl_deflate_amd.load_png(engine, files)
    for x, y in zip(xs, back):
        assert y.dtype == x.dtype and tuple(y.shape) == tuple(x.shape) and torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    one = hdl_deflate_amd.save_png(engine, xs[1], filter="paeth", idat=50)
    assert one == W.expected(xs[1].cpu().numpy(), mode=4, idat=50).file
    if xs[0].dim() == 2:                                      # (H, W, 1) is grey
        assert hdl_deflate_amd.save_png(engine, xs[1].unsqueeze(2)) == files[1]


@pytest.mark.parametrize("colour,depth", W.PAIRS)
def test_pillow_reads_the_files(engine, colour, depth):
    Image = pytest.importorskip("PIL.Image")
    import hdl_deflate_amd
    pix = pixels(colour, depth, 67, 66, 5)
    im = Image.open(io.BytesIO(hdl_deflate_amd.save_png(engine, dev(pix), idat=1000)))
    im.load()
    if depth == 16 and colour != 0:
        got = np.asarray(im.convert({2: "RGB", 4: "LA", 6: "RGBA"}[colour]))
        assert got.shape == pix.shape and (got == (pix >> 8)).all()
    else:
        got = np.asarray(im)
        assert got.shape == pix.shape and (got.astype(pix.dtype) == pix).all()


def test_the_adaptive_file_of_the_ramp_is_below_half_of_the_unfiltered_one(engine):
    """derived, not measured: on the noise-free ramp Sub leaves one byte value a row, which a 32-byte window deflates to a match a
    token; unfiltered, a row's period of 256 bytes lies outside the window.  The rule gives 7570 against 51918 stream bytes"""
    import hdl_deflate_amd
    a = W.ramp()
    adaptive, plain = hdl_deflate_amd.save_png(engine, dev(a)), hdl_deflate_amd.save_png(engine, dev(a), filter=0)
    assert adaptive == W.expected(a).file and plain == W.expected(a, mode=0).file
    assert (len(W.expected(a).z), len(W.expected(a, mode=0).z)) == (7570, 51918)
    assert 2 * len(adaptive) < len(plain)


def test_the_three_calls_are_captured_into_one_graph(engine):
    """filter, compress and write on one stream, a linear chain: captured once, launched twice, the same bytes both times"""
    arrays = [W.smooth((66, 67, 3), np.uint8, 1), W.noise((3, 1), np.uint8, 2), W.smooth((20, 300, 4), np.uint16, 3)]
    flat = torch.cat([dev(a).view(torch.uint8).reshape(-1) for a in arrays])
    shapes = [(a.shape[0], a.shape[1], a.shape[2] if a.ndim == 3 else 1, 8 * a.dtype.itemsize) for a in arrays]
    want = b"".join(W.expected(a, block=4096, idat=777).file for a in arrays)
    p = engine._png_plan(flat, shapes, "adaptive", 4096, 777, 32, 10, None, 64, True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        engine._png_launch(p)                                 # (a first run outside the capture: modules loaded)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        engine._png_launch(p)
    got = []
    for _ in range(2):
        p.out.zero_()
        p.res.zero_()
        g.replay()
        torch.cuda.synchronize()
        total = int(p.res[0])
        got.append(p.out[:total].cpu().numpy().tobytes())
    assert got[0] == want and got[1] == want
