"""GPU (-m gpu): hdlz_png_filter_ws and hdlz_png_write_ws inside guard bands (tests/guards.py), in the manner of
tests/test_gpu_zip_write_containment.py: every buffer of a call carved out of one patterned arena, each case run on the pattern and on
its complement.  (The compress call between the two is hdlz_compress_batch_bits as it stands: tests/test_gpu_containment.py holds it.)

The filter is given exactly the pixel bytes; the writer's rows are the CPU oracle's (joined_ref.member_of), and of a row only the bytes
[2, d_len) are put into the arena, of the streams only those of images without blocks.  Everything else -- the bytes around the pixels,
78 9C of every row and what lies behind it up to the pitch, the streams of images that have blocks, the initial content of every
output and of the scratch -- is the pattern in one run and its complement in the other, so a result that is the rule's in both runs
depends on none of it.

  bands and read-only regions untouched; written: the streams of d_raw, d_row_filter[0 .. rows), d_status, d_raw_off; d_file[0 ..
  total_len) when it fits (no byte when it does not), d_file_off, d_file_len, d_image_status, d_images, the record; d_work only inside
  what was passed."""
import numpy as np
import pytest
import torch

import guards
import joined_ref as J
import png_ref as P
import png_write_ref as W
import test_gpu_containment as C

pytestmark = pytest.mark.gpu
BAND = 1 << 16


def _specs_of(arrays, gap=0):
    from hdl_deflate_amd.png import SPEC_DTYPE
    sp = np.zeros(len(arrays), SPEC_DTYPE)
    at, blobs = 0, []
    for k, a in enumerate(arrays):
        _, w, h, colour, depth = W.scanlines(a)
        sp[k] = (at, w, h, depth, colour, 0)
        blobs.append(a.tobytes())
        at += len(blobs[-1]) + gap
    return sp, blobs, at - gap if arrays else 0


def filter_call(engine, label, arrays, mode, mis=(0, 0), filters=True, short_rows=None):
    L = engine.lib
    n = len(arrays)
    sp, blobs, pix_len = _specs_of(arrays)
    want = [W.expected(a, mode=mode) for a in arrays]
    total = sum(len(w.stream) for w in want)
    rows = sum(a.shape[0] for a in arrays)
    told = rows if short_rows is None else short_rows
    wb = L.hdlz_png_filter_work_bytes(n)
    specs = [("pix", pix_len, 16, BAND, True, mis[0]), ("specs", 24 * n, 8, BAND, True), ("raw", total, 16, max(BAND, 2 * total), False, mis[1]),
             ("filters", told, 1, BAND), ("status", 4 * n, 4, BAND), ("raw_off", 8 * (n + 1), 8, BAND), ("work", wb, 8, C.WORK_BAND)]

    def setup(a):
        a.fill("pix", b"".join(blobs))
        a.fill("specs", sp.tobytes())

    def call(a):
        rc = L.hdlz_png_filter_ws(a.ptr("pix"), pix_len, a.ptr("specs"), n, mode, told, a.ptr("raw"), total, a.ptr("filters") if filters else None,
                                  a.ptr("status"), a.ptr("raw_off"), a.ptr("work"), wb, C.stream_ptr())
        assert rc == 0, (label, L.hdlz_last_error())

    a, clean, runs = C.two_runs(specs, setup, call, ("raw", "filters", "status", "raw_off"))
    offs = np.cumsum([0] + [len(w.stream) for w in want])
    for r in runs:
        assert not np.frombuffer(r["status"].tobytes(), np.uint32).any(), label
        assert np.frombuffer(r["raw_off"].tobytes(), np.uint64).tolist() == offs.tolist(), label
        assert r["raw"].tobytes() == b"".join(w.stream for w in want), label
        if filters:
            assert r["filters"].tolist() == sum((w.filters for w in want), [])[:told], label
    allowed = {"raw": True, "status": True, "raw_off": True, "work": True}
    if filters:
        allowed["filters"] = True
    bad = guards.violations(a, clean, allowed)
    assert bad == [], (label, bad)
    parts = a.split(clean)
    assert not bool(parts["raw"][1].any()) and not bool(parts["status"][1].any()) and not bool(parts["raw_off"][1].any()), (label, "an output byte was not written")
    if filters:
        assert not bool(parts["filters"][1].any()), (label, "a row's filter was not written")


def write_call(engine, label, arrays, mode=W.ADAPTIVE, block=64, idat=7, cap_delta=0, out_align=64, flags=1, mis=(0, 0, 0), records=True):
    from hdl_deflate_amd.chain import plan_blocks
    from hdl_deflate_amd.png import IMAGE_DTYPE
    L = engine.lib
    n = len(arrays)
    sp, _, _ = _specs_of(arrays)
    want = [W.expected(a, mode=mode, block=block, idat=idat) for a in arrays]
    raw_off, blk_first, in_off, rows = [0], [0], [0], []
    for w in want:
        if len(w.stream) >= 5:
            for o, ln in plan_blocks(len(w.stream), block):
                z, end_bit, _, _ = J.member_of(w.stream[o:o + ln], 32, 10)
                rows.append((z, end_bit))
                in_off.append(in_off[-1] + ln)
        raw_off.append(raw_off[-1] + len(w.stream))
        blk_first.append(len(rows))
    B = len(rows)
    pitch = max([len(z) for z, _ in rows] + [4]) + 5              # (no multiple of anything: rows at every alignment)
    total = sum(len(w.file) for w in want)
    cap = total + cap_delta
    wb = L.hdlz_png_write_work_bytes(n, B)
    words = lambda v: np.array(v, np.uint64).tobytes()
    specs = [("specs", 24 * n, 8, BAND, True), ("raw", raw_off[-1], 16, BAND, True, mis[0]), ("raw_off", 8 * (n + 1), 8, BAND, True),
             ("fstatus", 4 * n, 4, BAND, True), ("in_off", 8 * (B + 1), 8, BAND, True), ("rows", B * pitch, 16, BAND, True, mis[1]),
             ("len", 4 * B, 4, BAND, True), ("end_bits", 8 * B, 8, BAND, True), ("status", 4 * B, 4, BAND, True), ("blk_first", 8 * (n + 1), 8, BAND, True),
             ("file", cap, 16, max(BAND, 2 * cap), False, mis[2]), ("file_off", 8 * n, 8, BAND), ("file_len", 8 * n, 8, BAND), ("ist", 4 * n, 4, BAND),
             ("images", 136 * n, 8, BAND), ("result", 24, 8, BAND), ("work", wb, 8, C.WORK_BAND)]

    def setup(a):
        a.fill("specs", sp.tobytes())
        for k, w in enumerate(want):
            if len(w.stream) < 5:
                a.fill("raw", w.stream, raw_off[k])              # (the stream of an image that has blocks stays the pattern)
        for key, v in (("raw_off", raw_off), ("in_off", in_off), ("blk_first", blk_first), ("end_bits", [r[1] for r in rows])):
            a.fill(key, words(v))
        a.fill("fstatus", bytes(4 * n))
        a.fill("len", np.array([len(r[0]) for r in rows], np.uint32).tobytes())
        a.fill("status", bytes(4 * B))
        image = a.view("rows").cpu().numpy().copy()              # the pattern, put back in ONE copy with the rows' bytes in it
        for b, (z, _) in enumerate(rows):
            image[b * pitch + 2:b * pitch + len(z)] = np.frombuffer(z[2:], np.uint8)      # (78 9C stays the pattern)
        a.fill("rows", image)

    def call(a):
        rc = L.hdlz_png_write_ws(a.ptr("specs"), n, a.ptr("raw"), a.ptr("raw_off"), a.ptr("fstatus"), a.ptr("in_off") if B else None,
                                 a.ptr("rows") if B else None, pitch, a.ptr("len") if B else None, a.ptr("end_bits") if B else None,
                                 a.ptr("status") if B else None, B, a.ptr("blk_first"), idat, flags, out_align, a.ptr("file") if cap else None, cap,
                                 a.ptr("file_off"), a.ptr("file_len"), a.ptr("ist"), a.ptr("images") if records else None, a.ptr("result"), a.ptr("work"),
                                 wb, C.stream_ptr())
        assert rc == 0, (label, L.hdlz_last_error())

    a, clean, runs = C.two_runs(specs, setup, call, ("file", "file_off", "file_len", "ist", "images", "result"))
    fits = cap >= total
    ix = P.index([w.file for w in want], flags, out_align)
    for r in runs:
        res = np.frombuffer(r["result"].tobytes(), np.uint64)
        st = np.frombuffer(r["result"].tobytes(), np.uint32)[4:]
        assert (int(res[0]), int(res[1]), int(st[0]), int(st[1])) == (total, W.NONE64, W.OK if fits else W.E_OUT_CAPACITY, 0), (label, res, st)
        assert np.frombuffer(r["file_len"].tobytes(), np.uint64).tolist() == [len(w.file) for w in want], label
        assert np.frombuffer(r["file_off"].tobytes(), np.uint64).tolist() == np.cumsum([0] + [len(w.file) for w in want])[:-1].tolist(), label
        assert not np.frombuffer(r["ist"].tobytes(), np.uint32).any(), label
        if fits:
            assert r["file"][:total].tobytes() == b"".join(w.file for w in want), (label, "the files")
        if records:
            got = np.frombuffer(r["images"].tobytes(), IMAGE_DTYPE)
            assert [tuple(int(g[f]) for f in P.FIELDS) for g in got] == [tuple(rec[f] for f in P.FIELDS) for rec in ix["images"]] and not got["reserved"].any(), label
    allowed = {"file_off": True, "file_len": True, "ist": True, "result": True, "work": True}
    if fits:
        allowed["file"] = total
    if records:
        allowed["images"] = True
    bad = guards.violations(a, clean, allowed)
    assert bad == [], (label, bad)
    parts = a.split(clean)
    assert not bool(parts["result"][1].any()) and not bool(parts["file_off"][1].any()) and not bool(parts["file_len"][1].any()), (label, "an output was not written")
    if fits:
        assert not bool(parts["file"][1][:total].any()), (label, "a byte of the files was not written")
    if records:
        assert not bool(parts["images"][1].any()), (label, "a record was not written")


def _mix():
    K = W.kernel_constants()
    return [W.noise((1, 1), np.uint8, 1), W.smooth((3, 5, 3), np.uint8, 2), W.smooth((K.BAND + 1, 3, 4), np.uint16, 3), W.noise((2, 1), np.uint8, 4),
            W.smooth((2, 17), np.uint8, 5), W.noise((3, 1, 2), np.uint8, 6), W.smooth((K.BAND, 23, 2), np.uint16, 7), W.smooth((1, 40, 3), np.uint16, 8)]


def test_the_filter_stays_inside_its_streams(engine):
    """rows that start at every alignment of d_raw, pixels at odd addresses; every mode"""
    K = W.kernel_constants()
    for mode in (0, 1, 2, 3, 4, W.ADAPTIVE):
        filter_call(engine, ("mix", mode), _mix(), mode, mis=(3 + mode, 5))
    for mis in ((0, 0), (1, 15), (15, 1), (8, 7)):
        filter_call(engine, ("mix", mis), _mix(), W.ADAPTIVE, mis=mis)
    wide = [W.smooth((3, K.STEP + 1), np.uint8, 1), W.smooth((2, K.ROW_REG_MAX // 6 + 1, 3), np.uint16, 2), W.noise((K.BAND + 1, K.STEP - 1), np.uint8, 3)]
    filter_call(engine, "rows past the wave step and the register row", wide, W.ADAPTIVE, mis=(7, 9))
    filter_call(engine, "the same, a fixed filter, no filters reported", wide, 4, mis=(1, 2), filters=False)
    filter_call(engine, "total_rows understated: the waves stride", _mix() * 4, W.ADAPTIVE, mis=(2, 3), short_rows=5)


def test_the_writer_stays_inside_the_files(engine):
    """members that straddle chunk seams, images without blocks between images that have some; every buffer of bytes at an odd address"""
    write_call(engine, "mix", _mix(), mis=(3, 5, 7))
    write_call(engine, "mix, room behind the files, RAW records", _mix(), cap_delta=100, out_align=1, flags=0, mis=(1, 0, 2))
    write_call(engine, "mix, no records, idat 1", _mix(), idat=1, records=False, mis=(0, 15, 1))
    write_call(engine, "mix, one chunk each", _mix(), idat=1 << 16, block=1 << 16, mis=(11, 1, 13))
    write_call(engine, "only images without blocks", [W.noise((1, 1), np.uint8, 1), W.noise((1, 1), np.uint16, 2), W.noise((1, 1, 3), np.uint8, 3)], mis=(5, 0, 9))
    for mis in (0, 1, 7, 8, 15):
        write_call(engine, ("files at every residue", mis), _mix()[1:4], mis=(mis, 15 - mis, mis))


def test_files_that_do_not_fit_are_not_begun(engine):
    total = sum(len(W.expected(a, block=64, idat=7).file) for a in _mix())
    for delta in (-1, -45, -total):
        write_call(engine, ("mix", delta), _mix(), cap_delta=delta, mis=(3, 1, 4))
