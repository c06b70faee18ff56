"""GPU (-m gpu): hdlz_png_index_ws and hdlz_png_decode_ws inside guard bands (tests/guards.py), in the manner of
tests/test_gpu_zip64_containment.py: every buffer of a call carved out of one patterned arena, each case run on the pattern and on its
complement.

  bands and read-only regions (the files and what stands around them, the two arrays of the index, the records the decode is given)
  untouched; the index writes d_images[0 .. min(n, image_cap)) and the record, the decode the slots of the images that passed its checks,
  d_image_status[0 .. count) and the record; d_work only inside what was passed; nothing at or behind out_cap;
  all results identical in both runs -- the runs differ in every byte around the files, in every byte outside the slots and in the
  initial content of every output and of the scratch, so none of those reaches a result, and a load outside the files would show in one
  of them -- and equal to the rule (png_ref)."""
import numpy as np
import pytest
import torch

import guards
import png_ref as P
import test_gpu_containment as C
import test_gpu_png as T

pytestmark = pytest.mark.gpu
BAND = 1 << 16


def _records(ix):
    from hdl_deflate_amd.png import IMAGE_DTYPE
    recs = np.zeros(len(ix["images"]), IMAGE_DTYPE)
    for k, r in enumerate(ix["images"]):
        for f in P.FIELDS:
            recs[f][k] = r[f]
    return recs


def _layout(files, gap, mis):
    """the files with `gap` bytes of the arena's pattern between them -> (offsets, the buffer's length)"""
    offs, at = [], mis
    for f in files:
        offs.append(at)
        at += len(f) + gap
    return offs, at


def index_call(engine, label, files, flags, out_align, cap, gap=0, mis=0):
    from hdl_deflate_amd.png import IMAGE_DTYPE
    L, n = engine.lib, len(files)
    offs, total = _layout(files, gap, mis)
    wb = L.hdlz_png_index_work_bytes(n, cap)
    specs = [("files", total, 16, BAND, True), ("off", 8 * n, 8, BAND, True), ("len", 8 * n, 8, BAND, True), ("images", 136 * cap, 8, BAND),
             ("result", 40, 8, BAND), ("work", wb, 8, C.WORK_BAND)]

    def setup(a):
        for f, o in zip(files, offs):
            a.fill("files", f, o)
        a.fill("off", np.array(offs, np.uint64).tobytes())
        a.fill("len", np.array([len(f) for f in files], np.uint64).tobytes())

    def call(a):
        rc = L.hdlz_png_index_ws(a.ptr("files"), total, a.ptr("off"), a.ptr("len"), n, flags, out_align, cap, a.ptr("images") if cap else None,
                                 a.ptr("result"), a.ptr("work"), wb, C.stream_ptr())
        assert rc == 0, (label, L.hdlz_last_error())

    a, clean, runs = C.two_runs(specs, setup, call, ("images", "result"))
    ix = P.index(files, flags, out_align, cap, offsets=offs, files_len=total)
    k = min(cap, n)
    for r in runs:
        res = np.frombuffer(r["result"].tobytes(), np.uint64)
        assert [int(x) for x in res[:4]] == [n, ix["total_z"], ix["total_raw"], ix["total_out"]] and int(res[4]) == ix["status"], (label, res)
        got = np.frombuffer(r["images"].tobytes(), IMAGE_DTYPE)[:k]
        assert [tuple(int(g[f]) for f in P.FIELDS) for g in got] == [tuple(rec[f] for f in P.FIELDS) for rec in ix["images"]], label
        assert not got["reserved"].any()
    bad = guards.violations(a, clean, {"images": 136 * k, "result": True, "work": True})
    assert bad == [], (label, bad)
    parts = a.split(clean)
    assert not bool(parts["images"][1][:136 * k].any()) and not bool(parts["result"][1].any()), (label, "not written")


def test_the_index_stays_inside_its_records(engine):
    small = [T.made(5 + k, 3 + k, *P.PAIRS[k % len(P.PAIRS)], k % 5, seed=k)[0] for k in range(7)]
    damaged = [c[1] for c in T._damaged()]
    index_call(engine, "seven, exact", small, P.EXPAND, 64, 7)
    index_call(engine, "seven, apart, at an odd address", small, P.RAW, 1, 7, gap=37, mis=3)
    index_call(engine, "seven, room for 12", small, P.EXPAND, 256, 12, gap=1)
    index_call(engine, "seven, room for 2", small, P.EXPAND, 16, 2, mis=1)
    index_call(engine, "the sizing call", small, P.EXPAND, 64, 0)
    index_call(engine, "every damaged file", damaged, P.EXPAND, 64, len(damaged), gap=5, mis=7)
    index_call(engine, "every damaged file, packed", damaged, P.RAW, 2, len(damaged))
    index_call(engine, "1500 images", (small + damaged[:6]) * 116, P.EXPAND, 64, 1500, mis=2)


def decode_call(engine, label, files, expect, flags, first, count, gap=0, mis=0, out_mis=0, slack=0, out_align=64):
    """one guarded hdlz_png_decode_ws over images [first, first + count) of the rule's own records"""
    L = engine.lib
    offs, flen = _layout(files, gap, mis)
    ix = P.index(files, flags, out_align, offsets=offs, files_len=flen)
    recs, im = _records(ix), ix["images"]
    last = im[first + count - 1]
    ok = last["status"] == P.OK
    base = im[first]["out_off"]
    total = last["out_off"] - base + (last["out_len"] if ok else 0)
    zb = last["z_off"] - im[first]["z_off"] + (P.r16(last["zlen"] + 8) if ok else 0)
    rb = last["raw_off"] - im[first]["raw_off"] + (P.r16(last["raw_len"]) if ok else 0)
    idat = sum(r["nidat"] for r in im[first:first + count])
    cap = total + slack
    wb = L.hdlz_png_decode_work_bytes(count, idat, zb, rb)
    specs = [("files", flen, 16, BAND, True), ("images", 136 * len(im), 8, BAND, True), ("out", cap, 64, max(BAND, 2 * cap), False, out_mis),
             ("status", 4 * count, 4, BAND), ("result", 24, 8, BAND), ("work", wb, 256, C.WORK_BAND)]

    def setup(a):
        for f, o in zip(files, offs):
            a.fill("files", f, o)
        a.fill("images", recs.tobytes())

    def call(a):
        rc = L.hdlz_png_decode_ws(a.ptr("files"), flen, a.ptr("images"), first, count, flags, idat, zb, rb, a.ptr("out") if cap else None, cap,
                                  a.ptr("status"), a.ptr("result"), a.ptr("work"), wb, C.stream_ptr())
        assert rc == 0, (label, L.hdlz_last_error())

    a, clean, runs = C.two_runs(specs, setup, call, ("out", "status", "result"))
    assert np.array_equal(runs[0]["status"], runs[1]["status"]) and np.array_equal(runs[0]["result"], runs[1]["result"]), (label, "depends on bytes the call was not given")
    may = torch.zeros(cap, dtype=torch.bool, device="cuda")
    for r in runs:
        st = r["status"].view(np.uint32)
        for k in range(count):
            rec, (want, data) = im[first + k], expect[first + k]
            o = rec["out_off"] - base
            assert st[k] == want, (label, first + k, int(st[k]), want)
            if want == P.OK:
                assert r["out"][o:o + rec["out_len"]].tobytes() == data, (label, first + k, "bytes")
            if rec["status"] == P.OK:                           # the image passed the checks: its slot may be written
                may[o:o + rec["out_len"]] = True
        res = np.frombuffer(r["result"].tobytes(), np.uint64)
        bad = [k for k in range(count) if expect[first + k][0] != P.OK]
        assert int(res[1]) == (bad[0] if bad else 2 ** 64 - 1) and int(res[0]) == (0 if bad else total) and int(res[2]) == (int(st[bad[0]]) if bad else 0), (label, res)
    found = guards.violations(a, clean, {"out": may, "status": True, "result": True, "work": True})
    assert found == [], (label, found)
    parts = a.split(clean)
    assert not bool(parts["status"][1].any()) and not bool(parts["result"][1].any()), (label, "not written")
    for k in range(count):                                      # an OK slot is written in full
        rec = im[first + k]
        if expect[first + k][0] == P.OK:
            assert not bool(parts["out"][1][rec["out_off"] - base:rec["out_off"] - base + rec["out_len"]].any()), (label, first + k, "slot not written")


def test_the_decode_stays_inside_the_slots(engine):
    """count >= 2 (a wave per image) and count == 1 (the one-stream route) -- every type, sound and damaged files, slots with gaps, a
    sub-range, an odd d_out, files apart at odd addresses, RAW and EXPAND, a large image on the whole-GPU path"""
    for flags in (P.EXPAND, P.RAW):
        made = [T.made(3 + 5 * k, 2 + 9 * k, *P.PAIRS[k % len(P.PAIRS)], [(r + k) % 5 for r in range(2 + 9 * k)], seed=k, flags=flags, idat=None if k % 2 else 9,
                       trns=bytes([3, 200]) if P.PAIRS[k % len(P.PAIRS)][0] == 3 else None) for k in range(15)]
        files, expect = [f for f, _ in made], [e for _, e in made]
        decode_call(engine, ("fifteen", flags), files, expect, flags, 0, 15, mis=3, out_mis=1 if flags == P.RAW else 0)
        decode_call(engine, ("fifteen, apart", flags), files, expect, flags, 0, 15, gap=11, mis=5, slack=100)
        decode_call(engine, ("a sub-range", flags), files, expect, flags, 4, 6, gap=2)
        decode_call(engine, ("packed slots", flags), files, expect, flags, 0, 15, out_align=1, out_mis=3)
        for e in (0, 7, 14):
            decode_call(engine, ("alone", e, flags), files, expect, flags, e, 1, mis=e)
    small = T.made(7, 5, 4, 8, 4, seed=6)
    files, expect = [small[0]], [small[1]]
    for label, f, want in T._damaged():
        files += [f, small[0]]
        expect += [P.decode(f, P.index([f])["images"][0]), small[1]]
    decode_call(engine, "the damaged files", files, expect, P.EXPAND, 0, len(files), gap=3, mis=1)
    for k in range(1, len(files), 2):
        decode_call(engine, ("a damaged file alone", k), files, expect, P.EXPAND, k, 1, mis=k % 7)
    big = T._noise()
    decode_call(engine, "a large image alone", [big[0]], [big[1]], P.EXPAND, 0, 1, mis=9)
    decode_call(engine, "a large image among small ones", [small[0], big[0], small[0]], [small[1], big[1], small[1]], P.EXPAND, 0, 3, gap=1)
