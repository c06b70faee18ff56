"""GPU (-m gpu): hdlz_tiff_index_ws and hdlz_tiff_decode_ws inside guard bands (tests/guards.py), in the manner of
tests/test_gpu_png_containment.py: every buffer of a call carved out of one patterned arena, each case run on the pattern and on its
complement.

  bands and read-only regions (the files and what stands around them, the arrays of the index, the records the decode is given)
  untouched; the index writes d_images[0 .. min(n, image_cap)) and the record, the decode the slots of the images that passed its checks,
  d_image_status[0 .. count) and the record; d_work only inside what the query sized; nothing at or behind out_cap;
  all results identical in both runs -- the runs differ in every byte around the files, in every byte outside the slots and in the
  initial content of every output and of the scratch, so none of those reaches a result, and a load outside the files would show in one
  of them -- and equal to the rule (tiff_ref);
  and index + decode captured into a graph and replayed."""
import numpy as np
import pytest
import torch

import guards
import tiff_ref as T
import test_gpu_containment as C
import test_gpu_tiff as G
from test_tiff_cpu import crafted

pytestmark = pytest.mark.gpu
BAND = 1 << 16


def _records(ix):
    from hdl_deflate_amd.tiff import IMAGE_DTYPE
    recs = np.zeros(len(ix["images"]), IMAGE_DTYPE)
    for k, r in enumerate(ix["images"]):
        for f in T.FIELDS:
            recs[f][k] = r[f]
    return recs


def _layout(files, gap, mis):
    offs, at = [], mis
    for f in files:
        offs.append(at)
        at += len(f) + gap
    return offs, at


def index_call(engine, label, files, out_align, cap, gap=0, mis=0, pages=None):
    from hdl_deflate_amd.tiff import IMAGE_DTYPE
    L, n = engine.lib, len(files)
    offs, total = _layout(files, gap, mis)
    wb = L.hdlz_tiff_index_work_bytes(n, cap)
    specs = [("files", total, 16, BAND, True), ("off", 8 * n, 8, BAND, True), ("len", 8 * n, 8, BAND, True), ("page", 4 * n, 4, BAND, True),
             ("images", 136 * cap, 8, BAND), ("result", 40, 8, BAND), ("work", wb, 8, C.WORK_BAND)]

    def setup(a):
        for f, o in zip(files, offs):
            a.fill("files", f, o)
        a.fill("off", np.array(offs, np.uint64).tobytes())
        a.fill("len", np.array([len(f) for f in files], np.uint64).tobytes())
        a.fill("page", np.array(pages if pages is not None else [0] * n, np.uint32).tobytes())

    def call(a):
        rc = L.hdlz_tiff_index_ws(a.ptr("files"), total, a.ptr("off"), a.ptr("len"), a.ptr("page") if pages is not None else None, n, out_align, cap,
                                  a.ptr("images") if cap else None, a.ptr("result"), a.ptr("work"), wb, C.stream_ptr())
        assert rc == 0, (label, L.hdlz_last_error())

    a, clean, runs = C.two_runs(specs, setup, call, ("images", "result"))
    ix = T.index(files, pages, out_align, cap, offsets=offs, files_len=total)
    k = min(cap, n)
    for r in runs:
        res = np.frombuffer(r["result"].tobytes(), np.uint64)
        assert [int(x) for x in res[:4]] == [n, ix["total_chunks"], ix["total_raw"], ix["total_out"]] and int(res[4]) == ix["status"], (label, res)
        got = np.frombuffer(r["images"].tobytes(), IMAGE_DTYPE)[:k]
        assert [tuple(int(g[f]) for f in T.FIELDS) for g in got] == [tuple(rec[f] for f in T.FIELDS) for rec in ix["images"]], label
        assert not got["reserved"].any()
    bad = guards.violations(a, clean, {"images": 136 * k, "result": True, "work": True})
    assert bad == [], (label, bad)
    parts = a.split(clean)
    assert not bool(parts["images"][1][:136 * k].any()) and not bool(parts["result"][1].any()), (label, "not written")


def _small(n=7):
    types = [(1, 8), (2, 16), (3, 32), (1, 64), (2, 8), (1, 16), (3, 64), (2, 32)]
    return [T.make_tiff([G.page(*types[k % 8], 1 + k % 4, 5 + 3 * k, 7 + 5 * k, k, predictor=3 if types[k % 8][0] == 3 and k % 4 == 2 else 1 + k % 2,
                                compression=(8, 1, 32946)[k % 3], pad=k % 2, **((dict(rps=3), dict(tile=(16, 16)), dict())[k % 3]))], big=bool(k % 2))
            for k in range(n)]


def test_the_index_stays_inside_its_records(engine):
    small = _small()
    damaged = [f for _, f, _ in crafted()]
    index_call(engine, "seven, exact", small, 64, 7)
    index_call(engine, "seven, apart, at an odd address", small, 1, 7, gap=37, mis=3)
    index_call(engine, "seven, room for 12", small, 256, 12, gap=1)
    index_call(engine, "seven, room for 2", small, 16, 2, mis=1)
    index_call(engine, "the sizing call", small, 64, 0)
    index_call(engine, "every crafted file", damaged, 64, len(damaged), gap=5, mis=7)
    index_call(engine, "every crafted file, packed", damaged, 2, len(damaged))
    stack = T.make_tiff([G.page(1, 8, 1, 4, 4, 1), G.page(1, 16, 3, 5, 6, 2, tile=(16, 16)), G.page(3, 32, 1, 3, 9, 3, predictor=3)], big=True)
    index_call(engine, "pages", [stack] * 6, 64, 6, gap=3, mis=1, pages=[0, 1, 2, 3, 70000, 1])
    index_call(engine, "1500 images", (small + damaged[:6]) * 116, 64, 1500, mis=2)


def decode_call(engine, label, files, first, count, gap=0, mis=0, out_mis=0, slack=0, out_align=64, short_chunks=0):
    """one guarded hdlz_tiff_decode_ws over images [first, first + count) of the rule's own records"""
    L = engine.lib
    offs, flen = _layout(files, gap, mis)
    ix = T.index(files, None, out_align, offsets=offs, files_len=flen)
    expect = [T.decode(f, rec) for f, rec in zip(files, ix["images"])]
    recs, im = _records(ix), ix["images"]
    last = im[first + count - 1]
    ok = last["status"] == T.OK
    base = im[first]["out_off"]
    total = last["out_off"] - base + (last["out_len"] if ok else 0)
    rb = last["raw_off"] - im[first]["raw_off"] + (T.raw16_of(last) if ok else 0)
    chunks = sum(r["nchunks"] for r in im[first:first + count]) - short_chunks
    cap = total + slack
    wb = L.hdlz_tiff_decode_work_bytes(count, chunks, rb)
    assert wb == T.decode_work_bytes(L, count, chunks, rb)
    specs = [("files", flen, 16, BAND, True), ("images", 136 * len(im), 8, BAND, True), ("out", cap, 64, max(BAND, 2 * cap), False, out_mis),
             ("status", 4 * count, 4, BAND), ("result", 24, 8, BAND), ("work", wb, 256, C.WORK_BAND)]

    def setup(a):
        for f, o in zip(files, offs):
            a.fill("files", f, o)
        a.fill("images", recs.tobytes())

    def call(a):
        rc = L.hdlz_tiff_decode_ws(a.ptr("files"), flen, a.ptr("images"), first, count, chunks, rb, a.ptr("out") if cap else None, cap,
                                   a.ptr("status"), a.ptr("result"), a.ptr("work"), wb, C.stream_ptr())
        assert rc == 0, (label, L.hdlz_last_error())

    a, clean, runs = C.two_runs(specs, setup, call, ("out", "status", "result"))
    assert np.array_equal(runs[0]["status"], runs[1]["status"]) and np.array_equal(runs[0]["result"], runs[1]["result"]), (label, "depends on bytes the call was not given")
    may = torch.zeros(cap, dtype=torch.bool, device="cuda")
    for r in runs:
        st = r["status"].view(np.uint32)
        fitted = 0
        for k in range(count):
            rec, (want, data) = im[first + k], expect[first + k]
            if short_chunks and rec["status"] == T.OK:          # the images whose chunks do not fit the list any more are refused
                fitted += rec["nchunks"]
                if fitted > chunks:
                    want, data = T.E_BAD_PARAM, None
            o = rec["out_off"] - base
            if want is T.DECODER:
                assert st[k] not in (T.OK, T.E_BAD_PARAM), (label, first + k, int(st[k]))
            else:
                assert st[k] == want, (label, first + k, int(st[k]), want)
            if want == T.OK:
                assert r["out"][o:o + rec["out_len"]].tobytes() == data, (label, first + k, "bytes")
            if rec["status"] == T.OK:                           # the image passed the checks: its slot may be written
                may[o:o + rec["out_len"]] = True
        res = np.frombuffer(r["result"].tobytes(), np.uint64)
        bad = [k for k in range(count) if st[k] != T.OK]
        assert int(res[1]) == (bad[0] if bad else 2 ** 64 - 1) and int(res[0]) == (0 if bad else total) and int(res[2]) == (int(st[bad[0]]) if bad else 0), (label, res)
    found = guards.violations(a, clean, {"out": may, "status": True, "result": True, "work": True})
    assert found == [], (label, found)
    parts = a.split(clean)
    assert not bool(parts["status"][1].any()) and not bool(parts["result"][1].any()), (label, "not written")
    for k in range(count):                                      # an OK slot is written in full
        rec = im[first + k]
        if runs[0]["status"].view(np.uint32)[k] == T.OK:
            assert not bool(parts["out"][1][rec["out_off"] - base:rec["out_off"] - base + rec["out_len"]].any()), (label, first + k, "slot not written")


def test_the_decode_stays_inside_the_slots(engine):
    """count >= 2 (a wave per chunk) and the one-chunk route -- every type, sound and damaged files, slots with gaps, a sub-range, an odd
    d_out, files apart at odd addresses, a chunk list too short, a large strip on the whole-GPU path"""
    files = _small(15)
    decode_call(engine, "fifteen", files, 0, 15, mis=3)
    decode_call(engine, "fifteen, apart", files, 0, 15, gap=11, mis=5, slack=100)
    decode_call(engine, "a sub-range", files, 4, 6, gap=2)
    decode_call(engine, "packed slots at an odd address", files, 0, 15, out_align=1, out_mis=3)
    decode_call(engine, "a chunk list three slots short", files, 0, 15, short_chunks=3)
    for e in (0, 7, 14):
        decode_call(engine, ("alone", e), files, e, 1, mis=e)
    geo = [T.make_tiff([dict(pg)], big=bool(k % 2)) for k, (_, pg) in enumerate(G._geometries())]
    decode_call(engine, "the geometries", geo, 0, len(geo), gap=1, mis=1, out_align=16, out_mis=5)
    small = files[3]
    mixed = [small]
    for _, f, _ in crafted():
        mixed += [f, small]
    decode_call(engine, "the crafted files", mixed, 0, len(mixed), gap=3, mis=1)
    pix = T.random_pixels(256, 256, 3, 1, 8, 77)
    pix[:, 128:] = pix[:, :128]
    big = T.make_tiff([dict(pix=pix, predictor=2)])
    decode_call(engine, "a large strip alone", [big], 0, 1, mis=9)
    decode_call(engine, "a large strip cut short, alone", [T.make_tiff([dict(pix=pix, predictor=2, damage=lambda k, d: d[:len(d) // 2])])], 0, 1, mis=2)
    decode_call(engine, "a large strip among small ones", [small, big, small], 0, 3, gap=1)


def test_index_and_decode_replay_from_a_graph(engine):
    """both calls captured on one stream and replayed: nothing is allocated, the host reads nothing in between, the results are the same"""
    from hdl_deflate_amd import _lib
    L = engine.lib
    files = _small(6)
    pix = T.random_pixels(256, 256, 3, 1, 8, 78)
    pix[:, 128:] = pix[:, :128]
    files.append(T.make_tiff([dict(pix=pix, predictor=2)]))
    ix = T.index(files)
    want = [T.decode(f, r)[1] for f, r in zip(files, ix["images"])]
    d, off, ln = G.staged(engine, files)
    n, total, big = 7, ix["total_out"], ix["images"][6]
    images = torch.zeros((n, 17), dtype=torch.int64, device="cuda")
    rec = torch.zeros(16, dtype=torch.int64, device="cuda")     # the three records
    iwork = torch.empty(L.hdlz_tiff_index_work_bytes(n, n), dtype=torch.uint8, device="cuda")
    out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    args6 = (big["chunk_off"], big["raw_off"])
    args1 = (1, T.raw16_of(big))
    w6 = torch.empty(L.hdlz_tiff_decode_work_bytes(6, *args6), dtype=torch.uint8, device="cuda")
    w1 = torch.empty(L.hdlz_tiff_decode_work_bytes(1, *args1), dtype=torch.uint8, device="cuda")

    def calls():
        s = torch.cuda.current_stream().cuda_stream
        assert L.hdlz_tiff_index_ws(d.data_ptr(), d.numel(), off.data_ptr(), ln.data_ptr(), None, n, 64, n, images.data_ptr(), rec.data_ptr(),
                                    iwork.data_ptr(), iwork.numel(), s) == 0
        assert L.hdlz_tiff_decode_ws(d.data_ptr(), d.numel(), images.data_ptr(), 0, 6, *args6, out.data_ptr(), big["out_off"], status.data_ptr(),
                                     rec[5:].data_ptr(), w6.data_ptr(), w6.numel(), s) == 0
        assert L.hdlz_tiff_decode_ws(d.data_ptr(), d.numel(), images.data_ptr(), 6, 1, *args1, out.data_ptr() + big["out_off"], big["out_len"],
                                     status[6:].data_ptr(), rec[8:].data_ptr(), w1.data_ptr(), w1.numel(), s) == 0
    calls()                                                      # eager once
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            calls()
    seen = []
    for k in range(2):
        images.fill_(-1 - k); rec.fill_(k); out.fill_(k); status.fill_(7); iwork.fill_(0x11 * k); w6.fill_(0x22 * k); w1.fill_(0x33 * k)
        g.replay()
        torch.cuda.synchronize()
        host = out.cpu().numpy().tobytes()
        slots = [host[r["out_off"]:r["out_off"] + r["out_len"]] for r in ix["images"]]
        seen.append((images.cpu().numpy().tobytes(), rec[:11].cpu().numpy().tobytes(), slots, status.cpu().numpy().tobytes()))
        r = _lib.TiffIndexResult.from_buffer_copy(rec[:5].cpu().numpy().tobytes())
        assert (r.status, r.nimages, r.total_out, r.total_chunks) == (T.OK, 7, total, ix["total_chunks"])
        assert [int(x) for x in status] == [0] * 7 and slots == want
        gaps = np.ones(total, bool)
        for r in ix["images"]:
            gaps[r["out_off"]:r["out_off"] + r["out_len"]] = False
        assert gaps.any() and (np.frombuffer(host, np.uint8)[gaps] == k).all()           # nothing outside the slots was written
    assert seen[0] == seen[1]
