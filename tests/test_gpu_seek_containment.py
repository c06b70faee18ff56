"""GPU (-m gpu): hdlz_seek_index_ws and hdlz_seek_read_ranges_ws inside guard bands (tests/guards.py), in the manner of
tests/test_gpu_zip64_containment.py: every buffer of a call carved out of one patterned arena, each case run on the pattern and on its
complement.

  bands and read-only regions (the file; for the read also the four arrays of the index and the ranges) untouched;
  the index call writes d_out inside its row (out_cap rounded down to 4) -- an OK stream exactly its bytes --, d_bit and d_pos
  [0 .. n], d_crc [0 .. n), d_win [0 .. 32768 n) when it holds the points and not a word of them when it does not, and the record;
  the read writes d_out[0 .. total_out) -- the pieces of OK ranges in full, nothing at or behind out_cap, no byte at all under
  HDLZ_E_OUT_CAPACITY --, d_range_off[0 .. R], d_range_status[0 .. R) and the record; d_work only inside what was passed;
  all results identical in both runs -- the runs differ in every byte behind the file, in the initial content of every output and of
  the scratch, so none of those reaches a result -- and equal to the reference (seek_ref)."""
import numpy as np
import pytest
import torch

import guards
import seek_ref as ref
import test_gpu_containment as C
from seek_ref import OK, E_OUT_CAPACITY, E_BAD_PARAM, E_BAD_CHECKSUM

pytestmark = pytest.mark.gpu
BAND = 1 << 16
WIN = 32768
FLAGS = {"zlib": 1, "gzip": 2}


def index_call(engine, label, z, container, span, P, out_cap, data, w, mis=0, want=OK, decoded=True):
    """w: the reference walk of the sound stream; decoded: the stream itself is sound and has room (want is then OK, or
    HDLZ_E_OUT_CAPACITY for too few points) -> (the route the record names, the points of that route's reference)"""
    L = engine.lib
    wb = L.hdlz_seek_index_work_bytes(len(z), FLAGS[container], out_cap, P)
    specs = [("file", len(z), 16, BAND, True, mis), ("out", out_cap, 4, max(BAND, 2 * out_cap)), ("bit", 8 * (P + 1), 8, BAND), ("pos", 8 * (P + 1), 8, BAND),
             ("crc", 4 * P, 4, BAND), ("win", WIN * P, 16, BAND), ("result", 40, 8, BAND), ("work", wb, 256, C.WORK_BAND)]

    def call(a):
        rc = L.hdlz_seek_index_ws(a.ptr("file"), len(z), FLAGS[container], span, a.ptr("out") if out_cap else None, out_cap,
                                  *[a.ptr(n) if P else None for n in ("bit", "pos", "crc", "win")], P, a.ptr("result"), a.ptr("work"), wb, C.stream_ptr())
        assert rc == 0, (label, L.hdlz_last_error())

    a, clean, runs = C.two_runs(specs, lambda a: a.fill("file", z), call, ("out", "bit", "pos", "crc", "win", "result"))
    written = want == OK
    route = int(np.frombuffer(runs[0]["result"].tobytes(), np.uint64)[4]) >> 32
    assert route in (1, 2), (label, route)
    ix = ref.route_index(w, span, route)
    n = len(ix.crc)
    for r in runs:
        res = np.frombuffer(r["result"].tobytes(), np.uint64)
        st = int(res[4]) & 0xFFFFFFFF
        assert st == want, (label, st)
        if want == OK:
            assert [int(x) for x in res[:4]] == [n, len(data), ix.bit[-1], ix.max_seg], (label, res)
            assert r["bit"].view(np.uint64)[:n + 1].tolist() == ix.bit and r["pos"].view(np.uint64)[:n + 1].tolist() == ix.pos, label
            assert r["crc"].view(np.uint32)[:n].tolist() == ix.crc and r["win"][:WIN * n].tobytes() == b"".join(ix.win), label
            assert r["out"][:len(data)].tobytes() == data, label
        elif decoded:
            assert want == E_OUT_CAPACITY and [int(x) for x in res[:4]] == [n, len(data), ix.bit[-1], 0], (label, res)
        else:
            assert [int(x) for x in res[:4]] == [0, 0, 0, 0], (label, res)
    assert np.array_equal(runs[0]["result"], runs[1]["result"]), (label, "depends on bytes the call was not given")
    row = out_cap & ~3
    allowed = {"out": len(data) if decoded else row, "result": True, "work": True}
    if written:
        allowed.update(bit=8 * (n + 1), pos=8 * (n + 1), crc=4 * n, win=WIN * n)
    bad = guards.violations(a, clean, allowed)
    assert bad == [], (label, bad)
    parts = a.split(clean)
    assert not bool(parts["result"][1].any()), (label, "record not written")
    if written:
        for name, k in (("bit", 8 * (n + 1)), ("pos", 8 * (n + 1)), ("crc", 4 * n), ("win", WIN * n), ("out", len(data))):
            assert not bool(parts[name][1][:k].any()), (label, name, "not written in full")
    return route, n


def test_the_index_call_stays_inside_its_arrays(engine):
    S = ref.streams()
    for name, span, extra, slack, mis in (("SYNC", 1024, 0, 0, 3), ("SYNC", 10000, 5, 64, 0), ("MEM1", 5000, 1, 4, 7), ("L0", 32768, 0, 0, 1),
                                          ("GZNAME", 1024, 2, 8, 5), ("ONE", 1024, 0, 0, 2), ("L9", 8192, 0, 3, 0)):
        container, z, data, spans = S[name]
        w = ref.walk(z, container)
        cap = ((len(data) + 3) & ~3) + slack
        route, n = index_call(engine, (name, span), z, container, span, len(w.boundaries), cap, data, w, mis=mis)
        index_call(engine, (name, span, "room for %d more" % extra), z, container, span, n + extra, cap, data, w, mis=mis)
    container, z, data, spans = S["SYNC"]
    w = ref.walk(z, container)
    cap = (len(data) + 3) & ~3
    route, n = index_call(engine, "room for every boundary", z, container, 1024, len(w.boundaries), cap, data, w)
    assert n > 2
    index_call(engine, "the sizing call", z, container, 1024, 0, cap, data, w, want=E_OUT_CAPACITY)
    index_call(engine, "one point short", z, container, 1024, n - 1, cap, data, w, mis=9, want=E_OUT_CAPACITY)
    bad = bytearray(z)
    bad[-1] ^= 1
    index_call(engine, "a damaged trailer", bytes(bad), container, 1024, n, cap, data, w, want=E_BAD_CHECKSUM, decoded=False)
    index_call(engine, "no room for the data", z, container, 1024, n, cap - 1000, data, w, want=E_OUT_CAPACITY, decoded=False)


def read_call(engine, label, z, ix, data, ranges, seg_cap=None, out_cap=None, task_cap=None, segment_status=None, mis=0, out_mis=0, slack=0):
    L = engine.lib
    n, R = len(ix.crc), len(ranges)
    seg_cap = ix.max_seg if seg_cap is None else seg_cap
    full = ref.expected(data, ix.pos, ranges, segment_status=segment_status)
    out_cap = full.total_out + slack if out_cap is None else out_cap
    task_cap = full.ntasks if task_cap is None else task_cap
    e = ref.expected(data, ix.pos, ranges, segment_status=segment_status, out_cap=out_cap, task_cap=task_cap)
    wb = L.hdlz_seek_ranges_work_bytes(R, task_cap, seg_cap, 0)
    specs = [("file", len(z), 16, BAND, True, mis), ("bit", 8 * (n + 1), 8, BAND, True), ("pos", 8 * (n + 1), 8, BAND, True), ("crc", 4 * n, 4, BAND, True),
             ("win", WIN * n, 16, BAND, True, 1), ("ranges", 16 * R, 8, BAND, True), ("out", out_cap, 16, max(BAND, 2 * out_cap), False, out_mis),
             ("range_off", 8 * (R + 1), 8, BAND), ("status", 4 * R, 4, BAND), ("result", 32, 8, BAND), ("work", wb, 256, C.WORK_BAND)]

    def setup(a):
        a.fill("file", z)
        a.fill("bit", np.array(ix.bit, np.uint64).tobytes())
        a.fill("pos", np.array(ix.pos, np.uint64).tobytes())
        a.fill("crc", np.array(ix.crc, np.uint32).tobytes())
        a.fill("win", b"".join(ix.win))
        a.fill("ranges", np.array(ranges, np.uint64).tobytes())

    def call(a):
        rc = L.hdlz_seek_read_ranges_ws(a.ptr("file"), len(z), a.ptr("bit"), a.ptr("pos"), a.ptr("crc"), a.ptr("win"), n, a.ptr("ranges"), R, 0, seg_cap,
                                        a.ptr("out") if out_cap else None, out_cap, a.ptr("range_off"), a.ptr("status"), task_cap, a.ptr("result"),
                                        a.ptr("work") if wb else None, wb, C.stream_ptr())
        assert rc == 0, (label, L.hdlz_last_error())

    a, clean, runs = C.two_runs(specs, setup, call, ("out", "range_off", "status", "result"))
    may = torch.zeros(out_cap, dtype=torch.bool, device="cuda")
    for r in runs:
        res = np.frombuffer(r["result"].tobytes(), np.uint64)
        assert [int(x) for x in res[:3]] == [e.total_out, e.ntasks, e.first_bad] and int(res[3]) == e.record_status, (label, res)
        assert r["range_off"].view(np.uint64).tolist() == e.range_off and r["status"].view(np.uint32).tolist() == e.status, label
        for k, piece in enumerate(e.pieces):
            if piece is not None and e.record_status != E_OUT_CAPACITY:
                assert r["out"][e.range_off[k]:e.range_off[k + 1]].tobytes() == piece, (label, k)
    for n_ in ("range_off", "status", "result"):
        assert np.array_equal(runs[0][n_], runs[1][n_]), (label, n_, "depends on bytes the call was not given")
    if e.record_status != E_OUT_CAPACITY:
        for k, st in enumerate(e.status):                       # a failed range may leave anything in its own piece, an OK one fills it
            may[e.range_off[k]:e.range_off[k + 1]] = True
    found = guards.violations(a, clean, {"out": may, "range_off": True, "status": True, "result": True, "work": True})
    assert found == [], (label, found)
    parts = a.split(clean)
    for name in ("range_off", "status", "result"):
        assert not bool(parts[name][1].any()), (label, name, "not written")
    if e.record_status != E_OUT_CAPACITY:
        for k, st in enumerate(e.status):
            if st == OK:
                assert not bool(parts["out"][1][e.range_off[k]:e.range_off[k + 1]].any()), (label, k, "piece not written")


def _ranges(pos, seed):
    rng = np.random.RandomState(seed)
    n, total = len(pos) - 1, pos[-1]
    rs = [(0, total), (0, 0), (total, total + 9), (7, 2), (total - 1, total + 1)]
    for k in rng.randint(0, n, size=8).tolist():
        p, q = pos[k], pos[k + 1]
        rs += [(p, q), (p + 1, q), (p, max(q - 1, p)), (max(p - 3, 0), min(q + 3, total)), ((p + q) // 2, (p + q) // 2 + 1), (p, pos[min(k + 3, n)])]
    return rs


def test_the_read_stays_inside_the_pieces(engine):
    S = ref.streams()
    for name, span, mis, out_mis, slack in (("SYNC", 1024, 3, 1, 0), ("MEM1", 5000, 0, 5, 100), ("L0", 32768, 1, 0, 0), ("GZNAME", 1024, 5, 7, 3), ("ONE", 1024, 2, 2, 0),
                                            ("FIXED", 2048, 7, 3, 0)):
        container, z, data, spans = S[name]
        ix = ref.index(ref.walk(z, container), span)
        read_call(engine, (name, span), z, ix, data, _ranges(ix.pos, span), mis=mis, out_mis=out_mis, slack=slack)
    container, z, data, spans = S["SYNC"]
    ix = ref.index(ref.walk(z, container), 1024)
    ranges = _ranges(ix.pos, 5)
    full = ref.expected(data, ix.pos, ranges)
    read_call(engine, "the sizing call", z, ix, data, ranges, out_cap=0, task_cap=0)
    read_call(engine, "one byte short", z, ix, data, ranges, out_cap=full.total_out - 1, out_mis=3)
    read_call(engine, "one task short", z, ix, data, ranges, task_cap=full.ntasks - 1)
    read_call(engine, "idle task slots", z, ix, data, ranges, task_cap=full.ntasks + 300, slack=17)
    # failed ranges keep to their own pieces
    k = 11
    crc = list(ix.crc)
    crc[k] ^= 0x80000000
    st = [OK] * len(ix.crc)
    st[k] = E_BAD_CHECKSUM
    rs = ranges + [(ix.pos[k], ix.pos[k + 1]), (ix.pos[k] - 1, ix.pos[k] + 1), (ix.pos[k - 2], ix.pos[k + 2])]
    read_call(engine, "a damaged CRC word", z, ix._replace(crc=crc), data, rs, segment_status=st, out_mis=1)
    seg = [ix.pos[j + 1] - ix.pos[j] for j in range(len(ix.crc))]
    cap = max(seg) - 1
    read_call(engine, "seg_cap below a segment", z, ix, data, rs, seg_cap=cap, segment_status=[OK if s <= cap else E_BAD_PARAM for s in seg])
    read_call(engine, "no ranges", z, ix, data, [])
