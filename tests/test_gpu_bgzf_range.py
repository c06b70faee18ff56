"""GPU (-m gpu): hdlz_bgzf_read_ranges_ws and Engine.read_bgzf (include/hdlz_bgzf_range.h) against bgzf_range_ref: the serial contract
in Python and slices of what a stock reader decodes.  File A: members of every block type and length, empty ones in front of, between
and behind the data; file B: 300 members of 64 bytes from this project's writer -- more tasks and more ranges than one workgroup of
the per-task and per-range kernels holds."""
import numpy as np
import pytest
import torch

import bgzf_ref
import bgzf_range_ref as ref
from bgzf_ref import OK, E_OUT_CAPACITY, E_BAD_PARAM, E_BAD_HEADER, E_BAD_CHECKSUM
from hdl_deflate_amd import _lib
from hdl_deflate_amd.errors import HdlzStatusError

pytestmark = pytest.mark.gpu

LEVELS = (0, 1, 6, 9)
NOBODY = ref.NOBODY


def dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype)).cuda()


def placed(n, phase, fill=0):
    """a uint8 device tensor of n bytes whose address is `phase` behind a multiple of 16"""
    raw = torch.full((n + 32,), fill, dtype=torch.uint8, device="cuda")
    skip = (phase - raw.data_ptr()) % 16
    return raw[skip:skip + n]


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


class File(object):
    """a BGZF file on the device with an index (default: the serial walk's)"""

    def __init__(self, f, index=None, phase=0):
        if index is None:
            w = bgzf_ref.walk(f)
            assert w.status == OK
            index = (w.off, w.out_off)
        self.f, self.off, self.out_off = f, list(index[0]), list(index[1])
        self.M = len(self.off) - 1
        self.d_file = placed(len(f), phase)
        self.d_file.copy_(dev(np.frombuffer(f, np.uint8)))
        self.d_off, self.d_out_off = dev(self.off, np.int64), dev(self.out_off, np.int64)


def words(ranges):
    return dev(np.array(ranges, dtype=np.uint64).reshape(-1, 2).view(np.int64))


class Got(object):
    pass


def read(L, F, ranges, flags=0, out_cap=0, task_cap=0, phase=0, fill=0xA5):
    """one call on fresh buffers filled with `fill` -> the record, range_off, the statuses, d_out (out_cap bytes)"""
    R = len(ranges)
    d_ranges = words(ranges) if R else None
    out = placed(out_cap, phase, fill)
    range_off = torch.full((R + 1,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((max(R, 1),), -1, dtype=torch.int32, device="cuda")
    result = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    wb = L.hdlz_bgzf_ranges_work_bytes(R, task_cap, flags)
    assert (wb == 0) == (R == 0)
    work = torch.full((max(wb, 1),), fill ^ 0x33, dtype=torch.uint8, device="cuda")
    rc = L.hdlz_bgzf_read_ranges_ws(F.d_file.data_ptr(), len(F.f), F.d_off.data_ptr(), F.d_out_off.data_ptr(), F.M,
                                    d_ranges.data_ptr() if R else None, R, flags, out.data_ptr() if out_cap else None, out_cap,
                                    range_off.data_ptr(), status.data_ptr(), task_cap, result.data_ptr(), work.data_ptr() if wb else None, wb,
                                    stream_ptr())
    assert rc == 0, L.hdlz_last_error()
    torch.cuda.synchronize()
    g = Got()
    g.rec = _lib.BgzfRangesResult.from_buffer_copy(result.cpu().numpy().tobytes())
    g.range_off, g.status, g.out = range_off.cpu().tolist(), status.cpu().tolist()[:R], out.cpu().numpy().tobytes()
    return g


def check(g, e, label=""):
    assert (g.rec.total_out, g.rec.ntasks, g.rec.first_bad, g.rec.status, g.rec.reserved) == \
        (e.total_out, e.ntasks, e.first_bad, e.record_status, 0), label
    assert g.range_off == e.range_off, label
    assert g.status == e.status, label
    if e.record_status == E_OUT_CAPACITY:
        return
    for r, piece in enumerate(e.pieces):
        if piece is not None:
            assert g.out[e.range_off[r]:e.range_off[r + 1]] == piece, (label, r)


def sized_read(L, F, ranges, flags=0, member_status=None, **kw):
    """the call with exactly the room the reference asks for, checked against it"""
    e = ref.expected(F.f, ranges, virtual=bool(flags & 1), index=(F.off, F.out_off), member_status=member_status)
    g = read(L, F, ranges, flags, out_cap=e.total_out, task_cap=e.ntasks, **kw)
    check(g, e)
    return g, e


@pytest.fixture(scope="module")
def files_a():
    return {level: ref.file_a(level) for level in LEVELS}


@pytest.fixture(scope="module")
def file_b(engine):
    """19200 bytes in blocks of 64: 300 members and the EOF member, by this project's writer"""
    data = bgzf_ref.data(19200, 77)
    f = engine.compress_bgzf(dev(np.frombuffer(data, np.uint8)), block=64).cpu().numpy().tobytes()
    w = bgzf_ref.walk(f)
    assert w.status == OK and w.nmembers == 301 and w.total_out == 19200
    return f, data


# ---- every edge, plain mode
@pytest.mark.parametrize("level", LEVELS)
def test_every_edge(engine, files_a, level):
    f, data = files_a[level]
    F = File(f)
    ranges = ref.edge_ranges(F.out_off, seed=level)
    assert len(ranges) <= 400
    g, e = sized_read(engine.lib, F, ranges)
    assert e.record_status == OK and set(e.status) == {OK}
    total = len(data)
    assert all(piece == data[min(x, total):min(y, total)] for piece, (x, y) in zip(e.pieces, ranges))      # (the reference itself)


def test_every_edge_of_300_members(engine, file_b):
    f, data = file_b
    F = File(f)
    ranges = ref.edge_ranges(F.out_off, seed=5, per_member=False)
    assert len(ranges) <= 400 and (0, len(data)) in ranges
    g, e = sized_read(engine.lib, F, ranges)
    assert e.ntasks > 600 and e.record_status == OK


# ---- virtual mode
def _virtual_batch(F, seed):
    """the edge ranges as virtual offsets, an alias picked for each end; both aliases of every boundary; the end of the file"""
    r = np.random.default_rng(seed)
    total = F.out_off[-1]

    def name(p):
        c = ref.aliases(F.off, F.out_off, p)
        return c[int(r.integers(len(c)))]
    plain = [(min(x, total), min(y, total)) for x, y in ref.edge_ranges(F.out_off, seed, limit=300) if x <= total]
    batch = [(name(x), name(y)) for x, y in plain]
    end = ref.virtual(F.off[F.M], 0)
    for b in range(F.M):
        isize = F.out_off[b + 1] - F.out_off[b]
        if isize <= 65535:                                              # (C[b], ISIZE) and (C[b + 1], 0): one position
            batch += [(ref.virtual(F.off[b], 0), ref.virtual(F.off[b], isize)), (ref.virtual(F.off[b], 0), ref.virtual(F.off[b + 1], 0)),
                      (ref.virtual(F.off[b], isize), end), (ref.virtual(F.off[b + 1], 0), end)]
    return batch + [(end, end), (ref.virtual(F.off[0], 0), end)]


@pytest.mark.parametrize("level", LEVELS)
def test_virtual_offsets(engine, files_a, level):
    f, data = files_a[level]
    F = File(f)
    batch = _virtual_batch(F, seed=10 + level)
    g, e = sized_read(engine.lib, F, batch, flags=ref.VIRTUAL)
    assert e.record_status == OK
    k = len(batch) - 4 * 2 - 2                                          # the two aliases of a boundary give the same bytes
    assert e.pieces[k] == e.pieces[k + 1] and e.pieces[-1] == data


def test_virtual_offsets_that_name_nothing(engine, files_a):
    f, data = files_a[6]
    F = File(f)
    end = ref.virtual(F.off[F.M], 0)
    good = _virtual_batch(F, seed=3)[:40]
    bad = [(ref.virtual(F.off[2] + 40, 0), end),                        # a coffset in the middle of a member
           (ref.virtual(F.off[0], 0), ref.virtual(F.off[3] - 1, 0)),
           (ref.virtual(F.off[2], 5001), end),                          # u > ISIZE
           (ref.virtual(F.off[0], 301), end),
           (ref.virtual(F.off[1], 1), end),                             # (an empty member holds u = 0 alone)
           (ref.virtual(F.off[0], 0), ref.virtual(F.off[F.M], 1)),      # (C[M], 1)
           (ref.virtual(F.off[F.M], 1), ref.virtual(F.off[F.M], 1)),
           (ref.virtual(F.off[4], 3), ref.virtual(F.off[2], 9)),        # p0 > p1
           (end, ref.virtual(F.off[0], 0)),
           (ref.virtual(F.off[F.M] + 28, 0), ref.virtual(F.off[F.M] + 28, 0))]       # the file's length is no member's offset
    batch = good[:7] + bad[:3] + good[7:20] + bad[3:8] + good[20:] + bad[8:]
    g, e = sized_read(engine.lib, F, batch, flags=ref.VIRTUAL)
    assert [st for st in e.status if st != OK] == [E_BAD_PARAM] * len(bad) and e.status.count(OK) == len(good)
    assert (e.record_status, e.first_bad) == (E_BAD_PARAM, 7)
    for r, st in enumerate(e.status):
        assert st == OK or e.range_off[r] == e.range_off[r + 1]


# ---- many ranges, and none
def test_many_single_bytes_and_an_empty_batch(engine, file_b):
    f, data = file_b
    F = File(f)
    pos = np.random.default_rng(9).integers(0, len(data), 600).tolist()
    g, e = sized_read(engine.lib, F, [(p, p + 1) for p in pos])
    assert (e.total_out, e.ntasks) == (600, 600) and g.out == bytes(data[p] for p in pos)
    for flags in (0, ref.VIRTUAL):
        g = read(engine.lib, F, [], flags)
        assert (g.rec.total_out, g.rec.ntasks, g.rec.first_bad, g.rec.status, g.rec.reserved) == (0, 0, NOBODY, OK, 0) and g.range_off == [0]
        g = read(engine.lib, F, [], flags, out_cap=16, task_cap=3)
        assert (g.rec.status, g.rec.first_bad) == (OK, NOBODY) and g.range_off == [0] and g.out == bytes([0xA5]) * 16


# ---- damage: statuses, not faults
def member_statuses(L, F):
    """what hdlz_bgzf_inflate_ws says about every member of the same file with the same index"""
    total = max(F.out_off[-1] - F.out_off[0], 0)
    out = torch.empty(max(total, 1), dtype=torch.uint8, device="cuda")
    status = torch.full((F.M,), -1, dtype=torch.int32, device="cuda")
    result = torch.empty(3, dtype=torch.int64, device="cuda")
    wb = L.hdlz_bgzf_inflate_work_bytes(F.M, 0)
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    rc = L.hdlz_bgzf_inflate_ws(F.d_file.data_ptr(), len(F.f), F.d_off.data_ptr(), F.d_out_off.data_ptr(), F.M, 0, out.data_ptr(), total,
                                status.data_ptr(), result.data_ptr(), work.data_ptr(), wb, stream_ptr())
    assert rc == 0, L.hdlz_last_error()
    torch.cuda.synchronize()
    return status.cpu().tolist()


def _damage_batch(F):
    o = F.out_off
    return ref.edge_ranges(o, seed=21, limit=120) + [(o[4] - 1, o[4]), (o[3], o[3] + 1), (o[3] + 100, o[3] + 200), (o[2], o[3]), (o[4], o[5])]


@pytest.mark.parametrize("kind", ["a bit of the deflate data", "the CRC word", "ISIZE and the index with it"])
def test_damage_in_member_3(engine, files_a, kind):
    f, data = files_a[6]
    w = bgzf_ref.walk(f)
    off, out_off = list(w.off), list(w.out_off)
    bad = bytearray(f)
    if kind == "a bit of the deflate data":
        bad[off[3] + 18 + 20000] ^= 0x10
    elif kind == "the CRC word":
        bad[off[4] - 8] ^= 0x01
    else:
        bad[off[4] - 4:off[4]] = (65281).to_bytes(4, "little")
        out_off = out_off[:4] + [x + 1 for x in out_off[4:]]
    F = File(bytes(bad), index=(off, out_off))
    ms = member_statuses(engine.lib, F)
    assert ms[3] != OK and [st for b, st in enumerate(ms) if b != 3] == [OK] * (F.M - 1)
    batch = _damage_batch(F)
    g, e = sized_read(engine.lib, F, batch, member_status=ms)
    touching = [r for r, (st, p0, p1, lo, hi) in enumerate(ref.resolve(off, out_off, batch)) if lo <= 3 < hi]
    assert len(touching) > 10 and [r for r, st in enumerate(e.status) if st != OK] == touching
    assert {g.status[r] for r in touching} == {ms[3]} and (g.rec.status, g.rec.first_bad) == (ms[3], touching[0])
    assert batch.index((out_off[4] - 1, out_off[4])) in touching        # the range that delivers member 3's last byte alone


def test_failed_tasks_beyond_the_first_workgroup(engine):
    """600 members under one range: its tasks span three workgroups of the per-task kernels, the failing ones sit in the second and the
    third; a second range in front of them is delivered"""
    f, parts = bgzf_ref.many_members()
    w = bgzf_ref.walk(f)
    F = File(bgzf_ref.with_crc_flipped(f, w.off, (300, 570)), index=(w.off, w.out_off))
    ms = member_statuses(engine.lib, F)
    assert [(b, st) for b, st in enumerate(ms) if st != OK] == [(300, E_BAD_CHECKSUM), (570, E_BAD_CHECKSUM)]
    ranges = [(0, w.total_out), (0, w.out_off[70])]
    g, e = sized_read(engine.lib, F, ranges, member_status=ms)
    assert e.ntasks == 600 + 70 and g.status == [ms[300], OK] and (g.rec.status, g.rec.first_bad) == (ms[300], 0)
    assert g.out[g.range_off[1]:g.range_off[2]] == b"".join(parts[:70])


def test_an_index_from_elsewhere_with_one_word_moved(engine, files_a):
    f, data = files_a[6]
    w = bgzf_ref.walk(f)
    off = list(w.off)
    off[3] += 1
    F = File(f, index=(off, w.out_off))
    ms = member_statuses(engine.lib, F)
    assert set(ms[2:4]) <= {E_BAD_PARAM, E_BAD_HEADER} and ms[:2] + ms[4:] == [OK] * (F.M - 2)
    batch = _damage_batch(F)
    e = ref.expected(f, batch, index=(w.off, w.out_off), member_status=ms)      # (the bytes of the sound ranges: by the true index)
    g = read(engine.lib, F, batch, out_cap=e.total_out, task_cap=e.ntasks)
    check(g, e)
    hit = [r for r, st in enumerate(g.status) if st != OK]
    assert hit and all(g.status[r] in (E_BAD_PARAM, E_BAD_HEADER) for r in hit) and g.status.count(OK) > 10


# ---- capacity
def test_capacity_one_short(engine, files_a):
    f, data = files_a[1]
    F = File(f)
    ranges = ref.edge_ranges(F.out_off, seed=2, limit=60) + [(5, 2)]
    full = ref.expected(f, ranges)
    for out_cap, task_cap in ((full.total_out - 1, full.ntasks), (full.total_out, full.ntasks - 1), (0, 0)):
        e = ref.expected(f, ranges, out_cap=out_cap, task_cap=task_cap)
        assert e.record_status == E_OUT_CAPACITY and e.status[-1] == E_BAD_PARAM and set(e.status[:-1]) == {E_OUT_CAPACITY}
        g = read(engine.lib, F, ranges, out_cap=out_cap, task_cap=task_cap, fill=0x5A)
        check(g, e)
        assert g.out == bytes([0x5A]) * out_cap                        # nothing decoded, d_out not written
        again = read(engine.lib, F, ranges, out_cap=g.rec.total_out, task_cap=g.rec.ntasks)      # the reported sizes are the ones to come back with
        check(again, full)
        assert (again.rec.status, again.rec.first_bad) == (E_BAD_PARAM, len(ranges) - 1)


# ---- alignment
@pytest.mark.parametrize("phase", [1, 15])
def test_file_and_output_at_any_address(engine, files_a, phase):
    f, data = files_a[9]
    F = File(f, phase=phase)
    assert F.d_file.data_ptr() % 16 == phase
    ranges = ref.edge_ranges(F.out_off, seed=phase, limit=100) + [(k, k + 40 + k) for k in range(1, 34)]      # heads and tails of every residue
    sized_read(engine.lib, F, ranges, phase=16 - phase)
    sized_read(engine.lib, F, ranges, phase=phase)


# ---- capture
def test_index_and_ranges_in_one_graph(engine, files_a):
    L = engine.lib
    f, data = files_a[6]
    n, w = len(f), bgzf_ref.walk(f)
    M = w.nmembers
    ranges = ref.edge_ranges(w.out_off, seed=4, limit=80)
    e = [ref.expected(f, ranges)]
    R, total, ntasks = len(ranges), e[0].total_out, e[0].ntasks
    d_file = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_ranges = words(ranges)
    off, ooff = torch.empty(M + 1, dtype=torch.int64, device="cuda"), torch.empty(M + 1, dtype=torch.int64, device="cuda")
    ires, rres = torch.empty(4, dtype=torch.int64, device="cuda"), torch.empty(4, dtype=torch.int64, device="cuda")
    iwb, rwb = L.hdlz_bgzf_index_work_bytes(n), L.hdlz_bgzf_ranges_work_bytes(R, ntasks, 0)
    iwork, rwork = torch.empty(iwb, dtype=torch.uint8, device="cuda"), torch.empty(rwb, dtype=torch.uint8, device="cuda")
    out = torch.empty(total, dtype=torch.uint8, device="cuda")
    range_off, status = torch.empty(R + 1, dtype=torch.int64, device="cuda"), torch.empty(R, dtype=torch.int32, device="cuda")

    def calls():
        s = stream_ptr()
        assert L.hdlz_bgzf_index_ws(d_file.data_ptr(), n, M, off.data_ptr(), ooff.data_ptr(), ires.data_ptr(), iwork.data_ptr(), iwb, s) == 0
        assert L.hdlz_bgzf_read_ranges_ws(d_file.data_ptr(), n, off.data_ptr(), ooff.data_ptr(), M, d_ranges.data_ptr(), R, 0, out.data_ptr(),
                                          total, range_off.data_ptr(), status.data_ptr(), ntasks, rres.data_ptr(), rwork.data_ptr(), rwb, s) == 0

    def fresh(k):
        for t in (out, iwork, rwork):
            t.fill_(0x3C + k)
        for t in (off, ooff, ires, rres, range_off, status):
            t.fill_(-2 - k)
        d_file.copy_(dev(np.frombuffer(f, np.uint8)))

    def answer():
        torch.cuda.synchronize()
        g = Got()
        g.rec = _lib.BgzfRangesResult.from_buffer_copy(rres.cpu().numpy().tobytes())
        g.range_off, g.status, g.out = range_off.cpu().tolist(), status.cpu().tolist(), out.cpu().numpy().tobytes()
        return g

    fresh(0)
    calls()
    plain = answer()
    check(plain, e[0], "eager")
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()                  # one linear stream, as the other _ws graph tests
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            calls()
    for launch in (1, 2):
        fresh(launch)
        g.replay()
        got = answer()
        check(got, e[0], ("graph", launch))
        assert off.cpu().tolist() == w.off and ooff.cpu().tolist() == w.out_off
        assert got.out == plain.out and got.range_off == plain.range_off and got.status == plain.status


# ---- Engine
def test_engine_read_bgzf(engine, files_a, file_b):
    f, data = files_a[6]
    F = File(f)
    total = len(data)
    ranges = [(0, 10), (299, 5301), (total - 3, total + 50), (70000, 70000), (0, total), (65500, 140000)]
    want = [data[x:y] for x, y in ranges]
    lens = np.cumsum([0] + [len(p) for p in want]).tolist()
    vr = [(ref.aliases(F.off, F.out_off, min(x, total))[0], ref.aliases(F.off, F.out_off, min(y, total))[-1]) for x, y in ranges]
    index = (F.d_off, F.d_out_off)
    for kw in ({}, {"index": index}):
        for rr, virtual in ((ranges, False), (words(ranges), False), (vr, True), (words(vr), True)):
            out, roff = engine.read_bgzf(F.d_file, rr, virtual=virtual, **kw)
            assert out.is_cuda and roff.is_cuda and roff.dtype == torch.int64
            assert roff.cpu().tolist() == lens and out.cpu().numpy().tobytes() == b"".join(want)
    # caller's buffers: one call, no sizing
    calls = []
    inner = engine._read_ranges
    engine._read_ranges = lambda *a: calls.append(a[6:8]) or inner(*a)
    try:
        buf = torch.empty(lens[-1] + 5, dtype=torch.uint8, device="cuda")
        out, roff = engine.read_bgzf(F.d_file, ranges, index=index, out=buf)
        assert len(calls) == 1 and out.data_ptr() == buf.data_ptr() and out.cpu().numpy().tobytes() == b"".join(want)
        with pytest.raises(ValueError):
            engine.read_bgzf(F.d_file, ranges, index=index, out=buf[:lens[-1] - 1])
        # groups: nine ranges, scratch for two at a time; the lowest failed range of all groups is named
        nine = [(k * 1000, k * 1000 + 70000) for k in range(9)]
        small = engine.lib.hdlz_bgzf_ranges_work_bytes(3, 6, 0)
        del calls[:]
        out, roff = engine.read_bgzf(F.d_file, nine, index=index, max_work_bytes=small)
        assert len(calls) >= 6 and out.cpu().numpy().tobytes() == b"".join(data[x:y] for x, y in nine)
        assert roff.cpu().tolist() == np.cumsum([0] + [len(data[x:y]) for x, y in nine]).tolist()
        nine[3], nine[7] = (9, 3), (8, 2)
        del calls[:]
        with pytest.raises(HdlzStatusError) as err:
            engine.read_bgzf(F.d_file, nine, index=index, max_work_bytes=small)
        assert err.value.status == E_BAD_PARAM and err.value.first_bad == 3 and len(calls) >= 3
    finally:
        engine._read_ranges = inner
    out, roff = engine.read_bgzf(F.d_file, [])
    assert out.numel() == 0 and roff.cpu().tolist() == [0]
    # a stopped index raises, as in inflate_bgzf
    with pytest.raises(HdlzStatusError) as err:
        engine.read_bgzf(dev(np.frombuffer(f[:-40], np.uint8)), [(0, 5)])
    assert err.value.first_bad == F.M - 2
    # host bytes in, host bytes out
    assert engine.read_bgzf_bytes(f, 250, 66000) == (OK, data[250:66000])
    assert engine.read_bgzf_bytes(f, total, total + 1) == (OK, b"") and engine.read_bgzf_bytes(f, 7, 3) == (E_BAD_PARAM, b"")
    broken = bytearray(f)
    broken[F.off[3] - 8] ^= 1                                           # member 2's CRC
    assert engine.read_bgzf_bytes(bytes(broken), 0, 100) == (OK, data[:100])
    assert engine.read_bgzf_bytes(bytes(broken), 0, 301)[0] == bgzf_ref.E_BAD_CHECKSUM
    # a file of this project's writer, read at ranges
    fb, db = file_b
    rb = [(int(a), int(a + n)) for a, n in zip(np.random.default_rng(1).integers(0, 19000, 50), np.random.default_rng(2).integers(0, 700, 50))]
    out, roff = engine.read_bgzf(dev(np.frombuffer(fb, np.uint8)), rb)
    assert out.cpu().numpy().tobytes() == b"".join(db[x:y] for x, y in rb)


def test_engine_read_bgzf_halves_groups_and_rebases_into_out(engine, file_b):
    """file B under a max_work_bytes that holds two ranges and a few tasks: a group of two ranges whose touched members do not fit
    is halved (every range of the first batch touches all 300 members), and with `out=` every group's piece lands behind the earlier
    ones -- also when a group's guess of its touched members does not hold"""
    fb, db = file_b
    d_file = dev(np.frombuffer(fb, np.uint8))
    query = engine.lib.hdlz_bgzf_ranges_work_bytes
    small = 8192 + 2 * (131072 + 256)                                    # groups of two ranges
    assert query(2, 4, 0) <= small < query(2, 600, 0) and query(1, 300, 0) <= small < query(3, 0, 0)
    calls = []
    inner = engine._read_ranges
    engine._read_ranges = lambda *a: calls.append((a[3].shape[0], a[6], a[7])) or inner(*a)       # ranges, out_cap, task_cap
    try:
        for out in (None, torch.empty(5 * 19200, dtype=torch.uint8, device="cuda")):
            # five ranges: (whole, whole) is halved, (46 members, 2 members) fits, the last range is a group of its own whose
            # 297 members are more than the guess behind `out` allows for
            five = [(0, 19200), (1, 19200), (64, 3000), (130, 194), (5, 19000)]
            want = [db[x:y] for x, y in five]
            del calls[:]
            got, roff = engine.read_bgzf(d_file, five, max_work_bytes=small, out=out)
            assert got.cpu().numpy().tobytes() == b"".join(want)
            assert roff.cpu().tolist() == np.cumsum([0] + [len(p) for p in want]).tolist()
            assert out is None or got.data_ptr() == out.data_ptr()
            sizes = [n for n, _, _ in calls]
            assert sizes[0] == 2 and sizes.count(1) >= 4 and sizes.count(2) >= 2, calls           # the first group was halved
            assert all(query(n, t, 0) <= small for n, _, t in calls), calls                       # no group's scratch exceeds the limit
        # `out=` with groups of two small ranges: one call per group, each piece behind the one before
        six = [(k * 3000 + 7, k * 3000 + 7 + 100 + k) for k in range(6)]
        out = torch.empty(2000, dtype=torch.uint8, device="cuda")
        del calls[:]
        got, roff = engine.read_bgzf(d_file, six, max_work_bytes=small, out=out)
        assert len(calls) == 3 and got.data_ptr() == out.data_ptr() and got.cpu().numpy().tobytes() == b"".join(db[x:y] for x, y in six)
        assert roff.cpu().tolist() == np.cumsum([0] + [100 + k for k in range(6)]).tolist()
        with pytest.raises(ValueError):
            engine.read_bgzf(d_file, six, max_work_bytes=small, out=out[:500])                    # the third group finds no room
    finally:
        engine._read_ranges = inner
