"""GPU (-m gpu): hdlz_seek_index_ws and hdlz_seek_read_ranges_ws (include/hdlz_seek.h) and their Engine methods against seek_ref: the
inflate walker's block boundaries, the point rule, windows, CRC-32 words and slices of what stock zlib decodes.  The streams are
seek_ref.streams() -- zlib at levels 0, 1, 6, 9, Z_FIXED, memLevel 1 and with sync flushes, both containers, gzip with FEXTRA and FNAME;
tests/test_seek_cabi.py asserts that their reference indexes reach every edge these tests rest on -- and crafted seams from
tests/deflate_craft.py, where the first token behind a point is a match into the window.
Both routes state their set S of boundaries (seek_ref.route_index: the wave route every block boundary, the chain route the first
header and the dynamic headers), so every index must equal the reference of the route the record names exactly; the invariants any
route must satisfy are asserted as well, on a stream above the gate of the whole-GPU chains that the chain route delivers."""
import zlib

import numpy as np
import pytest
import torch

import deflate_craft as craft
import seek_ref as ref
from seek_ref import OK, E_OUT_CAPACITY, E_BAD_DISTANCE, E_NO_EOF, E_BAD_PARAM, E_BAD_CHECKSUM
from hdl_deflate_amd import _lib, seek
from hdl_deflate_amd.errors import HdlzStatusError

pytestmark = pytest.mark.gpu

WIN = 32768
ROUTE_CHAIN, ROUTE_WAVE = 1, 2
FLAGS = {"zlib": _lib.SEEK_ZLIB, "gzip": _lib.SEEK_GZIP}


def dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype)).cuda()


def dev_bytes(b):
    return dev(np.frombuffer(bytes(b), np.uint8)) if len(b) else torch.empty(0, dtype=torch.uint8, device="cuda")


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def words(ranges):
    return dev(np.array(ranges, dtype=np.uint64).reshape(-1, 2).view(np.int64))


class Got(object):
    pass


def index_call(L, z, container, span, point_cap, out_cap, fill=0xA5):
    """one hdlz_seek_index_ws on fresh buffers filled with `fill` -> the record, the four arrays (point_cap long) and d_out"""
    n, P = len(z), point_cap
    d_file = dev_bytes(z)
    out = torch.full((max(out_cap, 1),), fill, dtype=torch.uint8, device="cuda")
    bit = torch.full((P + 1,), -1, dtype=torch.int64, device="cuda")
    pos = torch.full((P + 1,), -1, dtype=torch.int64, device="cuda")
    crc = torch.full((max(P, 1),), -1, dtype=torch.int32, device="cuda")
    win = torch.full((max(P, 1), WIN), fill, dtype=torch.uint8, device="cuda")
    result = torch.full((5,), -1, dtype=torch.int64, device="cuda")
    wb = L.hdlz_seek_index_work_bytes(n, FLAGS[container], out_cap, P)
    assert wb >= 768
    work = torch.full((wb,), fill ^ 0x33, dtype=torch.uint8, device="cuda")
    rc = L.hdlz_seek_index_ws(d_file.data_ptr() if n else None, n, FLAGS[container], span, out.data_ptr() if out_cap else None, out_cap,
                              *[t.data_ptr() if P else None for t in (bit, pos, crc, win)], P, result.data_ptr(), work.data_ptr(), wb, stream_ptr())
    assert rc == 0, L.hdlz_last_error()
    torch.cuda.synchronize()
    g = Got()
    g.rec = _lib.SeekResult.from_buffer_copy(result.cpu().numpy().tobytes())
    g.bit, g.pos = bit.cpu().numpy().view(np.uint64).tolist(), pos.cpu().numpy().view(np.uint64).tolist()
    g.crc, g.win, g.out = crc.cpu().numpy().view(np.uint32).tolist(), win.cpu().numpy(), out.cpu().numpy().tobytes()
    g.d = (bit, pos, crc, win, d_file)
    return g


def check_index(g, w, span, data, label="", route=None):
    """the index of the call against the reference of the route its record names (route: the one it must name) -> that reference"""
    r = g.rec
    assert r.route in (ROUTE_CHAIN, ROUTE_WAVE) and route in (None, r.route), (label, r.route)
    ix = ref.route_index(w, span, r.route)
    n = len(ix.crc)
    assert (r.npoints, r.total_out, r.end_bit, r.max_seg, r.status) == (n, len(data), ix.bit[-1], ix.max_seg, OK), label
    assert g.bit[:n + 1] == ix.bit and g.pos[:n + 1] == ix.pos, label
    assert g.crc[:n] == ix.crc, label
    for k in range(n):
        assert g.win[k].tobytes() == ix.win[k], (label, k)
    assert g.out[:len(data)] == data, label
    return ix


class DevIndex(object):
    """a reference index on the device (any word may be damaged first)"""

    def __init__(self, z, ix):
        self.z, self.n = z, len(ix.crc)
        self.d_file = dev_bytes(z)
        self.bit, self.pos = dev(np.array(ix.bit, np.uint64).view(np.int64)), dev(np.array(ix.pos, np.uint64).view(np.int64))
        self.crc = dev(np.array(ix.crc, np.uint32).view(np.int32))
        self.win = dev(np.frombuffer(b"".join(ix.win), np.uint8).reshape(self.n, WIN))
        self.max_seg = ix.max_seg


def read(L, D, ranges, seg_cap=None, out_cap=0, task_cap=0, fill=0xA5):
    """one hdlz_seek_read_ranges_ws on fresh buffers filled with `fill` -> the record, range_off, the statuses, d_out"""
    R = len(ranges)
    seg_cap = D.max_seg if seg_cap is None else seg_cap
    d_ranges = words(ranges) if R else None
    out = torch.full((max(out_cap, 1),), fill, dtype=torch.uint8, device="cuda")
    range_off = torch.full((R + 1,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((max(R, 1),), -1, dtype=torch.int32, device="cuda")
    result = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    wb = L.hdlz_seek_ranges_work_bytes(R, task_cap, seg_cap, 0)
    assert (wb == 0) == (R == 0)
    work = torch.full((max(wb, 1),), fill ^ 0x33, dtype=torch.uint8, device="cuda")
    rc = L.hdlz_seek_read_ranges_ws(D.d_file.data_ptr(), len(D.z), D.bit.data_ptr(), D.pos.data_ptr(), D.crc.data_ptr(), D.win.data_ptr(), D.n,
                                    d_ranges.data_ptr() if R else None, R, 0, seg_cap, out.data_ptr() if out_cap else None, out_cap,
                                    range_off.data_ptr(), status.data_ptr(), task_cap, result.data_ptr(), work.data_ptr() if wb else None, wb,
                                    stream_ptr())
    assert rc == 0, L.hdlz_last_error()
    torch.cuda.synchronize()
    g = Got()
    g.rec = _lib.SeekRangesResult.from_buffer_copy(result.cpu().numpy().tobytes())
    g.range_off, g.status, g.out = range_off.cpu().tolist(), status.cpu().tolist()[:R], out.cpu().numpy().tobytes()
    return g


def check(g, e, label="", fill=0xA5):
    assert (g.rec.total_out, g.rec.ntasks, g.rec.first_bad, g.rec.status, g.rec.reserved) == \
        (e.total_out, e.ntasks, e.first_bad, e.record_status, 0), label
    assert g.range_off == e.range_off, label
    assert g.status == e.status, label
    if e.record_status == E_OUT_CAPACITY:
        assert set(g.out) <= {fill}, label                       # nothing decoded, d_out not written
        return
    for r, piece in enumerate(e.pieces):
        if piece is not None:
            assert g.out[e.range_off[r]:e.range_off[r + 1]] == piece, (label, r)


def sized_read(L, D, data, pos, ranges, segment_status=None, **kw):
    """the call with exactly the room the reference asks for, checked against it"""
    e = ref.expected(data, pos, ranges, segment_status=segment_status)
    g = read(L, D, ranges, out_cap=e.total_out, task_cap=e.ntasks, **kw)
    check(g, e)
    return g, e


def edge_ranges(pos, seed, limit=150):
    """empty, whole file, inside one segment, ending exactly at a point, crossing several points, overlapping and repeated, in
    descending order, past the end (short), x > y"""
    rng = np.random.RandomState(seed)
    n, total = len(pos) - 1, pos[-1]
    rs = [(0, 0), (0, total), (0, total + 100), (total, total + 5), (total + 7, total + 9), (5, 3), (total, 0), (total - 1, total), (0, 1)]
    ks = sorted(set([0, 1, n - 1, n] + rng.randint(0, n + 1, size=12).tolist()))
    for k in ks:
        p = pos[k]
        lo, hi = pos[max(k - 1, 0)], pos[min(k + 1, n)]
        rs += [(p, p), (max(p - 1, 0), p), (p, min(p + 1, total)), (max(p - 1, 0), min(p + 1, total)), (lo, p), (p, hi), (min(lo + 1, p), max(hi - 1, p))]
        rs += [(p, pos[min(k + 3, n)]), (max(p - 7, 0), min(pos[min(k + 4, n)] + 9, total))]
        if hi - p > 40:
            rs += [(p + 17, p + 31)] * 2                          # inside one segment, twice
    rs = [r for r in dict.fromkeys(rs)][:limit - 8] + rs[9:13] + sorted(rs[13:17], reverse=True)      # repeats; a descending run
    return rs


@pytest.fixture(scope="module")
def streams():
    return ref.streams()


STREAMS = ("L1", "L6", "L9", "FIXED", "L0", "MEM1", "SYNC", "ONE", "GZ6", "GZNAME")
# who fills the points: the chain for any block types delivers what zlib writes by default; a stream below the chains' gate (ONE) and
# one that starts with a fixed block (FIXED: the other chain's, or nobody's) are the recording wave's
ROUTES = {"L1": ROUTE_CHAIN, "L6": ROUTE_CHAIN, "L9": ROUTE_CHAIN, "GZ6": ROUTE_CHAIN, "FIXED": ROUTE_WAVE, "ONE": ROUTE_WAVE,
          "L0": None, "MEM1": None, "SYNC": None, "GZNAME": None}


# ---- the index call
@pytest.mark.parametrize("name", STREAMS)
def test_the_index_is_the_reference(engine, streams, name):
    container, z, data, spans = streams[name]
    w = ref.walk(z, container)
    d_z = dev_bytes(z)
    pitch = (len(data) + 3) & ~3
    if container == "zlib":
        out, out_len, status, used, _ = engine.inflate_checked(d_z.reshape(1, -1), out_pitch=pitch)
    else:
        out, out_len, status, used, _ = engine.inflate_gzip(d_z.reshape(1, -1), out_pitch=pitch)
    assert status.cpu().tolist() == [OK] and out_len.cpu().tolist() == [len(data)]
    for span in spans:
        g = index_call(engine.lib, z, container, span, len(ref.index(w, span).crc), pitch)
        ix = check_index(g, w, span, data, (name, span), ROUTES[name])
        assert g.out[:len(data)] == out.cpu().numpy().tobytes()[:len(data)]              # the bytes of the one-stream call
        g = index_call(engine.lib, z, container, span, len(ix.crc), pitch)               # exactly the room of the route's points
        check_index(g, w, span, data, (name, span, "exact"), ROUTES[name])
    # room for more points than there are: the words behind them stay as they were
    g = index_call(engine.lib, z, container, spans[0], len(ref.index(w, spans[0]).crc) + 3, pitch + 8)
    ix = check_index(g, w, spans[0], data, name)
    n = len(ix.crc)
    g.bit, g.pos, g.crc, g.win = g.bit[:n + 4], g.pos[:n + 4], g.crc[:n + 3], g.win[:n + 3]
    assert g.bit[n + 1:] == [(1 << 64) - 1] * 3 and g.pos[n + 1:] == [(1 << 64) - 1] * 3 and g.crc[n:] == [(1 << 32) - 1] * 3
    assert set(g.win[n:].tobytes()) == {0xA5} and set(g.out[len(data):]) == {0xA5}


def test_point_cap_too_small_is_the_sizing_call(engine, streams):
    container, z, data, spans = streams["SYNC"]
    w = ref.walk(z, container)
    first = index_call(engine.lib, z, container, 1024, len(w.boundaries), len(data))
    ix = check_index(first, w, 1024, data)
    n = len(ix.crc)
    assert n > 4
    for P in (0, 1, n - 1):
        g = index_call(engine.lib, z, container, 1024, P, len(data))
        r = g.rec
        assert (r.npoints, r.total_out, r.end_bit, r.max_seg, r.status, r.route) == (n, len(data), ix.bit[-1], 0, E_OUT_CAPACITY, first.rec.route), P
        assert g.bit == [(1 << 64) - 1] * (P + 1) and g.pos == g.bit and g.crc[:P] == [(1 << 32) - 1] * P and set(g.win.tobytes()) == {0xA5}
        assert g.out[:len(data)] == data                         # (the stream is decoded and judged all the same)
    check_index(index_call(engine.lib, z, container, 1024, n, len(data)), w, 1024, data)


def test_a_stream_that_fails_gives_the_judged_status_and_no_index(engine, streams):
    for name, at, flip in (("L6", -1, 1), ("L6", -4, 0x80), ("GZ6", -5, 4), ("GZ6", -1, 1), ("GZNAME", 1, 0xFF), ("L6", 1000, 0x10)):
        container, z, data, spans = streams[name]
        bad = bytearray(z)
        bad[at] ^= flip
        bad = bytes(bad)
        pitch = (len(data) + 3) & ~3
        d_z = dev_bytes(bad).reshape(1, -1)
        one = (engine.inflate_checked if container == "zlib" else engine.inflate_gzip)(d_z, out_pitch=pitch)
        want = one[2].cpu().tolist()[0]
        assert want != OK, (name, at)
        g = index_call(engine.lib, bad, container, 4096, 200, pitch)
        r = g.rec
        assert (r.npoints, r.total_out, r.end_bit, r.max_seg, r.status) == (0, 0, 0, 0, want), (name, at)
        assert g.bit == [(1 << 64) - 1] * 201 and g.pos == g.bit and set(g.win.tobytes()) == {0xA5}
    # cut in front of the trailer; too short to start; no room for the data
    container, z, data, spans = streams["L9"]
    for cut, cap in ((len(z) - 2, len(data)), (3, len(data)), (len(z), len(data) - 4), (0, 64)):
        pitch = (cap + 3) & ~3
        g = index_call(engine.lib, z[:cut], container, 4096, 8, pitch)
        assert g.rec.status != OK and g.rec.npoints == 0 and g.bit == [(1 << 64) - 1] * 9, cut
        if cut:
            assert g.rec.status == engine.inflate_checked(dev_bytes(z[:cut]).reshape(1, -1), out_pitch=pitch)[2].cpu().tolist()[0], cut


def test_every_route_invariant_and_every_range_on_a_stream_above_the_chains_gate(engine, streams):
    """what ANY route must satisfy, on the index the device itself returned, and every range read back through that index"""
    container, z, data, spans = streams["L6"]
    assert len(z) > 16 * 2048                                    # far above HDLZ_INFLATE_PAR_MIN: the one-stream calls decode it by the chains
    w = ref.walk(z, container)
    true = {b.bit: b.pos for b in w.boundaries}
    span = 16384
    g = index_call(engine.lib, z, container, span, 64, len(data))
    n = g.rec.npoints
    assert g.rec.status == OK and g.rec.route == ROUTE_CHAIN and 1 <= n <= 64
    bit, pos = g.bit[:n + 1], g.pos[:n + 1]
    assert all(true.get(b) == p for b, p in zip(bit[:n], pos[:n]))           # every point is a true boundary
    assert bit[0] == w.boundaries[0].bit and pos[0] == 0                       # point 0 is the first header
    assert all(bit[k] < bit[k + 1] for k in range(n)) and all(pos[k] < pos[k + 1] for k in range(n - 1)) and pos[n - 1] <= pos[n]
    assert all(pos[k] // span > pos[k - 1] // span for k in range(1, n))
    assert (bit[n], pos[n], g.rec.max_seg) == (w.end_bit, len(data), max(pos[k + 1] - pos[k] for k in range(n)))
    for k in range(n):
        assert g.crc[k] == zlib.crc32(data[pos[k]:pos[k + 1]]) and g.win[k].tobytes() == ref.window(data, pos[k])
    D = DevIndex(z, ref.Index(bit, pos, g.crc[:n], [g.win[k].tobytes() for k in range(n)], g.rec.max_seg))
    g2, e = sized_read(engine.lib, D, data, pos, edge_ranges(pos, seed=6))
    assert e.record_status == E_BAD_PARAM and set(e.status) == {OK, E_BAD_PARAM}


# ---- ranges
@pytest.mark.parametrize("name,span", [("MEM1", 1024), ("L0", 32768), ("SYNC", 1024), ("FIXED", 2048), ("GZNAME", 1024), ("GZ6", 4096), ("L1", 65536), ("ONE", 1024)])
def test_every_edge(engine, streams, name, span):
    container, z, data, spans = streams[name]
    ix = ref.index(ref.walk(z, container), span)
    D = DevIndex(z, ix)
    ranges = edge_ranges(ix.pos, seed=span)
    g, e = sized_read(engine.lib, D, data, ix.pos, ranges)
    total = len(data)
    assert e.record_status == E_BAD_PARAM and e.status.count(E_BAD_PARAM) >= 2 and set(e.status) == {OK, E_BAD_PARAM}
    assert all(piece == data[min(x, total):min(y, total)] for piece, (x, y) in zip(e.pieces, ranges) if x <= y)      # (the reference itself)
    if name == "MEM1":
        assert e.ntasks > 512 and len(ix.crc) > 256             # more tasks than one workgroup of the per-task kernels holds


def test_the_sizing_call_and_short_room(engine, streams):
    container, z, data, spans = streams["SYNC"]
    ix = ref.index(ref.walk(z, container), 1024)
    D = DevIndex(z, ix)
    ranges = edge_ranges(ix.pos, seed=3, limit=60)
    full = ref.expected(data, ix.pos, ranges)
    for out_cap, task_cap in ((0, 0), (full.total_out - 1, full.ntasks), (full.total_out, full.ntasks - 1), (full.total_out, 0)):
        g = read(engine.lib, D, ranges, out_cap=out_cap, task_cap=task_cap)
        check(g, ref.expected(data, ix.pos, ranges, out_cap=out_cap, task_cap=task_cap), (out_cap, task_cap))
        assert g.rec.status == E_OUT_CAPACITY and (g.rec.total_out, g.rec.ntasks) == (full.total_out, full.ntasks)
    check(read(engine.lib, D, ranges, out_cap=full.total_out + 9, task_cap=full.ntasks + 70), full)      # idle task slots, spare room
    g = read(engine.lib, D, [])
    assert (g.rec.total_out, g.rec.ntasks, g.rec.first_bad, g.rec.status) == (0, 0, ref.NOBODY, OK) and g.range_off == [0]


# ---- crafted seams: the first token behind a point is a match into the window
def _seam(D_, length, kind, npre, D_bad=None):
    rng = np.random.RandomState(D_ + length)
    pre = rng.randint(0, 256, size=npre).tolist()
    tail = [(length, D_)] + rng.randint(0, 256, size=40).tolist() + [(9, 3), (258, min(D_, npre)), 1, 2, 3]
    if D_bad is not None:
        tail[0] = (length, D_bad)
    return craft.geometry_case("seam", [pre, tail], kind, status=OK if D_bad is None else E_BAD_DISTANCE)


SEAMS = [(1, 20, 33000), (1536, 70, 33000), (1537, 70, 33000), (2048, 258, 33000), (32768, 258, 33000), (32768, 5, 32768),
         (7, 100, 5000), (64, 258, 2500), (1537, 40, 1537), (1, 258, 1)]       # (distance, length, bytes in front of the point)


@pytest.mark.parametrize("kind", craft.GEO_KINDS)
def test_crafted_seams(engine, kind):
    for dist, length, npre in SEAMS:
        c = _seam(dist, length, kind, npre)
        w = ref.walk(c.z, "zlib")
        assert w.data == c.plain and [b.pos for b in w.boundaries] == [0, npre]
        span = max(npre, 1)
        ix = ref.index(w, span)
        assert ix.pos == [0, npre, len(c.plain)]
        label = (kind, dist, length, npre)
        got = check_index(index_call(engine.lib, c.z, "zlib", span, 2, (len(c.plain) + 3) & ~3), w, span, c.plain, label)
        assert got.pos == ix.pos or kind == "fixed"             # (the chain route knows no fixed header: one point)
        D = DevIndex(c.z, ix)
        ranges = [(npre, len(c.plain)), (npre, npre + 1), (npre + length - 1, npre + length + 3), (0, len(c.plain)), (npre - 1, npre + 2), (len(c.plain) - 1, len(c.plain))]
        g, e = sized_read(engine.lib, D, c.plain, ix.pos, ranges)
        assert e.record_status == OK, label


@pytest.mark.parametrize("kind", craft.GEO_KINDS)
def test_a_distance_beyond_the_streams_start_fails_at_a_seam_too(engine, kind):
    """distance pos + 1 at a point with pos < 32768: HDLZ_E_BAD_DISTANCE, as in the whole-stream decode -- read through the index of the
    twin stream whose distance is pos (the same code lengths, so the same bits everywhere else)"""
    npre = 5000
    good, bad = _seam(npre, 30, kind, npre), _seam(npre, 30, kind, npre, D_bad=npre + 1)
    assert len(good.z) == len(bad.z) and craft.distance_symbol(npre) == craft.distance_symbol(npre + 1)
    d_bad = dev_bytes(bad.z).reshape(1, -1)
    assert engine.inflate_checked(d_bad, out_pitch=8192)[2].cpu().tolist() == [E_BAD_DISTANCE]
    g = index_call(engine.lib, bad.z, "zlib", npre, 4, 8192)
    assert (g.rec.status, g.rec.npoints) == (E_BAD_DISTANCE, 0)
    ix = ref.index(ref.walk(good.z, "zlib"), npre)
    assert ix.pos == [0, npre, len(good.plain)]
    D = DevIndex(bad.z, ix)
    ranges = [(0, 10), (npre, npre + 5), (0, npre), (npre - 1, npre + 1), (npre + 100, npre + 101)]
    sized_read(engine.lib, D, good.plain, ix.pos, ranges, segment_status=[OK, E_BAD_DISTANCE])


# ---- damage: the stated status on exactly the ranges that touch the segment
def _touching(pos, k):
    """ranges that touch only segment k - 1, only k, both, and neither (k >= 2, k + 1 < n)"""
    return [(pos[k - 1], pos[k]), (pos[k], pos[k + 1]), (pos[k] - 1, pos[k] + 1), (pos[k] + 1, pos[k] + 2), (0, pos[k - 1]), (pos[k + 1], pos[-1]),
            (pos[k - 1] + 1, pos[k] - 1), (0, pos[-1])]


def test_a_flipped_window_byte(engine):
    c = _seam(1536, 70, "dynamic", 33000)
    ix = ref.index(ref.walk(c.z, "zlib"), 33000)
    win = [ix.win[0], bytearray(ix.win[1])]
    win[1][WIN - 1536 + 5] ^= 0x40                               # a byte the first match behind the point copies
    D = DevIndex(c.z, ix._replace(win=[bytes(x) for x in win]))
    ranges = [(0, 33000), (33000, 33001), (32999, 33001), (0, len(c.plain)), (10, 20), (len(c.plain) - 1, len(c.plain))]
    sized_read(engine.lib, D, c.plain, ix.pos, ranges, segment_status=[OK, E_BAD_CHECKSUM])


def test_a_flipped_bit_in_the_file(engine, streams):
    container, z, data, spans = streams["L0"]                    # stored blocks: a flipped data bit changes that byte and nothing else
    w = ref.walk(z, container)
    ix = ref.index(w, 32768)
    k = 2
    bad = bytearray(z)
    bad[(ix.bit[k] >> 3) + 200] ^= 0x04
    D = DevIndex(bytes(bad), ix)
    st = [OK] * len(ix.crc)
    st[k] = E_BAD_CHECKSUM
    sized_read(engine.lib, D, data, ix.pos, _touching(ix.pos, k), segment_status=st)
    # in a Huffman block the decoder may stop anywhere: the ranges that touch the segment fail, with one status, and no other does
    container, z, data, spans = streams["MEM1"]
    ix = ref.index(ref.walk(z, container), 5000)
    k = 7
    bad = bytearray(z)
    bad[(ix.bit[k] + ix.bit[k + 1]) >> 4] ^= 0x10
    ranges = _touching(ix.pos, k)
    e = ref.expected(data, ix.pos, ranges, segment_status=[OK] * k + [1] + [OK] * (len(ix.crc) - k - 1))
    g = read(engine.lib, DevIndex(bytes(bad), ix), ranges, out_cap=e.total_out, task_cap=e.ntasks)
    assert [s != OK for s in g.status] == [s != OK for s in e.status] and len({s for s in g.status if s != OK}) == 1
    assert all(g.out[e.range_off[r]:e.range_off[r + 1]] == p for r, p in enumerate(e.pieces) if p is not None)


def test_damaged_index_words(engine, streams):
    container, z, data, spans = streams["GZ6"]
    ix = ref.index(ref.walk(z, container), 4096)
    n, k = len(ix.crc), 9
    ranges = _touching(ix.pos, k)
    # d_crc[k] changed
    crc = list(ix.crc)
    crc[k] ^= 1
    st = [OK] * n
    st[k] = E_BAD_CHECKSUM
    sized_read(engine.lib, DevIndex(z, ix._replace(crc=crc)), data, ix.pos, ranges, segment_status=st)
    # d_bit[k] off by one: segment k - 1 stops at the true header, which is not the word's -- HDLZ_E_NO_EOF; segment k starts astray
    for delta in (1, -1):
        bit = list(ix.bit)
        bit[k] += delta
        e = ref.expected(data, ix.pos, ranges, segment_status=[OK] * (k - 1) + [E_NO_EOF, 1] + [OK] * (n - k - 1))
        g = read(engine.lib, DevIndex(z, ix._replace(bit=bit)), ranges, out_cap=e.total_out, task_cap=e.ntasks)
        assert [s for s in g.status] == [s if s != 1 else g.status[1] for s in e.status] and g.status[1] != OK, delta
        assert g.status[0] == g.status[2] == g.status[7] == E_NO_EOF
        assert all(g.out[e.range_off[r]:e.range_off[r + 1]] == p for r, p in enumerate(e.pieces) if p is not None)
    # words that are not ascending, or outside the file: HDLZ_E_BAD_PARAM, and no decoder starts
    for v in (ix.bit[k + 1], 8 * len(z) + 1):
        bit = list(ix.bit)
        bit[k] = v
        g = read(engine.lib, DevIndex(z, ix._replace(bit=bit)), [(ix.pos[k], ix.pos[k] + 1), (0, 5)], out_cap=6, task_cap=4)
        assert g.status == [E_BAD_PARAM, OK] and g.out[1:6] == data[:5], v
    # seg_cap below a segment
    seg = [ix.pos[j + 1] - ix.pos[j] for j in range(n)]
    big = max(range(2, n - 1), key=lambda j: seg[j])
    cap = seg[big] - 1
    st = [OK if s <= cap else E_BAD_PARAM for s in seg]
    assert st.count(E_BAD_PARAM) >= 1 and st[big] == E_BAD_PARAM
    sized_read(engine.lib, DevIndex(z, ix), data, ix.pos, _touching(ix.pos, big), segment_status=st, seg_cap=cap)


# ---- Engine
def test_engine_seek_index_and_read_seek(engine, streams):
    container, z, data, spans = streams["GZNAME"]
    d = dev_bytes(z)
    ix = ref.index(ref.walk(z, container), 1024)
    calls = []
    inner = engine._record

    def spy(fn, *a):
        calls.append(fn)
        return inner(fn, *a)
    engine._record = spy
    try:
        out, index, rec = engine.seek_index(d, container="gzip", span=1024, point_cap=5)      # a wrong guess: a second call
        assert calls == ["hdlz_seek_index_ws"] * 2
        del calls[:]
        out2, index2, rec2 = engine.seek_index(d, container="gzip", span=1024)
        assert calls == ["hdlz_seek_index_ws"]
    finally:
        del engine._record
    for o, i, r in ((out, index, rec), (out2, index2, rec2)):
        ix = ref.route_index(ref.walk(z, container), 1024, r.route)
        assert o.cpu().numpy().tobytes() == data and (r.npoints, r.status) == (len(ix.crc), OK)
        assert i.bit.cpu().tolist() == ix.bit and i.pos.cpu().tolist() == ix.pos and i.crc.cpu().numpy().view(np.uint32).tolist() == ix.crc
        assert (i.span, i.file_len, i.total, i.end_bit, i.max_seg, i.container, i.npoints) == (1024, len(z), len(data), ix.bit[-1], ix.max_seg, "gzip", len(ix.crc))
    total = len(data)
    ranges = [(0, 10), (299, 5301), (total - 3, total + 50), (70000, 70000), (0, total), (65500, 80000)]
    want = [data[x:y] for x, y in ranges]
    lens = np.cumsum([0] + [len(p) for p in want]).tolist()
    # dumps -> loads -> read_seek
    back = seek.loads(index.dumps(), device=d.device)
    assert back.dumps() == index.dumps() and len(index.dumps()) == seek.file_bytes(index.npoints)
    for i in (index, back):
        for rr in (ranges, words(ranges)):
            got, roff = engine.read_seek(d, rr, i)
            assert roff.cpu().tolist() == lens and got.cpu().numpy().tobytes() == b"".join(want)
    # groups: a scratch limit that holds few ranges at a time
    many = edge_ranges(ix.pos, seed=11, limit=90)
    many = [r for r in many if r[0] <= r[1]]
    got, roff = engine.read_seek(d, many, index, max_work_bytes=1 << 16)
    assert got.cpu().numpy().tobytes() == b"".join(data[x:y] for x, y in many)
    buf = torch.empty(sum(min(y, total) - min(x, total) for x, y in many) + 5, dtype=torch.uint8, device="cuda")
    got, roff = engine.read_seek(d, many, index, out=buf)
    assert got.data_ptr() == buf.data_ptr() and got.cpu().numpy().tobytes() == b"".join(data[x:y] for x, y in many)
    with pytest.raises(HdlzStatusError) as err:
        engine.read_seek(d, [(0, 5), (9, 3), (1, 2)], index)
    assert err.value.status == E_BAD_PARAM and err.value.first_bad == 1
    assert engine.read_seek_bytes(z, 1000, 70000) == (OK, data[1000:70000])
    assert engine.read_seek_bytes(z, 5, 9, index=back.to("cpu")) == (OK, data[5:9])
    bad = bytearray(z)
    bad[len(z) - 11 - 8] ^= 1                                    # the CRC-32 word, in front of ISIZE and the 11 bytes behind the member
    assert engine.read_seek_bytes(bytes(bad), 0, 10) == (E_BAD_CHECKSUM, b"")
    cz, czd = streams["L9"][1], streams["L9"][2]
    out, zi, rec = engine.seek_index(dev_bytes(cz), container="zlib", span=8192, out=torch.empty(len(czd), dtype=torch.uint8, device="cuda"))
    assert out.cpu().numpy().tobytes() == czd and zi.container == "zlib"
    assert engine.read_seek(dev_bytes(cz), [(60000, 65000)], zi)[0].cpu().numpy().tobytes() == czd[60000:65000]
    with pytest.raises(HdlzStatusError):
        engine.seek_index(dev_bytes(cz), container="gzip")


# ---- capture
def test_index_and_ranges_in_one_graph(engine, streams):
    L = engine.lib
    container, z, data, spans = streams["SYNC"]
    w = ref.walk(z, container)
    ix = check_index(index_call(L, z, container, 1024, len(w.boundaries), len(data)), w, 1024, data)      # npoints is a host word: the route's count
    n, P = len(z), len(ix.crc)
    ranges = edge_ranges(ix.pos, seed=4, limit=80)
    e = ref.expected(data, ix.pos, ranges)
    R, total, ntasks = len(ranges), e.total_out, e.ntasks
    d_file = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_ranges = words(ranges)
    cap = (len(data) + 3) & ~3
    dout = torch.empty(cap, dtype=torch.uint8, device="cuda")
    bit, pos = torch.empty(P + 1, dtype=torch.int64, device="cuda"), torch.empty(P + 1, dtype=torch.int64, device="cuda")
    crc, win = torch.empty(P, dtype=torch.int32, device="cuda"), torch.empty((P, WIN), dtype=torch.uint8, device="cuda")
    ires, rres = torch.empty(5, dtype=torch.int64, device="cuda"), torch.empty(4, dtype=torch.int64, device="cuda")
    iwb, rwb = L.hdlz_seek_index_work_bytes(n, FLAGS[container], cap, P), L.hdlz_seek_ranges_work_bytes(R, ntasks, ix.max_seg, 0)
    iwork, rwork = torch.empty(iwb, dtype=torch.uint8, device="cuda"), torch.empty(rwb, dtype=torch.uint8, device="cuda")
    out = torch.empty(total, dtype=torch.uint8, device="cuda")
    range_off, status = torch.empty(R + 1, dtype=torch.int64, device="cuda"), torch.empty(R, dtype=torch.int32, device="cuda")

    def calls():
        s = stream_ptr()
        assert L.hdlz_seek_index_ws(d_file.data_ptr(), n, FLAGS[container], 1024, dout.data_ptr(), cap, bit.data_ptr(), pos.data_ptr(), crc.data_ptr(),
                                    win.data_ptr(), P, ires.data_ptr(), iwork.data_ptr(), iwb, s) == 0
        assert L.hdlz_seek_read_ranges_ws(d_file.data_ptr(), n, bit.data_ptr(), pos.data_ptr(), crc.data_ptr(), win.data_ptr(), P, d_ranges.data_ptr(),
                                          R, 0, ix.max_seg, out.data_ptr(), total, range_off.data_ptr(), status.data_ptr(), ntasks, rres.data_ptr(),
                                          rwork.data_ptr(), rwb, s) == 0

    def fresh(v):
        for t in (dout, bit, pos, crc, win, ires, rres, iwork, rwork, out, range_off, status):
            t.fill_(v)
        d_file.copy_(dev_bytes(z))

    def answer():
        torch.cuda.synchronize()
        g = Got()
        g.rec = _lib.SeekRangesResult.from_buffer_copy(rres.cpu().numpy().tobytes())
        g.range_off, g.status, g.out = range_off.cpu().tolist(), status.cpu().tolist(), out.cpu().numpy().tobytes()
        i = Got()
        i.rec = _lib.SeekResult.from_buffer_copy(ires.cpu().numpy().tobytes())
        i.bit, i.pos = bit.cpu().numpy().view(np.uint64).tolist(), pos.cpu().numpy().view(np.uint64).tolist()
        i.crc, i.win, i.out = crc.cpu().numpy().view(np.uint32).tolist(), win.cpu().numpy(), dout.cpu().numpy().tobytes()
        return g, i
    fresh(0)
    calls()
    plain, pi = answer()
    check(plain, e, "eager")
    check_index(pi, ref.walk(z, container), 1024, data, "eager")
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()                  # one linear stream, as the other _ws graph tests
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            calls()
    for launch in (1, 2):
        fresh(launch)
        g.replay()
        got, gi = answer()
        check(got, e, ("graph", launch))
        check_index(gi, ref.walk(z, container), 1024, data, ("graph", launch))
        assert got.out == plain.out and got.range_off == plain.range_off and got.status == plain.status
