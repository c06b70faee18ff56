"""GPU (-m gpu): hdlz_bgzf_read_ranges_ws inside the guard bands of tests/guards.py, as tests/test_gpu_bgzf_containment.py runs the calls
of hdlz_bgzf.h: every buffer carved out of one patterned arena, on the pattern and on its complement -- no byte outside the stated
"writes" changes, the scratch stays inside work_bytes, and the results do not depend on the initial contents of the outputs and the
scratch, nor on the bytes around the inputs.  A forged index whose range lengths add up to more than 64 bits hold is refused whole: a
sum that wrapped to what the caller offered must not send a decoder to d_out + 2^63."""
import numpy as np
import pytest
import torch

import bgzf_ref
import bgzf_range_ref as ref
import guards
from bgzf_ref import OK, E_OUT_CAPACITY, E_BAD_CHECKSUM
from bgzf_range_ref import NOBODY
from hdl_deflate_amd import _lib

pytestmark = pytest.mark.gpu

BAND = 1 << 16
SALTS = (0x3C, 0x3C ^ 0xFF)


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def u8(a, dtype):
    return np.array(a, dtype).view(np.uint8)


@pytest.mark.parametrize("case", ["good", "damaged", "capacity"])
def test_read_ranges_inside_guard_bands(engine, case):
    L = engine.lib
    f, data = ref.file_a(6)
    w = bgzf_ref.walk(f)
    M = w.nmembers
    ms = [OK] * M
    if case == "damaged":
        f = f[:w.off[4] - 8] + bytes([f[w.off[4] - 8] ^ 0x80]) + f[w.off[4] - 7:]      # member 3's CRC
        ms[3] = E_BAD_CHECKSUM
    # slices of both edge members at every residue, whole members between them, one member alone, empty and bad ranges
    ranges = ref.edge_ranges(w.out_off, seed=8, limit=40) + [(k, 70000 + 3 * k) for k in range(1, 18)] + ([] if case == "good" else [(9, 3)])
    R = len(ranges)
    full = ref.expected(f, ranges, member_status=ms)
    out_cap = full.total_out - (1 if case == "capacity" else 0)
    e = ref.expected(f, ranges, member_status=ms, out_cap=out_cap)
    assert e.record_status == {"good": OK, "damaged": E_BAD_CHECKSUM, "capacity": E_OUT_CAPACITY}[case]
    T = full.ntasks + 3                                                  # idle task slots behind the last task
    wb = L.hdlz_bgzf_ranges_work_bytes(R, T, 0)
    specs = [("file", len(f), 16, BAND, True, 1), ("off", 8 * (M + 1), 8, BAND, True), ("out_off", 8 * (M + 1), 8, BAND, True),
             ("ranges", 16 * R, 8, BAND, True), ("out", out_cap, 16, BAND, False, 3), ("range_off", 8 * (R + 1), 8, BAND),
             ("status", 4 * R, 4, BAND), ("result", 32, 8, BAND), ("work", wb, 256, BAND)]
    fills = {"file": f, "off": u8(w.off, np.int64), "out_off": u8(w.out_off, np.int64), "ranges": u8(ranges, np.uint64)}
    clean, runs = None, []
    for salt in SALTS:
        a = guards.Arena(guards.Arena.size_for(specs), "cuda", salt)
        for s in specs:
            a.carve(*s)
        for name, d in fills.items():
            a.fill(name, d)
        rc = L.hdlz_bgzf_read_ranges_ws(a.ptr("file"), len(f), a.ptr("off"), a.ptr("out_off"), M, a.ptr("ranges"), R, 0, a.ptr("out"), out_cap,
                                        a.ptr("range_off"), a.ptr("status"), T, a.ptr("result"), a.ptr("work"), wb, stream_ptr())
        assert rc == 0, L.hdlz_last_error()
        torch.cuda.synchronize()
        u = a.untouched_flat()
        clean = u if clean is None else clean & u
        runs.append({n: a.view(n).cpu().numpy().copy() for n in ("out", "range_off", "status", "result")})
    sound = np.zeros(out_cap, bool)                                      # the pieces of the ranges that did not fail
    for r, piece in enumerate(e.pieces):
        if piece is not None:
            sound[e.range_off[r]:e.range_off[r + 1]] = True
    for run in runs:
        rec = _lib.BgzfRangesResult.from_buffer_copy(run["result"].tobytes())
        assert (rec.total_out, rec.ntasks, rec.first_bad, rec.status, rec.reserved) == (e.total_out, e.ntasks, e.first_bad, e.record_status, 0)
        assert list(run["range_off"].view(np.int64)) == e.range_off and list(run["status"].view(np.int32)) == e.status
        if case != "capacity":
            out = run["out"].tobytes()
            for r, piece in enumerate(e.pieces):
                assert piece is None or out[e.range_off[r]:e.range_off[r + 1]] == piece, r
    for n in ("range_off", "status", "result"):
        assert runs[0][n].tobytes() == runs[1][n].tobytes(), n
    assert np.array_equal(runs[0]["out"][sound], runs[1]["out"][sound])
    allowed = {"range_off": True, "status": True, "result": True, "work": True}
    if case != "capacity":
        allowed["out"] = True                                            # (a failed range's own piece is unspecified, and the call's to write)
    bad = guards.violations(a, clean, allowed)
    assert bad == [], bad
    parts = a.split(clean)
    assert not bool(parts["range_off"][1].any()) and not bool(parts["status"][1].any()) and not bool(parts["result"][1].any())
    if case == "good":
        assert not bool(parts["out"][1].any())                           # every byte of d_out[0 .. total_out) was delivered
    if case == "capacity":
        assert bool(parts["out"][1].all())                               # nothing decoded, d_out not written


@pytest.mark.parametrize("copies", [1, 90])
def test_a_forged_index_whose_lengths_wrap_is_refused(engine, copies):
    """O = [0, 2^63, 2^63 + 100] over two real members, the second of 100 bytes; the ranges (0, 2^63), (2^63, 2^63 + 100), (0, 2^63)
    have lengths that add up to 2^64 + 100, which wraps to 100 -- exactly what out_cap = 100 offers -- with range 1 a sound task whose
    piece would begin at d_out + 2^63.  The sum is held at 2^64 - 1 instead, which is HDLZ_E_OUT_CAPACITY: statuses only, nothing
    decoded, no byte outside the stated writes.  copies = 1: a range per thread of the scan, the sum saturates between threads;
    copies = 90: 270 ranges, two per thread, it saturates inside a thread's strip."""
    L = engine.lib
    f = bgzf_ref.member(bgzf_ref.data(300, 1), 6) + bgzf_ref.member(bgzf_ref.data(100, 2), 6) + bgzf_ref.EOF
    w = bgzf_ref.walk(f)
    M, top = 2, 1 << 63
    off, out_off = w.off[:M + 1], [0, top, top + 100]
    ranges = [(0, top), (top, top + 100), (0, top)] * copies
    R = T = len(ranges)                                                  # every range touches one member
    out_cap, sat = 100, (1 << 64) - 1
    want_off = [0]
    for x, y in ranges:
        want_off.append(min(want_off[-1] + y - x, sat))
    assert want_off[-1] == sat and sum(y - x for x, y in ranges[:3]) % (1 << 64) == out_cap
    wb = L.hdlz_bgzf_ranges_work_bytes(R, T, 0)
    specs = [("file", len(f), 16, BAND, True, 1), ("off", 8 * (M + 1), 8, BAND, True), ("out_off", 8 * (M + 1), 8, BAND, True),
             ("ranges", 16 * R, 8, BAND, True), ("out", out_cap, 16, BAND, False, 3), ("range_off", 8 * (R + 1), 8, BAND),
             ("status", 4 * R, 4, BAND), ("result", 32, 8, BAND), ("work", wb, 256, BAND)]
    fills = {"file": f, "off": u8(off, np.uint64), "out_off": u8(out_off, np.uint64), "ranges": u8(ranges, np.uint64)}
    clean, runs = None, []
    for salt in SALTS:
        a = guards.Arena(guards.Arena.size_for(specs), "cuda", salt)
        for s in specs:
            a.carve(*s)
        for name, d in fills.items():
            a.fill(name, d)
        rc = L.hdlz_bgzf_read_ranges_ws(a.ptr("file"), len(f), a.ptr("off"), a.ptr("out_off"), M, a.ptr("ranges"), R, 0, a.ptr("out"), out_cap,
                                        a.ptr("range_off"), a.ptr("status"), T, a.ptr("result"), a.ptr("work"), wb, stream_ptr())
        assert rc == 0, L.hdlz_last_error()
        torch.cuda.synchronize()
        u = a.untouched_flat()
        clean = u if clean is None else clean & u
        runs.append({n: a.view(n).cpu().numpy().copy() for n in ("range_off", "status", "result")})
    for run in runs:
        rec = _lib.BgzfRangesResult.from_buffer_copy(run["result"].tobytes())
        assert (rec.total_out, rec.ntasks, rec.first_bad, rec.status, rec.reserved) == (sat, T, NOBODY, E_OUT_CAPACITY, 0)
        assert list(run["range_off"].view(np.uint64)) == want_off and list(run["status"].view(np.int32)) == [E_OUT_CAPACITY] * R
    bad = guards.violations(a, clean, {"range_off": True, "status": True, "result": True, "work": True})
    assert bad == [], bad
    assert bool(a.split(clean)["out"][1].all())                          # nothing decoded, d_out not written
