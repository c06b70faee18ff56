"""GPU (-m gpu): hdlz_gzip_members_index_ws and hdlz_gzip_members_inflate_ws inside guard bands (tests/guards.py), in the manner of
tests/test_gpu_gunzip_containment.py: every buffer of a call carved out of one patterned arena, each case run on the pattern and on
its complement.

  bands and read-only regions (the file and what stands behind it, the index of the read) untouched;
  the index writes d_off / d_out_off [0 .. min(M, cap)] only, the read only the slots of the members that passed the index checks
  (an OK member exactly its slot), the status array, the record and the scratch it was given;
  all results identical in both runs -- the runs differ in every byte behind file_len, in every byte of a slot that was not decoded
  and in the initial content of every output and of the scratch, so none of those reaches a result -- and equal to the rules
  (gzip_members_ref)."""
import gzip

import numpy as np
import pytest
import torch

import guards
import gunzip_ref as G
import gzip_members_ref as R
import test_gpu_containment as C

pytestmark = pytest.mark.gpu
BAND = 1 << 16


def index_call(engine, label, z, cap, mis=0):
    L = engine.lib
    wb = L.hdlz_gzip_members_index_work_bytes(len(z))
    specs = [("file", len(z), 16, BAND, True, mis), ("off", 8 * (cap + 1), 8, BAND), ("out_off", 8 * (cap + 1), 8, BAND), ("result", 24, 8, BAND),
             ("work", wb, 256, C.WORK_BAND)]

    def call(a):
        rc = L.hdlz_gzip_members_index_ws(a.ptr("file"), len(z), cap, a.ptr("off"), a.ptr("out_off"), a.ptr("result"), a.ptr("work") if wb else None, wb,
                                          C.stream_ptr())
        assert rc == 0, (label, L.hdlz_last_error())

    a, clean, runs = C.two_runs(specs, lambda a: a.fill("file", z), call, ("off", "out_off", "result"))
    want_off, want_out = R.index_rule(z)
    M = len(want_off) - 1
    k = min(M, cap) + 1
    for r in runs:
        res = r["result"].view(np.uint64)
        assert (int(res[0]), int(res[1])) == (M, want_out[-1]) and list(r["result"].view(np.uint32)[4:]) == [R.E_OUT_CAPACITY if M > cap else 0, 0], label
        assert list(r["off"].view(np.int64)[:k]) == want_off[:k] and list(r["out_off"].view(np.int64)[:k]) == want_out[:k], label
    bad = guards.violations(a, clean, {"off": 8 * k, "out_off": 8 * k, "result": True, "work": True})
    assert bad == [], (label, bad)
    parts = a.split(clean)
    assert not bool(parts["off"][1][:8 * k].any()) and not bool(parts["result"][1].any()), (label, "not written")


def test_the_index_stays_inside_and_reads_nothing_behind_the_file(engine):
    ms, _ = R.many_members()
    x = R.clean_bytes(40000, 3)
    files = [("300 members", b"".join(ms), 300), ("300 members, room for 10", b"".join(ms), 10), ("ends in a magic without its flag byte", x + b"\x1f\x8b\x08", 4),
             ("ends one byte into a magic", x[:32767] + b"\x1f", 4), ("a window's last bytes", x[:32765] + b"\x1f\x8b\x08", 4),
             ("17 bytes", R.MAGIC + bytes(13), 1), ("one byte", b"\x1f", 0), ("empty", b"", 0),
             ("look-alikes every 4 bytes", R.MAGIC * 5000, 5000), ("stored over three windows", R.stored_of_length(100000, 4) + ms[0], 2)]
    for mis, (label, z, cap) in enumerate(files):
        index_call(engine, label, z, cap, mis=mis % 16)


def read_call(engine, oracle, label, z, off, out_off, out_cap, status=True, mis=0, out_mis=0):
    L, B = engine.lib, len(off) - 1
    wb = L.hdlz_gzip_members_inflate_work_bytes(B)
    off_b, out_b = (np.asarray(v, np.int64).view(np.uint8) for v in (off, out_off))
    specs = [("file", len(z), 16, BAND, True, mis), ("off", 8 * (B + 1), 8, BAND, True), ("out_off", 8 * (B + 1), 8, BAND, True),
             ("out", out_cap, 16, BAND, False, out_mis), ("status", 4 * B, 4, BAND), ("result", 24, 8, BAND), ("work", wb, 256, C.WORK_BAND)]

    def setup(a):
        a.fill("file", z)
        a.fill("off", off_b)
        a.fill("out_off", out_b)

    def call(a):
        rc = L.hdlz_gzip_members_inflate_ws(a.ptr("file"), len(z), a.ptr("off"), a.ptr("out_off"), B, a.ptr("out"), out_cap, a.ptr("status") if status else None,
                                            a.ptr("result"), a.ptr("work"), wb, C.stream_ptr())
        assert rc == 0, (label, L.hdlz_last_error())

    a, clean, runs = C.two_runs(specs, setup, call, ("out", "status", "result"))
    assert np.array_equal(runs[0]["result"], runs[1]["result"]) and (not status or np.array_equal(runs[0]["status"], runs[1]["status"])), (label, "depends on bytes the call was not given")
    may = torch.zeros(out_cap, dtype=torch.bool, device="cuda")
    first, sts = None, []
    for b in range(B):
        lo, hi = out_off[b] - out_off[0], out_off[b + 1] - out_off[0]
        want, data = R.verdict(oracle, z, off[b], off[b + 1], hi - lo, out_room=out_cap - lo)
        assert want is not None
        sts.append(want)
        if want != R.E_BAD_PARAM:
            may[lo:hi] = True                             # an OK member: exactly its slot; a failed one: anything inside it
        if want != R.OK and first is None:
            first = b
        for r in runs:
            assert want != R.OK or bytes(r["out"][lo:hi]) == data, (label, b)
            assert not status or int(r["status"].view(np.uint32)[b]) == want, (label, b, int(r["status"].view(np.uint32)[b]), want)
    res = runs[0]["result"]
    want_rec = (out_off[-1] - out_off[0], (1 << 64) - 1, 0) if first is None else (0, first, sts[first])
    assert (int(res.view(np.uint64)[0]), int(res.view(np.uint64)[1]), int(res.view(np.uint32)[4])) == want_rec, (label, want_rec)
    allowed = {"out": may, "result": True, "work": True}
    if status:
        allowed["status"] = True
    bad = guards.violations(a, clean, allowed)
    assert bad == [], (label, bad)
    parts = a.split(clean)
    ok = torch.zeros(out_cap, dtype=torch.bool, device="cuda")
    for b in range(B):
        if sts[b] == R.OK:
            ok[out_off[b] - out_off[0]:out_off[b + 1] - out_off[0]] = True
    assert not bool((parts["out"][1] & ok).any()), (label, "a byte of an OK member's slot was not written")
    assert not bool(parts["result"][1].any()) and (not status or not bool(parts["status"][1].any())), (label, "not written")
    if not status:
        assert bool(parts["status"][1].all()), (label, "d_member_status = NULL: nothing of that region may be written")
    return sts


def test_the_read_stays_inside_the_slots_of_the_members_it_decodes(engine, oracle):
    ms, datas = R.many_members()
    z = b"".join(ms[:120])
    off, out_off = R.index_rule(z)
    assert read_call(engine, oracle, "120 members", z, off, out_off, out_off[-1], mis=3, out_mis=5) == [R.OK] * 120
    read_call(engine, oracle, "120 members, no status array", z, off, out_off, out_off[-1] + 100, status=False, mis=1)
    # the last three slots end behind out_cap: not decoded, nothing of them written
    sts = read_call(engine, oracle, "out_cap inside member 117's slot", z, off, out_off, out_off[118] - 1, mis=9, out_mis=1)
    assert sts[:117] == [R.OK] * 117 and sts[117:] == [R.E_BAD_PARAM] * 3
    d = G.text(3000, 81)
    good = G.gz(d, name=b"c")
    parts = [(good, 3000), (good, 2999), (good, 3001), (G.gz(d, crc_xor=1), 3000), (good[:-2], 3000), (good + bytes(3), 3000), (G.gz(d, flg=0x40), 3000),
             (gzip.compress(b"", mtime=1), 0), (G.gz(d, level=0), 3000), (good[:9], 64), (good, 3000)]
    off = [0] + [int(o) for o in np.cumsum([len(p) for p, _ in parts])]
    out_off = [7] + [7 + int(o) for o in np.cumsum([n for _, n in parts])]
    sts = read_call(engine, oracle, "members that fail", b"".join(p for p, _ in parts), off, out_off, out_off[-1] - 7, mis=15, out_mis=11)
    assert sts == [R.OK, R.E_OUT_CAPACITY, R.E_BAD_CHECKSUM, R.E_BAD_CHECKSUM, R.E_NO_EOF, R.E_NO_EOF, R.E_BAD_HEADER, R.OK, R.OK, R.E_NO_EOF, R.OK]
