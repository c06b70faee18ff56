"""GPU (-m gpu): hdlz_zip_index_ws and hdlz_zip_inflate_ws inside guard bands (tests/guards.py), in the manner of
tests/test_gpu_gunzip_containment.py: every buffer of a call carved out of one patterned arena, each case run on the pattern and on its
complement.

  bands and read-only regions (the file and what stands behind it, the records hdlz_zip_inflate_ws is given) untouched;
  the index writes d_entries[0 .. min(nentries, entry_cap)) and the record, the read the slots of the entries that passed its checks,
  d_entry_status[0 .. count) and the record; d_work only inside what was passed; nothing at or behind out_cap;
  all results identical in both runs -- the runs differ in every byte behind file_len, in every byte outside the slots and in the
  initial content of every output and of the scratch, so none of those reaches a result -- and equal to the rule (zip_ref)."""
import numpy as np
import pytest
import torch

import guards
import zip_ref as Z
import test_gpu_containment as C

pytestmark = pytest.mark.gpu
BAND = 1 << 16


def index_call(engine, label, z, cap, out_align, mis=0):
    L = engine.lib
    wb = L.hdlz_zip_index_work_bytes(len(z), cap)
    specs = [("file", len(z), 16, BAND, True, mis), ("entries", 48 * cap, 8, BAND), ("result", 40, 8, BAND), ("work", wb, 8, C.WORK_BAND)]

    def call(a):
        rc = L.hdlz_zip_index_ws(a.ptr("file"), len(z), cap, out_align, a.ptr("entries") if cap else None, a.ptr("result"), a.ptr("work"), wb, C.stream_ptr())
        assert rc == 0, (label, L.hdlz_last_error())

    a, clean, runs = C.two_runs(specs, lambda a: a.fill("file", z), call, ("entries", "result"))
    ix = Z.index(z, out_align, cap)
    k = min(cap, ix["nentries"])
    for r in runs:
        res = np.frombuffer(r["result"].tobytes(), np.uint64)
        assert [int(x) for x in res[:4]] == [ix["nentries"], ix["total_out"], ix["cd_off"], ix["cd_size"]] and int(res[4]) == ix["status"], (label, res)
        from hdl_deflate_amd.zip import ENTRY_DTYPE
        got = np.frombuffer(r["entries"].tobytes(), ENTRY_DTYPE)[:k]
        assert [tuple(int(g[f]) for f in Z.FIELDS) for g in got] == Z.records(ix)[:k] and not got["reserved"].any(), label
    bad = guards.violations(a, clean, {"entries": 48 * k, "result": True, "work": True})
    assert bad == [], (label, bad)
    parts = a.split(clean)
    assert not bool(parts["entries"][1][:48 * k].any()) and not bool(parts["result"][1].any()), (label, "not written")
    return ix


def test_the_index_stays_inside_its_records(engine):
    nine = Z.make_zip(Z.base_items())
    for label, z, cap, align, mis in (("nine, exact", nine, 9, 1, 0), ("nine, room for 12", nine, 12, 64, 5), ("nine, room for 4", nine, 4, 256, 3),
                                      ("nine, the sizing call", nine, 0, 1, 1), ("names of 1 to 700", dict(Z.geometry_cases())["names of 1 to 700"], 200, 16, 7),
                                      ("a long record", dict(Z.geometry_cases())["a record of 46 + 3 * 65535"], 3, 1, 9),
                                      ("broken at entry 3", Z.file_damage_cases()[6][1], 8, 1, 2), ("a cut end record", Z.file_damage_cases()[1][1], 8, 1, 0),
                                      ("21 bytes", Z.file_damage_cases()[2][1], 2, 1, 11), ("a nested archive", Z.lookalike_cases()[2][1], 2, 4, 13)):
        index_call(engine, label, z, cap, align, mis)


def inflate_call(engine, label, z, out_align, first, count, in_len=0, mis=0, out_mis=0, slack=0):
    """one guarded hdlz_zip_inflate_ws over entries [first, first + count) of the rule's own index"""
    L = engine.lib
    ix, sts, flat = Z.read(z, out_align)
    ens = ix["entries"]
    from hdl_deflate_amd.zip import ENTRY_DTYPE
    recs = np.zeros(len(ens), ENTRY_DTYPE)
    for k, en in enumerate(ens):
        for f in Z.FIELDS:
            recs[f][k] = en[f]
    base = ens[first]["out_off"]
    total = ens[first + count - 1]["out_off"] - base + (ens[first + count - 1]["usize"] if ens[first + count - 1]["status"] == Z.OK else 0)
    cap = ((total + 3) & ~3 if count == 1 else total) + slack
    wb = L.hdlz_zip_inflate_work_bytes(count, in_len, cap)
    specs = [("file", len(z), 16, BAND, True, mis), ("entries", 48 * len(ens), 8, BAND, True), ("out", cap, 16, max(BAND, 2 * cap), False, out_mis),
             ("status", 4 * count, 4, BAND), ("result", 24, 8, BAND), ("work", wb, 256, C.WORK_BAND)]

    def setup(a):
        a.fill("file", z)
        a.fill("entries", recs.tobytes())

    def call(a):
        rc = L.hdlz_zip_inflate_ws(a.ptr("file"), len(z), a.ptr("entries"), first, count, in_len, a.ptr("out"), cap, a.ptr("status"), a.ptr("result"),
                                   a.ptr("work"), wb, C.stream_ptr())
        assert rc == 0, (label, L.hdlz_last_error())

    a, clean, runs = C.two_runs(specs, setup, call, ("out", "status", "result"))
    assert np.array_equal(runs[0]["status"], runs[1]["status"]) and np.array_equal(runs[0]["result"], runs[1]["result"]), (label, "depends on bytes the call was not given")
    single = count == 1 and cap >= 4 and out_mis % 4 == 0
    may = torch.zeros(cap, dtype=torch.bool, device="cuda")
    for r in runs:
        st = r["status"].view(np.uint32)
        for k in range(count):
            en, want = ens[first + k], sts[first + k]
            o = en["out_off"] - base
            assert (st[k] != Z.OK) if want is None else (st[k] == want), (label, first + k, int(st[k]), want)
            if want == Z.OK:
                assert r["out"][o:o + en["usize"]].tobytes() == flat[en["out_off"]:en["out_off"] + en["usize"]], (label, first + k, "bytes")
            if en["status"] == Z.OK:                            # the entry passed the checks: its slot may be written (single: its row)
                may[o:(cap & ~3) if single else o + en["usize"]] = True
        res = np.frombuffer(r["result"].tobytes(), np.uint64)
        bad = [k for k in range(count) if sts[first + k] != Z.OK]
        assert int(res[1]) == (bad[0] if bad else 2 ** 64 - 1) and int(res[0]) == (0 if bad else total) and int(res[2]) == (int(st[bad[0]]) if bad else 0), (label, res)
    found = guards.violations(a, clean, {"out": may, "status": True, "result": True, "work": True})
    assert found == [], (label, found)
    parts = a.split(clean)
    assert not bool(parts["status"][1].any()) and not bool(parts["result"][1].any()), (label, "not written")
    for k in range(count):                                      # an OK slot is written in full
        en = ens[first + k]
        if sts[first + k] == Z.OK:
            assert not bool(parts["out"][1][en["out_off"] - base:en["out_off"] - base + en["usize"]].any()), (label, first + k, "slot not written")
    return runs


def test_the_task_view_stays_inside_the_slots(engine):
    """count >= 2: deflated and stored entries of 0 to 70000 bytes at every alignment, slots with gaps between them (out_align 64), a
    sub-range, damaged entries among sound ones, room behind the last slot"""
    nine = Z.make_zip(Z.base_items())
    inflate_call(engine, "nine", nine, 1, 0, 9, mis=3, out_mis=1)
    inflate_call(engine, "nine, aligned slots", nine, 64, 0, 9, mis=0, slack=100)
    inflate_call(engine, "nine, a sub-range", nine, 1, 2, 5, mis=7, out_mis=2)
    inflate_call(engine, "nine, a stated bound", nine, 1, 0, 9, in_len=1 << 20)
    for k in (0, 1, 6, 7, 12, 14, 15):                         # flipped payload and CRC, a broken local signature, usize and csize off by one
        label, z, e, want = Z.entry_damage_cases()[k]
        inflate_call(engine, label, z, 1, 0, 9, mis=k, out_mis=k % 5)
    inflate_call(engine, "zipfile mixed", dict(Z.writer_cases())["zipfile mixed"], 1, 0, 27, mis=1, out_mis=3)
    inflate_call(engine, "one entry at an odd address", nine, 1, 4, 1, in_len=1 << 20, out_mis=1)       # (count == 1, but no row for the batch call's path)


def test_one_entry_takes_the_batch_calls_path_in_guarded_scratch(engine):
    """count == 1: small entries (one wave), a 3 MiB deflated entry (the whole-GPU chains, their scratch behind the call's own words) and
    a 3 MiB stored one (the flat copy and the tiles) -- intact and damaged"""
    nine = Z.make_zip(Z.base_items())
    for e in (0, 1, 3, 4, 7):
        c = Z.index(nine)["entries"][e]["csize"]
        inflate_call(engine, ("nine, alone", e), nine, 1, e, 1, in_len=c + 6, mis=e)
        inflate_call(engine, ("nine, alone, no bound", e), nine, 4, e, 1, in_len=0, slack=8)
    for k in (0, 1, 13, 14):
        label, z, e, want = Z.entry_damage_cases()[k]
        inflate_call(engine, (label, "alone"), z, 1, e, 1, in_len=Z.index(z)["entries"][e]["csize"] + 6)
    data = C.plain_bytes(3 << 20, 7)
    z = Z.make_zip([dict(name=b"head", data=Z.text(100, 1)), dict(name=b"three.bin", data=data, level=6), dict(name=b"raw.bin", data=data, method=0)])
    ix = Z.index(z, 16)
    for e in (1, 2):
        inflate_call(engine, ("3 MiB", e), z, 16, e, 1, in_len=ix["entries"][e]["csize"] + 6, mis=e)
    bad = bytearray(z)
    bad[ix["entries"][1]["cd_off"] + 16] ^= 1                   # the directory's CRC of the deflated entry
    bad[ix["entries"][2]["payload_off"] + 12345] ^= 1           # a byte of the stored one
    for e in (1, 2):
        runs = inflate_call(engine, ("3 MiB, damaged", e), bytes(bad), 16, e, 1, in_len=ix["entries"][e]["csize"] + 6)
        assert int(runs[0]["status"].view(np.uint32)[0]) == Z.E_BAD_CHECKSUM
