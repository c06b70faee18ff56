"""GPU (-m gpu): hdlz_zip64_index_ws, hdlz_zip64_inflate_ws and hdlz_zip64_write_ws inside guard bands (tests/guards.py), in the manner of
tests/test_gpu_zip_containment.py: every buffer of a call carved out of one patterned arena, each case run on the pattern and on its
complement.

  bands and read-only regions (the file and what stands behind it, the records hdlz_zip64_inflate_ws is given) untouched;
  the index writes d_entries[0 .. min(nentries, entry_cap)) and the record, the read the slots of the entries that passed its checks,
  d_entry_status[0 .. count) and the record; d_work only inside what was passed -- the index's scratch is sized from entry_cap --;
  nothing at or behind out_cap; the writer writes d_file[0 .. file_len) when it fits (no byte when it does not), d_entries[0 .. E), the
  record, d_work only inside what was passed;
  all results identical in both runs -- the runs differ in every byte behind file_len, in every byte outside the slots and in the
  initial content of every output and of the scratch, so none of those reaches a result -- and equal to the rule (zip64_ref)."""
import numpy as np
import pytest
import torch

import guards
import zip_ref as Z
import zip64_ref as R
import test_gpu_containment as C

pytestmark = pytest.mark.gpu
BAND = 1 << 16


def index_call(engine, label, z, cap, out_align, mis=0):
    from hdl_deflate_amd.zip import ENTRY64_DTYPE
    L = engine.lib
    wb = L.hdlz_zip64_index_work_bytes(len(z), cap)
    assert wb == 256 + (16 * cap + 255) // 256 * 256
    specs = [("file", len(z), 16, BAND, True, mis), ("entries", 64 * cap, 8, BAND), ("result", 40, 8, BAND), ("work", wb, 8, C.WORK_BAND)]

    def call(a):
        rc = L.hdlz_zip64_index_ws(a.ptr("file"), len(z), cap, out_align, a.ptr("entries") if cap else None, a.ptr("result"), a.ptr("work"), wb, C.stream_ptr())
        assert rc == 0, (label, L.hdlz_last_error())

    a, clean, runs = C.two_runs(specs, lambda a: a.fill("file", z), call, ("entries", "result"))
    ix = R.index(z, out_align, cap)
    k = min(cap, ix["nentries"])
    for r in runs:
        res = np.frombuffer(r["result"].tobytes(), np.uint64)
        assert [int(x) for x in res[:4]] == [ix["nentries"], ix["total_out"], ix["cd_off"], ix["cd_size"]] and int(res[4]) == ix["status"], (label, res)
        got = np.frombuffer(r["entries"].tobytes(), ENTRY64_DTYPE)[:k]
        assert [tuple(int(g[f]) for f in Z.FIELDS) for g in got] == Z.records(ix)[:k] and not got["reserved"].any() and not got["reserved2"].any(), label
    bad = guards.violations(a, clean, {"entries": 64 * k, "result": True, "work": True})
    assert bad == [], (label, bad)
    parts = a.split(clean)
    assert not bool(parts["entries"][1][:64 * k].any()) and not bool(parts["result"][1].any()), (label, "not written")
    return ix


def test_the_index_stays_inside_its_records(engine):
    three = R.make_zip64(R.three_items(), always=True)
    nine = Z.make_zip(Z.base_items())
    many = R.make_zip64([dict(name=b"%04d" % k, data=b"z" * (k % 5), method=0, ones=("L",) if k % 3 else ()) for k in range(3000)])
    bad = {c[0]: c[1] for c in R.bad_cases()}
    for label, z, cap, align, mis in (("three, exact", three, 3, 1, 0), ("three, room for 12", three, 12, 64, 5), ("three, room for 2", three, 2, 256, 3),
                                      ("three, the sizing call", three, 0, 1, 1), ("nine, no locator", nine, 9, 16, 7), ("nine, room for 4", nine, 4, 1, 2),
                                      ("3000 entries, exact", many, 3000, 1, 9), ("3000 entries, room for 1025", many, 1025, 4, 11),
                                      ("3000 entries, the sizing call", many, 0, 1, 0),
                                      ("a record straddling the piece", R.straddle_case(40), 3, 1, 13),
                                      ("r off by one", bad["r off by one"], 3, 1, 2), ("a field 4 bytes short", bad["a field 4 bytes short"], 3, 1, 6),
                                      ("a field overrunning m", bad["a field overrunning m in front of the ZIP64 one"], 3, 8, 1),
                                      ("21 bytes", Z.file_damage_cases()[2][1], 2, 1, 11)):
        index_call(engine, label, z, cap, align, mis)


def inflate_call(engine, label, z, out_align, first, count, in_len=0, mis=0, out_mis=0, slack=0):
    """one guarded hdlz_zip64_inflate_ws over entries [first, first + count) of the rule's own index"""
    from hdl_deflate_amd.zip import ENTRY64_DTYPE
    L = engine.lib
    ix, sts, flat = R.read(z, out_align)
    ens = ix["entries"]
    recs = np.zeros(len(ens), ENTRY64_DTYPE)
    for k, en in enumerate(ens):
        for f in Z.FIELDS:
            recs[f][k] = en[f]
    base = ens[first]["out_off"]
    total = ens[first + count - 1]["out_off"] - base + (ens[first + count - 1]["usize"] if ens[first + count - 1]["status"] == Z.OK else 0)
    cap = ((total + 3) & ~3 if count == 1 else total) + slack
    wb = L.hdlz_zip64_inflate_work_bytes(count, in_len, cap)
    specs = [("file", len(z), 16, BAND, True, mis), ("entries", 64 * len(ens), 8, BAND, True), ("out", cap, 16, max(BAND, 2 * cap), False, out_mis),
             ("status", 4 * count, 4, BAND), ("result", 24, 8, BAND), ("work", wb, 256, C.WORK_BAND)]

    def setup(a):
        a.fill("file", z)
        a.fill("entries", recs.tobytes())

    def call(a):
        rc = L.hdlz_zip64_inflate_ws(a.ptr("file"), len(z), a.ptr("entries"), first, count, in_len, a.ptr("out"), cap, a.ptr("status"), a.ptr("result"),
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


def test_the_read_stays_inside_the_slots(engine):
    """count >= 2 (the task view) and count == 1 (the one-stream route: one wave, the whole-GPU chains, the flat copy and the tiles)
    over 64-byte records: ZIP64 files and classic ones, sound and damaged entries, slots with gaps, a sub-range, an odd d_out"""
    three = R.make_zip64(R.three_items(), always=True)
    nine = Z.make_zip(Z.base_items())
    inflate_call(engine, "three", three, 1, 0, 3, mis=3, out_mis=1)
    inflate_call(engine, "three, aligned slots", three, 64, 0, 3, slack=100)
    inflate_call(engine, "nine", nine, 1, 0, 9, mis=5, out_mis=2)
    inflate_call(engine, "nine, a sub-range", nine, 16, 2, 5, in_len=1 << 20)
    inflate_call(engine, "a field 4 bytes short", dict((c[0], c[1]) for c in R.bad_cases())["a field 4 bytes short"], 1, 0, 3, mis=1)
    for k in (0, 1, 6, 13, 14):                                 # flipped payload and CRC, usize and csize off by one
        label, z, e, want = Z.entry_damage_cases()[k]
        inflate_call(engine, label, z, 1, 0, 9, mis=k, out_mis=k % 5)
        inflate_call(engine, (label, "alone"), z, 4, e, 1, in_len=R.index(z)["entries"][e]["csize"] + 6)
    for e in range(3):
        inflate_call(engine, ("three, alone", e), three, 4, e, 1, in_len=R.index(three)["entries"][e]["csize"] + 6, mis=e)
        inflate_call(engine, ("three, alone, no bound", e), three, 1, e, 1, in_len=0, slack=8)
    inflate_call(engine, "one entry at an odd address", nine, 1, 4, 1, in_len=1 << 20, out_mis=1)
    data = C.plain_bytes(3 << 20, 7)
    z = R.make_zip64([dict(name=b"head", data=Z.text(100, 1)), dict(name=b"three.bin", data=data, level=6), dict(name=b"raw.bin", data=data, method=0)], always=True)
    ix = R.index(z, 16)
    for e in (1, 2):
        inflate_call(engine, ("3 MiB", e), z, 16, e, 1, in_len=ix["entries"][e]["csize"] + 6, mis=e)


# ---- hdlz_zip64_write_ws, as tests/test_gpu_zip_write_containment.py guards hdlz_zip_write_ws: the rows are the CPU oracle's; of a row
# only the bytes [2, d_len - 4) of a DEFLATED entry are put into the arena, of the input only the bytes of a STORED entry, of the names
# exactly their bytes -- everything else is the pattern in one run and its complement in the other
def write_call(engine, label, case, zip64_from, cap_delta=0, out_align=1, mis=(0, 0, 0, 0), entries=True):
    import joined_ref as J
    import zip_write_ref as W
    from hdl_deflate_amd.zip import ENTRY64_DTYPE
    L = engine.lib
    items, block = case["items"], case["block"]
    w = R.expected(items, zip64_from, block=block, store=case["store"], out_align=out_align)
    raw, flags = W.encode_names([n for n, _ in items])
    E = len(items)
    ent_off, name_off, blk_first, in_off, rows = [0], [0], [0], [0], []
    for e, (_, data) in enumerate(items):
        data = bytes(data)
        ent_off.append(ent_off[-1] + len(data))
        name_off.append(name_off[-1] + len(raw[e]))
        for a, ln in W.plan(len(data), block, bool(case["store"] and case["store"][e])):
            z, end_bit, _, _ = J.member_of(data[a:a + ln], 32, 10)
            rows.append((z, end_bit, w.methods[e] == 8))
            in_off.append(in_off[-1] + ln)
        blk_first.append(len(rows))
    B = len(rows)
    pitch = max([len(z) for z, _, _ in rows] + [4]) + 5
    cap = len(w.file) + cap_delta
    wb = L.hdlz_zip64_write_work_bytes(E, B)
    assert wb == R.write_work_bytes(E, B)
    words = lambda v: np.array(v, np.uint64).tobytes()
    specs = [("in", ent_off[-1], 16, BAND, True, mis[0]), ("ent_off", 8 * (E + 1), 8, BAND, True), ("names", name_off[-1], 16, BAND, True, mis[1]),
             ("name_off", 8 * (E + 1), 8, BAND, True), ("in_off", 8 * (B + 1), 8, BAND, True), ("rows", B * pitch, 16, BAND, True, mis[2]),
             ("len", 4 * B, 4, BAND, True), ("end_bits", 8 * B, 8, BAND, True), ("status", 4 * B, 4, BAND, True), ("blk_first", 8 * (E + 1), 8, BAND, True),
             ("crc", 4 * E, 4, BAND, True), ("file", cap, 16, max(BAND, 2 * cap), False, mis[3]), ("entries", 64 * E, 8, BAND), ("result", 40, 8, BAND),
             ("work", wb, 8, C.WORK_BAND)]

    def setup(a):
        for e, (_, data) in enumerate(items):
            if w.methods[e] == 0:
                a.fill("in", bytes(data), ent_off[e])
        a.fill("names", b"".join(raw))
        for k, v in (("ent_off", ent_off), ("name_off", name_off), ("in_off", in_off), ("blk_first", blk_first), ("end_bits", [r[1] for r in rows])):
            a.fill(k, words(v))
        a.fill("len", np.array([len(r[0]) for r in rows], np.uint32).tobytes())
        a.fill("status", bytes(4 * B))
        a.fill("crc", np.array([en["crc"] for en in w.entries], np.uint32).tobytes())
        image = a.view("rows").cpu().numpy().copy()
        for b, (z, _, deflated) in enumerate(rows):
            if deflated:
                image[b * pitch + 2:b * pitch + len(z) - 4] = np.frombuffer(z[2:len(z) - 4], np.uint8)
        a.fill("rows", image)

    def call(a):
        rc = L.hdlz_zip64_write_ws(a.ptr("in"), a.ptr("ent_off"), a.ptr("names"), a.ptr("name_off"), E, a.ptr("in_off") if B else None,
                                   a.ptr("rows") if B else None, pitch, a.ptr("len") if B else None, a.ptr("end_bits") if B else None,
                                   a.ptr("status") if B else None, B, a.ptr("blk_first"), a.ptr("crc"), flags, W.dos_datetime(W.DATE_TIME), out_align,
                                   zip64_from, ent_off[-1], a.ptr("file") if cap else None, cap, a.ptr("entries") if entries else None, a.ptr("result"),
                                   a.ptr("work"), wb, C.stream_ptr())
        assert rc == 0, (label, L.hdlz_last_error())

    a, clean, runs = C.two_runs(specs, setup, call, ("file", "entries", "result"))
    fits = cap >= len(w.file)
    for r in runs:
        res = np.frombuffer(r["result"].tobytes(), np.uint64)
        st = np.frombuffer(r["result"].tobytes(), np.uint32)[8:]
        assert [int(x) for x in res[:4]] == [w.record[k] for k in ("file_len", "cd_off", "cd_size", "nstored")], (label, res)
        assert (int(st[0]), int(st[1])) == (Z.OK if fits else Z.E_OUT_CAPACITY, R.ONES32), (label, st)
        if fits:
            assert r["file"][:len(w.file)].tobytes() == w.file, (label, "the file")
        if entries:
            got = np.frombuffer(r["entries"].tobytes(), ENTRY64_DTYPE)
            assert [tuple(int(g[f]) for f in Z.FIELDS) for g in got] == Z.records(dict(entries=w.entries)), label
            assert not got["reserved"].any() and not got["reserved2"].any(), label
    allowed = {"result": True, "work": True}
    if fits:
        allowed["file"] = len(w.file)
    if entries:
        allowed["entries"] = True
    bad = guards.violations(a, clean, allowed)
    assert bad == [], (label, bad)
    parts = a.split(clean)
    assert not bool(parts["result"][1].any()), (label, "the record was not written")
    if fits:
        assert not bool(parts["file"][1][:len(w.file)].any()), (label, "a byte of the file was not written")
    if entries and E:
        assert not bool(parts["entries"][1].any()), (label, "a record was not written")


def test_the_writer_stays_inside_the_file(engine):
    """every buffer of bytes at an odd address; zip64_from = 0 (every extra), a value between (some), FFFFFFFF (none); a file that does
    not fit is not begun; 3000 entries (three to a thread of the plan) and 65536 rows (256 tiles of the scan)"""
    import zip_write_ref as W
    case = lambda label: {c["label"]: c for c in W.all_cases()}[label]
    alt = case("the forms alternating")
    write_call(engine, "alternating, always", alt, 0, mis=(3, 5, 7, 9))
    write_call(engine, "alternating, between", alt, R.between(alt["label"]), cap_delta=100, out_align=64, mis=(1, 0, 2, 0))
    write_call(engine, "alternating, standard, no records", alt, R.ONES32, entries=False, mis=(0, 15, 1, 15))
    for delta in (-1, None):
        n = len(R.written(alt["label"], 0).file)
        write_call(engine, ("alternating, always, does not fit", delta), alt, 0, cap_delta=-n if delta is None else delta, mis=(3, 1, 4, 1))
    for mis in (0, 7, 15):
        write_call(engine, ("names of 1 to 16", mis), case("names of 1 to 16 bytes"), R.between("names of 1 to 16 bytes"), mis=(mis, 15 - mis, mis, mis))
    write_call(engine, "long names", case("names of 300 and 65535 bytes"), 0, mis=(1, 3, 5, 7))
    write_call(engine, "1 .. 600 blocks", case("1 .. 600 blocks at block 32"), R.between("1 .. 600 blocks at block 32"), mis=(9, 0, 3, 5))
    write_call(engine, "no entry", case("no entry"), 0)
    many = dict(case("65535 empty entries"), items=case("65535 empty entries")["items"][:3000])
    write_call(engine, "3000 empty entries", many, 0, mis=(0, 7, 0, 2))
    big = dict(label="stored tiles", items=[("a", Z.noise(200000, 1)), ("b", b""), ("c", Z.noise(65536, 2)), ("d", Z.noise(65537, 3)), ("e", W.soft(5000, 4))],
               block=2048, store=[True, False, True, True, False])
    write_call(engine, "stored entries of several tiles", big, 70000, mis=(13, 2, 6, 11))
    write_call(engine, "65536 rows", W.shape_case("65536 rows across the seams"), 100000, mis=(3, 5, 7, 9))
