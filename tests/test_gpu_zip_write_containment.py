"""GPU (-m gpu): hdlz_zip_write_ws inside guard bands (tests/guards.py), in the manner of tests/test_gpu_zip_containment.py: every
buffer of the call carved out of one patterned arena, each case run on the pattern and on its complement.

The rows are the CPU oracle's (joined_ref.member_of), not a device compress: of a row only the bytes [2, d_len - 4) of a DEFLATED
entry are put into the arena, of the input only the bytes of a STORED entry, of the names exactly their bytes.  Everything else -- the
rows of stored entries, the input of deflated entries, the two header bytes and the trailer of every row and what lies behind it up to
the pitch, the bytes around the names, the initial content of the file, the records, the record and the scratch -- is the pattern in
one run and its complement in the other, so a result that is the rule's in both runs depends on none of it.

  bands and read-only regions untouched; written: d_file[0 .. file_len) when it fits (no byte when it does not), d_entries[0 .. E),
  the record, d_work only inside what was passed."""
import numpy as np
import pytest
import torch

import guards
import joined_ref as J
import zip_ref as Z
import zip_write_ref as W
import test_gpu_containment as C

pytestmark = pytest.mark.gpu
BAND = 1 << 16


def write_call(engine, label, case, cap_delta=0, out_align=1, mis=(0, 0, 0, 0), entries=True):
    L = engine.lib
    items, block = case["items"], case["block"]
    w = W.expected(items, block=block, store=case["store"], out_align=out_align)
    raw, flags = W.encode_names([n for n, _ in items])
    E = len(items)
    # the batch as Engine.compress_zip plans it, the rows from the oracle
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
    pitch = max([len(z) for z, _, _ in rows] + [4]) + 5           # (no multiple of anything: rows at every alignment)
    cap = len(w.file) + cap_delta
    wb = L.hdlz_zip_write_work_bytes(E, B)
    words = lambda v: np.array(v, np.uint64).tobytes()
    specs = [("in", ent_off[-1], 16, BAND, True, mis[0]), ("ent_off", 8 * (E + 1), 8, BAND, True), ("names", name_off[-1], 16, BAND, True, mis[1]),
             ("name_off", 8 * (E + 1), 8, BAND, True), ("in_off", 8 * (B + 1), 8, BAND, True), ("rows", B * pitch, 16, BAND, True, mis[2]),
             ("len", 4 * B, 4, BAND, True), ("end_bits", 8 * B, 8, BAND, True), ("status", 4 * B, 4, BAND, True), ("blk_first", 8 * (E + 1), 8, BAND, True),
             ("crc", 4 * E, 4, BAND, True), ("file", cap, 16, max(BAND, 2 * cap), False, mis[3]), ("entries", 48 * E, 8, BAND), ("result", 40, 8, BAND),
             ("work", wb, 8, C.WORK_BAND)]

    def setup(a):
        for e, (_, data) in enumerate(items):
            if w.methods[e] == 0:
                a.fill("in", bytes(data), ent_off[e])             # (a deflated entry's input stays the pattern)
        a.fill("names", b"".join(raw))
        for k, v in (("ent_off", ent_off), ("name_off", name_off), ("in_off", in_off), ("blk_first", blk_first), ("end_bits", [r[1] for r in rows])):
            a.fill(k, words(v))
        a.fill("len", np.array([len(r[0]) for r in rows], np.uint32).tobytes())
        a.fill("status", bytes(4 * B))
        a.fill("crc", np.array([en["crc"] for en in w.entries], np.uint32).tobytes())
        image = a.view("rows").cpu().numpy().copy()              # the pattern, put back in ONE copy with the rows' bytes in it
        for b, (z, _, deflated) in enumerate(rows):
            if deflated:
                image[b * pitch + 2:b * pitch + len(z) - 4] = np.frombuffer(z[2:len(z) - 4], np.uint8)      # (78 9C, the Adler-32 and a stored entry's rows stay the pattern)
        a.fill("rows", image)

    def call(a):
        rc = L.hdlz_zip_write_ws(a.ptr("in"), a.ptr("ent_off"), a.ptr("names"), a.ptr("name_off"), E, a.ptr("in_off") if B else None,
                                 a.ptr("rows") if B else None, pitch, a.ptr("len") if B else None, a.ptr("end_bits") if B else None,
                                 a.ptr("status") if B else None, B, a.ptr("blk_first"), a.ptr("crc"), flags, W.dos_datetime(W.DATE_TIME), out_align,
                                 ent_off[-1], a.ptr("file") if cap else None, cap, a.ptr("entries") if entries else None, a.ptr("result"), a.ptr("work"),
                                 wb, C.stream_ptr())
        assert rc == 0, (label, L.hdlz_last_error())

    a, clean, runs = C.two_runs(specs, setup, call, ("file", "entries", "result"))
    fits = cap >= len(w.file)
    from hdl_deflate_amd.zip import ENTRY_DTYPE
    for r in runs:
        res = np.frombuffer(r["result"].tobytes(), np.uint64)
        st = np.frombuffer(r["result"].tobytes(), np.uint32)[8:]
        assert [int(x) for x in res[:4]] == [w.record[k] for k in ("file_len", "cd_off", "cd_size", "nstored")], (label, res)
        assert (int(st[0]), int(st[1])) == (W.OK if fits else W.E_OUT_CAPACITY, W.NONE), (label, st)
        if fits:
            assert r["file"][:len(w.file)].tobytes() == w.file, (label, "the file")
        if entries:
            got = np.frombuffer(r["entries"].tobytes(), ENTRY_DTYPE)
            assert [tuple(int(g[f]) for f in Z.FIELDS) for g in got] == Z.records(dict(entries=w.entries)) and not got["reserved"].any(), label
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


def _case(label):
    return {c["label"]: c for c in W.all_cases()}[label]


def test_the_writer_stays_inside_the_file(engine):
    """deflated and stored entries alternating, entries without blocks, empty ones; every buffer of bytes at an odd address"""
    write_call(engine, "alternating", _case("the forms alternating"), mis=(3, 5, 7, 9))
    write_call(engine, "alternating, room behind the file", _case("the forms alternating"), cap_delta=100, out_align=64, mis=(1, 0, 2, 0))
    write_call(engine, "alternating, no records", _case("the forms alternating"), entries=False, mis=(0, 15, 1, 15))
    write_call(engine, "store=", _case("store= entries"), mis=(11, 1, 13, 4))
    write_call(engine, "ties", _case("ties: c - u of -1, 0 and +1"), mis=(2, 2, 2, 2))
    write_call(engine, "sizes", _case("sizes 0 .. 49 at block 32"), mis=(6, 3, 9, 12))
    write_call(engine, "incompressible", _case("incompressible entries with blocks"), mis=(5, 0, 0, 1))


def test_payloads_at_every_residue_and_long_names(engine):
    for mis in (0, 1, 7, 8, 15):
        write_call(engine, ("names of 1 to 16", mis), _case("names of 1 to 16 bytes"), mis=(mis, 15 - mis, mis, mis))
    write_call(engine, "long names", _case("names of 300 and 65535 bytes"), mis=(1, 3, 5, 7))
    write_call(engine, "a UTF-8 name", _case("a name that is not ASCII"), mis=(0, 1, 0, 3))


def test_tiles_of_rows_and_entry_counts(engine):
    write_call(engine, "1 .. 600 blocks", _case("1 .. 600 blocks at block 32"), mis=(9, 0, 3, 5))
    write_call(engine, "no entry", _case("no entry"))
    write_call(engine, "one entry", _case("one entry"), mis=(1, 1, 1, 1))
    many = dict(_case("65535 empty entries"), items=_case("65535 empty entries")["items"][:3000])
    write_call(engine, "3000 empty entries", many, mis=(0, 7, 0, 2))
    big = dict(label="stored tiles", items=[("a", Z.noise(200000, 1)), ("b", b""), ("c", Z.noise(65536, 2)), ("d", Z.noise(65537, 3)), ("e", W.soft(5000, 4))],
               block=2048, store=[True, False, True, True, False])
    write_call(engine, "stored entries of several tiles", big, mis=(13, 2, 6, 11))


def test_many_tiles_and_rowless_runs(engine):
    """zip_write_ref.shape_cases(): 65536 rows -- 256 tiles of the scan, so pre[0 .. B], cnt[0 .. B] and the look-back words of more
    than one window, and the gather with 256 rows a workgroup -- and the runs of entries without rows, where a lane searches alone;
    a write outside the scratch passed, which the file's bytes cannot show, is a violation here"""
    write_call(engine, "65536 rows", W.shape_case("65536 rows across the seams"), mis=(3, 5, 7, 9))
    write_call(engine, "rowless runs", W.shape_case("rowless runs of 62 to 200 entries"), mis=(1, 7, 5, 3))


def test_a_file_that_does_not_fit_is_not_begun(engine):
    for delta in (-1, -22, None):
        case = _case("the forms alternating")
        n = len(W.written(case["label"]).file)
        write_call(engine, ("alternating", delta), case, cap_delta=-n if delta is None else delta, mis=(3, 1, 4, 1))
