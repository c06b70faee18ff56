"""GPU (-m gpu): hdlz_zip64_index_ws / hdlz_zip64_inflate_ws / Engine.zip_index(zip64=) / Engine.inflate_zip / load_npz on ZIP64 files, and
(the second half) hdlz_zip64_write_ws / Engine.compress_zip(zip64=) / save_npz against THE FILE RULE of zip64_ref.expected.

The archives are those of tests/zip64_ref.py (hand-built ones and zipfile's, fixed seeds); what the index and every entry must answer is
zip64_ref.index and zip_ref.judge, the rule of include/hdlz_zip64.h in Python, which tests/test_zip64_cabi.py holds against zipfile,
unzip and numpy on the same archives.  For every case the records and the result are compared with the rule, then the entries are read
and compared.  Five cases are files of more than 4 GiB that never leave the device, one read and four written: only real sizes catch a truncated 64-bit value."""
import io
import struct
import zipfile
import zlib

import numpy as np
import pytest
import torch

import zip_ref as Z
import zip64_ref as R

pytestmark = pytest.mark.gpu


def _whole(engine, label, z, out_align=1, zip64=True):
    """index the file by the new call and read it twice -- ONE call over all entries and as Engine.inflate_zip routes it"""
    d = Z.stage(z)
    zi = engine.zip_index(d, out_align=out_align, zip64=zip64)
    ix = R.check_index(label, z, zi, out_align)
    _, sts, flat = R.read(z, out_align)
    n = ix["nentries"]
    if n:
        out, out_off, status, rec = R.run_inflate(engine, d, zi, 0, n)
        Z.check_read((label, "one call"), z, ix, sts, flat, 0, out, out_off, status)
        bad = [k for k, s in enumerate(sts) if s != Z.OK]
        assert (rec.status, rec.first_bad) == ((Z.OK, 2 ** 64 - 1) if not bad else (int(status[bad[0]]) & 0xFFFFFFFF, bad[0])), (label, rec.status, rec.first_bad)
        assert rec.out_len == (ix["total_out"] if not bad else 0)
    out, out_off, status = engine.inflate_zip(d, zi)
    Z.check_read((label, "routed"), z, ix, sts, flat, 0, out, out_off, status)
    return d, zi, ix, sts, flat


@pytest.mark.parametrize("label", [c[0] for c in R.crafted_cases()])
def test_crafted_zip64_files(engine, label):
    """0, 1 and 3 entries in the "always" layout; all 16 subsets of {usize, csize, L, disk} all ones, the field supplying exactly those;
    the field in front of, between and behind other fields; a comment; an extensible data sector; true classic values beside a locator"""
    z = dict(R.crafted_cases())[label]
    d, zi, ix, sts, flat = _whole(engine, label, z)
    assert sts == [Z.OK] * len(sts) and zi.record.status == Z.OK
    assert zi.names == [i.orig_filename for i in zipfile.ZipFile(io.BytesIO(z)).infolist()]
    auto = engine.zip_index(d)                                   # a file below 4 GiB: the classic call first
    if Z.index(z)["status"] != Z.OK:                             # ... and the new one where that failed in step 1 (the locator)
        assert auto.zip64 and auto.host.tobytes() == zi.host.tobytes()
    else:                                                       # the classic call answered: what it always returned
        assert not auto.zip64 and Z.check_index(label, z, auto) is not None
    if len(sts) == 3:
        for e in range(3):                                       # every entry alone: the one-stream route
            out, out_off, status, rec = R.run_inflate(engine, d, zi, e, 1, int(zi.host["csize"][e]) + 6)
            Z.check_read((label, "alone", e), z, ix, sts, flat, e, out, out_off, status)
            assert rec.status == Z.OK and rec.out_len == ix["entries"][e]["usize"]


@pytest.mark.parametrize("label", [c[0] for c in R.many_cases()])
def test_more_entries_than_a_classic_directory_holds(engine, label):
    """zipfile's files of 65535 (no locator), 65536 and 65537 entries; 131073 crafted ones, two windows of 65536 in the walk and the
    scan; the sizing call, entry_cap = nentries - 1 and nentries"""
    z = dict(R.many_cases())[label]
    d = Z.stage(z)
    ix = R.index(z)
    n = ix["nentries"]
    assert ix["status"] == Z.OK and n == int(label.split()[1])
    auto = engine.zip_index(d)
    assert auto.zip64 == (n > 65535) and auto.record.nentries == n and auto.record.status == Z.OK
    zi = engine.zip_index(d, zip64=True)
    R.check_index(label, z, zi, ix=ix)
    assert zi.names[-1] == "%06d" % (n - 1) and zi.names[65534] == "065534"
    for cap in (0, n - 1, n):
        zc = engine.zip_index(d, entry_cap=cap, zip64=True)
        R.check_index((label, "entry_cap", cap), z, zc, 1, cap)
        assert zc.record.status == (Z.OK if cap == n else Z.E_OUT_CAPACITY) and len(zc.host) == cap and zc.record.nentries == n
    R.check_index((label, "out_align 64"), z, engine.zip_index(d, out_align=64, zip64=True), 64)
    _, sts, flat = R.read(z)
    first = n - 5000                                              # a range behind entry 65536 where there is one
    out, out_off, status = engine.inflate_zip(d, zi, first, 5000)
    Z.check_read((label, "the last 5000"), z, ix, sts, flat, first, out, out_off, status)
    assert any(ix["entries"][k]["usize"] for k in range(first, n))


def test_records_straddle_the_staging_piece_at_every_residue(engine):
    """a central record of 46 + 4 + 28 bytes, the ZIP64 field its last 28, starting 0 to 78 bytes in front of the first 16 KiB piece's end"""
    for k in R.STRADDLES:
        z = R.straddle_case(k)
        d = Z.stage(z)
        zi = engine.zip_index(d, zip64=True)
        ix = R.check_index(("straddle", k), z, zi)
        assert zi.record.status == Z.OK and [e["status"] for e in ix["entries"]] == [Z.OK] * 3
        if k % 13 == 0:
            _whole(engine, ("straddle", k), z)


@pytest.mark.parametrize("label", [c[0] for c in Z.all_archives()])
def test_files_without_zip64_read_as_by_the_classic_call(engine, label):
    """every archive of zip_ref through the new call: the classic call's records widened, the same result record, the same bytes read"""
    z = dict(Z.all_archives())[label]
    d = Z.stage(z)
    for align in (1, 16):
        old, new = engine.zip_index(d, out_align=align, zip64=False), engine.zip_index(d, out_align=align, zip64=True)
        assert not old.zip64 and new.zip64
        R.check_index(label, z, new, align)
        if label == "a ZIP64 locator":                           # (the classic rule refuses the locator itself; the new one what it points at)
            assert old.record.status == new.record.status == Z.E_BAD_HEADER
            continue
        assert bytes(old.record) == bytes(new.record), label
        for f in Z.FIELDS:
            assert np.array_equal(old.host[f].astype(np.uint64), new.host[f].astype(np.uint64)), (label, f)
        assert old.names == new.names
    if len(new.host) and len(new.host) <= 1000:
        a, b = engine.inflate_zip(d, old), engine.inflate_zip(d, new)
        assert torch.equal(a[2], b[2]) and torch.equal(a[1], b[1]), label
        ok = (a[2] == 0).cpu().numpy()
        for k in np.nonzero(ok)[0]:
            o, u = int(a[1][k]), int(old.host["usize"][k])
            assert torch.equal(a[0][o:o + u], b[0][o:o + u]), (label, k)


@pytest.mark.parametrize("k", range(len(R.bad_cases())), ids=[c[0] for c in R.bad_cases()])
def test_one_edit_away_from_a_good_file(engine, k):
    """the damaged end records: the status and the zeroed record; the damaged fields: exactly that entry fails, its neighbours read"""
    label, z, want, kept, e = R.bad_cases()[k]
    d, zi, ix, sts, flat = _whole(engine, label, z)
    r = zi.record
    assert (r.status, r.nentries, len(zi.host)) == (want, kept, kept)
    if not kept:
        assert (r.total_out, r.cd_off, r.cd_size, r.reserved) == (0, 0, 0, 0)
        assert engine.zip_index(d).record.status == want          # ("auto": both calls refuse it)
    else:
        assert [int(s) != Z.OK for s in zi.host["status"]] == [j == e for j in range(kept)] and int(zi.host["status"][e]) == Z.E_BAD_HEADER
        assert int(zi.host["payload_off"][e]) == 0
        status, files = engine.read_zip_bytes(z)
        assert status == Z.E_BAD_HEADER and sorted(files) == ["first.txt", "third.txt"] and files["third.txt"] == R.three_items()[2]["data"]


def test_load_npz_reads_a_zip64_npz(engine):
    """load_npz needs nothing but what the index gives it: numpy.savez's layout once it passes the limits (every size and offset in the
    ZIP64 field), stored and deflated"""
    from hdl_deflate_amd import load_npz
    arrays = dict(a=np.arange(5000, dtype=np.int64), b=np.linspace(0, 1, 3000, dtype=np.float32), e=np.frombuffer(Z.text(40000, 5), np.uint8).reshape(200, 200))
    items = []
    for j, (name, a) in enumerate(arrays.items()):
        buf = io.BytesIO()
        np.lib.format.write_array(buf, a)
        items.append(dict(name=name.encode() + b".npy", data=buf.getvalue(), method=(0, 8, 8)[j]))
    z = R.make_zip64(items, always=True)
    want = np.load(io.BytesIO(z))
    got = load_npz(engine, z)
    assert sorted(got) == sorted(arrays)
    for name in arrays:
        assert np.array_equal(got[name].cpu().numpy(), want[name]), name


def _crafted_records(rows):
    from hdl_deflate_amd.zip import ENTRY64_DTYPE
    recs = np.zeros(len(rows), ENTRY64_DTYPE)
    for k, row in enumerate(rows):
        for f, v in row.items():
            recs[f][k] = v
    return torch.from_numpy(recs.view(np.int64).reshape(len(rows), 8).copy()).cuda()


def test_past_four_gib(engine):
    """ONE file of 2^32 + 5 + a few hundred bytes, built and verified on the device: a stored entry of 2^32 + 5 random bytes (usize and
    csize in the ZIP64 field; read back by the count == 1 route: the flat copy and the tile CRC) and behind it a deflated and a stored
    small entry whose local offsets, like cd_off, lie behind 2^32.  The tail is parsed by zip64_ref from slices copied to the host, and
    zipfile opens the device tensor through a file-like view: infolist() and read() of the small entries are a stock reader's CRC
    check on bytes behind the 4 GiB mark.  The big entry's CRC word is Engine.crc32's, which is pinned elsewhere.  Then the limits of
    hdlz_zip64_inflate_ws on records by hand, in the buffers this test has anyway."""
    n = (1 << 32) + 5
    g = torch.Generator(device="cuda").manual_seed(64)
    big = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
    crc = int(engine.crc32(big).cpu()[0])
    small = [(b"small.txt", Z.text(3000, 71), 8), (b"raw.bin", Z.noise(500, 72), 0)]
    head = Z.SIG_LOCAL + struct.pack("<HHHHHIIIHH", 45, 0, 0, 0, 0x21, crc, R.ONES32, R.ONES32, 7, 20) + b"big.bin" + R.field(1, struct.pack("<QQ", n, n))
    cd = Z.SIG_CD + struct.pack("<HHHHHHIIIHHHHHII", 45, 45, 0, 0, 0, 0x21, crc, R.ONES32, R.ONES32, 7, 20, 0, 0, 0, 0, 0) + b"big.bin" + \
        R.field(1, struct.pack("<QQ", n, n))
    tail, off = b"", len(head) + n
    for name, data, method in small:
        raw = Z.deflate(data) if method else data
        cd += Z.SIG_CD + struct.pack("<HHHHHHIIIHHHHHII", 45, 45, 0, method, 0, 0x21, zlib.crc32(data), len(raw), len(data), len(name), 12, 0, 0, 0, 0,
                                     R.ONES32) + name + R.field(1, struct.pack("<Q", off + len(tail)))
        tail += Z.SIG_LOCAL + struct.pack("<HHHHHIIIHH", 20, 0, method, 0, 0x21, zlib.crc32(data), len(raw), len(data), len(name), 0) + name + raw
    cd_off = off + len(tail)
    tail += cd + R.SIG_END64 + struct.pack("<QHHIIQQQQ", 44, 45, 45, 0, 0, 3, 3, len(cd), cd_off) + Z.SIG_LOCATOR + struct.pack("<IQI", 0, cd_off + len(cd), 1)
    tail += Z.SIG_EOCD + struct.pack("<HHHHIIH", 0, 0, 3, 3, len(cd), R.ONES32, 0)          # ("equal or all ones": only cd_off needs the ZIP64 value)
    d = torch.empty(len(head) + n + len(tail) + 64, dtype=torch.uint8, device="cuda")[:len(head) + n + len(tail)]
    d[:len(head)] = torch.frombuffer(bytearray(head), dtype=torch.uint8).cuda()
    d[len(head):len(head) + n] = big
    d[len(head) + n:] = torch.frombuffer(bytearray(tail), dtype=torch.uint8).cuda()
    assert cd_off > 1 << 32 and d.numel() > 1 << 32

    zi = engine.zip_index(d, out_align=16)                      # "auto": a file of 2^32 bytes or more goes to the new call
    assert zi.zip64
    ix = R.check_index("past 4 GiB", R.DeviceBytes(d), zi, 16)
    assert zi.record.status == Z.OK and [int(s) for s in zi.host["status"]] == [Z.OK] * 3 and zi.names == ["big.bin", "small.txt", "raw.bin"]
    assert [int(x) for x in zi.host["usize"]] == [n, 3000, 500] and int(zi.host["payload_off"][0]) == len(head) and int(zi.host["payload_off"][1]) > 1 << 32
    zf = zipfile.ZipFile(R.DeviceFile(d))
    infos = zf.infolist()
    assert [(i.orig_filename, i.file_size, i.compress_size, i.CRC) for i in infos] == \
        [(nm, int(u), int(c), int(k)) for nm, u, c, k in zip(zi.names, zi.host["usize"], zi.host["csize"], zi.host["crc"])]
    assert [i.header_offset for i in infos] == [0, off, off + 30 + 9 + int(zi.host["csize"][1])] and zf.start_dir == cd_off
    for info, (name, data, method) in zip(infos[1:], small):
        assert zf.read(info) == data

    out, out_off, status = engine.inflate_zip(d, zi)
    assert [int(s) for s in status.cpu()] == [Z.OK] * 3 and [int(o) for o in out_off.cpu()] == [int(o) for o in zi.host["out_off"]]
    assert torch.equal(out[:n], big)
    for k, (name, data, method) in enumerate(small, 1):
        o = int(out_off[k])
        assert out[o:o + len(data)].cpu().numpy().tobytes() == data, name
    # one flipped byte behind the 4 GiB mark of the big entry fails its CRC
    at = len(head) + (1 << 32) + 2
    d[at] ^= 1
    out2, off2, status2, rec = R.run_inflate(engine, d, zi, 0, 1, 0)
    assert int(status2[0]) == Z.E_BAD_CHECKSUM and rec.first_bad == 0
    d[at] ^= 1
    del out2

    # the stated limits, on records by hand (nothing of these entries is decoded): a slot of 2^32 bytes or more in a call of several
    # entries or at an odd d_out; a deflated slot above 2^32 - 512; a deflated payload above 2^28 - 7
    from hdl_deflate_amd import _lib
    base = dict(cd_off=cd_off, payload_off=len(head), crc=crc, status=0)
    recs = _crafted_records([dict(base, csize=n, usize=n, method=0, out_off=0), dict(base, csize=100, usize=(1 << 32) + 5, method=8, out_off=0),
                             dict(base, csize=(1 << 28) - 6, usize=1000, method=8, out_off=0), dict(base, csize=10, usize=10, method=0, out_off=n + 11)])
    st = torch.zeros(4, dtype=torch.int32, device="cuda")

    def call(first, count, o=out, cap=out.numel()):
        need = engine.lib.hdlz_zip64_inflate_work_bytes(count, 0, cap)
        r = engine._record("hdlz_zip64_inflate_ws", _lib.ZipInflateResult, engine._scratch(need, None), d.data_ptr(), d.numel(), recs.data_ptr(), first,
                           count, 0, o.data_ptr(), cap, st.data_ptr())
        return r.status, [int(s) for s in st[:count].cpu()]

    assert out.numel() >= n + 3
    assert call(1, 1) == (Z.E_OUT_CAPACITY, [Z.E_OUT_CAPACITY])
    assert call(2, 1) == (Z.E_BAD_PARAM, [Z.E_BAD_PARAM])
    assert call(0, 1, out[1:], out.numel() - 1) == (Z.E_BAD_PARAM, [Z.E_BAD_PARAM])          # no row for the one-stream path
    spare = torch.empty(n + 32, dtype=torch.uint8, device="cuda")
    rs, sts = call(0, 4, spare, n + 21)                          # several entries: the big one is refused, the small stored one behind it is read
    assert (rs, sts[:3]) == (Z.E_BAD_PARAM, [Z.E_BAD_PARAM, Z.E_OUT_CAPACITY, Z.E_BAD_PARAM]) and sts[3] == Z.E_BAD_CHECKSUM


# ---- the writer: hdlz_zip64_write_ws through Engine.compress_zip(zip64=), against THE FILE RULE as zip64_ref.expected states it
import zip_write_ref as W                 # noqa: E402
from test_gpu_zip_write import _stage     # noqa: E402

WRITE_CASES = {c["label"]: c for c in W.all_cases()}


def _write(engine, case, zip64, out_align=1, **kw):
    items = case["items"]
    return engine.compress_zip(_stage(items), [len(d) for _, d in items], [n for n, _ in items], block=case["block"], store=case["store"],
                               out_align=out_align, zip64=zip64, **kw)


def _read_back(engine, label, items, out, index, out_align):
    """the writer's records are the index call's for the written file (rule 7), and Engine.zip_index / Engine.inflate_zip read it back"""
    zi = engine.zip_index(out, out_align=out_align, zip64=True)
    assert zi.record.status == Z.OK and len(zi.host) == len(index.host), label
    for f in Z.FIELDS:                                            # (by field: an index of the classic writer has the 48-byte records)
        assert np.array_equal(zi.host[f].astype(np.uint64), index.host[f].astype(np.uint64)), (label, f)
    assert (zi.record.nentries, zi.record.total_out, zi.record.cd_off, zi.record.cd_size) == \
        (index.record.nentries, index.record.total_out, index.record.cd_off, index.record.cd_size), label
    assert zi.names == [n for n, _ in items] == index.names, label
    auto = engine.zip_index(out, out_align=out_align)
    assert auto.record.status == Z.OK and auto.names == zi.names, label
    data, off, status = engine.inflate_zip(out, auto)
    assert bool((status == Z.OK).all()), (label, status.cpu().numpy()[:20])
    data, off = data.cpu().numpy(), off.cpu().numpy()
    for k in range(0, len(items), max(1, len(items) // 200)):
        assert data[off[k]:off[k] + len(items[k][1])].tobytes() == bytes(items[k][1]), (label, k)


@pytest.mark.parametrize("label", list(WRITE_CASES))
def test_at_the_standard_value_the_file_is_the_classic_writers(engine, label):
    """zip64_from = FFFFFFFF: byte for byte what hdlz_zip_write_ws writes, and its records widened"""
    case = WRITE_CASES[label]
    for out_align in (1, 64):
        classic, cindex = _write(engine, case, "auto", out_align)
        out, index = _write(engine, case, 0xFFFFFFFF, out_align)
        assert not cindex.zip64 and index.zip64 and torch.equal(out, classic), label
        R.check_written(label, R.written(label, R.ONES32, out_align), out, index)
        assert bytes(index.write_record) == bytes(cindex.write_record), label
        for f in Z.FIELDS:
            assert np.array_equal(index.host[f].astype(np.uint64), cindex.host[f].astype(np.uint64)), (label, f)


@pytest.mark.parametrize("how", ("always", "between"))
@pytest.mark.parametrize("label", list(WRITE_CASES))
def test_the_file_with_zip64_fields_is_the_rules(engine, label, how):
    """zip64_from = 0, and a value between the case's smallest and largest size or offset (zip64_ref.between: local-only, offset-only
    and mixed extras all occur, which tests/test_zip64_cabi.py asserts from the reference's arrays)"""
    case = WRITE_CASES[label]
    zip64 = "always" if how == "always" else R.between(label)
    for out_align in (1, 64):
        out, index = _write(engine, case, zip64, out_align)
        R.check_written((label, how), R.written(label, 0 if how == "always" else zip64, out_align), out, index)
        _read_back(engine, (label, how), case["items"], out, index, out_align)
    zf = zipfile.ZipFile(io.BytesIO(out.cpu().numpy().tobytes()))
    assert [i.filename for i in zf.infolist()] == [n for n, _ in case["items"]] and (len(case["items"]) > 5000 or zf.testzip() is None)


@pytest.mark.parametrize("E", (65535, 65536, 131073))
def test_many_entries_written(engine, E):
    """"auto": 65535 entries are the classic call's (no ZIP64 end record), 65536 and 131073 the new one's, with the record and the locator"""
    items = R.many_items(E)
    case = dict(items=items, block=32, store=None)
    out, index = _write(engine, case, "auto")
    w = R.expected(items)
    assert index.zip64 == (E > 65535) == w.end64
    if index.zip64:
        R.check_written(E, w, out, index)
    else:
        W.check_written(E, W.expected(items), out, index)
        assert out.cpu().numpy().tobytes() == w.file
    _read_back(engine, E, items, out, index, 1)
    assert len(zipfile.ZipFile(io.BytesIO(w.file)).infolist()) == E


def _direct(engine, case, cap, zip64_from, out_align=1, tamper=None):
    """hdlz_zip64_write_ws itself over the case's batch, the file's buffer exactly `cap` bytes in front of a canary"""
    from hdl_deflate_amd.zip import ENTRY64_DTYPE
    items = case["items"]
    z = engine._zip_batch(_stage(items), [len(d) for _, d in items], [n for n, _ in items], case["block"], 32, 10, case["store"])
    z.zip64_from = zip64_from
    if tamper:
        tamper(z)
    buf = torch.full((cap + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    rec, res, back = engine._zip_write(z, buf[:cap], W.DATE_TIME, out_align)
    assert bool((buf[cap:] == 0x5A).all()), "bytes at or behind file_cap were written"
    return rec, buf, np.frombuffer(back.tobytes(), dtype=ENTRY64_DTYPE)


def test_write_capacity(engine):
    """file_cap = file_len, file_len - 1 and 0 (the sizing call): the true lengths, the records, and not a byte of a file that does not fit"""
    for label, f in (("the forms alternating", None), ("1 .. 600 blocks at block 32", 0), ("no entry", 0)):
        f = R.between(label) if f is None else f
        w = R.written(label, f)
        n = len(w.file)
        for cap in (n, n - 1, 0):
            rec, buf, ents = _direct(engine, WRITE_CASES[label], cap, f)
            want = dict(w.record, status=W.OK if cap >= n else W.E_OUT_CAPACITY)
            assert {k: getattr(rec, k) for k in want} == want, (label, cap)
            if cap >= n:
                assert buf[:n].cpu().numpy().tobytes() == w.file, (label, cap)
            else:
                assert bool((buf == 0x5A).all()), (label, cap, "an archive that does not fit is not begun")
            assert [tuple(int(r[k]) for k in Z.FIELDS) for r in ents] == Z.records(dict(entries=w.entries)), (label, cap)


def test_a_failing_block_still_fails_its_entry(engine):
    case = WRITE_CASES["1 .. 600 blocks at block 32"]              # entries own rows [0, 1, 256, 512, 515, 772, 1372)

    def two(z):
        z.status[600] = W.E_SHORT_INPUT                           # entry 4
        z.status[300] = Z.E_BAD_HEADER                            # entry 2: the larger status, the lower entry

    for f in (0, R.ONES32):
        rec, buf, ents = _direct(engine, case, len(R.written(case["label"], f).file), f, tamper=two)
        assert (rec.status, rec.first_bad, rec.file_len, rec.cd_off, rec.cd_size, rec.nstored) == (Z.E_BAD_HEADER, 2, 0, 0, 0, 0)
        assert [int(s) for s in ents["status"]] == [W.OK, W.OK, Z.E_BAD_HEADER, W.OK, W.E_SHORT_INPUT, W.OK]
        assert not ents["csize"].any() and not ents["payload_off"].any() and not ents["usize"].any()


def test_save_npz_with_zip64_always_is_what_numpy_loads(engine):
    from hdl_deflate_amd import load_npz, save_npz
    arrays = W.npz_arrays()
    tensors = {k: torch.from_numpy(np.array(v)).cuda() for k, v in arrays.items()}      # (np.array: a 0-d array stays 0-d)
    for compressed in (True, False):
        out = save_npz(engine, tensors, compressed=compressed, zip64="always")
        z = out.cpu().numpy().tobytes()
        assert z == R.expected(W.npz_items(arrays), 0, block=1 << 16, store=None if compressed else [True] * len(arrays)).file
        got = np.load(io.BytesIO(z))
        assert sorted(got.files) == sorted(arrays) and all(np.array_equal(got[k], v) for k, v in arrays.items())
        back = load_npz(engine, out)
        assert sorted(back) == sorted(arrays) and all(np.array_equal(back[k].cpu().numpy(), v) for k, v in arrays.items())
    assert engine.write_zip_bytes({"a.txt": Z.text(500, 1), "b": b""}, zip64="always") == R.expected([("a.txt", Z.text(500, 1)), ("b", b"")], 0, block=1 << 16).file


# ---- written past 4 GiB: only real sizes catch a truncated 64-bit value; the bulk bytes never leave the device
def _opened(out, index):
    """zipfile on the device tensor: its infolist against the writer's records -> (ZipFile, infos)"""
    zf = zipfile.ZipFile(R.DeviceFile(out))
    infos = zf.infolist()
    assert [(i.orig_filename, i.file_size, i.compress_size, i.CRC, i.compress_type) for i in infos] == \
        [(nm, int(u), int(c), int(k), int(m)) for nm, u, c, k, m in zip(index.names, index.host["usize"], index.host["csize"], index.host["crc"], index.host["method"])]
    assert zf.start_dir == index.record.cd_off
    return zf, infos


def test_written_offsets_past_four_gib(engine):
    """(a) two stored entries of 2^31 + 4096 bytes, then four small ones (two deflated), "auto": no size needs a ZIP64 field, the local
    offsets of the small entries and cd_off do"""
    n = (1 << 31) + 4096
    g = torch.Generator(device="cuda").manual_seed(65)
    small = [("s1.txt", W.soft(3000, 1)), ("r1.bin", Z.noise(500, 2)), ("s2.txt", W.soft(70000, 3)), ("tiny", b"abc")]
    tail = torch.frombuffer(bytearray(b"".join(d for _, d in small)), dtype=torch.uint8).cuda()
    d_in = torch.empty(2 * n + tail.numel(), dtype=torch.uint8, device="cuda")
    d_in[:2 * n] = torch.randint(0, 256, (2 * n,), dtype=torch.uint8, device="cuda", generator=g)
    d_in[2 * n:] = tail
    names = ["big0.bin", "big1.bin"] + [nm for nm, _ in small]
    out, index = engine.compress_zip(d_in, [n, n] + [len(d) for _, d in small], names, store=[True, True, False, False, False, False], out_align=16)
    assert index.zip64 and out.numel() > 1 << 32 and index.write_record.file_len == out.numel()
    host = index.host
    assert [int(m) for m in host["method"]] == [0, 0, 8, 0, 8, 0] and [int(u) for u in host["usize"]] == [n, n, 3000, 500, 70000, 3]
    L, want = 0, []
    for k, nm in enumerate(names):                              # no local extra anywhere: every size is below FFFFFFFF
        want.append(L + 30 + len(nm))
        L = want[-1] + int(host["csize"][k])
    assert [int(p) for p in host["payload_off"]] == want and L == index.record.cd_off > 1 << 32 and want[2] > 1 << 32
    assert int(host["crc"][0]) == int(engine.crc32(d_in[:n]).cpu()[0]) and int(host["crc"][1]) == int(engine.crc32(d_in[n:2 * n]).cpu()[0])
    ix = R.check_index("(a)", R.DeviceBytes(out), index, 16)     # the tail parsed by the index rule: the writer's records are its answer
    assert ix["status"] == Z.OK and [e["status"] for e in ix["entries"]] == [Z.OK] * 6
    zf, infos = _opened(out, index)
    assert [i.header_offset for i in infos] == [p - 30 - len(nm) for p, nm in zip(want, names)]
    assert [i.extract_version for i in infos] == [20, 20, 45, 45, 45, 45]      # the offset alone moved into the ZIP64 field
    for info, (nm, data) in zip(infos[2:], small):
        assert zf.read(info) == data, nm                         # a stock reader's CRC check on bytes behind the 4 GiB mark
    zi = engine.zip_index(out, out_align=16)
    assert zi.zip64 and zi.host.tobytes() == host.tobytes()
    back, off, status = engine.inflate_zip(out, zi)
    assert [int(s) for s in status.cpu()] == [Z.OK] * 6
    assert torch.equal(back[:n], d_in[:n]) and torch.equal(back[int(off[1]):int(off[1]) + n], d_in[n:2 * n])
    for k, (nm, data) in enumerate(small, 2):
        assert back[int(off[k]):int(off[k]) + len(data)].cpu().numpy().tobytes() == data, nm


def test_written_one_stored_entry_past_four_gib(engine):
    """(b) one stored entry of 2^32 + 5 bytes: usize and csize in both extras; read back by the count == 1 route"""
    n = (1 << 32) + 5
    g = torch.Generator(device="cuda").manual_seed(66)
    d_in = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
    out, index = engine.compress_zip(d_in, [n], ["big.bin"], store=[True], out_align=16)
    assert index.zip64 and index.write_record.nstored == 1 and out.numel() == 30 + 7 + 20 + n + 46 + 7 + 20 + 56 + 20 + 22
    assert (int(index.host["usize"][0]), int(index.host["csize"][0]), int(index.host["payload_off"][0])) == (n, n, 57)
    assert int(index.host["crc"][0]) == int(engine.crc32(d_in).cpu()[0])
    head = out[:57].cpu().numpy().tobytes()
    assert head[4:6] == b"\x2d\x00" and head[18:26] == b"\xff" * 8 and head[28:30] == b"\x14\x00" and head[37:] == struct.pack("<HHQQ", 1, 16, n, n)
    cd = out[57 + n:57 + n + 73].cpu().numpy().tobytes()
    assert cd[4:8] == b"\x2d\x00\x2d\x00" and cd[20:28] == b"\xff" * 8 and cd[30:32] == b"\x14\x00" and cd[42:46] == bytes(4) and \
        cd[53:] == struct.pack("<HHQQ", 1, 16, n, n)
    R.check_index("(b)", R.DeviceBytes(out), index, 16)
    zf, infos = _opened(out, index)
    assert infos[0].header_offset == 0 and infos[0].extract_version == 45
    zi = engine.zip_index(out, out_align=16)
    assert zi.zip64 and zi.host.tobytes() == index.host.tobytes()
    back, off, status = engine.inflate_zip(out, zi)
    assert int(status[0]) == Z.OK and torch.equal(back, d_in)


def test_written_one_deflated_entry_past_four_gib(engine):
    """(c) 2^32 + 5 zero bytes at blocks of 64 KiB, deflated: usize goes into the ZIP64 field and csize does not; reading it is the stated
    limit of hdlz_zip64_inflate_ws (a deflated slot above 2^32 - 512): HDLZ_E_OUT_CAPACITY"""
    n = (1 << 32) + 5
    d_in = torch.zeros(n, dtype=torch.uint8, device="cuda")
    out, index = engine.compress_zip(d_in, [n], ["zeros"], out_align=16)
    del d_in
    c = int(index.host["csize"][0])
    assert index.zip64 and int(index.host["method"][0]) == 8 and int(index.host["usize"][0]) == n and c < 1 << 32 and index.write_record.nstored == 0
    assert out.numel() == 30 + 5 + 20 + c + 46 + 5 + 12 + 22 and int(index.host["payload_off"][0]) == 55      # no ZIP64 end record: cd_off and cd_size are small
    head = out[:55].cpu().numpy().tobytes()
    assert head[18:26] == b"\xff" * 8 and head[35:] == struct.pack("<HHQQ", 1, 16, n, c)
    cd = out[55 + c:55 + c + 63].cpu().numpy().tobytes()
    assert cd[20:28] == struct.pack("<II", c, R.ONES32) and cd[51:] == struct.pack("<HHQ", 1, 8, n)
    R.check_index("(c)", R.DeviceBytes(out), index, 16)
    zf, infos = _opened(out, index)
    assert infos[0].extract_version == 45
    zi = engine.zip_index(out, out_align=16, zip64=True)
    assert zi.host.tobytes() == index.host.tobytes()
    back, off, status = engine.inflate_zip(out, zi)               # (its room is the whole slot: a refused entry is not decoded)
    assert [int(x) for x in status.cpu()] == [Z.E_OUT_CAPACITY]


def test_save_npz_to_load_npz_past_four_gib(engine):
    """a dictionary whose stored arrays total more than 4 GiB, one of them alone: save_npz ("auto") writes ZIP64, load_npz reads the
    .npy headers of entries behind and across the 4 GiB mark and returns views that equal the tensors, all on the device"""
    from hdl_deflate_amd import load_npz, save_npz
    g = torch.Generator(device="cuda").manual_seed(67)
    big = torch.randint(0, 256, ((1 << 32) + 64,), dtype=torch.uint8, device="cuda", generator=g).view(torch.int64)
    tensors = {"head": torch.arange(1000, dtype=torch.float32, device="cuda"), "big": big,
               "tail": torch.arange(7 * 300, dtype=torch.int32, device="cuda").reshape(7, 300)}
    out = save_npz(engine, tensors, compressed=False)
    assert out.numel() > (1 << 32) + 64
    zi = engine.zip_index(out)
    assert zi.zip64 and zi.names == ["head.npy", "big.npy", "tail.npy"] and int(zi.host["usize"][1]) == (1 << 32) + 64 + 128
    assert int(zi.host["payload_off"][2]) > 1 << 32 and [int(m) for m in zi.host["method"]] == [0, 0, 0]
    infos = zipfile.ZipFile(R.DeviceFile(out)).infolist()
    assert [(i.orig_filename, i.file_size, i.CRC) for i in infos] == [(n, int(u), int(c)) for n, u, c in zip(zi.names, zi.host["usize"], zi.host["crc"])]
    del zi
    back = load_npz(engine, out)
    assert sorted(back) == sorted(tensors)
    for name, t in tensors.items():
        assert back[name].dtype == t.dtype and back[name].shape == t.shape and torch.equal(back[name], t), name
