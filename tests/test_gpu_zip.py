"""GPU (-m gpu): hdlz_zip_index_ws / hdlz_zip_inflate_ws / Engine.zip_index / Engine.inflate_zip / Engine.read_zip_bytes / load_npz.

The archives are those of tests/zip_ref.py (zipfile, numpy and hand-built ones, fixed seeds); what the index and every entry must answer
is zip_ref.index and zip_ref.judge, the rule of include/hdlz_zip.h in Python, which tests/test_zip_cabi.py holds against zipfile on
the same archives.  Entries are read on both routes: many in a call (the task view of the wave-per-member decoder) and alone in a call
(the batch call's path)."""
import io
import time
import zipfile

import numpy as np
import pytest

import zip_ref as Z

pytestmark = pytest.mark.gpu


def _whole(engine, label, z, out_align=1):
    """index the file and read it twice -- ONE call over all entries (count >= 2) and as Engine.inflate_zip routes it -- against the rule"""
    d = Z.stage(z)
    zi = engine.zip_index(d, out_align=out_align)
    ix = Z.check_index(label, z, zi, out_align)
    _, sts, flat = Z.read(z, out_align)
    n = ix["nentries"]
    if n:
        out, out_off, status, rec = Z.run_inflate(engine, d, zi, 0, n)
        Z.check_read((label, "one call"), z, ix, sts, flat, 0, out, out_off, status)
        bad = [k for k, s in enumerate(sts) if s != Z.OK]
        assert (rec.status, rec.first_bad) == ((Z.OK, 2 ** 64 - 1) if not bad else (int(status[bad[0]]) & 0xFFFFFFFF, bad[0])), (label, rec.status, rec.first_bad)
        assert rec.out_len == (ix["total_out"] if not bad else 0)
    out, out_off, status = engine.inflate_zip(d, zi)
    Z.check_read((label, "routed"), z, ix, sts, flat, 0, out, out_off, status)
    return d, zi, ix, sts, flat


@pytest.mark.parametrize("label", [c[0] for c in Z.writer_cases()])
def test_archives_of_zipfile_and_numpy(engine, label):
    """deflate levels 1, 6 and 9 and stored entries of 0 to 70000 bytes, names of 1 to 300 bytes, entry extras and comments, an archive
    comment, a directory entry; numpy.savez_compressed (local extra 20 bytes, central extra none) and numpy.savez; data descriptors"""
    z = dict(Z.writer_cases())[label]
    d, zi, ix, sts, flat = _whole(engine, label, z)
    assert sts == [Z.OK] * len(sts) and zi.record.status == Z.OK
    zf = zipfile.ZipFile(io.BytesIO(z))
    assert zi.names == [i.orig_filename for i in zf.infolist()]
    if label == "zipfile mixed":
        assert "d/" in zi.names and max(len(n) for n in zi.names) == 300 and {0, 8} == set(zi.host["method"])
        assert 70000 in zi.host["usize"][zi.host["method"] == 0] and 70000 in zi.host["usize"][zi.host["method"] == 8]


@pytest.mark.parametrize("label", [c[0] for c in Z.lookalike_cases()])
def test_lookalike_signatures(engine, label):
    """PK\\1\\2, PK\\3\\4 and PK\\5\\6 inside names, extras, comments and stored payloads; an end record inside the archive comment that
    does not fit; a stored entry that is itself a complete ZIP and ends within the search window"""
    z = dict(Z.lookalike_cases())[label]
    d, zi, ix, sts, flat = _whole(engine, label, z)
    assert sts == [Z.OK] * len(sts) and zi.record.status == Z.OK and len(sts) >= 2


@pytest.mark.parametrize("label", [c[0] for c in Z.geometry_cases()])
def test_directory_geometry(engine, label):
    """65535 empty entries; a directory of more than three staging pieces whose records straddle the boundaries; one record of
    46 + 3 * 65535 bytes; entry_cap of 0, nentries - 1 and nentries; out_align of 1, 64 and 256"""
    z = dict(Z.geometry_cases())[label]
    d, zi, ix, sts, flat = _whole(engine, label, z)
    n = ix["nentries"]
    assert sts == [Z.OK] * n and zi.record.status == Z.OK
    for cap in (0, n - 1, n):
        zc = engine.zip_index(d, entry_cap=cap)
        Z.check_index((label, "entry_cap", cap), z, zc, 1, cap)
        assert zc.record.status == (Z.OK if cap == n else Z.E_OUT_CAPACITY) and len(zc.host) == cap
    for align in (64, 256):
        if n <= 1000:
            _whole(engine, (label, "out_align", align), z, align)
        else:
            Z.check_index((label, "out_align", align), z, engine.zip_index(d, out_align=align), align)


def test_out_align_moves_the_slots_of_real_entries(engine):
    z = dict(Z.writer_cases())["zipfile mixed"]
    for align in (64, 256):
        d, zi, ix, sts, flat = _whole(engine, ("mixed", align), z, align)
        assert all(int(o) % align == 0 for o in zi.host["out_off"]) and zi.record.total_out > Z.index(z)["total_out"]


@pytest.mark.parametrize("k", range(len(Z.entry_damage_cases())), ids=[c[0] for c in Z.entry_damage_cases()])
def test_a_damaged_entry_fails_alone_on_both_routes(engine, k):
    """exactly that entry fails, its neighbours stay OK and byte-exact; read alone (count == 1, the one-stream route) it has the same
    verdict"""
    label, z, e, want = Z.entry_damage_cases()[k]
    d, zi, ix, sts, flat = _whole(engine, label, z, 4)
    assert [s != Z.OK for s in sts] == [j == e for j in range(9)] and (want is None or sts[e] == want)
    many = Z.run_inflate(engine, d, zi, 0, 9)
    for in_len in (int(zi.host["csize"][e]) + 6, 0):           # the bound stated (a large payload: the whole GPU) and not stated (one wave)
        out, out_off, status, rec = Z.run_inflate(engine, d, zi, e, 1, in_len)
        assert int(status[0]) == int(many[2][e]) and rec.status == int(status[0]) & 0xFFFFFFFF and rec.first_bad == 0, (label, in_len, int(status[0]))
    for j in (e - 1, e + 1):                                    # the neighbours alone
        out, out_off, status, rec = Z.run_inflate(engine, d, zi, j, 1, int(zi.host["csize"][j]) + 6)
        Z.check_read((label, "neighbour alone", j), z, ix, sts, flat, j, out, out_off, status)
        assert rec.status == Z.OK and rec.out_len == ix["entries"][j]["usize"]


@pytest.mark.parametrize("k", range(len(Z.file_damage_cases())), ids=[c[0] for c in Z.file_damage_cases()])
def test_file_level_damage(engine, k):
    """a ZIP64 locator, a cut end record, an entry count off by one, cd_off + cd_size != p, a directory signature broken at entry 3 of
    8: the record's status, and the entries in front of the stop stay indexed and readable"""
    label, z, want, kept = Z.file_damage_cases()[k]
    d, zi, ix, sts, flat = _whole(engine, label, z)
    assert (zi.record.status, zi.record.nentries, len(zi.host)) == (want, kept, kept) and sts == [Z.OK] * kept
    status, files = engine.read_zip_bytes(z)
    assert status == want and len(files) == kept
    if kept:
        assert files == {it["name"].decode(): it["data"] for it in Z.base_items()[:kept]}


def test_every_sub_range_equals_the_whole_read(engine):
    z = Z.make_zip(Z.base_items())
    for align in (1, 16):
        d, zi, ix, sts, flat = _whole(engine, "nine entries", z, align)
        for first in range(9):
            for count in range(0, 10 - first):
                out, out_off, status = engine.inflate_zip(d, zi, first=first, count=count)
                assert status.numel() == count
                Z.check_read(("sub-range", align, first, count), z, ix, sts, flat, first, out, out_off, status)
                if count >= 2:
                    out, out_off, status, rec = Z.run_inflate(engine, d, zi, first, count)
                    Z.check_read(("sub-range, one call", align, first, count), z, ix, sts, flat, first, out, out_off, status)
                    assert rec.status == Z.OK and rec.out_len == out.numel()


def test_a_refused_index_record_is_not_decoded(engine):
    """the index may come from elsewhere: the checks of hdlz_zip_inflate_ws in front of the decode, on both routes"""
    import torch
    z = Z.make_zip(Z.base_items())
    d = Z.stage(z)
    zi = engine.zip_index(d)
    host = zi.host.copy()
    host["payload_off"][0] = 29                                 # in front of any payload
    host["payload_off"][2] = len(z) - 100                       # the payload would run out of the file
    host["out_off"][4] = 1 << 40                                # the slot lies behind out_cap
    host["csize"][7] = 1 << 28                                  # above what the decoder's 32-bit positions hold
    host["status"][8] = Z.E_BAD_BTYPE
    from hdl_deflate_amd.zip import ZipIndex
    bad = ZipIndex(torch.from_numpy(np.frombuffer(host.tobytes(), np.int64).reshape(-1, 6).copy()).cuda(), zi.record, host, zi.names, 1)
    out, out_off, status, rec = Z.run_inflate(engine, d, bad, 0, 9)
    st = [int(s) for s in status]
    assert st == [Z.E_BAD_PARAM, 0, Z.E_BAD_PARAM, 0, Z.E_BAD_PARAM, 0, 0, Z.E_BAD_PARAM, Z.E_BAD_BTYPE] and (rec.status, rec.first_bad) == (Z.E_BAD_PARAM, 0)
    ix, sts, flat = Z.read(z)
    for j in (1, 3, 5, 6):
        en = ix["entries"][j]
        assert out[en["out_off"]:en["out_off"] + en["usize"]].cpu().numpy().tobytes() == flat[en["out_off"]:en["out_off"] + en["usize"]]
    for j in (0, 2, 7, 8):
        assert int(Z.run_inflate(engine, d, bad, j, 1, 1 << 20)[2][0]) == st[j]
    # the stated bound: count >= 2, csize above it; count == 1, csize + 6 above it
    assert [int(s) for s in Z.run_inflate(engine, d, zi, 2, 2, 300)[2]] == [Z.E_BAD_PARAM, 0]
    c = int(zi.host["csize"][2])
    assert int(Z.run_inflate(engine, d, zi, 2, 1, c + 5)[2][0]) == Z.E_BAD_PARAM and int(Z.run_inflate(engine, d, zi, 2, 1, c + 6)[2][0]) == Z.OK


def _timed(fn, reps):
    import torch
    best = None
    for _ in range(reps):                                       # (best of three: a clock tick of the box must not fail the test)
        torch.cuda.synchronize()
        t0 = time.time()
        fn()
        torch.cuda.synchronize()
        best = time.time() - t0 if best is None else min(best, time.time() - t0)
    return best


def test_a_large_entry_alone_takes_the_whole_gpu(engine):
    """a 1 MiB level-6 entry read alone (count == 1) takes at most 1/5 of the time of the same entry read inside a two-entry call (the
    wave-per-member decoder): the criterion tests/test_gpu_gunzip.py uses to show that the whole-GPU chains ran"""
    data = Z.text(1 << 20, 70)
    z = Z.make_zip([dict(name=b"large.bin", data=data, level=6), dict(name=b"small.txt", data=Z.text(100, 71))])
    d = Z.stage(z)
    zi = engine.zip_index(d, out_align=16)
    c = int(zi.host["csize"][0])
    assert c >= Z.LARGE_MIN
    out, out_off, status, rec = Z.run_inflate(engine, d, zi, 0, 1, c + 6)
    assert rec.status == Z.OK and out.cpu().numpy().tobytes() == data
    out2, _, status2, rec2 = Z.run_inflate(engine, d, zi, 0, 2)
    assert rec2.status == Z.OK and out2[:1 << 20].cpu().numpy().tobytes() == data
    t_one = _timed(lambda: Z.run_inflate(engine, d, zi, 0, 1, c + 6), 3)
    t_two = _timed(lambda: Z.run_inflate(engine, d, zi, 0, 2), 1)
    print("1 MiB entry: alone %.3f ms, inside a two-entry call %.3f ms" % (t_one * 1e3, t_two * 1e3))
    assert t_one * 5 <= t_two, (t_one, t_two)
    out3, off3, st3 = engine.inflate_zip(d, zi)                  # routed: the large entry alone, the small one in a run of one
    assert [int(s) for s in st3] == [0, 0] and out3[:1 << 20].cpu().numpy().tobytes() == data


def test_a_4_mib_stored_entry_alone(engine):
    data = Z.noise(4 << 20, 72)
    z = Z.make_zip([dict(name=b"a", data=Z.text(33, 73)), dict(name=b"stored.bin", data=data, method=0), dict(name=b"b", data=b"xyz", method=0)])
    d = Z.stage(z)
    for align in (1, 64):                                       # (align 1: the slot starts at 33 -- the task view's copy, one workgroup)
        zi = engine.zip_index(d, out_align=align)
        out, out_off, status, rec = Z.run_inflate(engine, d, zi, 1, 1, 0)
        assert rec.status == Z.OK and rec.out_len == 4 << 20 and out.cpu().numpy().tobytes() == data
        out, out_off, status = engine.inflate_zip(d, zi)
        ix, sts, flat = Z.read(z, align)
        Z.check_read(("4 MiB stored", align), z, ix, sts, flat, 0, out, out_off, status)
    bad = bytearray(z)
    bad[zi.host["payload_off"][1] + (3 << 20)] ^= 1
    assert [int(s) for s in engine.inflate_zip(Z.stage(bytes(bad)), zi)[2]] == [0, Z.E_BAD_CHECKSUM, 0]


def test_the_calls_are_hip_graph_capturable(engine):
    """index + a count >= 2 read + a count == 1 read with caller scratch captured into ONE HIP graph and replayed three times: nothing is
    allocated, the host reads nothing in between, and the results are identical each time"""
    import torch
    from hdl_deflate_amd import _lib
    L = engine.lib
    items = [dict(name=b"g%d" % k, data=Z.text(3000 + 500 * k, 80 + k), level=(1, 6, 9)[k % 3], method=(8, 0)[k % 2]) for k in range(5)]
    items.append(dict(name=b"big", data=Z.text(300000, 90), level=6))
    z = Z.make_zip(items)
    ix, sts, flat = Z.read(z, 16)
    d = Z.stage(z)
    n, total = 6, ix["total_out"]
    big = ix["entries"][5]
    entries = torch.zeros((n, 6), dtype=torch.int64, device="cuda")
    rec = torch.zeros(16, dtype=torch.int64, device="cuda")     # the three records
    iwork = torch.empty(L.hdlz_zip_index_work_bytes(len(z), n), dtype=torch.uint8, device="cuda")
    out = torch.zeros((total + 3) & ~3, dtype=torch.uint8, device="cuda")
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    cap1 = (big["usize"] + 3) & ~3
    w5 = torch.empty(L.hdlz_zip_inflate_work_bytes(5, 0, big["out_off"]), dtype=torch.uint8, device="cuda")
    w1 = torch.empty(L.hdlz_zip_inflate_work_bytes(1, big["csize"] + 6, cap1), dtype=torch.uint8, device="cuda")

    def calls():
        s = torch.cuda.current_stream().cuda_stream
        assert L.hdlz_zip_index_ws(d.data_ptr(), len(z), n, 16, entries.data_ptr(), rec.data_ptr(), iwork.data_ptr(), iwork.numel(), s) == 0
        assert L.hdlz_zip_inflate_ws(d.data_ptr(), len(z), entries.data_ptr(), 0, 5, 0, out.data_ptr(), big["out_off"], status.data_ptr(),
                                     rec[5:].data_ptr(), w5.data_ptr(), w5.numel(), s) == 0
        assert L.hdlz_zip_inflate_ws(d.data_ptr(), len(z), entries.data_ptr(), 5, 1, big["csize"] + 6, out.data_ptr() + big["out_off"], cap1,
                                     status[5:].data_ptr(), rec[8:].data_ptr(), w1.data_ptr(), w1.numel(), s) == 0
    calls()                                                      # eager once
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            calls()
    seen = []
    for k in range(3):
        entries.fill_(-1 - k); rec.fill_(k); out.fill_(k); status.fill_(7); iwork.fill_(0x11 * k); w5.fill_(0x22 * k); w1.fill_(0x33 * k)
        g.replay()
        torch.cuda.synchronize()
        host = out[:total].cpu().numpy().tobytes()
        slots = b"".join(host[en["out_off"]:en["out_off"] + en["usize"]] for en in ix["entries"])       # (the gaps between the slots keep the fill)
        seen.append((entries.cpu().numpy().tobytes(), rec[:11].cpu().numpy().tobytes(), slots, status.cpu().numpy().tobytes()))
        r = _lib.ZipIndexResult.from_buffer_copy(rec[:5].cpu().numpy().tobytes())
        assert (r.status, r.nentries, r.total_out) == (Z.OK, 6, total)
        assert [int(x) for x in status] == [0] * 6
        assert slots == b"".join(flat[en["out_off"]:en["out_off"] + en["usize"]] for en in ix["entries"])
        gaps = np.ones(total, bool)
        for en in ix["entries"]:
            gaps[en["out_off"]:en["out_off"] + en["usize"]] = False
        assert gaps.any() and (np.frombuffer(host, np.uint8)[gaps] == k).all()           # nothing outside the slots was written
    assert seen[0] == seen[1] == seen[2]


def test_read_zip_bytes_reads_files_as_zipfile_does(engine):
    for label, z in Z.writer_cases() + Z.lookalike_cases()[2:]:
        zf = zipfile.ZipFile(io.BytesIO(z))
        assert engine.read_zip_bytes(z) == (Z.OK, {n: zf.read(n) for n in zf.namelist()}), label
    label, z, e, want = Z.entry_damage_cases()[1]
    status, files = engine.read_zip_bytes(z)
    assert status == want and len(files) == 8 and "e%d.txt" % e not in files
    assert engine.read_zip_bytes(b"not a zip file at all, but long enough") == (Z.E_BAD_HEADER, {}) and engine.read_zip_bytes(b"") == (Z.E_NO_EOF, {})


def test_load_npz_gives_device_tensors_equal_to_numpy_load(engine):
    import torch
    from hdl_deflate_amd import load_npz
    r = np.random.default_rng(95)
    arrays = dict(i64=r.integers(-2 ** 62, 2 ** 62, (300, 7), dtype=np.int64), f32=r.standard_normal((64, 33)).astype(np.float32),
                  f16=r.standard_normal(5001).astype(np.float16), u8=r.integers(0, 256, (3, 5, 7000), dtype=np.uint8),
                  scalar=np.float32(3.25), scalar_i64=np.array(-5, np.int64), empty=np.zeros((0, 4), np.float16), empty_u8=np.zeros(0, np.uint8),
                  big=np.arange(1 << 18, dtype=np.int64))
    for save in (np.savez_compressed, np.savez):
        buf = io.BytesIO()
        save(buf, **arrays)
        z = buf.getvalue()
        want = np.load(io.BytesIO(z))
        for source in (z, Z.stage(z)):
            got = load_npz(engine, source)
            assert sorted(got) == sorted(want.files)
            for name in want.files:
                t, a = got[name], want[name]
                assert t.is_cuda and t.data_ptr() != 0 or t.numel() == 0, name
                assert t.is_cuda and tuple(t.shape) == a.shape and str(t.dtype).split(".")[1] == str(a.dtype), (name, t.shape, t.dtype)
                assert np.array_equal(t.cpu().numpy(), a), name
    f = io.BytesIO()
    np.savez(f, fortran=np.asfortranarray(np.arange(6).reshape(2, 3)))
    with pytest.raises(Exception, match="Fortran"):
        load_npz(engine, f.getvalue())
    f = io.BytesIO()
    np.savez(f, obj=np.array([{"a": 1}], dtype=object))
    with pytest.raises(Exception, match="object"):
        load_npz(engine, f.getvalue())
