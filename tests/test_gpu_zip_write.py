"""GPU (-m gpu): hdlz_zip_write_ws / Engine.compress_zip / Engine.write_zip_bytes / save_npz.

The cases are those of tests/zip_write_ref.py; what the file, the record and d_entries must be is zip_write_ref.expected, THE FILE RULE
of include/hdlz_zip_write.h in Python, which tests/test_zip_write_cabi.py holds against zipfile, numpy.load and the index rule on the
same cases.  Every case: the file byte for byte, the record, the entries' records, and the round trip through Engine.zip_index and
Engine.inflate_zip with every entry HDLZ_OK."""
import io
import zipfile
import zlib

import numpy as np
import pytest
import torch

import zip_ref as Z
import zip_write_ref as W

pytestmark = pytest.mark.gpu


def _stage(items, mis=3):
    """the entries' bytes one behind the other on the device, at an odd address, with bytes behind them that are no entry's"""
    data = b"".join(bytes(d) for _, d in items)
    return torch.frombuffer(bytearray(b"\x55" * mis + data + b"\xAA" * 64), dtype=torch.uint8).cuda()[mis:mis + len(data)]


def _write(engine, case, out_align=1, **kw):
    items = case["items"]
    return engine.compress_zip(_stage(items), [len(d) for _, d in items], [n for n, _ in items], block=case["block"], store=case["store"],
                               out_align=out_align, **kw)


def _round_trip(engine, label, case, out, index, out_align):
    """the writer's index is the reader's: zip_index gives the same records, inflate_zip reads every entry back"""
    items = case["items"]
    zi = engine.zip_index(out, out_align=out_align)
    assert zi.record.status == Z.OK and Z.device_records(zi) == Z.device_records(index), label
    assert (zi.record.nentries, zi.record.total_out, zi.record.cd_off, zi.record.cd_size) == \
        (index.record.nentries, index.record.total_out, index.record.cd_off, index.record.cd_size), label
    assert zi.names == [n for n, _ in items] == index.names, label
    data, off, status = engine.inflate_zip(out, index)
    assert bool((status == Z.OK).all()), (label, status.cpu().numpy()[:20])
    data, off = data.cpu().numpy(), off.cpu().numpy()
    step = max(1, len(items) // 200)
    for k in range(0, len(items), step):
        assert data[off[k]:off[k] + len(items[k][1])].tobytes() == bytes(items[k][1]), (label, k)


@pytest.mark.parametrize("label", [c["label"] for c in W.all_cases()])
def test_the_file_is_the_rules(engine, label):
    case = {c["label"]: c for c in W.all_cases()}[label]
    for out_align in (1, 64):
        out, index = _write(engine, case, out_align)
        W.check_written(label, W.written(label, out_align), out, index)
        _round_trip(engine, label, case, out, index, out_align)
    zf = zipfile.ZipFile(io.BytesIO(out.cpu().numpy().tobytes()))
    assert zf.testzip() is None and [i.filename for i in zf.infolist()] == [n for n, _ in case["items"]]


def test_block_sizes_and_a_date(engine):
    """the same entries at blocks of 64, 2048 and 65536 bytes (one, few and many tiles of the compressor a block), a date of its own"""
    items = [("a.txt", W.soft(70000, 1)), ("b.bin", Z.noise(5000, 2)), ("c.txt", W.soft(4100, 3)), ("d", b""), ("e.txt", Z.text(2048, 4))]
    for block in (64, 2048, 1 << 16):
        case = dict(label="blocks of %d" % block, items=items, block=block, store=None)
        dt = (2024, 2, 29, 23, 59, 58)
        out, index = _write(engine, case, 16, date_time=dt)
        w = W.expected(items, block=block, out_align=16, date_time=dt)
        W.check_written(case["label"], w, out, index)
        _round_trip(engine, case["label"], case, out, index, 16)
        assert zipfile.ZipFile(io.BytesIO(w.file)).infolist()[0].date_time == dt and w.methods[:4] == [8, 0, 8, 0]


def _direct(engine, case, cap, out_align=1, tamper=None):
    """hdlz_zip_write_ws itself over the case's batch, the file's buffer exactly `cap` bytes in front of a canary"""
    items = case["items"]
    z = engine._zip_batch(_stage(items), [len(d) for _, d in items], [n for n, _ in items], case["block"], 32, 10, case["store"])
    if tamper:
        tamper(z)
    buf = torch.full((cap + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    rec, res, back = engine._zip_write(z, buf[:cap], W.DATE_TIME, out_align)
    assert bool((buf[cap:] == 0x5A).all()), "bytes at or behind file_cap were written"
    from hdl_deflate_amd.zip import ENTRY_DTYPE
    return rec, buf, np.frombuffer(back.tobytes(), dtype=ENTRY_DTYPE)


def test_capacity(engine):
    """file_cap = file_len, file_len - 1 and 0 (the sizing call): the true lengths are reported, nothing at or behind file_cap is written"""
    for label in ("the forms alternating", "1 .. 600 blocks at block 32", "no entry"):
        case = {c["label"]: c for c in W.all_cases()}[label]
        w = W.written(label)
        n = len(w.file)
        for cap in (n, n - 1, 0):
            rec, buf, ents = _direct(engine, case, cap)
            want = dict(w.record, status=W.OK if cap >= n else W.E_OUT_CAPACITY)
            assert {k: getattr(rec, k) for k in want} == want, (label, cap)
            if cap >= n:
                assert buf[:n].cpu().numpy().tobytes() == w.file, (label, cap)
            else:
                assert bool((buf == 0x5A).all()), (label, cap, "an archive that does not fit is not begun")
            assert [tuple(int(r[f]) for f in Z.FIELDS) for r in ents] == Z.records(dict(entries=w.entries)), (label, cap)


def test_a_failing_block_fails_its_entry(engine):
    """the first cause of rule 1: one block's status word says HDLZ_E_SHORT_INPUT, another's a larger status"""
    case = {c["label"]: c for c in W.all_cases()}["1 .. 600 blocks at block 32"]       # entries own rows [0, 1, 256, 512, 515, 772, 1372)

    def one(z):
        z.status[600] = W.E_SHORT_INPUT                       # entry 4

    def two(z):
        z.status[600] = W.E_SHORT_INPUT
        z.status[300] = Z.E_BAD_HEADER                        # entry 2: the larger status, the lower entry
        z.status[301] = W.E_OUT_CAPACITY

    def in_one_entry(z):
        z.status[1000] = W.E_SHORT_INPUT                      # entry 5: its numerically largest status
        z.status[1371] = W.E_BAD_PARAM
        z.status[772] = W.E_OUT_CAPACITY

    for tamper, status, first in ((one, W.E_SHORT_INPUT, 4), (two, Z.E_BAD_HEADER, 2), (in_one_entry, W.E_BAD_PARAM, 5)):
        rec, buf, ents = _direct(engine, case, len(W.written(case["label"]).file), tamper=tamper)
        assert (rec.status, rec.first_bad, rec.file_len, rec.cd_off, rec.cd_size, rec.nstored) == (status, first, 0, 0, 0, 0), tamper.__name__
        assert int(ents["status"][first]) == status and int(ents["status"][0]) == W.OK
        assert not ents["csize"].any() and not ents["payload_off"].any()


def test_block_lengths_that_do_not_add_up(engine):
    """the third cause: the lengths of one entry's blocks, taken from d_in_off, are not its length"""
    case = {c["label"]: c for c in W.all_cases()}["store= entries"]                  # entries 0, 3 and 5 have blocks

    def shift(z):
        first = int(z.blk_first[3])
        z.in_off[first:] += 1                                 # entry 0's last block grows by a byte; the later entries keep their lengths

    def contradict(z):
        z.end_bits[int(z.blk_first[3])] += 8                  # the second cause: an end bit the row's length does not carry

    def descend(z):
        z.in_off[1] += 100                                    # entry 0: a block of 132 bytes, then one of -68; the sum is still its length

    for tamper, first in ((shift, 0), (contradict, 3), (descend, 0)):
        rec, buf, ents = _direct(engine, case, len(W.written(case["label"]).file), tamper=tamper)
        assert (rec.status, rec.first_bad, rec.file_len) == (W.E_BAD_PARAM, first, 0), tamper.__name__
        assert [int(s) for s in ents["status"]] == [W.E_BAD_PARAM if e == first else W.OK for e in range(6)]


def test_large_entries_get_a_crc_call_of_their_own(engine):
    """Engine.compress_zip's CRC-32 routing: entries of ZIP_CRC_TILED_MIN bytes and more by hdlz_crc32_ws into their own word, the runs of
    smaller ones around them by one hdlz_crc32_batch_ws each; the words stand in the headers, which are compared byte for byte"""
    label = "entries around ZIP_CRC_TILED_MIN"
    case = {c["label"]: c for c in W.all_cases()}[label]
    assert engine.ZIP_CRC_TILED_MIN == W.CRC_TILED_MIN
    calls = []
    tiled, batch = engine.crc32, engine.crc32_batch
    engine.crc32 = lambda d, **kw: (calls.append(("tiled", d.numel())), tiled(d, **kw))[1]
    engine.crc32_batch = lambda d, **kw: (calls.append(("batch", d.numel())), batch(d, **kw))[1]
    try:
        out, index = _write(engine, case)
    finally:
        del engine.crc32, engine.crc32_batch
    sizes = [len(d) for _, d in case["items"]]
    assert calls == [("batch", sizes[0] + sizes[1]), ("tiled", sizes[2]), ("batch", sizes[3] + sizes[4]), ("tiled", sizes[5]), ("tiled", sizes[6]),
                     ("batch", sizes[7])], calls
    W.check_written(label, W.written(label), out, index)
    assert [int(c) for c in index.host["crc"]] == [zlib.crc32(bytes(d)) for _, d in case["items"]]


def test_engine_raises_with_first_bad(engine):
    from hdl_deflate_amd import HdlzStatusError
    items = [("ok", W.soft(100, 1)), ("n" * 65536, W.soft(100, 2))]     # a name of 65536 bytes: the fourth cause
    with pytest.raises(HdlzStatusError) as e:
        engine.compress_zip(_stage(items), [100, 100], [n for n, _ in items], block=32)
    assert e.value.status == W.E_BAD_PARAM and e.value.first_bad == 1


# ---- .npz and bytes
def _tensors():
    return {name: torch.from_numpy(np.array(a)).cuda() for name, a in W.npz_arrays().items()}      # (np.array: a 0-d array stays 0-d)


@pytest.mark.parametrize("compressed", (True, False))
def test_save_npz_is_what_numpy_loads(engine, compressed):
    import hdl_deflate_amd
    arrays, tensors = W.npz_arrays(), _tensors()
    f = hdl_deflate_amd.save_npz(engine, tensors, compressed=compressed)
    assert f.is_cuda and f.dtype == torch.uint8 and f.dim() == 1
    z = f.cpu().numpy().tobytes()
    assert z == W.expected(W.npz_items(arrays), block=1 << 16, store=None if compressed else [True] * len(arrays)).file
    back = np.load(io.BytesIO(z))
    assert sorted(back.files) == sorted(arrays)
    for name, a in arrays.items():
        assert back[name].dtype == a.dtype and back[name].shape == a.shape and np.array_equal(back[name], a), name
    methods = {i.compress_type for i in zipfile.ZipFile(io.BytesIO(z)).infolist()}
    assert methods == ({0, 8} if compressed else {0})
    again = hdl_deflate_amd.load_npz(engine, f)
    assert sorted(again) == sorted(tensors)
    for name, t in tensors.items():
        assert again[name].dtype == t.dtype and again[name].shape == t.shape and torch.equal(again[name], t), name


def test_save_npz_refuses_a_dtype_without_a_descr(engine):
    import hdl_deflate_amd
    with pytest.raises(hdl_deflate_amd.Error):
        hdl_deflate_amd.save_npz(engine, {"x": torch.zeros(4, dtype=torch.bfloat16, device="cuda")})
    t = torch.arange(12, device="cuda").reshape(3, 4).t()     # not contiguous: written in C order
    back = np.load(io.BytesIO(hdl_deflate_amd.save_npz(engine, {"t": t}).cpu().numpy().tobytes()))
    assert np.array_equal(back["t"], t.cpu().numpy())


def test_write_zip_bytes_and_read_zip_bytes(engine):
    files = {"a/text.txt": W.soft(5000, 1), "noise.bin": Z.noise(3000, 2), "empty": b"", "übung.txt": Z.text(77, 3), "abc": b"abc"}
    z = engine.write_zip_bytes(files, block=2048)
    assert z == W.expected(list(files.items()), block=2048).file
    zf = zipfile.ZipFile(io.BytesIO(z))
    assert zf.testzip() is None and {i.filename: zf.read(i) for i in zf.infolist()} == files
    st, back = engine.read_zip_bytes(z)
    assert st == Z.OK and back == files
