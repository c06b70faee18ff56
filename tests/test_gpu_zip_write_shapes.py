"""GPU (-m gpu): hdlz_zip_write_ws / Engine.compress_zip at the shapes its kernels branch on -- zip_write_ref.shape_cases(): thousands
of entries (the wave search in two and three rounds, the plan's sixteen waves and its ragged last thread), runs of entries without rows
(the lone search), 65535 and 65536 rows (16 and 256 rows a workgroup, more than 128 tiles of the scan), 65535 entries with more rows
than that, and stored tiles among hundreds of entries.  tests/test_zip_write_cabi.py proves from each case's arrays that it reaches
its branch.

What the file, the record and the records must be is zip_write_ref.expected, as in tests/test_gpu_zip_write.py; the round trip through
Engine.zip_index and Engine.inflate_zip compares the WHOLE output, since these cases are there for the entries in the middle."""
import io
import zipfile

import numpy as np
import pytest

import zip_ref as Z
import zip_write_ref as W
from test_gpu_zip_write import _direct, _write

pytestmark = pytest.mark.gpu


def _round_trip_whole(engine, label, case, out, index, out_align):
    items = case["items"]
    zi = engine.zip_index(out, out_align=out_align)
    assert zi.record.status == Z.OK and zi.host.tobytes() == index.host.tobytes(), label
    assert (zi.record.nentries, zi.record.total_out, zi.record.cd_off, zi.record.cd_size) == \
        (index.record.nentries, index.record.total_out, index.record.cd_off, index.record.cd_size), label
    assert zi.names == [n for n, _ in items] == index.names, label
    data, off, status = engine.inflate_zip(out, index)
    status = status.cpu().numpy()
    assert not status.any(), (label, np.nonzero(status)[0][:8], status[np.nonzero(status)[0][:8]])
    data, off = data.cpu().numpy(), off.cpu().numpy()
    if out_align == 1:
        assert data.tobytes() == b"".join(bytes(d) for _, d in items), (label, "the flat output")
    else:
        for k, (_, d) in enumerate(items):
            assert off[k] % out_align == 0 and data[off[k]:off[k] + len(d)].tobytes() == bytes(d), (label, k)


@pytest.mark.parametrize("label", W.SHAPE_LABELS)
def test_the_file_is_the_rules_at_every_shape(engine, label):
    case = W.shape_case(label)
    for out_align in (1,) if label in W.LARGE_SHAPES else (1, 64):
        out, index = _write(engine, case, out_align)
        W.check_written(label, W.written(label, out_align), out, index)
        _round_trip_whole(engine, label, case, out, index, out_align)
    if len(case["items"]) < 10000:
        zf = zipfile.ZipFile(io.BytesIO(out.cpu().numpy().tobytes()))
        assert zf.testzip() is None and [i.filename for i in zf.infolist()] == [n for n, _ in case["items"]]


# ---- failures at scale
def _fails(engine, label, tamper, want):
    """one _direct run: `want` {entry: status} are the only entries that fail; the record names the largest status and the lowest
    entry, and no length, offset or size is reported"""
    case = W.shape_case(label)
    rec, buf, ents = _direct(engine, case, len(W.written(label).file), tamper=tamper)
    assert (rec.status, rec.first_bad) == (max(want.values()), min(want)), (label, tamper.__name__, rec.status, rec.first_bad)
    assert (rec.file_len, rec.cd_off, rec.cd_size, rec.nstored) == (0, 0, 0, 0), (label, tamper.__name__)
    status = np.zeros(len(case["items"]), np.uint32)
    for e, s in want.items():
        status[e] = s
    assert np.array_equal(ents["status"], status), (label, tamper.__name__, np.nonzero(ents["status"] != status)[0][:8])
    assert not ents["csize"].any() and not ents["payload_off"].any(), (label, tamper.__name__)


def test_a_failing_row_far_behind_the_first_window_of_tiles(engine):
    """65536 rows: a status in tile 78 of a stored entry of 16383 rows, an end bit that contradicts its row in tile 195 of a deflated
    one of 20000 rows -- the counts' difference cnt[F1] - cnt[F0] taken across look-back windows --, and both (rule 6)"""
    label = "65536 rows across the seams"
    (e1, b1), (e2, b2) = W.SEAM_STATUS, W.SEAM_CONTRADICTION

    def status(z):
        z.status[b1] = W.E_SHORT_INPUT

    def contradict(z):
        z.end_bits[b2] += 8

    def both(z):
        status(z)
        contradict(z)

    _fails(engine, label, status, {e1: W.E_SHORT_INPUT})
    _fails(engine, label, contradict, {e2: W.E_BAD_PARAM})
    _fails(engine, label, both, {e1: W.E_SHORT_INPUT, e2: W.E_BAD_PARAM})


def test_failures_in_several_waves_of_the_plan(engine):
    """4097 entries, 5 a thread of the plan, entry e in its wave e // 320: the waves' worst status, lowest failed entry and stored count
    combined through LDS"""
    label = "4097 entries of 1 to 3 rows"
    first = [int(f) for f in W.batch_arrays(W.shape_case(label))[0]]
    a, b, c, last = W.FAIL_ENTRIES

    def three_waves(z):
        z.status[first[a]] = W.E_OUT_CAPACITY
        z.end_bits[first[b + 1] - 1] += 8
        z.status[first[c]] = W.E_SHORT_INPUT

    def ragged_last_thread(z):
        z.status[first[last + 1] - 1] = W.E_SHORT_INPUT

    def lowest_is_largest(z):
        z.end_bits[first[a]] += 8
        z.status[first[b]] = W.E_OUT_CAPACITY
        z.status[first[last]] = W.E_SHORT_INPUT

    _fails(engine, label, three_waves, {a: W.E_OUT_CAPACITY, b: W.E_BAD_PARAM, c: W.E_SHORT_INPUT})
    _fails(engine, label, ragged_last_thread, {last: W.E_SHORT_INPUT})
    _fails(engine, label, lowest_is_largest, {a: W.E_BAD_PARAM, b: W.E_OUT_CAPACITY, last: W.E_SHORT_INPUT})


def test_capacity_at_65536_rows(engine):
    """file_cap = file_len, file_len - 1 and 0: the lengths are reported, the canary behind file_cap is intact (_direct), and a file
    that does not fit is not begun"""
    label = "65536 rows across the seams"
    case, w = W.shape_case(label), W.written(label)
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
