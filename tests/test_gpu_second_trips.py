"""GPU (-m gpu): the second trip of every capped grid, one-workgroup loop and one-wave round of the container, index and checksum
kernels, at the thresholds tests/second_trips.py derives from the launch code -- crc_tiles' prefetched tile and crc_finish's Horner
step (hdlz_crc32_ws and, through their other callers, the gzip join / unjoin, hdlz_gunzip_ws and a stored ZIP entry), k_gzm_seam with
two to four windows a thread, k_bgzf_seam's second and later rounds and k_bgzf_emit's second workgroup, lowest_word's second word,
the heads kernels' grid stride, and the finishing loops of both joins.

Every expected value comes from an independent reference: zlib.crc32, zlib.decompress, gzip.decompress, zipfile,
gzip_members_ref.index_rule / verdict, bgzf_ref.walk, gunzip_ref.member, joined_ref.member_of -- never from the library.  The files
and batches are those of tests/second_trips.py, which tests/test_second_trips_cpu.py holds against the same references on the CPU.

Deliberately left out: the second 64-tile window of tile_lookback (it is reached only when 64 tiles in a row have published no
prefix yet: timing, which a test cannot force); the tiled gunzip path past 65535 rows (rows of 64 KiB and more: 4 GiB of output);
any grid cap of 2^20 (k_crc32_batch, k_gunzip_crc_rows, k_zip_crc_slots: a million blocks and more).  hdlz_bgzf_inflate_ws takes no
mapping hint (its flags must be 0), so it runs once; the three hints run through hdlz_unjoin_ws."""
import gzip
import io
import zipfile
import zlib

import numpy as np
import pytest
import torch

import bgzf_ref
import gunzip_ref as G
import gzip_ref
import joined_ref
import second_trips as S
import zip_ref as Z
from gzip_calls import ZlibCall
from hdl_deflate_amd import _lib
from hdl_deflate_amd.errors import HdlzStatusError
from second_trips import OK, E_SHORT_INPUT, E_OUT_CAPACITY, E_NO_EOF, E_BAD_HEADER, E_BAD_CHECKSUM

pytestmark = pytest.mark.gpu

LANE, WAVE, GROUP = 2, 4, 64
NOBODY = (1 << 64) - 1
TILE = S.CRC_TILE
SENTINEL = -0x0123456789ABCDEF
BEYOND = S.CRC_GRID_MAX * TILE + 100          # an output byte of tile 1024: the second trip of workgroup 0


def dev_bytes(b, slack=64):
    """the bytes on the device, with bytes behind them that are not theirs -> the tensor of exactly the bytes"""
    return torch.frombuffer(bytearray(bytes(b) + b"\xAA" * slack), dtype=torch.uint8).cuda()[:len(b)]


def dev_i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def host(t):
    return t.cpu().numpy().tobytes()


def first_diff(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return ("shapes", a.shape, b.shape)
    bad = np.nonzero(a != b)[0]
    return None if not len(bad) else (int(bad[0]), a[bad[0]].item(), b[bad[0]].item(), len(bad))


# ---- hdlz_crc32_ws
_crc_host = {}


def crc_host(kind):
    if kind not in _crc_host:
        n = max(S.CRC_TILE_COUNTS) * TILE + 7 + 48
        _crc_host[kind] = (np.random.default_rng(47).integers(0, 256, n, dtype=np.uint8) if kind == "random" else
                           np.full(n, 0 if kind == "zeros" else 255, np.uint8))
    return _crc_host[kind]


def device_crcs(L, d_buf, cases):
    """hdlz_crc32_ws of d_buf[a : a + n] for every (a, n): junk in the result words and in the scratch beforehand, one sync"""
    words = torch.full((len(cases),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    wb = max(L.hdlz_crc32_work_bytes(n) for _, n in cases)
    work = torch.full((max(wb, 4) // 4,), -1, dtype=torch.int32, device="cuda")
    for k, (a, n) in enumerate(cases):
        need = L.hdlz_crc32_work_bytes(n)
        rc = L.hdlz_crc32_ws(d_buf.data_ptr() + a, n, words.data_ptr() + 4 * k, work.data_ptr(), need, stream_ptr())
        assert rc == 0, L.hdlz_last_error()
    torch.cuda.synchronize()
    return [int(w) & 0xFFFFFFFF for w in words.cpu().numpy()]


def zlib_crcs(hb, a, lengths):
    """zlib.crc32(hb[a : a + n]) for ascending n, one pass over the bytes"""
    out, c, at = {}, 0, a
    for n in sorted(lengths):
        c = zlib.crc32(hb[at:a + n], c)
        at = a + n
        out[n] = c
    return out


@pytest.mark.parametrize("kind", ["random", "zeros", "ff"])
def test_crc32_of_1023_to_2049_tiles(engine, kind):
    """1023, 1024, 1025, 2047, 2048, 2049 tiles, each exact, plus 7 bytes and minus 1 byte: from 1024 tiles on thread 0 of the
    finishing workgroup takes a second Horner step (from 2048 a third), from 1025 tiles on workgroup 0 of the tile kernel takes the
    tile it prefetched and stages its strips again (from 2049 a third).  Base pointers 0, 1 and 15 bytes off a 16-byte boundary, the
    slices inside one larger buffer; zeros: only the length speaks"""
    h = crc_host(kind)
    d = torch.from_numpy(h).cuda()
    assert d.data_ptr() % 16 == 0
    lengths = [t * TILE + e for t in S.CRC_TILE_COUNTS for e in (0, 7, -1)]
    cases = [(16 + a, n) for a in (0, 1, 15) for n in lengths]
    got = device_crcs(engine.lib, d, cases)
    hb = memoryview(h)
    want = {a: zlib_crcs(hb, 16 + a, lengths) for a in (0, 1, 15)}
    bad = [(a - 16, n // TILE, n % TILE, hex(g)) for (a, n), g in zip(cases, got) if g != want[a - 16][n]]
    assert bad == [], bad[:8]
    if kind == "random":
        n = S.CRC_CALLER_BYTES
        t = engine.crc32(d[17:17 + n])
        assert t.dtype == torch.uint32 and int(t.cpu().numpy()[0]) == want[1][n]


# ---- the same two functions through their other callers: 1025 tiles + 7 bytes of output each
def test_gzip_joined_stream_of_1025_tiles(engine):
    """compress_joined(container="gzip") writes the CRC-32 of hdlz_crc32_ws, inflate_joined verifies it by k_unjoin_gzip_tiles and
    crc_finish; a literal flipped in the last member -- an output byte of tile 1024 -- must end E_BAD_CHECKSUM"""
    n = S.CRC_CALLER_BYTES
    data = S.literal_data(n)
    d = dev_bytes(data)
    z, offs = engine.compress_joined(d, block=65536, container="gzip")
    zb = host(z)
    assert int.from_bytes(zb[-8:-4], "little") == zlib.crc32(data) and int.from_bytes(zb[-4:], "little") == n
    assert gzip.decompress(zb) == data
    assert host(engine.inflate_joined(z, offs, block=65536, total=n, container="gzip")) == data
    # literal i of a member is the eight bits from bit 3 + 8 i on, most significant first: its lowest bit is bit 2 of byte i + 1
    o = [int(x) for x in offs.cpu().numpy()]
    b, i = BEYOND // 65536, BEYOND % 65536
    assert len(o) - 1 == -(-n // 65536) and b == len(o) - 2
    bad = bytearray(zb)
    bad[o[b] + i + 1] ^= 0x04
    dec = zlib.decompressobj(-15)
    wrong = dec.decompress(bytes(bad[10:]))
    assert dec.eof and len(wrong) == n and [k for k in range(BEYOND - 2, BEYOND + 3) if wrong[k] != data[k]] == [BEYOND]
    assert wrong[:BEYOND] == data[:BEYOND] and wrong[BEYOND + 1:] == data[BEYOND + 1:], "one output byte of tile 1024 differs, nothing else"
    with pytest.raises(HdlzStatusError) as e:
        engine.inflate_joined(dev_bytes(bad), offs, block=65536, total=n, container="gzip")
    assert e.value.status == E_BAD_CHECKSUM


def test_one_gzip_member_of_1025_tiles(engine):
    """hdlz_gunzip_ws with one long row: k_gunzip_crc_tiles and k_gunzip_crc_finish"""
    n = S.CRC_CALLER_BYTES
    data = crc_host("random")[:n].tobytes()
    z = G.header(name=b"second trip") + S.stored_deflate(data) + G.trailer(data)
    assert G.zaccepts(z) == (data, len(z))
    at = z.index(data[BEYOND:BEYOND + 32], BEYOND)            # where output byte BEYOND stands in the stored blocks
    pitch = (n + 15) // 16 * 16
    for flip in (False, True):
        zz = bytearray(z)
        want = bytearray(data)
        if flip:
            zz[at] ^= 0x10
            want[BEYOND] ^= 0x10
            assert G.zaccepts(bytes(zz)) is None
        out, ol, st, used, crc = engine.inflate_gzip(dev_bytes(zz), in_len=len(zz), nblocks=1, out_pitch=pitch)
        torch.cuda.synchronize()
        got = (int(st.item()), int(ol.item()), int(used.item()), int(crc.item()) & 0xFFFFFFFF)
        if flip:
            assert got == (E_BAD_CHECKSUM, 0, len(z), zlib.crc32(want)), got
        else:
            assert got == (OK, n, len(z), zlib.crc32(data)), got
            assert host(out[0, :n]) == data


def test_one_stored_zip_entry_of_1025_tiles(engine):
    """hdlz_zip_inflate_ws with one large entry: k_zip_crc_tiles and k_zip_crc_finish"""
    n = S.CRC_CALLER_BYTES
    data = crc_host("random")[:n].tobytes()
    z = Z.make_zip([dict(name=b"a", data=Z.text(33, 73)), dict(name=b"stored.bin", data=data, method=0)])
    assert zipfile.ZipFile(io.BytesIO(z)).read("stored.bin") == data
    d = Z.stage(z)
    zi = engine.zip_index(d, out_align=64)
    out, out_off, status = engine.inflate_zip(d, zi)
    assert [int(s) for s in status.cpu()] == [OK, OK]
    o = int(out_off[1])
    assert host(out[o:o + n]) == data
    bad = bytearray(z)
    bad[int(zi.host["payload_off"][1]) + BEYOND] ^= 1
    with pytest.raises(zipfile.BadZipFile):
        zipfile.ZipFile(io.BytesIO(bytes(bad))).read("stored.bin")
    assert [int(s) for s in engine.inflate_zip(Z.stage(bytes(bad)), zi)[2].cpu()] == [OK, E_BAD_CHECKSUM]


# ---- hdlz_gzip_members_index_ws with two to four windows a thread of k_gzm_seam
def gzm_index(engine, d, n, cap):
    """-> (off, out_off: cap + 1 words and nine sentinels behind, the record); junk in the scratch"""
    L = engine.lib
    off, out_off = (torch.full((cap + 10,), SENTINEL, dtype=torch.int64, device="cuda") for _ in range(2))
    res = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    wb = L.hdlz_gzip_members_index_work_bytes(n)
    work = torch.full((max(wb, 1),), 0xA5, dtype=torch.uint8, device="cuda")
    rc = L.hdlz_gzip_members_index_ws(d.data_ptr(), n, cap, off.data_ptr(), out_off.data_ptr(), res.data_ptr(), work.data_ptr(), wb, stream_ptr())
    assert rc == 0, L.hdlz_last_error()
    torch.cuda.synchronize()
    return off.cpu().numpy(), out_off.cpu().numpy(), _lib.GzipMembersIndexResult.from_buffer_copy(host(res))


@pytest.mark.parametrize("label", list(S.gzm_shapes()))
def test_gzip_members_index_with_several_windows_a_thread(engine, label):
    """513 windows (K = 2), 1025 windows + 100 bytes (K = 3, a last window of 100 bytes) and 1537 windows (K = 4), the last threads of
    the seam workgroup without a window: candidates in two consecutive windows of one thread, in the last window of a thread and
    the first of the next, behind three shares without any, at k WIN + d, d = -3 .. 3, inside a share and between two, and 8192 of
    them in a thread's second window -- against the index rule; member_cap = M, M - 1, two values that end between a thread's
    windows, 0: no word behind min(M, cap)"""
    z, plan = S.gzm_file(label)
    cands = S.gzm_planted(plan)
    want_off, want_out = S.index_rule_arrays(z, cands)
    M = len(cands)
    d = dev_bytes(z, 32)
    for cap in S.gzm_caps(plan, cands):
        off, out_off, rec = gzm_index(engine, d, len(z), cap)
        k = min(M, cap) + 1
        assert (rec.nmembers, rec.total_out, rec.reserved) == (M, int(want_out[-1]), 0), (cap, rec.nmembers, M, rec.total_out, int(want_out[-1]))
        assert rec.status == (E_OUT_CAPACITY if M > cap else OK), (cap, rec.status)
        assert first_diff(off[:k], want_off[:k]) is None, (cap, "off", first_diff(off[:k], want_off[:k]))
        assert first_diff(out_off[:k], want_out[:k]) is None, (cap, "out_off", first_diff(out_off[:k], want_out[:k]))
        assert (off[k:] == SENTINEL).all() and (out_off[k:] == SENTINEL).all(), (cap, "words behind min(M, cap) were written")


# ---- hdlz_bgzf_index_ws past one round of the seam wave
def bgzf_index(engine, d, n, cap, junk):
    L = engine.lib
    off, out_off = (torch.full((cap + 1 + 8,), junk, dtype=torch.int64, device="cuda") for _ in range(2))
    res = torch.full((4,), junk, dtype=torch.int64, device="cuda")
    wb = L.hdlz_bgzf_index_work_bytes(n)
    work = torch.full((max(wb, 8) // 8,), junk, dtype=torch.int64, device="cuda")
    rc = L.hdlz_bgzf_index_ws(d.data_ptr(), n, cap, off.data_ptr(), out_off.data_ptr(), res.data_ptr(), work.data_ptr(), wb, stream_ptr())
    assert rc == 0, L.hdlz_last_error()
    torch.cuda.synchronize()
    r = _lib.BgzfIndexResult.from_buffer_copy(host(res))
    return off.cpu().numpy(), out_off.cpu().numpy(), (r.nmembers, r.total_out, r.file_used, r.status, r.eof_marker)


def check_bgzf_index(engine, label, f, cap=None):
    """the index against the serial walk, on two kinds of junk in the outputs and the scratch"""
    w = bgzf_ref.walk(f)
    cap = w.nmembers if cap is None else cap
    record = w.record() if w.nmembers <= cap else (w.nmembers, w.total_out, w.file_used, E_OUT_CAPACITY, 0)
    k = min(w.nmembers, cap) + 1
    d = dev_bytes(f, 1)
    for junk in (-1, 0x0102030405060708):
        off, out_off, rec = bgzf_index(engine, d, len(f), cap, junk)
        assert rec == record, (label, cap, rec, record)
        assert first_diff(off[:k], w.off[:k]) is None, (label, cap, "off", first_diff(off[:k], w.off[:k]))
        assert first_diff(out_off[:k], w.out_off[:k]) is None, (label, cap, "out_off", first_diff(out_off[:k], w.out_off[:k]))
        assert (off[k:] == junk).all() and (out_off[k:] == junk).all(), (label, cap, "words behind min(nmembers, cap) were written")
    return w


@pytest.mark.parametrize("label", list(S.bgzf_shapes()))
def test_bgzf_index_past_one_round_of_the_seam_wave(engine, label):
    """65, 129 and 259 windows of members of every level: `prev` of lane 0 in a later round; a look-alike header that makes window 64
    (lane 0 of round two), window 63 and window 127 (lane 63 of two rounds) guess wrong, landing on a true start or running off into
    data: take < 64, the repair walk and the round that starts behind it; more than 256 windows: k_bgzf_emit's second workgroup"""
    f, _, _ = S.bgzf_file(label)
    w = check_bgzf_index(engine, label, f)
    assert w.status == OK and w.file_used == len(f)


@pytest.mark.parametrize("window, first", [(70, False), (200, True)])
def test_bgzf_index_stops_in_a_later_round(engine, window, first):
    """a member's magic broken in window 70 (its second member: the scan's own stop status, found in round two) and in window 200
    (its first member: the window guesses wrong, the repair walk stops) -- the windows behind must not reach the result"""
    f, _, _ = S.bgzf_file("259 windows")
    g = S.bgzf_damaged(f, bgzf_ref.walk(f).off, window, first)
    w = check_bgzf_index(engine, (window, first), g)
    assert w.status == E_BAD_HEADER and w.file_used // S.BGZF_WIN == window


def test_bgzf_index_member_cap_inside_window_256(engine):
    f, _, _ = S.bgzf_file("259 windows")
    w = bgzf_ref.walk(f)
    b256 = next(b for b, o in enumerate(w.off) if o // S.BGZF_WIN >= S.BGZF_EMIT_THREADS)
    for cap in (b256 + 1, b256 + 4, w.nmembers - 1, b256 - 1):
        check_bgzf_index(engine, "cap", f, cap=cap)


# ---- more than 65536 streams: the grid stride of k_gunzip_heads
def test_gunzip_of_65836_streams(engine, oracle):
    """mostly gzip.compress(b""), a real member every 1021 streams; the five streams that are not OK stand at indices >= 65536, where
    a wave takes its second stream: their statuses, in_used and out_len must land at b, not at b - 65536"""
    zs, bad = S.many_gzip_streams()
    memo = {z: G.expect(oracle, z, 64) for z in set(zs)}
    rows, ol, st, used, crc = G.run(engine, zs, 64)
    for name, got in (("status", st), ("out_len", ol), ("in_used", used), ("crc", crc)):
        want = np.array([memo[z][name] for z in zs], np.uint32)
        assert first_diff(got, want) is None, (name, first_diff(got, want))
    assert sorted(np.nonzero(st)[0].tolist()) == sorted(bad)
    for b, z in enumerate(zs):
        if z is not S.EMPTY_GZ and memo[z]["status"] == OK:
            assert rows[b, :ol[b]].tobytes() == memo[z]["data"], b


# ---- the judges' words past one word a thread (lowest_word), and the grid stride of k_gzm_heads
PLANTS = [(), (S.PLANT_HIGH,), (S.PLANT_LOW, S.PLANT_HIGH)]
PLANT_IDS = ["none", "group 256", "groups 3 and 256"]


@pytest.mark.parametrize("planted", PLANTS, ids=PLANT_IDS)
def test_gzip_members_read_of_65836_members(engine, oracle, planted):
    z, off, out_off, datas = S.many_gzip_members(planted)
    v = S.verdicts_memoised(oracle, z, off, out_off)
    out, st, rec = engine.inflate_gzip_members(dev_bytes(z, 32), index=(dev_i64(off), dev_i64(out_off)))
    torch.cuda.synchronize()
    st = st.cpu().numpy()
    assert first_diff(st, np.array([s for s, _ in v], np.int32)) is None, first_diff(st, np.array([s for s, _ in v], np.int32))
    assert np.nonzero(st)[0].tolist() == sorted(planted), "exactly the planted members are marked"
    got, want = np.frombuffer(host(out), np.uint8), np.frombuffer(b"".join(datas), np.uint8)
    keep = np.ones(len(want), bool)
    for b in planted:
        keep[out_off[b]:out_off[b + 1]] = False
    assert len(got) == len(want) and np.array_equal(got[keep], want[keep])
    if planted:
        assert (rec.status, rec.first_bad, rec.out_len, rec.reserved) == (E_BAD_CHECKSUM, min(planted), 0, 0), (rec.status, rec.first_bad)
    else:
        assert (rec.status, rec.first_bad, rec.out_len, rec.reserved) == (OK, NOBODY, len(want), 0), (rec.status, rec.first_bad)


@pytest.mark.parametrize("planted", PLANTS, ids=PLANT_IDS)
def test_bgzf_read_of_65836_members(engine, planted):
    L = engine.lib
    f, datas = S.many_bgzf_members()
    w = bgzf_ref.walk(f)
    data = b"".join(datas)
    g = bgzf_ref.with_crc_flipped(f, w.off, planted)
    B, total = w.nmembers, len(data)
    d_off, d_out_off = dev_i64(w.off), dev_i64(w.out_off)
    out = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    member = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    result = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    wb = L.hdlz_bgzf_inflate_work_bytes(B, 0)
    work = torch.full((wb,), 0x5A, dtype=torch.uint8, device="cuda")
    rc = L.hdlz_bgzf_inflate_ws(dev_bytes(g, 1).data_ptr(), len(g), d_off.data_ptr(), d_out_off.data_ptr(), B, 0, out.data_ptr(), total,
                                member.data_ptr(), result.data_ptr(), work.data_ptr(), wb, stream_ptr())
    assert rc == 0, L.hdlz_last_error()
    torch.cuda.synchronize()
    r = _lib.BgzfInflateResult.from_buffer_copy(host(result))
    st = member.cpu().numpy()
    assert np.nonzero(st)[0].tolist() == sorted(planted) and all(st[b] == E_BAD_CHECKSUM for b in planted)
    assert host(out[total:]) == b"\xa5" * 64
    if planted:
        assert (r.status, r.first_bad, r.out_len) == (E_BAD_CHECKSUM, min(planted), 0), (r.status, r.first_bad)
    else:
        assert (r.status, r.first_bad, r.out_len) == (OK, NOBODY, total), (r.status, r.first_bad)
        assert host(out[:total]) == data


def unjoin(L, gz, stream, off, out_off, flags):
    """one hdlz_unjoin_ws / hdlz_unjoin_gzip_ws: junk in every output -> (record, member statuses, out)"""
    B, total = len(off) - 1, int(out_off[-1])
    work_bytes, call, Result = (L.hdlz_unjoin_gzip_work_bytes, L.hdlz_unjoin_gzip_ws, _lib.UnjoinGzipResult) if gz else \
        (L.hdlz_unjoin_work_bytes, L.hdlz_unjoin_ws, _lib.UnjoinResult)
    d_stream, d_off, d_out_off = dev_bytes(stream, 8), dev_i64(off), dev_i64(out_off)
    out = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    member = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    result = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    wb = work_bytes(B, total, flags)
    work = torch.full((max(wb, 1),), 0x5A, dtype=torch.uint8, device="cuda")
    rc = call(d_stream.data_ptr(), len(stream), d_off.data_ptr(), d_out_off.data_ptr(), 0, B, flags, out.data_ptr(), total, member.data_ptr(),
              result.data_ptr(), work.data_ptr(), wb, stream_ptr())
    assert rc == 0, L.hdlz_last_error()
    torch.cuda.synchronize()
    assert host(out[total:]) == b"\xa5" * 64
    return Result.from_buffer_copy(host(result)), member.cpu().numpy(), out[:total]


def without_marker(stream, offsets, members):
    """the stream with FF FF -> FF FE at the end of each of `members`"""
    z = bytearray(stream)
    for k in members:
        assert z[offsets[k + 1] - 2:offsets[k + 1]] == b"\xff\xff"
        z[offsets[k + 1] - 1] ^= 0x01
    return bytes(z)


def check_unjoin(engine, gz, j, out_off, data, flags, planted):
    rec, st, out = unjoin(engine.lib, gz, without_marker(j.stream, j.offsets, planted), j.offsets, out_off, flags)
    check = rec.crc if gz else rec.adler
    assert np.nonzero(st)[0].tolist() == sorted(planted) and all(st[b] == E_NO_EOF for b in planted), (flags, planted, np.nonzero(st)[0][:8])
    if planted:
        assert (rec.status, rec.first_bad, rec.out_len, check) == (E_NO_EOF, min(planted), 0, 0), (flags, planted, rec.status, rec.first_bad)
    else:
        assert (rec.status, rec.first_bad, rec.out_len, check) == (OK, NOBODY, len(data), j.crc if gz else j.adler), (flags, rec.status, rec.first_bad)
        assert host(out) == data


@pytest.mark.parametrize("flags", [LANE, WAVE, GROUP])
def test_unjoin_of_65836_members_under_every_mapping(engine, flags):
    """hdlz_unjoin_ws: k_unjoin_finish takes lowest_word with 256 threads -- a second word from 65537 members on"""
    blocks, mlen, data = S.pooled_batch(S.MANY, True)
    j = joined_ref.expected_joined(blocks, 32, 10)
    assert zlib.decompress(j.stream) == data and np.array_equal(np.diff(j.offsets), mlen)
    out_off = np.concatenate([[0], np.cumsum([len(b) for b in blocks])])
    for planted in PLANTS:
        check_unjoin(engine, False, j, out_off, data, flags, planted)
    d = dev_bytes(j.stream, 8)
    back = engine.inflate_joined(d, dev_i64(j.offsets), out_offsets=dev_i64(out_off), total=len(data), flags=flags)
    assert host(back) == data


def test_unjoin_gzip_of_262401_members(engine):
    """hdlz_unjoin_gzip_ws: k_unjoin_gzip_finish takes lowest_word with CRC_FIN_THREADS = 1024 threads, so ITS second word comes with
    judge group 1024 -- 262145 members and more"""
    threads = S.LOWEST_THREADS["unjoin gzip"]
    B = S.JOIN_ROWS[1]
    assert B >= S.THRESHOLDS["lowest_word"]["unjoin gzip"]["second"] + 5
    blocks, mlen, data = S.pooled_batch(B, True)
    g = gzip_ref.expected_gzip(blocks, 32, 10)
    assert gzip.decompress(g.stream) == data
    out_off = np.concatenate([[0], np.cumsum([len(b) for b in blocks])])
    high = threads * S.JT + 5
    for planted in ((), (high,), (S.PLANT_LOW, high)):
        check_unjoin(engine, True, g, out_off, data, 0, planted)


# ---- the joins of more than 65536 and more than 262144 rows
class GzipCall(ZlibCall):
    """the buffers of one CRC + compress + gzip join (tests/test_gpu_gzip.py's Call)"""

    def __init__(self, engine, blocks, **kw):
        ZlibCall.__init__(self, engine, blocks, **kw)
        self.cap = self.L.hdlz_join_gzip_bound(self.B, kw["bound"])
        self.stream = torch.zeros(self.cap, dtype=torch.uint8, device="cuda")
        self.n = sum(len(b) for b in blocks)
        self.crc = torch.full((1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        self.crc_wb = self.L.hdlz_crc32_work_bytes(self.n)
        self.crc_work = torch.zeros(max(self.crc_wb, 4) // 4, dtype=torch.int32, device="cuda")

    def join(self):
        L = self.L
        rc = L.hdlz_crc32_ws(self.d_in.data_ptr(), self.n, self.crc.data_ptr(), self.crc_work.data_ptr(), self.crc_wb, stream_ptr())
        assert rc == 0, L.hdlz_last_error()
        rc = L.hdlz_join_gzip_ws(self.rows.data_ptr(), self.pitch, self.out_len.data_ptr(), self.end_bits.data_ptr(), self.status.data_ptr(),
                                 self.in_off.data_ptr(), self.in_len, self.B, self.crc.data_ptr(), self.stream.data_ptr(), self.cap,
                                 self.off.data_ptr(), self.result.data_ptr(), self.work.data_ptr(), self.wb, stream_ptr())
        assert rc == 0, L.hdlz_last_error()

    def record(self):
        torch.cuda.synchronize()
        r = _lib.JoinGzipResult.from_buffer_copy(host(self.result))
        return r.stream_len, r.status, r.crc


@pytest.mark.parametrize("container", ["zlib", "gzip"])
@pytest.mark.parametrize("B", S.JOIN_ROWS)
def test_join_of_more_rows_than_one_trip_of_the_finish(engine, B, container):
    """256 * 256 + 1 and 1024 * 256 + 257 ragged blocks of 5 .. 64 bytes: every thread of k_join_finish / k_join_gzip_finish takes a
    second tile (t += 256), and the lift of the gzip index by 8 takes a second row a thread in workgroups 0 and 1 of 1024.  The
    stream is read by stock zlib, the checksum is the host's, d_off the cumulative sum of joined_ref's member lengths; a failed row
    in tile 300 (of 257 tiles: in tile 256) is the record's status"""
    gz = container == "gzip"
    blocks, mlen, data = S.pooled_batch(B)
    Call, head = (GzipCall, 10) if gz else (ZlibCall, 2)
    c = Call(engine, blocks, bound=64)
    c.compress()
    c.join()
    slen, st, check = c.record()
    want_off = head + np.concatenate([[0], np.cumsum(mlen)])
    assert (slen, st, check) == (int(want_off[-1]) + (10 if gz else 6), OK, zlib.crc32(data) if gz else zlib.adler32(data)), (slen, st, hex(check))
    assert first_diff(c.off.cpu().numpy(), want_off) is None, first_diff(c.off.cpu().numpy(), want_off)
    z = host(c.stream[:slen])
    assert (gzip.decompress(z) if gz else zlib.decompress(z)) == data
    failed = list(blocks)
    failed[S.join_failed_row(B)] = b"abcd"
    c = Call(engine, failed, bound=64)
    c.compress()
    c.join()
    assert c.record() == (0, E_SHORT_INPUT, 0)
