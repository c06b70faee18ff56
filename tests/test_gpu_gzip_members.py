"""GPU (-m gpu): include/hdlz_gzip_members.h on the device -- the index against the numpy rule of tests/gzip_members_ref.py (member
starts and planted look-alikes around every multiple of 4 KiB, the file's ends, capacity, the guesses), the verified read against the
member verdict (300 members, every header field, sub-ranges, every way a member can miss its slot or its span, a BGZF file), and
Engine.read_gzip_bytes against Engine.inflate_gzip_bytes on clean and crafted files WITH the route each file must take: the clean
files need no repair by the rule alone (tests/test_gzip_members_cabi.py), so the fallback cannot hide a failing device path."""
import gzip

import numpy as np
import pytest
import torch

import gunzip_ref as G
import gzip_members_ref as R

pytestmark = pytest.mark.gpu
SENTINEL = -0x0123456789ABCDEF


def dev(z):
    return torch.from_numpy(np.frombuffer(bytes(z) + b"\xAA" * 32, np.uint8).copy()).cuda()[:len(z)]


def raw_index(engine, z, cap):
    """hdlz_gzip_members_index_ws with room for exactly `cap` members -> (off, out_off: cap + 1 words with a sentinel behind, record)"""
    from hdl_deflate_amd import _lib
    L, d = engine.lib, dev(z)
    off, out_off = (torch.full((cap + 2,), SENTINEL, dtype=torch.int64, device="cuda") for _ in range(2))
    res = torch.zeros(3, dtype=torch.int64, device="cuda")
    wb = L.hdlz_gzip_members_index_work_bytes(len(z))
    work = torch.empty(max(wb, 1), dtype=torch.uint8, device="cuda")
    rc = L.hdlz_gzip_members_index_ws(d.data_ptr() if len(z) else None, len(z), cap, off.data_ptr(), out_off.data_ptr(), res.data_ptr(),
                                      work.data_ptr() if wb else None, wb, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.hdlz_last_error()
    return off.cpu().tolist(), out_off.cpu().tolist(), _lib.GzipMembersIndexResult.from_buffer_copy(res.cpu().numpy().tobytes())


def check_index(engine, label, z, cap=None):
    want_off, want_out = R.index_rule(z)
    M = len(want_off) - 1
    cap = M if cap is None else cap
    off, out_off, rec = raw_index(engine, z, cap)
    k = min(M, cap) + 1
    assert (rec.nmembers, rec.total_out, rec.reserved) == (M, want_out[-1], 0), (label, rec.nmembers, M, rec.total_out, want_out[-1])
    assert rec.status == (R.E_OUT_CAPACITY if M > cap else R.OK), (label, rec.status)
    assert off[:k] == want_off[:k], (label, [(i, a, b) for i, (a, b) in enumerate(zip(off[:k], want_off[:k])) if a != b][:5])
    assert out_off[:k] == want_out[:k], (label, [(i, a, b) for i, (a, b) in enumerate(zip(out_off[:k], want_out[:k])) if a != b][:5])
    assert set(off[k:]) <= {SENTINEL} and set(out_off[k:]) <= {SENTINEL}, (label, "words behind min(M, cap) were written")
    return want_off


# ---- the index
@pytest.mark.parametrize("d", range(-3, 4))
def test_index_member_starts_and_lookalikes_around_every_4k(engine, d):
    """even multiples of 4 KiB (+ d): a member starts there; odd ones: a look-alike planted in a stored payload -- up to 256 KiB"""
    starts = [0] + [k * 4096 + d for k in range(2, 65, 2)]
    planted = [k * 4096 + d for k in range(1, 65, 2)]
    z = R.plant(R.place(starts, 65 * 4096 + 100, seed=d + 3), planted)
    assert R.candidates(z) == sorted(starts + planted)
    check_index(engine, d, z)


def test_index_edges_of_the_file_and_of_the_rule(engine):
    x = R.clean_bytes(5000, 1)
    files = [("empty", b""), ("1 byte", b"\x1f"), ("3 bytes", b"\x1f\x8b\x08"), ("4 bytes", R.MAGIC), ("4 other bytes", b"abcd"),
             ("17 bytes", R.MAGIC + bytes(13)), ("17 bytes with an ISIZE", bytes(13) + b"\x05\0\0\0"), ("18 bytes", bytes(14) + b"\x05\0\0\0"),
             ("the guess clamped", bytes(14) + b"\xff\xff\xff\xff"), ("no magic in front", x), ("two adjacent look-alikes", x[:777] + R.MAGIC * 2 + x[777:]),
             ("a candidate at file_len - 4", x + R.MAGIC), ("none at file_len - 3", x + R.MAGIC[:3]), ("none at file_len - 3, a flag behind", x[:3000] + R.MAGIC[:3]),
             ("a reserved flag bit", x[:100] + b"\x1f\x8b\x08\x20" + x[100:]), ("flag 1F", x[:100] + b"\x1f\x8b\x08\x1f" + x[100:]),
             ("a candidate every 3 bytes", x[:1000] + b"\x1f\x8b\x08" * 700 + x[1000:]), ("a candidate every 4 bytes", R.MAGIC * 9000),
             ("members of 23 bytes", R.stored(b"") * 3000),
             ("a stored member over seven windows", R.stored_of_length(7 * 32768 + 11, 5) + R.stored(b"tail")),
             ("a look-alike whose guess is clamped", R.plant(R.stored_of_length(40000, 6), [20000], R.MAGIC) + b"\xff\xff\xff\xff" + R.stored(b"z"))]
    for label, z in files:
        off = check_index(engine, label, z)
        if label == "a candidate at file_len - 4":
            assert off[-2] == len(z) - 4
        if label.startswith("none at"):
            assert off == [0, len(z)]
    z = dict(files)["members of 23 bytes"]
    for cap in (0, 1, 5, 2999, 3000, 3001):
        check_index(engine, ("member_cap", cap), z, cap)
    off, out_off, rec = engine.gzip_index(dev(z), member_cap=7)                 # the engine asks once more with the true count
    assert rec.status == R.OK and rec.nmembers == 3000 and off.cpu().tolist() == R.index_rule(z)[0]


# ---- the verified read
def read(engine, z, off, out_off, out_cap=None, members=None):
    d = dev(z)
    idx = (torch.tensor(off, dtype=torch.int64).cuda(), torch.tensor(out_off, dtype=torch.int64).cuda())
    if out_cap is None:
        out, st, rec = engine.inflate_gzip_members(d, index=idx, members=members)
    else:
        out = torch.empty(out_cap, dtype=torch.uint8, device="cuda")
        B = len(off) - 1
        st = torch.empty(B, dtype=torch.int32, device="cuda")
        from hdl_deflate_amd import _lib
        res = engine._gzip_members_call(d, idx[0], idx[1], B, out, out_cap, st)
        rec = _lib.GzipMembersInflateResult.from_buffer_copy(res.cpu().numpy().tobytes())
    torch.cuda.synchronize()
    return bytes(out.cpu().numpy().tobytes()), st.cpu().tolist(), rec


def check_read(engine, oracle, label, z, off, out_off, out_cap=None):
    out, st, rec = read(engine, z, off, out_off, out_cap)
    room = out_off[-1] - out_off[0] if out_cap is None else out_cap
    first = None
    for b in range(len(off) - 1):
        want, data = R.verdict(oracle, z, off[b], off[b + 1], out_off[b + 1] - out_off[b], out_room=room - (out_off[b] - out_off[0]))
        if want is None:
            assert st[b] != R.OK, (label, b)
        else:
            assert st[b] == want, (label, b, st[b], want)
        if st[b] == R.OK:
            assert out[out_off[b] - out_off[0]:out_off[b + 1] - out_off[0]] == data, (label, b, "bytes")
        elif first is None:
            first = b
    if first is None:
        assert (rec.status, rec.first_bad, rec.out_len, rec.reserved) == (R.OK, (1 << 64) - 1, out_off[-1] - out_off[0], 0), label
    else:
        assert (rec.status, rec.first_bad, rec.out_len) == (st[first], first, 0), (label, rec.status, rec.first_bad)
    return st


def test_read_300_members_of_every_level(engine, oracle):
    ms, datas = R.many_members()
    z = b"".join(ms)
    off, out_off, rec = engine.gzip_index(dev(z))
    off, out_off = off.cpu().tolist(), out_off.cpu().tolist()
    assert rec.nmembers == 300 and (off, out_off) == R.index_rule(z)
    assert out_off == [0] + list(np.cumsum([len(d) for d in datas])) and any(o % 4 for o in out_off)      # the guess is right; slots unaligned
    assert check_read(engine, oracle, "300", z, off, out_off) == [R.OK] * 300
    out, st, rec = engine.inflate_gzip_members(dev(z))
    assert bytes(out.cpu().numpy().tobytes()) == b"".join(datas) and rec.out_len == len(out)
    for b0, b1 in ((17, 123), (0, 1), (299, 300), (7, 8), (150, 150)):       # sub-ranges: member 7 is gzip.compress(b"")
        out, st, rec = engine.inflate_gzip_members(dev(z), members=(b0, b1))
        assert bytes(out.cpu().numpy().tobytes()) == b"".join(datas[b0:b1]) and st.cpu().tolist() == [R.OK] * (b1 - b0) and rec.status == R.OK


def test_read_every_header_field_as_members_of_one_file(engine, oracle):
    cases = G.header_cases()
    off = [0] + list(np.cumsum([len(c) for _, c in cases]))
    z = b"".join(c for _, c in cases)
    out_off = [0]
    for label, c in cases:
        e = G.member(oracle, c, 300)
        out_off.append(out_off[-1] + (e["out_len"] if e["status"] == R.OK else 300))
    st = check_read(engine, oracle, "header cases", z, [int(o) for o in off], out_off)
    ok = [label for (label, _), s in zip(cases, st) if s == R.OK]
    assert "all four" in ok and "XLEN 65535 FHCRC" in ok and "gzip.compress(b\"\")" in ok and "name of 300, comment of 64" in ok
    assert len(ok) == sum(1 for _, c in cases if G.zaccepts(c) is not None and G.zaccepts(c)[1] == len(c))


def test_read_members_that_miss_their_slot_or_their_span(engine, oracle):
    d = G.text(2000, 61)
    good = G.gz(d, name=b"g")
    parts = [("good", good, 2000), ("longer than its slot", good, 1999), ("shorter than its slot", good, 2001), ("wrong CRC", G.gz(d, crc_xor=4), 2000),
             ("wrong ISIZE", G.gz(d, isize_add=1), 2000), ("ISIZE is the slot's, not the data's", G.gz(d, isize_add=1), 2001), ("cut", good[:-3], 2000),
             ("cut in the payload", good[:200], 2000), ("padding behind", good + bytes(5), 2000), ("a slot of nothing", good, 0),
             ("an empty member", gzip.compress(b"", mtime=1), 0), ("an empty member, a slot of 1", gzip.compress(b"", mtime=1), 1), ("good again", good, 2000)]
    off = [0] + list(np.cumsum([len(p) for _, p, _ in parts]))
    out_off = [5] + [5 + int(o) for o in np.cumsum([n for _, _, n in parts])]
    z = b"".join(p for _, p, _ in parts)
    st = check_read(engine, oracle, "slots and spans", z, [int(o) for o in off], out_off)
    assert st == [R.OK, R.E_OUT_CAPACITY, R.E_BAD_CHECKSUM, R.E_BAD_CHECKSUM, R.E_BAD_CHECKSUM, R.E_BAD_CHECKSUM, R.E_NO_EOF, st[7], R.E_NO_EOF,
                  st[9], R.OK, R.E_BAD_CHECKSUM, R.OK] and st[7] != R.OK and st[9] != R.OK
    # the index checks: a reversed span, a span behind the file, a reversed slot, a slot that ends behind out_cap
    n = len(good)
    zz = good * 4
    assert check_read(engine, oracle, "reversed span", zz, [0, 2 * n, n, 4 * n], [0, 2000, 4000, 6000]) == [R.E_NO_EOF, R.E_BAD_PARAM, R.E_NO_EOF]
    assert check_read(engine, oracle, "behind the file", zz, [0, n, 2 * n, 4 * n + 1], [0, 2000, 4000, 6000]) == [R.OK, R.OK, R.E_BAD_PARAM]
    e = gzip.compress(b"", mtime=1)              # (an empty member in front: the slot behind a reversed one overlaps it, and it writes nothing)
    assert check_read(engine, oracle, "reversed slot", e + zz, [0, 20, 20 + n, 20 + 2 * n], [0, 2000, 0, 2000]) == [R.E_BAD_CHECKSUM, R.E_BAD_PARAM, R.OK]
    assert check_read(engine, oracle, "behind out_cap", zz, [0, n, 2 * n, 3 * n], [0, 2000, 4000, 6000], out_cap=5999) == [R.OK, R.OK, R.E_BAD_PARAM]


def test_read_a_bgzf_file_without_its_size_field(engine):
    data = (G.text(200000, 71) + R.clean_bytes(150001, 72)) * 2
    d = torch.from_numpy(np.frombuffer(data + bytes(32), np.uint8).copy()).cuda()[:len(data)]
    for stored in (False, True):
        f = engine.compress_bgzf(d, stored=stored)
        boff, bout, brec = engine.bgzf_index(f)
        off, out_off, rec = engine.gzip_index(f)
        assert rec.status == R.OK and torch.equal(off, boff) and torch.equal(out_off, bout), "the guess is BGZF's own index"
        out, st, rec = engine.inflate_gzip_members(f, index=(off, out_off))
        assert rec.status == R.OK and int(st.abs().sum()) == 0 and torch.equal(out, engine.inflate_bgzf(f)) and torch.equal(out, d)


# ---- the file level
def _cases():
    return R.file_cases()


@pytest.mark.parametrize("k", range(len(_cases())), ids=[label for label, _, _ in _cases()])
def test_read_gzip_bytes_is_inflate_gzip_bytes_by_the_expected_route(engine, k):
    label, z, repairs = _cases()[k]
    want = engine.inflate_gzip_bytes(z)
    assert want[0] != R.E_OUT_CAPACITY and (want == (R.OK, gzip.decompress(z)) if R.gzip_accepts(z) is not None else want[0] != R.OK)
    assert engine.read_gzip_bytes(z) == want, label
    out, report = engine.read_gzip(dev(z))
    assert (report.status, bytes(out.cpu().numpy().tobytes())) == want
    assert report.repairs == repairs and report.big == 0, (label, report.repairs, repairs)       # a condition, not a tolerance
    assert report.candidates == len(R.candidates(z)) and len(report.member_status) == report.candidates
    if repairs == 0:
        assert report.members == report.candidates and not report.member_status.any()


def test_big_member_forced_low_changes_the_route_not_the_bytes(engine):
    for label, z, _ in [_cases()[k] for k in (0, 1, 3, 4, 5)]:
        want = engine.inflate_gzip_bytes(z)
        for big in (1, 2000):
            d = dev(z)
            out, report = engine.read_gzip(d, big_member=big)
            assert (report.status, bytes(out.cpu().numpy().tobytes())) == want, (label, big)
            off = R.index_rule(z)[0]
            nbig = sum(1 for b in range(len(off) - 1) if off[b + 1] - off[b] >= big)
            assert (report.big > 0) == (nbig > 0) and (big != 1 or (report.big + report.repairs == report.members and (report.member_status == -1).all())), (label, big)
