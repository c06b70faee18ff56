"""GPU (-m gpu): BGZF on the device (include/hdlz_bgzf.h) -- hdlz_crc32_batch_ws against zlib.crc32, hdlz_bgzf_join_ws byte for byte
against bgzf_ref's framing of the CPU oracle's rows and read by Python's gzip, hdlz_bgzf_index_ws against bgzf_ref's serial walk (both
arrays and the whole record) on files that stock zlib built, hdlz_bgzf_inflate_ws on all of them and on damaged ones, and the Engine's
methods.  bgzf_ref itself is held against gzip.decompress in tests/test_bgzf_cabi.py."""
import gzip
import zlib

import numpy as np
import pytest
import torch

import bgzf_ref
from bgzf_ref import OK, E_OUT_CAPACITY, E_NO_EOF, E_BAD_PARAM, E_BAD_HEADER, E_BAD_CHECKSUM, EOF, member
from hdl_deflate_amd import _lib
from hdl_deflate_amd.constants import out_bound, pitch_for
from hdl_deflate_amd.errors import Error, HdlzStatusError

pytestmark = pytest.mark.gpu

NOBODY = (1 << 64) - 1
LEVELS = (0, 1, 6, 9)
W = 65536


def dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype)).cuda()


def dev_bytes(b, slack=0):
    return dev(np.frombuffer(bytes(b) + bytes(slack), np.uint8))


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


# ---- hdlz_crc32_batch_ws
LENGTHS = [0, 1, 3, 4, 127, 128, 129, 32767, 32768, 32769, 65536, 70001]


def test_crc32_batch_ragged_at_odd_offsets(engine):
    """one ragged batch of every length, twice over, the buffer one and fifteen bytes off a 16-byte boundary: block starts of every
    alignment; the blocks lie back to back, so a byte read from a neighbour changes a word"""
    L = engine.lib
    lens = LENGTHS + LENGTHS[::-1]
    h = np.random.default_rng(41).integers(0, 256, sum(lens) + 64, dtype=np.uint8)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    d = dev(h)
    assert d.data_ptr() % 16 == 0
    for shift, first in ((1, 0), (15, 1000)):
        d_off = dev(offs + first)                                     # d_off[0] need not be 0: offsets are relative to it
        crc = torch.full((len(lens),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        rc = L.hdlz_crc32_batch_ws(d.data_ptr() + shift, d_off.data_ptr(), 0, 0, len(lens), crc.data_ptr(), stream_ptr())
        assert rc == 0, L.hdlz_last_error()
        got = [int(x) & 0xFFFFFFFF for x in crc.cpu().numpy()]
        hb = h.tobytes()
        want = [zlib.crc32(hb[shift + a:shift + b]) for a, b in zip(offs, offs[1:])]
        assert got == want, [(n, hex(g), hex(w)) for n, g, w in zip(lens, got, want) if g != w][:6]


@pytest.mark.parametrize("kind", ["random", "zeros"])
def test_crc32_batch_pitched(engine, kind):
    """three rows of every length at an odd pitch (zeros: only the length speaks); the Engine's method on the same rows"""
    L = engine.lib
    for n in LENGTHS:
        pitch = n + 3
        h = np.random.default_rng(n).integers(0, 256, 3 * pitch + 16, dtype=np.uint8) if kind == "random" else np.zeros(3 * pitch + 16, np.uint8)
        d = dev(h)
        crc = torch.full((3,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        rc = L.hdlz_crc32_batch_ws(d.data_ptr() + 1, None, pitch, n, 3, crc.data_ptr(), stream_ptr())
        assert rc == 0, L.hdlz_last_error()
        hb = h.tobytes()
        assert [int(x) & 0xFFFFFFFF for x in crc.cpu().numpy()] == [zlib.crc32(hb[1 + b * pitch:1 + b * pitch + n]) for b in range(3)], n
        t = engine.crc32_batch(d[1:1 + 3 * pitch].view(3, pitch), length=n)
        assert t.dtype == torch.uint32 and [int(x) for x in t.cpu().numpy()] == [zlib.crc32(hb[1 + b * pitch:1 + b * pitch + n]) for b in range(3)]


# ---- hdlz_bgzf_join_ws
class Write(object):
    """CRC + compress + BGZF join of a ragged batch: every output pre-filled with junk"""

    def __init__(self, engine, blocks, bound, cap=None):
        L = self.L = engine.lib
        B = self.B = len(blocks)
        self.pitch = pitch_for(max(bound, 5))
        flat = np.frombuffer(b"".join(blocks) + bytes(64), np.uint8)
        self.in_off = dev(np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).astype(np.int64))
        self.d_in = dev(flat)
        self.rows = torch.full((max(B, 1), self.pitch), 0xA5, dtype=torch.uint8, device="cuda")
        self.out_len, self.status, self.crc = (torch.full((max(B, 1),), -1, dtype=torch.int32, device="cuda") for _ in range(3))
        self.cap = L.hdlz_bgzf_bound(B, bound) if cap is None else cap
        self.file = torch.full((self.cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        self.off = torch.full((B + 1,), -1, dtype=torch.int64, device="cuda")
        self.result = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        wb = L.hdlz_bgzf_join_work_bytes(B)
        self.work = torch.full((max(wb, 8) // 8,), -1, dtype=torch.int64, device="cuda")
        rc = L.hdlz_crc32_batch_ws(self.d_in.data_ptr(), self.in_off.data_ptr(), 0, 0, B, self.crc.data_ptr(), stream_ptr())
        assert rc == 0, L.hdlz_last_error()
        if B:
            rc = L.hdlz_compress_batch(self.d_in.data_ptr(), self.in_off.data_ptr(), 0, bound, B, 32, 10, self.rows.data_ptr(), self.pitch,
                                       self.out_len.data_ptr(), self.status.data_ptr(), stream_ptr())
            assert rc == 0, L.hdlz_last_error()
        rc = L.hdlz_bgzf_join_ws(self.rows.data_ptr(), self.pitch, self.out_len.data_ptr(), self.status.data_ptr(), self.in_off.data_ptr(), bound,
                                 B, self.crc.data_ptr(), self.file.data_ptr(), self.cap, self.off.data_ptr(), self.result.data_ptr(),
                                 self.work.data_ptr() if wb else None, wb, stream_ptr())
        assert rc == 0, L.hdlz_last_error()
        torch.cuda.synchronize()
        self.rec = _lib.BgzfJoinResult.from_buffer_copy(self.result.cpu().numpy().tobytes())
        self.bytes = self.file.cpu().numpy().tobytes()
        self.offsets = [int(x) for x in self.off.cpu().numpy()]


def oracle_rows(oracle, blocks):
    rows = []
    for b in blocks:
        rc, z = oracle.compress(bytes(b), 32, 10)
        assert rc == 0
        rows.append(z)
    return rows


def ragged(lengths, seed):
    r = np.random.default_rng(seed)
    pool = bgzf_ref.data(1 << 16, seed)
    return [pool[a:a + n] for n in lengths for a in [int(r.integers(0, (1 << 16) - n + 1))]]


WRITER_BATCHES = [("fives", [5] * 7, 64), ("small", [5, 31, 31, 6, 17, 31, 5], 31), ("2k", [2048, 5, 2047, 2048, 31, 1999], 2048),
                  ("tiles", [5 + k % 60 for k in range(513)], 64), ("one large", [57344], 57344)]


@pytest.mark.parametrize("label, lengths, bound", WRITER_BATCHES, ids=[b[0] for b in WRITER_BATCHES])
def test_the_file_is_the_framing_of_the_rows(engine, oracle, label, lengths, bound):
    blocks = ragged(lengths, len(lengths))
    want, offs = bgzf_ref.framed_rows(oracle_rows(oracle, blocks), blocks)
    w = Write(engine, blocks, bound)
    assert (w.rec.file_len, w.rec.status, w.rec.first_bad) == (len(want), OK, 0xFFFFFFFF)
    assert w.offsets == offs
    assert w.bytes[:len(want)] == want, next(k for k in range(len(want)) if w.bytes[k] != want[k])
    assert gzip.decompress(w.bytes[:len(want)]) == b"".join(blocks)
    assert w.bytes[w.cap:] == b"\xa5" * 64
    walk = bgzf_ref.walk(want)
    assert walk.off[:-1] == offs and walk.record() == (len(blocks) + 1, sum(lengths), len(want), OK, 1)


def test_no_blocks_and_a_short_capacity(engine, oracle):
    w = Write(engine, [], 64)
    assert (w.rec.file_len, w.rec.status, w.rec.first_bad) == (28, OK, 0xFFFFFFFF) and w.bytes[:28] == EOF and w.offsets == [0] and w.cap == 28
    blocks = ragged([40, 5, 64, 33, 12], 9)
    want, offs = bgzf_ref.framed_rows(oracle_rows(oracle, blocks), blocks)
    for cap in (len(want) - 1, len(want) - 28, offs[3] + 5, 17, 0):
        w = Write(engine, blocks, 64, cap=cap)
        assert (w.rec.file_len, w.rec.status, w.rec.first_bad) == (len(want), E_OUT_CAPACITY, 0xFFFFFFFF), cap
        assert w.offsets == offs
        fits = max(o for o in [0] + offs if o <= cap)
        assert w.bytes[:fits] == want[:fits], cap
        assert w.bytes[cap:] == b"\xa5" * 64, cap                       # never a byte at or behind file_cap


def test_the_limits_of_a_member(engine, oracle):
    """bytes of 144 .. 255 cost nine bits each as literals: 58230 of them always fit a member, 65536 of them do not"""
    r = np.random.default_rng(5)
    fits, over = (bytes(r.integers(144, 256, n, dtype=np.uint8)) for n in (58230, 65536))
    rows = oracle_rows(oracle, [fits, over])
    assert len(rows[0]) <= 65516 < len(rows[1])
    w = Write(engine, [fits], 58230)
    want, _ = bgzf_ref.framed_rows(rows[:1], [fits])
    assert (w.rec.file_len, w.rec.status) == (len(want), OK) and w.bytes[:len(want)] == want and gzip.decompress(want) == fits
    w = Write(engine, [fits[:100], over, fits[:50]], 65536)
    assert (w.rec.file_len, w.rec.status, w.rec.first_bad) == (0, E_OUT_CAPACITY, 1)
    w = Write(engine, [fits[:100], b"abcd", over], 65536)              # the worst status comes first (E_SHORT_INPUT = 1 < E_OUT_CAPACITY = 2)
    assert (w.rec.file_len, w.rec.status, w.rec.first_bad) == (0, E_OUT_CAPACITY, 1)


# ---- the files of the index and the reader tests: built by stock zlib, once
def stored(size, seed, fill=None):
    """a level-0 member of exactly `size` bytes -> (member, payload): 26 bytes of frame, the payload verbatim behind a stored block's
    five header bytes, and, where zlib closes a long payload with a second, empty stored block (BFINAL is honoured), five more"""
    for n in (size - 31, size - 36):
        payload = bytearray(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes())
        if fill:
            at, what = fill
            payload[at:at + len(what)] = what
        m = member(bytes(payload), 0) if n <= 65500 else b""
        if len(m) == size:
            break
    assert len(m) == size and m[23:23 + n] == payload
    return m, bytes(payload)


_files = {}


def files():
    """label -> (file, data or None): every file of the index tests"""
    if _files:
        return _files
    sizes = (0, 1, 100, 65280, 65536)
    for level in LEVELS:
        parts = [bgzf_ref.data(n, 7 * n + level) for n in sizes if not (level == 0 and n == 65536)]      # (stored: 64 KiB do not fit)
        parts.insert(3, b"")                                          # an empty member in the middle
        body = b"".join(member(p, level) for p in parts)
        _files["level %d with EOF" % level] = (body + EOF, b"".join(parts))
        _files["level %d without EOF" % level] = (body, b"".join(parts))
    # member starts exactly at, one byte before and 17 bytes before a multiple of 65536 (the last: a header that straddles the seam)
    ms = [stored(W, 1), stored(W - 1, 2), stored(W - 16, 3), stored(40000, 4)]
    assert [sum(len(m[0]) for m in ms[:k]) for k in (1, 2, 3)] == [W, 2 * W - 1, 3 * W - 17]
    tail = [bgzf_ref.data(n, n) for n in (30000, 65536, 9, 50000)]
    _files["seams"] = (b"".join(m[0] for m in ms) + b"".join(member(p, 6) for p in tail) + EOF, b"".join(m[1] for m in ms) + b"".join(tail))
    # a complete look-alike header inside a stored payload, in FRONT of its window's true start: M0 [0, 40000), M1 [40000, 100000) stored,
    # M2 at 100000 is window 1's true start; the fake stands at 70000.  Variant 1: its size leads to 100000 (and the four bytes in
    # front of that, M1's ISIZE, pass for its own); variant 2: its size leads into M1's payload.
    for label, fake_size in (("fake header lands on a true start", 30000), ("fake header runs off into data", 20000)):
        m0 = stored(40000, 5)
        m1 = stored(60000, 6, fill=(70000 - 40000 - 23, bgzf_ref.header(fake_size)))
        rest = [bgzf_ref.data(n, n + 1) for n in (20000, 65536, 300)]
        f = m0[0] + m1[0] + b"".join(member(p, 6) for p in rest) + EOF
        assert bgzf_ref.is_header(f[70000:70018]) and f[100000:100004] == b"\x1f\x8b\x08\x04"
        _files[label] = (f, m0[1] + m1[1] + b"".join(rest))
    for label, f, _ in bgzf_ref.damaged_files():
        _files[label] = (f, None)
    long_garbage = _files["seams"][0] + bytes(2 * W) + EOF                 # the walk stops two windows in front of the file's end
    _files["windows behind the stop"] = (long_garbage, None)
    return _files


FILE_LABELS = ["level %d %s EOF" % (lv, w) for lv in LEVELS for w in ("with", "without")] + \
    ["seams", "fake header lands on a true start", "fake header runs off into data", "windows behind the stop"] + [c[0] for c in bgzf_ref.damaged_files()]


class Index(object):
    def __init__(self, L, f, cap=None, junk=-1):
        w = bgzf_ref.walk(f)
        self.cap = cap = w.nmembers if cap is None else cap
        self.d_file = dev_bytes(f, 1)
        self.off, self.out_off = (torch.full((cap + 1 + 8,), junk, dtype=torch.int64, device="cuda") for _ in range(2))
        self.result = torch.full((4,), junk, dtype=torch.int64, device="cuda")
        wb = L.hdlz_bgzf_index_work_bytes(len(f))
        self.work = torch.full((max(wb, 8) // 8,), junk, dtype=torch.int64, device="cuda")
        rc = L.hdlz_bgzf_index_ws(self.d_file.data_ptr() if f else None, len(f), cap, self.off.data_ptr(), self.out_off.data_ptr(),
                                  self.result.data_ptr(), self.work.data_ptr() if wb else None, wb, stream_ptr())
        assert rc == 0, L.hdlz_last_error()
        torch.cuda.synchronize()
        r = _lib.BgzfIndexResult.from_buffer_copy(self.result.cpu().numpy().tobytes())
        self.record = (r.nmembers, r.total_out, r.file_used, r.status, r.eof_marker)
        self.offs, self.out_offs = ([int(x) for x in t.cpu().numpy()] for t in (self.off, self.out_off))


@pytest.mark.parametrize("label", FILE_LABELS)
def test_the_index_is_the_serial_walk(engine, label):
    f, data = files()[label]
    w = bgzf_ref.walk(f)
    if data is not None:
        assert w.status == OK and gzip.decompress(f) == data
    for junk in (-1, 0x0102030405060708):                              # neither the outputs' nor the scratch's contents reach a result
        x = Index(engine.lib, f, junk=junk)
        assert x.record == w.record(), (label, x.record, w.record())
        assert x.offs[:w.nmembers + 1] == w.off and x.out_offs[:w.nmembers + 1] == w.out_off, label
        assert x.offs[w.nmembers + 1:] == [junk] * 8 and x.out_offs[w.nmembers + 1:] == [junk] * 8


def test_the_speculation_is_what_the_fake_headers_break(engine):
    """the two look-alike files are what they claim: window 1's first header-shaped bytes are the fake, and a walk from it counts wrong"""
    for label, lands in (("fake header lands on a true start", True), ("fake header runs off into data", False)):
        f, _ = files()[label]
        first = next(p for p in range(W, 2 * W) if bgzf_ref.is_header(f[p:p + 18]))
        assert first == 70000 and bgzf_ref.walk(f).off[2] == 100000
        size = int.from_bytes(f[first + 16:first + 18], "little") + 1
        assert (first + size == 100000) == lands and (lands or not bgzf_ref.is_header(f[first + size:first + size + 18]))


def test_member_cap_one_too_small(engine):
    f, _ = files()["level 6 with EOF"]
    w = bgzf_ref.walk(f)
    for cap in (w.nmembers - 1, 2, 0):
        x = Index(engine.lib, f, cap=cap)
        assert x.record == (w.nmembers, w.total_out, w.file_used, E_OUT_CAPACITY, 0)      # the true counts: the caller can call again
        assert x.offs[:cap + 1] == w.off[:cap + 1] and x.out_offs[:cap + 1] == w.out_off[:cap + 1]
        assert x.offs[cap + 1:] == [-1] * 8 and x.out_offs[cap + 1:] == [-1] * 8      # no word behind member_cap
    x = Index(engine.lib, f, cap=w.nmembers + 5)
    assert x.record == w.record() and x.offs[:w.nmembers + 1] == w.off and x.offs[w.nmembers + 1:] == [-1] * (5 + 8)


# ---- hdlz_bgzf_inflate_ws
class Read(object):
    """one hdlz_bgzf_inflate_ws call: every output pre-filled with junk"""

    def __init__(self, L, f, off, out_off, out_cap=None, file_len=None, fill=0xA5, shift=0):
        B = len(off) - 1
        total = out_off[-1] - out_off[0]
        self.out_cap = out_cap = total if out_cap is None else out_cap
        self.d_file, self.d_off, self.d_out_off = dev_bytes(f, 1), dev(off, np.int64), dev(out_off, np.int64)
        self.out = torch.full((shift + out_cap + 64,), fill, dtype=torch.uint8, device="cuda")
        self.member = torch.full((max(B, 1),), -1, dtype=torch.int32, device="cuda")
        self.result = torch.full((3,), -1, dtype=torch.int64, device="cuda")
        wb = L.hdlz_bgzf_inflate_work_bytes(B, 0)
        self.work = torch.full((max(wb, 1),), fill ^ 0xFF, dtype=torch.uint8, device="cuda")
        rc = L.hdlz_bgzf_inflate_ws(self.d_file.data_ptr(), len(f) if file_len is None else file_len, self.d_off.data_ptr(),
                                    self.d_out_off.data_ptr(), B, 0, self.out.data_ptr() + shift if out_cap else None, out_cap,
                                    self.member.data_ptr(), self.result.data_ptr(), self.work.data_ptr() if wb else None, wb, stream_ptr())
        assert rc == 0, L.hdlz_last_error()
        torch.cuda.synchronize()
        r = _lib.BgzfInflateResult.from_buffer_copy(self.result.cpu().numpy().tobytes())
        self.rec = (r.status, r.first_bad, r.out_len)
        self.members = [int(x) for x in self.member.cpu().numpy()[:B]]
        o = self.out.cpu().numpy().tobytes()
        self.bytes, self.slack, self.fill = o[shift:shift + out_cap], o[shift + out_cap:], fill


@pytest.mark.parametrize("label", FILE_LABELS)
def test_every_file_decodes_to_its_data(engine, label):
    """the sound files whole; of the damaged ones the members in front of the failure (their index stays valid)"""
    f, data = files()[label]
    w = bgzf_ref.walk(f)
    if data is None:
        data = gzip.decompress(f[:w.file_used]) if w.nmembers and "ISIZE" not in label else None
    if data is None:                                                   # (nothing sound to read in front of the failure)
        return
    r = Read(engine.lib, f, w.off, w.out_off, shift=1)                 # (slots need no alignment: the output starts at an odd address)
    assert r.rec == (OK, NOBODY, len(data)), (label, r.rec, r.members)
    assert r.bytes == data and not any(r.members) and r.slack == bytes([r.fill]) * 64


def base_file():
    """eleven members of every block type, 150 KiB of data"""
    if "base" not in _files:
        parts = [bgzf_ref.data(n, 90 + n) for n in (3000, 65536, 1, 0, 20000, 65280, 700, 40000, 12, 5000, 31)]
        levels = (6, 9, 1, 6, 0, 1, 6, 0, 9, 1, 6)
        _files["base"] = (b"".join(member(p, lv) for p, lv in zip(parts, levels)) + EOF, parts)
    return _files["base"]


def damaged(f, at, xor):
    z = bytearray(f)
    z[at] ^= xor
    return bytes(z)


@pytest.mark.parametrize("k", [0, 4, 10])
def test_damage_in_one_member(engine, k):
    f, parts = base_file()
    w = bgzf_ref.walk(f)
    lo, hi, L = w.off[k], w.off[k + 1], engine.lib

    def verdict(g, off=w.off, out_off=w.out_off):
        r = Read(L, g, off, out_off)
        assert r.rec[2] == 0 and [b for b, s in enumerate(r.members) if s] == [k], (r.rec, r.members)      # exactly that member is marked
        assert r.members[k] == r.rec[0] and r.rec[1] == k
        return r.rec[0]
    for at in (hi - 8, hi - 5):                                        # a CRC byte
        assert verdict(damaged(f, at, 0x10)) == E_BAD_CHECKSUM
    # ISIZE changed: with the file's old index the slot contradicts the member; with the damaged file's own index the slot is the
    # word's -- one more than the data: the decoded length differs; one less: the decoder runs out of room
    more = f[:hi - 4] + (len(parts[k]) + 1).to_bytes(4, "little") + f[hi:]
    less = f[:hi - 4] + (len(parts[k]) - 1).to_bytes(4, "little") + f[hi:]
    assert verdict(more) == E_BAD_PARAM and verdict(less) == E_BAD_PARAM
    wm, wl = bgzf_ref.walk(more), bgzf_ref.walk(less)
    assert wm.status == wl.status == OK and wm.off == wl.off == w.off
    assert verdict(more, out_off=wm.out_off) == E_BAD_CHECKSUM
    assert verdict(less, out_off=wl.out_off) == E_OUT_CAPACITY
    st = verdict(damaged(f, lo + 18 + (hi - lo - 26) // 2, 0x04))       # a data bit: the decode fails, or the length or the CRC does
    assert st != OK
    for at in (0, 3, 12):                                              # the header is validated again: the index may come from elsewhere
        assert verdict(damaged(f, lo + at, 0x01)) == E_BAD_HEADER
    assert verdict(damaged(f, lo + 16, 0x01)) == E_BAD_PARAM           # BSIZE contradicts the index
    # a deflate stream that ends one byte in front of the trailer
    m = f[lo:hi]
    padded = bgzf_ref.frame(m[18:-8] + b"\x00", int.from_bytes(m[-8:-4], "little"), len(parts[k]))
    g = f[:lo] + padded + f[hi:]
    assert verdict(g, off=w.off[:k + 1] + [o + 1 for o in w.off[k + 1:]]) == E_NO_EOF


@pytest.mark.parametrize("bad", [(70, 300, 570), (570,), (300,)], ids=["70-300-570", "570", "300"])
def test_failed_members_beyond_the_first_wave_and_workgroup(engine, bad):
    """600 members: the failing ones sit in other waves and other workgroups of the judge than member 0 -- the lowest one is reported"""
    f, parts = bgzf_ref.many_members()
    w = bgzf_ref.walk(f)
    assert w.status == OK and w.nmembers == 601
    r = Read(engine.lib, bgzf_ref.with_crc_flipped(f, w.off, bad), w.off, w.out_off)
    assert r.rec == (E_BAD_CHECKSUM, bad[0], 0), r.rec
    assert [(b, s) for b, s in enumerate(r.members) if s] == [(b, E_BAD_CHECKSUM) for b in bad]      # exactly those members are marked


def test_sub_ranges_and_a_short_capacity(engine):
    f, parts = base_file()
    w = bgzf_ref.walk(f)
    data, L = b"".join(parts), engine.lib
    for b0, b1 in ((0, 12), (3, 4), (1, 2), (5, 11), (4, 4), (11, 12)):
        r = Read(L, f, w.off[b0:b1 + 1], w.out_off[b0:b1 + 1], shift=3)
        assert r.rec == (OK, NOBODY, w.out_off[b1] - w.out_off[b0]) and r.bytes == data[w.out_off[b0]:w.out_off[b1]], (b0, b1)
        assert r.slack == b"\xa5" * 64
    # out_cap one byte short: the last data member's slot ends behind it (and so does the EOF member's empty one): refused, not decoded
    r = Read(L, f, w.off, w.out_off, out_cap=len(data) - 1)
    assert r.rec == (E_BAD_PARAM, 10, 0) and r.members == [0] * 10 + [E_BAD_PARAM] * 2
    assert r.bytes[:w.out_off[10]] == data[:w.out_off[10]] and r.slack == b"\xa5" * 64
    # an index that leaves the file, runs backwards or skips a byte
    assert Read(L, f, w.off, w.out_off, file_len=len(f) - 1).rec[:2] == (E_BAD_PARAM, 11)
    for bad in (w.off[:5] + [w.off[4]] + w.off[6:], w.off[:5] + [w.off[5] + 1] + w.off[6:]):
        r = Read(L, f, bad, w.out_off)
        assert r.rec[:2] == (E_BAD_PARAM, 4) and [b for b, s in enumerate(r.members) if s] == [4, 5]


# ---- the Engine
def test_engine_round_trips(engine, oracle):
    n = 3 * 57344 + 1234
    data = bgzf_ref.data(n, 1)
    text = bgzf_ref.data(2 * n, 2)[:n]                                 # (64 KiB blocks of random bytes do not fit a member)
    for src, block, nb in ((data, 57344, 4), (data, 2048, 85), (text, 65536, 3)):
        d = dev_bytes(src)
        z = engine.compress_bgzf(d, block=block)
        zb = z.cpu().numpy().tobytes()
        assert gzip.decompress(zb) == src and zb.endswith(EOF)
        w = bgzf_ref.walk(zb)
        assert w.record() == (nb + 1, n, len(zb), OK, 1)
        off, out_off, rec = engine.bgzf_index(z)
        assert (rec.nmembers, rec.total_out, rec.file_used, rec.status, rec.eof_marker) == w.record()
        assert list(off.cpu().numpy()) == w.off and list(out_off.cpu().numpy()) == w.out_off
        off2, _, rec2 = engine.bgzf_index(z, member_cap=1)             # a guess that is too small: called once more
        assert list(off2.cpu().numpy()) == w.off and rec2.status == OK
        assert engine.inflate_bgzf(z).cpu().numpy().tobytes() == src
        part = engine.inflate_bgzf(z, index=(off, out_off), members=(1, 3))
        assert part.cpu().numpy().tobytes() == src[w.out_off[1]:w.out_off[3]]
    from hdl_deflate_amd.chain import plan_blocks
    blocks = [data[o:o + ln] for o, ln in plan_blocks(n, 57344)]
    want, _ = bgzf_ref.framed_rows(oracle_rows(oracle, blocks), blocks)
    assert engine.compress_bgzf_bytes(data) == want
    assert engine.inflate_bgzf_bytes(want) == (OK, data)
    assert engine.compress_bgzf_bytes(b"") == EOF and engine.inflate_bgzf_bytes(EOF) == (OK, b"") and engine.inflate_bgzf_bytes(b"") == (OK, b"")
    for short in (b"a", b"abcd"):
        with pytest.raises(Error):
            engine.compress_bgzf_bytes(short)
    for block in (31, 65537):
        with pytest.raises(ValueError):
            engine.compress_bgzf(d, block=block)
    r = np.random.default_rng(8)
    with pytest.raises(HdlzStatusError) as e:                          # 64 KiB of nine-bit literals do not fit a member
        engine.compress_bgzf(dev_bytes(data[:70000] + bytes(r.integers(144, 256, 65536, dtype=np.uint8)), 16), block=65536)
    assert e.value.status == E_OUT_CAPACITY and e.value.first_bad == 1


def test_engine_reads_files_of_other_writers(engine):
    """dynamic and stored blocks, as bgzip and htslib write them: nothing but the bytes is needed"""
    f, parts = base_file()
    data = b"".join(parts)
    assert any((f[o + 18] >> 1) & 3 == 2 for o in bgzf_ref.walk(f).off[:-1])       # (a dynamic block is among them)
    assert engine.inflate_bgzf_bytes(f) == (OK, data)
    assert engine.inflate_bgzf_bytes(f[:-28]) == (OK, data)                          # a missing EOF marker is no error
    w = bgzf_ref.walk(f)
    bad = damaged(f, w.off[6] - 6, 0x01)
    assert engine.inflate_bgzf_bytes(bad) == (E_BAD_CHECKSUM, b"")
    with pytest.raises(HdlzStatusError) as e:
        engine.inflate_bgzf(dev_bytes(bad))
    assert e.value.status == E_BAD_CHECKSUM and e.value.first_bad == 5
    with pytest.raises(HdlzStatusError) as e:                                          # a cut file: the index says where
        engine.inflate_bgzf(dev_bytes(f[:w.off[7] + 100]))
    assert e.value.status == E_NO_EOF and e.value.first_bad == 7
    off, out_off, rec = engine.bgzf_index(dev_bytes(f[:w.off[7] + 100]))
    assert rec.status == E_NO_EOF and rec.nmembers == 7
    head = engine.inflate_bgzf(dev_bytes(f[:w.off[7] + 100]), index=(off, out_off))      # the members in front of the failure stay readable
    assert head.cpu().numpy().tobytes() == data[:w.out_off[7]]
