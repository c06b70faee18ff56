"""What hdlz_gunzip_ws must answer (a helper module like checked_ref.py, not a conftest): the member rule of include/hdlz_gunzip.h as
a serial text, the builder of members with hand-made headers, and the cases the CPU and the GPU tests share.

The accept / reject reference is stock zlib -- zlib.decompressobj(31) -- and gzip.decompress; the rule's decode step is the CPU oracle
(bit-exact with the device's unchecked decode, statuses included), never the library's own call."""
import functools
import gzip
import zlib

import numpy as np

OK, E_SHORT_INPUT, E_OUT_CAPACITY, E_NO_EOF, E_BAD_HEADER, E_BAD_CHECKSUM = 0, 1, 2, 5, 11, 12
FTEXT, FHCRC, FEXTRA, FNAME, FCOMMENT = 1, 2, 4, 8, 16


# ---- the rule
def walk(z):
    """step 1 -> (status, p)"""
    n = len(z)
    if n < 10:
        return E_NO_EOF, 0
    flg = z[3]
    if z[:3] != b"\x1f\x8b\x08" or flg & 0xE0:
        return E_BAD_HEADER, 0
    pos = 10
    if flg & FEXTRA:
        if pos + 2 > n:
            return E_NO_EOF, 0
        xlen = z[pos] | z[pos + 1] << 8
        pos += 2
        if pos + xlen > n:
            return E_NO_EOF, 0
        pos += xlen
    for field in (FNAME, FCOMMENT):
        if flg & field:
            end = z.find(b"\0", pos)
            if end < 0:
                return E_NO_EOF, 0
            pos = end + 1
    if flg & FHCRC:
        if pos + 2 > n:
            return E_NO_EOF, 0
        if z[pos] | z[pos + 1] << 8 != zlib.crc32(z[:pos]) & 0xFFFF:
            return E_BAD_HEADER, 0
        pos += 2
    return OK, pos


def member(oracle, z, cap):
    """the five steps for one stream -> dict(status, out_len, in_used, crc[, data]); status None: "any status but OK" (the reference
    decoder is more lenient than zlib in places; no case of these tests goes there)"""
    z = bytes(z)
    fail = dict(out_len=0, in_used=0, crc=0)
    st, p = walk(z)
    if st != OK:
        return dict(status=st, **fail)
    rc, ref = oracle.inflate(b"\0\0" + z[p:], out_cap=cap)          # the decoder skips two bytes unread
    if rc != OK:
        return dict(status=rc, **fail)
    d = zlib.decompressobj(-15)
    try:
        assert d.decompress(z[p:]) == ref and d.eof
    except (zlib.error, AssertionError):
        return dict(status=None, **fail)
    end = len(z) - len(d.unused_data)
    if end + 8 > len(z):
        return dict(status=E_NO_EOF, **fail)
    crc = zlib.crc32(ref)
    if int.from_bytes(z[end:end + 4], "little") != crc or int.from_bytes(z[end + 4:end + 8], "little") != len(ref) & 0xFFFFFFFF:
        return dict(status=E_BAD_CHECKSUM, out_len=0, in_used=end + 8, crc=crc)
    return dict(status=OK, out_len=len(ref), in_used=end + 8, crc=crc, data=ref)


def zaccepts(z):
    """stock zlib on the same bytes -> (data, consumed), or None when it refuses or does not reach the member's end"""
    d = zlib.decompressobj(31)
    try:
        out = d.decompress(bytes(z))
    except zlib.error:
        return None
    return (out, len(z) - len(d.unused_data)) if d.eof else None


_expected = {}


def expect(oracle, z, cap):
    """member(), computed once per (stream, capacity)"""
    key = (bytes(z), cap)
    if key not in _expected:
        _expected[key] = member(oracle, z, cap)
    return _expected[key]


def check(label, exp, st, ol, used, crc, row):
    st, ol, used, crc = int(st), int(ol), int(used), int(crc) & 0xFFFFFFFF
    if exp["status"] is None:
        assert st != OK, (label, "must not be OK")
        return
    assert st == exp["status"], (label, "status", st, exp["status"])
    assert (ol, used, crc) == (exp["out_len"], exp["in_used"], exp["crc"]), (label, "out_len, in_used, crc", (ol, used, hex(crc)), exp)
    if "data" in exp:
        assert bytes(row[:ol]) == exp["data"], (label, "bytes")


# ---- members with hand-made headers
def header(extra=None, name=None, comment=None, hcrc=False, flg=0, cm=8, magic=b"\x1f\x8b", hcrc_xor=0):
    flg |= (FEXTRA if extra is not None else 0) | (FNAME if name is not None else 0) | (FCOMMENT if comment is not None else 0) | \
        (FHCRC if hcrc else 0)
    h = magic + bytes([cm, flg]) + (1700000000).to_bytes(4, "little") + b"\x02\x03"
    if extra is not None:
        h += len(extra).to_bytes(2, "little") + extra
    for s in (name, comment):
        if s is not None:
            h += s + b"\0"
    if hcrc:
        h += ((zlib.crc32(h) & 0xFFFF) ^ hcrc_xor).to_bytes(2, "little")
    return h


def deflate(data, level=6, strategy=0, full_flush_at=None):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    if full_flush_at is None:
        return c.compress(data) + c.flush()
    return c.compress(data[:full_flush_at]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(data[full_flush_at:]) + c.flush()


def trailer(data, crc_xor=0, isize_add=0):
    return (zlib.crc32(data) ^ crc_xor).to_bytes(4, "little") + ((len(data) + isize_add) & 0xFFFFFFFF).to_bytes(4, "little")


def gz(data, level=6, strategy=0, full_flush_at=None, crc_xor=0, isize_add=0, **hdr):
    return header(**hdr) + deflate(data, level, strategy, full_flush_at) + trailer(data, crc_xor, isize_add)


def text(n, seed):
    r = np.random.default_rng(seed)
    return bytes(r.choice(np.frombuffer(b"abcdefgh \n", np.uint8), n))


# ---- the cases: [(label, stream)]
@functools.lru_cache(maxsize=None)
def header_cases():
    d = text(300, 1)
    r = np.random.default_rng(2)
    name300 = bytes(r.integers(1, 256, 300, dtype=np.uint8))
    c = [("no flags", gz(d)), ("FTEXT", gz(d, flg=FTEXT)), ("FEXTRA", gz(d, extra=b"ab\x02\x00xy")), ("FNAME", gz(d, name=b"file.txt")),
         ("FCOMMENT", gz(d, comment=b"a comment")), ("FHCRC", gz(d, hcrc=True)),
         ("all four", gz(d, extra=b"ab\x02\x00xy", name=b"file.txt", comment=b"a comment", hcrc=True, flg=FTEXT)),
         ("XLEN 0", gz(d, extra=b"")), ("XLEN 65535", gz(d, extra=bytes(r.integers(0, 256, 65535, dtype=np.uint8)))),
         ("XLEN 65535 FHCRC", gz(d, extra=bytes(r.integers(0, 256, 65535, dtype=np.uint8)), name=b"n", hcrc=True)),
         ("name of 300", gz(d, name=name300)), ("name of 300, comment of 64", gz(d, name=name300, comment=b"c" * 64)),
         ("name of 63", gz(d, name=b"n" * 63)), ("name of 64", gz(d, name=b"n" * 64)), ("empty name and comment", gz(d, name=b"", comment=b""))]
    c += [("payload at %d mod 16" % ((11 + k) % 16), gz(d, name=b"n" * k)) for k in range(16)]
    c += [("FHCRC wrong by bit %d" % b, gz(d, name=b"x", hcrc=True, hcrc_xor=1 << b)) for b in (0, 15)]
    c += [("reserved flag 0x%02X" % f, gz(d, flg=f)) for f in (0x20, 0x40, 0x80)]
    c += [("CM = 7", gz(d, cm=7)), ("wrong magic", gz(d, magic=b"\x1f\x8c")), ("zlib framing", zlib.compress(d))]
    full = gz(text(40, 3), extra=b"abcd", name=b"name", comment=b"comm", hcrc=True)
    assert walk(full)[1] == 28 and len(full) > 40
    c += [("cut at %d" % k, full[:k]) for k in range(0, 41)]
    c += [("unterminated name", header(name=b"never ends")[:-1]), ("unterminated comment", header(name=b"n", comment=b"never ends")[:-1]),
          ("XLEN past the end", header(extra=b"1234567890")[:-3]), ("XLEN cut", b"\x1f\x8b\x08\x04" + bytes(6) + b"\x05"),
          ("gzip.compress(b\"\")", gzip.compress(b""))]
    assert len(gzip.compress(b"")) == 20
    return c


@functools.lru_cache(maxsize=None)
def payload_cases():
    d = text(60000, 4)
    rnd = bytes(np.random.default_rng(5).integers(0, 256, 3000, dtype=np.uint8))
    return [("stored", gz(d[:40000], level=0)), ("fixed", gz(d[:20000], strategy=zlib.Z_FIXED)), ("level 1", gz(d, level=1)),
            ("level 6", gz(d, level=6)), ("level 9", gz(d, level=9, name=b"nine")), ("random bytes", gz(rnd)),
            ("several blocks", gz(d[:50000] + rnd * 2 + d[:500], level=6)), ("full flush", gz(d[:30000], full_flush_at=12345, comment=b"c")),
            ("huffman only", gz(d[:9000], strategy=zlib.Z_HUFFMAN_ONLY)), ("empty", gz(b"", name=b"e"))]


@functools.lru_cache(maxsize=None)
def trailer_cases():
    d = text(5000, 6)
    z = gz(d, name=b"t")
    end = len(z) - 8
    second = gz(text(700, 7), hcrc=True)
    return [("cut at end + 7", z[:end + 7]), ("cut at end + 4", z[:end + 4]), ("cut at end + 3", z[:end + 3]), ("cut at end", z[:end]),
            ("CRC bit 0", gz(d, name=b"t", crc_xor=1)), ("CRC bit 31", gz(d, name=b"t", crc_xor=1 << 31)),
            ("ISIZE + 1", gz(d, name=b"t", isize_add=1)), ("ISIZE + 2^20", gz(d, name=b"t", isize_add=1 << 20)), ("ISIZE - 1", gz(d, name=b"t", isize_add=-1)),
            ("a second member behind", z + second), ("garbage behind", z + b"garbage"), ("intact", z)]


def all_cases():
    return header_cases() + payload_cases() + trailer_cases()


def lengths_case(lengths, seed=8):
    """members whose decoded lengths are `lengths`, with names of growing length in front (every payload alignment)"""
    return [gz(text(n, seed + k), level=(1, 6, 9)[k % 3], name=b"n" * k) for k, n in enumerate(lengths)]


# ---- running the device call
def run(engine, zs, pitch, ragged=True, in_len=None, out=None, work=None):
    """the streams as one hdlz_gunzip_ws call -- ragged: back to back; else rows of the longest stream's length, every stream padded
    with bytes that are not zero -> (rows, out_len, status, in_used, crc) as numpy (status .. crc as uint32)"""
    import torch
    if ragged:
        flat = torch.from_numpy(np.frombuffer(b"".join(zs) + b"\xAA" * 64, np.uint8).copy()).cuda()
        offs = torch.from_numpy(np.concatenate([[0], np.cumsum([len(z) for z in zs])]).astype(np.int64)).cuda()
        res = engine.inflate_gzip(flat, in_off=offs, in_len=in_len if in_len is not None else max(len(z) for z in zs), out_pitch=pitch, out=out, work=work)
    else:
        n = max(len(z) for z in zs)
        rows = torch.from_numpy(np.frombuffer(b"".join(z + b"\xAA" * (n - len(z)) for z in zs), np.uint8).copy().reshape(len(zs), n)).cuda()
        res = engine.inflate_gzip(rows, out_pitch=pitch, out=out, work=work)
    torch.cuda.synchronize()
    return (res[0].cpu().numpy(),) + tuple(t.cpu().numpy().view(np.uint32) for t in res[1:])
