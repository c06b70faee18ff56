"""What the BGZF calls must answer (include/hdlz_bgzf.h; a helper module like gzip_ref.py, not a conftest): members built by stock zlib
(raw deflate at any level, framed by hand), the framing of a compressor's rows, and the serial walk that is the contract of
hdlz_bgzf_index_ws, stated once -- never from device output.  tests/test_bgzf_cabi.py holds all of it against gzip.decompress."""
import zlib

import numpy as np

OK, E_OUT_CAPACITY, E_NO_EOF, E_BAD_PARAM, E_BAD_HEADER, E_BAD_CHECKSUM = 0, 2, 5, 8, 11, 12
HEAD, TAIL = 18, 8
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
WINDOW = 65536


def header(size, mtime=0, xfl=0, os_=0xFF):
    """the 18 bytes in front of a member of `size` bytes"""
    assert 1 <= size <= 65536
    return (b"\x1f\x8b\x08\x04" + mtime.to_bytes(4, "little") + bytes([xfl, os_]) + b"\x06\x00" + b"BC\x02\x00" + (size - 1).to_bytes(2, "little"))


def frame(deflate, data_crc, isize, **kw):
    """a complete raw deflate stream -> the member around it"""
    return header(HEAD + len(deflate) + TAIL, **kw) + deflate + (data_crc & 0xFFFFFFFF).to_bytes(4, "little") + (isize & 0xFFFFFFFF).to_bytes(4, "little")


def member(data, level=6, **kw):
    """a member that holds `data` (at most 64 KiB), compressed by zlib at `level` (0: stored blocks, the payload verbatim)"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return frame(c.compress(data) + c.flush(), zlib.crc32(data), len(data), **kw)


def framed_rows(rows, blocks):
    """the writer's file: row b (a zlib stream of ONE final fixed block, as hdlz_compress_batch leaves it) of input block b -> member b,
    the EOF member behind the last.  -> (file, offsets[B + 1])"""
    out, offs = b"", []
    for row, blk in zip(rows, blocks):
        assert row[0] == 0x78 and int.from_bytes(row[:2], "big") % 31 == 0      # a zlib header
        offs.append(len(out))
        out += frame(row[2:-4], zlib.crc32(blk), len(blk))
    offs.append(len(out))
    return out + EOF, offs


def is_header(h):
    return len(h) >= 16 and h[0:4] == b"\x1f\x8b\x08\x04" and h[10:12] == b"\x06\x00" and h[12:16] == b"BC\x02\x00"


class Walk(object):
    """status, nmembers, total_out, file_used, eof_marker; off / out_off: nmembers + 1 words each"""

    def record(self):
        return (self.nmembers, self.total_out, self.file_used, self.status, self.eof_marker)


def walk(f):
    """THE CONTRACT of hdlz_bgzf_index_ws (include/hdlz_bgzf.h), step by step"""
    w = Walk()
    p = b = o = 0
    w.off, w.out_off = [], []
    last = None
    while True:
        if p == len(f):
            w.status = OK
            break
        if len(f) - p < HEAD:
            w.status = E_NO_EOF
            break
        size = int.from_bytes(f[p + 16:p + 18], "little") + 1
        if not is_header(f[p:p + HEAD]) or size < 28:
            w.status = E_BAD_HEADER
            break
        if p + size > len(f):
            w.status = E_NO_EOF
            break
        isize = int.from_bytes(f[p + size - 4:p + size], "little")
        if isize > 65536:
            w.status = E_BAD_HEADER
            break
        w.off.append(p)
        w.out_off.append(o)
        last = (size, isize)
        p, o, b = p + size, o + isize, b + 1
    w.off.append(p)
    w.out_off.append(o)
    w.nmembers, w.total_out, w.file_used = b, o, p
    w.eof_marker = 1 if w.status == OK and last == (28, 0) else 0
    return w


def data(n, seed):
    """n bytes: the first half text of ten letters, the second half random"""
    r = np.random.default_rng(seed)
    text = bytes(r.choice(np.frombuffer(b"abcdefgh \n", np.uint8), n))
    return text[:n // 2] + bytes(r.integers(0, 256, n - n // 2, dtype=np.uint8))


def many_members(count=600):
    """`count` members of 1 to 64 data bytes and the EOF member -> (file, the members' data): more members than one wave and than two
    workgroups of the per-member kernels hold"""
    r = np.random.default_rng(count)
    parts = [data(int(n), 1000 + k) for k, n in enumerate(r.integers(1, 65, count))]
    return b"".join(member(p, 6) for p in parts) + EOF, parts


def with_crc_flipped(f, off, members):
    """the file with a byte of the CRC word flipped in each of `members` (off: the index of the serial walk)"""
    z = bytearray(f)
    for b in members:
        z[off[b + 1] - 8] ^= 0x10
    return bytes(z)


def damaged_files():
    """(label, file, what the walk must say) -- also the cut and garbage cases of tests/test_gpu_bgzf.py"""
    parts = [data(n, 50 + n) for n in (300, 0, 5000, 65280, 12)]
    ms = [member(p, 6) for p in parts]
    f = b"".join(ms)
    a = len(ms[0]) + len(ms[1])                                          # where member 2 starts
    o = len(parts[0])
    yield "cut inside a header", f[:a + 7], (2, o, a, E_NO_EOF, 0)
    yield "cut behind BSIZE", f[:a + 18], (2, o, a, E_NO_EOF, 0)
    yield "cut inside the data", f[:a + 200], (2, o, a, E_NO_EOF, 0)
    yield "cut inside the trailer", f[:a + len(ms[2]) - 3], (2, o, a, E_NO_EOF, 0)
    yield "garbage behind the last member", f + b"trailing garbage, more than a header long", (5, sum(map(len, parts)), len(f), E_BAD_HEADER, 0)
    yield "short garbage behind the last member", f + EOF + b"xyz", (6, sum(map(len, parts)), len(f) + 28, E_NO_EOF, 0)
    big = bytearray(f)
    big[a + len(ms[2]) - 4:a + len(ms[2])] = (65537).to_bytes(4, "little")
    yield "ISIZE = 65537", bytes(big), (2, o, a, E_BAD_HEADER, 0)
    ok = bytearray(f)
    ok[a + len(ms[2]) - 4:a + len(ms[2])] = (65536).to_bytes(4, "little")
    yield "ISIZE = 65536", bytes(ok), (5, sum(map(len, parts)) - 5000 + 65536, len(f), OK, 0)
    tiny = f[:a] + header(27) + bytes(9) + f[a:]
    yield "size = 27", tiny, (2, o, a, E_BAD_HEADER, 0)
    for at, name in ((0, "ID1"), (3, "FLG"), (10, "XLEN"), (12, "SI1"), (14, "SLEN")):
        bad = bytearray(f)
        bad[a + at] ^= 1
        yield "header byte " + name, bytes(bad), (2, o, a, E_BAD_HEADER, 0)
    free = bytearray(f)
    for at in range(4, 10):                                              # MTIME, XFL, OS may be anything
        free[a + at] ^= 0x5A
    yield "MTIME, XFL, OS", bytes(free), (5, sum(map(len, parts)), len(f), OK, 0)
    yield "empty", b"", (0, 0, 0, OK, 0)
    yield "the EOF member alone", EOF, (1, 0, 28, OK, 1)
    yield "seventeen bytes", f[:17], (0, 0, 0, E_NO_EOF, 0)
