"""The reference of the seek tests (include/hdlz_seek.h), pure Python: a small inflate walker that returns every block boundary
(bit, pos, btype) of a zlib or gzip stream, the point rule over boundaries, the windows and CRC-32 words of an index, and what a batch of
ranges must deliver.  The walker decodes symbols only to count bytes -- the data itself is zlib's."""
import functools
import zlib
from collections import namedtuple

WINDOW = 32768
OK, E_OUT_CAPACITY, E_BAD_DISTANCE, E_NO_EOF, E_BAD_PARAM, E_BAD_CHECKSUM = 0, 2, 4, 5, 8, 12

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]

Boundary = namedtuple("Boundary", "bit pos btype")
Walk = namedtuple("Walk", "boundaries end_bit total payload data")       # payload: the byte where the deflate data starts
Index = namedtuple("Index", "bit pos crc win max_seg")                   # bit, pos: n + 1 words; crc: n words; win: n slots of 32768 bytes


class _Bits(object):
    def __init__(self, z, at):
        self.z = bytes(z) + bytes(8)
        self.p = at

    def peek(self, n):                       # n <= 24
        return (int.from_bytes(self.z[self.p >> 3:(self.p >> 3) + 4], "little") >> (self.p & 7)) & ((1 << n) - 1)

    def take(self, n):
        r = self.peek(n)
        self.p += n
        return r


def _decoder(lengths):
    """canonical code -> (fast, slow): fast[the next 9 stream bits] = (symbol, length) for codes of up to 9 bits, slow[(length, code
    read MSB first)] = symbol for the longer ones"""
    code, fast, slow = 0, [None] * 512, {}
    for l in range(1, 16):
        for s, sl in enumerate(lengths):
            if sl == l:
                if l <= 9:
                    rc = int(format(code, "0%db" % l)[::-1], 2)
                    for hi in range(1 << (9 - l)):
                        fast[rc | hi << l] = (s, l)
                else:
                    slow[(l, code)] = s
                code += 1
        code <<= 1
    return fast, slow


def _symbol(b, table):
    bits = b.peek(15)
    e = table[0][bits & 511]
    if e is not None:
        b.p += e[1]
        return e[0]
    code = int(format(bits & 511, "09b")[::-1], 2)
    for l in range(10, 16):
        code = (code << 1) | ((bits >> (l - 1)) & 1)
        s = table[1].get((l, code))
        if s is not None:
            b.p += l
            return s
    raise ValueError("no code")


_FIXED = None


def gzip_payload(z):
    """the offset of the first deflate byte of a gzip member (RFC 1952)"""
    assert z[:3] == b"\x1f\x8b\x08"
    flg, p = z[3], 10
    if flg & 4:
        p += 2 + z[p] + 256 * z[p + 1]
    if flg & 8:
        p = z.index(b"\0", p) + 1
    if flg & 16:
        p = z.index(b"\0", p) + 1
    if flg & 2:
        p += 2
    return p


def walk_deflate(z, at):
    """raw deflate from byte `at` of z -> (boundaries, end_bit, total)"""
    global _FIXED
    if _FIXED is None:
        _FIXED = (_decoder([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _decoder([5] * 30))
    b, pos, out = _Bits(z, 8 * at), 0, []
    while True:
        out.append(Boundary(b.p, pos, (b.peek(3) >> 1) & 3))
        final, btype = b.take(1), b.take(2)
        if btype == 0:
            b.p = (b.p + 7) & ~7
            n = b.take(16)
            assert b.take(16) == n ^ 0xFFFF
            b.p += 8 * n
            pos += n
        else:
            if btype == 1:
                lit, dist = _FIXED
            else:
                assert btype == 2
                hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[CL_ORDER[i]] = b.take(3)
                clt, lens = _decoder(cl), []
                while len(lens) < hlit + hdist:
                    s = _symbol(b, clt)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + b.take(2))
                    elif s == 17:
                        lens += [0] * (3 + b.take(3))
                    else:
                        lens += [0] * (11 + b.take(7))
                assert len(lens) == hlit + hdist
                lit, dist = _decoder(lens[:hlit]), _decoder(lens[hlit:])
            while True:
                s = _symbol(b, lit)
                if s < 256:
                    pos += 1
                elif s == 256:
                    break
                else:
                    pos += LBASE[s - 257] + b.take(LEXT[s - 257])
                    b.take(DEXT[_symbol(b, dist)])
        if final:
            return out, b.p, pos


@functools.lru_cache(maxsize=None)
def walk(z, container):
    """every block boundary of the zlib stream or (first) gzip member z -> a Walk"""
    z = bytes(z)
    if container == "gzip":
        at = gzip_payload(z)
        data = zlib.decompressobj(31).decompress(z)
    else:
        at = 2
        data = zlib.decompressobj(15).decompress(z)
    bd, end_bit, total = walk_deflate(z, at)
    assert total == len(data)
    return Walk(tuple(bd), end_bit, total, at, data)


def points(boundaries, span):
    """the point rule: boundaries (bit, pos, ...) in stream order, the first one the stream's first header -> the selected ones"""
    out = [boundaries[0]]
    for a, b in zip(boundaries, boundaries[1:]):
        if b[1] // span > a[1] // span:
            out.append(b)
    return out


def window(data, pos):
    h = min(WINDOW, pos)
    return bytes(WINDOW - h) + data[pos - h:pos]


def index(w, span, boundaries=None):
    """the index of a Walk at `span` (boundaries: a subset S of w.boundaries that holds the first; default all)"""
    pts = points(list(w.boundaries if boundaries is None else boundaries), span)
    bit = [p[0] for p in pts] + [w.end_bit]
    pos = [p[1] for p in pts] + [w.total]
    crc = [zlib.crc32(w.data[pos[k]:pos[k + 1]]) for k in range(len(pts))]
    win = [window(w.data, pos[k]) for k in range(len(pts))]
    return Index(bit, pos, crc, win, max(pos[k + 1] - pos[k] for k in range(len(pts))))


def route_index(w, span, route):
    """the index a route must give: 2, the wave route -- S = every block boundary; 1, the chain route -- S = the stream's first header
    and every header of a dynamic block (the nodes of the whole-GPU chain for any block types)"""
    assert route in (1, 2)
    return index(w, span, None if route == 2 else [b for k, b in enumerate(w.boundaries) if k == 0 or b.btype == 2])


def shift_to_byte(z, bit, end_bit=None):
    """the bits of z from `bit` on (up to end_bit), moved to a byte boundary"""
    v = int.from_bytes(z, "little") >> bit
    n = 8 * len(z) - bit if end_bit is None else end_bit - bit
    if end_bit is not None:
        v &= (1 << n) - 1
    return v.to_bytes((n + 7) // 8 + 1, "little")


def decode_segment(z, w, ix, k):
    """segment k of an index of the Walk w re-decoded with stock zlib, from nothing but its point and its window.  Block by block,
    because moving the bits breaks the byte alignment a stored block rests on: a Huffman block is raw deflate from its header bit moved
    to a byte boundary and cut at the next header, its BFINAL bit set so that zlib ends with it, with the 32 KiB in front of it -- the
    window, then what the segment gave so far -- as the dictionary; a stored block is its bytes"""
    bd = list(w.boundaries) + [Boundary(w.end_bit, w.total, 0)]
    out = bytearray()
    for b, nxt in zip(bd, bd[1:]):
        if not ix.bit[k] <= b.bit < ix.bit[k + 1]:
            continue
        n = nxt.pos - b.pos
        assert b.pos == ix.pos[k] + len(out)
        if b.btype == 0:
            at = (b.bit + 3 + 7) // 8
            assert int.from_bytes(z[at:at + 2], "little") == n
            out += z[at + 4:at + 4 + n]
        elif n:
            d = zlib.decompressobj(wbits=-15, zdict=(ix.win[k] + bytes(out))[-WINDOW:])
            bits = bytearray(shift_to_byte(z, b.bit, nxt.bit))
            bits[0] |= 1
            out += d.decompress(bytes(bits))
            assert d.eof and len(out) == nxt.pos - ix.pos[k]
    return bytes(out)


def resolve(pos, ranges):
    """per range: (status, p0, p1, lo, hi) -- the tasks are segments lo .. hi - 1"""
    n, total, out = len(pos) - 1, pos[-1], []
    for x, y in ranges:
        if x > y:
            out.append((E_BAD_PARAM, 0, 0, 0, 0))
            continue
        p0, p1 = min(x, total), min(y, total)
        if p1 == p0:
            out.append((OK, p0, p1, 0, 0))
            continue
        lo = max(k for k in range(n) if pos[k] <= p0)
        hi = max(k for k in range(n) if pos[k] < p1) + 1
        out.append((OK, p0, p1, lo, hi))
    return out


Expected = namedtuple("Expected", "status pieces range_off total_out ntasks record_status first_bad")
NOBODY = (1 << 64) - 1


def expected(data, pos, ranges, segment_status=None, out_cap=None, task_cap=None):
    """what a batch of ranges delivers: slices of the data (None for a failed range), the scan, the record.  segment_status: the
    status of every segment (default: all OK) -- a range takes that of its lowest failing one"""
    res = resolve(pos, ranges)
    lens = [p1 - p0 for _, p0, p1, _, _ in res]
    range_off = [sum(lens[:r]) for r in range(len(ranges) + 1)]
    ntasks = sum(hi - lo for _, _, _, lo, hi in res)
    capacity = (out_cap is not None and range_off[-1] > out_cap) or (task_cap is not None and ntasks > task_cap)
    status, pieces = [], []
    for st, p0, p1, lo, hi in res:
        if st == OK and capacity:
            st = E_OUT_CAPACITY
        elif st == OK and segment_status is not None:
            st = next((segment_status[k] for k in range(lo, hi) if segment_status[k] != OK), OK)
        status.append(st)
        pieces.append(data[p0:p1] if st == OK else None)
    bad = [r for r, st in enumerate(status) if st != OK]
    if capacity:
        rs, fb = E_OUT_CAPACITY, NOBODY
    else:
        rs, fb = (status[bad[0]], bad[0]) if bad else (OK, NOBODY)
    return Expected(status, pieces, range_off, range_off[-1], ntasks, rs, fb)


# ---- the streams of the tests: 64 to 300 KiB of output from stock zlib, every block type, both containers
def data(n, seed):
    """n bytes of text-like data: words of a small vocabulary, runs, and stretches of noise (which zlib stores)"""
    import random
    rng = random.Random(seed)
    vocab = [bytes(rng.randrange(97, 123) for _ in range(rng.randrange(2, 10))) for _ in range(400)]
    out = bytearray()
    while len(out) < n:
        k = rng.randrange(10)
        if k == 0:
            out += bytes(rng.getrandbits(8) for _ in range(rng.randrange(200, 3000)))
        elif k == 1:
            out += bytes([rng.randrange(256)]) * rng.randrange(10, 600)
        else:
            out += b" ".join(rng.choice(vocab) for _ in range(rng.randrange(50, 400)))
    return bytes(out[:n])


def deflate(d, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem=8, flush_every=0, wbits=15):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, mem, strategy)
    if not flush_every:
        return c.compress(d) + c.flush()
    return b"".join(c.compress(d[i:i + flush_every]) + c.flush(zlib.Z_SYNC_FLUSH) for i in range(0, len(d), flush_every)) + c.flush()


def gzip_member(d, raw, fextra=b"", fname=b"", behind=b""):
    """a gzip member around the raw deflate stream `raw` of d, with FEXTRA / FNAME fields and bytes behind the trailer"""
    flg = (4 if fextra else 0) | (8 if fname else 0)
    head = b"\x1f\x8b\x08" + bytes([flg]) + bytes(4) + b"\x00\x03"
    if fextra:
        head += len(fextra).to_bytes(2, "little") + fextra
    if fname:
        head += fname + b"\0"
    return head + raw + zlib.crc32(d).to_bytes(4, "little") + (len(d) & 0xFFFFFFFF).to_bytes(4, "little") + behind


@functools.lru_cache(maxsize=None)
def streams():
    """name -> (container, z, data, spans): the spans each stream is indexed at"""
    out = {}
    d1, d2, d3, d4 = data(65536, 1), data(200000, 2), data(300000, 3), data(90000, 4)
    out["L1"] = ("zlib", deflate(d2, 1), d2, (4096, 65536))
    out["L6"] = ("zlib", deflate(d3, 6), d3, (1024, 16384))
    out["L9"] = ("zlib", deflate(d1, 9), d1, (8192,))
    out["FIXED"] = ("zlib", deflate(d4, 6, zlib.Z_FIXED, flush_every=7001), d4, (2048,))
    out["L0"] = ("zlib", deflate(d2, 0), d2, (1024, 32768))
    out["MEM1"] = ("zlib", deflate(d3, 6, mem=1), d3, (1024, 5000))
    out["SYNC"] = ("zlib", deflate(d4, 6, flush_every=2500), d4, (1024, 10000))
    out["ONE"] = ("zlib", deflate(d1[:3000], 6), d1[:3000], (1024,))
    out["GZ6"] = ("gzip", deflate(d2, 6, mem=4, wbits=31), d2, (4096,))
    out["GZNAME"] = ("gzip", gzip_member(d4, deflate(d4, 9, mem=2, wbits=-15), fextra=b"AP\x03\x00xyz", fname=b"seek.txt", behind=b"\x1f\x8b trailing"),
                     d4, (1024, 65536))
    return out
