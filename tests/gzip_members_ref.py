"""What hdlz_gzip_members_index_ws and hdlz_gzip_members_inflate_ws must answer (a helper module like gunzip_ref.py, not a conftest):
the index rule of include/hdlz_gzip_members.h in numpy, the member verdict on top of gunzip_ref.member, the repair loop of
Engine.read_gzip as a serial text over stock zlib, a builder that places stored-block members at exact file offsets, and the case
files the CPU and the GPU tests share."""
import bisect
import functools
import gzip
import zlib

import numpy as np

import gunzip_ref as G

OK, E_OUT_CAPACITY, E_NO_EOF, E_BAD_PARAM, E_BAD_HEADER, E_BAD_CHECKSUM = 0, 2, 5, 8, 11, 12
MAGIC = b"\x1f\x8b\x08\x00"


# ---- the index rule
def candidates(z):
    a = np.frombuffer(bytes(z), np.uint8)
    n = len(a)
    if n == 0:
        return []
    c = {0}
    if n >= 4:
        hit = (a[:-3] == 0x1F) & (a[1:-2] == 0x8B) & (a[2:-1] == 8) & ((a[3:] & 0xE0) == 0)
        c |= set(int(p) for p in np.nonzero(hit)[0])
    return sorted(c)


def index_rule(z):
    """-> (off, out_off): M + 1 words each, as Python ints"""
    z = bytes(z)
    off = candidates(z) + [len(z)]
    out_off = [0]
    for b in range(len(off) - 1):
        span = off[b + 1] - off[b]
        g = 0 if span < 18 else min(int.from_bytes(z[off[b + 1] - 4:off[b + 1]], "little"), 1032 * span + 258)
        out_off.append(out_off[-1] + g)
    return off, out_off


# ---- the member verdict
def verdict(oracle, z, s, e, n_slot, file_len=None, out_room=None):
    """steps 1 .. 5 of the read for the member z[s : e) with a slot of n_slot bytes -> (status, data or None); status None: "any
    status but OK" (gunzip_ref.member).  out_room: the bytes from the slot's start to out_cap"""
    file_len = len(z) if file_len is None else file_len
    if e < s or e > file_len or e - s >= 1 << 28 or n_slot < 0 or n_slot >= (1 << 32) - 512 or (out_room is not None and n_slot > out_room):
        return E_BAD_PARAM, None
    m = G.member(oracle, bytes(z[s:e]), n_slot)
    st = m["status"]
    if st not in (OK, E_BAD_CHECKSUM) or m["in_used"] == 0:
        return st, None                                   # the header's and the decoder's status, and a trailer that is cut, come first
    if m["in_used"] != e - s:
        return E_NO_EOF, None
    if st == OK and m["out_len"] != n_slot:
        return E_BAD_CHECKSUM, None
    if int.from_bytes(z[e - 4:e], "little") != n_slot & 0xFFFFFFFF:
        return E_BAD_CHECKSUM, None
    return st, m.get("data")


def verdicts(oracle, z, index=None):
    off, out_off = index_rule(z) if index is None else index
    return [verdict(oracle, z, off[b], off[b + 1], out_off[b + 1] - out_off[b]) for b in range(len(off) - 1)]


# ---- the repair loop: Engine.read_gzip as a serial text.  `ok`: per candidate, did it verify (None: none did -- the serial reader alone)
def serial_member(z, pos):
    """stock zlib on one member at pos -> (data, consumed) or None"""
    return G.zaccepts(z[pos:])


def read_rule(z, ok=None, big=None):
    """-> (data or None when the file is refused, repairs, big, members)"""
    z = bytes(z)
    off, _ = index_rule(z)
    M, n = len(off) - 1, len(z)
    ok = [False] * M if ok is None else ok
    pieces, pos, repairs, nbig, members = [], 0, 0, 0, 0
    while pos < n:
        if members:
            pos = n - len(z[pos:].lstrip(b"\0"))
            if pos == n:
                break
        b = bisect.bisect_left(off, pos, 0, M)
        b = b if b < M and off[b] == pos else None
        if b is not None and ok[b] is not False and not (big and off[b + 1] - off[b] >= big):
            while b < M and ok[b] is not False and not (big and off[b + 1] - off[b] >= big):
                pieces.append(ok[b])
                members += 1
                b += 1
            pos = off[b]
            continue
        if b is not None and big and off[b + 1] - off[b] >= big:
            nbig += 1
        else:
            repairs += 1
        m = serial_member(z, pos)
        if m is None:
            return None, repairs, nbig, members
        pieces.append(m[0])
        members += 1
        pos += m[1]
    return b"".join(pieces), repairs, nbig, members


def read_with_rules(oracle, z, big=None):
    """the whole route on the CPU: the index rule, every member's verdict, the repair loop"""
    v = verdicts(oracle, z)
    assert all(st is not None for st, _ in v), "a case whose reference status is undetermined"
    return read_rule(z, [d if st == OK else False for st, d in v], big)


def gzip_accepts(z):
    try:
        return gzip.decompress(bytes(z))
    except Exception:
        return None


# ---- stored-block members at exact offsets
def clean_bytes(n, seed):
    """n random bytes without 1F: no magic inside, whatever stands around them"""
    a = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
    a[a == 0x1F] = 0x20
    return a.tobytes()


def stored(payload):
    """a member of stored blocks: 23 + len(payload) bytes for one block (a payload of up to 65535 bytes), 5 more per further block"""
    body, k = b"", 0
    while True:
        part = payload[k:k + 65535]
        k += len(part)
        final = k >= len(payload)
        body += bytes([1 if final else 0]) + len(part).to_bytes(2, "little") + (len(part) ^ 0xFFFF).to_bytes(2, "little") + part
        if final:
            break
    return G.header() + body + G.trailer(payload)


def stored_of_length(total, seed):
    """a stored member of exactly `total` bytes (>= 23) whose only candidate is its own header"""
    blocks = max(1, -(-(total - 18) // 65540))
    n = total - 18 - 5 * blocks
    assert n >= 0
    for k in range(64):
        m = stored(clean_bytes(n, seed + 1000 * k))
        assert len(m) == total
        if candidates(m) == [0]:
            return m
    raise AssertionError("no clean stored member of %d bytes" % total)


def place(starts, total, seed=0):
    """a file of `total` bytes whose members start exactly at `starts` (sorted, from 0): stored members, one candidate each"""
    assert starts[0] == 0 and list(starts) == sorted(set(starts))
    ends = list(starts[1:]) + [total]
    return b"".join(stored_of_length(e - s, seed + 7 * i) for i, (s, e) in enumerate(zip(starts, ends)))


def plant(z, positions, what=MAGIC):
    """`what` written over z at every position (inside payloads: the file is then no longer a valid one, which the index does not mind)"""
    a = bytearray(z)
    for p in positions:
        a[p:p + len(what)] = what
    return bytes(a)


# ---- the files the tests share
@functools.lru_cache(maxsize=None)
def many_members():
    """300 members of levels 0 to 9 with lengths 0 to 5000, gzip.compress(b"") among them; every candidate is a member's start"""
    r = np.random.default_rng(11)
    ms, datas = [], []
    k = 0
    while len(ms) < 300:
        n = int(r.integers(0, 5001)) if len(ms) % 50 else (0, 5000, 1, 17, 4999, 2)[len(ms) // 50]
        d = G.text(n, 100 + k) if k % 3 else clean_bytes(n, 100 + k)
        k += 1
        m = gzip.compress(b"", mtime=1) if len(ms) == 7 else G.gz(d, level=len(ms) % 10, name=(b"n" * (len(ms) % 5) if len(ms) % 4 == 0 else None))
        if len(ms) == 7:
            d = b""
        if candidates(m) != [0]:
            continue
        ms.append(m)
        datas.append(d)
    return ms, datas


@functools.lru_cache(maxsize=None)
def file_cases():
    """[(label, file, expected repairs)] -- the clean files need none by the rule alone"""
    ms, _ = many_members()
    a, b, c = G.gz(G.text(3000, 41), name=b"a"), G.gz(G.text(700, 42), level=9, hcrc=True), G.gz(G.text(12000, 43), level=1)
    for m in (a, b, c):
        assert candidates(m) == [0]
    inner = G.gz(G.text(500, 44), name=b"inner.gz")
    nested = stored(clean_bytes(100, 45) + inner + clean_bytes(200, 46))
    assert candidates(nested) == [0, 10 + 5 + 100]
    bad = bytearray(b)
    bad[len(b) // 2] ^= 0x55
    return [("one member", a, 0), ("three members", a + b + c, 0), ("300 members", b"".join(ms), 0), ("empty members", gzip.compress(b"", mtime=1) * 3, 0),
            ("a nested .gz in a stored block", a + nested + b, 1), ("zero padding between and behind", a + bytes(37) + b + bytes(512), 2),
            ("garbage behind", a + b + b"garbage", 2), ("a corrupt member in the middle", a + bytes(bad) + c, 1),
            ("a 3-byte tail", a + b + b"\x1f\x8b\x08", 2), ("empty input", b"", 0), ("no magic in front", b"plain text, not a gzip file at all", 1),
            ("a cut last member", a + b[:-3], 1), ("zeros only behind", a + bytes(9), 1)]
