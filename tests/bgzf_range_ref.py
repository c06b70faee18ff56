"""What hdlz_bgzf_read_ranges_ws must answer (include/hdlz_bgzf_range.h; a helper module like bgzf_ref.py, not a conftest): the serial
contract of the call as plain Python, the expected bytes from gzip.decompress slices, and the .gzi layout written with struct --
never from device output, and independent of hdl_deflate_amd/bgzf.py.  tests/test_bgzf_range_cabi.py holds resolve against a per-byte
map before any kernel is trusted to it."""
import gzip
import struct

import bgzf_ref
from bgzf_ref import OK, E_OUT_CAPACITY, E_BAD_PARAM

VIRTUAL = 1
NOBODY = (1 << 64) - 1


def virtual(c, u):
    return c << 16 | u


def _position(off, out_off, v):
    """a virtual offset -> its position in the data, or None (step 1, virtual mode)"""
    M = len(off) - 1
    c, u = v >> 16, v & 0xFFFF
    if c not in off:
        return None
    b = off.index(c)
    if b == M:
        return out_off[M] if u == 0 else None
    return out_off[b] + u if u <= out_off[b + 1] - out_off[b] else None


def resolve(off, out_off, ranges, virtual=False):
    """THE CONTRACT of hdlz_bgzf_read_ranges_ws, steps 1 and 3, for an ascending index -> per range (status, p0, p1, lo, hi): the tasks are
    members lo .. hi - 1; a range without tasks has lo = hi = 0"""
    M = len(off) - 1
    res = []
    for x, y in ranges:
        if virtual:
            p0, p1 = _position(off, out_off, x), _position(off, out_off, y)
            bad = p0 is None or p1 is None or p0 > p1
        else:
            bad = x > y
            if not bad:
                p0, p1 = min(max(x, out_off[0]), out_off[M]), min(max(y, out_off[0]), out_off[M])
        if bad:
            res.append((E_BAD_PARAM, 0, 0, 0, 0))
            continue
        lo = hi = 0
        if p0 < p1:
            lo = min(b for b in range(M) if out_off[b + 1] > p0)
            hi = min([b for b in range(lo, M) if out_off[b] >= p1] + [M])
        res.append((OK, p0, p1, lo, hi))
    return res


class Expected(object):
    """range_off[R + 1], total_out, ntasks, status[R], first_bad, record_status, pieces[R] (bytes; None for a failed range)"""


def expected(f, ranges, virtual=False, index=None, member_status=None, out_cap=None, task_cap=None):
    """the whole answer for file f (bytes): index = (off, out_off) (default: the serial walk); member_status[b]: what the member's own
    decode and trailer say (default: all OK -- the caller has it from hdlz_bgzf_inflate_ws or knows the damage); the capacities
    default to room enough"""
    if index is None:
        w = bgzf_ref.walk(f)
        assert w.status == OK
        index = (w.off, w.out_off)
    off, out_off = list(index[0]), list(index[1])
    M = len(off) - 1
    ms = [OK] * M if member_status is None else list(member_status)
    e = Expected()
    res = resolve(off, out_off, ranges, virtual)
    e.range_off, e.status, e.pieces, e.ntasks = [0], [], [], 0
    for st, p0, p1, lo, hi in res:
        e.range_off.append(e.range_off[-1] + p1 - p0)
        e.ntasks += hi - lo
    e.total_out = e.range_off[-1]
    capacity = (out_cap is not None and e.total_out > out_cap) or (task_cap is not None and e.ntasks > task_cap)
    for st, p0, p1, lo, hi in res:
        if st == OK and capacity:
            st = E_OUT_CAPACITY
        elif st == OK:
            st = next((ms[b] for b in range(lo, hi) if ms[b] != OK), OK)
        e.status.append(st)
        if st != OK:
            e.pieces.append(None)
            continue
        if p0 == p1:
            e.pieces.append(b"")
        else:                                # the members of this range alone, by a stock reader
            span = gzip.decompress(f[off[lo]:off[hi]])
            assert len(span) == out_off[hi] - out_off[lo]
            e.pieces.append(span[p0 - out_off[lo]:p1 - out_off[lo]])
    bad = [r for r, st in enumerate(e.status) if st != OK]
    if capacity:
        e.record_status, e.first_bad = E_OUT_CAPACITY, NOBODY
    elif bad:
        e.record_status, e.first_bad = e.status[bad[0]], bad[0]
    else:
        e.record_status, e.first_bad = OK, NOBODY
    return e


def gzi(off, out_off):
    """the .gzi file of an index (the layout stated in the issue and in hdl_deflate_amd/bgzf.py): count, then (compressed offset,
    uncompressed offset) of every member but member 0 that holds data"""
    pairs = [(off[b], out_off[b]) for b in range(1, len(off) - 1) if out_off[b + 1] != out_off[b]]
    return struct.pack("<Q", len(pairs)) + b"".join(struct.pack("<Q", c) + struct.pack("<Q", u) for c, u in pairs)


# ---- the files and batches of the GPU tests
PARTS_A = (300, 0, 5000, 65280, 12, 65536, 1, 0, 40000)


def file_a(level):
    """file A: members of these lengths (the 65536 bytes are zeros; stored blocks of 64 KiB do not fit a member, so level 0 drops that
    part) and the EOF member -> (file, data)"""
    parts = [bytes(n) if n == 65536 else bgzf_ref.data(n, n + level) for n in PARTS_A if level or n != 65536]
    return b"".join(bgzf_ref.member(p, level) for p in parts) + bgzf_ref.EOF, b"".join(parts)


def edge_ranges(out_off, seed, limit=400, per_member=True):
    """plain-mode ranges around every member boundary: from {O[b] - 1, O[b], O[b] + 1} to the same set at every later boundary, thinned to
    a seeded sample, behind the cases that are always there, which stand twice (once more reversed at the end): `limit` in all, or
    twice the fixed cases alone where `limit` is smaller than that (per_member=False, for files of hundreds of members: without the
    first and last byte of every member)"""
    import numpy as np
    M, total = len(out_off) - 1, out_off[-1]
    full = [b for b in range(M) if out_off[b + 1] > out_off[b]]
    must = []
    for b in full if per_member else full[:2] + full[-2:]:               # the single first and last byte of every member that holds data
        must += [(out_off[b], out_off[b] + 1), (out_off[b + 1] - 1, out_off[b + 1])]
    big = max(full, key=lambda b: out_off[b + 1] - out_off[b])
    must.append((out_off[big] + 7, out_off[big + 1] - 9))               # inside one member
    for b in range(1, M):                                                # across empty members
        if out_off[b] == out_off[b + 1] and 0 < out_off[b] < total:
            must.append((out_off[b] - 1, out_off[b] + 1))
    must += [(0, total), (0, 0), (total // 2, total // 2), (total, total), (total - 5, total + 1000), (0, 1 << 62), (total + 1, total + 9),
             (1 << 62, 1 << 63)]
    must += [must[0], must[0], (10, 200), (100, 300), (150, 160)]       # duplicates and overlaps
    marks = sorted({p for b in range(M + 1) for p in (out_off[b] - 1, out_off[b], out_off[b] + 1) if p >= 0})
    pairs = [(x, y) for i, x in enumerate(marks) for y in marks[i:]]
    r = np.random.default_rng(seed)
    take = min(len(pairs), max(0, limit - 2 * len(must)))
    sample = [pairs[k] for k in sorted(r.choice(len(pairs), take, replace=False))] if take else []
    return must + sample[::-1] + must[::-1]                              # (descending order: the sample and the fixed cases once more, reversed)


def aliases(off, out_off, p):
    """every virtual offset that names position p"""
    M = len(off) - 1
    return [virtual(off[b], p - out_off[b]) for b in range(M + 1)
            if out_off[b] <= p and p - out_off[b] <= 65535 and p - out_off[b] <= (out_off[b + 1] - out_off[b] if b < M else 0)]
