"""Where a capped grid, a one-workgroup loop or a one-wave round takes its SECOND item (a helper module like gzip_ref.py, not a conftest).

The container, index and checksum kernels cap their grids at a constant, let one finishing workgroup walk a strided share of the
work, or let one wave take 64 windows a round.  What such a kernel carries from one item to the next -- a prefetched tile, a Horner
step, a `prev` handed on, a row index that must stay b -- runs only from a threshold on.  This module reads the caps out of the
sources as text (a pattern that no longer matches fails the import: whoever changes a cap moves the shapes), derives the thresholds,
and builds the files and batches that tests/test_second_trips_cpu.py holds against their references alone and that
tests/test_gpu_second_trips.py runs on the device.  Everything is generated, nothing is read from device output, and every builder
is linear in the size of what it builds."""
import functools
import gzip
import os
import re
import zlib

import numpy as np

import bgzf_ref
import gunzip_ref as G
import gzip_members_ref as R
import joined_ref

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hdl_deflate_amd", "csrc")
OK, E_SHORT_INPUT, E_OUT_CAPACITY, E_NO_EOF, E_BAD_PARAM, E_BAD_HEADER, E_BAD_CHECKSUM = 0, 1, 2, 5, 8, 11, 12


# ---- the caps, from the sources
@functools.lru_cache(maxsize=None)
def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def source_const(name, pattern):
    """the one number `pattern` (one group) finds in csrc/`name`; every match must agree"""
    found = set(re.findall(pattern, _source(name), re.S))
    if len(found) != 1:
        raise AssertionError("csrc/%s: %r matches %s -- the launch code changed: derive the thresholds of tests/second_trips.py again"
                             % (name, pattern, sorted(found) or "nothing"))
    return int(found.pop())


def _has(name, pattern):
    if not re.search(pattern, _source(name), re.S):
        raise AssertionError("csrc/%s: %r matches nothing -- the launch code changed: derive the thresholds of tests/second_trips.py again"
                             % (name, pattern))


CRC_TILE = source_const("hdlz_crc32.h", r"constexpr uint32_t CRC_TILE = (\d+)u")
CRC_GRID_MAX = source_const("hdlz_crc32.h", r"constexpr uint32_t CRC_GRID_MAX = (\d+)u")
CRC_FIN_THREADS = source_const("hdlz_crc32.h", r"constexpr uint32_t CRC_FIN_THREADS = (\d+)u")
_has("hdlz_crc32.hip", r"nt < CRC_GRID_MAX \? nt : CRC_GRID_MAX")
GZM_WIN = 1 << source_const("hdlz_gzip_members.hip", r"constexpr uint32_t WIN_LOG2 = (\d+)u, WIN = 1u << WIN_LOG2")
SEAM_THREADS = source_const("hdlz_gzip_members.hip", r"constexpr uint32_t SEAM_THREADS = (\d+)u")
_has("hdlz_gzip_members.hip", r"K = \(W \+ SEAM_THREADS - 1u\) / SEAM_THREADS")
BGZF_WIN = 1 << source_const("hdlz_bgzf.hip", r"constexpr uint32_t WIN_LOG2 = (\d+)u, WIN = 1u << WIN_LOG2")
BGZF_SEAM_LANES = source_const("hdlz_bgzf.hip", r"__launch_bounds__\((\d+)\) void k_bgzf_seam")
BGZF_EMIT_THREADS = source_const("hdlz_bgzf.hip", r"launch\(k_bgzf_emit, dim3\(\(unsigned\)\(\(W \+ \d+u\) / (\d+)u\)\)")
JT = source_const("hdlz_frame.h", r"constexpr uint32_t JT = (\d+)u")
# the finishing workgroups that take lowest_word's share of the judges' words
LOWEST_THREADS = {"bgzf": source_const("hdlz_bgzf.hip", r"lowest_word\(a\.len, ngroups, tid, (\d+)u\)"),
                  "gzip members": source_const("hdlz_gzip_members.hip", r"lowest_word\(a\.len, ngroups, tid, (\d+)u\)"),
                  "unjoin": source_const("hdlz_unjoin.hip", r"lowest_word\(a\.len, ngroups, tid, (\d+)u\)")}
_has("hdlz_unjoin.hip", r"lowest_word\(a\.len, ngroups, tid, CRC_FIN_THREADS\)")
LOWEST_THREADS["unjoin gzip"] = CRC_FIN_THREADS
JOIN_FIN_THREADS = source_const("hdlz_join.hip", r"for \(uint32_t t = tid; t < ntiles; t \+= (\d+)u\)")
JOIN_LIFT_GRID = source_const("hdlz_join.hip", r"ntiles < (\d+)u \? \(ntiles \? ntiles : 1u\) : \d+u")
JOIN_LIFT_THREADS = source_const("hdlz_join.hip", r"b \+= \(uint64_t\)gridDim\.x \* (\d+)u\) a\.off\[b\] \+= GZ_LIFT")
GUNZIP_HEADS_GRID = source_const("hdlz_gunzip.hip", r"a\.nstreams < (\d+)u \? a\.nstreams : \d+u;\s*hipLaunchKernelGGL\(gunzip::k_gunzip_heads")
GZM_HEADS_GRID = source_const("hdlz_gzip_members.hip", r"a\.nmembers < (\d+)u \? a\.nmembers : \d+u;\s*hipLaunchKernelGGL\(gzm::k_gzm_heads")


def strided(cap, per=1):
    """`cap` workers that stride over items, `per` units an item: the smallest unit counts at which a worker takes a second and a
    third item, and the counts between at which some workers take one item more than others (the ragged case)"""
    return {"second": cap * per + 1, "third": 2 * cap * per + 1, "ragged": (cap * per + 1, 2 * cap * per - 1)}


THRESHOLDS = {
    # tiles of 32 KiB: a workgroup of crc_tiles takes tile blockIdx.x + CRC_GRID_MAX
    "crc_tiles": strided(CRC_GRID_MAX),
    # crc_finish numbers ntiles + 1 words (the initial register is one more): thread 0 takes a second word from CRC_FIN_THREADS tiles on
    "crc_finish": {"second": CRC_FIN_THREADS, "third": 2 * CRC_FIN_THREADS, "ragged": (CRC_FIN_THREADS, 2 * CRC_FIN_THREADS - 2)},
    # windows of 32 KiB: K = ceil(W / SEAM_THREADS) consecutive windows a thread; from K = 2 on the last threads have none
    "gzm_seam": {"second": SEAM_THREADS + 1, "third": 2 * SEAM_THREADS + 1, "fourth": 3 * SEAM_THREADS + 1},
    # windows of 64 KiB: one wave, BGZF_SEAM_LANES windows a round; k_bgzf_emit's second workgroup
    "bgzf_seam": strided(BGZF_SEAM_LANES),
    "bgzf_emit": strided(BGZF_EMIT_THREADS),
    # members: a judge workgroup of JT members leaves one word; the finishing workgroup strides over the words
    "lowest_word": {k: strided(v, JT) for k, v in LOWEST_THREADS.items()},
    # rows: a join tile holds JT rows; the finishing workgroup strides over the tiles, the gzip lift over the rows
    "join_finish": strided(JOIN_FIN_THREADS, JT),
    "join_gzip_lift": strided(JOIN_LIFT_GRID, JOIN_LIFT_THREADS),
    # streams / members: a wave each, the grid strides
    "gunzip_heads": strided(GUNZIP_HEADS_GRID),
    "gzm_heads": strided(GZM_HEADS_GRID),
}

CRC_TILE_COUNTS = sorted({THRESHOLDS["crc_finish"]["second"] - 1, THRESHOLDS["crc_finish"]["second"], THRESHOLDS["crc_tiles"]["second"],
                          THRESHOLDS["crc_finish"]["third"] - 1, THRESHOLDS["crc_finish"]["third"], THRESHOLDS["crc_tiles"]["third"]})
CRC_CALLER_BYTES = THRESHOLDS["crc_tiles"]["second"] * CRC_TILE + 7          # the other callers of crc_tiles / crc_finish: one case each
MANY = max(GUNZIP_HEADS_GRID, GZM_HEADS_GRID, LOWEST_THREADS["bgzf"] * JT) + 300
PLANT_HIGH, PLANT_LOW = LOWEST_THREADS["bgzf"] * JT + 5, 3 * JT + 5            # judge group 256 (a second word of thread 0) and group 3
JOIN_ROWS = (THRESHOLDS["join_finish"]["second"], JOIN_LIFT_GRID * JOIN_LIFT_THREADS + JT + 1)


def join_failed_row(B):
    """the row that fails: in tile 300, a second tile of thread 44 of the finishing workgroup -- or, in a batch without one, the
    last row: thread 0's second tile"""
    return 300 * JT + 7 if B > 301 * JT else B - 1


# ---- hdlz_gzip_members_index_ws: planted look-alikes in clean bytes
def gzm_shapes():
    """label -> file length: K = 2; K = 3 with a last window of 100 bytes; K = 4"""
    t = THRESHOLDS["gzm_seam"]
    return {"K=2": t["second"] * GZM_WIN, "K=3 ragged": t["third"] * GZM_WIN + 100, "K=4": t["fourth"] * GZM_WIN}


@functools.lru_cache(maxsize=None)
def gzm_file(label):
    """-> (file, plan): clean bytes (no 1F) with the magic planted.  plan: name -> the planted positions; thread t of k_gzm_seam owns
    windows [t K, t K + K).  The file is no valid gzip file, which the index does not mind."""
    n = gzm_shapes()[label]
    W = -(-n // GZM_WIN)
    K = -(-W // SEAM_THREADS)
    assert K >= 2 and 52 * K < W
    win = GZM_WIN
    plan = {
        "two consecutive windows of one thread": [5 * K * win + 1000, (5 * K + 1) * win + 2000],
        "the last window of a thread and the first of the next": [(10 * K - 1) * win + 3000, 10 * K * win + 4000],
        "in front of three empty shares": [(20 * K - 1) * win + 77],
        "behind three empty shares": [23 * K * win + 5],                      # threads 20, 21, 22 own no candidate at all
        "seams inside a share": [((30 + i) * K + 1) * win + i - 3 for i in range(7)],
        "seams between two shares": [(40 + i) * K * win + i - 3 for i in range(7)],
        "a dense second window": [(50 * K + 1) * win + 4 * j for j in range(win // 4)],
        "the last windows": [(W - 2) * win + 9] + ([(W - 1) * win + 50] if n - (W - 1) * win >= 54 else []),
    }
    special = {p // win for ps in plan.values() for p in ps}
    keep_out = set(range(20 * K, 23 * K)) | {w + d for w in special for d in (-1, 0, 1)}
    r = np.random.default_rng(W)
    plan["every seventh window"] = [w * win + 16 + int(r.integers(0, win - 64)) for w in range(3, W - 2, 7) if w not in keep_out]
    a = np.frombuffer(R.clean_bytes(n, 7 + W), np.uint8).copy()
    magic = np.frombuffer(R.MAGIC, np.uint8)
    dense = plan["a dense second window"][0]
    a[dense:dense + win] = np.tile(magic, win // 4)
    for name, ps in plan.items():
        if name != "a dense second window":
            for i, p in enumerate(ps):
                a[p:p + 4] = magic
                if name == "every seventh window" and i % 2:
                    isize = np.frombuffer(int(r.integers(1, 60000)).to_bytes(4, "little"), np.uint8).copy()
                    isize[isize == 0x1F] = 0x20
                    a[p - 4:p] = isize                       # the word in front: a guess below the clamp
                elif name != "every seventh window":
                    a[p - 4:p] = 0xFF                        # the guess is the clamp 1032 span + 258, which tells where the member began
    return a.tobytes(), plan


def gzm_planted(plan):
    return sorted({0} | {p for ps in plan.values() for p in ps})


def gzm_caps(plan, cands):
    """the member_cap values: M, M - 1, one that ends inside the dense second window, one that ends with the first of two consecutive
    windows of one thread (the second one's cbase is above it), 0"""
    M = len(cands)
    inside = cands.index(plan["a dense second window"][0]) + 4000
    first = cands.index(plan["two consecutive windows of one thread"][0])
    return [M, M - 1, inside, first, 0]


def index_rule_arrays(z, cands):
    """gzip_members_ref.index_rule over known candidates, as int64 arrays"""
    off = np.array(list(cands) + [len(z)], np.int64)
    span = np.diff(off)
    a = np.frombuffer(z, np.uint8)
    at = off[1:]
    isize = np.zeros(len(span), np.int64)
    ok = span >= 18
    for k in range(4):
        isize[ok] |= a[at[ok] - 4 + k].astype(np.int64) << (8 * k)
    g = np.where(ok, np.minimum(isize, 1032 * span + 258), 0)
    return off, np.concatenate([[0], np.cumsum(g)]).astype(np.int64)


# ---- hdlz_bgzf_index_ws: files of 65, 129 and 259 windows
def bgzf_stored(size, seed, fake=None):
    """a member of exactly `size` bytes that holds ONE stored block -> (member, payload); fake = (payload index, bytes) written over it"""
    n = size - 31
    assert 0 <= n <= 65505
    payload = bytearray(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes())
    if fake:
        at, what = fake
        assert 0 <= at and at + len(what) <= n
        payload[at:at + len(what)] = what
    payload = bytes(payload)
    m = bgzf_ref.frame(b"\x01" + n.to_bytes(2, "little") + (n ^ 0xFFFF).to_bytes(2, "little") + payload, zlib.crc32(payload), n)
    assert len(m) == size
    return m, payload


FAKE_AT, TRUE_AT = 10000, 30000          # in a window that guesses wrong: the look-alike header and the window's true first member


def bgzf_shapes():
    """label -> (windows, {window: the fake header lands on a true start}, windows of small members).  Window 64 alone: lane 0 of
    round two after a whole first round; windows 63 and 127: lane 63 of rounds one and two (the round behind a repair starts at 64)"""
    s, e = THRESHOLDS["bgzf_seam"], THRESHOLDS["bgzf_emit"]
    L = BGZF_SEAM_LANES
    return {"65 windows, window 64 lands": (s["second"], {L: True}, ()),
            "65 windows, window 63 runs off": (s["second"], {L - 1: False}, ()),
            "129 windows, 63 lands, 127 runs off": (s["third"], {L - 1: True, 2 * L - 1: False}, ()),
            "129 windows, 64 runs off, 127 lands": (s["third"], {L: False, 2 * L - 1: True}, ()),
            "259 windows": (e["second"] + 2, {L - 1: False, L: True, 2 * L - 1: True}, (70, 200, e["second"] - 1, e["second"]))}


@functools.lru_cache(maxsize=None)
def bgzf_file(label):
    """-> (file, data, fakes): members of levels 0, 1, 6, 9 and mixed sizes, the EOF member last; in front of every window of `fakes` a
    stored member that straddles the window's start and holds a complete look-alike header FAKE_AT bytes into the window"""
    nwin, fakes, small = bgzf_shapes()[label]
    Wb = BGZF_WIN
    limit = nwin * Wb - 28
    r = np.random.default_rng(nwin + 31 * len(fakes))
    parts, datas, p, k = [], [], 0, 0
    sizes = (0, 1, 100, 3000, 20000, 40000, 57344, 65280, 65280, 40000)
    while p < (nwin - 1) * Wb + 1000:
        k += 1
        nxt = min([w for w in fakes if w * Wb > p], default=None)
        gap = nxt * Wb - p if nxt is not None else None
        if gap is not None and gap <= 30000:
            size = gap + TRUE_AT
            head = bgzf_ref.header(TRUE_AT - FAKE_AT if fakes[nxt] else TRUE_AT - FAKE_AT - 5000)
            m, d = bgzf_stored(size, 5000 + k, fake=(gap + FAKE_AT - 23, head))
        elif gap is not None and gap < 130000:
            m, d = bgzf_stored(min(60000, gap - 15000), 5000 + k)
        else:
            n = 3000 if p // Wb in small else sizes[int(r.integers(0, len(sizes)))]
            n = min(n, limit - p - 400)
            level = (0, 1, 6, 9)[k % 4]
            if level == 0:
                m, d = bgzf_stored(n + 31, 5000 + k)
            else:
                d = bgzf_ref.data(n, 5000 + k)
                m = bgzf_ref.member(d, level)
        parts.append(m)
        datas.append(d)
        p += len(m)
    assert p <= limit
    f = b"".join(parts) + bgzf_ref.EOF
    assert -(-len(f) // Wb) == nwin
    return f, b"".join(datas), dict(fakes)


def header_shaped(f):
    """every position of f at which bgzf_ref.is_header holds (and 18 bytes lie inside the file), ascending"""
    a = np.frombuffer(f, np.uint8)
    n = len(a) - 17
    hit = np.ones(n, bool)
    for at, want in ((0, 0x1F), (1, 0x8B), (2, 8), (3, 4), (10, 6), (11, 0), (12, 0x42), (13, 0x43), (14, 2), (15, 0)):
        hit &= a[at:at + n] == want
    return np.nonzero(hit)[0]


def bgzf_wrong_guesses(f, off):
    """the windows whose first header-shaped bytes are not the window's first member start (off: the serial walk's, ascending)"""
    Wb = BGZF_WIN
    nwin = -(-len(f) // Wb)
    hits, starts = header_shaped(f), np.array(off, np.int64)
    lo = np.arange(nwin, dtype=np.int64) * Wb

    def first_in(pos):
        i = np.searchsorted(pos, lo)
        v = np.where(i < len(pos), pos[np.minimum(i, len(pos) - 1)], -1)
        return np.where((v >= lo) & (v < lo + Wb), v, -1)
    return [int(w) for w in np.nonzero(first_in(hits) != first_in(starts))[0]]


def bgzf_damaged(f, off, window, first):
    """f with the magic of a member that starts in `window` broken: the window's first start, or its second one"""
    starts = [o for o in off[:-1] if o // BGZF_WIN == window]
    assert len(starts) >= 3
    z = bytearray(f)
    z[starts[0 if first else 1]] ^= 1
    return bytes(z)


# ---- more members than one grid of waves and than one word a thread of the finishing workgroup
EMPTY_GZ = gzip.compress(b"", mtime=1)


def _real_at(b):
    return b % 1021 == 5 or b in (PLANT_HIGH, PLANT_LOW)


@functools.lru_cache(maxsize=None)
def many_gzip_streams():
    """MANY streams for hdlz_gunzip_ws: mostly gzip.compress(b""), a real member every 1021 streams; the streams that are not OK stand
    at indices >= 65536 only -> (streams, {index: why})"""
    reals = [G.gz(G.text(n, 900 + n), level=(1, 6, 9)[n % 3], name=b"n" * (n % 5)) for n in (1, 17, 40, 64)]
    zs = [reals[b % 4] if _real_at(b) else EMPTY_GZ for b in range(MANY)]
    d = G.text(33, 950)
    grid = GUNZIP_HEADS_GRID
    bad = {grid: ("wrong magic", G.gz(d, magic=b"\x1f\x8c")), grid + 3: ("wrong CRC", G.gz(d, crc_xor=0x100)),
           grid + 100: ("ISIZE + 1", G.gz(d, isize_add=1)), grid + 101: ("cut trailer", G.gz(d)[:-3]),
           MANY - 1: ("reserved flag", G.gz(d, flg=0x40))}
    for b, (_, z) in bad.items():
        zs[b] = z
    return zs, {b: why for b, (why, _) in bad.items()}


@functools.lru_cache(maxsize=None)
def many_gzip_members(planted=()):
    """MANY members back to back with their true index; the members of `planted` carry a wrong CRC -> (file, off, out_off, datas)"""
    texts = [G.text(n, 900 + n) for n in (1, 17, 40, 64)]
    ms, datas = [], []
    for b in range(MANY):
        d = texts[b % 4] if _real_at(b) else b""
        ms.append(EMPTY_GZ if not d and b not in planted else G.gz(d, level=(1, 6, 9)[b % 3], crc_xor=0x4000 if b in planted else 0))
        datas.append(d)
    off = np.concatenate([[0], np.cumsum([len(m) for m in ms])]).astype(np.int64)
    out_off = np.concatenate([[0], np.cumsum([len(d) for d in datas])]).astype(np.int64)
    return b"".join(ms), off, out_off, datas


def verdicts_memoised(oracle, z, off, out_off):
    """gzip_members_ref.verdict of every member, one oracle call per distinct (member bytes, slot) -> [(status, data)]"""
    memo, out = {}, []
    for b in range(len(off) - 1):
        m, slot = z[off[b]:off[b + 1]], int(out_off[b + 1] - out_off[b])
        if (m, slot) not in memo:
            memo[(m, slot)] = R.verdict(oracle, m, 0, len(m), slot)
        out.append(memo[(m, slot)])
    return out


@functools.lru_cache(maxsize=None)
def many_bgzf_members():
    """MANY members, mostly of the EOF member's shape -> (file, datas): the serial walk gives the index"""
    reals = [bgzf_ref.data(n, 700 + n) for n in (1, 17, 40, 64)]
    ms, datas = [], []
    built = {}
    for b in range(MANY):
        if _real_at(b):
            d = reals[b % 4]
            if (d, b % 3) not in built:
                built[(d, b % 3)] = bgzf_ref.member(d, (1, 6, 9)[b % 3])
            ms.append(built[(d, b % 3)])
            datas.append(d)
        else:
            ms.append(bgzf_ref.EOF)
            datas.append(b"")
    return b"".join(ms), datas


# ---- joins: ragged blocks drawn from a small pool, so that the CPU oracle compresses each distinct block once
@functools.lru_cache(maxsize=None)
def block_pool(multiple_of_4):
    """120 distinct blocks of 5 .. 64 bytes (multiple_of_4: 8 .. 64, lengths the unjoin's dword slots ask for)"""
    r = np.random.default_rng(77)
    text = bgzf_ref.data(1 << 14, 78)
    lens = [4 * int(r.integers(2, 17)) if multiple_of_4 else int(r.integers(5, 65)) for _ in range(120)]
    return [text[a:a + n] for n in lens for a in [int(r.integers(0, (1 << 14) - n))]]


@functools.lru_cache(maxsize=None)
def pooled_batch(B, multiple_of_4=False):
    """-> (blocks, member lengths int64[B], data): B blocks of the pool and, from joined_ref.member_of, the length of every member"""
    pool = block_pool(multiple_of_4)
    pick = np.random.default_rng(B).integers(0, len(pool), B)
    mlen = np.array([len(joined_ref.member_of(p, 32, 10)[3]) for p in pool], np.int64)
    blocks = [pool[k] for k in pick]
    return blocks, mlen[pick], b"".join(blocks)


def stored_deflate(payload):
    """the payload as stored blocks of up to 65535 bytes (gzip_members_ref.stored's body, built in linear time)"""
    parts = []
    for k in range(0, max(len(payload), 1), 65535):
        part = payload[k:k + 65535]
        parts.append(bytes([1 if k + 65535 >= len(payload) else 0]) + len(part).to_bytes(2, "little") + (len(part) ^ 0xFFFF).to_bytes(2, "little"))
        parts.append(part)
    return b"".join(parts)


def literal_data(n):
    """n bytes below 144 with no three bytes repeated within 144 positions: the compressor finds no match, every byte is a literal of
    eight bits in a fixed block"""
    return ((np.arange(n, dtype=np.int64) * 37) % 144).astype(np.uint8).tobytes()
