"""What hdlz_zip_write_ws and Engine.compress_zip must answer (a helper module like zip_ref.py, not a conftest): THE FILE RULE of
include/hdlz_zip_write.h as a serial text in plain Python, built from joined_ref.member_of (the CPU oracle's rows, the end bit and the
marker) and zlib.crc32 -- never from device output --, and the case lists the CPU and the GPU tests share: all_cases(), thorough
about the format and small, and shape_cases(), large in what the kernels branch on, with a model of the gather's row lookup that
proves which branch a case reaches.
tests/test_zip_write_cabi.py holds this rule against zipfile, numpy.load and the index rule of zip_ref.py on every case."""
import functools
import io
import struct
import zlib

import numpy as np

import joined_ref as J
import zip_ref as Z

OK, E_SHORT_INPUT, E_OUT_CAPACITY, E_BAD_PARAM = 0, 1, 2, 8
FLAG_UTF8 = 0x800
DATE_TIME = (1980, 1, 1, 0, 0, 0)
NONE = 0xFFFFFFFF


def dos_datetime(dt):
    y, mo, d, h, mi, s = dt
    return ((y - 1980) << 9 | mo << 5 | d) << 16 | (h << 11 | mi << 5 | s >> 1)


def plan(n, block, stored=False):
    """the blocks of an entry of n bytes as Engine.compress_zip cuts them: none under 5 bytes or when it is to be stored"""
    from hdl_deflate_amd.chain import plan_blocks
    return [] if stored or n < 5 else plan_blocks(n, block)


class Written(object):
    """file: the rule's bytes; record: dict(file_len, cd_off, cd_size, nstored, status, first_bad); entries: the dicts of
    zip_ref.index for this file (rule 7); methods: 0 / 8 per entry; pads: the pad bits of every member of every deflated entry;
    diffs: c_e - u_e of the deflated FORM of every entry that has blocks (None without blocks)"""


def encode_names(names):
    raw = [n.encode("utf-8") if isinstance(n, str) else bytes(n) for n in names]
    return raw, (FLAG_UTF8 if any(max(r, default=0) > 127 for r in raw) else 0)


def expected(items, block=32, cwindow=32, maxmatch=10, store=None, date_time=DATE_TIME, out_align=1, file_cap=None):
    """items: [(name, data)] -> Written.  The block plan, the names' encoding and the flags are Engine.compress_zip's."""
    raw, flags = encode_names([n for n, _ in items])
    dt = dos_datetime(date_time)
    time, date = dt & 0xFFFF, dt >> 16
    w = Written()
    body, cd = bytearray(), bytearray()
    w.entries, w.methods, w.pads, w.diffs = [], [], [], []
    o = 0
    for e, (nm, (_, data)) in enumerate(zip(raw, items)):
        data = bytes(data)
        assert len(nm) <= 65535 and len(data) < 0xFFFFFFFF
        blocks = plan(len(data), block, bool(store and store[e]))
        method, payload, diff = 0, data, None
        if blocks:
            parts = [J.member_of(data[a:a + ln], cwindow, maxmatch) for a, ln in blocks]
            deflated = b"".join(p[3] for p in parts) + b"\x03\x00"
            diff = len(deflated) - len(data)
            if diff < 0:                                         # rule 3: chosen iff c_e < u_e
                method, payload = 8, deflated
                w.pads += [p[2] for p in parts]
        crc = zlib.crc32(data)
        L = len(body)
        body += Z.SIG_LOCAL + struct.pack("<HHHHHIIIHH", 20, flags, method, time, date, crc, len(payload), len(data), len(nm), 0) + nm + payload
        o = -(-o // out_align) * out_align
        w.entries.append(dict(cd_off=len(cd), payload_off=L + 30 + len(nm), out_off=o, csize=len(payload), usize=len(data), crc=crc,
                              method=method, flags=flags, name_len=len(nm), status=OK, name=nm))
        o += len(data)
        cd += Z.SIG_CD + struct.pack("<HHHHHHIIIHHHHHII", 20, 20, flags, method, time, date, crc, len(payload), len(data), len(nm), 0, 0, 0, 0, 0, L) + nm
        w.methods.append(method)
        w.diffs.append(diff)
    E = len(items)
    for en in w.entries:
        en["cd_off"] += len(body)
    w.file = bytes(body + cd + Z.SIG_EOCD + struct.pack("<HHHHIIH", 0, 0, E, E, len(cd), len(body), 0))
    assert len(body) < 0xFFFFFFFF and len(w.file) <= 0xFFFFFFFF
    status = E_OUT_CAPACITY if file_cap is not None and len(w.file) > file_cap else OK
    w.record = dict(file_len=len(w.file), cd_off=len(body), cd_size=len(cd), nstored=w.methods.count(0), status=status, first_bad=NONE)
    return w


def bound(nentries, total_in, names_len):
    return 22 + 76 * nentries + 2 * names_len + total_in


def work_bytes(nentries, nblocks):
    r = lambda x: (x + 255) // 256 * 256
    return r(8 + 16 * ((nblocks + 255) // 256)) + 2 * r(8 * (nblocks + 1)) + 256 + 3 * r(8 * (nentries + 1)) + 3 * r(4 * (nentries + 1))


def soft(n, seed):
    """n bytes that deflate also in blocks of 32: a period of seven letters, started anywhere, with a foreign byte now and then"""
    r = np.random.default_rng(seed)
    d = (np.arange(n) + seed) % 7 + 97
    d[r.integers(0, max(n, 1), n // 23)] = 35
    return bytes(d.astype(np.uint8))


# ---- the cases: dict(label, items, block, store)
def _case(label, items, block=32, store=None):
    return dict(label=label, items=items, block=block, store=store)


@functools.lru_cache(maxsize=None)
def tie_entries():
    """{-1, 0, +1: data} -- entries whose deflated form is one byte shorter than, as long as and one byte longer than the entry, found
    in a small family: d distinct bytes from 0x30 (literals of eight bits) or 0x90 (nine bits) on, then k repeats of the last one (one
    block at block=64).  The literals' widths matter: the marker is 4 or 5 bytes by the pad bits, so c - u steps over a value."""
    found = {}
    for base in (0x30, 0x90):
        for d in range(1, 17):
            for k in range(0, 33):
                data = bytes(range(base, base + d)) + bytes([base + d - 1]) * k
                if len(data) < 5:
                    continue
                m = J.member_of(data, 32, 10)[3]
                diff = len(m) + 2 - len(data)
                if diff in (-1, 0, 1) and diff not in found:
                    found[diff] = data
    return found


@functools.lru_cache(maxsize=None)
def size_cases():
    sizes = _case("sizes 0 .. 49 at block 32", [("s%02d.txt" % n, soft(n, 100 + n)) for n in (0, 1, 4, 5, 31, 32, 33, 47, 48, 49)])
    # 1, 255, 256, 3, 257 and 600 blocks: entry boundaries at rows 1, 256, 512 (both on a tile seam), 515, 772 and 1372 (inside a tile)
    tiles = _case("1 .. 600 blocks at block 32", [("b%03d.bin" % k, soft(32 * k, 200 + k)) for k in (1, 255, 256, 3, 257, 600)])
    return [sizes, tiles]


@functools.lru_cache(maxsize=None)
def member_cases():
    ties = tie_entries()
    crafted = _case("ties: c - u of -1, 0 and +1", [("tie%+d" % d, ties[d]) for d in sorted(ties)], block=64)
    # a run that deflates well, then j literals of nine bits each: every one moves the end-of-block code by a bit
    pads = _case("pad bits 0 .. 7", [("p%d" % j, b"a" * 40 + bytes(range(0xC0, 0xC0 + j))) for j in range(8)], block=64)
    noisy = _case("incompressible entries with blocks", [("n%d" % n, Z.noise(n, 400 + n)) for n in (5, 31, 32, 33, 100, 700)])
    forced = _case("store= entries", [("f%d" % k, soft(200 + k, 500 + k)) for k in range(6)], store=[False, True, True, False, True, False])
    mix = [(("t%d" if k % 2 == 0 else "r%d") % k, soft(90 + 7 * k, 600 + k) if k % 2 == 0 else Z.noise(90 + 7 * k, 600 + k)) for k in range(12)]
    mixed = _case("the forms alternating", mix + [("empty", b""), ("tiny", b"abc")], store=[k % 4 == 0 and k % 8 != 0 for k in range(12)] + [False, False])
    return [crafted, pads, noisy, forced, mixed]


@functools.lru_cache(maxsize=None)
def name_cases():
    r = np.random.default_rng(21)
    word = lambda n: bytes(r.integers(97, 123, n, dtype=np.uint8)).decode()
    # a deflated and a stored entry per residue: the name's length (1 .. 16) is what puts the payload at residue k mod 16 -- the
    # local header starts where the rule put the end of the entry in front of it
    items = []
    for k in range(32):
        at = expected(items).record["cd_off"]
        n = (k % 16 - at - 30) % 16 or 16
        items.append((word(n), soft(40 + 3 * k, 700 + k) if k < 16 else Z.noise(40 + k, 700 + k)))
    every = _case("names of 1 to 16 bytes", items)
    long_ = _case("names of 300 and 65535 bytes", [("front", soft(64, 1)), (word(300), soft(100, 2)), (word(65535), soft(500, 3)), ("back", Z.noise(50, 4))])
    utf8 = _case("a name that is not ASCII", [("d/ümläut.txt", soft(100, 5)), ("plain.txt", Z.text(60, 6))])
    return [every, long_, utf8]


@functools.lru_cache(maxsize=None)
def count_cases():
    return [_case("no entry", []), _case("one entry", [("only.txt", Z.text(300, 7))]),
            _case("65535 empty entries", [("%05d" % k, b"") for k in range(65535)])]


CRC_TILED_MIN = 1 << 17          # Engine.ZIP_CRC_TILED_MIN: from here on an entry's CRC-32 is a call of its own


@functools.lru_cache(maxsize=None)
def large_cases():
    """entries on both sides of Engine.ZIP_CRC_TILED_MIN: a run of small ones in front of, between and behind two large ones (one of
    them exactly the threshold and stored), an empty run among them"""
    items = [("front.txt", soft(300, 1)), ("front.bin", Z.noise(50, 2)), ("large.txt", soft(CRC_TILED_MIN + 9001, 3)), ("empty", b""),
             ("between.txt", soft(4000, 4)), ("large.bin", Z.noise(CRC_TILED_MIN, 5)), ("large2.txt", soft(CRC_TILED_MIN + 1, 6)), ("back.txt", soft(77, 7))]
    return [_case("entries around ZIP_CRC_TILED_MIN", items, block=1 << 16, store=[False, False, False, False, False, True, False, False])]


def all_cases():
    return size_cases() + member_cases() + name_cases() + count_cases() + large_cases()


@functools.lru_cache(maxsize=None)
def written(label, out_align=1):
    c = {c["label"]: c for c in all_cases()}.get(label) or shape_case(label)
    return expected(c["items"], block=c["block"], store=c["store"], out_align=out_align)


# ---- the shapes: cases that are large in what the kernels of hdlz_zip_write.hip BRANCH on -- entries, rows, rowless runs, tiles --,
# kept out of all_cases().  Their entries are concatenations of a few dozen blocks of 32 bytes, so member_of, which caches by content,
# meets every row of every case after the first few dozen calls; an entry's length is a multiple of 32, so plan_blocks cuts it at
# the alphabet's blocks.
@functools.lru_cache(maxsize=None)
def alphabet():
    """(32 soft blocks, 16 noise blocks) of 32 bytes: members of 20 to 23 and of 39 to 41 bytes, pad bits 1 to 7 among them -- an
    entry of soft blocks alone is deflated, one of noise blocks alone is stored with its rows"""
    return tuple(soft(32, 9000 + k) for k in range(32)), tuple(Z.noise(32, 9100 + k) for k in range(16))


def of_blocks(r, k, form):
    """an entry of k alphabet blocks drawn with the generator r; form "s": soft, "n": noise, "m": mixed, a noise block in five"""
    s, n = alphabet()
    noisy = {"s": np.zeros(k, bool), "n": np.ones(k, bool), "m": r.integers(0, 5, k) == 0}[form]
    pick = r.integers(0, 1 << 16, k)
    return b"".join(n[p % len(n)] if q else s[p % len(s)] for p, q in zip(pick.tolist(), noisy.tolist()))


def _name(e):
    return "abcde"[:e % 6] + "%d" % e                            # (unique, 1 to 10 bytes: the records' sizes vary from entry to entry)


ROWLESS = (b"", b"abc", soft(40, 77))                            # entries without rows: empty, under 5 bytes, store=True


def _rowless(items, store, k):
    items.append((_name(len(items)), ROWLESS[k % 3]))
    store.append(k % 3 == 2)


def many_entries(E, seed, rows=(1, 2, 3), weights=None, run=None):
    """E entries of 1 to 3 rows (or of `rows`, drawn with `weights`), about one in 8 of them noise and one in 8 mixed, and about one
    in 16 without rows; run = (entry, length): from that entry on `length` entries without rows, one with rows on either side"""
    r = np.random.default_rng(seed)
    nrows = r.choice(rows, E, p=weights).tolist()
    kind = r.integers(0, 16, E).tolist()
    lo, hi = (run[0], run[0] + run[1]) if run else (E, E)
    items, store = [], []
    for e in range(E):
        beside = e in (lo - 1, hi)
        k = max(nrows[e], 1) if beside else nrows[e]
        if lo <= e < hi or k == 0 or (kind[e] == 0 and not beside and e not in FAIL_ENTRIES):
            _rowless(items, store, e)
        else:
            items.append((_name(e), of_blocks(r, k, "n" if kind[e] in (1, 2) else "m" if kind[e] in (3, 4) else "s")))
            store.append(False)
    return items, store


MANY = (63, 64, 4095, 4096, 4097, 1023, 1024, 1025, 2049)       # E + 1 around 64 and 4096 for the search, E around 1024 k for the plan
FAIL_ENTRIES = (330, 700, 4000, 4096)                            # the entries the failure tests at E = 4097 tamper with: they have rows
RUNS, RUN_ROWS = (62, 63, 64, 65, 200), (1, 2, 3, 4)
SEAM_ROWS = (1, 255, 256, 257, 63, 64, 65, 4096, 16383, 16385, 20000, 3000, 5000, 2, 2)
SEAM_FORMS = "ssmnsnsmnsmnsss"
SEAM_STATUS, SEAM_CONTRADICTION = (8, 20000), (10, 50000)       # (entry, row) the failure tests at 65536 rows tamper with
MANY_ROWS_RUN = (30000, 100)                                     # the run of rowless entries in the 65535-entry case
BIG_STORED = (65535, 65536, 65537, 3 * 65536 + 1)
SHAPE_LABELS = tuple("%d entries of 1 to 3 rows" % E for E in MANY) + ("rowless runs of 62 to 200 entries", "65535 rows across the seams",
                                                                       "65536 rows across the seams", "65535 entries and more rows",
                                                                       "stored tiles among 300 entries")
LARGE_SHAPES = SHAPE_LABELS[-3:-1]                               # the two cases that take 256 rows a workgroup


@functools.lru_cache(maxsize=None)
def shape_case(label):
    """one case of SHAPE_LABELS, built when it is asked for (the labels alone cost nothing at collection)"""
    at = SHAPE_LABELS.index(label)
    if at < len(MANY):
        # search widths: E + 1 = 64 words are one round of wave_upper_bound, 65 two (chunk = 2), 4096 two, 4097 and 4098 three
        # (chunk = 65: the second round is wider than 64 again).  ragged plan: per = ceil(E / 1024) entries a thread of k_zipw_plan,
        # a last thread with fewer at 1025, 4095 and 4097, none ragged at 1023, 1024, 2049 and 4096
        items, store = many_entries(MANY[at], 9200 + at)
        return _case(label, items, store=store)
    if label.startswith("rowless"):
        # the lone binary search of the gather: a row whose entry lies 64 or more entries behind the wave's first row's.  Every triple
        # -- an entry of k rows, R entries without rows, an entry of rows -- starts at a wave's first row (4 rows a wave), so the row
        # in front of the run stands at position k - 1 and, for k < 4, the row behind the run in the same wave: 63 or more entries
        # lie between them from R = 63 on
        r = np.random.default_rng(9300)
        items, store = [], []
        for R in RUNS:
            for k in RUN_ROWS:
                items.append((_name(len(items)), of_blocks(r, k, "sn"[k % 2])))
                store.append(False)
                for j in range(R):
                    _rowless(items, store, j)
                items.append((_name(len(items)), of_blocks(r, (4 - k) or 4, "sm"[R % 2])))
                store.append(False)
        return _case(label, items, store=store)
    if label.endswith("rows across the seams"):
        # the dispatch seam ROWS_MANY_MIN: the same entries cut to 65535 rows (16 rows a workgroup) and to 65536 (256 rows, 64 a wave);
        # entries begin on and beside wave, group and tile seams, three are noise (stored with rows over many tiles and groups)
        n = int(label.split()[0])
        r = np.random.default_rng(9400)
        data = [of_blocks(r, k, f) for k, f in zip(SEAM_ROWS, SEAM_FORMS)]
        items, left = [], n
        for e, d in enumerate(data):
            if left:
                items.append((_name(e), d[:32 * min(left, SEAM_ROWS[e])]))
                left -= min(left, SEAM_ROWS[e])
        return _case(label, items)
    if label.startswith("65535 entries"):
        # many entries and many rows at once: three rounds of the search with 64 rows a wave, per = 64 in the plan, and one run of 100
        # rowless entries so that the lone search is reached with 64 rows a wave, too
        items, store = many_entries(65535, 9500, rows=(0, 1, 2, 3), weights=(0.15, 0.5, 0.25, 0.1), run=MANY_ROWS_RUN)
        return _case(label, items, store=store)
    # stored tiles among many entries: the `tiles` workgroups search tile0[0 .. E] of about 300 entries, most of them of one tile or of
    # none.  (Their strided path needs more than 2^17 tiles, 8 GiB of stored entries: out of reach at test size, and not tested.)
    r = np.random.default_rng(9600)
    kind = r.integers(0, 8, 300).tolist()
    items, store = [], []
    for e in range(300):
        big = {40: 0, 41: 1, 150: 2, 299: 3}.get(e)
        if big is not None:
            items.append((_name(e), Z.noise(BIG_STORED[big], 9600 + e)))
        elif e in (3, 100, 298):
            items.append((_name(e), soft(3000 + 1111 * (e % 7), 9600 + e)))       # deflated, with rows
        else:
            items.append((_name(e), b"wxyz"[:kind[e] % 4 + 1] if kind[e] < 6 else b""))
        store.append(big is not None)
    return _case(label, items, block=2048, store=store)


def shape_cases():
    return [shape_case(label) for label in SHAPE_LABELS]


# ---- a model of the gather's row lookup, for the CPU test that proves from a case's arrays which branch the case reaches.  It
# asserts the CASES, never the device: what the file must be comes from expected() alone.
@functools.lru_cache(maxsize=None)
def kernel_constants():
    """the constants of hdlz_zip_write.hip and hdlz_frame.h the regimes hang on, read out of the source text"""
    import os
    import re
    from types import SimpleNamespace
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hdl_deflate_amd", "csrc")
    found = {}
    for name, path in (("ROWS_FEW", "hdlz_zip_write.hip"), ("ROWS_MAX", "hdlz_zip_write.hip"), ("ROWS_MANY_MIN", "hdlz_zip_write.hip"),
                       ("PLAN_THREADS", "hdlz_zip_write.hip"), ("STORE_TILE", "hdlz_zip_write.hip"), ("JT", "hdlz_frame.h")):
        m = re.findall(r"\b%s\s*=\s*([0-9u< ]+?)\s*[,;]" % name, open(os.path.join(csrc, path)).read())
        assert len(m) == 1, (name, m)
        expr = m[0].replace("u", "")
        assert re.fullmatch(r"[0-9]+( << [0-9]+)?", expr), (name, m[0])
        found[name] = eval(expr, {"__builtins__": {}})
    return SimpleNamespace(**found)


def wave_upper_bound(v, x):
    """wave_upper_bound of hdlz_zip_write.hip over the ascending numpy array v -> (how many words are <= x, rounds of loads)"""
    base, width, rounds = 0, len(v), 1
    lanes = np.arange(64)
    while width > 64:
        chunk = (width + 63) // 64
        p = (lanes + 1) * chunk - 1                              # lane i probes the last word of chunk i
        c = int(np.count_nonzero(v[base + p[p < width]] <= x))
        base += c * chunk
        width = min(width - c * chunk, chunk)
        rounds += 1
    return base + int(np.count_nonzero(v[base:base + width] <= x)), rounds


def gather_lookup(blk_first, nblocks):
    """the row lookup of k_zipw_gather -> a namespace: rows_per_group, per (rows a wave), rounds[wave] (the loads of the wave's own
    search), fallback[row] (the lane searches alone) and entry[row] (what the lookup finds: -1 for a row that no entry owns)"""
    from types import SimpleNamespace
    k = kernel_constants()
    F = np.asarray(blk_first, np.int64)
    E = len(F) - 1
    group = k.ROWS_MAX if nblocks >= k.ROWS_MANY_MIN else k.ROWS_FEW
    per = group // 4
    nwaves = -(-nblocks // group) * 4
    rounds, fallback, entry = np.zeros(nwaves, np.int64), np.zeros(nblocks, bool), np.full(nblocks, -1, np.int64)
    far = np.iinfo(np.int64).max
    for w in range(nwaves):
        b0 = w * per
        ub0, rounds[w] = wave_upper_bound(F, b0)
        nxt = np.full(64, far, np.int64)                         # lane l holds F[ub0 + l], or "none" behind F[E]
        nxt[:max(0, min(64, E + 1 - ub0))] = F[ub0:ub0 + 64]
        b = np.arange(b0, min(b0 + per, nblocks))
        c = np.searchsorted(nxt, b, side="right")                # the ballot: how many of the 64 words are <= b
        ub = ub0 + c
        alone = c == 64
        ub[alone] = np.searchsorted(F, b[alone], side="right")
        fallback[b] = alone
        entry[b] = np.where((ub >= 1) & (ub <= E), ub - 1, -1)
    return SimpleNamespace(rows_per_group=group, per=per, rounds=rounds, fallback=fallback, entry=entry)


def plan_share(E):
    """k_zipw_plan's split of E entries -> (per, threads that take `per` entries, entries of the one thread behind them that takes fewer)"""
    per = -(-E // kernel_constants().PLAN_THREADS)
    return per, (E // per if per else 0), (E % per if per else 0)


def batch_arrays(case):
    """(blk_first, nblocks) of a case as Engine.compress_zip plans it"""
    first = [0]
    for e, (_, d) in enumerate(case["items"]):
        first.append(first[-1] + len(plan(len(d), case["block"], bool(case["store"] and case["store"][e]))))
    return first, first[-1]


# ---- .npz: the entries save_npz hands to compress_zip, from the same headers
def npz_arrays():
    """name -> numpy array: every dtype of save_npz's table, a 0-d and an empty array among them"""
    r = np.random.default_rng(33)
    a = dict(b1=r.integers(0, 2, 77).astype(np.bool_), u1=r.integers(0, 256, (5, 41)).astype(np.uint8), i1=r.integers(-128, 128, 300).astype(np.int8),
             i2=np.arange(-700, 700, dtype=np.int16), i4=np.arange(5000, dtype=np.int32).reshape(50, 100), i8=np.arange(3000, dtype=np.int64) * 7,
             f2=np.linspace(0, 1, 333, dtype=np.float16), f4=np.linspace(0, 1, 3000, dtype=np.float32), f8=r.standard_normal(129),
             c8=(r.standard_normal(65) + 1j * r.standard_normal(65)).astype(np.complex64), c16=r.standard_normal(33) + 1j * r.standard_normal(33),
             scalar=np.array(2.5, dtype=np.float32), big=(np.arange(40000, dtype=np.int32) % 1000), empty=np.zeros((0, 3), np.uint8))
    return a


def npy_entry(arr):
    """the .npy version 1.0 entry of an array: numpy's own header writer, then the bytes in C order"""
    h = io.BytesIO()
    np.lib.format.write_array_header_1_0(h, {"descr": np.lib.format.dtype_to_descr(arr.dtype), "fortran_order": False, "shape": arr.shape})
    return h.getvalue() + np.ascontiguousarray(arr).tobytes()


def npz_items(arrays):
    return [(name + ".npy", npy_entry(a)) for name, a in arrays.items()]


# ---- running the device call
def check_written(label, w, out, index):
    """what Engine.compress_zip returned against the rule: the file byte for byte, the record, the entries' records"""
    got = out.cpu().numpy().tobytes()
    r = index.write_record
    assert (r.file_len, r.cd_off, r.cd_size, r.nstored, r.status, r.first_bad) == tuple(w.record[k] for k in ("file_len", "cd_off", "cd_size", "nstored", "status", "first_bad")), \
        (label, (r.file_len, r.cd_off, r.cd_size, r.nstored, r.status, r.first_bad), w.record)
    if got != w.file:
        at = next(i for i, (x, y) in enumerate(zip(got, w.file)) if x != y) if len(got) == len(w.file) else min(len(got), len(w.file))
        raise AssertionError((label, "the file differs at byte", at, got[max(0, at - 8):at + 8].hex(), w.file[max(0, at - 8):at + 8].hex()))
    want = Z.records(dict(entries=w.entries))
    have = Z.device_records(index)
    assert have == want, (label, [(k, g, x) for k, (g, x) in enumerate(zip(have, want)) if g != x][:3])
    assert not index.host["reserved"].any(), label
