"""What hdlz_zip_index_ws and hdlz_zip_inflate_ws must answer (a helper module like gunzip_ref.py, not a conftest): the index rule and
the judgement of include/hdlz_zip.h as a serial text in plain Python, with zlib and zlib.crc32 for the decode; a builder of archives by
hand; and the archives the CPU and the GPU tests share.  tests/test_zip_cabi.py holds this rule against zipfile on every one of them."""
import functools
import io
import struct
import zipfile
import zlib

import numpy as np

OK, E_OUT_CAPACITY, E_BAD_BTYPE, E_NO_EOF, E_BAD_PARAM, E_BAD_HEADER, E_BAD_CHECKSUM = 0, 2, 3, 5, 8, 11, 12
SIG_LOCAL, SIG_CD, SIG_EOCD, SIG_LOCATOR = b"PK\x03\x04", b"PK\x01\x02", b"PK\x05\x06", b"PK\x06\x07"
LARGE_MIN = 16384


def _u16(z, at):
    return z[at] | z[at + 1] << 8


def _u32(z, at):
    return int.from_bytes(z[at:at + 4], "little")


# ---- the index rule
def end_record(z):
    """step 1 -> (status, p, cd_off, cd_size, total)"""
    n = len(z)
    if n < 22:
        return E_NO_EOF, 0, 0, 0, 0
    p = None
    for q in range(n - 22, max(0, n - 22 - 65535) - 1, -1):          # the largest fitting offset
        if z[q:q + 4] == SIG_EOCD and q + 22 + _u16(z, q + 20) == n:
            p = q
            break
    if p is None:
        return E_BAD_HEADER, 0, 0, 0, 0
    if p >= 20 and z[p - 20:p - 16] == SIG_LOCATOR:
        return E_BAD_HEADER, 0, 0, 0, 0
    total, cd_size, cd_off = _u16(z, p + 10), _u32(z, p + 12), _u32(z, p + 16)
    if _u16(z, p + 4) or _u16(z, p + 6) or _u16(z, p + 8) != total or cd_off + cd_size != p:
        return E_BAD_HEADER, 0, 0, 0, 0
    return OK, p, cd_off, cd_size, total


def index(z, out_align=1, entry_cap=None):
    """the whole rule -> dict(status, nentries, total_out, cd_off, cd_size, entries); entries: a dict per PASSED entry (all of them,
    whatever entry_cap: the device writes the first entry_cap)"""
    z = bytes(z)
    st, p, cd_off, cd_size, total = end_record(z)
    if st != OK:
        return dict(status=st, nentries=0, total_out=0, cd_off=0, cd_size=0, entries=[])
    starts, q, walk = [], cd_off, OK
    for _ in range(total):
        if q + 46 > p or z[q:q + 4] != SIG_CD:
            walk = E_BAD_HEADER
            break
        q2 = q + 46 + _u16(z, q + 28) + _u16(z, q + 30) + _u16(z, q + 32)
        if q2 > p:
            walk = E_BAD_HEADER
            break
        starts.append(q)
        q = q2
    else:
        if q != p:
            walk = E_BAD_HEADER
    entries, o = [], 0
    for q in starts:
        flags, method, crc, csize, usize = _u16(z, q + 8), _u16(z, q + 10), _u32(z, q + 16), _u32(z, q + 20), _u32(z, q + 24)
        name_len, disk, L = _u16(z, q + 28), _u16(z, q + 34), _u32(z, q + 42)
        s, payload = OK, 0
        if flags & 0x41:
            s = E_BAD_BTYPE
        elif method not in (0, 8):
            s = E_BAD_BTYPE
        elif 0xFFFFFFFF in (csize, usize, L) or disk:
            s = E_BAD_HEADER
        elif method == 0 and csize != usize:
            s = E_BAD_HEADER
        elif L + 30 > cd_off or z[L:L + 4] != SIG_LOCAL:
            s = E_BAD_HEADER
        else:
            payload = L + 30 + _u16(z, L + 26) + _u16(z, L + 28)
            if payload + csize > cd_off:
                s, payload = E_BAD_HEADER, 0
        o = -(-o // out_align) * out_align
        entries.append(dict(cd_off=q, payload_off=payload, out_off=o, csize=csize, usize=usize, crc=crc, method=method, flags=flags,
                            name_len=name_len, status=s, name=z[q + 46:q + 46 + name_len]))
        o += usize if s == OK else 0
    n = len(entries)
    status = E_OUT_CAPACITY if entry_cap is not None and n > entry_cap else walk
    return dict(status=status, nentries=n, total_out=o, cd_off=cd_off, cd_size=cd_size, entries=entries)


FIELDS = ("cd_off", "payload_off", "out_off", "csize", "usize", "crc", "method", "flags", "name_len", "status")


# ---- the judgement
def judge(z, en, file_len=None):
    """one entry read -> (status, bytes or None).  status None: "any status but OK" -- zlib refuses the payload, and which word the
    device's decoder has for it is that decoder's business"""
    z = bytes(z)
    if en["status"] != OK:
        return en["status"], None
    p, c, u = en["payload_off"], en["csize"], en["usize"]
    if p < 30 or p + c + 4 > (len(z) if file_len is None else file_len):
        return E_BAD_PARAM, None
    if en["method"] == 0:
        data = z[p:p + u]
    else:
        if c > (1 << 28) - 7:
            return E_BAD_PARAM, None
        d = zlib.decompressobj(-15)
        try:
            data = d.decompress(z[p:p + c + 4])           # (the decoder's stream: the payload and the four bytes behind it)
        except zlib.error:
            return None, None
        if not d.eof:
            return None, None
        if len(data) > u:
            return E_OUT_CAPACITY, None
        if len(data) != u:
            return E_BAD_CHECKSUM, None
        if c + 4 - len(d.unused_data) != c:
            return E_NO_EOF, None
    if zlib.crc32(data) != en["crc"]:
        return E_BAD_CHECKSUM, None
    return OK, data


@functools.lru_cache(maxsize=None)
def read(z, out_align=1):
    """index and judgement of a whole file -> (the index, [status per entry], the flat output as the device leaves it inside the
    slots of the OK entries -- zeros elsewhere)"""
    ix = index(z, out_align)
    flat = bytearray(ix["total_out"])
    sts = []
    for en in ix["entries"]:
        st, data = judge(z, en)
        sts.append(st)
        if st == OK:
            flat[en["out_off"]:en["out_off"] + en["usize"]] = data
    return ix, sts, bytes(flat)


# ---- archives by hand
def deflate(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def make_zip(items, comment=b"", total=None, cd_gap=b""):
    """items: dicts with name and data (bytes) and, optionally, method (0 / 8), level, lextra / cextra (the local and the central extra
    field), ccomment, flags, lname (another name in the local header), descriptor (sizes and CRC behind the payload, zeros in the local
    header, flag bit 3) -> the file's bytes"""
    body, cd = bytearray(), bytearray()
    for it in items:
        name, data, method = it["name"], it["data"], it.get("method", 8)
        raw = deflate(data, it.get("level", 6)) if method == 8 else data
        flags = it.get("flags", 0) | (8 if it.get("descriptor") else 0)
        crc, lname, lextra = zlib.crc32(data), it.get("lname", name), it.get("lextra", b"")
        off = len(body)
        lc, ls, lu = (0, 0, 0) if it.get("descriptor") else (crc, len(raw), len(data))
        body += SIG_LOCAL + struct.pack("<HHHHHIIIHH", 20, flags, method, 0, 0x21, lc, ls, lu, len(lname), len(lextra)) + lname + lextra + raw
        if it.get("descriptor"):
            body += b"PK\x07\x08" + struct.pack("<III", crc, len(raw), len(data))
        cextra, cc = it.get("cextra", b""), it.get("ccomment", b"")
        cd += SIG_CD + struct.pack("<HHHHHHIIIHHHHHII", 20, 20, flags, method, 0, 0x21, crc, len(raw), len(data), len(name), len(cextra),
                                   len(cc), 0, 0, 0, off) + name + cextra + cc
    body += cd_gap
    n = len(items) if total is None else total
    return bytes(body + cd + SIG_EOCD + struct.pack("<HHHHIIH", 0, 0, n, n, len(cd), len(body), len(comment)) + comment)


def text(n, seed):
    r = np.random.default_rng(seed)
    return bytes(r.choice(np.frombuffer(b"abcdefgh \n", np.uint8), n))


def noise(n, seed):
    return bytes(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8))


class _Unseekable(object):
    """a stream zipfile cannot seek in: it writes data descriptors"""

    def __init__(self):
        self.buf = io.BytesIO()

    def write(self, b):
        return self.buf.write(b)

    def flush(self):
        pass


# ---- the archives: [(label, bytes)]
@functools.lru_cache(maxsize=None)
def writer_cases():
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w") as zf:
        zf.comment = b"an archive comment"
        k = 0
        for n in (0, 1, 5, 257, 2048, 70000):                     # (70000: above the 65536 the task view's comment names)
            zf.writestr(zipfile.ZipInfo("stored/%d.bin" % n), text(n, 10 + n), zipfile.ZIP_STORED)
            for level in (1, 6, 9):
                zi = zipfile.ZipInfo("n" * (1 + (37 * k) % 300))  # names of 1 to 300 bytes
                if k % 3 == 0:
                    zi.extra = struct.pack("<HH", 0x7075, 5) + b"extra"
                if k % 4 == 0:
                    zi.comment = b"an entry comment %d" % k
                zf.writestr(zi, text(n, 20 + k), zipfile.ZIP_DEFLATED, compresslevel=level)
                k += 1
        zf.writestr(zipfile.ZipInfo("n" * 300), text(900, 3), zipfile.ZIP_DEFLATED)
        zf.writestr(zipfile.ZipInfo("d/"), b"")
        zf.writestr("d/ümläut.txt", text(100, 4), zipfile.ZIP_DEFLATED)      # (flag bit 11: a UTF-8 name)
    arrays = dict(a=np.arange(5000, dtype=np.int64), b=np.linspace(0, 1, 3000, dtype=np.float32), c=np.float16(2.5),
                  d=np.zeros((0, 3), np.uint8), e=np.frombuffer(text(40000, 5), np.uint8).reshape(200, 200))
    nz, ns = io.BytesIO(), io.BytesIO()
    np.savez_compressed(nz, **arrays)
    np.savez(ns, **arrays)
    un = _Unseekable()
    with zipfile.ZipFile(un, "w", zipfile.ZIP_DEFLATED) as zf:
        for k, n in enumerate((0, 3, 1000, 30000)):
            zf.writestr("dd%d.txt" % k, text(n, 30 + k))
        zf.writestr(zipfile.ZipInfo("dd_stored"), text(777, 6), zipfile.ZIP_STORED)
    dd = un.buf.getvalue()
    assert dd[6] & 8 and dd[14:26] == bytes(12)                   # flag bit 3; CRC and sizes zero in the local header
    z = nz.getvalue()
    assert _u16(z, 28) == 20 and _u16(z, index(z)["entries"][0]["cd_off"] + 30) == 0       # local extra 20 bytes, central extra none
    return [("zipfile mixed", buf.getvalue()), ("savez_compressed", z), ("savez", ns.getvalue()), ("data descriptors", dd)]


@functools.lru_cache(maxsize=None)
def lookalike_cases():
    sigs = SIG_CD + bytes(42) + SIG_LOCAL + bytes(26) + SIG_EOCD + bytes(18)
    inner = make_zip([dict(name=b"inner.txt", data=text(50, 7))])
    items = [dict(name=b"PK\x01\x02PK\x03\x04PK\x05\x06", data=text(300, 8), lextra=struct.pack("<HH", 0x9999, len(sigs)) + sigs,
                  cextra=struct.pack("<HH", 0x9999, len(sigs)) + sigs, ccomment=sigs),
             dict(name=b"stored-signatures", data=sigs * 3, method=0),
             dict(name=b"plain", data=text(1000, 9))]
    # an end record inside the archive comment that does not fit (its comment length says 0, but bytes follow it)
    fake = SIG_EOCD + struct.pack("<HHHHIIH", 0, 0, 1, 1, 46, 0, 0)
    nested = make_zip([dict(name=b"first", data=text(200, 11)), dict(name=b"inner.zip", data=inner, method=0)])
    assert len(nested) - nested.rindex(inner) - len(inner) < 65535          # the inner end record lies inside the search window
    return [("signatures everywhere", make_zip(items, comment=b"c" + SIG_EOCD + b"PK\x01\x02")),
            ("an end record in the comment", make_zip(items[1:], comment=b"xx" + fake + b"tail")),
            ("a nested archive", nested)]


@functools.lru_cache(maxsize=None)
def geometry_cases():
    r = np.random.default_rng(12)
    many = make_zip([dict(name=b"%05d" % k, data=b"", method=0) for k in range(65535)])
    names = [bytes(r.integers(97, 123, int(n), dtype=np.uint8)) for n in r.integers(1, 701, 160)]
    long_dir = make_zip([dict(name=nm, data=text(20 + k, 40 + k), level=(1, 6, 9)[k % 3], method=(8, 8, 0)[k % 3]) for k, nm in enumerate(names)])
    assert index(long_dir)["cd_size"] > 3 * 16384                    # more than three staging pieces
    big = noise(2 * 65535, 13)
    one = make_zip([dict(name=b"before", data=text(64, 14)),
                    dict(name=text(65535, 17).replace(b"\n", b"_"), data=text(500, 15), cextra=struct.pack("<HH", 0x9999, 65531) + big[:65531],
                         ccomment=big[65535:]),
                    dict(name=b"after", data=text(64, 16), method=0)])
    assert index(one)["entries"][2]["cd_off"] - index(one)["entries"][1]["cd_off"] == 46 + 3 * 65535
    return [("65535 empty entries", many), ("names of 1 to 700", long_dir), ("a record of 46 + 3 * 65535", one)]


def base_items():
    """nine entries, deflated and stored, that the damage and the sub-range cases share"""
    return [dict(name=b"e%d.txt" % k, data=text(n, 50 + k), method=m, level=(1, 6, 9)[k % 3], lextra=b"\x11\x11\x02\x00ab" if k % 2 else b"")
            for k, (n, m) in enumerate(((300, 8), (0, 0), (5000, 8), (257, 0), (40000, 8), (1, 8), (2048, 0), (70000, 8), (10, 0)))]


def patch_cd(z, e, at, fmt, fn):
    """the archive with one field of entry e's central record changed: fn(old) at offset `at` of the record"""
    ix = index(z)
    q = ix["entries"][e]["cd_off"] + at
    b = bytearray(z)
    old = struct.unpack_from(fmt, b, q)[0]
    struct.pack_into(fmt, b, q, fn(old) & (0xFFFFFFFF if fmt == "<I" else 0xFFFF))
    return bytes(b)


@functools.lru_cache(maxsize=None)
def entry_damage_cases():
    """[(label, bytes, the entry that must fail, its status)] -- exactly that entry fails (damage on a deflated and on a stored one)"""
    z = make_zip(base_items())
    ix = index(z)
    out = []
    for e in (2, 3):                                              # entry 2 is deflated, entry 3 stored
        en = ix["entries"][e]
        b = bytearray(z)
        b[en["payload_off"] + en["csize"] // 2] ^= 0x10
        st = E_BAD_CHECKSUM if en["method"] == 0 else judge(bytes(b), en)[0]
        out.append(("payload byte flipped, entry %d" % e, bytes(b), e, st))
        out.append(("directory CRC flipped, entry %d" % e, patch_cd(z, e, 16, "<I", lambda v: v ^ 0x100), e, E_BAD_CHECKSUM))
        loc = bytearray(z)
        loc[_u32(z, en["cd_off"] + 42) + 2] ^= 1
        out.append(("local signature broken, entry %d" % e, bytes(loc), e, E_BAD_HEADER))
        out.append(("encryption flag, entry %d" % e, patch_cd(z, e, 8, "<H", lambda v: v | 1), e, E_BAD_BTYPE))
        out.append(("method 12, entry %d" % e, patch_cd(z, e, 10, "<H", lambda v: 12), e, E_BAD_BTYPE))
        out.append(("local offset behind cd_off, entry %d" % e, patch_cd(z, e, 42, "<I", lambda v: ix["cd_off"] + 8), e, E_BAD_HEADER))
    out.append(("usize + 1", patch_cd(z, 2, 24, "<I", lambda v: v + 1), 2, E_BAD_CHECKSUM))
    out.append(("usize - 1", patch_cd(z, 2, 24, "<I", lambda v: v - 1), 2, E_OUT_CAPACITY))
    out.append(("csize - 1", patch_cd(z, 2, 20, "<I", lambda v: v - 1), 2, E_NO_EOF))
    out.append(("csize + 1", patch_cd(z, 2, 20, "<I", lambda v: v + 1), 2, E_NO_EOF))
    out.append(("stored: usize + 1", patch_cd(z, 3, 24, "<I", lambda v: v + 1), 3, E_BAD_HEADER))
    return out


@functools.lru_cache(maxsize=None)
def file_damage_cases():
    """[(label, bytes, the record's status, entries that stay indexed)]"""
    items = base_items()[:8]
    z = make_zip(items)
    ix = index(z)
    p = ix["cd_off"] + ix["cd_size"]
    locator = SIG_LOCATOR + struct.pack("<IQI", 0, 0, 1)
    sig3 = bytearray(z)
    sig3[ix["entries"][3]["cd_off"] + 1] ^= 0x20
    shifted = bytearray(z)
    struct.pack_into("<I", shifted, p + 16, ix["cd_off"] + 1)
    return [("a ZIP64 locator", make_zip(items, cd_gap=b"")[:p] + locator + z[p:], E_BAD_HEADER, 0),
            ("a cut end record", z[:-1], E_BAD_HEADER, 0),
            ("only 21 bytes", z[-21:], E_NO_EOF, 0),
            ("an entry count one too many", make_zip(items, total=9), E_BAD_HEADER, 8),
            ("an entry count one too few", make_zip(items, total=7), E_BAD_HEADER, 7),
            ("cd_off + cd_size != p", bytes(shifted), E_BAD_HEADER, 0),
            ("directory signature broken at entry 3 of 8", bytes(sig3), E_BAD_HEADER, 3)]


def all_archives():
    """every archive the GPU tests index: (label, bytes)"""
    return (list(writer_cases()) + list(lookalike_cases()) + list(geometry_cases()) + [(c[0], c[1]) for c in entry_damage_cases()] +
            [(c[0], c[1]) for c in file_damage_cases()] + [("nine entries", make_zip(base_items()))])


# ---- running the device calls
def records(ix):
    """the index's entries as tuples in FIELDS order"""
    return [tuple(int(en[f]) for f in FIELDS) for en in ix["entries"]]


def device_records(zi):
    return [tuple(int(r[f]) for f in FIELDS) for r in zi.host]


def stage(z, slack=b"\xAA" * 64):
    """the file on the device, with bytes behind it that are not the file's -> the tensor of exactly the file"""
    import torch
    return torch.frombuffer(bytearray(bytes(z) + slack), dtype=torch.uint8).cuda()[:len(z)]


def check_index(label, z, zi, out_align=1, entry_cap=None):
    """a ZipIndex against the rule: the record and every record written"""
    ix = index(z, out_align, entry_cap)
    r = zi.record
    assert (r.status, r.nentries, r.total_out, r.cd_off, r.cd_size) == (ix["status"], ix["nentries"], ix["total_out"], ix["cd_off"], ix["cd_size"]), \
        (label, (r.status, r.nentries, r.total_out, r.cd_off, r.cd_size), {k: v for k, v in ix.items() if k != "entries"})
    want = records(ix)[:len(zi.host)]
    got = device_records(zi)
    assert len(got) == (ix["nentries"] if entry_cap is None else min(entry_cap, ix["nentries"])), (label, len(got))
    assert got == want, (label, [(k, g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w][:3])
    return ix


def check_read(label, z, ix, sts, flat, first, out, out_off, status):
    """what Engine.inflate_zip returned for entries [first, first + len(status)) against zip_ref.read's results of the whole file"""
    out, out_off, status = out.cpu().numpy(), out_off.cpu().numpy(), status.cpu().numpy().view(np.uint32)
    base = ix["entries"][first]["out_off"] if len(status) else 0
    for k in range(len(status)):
        en, want = ix["entries"][first + k], sts[first + k]
        assert int(out_off[k]) == en["out_off"] - base, (label, first + k, "out_off")
        if want is None:
            assert status[k] != OK, (label, first + k, "must not be OK")
            continue
        assert status[k] == want, (label, first + k, "status", int(status[k]), want)
        if want == OK:
            assert out[out_off[k]:out_off[k] + en["usize"]].tobytes() == flat[en["out_off"]:en["out_off"] + en["usize"]], (label, first + k, "bytes")


def run_inflate(engine, d, zi, first, count, in_len=0):
    """ONE hdlz_zip_inflate_ws over entries [first, first + count) of a ZipIndex, the output exactly as large as the range asks
    (count == 1: rounded up to 4, the row of the one-stream route) -> (out, out_off, status, the call's record)"""
    import torch
    from hdl_deflate_amd import _lib
    host, last = zi.host, first + count - 1
    total = int(host["out_off"][last] - host["out_off"][first]) + (int(host["usize"][last]) if host["status"][last] == OK else 0) if count else 0
    cap = (total + 3) & ~3 if count == 1 else total
    out = torch.zeros(cap + 64, dtype=torch.uint8, device=d.device)
    status = torch.full((count,), 0x55555555, dtype=torch.int32, device=d.device)
    need = engine.lib.hdlz_zip_inflate_work_bytes(count, in_len, cap)
    rec = engine._record("hdlz_zip_inflate_ws", _lib.ZipInflateResult, engine._scratch(need, None), d.data_ptr(), d.numel(), zi.entries.data_ptr(),
                         first, count, in_len, out.data_ptr(), cap, status.data_ptr())
    assert bool((out[cap:] == 0).all()), "bytes at or behind out_cap were written"
    out_off = zi.entries[first:first + count, 2] - (zi.entries[first, 2] if count else 0)
    return out[:total], out_off, status, rec
