"""What hdlz_zip64_index_ws, hdlz_zip64_inflate_ws and hdlz_zip64_write_ws must answer (a helper module like zip_ref.py and
zip_write_ref.py, which it builds on, not a conftest): THE INDEX RULE and THE FILE RULE of include/hdlz_zip64.h as serial texts in plain
Python (index, expected); a builder of ZIP64 archives by hand (zipfile cannot be made to write most of these layouts); and the
archives and the writer's cases the CPU and the GPU tests share.  tests/test_zip64_cabi.py holds this rule against
zipfile, unzip and numpy on them.  The judgement of an entry is zip_ref.judge: it is the same in 64 bits."""
import functools
import io
import struct
import zipfile
import zlib

import numpy as np

import zip_ref as Z
from zip_ref import OK, E_OUT_CAPACITY, E_BAD_BTYPE, E_NO_EOF, E_BAD_PARAM, E_BAD_HEADER, E_BAD_CHECKSUM, _u16, _u32  # noqa: F401

SIG_END64 = b"PK\x06\x06"
ONES16, ONES32 = 0xFFFF, 0xFFFFFFFF
FIELDS = Z.FIELDS


def _u64(z, at):
    return int.from_bytes(z[at:at + 8], "little")


class DeviceBytes(object):
    """a flat uint8 device tensor read like bytes -- z[at], z[a:b], len(z) -- one small copy a read: what lets the rule below parse the
    tail of a file of more than 4 GiB that never leaves the device"""

    def __init__(self, d):
        self.d = d

    def __len__(self):
        return self.d.numel()

    def __getitem__(self, k):
        if isinstance(k, slice):
            return self.d[k].cpu().numpy().tobytes()
        return int(self.d[k])


class DeviceFile(object):
    """the same tensor as the binary file zipfile.ZipFile opens: read / seek / tell from slices of it, so a stock reader sees only
    the directory and what is asked of it"""

    def __init__(self, d):
        self.d, self.pos = d, 0

    def seekable(self):
        return True

    def tell(self):
        return self.pos

    def seek(self, off, whence=0):
        self.pos = off + (0, self.pos, self.d.numel())[whence]
        return self.pos

    def read(self, n=-1):
        end = self.d.numel() if n is None or n < 0 else min(self.d.numel(), self.pos + n)
        out = self.d[self.pos:end].cpu().numpy().tobytes()
        self.pos = max(self.pos, end)
        return out


# ---- the index rule
def end_record(z):
    """step 1 -> (status, D, cd_off, cd_size, total): D is where the directory ends"""
    bad = (E_BAD_HEADER, 0, 0, 0, 0)
    n = len(z)
    if n < 22:
        return E_NO_EOF, 0, 0, 0, 0
    p, lo = None, max(0, n - 22 - 65535)
    tail = z[lo:n]                                                   # (one read of the search window)
    for q in range(n - 22, lo - 1, -1):                               # the largest fitting offset
        if tail[q - lo:q - lo + 4] == Z.SIG_EOCD and q + 22 + _u16(tail, q - lo + 20) == n:
            p = q
            break
    if p is None:
        return bad
    c_disk, c_cddisk, c_here, c_total, c_size, c_off = _u16(z, p + 4), _u16(z, p + 6), _u16(z, p + 8), _u16(z, p + 10), _u32(z, p + 12), _u32(z, p + 16)
    if p >= 20 and z[p - 20:p - 16] == Z.SIG_LOCATOR:
        if _u32(z, p - 16) != 0 or _u32(z, p - 4) > 1:
            return bad
        r = _u64(z, p - 12)
        if r + 56 > p - 20 or z[r:r + 4] != SIG_END64:
            return bad
        s = _u64(z, r + 4)
        if s < 44 or r + 12 + s != p - 20:
            return bad
        total = _u64(z, r + 32)
        if _u32(z, r + 16) or _u32(z, r + 20) or _u64(z, r + 24) != total:
            return bad
        cd_size, cd_off = _u64(z, r + 40), _u64(z, r + 48)
        if cd_off + cd_size != r:
            return bad
        if total > cd_size // 46:
            return bad
        for classic, true, ones in ((c_disk, 0, ONES16), (c_cddisk, 0, ONES16), (c_here, total, ONES16), (c_total, total, ONES16),
                                    (c_size, cd_size, ONES32), (c_off, cd_off, ONES32)):
            if classic != true and classic != ones:
                return bad
        return OK, r, cd_off, cd_size, total
    if c_disk or c_cddisk or c_here != c_total or c_off + c_size != p:
        return bad
    return OK, p, c_off, c_size, c_total


def zip64_field(z, q):
    """the data of X, the first extra field with id 0001 of the central record at q (b"" without one)"""
    n, m = _u16(z, q + 28), _u16(z, q + 30)
    x = z[q + 46 + n:q + 46 + n + m]
    at = 0
    while m - at >= 4:
        fid, ln = _u16(x, at), _u16(x, at + 2)
        if ln > m - at - 4:
            break
        if fid == 1:
            return x[at + 4:at + 4 + ln]
        at += 4 + ln
    return b""


def index(z, out_align=1, entry_cap=None):
    """the whole rule -> dict(status, nentries, total_out, cd_off, cd_size, entries); entries: a dict per PASSED entry (all of them,
    whatever entry_cap: the device writes the first entry_cap, and total_out counts those only)"""
    z = z if isinstance(z, DeviceBytes) else bytes(z)
    st, D, cd_off, cd_size, total = end_record(z)
    if st != OK:
        return dict(status=st, nentries=0, total_out=0, cd_off=0, cd_size=0, entries=[])
    starts, q, walk = [], cd_off, OK
    for _ in range(total):
        if q + 46 > D or z[q:q + 4] != Z.SIG_CD:
            walk = E_BAD_HEADER
            break
        q2 = q + 46 + _u16(z, q + 28) + _u16(z, q + 30) + _u16(z, q + 32)
        if q2 > D:
            walk = E_BAD_HEADER
            break
        starts.append(q)
        q = q2
    else:
        if q != D:
            walk = E_BAD_HEADER
    entries, o, total_out = [], 0, 0
    for k, q in enumerate(starts):
        flags, method, crc, csize, usize = _u16(z, q + 8), _u16(z, q + 10), _u32(z, q + 16), _u32(z, q + 20), _u32(z, q + 24)
        name_len, disk, L = _u16(z, q + 28), _u16(z, q + 34), _u32(z, q + 42)
        s, payload = OK, 0
        if flags & 0x41:
            s = E_BAD_BTYPE
        elif method not in (0, 8):
            s = E_BAD_BTYPE
        else:
            x, short = zip64_field(z, q), False
            vals = [usize, csize, L]
            for j in range(3):                                        # usize, csize, L: 8 bytes each, only where the word is all ones
                if vals[j] == ONES32 and not short:
                    if len(x) < 8:
                        short = True
                    else:
                        vals[j], x = _u64(x, 0), x[8:]
            usize, csize, L = vals
            if disk == ONES16 and not short:
                if len(x) < 4:
                    short = True
                else:
                    disk = _u32(x, 0)
            if short:
                s = E_BAD_HEADER
            elif disk:
                s = E_BAD_HEADER
            elif method == 0 and csize != usize:
                s = E_BAD_HEADER
            elif L + 30 > cd_off or z[L:L + 4] != Z.SIG_LOCAL:
                s = E_BAD_HEADER
            else:
                payload = L + 30 + _u16(z, L + 26) + _u16(z, L + 28)
                if payload + csize > cd_off:
                    s, payload = E_BAD_HEADER, 0
        o = -(-o // out_align) * out_align
        entries.append(dict(cd_off=q, payload_off=payload, out_off=o, csize=csize, usize=usize, crc=crc, method=method, flags=flags,
                            name_len=name_len, status=s, name=z[q + 46:q + 46 + name_len]))
        o += usize if s == OK else 0
        if entry_cap is None or k < entry_cap:
            total_out = o
    n = len(entries)
    status = E_OUT_CAPACITY if entry_cap is not None and n > entry_cap else walk
    return dict(status=status, nentries=n, total_out=total_out, cd_off=cd_off, cd_size=cd_size, entries=entries)


@functools.lru_cache(maxsize=None)
def read(z, out_align=1):
    """zip_ref.read under this rule -> (the index, [status per entry], the flat output)"""
    ix = index(z, out_align)
    flat = bytearray(ix["total_out"])
    sts = []
    for en in ix["entries"]:
        st, data = Z.judge(z, en)
        sts.append(st)
        if st == OK:
            flat[en["out_off"]:en["out_off"] + en["usize"]] = data
    return ix, sts, bytes(flat)


# ---- archives by hand
def field(fid, data):
    return struct.pack("<HH", fid, len(data)) + data


def make_zip64(items, comment=b"", locator=True, classic="ones", sector=b"", always=False):
    """items: as zip_ref.make_zip takes them (name, data, method, level, lextra, cextra, ccomment, flags) and
         ones     which of "usize", "csize", "L", "disk" are all ones in the central record, the ZIP64 field supplying exactly those
                  (always=True: usize, csize and L for every item); a local header whose sizes are named gets FFFFFFFF sizes and
                  the 20-byte local field
         before / after   extra fields in front of / behind the ZIP64 one in the central record
         xdata    the ZIP64 field's data instead of what `ones` asks for; xdrop: the field left out altogether
         disk     the disk start the field supplies (default 0)
    locator: the ZIP64 end record and locator in front of the classic end record, whose six values are all ones (classic="ones") or
    the true ones as far as they fit (classic="true"); sector: the ZIP64 end record's extensible data"""
    body, cd = bytearray(), bytearray()
    for it in items:
        name, data, method = it["name"], it["data"], it.get("method", 8)
        raw = Z.deflate(data, it.get("level", 6)) if method == 8 else data
        flags, crc = it.get("flags", 0), zlib.crc32(data)
        ones = it.get("ones", ("usize", "csize", "L") if always else ())
        off = len(body)
        lextra = it.get("lextra", b"")
        ls, lu = len(raw), len(data)
        sized = "usize" in ones or "csize" in ones
        if sized:
            lextra = field(1, struct.pack("<QQ", lu, ls)) + lextra
            ls = lu = ONES32
        body += Z.SIG_LOCAL + struct.pack("<HHHHHIIIHH", 45 if sized else 20, flags, method, 0, 0x21, crc, ls, lu, len(name), len(lextra)) + name + lextra + raw
        x = b""
        for key, fmt, val in (("usize", "<Q", len(data)), ("csize", "<Q", len(raw)), ("L", "<Q", off), ("disk", "<I", it.get("disk", 0))):
            if key in ones:
                x += struct.pack(fmt, val)
        x = it.get("xdata", x)
        cextra = it.get("before", b"") + (b"" if it.get("xdrop") or not (ones or "xdata" in it) else field(1, x)) + it.get("after", b"") + it.get("cextra", b"")
        cc = it.get("ccomment", b"")
        cd += Z.SIG_CD + struct.pack("<HHHHHHIIIHHHHHII", 45 if ones else 20, 45 if ones else 20, flags, method, 0, 0x21, crc,
                                     ONES32 if "csize" in ones else len(raw), ONES32 if "usize" in ones else len(data), len(name), len(cextra),
                                     len(cc), ONES16 if "disk" in ones else 0, 0, 0, ONES32 if "L" in ones else off) + name + cextra + cc
    n, cd_off, cd_size = len(items), len(body), len(cd)
    tail = b""
    if locator:
        tail += SIG_END64 + struct.pack("<QHHIIQQQQ", 44 + len(sector), 45, 45, 0, 0, n, n, cd_size, cd_off) + sector
        tail += Z.SIG_LOCATOR + struct.pack("<IQI", 0, cd_off + cd_size, 1)
    if locator and classic == "ones":
        end = struct.pack("<HHHHIIH", ONES16, ONES16, ONES16, ONES16, ONES32, ONES32, len(comment))
    else:
        end = struct.pack("<HHHHIIH", 0, 0, min(n, ONES16), min(n, ONES16), min(cd_size, ONES32), min(cd_off, ONES32), len(comment))
    return bytes(body + cd + tail + Z.SIG_EOCD + end + comment)


def three_items():
    return [dict(name=b"first.txt", data=Z.text(300, 61)), dict(name=b"second.bin", data=Z.noise(77, 62), method=0),
            dict(name=b"third.txt", data=Z.text(5000, 63), level=9)]


SUBSETS = [tuple(k for j, k in enumerate(("usize", "csize", "L", "disk")) if s >> j & 1) for s in range(16)]
OTHER_A, OTHER_B = field(0x5455, b"\x01" + struct.pack("<I", 1700000000)), field(0x000A, bytes(28))


@functools.lru_cache(maxsize=None)
def crafted_cases():
    """[(label, bytes)]: well-formed files every reader accepts"""
    out = [("always, %d entries" % n, make_zip64(three_items()[:n], always=True)) for n in (0, 1, 3)]
    for ones in SUBSETS:                                              # entry 1 (stored) and entry 2 (deflated) carry the subset
        items = three_items()
        items[1]["ones"] = items[2]["ones"] = ones
        out.append(("all ones: %s" % ("+".join(ones) or "nothing"), make_zip64(items, locator=bool(len(ones) & 1), classic="true")))
    for label, before, after in (("in front", b"", OTHER_A + OTHER_B), ("between", OTHER_A, OTHER_B), ("behind", OTHER_A + OTHER_B, b"")):
        items = three_items()
        for it in items:
            it.update(ones=("usize", "csize", "L"), before=before, after=after)
        out.append(("the ZIP64 field %s other fields" % label, make_zip64(items)))
    out.append(("a comment behind the end record", make_zip64(three_items(), always=True, comment=b"a comment of some length")))
    out.append(("an extensible data sector", make_zip64(three_items(), always=True, sector=bytes(range(12)))))
    out.append(("a locator, true classic values", make_zip64(three_items(), classic="true")))
    return out


def _zipfile_many(n):
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w") as zf:
        for k in range(n):
            zf.writestr(zipfile.ZipInfo("%06d" % k), b"x" if k % 1000 == 7 else b"")
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def many_cases():
    """zipfile-written files around 65535 entries (65536 on: counts FFFF, a locator, true cd_size and cd_off) and a crafted one of
    131073 entries, which crosses two windows of 65536 in the walk and the scan"""
    big = make_zip64([dict(name=b"%06d" % k, data=b"y" * (k % 3) if k % 4099 == 0 else b"", method=0, ones=("L",) if k % 2 else ()) for k in range(131073)])
    return [("zipfile, %d entries" % n, _zipfile_many(n)) for n in (65535, 65536, 65537)] + [("crafted, 131073 entries", big)]


def straddle_case(k):
    """two entries whose second central record (46 + 4 + 28 bytes, the ZIP64 field at its end) starts k bytes in front of the first
    16 KiB staging piece's end"""
    first = dict(name=b"n" * (16384 - k - 46 - 28), data=b"one", method=0, ones=("usize", "csize", "L"))
    z = make_zip64([first, dict(name=b"two.", data=Z.text(40, 64), ones=("usize", "csize", "L")), dict(name=b"three", data=b"3", method=0)])
    assert index(z)["entries"][1]["cd_off"] - index(z)["cd_off"] == 16384 - k
    return z


STRADDLES = range(0, 46 + 4 + 28 + 1)


def _patch(z, at, fmt, value):
    b = bytearray(z)
    struct.pack_into(fmt, b, at, value)
    return bytes(b)


@functools.lru_cache(maxsize=None)
def bad_cases():
    """[(label, bytes, the record's status, entries indexed, the entry that fails or None)]: each one edit away from a good file"""
    good = make_zip64(three_items(), always=True)
    ix = index(good)
    assert ix["status"] == OK and [e["status"] for e in ix["entries"]] == [OK] * 3
    r = ix["cd_off"] + ix["cd_size"]
    p = r + 56 + 20
    assert good[p:p + 4] == Z.SIG_EOCD and good[r:r + 4] == SIG_END64
    sector = make_zip64(three_items(), always=True, sector=bytes(12))
    true = make_zip64(three_items(), always=True, classic="true")

    def entry(**kw):
        items = three_items()
        for it in items:
            it["ones"] = ("usize", "csize", "L")
        items[1].update(kw)
        return make_zip64(items)

    files = [("locator disk 1", _patch(good, p - 16, "<I", 1)), ("disk count 2", _patch(good, p - 4, "<I", 2)),
             ("r off by one", _patch(good, p - 12, "<Q", r + 1)), ("a broken ZIP64 end signature", _patch(good, r, "<I", 0x06064B51)),
             ("s too small", _patch(good, r + 4, "<Q", 43)), ("s not fitting", _patch(sector, r + 4, "<Q", 44)),
             ("cd_off + cd_size != r", _patch(good, r + 48, "<Q", ix["cd_off"] + 1)), ("entries on this disk != total", _patch(good, r + 24, "<Q", 2)),
             ("total > cd_size / 46", _patch(_patch(good, r + 24, "<Q", ix["cd_size"] // 46 + 1), r + 32, "<Q", ix["cd_size"] // 46 + 1)),
             ("a classic count that is neither", _patch(true, p + 10, "<H", 2))]
    out = [(label, z, E_BAD_HEADER, 0, None) for label, z in files]
    out.append(("a needed value with no field", entry(xdrop=True), OK, 3, 1))
    out.append(("a field 4 bytes short", entry(xdata=bytes(20)), OK, 3, 1))
    out.append(("a field overrunning m in front of the ZIP64 one", entry(before=struct.pack("<HH", 0x9999, 200)), OK, 3, 1))
    out.append(("a disk start of 1 through the field", entry(ones=("usize", "csize", "L", "disk"), disk=1), OK, 3, 1))
    return out


def all_cases():
    """every archive the GPU tests index but the large ones: (label, bytes)"""
    return list(crafted_cases()) + [(c[0], c[1]) for c in bad_cases()]


# ---- THE FILE RULE of include/hdlz_zip64.h (hdlz_zip64_write_ws): zip_write_ref.expected with the ZIP64 forms
def write_bound(nentries, total_in, names_len):
    return 98 + 124 * nentries + 2 * names_len + total_in


def write_work_bytes(nentries, nblocks):
    r = lambda x: (x + 255) // 256 * 256
    return r(8 + 16 * ((nblocks + 255) // 256)) + 2 * r(8 * (nblocks + 1)) + 256 + 4 * r(8 * (nentries + 1)) + 2 * r(4 * (nentries + 1))


def expected(items, zip64_from=ONES32, block=32, cwindow=32, maxmatch=10, store=None, date_time=None, out_align=1, file_cap=None):
    """items: [(name, data)] -> zip_write_ref.Written under THE FILE RULE of hdlz_zip64.h, and on it: local[e] / central[e], the tuples of
    ("usize", "csize", "L") that stand in entry e's local / central ZIP64 extra, and end64: the ZIP64 end record is there"""
    import joined_ref as J
    import zip_write_ref as W
    raw, flags = W.encode_names([n for n, _ in items])
    dt = W.dos_datetime(date_time or W.DATE_TIME)
    time, date = dt & 0xFFFF, dt >> 16
    w = W.Written()
    body, cd = bytearray(), bytearray()
    w.entries, w.methods, w.local, w.central = [], [], [], []
    o, f = 0, zip64_from
    for e, (nm, (_, data)) in enumerate(zip(raw, items)):
        data = bytes(data)
        blocks = W.plan(len(data), block, bool(store and store[e]))
        method, payload = 0, data
        if blocks:
            deflated = b"".join(J.member_of(data[a:a + ln], cwindow, maxmatch)[3] for a, ln in blocks) + b"\x03\x00"
            if len(deflated) < len(data):
                method, payload = 8, deflated
        crc, u, c, L = zlib.crc32(data), len(data), len(payload), len(body)
        loc = ("usize", "csize") if u >= f or c >= f else ()
        cen = tuple(k for k, v in (("usize", u), ("csize", c), ("L", L)) if v >= f)
        ver = 45 if loc or cen else 20
        lx = struct.pack("<HHQQ", 1, 16, u, c) if loc else b""
        body += Z.SIG_LOCAL + struct.pack("<HHHHHIIIHH", ver, flags, method, time, date, crc, ONES32 if loc else c, ONES32 if loc else u, len(nm), len(lx)) + nm + lx
        pay = len(body)
        body += payload
        cx = field(1, b"".join(struct.pack("<Q", v) for k, v in (("usize", u), ("csize", c), ("L", L)) if k in cen)) if cen else b""
        o = -(-o // out_align) * out_align
        w.entries.append(dict(cd_off=len(cd), payload_off=pay, out_off=o, csize=c, usize=u, crc=crc, method=method, flags=flags, name_len=len(nm),
                              status=OK, name=nm))
        o += u
        cd += Z.SIG_CD + struct.pack("<HHHHHHIIIHHHHHII", ver, ver, flags, method, time, date, crc, ONES32 if "csize" in cen else c,
                                     ONES32 if "usize" in cen else u, len(nm), len(cx), 0, 0, 0, 0, ONES32 if "L" in cen else L) + nm + cx
        w.methods.append(method)
        w.local.append(loc)
        w.central.append(cen)
    E, cd_off, cd_size = len(items), len(body), len(cd)
    for en in w.entries:
        en["cd_off"] += cd_off
    w.end64 = E > 65535 or cd_off >= f or cd_size >= f
    tail = b""
    if w.end64:
        tail = SIG_END64 + struct.pack("<QHHIIQQQQ", 44, 45, 45, 0, 0, E, E, cd_size, cd_off) + Z.SIG_LOCATOR + struct.pack("<IQI", 0, cd_off + cd_size, 1)
    tail += Z.SIG_EOCD + struct.pack("<HHHHIIH", 0, 0, min(E, ONES16), min(E, ONES16), ONES32 if cd_size >= f else cd_size, ONES32 if cd_off >= f else cd_off, 0)
    w.file = bytes(body + cd + tail)
    status = E_OUT_CAPACITY if file_cap is not None and len(w.file) > file_cap else OK
    w.record = dict(file_len=len(w.file), cd_off=cd_off, cd_size=cd_size, nstored=w.methods.count(0), status=status, first_bad=ONES32)
    return w


@functools.lru_cache(maxsize=None)
def written(label, zip64_from=ONES32, out_align=1):
    import zip_write_ref as W
    c = {c["label"]: c for c in W.all_cases()}[label]
    return expected(c["items"], zip64_from, block=c["block"], store=c["store"], out_align=out_align)


@functools.lru_cache(maxsize=None)
def between(label):
    """a zip64_from for a case of zip_write_ref.all_cases(): the median of its entries' sizes and local offsets and of cd_off (0 without
    entries), so that some values lie on either side of it"""
    w = written(label)
    vals = sorted([en["usize"] for en in w.entries] + [en["csize"] for en in w.entries] + local_offsets(w) + [w.record["cd_off"]])
    return vals[len(vals) // 2] if w.entries else 0


def local_offsets(w):
    return [en["payload_off"] - 30 - en["name_len"] - (20 if loc else 0) for en, loc in zip(w.entries, getattr(w, "local", [()] * len(w.entries)))]


def many_items(E):
    """E tiny entries: the count is what matters -- most are empty, some hold a few bytes (stored: under 5)"""
    return [("%07d" % k, b"abc"[:k % 4] if k % 997 == 0 else b"") for k in range(E)]


def check_written(label, w, out, index):
    """what Engine.compress_zip returned through hdlz_zip64_write_ws against the rule: the file byte for byte, the record, the records"""
    got = out.cpu().numpy().tobytes()
    r = index.write_record
    have = (r.file_len, r.cd_off, r.cd_size, r.nstored, r.status, r.first_bad)
    assert have == tuple(w.record[k] for k in ("file_len", "cd_off", "cd_size", "nstored", "status", "first_bad")), (label, have, w.record)
    if got != w.file:
        at = next(i for i, (x, y) in enumerate(zip(got, w.file)) if x != y) if len(got) == len(w.file) else min(len(got), len(w.file))
        raise AssertionError((label, "the file differs at byte", at, got[max(0, at - 8):at + 8].hex(), w.file[max(0, at - 8):at + 8].hex()))
    assert index.zip64 and index.host.dtype.itemsize == 64 and not index.host["reserved"].any() and not index.host["reserved2"].any(), label
    for f in FIELDS:
        want = np.array([en[f] for en in w.entries], dtype=np.uint64)
        diff = np.nonzero(index.host[f].astype(np.uint64) != want)[0]
        assert not len(diff), (label, f, int(diff[0]), int(index.host[f][diff[0]]), int(want[diff[0]]))


# ---- running the device calls
def check_index(label, z, zi, out_align=1, entry_cap=None, ix=None):
    """a ZipIndex of hdlz_zip64_index_ws against the rule (ix: the rule's answer where the caller has it): the record and every
    record written"""
    ix = index(z, out_align, entry_cap) if ix is None else ix
    r = zi.record
    assert zi.zip64 and zi.host.dtype.itemsize == 64 and not zi.host["reserved"].any() and not zi.host["reserved2"].any(), label
    assert (r.status, r.nentries, r.total_out, r.cd_off, r.cd_size) == (ix["status"], ix["nentries"], ix["total_out"], ix["cd_off"], ix["cd_size"]), \
        (label, (r.status, r.nentries, r.total_out, r.cd_off, r.cd_size), {k: v for k, v in ix.items() if k != "entries"})
    k = ix["nentries"] if entry_cap is None else min(entry_cap, ix["nentries"])
    assert len(zi.host) == k, (label, len(zi.host))
    for f in FIELDS:                                                  # (by field, as arrays: the files of 10^5 entries stay quick)
        want = np.array([en[f] for en in ix["entries"][:k]], dtype=np.uint64)
        diff = np.nonzero(zi.host[f].astype(np.uint64) != want)[0]
        assert not len(diff), (label, f, int(diff[0]), int(zi.host[f][diff[0]]), int(want[diff[0]]))
    return ix


def run_inflate(engine, d, zi, first, count, in_len=0):
    """zip_ref.run_inflate with hdlz_zip64_inflate_ws"""
    import torch
    from hdl_deflate_amd import _lib
    host, last = zi.host, first + count - 1
    total = int(host["out_off"][last] - host["out_off"][first]) + (int(host["usize"][last]) if host["status"][last] == OK else 0) if count else 0
    cap = (total + 3) & ~3 if count == 1 else total
    out = torch.zeros(cap + 64, dtype=torch.uint8, device=d.device)
    status = torch.full((count,), 0x55555555, dtype=torch.int32, device=d.device)
    need = engine.lib.hdlz_zip64_inflate_work_bytes(count, in_len, cap)
    rec = engine._record("hdlz_zip64_inflate_ws", _lib.ZipInflateResult, engine._scratch(need, None), d.data_ptr(), d.numel(), zi.entries.data_ptr(),
                         first, count, in_len, out.data_ptr(), cap, status.data_ptr())
    assert bool((out[cap:] == 0).all()), "bytes at or behind out_cap were written"
    out_off = zi.entries[first:first + count, 2] - (zi.entries[first, 2] if count else 0)
    return out[:total], out_off, status, rec
