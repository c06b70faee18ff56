#!/usr/bin/env python
"""Evidence for hdlz_zip64_index_ws / hdlz_zip64_inflate_ws / hdlz_zip64_write_ws (include/hdlz_zip64.h) -> profiles/zip64.txt, one sub-command per part; each
replaces its own section of --out and leaves the others.  HIP events around each call, the calls of a part in turn within a repeat,
median of --repeats (at least 10) after --warmup; a call's spread is max - min over its repeats (tools/probe_gunzip.py's timed).

  index     section 1: hdlz_zip64_index_ws against hdlz_zip_index_ws of the same library on the two files of profiles/zip.txt section 2
            (1000 and 65535 entries).  bar: median(new) - median(classic) <= max(10 % of the classic median, 3 x the classic spread)
  many      section 2, no bar: the index of 131073 and 1048576 entries, and the slope over 65535 entries
  big       section 3, no bar: one stored entry of 2^32 + 5 bytes read by hdlz_zip64_inflate_ws (count == 1: the flat copy and the tile
            CRC), next to torch's device copy of the same bytes
  write     section 5: hdlz_zip64_write_ws at zip64_from = FFFFFFFF against hdlz_zip_write_ws of the same library on the shapes of
            profiles/zip_write.txt (one entry at 64 KiB blocks, 4096 entries of 2 KiB blocks, one stored entry, 65535 entries of 64 bytes),
            in turn; bar: as in section 1.  Then, no bar: the issue's files past 4 GiB written -- (a) two stored entries of 2^31 + 4096
            bytes and four small ones, (b) one stored entry of 2^32 + 5 bytes
  ab --parent LIB    section 4: hdlz_zip_index_ws and hdlz_zip_inflate_ws of this build -- its read kernels are now instances of the templates
            both record types share -- against the parent commit's library, in turn.  bar: as in section 1"""
import argparse
import os
import struct
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from probe_unjoin import put_section      # noqa: E402
from probe_gunzip import line, stat, text, timed      # noqa: E402
from probe_zip import _bind, deflate, make_zip      # noqa: E402


def index_calls(eng, d, n, zip64):
    """-> the call over the file on the device, entry_cap = nentries = n, out_align 16 (buffers kept alive by the closure)"""
    import torch
    L = eng.lib
    words, fn, wbf = (8, L.hdlz_zip64_index_ws, L.hdlz_zip64_index_work_bytes) if zip64 else (6, L.hdlz_zip_index_ws, L.hdlz_zip_index_work_bytes)
    ent = torch.empty((n, words), dtype=torch.int64, device="cuda")
    wb = wbf(d.numel(), n)
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    res = torch.zeros(8, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    return (lambda: fn(d.data_ptr(), d.numel(), n, 16, ent.data_ptr(), res.data_ptr(), work.data_ptr(), wb, st)), res, ent


def stage(z):
    import torch
    return torch.frombuffer(bytearray(z + bytes(64)), dtype=torch.uint8).cuda()[:len(z)]


def cmd_index(args):
    import torch
    from hdl_deflate_amd import Engine
    eng = Engine()
    lines = ["command: python tools/probe_zip64.py index --repeats %d" % args.repeats,
             "(a) hdlz_zip_index_ws, (b) hdlz_zip64_index_ws, the same library, the same file (no locator), entry_cap = nentries, in turn",
             "bar: median(b) - median(a) <= max(0.10 median(a), 3 spread(a))", ""]
    bad = 0
    for n, size in ((1000, 4096), (65535, 64)):
        datas = [text(size, 200 + k % 16) for k in range(n)]
        raws = {k: deflate(datas[k]) for k in range(16)}
        z = make_zip([(b"dir/entry%05d.txt" % k, datas[k], 8, raws[k % 16]) for k in range(n)])
        d = stage(z)
        (a, ra, ea), (b, rb, eb) = index_calls(eng, d, n, False), index_calls(eng, d, n, True)
        t = timed([("classic", a), ("zip64", b)], args.repeats, args.warmup)
        torch.cuda.synchronize()
        assert torch.equal(ra[:5], rb[:5]) and int(ra[4]) == 0 and torch.equal(ea[:, :3], eb[:, :3])      # the same result, the same offsets
        (ma, sa), (mb, _) = stat(t["classic"]), stat(t["zip64"])
        allowed = max(0.10 * ma, 3.0 * sa)
        ok = mb - ma <= allowed
        bad += not ok
        lines += ["%d entries of %d bytes, a file of %d bytes:" % (n, size, len(z)), line("(a) hdlz_zip_index_ws", t["classic"]),
                  line("(b) hdlz_zip64_index_ws", t["zip64"]),
                  "  b - a = %.1f us (%.1f %%), allowed %.1f us: %s" % (mb - ma, 100.0 * (mb - ma) / ma, allowed, "PASS" if ok else "FAIL"), ""]
    put_section(args.out, "1. hdlz_zip64_index_ws against hdlz_zip_index_ws on classic files", lines)
    return bad


def many_zip(n):
    """n empty stored entries with seven-digit names, ZIP64 end record and locator, classic values all ones"""
    body, cd = bytearray(), bytearray()
    for k in range(n):
        name = b"%07d" % k
        off = len(body)
        body += b"PK\x03\x04" + struct.pack("<HHHHHIIIHH", 20, 0, 0, 0, 0x21, 0, 0, 0, len(name), 0) + name
        cd += b"PK\x01\x02" + struct.pack("<HHHHHHIIIHHHHHII", 20, 20, 0, 0, 0, 0x21, 0, 0, 0, len(name), 0, 0, 0, 0, 0, off) + name
    end = b"PK\x06\x06" + struct.pack("<QHHIIQQQQ", 44, 45, 45, 0, 0, n, n, len(cd), len(body)) + b"PK\x06\x07" + struct.pack("<IQI", 0, len(body) + len(cd), 1)
    return bytes(body + cd + end + b"PK\x05\x06" + struct.pack("<HHHHIIH", 0xFFFF, 0xFFFF, 0xFFFF, 0xFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0))


def cmd_many(args):
    import torch
    from hdl_deflate_amd import Engine
    eng = Engine()
    lines = ["command: python tools/probe_zip64.py many --repeats %d" % args.repeats,
             "hdlz_zip64_index_ws, entry_cap = nentries, empty stored entries with 7-byte names (a central record of 53 bytes); no bar", ""]
    med = {}
    for n in (65535, 131073, 1048576):
        d = stage(many_zip(n))
        call, res, ent = index_calls(eng, d, n, True)
        t = timed([("index", call)], args.repeats, args.warmup)
        torch.cuda.synchronize()
        assert int(res[0]) == n and int(res[4]) == 0 and int(ent[n - 1, 0]) == int(res[2]) + 53 * (n - 1)
        med[n] = stat(t["index"])[0]
        lines += [line("%d entries, a file of %d bytes" % (n, d.numel()), t["index"], "   %.3f us an entry" % (med[n] / n))]
    lines += ["", "  slope: %.3f us an entry from 65535 to 131073, %.3f us an entry from 131073 to 1048576" %
              ((med[131073] - med[65535]) / (131073 - 65535), (med[1048576] - med[131073]) / (1048576 - 131073)), ""]
    put_section(args.out, "2. many entries: the serial walk's slope", lines)
    return 0


def cmd_big(args):
    import torch
    from hdl_deflate_amd import Engine
    eng = Engine()
    L = eng.lib
    n = (1 << 32) + 5
    big = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    crc = int(eng.crc32(big).cpu()[0])
    x = struct.pack("<HHQQ", 1, 16, n, n)
    head = b"PK\x03\x04" + struct.pack("<HHHHHIIIHH", 45, 0, 0, 0, 0x21, crc, 0xFFFFFFFF, 0xFFFFFFFF, 7, 20) + b"big.bin" + x
    cd = b"PK\x01\x02" + struct.pack("<HHHHHHIIIHHHHHII", 45, 45, 0, 0, 0, 0x21, crc, 0xFFFFFFFF, 0xFFFFFFFF, 7, 20, 0, 0, 0, 0, 0) + b"big.bin" + x
    cd_off = len(head) + n
    tail = cd + b"PK\x06\x06" + struct.pack("<QHHIIQQQQ", 44, 45, 45, 0, 0, 1, 1, len(cd), cd_off) + b"PK\x06\x07" + struct.pack("<IQI", 0, cd_off + len(cd), 1) + \
        b"PK\x05\x06" + struct.pack("<HHHHIIH", 0, 0, 1, 1, len(cd), 0xFFFFFFFF, 0)
    d = torch.empty(len(head) + n + len(tail), dtype=torch.uint8, device="cuda")
    d[:len(head)] = torch.frombuffer(bytearray(head), dtype=torch.uint8).cuda()
    d[len(head):len(head) + n] = big
    d[len(head) + n:] = torch.frombuffer(bytearray(tail), dtype=torch.uint8).cuda()
    zi = eng.zip_index(d, out_align=16)
    assert zi.zip64 and zi.record.status == 0 and int(zi.host["usize"][0]) == n
    cap = (n + 3) & ~3
    out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    res = torch.zeros(3, dtype=torch.int64, device="cuda")
    wb = L.hdlz_zip64_inflate_work_bytes(1, 0, cap)
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    dst = torch.empty(n, dtype=torch.uint8, device="cuda")

    def copy():
        dst.copy_(big)
        return 0

    calls = [("read", lambda: L.hdlz_zip64_inflate_ws(d.data_ptr(), d.numel(), zi.entries.data_ptr(), 0, 1, 0, out.data_ptr(), cap, status.data_ptr(),
                                                      res.data_ptr(), work.data_ptr(), wb, st)), ("copy", copy)]
    t = timed(calls, args.repeats, args.warmup)
    torch.cuda.synchronize()
    assert int(status[0]) == 0 and int(res[0]) == n and torch.equal(out[:n], big)
    mr, mc = stat(t["read"])[0], stat(t["copy"])[0]
    lines = ["command: python tools/probe_zip64.py big --repeats %d" % args.repeats,
             "one stored entry of 2^32 + 5 random bytes in a file of %d bytes; no bar" % d.numel(), "",
             line("hdlz_zip64_inflate_ws, count == 1 (copy + CRC-32 + verdict)", t["read"], "   %.0f GB/s of payload" % (n / mr / 1e3)),
             line("torch: dst.copy_(src) of the same bytes", t["copy"], "   %.0f GB/s" % (n / mc / 1e3)), ""]
    put_section(args.out, "3. one stored entry past 4 GiB", lines)
    return 0


def cmd_ab(args):
    import torch
    from hdl_deflate_amd import Engine
    eng = Engine()
    P = _bind(args.parent)
    st = torch.cuda.current_stream().cuda_stream
    lines = ["command: python tools/probe_zip64.py ab --parent <libhdlz.so of the parent commit> --repeats %d" % args.repeats,
             "(a) the parent's library, (b) this build, the same buffers, in turn; bar: median(b) - median(a) <= max(0.10 median(a), 3 spread(a))", ""]
    bad = 0
    big = text(16 << 20, 7)
    files = [("1000 entries of 4096 bytes", [(b"dir/entry%05d.txt" % k, text(4096, 200 + k % 16), 8, None) for k in range(1000)], (0, 1000, 0)),
             ("one 16 MiB level-6 entry", [(b"big.txt", big, 8, None)], (0, 1, None)), ("one 16 MiB stored entry", [(b"big.bin", big, 0, None)], (0, 1, None))]
    for label, items, (first, count, in_len) in files:
        raws = {}
        items = [(nm, dt, m, raws.setdefault(dt, deflate(dt)) if m else None) for nm, dt, m, _ in items]
        d = stage(make_zip(items))
        zi = eng.zip_index(d, out_align=16, zip64=False)
        n = len(zi)
        assert zi.record.status == 0 and not zi.zip64
        h = zi.host
        il = int(h["csize"][0]) + 6 if in_len is None else in_len
        total = int(h["out_off"][n - 1] + h["usize"][n - 1])
        cap = (total + 3) & ~3
        out, status, res = torch.zeros(cap, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(8, dtype=torch.int64, device="cuda")
        ent = torch.empty((n, 6), dtype=torch.int64, device="cuda")
        wb, wi = eng.lib.hdlz_zip_inflate_work_bytes(count, il, cap), eng.lib.hdlz_zip_index_work_bytes(d.numel(), n)
        assert wb == P.hdlz_zip_inflate_work_bytes(count, il, cap)
        work = torch.empty(max(wb, wi), dtype=torch.uint8, device="cuda")
        for what, mk in (("hdlz_zip_inflate_ws", lambda L: (lambda: L.hdlz_zip_inflate_ws(d.data_ptr(), d.numel(), zi.entries.data_ptr(), first, count, il, out.data_ptr(),
                                                                                          cap, status.data_ptr(), res.data_ptr(), work.data_ptr(), wb, st))),
                         ("hdlz_zip_index_ws", lambda L: (lambda: L.hdlz_zip_index_ws(d.data_ptr(), d.numel(), n, 16, ent.data_ptr(), res[4:].data_ptr(), work.data_ptr(),
                                                                                      wi, st)))):
            if what == "hdlz_zip_index_ws" and n == 1:
                continue
            t = timed([("parent", mk(P)), ("this", mk(eng.lib))], args.repeats, args.warmup)
            torch.cuda.synchronize()
            assert int((status != 0).sum()) == 0 and (what != "hdlz_zip_index_ws" or torch.equal(ent, zi.entries))
            (ma, sa), (mb, _) = stat(t["parent"]), stat(t["this"])
            allowed = max(0.10 * ma, 3.0 * sa)
            ok = mb - ma <= allowed
            bad += not ok
            lines += ["%s, %s:" % (label, what), line("(a) parent", t["parent"]), line("(b) this build", t["this"]),
                      "  b - a = %.1f us (%.1f %%), allowed %.1f us: %s" % (mb - ma, 100.0 * (mb - ma) / ma, allowed, "PASS" if ok else "FAIL"), ""]
    put_section(args.out, "4. the classic calls against the parent commit's library", lines)
    return bad


class Writer64(object):
    """probe_zip_write.Writer's batch through hdlz_zip64_write_ws: buffers of its own, the same inputs"""

    def __init__(self, w, zip64_from):
        import torch
        z, L = w.z, w.L
        self.w, self.zip64_from = w, zip64_from
        self.cap = L.hdlz_zip64_write_bound(z.E, z.B, w.block, z.total, z.names.numel())
        self.out = torch.empty(self.cap, dtype=torch.uint8, device="cuda")
        self.res = torch.zeros(5 + 8 * z.E, dtype=torch.int64, device="cuda")
        self.wb = L.hdlz_zip64_write_work_bytes(z.E, z.B)
        self.work = torch.empty(self.wb, dtype=torch.uint8, device="cuda")

    def call(self):
        w, z, p = self.w, self.w.z, (lambda t: t.data_ptr() if self.w.z.B else None)
        return lambda: w.L.hdlz_zip64_write_ws(z.d_in.data_ptr(), z.ent_off.data_ptr(), z.names.data_ptr(), z.name_off.data_ptr(), z.E, p(z.in_off),
                                               p(z.rows), z.pitch, p(z.len), p(z.end_bits), p(z.status), z.B, z.blk_first.data_ptr(), z.crc.data_ptr(),
                                               z.flags, 0x210000, 16, self.zip64_from, z.total, self.out.data_ptr(), self.cap, self.res[5:].data_ptr(),
                                               self.res.data_ptr(), self.work.data_ptr(), self.wb, w.st)

    def record(self):
        import torch
        torch.cuda.synchronize()
        return self.w.Result.from_buffer_copy(self.res[:5].cpu().numpy().tobytes())


def cmd_write(args):
    import numpy as np
    import torch
    from hdl_deflate_amd import Engine
    from hdl_deflate_amd.data import make_blocks
    from probe_zip_write import Writer
    eng = Engine()
    lines = ["command: python tools/probe_zip64.py write --repeats %d" % args.repeats,
             "(a) hdlz_zip_write_ws, (b) hdlz_zip64_write_ws at zip64_from = FFFFFFFF, the same library, the same batch, in turn; the files are equal",
             "bar: median(b) - median(a) <= max(0.10 median(a), 3 spread(a))", ""]
    bad = 0
    gib = 1 << 30
    small = torch.from_numpy(np.frombuffer(text(65535 * 64, 3), np.uint8).copy()).cuda()
    shapes = [("one entry of 1 GiB at 64 KiB blocks", lambda: make_blocks(gib >> 11, 2048, "cuda", seed=7, families=(1, 2)).reshape(-1), 1, 1 << 16, None),
              ("1 GiB as 4096 entries at 2 KiB blocks", lambda: make_blocks(gib >> 11, 2048, "cuda", seed=7, families=(1, 2)).reshape(-1), 4096, 2048, None),
              ("one stored entry of 1 GiB", lambda: torch.randint(0, 256, (gib,), dtype=torch.uint8, device="cuda"), 1, 1 << 16, True),
              ("65535 entries of 64 bytes, a block each", lambda: small, 65535, 64, None),
              ("65535 entries of 64 bytes, no blocks", lambda: small, 65535, 64, True)]
    for what, make, E, block, store in shapes:
        d = make()
        w = Writer(eng, d, [d.numel() // E] * E, ["dir/entry%05d.txt" % k for k in range(E)], block, store=[True] * E if store else None)
        w64 = Writer64(w, 0xFFFFFFFF)
        t = timed([("classic", w.call()), ("zip64", w64.call())], args.repeats, args.warmup)
        ra, rb = w.record(), w64.record()
        assert ra.status == rb.status == 0 and bytes(ra) == bytes(rb) and torch.equal(w.out[:ra.file_len], w64.out[:rb.file_len])
        (ma, sa), (mb, sb) = stat(t["classic"]), stat(t["zip64"])
        allowed = max(0.10 * ma, 3 * sa)
        held = mb - ma <= allowed
        bad += not held
        lines += ["%s (%d rows, the file %d bytes):" % (what, w.z.B, ra.file_len), line("hdlz_zip_write_ws", t["classic"]), line("hdlz_zip64_write_ws", t["zip64"]),
                  "  zip64 - classic = %+.1f us, allowed %.1f us: %s" % (mb - ma, allowed, "held" if held else "MISSED"), ""]
        del w, w64, d
        torch.cuda.empty_cache()
    lines += ["the files past 4 GiB, written (hdlz_zip64_write_ws alone, zip64_from = FFFFFFFF; no bar):", ""]
    n = (1 << 31) + 4096
    for what, lens, store in (("(a) two stored entries of 2^31 + 4096 bytes, four small ones", [n, n, 3000, 500, 70000, 3], [True, True, False, True, False, True]),
                              ("(b) one stored entry of 2^32 + 5 bytes", [(1 << 32) + 5], [True])):
        d = torch.randint(0, 256, (sum(lens),), dtype=torch.uint8, device="cuda")
        if len(lens) > 1:
            d[2 * n:] = torch.from_numpy(np.frombuffer(text(sum(lens[2:]), 5), np.uint8).copy()).cuda()
        w = Writer(eng, d, lens, ["e%d" % k for k in range(len(lens))], 1 << 16, store=store)
        w64 = Writer64(w, 0xFFFFFFFF)
        t = timed([("zip64", w64.call())], max(5, args.repeats // 4), 2)
        r = w64.record()
        assert r.status == 0 and r.file_len > 1 << 32
        lines += ["%s (the file %d bytes):" % (what, r.file_len), line("hdlz_zip64_write_ws", t["zip64"], "   %.0f GB/s of file" % (r.file_len / stat(t["zip64"])[0] / 1e3)), ""]
        del w, w64, d
        torch.cuda.empty_cache()
    put_section(args.out, "5. hdlz_zip64_write_ws against hdlz_zip_write_ws, and the files past 4 GiB written", lines)
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("cmd", choices=("index", "many", "big", "ab", "write"))
    ap.add_argument("--parent", help="ab: the parent commit's libhdlz.so")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zip64.txt"))
    args = ap.parse_args()
    assert args.repeats >= 10
    return {"index": cmd_index, "many": cmd_many, "big": cmd_big, "ab": cmd_ab, "write": cmd_write}[args.cmd](args)


if __name__ == "__main__":
    sys.exit(main())
