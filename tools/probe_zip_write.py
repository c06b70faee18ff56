#!/usr/bin/env python
"""Evidence for hdlz_zip_write_ws (include/hdlz_zip_write.h) -> profiles/zip_write.txt, one sub-command per part; each replaces its own
section of --out and leaves the others.  HIP events around each call, the calls of a part in turn within a repeat, median of --repeats
after --warmup; a call's spread is max - min over its repeats.

  (section 1, no GPU: python tools/probe_unjoin.py codeobj --parent <csrc/_obj of a build of the parent commit> --sources <every source
   of build.sh but hdlz_zip_write and hdlz_api> --out profiles/zip_write.txt -- the resource lines of every existing kernel)
  gather                   section 2: hdlz_zip_write_ws against hdlz_join_gzip_ws on the SAME rows: one entry of 1 GiB of text at 64 KiB
                           blocks, and 2^20 x 2 KiB (2 GiB) as 4096 entries; allowed excess: the larger spread of the two calls plus one launch
                           boundary (5 us) per launch the writer makes beyond the gzip join's
  stored                   section 3, no bar: one entry of 1 GiB of random bytes without blocks against torch's device copy of the same bytes
  many                     section 4, no bar: 65535 entries of 64 bytes, the whole call with and without d_entries, and the same
                           entries without blocks
  crc                      section 5: one entry of 64 KiB .. 64 MiB through hdlz_crc32_batch_ws and through hdlz_crc32_ws: where
                           Engine.ZIP_CRC_TILED_MIN belongs
  ab --parent LIB          section 6: hdlz_join_gzip_ws and hdlz_zip_inflate_ws of this build against the parent commit's library"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from probe_unjoin import put_section      # noqa: E402
from probe_gunzip import LAUNCH_US, line, stat, text, timed      # noqa: E402

EXTRA_LAUNCHES = 1      # the writer: zero, scan, plan, gather; the gzip join: zero, k_join, finish


def _bind(path):
    from hdl_deflate_amd import _lib
    L = ctypes.CDLL(path)
    for t in (_lib.SIGNATURES, _lib.JOIN_SIGNATURES, _lib.GZIP_SIGNATURES, _lib.BGZF_SIGNATURES, _lib.ZIP_SIGNATURES):
        for name, (restype, argtypes) in t.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
    return L


class Writer(object):
    """one batch on the device (Engine._zip_batch) and the buffers of hdlz_zip_write_ws over it"""

    def __init__(self, eng, d_in, lens, names, block, store=None):
        import torch
        from hdl_deflate_amd import _lib
        self.eng, self.L, self.block = eng, eng.lib, block
        self.z = z = eng._zip_batch(d_in, lens, names, block, 32, 10, store)
        self.cap = self.L.hdlz_zip_write_bound(z.E, z.B, block, z.total, z.names.numel())
        self.out = torch.empty(self.cap, dtype=torch.uint8, device="cuda")
        self.res = torch.zeros(5 + 6 * z.E, dtype=torch.int64, device="cuda")
        self.wb = self.L.hdlz_zip_write_work_bytes(z.E, z.B)
        self.work = torch.empty(self.wb, dtype=torch.uint8, device="cuda")
        self.st = torch.cuda.current_stream().cuda_stream
        self.Result = _lib.ZipWriteResult

    def call(self, entries=True):
        z, p = self.z, (lambda t: t.data_ptr() if self.z.B else None)
        return lambda: self.L.hdlz_zip_write_ws(z.d_in.data_ptr(), z.ent_off.data_ptr(), z.names.data_ptr(), z.name_off.data_ptr(), z.E, p(z.in_off),
                                                p(z.rows), z.pitch, p(z.len), p(z.end_bits), p(z.status), z.B, z.blk_first.data_ptr(), z.crc.data_ptr(),
                                                z.flags, 0x210000, 16, z.total, self.out.data_ptr(), self.cap, self.res[5:].data_ptr() if entries else None,
                                                self.res.data_ptr(), self.work.data_ptr(), self.wb, self.st)

    def record(self):
        import torch
        torch.cuda.synchronize()
        return self.Result.from_buffer_copy(self.res[:5].cpu().numpy().tobytes())

    def verify(self, data_of):
        """the first and the last entry read back through the index the writer left: a stored one compared in place, a deflated one of
        up to 16 MiB read by Engine.inflate_zip (a larger one is the caller's to check) -> the record, the records on the host"""
        import torch
        from hdl_deflate_amd import _lib
        from hdl_deflate_amd.zip import ZipIndex, ENTRY_DTYPE
        rec = self.record()
        assert rec.status == 0, rec.status
        host = np.frombuffer(self.res[5:].cpu().numpy().tobytes(), dtype=ENTRY_DTYPE)
        zi = ZipIndex(self.res[5:].view(self.z.E, 6), _lib.ZipIndexResult(self.z.E, 0, rec.cd_off, rec.cd_size, 0, 0), host, [""] * self.z.E, 16)
        for e in sorted({0, self.z.E - 1}):
            want, h = data_of(e), host[e]
            assert int(h["status"]) == 0 and int(h["usize"]) == want.numel()
            if h["method"] == 0:
                assert torch.equal(self.out[int(h["payload_off"]):int(h["payload_off"]) + want.numel()], want), e
            elif want.numel() <= 16 << 20:
                out, off, status = self.eng.inflate_zip(self.out[:rec.file_len], zi, first=e, count=1)
                assert int(status[0]) == 0 and torch.equal(out[:want.numel()], want), e
        return rec, host


def gzip_join(eng, w):
    """hdlz_join_gzip_ws over the rows of a Writer's batch (all of them one stream)"""
    import torch
    L, z = eng.lib, w.z
    cap = L.hdlz_join_gzip_bound(z.B, w.block)
    out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    off = torch.empty(z.B + 1, dtype=torch.int64, device="cuda")
    res = torch.zeros(2, dtype=torch.int64, device="cuda")
    wb = L.hdlz_join_gzip_work_bytes(z.B)
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    crc = torch.zeros(1, dtype=torch.int32, device="cuda")
    keep = (out, off, res, work, crc)
    return keep, lambda: L.hdlz_join_gzip_ws(z.rows.data_ptr(), z.pitch, z.len.data_ptr(), z.end_bits.data_ptr(), z.status.data_ptr(), z.in_off.data_ptr(),
                                             w.block, z.B, crc.data_ptr(), out.data_ptr(), cap, off.data_ptr(), res.data_ptr(), work.data_ptr(), wb, w.st)


def cmd_gather(args):
    import torch
    from hdl_deflate_amd import Engine, _lib
    from hdl_deflate_amd.data import make_blocks
    eng = Engine()
    lines = ["command: python tools/probe_zip_write.py gather --repeats %d" % args.repeats,
             "both calls on the same rows of one hdlz_compress_batch_bits; bar: median(zip) - median(gzip join) <= max(spread) + %d x %.0f us" % (EXTRA_LAUNCHES, LAUNCH_US),
             "(the writer makes %d launch more than the gzip join: zero, scan, plan, gather against zero, k_join, finish)" % EXTRA_LAUNCHES, ""]
    bad = 0
    for what, total, E, block in (("one entry of %d GiB at 64 KiB blocks" % args.gib, args.gib << 30, 1, 1 << 16),
                                  ("%d x 2 KiB as 4096 entries" % (args.gib << 20), args.gib << 31, 4096, 2048)):
        d = make_blocks(total >> 11, 2048, "cuda", seed=7, families=(1, 2)).reshape(-1)
        w = Writer(eng, d, [total // E] * E, ["e%04d" % k for k in range(E)], block)
        keep, gz = gzip_join(eng, w)
        t = timed([("zip", w.call()), ("gzip", gz)], args.repeats, args.warmup)
        per = total // E
        rec, host = w.verify(lambda e: d[e * per:(e + 1) * per])
        g = _lib.JoinGzipResult.from_buffer_copy(keep[2].cpu().numpy().tobytes())
        assert g.status == 0 and rec.nstored == 0
        if E == 1:                                              # the same members: the entry's payload is the gzip stream's, 03 00 included
            p0, c = int(host[0]["payload_off"]), int(host[0]["csize"])
            assert c + 18 == g.stream_len and torch.equal(w.out[p0:p0 + c], keep[0][10:10 + c])
        (mz, sz), (mg, sg) = stat(t["zip"]), stat(t["gzip"])
        allowed = max(sz, sg) + EXTRA_LAUNCHES * LAUNCH_US
        held = mz - mg <= allowed
        bad += not held
        lines += ["%s (%d rows; the file %d bytes, the gzip stream %d):" % (what, w.z.B, rec.file_len, g.stream_len),
                  line("hdlz_zip_write_ws", t["zip"], "   %.0f GB/s of file" % (rec.file_len / mz / 1e3)),
                  line("hdlz_join_gzip_ws", t["gzip"], "   %.0f GB/s of stream" % (g.stream_len / mg / 1e3)),
                  "  zip - gzip join = %+.1f us, allowed %.1f us: %s" % (mz - mg, allowed, "held" if held else "MISSED"), ""]
        del w, keep, gz, d
        torch.cuda.empty_cache()
    put_section(args.out, "2. the gather against the gzip join on the same rows", lines)
    return 1 if bad else 0


def cmd_stored(args):
    import torch
    from hdl_deflate_amd import Engine
    eng = Engine()
    n = args.gib << 30
    src = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    w = Writer(eng, src, [n], ["stored.bin"], 1 << 16, store=[True])

    def copy():
        dst.copy_(src)
        return 0
    t = timed([("zip", w.call()), ("copy", copy)], args.repeats, args.warmup)
    rec, _ = w.verify(lambda e: src)
    assert rec.nstored == 1 and w.z.B == 0
    mz, mc = stat(t["zip"])[0], stat(t["copy"])[0]
    lines = ["command: python tools/probe_zip_write.py stored --repeats %d" % args.repeats,
             "one entry of %d GiB of random bytes without blocks -- the plan, the tiles of 64 KiB, the headers -- against a device copy of the same bytes; no bar" % args.gib, "",
             line("hdlz_zip_write_ws, one stored entry", t["zip"], "   %.0f GB/s of payload" % (n / mz / 1e3)),
             line("torch copy_ of the same bytes", t["copy"], "   %.0f GB/s (read + write: twice that)" % (n / mc / 1e3)), ""]
    put_section(args.out, "3. the stored copy against a device copy", lines)
    return 0


def cmd_many(args):
    import torch
    from hdl_deflate_amd import Engine
    eng = Engine()
    E, n = 65535, 64
    data = torch.from_numpy(np.frombuffer(text(E * n, 3), np.uint8).copy()).cuda()
    names = ["dir/entry%05d.txt" % k for k in range(E)]
    lines = ["command: python tools/probe_zip_write.py many --repeats %d" % args.repeats,
             "65535 entries of 64 bytes; the headers, the names and d_entries are written by the gather's launch (a wave per entry); no bar", ""]
    for what, store in (("a block per entry", None), ("no blocks (store=)", [True] * E)):
        w = Writer(eng, data, [n] * E, names, 64, store=store)
        t = timed([("with", w.call(True)), ("without", w.call(False))], args.repeats, args.warmup)
        w.call(True)()
        rec, _ = w.verify(lambda e: data[e * n:(e + 1) * n])
        lines += ["%s (%d rows, %d entries stored, the file %d bytes):" % (what, w.z.B, rec.nstored, rec.file_len),
                  line("hdlz_zip_write_ws with d_entries", t["with"], "   %.3f us an entry" % (stat(t["with"])[0] / E)),
                  line("hdlz_zip_write_ws without d_entries", t["without"]), ""]
        del w
    put_section(args.out, "4. 65535 entries of 64 bytes", lines)
    return 0


def cmd_crc(args):
    import torch
    from hdl_deflate_amd import Engine
    eng = Engine()
    L = eng.lib
    st = torch.cuda.current_stream().cuda_stream
    lines = ["command: python tools/probe_zip_write.py crc --repeats %d" % args.repeats,
             "one entry: (a) hdlz_crc32_batch_ws, a workgroup per entry; (b) hdlz_crc32_ws, the 32 KiB tiles and the finishing workgroup", ""]
    buf = torch.randint(0, 256, ((64 << 20) + 64,), dtype=torch.uint8, device="cuda")
    crc = torch.zeros(2, dtype=torch.int32, device="cuda")
    cross = None
    n = 64 << 10
    while n <= 64 << 20:
        off = torch.tensor([0, n], dtype=torch.int64, device="cuda")
        wb = L.hdlz_crc32_work_bytes(n)
        work = torch.empty(wb, dtype=torch.uint8, device="cuda")
        t = timed([("batch", lambda: L.hdlz_crc32_batch_ws(buf.data_ptr(), off.data_ptr(), 0, 0, 1, crc.data_ptr(), st)),
                   ("tiled", lambda: L.hdlz_crc32_ws(buf.data_ptr(), n, crc[1:].data_ptr(), work.data_ptr(), wb, st))], args.repeats, args.warmup)
        c = crc.cpu().numpy()
        assert c[0] == c[1]
        mb, mt = stat(t["batch"])[0], stat(t["tiled"])[0]
        if mt < mb and cross is None:
            cross = n
        if mt >= mb:
            cross = None                                        # (the smallest size FROM WHICH the tiled call is the faster one)
        lines += ["%6d KiB:  batch %10.1f us (spread %7.1f)   tiled %8.1f us (spread %6.1f)   tiled / batch = %.3f" %
                  (n >> 10, mb, stat(t["batch"])[1], mt, stat(t["tiled"])[1], mt / mb)]
        n *= 2
    lines += ["", "the tiled call is the faster one from %s on: Engine.ZIP_CRC_TILED_MIN" % ("%d KiB" % (cross >> 10) if cross else "no size measured"), ""]
    put_section(args.out, "5. ZIP_CRC_TILED_MIN: one entry through hdlz_crc32_batch_ws and through hdlz_crc32_ws", lines)
    return 0


def cmd_ab(args):
    import torch
    from hdl_deflate_amd import _lib, Engine
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import zip_ref as Z
    L, Pa = _lib.load(), _bind(args.parent)
    eng = Engine()
    lines = ["command: python tools/probe_zip_write.py ab --parent <libhdlz.so of a build of the parent commit> --repeats %d" % args.repeats,
             "within a repeat: parent, this build, parent again; the bar: |this build - the parent's mean median| <= the larger of the",
             "difference of the parent's two medians and the parent's larger spread", ""]
    bad = 0
    from hdl_deflate_amd.data import make_blocks
    d = make_blocks(1 << 15, 2048, "cuda", seed=9, families=(1, 2)).reshape(-1)          # 64 MiB at 64 KiB blocks
    w = Writer(eng, d, [d.numel()], ["e"], 1 << 16)
    keep, _ = gzip_join(eng, w)
    out, off, res, work, crc = keep
    z, st = w.z, w.st

    def join(lib):
        return lib.hdlz_join_gzip_ws(z.rows.data_ptr(), z.pitch, z.len.data_ptr(), z.end_bits.data_ptr(), z.status.data_ptr(), z.in_off.data_ptr(), w.block,
                                     z.B, crc.data_ptr(), out.data_ptr(), out.numel(), off.data_ptr(), res.data_ptr(), work.data_ptr(), work.numel(), st)
    datas = [text(57344, 300 + k) for k in range(64)]
    f = Z.make_zip([dict(name=b"%04d" % k, data=datas[k % 64]) for k in range(1024)])
    df = torch.frombuffer(bytearray(f + bytes(64)), dtype=torch.uint8).cuda()[:len(f)]
    zi = eng.zip_index(df)
    total = int(zi.record.total_out)
    zout = torch.empty(total, dtype=torch.uint8, device="cuda")
    zst = torch.zeros(1024, dtype=torch.int32, device="cuda")
    zres = torch.zeros(3, dtype=torch.int64, device="cuda")
    zwb = L.hdlz_zip_inflate_work_bytes(1024, 0, total)
    zwork = torch.empty(zwb, dtype=torch.uint8, device="cuda")

    def read(lib):
        return lib.hdlz_zip_inflate_ws(df.data_ptr(), len(f), zi.entries.data_ptr(), 0, 1024, 0, zout.data_ptr(), total, zst.data_ptr(), zres.data_ptr(),
                                       zwork.data_ptr(), zwb, st)
    for what, call in (("hdlz_join_gzip_ws, 64 MiB in %d rows" % z.B, join), ("hdlz_zip_inflate_ws, 1024 entries of 56 KiB", read)):
        t = timed([("p1", lambda: call(Pa)), ("new", lambda: call(L)), ("p2", lambda: call(Pa))], args.repeats, args.warmup)
        (m1, s1), (mn, sn), (m2, s2) = stat(t["p1"]), stat(t["new"]), stat(t["p2"])
        allowed = max(abs(m1 - m2), s1, s2)
        held = abs(mn - (m1 + m2) / 2) <= allowed
        bad += not held
        lines += [what + ":", line("parent, first in the repeat", t["p1"]), line("this build", t["new"]), line("parent, last in the repeat", t["p2"]),
                  "  this build - parent %+.1f us, allowed %.1f us: %s" % (mn - (m1 + m2) / 2, allowed, "held" if held else "MISSED"), ""]
    assert int((zst != 0).sum()) == 0 and zout[:57344].cpu().numpy().tobytes() == datas[0]
    put_section(args.out, "6. existing calls against the parent commit's library", lines)
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("cmd", choices=("gather", "stored", "many", "crc", "ab"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zip_write.txt"))
    ap.add_argument("--parent", help="ab: the parent commit's libhdlz.so")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gib", type=int, default=1, help="gather, stored: the bytes of the shape, in GiB")
    args = ap.parse_args()
    return {"gather": cmd_gather, "stored": cmd_stored, "many": cmd_many, "crc": cmd_crc, "ab": cmd_ab}[args.cmd](args)


if __name__ == "__main__":
    sys.exit(main())
