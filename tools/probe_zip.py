#!/usr/bin/env python
"""Evidence for hdlz_zip_index_ws / hdlz_zip_inflate_ws (include/hdlz_zip.h) -> profiles/zip.txt, one sub-command per part; each replaces
its own section of --out and leaves the others.  HIP events around each call, the calls of a part in turn within a repeat, median of
--repeats (at least 10) after --warmup; a call's spread is max - min over its repeats.

  (section 1, no GPU: python tools/probe_unjoin.py codeobj --parent <csrc/_obj of a build of the parent commit> --sources <every source
   of build.sh but hdlz_zip and hdlz_api> --out profiles/zip.txt -- the resource lines of every existing kernel)
  index                    section 2: hdlz_zip_index_ws on archives of 1000 and 65535 entries, next to the time to read the same file
                           (hdlz_zip_inflate_ws over all entries), and the ratio
  frame                    section 3: hdlz_zip_inflate_ws against hdlz_bgzf_inflate_ws on the same deflate payloads (4096 x 56 KiB), and
                           against hdlz_gunzip_ws for one 16 MiB level-6 payload; allowed excess: the larger same-build spread of the
                           two calls plus one launch boundary (5 us)
  crossover                section 4, no bar: one entry of 4 KiB .. 1 MiB on both routes (count == 1 with the bound stated; the same entry
                           as the first of a two-entry call): where HDLZ_ZIP_LARGE_MIN belongs
  stored                   section 5, no bar: the flat copy of one 64 MiB stored entry against torch's device copy of the same bytes
  ab --parent LIB          section 6: hdlz_gunzip_ws and hdlz_bgzf_inflate_ws of this build against the parent commit's library"""
import argparse
import ctypes
import os
import struct
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from probe_unjoin import put_section      # noqa: E402
from probe_gunzip import LAUNCH_US, line, stat, text, timed      # noqa: E402


def _bind(path):
    from hdl_deflate_amd import _lib
    L = ctypes.CDLL(path)
    for t in (_lib.SIGNATURES, _lib.GZIP_SIGNATURES, _lib.BGZF_SIGNATURES, _lib.GUNZIP_SIGNATURES, _lib.ZIP_SIGNATURES):
        for name, (restype, argtypes) in t.items():
            if hasattr(L, name):                            # (the parent has no hdlz_zip_*)
                fn = getattr(L, name)
                fn.restype, fn.argtypes = restype, argtypes
    return L


def make_zip(payloads):
    """[(name, data, method, raw deflate or None)] -> the file's bytes (tests/zip_ref.py's layout, the deflate given)"""
    body, cd = bytearray(), bytearray()
    for name, data, method, raw in payloads:
        raw = data if method == 0 else raw
        crc, off = zlib.crc32(data), len(body)
        body += b"PK\x03\x04" + struct.pack("<HHHHHIIIHH", 20, 0, method, 0, 0x21, crc, len(raw), len(data), len(name), 0) + name + raw
        cd += b"PK\x01\x02" + struct.pack("<HHHHHHIIIHHHHHII", 20, 20, 0, method, 0, 0x21, crc, len(raw), len(data), len(name), 0, 0, 0, 0, 0, off) + name
    return bytes(body + cd + b"PK\x05\x06" + struct.pack("<HHHHIIH", 0, 0, len(payloads), len(payloads), len(cd), len(body), 0))


def deflate(d, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(d) + c.flush()


class Zip(object):
    """an archive on the device with its index and the buffers of one hdlz_zip_inflate_ws over entries [first, first + count)"""

    def __init__(self, eng, z, out_align=16):
        import torch
        self.eng, self.L, self.n = eng, eng.lib, len(z)
        self.d = torch.frombuffer(bytearray(z + bytes(64)), dtype=torch.uint8).cuda()[:len(z)]
        self.zi = eng.zip_index(self.d, out_align=out_align)
        assert self.zi.record.status == 0
        self.st = torch.cuda.current_stream().cuda_stream
        self.res = torch.zeros(8, dtype=torch.int64, device="cuda")
        self.calls = {}

    def index_call(self):
        import torch
        cap = len(self.zi)
        ent = torch.empty((cap, 6), dtype=torch.int64, device="cuda")
        wb = self.L.hdlz_zip_index_work_bytes(self.n, cap)
        work = torch.empty(wb, dtype=torch.uint8, device="cuda")
        self.keep = (ent, work)
        return lambda: self.L.hdlz_zip_index_ws(self.d.data_ptr(), self.n, cap, 16, ent.data_ptr(), self.res.data_ptr(), work.data_ptr(), wb, self.st)

    def read_call(self, first, count, in_len):
        import torch
        h = self.zi.host
        last = first + count - 1
        total = int(h["out_off"][last] - h["out_off"][first] + h["usize"][last])
        cap = (total + 3) & ~3
        out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        status = torch.zeros(count, dtype=torch.int32, device="cuda")
        wb = self.L.hdlz_zip_inflate_work_bytes(count, in_len, cap)
        work = torch.empty(wb, dtype=torch.uint8, device="cuda")
        self.calls[(first, count)] = (out, status, work)
        return lambda: self.L.hdlz_zip_inflate_ws(self.d.data_ptr(), self.n, self.zi.entries.data_ptr(), first, count, in_len, out.data_ptr(), cap,
                                                  status.data_ptr(), self.res[5:].data_ptr(), work.data_ptr(), wb, self.st)

    def verify(self, first, count, datas):
        import torch
        torch.cuda.synchronize()
        out, status, _ = self.calls[(first, count)]
        assert int((status != 0).sum()) == 0, status
        h = self.zi.host
        for k, want in ((0, datas[0]), (count - 1, datas[-1])):      # datas: the first and the last entry's bytes
            o = int(h["out_off"][first + k] - h["out_off"][first])
            assert out[o:o + len(want)].cpu().numpy().tobytes() == want


def cmd_index(args):
    from hdl_deflate_amd import Engine
    eng = Engine()
    lines = ["command: python tools/probe_zip.py index --repeats %d" % args.repeats,
             "(a) hdlz_zip_index_ws, (b) hdlz_zip_inflate_ws over all entries of the same file in one call (count >= 2); no bar", ""]
    for n, size in ((1000, 4096), (65535, 64)):
        datas = [text(size, 200 + k % 16) for k in range(n)]
        raws = {k: deflate(datas[k]) for k in range(16)}
        z = make_zip([(b"dir/entry%05d.txt" % k, datas[k], 8, raws[k % 16]) for k in range(n)])
        a = Zip(eng, z)
        t = timed([("index", a.index_call()), ("read", a.read_call(0, n, 0))], args.repeats, args.warmup)
        a.verify(0, n, [datas[0], datas[n - 1]])
        mi, mr = stat(t["index"])[0], stat(t["read"])[0]
        lines += ["%d entries of %d bytes, a file of %d bytes, a directory of %d:" % (n, size, len(z), a.zi.record.cd_size),
                  line("(a) hdlz_zip_index_ws", t["index"]), line("(b) hdlz_zip_inflate_ws, all entries", t["read"]),
                  "  index / read = %.3f; %.3f us an entry" % (mi / mr, mi / n), ""]
        del a
    put_section(args.out, "2. the index next to the read of the same file", lines)
    return 0


def cmd_frame(args):
    import torch
    from hdl_deflate_amd import Engine, _lib
    eng = Engine()
    L = eng.lib
    st = torch.cuda.current_stream().cuda_stream
    lines = ["command: python tools/probe_zip.py frame --repeats %d" % args.repeats,
             "bar: median(zip) - median(other) <= max(spread zip, spread other) + %.0f us (one launch boundary)" % LAUNCH_US, ""]
    bad = 0
    # 4096 x 56 KiB: the same deflate payloads (level 6, 64 distinct) as BGZF members and as ZIP entries
    B, n, kinds = 4096, 57344, 64
    datas = [text(n, 300 + k) for k in range(kinds)]
    raws = [deflate(d) for d in datas]
    hdr = bytes([0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF, 6, 0, 0x42, 0x43, 2, 0])
    members = [hdr + struct.pack("<H", len(r) + 25) + r + struct.pack("<II", zlib.crc32(d), len(d)) for r, d in zip(raws, datas)]
    f = b"".join(members[k % kinds] for k in range(B)) + bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    df = torch.frombuffer(bytearray(f + bytes(64)), dtype=torch.uint8).cuda()[:len(f)]
    off, out_off, rec = eng.bgzf_index(df)
    M = off.numel() - 2                                         # (without the EOF member)
    assert rec.status == 0 and M == B
    bout = torch.empty(B * n, dtype=torch.uint8, device="cuda")
    bres = torch.zeros(3, dtype=torch.int64, device="cuda")
    bwb = L.hdlz_bgzf_inflate_work_bytes(M, 0)
    bwork = torch.empty(bwb, dtype=torch.uint8, device="cuda")
    a = Zip(eng, make_zip([(b"%04d" % k, datas[k % kinds], 8, raws[k % kinds]) for k in range(B)]), out_align=1)
    calls = [("zip", a.read_call(0, B, 0)),
             ("bgzf", lambda: L.hdlz_bgzf_inflate_ws(df.data_ptr(), len(f), off.data_ptr(), out_off.data_ptr(), M, 0, bout.data_ptr(), bout.numel(), None,
                                                     bres.data_ptr(), bwork.data_ptr(), bwb, st))]
    t = timed(calls, args.repeats, args.warmup)
    a.verify(0, B, [datas[0], datas[(B - 1) % kinds]])
    assert bout[:n].cpu().numpy().tobytes() == datas[0] and _lib.BgzfInflateResult.from_buffer_copy(bres.cpu().numpy().tobytes()).status == 0
    (mz, sz), (mb, sb) = stat(t["zip"]), stat(t["bgzf"])
    allowed = max(sz, sb) + LAUNCH_US
    held = mz - mb <= allowed
    bad += not held
    lines += ["%d x %d bytes (%d bytes of deflate each, about):" % (B, n, len(raws[0])), line("hdlz_zip_inflate_ws, one call", t["zip"]),
              line("hdlz_bgzf_inflate_ws", t["bgzf"]), "  zip - bgzf = %+.1f us, allowed %.1f us: %s" % (mz - mb, allowed, "held" if held else "MISSED"), ""]
    del a, bout
    # one 16 MiB level-6 payload: a ZIP entry alone against a gzip member alone
    d = text(16 << 20, 9)
    raw = deflate(d)
    g = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + raw + struct.pack("<II", zlib.crc32(d), len(d))
    dg = torch.frombuffer(bytearray(g + bytes(64)), dtype=torch.uint8).cuda()
    cap = 16 << 20
    gout = torch.empty(cap, dtype=torch.uint8, device="cuda")
    gres = [torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(4)]
    gwb = L.hdlz_gunzip_work_bytes(1, len(g), cap, 0)
    gwork = torch.empty(gwb, dtype=torch.uint8, device="cuda")
    a = Zip(eng, make_zip([(b"big.bin", d, 8, raw)]))
    calls = [("zip", a.read_call(0, 1, len(raw) + 6)),
             ("gz", lambda: L.hdlz_gunzip_ws(dg.data_ptr(), None, len(g), len(g), 1, gout.data_ptr(), cap, *[x.data_ptr() for x in gres], gwork.data_ptr(), gwb, st))]
    t = timed(calls, args.repeats, args.warmup)
    a.verify(0, 1, [d])
    assert int(gres[1].item()) == 0 and int(gres[0].item()) == len(d)
    (mz, sz), (mg, sg) = stat(t["zip"]), stat(t["gz"])
    allowed = max(sz, sg) + LAUNCH_US
    held = mz - mg <= allowed
    bad += not held
    lines += ["one 16 MiB entry (%d bytes of deflate), alone in its call:" % len(raw), line("hdlz_zip_inflate_ws, count == 1", t["zip"]),
              line("hdlz_gunzip_ws, nstreams == 1", t["gz"]), "  zip - gunzip = %+.1f us, allowed %.1f us: %s" % (mz - mg, allowed, "held" if held else "MISSED"), ""]
    put_section(args.out, "3. what the frame costs: against hdlz_bgzf_inflate_ws and hdlz_gunzip_ws on the same payloads", lines)
    return 1 if bad else 0


def cmd_crossover(args):
    from hdl_deflate_amd import Engine
    eng = Engine()
    lines = ["command: python tools/probe_zip.py crossover --repeats %d" % args.repeats,
             "one level-6 entry of text: (a) alone, count == 1, in_len = csize + 6; (b) the first of a two-entry call (the second: 16 bytes); no bar", ""]
    small = b"0123456789abcdef"
    cross = None
    for kib in (4, 8, 16, 32, 64, 128, 256, 512, 1024):
        d = text(kib << 10, 400 + kib)
        raw = deflate(d)
        a = Zip(eng, make_zip([(b"e", d, 8, raw), (b"s", small, 0, None)]))
        t = timed([("one", a.read_call(0, 1, len(raw) + 6)), ("two", a.read_call(0, 2, 0))], args.repeats, args.warmup)
        a.verify(0, 1, [d]); a.verify(0, 2, [d, small])
        mo, mt = stat(t["one"])[0], stat(t["two"])[0]
        if cross is None and mo < mt:
            cross = (kib, len(raw))
        lines += ["%4d KiB (csize %7d):  alone %9.1f us (spread %7.1f)   in a two-entry call %9.1f us (spread %7.1f)   alone / two = %.3f" %
                  (kib, len(raw), mo, stat(t["one"])[1], mt, stat(t["two"])[1], mo / mt)]
        del a
    lines += ["", "the call of its own is the faster one from %s on" % ("%d KiB (csize %d)" % cross if cross else "no size measured"), ""]
    put_section(args.out, "4. the HDLZ_ZIP_LARGE_MIN crossover: an entry alone against the same entry in a batch", lines)
    return 0


def cmd_stored(args):
    import torch
    from hdl_deflate_amd import Engine
    eng = Engine()
    n = 64 << 20
    d = np.random.default_rng(5).integers(0, 256, n, dtype=np.uint8).tobytes()
    a = Zip(eng, make_zip([(b"stored.bin", d, 0, None)]))
    src = torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda()
    dst = torch.empty_like(src)

    def copy():
        dst.copy_(src)
        return 0
    t = timed([("zip", a.read_call(0, 1, 0)), ("copy", copy)], args.repeats, args.warmup)
    a.verify(0, 1, [d])
    mz, mc = stat(t["zip"])[0], stat(t["copy"])[0]
    lines = ["command: python tools/probe_zip.py stored --repeats %d" % args.repeats,
             "one stored entry of 64 MiB alone in its call -- the checks, the flat copy, the CRC-32 tiles, the verdict -- against a device copy of 64 MiB; no bar", "",
             line("hdlz_zip_inflate_ws, count == 1, stored", t["zip"], "   %.0f GB/s of payload" % (n / mz / 1e3)),
             line("torch copy_ of the same bytes", t["copy"], "   %.0f GB/s (read + write: twice that)" % (n / mc / 1e3)),
             "  (bench.py's device_copy_GBps counts read + write; the call also reads the slot once more for the CRC-32)", ""]
    put_section(args.out, "5. the stored copy against a device copy", lines)
    return 0


def cmd_ab(args):
    import torch
    from hdl_deflate_amd import _lib, Engine
    L, Pa = _lib.load(), _bind(args.parent)
    eng = Engine()
    st = torch.cuda.current_stream().cuda_stream
    lines = ["command: python tools/probe_zip.py ab --parent <libhdlz.so of a build of the parent commit> --repeats %d" % args.repeats,
             "within a repeat: parent, this build, parent again; the bar: |this build - the parent's mean median| <= the larger of the",
             "difference of the parent's two medians and the parent's larger spread", ""]
    bad = 0
    data = torch.from_numpy(np.frombuffer(text(16 << 20, 9), np.uint8).copy()).cuda()
    f = eng.compress_bgzf(data, block=57344)
    off, out_off, rec = eng.bgzf_index(f)
    M = off.numel() - 1
    out = torch.empty(data.numel(), dtype=torch.uint8, device="cuda")
    res = torch.zeros(3, dtype=torch.int64, device="cuda")
    wb = L.hdlz_bgzf_inflate_work_bytes(M, 0)
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    d = text(4 << 20, 11)
    g = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + deflate(d) + struct.pack("<II", zlib.crc32(d), len(d))
    dg = torch.frombuffer(bytearray(g + bytes(64)), dtype=torch.uint8).cuda()
    gout = torch.empty(4 << 20, dtype=torch.uint8, device="cuda")
    gres = [torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(4)]
    gwb = L.hdlz_gunzip_work_bytes(1, len(g), 4 << 20, 0)
    gwork = torch.empty(gwb, dtype=torch.uint8, device="cuda")

    def bgzf(lib):
        return lib.hdlz_bgzf_inflate_ws(f.data_ptr(), f.numel(), off.data_ptr(), out_off.data_ptr(), M, 0, out.data_ptr(), out.numel(), None,
                                        res.data_ptr(), work.data_ptr(), wb, st)

    def gunzip(lib):
        return lib.hdlz_gunzip_ws(dg.data_ptr(), None, len(g), len(g), 1, gout.data_ptr(), 4 << 20, *[x.data_ptr() for x in gres], gwork.data_ptr(), gwb, st)
    for what, call in (("hdlz_bgzf_inflate_ws, 16 MiB in %d members" % M, bgzf), ("hdlz_gunzip_ws, one 4 MiB member", gunzip)):
        t = timed([("p1", lambda: call(Pa)), ("new", lambda: call(L)), ("p2", lambda: call(Pa))], args.repeats, args.warmup)
        (m1, s1), (mn, sn), (m2, s2) = stat(t["p1"]), stat(t["new"]), stat(t["p2"])
        allowed = max(abs(m1 - m2), s1, s2)
        held = abs(mn - (m1 + m2) / 2) <= allowed
        bad += not held
        lines += [what + ":", line("parent, first in the repeat", t["p1"]), line("this build", t["new"]), line("parent, last in the repeat", t["p2"]),
                  "  this build - parent %+.1f us, allowed %.1f us: %s" % (mn - (m1 + m2) / 2, allowed, "held" if held else "MISSED"), ""]
    assert torch.equal(out, data) and gout.cpu().numpy().tobytes() == d
    put_section(args.out, "6. existing calls against the parent commit's library", lines)
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("cmd", choices=("index", "frame", "crossover", "stored", "ab"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zip.txt"))
    ap.add_argument("--parent")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert args.repeats >= 10
    return {"index": cmd_index, "frame": cmd_frame, "crossover": cmd_crossover, "stored": cmd_stored, "ab": cmd_ab}[args.cmd](args)


if __name__ == "__main__":
    sys.exit(main())
