#!/usr/bin/env python
"""Evidence for hdlz_gunzip_ws (include/hdlz_gunzip.h) -> profiles/gunzip.txt, one sub-command per part; each replaces its own section
of --out and leaves the others.  HIP events around each call, the calls of a part in turn within a repeat, median of --repeats (at
least 10) after --warmup; a call's spread is max - min over its repeats.

  (section 1, no GPU: python tools/probe_unjoin.py codeobj --parent <csrc/_obj of a build of the parent commit> --sources <every source
   of build.sh but hdlz_gunzip and hdlz_api> --out profiles/gunzip.txt -- the resource lines of every existing kernel)
  crc --dbg LIB            section 2: the CRC tiles pass alone on ONE long row (64 MiB and 1 MiB) against hdlz_crc32_ws on the same
                           buffer: the same tile code, so it may take longer by no more than the larger of the two calls' spreads
                           plus one launch boundary (5 us).  LIB: a build with -DHDLZ_DEBUG_EXPORTS, which exports the
                           pass (HDLZ_VARIANT=dbg HDLZ_DEFS=-DHDLZ_DEBUG_EXPORTS HDLZ_ONLY="hdlz_gunzip hdlz_inflate_par" csrc/build.sh)
  frame                    section 3, no bar: hdlz_gunzip_ws against hdlz_inflate_checked on the same payloads in zlib framing --
                           4096 x 64 KiB and 65536 x 2 KiB (wave per stream on both sides), one 16 MiB level-6 stream (against the
                           checked call's own choice, the whole GPU, and against its wave-per-stream mapping)
  ab --parent LIB          section 4: hdlz_inflate_checked and hdlz_bgzf_inflate_ws of this build against the parent commit's library,
                           parent / this build / parent within a repeat: the difference is held against the parent's two series"""
import argparse
import ctypes
import os
import statistics
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from probe_unjoin import put_section      # noqa: E402

LAUNCH_US = 5.0
WAVE = 4


def _bind(path):
    from hdl_deflate_amd import _lib
    L = ctypes.CDLL(path)
    for t in (_lib.SIGNATURES, _lib.GZIP_SIGNATURES, _lib.BGZF_SIGNATURES, _lib.GUNZIP_SIGNATURES):
        for name, (restype, argtypes) in t.items():
            if hasattr(L, name):                            # (the parent has no hdlz_gunzip_ws)
                fn = getattr(L, name)
                fn.restype, fn.argtypes = restype, argtypes
    return L


def timed(calls, repeats, warmup):
    import torch
    times = {k: [] for k, _ in calls}
    for rep in range(warmup + repeats):
        for name, fn in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn()
            e1.record()
            e1.synchronize()
            assert rc == 0, name
            if rep >= warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    return times


def stat(t):
    return statistics.median(t), max(t) - min(t)


def line(name, t, extra=""):
    m, s = stat(t)
    return "  %-58s median %10.1f us   min %10.1f   max %10.1f   spread %8.1f%s" % (name, m, min(t), max(t), s, extra)


def text(n, seed):
    r = np.random.default_rng(seed)
    words = [bytes(r.integers(97, 123, r.integers(2, 10), dtype=np.uint8)) for _ in range(400)]
    out = b" ".join(words[i] for i in r.integers(0, 400, n // 5 + 16))
    return out[:n]


def cmd_crc(args):
    import torch
    D = ctypes.CDLL(args.dbg)
    L = _bind(args.dbg)
    D.hdlz_debug_gunzip_crc.restype = ctypes.c_int
    D.hdlz_debug_gunzip_crc.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64] + [ctypes.c_void_p] * 5
    st = torch.cuda.current_stream().cuda_stream
    lines = ["command: python tools/probe_gunzip.py crc --dbg <a build with -DHDLZ_DEBUG_EXPORTS> --repeats %d" % args.repeats,
             "one row, out_pitch = its length; (a) hdlz_crc32_ws, (b) k_gunzip_crc_tiles + k_gunzip_crc_finish (n read from d_out_len[0])",
             "bar: median(b) - median(a) <= max(spread a, spread b) + %.0f us (one launch boundary)" % LAUNCH_US, ""]
    bad = 0
    for n in (64 << 20, 1 << 20):
        buf = torch.randint(0, 256, (n + 4096,), dtype=torch.uint8, device="cuda")
        want = zlib.crc32(buf[:n].cpu().numpy().tobytes())
        wb = L.hdlz_crc32_work_bytes(n)
        work, tiles = (torch.empty(wb, dtype=torch.uint8, device="cuda") for _ in range(2))
        crc, crcw = (torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(2))
        ol = torch.tensor([n], dtype=torch.int32, device="cuda")
        ok = torch.zeros(1, dtype=torch.int32, device="cuda")
        calls = [("a", lambda: L.hdlz_crc32_ws(buf.data_ptr(), n, crc.data_ptr(), work.data_ptr(), wb, st)),
                 ("b", lambda: D.hdlz_debug_gunzip_crc(buf.data_ptr(), n, 1, ol.data_ptr(), ok.data_ptr(), crcw.data_ptr(), tiles.data_ptr(), st))]
        t = timed(calls, args.repeats, args.warmup)
        assert int(crc.item()) & 0xFFFFFFFF == want == int(crcw.item()) & 0xFFFFFFFF, (hex(want), crc, crcw)
        (ma, sa), (mb, sb) = stat(t["a"]), stat(t["b"])
        allowed = max(sa, sb) + LAUNCH_US
        held = mb - ma <= allowed
        bad += not held
        lines += ["%d MiB:" % (n >> 20), line("(a) hdlz_crc32_ws", t["a"], "   %.0f GB/s" % (n / ma / 1e3)), line("(b) the tiles pass of hdlz_gunzip_ws", t["b"]),
                  "  (b) - (a) = %+.1f us, allowed %.1f us: %s; both words equal zlib.crc32" % (mb - ma, allowed, "held" if held else "MISSED"), ""]
    put_section(args.out, "2. the CRC tiles pass on one long row against hdlz_crc32_ws", lines)
    return 1 if bad else 0


class Shape(object):
    """B streams, the same raw deflate payloads in gzip and in zlib framing, ragged; `kinds` distinct payloads repeated"""

    def __init__(self, L, B, n, kinds, level=6):
        import torch
        self.L, self.B, self.n = L, B, n
        raws = []
        for k in range(kinds):
            d = text(n, 100 + k)
            c = zlib.compressobj(level, zlib.DEFLATED, -15)
            raws.append((c.compress(d) + c.flush(), d))
        hdr = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03"
        gz = [hdr + r + zlib.crc32(d).to_bytes(4, "little") + len(d).to_bytes(4, "little") for r, d in raws]
        zl = [b"\x78\x9c" + r + zlib.adler32(d).to_bytes(4, "big") for r, d in raws]
        self.data0 = raws[0][1]
        self.pitch = (n + 15) // 16 * 16
        self.st = torch.cuda.current_stream().cuda_stream

        def stage(zs):
            order = [zs[k % kinds] for k in range(B)]
            flat = torch.from_numpy(np.frombuffer(b"".join(order) + bytes(64), np.uint8).copy()).cuda()
            off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(z) for z in order])]).astype(np.int64)).cuda()
            return flat, off, max(len(z) for z in zs)
        self.gz, self.zl = stage(gz), stage(zl)
        self.out = torch.empty((B, self.pitch), dtype=torch.uint8, device="cuda")
        self.res = [torch.empty(B, dtype=torch.int32, device="cuda") for _ in range(4)]
        self.bound = self.gz[2] if B == 1 else 0                 # (many short streams: no bound; one stream: its length)
        wb = max(L.hdlz_gunzip_work_bytes(B, self.bound, self.pitch, 1), L.hdlz_inflate_checked_work_bytes(B, self.bound, self.pitch, 0, 1))
        self.work, self.wb = torch.empty(wb, dtype=torch.uint8, device="cuda"), wb

    def gunzip(self):
        return self.L.hdlz_gunzip_ws(self.gz[0].data_ptr(), self.gz[1].data_ptr(), 0, self.bound, self.B, self.out.data_ptr(), self.pitch,
                                     *[t.data_ptr() for t in self.res], self.work.data_ptr(), self.wb, self.st)

    def checked(self, flags, lib=None):
        return (lib or self.L).hdlz_inflate_checked(self.zl[0].data_ptr(), self.zl[1].data_ptr(), 0, self.bound, self.B, flags, 0, self.out.data_ptr(),
                                                    self.pitch, *[t.data_ptr() for t in self.res], self.work.data_ptr(), self.wb, self.st)

    def verify(self):
        import torch
        torch.cuda.synchronize()
        assert int((self.res[1] != 0).sum()) == 0 and int((self.res[0] != self.n).sum()) == 0
        assert self.out[0, :self.n].cpu().numpy().tobytes() == self.data0


def cmd_frame(args):
    from hdl_deflate_amd import _lib
    L = _lib.load()
    lines = ["command: python tools/probe_gunzip.py frame --repeats %d" % args.repeats,
             "the same raw deflate payloads (level 6, text) with a 10-byte gzip header + CRC-32 + ISIZE and with 78 9C + Adler-32; ragged; no bar", ""]
    for B, n, kinds, what in ((4096, 65536, 64, "tiles: 2 per row"), (65536, 2048, 256, "a workgroup per row")):
        s = Shape(L, B, n, kinds)
        t = timed([("gz", s.gunzip), ("zl", lambda: s.checked(WAVE))], args.repeats, args.warmup)
        s.gunzip(); s.verify()
        s.checked(WAVE); s.verify()
        mg, mz = stat(t["gz"])[0], stat(t["zl"])[0]
        lines += ["%d x %d bytes (the CRC-32 pass: %s):" % (B, n, what), line("hdlz_gunzip_ws", t["gz"]),
                  line("hdlz_inflate_checked, HDLZ_INFLATE_WAVE_PER_STREAM", t["zl"]), "  ratio %.3f (%+.1f us)" % (mg / mz, mg - mz), ""]
        del s
    s = Shape(L, 1, 16 << 20, 1)
    t = timed([("gz", s.gunzip), ("zl", lambda: s.checked(0))], args.repeats, args.warmup)
    s.gunzip(); s.verify()
    tw = timed([("wave", lambda: s.checked(WAVE))], 2, 0)
    s.verify()
    mg, mz = stat(t["gz"])[0], stat(t["zl"])[0]
    lines += ["one 16 MiB stream (%d bytes of deflate):" % (s.gz[2] - 18), line("hdlz_gunzip_ws", t["gz"]),
              line("hdlz_inflate_checked, default mapping (the whole GPU)", t["zl"]), "  ratio %.3f (%+.1f us)" % (mg / mz, mg - mz),
              line("hdlz_inflate_checked, HDLZ_INFLATE_WAVE_PER_STREAM (2 repeats)", tw["wave"]), "  ratio %.5f" % (mg / stat(tw["wave"])[0]), ""]
    put_section(args.out, "3. what the frame costs: hdlz_gunzip_ws against hdlz_inflate_checked on the same payloads", lines)
    return 0


def cmd_ab(args):
    import torch
    from hdl_deflate_amd import _lib, Engine
    L, Pa = _lib.load(), _bind(args.parent)
    eng = Engine()
    lines = ["command: python tools/probe_gunzip.py ab --parent <libhdlz.so of a build of the parent commit> --repeats %d" % args.repeats,
             "within a repeat: parent, this build, parent again; the bar: |this build - the parent's mean median| <= the larger of the",
             "difference of the parent's two medians and the parent's larger spread", ""]
    bad = 0
    s = Shape(L, 4096, 65536, 64)
    data = torch.from_numpy(np.frombuffer(text(16 << 20, 9), np.uint8).copy()).cuda()
    f = eng.compress_bgzf(data, block=57344)
    off, out_off, rec = eng.bgzf_index(f)
    M = off.numel() - 1
    out = torch.empty(data.numel(), dtype=torch.uint8, device="cuda")
    res = torch.zeros(3, dtype=torch.int64, device="cuda")
    wb = L.hdlz_bgzf_inflate_work_bytes(M, 0)
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")

    def bgzf(lib):
        return lib.hdlz_bgzf_inflate_ws(f.data_ptr(), f.numel(), off.data_ptr(), out_off.data_ptr(), M, 0, out.data_ptr(), out.numel(), None,
                                        res.data_ptr(), work.data_ptr(), wb, s.st)
    for what, call in (("hdlz_inflate_checked, 4096 x 64 KiB, default mapping", lambda lib: s.checked(0, lib)),
                       ("hdlz_bgzf_inflate_ws, 16 MiB in %d members" % M, bgzf)):
        t = timed([("p1", lambda: call(Pa)), ("new", lambda: call(L)), ("p2", lambda: call(Pa))], args.repeats, args.warmup)
        (m1, s1), (mn, sn), (m2, s2) = stat(t["p1"]), stat(t["new"]), stat(t["p2"])
        allowed = max(abs(m1 - m2), s1, s2)
        held = abs(mn - (m1 + m2) / 2) <= allowed
        bad += not held
        lines += [what + ":", line("parent, first in the repeat", t["p1"]), line("this build", t["new"]), line("parent, last in the repeat", t["p2"]),
                  "  this build - parent %+.1f us, allowed %.1f us: %s" % (mn - (m1 + m2) / 2, allowed, "held" if held else "MISSED"), ""]
    assert torch.equal(out, data)
    put_section(args.out, "4. existing calls against the parent commit's library", lines)
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("cmd", choices=("crc", "frame", "ab"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gunzip.txt"))
    ap.add_argument("--dbg")
    ap.add_argument("--parent")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert args.repeats >= 10
    return {"crc": cmd_crc, "frame": cmd_frame, "ab": cmd_ab}[args.cmd](args)


if __name__ == "__main__":
    sys.exit(main())
