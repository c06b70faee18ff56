"""What does the checked inflate call cost?  hdlz_inflate_batch_ws against hdlz_inflate_checked, alternated in one process, device
events around every repetition, median and spread per shape; and -- with --parent-lib -- the unchecked configs[3] step of another build
of the library (the parent commit's, built side by side with HDLZ_VARIANT) alternated with this one's, the margin being the spread of
the parent against itself in the same run.

    python tools/probe_checked.py [--reps 20] [--parent-lib hdl_deflate_amd/lib/libhdlz_parent.so] > profiles/checked_inflate.txt
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/probe_checked.py --trace     # the judging pass's own kernels
    python tools/probe_checked.py --parse-trace DIR                                                   # ... per shape

--trace runs every shape's checked call TRACE_REPS times and nothing else, so that the k_adler_* dispatches of the trace can be told
apart by their order."""
import argparse
import csv
import ctypes
import glob
import multiprocessing as mp
import os
import statistics
import sys
import zlib

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
TRACE_REPS = 4
COPY_TBS = 6.29          # HBM traffic of a float4 copy on this part, TB/s, bytes read + bytes written (measured; 8.0 by the data sheet)


def _zfixed_many(args):
    blob, n = args
    out, lens = [], []
    for k in range(0, len(blob), n):
        co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
        z = co.compress(blob[k:k + n]) + co.flush()
        out.append(z)
        lens.append(len(z))
    return b"".join(out), lens


def _words(n, seed, vocab=4096, wlen=8):
    rng = np.random.default_rng(seed)
    w = rng.integers(97, 123, (vocab, wlen), dtype=np.uint8)
    w[:, -1] = 32
    return w[rng.integers(0, vocab, (n + wlen - 1) // wlen)].tobytes()[:n]


class Shape(object):
    """one call shape: the arguments both entry points take, output and result buffers, scratch of the checked query's size"""
    def __init__(self, torch, eng, name, d_in, d_off, in_pitch, in_len, n, flags, pitch, out_bytes):
        self.name, self.d_in, self.d_off, self.in_pitch, self.in_len, self.n, self.flags, self.pitch = name, d_in, d_off, in_pitch, in_len, n, flags, pitch
        self.out_bytes = out_bytes
        dev = d_in.device
        self.out = torch.empty((n, pitch), dtype=torch.uint8, device=dev)
        self.ol, self.st, self.used, self.ad = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4))
        ragged = 0 if d_off is None else 1
        self.wb = eng.lib.hdlz_inflate_checked_work_bytes(n, in_len, pitch, flags, ragged)
        self.share = self.wb - eng.lib.hdlz_inflate_work_bytes(n, in_len, pitch, flags, ragged)
        self.work = torch.empty(self.wb, dtype=torch.uint8, device=dev)

    def args(self):
        return (self.d_in.data_ptr(), None if self.d_off is None else self.d_off.data_ptr(), self.in_pitch, self.in_len, self.n, self.flags, 0,
                self.out.data_ptr(), self.pitch, self.ol.data_ptr(), self.st.data_ptr())

    def unchecked(self, lib, stream):
        # (the same scratch minus the judging pass's share: what the checked call hands to its decode)
        rc = lib.hdlz_inflate_batch_ws(*self.args(), self.work.data_ptr() + self.share, self.wb - self.share, stream)
        assert rc == 0, rc

    def checked(self, lib, stream):
        rc = lib.hdlz_inflate_checked(*self.args(), self.used.data_ptr(), self.ad.data_ptr(), self.work.data_ptr(), self.wb, stream)
        assert rc == 0, rc


def shape_names(which):
    """(name, output bytes) of the shapes make_shapes builds, in its order"""
    names = []
    if which & 1:
        names += [("%d x 2 KiB Z_FIXED%s" % (nb, " (configs[3])" if nb == 1 << 20 else ""), nb * 2048) for nb in (1 << 20, 12288, 2000)]
    if which & 2:
        names.append(("256 x 1 MiB zlib level 6", 256 << 20))
    if which & 4:
        names.append(("ONE 16 MiB own stream", 16 << 20))
    if which & 16:
        names.append(("ONE 256 MiB own stream", 256 << 20))
    if which & 8:
        names.append(("ONE 16 MiB zlib level 6 stream", 16 << 20))
    return names


def host_streams(which):
    """the 2^20 Z_FIXED streams of configs[3] (bench.py's: blocks of families 1 / 2 / 4), compressed by stock zlib on 12 host cores"""
    if not which & 1:
        return None
    import torch
    from hdl_deflate_amd.data import make_blocks
    B, n = 1 << 20, 2048
    host = make_blocks(B, n, torch.device("cuda", 0), seed=4, families=(1, 2, 4)).cpu().numpy()
    per = 4096
    pool = mp.get_context("fork").Pool(12)
    try:
        parts = pool.map(_zfixed_many, [(host[k:k + per].tobytes(), n) for k in range(0, B, per)])
    finally:
        pool.close()
        pool.join()
    lens = np.fromiter((l for _, ls in parts for l in ls), dtype=np.int64, count=B)
    off = np.zeros(B + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    return np.frombuffer(b"".join(p for p, _ in parts) + bytes(64), dtype=np.uint8).copy(), off


def make_shapes(torch, eng, which, hs):
    from hdl_deflate_amd.data import make_blocks
    dev = torch.device("cuda", 0)
    shapes = []
    if which & 1:
        B, n = 1 << 20, 2048
        d_in, d_off = torch.from_numpy(hs[0]).to(dev), torch.from_numpy(hs[1]).to(dev)
        for nb in (B, 12288, 2000):
            shapes.append(Shape(torch, eng, "%d x 2 KiB Z_FIXED%s" % (nb, " (configs[3])" if nb == B else ""), d_in, d_off[:nb + 1].contiguous(), 0, 0, nb,
                                1, n, nb * n))
    if which & 2:
        kinds = [zlib.compress(_words(1 << 20, 60 + k), 6) for k in range(8)]
        pitch = (max(len(z) for z in kinds) + 64 + 15) // 16 * 16
        host = np.zeros((256, pitch), np.uint8)
        for b in range(256):
            host[b, :len(kinds[b % 8])] = np.frombuffer(kinds[b % 8], np.uint8)
        shapes.append(Shape(torch, eng, "256 x 1 MiB zlib level 6", torch.from_numpy(host).to(dev), None, pitch, pitch, 256, 0, (1 << 20) + 64, 256 << 20))
    for bit, mib in ((4, 16), (16, 256)):
        if which & bit:
            n = mib << 20
            d = make_blocks(n // 2048 + 1, 2048, dev, seed=5).reshape(-1)
            out, ol, st = eng.compress_stream(d, n)
            zn = int(ol.item())
            assert int(st.item()) == 0
            zin = torch.zeros((1, (zn + 64 + 15) // 16 * 16), dtype=torch.uint8, device=dev)
            zin[0, :zn] = out[:zn]
            del d, out
            torch.cuda.empty_cache()
            shapes.append(Shape(torch, eng, "ONE %d MiB own stream" % mib, zin, None, zin.shape[1], zn, 1, 0, n + 64, n))
    if which & 8:
        n = 16 << 20
        z = zlib.compress(_words(n, 51), 6)
        zin = torch.from_numpy(np.frombuffer(z + bytes(64), np.uint8).copy()).to(dev).reshape(1, -1)
        shapes.append(Shape(torch, eng, "ONE 16 MiB zlib level 6 stream", zin, None, zin.shape[1], len(z), 1, 0, n + 64, n))
    return shapes


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    return "median %8.3f ms  (min %8.3f, max %8.3f, n = %d)" % (statistics.median(v), min(v), max(v), len(v))


def load_other(path):
    L = ctypes.CDLL(path)
    vp, u64, u32, ci = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    L.hdlz_inflate_batch_ws.restype = ci
    L.hdlz_inflate_batch_ws.argtypes = [vp, vp, u64, u32, u64, u32, u32, vp, u64, vp, vp, vp, ctypes.c_size_t, vp]
    return L


def parse_trace(d, names):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "k_adler" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    main = [r for r in rows if "k_adler_finish" not in r[2]]
    fin = [r for r in rows if "k_adler_finish" in r[2]]
    print("judging pass, kernel time from the trace (%d dispatches of k_adler_rows / _tiles, %d of k_adler_finish)" % (len(main), len(fin)))
    fi = 0
    for k, (name, out_bytes) in enumerate(names):
        mine = main[k * TRACE_REPS:(k + 1) * TRACE_REPS]
        if not mine:
            break
        tiled = "tiles" in mine[0][2]
        us = [m[1] / 1e3 for m in mine[1:]]
        fus = []
        if tiled:
            fus = [f[1] / 1e3 for f in fin[fi + 1:fi + TRACE_REPS]]
            fi += TRACE_REPS
        med = statistics.median(us)
        print("  %-34s %-13s %9.1f us (min %.1f max %.1f)%s  -> %7.1f GB/s of output read  (%.0f %% of the %.2f TB/s a float4 copy moves, read + written)" %
              (name, "k_adler_tiles" if tiled else "k_adler_rows", med, min(us), max(us),
               "  + finish %.1f us" % statistics.median(fus) if fus else "", out_bytes / med / 1e3, 100.0 * (out_bytes / med / 1e3) / (COPY_TBS * 1e3), COPY_TBS))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--which", type=int, default=31, help="bit mask: 1 = the 2 KiB batches, 2 = 256 x 1 MiB, 4 = 16 MiB own, 8 = 16 MiB zlib, 16 = 256 MiB own")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--parse-trace", default=None)
    a = ap.parse_args()
    if a.parse_trace:
        parse_trace(a.parse_trace, shape_names(a.which))
        return
    hs = host_streams(a.which)
    import torch
    import hdl_deflate_amd
    torch.cuda.set_device(0)
    eng = hdl_deflate_amd.Engine()
    lib, stream = eng.lib, torch.cuda.current_stream().cuda_stream
    shapes = make_shapes(torch, eng, a.which, hs)
    assert [s.name for s in shapes] == [n for n, _ in shape_names(a.which)]
    if a.trace:
        for s in shapes:
            for _ in range(TRACE_REPS):
                s.checked(lib, stream)
            torch.cuda.synchronize()
            assert int((s.st != 0).sum().item()) == 0
        return
    print("hdlz_inflate_batch_ws against hdlz_inflate_checked: device events, alternated, %d repetitions after 3 warm-up rounds" % a.reps)
    for s in shapes:
        for _ in range(3):
            s.unchecked(lib, stream)
            s.checked(lib, stream)
        torch.cuda.synchronize()
        assert int((s.st != 0).sum().item()) == 0, s.name
        tu, tc = [], []
        for _ in range(a.reps):
            tu.append(timed(torch, lambda: s.unchecked(lib, stream)))
            tc.append(timed(torch, lambda: s.checked(lib, stream)))
        mu, mc = statistics.median(tu), statistics.median(tc)
        print("%s   (output %d MiB, judging share of the scratch %d bytes)" % (s.name, s.out_bytes >> 20, s.share))
        print("    unchecked  %s   %7.1f GB/s" % (stats(tu), s.out_bytes / mu / 1e6))
        print("    checked    %s   %7.1f GB/s" % (stats(tc), s.out_bytes / mc / 1e6))
        print("    extra      %8.3f ms = %.1f %%; the output read once in that time: %.1f GB/s" % (mc - mu, 100.0 * (mc - mu) / mu, s.out_bytes / max(mc - mu, 1e-6) / 1e6))
    if a.parent_lib and shapes and (a.which & 1):
        s = shapes[0]
        other = load_other(a.parent_lib)
        print("the unchecked path did not move: %s, hdlz_inflate_batch_ws of %s (P) and of this build (C), alternated P C P C .." % (s.name, a.parent_lib))
        for _ in range(3):
            s.unchecked(other, stream)
            s.unchecked(lib, stream)
        p1, p2, c = [], [], []
        for k in range(a.reps):
            (p1 if k % 2 == 0 else p2).append(timed(torch, lambda: s.unchecked(other, stream)))
            c.append(timed(torch, lambda: s.unchecked(lib, stream)))
        print("    parent, even rounds  %s" % stats(p1))
        print("    parent, odd rounds   %s" % stats(p2))
        print("    change               %s" % stats(c))
        mp_ = statistics.median(p1 + p2)
        print("    change - parent = %+.3f ms (%+.2f %%); margin (parent against itself, even - odd rounds) = %+.3f ms" %
              (statistics.median(c) - mp_, 100.0 * (statistics.median(c) - mp_) / mp_, statistics.median(p1) - statistics.median(p2)))


if __name__ == "__main__":
    main()
