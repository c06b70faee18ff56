#!/usr/bin/env python
"""Evidence for hdlz_png_filter_ws / hdlz_png_write_ws (include/hdlz_png_write.h) -> profiles/png_write.txt, on the three workloads of
profiles/png.txt (the pictures of tools/probe_png.py):

  4096 images of 64 x 64 RGBA        (64 distinct ones, each 64 times)
  256 images of 512 x 512 RGB        (16 distinct ones, each 16 times)
  one 4096 x 4096 RGBA image         smooth plus noise

  encode_png      the three calls of Engine.encode_png (filter, ONE hdlz_compress_batch_bits, write), no host sync inside, against its
                  yardstick measured in the same run: hdlz_compress_batch_bits + hdlz_join_batch_ws over the same already-filtered bytes
                  and the same blocks -- what the library did before it wrote PNG
  kernels         the kernel times of one profiled repeat (torch.profiler, device activity), by kernel name
  filter / copy   hdlz_png_filter_ws against a device-to-device copy of the stream's bytes, in the same run
  HBM traffic     --counters: FETCH_SIZE and WRITE_SIZE of k_pngw_filter from two counters-only rocprofv3 runs of their own (the two do
                  not fit one pass) over 5 images of 4096 x 4096 RGBA -- 320 MiB of pixels, past the 256 MiB Infinity Cache --, against
                  the algorithmic bytes (pixels in + streams out).  FETCH_SIZE is doubled: on gfx950 it tallies a wide read at half.
  file sizes      against Pillow's default writer where Pillow is installed, for information

HIP events around the calls, the PNG calls and the yardstick in turn within a repeat; median, min and max of --repeats after --warmup."""
import argparse
import csv
import glob
import io
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
NAMES = ("4096 x 64x64 RGBA", "256 x 512x512 RGB", "1 x 4096x4096 RGBA")


def workload(name):
    from probe_png import picture
    if name == NAMES[0]:
        w, h, ch, distinct, times = 64, 64, 4, 64, 64
    elif name == NAMES[1]:
        w, h, ch, distinct, times = 512, 512, 3, 16, 16
    else:
        w, h, ch, distinct, times = 4096, 4096, 4, 1, 1
    pics = [picture(w, h, ch, k) for k in range(distinct)]
    return pics * times, (h, w, ch, 8)


def timed(fn, torch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def measure(eng, name, repeats, warmup):
    import ctypes
    import torch
    from hdl_deflate_amd import _lib
    pics, shape = workload(name)
    n = len(pics)
    flat = torch.frombuffer(bytearray(b"".join(pics)), dtype=torch.uint8).cuda()
    p = eng._png_plan(flat, [shape] * n, "adaptive", 1 << 16, 1 << 16, 32, 10, None, 64, True)
    L = eng.lib
    # the yardstick's buffers: the join of the same rows
    jw = eng._scratch(L.hdlz_join_work_bytes(p.B), None, full=True)
    joined = torch.empty(L.hdlz_join_bound(p.B, p.block), dtype=torch.uint8, device="cuda")
    joff = torch.empty(p.B + 1, dtype=torch.int64, device="cuda")
    jres = torch.empty(ctypes.sizeof(_lib.JoinResult) // 8, dtype=torch.int64, device="cuda")
    copy_dst = torch.empty_like(p.raw)

    def encode():
        eng._png_launch(p)

    def filt():
        eng._check(L.hdlz_png_filter_ws(p.d_pix.data_ptr(), p.d_pix.numel(), p.specs.data_ptr(), n, p.mode, p.total_rows, p.raw.data_ptr(), p.total_raw,
                                        p.row_filter.data_ptr(), p.fstatus.data_ptr(), p.raw_off.data_ptr(), p.fwork[1], p.fwork[2], eng._stream()), "filter")

    def copy():
        copy_dst.copy_(p.raw)

    def yard():
        eng._check(L.hdlz_compress_batch_bits(p.cin.data_ptr(), p.in_off.data_ptr(), 0, p.block, p.B, p.cwindow, p.maxmatch, p.rows.data_ptr(), p.pitch,
                                              p.len.data_ptr(), p.status.data_ptr(), p.end_bits.data_ptr(), eng._stream()), "compress")
        eng._check(L.hdlz_join_batch_ws(p.rows.data_ptr(), p.pitch, p.len.data_ptr(), p.end_bits.data_ptr(), p.status.data_ptr(), p.in_off.data_ptr(), p.block,
                                        p.B, joined.data_ptr(), joined.numel(), joff.data_ptr(), jres.data_ptr(), jw[1], jw[2], eng._stream()), "join")

    encode()
    torch.cuda.synchronize()
    rec = _lib.PngWriteResult.from_buffer_copy(p.res[:p.nres].cpu().numpy().tobytes())
    assert rec.status == 0, rec.status
    yard()
    assert _lib.JoinResult.from_buffer_copy(jres.cpu().numpy().tobytes()).status == 0
    fns = {"encode_png (filter + compress + write)": encode, "yardstick (compress + join)": yard, "hdlz_png_filter_ws": filt, "device-to-device copy of the streams": copy}
    times = {k: [] for k in fns}
    for rep in range(warmup + repeats):
        for k, fn in fns.items():
            t = timed(fn, torch)
            if rep >= warmup:
                times[k].append(t)
    pix_bytes, mb = flat.numel(), 1e6
    lines = ["workload: %s -- %d images, %.1f MB of pixels, %.1f MB of filtered streams in %d blocks, %.1f MB of PNG files" %
             (name, n, pix_bytes / mb, p.total_raw / mb, p.B, rec.total_len / mb)]
    for k, t in times.items():
        lines.append("  %-40s median %10.1f us   min %10.1f   max %10.1f" % (k, statistics.median(t), min(t), max(t)))
    m = {k: statistics.median(t) for k, t in times.items()}
    ke, ky, kf, kc = list(fns)
    lines.append("  encode_png / yardstick: %.2fx    filter / copy: %.2fx    filter: %.1f GB/s of pixels in + streams out" %
                 (m[ke] / m[ky], m[kf] / m[kc], (pix_bytes + p.total_raw) / m[kf] / 1e3))
    try:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            encode()
            torch.cuda.synchronize()
        per = {}
        for ev in prof.key_averages():
            us = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
            if not us or "Memcpy" in ev.key or "Memset" in ev.key:
                continue
            key = ev.key.split("(")[0][-60:]
            per[key] = per.get(key, 0.0) + us
        fl = sum(us for k, us in per.items() if "k_pngw_plan" in k or "k_pngw_filter" in k)
        wr = sum(us for k, us in per.items() if "k_pngw_" in k) - fl
        co = sum(us for k, us in per.items() if "k_pngw_" not in k)
        lines.append("  steps (kernel time of one profiled repeat, us): filter %.1f; compress %.1f; write %.1f" % (fl, co, wr))
        lines.append("  the filter step %s the compress step" % ("costs LESS than" if fl < co else "costs MORE than"))
        for k, us in sorted(per.items(), key=lambda kv: -kv[1])[:8]:
            lines.append("    %-62s %10.1f us" % (k, us))
    except Exception as e:                                   # the totals stand without the breakdown
        lines.append("  steps: the profiler gave no kernel times here (%s: %s)" % (type(e).__name__, e))
    try:
        from PIL import Image
        h, w, ch, _ = shape
        a = np.frombuffer(pics[0], np.uint8).reshape(h, w, ch)
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, format="PNG")
        ours = int(p.file_len[0])
        lines.append("  file size of the first image: %d bytes here, %d bytes from Pillow's default writer (%.2fx)" % (ours, buf.tell(), ours / buf.tell()))
    except ImportError:
        lines.append("  file sizes against Pillow: Pillow is not installed here")
    return lines


def filter_only():
    """the child of a counters run: the filter call alone, three times, over 5 images of 4096 x 4096 RGBA made on the device"""
    import torch
    import hdl_deflate_amd
    eng = hdl_deflate_amd.Engine()
    h = w = 4096
    y, x, c = torch.meshgrid(torch.arange(h, device="cuda"), torch.arange(w, device="cuda"), torch.arange(4, device="cuda"), indexing="ij")
    one = ((x * 3 + y * 5 + c * 17 + torch.randint(0, 4, (h, w, 4), device="cuda")) & 255).to(torch.uint8).reshape(-1)
    flat = one.repeat(5)
    del x, y, c
    p = eng._png_plan(flat, [(h, w, 4, 8)] * 5, "adaptive", 1 << 16, 1 << 16, 32, 10, torch.empty(16, dtype=torch.uint8, device="cuda"), 64, True)
    for _ in range(3):
        eng._check(eng.lib.hdlz_png_filter_ws(p.d_pix.data_ptr(), p.d_pix.numel(), p.specs.data_ptr(), 5, p.mode, p.total_rows, p.raw.data_ptr(), p.total_raw,
                                              p.row_filter.data_ptr(), p.fstatus.data_ptr(), p.raw_off.data_ptr(), p.fwork[1], p.fwork[2], eng._stream()), "filter")
    torch.cuda.synchronize()
    assert int(p.fstatus.abs().sum()) == 0
    print("ALGORITHMIC %d %d" % (flat.numel(), p.total_raw))


def counters():
    """two counters-only runs of their own -> the lines of the report"""
    got, algo = {}, None
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--pmc", counter, "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--filter-only"]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
            for line in r.stdout.splitlines():
                if line.startswith("ALGORITHMIC"):
                    algo = tuple(int(v) for v in line.split()[1:])
            vals = []
            for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
                for row in csv.DictReader(open(f)):
                    if "k_pngw_filter" in row.get("Kernel_Name", "") and row.get("Counter_Name") == counter:
                        vals.append(float(row["Counter_Value"]))
            if r.returncode != 0 or not vals:
                return ["HBM traffic of k_pngw_filter: the counters run gave nothing here (rc %d, %d rows): %s" % (r.returncode, len(vals), r.stdout[-300:].replace("\n", " | "))]
            got[counter] = statistics.mean(vals) * 1024.0
    fetch, write = 2.0 * got["FETCH_SIZE"], got["WRITE_SIZE"]
    lines = ["HBM traffic of k_pngw_filter, 5 x 4096x4096 RGBA, adaptive (per dispatch, mean of 3; FETCH_SIZE doubled: gfx950 tallies wide reads at half)"]
    if algo:
        lines.append("  algorithmic: %.1f MB of pixels in, %.1f MB of streams out" % (algo[0] / 1e6, algo[1] / 1e6))
        lines.append("  measured:    %.1f MB fetched (%.2fx the pixels), %.1f MB written (%.2fx the streams)" % (fetch / 1e6, fetch / algo[0], write / 1e6, write / algo[1]))
    else:
        lines.append("  measured:    %.1f MB fetched, %.1f MB written" % (fetch / 1e6, write / 1e6))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_write.txt"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default=None)
    ap.add_argument("--counters", action="store_true", help="also the two counters-only rocprofv3 runs")
    ap.add_argument("--filter-only", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.filter_only:
        return filter_only()
    lines = ["command: python tools/probe_png_write.py --repeats %d --warmup %d%s" % (args.repeats, args.warmup, " --counters" if args.counters else ""), ""]
    if args.counters:                                        # in front of the engine: the children are the only processes on the GPU then
        lines += counters() + [""]
    import hdl_deflate_amd
    eng = hdl_deflate_amd.Engine()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name in NAMES:
        if args.only and args.only not in name:
            continue
        lines += measure(eng, name, args.repeats, args.warmup) + [""]
        with open(args.out, "w") as f:                        # (kept as far as it got)
            f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
