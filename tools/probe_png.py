#!/usr/bin/env python
"""Evidence for hdlz_png_index_ws / hdlz_png_decode_ws (include/hdlz_png.h) -> profiles/png.txt: the time per step (index, gather + CRC,
decode, unfilter + expand) and the total of Engine.png_index + Engine.decode_png on three workloads, next to the yardstick -- the checked
inflate (Engine.inflate_checked, which is what inflate_bytes(verify=True) runs on the device) over the same zlib payloads, already
gathered.

  4096 images of 64 x 64 RGBA        (64 distinct ones, each 64 times)
  256 images of 512 x 512 RGB        (16 distinct ones, each 16 times)
  one 4096 x 4096 RGBA image         smooth plus noise, level 6, adaptive filters (the minimum sum of absolute differences per row), so all
                                     five filter types occur; IDAT chunks of 64 KiB

Totals: HIP events around the calls of Engine.decode_png (no host sync inside), the PNG calls and the yardstick in turn within a repeat,
median of --repeats after --warmup, spread = max - min.  --adam7 (-> profiles/png_adam7.txt): on each workload decode_png over the same
pixels stored plain and Adam7 interlaced (tests/png_adam7_ref.py's encoder, adaptive filters inside every pass), in turn within a repeat,
and the kernel times of k_png_unfilter and k_png_deinterlace of one profiled repeat.  --retime: decode_png alone on the three plain
workloads, every run listed, for comparing two builds of the library in one session: a process a build (HDLZ_LIB), or --against PATH,
which loads the second build into the same process and times the two call by call in turn.  Steps: the kernels of one more repeat, profiler on (torch.profiler, device
activity), summed by kernel name -- gather + CRC: k_png_plan, k_png_list, k_png_gather, k_png_crc; decode: every kernel that is not
k_png_*; unfilter + expand: k_png_unfilter, k_png_expand; judge: k_png_adler, k_png_judge, k_png_finish.  The profiled pass is not timed."""
import argparse
import os
import statistics
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import png_ref as P      # noqa: E402
import png_adam7_ref as A      # noqa: E402


def adaptive(rows, h, rb, bpp):
    """per row the filter with the least sum of absolute (signed) residuals -> the list of filter types"""
    a = np.frombuffer(rows, np.uint8).reshape(h, rb).astype(np.int16)
    z = np.zeros((h, bpp), np.int16)
    left = np.concatenate([z, a[:, :-bpp]], axis=1)
    up = np.concatenate([np.zeros((1, rb), np.int16), a[:-1]], axis=0)
    ul = np.concatenate([z, up[:, :-bpp]], axis=1)
    p = left + up - ul
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
    pae = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    cost = [np.abs(((a - q) & 255).astype(np.uint8).view(np.int8).astype(np.int32)).sum(axis=1) for q in (0 * a, left, up, (left + up) >> 1, pae)]
    return [int(x) for x in np.argmin(np.stack(cost), axis=0)]


def picture(w, h, ch, seed):
    """smooth plus noise, in bands of 16 rows of five kinds, so that every filter type is some row's best: noise; rows of one level;
    columns of one level; a smooth surface; hard diagonal edges"""
    r = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    kind = ((y // 16 + seed) % 5)[:, :, None]
    c = np.arange(ch)[None, None, :] * 9
    noise = r.integers(0, 256, (h, w, ch))
    small = r.integers(-2, 3, (h, w, ch))
    rows = ((y * 37 + seed * 11) % 200)[:, :, None] + c + small
    cols = ((x * 53 + seed * 7) % 200)[:, :, None] + c + small
    smooth = (128 + 100 * np.sin(x / (17.0 + seed % 5)) * np.cos(y / 23.0))[:, :, None] + c + r.integers(-6, 7, (h, w, ch))
    edges = (((x + y) // 24 % 2) * 180 + ((x - y) // 40 % 2) * 40)[:, :, None] + c + small
    a = np.where(kind == 0, noise, np.where(kind == 1, rows, np.where(kind == 2, cols, np.where(kind == 3, smooth, edges))))
    return np.clip(a, 0, 255).astype(np.uint8).tobytes()


def workload(name, interlaced=False):
    if name == "4096 x 64x64 RGBA":
        w, h, colour, distinct, times, idat = 64, 64, 6, 64, 64, None
    elif name == "256 x 512x512 RGB":
        w, h, colour, distinct, times, idat = 512, 512, 2, 16, 16, 65536
    else:
        w, h, colour, distinct, times, idat = 4096, 4096, 6, 1, 1, 65536
    ch = P.CHANNELS[colour]
    files, first = [], None
    for k in range(distinct):
        rows = picture(w, h, ch, k)
        first = first or rows
        if interlaced:                                       # the same pixels; the adaptive choice is made inside every pass
            fl = sum((adaptive(sub, g[5], g[6], ch) for sub, g in zip(A.interlace_rows(rows, w, h, colour, 8), A.passes_of(w, h, colour, 8))), [])
            files.append(A.make_adam7(w, h, colour, 8, rows=rows, filters=fl, level=6, idat=idat))
            continue
        files.append(P.make_png(w, h, colour, 8, rows=rows, filters=adaptive(rows, h, w * ch, ch), level=6, idat=idat))
    return files * times, first


def measure(eng, name, repeats, warmup):
    import torch
    files, first = workload(name)
    blob = b"".join(files)
    d = torch.frombuffer(bytearray(blob + bytes(16)), dtype=torch.uint8).cuda()[:len(blob)]
    lens = np.array([len(f) for f in files], np.int64)
    off, ln = torch.from_numpy(np.cumsum(lens) - lens).cuda(), torch.from_numpy(lens).cuda()
    pi = eng.png_index(d, off, ln)
    h = pi.host
    assert (h["status"] == 0).all()
    out, status = eng.decode_png(d, pi)
    assert int((status != 0).sum()) == 0
    assert out[:len(first)].cpu().numpy().tobytes() == first          # (8-bit RGB and RGBA: the pixels are the encoder's scanlines)
    # the yardstick's input: the zlib payloads, gathered, and their ragged index
    nd = len(set(files))                                     # (the distinct files come first)
    zs = [P.chunks_of(f, P.index([f])["images"][0])[1] for f in files[:nd]] * (len(files) // nd)
    zoff = np.concatenate([[0], np.cumsum([len(z) for z in zs])]).astype(np.int64)
    dz = torch.frombuffer(bytearray(b"".join(zs) + bytes(64)), dtype=torch.uint8).cuda()
    dzo = torch.from_numpy(zoff).cuda()
    pitch = (int(h["raw_len"].max()) + 3) & ~3
    yout = torch.empty((len(files), pitch), dtype=torch.uint8, device="cuda")
    ywork = torch.empty(eng.lib.hdlz_inflate_checked_work_bytes(len(files), int(max(len(z) for z in zs)), pitch, 0, 1), dtype=torch.uint8, device="cuda")

    def png():
        eng.decode_png(d, pi, out=out)

    def alone():                                             # every large image in a call of its own, whatever their number
        keep, eng.PNG_ALONE_US = eng.PNG_ALONE_US, 0.0
        try:
            eng.decode_png(d, pi, out=out)
        finally:
            eng.PNG_ALONE_US = keep

    def index():
        eng.png_index(d, off, ln)

    def yard():
        res = eng.inflate_checked(dz, in_off=dzo, in_len=int(max(len(z) for z in zs)), out_pitch=pitch, out=yout, work=ywork)
        return res

    assert int((yard()[2] != 0).sum()) == 0
    times = {"index (one host sync inside)": [], "decode_png": [], "inflate_checked (yardstick)": []}
    large = int((h["zlen"] >= P.LARGE_MIN).sum())
    routed_alone = large * eng.PNG_ALONE_US <= int(h["raw_len"].max()) * eng.PNG_WAVE_US_PER_BYTE
    fns = [index, png, yard]
    if large > 1:
        times["decode_png, every large image alone"] = []
        fns.append(alone)
    for rep in range(warmup + repeats):
        for key, fn in zip(times, fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= warmup:
                times[key].append(e0.elapsed_time(e1) * 1e3)
    lines = ["workload: %s -- %d files, %.1f MB of PNG, %.1f MB of zlib streams, %.1f MB of pixels; %d decode call(s)" %
             (name, len(files), len(blob) / 1e6, zoff[-1] / 1e6, pi.record.total_out / 1e6,
              large + (1 if large < len(files) else 0) if routed_alone else 1)]
    if large > 1:
        lines.append("  %d images of HDLZ_PNG_LARGE_MIN compressed bytes and more: Engine.decode_png routes them %s" %
                     (large, "alone, a call each" if routed_alone else "together, in ONE call (a wave each): their calls would cost more than the longest costs a wave"))
    for key, t in times.items():
        lines.append("  %-34s median %10.1f us   min %10.1f   max %10.1f   spread %8.1f" % (key, statistics.median(t), min(t), max(t), max(t) - min(t)))
    m = {k: statistics.median(t) for k, t in times.items()}
    lines.append("  decode_png / yardstick: %.2fx   (index + decode_png) / yardstick: %.2fx" %
                 (m["decode_png"] / m["inflate_checked (yardstick)"], (m["decode_png"] + m["index (one host sync inside)"]) / m["inflate_checked (yardstick)"]))
    try:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            index()
            png()
            torch.cuda.synchronize()
        steps = {"index": 0.0, "gather + CRC": 0.0, "decode": 0.0, "unfilter + expand": 0.0, "judge (Adler-32, verdicts)": 0.0}
        per = {}
        for ev in prof.key_averages():
            us = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
            n = ev.key
            if not us or "Memcpy" in n or "Memset" in n:
                continue
            step = "index" if "k_png_parse" in n or "k_png_offsets" in n else \
                "gather + CRC" if any(k in n for k in ("k_png_plan", "k_png_list", "k_png_gather", "k_png_crc")) else \
                "unfilter + expand" if "k_png_unfilter" in n or "k_png_expand" in n else \
                "judge (Adler-32, verdicts)" if "k_png_" in n else "decode"
            steps[step] += us
            per[n.split("(")[0][-60:]] = per.get(n.split("(")[0][-60:], 0.0) + us
        lines.append("  steps (kernel time of one profiled repeat, us): " + "; ".join("%s %.1f" % kv for kv in steps.items()))
        lines.append("  unfilter + expand %s the decode step (%.1f us against %.1f us)" %
                     ("costs LESS than" if steps["unfilter + expand"] < steps["decode"] else "costs MORE than", steps["unfilter + expand"], steps["decode"]))
        for n, us in sorted(per.items(), key=lambda kv: -kv[1])[:8]:
            lines.append("    %-62s %10.1f us" % (n, us))
    except Exception as e:                                   # the totals stand without the breakdown
        lines.append("  steps: the profiler gave no kernel times here (%s: %s)" % (type(e).__name__, e))
    return lines


def staged(files):
    import torch
    blob = b"".join(files)
    d = torch.frombuffer(bytearray(blob + bytes(16)), dtype=torch.uint8).cuda()[:len(blob)]
    lens = np.array([len(f) for f in files], np.int64)
    return d, torch.from_numpy(np.cumsum(lens) - lens).cuda(), torch.from_numpy(lens).cuda()


def timed(fns, repeats, warmup):
    """the functions in turn within a repeat -> {name: [us]}"""
    import torch
    times = {k: [] for k in fns}
    for rep in range(warmup + repeats):
        for key, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= warmup:
                times[key].append(e0.elapsed_time(e1) * 1e3)
    return times


def measure_adam7(eng, name, repeats, warmup):
    import torch
    from torch.profiler import profile, ProfilerActivity
    legs = {}
    for key, lace in (("plain", False), ("interlaced", True)):
        files, first = workload(name, lace)
        d, off, ln = staged(files)
        pi = eng.png_index(d, off, ln, interlaced=lace)
        assert (pi.host["status"] == 0).all() and (pi.host["interlace"] == int(lace)).all()
        out, status = eng.decode_png(d, pi)
        assert int((status != 0).sum()) == 0 and out[:len(first)].cpu().numpy().tobytes() == first
        legs[key] = (d, pi, out, sum(len(f) for f in files))
    assert torch.equal(legs["plain"][2], legs["interlaced"][2])           # the same pixels, slot for slot
    fns = {key: (lambda d=d, pi=pi, out=out: eng.decode_png(d, pi, out=out)) for key, (d, pi, out, _) in legs.items()}
    times = timed(fns, repeats, warmup)
    lines = ["workload: %s -- %.1f MB of pixels; %.1f MB of PNG plain, %.1f MB interlaced (raw streams %.1f and %.1f MB)" %
             (name, legs["plain"][1].record.total_out / 1e6, legs["plain"][3] / 1e6, legs["interlaced"][3] / 1e6,
              legs["plain"][1].record.total_raw / 1e6, legs["interlaced"][1].record.total_raw / 1e6)]
    for key, t in times.items():
        lines.append("  decode_png %-12s median %10.1f us   min %10.1f   max %10.1f   runs %s" %
                     (key, statistics.median(t), min(t), max(t), " ".join("%.1f" % x for x in t)))
    lines.append("  interlaced / plain: %.2fx" % (statistics.median(times["interlaced"]) / statistics.median(times["plain"])))
    for key, fn in fns.items():
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        per, rest = {}, 0.0
        for ev in prof.key_averages():
            us = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
            if not us or "Memcpy" in ev.key or "Memset" in ev.key:
                continue
            hit = [k for k in ("k_png_unfilter", "k_png_deinterlace", "k_png_expand") if k in ev.key]
            if hit:
                per[hit[0]] = per.get(hit[0], 0.0) + us
            else:
                rest += us
        lines.append("  kernels, %-12s %s; every other kernel %.1f us" % (key + ":", "; ".join("%s %.1f us" % kv for kv in sorted(per.items())), rest))
    return lines


def retime(engines, name, repeats, warmup):
    """engines: {label: Engine}, each over its own build of the library: decode_png of the same staged files, in turn within a repeat"""
    import torch
    files, first = workload(name)
    d, off, ln = staged(files)
    fns, outs = {}, []
    for label, eng in engines.items():
        pi = eng.png_index(d, off, ln)
        out, status = eng.decode_png(d, pi)
        assert int((status != 0).sum()) == 0 and out[:len(first)].cpu().numpy().tobytes() == first
        outs.append(out)
        fns[label] = lambda eng=eng, pi=pi, out=out: eng.decode_png(d, pi, out=out)
    assert all(torch.equal(o, outs[0]) for o in outs)
    times = timed(fns, repeats, warmup)
    lines = ["retime %s" % name]
    for label, t in times.items():
        lines.append("  %-8s decode_png median %10.1f us   min %10.1f   max %10.1f   runs %s" %
                     (label, statistics.median(t), min(t), max(t), " ".join("%.1f" % x for x in t)))
    if len(times) == 2:
        (la, ta), (lb, tb) = times.items()
        lines.append("  the median of %s %s inside the min-max of %s" % (lb, "LIES" if min(ta) <= statistics.median(tb) <= max(ta) else "does NOT lie", la))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--adam7", action="store_true")
    ap.add_argument("--retime", action="store_true")
    ap.add_argument("--against", default=None, help="--retime: another build of the library, timed in turn with the loaded one in one process")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    import hdl_deflate_amd
    from hdl_deflate_amd import _lib
    eng = hdl_deflate_amd.Engine()
    mode = " --adam7" if args.adam7 else " --retime" if args.retime else ""
    args.out = args.out or os.path.join(ROOT, "profiles", "png_adam7.txt" if args.adam7 else "png_retime.txt" if args.retime else "png.txt")
    lines = ["command: python tools/probe_png.py%s --repeats %d --warmup %d" % (mode, args.repeats, args.warmup)]
    lines += ["library: %s" % os.path.basename(_lib.LIB_PATH)] if mode else \
        ["HDLZ_PNG_LARGE_MIN is HDLZ_ZIP_LARGE_MIN's 16384: the crossover was not re-measured for PNG here."]
    lines.append("")
    engines = {"this": eng}
    if args.against:                                          # (a second handle: its own code object, its own Engine)
        _lib._lib, _lib.LIB_PATH = None, os.path.abspath(args.against)
        engines = {"against": hdl_deflate_amd.Engine(), "this": eng}
        assert engines["against"].lib is not eng.lib
        lines.insert(2, "against: %s, both in one process, call by call in turn" % os.path.basename(args.against))
    for name in ("4096 x 64x64 RGBA", "256 x 512x512 RGB", "1 x 4096x4096 RGBA"):
        if args.only and args.only not in name:
            continue
        if args.adam7:
            lines += measure_adam7(eng, name, args.repeats, args.warmup) + [""]
        elif args.retime:
            lines += retime(engines, name, args.repeats, args.warmup)
        else:
            lines += measure(eng, name, args.repeats, args.warmup) + [""]
        with open(args.out, "w") as f:                        # (kept as far as it got)
            f.write("\n".join(lines) + "\n")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
