#!/usr/bin/env python
"""Evidence for hdlz_tiff_index_ws / hdlz_tiff_decode_ws (include/hdlz_tiff.h) -> profiles/tiff.txt: the total of Engine.decode_tiff and
the time per step (plan, decode, Adler-32 and verdicts, unpredict) on four workloads, next to the yardstick -- the checked inflate
(Engine.inflate_checked) over the same zlib payloads, the chunks, already laid out as a batch -- and the kernel time of
k_tiff_unpredict next to a device-to-device copy of the same decoded bytes.

  4096 images of 64 x 64 RGBA, one strip each            (64 distinct ones, each 64 times), predictor 2
  256 images of 512 x 512 RGB in 128 x 128 tiles         (16 distinct ones, each 16 times), predictor 2
  one 4096 x 4096 float32 image in 256 x 256 tiles       predictor 3, and the same pixels with predictor 2

Totals: HIP events around the calls (no host sync inside), decode_tiff and the yardstick in turn within a repeat, median of --repeats
after --warmup.  Steps: the kernels of one more repeat, profiler on (torch.profiler, device activity), summed by kernel name; the
profiled pass is not timed."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import tiff_ref as T      # noqa: E402
from probe_png import picture, staged, timed      # noqa: E402


def surface(n, seed):
    """a smooth float32 surface plus a little noise: an elevation model's kind of data"""
    y, x = np.mgrid[0:n, 0:n].astype(np.float32)
    r = np.random.default_rng(seed)
    return (1000.0 + 300.0 * np.sin(x / 97.0) * np.cos(y / 131.0) + 0.01 * x + r.normal(0.0, 0.05, (n, n))).astype(np.float32)


def workload(name):
    if name == "4096 x 64x64 RGBA, one strip":
        pages = [dict(pix=np.frombuffer(picture(64, 64, 4, k), np.uint8).reshape(64, 64, 4), predictor=2) for k in range(64)]
        times = 64
    elif name == "256 x 512x512 RGB, 128x128 tiles":
        pages = [dict(pix=np.frombuffer(picture(512, 512, 3, k), np.uint8).reshape(512, 512, 3), predictor=2, tile=(128, 128)) for k in range(16)]
        times = 16
    else:
        pages = [dict(pix=surface(4096, 1), predictor=3 if "predictor 3" in name else 2, tile=(256, 256))]
        times = 1
    files = [T.make_tiff([pg]) for pg in pages]
    return files * times, pages[0]["pix"].tobytes(), len(files)


def measure(eng, name, repeats, warmup):
    import torch
    from torch.profiler import profile, ProfilerActivity
    files, first, nd = workload(name)
    d, off, ln = staged(files)
    ti = eng.tiff_index(d, off, ln)
    h = ti.host
    assert (h["status"] == 0).all()
    out, status = eng.decode_tiff(d, ti)
    assert int((status != 0).sum()) == 0 and out[:len(first)].cpu().numpy().tobytes() == first
    # the yardstick's input: every chunk's zlib stream, back to back, and their ragged index
    zs = []
    for f in files[:nd]:
        rec = T.index([f])["images"][0]
        zs += [f[o:o + n] for o, n in (T.chunk_words(f, rec, k) for k in range(rec["nchunks"]))]
    zs = zs * (len(files) // nd)
    zoff = np.concatenate([[0], np.cumsum([len(z) for z in zs])]).astype(np.int64)
    dz = torch.frombuffer(bytearray(b"".join(zs) + bytes(64)), dtype=torch.uint8).cuda()
    dzo = torch.from_numpy(zoff).cuda()
    full = int((h["tile_w"].astype(np.int64) * h["tile_h"] * h["samples"] * (h["bits"] // 8)).max())
    pitch = (full + 3) & ~3
    zmax = int(max(len(z) for z in zs))
    yout = torch.empty((len(zs), pitch), dtype=torch.uint8, device="cuda")
    ywork = torch.empty(eng.lib.hdlz_inflate_checked_work_bytes(len(zs), zmax, pitch, 0, 1), dtype=torch.uint8, device="cuda")
    raw = torch.empty(int(ti.record.total_raw), dtype=torch.uint8, device="cuda")
    raw2 = torch.empty_like(raw)
    fns = {"decode_tiff": lambda: eng.decode_tiff(d, ti, out=out),
           "inflate_checked (yardstick)": lambda: eng.inflate_checked(dz, in_off=dzo, in_len=zmax, out_pitch=pitch, out=yout, work=ywork),
           "copy of the decoded bytes": lambda: raw2.copy_(raw)}
    assert int((fns["inflate_checked (yardstick)"]()[2] != 0).sum()) == 0
    times = timed(fns, repeats, warmup)
    m = {k: statistics.median(t) for k, t in times.items()}
    lines = ["workload: %s -- %d files, %d chunks, %.1f MB of TIFF, %.1f MB of zlib streams, %.1f MB decoded, %.1f MB of pixels" %
             (name, len(files), len(zs), d.numel() / 1e6, zoff[-1] / 1e6, ti.record.total_raw / 1e6, ti.record.total_out / 1e6)]
    for key, t in times.items():
        lines.append("  %-34s median %10.1f us   min %10.1f   max %10.1f   spread %8.1f" % (key, m[key], min(t), max(t), max(t) - min(t)))
    lines.append("  decode_tiff / yardstick: %.2fx" % (m["decode_tiff"] / m["inflate_checked (yardstick)"]))
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fns["decode_tiff"]()
        torch.cuda.synchronize()
    steps = {"plan": 0.0, "decode": 0.0, "unpredict": 0.0, "judge (Adler-32, verdicts)": 0.0}
    per = {}
    for ev in prof.key_averages():
        us = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
        n = ev.key
        if not us or "Memcpy" in n or "Memset" in n:
            continue
        step = "plan" if "k_tiff_plan" in n or "k_tiff_chunks" in n else "unpredict" if "k_tiff_unpredict" in n else \
            "judge (Adler-32, verdicts)" if "k_tiff_" in n else "decode"
        steps[step] += us
        per[n.split("(")[0][-60:]] = per.get(n.split("(")[0][-60:], 0.0) + us
    lines.append("  steps (kernel time of one profiled repeat, us): " + "; ".join("%s %.1f" % kv for kv in steps.items()))
    lines.append("  k_tiff_unpredict %.1f us = %.1f %% of the decode step (%.1f us); the copy of the same %.1f MB: %.1f us (%.2fx)" %
                 (steps["unpredict"], 100.0 * steps["unpredict"] / max(steps["decode"], 1e-9), steps["decode"], raw.numel() / 1e6,
                  m["copy of the decoded bytes"], steps["unpredict"] / m["copy of the decoded bytes"]))
    for n, us in sorted(per.items(), key=lambda kv: -kv[1])[:8]:
        lines.append("    %-62s %10.1f us" % (n, us))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiff.txt"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    import hdl_deflate_amd
    eng = hdl_deflate_amd.Engine()
    lines = ["command: python tools/probe_tiff.py --repeats %d --warmup %d" % (args.repeats, args.warmup),
             "HDLZ_TIFF_LARGE_MIN is HDLZ_PNG_LARGE_MIN's 16384: the crossover was not re-measured for TIFF here.", ""]
    for name in ("4096 x 64x64 RGBA, one strip", "256 x 512x512 RGB, 128x128 tiles", "1 x 4096x4096 float32, 256x256 tiles, predictor 3",
                 "1 x 4096x4096 float32, 256x256 tiles, predictor 2"):
        if args.only and args.only not in name:
            continue
        lines += measure(eng, name, args.repeats, args.warmup) + [""]
        with open(args.out, "w") as f:                        # (kept as far as it got)
            f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
