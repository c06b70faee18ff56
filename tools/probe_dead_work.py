#!/usr/bin/env python3
"""per-input time of the one-tile compress kernel (hdlz_compress_batch, CWINDOW 32, MATCH10, 2^18 blocks of 2 KiB, HIP events) for the
library named in HDLZ_LIB: each bench family alone, 2 KiB Zipf text and all-digit blocks.  The kernel skips bit planes that are constant
and tiles without a match candidate, so its time depends on the data: run it for libhdlz.so, libhdlz_alllive.so and a
parent build and set the lines side by side.
usage: HDLZ_LIB=hdl_deflate_amd/lib/libhdlz_X.so tools/probe_dead_work.py [nblocks]"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from hdl_deflate_amd import Engine
from hdl_deflate_amd.data import make_blocks, make_text_blocks

NB = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 18
N = 2048
e = Engine()


def timed(d, reps=8):
    out, ol, st = e.compress_batch(d, cwindow=32, maxmatch=10)
    for _ in range(2):
        e.compress_batch(d, cwindow=32, maxmatch=10, out=out)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _, ol, st = e.compress_batch(d, cwindow=32, maxmatch=10, out=out)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    assert int(st.max().item()) == 0
    return sum(ms) / len(ms), min(ms), max(ms), float(ol.sum().item()) / d.numel()


inputs = [("family %d" % f, lambda f=f: make_blocks(NB, N, "cuda", seed=3, families=(f,))) for f in (1, 2, 3, 4)]
inputs.append(("families 1-4", lambda: make_blocks(NB, N, "cuda", seed=3)))
inputs.append(("zipf text", lambda: make_text_blocks(NB, N, "cuda", seed=3)))
inputs.append(("digits", lambda: (torch.randint(0, 10, (NB, N), device="cuda", dtype=torch.int32) + 48).to(torch.uint8)))
print("library %s, %d blocks of %d bytes" % (os.environ.get("HDLZ_LIB", "(default)"), NB, N))
for name, make in inputs:
    d = make()
    avg, lo, hi, ratio = timed(d)
    print("%-14s %7.3f ms  (min %7.3f max %7.3f)  %6.1f GB/s  ratio %.3f" % (name, avg, lo, hi, d.numel() / avg / 1e6, ratio), flush=True)
    del d
    torch.cuda.empty_cache()
