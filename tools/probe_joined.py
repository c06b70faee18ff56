#!/usr/bin/env python
"""Times the joined-stream path against the calls it is built from, on one GPU:
    (a) hdlz_compress_batch          (b) hdlz_compress_batch_bits
    (c) hdlz_archive_batch_ws        (d) hdlz_join_batch_ws          -- (c) and (d) on the rows of (b)
for two shapes of the same 2 GiB: 2^20 blocks of 2 KiB (BASELINE configs[1]) and 2^15 blocks of 64 KiB.  HIP events around every
call, the four calls in turn within a repeat (so drift hits all of them alike), warm-up repeats first (code objects, first touch of
every buffer), median of the timed repeats; the spread of a call is stated from the same repeats.  Writes the table to --out.

Yardsticks (both are existing code in the same run): (d) within 15 % of (c) -- the join moves the same bytes plus at most 5 per row,
reads one trailer per row and has a second small launch --, and (b) within the run-to-run spread of (a)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hdl_deflate_amd                                         # noqa: E402
from hdl_deflate_amd.constants import pitch_for               # noqa: E402
from hdl_deflate_amd.data import make_blocks                  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "joined_stream.txt"))
    ap.add_argument("--log2-bytes", type=int, default=31)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a HIP device: there is nothing to time without one"
    eng = hdl_deflate_amd.Engine()
    L = eng.lib
    total = 1 << args.log2_bytes
    data = make_blocks(total // 2048, 2048, "cuda", seed=5)
    st = torch.cuda.current_stream().cuda_stream
    lines = ["joined stream: %d bytes of the four bench families, %s, median of %d after %d warm-up repeats, HIP events, ms" %
             (total, torch.cuda.get_device_name(0), args.repeats, args.warmup), ""]
    for n in (2048, 65536):
        B, pitch = total // n, pitch_for(n)
        rows = torch.empty((B, pitch), dtype=torch.uint8, device="cuda")
        out_len, status = (torch.empty(B, dtype=torch.int32, device="cuda") for _ in range(2))
        bits = torch.empty(B, dtype=torch.int64, device="cuda")
        cap = L.hdlz_join_bound(B, n)
        dst = torch.empty(cap, dtype=torch.uint8, device="cuda")           # archive and stream in turn: the same destination
        off = torch.empty(B + 1, dtype=torch.int64, device="cuda")
        res = torch.empty(2, dtype=torch.int64, device="cuda")
        wb = max(L.hdlz_archive_work_bytes(B), L.hdlz_join_work_bytes(B))
        work = torch.empty(wb // 8, dtype=torch.int64, device="cuda")
        calls = {
            "(a) hdlz_compress_batch": lambda: L.hdlz_compress_batch(data.data_ptr(), None, n, n, B, 32, 10, rows.data_ptr(), pitch,
                                                                     out_len.data_ptr(), status.data_ptr(), st),
            "(b) hdlz_compress_batch_bits": lambda: L.hdlz_compress_batch_bits(data.data_ptr(), None, n, n, B, 32, 10, rows.data_ptr(), pitch,
                                                                               out_len.data_ptr(), status.data_ptr(), bits.data_ptr(), st),
            "(c) hdlz_archive_batch_ws": lambda: L.hdlz_archive_batch_ws(rows.data_ptr(), pitch, out_len.data_ptr(), B, dst.data_ptr(), cap,
                                                                         off.data_ptr(), work.data_ptr(), wb, st),
            "(d) hdlz_join_batch_ws": lambda: L.hdlz_join_batch_ws(rows.data_ptr(), pitch, out_len.data_ptr(), bits.data_ptr(),
                                                                   status.data_ptr(), None, n, B, dst.data_ptr(), cap, off.data_ptr(),
                                                                   res.data_ptr(), work.data_ptr(), wb, st),
        }
        times = {k: [] for k in calls}
        for rep in range(args.warmup + args.repeats):
            for name, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = fn()
                e1.record()
                e1.synchronize()
                assert rc == 0, (name, L.hdlz_last_error())
                if rep >= args.warmup:
                    times[name].append(e0.elapsed_time(e1))
        rec = hdl_deflate_amd._lib.JoinResult.from_buffer_copy(res.cpu().numpy().tobytes())
        assert rec.status == 0 and int(status.max()) == 0, (rec.status, int(status.max()))
        med = {k: statistics.median(v) for k, v in times.items()}
        lines.append("%d blocks of %d bytes (rows of %d): joined stream %d bytes, ratio %.4f" % (B, n, pitch, rec.stream_len, rec.stream_len / total))
        for k, v in times.items():
            lines.append("  %-30s median %8.3f   min %8.3f   max %8.3f   %7.1f GB/s of input" % (k, med[k], min(v), max(v), total / med[k] / 1e6))
        a, b, c, d = (med[k] for k in calls)
        spread = (max(times["(a) hdlz_compress_batch"]) - min(times["(a) hdlz_compress_batch"])) / a
        lines.append("  (d) / (c) = %.3f   (yardstick: <= 1.15)" % (d / c))
        lines.append("  (b) / (a) = %.4f   ((a)'s own spread over its repeats, (max - min) / median: %.4f)" % (b / a, spread))
        lines.append("")
        del rows, dst
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
