"""What profiles/seek.txt records (include/hdlz_seek.h): the index call against the plain one-stream read of the same .gz file, the ranged
read through the index against hdlz_bgzf_read_ranges_ws over the same data in 56 KiB members, and the latency of one segment at each
span.  Wall clock around Engine calls with a device synchronisation on either side, median of `--reps`; the Engine paths of both ranged
reads are the same code (Engine._ranged_read), sizing call included.

    python tools/probe_seek.py [--mib 16] [--reps 5]"""
import argparse
import os
import statistics
import sys
import time
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import hdl_deflate_amd  # noqa: E402


def text(n, seed):
    rng = np.random.RandomState(seed)
    vocab = [bytes(rng.randint(97, 123, size=rng.randint(2, 10)).astype(np.uint8)) for _ in range(4000)]
    ids = rng.zipf(1.3, size=n // 4) % len(vocab)
    return b" ".join(vocab[i] for i in ids)[:n]


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out), min(out), max(out), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    E = hdl_deflate_amd.Engine()
    n = a.mib << 20
    data = text(n, 1)
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    z = c.compress(data) + c.flush()
    d_z = torch.from_numpy(np.frombuffer(z, np.uint8).copy()).cuda()
    d_data = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    print("data: %d bytes of text, gzip -6: %d bytes (%.3f)" % (n, len(z), len(z) / n))
    out = torch.empty(n, dtype=torch.uint8, device="cuda")

    # 1. the index call against the plain read (hdlz_gunzip_ws, one stream: the whole-GPU chains)
    plain = timed(lambda: E.inflate_gzip(d_z.reshape(1, -1), out_pitch=n, out=out.reshape(1, -1)), a.reps)
    assert plain[3][2].cpu().tolist() == [0]
    print("plain read  hdlz_gunzip_ws                         %9.2f ms  (min %.2f, max %.2f)  %.2f GB/s of output" % (plain[0], plain[1], plain[2], n / plain[0] / 1e6))
    indexes = {}
    for span in (1 << 16, 1 << 18, 1 << 20):
        cap = n // span + 2
        t = timed(lambda: E.seek_index(d_z, container="gzip", span=span, point_cap=cap, out=out), a.reps)
        _, ix, rec = t[3]
        assert rec.status == 0 and bytes(out.cpu().numpy().tobytes()) == data
        indexes[span] = ix
        print("index call  span %7d: %5d points, max_seg %7d  %9.2f ms  (min %.2f, max %.2f)  ratio to the plain read %.1f"
              % (span, ix.npoints, ix.max_seg, t[0], t[1], t[2], t[0] / plain[0]))

    # 2. ranged reads through the index at span 64 KiB against BGZF ranges over the same data at 56 KiB members
    rng = np.random.RandomState(7)
    small = [(int(p), int(p) + 256) for p in rng.randint(0, n - 256, size=4096)]
    whole = [(0, n)]
    bg = E.compress_bgzf(d_data, block=57344)
    bix = E.bgzf_index(bg)[:2]
    ix = indexes[1 << 16]
    for label, ranges in (("4096 ranges of 256 bytes", small), ("one range over everything", whole)):
        want = b"".join(data[x:y] for x, y in ranges)
        ts = timed(lambda: E.read_seek(d_z, ranges, ix), a.reps)
        tb = timed(lambda: E.read_bgzf(bg, ranges, index=bix), a.reps)
        assert bytes(ts[3][0].cpu().numpy().tobytes()) == want and bytes(tb[3][0].cpu().numpy().tobytes()) == want
        print("%-26s read_seek %9.2f ms (min %.2f, max %.2f)   read_bgzf %9.2f ms (min %.2f, max %.2f)   ratio %.2f"
              % (label, ts[0], ts[1], ts[2], tb[0], tb[1], tb[2], ts[0] / tb[0]))

    # 3. one segment: a one-byte range in the middle of the longest segment, per span
    for span, ix in sorted(indexes.items()):
        pos = ix.pos.cpu().tolist()
        k = max(range(ix.npoints), key=lambda j: pos[j + 1] - pos[j])
        p = (pos[k] + pos[k + 1]) // 2
        t = timed(lambda: E.read_seek(d_z, [(p, p + 1)], ix), a.reps)
        assert bytes(t[3][0].cpu().numpy().tobytes()) == data[p:p + 1]
        print("one segment span %7d: %7d bytes  %8.2f ms  (min %.2f, max %.2f; the sizing call and two host syncs included)"
              % (span, pos[k + 1] - pos[k], t[0], t[1], t[2]))


if __name__ == "__main__":
    main()
