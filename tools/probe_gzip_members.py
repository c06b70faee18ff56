#!/usr/bin/env python
"""Evidence for include/hdlz_gzip_members.h -> profiles/gzip_members.txt (needs the GPU).  HIP events around each call, the calls of a
part in turn within a repeat, median of --repeats after --warmup, spread = max - min over the repeats.  Nothing here is a bar a test
holds: the numbers are recorded.

  1  the index rate: hdlz_gzip_members_index_ws on a file of --index-mib MiB (a BGZF file repeated: real members, real look-alike
     density) against hdlz_crc32_ws on the same buffer in the same run.  Both read every byte once.  Target: index <= 1.25 x CRC.
  2  the index and the read against the BGZF pair on the same BGZF file: the same members, the same decoder -- the difference is the
     cost of having no size field.
  3  Engine.read_gzip_bytes against Engine.inflate_gzip_bytes (the serial loop) on a file of 4096 members; host clock around calls that
     end in a device synchronise, staging included on both sides.
  4  the big_member default: ONE member of S compressed bytes through the wave-per-member read and through the one-stream route
     (hdlz_gunzip_ws, one stream), for S from 512 bytes to 4 MiB -> the span where the two cost the same."""
import argparse
import gzip
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(calls, repeats, warmup):
    import torch
    times = {k: [] for k, _ in calls}
    for rep in range(warmup + repeats):
        for name, fn in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    return times


def line(name, t, nbytes=None):
    med = statistics.median(t)
    s = "  %-44s median %10.1f us   min %10.1f   max %10.1f   spread %8.1f" % (name, med, min(t), max(t), max(t) - min(t))
    return s + ("   %8.1f GB/s" % (nbytes / med / 1e3) if nbytes else "")


def text(n, seed):
    r = np.random.default_rng(seed)
    words = [bytes(r.integers(97, 123, int(k), dtype=np.uint8)) for k in r.integers(2, 10, 4096)]
    out = b" ".join(words[int(i)] for i in r.integers(0, 4096, n // 5 + 16))
    return out[:n]


def main():
    import torch
    from hdl_deflate_amd import Engine, _lib
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gzip_members.txt"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--index-mib", type=int, default=256)
    a = ap.parse_args()
    E = Engine()
    L = E.lib
    st = torch.cuda.current_stream().cuda_stream
    rows = ["hdlz_gzip_members.h on %s; HIP events, median of %d after %d warm-up calls; times in us" % (torch.cuda.get_device_name(0), a.repeats, a.warmup), ""]

    # ---- 1 and 2: a BGZF file
    base = text(64 << 20, 1)
    data = base[:48 << 20]
    d = torch.from_numpy(np.frombuffer(data + bytes(32), np.uint8).copy()).cuda()[:len(data)]
    f = E.compress_bgzf(d)
    n = f.numel()
    boff, bout, brec = E.bgzf_index(f)
    goff, gout, grec = E.gzip_index(f)
    M = int(grec.nmembers)
    same = bool(torch.equal(boff, goff) and torch.equal(bout, gout))
    reps = max(1, (a.index_mib << 20) // n + 1)
    big = f.repeat(reps)
    N = big.numel()
    cap = N // 4096 + 16
    off, out_off = (torch.empty(cap + 1, dtype=torch.int64, device="cuda") for _ in range(2))
    res = torch.zeros(4, dtype=torch.int64, device="cuda")
    wb = L.hdlz_gzip_members_index_work_bytes(N)
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    cw = L.hdlz_crc32_work_bytes(N)
    cwork = torch.empty(max(cw, 256), dtype=torch.uint8, device="cuda")
    crc = torch.zeros(1, dtype=torch.int32, device="cuda")
    bwb = L.hdlz_bgzf_index_work_bytes(N)
    bwork = torch.empty(bwb, dtype=torch.uint8, device="cuda")

    def idx():
        assert L.hdlz_gzip_members_index_ws(big.data_ptr(), N, cap, off.data_ptr(), out_off.data_ptr(), res.data_ptr(), work.data_ptr(), wb, st) == 0

    def crc_pass():
        assert L.hdlz_crc32_ws(big.data_ptr(), N, crc.data_ptr(), cwork.data_ptr(), cw, st) == 0

    def bidx():
        assert L.hdlz_bgzf_index_ws(big.data_ptr(), N, cap, off.data_ptr(), out_off.data_ptr(), res.data_ptr(), bwork.data_ptr(), bwb, st) == 0

    t = timed([("hdlz_gzip_members_index_ws", idx), ("hdlz_crc32_ws", crc_pass), ("hdlz_bgzf_index_ws", bidx)], a.repeats, a.warmup)
    idx()
    rec = _lib.GzipMembersIndexResult.from_buffer_copy(res.cpu().numpy().tobytes()[:24])
    ratio = statistics.median(t["hdlz_gzip_members_index_ws"]) / statistics.median(t["hdlz_crc32_ws"])
    rows += ["1  the index rate: a file of %d bytes (%.1f MiB; %d copies of a BGZF file of %d members), %d candidates found" % (N, N / 2**20, reps, M, rec.nmembers)]
    rows += [line(k, v, N) for k, v in t.items()]
    rows += ["  index / CRC pass = %.3f   (target <= 1.25: %s)" % (ratio, "met" if ratio <= 1.25 else "MISSED"), ""]

    total = int(gout[-1].item())
    out = torch.empty(total, dtype=torch.uint8, device="cuda")
    mst = torch.empty(M, dtype=torch.int32, device="cuda")
    rwb, bwb2 = L.hdlz_gzip_members_inflate_work_bytes(M), L.hdlz_bgzf_inflate_work_bytes(M, 0)
    rwork, bwork2 = torch.empty(rwb, dtype=torch.uint8, device="cuda"), torch.empty(bwb2, dtype=torch.uint8, device="cuda")
    off1, out1 = (torch.empty(M + 1, dtype=torch.int64, device="cuda") for _ in range(2))
    w1 = torch.empty(L.hdlz_gzip_members_index_work_bytes(n), dtype=torch.uint8, device="cuda")
    w2 = torch.empty(L.hdlz_bgzf_index_work_bytes(n), dtype=torch.uint8, device="cuda")

    def gidx1():
        assert L.hdlz_gzip_members_index_ws(f.data_ptr(), n, M, off1.data_ptr(), out1.data_ptr(), res.data_ptr(), w1.data_ptr(), w1.numel(), st) == 0

    def bidx1():
        assert L.hdlz_bgzf_index_ws(f.data_ptr(), n, M, off1.data_ptr(), out1.data_ptr(), res.data_ptr(), w2.data_ptr(), w2.numel(), st) == 0

    def gread():
        assert L.hdlz_gzip_members_inflate_ws(f.data_ptr(), n, goff.data_ptr(), gout.data_ptr(), M, out.data_ptr(), total, mst.data_ptr(), res.data_ptr(),
                                              rwork.data_ptr(), rwb, st) == 0

    def bread():
        assert L.hdlz_bgzf_inflate_ws(f.data_ptr(), n, goff.data_ptr(), gout.data_ptr(), M, 0, out.data_ptr(), total, mst.data_ptr(), res.data_ptr(),
                                      bwork2.data_ptr(), bwb2, st) == 0

    t = timed([("hdlz_gzip_members_index_ws", gidx1), ("hdlz_bgzf_index_ws", bidx1), ("hdlz_gzip_members_inflate_ws", gread), ("hdlz_bgzf_inflate_ws", bread)],
              a.repeats, a.warmup)
    gread()
    ok = int(mst.abs().sum().item()) == 0 and bool(torch.equal(out, d))
    rows += ["2  against the BGZF pair: a BGZF file of %d bytes, %d members, %d bytes of data; the two indexes are %s; the new read verified every member: %s"
             % (n, M, total, "identical" if same else "DIFFERENT", ok)]
    rows += [line(k, v, n if "index" in k else total) for k, v in t.items()] + [""]

    # ---- 3: 4096 members against the serial loop
    r = np.random.default_rng(3)
    members = [gzip.compress(base[int(o):int(o) + int(k)], 6, mtime=0) for o, k in zip(r.integers(0, 60 << 20, 4096), r.integers(2000, 30000, 4096))]
    z = b"".join(members)
    want = gzip.decompress(z)
    ts = {"read_gzip_bytes": [], "inflate_gzip_bytes": []}
    for rep in range(3):
        for name in ts:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = getattr(E, name)(z)
            torch.cuda.synchronize()
            ts[name].append((time.perf_counter() - t0) * 1e6)
            assert got == (0, want), name
    _, report = E.read_gzip(E._stage(z)[:len(z)])
    rows += ["3  against the serial loop: %d members, %d bytes -> %d bytes; host clock, staging and the copy back included, 3 calls each (the first is the warm-up)"
             % (len(members), len(z), len(want))]
    rows += [line(k, v[1:], len(want)) for k, v in ts.items()]
    rows += ["  route: candidates %d, members %d, repairs %d, big %d;  serial / parallel = %.1f" %
             (report.candidates, report.members, report.repairs, report.big,
              statistics.median(ts["inflate_gzip_bytes"][1:]) / statistics.median(ts["read_gzip_bytes"][1:])), ""]

    # ---- 4: one member of S compressed bytes, by its wave and by the one-stream route
    rows += ["4  the big_member default: ONE member of S compressed bytes (level 6 text): the wave-per-member read against Engine.inflate_gzip with one stream",
             "   (the one-stream route as read_gzip takes it: the call, and the host reads of status, length and bytes consumed)"]
    cross = None
    src = base[36 << 20:60 << 20]
    for S in (512, 1024, 2048, 4096, 8192, 16384, 32768, 65536, 131072, 262144, 524288, 1 << 20, 1 << 22):
        raw = src[:int(S * 3.2)]
        m = gzip.compress(raw, 6, mtime=0)
        while len(m) < S and len(raw) < len(src):
            raw = src[:int(len(raw) * 1.1) + 64]
            m = gzip.compress(raw, 6, mtime=0)
        dz = E._stage(m)[:len(m)]
        o1 = torch.tensor([0, len(m)], dtype=torch.int64, device="cuda")
        o2 = torch.tensor([0, len(raw)], dtype=torch.int64, device="cuda")
        o = torch.empty(len(raw), dtype=torch.uint8, device="cuda")
        s1 = torch.empty(1, dtype=torch.int32, device="cuda")
        wk = torch.empty(L.hdlz_gzip_members_inflate_work_bytes(1), dtype=torch.uint8, device="cuda")

        def wave():
            assert L.hdlz_gzip_members_inflate_ws(dz.data_ptr(), len(m), o1.data_ptr(), o2.data_ptr(), 1, o.data_ptr(), len(raw), s1.data_ptr(), res.data_ptr(),
                                                  wk.data_ptr(), wk.numel(), st) == 0

        def one():
            stt, _, used = E._gzip_one(dz, 0, len(raw))
            assert stt == 0 and used == len(m)

        reps_s = 5 if S >= 1 << 20 else 10
        t = timed([("wave", wave), ("one-stream", one)], reps_s, 2)
        wave()
        assert int(s1.item()) == 0
        tw, to = statistics.median(t["wave"]), statistics.median(t["one-stream"])
        rows += ["  S = %8d (%9d bytes out)   wave %10.1f us (spread %7.1f)   one-stream %10.1f us (spread %7.1f)   wave / one-stream %6.2f"
                 % (len(m), len(raw), tw, max(t["wave"]) - min(t["wave"]), to, max(t["one-stream"]) - min(t["one-stream"]), tw / to)]
        if cross is None and tw > to:
            cross = len(m)
    rows += ["  ONE member alone: the wave costs more than the one-stream route from S = %s on.  The waves of a file run side by side, the" % cross,
             "  one-stream calls one behind the other: M members of S bytes are faster by waves while S is below M times that span.",
             "  Engine.GZIP_BIG_MEMBER = %d: the smallest power of two above BGZF's largest member (65536), so that blocked files stay on the wave route" % E.GZIP_BIG_MEMBER, ""]

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(rows) + "\n")
    print("\n".join(rows))


if __name__ == "__main__":
    main()
