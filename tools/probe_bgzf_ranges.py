#!/usr/bin/env python
"""Times of hdlz_bgzf_read_ranges_ws (include/hdlz_bgzf_range.h) against the only route the PARENT commit's library offers to bytes
[p0, p1) of a BGZF file -- hdlz_bgzf_inflate_ws of the whole file, then device copies of the slices --, on the files of
tools/probe_bgzf.py (the four bench families, 2^30 bytes, block = 57344 and block = 2048) -> profiles/bgzf_ranges.txt:

  (pw) parent hdlz_bgzf_inflate_ws, the whole file
  (nw) this commit's hdlz_bgzf_inflate_ws, the whole file: the member decoder gained the task view, its other callers must not pay
  (r1) hdlz_bgzf_read_ranges_ws, ONE range that covers the whole file
  (s)  hdlz_bgzf_read_ranges_ws, 4096 ranges of 256 bytes at seeded random positions
  (ps) the parent's route to the same bytes: (pw), then 4096 device-to-device copies issued from a host loop -- (ps) - (pw) is the
       host's launch rate, not a device slice copy
  (m)  hdlz_bgzf_read_ranges_ws, 4096 ranges of 1 MiB at seeded random positions
  (pm) the parent's route to the same bytes

HIP events around each call, every call in turn within a repeat, median of --repeats after --warmup.  No threshold is set: the
expectations stand next to the numbers.

    python tools/probe_bgzf_ranges.py --parent <libhdlz.so of a build of the parent commit>"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NRANGES = 4096


def _bind(path):
    from hdl_deflate_amd import _lib
    L = ctypes.CDLL(path)
    for t in (_lib.SIGNATURES, _lib.JOIN_SIGNATURES, _lib.UNJOIN_SIGNATURES, _lib.GZIP_SIGNATURES, _lib.BGZF_SIGNATURES):
        for name, (restype, argtypes) in t.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="libhdlz.so of a build of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgzf_ranges.txt"))
    ap.add_argument("--log2-bytes", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import numpy as np
    import torch
    import hdl_deflate_amd
    from hdl_deflate_amd import _lib
    from hdl_deflate_amd.constants import pitch_for
    from hdl_deflate_amd.data import make_blocks
    assert torch.cuda.is_available(), "the probe needs a HIP device: there is nothing to time without one"
    eng = hdl_deflate_amd.Engine()
    L, P = eng.lib, _bind(args.parent)
    assert not hasattr(P, "hdlz_bgzf_read_ranges_ws"), "--parent must be a build of the parent commit"
    st = torch.cuda.current_stream().cuda_stream
    whole = make_blocks((1 << args.log2_bytes) // 2048, 2048, "cuda", seed=5).reshape(-1)
    lines = ["BGZF range reads against the parent commit's route (the whole file, then device copies): the four bench families, %s, median of" %
             torch.cuda.get_device_name(0),
             "%d after %d warm-up repeats, HIP events around each call, ms; every call in turn within a repeat." % (args.repeats, args.warmup),
             "command: python tools/probe_bgzf_ranges.py --parent <libhdlz.so of the parent commit> --log2-bytes %d" % args.log2_bytes, ""]
    for n in (57344, 2048):
        B = whole.numel() // n
        total = B * n
        data = whole[:total]
        pitch = pitch_for(n)
        rows = torch.empty((B, pitch), dtype=torch.uint8, device="cuda")
        out_len, status, crcs = (torch.empty(B, dtype=torch.int32, device="cuda") for _ in range(3))
        fcap = L.hdlz_bgzf_bound(B, n)
        d_file = torch.empty(fcap, dtype=torch.uint8, device="cuda")
        boff = torch.empty(B + 1, dtype=torch.int64, device="cuda")
        bres = torch.zeros(2, dtype=torch.int64, device="cuda")
        jwb = L.hdlz_bgzf_join_work_bytes(B)
        jwork = torch.empty(jwb // 8, dtype=torch.int64, device="cuda")
        assert L.hdlz_crc32_batch_ws(data.data_ptr(), None, n, n, B, crcs.data_ptr(), st) == 0
        assert L.hdlz_compress_batch(data.data_ptr(), None, n, n, B, 32, 10, rows.data_ptr(), pitch, out_len.data_ptr(), status.data_ptr(), st) == 0
        assert L.hdlz_bgzf_join_ws(rows.data_ptr(), pitch, out_len.data_ptr(), status.data_ptr(), None, n, B, crcs.data_ptr(), d_file.data_ptr(),
                                   fcap, boff.data_ptr(), bres.data_ptr(), jwork.data_ptr(), jwb, st) == 0, L.hdlz_last_error()
        br = _lib.BgzfJoinResult.from_buffer_copy(bres.cpu().numpy().tobytes())
        assert br.status == 0
        del rows, jwork
        flen, M = br.file_len, B + 1
        ioff, iout = (torch.empty(M + 1, dtype=torch.int64, device="cuda") for _ in range(2))
        ires = torch.zeros(4, dtype=torch.int64, device="cuda")
        iwb = L.hdlz_bgzf_index_work_bytes(flen)
        iwork = torch.empty(iwb, dtype=torch.uint8, device="cuda")
        assert L.hdlz_bgzf_index_ws(d_file.data_ptr(), flen, M, ioff.data_ptr(), iout.data_ptr(), ires.data_ptr(), iwork.data_ptr(), iwb, st) == 0
        x = _lib.BgzfIndexResult.from_buffer_copy(ires.cpu().numpy().tobytes())
        assert (x.nmembers, x.total_out, x.status) == (M, total, 0)
        back = torch.empty(total, dtype=torch.uint8, device="cuda")
        pres = torch.zeros(3, dtype=torch.int64, device="cuda")
        pwb = P.hdlz_bgzf_inflate_work_bytes(M, 0)
        pwork = torch.empty(pwb, dtype=torch.uint8, device="cuda")
        rng = np.random.default_rng(11)
        batches = {}
        for key, length in (("one", total), ("small", 256), ("large", 1 << 20)):
            R = 1 if key == "one" else NRANGES
            begin = np.zeros(1, np.int64) if key == "one" else rng.integers(0, total - length, R)
            pairs = np.stack([begin, begin + length], axis=1).astype(np.int64)
            d_ranges = torch.from_numpy(pairs).cuda()
            roff = torch.empty(R + 1, dtype=torch.int64, device="cuda")
            rres = torch.zeros(4, dtype=torch.int64, device="cuda")
            swb = L.hdlz_bgzf_ranges_work_bytes(R, 0, 0)
            swork = torch.empty(swb, dtype=torch.uint8, device="cuda")

            def call(out, out_cap, task_cap, work, wb, d_ranges=d_ranges, R=R, roff=roff, rres=rres):
                return L.hdlz_bgzf_read_ranges_ws(d_file.data_ptr(), flen, ioff.data_ptr(), iout.data_ptr(), M, d_ranges.data_ptr(), R, 0,
                                                  out.data_ptr() if out is not None else None, out_cap, roff.data_ptr(), None, task_cap,
                                                  rres.data_ptr(), work.data_ptr(), wb, st)
            assert call(None, 0, 0, swork, swb) == 0, L.hdlz_last_error()              # the sizing call
            rec = _lib.BgzfRangesResult.from_buffer_copy(rres.cpu().numpy().tobytes())
            assert rec.total_out == R * length
            del swork
            wb = L.hdlz_bgzf_ranges_work_bytes(R, rec.ntasks, 0)
            work = torch.empty(wb, dtype=torch.uint8, device="cuda")
            out = torch.empty(rec.total_out, dtype=torch.uint8, device="cuda")
            batches[key] = (pairs.tolist(), rec, out, work, wb, call, rres, length)

        def parent_whole(P=P):
            return P.hdlz_bgzf_inflate_ws(d_file.data_ptr(), flen, ioff.data_ptr(), iout.data_ptr(), M, 0, back.data_ptr(), total, None,
                                          pres.data_ptr(), pwork.data_ptr(), pwb, st)

        def ranges(key):
            pairs, rec, out, work, wb, call, rres, length = batches[key]
            return call(out, rec.total_out, rec.ntasks, work, wb)

        def parent_route(key):
            pairs, rec, out, work, wb, call, rres, length = batches[key]
            rc = parent_whole()
            for k, (a, b) in enumerate(pairs):
                out[k * length:(k + 1) * length].copy_(back[a:b], non_blocking=True)
            return rc
        calls = [("(pw) parent hdlz_bgzf_inflate_ws, the whole file", parent_whole, None),
                 ("(nw) hdlz_bgzf_inflate_ws, the whole file", lambda: parent_whole(L), None),
                 ("(r1) read_ranges, one range = the whole file", lambda: ranges("one"), "one"),
                 ("(s)  read_ranges, 4096 ranges of 256 bytes", lambda: ranges("small"), "small"),
                 ("(ps) parent: the whole file + 4096 copies of 256 bytes", lambda: parent_route("small"), "small"),
                 ("(m)  read_ranges, 4096 ranges of 1 MiB", lambda: ranges("large"), "large"),
                 ("(pm) parent: the whole file + 4096 copies of 1 MiB", lambda: parent_route("large"), "large")]
        times = {k: [] for k, _, _ in calls}
        for rep in range(args.warmup + args.repeats):
            for name, fn, key in calls:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = fn()
                e1.record()
                e1.synchronize()
                assert rc == 0, (name, L.hdlz_last_error())
                if rep >= args.warmup:
                    times[name].append(e0.elapsed_time(e1))
                if rep == 0 and key is not None:                       # the bytes, once: the first and last ranges and 62 between them
                    pairs, rec, out, work, wb, call, rres, length = batches[key]
                    if name.startswith(("(r1)", "(s)", "(m)")):
                        got = _lib.BgzfRangesResult.from_buffer_copy(rres.cpu().numpy().tobytes())
                        assert (got.status, got.total_out, got.ntasks) == (0, rec.total_out, rec.ntasks), (name, got.status, got.first_bad)
                    for k in range(0, len(pairs), max(1, len(pairs) // 64)):
                        assert torch.equal(out[k * length:(k + 1) * length], data[pairs[k][0]:pairs[k][1]]), (name, k)
                    out.zero_()
        med = {k[:4]: statistics.median(v) for k, v in times.items()}
        lines.append("%d members of %d bytes of data and the EOF member, %d bytes of data, file of %d bytes" % (B, n, total, flen))
        for name, _, key in calls:
            v = times[name]
            note = "" if key is None else "   ntasks %d, %d bytes out" % (batches[key][1].ntasks, batches[key][1].total_out)
            lines.append("  %-58s median %9.3f   min %9.3f   max %9.3f%s" % (name, med[name[:4]], min(v), max(v), note))
        lines.append("  (nw) / (pw) = %.3f   (r1) / (pw) = %.3f   (s) / (ps) = %.4f   (m) / (pm) = %.3f   (s) per task %.2f us   (m) per task %.2f us" %
                     (med["(nw)"] / med["(pw)"], med["(r1)"] / med["(pw)"], med["(s) "] / med["(ps)"], med["(m) "] / med["(pm)"],
                      1e3 * med["(s) "] / batches["small"][1].ntasks, 1e3 * med["(m) "] / batches["large"][1].ntasks))
        lines.append("")
        del batches, back, d_file
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
