#!/usr/bin/env python
"""Times of the BGZF calls (include/hdlz_bgzf.h) against the gzip form of the joined stream as the PARENT commit's library runs it, on
the data of tools/probe_gzip.py (the four bench families), at block = 57344 and block = 2048 -> profiles/bgzf.txt:

  (c)  hdlz_crc32_batch_ws over the input blocks
  (jb) hdlz_bgzf_join_ws alone           against (jg) the parent's hdlz_join_gzip_ws alone
  (wb) the BGZF write: CRC per block + hdlz_compress_batch + join
                                         against (wg) the parent's hdlz_crc32_ws + hdlz_compress_batch_bits + hdlz_join_gzip_ws
  (ix) hdlz_bgzf_index_ws
  (rb) hdlz_bgzf_inflate_ws              against (ug) the parent's hdlz_unjoin_gzip_ws with HDLZ_INFLATE_WAVE_PER_STREAM: the same decoder
                                         (one wave per member) runs on both sides

HIP events around each call, every call in turn within a repeat, median of --repeats after --warmup.  No threshold is set: the
expectations stand next to the numbers.

    python tools/probe_bgzf.py --parent <libhdlz.so of a build of the parent commit>"""
import argparse
import ctypes
import gzip
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WAVE = 4


def _bind(path):
    from hdl_deflate_amd import _lib
    L = ctypes.CDLL(path)
    for t in (_lib.SIGNATURES, _lib.JOIN_SIGNATURES, _lib.UNJOIN_SIGNATURES, _lib.GZIP_SIGNATURES):
        for name, (restype, argtypes) in t.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="libhdlz.so of a build of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgzf.txt"))
    ap.add_argument("--log2-bytes", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    import hdl_deflate_amd
    from hdl_deflate_amd import _lib
    from hdl_deflate_amd.constants import pitch_for
    from hdl_deflate_amd.data import make_blocks
    assert torch.cuda.is_available(), "the probe needs a HIP device: there is nothing to time without one"
    eng = hdl_deflate_amd.Engine()
    L, P = eng.lib, _bind(args.parent)
    assert not hasattr(P, "hdlz_bgzf_join_ws"), "--parent must be a build of the parent commit"
    st = torch.cuda.current_stream().cuda_stream
    whole = make_blocks((1 << args.log2_bytes) // 2048, 2048, "cuda", seed=5).reshape(-1)
    lines = ["BGZF against the gzip form of the joined stream (the parent commit's library): the four bench families, %s, median of %d after %d" %
             (torch.cuda.get_device_name(0), args.repeats, args.warmup),
             "warm-up repeats, HIP events around each call, ms; every call in turn within a repeat.",
             "command: python tools/probe_bgzf.py --parent <libhdlz.so of the parent commit> --log2-bytes %d" % args.log2_bytes, ""]
    for n in (57344, 2048):
        B = whole.numel() // n
        total = B * n
        data = whole[:total]
        pitch = pitch_for(n)
        rows = torch.empty((B, pitch), dtype=torch.uint8, device="cuda")
        out_len, status, crcs = (torch.empty(B, dtype=torch.int32, device="cuda") for _ in range(3))
        bits = torch.empty(B, dtype=torch.int64, device="cuda")
        crc1 = torch.zeros(1, dtype=torch.int32, device="cuda")
        cwb = P.hdlz_crc32_work_bytes(total)
        cwork = torch.empty(cwb // 4, dtype=torch.int32, device="cuda")
        bcap, gcap = L.hdlz_bgzf_bound(B, n), P.hdlz_join_gzip_bound(B, n)
        bdst, gdst = torch.empty(bcap, dtype=torch.uint8, device="cuda"), torch.empty(gcap, dtype=torch.uint8, device="cuda")
        boff, goff = (torch.empty(B + 1, dtype=torch.int64, device="cuda") for _ in range(2))
        bres, gres = (torch.zeros(2, dtype=torch.int64, device="cuda") for _ in range(2))
        jwb = L.hdlz_bgzf_join_work_bytes(B)
        jwork = torch.empty(jwb // 8, dtype=torch.int64, device="cuda")
        back = torch.empty(total, dtype=torch.uint8, device="cuda")
        ures, rres = (torch.zeros(3, dtype=torch.int64, device="cuda") for _ in range(2))
        uwb = P.hdlz_unjoin_gzip_work_bytes(B, total, WAVE)
        uwork = torch.empty(uwb, dtype=torch.uint8, device="cuda")
        M = B + 1                                                      # the members of the file: the blocks and the EOF member
        ioff, iout = (torch.empty(M + 1, dtype=torch.int64, device="cuda") for _ in range(2))
        ires = torch.zeros(4, dtype=torch.int64, device="cuda")
        rwb = L.hdlz_bgzf_inflate_work_bytes(M, 0)
        rwork = torch.empty(rwb, dtype=torch.uint8, device="cuda")
        lens = {}
        crc_b = lambda: L.hdlz_crc32_batch_ws(data.data_ptr(), None, n, n, B, crcs.data_ptr(), st)
        crc_g = lambda: P.hdlz_crc32_ws(data.data_ptr(), total, crc1.data_ptr(), cwork.data_ptr(), cwb, st)
        comp_b = lambda: L.hdlz_compress_batch(data.data_ptr(), None, n, n, B, 32, 10, rows.data_ptr(), pitch, out_len.data_ptr(), status.data_ptr(), st)
        comp_g = lambda: P.hdlz_compress_batch_bits(data.data_ptr(), None, n, n, B, 32, 10, rows.data_ptr(), pitch, out_len.data_ptr(),
                                                    status.data_ptr(), bits.data_ptr(), st)
        join_b = lambda: L.hdlz_bgzf_join_ws(rows.data_ptr(), pitch, out_len.data_ptr(), status.data_ptr(), None, n, B, crcs.data_ptr(),
                                             bdst.data_ptr(), bcap, boff.data_ptr(), bres.data_ptr(), jwork.data_ptr(), jwb, st)
        join_g = lambda: P.hdlz_join_gzip_ws(rows.data_ptr(), pitch, out_len.data_ptr(), bits.data_ptr(), status.data_ptr(), None, n, B,
                                             crc1.data_ptr(), gdst.data_ptr(), gcap, goff.data_ptr(), gres.data_ptr(), jwork.data_ptr(), jwb, st)

        def index():
            iwb = L.hdlz_bgzf_index_work_bytes(lens["b"])
            return L.hdlz_bgzf_index_ws(bdst.data_ptr(), lens["b"], M, ioff.data_ptr(), iout.data_ptr(), ires.data_ptr(), lens["iwork"].data_ptr(), iwb, st)

        def read_b():
            return L.hdlz_bgzf_inflate_ws(bdst.data_ptr(), lens["b"], ioff.data_ptr(), iout.data_ptr(), M, 0, back.data_ptr(), total, None,
                                          rres.data_ptr(), rwork.data_ptr(), rwb, st)

        def read_g():
            return P.hdlz_unjoin_gzip_ws(gdst.data_ptr(), lens["g"], goff.data_ptr(), None, n, B, WAVE, back.data_ptr(), total, None,
                                         ures.data_ptr(), uwork.data_ptr(), uwb, st)
        # both files once, in front of the timed repeats (the gzip join needs the end bits: its rows come from the _bits call)
        assert crc_b() == 0 and comp_b() == 0 and join_b() == 0, L.hdlz_last_error()
        br = _lib.BgzfJoinResult.from_buffer_copy(bres.cpu().numpy().tobytes())
        assert crc_g() == 0 and comp_g() == 0 and join_g() == 0, P.hdlz_last_error()
        gr = _lib.JoinGzipResult.from_buffer_copy(gres.cpu().numpy().tobytes())
        assert br.status == 0 and gr.status == 0, (br.status, br.first_bad, gr.status)
        lens["b"], lens["g"] = br.file_len, gr.stream_len
        lens["iwork"] = torch.empty(L.hdlz_bgzf_index_work_bytes(br.file_len) // 8, dtype=torch.int64, device="cuda")
        head = bdst[:min(br.file_len, 1 << 22)].cpu().numpy().tobytes()
        head = head[:head.rfind(b"\x1f\x8b\x08\x04")]                   # whole members only
        assert gzip.decompress(head) == data[:len(gzip.decompress(head))].cpu().numpy().tobytes()
        calls = [("(c)  hdlz_crc32_batch_ws", crc_b),
                 ("(cg) parent hdlz_crc32_ws", crc_g),
                 ("(jg) parent hdlz_join_gzip_ws", join_g),
                 ("(wg) parent CRC + compress_bits + gzip join", lambda: crc_g() or comp_g() or join_g()),
                 ("(ug) parent hdlz_unjoin_gzip_ws, wave per member", read_g),
                 ("(wb) BGZF write: CRC + compress + join", lambda: crc_b() or comp_b() or join_b()),
                 ("(jb) hdlz_bgzf_join_ws", join_b),
                 ("(ix) hdlz_bgzf_index_ws", index),
                 ("(rb) hdlz_bgzf_inflate_ws", read_b)]
        times = {k: [] for k, _ in calls}
        for rep in range(args.warmup + args.repeats):
            for name, fn in calls:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = fn()
                e1.record()
                e1.synchronize()
                assert rc == 0, (name, L.hdlz_last_error())
                if rep >= args.warmup:
                    times[name].append(e0.elapsed_time(e1))
                if rep == 0 and name.startswith("(ix)"):
                    x = _lib.BgzfIndexResult.from_buffer_copy(ires.cpu().numpy().tobytes())
                    assert (x.nmembers, x.total_out, x.file_used, x.status, x.eof_marker) == (M, total, br.file_len, 0, 1), (x.nmembers, x.status)
                    assert torch.equal(ioff[:M], boff)
                if rep == 0 and name.startswith(("(rb)", "(ug)")):
                    u = _lib.UnjoinGzipResult.from_buffer_copy((rres if name.startswith("(rb)") else ures).cpu().numpy().tobytes())
                    assert (u.status, u.out_len) == (0, total), (name, u.status, u.first_bad)
                    assert torch.equal(back, data)
                    back.zero_()
        med = {k[:4]: statistics.median(v) for k, v in times.items()}
        lines.append("%d blocks of %d bytes (rows of %d), %d bytes of input: BGZF file %d bytes (ratio %.4f), gzip stream %d bytes" %
                     (B, n, pitch, total, br.file_len, br.file_len / total, gr.stream_len))
        for k, _ in calls:
            v = times[k]
            lines.append("  %-50s median %8.3f   min %8.3f   max %8.3f   %8.1f GB/s of input" % (k, med[k[:4]], min(v), max(v), total / med[k[:4]] / 1e6))
        lines.append("  (jb) / (jg) = %.3f   (wb) / (wg) = %.3f   (ix) / (rb) = %.3f   (rb) / (ug) = %.3f   (c) / (cg) = %.3f" %
                     (med["(jb)"] / med["(jg)"], med["(wb)"] / med["(wg)"], med["(ix)"] / med["(rb)"], med["(rb)"] / med["(ug)"], med["(c) "] / med["(cg)"]))
        lines.append("")
        del rows, bdst, gdst, back
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
