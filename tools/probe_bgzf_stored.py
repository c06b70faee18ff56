#!/usr/bin/env python
"""Evidence for hdlz_bgzf_join_stored_ws (include/hdlz_bgzf_stored.h) -> profiles/bgzf_stored.txt, one sub-command per part; each
replaces its own sections of --out and leaves the others:

  codeobj --parent OBJDIR   (no GPU) section 1: the code objects of hdlz_join.hip's five kernels in a build of the parent commit (its
                            csrc/_obj) beside this build's -- names, the six resource fields, the instruction sequences -- and the
                            resources of the two new kernels of hdlz_bgzf_stored.hip.
  time --parent LIB         sections 2 to 5, on the 1 GiB inputs of profiles/bgzf.txt (the four bench families) and on random bytes;
                            HIP events around each call, every call in turn within a repeat, median of --repeats after --warmup:
                            2. THE ONE BAR: on the all-compressible inputs (57344-byte and 2 KiB blocks) hdlz_bgzf_join_stored_ws
                               against the PARENT library's hdlz_bgzf_join_ws from the same rows; the files must be identical; the
                               allowed excess is the larger of the two calls' own spreads (min to max over the repeats)
                            3. without a bar: the join alone and the whole write (CRC + compress + join) for random bytes and for a
                               half-and-half input at 65280-byte blocks
                            4. without a bar: hdlz_bgzf_inflate_ws of the all-stored file against the all-fixed 57344-byte file
                            5. file sizes: the older writer at 57344 against this one at 65280

  framing --parent LIB      the bar of section 2 for a change that leaves every entry point's bytes alone: hdlz_join_batch_ws,
                            hdlz_bgzf_join_ws and hdlz_bgzf_join_stored_ws of this build against the same call of the PARENT library,
                            at section 2's two shapes, from the same rows; both sides' outputs must be identical.  Writes
                            section 2 of profiles/framing_shared.txt (or --out).

    python tools/probe_bgzf_stored.py codeobj --parent <csrc/_obj of a build of the parent commit>
    python tools/probe_bgzf_stored.py time --parent <libhdlz.so of a build of the parent commit>
    python tools/probe_bgzf_stored.py framing --parent <libhdlz.so of a build of the parent commit>"""
import argparse
import ctypes
import gzip
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from probe_unjoin import FIELDS, code_tag, kernels_of, put_section      # noqa: E402

OLD_KERNELS = ("hdlz::k_join<false>", "hdlz::k_join<true>", "hdlz::k_join_finish", "hdlz::k_join_gzip_finish", "hdlz::k_bgzf_join_finish")


def cmd_codeobj(args):
    new_dir = os.path.join(ROOT, "hdl_deflate_amd", "csrc", "_obj")
    old = kernels_of(os.path.join(args.parent, "hdlz_join.o"))
    new = kernels_of(os.path.join(new_dir, "hdlz_join.o"))
    fmt = lambda v: " ".join("%d" % v[f] for f in FIELDS)
    lines = ["code-object metadata, parent build | this build (%s)" % ", ".join(f[1:] for f in FIELDS),
             "command: python tools/probe_bgzf_stored.py codeobj --parent <csrc/_obj of a build of the parent commit>", "", "hdlz_join:"]
    differ = 0
    assert sorted(old) == sorted(OLD_KERNELS), sorted(old)
    for name in sorted(set(old) | set(new)):
        o, n = old.get(name), new.get(name)
        tag = "NEW" if o is None else "MISSING" if n is None else "same" if fmt(o) == fmt(n) else "DIFFERS"
        code = code_tag(o["code"], n["code"]) if o and n else ""
        differ += tag != "same" or code.startswith("differs")
        lines.append("  %-34s %-24s | %-24s %s%s" % (name, fmt(o) if o else "-", fmt(n) if n else "-", tag, code and "; " + code))
    lines += ["", "existing kernels that differ, are missing or have company in their file: %d" % differ, "", "hdlz_bgzf_stored (new):"]
    for name, k in sorted(kernels_of(os.path.join(new_dir, "hdlz_bgzf_stored.o")).items()):
        lines.append("  %-34s VGPRs %d, SGPRs %d, scratch %d bytes, spilled %d + %d, LDS %d bytes, %d instructions" %
                     (name, k[".vgpr_count"], k[".sgpr_count"], k[".private_segment_fixed_size"], k[".vgpr_spill_count"], k[".sgpr_spill_count"],
                      k[".group_segment_fixed_size"], len(k["code"])))
    put_section(args.out, "1. code objects: the existing join kernels against the parent build, the new kernels (no GPU)", lines)
    return 1 if differ else 0


def _bind(path):
    from hdl_deflate_amd import _lib
    L = ctypes.CDLL(path)
    for t in (_lib.SIGNATURES, _lib.JOIN_SIGNATURES, _lib.UNJOIN_SIGNATURES, _lib.GZIP_SIGNATURES, _lib.BGZF_SIGNATURES, _lib.BGZF_STORED_SIGNATURES):
        for name, (restype, argtypes) in t.items():
            if not hasattr(L, name):                            # (a parent older than the stored writer)
                continue
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
    return L


class Batch(object):
    """`data` cut into B blocks of n bytes: CRC words and rows (this build's library), and room for both joins"""

    def __init__(self, L, data, n):
        import torch
        from hdl_deflate_amd.constants import pitch_for
        self.L, self.n, self.B = L, n, data.numel() // n
        B = self.B
        self.total = B * n
        self.data = data[:self.total]
        self.pitch = pitch_for(n)
        self.st = torch.cuda.current_stream().cuda_stream
        self.rows = torch.empty((B, self.pitch), dtype=torch.uint8, device="cuda")
        self.out_len, self.status, self.crcs = (torch.empty(B, dtype=torch.int32, device="cuda") for _ in range(3))
        self.cap = max(L.hdlz_bgzf_bound(B, n), L.hdlz_bgzf_stored_bound(B, n))
        self.file, self.old_file = (torch.zeros(self.cap, dtype=torch.uint8, device="cuda") for _ in range(2))
        self.off, self.old_off = (torch.empty(B + 1, dtype=torch.int64, device="cuda") for _ in range(2))
        self.res, self.old_res = torch.zeros(3, dtype=torch.int64, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda")
        self.wb = L.hdlz_bgzf_join_stored_work_bytes(B)
        self.work = torch.empty(self.wb // 8, dtype=torch.int64, device="cuda")

    def crc(self):
        return self.L.hdlz_crc32_batch_ws(self.data.data_ptr(), None, self.n, self.n, self.B, self.crcs.data_ptr(), self.st)

    def compress(self):
        return self.L.hdlz_compress_batch(self.data.data_ptr(), None, self.n, self.n, self.B, 32, 10, self.rows.data_ptr(), self.pitch,
                                          self.out_len.data_ptr(), self.status.data_ptr(), self.st)

    def join_stored(self):
        return self.L.hdlz_bgzf_join_stored_ws(self.data.data_ptr(), None, self.n, self.n, self.rows.data_ptr(), self.pitch, self.out_len.data_ptr(),
                                               self.status.data_ptr(), self.B, self.crcs.data_ptr(), self.file.data_ptr(), self.cap, self.off.data_ptr(),
                                               None, self.res.data_ptr(), self.work.data_ptr(), self.wb, self.st)

    def join_older(self, lib):
        return lib.hdlz_bgzf_join_ws(self.rows.data_ptr(), self.pitch, self.out_len.data_ptr(), self.status.data_ptr(), None, self.n, self.B,
                                     self.crcs.data_ptr(), self.old_file.data_ptr(), self.cap, self.old_off.data_ptr(), self.old_res.data_ptr(),
                                     self.work.data_ptr(), self.wb, self.st)

    def record(self):
        from hdl_deflate_amd import _lib
        return _lib.BgzfStoredResult.from_buffer_copy(self.res.cpu().numpy().tobytes())

    def check_head(self):
        """the first members of the file through Python's gzip"""
        head = self.file[:min(self.record().file_len, 1 << 21)].cpu().numpy().tobytes()
        head = head[:head.rfind(b"\x1f\x8b\x08\x04")]                   # whole members only
        back = gzip.decompress(head)
        assert len(back) >= self.n and back == self.data[:len(back)].cpu().numpy().tobytes()


def timed(calls, repeats, warmup, last_error):
    import torch
    times = {k: [] for k, _ in calls}
    for rep in range(warmup + repeats):
        for name, fn in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn()
            e1.record()
            e1.synchronize()
            assert rc == 0, (name, last_error())
            if rep >= warmup:
                times[name].append(e0.elapsed_time(e1))
    return times


def row(name, v, total):
    med = statistics.median(v)
    return "  %-52s median %8.3f   min %8.3f   max %8.3f   %8.1f GB/s of input" % (name, med, min(v), max(v), total / med / 1e6)


def cmd_time(args):
    import torch
    import hdl_deflate_amd
    from hdl_deflate_amd import _lib
    from hdl_deflate_amd.data import make_blocks
    assert torch.cuda.is_available(), "the probe needs a HIP device: there is nothing to time without one"
    assert args.repeats >= 10
    eng = hdl_deflate_amd.Engine()
    L, P = eng.lib, _bind(args.parent)
    assert not hasattr(P, "hdlz_bgzf_join_stored_ws"), "--parent must be a build of the parent commit"
    nbytes = 1 << args.log2_bytes
    families = make_blocks(nbytes // 2048, 2048, "cuda", seed=5).reshape(-1)
    head = ["%s, median of %d after %d warm-up repeats, HIP events around each call, ms; every call in turn within a repeat." %
            (torch.cuda.get_device_name(0), args.repeats, args.warmup),
            "command: python tools/probe_bgzf_stored.py time --parent <libhdlz.so of the parent commit> --log2-bytes %d" % args.log2_bytes, ""]
    # ---- 2. the one bar
    lines, sizes, fixed_file = list(head), [], None
    # (every 2 KiB of the bench data is of another family, and one of the four is random bytes: at 57344-byte blocks every block
    # compresses; at 2 KiB blocks a quarter would be stored, so the bar's 2 KiB input leaves that family out -- section 3 has the four)
    compressible = make_blocks(nbytes // 2048, 2048, "cuda", seed=5, families=(1, 2, 4)).reshape(-1)
    for n, source in ((57344, families), (2048, compressible)):
        b = Batch(L, source, n)
        assert b.crc() == 0 and b.compress() == 0 and b.join_stored() == 0 and b.join_older(P) == 0, L.hdlz_last_error()
        r = b.record()
        o = _lib.BgzfJoinResult.from_buffer_copy(b.old_res.cpu().numpy().tobytes())
        assert (r.status, r.nstored, r.first_bad) == (0, 0, 0xFFFFFFFF) and (o.status, o.file_len) == (0, r.file_len), (r.status, r.nstored, o.status)
        assert torch.equal(b.file[:r.file_len], b.old_file[:r.file_len]) and torch.equal(b.off, b.old_off)      # identical files
        b.check_head()
        t = timed([("(jp) parent hdlz_bgzf_join_ws", lambda: b.join_older(P)), ("(js) hdlz_bgzf_join_stored_ws", b.join_stored)],
                  args.repeats, args.warmup, L.hdlz_last_error)
        vp, vs = t["(jp) parent hdlz_bgzf_join_ws"], t["(js) hdlz_bgzf_join_stored_ws"]
        mp, ms = statistics.median(vp), statistics.median(vs)
        allowed = max(max(vp) - min(vp), max(vs) - min(vs))
        lines.append("%d blocks of %d bytes (%s), %d bytes of input, every member fixed: file %d bytes, identical on both sides" %
                     (b.B, n, "the four bench families" if source is families else "the three bench families that compress", b.total, r.file_len))
        lines += [row(k, v, b.total) for k, v in t.items()]
        lines.append("  (js) / (jp) = %.4f   excess %.4f ms, allowed %.4f ms (spreads: parent %.4f, new %.4f): the bar is %s" %
                     (ms / mp, ms - mp, allowed, max(vp) - min(vp), max(vs) - min(vs), "HELD" if ms - mp <= allowed else "MISSED"))
        lines.append("")
        if n == 57344:
            sizes.append(("the four bench families", "older writer, 57344-byte blocks", b.total, o.file_len))
            fixed_file = (b.file[:r.file_len].clone(), b.B, b.total, b.data)
        del b
    del compressible
    put_section(args.out, "2. the one bar: hdlz_bgzf_join_stored_ws against the parent's hdlz_bgzf_join_ws, all members fixed", lines)
    # ---- 3. random bytes and a half-and-half input at 65280-byte blocks
    B = nbytes // 65280
    n = 65280
    random = torch.randint(0, 256, (B * n,), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(7))
    half = families[:B * n].clone().view(B, n)
    half[1::2] = random.view(B, n)[1::2]                                # blocks alternate: bench families, random bytes
    lines, stored_file = list(head), None
    for label, data, n in (("random bytes", random, 65280), ("half and half (blocks alternate: bench families, random bytes)", half.reshape(-1), 65280),
                           ("the four bench families", families, 65280), ("the four bench families, a quarter of the blocks random bytes", families, 2048)):
        b = Batch(L, data, n)
        assert b.crc() == 0 and b.compress() == 0 and b.join_stored() == 0, L.hdlz_last_error()
        r = b.record()
        assert r.status == 0, (label, r.status, r.first_bad)
        b.check_head()
        sizes.append((label, "this writer, %d-byte blocks (%d of %d members stored)" % (n, r.nstored, b.B), b.total, r.file_len))
        if data is families and n == 65280:
            continue
        calls = [("(js) hdlz_bgzf_join_stored_ws", b.join_stored), ("(ws) the write: CRC + compress + stored join", lambda: b.crc() or b.compress() or b.join_stored())]
        if n == 2048:                                                   # (no block fails there: the older join runs too, for another file)
            assert b.join_older(P) == 0
            o = _lib.BgzfJoinResult.from_buffer_copy(b.old_res.cpu().numpy().tobytes())
            assert o.status == 0
            sizes.append((label, "older writer, 2048-byte blocks", b.total, o.file_len))
            calls.insert(0, ("(jp) parent hdlz_bgzf_join_ws (every member fixed)", lambda: b.join_older(P)))
        t = timed(calls, args.repeats, args.warmup, L.hdlz_last_error)
        tiles = (b.B + 255) // 256
        lines.append("%s: %d blocks of %d bytes, %d bytes of input, %d members stored: file %d bytes; %d workgroups of 256 rows on %d CUs" %
                     (label, b.B, n, b.total, r.nstored, r.file_len, tiles, torch.cuda.get_device_properties(0).multi_processor_count))
        lines += [row(k, v, b.total) for k, v in t.items()]
        lines.append("")
        if data is random:
            assert r.nstored == b.B and r.file_len == b.total + 31 * b.B + 28
            stored_file = (b.file[:r.file_len].clone(), b.B, b.total, b.data)
        del b
    put_section(args.out, "3. without a bar: the stored join and the whole write at 65280-byte blocks", lines)
    # ---- 4. the existing reader on the all-stored file against the all-fixed one
    lines = list(head)
    for label, (f, nb, total, data) in (("all fixed, 57344-byte blocks of the bench families", fixed_file), ("all stored, 65280-byte blocks of random bytes", stored_file)):
        M = nb + 1
        st = torch.cuda.current_stream().cuda_stream
        ioff, iout = (torch.empty(M + 1, dtype=torch.int64, device="cuda") for _ in range(2))
        ires, rres = torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(3, dtype=torch.int64, device="cuda")
        iwb, rwb = L.hdlz_bgzf_index_work_bytes(f.numel()), L.hdlz_bgzf_inflate_work_bytes(M, 0)
        iwork, rwork = torch.empty(iwb // 8, dtype=torch.int64, device="cuda"), torch.empty(rwb, dtype=torch.uint8, device="cuda")
        back = torch.zeros(total, dtype=torch.uint8, device="cuda")
        assert L.hdlz_bgzf_index_ws(f.data_ptr(), f.numel(), M, ioff.data_ptr(), iout.data_ptr(), ires.data_ptr(), iwork.data_ptr(), iwb, st) == 0
        x = _lib.BgzfIndexResult.from_buffer_copy(ires.cpu().numpy().tobytes())
        assert (x.nmembers, x.total_out, x.file_used, x.status, x.eof_marker) == (M, total, f.numel(), 0, 1), (x.nmembers, x.status)
        read = lambda: L.hdlz_bgzf_inflate_ws(f.data_ptr(), f.numel(), ioff.data_ptr(), iout.data_ptr(), M, 0, back.data_ptr(), total, None,
                                              rres.data_ptr(), rwork.data_ptr(), rwb, st)
        assert read() == 0
        u = _lib.BgzfInflateResult.from_buffer_copy(rres.cpu().numpy().tobytes())
        assert (u.status, u.out_len) == (0, total) and torch.equal(back, data), (label, u.status, u.first_bad)
        t = timed([("(rb) hdlz_bgzf_inflate_ws", read)], args.repeats, args.warmup, L.hdlz_last_error)
        lines.append("%s: %d members, file %d bytes, %d bytes of data" % (label, M, f.numel(), total))
        lines += [row(k, v, total) for k, v in t.items()]
        lines.append("")
        del back
    put_section(args.out, "4. without a bar: hdlz_bgzf_inflate_ws of the all-stored file against the all-fixed file", lines)
    # ---- 5. sizes
    lines = ["%-66s %-62s %12s %12s %8s" % ("input", "writer", "input bytes", "file bytes", "ratio")]
    for label, writer, total, size in sizes:
        lines.append("%-66s %-62s %12d %12d %8.4f" % (label, writer, total, size, size / total))
    lines += ["", "random bytes through the older writer: a fixed-Huffman member of n bytes that do not compress is about 9 n / 8 + 26 bytes (1.125 and more),",
              "and from 58231 bytes on it may not fit a member at all (HDLZ_E_OUT_CAPACITY); stored it is n + 31."]
    put_section(args.out, "5. file sizes", lines)
    return 0


def cmd_framing(args):
    import torch
    import hdl_deflate_amd
    from hdl_deflate_amd import _lib
    from hdl_deflate_amd.data import make_blocks
    assert torch.cuda.is_available(), "the probe needs a HIP device: there is nothing to time without one"
    assert args.repeats >= 10
    eng = hdl_deflate_amd.Engine()
    L, P = eng.lib, _bind(args.parent)
    nbytes = 1 << args.log2_bytes
    lines = ["%s, median of %d after %d warm-up repeats, HIP events around each call, ms; every call in turn within a repeat." %
             (torch.cuda.get_device_name(0), args.repeats, args.warmup),
             "command: python tools/probe_bgzf_stored.py framing --parent <libhdlz.so of the parent commit> --log2-bytes %d" % args.log2_bytes, ""]
    missed = 0
    for n, fam, label in ((57344, None, "the four bench families"), (2048, (1, 2, 4), "the three bench families that compress")):
        data = (make_blocks(nbytes // 2048, 2048, "cuda", seed=5, families=fam) if fam else make_blocks(nbytes // 2048, 2048, "cuda", seed=5)).reshape(-1)
        b = Batch(L, data, n)
        del data
        bits = torch.empty(b.B, dtype=torch.int64, device="cuda")
        zcap = L.hdlz_join_bound(b.B, n)
        assert zcap <= b.cap
        zres = torch.zeros(2, dtype=torch.int64, device="cuda")
        assert b.crc() == 0 and L.hdlz_compress_batch_bits(b.data.data_ptr(), None, n, n, b.B, 32, 10, b.rows.data_ptr(), b.pitch, b.out_len.data_ptr(),
                                                           b.status.data_ptr(), bits.data_ptr(), b.st) == 0, L.hdlz_last_error()
        # every call writes into file / off / res of its side: (file, off, res) for this build, (old_file, old_off, res2) for the parent
        res2 = torch.zeros(3, dtype=torch.int64, device="cuda")
        side = {L: (b.file, b.off, b.res), P: (b.old_file, b.old_off, res2)}
        zlib_join = lambda lib: lib.hdlz_join_batch_ws(b.rows.data_ptr(), b.pitch, b.out_len.data_ptr(), bits.data_ptr(), b.status.data_ptr(), None, n, b.B,
                                                       side[lib][0].data_ptr(), zcap, side[lib][1].data_ptr(), zres.data_ptr(), b.work.data_ptr(), b.wb, b.st)
        fixed = lambda lib: lib.hdlz_bgzf_join_ws(b.rows.data_ptr(), b.pitch, b.out_len.data_ptr(), b.status.data_ptr(), None, n, b.B, b.crcs.data_ptr(),
                                                  side[lib][0].data_ptr(), b.cap, side[lib][1].data_ptr(), side[lib][2].data_ptr(), b.work.data_ptr(), b.wb, b.st)
        stored = lambda lib: lib.hdlz_bgzf_join_stored_ws(b.data.data_ptr(), None, n, n, b.rows.data_ptr(), b.pitch, b.out_len.data_ptr(), b.status.data_ptr(),
                                                          b.B, b.crcs.data_ptr(), side[lib][0].data_ptr(), b.cap, side[lib][1].data_ptr(), None,
                                                          side[lib][2].data_ptr(), b.work.data_ptr(), b.wb, b.st)
        lines.append("%d blocks of %d bytes (%s), %d bytes of input" % (b.B, n, label, b.total))
        for name, call, words in (("hdlz_join_batch_ws", zlib_join, 0), ("hdlz_bgzf_join_ws", fixed, 2), ("hdlz_bgzf_join_stored_ws", stored, 3)):
            for lib in (P, L):
                side[lib][0].zero_()
                assert call(lib) == 0, lib.hdlz_last_error()
            rec = (zres if words == 0 else b.res).cpu().numpy()
            assert int(rec[words - 1 if words else 1]) & 0xFFFFFFFF == 0, (name, rec)          # the status word
            size = int(rec[0])
            assert torch.equal(b.file[:size], b.old_file[:size]) and torch.equal(b.off, b.old_off), name      # identical on both sides
            if words:
                assert torch.equal(b.res[:words], side[P][2][:words]), name
            t = timed([("(p) parent " + name, lambda: call(P)), ("(n) " + name, lambda: call(L))], args.repeats, args.warmup, L.hdlz_last_error)
            vp, vn = t["(p) parent " + name], t["(n) " + name]
            mp, mn = statistics.median(vp), statistics.median(vn)
            allowed = max(max(vp) - min(vp), max(vn) - min(vn))
            held = mn - mp <= allowed
            missed += not held
            lines += [row(k, v, b.total) for k, v in t.items()]
            lines.append("  output %d bytes, identical on both sides; (n) / (p) = %.4f   excess %.4f ms, allowed %.4f ms (spreads: parent %.4f, new %.4f): "
                         "the bar is %s" % (size, mn / mp, mn - mp, allowed, max(vp) - min(vp), max(vn) - min(vn), "HELD" if held else "MISSED"))
        lines.append("")
        del b
    put_section(args.out, "2. the bar of profiles/bgzf_stored.txt, section 2, for the three tile joins against the parent's", lines)
    return 1 if missed else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=("codeobj", "time", "framing"))
    ap.add_argument("--parent", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgzf_stored.txt"))
    ap.add_argument("--log2-bytes", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if args.cmd == "framing" and args.out == ap.get_default("out"):
        args.out = os.path.join(ROOT, "profiles", "framing_shared.txt")
    return {"codeobj": cmd_codeobj, "time": cmd_time, "framing": cmd_framing}[args.cmd](args)


if __name__ == "__main__":
    sys.exit(main())
