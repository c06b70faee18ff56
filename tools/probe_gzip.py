#!/usr/bin/env python
"""Evidence for the gzip form of the joined stream (include/hdlz_gzip.h), the sections of profiles/gzip_joined.txt, one sub-command each:

  codeobj --parent OBJDIR    (no GPU) the code-object metadata of every kernel of hdlz_join / hdlz_unjoin in a build of the parent
                             commit (its csrc/_obj) beside this build's, and the new kernels (hdlz_crc32 included) next to them.
  time --parent LIB          2 GiB of the four bench families as 2^20 x 2 KiB and 2^15 x 64 KiB blocks, HIP events, every call in turn
                             within a repeat, median of --repeats after --warmup: the CRC pass alone; the gzip join against the zlib
                             join; CRC + compress + gzip join against compress + zlib join; the gzip unjoin against the zlib unjoin.
                             THE BAR: the CRC pass takes no longer than hdlz_compress_batch_bits of the same input -- the PARENT
                             commit's library (LIB), timed twice in every repeat: the two parent columns against each other are the
                             run's own noise.  --variant LIB2 adds the CRC pass of another build (build.sh crcbank) to the same run.
  counters [--variant LIB2]  SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE of k_crc32_tiles from a counters-only rocprofv3 run of the
                             `crc-only` sub-command (a child process per library), summed over the kernel's dispatches.
  crc-only                   hdlz_crc32_ws of 256 MiB, five times (what `counters` profiles); checks the word against zlib.

Every sub-command replaces its own section of --out and leaves the others."""
import argparse
import csv
import ctypes
import glob
import os
import statistics
import subprocess
import sys
import tempfile
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import probe_unjoin                                             # noqa: E402  (put_section, kernels_of, FIELDS)


def cmd_codeobj(args):
    new_dir = os.path.join(ROOT, "hdl_deflate_amd", "csrc", "_obj")
    F = probe_unjoin.FIELDS
    fmt = lambda v: "-" if v is None else " ".join("%d" % v[f] for f in F)
    body = lambda v: [i for i in v["code"] if i != "s_nop 0"]          # (the last kernel of a code object carries the section's padding)
    lines = ["code-object metadata, parent build | this build (%s)" % ", ".join(f[1:] for f in F),
             "command: python tools/probe_gzip.py codeobj --parent <csrc/_obj of a build of the parent commit>", ""]
    differ = 0
    for src in ("hdlz_join", "hdlz_unjoin", "hdlz_crc32"):
        old_path = os.path.join(args.parent, src + ".o")
        old = probe_unjoin.kernels_of(old_path) if os.path.exists(old_path) else {}
        new = probe_unjoin.kernels_of(os.path.join(new_dir, src + ".o"))
        lines.append(src + ":")
        for name in sorted(set(old) | set(new)):
            o, n = old.get(name), new.get(name)
            tag = "new" if o is None else "MISSING" if n is None else "same" if fmt(o) == fmt(n) else "DIFFERS"
            code = ""
            if o and n:
                code = "; instructions identical (%d)" % len(body(n)) if body(o) == body(n) else "; instructions differ (%d -> %d)" % (len(body(o)), len(body(n)))
            differ += tag in ("MISSING", "DIFFERS") or "differ (" in code
            lines.append("  %-44s %-24s | %-26s %s%s" % (name, fmt(o), fmt(n), tag, code))
    lines += ["", "existing kernels that differ or are missing: %d   (instructions compared without the trailing s_nop padding of a code object's last kernel)" % differ]
    probe_unjoin.put_section(args.out, "1. code objects of the existing kernels (no GPU)", lines)
    return 1 if differ else 0


def _bind(path):
    from hdl_deflate_amd import _lib
    L = ctypes.CDLL(path)
    tables = [_lib.SIGNATURES, _lib.JOIN_SIGNATURES, _lib.UNJOIN_SIGNATURES, _lib.GZIP_SIGNATURES]
    for t in tables:
        for name, (restype, argtypes) in t.items():
            if hasattr(L, name):                                # (the parent commit's library has nothing of hdlz_gzip.h)
                fn = getattr(L, name)
                fn.restype, fn.argtypes = restype, argtypes
    return L


def cmd_time(args):
    import torch
    import hdl_deflate_amd
    from hdl_deflate_amd import _lib
    from hdl_deflate_amd.constants import pitch_for
    from hdl_deflate_amd.data import make_blocks
    assert torch.cuda.is_available(), "the probe needs a HIP device: there is nothing to time without one"
    eng = hdl_deflate_amd.Engine()
    L, P = eng.lib, _bind(args.parent)
    V = _bind(args.variant) if args.variant else None
    total = 1 << args.log2_bytes
    data = make_blocks(total // 2048, 2048, "cuda", seed=5).reshape(-1)
    st = torch.cuda.current_stream().cuda_stream
    crc_want = zlib.crc32(data.cpu().numpy())
    lines = ["gzip form of the joined stream: %d bytes of the four bench families, %s, median of %d after %d warm-up repeats, HIP events, ms;" %
             (total, torch.cuda.get_device_name(0), args.repeats, args.warmup),
             "every call in turn within a repeat.  command: python tools/probe_gzip.py time --parent <libhdlz.so of the parent commit>" +
             (" --variant <lib/libhdlz_crcbank.so>" if V else ""), ""]
    crc = torch.zeros(2, dtype=torch.int32, device="cuda")
    cwb = L.hdlz_crc32_work_bytes(total)
    cwork = torch.empty(cwb // 4, dtype=torch.int32, device="cuda")
    missed = 0
    for n in (2048, 65536):
        B, pitch = total // n, pitch_for(n)
        rows = torch.empty((B, pitch), dtype=torch.uint8, device="cuda")
        out_len, status = (torch.empty(B, dtype=torch.int32, device="cuda") for _ in range(2))
        bits = torch.empty(B, dtype=torch.int64, device="cuda")
        zcap, gcap = L.hdlz_join_bound(B, n), L.hdlz_join_gzip_bound(B, n)
        zdst, gdst = torch.empty(zcap, dtype=torch.uint8, device="cuda"), torch.empty(gcap, dtype=torch.uint8, device="cuda")
        zoff, goff = (torch.empty(B + 1, dtype=torch.int64, device="cuda") for _ in range(2))
        zres, gres = (torch.zeros(2, dtype=torch.int64, device="cuda") for _ in range(2))
        jwb = L.hdlz_join_work_bytes(B)
        jwork = torch.empty(jwb // 8, dtype=torch.int64, device="cuda")
        back = torch.empty(total, dtype=torch.uint8, device="cuda")
        ures = torch.zeros(3, dtype=torch.int64, device="cuda")
        uwb = max(L.hdlz_unjoin_work_bytes(B, total, 0), L.hdlz_unjoin_gzip_work_bytes(B, total, 0))
        uwork = torch.empty(uwb, dtype=torch.uint8, device="cuda")
        compress = lambda lib: lib.hdlz_compress_batch_bits(data.data_ptr(), None, n, n, B, 32, 10, rows.data_ptr(), pitch, out_len.data_ptr(),
                                                            status.data_ptr(), bits.data_ptr(), st)
        crc32 = lambda lib, k: lib.hdlz_crc32_ws(data.data_ptr(), total, crc.data_ptr() + 4 * k, cwork.data_ptr(), cwb, st)
        zjoin = lambda: L.hdlz_join_batch_ws(rows.data_ptr(), pitch, out_len.data_ptr(), bits.data_ptr(), status.data_ptr(), None, n, B,
                                             zdst.data_ptr(), zcap, zoff.data_ptr(), zres.data_ptr(), jwork.data_ptr(), jwb, st)
        gjoin = lambda: L.hdlz_join_gzip_ws(rows.data_ptr(), pitch, out_len.data_ptr(), bits.data_ptr(), status.data_ptr(), None, n, B,
                                            crc.data_ptr(), gdst.data_ptr(), gcap, goff.data_ptr(), gres.data_ptr(), jwork.data_ptr(), jwb, st)
        lens = {}

        def zunjoin():
            return L.hdlz_unjoin_ws(zdst.data_ptr(), lens["z"], zoff.data_ptr(), None, n, B, 0, back.data_ptr(), total, None, ures.data_ptr(),
                                    uwork.data_ptr(), uwb, st)

        def gunjoin():
            return L.hdlz_unjoin_gzip_ws(gdst.data_ptr(), lens["g"], goff.data_ptr(), None, n, B, 0, back.data_ptr(), total, None, ures.data_ptr(),
                                         uwork.data_ptr(), uwb, st)
        # the lengths of the two streams, once, in front of the timed repeats
        assert crc32(L, 0) == 0 and compress(L) == 0 and zjoin() == 0 and gjoin() == 0, L.hdlz_last_error()
        zr = _lib.JoinResult.from_buffer_copy(zres.cpu().numpy().tobytes())
        gr = _lib.JoinGzipResult.from_buffer_copy(gres.cpu().numpy().tobytes())
        assert zr.status == 0 and gr.status == 0 and gr.stream_len == zr.stream_len + 12
        lens["z"], lens["g"] = zr.stream_len, gr.stream_len
        calls = [("(p1) parent hdlz_compress_batch_bits", lambda: compress(P)),
                 ("(c)  hdlz_crc32_ws", lambda: crc32(L, 0))]
        if V:
            calls.append(("(cv) hdlz_crc32_ws, bank-private tables", lambda: crc32(V, 1)))
        calls += [("(p2) parent hdlz_compress_batch_bits", lambda: compress(P)),
                  ("(n)  hdlz_compress_batch_bits", lambda: compress(L)),
                  ("(jz) hdlz_join_batch_ws", zjoin),
                  ("(jg) hdlz_join_gzip_ws", gjoin),
                  ("(wz) compress + zlib join", lambda: compress(L) or zjoin()),
                  ("(wg) CRC + compress + gzip join", lambda: crc32(L, 0) or compress(L) or gjoin()),
                  ("(uz) hdlz_unjoin_ws", zunjoin),
                  ("(ug) hdlz_unjoin_gzip_ws", gunjoin)]
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
                if name.startswith(("(uz)", "(ug)")) and rep == 0:
                    u = _lib.UnjoinGzipResult.from_buffer_copy(ures.cpu().numpy().tobytes())
                    assert (u.status, u.out_len) == (0, total), (name, u.status, u.first_bad)
                    assert torch.equal(back[:1 << 24], data[:1 << 24])
        got = [int(x) & 0xFFFFFFFF for x in crc.cpu().numpy()]
        assert got[0] == crc_want, (hex(got[0]), hex(crc_want))
        if V:
            assert got[0] == got[1], "the two layouts disagree"
        med = {k: statistics.median(v) for k, v in times.items()}
        lines.append("%d blocks of %d bytes (rows of %d): gzip stream %d bytes, ratio %.4f; CRC-32 %08X" % (B, n, pitch, gr.stream_len, gr.stream_len / total, got[0]))
        for k, _ in calls:
            v = times[k]
            lines.append("  %-42s median %8.3f   min %8.3f   max %8.3f   %8.1f GB/s of input" % (k, med[k], min(v), max(v), total / med[k] / 1e6))
        m = lambda tag: med[next(k for k in med if k.startswith(tag))]
        parent = (m("(p1)") + m("(p2)")) / 2
        noise = abs(m("(p1)") - m("(p2)")) / parent
        ok = m("(c)") <= min(m("(p1)"), m("(p2)"))
        missed += not ok
        lines.append("  THE BAR  (c) <= parent compress: %.3f ms (%.3f TB/s) against %.3f / %.3f ms: %s   (parent against parent: %.4f of their mean)" %
                     (m("(c)"), total / m("(c)") / 1e9, m("(p1)"), m("(p2)"), "met" if ok else "MISSED", noise))
        lines.append("  (jg) / (jz) = %.3f   (wg) / (wz) = %.3f   (ug) / (uz) = %.3f   (n) / parent = %.4f" %
                     (m("(jg)") / m("(jz)"), m("(wg)") / m("(wz)"), m("(ug)") / m("(uz)"), m("(n)") / parent))
        if V:
            lines.append("  (cv) / (c) = %.3f" % (m("(cv)") / m("(c)")))
        lines.append("")
        del rows, zdst, gdst, back
    probe_unjoin.put_section(args.out, "2. times (one GPU)", lines)
    return 1 if missed else 0


def cmd_crc_only(args):
    import torch
    import hdl_deflate_amd
    eng = hdl_deflate_amd.Engine()
    n = 1 << 28
    d = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda")
    want = zlib.crc32(d.cpu().numpy().tobytes())
    for _ in range(5):
        got = int(eng.crc32(d).cpu().numpy()[0])
        assert got == want, (hex(got), hex(want))
    print("crc-only: %08X, %d bytes, five calls" % (want, n))
    return 0


def cmd_counters(args):
    names = ("SQ_LDS_BANK_CONFLICT", "SQ_LDS_IDX_ACTIVE")
    lines = ["LDS counters of k_crc32_tiles over five calls of hdlz_crc32_ws on 256 MiB of random bytes (rocprofv3 --pmc, a counters-only run",
             "of `tools/probe_gzip.py crc-only`, one child process per library; summed over the kernel's dispatches)", ""]
    libs = [("sliced tables, table[k][byte] (the default build)", None)] + ([("bank-private table, table[byte][lane] (build.sh crcbank)", args.variant)] if args.variant else [])
    for label, lib in libs:
        with tempfile.TemporaryDirectory() as d:
            env = dict(os.environ)
            if lib:
                env["HDLZ_LIB"] = os.path.abspath(lib)
            subprocess.check_call(["rocprofv3", "--pmc"] + list(names) + ["-d", d, "-o", "crc", "--output-format", "csv", "--",
                                   sys.executable, os.path.abspath(__file__), "crc-only"], env=env, cwd=ROOT)
            total = dict.fromkeys(names, 0.0)
            dispatches = set()
            for path in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
                for row in csv.DictReader(open(path)):
                    if "k_crc32_tiles" in row["Kernel_Name"] and row["Counter_Name"] in total:
                        total[row["Counter_Name"]] += float(row["Counter_Value"])
                        dispatches.add(row["Dispatch_Id"])
        conflict, active = total[names[0]], total[names[1]]
        lines.append("  %-58s %d dispatches   %s %.4g   %s %.4g   conflict / active = %.3f" %
                     (label, len(dispatches), names[0], conflict, names[1], active, conflict / active if active else float("nan")))
    probe_unjoin.put_section(args.out, "3. LDS counters of the two table layouts", lines)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=("codeobj", "time", "counters", "crc-only"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gzip_joined.txt"))
    ap.add_argument("--parent")
    ap.add_argument("--variant", help="time / counters: a second build of the library whose CRC pass is measured too (build.sh crcbank)")
    ap.add_argument("--log2-bytes", type=int, default=31)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    return {"codeobj": cmd_codeobj, "time": cmd_time, "counters": cmd_counters, "crc-only": cmd_crc_only}[args.cmd](args)


if __name__ == "__main__":
    sys.exit(main())
