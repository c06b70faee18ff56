#!/usr/bin/env python
"""Evidence for hdlz_unjoin_ws (include/hdlz_unjoin.h), three sections of profiles/unjoin.txt, one sub-command each:

  codeobj --parent OBJDIR   (no GPU) the code-object metadata of every kernel in hdlz_inflate_tok / _grp / _dyn / hdlz_checksum (or of
                            --sources A,B,...) of a build of the parent commit (its csrc/_obj) beside this build's: the existing
                            instantiations must be the same, the member twins are listed next to them.  Each kernel's instructions
                            (llvm-objdump -d) are compared too: identical / same opcodes, registers renamed / identical but for
                            the offsets of scalar loads, for the pc-relative distance to a constant table, or for the exchanged
                            sources of commutative instructions (each named as such) / differs.  With
                            hdlz_join and hdlz_bgzf_stored among the sources, the kernels of MOVED are listed against the parent's
                            kernels they took the place of; a pair that differs there is settled by its timing and not counted.
  time                      (a) hdlz_inflate_checked of the per-block rows as a ragged archive, forced to the mapping (b) chooses,
                            (b) hdlz_unjoin_ws of the joined stream; 2 GiB of the four bench families as 2 KiB and as 64 KiB blocks,
                            HIP events, calls alternated in one process.  Yardstick: (b) <= 1.15 x (a).
  ab --parent LIB           hdlz_inflate_batch_ws of the parent commit's library against this build's, parent / new / new / parent in
                            child processes: same bytes, and the difference inside the parent's own spread.

Every sub-command replaces its own section of --out and leaves the others."""
import argparse
import hashlib
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LLVM = os.environ.get("HDLZ_LLVM_BIN", "/opt/rocm/llvm/bin")
FIELDS = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count", ".group_segment_fixed_size")
SOURCES = ("hdlz_inflate_tok", "hdlz_inflate_grp", "hdlz_inflate_dyn", "hdlz_checksum")


def put_section(path, title, lines):
    """replace the section `== title` of the file (or append it)"""
    text = open(path).read() if os.path.exists(path) else ""
    parts = re.split(r"(?m)^(?=== )", text)
    body = "== %s\n%s\n\n" % (title, "\n".join(lines))
    for k, p in enumerate(parts):
        if p.startswith("== %s\n" % title):
            parts[k] = body
            break
    else:
        parts.append(body)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("".join(parts))
    print(body)


def kernels_of(obj):
    """{demangled kernel name: {field: value, "code": [instruction text]}} of the gfx950 code object inside a hipcc object file"""
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat"), os.path.join(d, "co")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat, "--output=" + co,
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"])
        notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co]).decode()
        asm = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", co]).decode()
    code = {}                                                  # symbol -> its instructions without address and encoding
    for part in re.split(r"(?m)^[0-9a-f]+ <", asm)[1:]:
        code[part[:part.index(">")]] = [l.split("//")[0].strip() for l in part.splitlines()[1:] if l.strip()]
    out = {}
    for blk in re.split(r"(?m)^\s*- \.agpr_count", notes)[1:]:
        sym = re.search(r"(?m)^\s*\.name:\s*(\S+)", blk).group(1)
        name = subprocess.check_output(["c++filt", sym]).decode().strip()
        k = out[re.sub(r"\(.*", "", name).replace("void ", "")] = {f: int(re.search(r"(?m)^\s*%s:\s*(\d+)" % re.escape(f), blk).group(1)) for f in FIELDS}
        k["code"] = code[sym]
        while k["code"] and k["code"][-1].split()[0] in ("s_nop", "s_code_end", "..."):      # the padding behind a kernel
            k["code"].pop()
    return out


def code_tag(old, new):
    """how two instruction sequences compare; register numbers (v12, s[4:5], a3) are what "renamed" forgives"""
    if old == new:
        return "identical (%d instructions)" % len(new)
    blank = lambda seq: [re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])", r"\1#", i) for i in seq]
    if blank(old) == blank(new):
        return "same opcodes, registers renamed (%d instructions)" % len(new)
    args = lambda seq: [re.sub(r"^(s_load_dword\w* .*), 0x[0-9a-f]+$", r"\1, #", i) for i in seq]
    if args(old) == args(new):
        return "identical but for the offsets of scalar loads: the argument record changed (%d instructions)" % len(new)
    if len(old) == len(new):
        # a table's address is pc-relative (s_getpc_b64, then s_add_u32 with the distance): it moves with the size of the kernels that
        # stand between; and a commutative scalar op may come out with its two sources exchanged
        pcrel = lambda k: k > 0 and old[k - 1].startswith("s_getpc_b64") and old[k].startswith("s_add_u32") and new[k].startswith("s_add_u32")
        def swapped(a, b):
            m, n = re.match(r"^(s_and_b64|s_or_b64|v_lshl_add_u64) (\S+), (\S+), (.*)$", a), re.match(r"^(s_and_b64|s_or_b64|v_lshl_add_u64) (\S+), (\S+), (.*)$", b)
            if not m or not n or m.group(1, 2) != n.group(1, 2):
                return False
            x, y = [m.group(3)] + m.group(4).split(", "), [n.group(3)] + n.group(4).split(", ")
            return sorted(x) == sorted(y)
        bad = [k for k in range(len(new)) if old[k] != new[k]]
        if all(pcrel(k) for k in bad):
            return "identical but for the pc-relative distance to a constant table (%d instructions)" % len(new)
        if all(pcrel(k) or swapped(old[k], new[k]) for k in bad):
            return "identical but for the sources of %d commutative instructions exchanged (%d instructions)" % (sum(not pcrel(k) for k in bad), len(new))
    return "differs (%d -> %d instructions)" % (len(old), len(new))


def canon(name):
    """an existing instantiation under the name it had before the MEMBERS flag: the default (false) flag dropped (on both sides: a
    parent that has the flag already compares like with like)"""
    name = re.sub(r"(k_inflate_tok<[^,]+, \d+u), false>", r"\1>", name)
    name = re.sub(r"(k_inflate_dyn<(?:true|false)), false>", r"\1>", name)
    return name.replace("k_inflate_grp<false>", "k_inflate_grp")


# the one BGZF writer (hdlz_bgzf_stored.hip) against the kernels it took the place of, which stood in two files: this build's name ->
# (the parent's source, the parent's names); the zlib/gzip join keeps its file and lost its template flag
MOVED = {"hdlz::k_bgzf_join<false>": ("hdlz_join", ["hdlz::k_join<true>"]),
         "hdlz::k_bgzf_join<true>": ("hdlz_bgzf_stored", ["hdlz::k_bgzf_join_stored"]),
         "hdlz::k_bgzf_join_finish": ("hdlz_join", ["hdlz::k_bgzf_join_finish"]),
         "hdlz::k_bgzf_join_finish ": ("hdlz_bgzf_stored", ["hdlz::k_bgzf_join_stored_finish"]),
         "hdlz::k_join": ("hdlz_join", ["hdlz::k_join<false>"])}


def moved_lines(parent, new_dir, fmt):
    """the kernels of MOVED, each against its parent: a pair that differs is a different function now and is settled by its timing"""
    lines, objs = ["moved or merged kernels (this build | the parent's kernel it is compared with):"], {}
    load = lambda d, src: objs.setdefault((d, src), kernels_of(os.path.join(d, src + ".o")))
    for name, (src, olds) in sorted(MOVED.items()):
        n = load(new_dir, "hdlz_join" if name == "hdlz::k_join" else "hdlz_bgzf_stored")[name.strip()]
        for old in olds:
            o = load(parent, src)[old]
            lines.append("  %-28s %-24s | %-34s %-24s %s" % (name.strip(), fmt(n), old, fmt(o), code_tag(o["code"], n["code"])))
    return lines


def cmd_codeobj(args):
    new_dir = os.path.join(ROOT, "hdl_deflate_amd", "csrc", "_obj")
    lines = ["code-object metadata, parent build | this build (%s)" % ", ".join(f[1:] for f in FIELDS),
             "command: python tools/probe_unjoin.py codeobj --parent <csrc/_obj of a build of the parent commit>" +
             (" --sources " + args.sources if args.sources else ""), ""]
    differ, notes = 0, []
    fmt = lambda v: "-" if v is None else " ".join("%d" % v[f] for f in FIELDS)
    sources = args.sources.split(",") if args.sources else SOURCES
    # MOVED records ONE past change: it applies against a parent that still has the kernels it names; any later parent has this build's
    # names already and is compared kernel by kernel like everything else
    moved = {"hdlz_join", "hdlz_bgzf_stored"} <= set(sources) and "hdlz::k_join<true>" in kernels_of(os.path.join(args.parent, "hdlz_join.o"))
    gone = {(src, old) for src, olds in MOVED.values() for old in olds} if moved else set()
    for src in sources:
        old = {canon(k): v for k, v in kernels_of(os.path.join(args.parent, src + ".o")).items()}
        new = {canon(k): (k, v) for k, v in kernels_of(os.path.join(new_dir, src + ".o")).items()}
        lines.append(src + ":")
        for name in sorted(set(old) | set(new)):
            if (src, name) in gone or (moved and name in MOVED):
                continue
            o = old.get(name)
            full, n = new.get(name, (name, None))
            tag = "twin (new)" if o is None else "MISSING" if n is None else "same" if fmt(o) == fmt(n) else "DIFFERS"
            code = code_tag(o["code"], n["code"]) if o and n else ""
            differ += tag in ("MISSING", "DIFFERS") or code.startswith("differs")
            lines.append("  %-60s %-24s | %-24s %s%s" % (full, fmt(o), fmt(n), tag, code and "; " + code))
            if o is None and (n[".private_segment_fixed_size"] or n[".vgpr_spill_count"] or n[".sgpr_spill_count"]):
                notes.append("  finding: %s -- scratch %d bytes, %d VGPRs and %d SGPRs spilled" %
                             (full, n[".private_segment_fixed_size"], n[".vgpr_spill_count"], n[".sgpr_spill_count"]))
    lines.append("")
    if moved:
        lines += moved_lines(args.parent, new_dir, fmt) + [""]
    lines.append("existing instantiations that differ or are missing: %d" % differ)
    lines.extend(notes or ["  no twin uses scratch or spills"])
    put_section(args.out, "1. code objects of the existing kernels (no GPU)", lines)
    return 1 if differ else 0


def _setup(eng, total, n):
    """compress `total` bytes in blocks of n -> the rows as a ragged archive and the joined stream, both with their indices"""
    import torch
    from hdl_deflate_amd.constants import pitch_for
    from hdl_deflate_amd.data import make_blocks
    L = eng.lib
    st = torch.cuda.current_stream().cuda_stream
    B, pitch = total // n, pitch_for(n)
    data = make_blocks(total // 2048, 2048, "cuda", seed=5).reshape(-1)
    rows = torch.empty((B, pitch), dtype=torch.uint8, device="cuda")
    out_len, status = (torch.empty(B, dtype=torch.int32, device="cuda") for _ in range(2))
    bits = torch.empty(B, dtype=torch.int64, device="cuda")
    assert L.hdlz_compress_batch_bits(data.data_ptr(), None, n, n, B, 32, 10, rows.data_ptr(), pitch, out_len.data_ptr(), status.data_ptr(),
                                      bits.data_ptr(), st) == 0
    cap = L.hdlz_join_bound(B, n)
    wb = max(L.hdlz_archive_work_bytes(B), L.hdlz_join_work_bytes(B))
    work = torch.empty(wb // 8, dtype=torch.int64, device="cuda")
    arch, joined = (torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(2))
    aoff, joff = (torch.empty(B + 1, dtype=torch.int64, device="cuda") for _ in range(2))
    res = torch.empty(2, dtype=torch.int64, device="cuda")
    assert L.hdlz_archive_batch_ws(rows.data_ptr(), pitch, out_len.data_ptr(), B, arch.data_ptr(), cap, aoff.data_ptr(), work.data_ptr(), wb, st) == 0
    assert L.hdlz_join_batch_ws(rows.data_ptr(), pitch, out_len.data_ptr(), bits.data_ptr(), status.data_ptr(), None, n, B, joined.data_ptr(), cap,
                                joff.data_ptr(), res.data_ptr(), work.data_ptr(), wb, st) == 0
    torch.cuda.synchronize()
    assert int(status.max()) == 0
    slen = int(joff[B]) + 6
    del rows, work
    return data, B, arch, aoff, joined, joff, slen


def cmd_time(args):
    import torch
    import hdl_deflate_amd
    from hdl_deflate_amd import _lib
    eng = hdl_deflate_amd.Engine()
    L = eng.lib
    st = torch.cuda.current_stream().cuda_stream
    total = 1 << args.log2_bytes
    lines = ["%d bytes of the four bench families, %s, median of %d after %d warm-up repeats, HIP events, ms" %
             (total, torch.cuda.get_device_name(0), args.repeats, args.warmup),
             "command: python tools/probe_unjoin.py time --log2-bytes %d --repeats %d --warmup %d" % (args.log2_bytes, args.repeats, args.warmup), ""]
    for n in (2048, 65536):
        data, B, arch, aoff, joined, joff, slen = _setup(eng, total, n)
        # the mapping (b) chooses from B: (a) is forced to it
        hint = 64 if 8192 <= B <= 16384 else 4 if B <= 22528 else 2
        out = torch.empty(total, dtype=torch.uint8, device="cuda")
        res4 = [torch.empty(B, dtype=torch.int32, device="cuda") for _ in range(4)]
        cwb = L.hdlz_inflate_checked_work_bytes(B, 0, n, hint, 1)
        uwb = L.hdlz_unjoin_work_bytes(B, total, 0)
        work = torch.empty(max(cwb, uwb), dtype=torch.uint8, device="cuda")
        rec = torch.empty(3, dtype=torch.int64, device="cuda")
        calls = {
            "(a) hdlz_inflate_checked": lambda: L.hdlz_inflate_checked(arch.data_ptr(), aoff.data_ptr(), 0, 0, B, hint, 0, out.data_ptr(), n,
                                                                       *[t.data_ptr() for t in res4], work.data_ptr(), cwb, st),
            "(b) hdlz_unjoin_ws": lambda: L.hdlz_unjoin_ws(joined.data_ptr(), slen, joff.data_ptr(), None, n, B, 0, out.data_ptr(), total, None,
                                                           rec.data_ptr(), work.data_ptr(), uwb, st),
        }
        times = {k: [] for k in calls}
        for rep in range(args.warmup + args.repeats):
            for name, fn in calls.items():
                out.zero_()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = fn()
                e1.record()
                e1.synchronize()
                assert rc == 0, (name, L.hdlz_last_error())
                assert torch.equal(out, data), name
                if rep >= args.warmup:
                    times[name].append(e0.elapsed_time(e1))
        r = _lib.UnjoinResult.from_buffer_copy(rec.cpu().numpy().tobytes())
        assert (r.status, r.out_len) == (0, total) and int(res4[1].max()) == 0, (r.status, r.out_len)
        med = {k: statistics.median(v) for k, v in times.items()}
        lines.append("%d members of %d bytes (mapping hint %d): joined stream %d bytes" % (B, n, hint, slen))
        for k, v in times.items():
            lines.append("  %-26s median %8.3f   min %8.3f   max %8.3f   %7.1f GB/s of output" % (k, med[k], min(v), max(v), total / med[k] / 1e6))
        a, b = (med[k] for k in calls)
        va = times["(a) hdlz_inflate_checked"]
        lines.append("  (b) / (a) = %.3f   (yardstick: <= 1.15; (a)'s own spread, (max - min) / median: %.4f)" % (b / a, (max(va) - min(va)) / a))
        lines.append("")
        del data, arch, joined, out, work
    put_section(args.out, "2. hdlz_unjoin_ws against hdlz_inflate_checked of the same members", lines)
    return 0


def cmd_ab_child(args):
    """one library (HDLZ_LIB), hdlz_inflate_batch_ws of 2^18 ragged streams of 2 KiB blocks: prints the median and a digest of the output"""
    import ctypes
    import torch                                               # (first: libhdlz resolves to the HIP runtime torch loaded)
    import hdl_deflate_amd
    from hdl_deflate_amd import _lib
    if not hasattr(ctypes.CDLL(_lib.LIB_PATH), "hdlz_unjoin_ws"):
        _lib.UNJOIN_SIGNATURES = {}                            # the parent commit's library: nothing of hdlz_unjoin.h to bind
    eng = hdl_deflate_amd.Engine()
    L = eng.lib
    st = torch.cuda.current_stream().cuda_stream
    n, total = 2048, 1 << 29
    data, B, arch, aoff, joined, joff, slen = _setup(eng, total, n)
    out = torch.zeros((B, n), dtype=torch.uint8, device="cuda")
    ol, s = (torch.empty(B, dtype=torch.int32, device="cuda") for _ in range(2))
    wb = L.hdlz_inflate_work_bytes(B, 0, n, 0, 1)
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    ts = []
    for rep in range(args.warmup + args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = L.hdlz_inflate_batch_ws(arch.data_ptr(), aoff.data_ptr(), 0, 0, B, 0, 0, out.data_ptr(), n, ol.data_ptr(), s.data_ptr(), work.data_ptr(), wb, st)
        e1.record()
        e1.synchronize()
        assert rc == 0
        if rep >= args.warmup:
            ts.append(e0.elapsed_time(e1))
    assert int(s.max()) == 0 and torch.equal(out.reshape(-1), data)
    h = hashlib.sha256(out.cpu().numpy().tobytes() + ol.cpu().numpy().tobytes()).hexdigest()[:16]
    print("AB %.4f %.4f %.4f %s" % (statistics.median(ts), min(ts), max(ts), h))
    return 0


def cmd_ab(args):
    new = os.path.join(ROOT, "hdl_deflate_amd", "lib", "libhdlz.so")
    lines = ["hdlz_inflate_batch_ws, 2^18 ragged streams (2 KiB blocks of the four bench families, lane mapping), median of %d after %d, ms; one child"
             " process per run" % (args.repeats, args.warmup), "command: python tools/probe_unjoin.py ab --parent <libhdlz.so of the parent commit>", ""]
    runs = []
    for tag, lib in (("parent", args.parent), ("new", new), ("new", new), ("parent", args.parent)):
        env = dict(os.environ, HDLZ_LIB=lib)
        outp = subprocess.run([sys.executable, os.path.abspath(__file__), "ab-child", "--repeats", str(args.repeats), "--warmup", str(args.warmup)],
                              env=env, stdout=subprocess.PIPE, timeout=300, check=True).stdout.decode()
        med, lo, hi, h = re.search(r"AB (\S+) (\S+) (\S+) (\S+)", outp).groups()
        runs.append((tag, float(med), float(lo), float(hi), h))
        lines.append("  %-7s median %8.4f   min %8.4f   max %8.4f   sha256 of out + out_len %s" % runs[-1])
    p = [r[1] for r in runs if r[0] == "parent"]
    q = [r[1] for r in runs if r[0] == "new"]
    lines.append("")
    lines.append("same bytes: %s;  new / parent (means of the medians) = %.4f;  the parent's own two runs differ by %.4f of their mean" %
                 (len({r[4] for r in runs}) == 1, sum(q) / sum(p), abs(p[0] - p[1]) / (sum(p) / 2)))
    put_section(args.out, "3. hdlz_inflate_batch_ws: the parent's library against this build's", lines)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=("codeobj", "time", "ab", "ab-child"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unjoin.txt"))
    ap.add_argument("--parent")
    ap.add_argument("--sources", help="codeobj: comma-separated source names in place of the default four")
    ap.add_argument("--log2-bytes", type=int, default=31)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    return {"codeobj": cmd_codeobj, "time": cmd_time, "ab": cmd_ab, "ab-child": cmd_ab_child}[args.cmd](args)


if __name__ == "__main__":
    sys.exit(main())
