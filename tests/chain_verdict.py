"""Which of the two whole-GPU inflate chains delivered a stream (a helper module like checked_ref.py, not a conftest).

hdlz_inflate_par.hip (k_par_*: streams of fixed blocks) and hdlz_inflate_any.hip (k_any_*: any block types) hand whatever they cannot do
to the serial decoder, so status and bytes say nothing about them.  Both leave their verdict in control words in the caller's scratch:
`run` sends streams through Engine.inflate_batch with a scratch of its own (filled with 0x5A first) and reads those words back as a
`Verdict` per stream.  Where the words lie is asked of lib/libhdlz_dbg.so (`csrc/build.sh dbg`: the same kernels plus the host-only
hdlz_debug_par_offsets); which word is which -- the enums C_*, A_*, W_* -- and every limit of the chains is read from the kernels'
sources (`source_constants`), and the list sizes of hdlz_inflate_any.hip's lay_of are restated in `lay` with the source lines they
restate asserted to be there.  Nothing here holds a word index or a W_* value of its own."""
import collections
import ctypes
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "hdl_deflate_amd", "csrc")
DBG = os.path.join(REPO, "hdl_deflate_amd", "lib", "libhdlz_dbg.so")
DBG_BUILD = "hdl_deflate_amd/csrc/build.sh dbg"

ENUMS = (("hdlz_inflate_par.h", "C_"), ("hdlz_inflate_any.hip", "A_"), ("hdlz_inflate_any.hip", "W_"))
NUMBERS = (("hdlz_inflate_any.hip", ("PB_MAX", "FIX_MAX_BITS", "FIRST_FIX_BITS", "WALK_ROUNDS", "REQ_MAX", "ANY_MIN", "HEAD", "CH_MAX")),
           ("hdlz_inflate_par.h", ("MAXCROSS", "CH_BITS_MAX", "FIRST_BIT", "HDLZ_HOPS")))
# the lines of lay_of (hdlz_inflate_any.hip), layout_of (hdlz_inflate_par.hip) and passes_for (hdlz_inflate_par.h) that `lay`,
# `fixed_pieces` and `passes_for` restate: white space aside they must stand in the source as they stand here
RESTATED = (("hdlz_inflate_any.hip", (
    "L.pb = zn >= (4u << 20) ? 2048u : 1024u;",
    "L.nchunks = (uint32_t)((nbits + L.pb - 1u) / L.pb);",
    "L.candcap = (uint32_t)(nbits / 128u) + 1024u;",
    "L.maxb = zn / 1024u < 64u ? 64u : zn / 1024u > 8000u ? 8000u : zn / 1024u;",
    "L.maxreq = 2u * L.maxb;",
    "L.mapcap = L.nchunks / 16u + 1024u;",
    "if (L.mapcap > 2u * L.nchunks + 64u) L.mapcap = 2u * L.nchunks + 64u;",
    "L.maxx = 2u * L.maxb + 256u + L.mapcap + L.nchunks / 8u;",
    "L.maxs = zn / 512u + 256u;",
    "L.tcap = 3u * L.pb / 8u;",
    "const uint32_t nitems = L.nchunks + L.maxx;",
    "const uint32_t passes = par::passes_for(nitems);")),
    ("hdlz_inflate_par.hip", (
        "const uint64_t ztot = (uint64_t)zn * nstr;",
        "const uint32_t chbits = ztot < (5u << 18) ? CH_BITS_MAX / 8u : ztot < (3u << 20) ? CH_BITS_MAX / 4u : ztot < (24u << 20) ? CH_BITS_MAX / 2u : CH_BITS_MAX;",
        "const uint32_t nchunks = (8u * zn - FIRST_BIT + chbits - 1u) / chbits;",
        "const uint32_t passes = passes_for(nchunks);")),
    ("hdlz_inflate_par.h", (
        "for (uint64_t reach = 1; reach < (uint64_t)nitems + 1u; reach *= HOPS) passes++;",
        "return passes > (uint32_t)(C_NCROSS - C_PASS0) ? (uint32_t)(C_NCROSS - C_PASS0) : passes;")))


def _strip(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _enum(text, prefix, known, where):
    """name -> value of the one `enum { PREFIX.. }` of the (comment-free) text; `known`: names an initialiser may refer to"""
    out = {}
    for body in re.findall(r"\benum\s*\{([^}]*)\}", text):
        items = [i.strip() for i in body.split(",") if i.strip()]
        if not items or not all(i.startswith(prefix) for i in items):
            continue
        assert not out, "%s: two enums of %s* names" % (where, prefix)
        nxt = 0
        for it in items:
            m = re.match(r"^(\w+)(?:\s*=\s*(?:par::)?(\w+))?$", it)
            assert m, "%s: cannot read the enumerator `%s`" % (where, it)
            if m.group(2) is not None:
                v = m.group(2)
                nxt = int(v.rstrip("u"), 0) if re.match(r"^(0x[0-9a-fA-F]+|\d+)u?$", v) else dict(known, **out).get(v)
                assert nxt is not None, "%s: `%s` refers to the unknown name %s" % (where, it, v)
            out[m.group(1)] = nxt
            nxt += 1
    assert out, "%s: no enum of %s* names found -- tests/chain_verdict.py reads the control words' indices from it" % (where, prefix)
    return out


_cache = {}


def source_constants(csrc=CSRC):
    """the enums C_*, A_*, W_* and the chains' limits as the sources state them -> dict name -> int.  Fails with the file and the name
    when one can no longer be read, or when a formula restated in this module no longer stands in the source"""
    if csrc in _cache:
        return _cache[csrc]
    texts, out = {}, {}

    def text_of(fname):
        if fname not in texts:
            with open(os.path.join(csrc, fname)) as f:
                texts[fname] = _strip(f.read())
        return texts[fname]
    for fname, prefix in ENUMS:
        out.update(_enum(text_of(fname), prefix, out, fname))
    for fname, names in NUMBERS:
        for name in names:
            m = re.findall(r"^\s*(?:constexpr\s+uint32_t\s+(?:\w+\s*=\s*\w+\s*,\s*)*%s\s*=|#\s*define\s+%s\s)\s*(\d+)u?\b" % (name, name), text_of(fname), flags=re.M)
            assert len(m) == 1, "%s: cannot read the constant %s (found %r) -- tests/chain_verdict.py and the chain cases derive their sizes from it" % (fname, name, m)
            out[name] = int(m[0])
    for fname, lines in RESTATED:
        flat = re.sub(r"\s+", "", text_of(fname))
        for line in lines:
            assert re.sub(r"\s+", "", line) in flat, \
                "%s no longer holds `%s`: restate the new formula in tests/chain_verdict.py (lay / fixed_pieces / passes_for)" % (fname, line)
    for name in ("C_FALLBACK", "C_OK", "C_TOTAL", "C_MARK", "C_PASS0", "C_NCROSS", "C_WORDS", "C_NOTFIXED", "A_NCAND", "A_NBLK", "A_NX", "A_NS",
                 "A_OVER", "A_WHY", "A_NREQ", "A_NREQP", "A_OPEN", "W_WALK_OWNER", "W_WALK_FIX", "W_TCAP", "W_ITEMS", "W_NODE"):
        assert name in out, "the sources no longer define %s" % name
    assert max(v for k, v in out.items() if k.startswith("A_")) < out["C_WORDS"]
    _cache[csrc] = out
    return out


Lay = collections.namedtuple("Lay", "pb nchunks candcap maxb maxreq mapcap maxx maxs tcap")


def lay(zn):
    """the list sizes of the chain for any block types for a stream (or a batch's in_len) of zn bytes: lay_of restated (RESTATED)"""
    source_constants()                                     # (the restated lines still stand in the source)
    nbits = 8 * zn
    pb = 2048 if zn >= (4 << 20) else 1024
    nchunks = (nbits + pb - 1) // pb
    candcap = nbits // 128 + 1024
    maxb = 64 if zn // 1024 < 64 else 8000 if zn // 1024 > 8000 else zn // 1024
    mapcap = min(nchunks // 16 + 1024, 2 * nchunks + 64)
    maxx = 2 * maxb + 256 + mapcap + nchunks // 8
    return Lay(pb, nchunks, candcap, maxb, 2 * maxb, mapcap, maxx, zn // 512 + 256, 3 * pb // 8)


def passes_for(nitems, k):
    passes, reach = 1, 1
    while reach < nitems + 1:
        reach *= k["HDLZ_HOPS"]
        passes += 1
    return min(passes, k["C_NCROSS"] - k["C_PASS0"])


def fixed_pieces(zn, nstr, k):
    """the pieces of the fixed-block chain for one stream of a launch of nstr streams of zn bytes: layout_of restated"""
    ztot, cb = zn * nstr, k["CH_BITS_MAX"]
    chbits = cb // 8 if ztot < (5 << 18) else cb // 4 if ztot < (3 << 20) else cb // 2 if ztot < (24 << 20) else cb
    return (8 * zn - k["FIRST_BIT"] + chbits - 1) // chbits


# ------------------------------------------------------------------------------------------------------------------------ the layout
_dbg = []


def debug_lib():
    """lib/libhdlz_dbg.so through ctypes, loaded beside the library the engine runs (RTLD_LOCAL: the two share no symbol); only its
    host arithmetic is called"""
    if not _dbg:
        own = os.environ.get("HDLZ_LIB")               # an A/B build that has the export itself (and maybe a layout of its own) answers for itself
        if own and os.path.exists(own):
            import torch  # noqa: F401
            L = ctypes.CDLL(own)
            if hasattr(L, "hdlz_debug_par_offsets"):
                _dbg.append(_typed(L))
                return _dbg[0]
        assert os.path.exists(DBG), "lib/libhdlz_dbg.so is not built: " + DBG_BUILD
        import torch  # noqa: F401  (first, as hdl_deflate_amd/_lib.py does: the HIP runtime the library needs must be torch's, or a
        #                             process that asks for the layout before it creates its engine ends up with two runtimes and no device)
        L = ctypes.CDLL(DBG, mode=getattr(ctypes, "RTLD_LOCAL", 0))
        assert hasattr(L, "hdlz_debug_par_offsets"), "lib/libhdlz_dbg.so lacks hdlz_debug_par_offsets: " + DBG_BUILD
        _dbg.append(_typed(L))
    return _dbg[0]


def _typed(L):
    L.hdlz_debug_par_offsets.restype = ctypes.c_size_t
    L.hdlz_debug_par_offsets.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32,
                                         ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]
    L.hdlz_inflate_work_bytes.restype = ctypes.c_size_t
    L.hdlz_inflate_work_bytes.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int]
    return L


Layout = collections.namedtuple("Layout", "stride o_ctl o_any")


def layout(in_len, nstreams, out_pitch, flags=0):
    """where the control words of stream 0 lie (stream s: + s * stride) -> Layout; stride 0: the whole-GPU path has no layout for the
    shape; o_any None: the chain for any block types is not launched (its share of the scratch is empty)"""
    oc, oa = ctypes.c_size_t(0), ctypes.c_size_t(0)
    stride = debug_lib().hdlz_debug_par_offsets(in_len, nstreams, out_pitch, flags, ctypes.byref(oc), ctypes.byref(oa))
    if stride == 0:
        return Layout(0, None, None)
    return Layout(stride, oc.value, oa.value if oa.value < stride else None)


class Verdict(object):
    """by: "fixed" | "any" | "serial", decided as k_par_finish decides; the counters of the chain for any block types (None when it was
    not launched); why_names: the W_* bits of `why`; fixed / any: the chain's 64 control words (None: not launched)"""
    COUNTERS = (("ncand", "A_NCAND"), ("nblk", "A_NBLK"), ("nx", "A_NX"), ("ns", "A_NS"), ("over", "A_OVER"), ("why", "A_WHY"),
                ("nreq", "A_NREQ"), ("reqp", "A_NREQP"), ("open", "A_OPEN"))

    def __init__(self, fixed, any_, fpasses, apasses, k):
        self.fixed, self.any = fixed, any_
        self.by = "serial"
        for name, _ in self.COUNTERS:
            setattr(self, name, None)
        self.total, self.why_names = None, frozenset()
        if fixed is not None:
            left = 0 if fixed[k["C_MARK"]] == 0 else fixed[k["C_PASS0"] + fpasses - 1]
            if fixed[k["C_FALLBACK"]] == 0 and left == 0:
                self.by, self.total = "fixed", fixed[k["C_TOTAL"]]
        if any_ is not None:
            for name, word in self.COUNTERS:
                setattr(self, name, any_[k[word]])
            self.why_names = frozenset(n for n, v in k.items() if n.startswith("W_") and self.why & v)
            assert self.why & ~sum(v for n, v in k.items() if n.startswith("W_")) == 0, hex(self.why)
            aleft = 0 if any_[k["C_MARK"]] == 0 else any_[k["C_PASS0"] + apasses - 1]
            if self.by == "serial" and any_[k["C_FALLBACK"]] == 0 and any_[k["C_OK"]] != 0 and aleft == 0:
                self.by, self.total = "any", any_[k["C_TOTAL"]]
        if fixed is not None:
            # k_par_finish leaves its own decision in the fixed chain's C_OK: the restated one must be the same
            assert (fixed[k["C_OK"]] != 0) == (self.by != "serial"), ("the restated verdict differs from k_par_finish's", self.by, fixed[:8])

    def __repr__(self):
        return "Verdict(%s ncand %s nblk %s nx %s ns %s over %s why %s nreq %s reqp %s total %s)" % (
            self.by, self.ncand, self.nblk, self.nx, self.ns, self.over, "+".join(sorted(self.why_names)) or self.why, self.nreq, self.reqp, self.total)


Result = collections.namedtuple("Result", "status data in_used verdict")


class Call(object):
    """one inflate_batch call with buffers of its own: launch() refills the scratch with 0x5A and calls (capturable), results() reads
    statuses, bytes and verdicts back.  zs: one stream (bytes) or a list; a list goes as one fixed-pitch batch (in_len = the pitch, every
    row zero-padded) or, ragged, as one flat buffer with offsets and in_len as the stated bound"""

    def __init__(self, engine, zs, cap, flags=0, obsize=0, ragged=False):
        import numpy as np
        import torch
        self.engine, self.cap, self.flags, self.obsize, self.ragged = engine, cap, flags, obsize, ragged
        self.single = isinstance(zs, (bytes, bytearray))
        self.zs = [bytes(zs)] if self.single else [bytes(z) for z in zs]
        n = len(self.zs)
        pitch = (max(len(z) for z in self.zs) + 64 + 15) // 16 * 16
        self.in_len = len(self.zs[0]) if self.single else pitch
        if ragged:
            assert not self.single
            self.d_in = torch.from_numpy(np.frombuffer(b"".join(self.zs) + bytes(64), np.uint8).copy()).cuda()
            self.d_off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(z) for z in self.zs])]).astype(np.int64)).cuda()
            self.rows = self.zs
        else:
            host = np.zeros((n, pitch), np.uint8)
            for i, z in enumerate(self.zs):
                host[i, :len(z)] = np.frombuffer(z, np.uint8)
            self.d_in, self.d_off = torch.from_numpy(host).cuda(), None
            self.rows = self.zs if self.single else [host[i].tobytes() for i in range(n)]      # (what the decoder reads: the oracle's input)
        wb = engine.lib.hdlz_inflate_work_bytes(n, self.in_len, cap, flags, 1 if ragged else 0)
        self.work = torch.empty(wb, dtype=torch.uint8, device="cuda")
        self.out = torch.empty((n, cap), dtype=torch.uint8, device="cuda")
        self.lay = layout(self.in_len, n, cap, flags)
        # one group: launch_inflate_par takes the caller's scratch as its budget, group_size keeps all n streams together when
        # n * stride fits in it, and layout_of for n streams is what the debug call evaluated
        if self.lay.stride:
            assert self.lay.stride * n <= wb, ("the scratch of hdlz_inflate_work_bytes does not hold the batch as ONE group", n, self.lay.stride, wb)
            assert self.lay.o_ctl % 256 == 0 and (self.lay.o_any is None or (self.lay.o_any % 256 == 0 and 0 < self.lay.o_any < self.lay.stride))
        self.res = None

    def launch(self):
        self.work.fill_(0x5A)
        self.res = self.engine.inflate_batch(self.d_in, in_off=self.d_off, in_len=self.in_len, out_pitch=self.cap, flags=self.flags,
                                             obsize=self.obsize, out=self.out, work=self.work)

    def results(self):
        import torch
        torch.cuda.synchronize()
        k = source_constants()
        out, ol, st = self.res[0].cpu().numpy(), self.res[1].cpu().numpy(), self.res[2].cpu().numpy()
        n, L = len(self.zs), self.lay
        words = self.work.view(torch.int32)
        got = []
        fpasses = passes_for(fixed_pieces(self.in_len, n, k), k)
        a = lay(self.in_len)
        apasses = passes_for(a.nchunks + a.maxx, k)
        for s in range(n):
            fixed = any_ = None
            if L.stride:
                o = (s * L.stride + L.o_ctl) // 4
                fixed = [v & 0xFFFFFFFF for v in words[o:o + k["C_WORDS"]].cpu().tolist()]
                if L.o_any is not None:
                    o = (s * L.stride + L.o_any) // 4
                    any_ = [v & 0xFFFFFFFF for v in words[o:o + k["C_WORDS"]].cpu().tolist()]
            got.append(Result(int(st[s]), out[s, :int(ol[s])].tobytes(), None, Verdict(fixed, any_, fpasses, apasses, k)))
        return got


def run(engine, zs, cap, flags=0, obsize=0, ragged=False):
    """one stream (bytes) or a batch (list) through Engine.inflate_batch -> Result (status, bytes, in_used: None -- inflate_batch does
    not report it --, Verdict), or a list of them"""
    c = Call(engine, zs, cap, flags, obsize, ragged)
    c.launch()
    r = c.results()
    return r[0] if c.single else r
