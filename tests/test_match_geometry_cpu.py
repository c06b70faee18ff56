"""CPU: the crafted match geometry of tests/deflate_craft.py against stock zlib and the C oracle, and the grid against the kernels.

Every inflate decoder chooses by comparisons of a match's distance and length with constants of its own whether the source bytes come
out of its LDS ring, out of its flushed output or out of a marker resolved later.  The generator puts distances and lengths on those
comparisons and next to them; here its streams are held against stock zlib and the oracle -- the checker of every GPU test in
tests/test_gpu_match_geometry.py --, its coverage is asserted so that it cannot rot into easy cases, and the grids are recomputed from
the constants in the kernels' sources: a ring that changes its size fails this file until the grid moves with it."""
import os
import re
import time
import zlib

from conftest import REPO
import deflate_craft as C

CSRC = os.path.join(REPO, "hdl_deflate_amd", "csrc")
CONSTANTS = (("hdlz_inflate_tok.hip", ("HDLZ_TOK_RING",)), ("hdlz_inflate_grp.hip", ("RB", "FLUSH")),
             ("hdlz_inflate_dyn.hip", ("DRING", "WCAP", "DCHUNK")), ("hdlz_inflate_par.hip", ("HRING", "SPAN")))


def zlib_verdict(z):
    """-> (accepted, bytes): accepted = stock zlib reaches the end of the stream, checksum included"""
    d = zlib.decompressobj()
    try:
        out = d.decompress(z)
    except zlib.error:
        return False, None
    return d.eof, out


def kernel_constants(csrc=CSRC):
    """the ring sizes as the kernels' sources state them: `constexpr uint32_t NAME = <number>` or `#define NAME <number>`"""
    out = {}
    for fname, names in CONSTANTS:
        with open(os.path.join(csrc, fname)) as f:
            text = f.read()
        for name in names:
            m = re.findall(r"^\s*(?:constexpr\s+uint32_t\s+%s\s*=|#\s*define\s+%s\s)\s*(\d+)u?\b" % (name, name), text, flags=re.M)
            assert len(m) == 1, (fname, name, m)
            out[name] = int(m[0])
    return out


def thresholds(k):
    """name -> the derived comparison values of the kernels (the expressions behind NEAR, URGENT, HREACH and the ring test of k_inflate_dyn)"""
    t = {"tok NEAR = RINGB - 16": k["HDLZ_TOK_RING"] - 16, "tok NEAR + 3": k["HDLZ_TOK_RING"] - 16 + 3, "tok URGENT = RINGB - 52": k["HDLZ_TOK_RING"] - 52,
         "grp NEAR = RB - 32": k["RB"] - 32, "dyn DRING - 512": k["DRING"] - 512, "par HREACH = HRING - 128": k["HRING"] - 128}
    for l in (3, 16, 64, 258):
        t["dyn DRING - 512 - %d" % l] = k["DRING"] - 512 - l
    return t


def grid_gaps(k):
    """what GEO_DISTANCES lacks of T - 1, T, T + 1 over the thresholds of the constants k"""
    return [(name, v) for name, T in sorted(thresholds(k).items()) for v in (T - 1, T, T + 1) if v not in C.GEO_DISTANCES]


def test_generation_stays_quick():
    """a few seconds on one core; the bound only catches a writer gone quadratic"""
    t0 = time.time()
    [C.geometry_stream(D, kind, long_) for D in C.GEO_DISTANCES for kind in C.GEO_KINDS for long_ in (False, True)]
    C.geometry_rejected()
    C.geometry_mixed(1, "fixed", 1 << 20)
    C.geometry_mixed(2, "dynamic", 1 << 20)
    assert time.time() - t0 < 30


def test_the_grid_follows_the_kernels():
    k = kernel_constants()
    assert sorted(k) == sorted(["HDLZ_TOK_RING", "RB", "DRING", "WCAP", "DCHUNK", "HRING", "SPAN", "FLUSH"])
    assert not grid_gaps(k), grid_gaps(k)
    for name in ("WCAP", "DCHUNK", "SPAN", "FLUSH", "HRING", "RB", "DRING", "HDLZ_TOK_RING"):      # the sizes themselves
        assert all(v in C.GEO_DISTANCES for v in (k[name] - 1, k[name], k[name] + 1)), name
    assert C.GEO_DISTANCES == tuple(sorted(C.GEO_DISTANCES)) and len(C.GEO_DISTANCES) == 116 and len(C.GEO_LENGTHS) == 39
    assert min(C.GEO_DISTANCES) == 1 and max(C.GEO_DISTANCES) == 32768 and (min(C.GEO_LENGTHS), max(C.GEO_LENGTHS)) == (3, 258)
    # the check itself: a ring of another size is noticed
    for name in ("HDLZ_TOK_RING", "RB", "DRING", "HRING"):
        assert grid_gaps(dict(k, **{name: k[name] // 2 + 40})), name


def test_helpers():
    import random
    assert C.canonical(C.FIXED_LL)[0] == (0b00001100, 8) and C.canonical(C.FIXED_LL)[144] == (0b000010011, 9)      # 00110000, 110010000 reversed
    assert C.canonical(C.FIXED_LL)[256] == (0, 7) and C.canonical(C.FIXED_LL)[280] == (0b00000011, 8) and C.canonical(C.FIXED_DL)[29] == (0b10111, 5)
    w = C.Bits()
    b = C.emit_fixed_block(w, [97, (258, 1), (3, 1)], True)
    assert b["span"] == (0, 3) and w.pos == 3 + 8 + (8 + 5) + (7 + 5) + 7
    assert C.token_bits(C.FIXED_LL, C.FIXED_DL, [97, 200, (258, 1), (3, 32768), (257, 5)]) == [8, 9, 13, 7 + 5 + 13, 8 + 5 + 5 + 1]
    assert zlib.decompress(C.wrap(w.bytes(), b"a" * 262)) == b"a" * 262
    r = random.Random(3)
    for n in (1, 2, 3, 40, 286):
        for shape in ("flat", "steep"):
            freq = dict((s, 1 if shape == "flat" else 1 << min(s, 40)) for s in r.sample(range(286), n))
            lens = C.limited_lengths(freq)
            assert sorted(lens) == sorted(freq) and max(lens.values()) <= 15
            assert C.kraft(lens.values()) == (1 << 15 if n > 1 else 1 << 14)
    assert max(C.limited_lengths(dict((s, 1 << s) for s in range(40))).values()) == 15                           # (it was limited)
    assert C.limited_lengths({0: 8, 1: 4, 2: 2, 3: 1, 4: 1}) == {0: 1, 1: 2, 2: 3, 3: 4, 4: 4}
    ll, dl = C.frequency_lengths([97] * 9 + [(5, 3)] * 4 + [98])
    assert len(ll) == 260 and ll[256] and ll[259] and ll[97] == 1 and dl == [0, 0, 1]
    assert C.frequency_lengths([97, 98]) == (C.sparse(257, {97: 2, 98: 2, 256: 1}), [0])
    assert C.frequency_lengths([])[0] == C.sparse(257, {256: 1})


def test_every_stream_zlib_and_oracle_agree(oracle):
    """the same verdict from stock zlib and from the oracle, the status the generator states, the bytes of its own tokens"""
    G = C.geometry()
    assert [len(G[k]) for k in ("short", "long", "reach", "short_by_one", "obsize")] == [232, 232, 12, 10, 4]
    cases = G["short"] + G["long"] + G["reach"] + G["short_by_one"] + G["obsize"] + list(C.geometry_large())
    assert len(set(c.name for c in cases)) == len(cases)
    for c in cases:
        ok, out = zlib_verdict(c.z)
        rc, ref = oracle.inflate(c.z, out_cap=(1 << 20) + 4096)
        assert ok == (rc == 0), (c.name, "zlib accepts" if ok else "zlib rejects", "oracle status", rc)
        assert rc == c.status, (c.name, rc, c.status)
        if ok:
            assert out == c.plain and ref == c.plain, c.name
        else:
            assert ref == b"" and c.plain is None
    assert [c.status for c in G["short_by_one"]] == [C.E_BAD_DISTANCE] * 10 and all(c.status == 0 for c in G["reach"])
    for c in G["reach"]:
        assert len(c.plain) == c.D + 258 and c.plain[c.D:] == (c.plain[:c.D] * (258 // c.D + 1))[:258], c.name      # (from byte 0 on)
    for c in G["obsize"]:
        for obsize in (c.D - 1, c.D, c.D + 1, 0):
            rc, ref = oracle.inflate(c.z, obsize=obsize)
            assert (rc == C.E_BAD_DISTANCE) == (obsize != 0 and obsize < c.D + 1) and rc in (0, C.E_BAD_DISTANCE), (c.name, obsize, rc)
            assert ref == (c.plain if rc == 0 else b"")


def test_what_the_streams_are_made_of():
    G = C.geometry()
    seen = set()
    for k, c in enumerate(G["short"] + G["long"]):
        D, kind = C.GEO_DISTANCES[(k % 232) // 2], C.GEO_KINDS[k % 2]
        assert (c.D, c.kind) == (D, kind) and len(c.blocks) == 1 and (c.raw[0] & 7) == (3 if kind == "fixed" else 5)
        pre, body = c.tokens[:c.first_match], c.tokens[c.first_match:]
        assert all(isinstance(t, int) for t in pre) and not isinstance(body[0], int)
        lo = max(D, 64, 4400 if k >= 232 else 0)
        assert lo <= len(pre) < lo + 64
        assert sorted(t[0] for t in body if not isinstance(t, int)) == list(C.GEO_LENGTHS) and all(t[1] == D for t in body if not isinstance(t, int))
        gaps, run = [], 0
        for t in body[1:] + [(0, 0)]:
            if isinstance(t, int):
                run += 1
            else:
                gaps.append(run)
                run = 0
        assert len(gaps) == 39 and max(gaps) <= 3
        seen |= set(gaps)
        if k >= 232:
            assert len(c.z) >= 4400 > 4096                           # above HDLZ_INFLATE_PAR_MIN (2048) and ANY_MIN (4096)
    assert seen == set((0, 1, 2, 3))
    assert set(G["short"][-1].tokens[:32768]) == set(range(256))                                                # (random literals: all of them)
    # the same tokens in both kinds
    for a, b in zip(G["short"][0::2], G["short"][1::2]):
        assert a.tokens == b.tokens and a.plain == b.plain and a.raw != b.raw
    fixed, dyn = C.geometry_large()
    for c, nblocks in ((fixed, 1), (dyn, 3)):
        assert len(c.blocks) == nblocks and 1 << 20 <= len(c.plain) < (1 << 20) + 262 and 60000 < len(c.tokens) <= 30000 * max(nblocks, 3)
        ms = [t for t in c.tokens if not isinstance(t, int)]
        assert set(t[0] for t in ms) == set(C.GEO_LENGTHS) and set(t[1] for t in ms) == set(C.GEO_DISTANCES)
        assert 80000 < len(c.z) < 110000
    assert (fixed.raw[0] & 7) == 3 and (dyn.raw[0] & 7) == 4


def test_coverage_of_what_was_generated():
    G = C.geometry()
    dyn = [c for c in G["short"] if c.kind == "dynamic"]
    assert len(dyn) == 116
    stats = [C.window_stats(c) for c in dyn]
    assert sum(1 for m, b in stats if m >= 3) >= 100, stats                    # three matches begin within one 64-bit decode window
    assert sum(1 for m, b in stats if b > 448) >= 60, stats                    # one window's tokens exceed WCAP output bytes
    # window_stats against a count that slides bit by bit
    for c in dyn[::29]:
        body = list(zip(c.token_pos, c.tokens))[c.first_match:]
        bm = bb = 0
        for p0 in range(body[0][0] - 63, body[-1][0] + 1):
            inside = [t for p, t in body if p0 <= p < p0 + 64]
            bm = max(bm, sum(1 for t in inside if not isinstance(t, int)))
            bb = max(bb, sum(1 if isinstance(t, int) else t[0] for t in inside))
        assert (bm, bb) == C.window_stats(c), c.name
    for c in G["short"] + G["long"]:
        ms = [t for t in c.tokens if not isinstance(t, int)]
        if 3 <= c.D <= 257:                                                   # (inside the length grid's range)
            assert any(t[1] < t[0] for t in ms) and any(t[1] >= t[0] for t in ms), c.name
        # token_pos: the last token ends where the end-of-block code begins
        assert c.token_pos == sorted(c.token_pos) and c.token_pos[-1] < 8 * len(c.raw)
    phases = set(c.first_match % 64 for c in G["short"] + G["long"])
    assert len(phases) >= 48, sorted(phases)
    assert max(len(c.plain) for c in G["short"] + G["long"]) <= 65536 - 16
