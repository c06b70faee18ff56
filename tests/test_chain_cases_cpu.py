"""CPU: the crafted streams for the limits of the whole-GPU inflate chains (deflate_craft.chain_cases) against stock zlib and the C
oracle, their declared properties against the constants in the kernels' sources, and the reader of those sources (chain_verdict.py).

tests/test_gpu_chain_verdicts.py asserts which chain delivered each of these streams; that only means something while each stream sits
where its name says: on the last value a limit takes or on the first it gives up.  Here every such property is measured from the case's
own records and held against the limit computed from the sources, every embedded header image is read by stock zlib as the block header
it pretends to be, and the check itself is shown to notice a limit that moves."""
import os
import re
import shutil
import time
import zlib

import pytest

from conftest import REPO
import chain_verdict as V
import deflate_craft as C

# the values the verdicts of tests/test_gpu_chain_verdicts.py were recorded with.  A limit that moves fails here, with the cases that sit
# on it: the builder follows most constants, the pinned verdicts and profiles/chain_verdicts.txt do not
RECORDED_WITH = dict(PB_MAX=2048, FIX_MAX_BITS=16384, FIRST_FIX_BITS=4096, WALK_ROUNDS=3, REQ_MAX=1024, ANY_MIN=4096, MAXCROSS=4096,
                     CH_MAX=8, HEAD=256)
LIMIT_OF = dict(FIX_MAX_BITS="FIX", FIRST_FIX_BITS="FIRST_FIX", WALK_ROUNDS="WALK", MAXCROSS="MAXCROSS", REQ_MAX="REQ_MAX")


def test_the_sources_can_be_read(tmp_path):
    k = V.source_constants()
    for name in ("PB_MAX", "FIX_MAX_BITS", "FIRST_FIX_BITS", "WALK_ROUNDS", "REQ_MAX", "ANY_MIN", "MAXCROSS", "CH_MAX", "HEAD"):
        assert k[name] > 0, name
    assert len(set(v for n, v in k.items() if n.startswith("W_"))) == len([n for n in k if n.startswith("W_")]) >= 15
    assert all(v & (v - 1) == 0 for n, v in k.items() if n.startswith("W_"))             # bits
    assert sorted(v for n, v in k.items() if n.startswith("A_")) == list(range(k["C_ANY0"], k["C_ANY0"] + 9))
    assert k["PB_MAX"] == max(V.lay(1 << 20).pb, V.lay(8 << 20).pb) and V.lay(4096).maxb == 64
    # ... and a source it can no longer read says which name is missing
    for fname, old, new, word in (("hdlz_inflate_any.hip", r"constexpr uint32_t WALK_ROUNDS = \d+;", "constexpr uint32_t WALK_ROUNDS = ROUNDS;", "WALK_ROUNDS"),
                                  ("hdlz_inflate_any.hip", r"enum \{ W_OVER = 1,", "enum { X_OVER = 1,", "W_"),
                                  ("hdlz_inflate_any.hip", r"L\.maxs = zn / 512u \+ 256u;", "L.maxs = zn / 256u + 256u;", "L.maxs"),
                                  ("hdlz_inflate_par.h", r"enum \{ C_FALLBACK = 0,", "enum { C_FALLBACK = FIRST,", "C_FALLBACK")):
        d = str(tmp_path / ("csrc_" + re.sub(r"\W", "", word)))
        shutil.copytree(V.CSRC, d, ignore=shutil.ignore_patterns("_obj*", "*.o"))
        with open(os.path.join(d, fname)) as f:
            text = f.read()
        assert len(re.findall(old, text)) == 1, old
        with open(os.path.join(d, fname), "w") as f:
            f.write(re.sub(old, new, text))
        with pytest.raises(AssertionError) as e:
            V.source_constants(d)
        assert word in str(e.value) and fname in str(e.value), str(e.value)


def test_generation_stays_quick():
    t0 = time.time()
    cs = C.chain_cases()
    assert time.time() - t0 < 30 and len(cs) >= 45
    assert sum(1 for c in cs if c.big) == 2 and all(len(c.z) <= 140000 for c in cs if not c.big)


def test_the_gpu_module_names_every_case():
    import test_gpu_chain_verdicts as G
    assert G.CASE_NAMES == tuple(c.name for c in C.chain_cases())


def test_every_valid_case_inflates_to_its_plain_bytes(oracle):
    for c in C.chain_cases():
        if c.plain is None:
            continue
        assert zlib.decompress(c.z) == c.plain, c.name
        assert oracle.inflate(c.z, out_cap=len(c.plain) + 64) == (0, c.plain), c.name


def test_damaged_cases_are_rejected(oracle):
    bad = [c for c in C.chain_cases() if c.plain is None]
    assert len(bad) == 2 and sorted(c.name.split(":")[0] for c in bad) == ["damaged (header)", "damaged (payload)"]
    for c in bad:
        n = c.neighbour
        assert len(c.z) == len(n.z) and sum(bin(a ^ b).count("1") for a, b in zip(c.z, n.z)) == 1
        rc, got = oracle.inflate(c.z, out_cap=len(n.plain) + 64)
        assert rc != 0, (c.name, rc)
        with pytest.raises(zlib.error):
            zlib.decompress(c.z)


def _blocks_measured(c):
    """the bit positions of the case's records, measured again from its tokens: every block begins where the one before it ended, a
    payload and its tokens' bits end at the end-of-block code"""
    pos = 16
    for r in c.records:
        assert r["hdr"] == pos, (c.name, r["kind"], r["hdr"], pos)
        if r["kind"] == "zlib":                        # (bulk made by zlib: whole bytes, closed with a full flush)
            assert r["hdr"] % 8 == 0 and c.z[r["end"] // 8 - 4:r["end"] // 8] == b"\x00\x00\xff\xff"
        elif r["kind"] == "stored":
            assert r["data"] == (r["hdr"] + 3 + 7) // 8 * 8 + 32 and r["end"] == r["data"] + 8 * r["length"]
            assert c.z[r["data"] // 8 - 4:r["data"] // 8 - 2] == r["length"].to_bytes(2, "little")
        else:
            n = sum(C.token_bits(r["ll"], r["dl"], r["tokens"])) if r["tokens"] is not None else r["ntokens"]
            assert r["pay"] + n == r["eob"] and r["eob"] + r["ll"][256] == r["end"], (c.name, r["kind"])
            assert (int.from_bytes(c.z[r["hdr"] // 8:r["hdr"] // 8 + 2], "little") >> (r["hdr"] % 8 + 1)) & 3 == (2 if r["kind"] == "dynamic" else 1)
        pos = r["end"]


def test_every_declared_property_is_measured():
    K = V.source_constants()
    wrong = []
    for c in C.chain_cases():
        if c.plain is None:
            continue
        _blocks_measured(c)
        L = V.lay(len(c.z))
        wrong += C.off_limit(c, K, L)
        # what the properties claim, counted again from the records
        fixed = [r for r in c.records if r["kind"] == "fixed"]
        stored = [r for r in c.records if r["kind"] == "stored" and r["length"]]
        for what, (m, key, side) in c.props.items():
            if key == "MAXCROSS":
                assert m == len(fixed) == len(c.records)
            elif key == "maxs":
                assert m == len(stored) and len(c.records) == m + 20 and not c.ndyn
            elif key == "maxb":
                assert m == c.ndyn + len(c.images)
            elif key == "WALK":
                assert m == len(c.images)
                w = [r for r in c.records if r.get("ll") == C.WRITER_LL][0]
                pays = [b + C.header_image()[1] for b in c.images] + [w["eob"]]
                assert all(w["pay"] < b for b in c.images) and min(b - a for a, b in zip(pays, pays[1:])) >= 3 * L.pb      # a whole piece of its own behind every image
            elif key in ("FIX", "FIRST_FIX"):
                r = fixed[0]
                assert m == r["eob"] - r["pay"]
                starts = C.fixed_walk_starts(r["pay"], C.token_bits(r["ll"], r["dl"], r["tokens"]) + [7], L.pb)
                if key == "FIX":                       # k_any_walk gives the block up when it would begin an item FIX_MAX_BITS behind the payload
                    assert (max(starts) >= r["pay"] + K["FIX_MAX_BITS"] or r["eob"] >= max(starts) + L.pb) == (side == "first"), c.name
            elif key == "candcap":
                assert m == len(C.find_passes(c.z))
            elif key == "tcap":
                r = [r for r in c.records if r.get("ll") == C.ONE_BIT_LL][0]
                assert (r["eob"] - r["pay"]) // L.pb >= 15 and r["ll"][97] == 1
        if c.expect == "any":                          # the gate of the chain for any block types: no fixed block first, or a short one
            assert (c.z[2] >> 1) & 3 != 1 or c.exactly.get("open") == 1, c.name
        assert len(c.z) >= K["ANY_MIN"], c.name
    assert not wrong, wrong
    # each limit has a case on its last taken value and one on the first given up
    sides = {}
    for c in C.chain_cases():
        for m, key, side in c.props.values():
            sides.setdefault(key, set()).add(side)
    for key in ("FIX", "FIRST_FIX", "WALK", "MAXCROSS", "maxb", "maxs", "candcap"):
        assert {"last", "first"} <= sides[key], (key, sides[key])
    assert {0, 1, 1023} <= sides["pb"] and set(range(8)) <= sides["byte"]


def test_a_limit_that_moves_is_noticed():
    """the check of the test above, tried: with one constant changed the cases of that limit, and no others, are reported"""
    K, cs = V.source_constants(), [c for c in C.chain_cases() if c.plain is not None]
    for name, value in (("FIX_MAX_BITS", K["FIX_MAX_BITS"] // 2), ("FIX_MAX_BITS", K["FIX_MAX_BITS"] + 1), ("FIRST_FIX_BITS", K["FIRST_FIX_BITS"] + 1),
                        ("WALK_ROUNDS", K["WALK_ROUNDS"] + 1), ("WALK_ROUNDS", K["WALK_ROUNDS"] - 1), ("MAXCROSS", K["MAXCROSS"] - 1),
                        ("MAXCROSS", 2 * K["MAXCROSS"]), ("REQ_MAX", 2 * K["REQ_MAX"])):
        named = [x for c in cs for x in C.off_limit(c, dict(K, **{name: value}), V.lay(len(c.z)))]
        want = set(c.name for c in cs if any(key == LIMIT_OF[name] and side != "below" for m, key, side in c.props.values()))
        may = set(c.name for c in cs if any(key == LIMIT_OF[name] for m, key, side in c.props.values()))
        got = set(x.split(": ")[0] + ": " + x.split(": ")[1] for x in named)
        assert want and want <= got <= may, (name, value, named)
    for field, shift in (("maxb", -32), ("maxb", 1), ("maxs", 1), ("candcap", -1), ("maxx", 2000), ("tcap", 1024), ("pb", 1024)):
        named = [x for c in cs for x in C.off_limit(c, K, V.lay(len(c.z))._replace(**{field: getattr(V.lay(len(c.z)), field) + shift}))]
        assert named and all(field in x for x in named), (field, named)


def test_the_limits_are_those_the_verdicts_were_recorded_with():
    K = V.source_constants()
    moved = [n for n, v in RECORDED_WITH.items() if K[n] != v]
    cs = C.chain_cases()
    on = dict((n, [c.name for c in cs if any(key == LIMIT_OF.get(n) for m, key, side in c.props.values())]) for n in moved)
    assert not moved, ("these constants moved; the cases on them follow, so run tests/test_gpu_chain_verdicts.py on a GPU, record "
                       "profiles/chain_verdicts.txt again and update RECORDED_WITH", dict((n, (RECORDED_WITH[n], K[n], on[n])) for n in moved))
    assert V.lay(60000).maxb == 64 and V.lay(5000).maxs == 5000 // 512 + 256, "the list sizes of lay_of moved: as above"


def test_every_header_image_is_a_header_to_stock_zlib():
    img, hbits = C.header_image()
    n = 0
    for c in C.chain_cases():
        for bit in c.images:
            tail = c.z[bit >> 3:(bit >> 3) + len(img) + 1]
            shifted = (int.from_bytes(tail, "little") >> (bit & 7)).to_bytes(len(tail), "little")[:len(img)]
            assert shifted == img, (c.name, bit)
            d = zlib.decompressobj(-15)
            assert d.decompress(shifted) == b"a" * 8 and d.eof, (c.name, bit)        # the header and its symbols, to the end-of-block code
            n += 1
    assert n >= 1 + 2 + 3 + 1 + 62 + 63 + 64 + 2 and hbits == 101
    assert all(len(C.find_passes(c.z[:2] + img + bytes(8))) >= 1 for c in C.chain_cases()[:1])       # ... and to k_any_find's tests


def _gpu_shapes():
    """(in_len, streams, out_pitch) of the calls tests/test_gpu_chain_verdicts.py makes with the chain cases"""
    cs = C.chain_cases()
    small = [c for c in cs if not c.big]
    cap = lambda c: (len(c.plain if c.plain is not None else c.neighbour.plain) + 64 + 15) // 16 * 16
    pitch = (max(len(c.z) for c in small) + 64 + 15) // 16 * 16
    return [(len(c.z), 1, cap(c)) for c in cs] + [(pitch, len(small), max(cap(c) for c in small))]


def test_the_debug_variant_lays_the_control_words_out():
    """lib/libhdlz_dbg.so on the CPU (host arithmetic only): for every shape of the GPU test the fixed-block chain's control words lie at
    the front of a stream's scratch (offset 0: layout_of hands them out first), the other chain's at a non-zero offset, both 256-aligned
    and below the stride, and the scratch hdlz_inflate_work_bytes asks for holds all streams at that stride -- one group"""
    L, K = V.debug_lib(), V.source_constants()
    for in_len, n, cap in _gpu_shapes():
        lay = V.layout(in_len, n, cap)
        assert lay.stride and lay.stride % 256 == 0 and lay.o_ctl == 0, (in_len, n, lay)
        assert lay.o_any is not None and lay.o_any % 256 == 0 and 4 * K["C_WORDS"] <= lay.o_any <= lay.stride - 4 * K["C_WORDS"], (in_len, n, lay)
        for ragged in (0, 1):
            assert lay.stride * n <= L.hdlz_inflate_work_bytes(n, in_len, cap, 0, ragged), (in_len, n, ragged)
    assert V.layout(K["ANY_MIN"] - 1, 1, 65536).o_any is None             # below ANY_MIN the chain for any block types is not launched
    assert V.layout(5000, 65, 65536).o_any is None                       # ... nor for more streams than any_batch_max
    assert V.layout(5000, 1, 65536, 128).o_any is None                   # ... nor under the one-fixed-block hint
