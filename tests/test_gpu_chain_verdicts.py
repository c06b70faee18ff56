"""GPU (-m gpu): which of the two whole-GPU inflate chains delivered a stream -- asserted, not inferred from a timing.

k_par_* (hdlz_inflate_par.hip: streams of fixed blocks) and k_any_* (hdlz_inflate_any.hip: any block types) hand whatever they cannot do
to the serial decoder, whose bytes are as good: a chain that rejected every 15-bit code or never repaired a false positive would pass
every bytes-against-oracle test.  Here every stream goes through tests/chain_verdict.py, which reads the chains' control words out of the
call's scratch: the crafted streams of deflate_craft.chain_cases() -- one on the last value each limit takes, one on the first it gives
up -- must get the verdict they declare, alone, in a fixed-pitch and a ragged batch, and in a captured graph; the large crafted streams
of the other suites and a few natural ones have their verdicts pinned below.  Status, length and bytes are the oracle's throughout.
The kernels run in the library the session's engine loaded; lib/libhdlz_dbg.so is loaded beside it only to ask where the words lie."""
import os
import zlib

import pytest

import chain_verdict as V
import deflate_craft as C

pytestmark = pytest.mark.gpu

# the names of deflate_craft.chain_cases(), so that collecting this module generates nothing (tests/test_chain_cases_cpu.py holds the
# list against the generator)
CASE_NAMES = (
    "trees: 15-bit codes", "trees: 7-bit code-length code", "trees: HLIT 257", "trees: HLIT 286", "trees: one-code distance set",
    "trees: empty distance set", "trees: repeat crosses into the distances",
    "position: payload at 0 mod 1024", "position: payload at 1 mod 1024", "position: payload at 1023 mod 1024", "position: header at 1023 mod 1024",
    "end-of-block: a 15-bit code that starts at 1023 mod 1024", "end-of-block: a 15-bit code that starts at 0 mod 1024",
    "false positives: 1 in a row inside one block", "false positives: 2 in a row inside one block", "false positives: 3 in a row inside one block",
    "false positives: a request longer than REQ_MAX pieces",
    "lists: 63 candidate blocks", "lists: 64 candidate blocks", "lists: 65 candidate blocks",
    "lists: no more than candcap positions pass the search", "lists: one more than candcap positions pass the search",
    "stored: no more non-empty stored blocks than maxs", "stored: one more non-empty stored blocks than maxs",
    "stored: the last block ends at the trailer, header at bit 0", "stored: the last block ends at the trailer, header at bit 1",
    "stored: the last block ends at the trailer, header at bit 2", "stored: the last block ends at the trailer, header at bit 3",
    "stored: the last block ends at the trailer, header at bit 4", "stored: the last block ends at the trailer, header at bit 5",
    "stored: the last block ends at the trailer, header at bit 6", "stored: the last block ends at the trailer, header at bit 7",
    "fixed: a block of 16393 bits behind a dynamic one", "fixed: a block of 16394 bits behind a dynamic one",
    "fixed first: its end-of-block code 4095 bits in, a dynamic block behind it", "fixed first: its end-of-block code 4095 bits in, a stored block behind it",
    "fixed first: its end-of-block code 4096 bits in, a dynamic block behind it", "fixed first: its end-of-block code 4096 bits in, a stored block behind it",
    "fixed first: another fixed block behind it", "fixed chain: 4096 short fixed blocks", "fixed chain: 4097 short fixed blocks",
    "tokens: one stretch of 16 pieces with a token per bit", "tokens: a token per bit throughout",
    "pb = 2048: positions of headers and payloads", "pb = 2048: two false positives in a row",
    "damaged (header): position: payload at 0 mod 1024",
    "damaged (payload): end-of-block: a 15-bit code that starts at 1023 mod 1024")

_oracle_memo, _alone_memo = {}, {}


def _ref(oracle, z, cap):
    if (z, cap) not in _oracle_memo:
        _oracle_memo[(z, cap)] = oracle.inflate(z, out_cap=cap)
    return _oracle_memo[(z, cap)]


def _cap(n):
    return (n + 64 + 15) // 16 * 16


def _case_cap(c):
    return _cap(len(c.plain if c.plain is not None else c.neighbour.plain))


def _case(name):
    return dict((c.name, c) for c in C.chain_cases())[name]


def _alone(engine, c):
    if c.name not in _alone_memo:
        _alone_memo[c.name] = V.run(engine, c.z, _case_cap(c))
    return _alone_memo[c.name]


def _shows(v, evidence, K):
    """does the verdict show the named reason of a give-up?"""
    if evidence.startswith("W_"):
        return evidence in v.why_names
    if evidence == "A_OVER":
        return v.over != 0
    if evidence == "C_NCROSS":                         # k_par_ends: more end-of-block codes than the list holds
        return v.fixed[K["C_NCROSS"]] > K["MAXCROSS"]
    if evidence == "A_OPEN":                           # k_any_zero left the gate shut: no kernel of the chain ran, all its words are zero
        return v.open == 0 and not any(v.any)
    raise AssertionError(evidence)


def _judge(c, r, expect, ref, what):
    """one stream's result against the oracle's (status, bytes), its verdict against the declared one"""
    K = V.source_constants()
    v = r.verdict
    assert (r.status, len(r.data)) == (ref[0], len(ref[1])) and r.data == ref[1], (what, c.name, r.status, len(r.data), ref[0], len(ref[1]), v)
    if c.plain is not None:
        assert r.status == 0 and r.data == c.plain, (what, c.name)
    else:
        assert r.status != 0 and v.by == "serial", (what, c.name, r.status, v)
        return
    assert v.by == expect, (what, c.name, "expected " + expect, v)
    if expect == "serial":
        assert any(_shows(v, e, K) for e in c.evidence), (what, c.name, "no sign of " + " / ".join(c.evidence), v)
    else:
        assert not v.why and not v.over, (what, c.name, v)
    if expect == c.expect:                             # (the counters of the stream under the list sizes it was built for)
        for name, n in c.exactly.items():
            assert getattr(v, name) == n, (what, c.name, name, n, v)
        for name, n in c.at_least.items():
            assert getattr(v, name) is not None and getattr(v, name) >= n, (what, c.name, name, n, v)


def test_the_debug_variant_is_built():
    assert os.path.exists(V.DBG), "lib/libhdlz_dbg.so is not built: " + V.DBG_BUILD
    assert V.layout(5000, 1, 65536).stride


def test_the_names_are_the_generators():
    assert CASE_NAMES == tuple(c.name for c in C.chain_cases())


# ------------------------------------------------------------------------------------------------------ the crafted limits, one call each
@pytest.mark.parametrize("name", CASE_NAMES)
def test_case_alone(engine, oracle, name):
    c = _case(name)
    r = _alone(engine, c)
    _judge(c, r, c.expect, _ref(oracle, c.z, _case_cap(c)), "alone")
    if c.expect == "any":
        assert r.verdict.total == len(c.plain)


# ------------------------------------------------------------------------------------------------------ ... and together
def _small():
    return [c for c in C.chain_cases() if not c.big]


def _judge_batch(call, oracle, what):
    cs = _small()
    L = V.lay(call.in_len)                             # the lists of the chain for any block types are sized by the call's in_len
    got = call.results()
    changed = []
    for c, r, row in zip(cs, got, call.rows):
        expect = c.expect_at(L)
        _judge(c, r, expect, _ref(oracle, row, call.cap), what)
        if expect != c.expect:
            changed.append(c.name)
    # the streams whose verdict the longer in_len changes are the ones built on a list size, and only those
    assert sorted(changed) == sorted(c.name for c in cs if c.expect == "serial" and set(c.evidence) & {"A_OVER", "W_TCAP"}
                                     and c.expect_at(L) == "any"), changed
    return got


@pytest.mark.parametrize("ragged", (False, True))
def test_cases_in_one_batch(engine, oracle, ragged):
    """all but the two 4 MiB streams in ONE call, valid and damaged ones, taken and given up: every stream gets the verdict it got alone --
    a give-up or a damaged stream does not drag a neighbour down.  (A stream that is given up alone because one of ITS lists is full
    -- maxb, maxs, candcap, maxx: sized by in_len -- is taken in a call whose in_len is larger: expect_at says which.)"""
    cs = _small()
    call = V.Call(engine, [c.z for c in cs], max(_case_cap(c) for c in cs), ragged=ragged)
    call.launch()
    _judge_batch(call, oracle, "ragged batch" if ragged else "fixed-pitch batch")


def test_one_batch_in_a_hip_graph(engine, oracle):
    """the fixed-pitch batch captured once and replayed three times, the scratch refilled with 0x5A (inside the graph and in front of
    every replay) and the output cleared: the same verdicts and bytes every time"""
    import torch
    cs = _small()
    call = V.Call(engine, [c.z for c in cs], max(_case_cap(c) for c in cs))
    call.launch()
    first = _judge_batch(call, oracle, "eager")
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(s), torch.cuda.graph(g, stream=s):
        call.launch()
    for rep in range(3):
        call.out.zero_()
        call.work.fill_(0x5A)
        g.replay()
        got = _judge_batch(call, oracle, "graph replay %d" % rep)
        for c, a, b in zip(cs, first, got):
            assert (a.status, a.data, a.verdict.by, a.verdict.why, a.verdict.nblk) == (b.status, b.data, b.verdict.by, b.verdict.why, b.verdict.nblk), (rep, c.name)


# ------------------------------------------------------------------------------------------------------ the streams of the other suites
# What each large stream of the other crafted suites and a few natural ones must be delivered by.  The rule of a group holds for all of
# its valid streams; a stream a chain gives up is listed by its label with the W_* bits (or A_OVER) that name the limit in the code.
GROUP_RULE = {"crafted trees": "any", "geometry large fixed": "fixed", "geometry large dynamic": "any", "geometry long fixed": "fixed",
              "geometry long dynamic": "any", "natural text": "any", "natural own": "fixed", "natural Z_FIXED": "fixed"}
GIVEN_UP = {}


def _text(n, seed):
    from test_gpu_single_stream import _text as text
    return text(n, seed)


def existing_streams(engine=None):
    """-> [(group, label, z, plain or None, capacity, own dynamic blocks or None)]"""
    out = []
    lcap = _cap(max(len(p) for _, _, p in C.large() if p is not None) + 4096)
    for label, z, plain in C.large():
        # (deflate_craft.large: random_stream(.., 40, ..) has 40 crafted blocks, the all-symbols stream one)
        out.append(("crafted trees", label, z, plain, lcap, (40 if label.startswith("random_") else 1) if plain is not None else None))
    fixed, dyn = C.geometry_large()
    out.append(("geometry large fixed", fixed.name, fixed.z, fixed.plain, (1 << 20) + 4096, 0))
    out.append(("geometry large dynamic", dyn.name, dyn.z, dyn.plain, (1 << 20) + 4096, len(dyn.blocks)))
    for c in C.geometry()["long"]:
        out.append(("geometry long " + c.kind, c.name, c.z, c.plain, 65536, len(c.blocks) if c.kind == "dynamic" else 0))
    for level in (1, 6, 9):
        d = _text(300000, 500 + level)
        out.append(("natural text", "text level %d" % level, zlib.compress(d, level), d, _cap(len(d)), None))
    d = _text(400000, 510)
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_FIXED)
    z = co.compress(d) + co.flush()
    assert (z[2] & 7) == 2                             # BFINAL = 0, BTYPE = 01: more than one fixed block
    out.append(("natural Z_FIXED", "Z_FIXED, several blocks", z, d, _cap(len(d)), 0))
    if engine is not None:
        from hdl_deflate_amd.data import make_blocks
        blocks = make_blocks(256, 2048, "cuda", seed=9).reshape(-1)
        o, ol, st = engine.compress_stream(blocks, blocks.numel() - 16)
        assert int(st.item()) == 0
        d = blocks[:blocks.numel() - 16].cpu().numpy().tobytes()
        out.append(("natural own", "compress_stream's own output", o[:int(ol.item())].cpu().numpy().tobytes(), d, _cap(len(d)), 0))
    return out


def _judge_existing(engine, oracle, groups):
    K = V.source_constants()
    wrong = []
    for group, label, z, plain, cap, ndyn in existing_streams(engine):
        if group not in groups or (plain is None) != ("damaged" in groups):
            continue
        r = V.run(engine, z, cap)
        v = r.verdict
        ref = _ref(oracle, z, cap)
        if (r.status, r.data) != ref or (plain is not None and ref != (0, plain)):
            wrong.append((label, "status %d, %d bytes; the oracle: status %d, %d bytes" % (r.status, len(r.data), ref[0], len(ref[1]))))
            continue
        if plain is None:
            if ref[0] != 0 and v.by != "serial":
                wrong.append((label, "a stream the oracle rejects", v))
            continue
        if ndyn and not (v.nblk is not None and v.nblk >= ndyn):        # every true header is a candidate, whatever the verdict
            wrong.append((label, "%d dynamic blocks" % ndyn, v))
        if label in GIVEN_UP:
            if v.by != "serial" or not all(_shows(v, e, K) for e in GIVEN_UP[label]):
                wrong.append((label, "pinned: serial with " + "+".join(GIVEN_UP[label]), v))
        elif v.by != GROUP_RULE[group] or (v.why or 0) != 0 or (v.over or 0) != 0:
            wrong.append((label, "pinned: " + GROUP_RULE[group], v))
    assert not wrong, (len(wrong), wrong[:10])


def test_crafted_tree_streams(engine, oracle):
    """the six streams of 40 crafted blocks and the all-symbols stream of test_gpu_crafted_trees.py: the chain for any block types decodes
    them, and lists every one of their headers"""
    _judge_existing(engine, oracle, ("crafted trees",))


def test_crafted_tree_streams_damaged(engine, oracle):
    """... their header flips and spoiled headers: a stream the oracle rejects is the serial decoder's, one a flip left valid is anybody's"""
    _judge_existing(engine, oracle, ("crafted trees", "damaged"))


def test_match_geometry_large(engine, oracle):
    """the two 1 MiB mixed-geometry streams of test_gpu_match_geometry.py: the fixed one by the fixed-block chain, the dynamic one by the other"""
    _judge_existing(engine, oracle, ("geometry large fixed", "geometry large dynamic"))


@pytest.mark.parametrize("kind", C.GEO_KINDS)
def test_match_geometry_long_preamble(engine, oracle, kind):
    """the 116 long-preamble streams of each kind: fixed -> the fixed-block chain, dynamic -> the chain for any block types"""
    _judge_existing(engine, oracle, ("geometry long " + kind,))


def test_natural_streams(engine, oracle):
    """what the timing bars of test_gpu_single_stream.py stand for: text at levels 1, 6 and 9 is the chain's for any block types; the
    library's own stream and a Z_FIXED stream of several blocks are the fixed-block chain's"""
    _judge_existing(engine, oracle, ("natural text", "natural own", "natural Z_FIXED"))


# ------------------------------------------------------------------------------------------------------ the table of profiles/
def verdict_table(engine):
    """every stream of this module alone -> the lines of profiles/chain_verdicts.txt"""
    rows = [("chain case", c.name, c.z, _case_cap(c)) for c in C.chain_cases()] + [(g, l, z, cap) for g, l, z, p, cap, n in existing_streams(engine)]
    lines = ["%-24s %-84s %9s  %-6s %6s %5s %5s %4s %4s  %s" % ("group", "label", "z bytes", "by", "ncand", "nblk", "nx", "ns", "nreq", "why")]
    for group, label, z, cap in rows:
        v = V.run(engine, z, cap).verdict
        f = lambda x: "-" if x is None else "%d" % x
        why = "+".join(sorted(v.why_names)) + ("+A_OVER" if v.over else "")
        lines.append("%-24s %-84s %9d  %-6s %6s %5s %5s %4s %4s  %s" % (group, label, len(z), v.by, f(v.ncand), f(v.nblk), f(v.nx), f(v.ns), f(v.nreq), why.strip("+") or "-"))
    return lines
