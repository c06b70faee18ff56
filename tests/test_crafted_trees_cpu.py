"""CPU: the crafted dynamic-tree headers of tests/deflate_craft.py against stock zlib and the C oracle.

The oracle is the checker of every GPU decoder, so what it accepts has to be what zlib accepts -- for every header, with no case set
aside: the two that used to differ (a single distance code whose length is not 1; an end-of-block code alone with a length other than
1) are in the catalogue.  The generator is checked here as well, before any GPU test relies on it: its expectations come from its own
token lists, and the coverage assertions keep it from rotting into easy cases."""
import time
import zlib

import deflate_craft as C


def zlib_verdict(z):
    """-> (accepted, bytes): accepted = stock zlib reaches the end of the stream, checksum included"""
    d = zlib.decompressobj()
    try:
        out = d.decompress(z)
    except zlib.error:
        return False, None
    return d.eof, out


def test_generation_stays_quick():
    """a second or two on one core; the bound only catches a writer gone quadratic"""
    t0 = time.time()
    C.catalogue()
    [C.random_stream(1000 + s, 1 + s % 4, 40) for s in range(300)]
    C.random_stream(1, 40, 1500)
    assert time.time() - t0 < 30


def test_helpers():
    import random
    r = random.Random(1)
    for n, ml in ((2, 15), (3, 15), (16, 15), (17, 15), (30, 15), (30, 5), (19, 7), (143, 7), (144, 15), (286, 15), (286, 9), (200, 12)):
        lens = C.complete_code(n, r, ml)
        assert len(lens) == n and C.kraft(lens) == 1 << 15
        assert max(lens) == (ml if ml < n <= 1 << ml else max(lens))
    assert C.complete_code(286, r, 15).count(15) >= 2 and max(C.complete_code(143, r, 7)) == 8
    for lengths in ([0] * 300, [5] * 7 + [0] * 2 + [3] + [0] * 10 + [0] * 139 + [7] * 4, [1, 2, 3, 3] * 9):
        got = []
        for op in C.rle_ops(lengths):
            got += [(got[-1] if C.op_sym(op) == 16 else 0 if isinstance(op, tuple) else op)] * C.op_rep(op)
        assert got == lengths
    assert C.DBASE[:6] == (1, 2, 3, 4, 5, 7) and C.DBASE[29] == 24577 and [C.length_symbol(v) for v in (3, 10, 11, 12, 257, 258)] == [257, 264, 265, 265, 284, 285]
    assert C.wrap(b"", b"abc")[-4:] == zlib.adler32(b"abc").to_bytes(4, "big")


def test_every_case_zlib_and_oracle_agree(oracle):
    S = C.suite()
    cases = S["catalogue"] + S["random"]
    assert len(S["random"]) == 300
    for c in cases:
        ok, out = zlib_verdict(c.z)
        rc, ref = oracle.inflate(c.z)
        assert ok == (rc == 0), (c.name, "zlib accepts" if ok else "zlib rejects", "oracle status", rc)
        assert rc == c.status, (c.name, rc, c.status)
        if ok:
            assert out == c.plain and ref == c.plain, c.name


def test_the_two_single_code_rules(oracle):
    """an incomplete set is one code OF LENGTH 1 (or, for distances, none): zlib's inflate_table takes an incomplete set only with
    max == 1, puff only with count[0] + count[1] == n.  Counting the codes alone accepted these."""
    by_name = dict((c.name, c) for c in C.suite()["catalogue"])
    for name in ("single_distance_code_of_length_5", "single_distance_code_of_length_2_at_0", "end_of_block_only_length_3",
                 "end_of_block_only_length_15"):
        c = by_name[name]
        assert not zlib_verdict(c.z)[0], name
        assert oracle.inflate(c.z)[0] == C.E_BAD_TREE, name
    for name in ("eob_only", "one_distance_code_at_0", "one_distance_code_at_3", "one_distance_code_at_29"):
        c = by_name[name]
        assert zlib_verdict(c.z) == (True, c.plain) and oracle.inflate(c.z) == (0, c.plain), name
    from conftest import empty_distance_stream
    z = empty_distance_stream()
    assert zlib_verdict(z) == (True, b"aaaaa") and oracle.inflate(z) == (0, b"aaaaa")


def test_catalogue_holds_what_it_names():
    cat = C.suite()["catalogue"]
    by_name = dict((c.name, c) for c in cat)
    want = ["all_symbols_rle", "all_symbols_plain", "eob_only", "one_distance_code_at_0", "one_distance_code_at_3", "one_distance_code_at_29",
            "repeat16_crosses", "repeat18_crosses", "code_length_code_7_bits", "hclen_smallest", "flat_8_9", "coded_143", "coded_144",
            "coded_145", "coded_286"] + ["alternating_offset%d" % k for k in range(8)]
    assert [c.name for c in cat if c.status == 0] == want
    rejected = dict((c.name, c.status) for c in cat if c.status != 0)
    assert sorted(n for n, s in rejected.items() if s != C.E_BAD_TREE) == ["distance_before_the_start", "unused_code_of_one_distance_code",
                                                                           "unused_code_of_one_literal_code"]
    assert rejected["distance_before_the_start"] == C.E_BAD_DISTANCE and rejected["unused_code_of_one_literal_code"] == C.E_BAD_SYMBOL
    for n in ("first_op_is_16", "repeat_overruns", "no_end_of_block", "literals_oversubscribed", "literals_incomplete_two_codes",
              "literals_incomplete_2_2_2_15", "distances_oversubscribed", "distances_incomplete_two_codes", "distances_30_of_5_bits",
              "single_distance_code_of_length_5", "end_of_block_only_length_3", "code_length_code_incomplete",
              "code_length_code_oversubscribed", "hlit_287", "hlit_288", "hdist_31", "hdist_32"):
        assert rejected[n] == C.E_BAD_TREE
    b = by_name["all_symbols_rle"].blocks[0]
    assert (b["ncoded"], b["ndcoded"], b["max_ll"], b["max_dl"]) == (286, 30, 15, 15) and len(by_name["all_symbols_rle"].plain) > 32768
    assert by_name["flat_8_9"].blocks[0]["max_ll"] == 9 and by_name["hclen_smallest"].blocks[0]["hclen"] == 5
    assert by_name["code_length_code_7_bits"].blocks[0]["hclen"] == 19
    for k in range(8):
        bl = by_name["alternating_offset%d" % k].blocks
        assert len(bl) == 6 and bl[0]["offset"] == k and [x["ncoded"] for x in bl] == [286, 2] * 3


def test_coverage_of_what_was_generated():
    S = C.suite()
    blocks = [b for c in S["catalogue"] + S["random"] if c.status == 0 for b in c.blocks]
    rblocks = [b for c in S["random"] for b in c.blocks]
    for bl in (blocks, rblocks):                       # the random streams alone reach every corner too
        assert any(b["max_ll"] == 15 for b in bl) and any(b["max_dl"] == 15 for b in bl) and any(b["max_cl"] == 7 for b in bl)
        for n in (2, 143, 144, 145, 286):
            assert any(b["ncoded"] == n for b in bl), n
        assert any(b["ndcoded"] == 1 for b in bl) and any(b["ndcoded"] == 0 for b in bl) and any(b["ndcoded"] == 30 for b in bl)
        assert any(b["cross"] for b in bl)
        assert set(b["offset"] for b in bl) == set(range(8))
        assert any(b["rle"] for b in bl) and any(not b["rle"] for b in bl)
    assert max(len(c.plain) for c in S["catalogue"] + S["random"] if c.status == 0) <= 65536 - 16


def test_truncations_and_header_flips(oracle):
    """cut streams: zlib gives no verdict (it waits for more input), the oracle must not call a stream cut inside its blocks good;
    flips: every one lands inside a header and changes the stream"""
    S = C.suite()
    by_name = dict((c.name, c) for c in S["catalogue"])
    k = 0
    for n in C.TRUNCATED:
        c = by_name[n]
        for cut in range(5, len(c.z)):
            z = S["cuts"][k]
            k += 1
            assert z == c.z[:cut] and not zlib_verdict(z)[0]
            rc, ref = oracle.inflate(z)
            assert (rc, ref) == (0, c.plain) or (rc != 0 and ref == b""), (n, cut)
            assert rc != 0 or cut > len(c.z) - 4, (n, cut)                    # only a cut inside the trailer may pass
    assert k == len(S["cuts"])
    rnd = S["random"][3::7][:40]
    assert len(rnd) == 40
    for i, m in enumerate(S["flips"]):
        c = rnd[i // 3]
        diff = [j for j in range(len(m)) if m[j] != c.z[j]]
        assert len(m) == len(c.z) and len(diff) == 1
        bit = 8 * diff[0] + (m[diff[0]] ^ c.z[diff[0]]).bit_length() - 1
        assert any(a <= bit < b for a, b in c.spans)
    verdicts = [(zlib_verdict(m)[0], oracle.inflate(m, out_cap=65536)[0] == 0) for m in S["flips"]]
    assert sum(1 for v in verdicts if not v[1]) >= 60                         # most header flips are fatal; the rest change the output


def test_large_streams(oracle):
    """the streams of the whole-GPU test: the valid ones are zlib's and the oracle's, the spoiled ones are rejected by both with
    everything in front of the spoiled header decoded"""
    L = C.large()
    assert len(L) == 7 + 3 + 56
    for label, z, plain in L[:7]:
        assert 40000 < len(z) < 100000 and zlib_verdict(z) == (True, plain) and oracle.inflate(z, out_cap=1 << 20) == (0, plain), label
    for k, (label, z, plain) in enumerate(L[7:10]):
        assert plain is None and C.SPOILS[k] in label and not zlib_verdict(z)[0], label
        assert oracle.inflate(z, out_cap=1 << 20) == (C.E_BAD_TREE, b""), label
        good = L[k][1]
        n = next(i for i in range(len(z)) if z[i] != good[i])
        assert 0.3 * len(good) < n < 0.7 * len(good), label                        # (the streams part at the spoiled header)
