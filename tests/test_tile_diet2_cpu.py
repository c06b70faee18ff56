"""The premises of tests/test_gpu_tile_diet2.py, held against the oracle's tokens on the CPU: every crafted input of
tests/tile_diet2_craft.py shows what it was built for -- "this block is all literals", "this position takes distance d" -- at the position
it was built for.  No case is left out: an input that does not show its token is a bug of the crafting."""
import numpy as np
import pytest

import compress_craft as craft
import tile_diet2_craft as diet2
import tile_diet_craft as diet


def _tokens(oracle, c):
    pos, ln, ds = craft.token_arrays(oracle, c.data, c.cw, c.mm)
    assert int(pos[-1] + max(int(ln[-1]), 1)) == len(c.data), c.label         # the tokens cover the block
    return pos, ln, ds


@pytest.mark.parametrize("family", diet2.FAMILIES, ids=lambda f: f.__name__)
def test_every_case_shows_its_tokens(oracle, family):
    cases = family()
    assert cases
    wrong = []
    for c in cases:
        assert c.expect and c.route == "tile" and 5 <= len(c.data) <= diet.TILE, c.label
        bad = diet.check(c, *_tokens(oracle, c))
        if bad:
            wrong.append((c.label, bad[:3]))
    assert not wrong, "%d of %d cases miss their tokens; first: %r" % (len(wrong), len(cases), wrong[:3])


def test_the_cases_reach_the_edges_they_were_built_for(oracle):
    # A: all three alphabets at every length; the mixed ones hold 143, 144, 0 and 255 in every byte lane where the length allows
    free = diet2.literal_tiles()
    assert {(c.label.split()[1], len(c.data)) for c in free} == {(k, n) for k in ("low", "high", "mixed") for n in diet2.LIT_SIZES}
    for c in free:
        kind = c.label.split()[1]
        assert kind != "low" or max(c.data) < 144
        assert kind != "high" or min(c.data) >= 144
        if kind == "mixed" and len(c.data) >= 2046:
            assert {(q % 4, v) for q, v in enumerate(c.data) if v in diet2.EDGE_BYTES} >= {(m, v) for m in range(4) for v in diet2.EDGE_BYTES}
    # a short block CAN be all literals (the oracle has no padding: nothing behind the end matches) -- every short length is
    assert all(c.expect == (("all_lit",),) for c in free if len(c.data) < 2046)
    near = diet2.literal_tile_neighbours()
    hist = [c for c in near if c.label.startswith("false history")]
    assert len(hist) == 3 and all(c.data[:min(3, d)] == c.data[2048 - d:2048 - d + 3][:min(3, d)] for c, d in zip(hist, (3, 17, 32)))
    last = [c for c in near if c.label.startswith("last eligible")]
    for c in last:                                                   # exactly ONE match in the block, at n - 5
        pos, ln, ds = _tokens(oracle, c)
        assert int((ln > 0).sum()) == 1 and int(pos[ln > 0][0]) == len(c.data) - 5
    # B: every distance at every site, both windows; the window of 20 refuses 21 .. 32
    groups = diet2.distance_groups()
    for cw in (32, 20):
        toks = {(e[3], e[1]) for c in groups if c.label.startswith("planted") and c.cw == cw for e in c.expect if e[0] == "tok"}
        sites = lambda d: {d, 32 * 5 + 10, 32 * 9 + 30, 32 * 13 + 31, 32 * 63 + 5}
        assert toks == {(d, p) for d in range(1, min(cw, 32) + 1) for p in sites(d)}
        none = {c.label for c in groups if c.label.startswith("planted") and c.cw == cw and all(e[0] == "nomatch" for e in c.expect)}
        assert len(none) == 32 - min(cw, 32)
    assert len([c for c in groups if c.label.startswith("lane 0 i=d-1")]) == 30
    pairs = {tuple(int(x) for x in c.label.split()[1].split("/")) for c in groups if c.label.startswith("pair")}
    assert pairs == set(diet2.PAIRS_APART) | set(diet2.PAIRS_NEXT)
    for c in groups:
        if c.label.startswith("pair"):                               # both candidates are there: the trigram at p, at p - near and at p - far
            near_d, far_d = (int(x) for x in c.label.split()[1].split("/"))
            p = c.expect[1][1]
            t = c.data[p:p + 3]
            assert c.data[p - near_d:p - near_d + 3] == t and c.data[p - far_d:p - far_d + 3] == t and c.expect[1] == ("tok", p, 3, near_d)
    assert {(n >> 2 == f >> 2) for n, f in pairs} == {True, False}    # pairs inside one aligned group of four, and across two
    # C: every length at every distance behind every edge literal in every byte lane
    for mm in (10, 5):
        for d in diet2.LENGTH_DISTS:
            c = next(c for c in diet2.lengths_and_literals() if c.label == "lengths d=%d mm=%d" % (d, mm))
            got = {(e[2], c.data[e[1] - 1], (e[1] - 1) % 4) for e in c.expect if e[0] == "tok"}
            assert {(g[0], g[1]) for g in got} == {(min(L, mm), v) for L in range(3, 11) for v in diet2.EDGE_BYTES}
            assert {(g[1], g[2]) for g in got} == {(v, m) for v in diet2.EDGE_BYTES for m in range(4)}
    # D
    assert [len(c.data) for c in diet2.adler_extremes()] == [2048, 2047, 5, 5, 2048]
    assert len(diet2.all_cases()) <= 300


def test_the_alternating_batch_alternates(oracle):
    """the batch of the GPU test at a small grid: kinds alternate along every wave's sequence, the match-free blocks are all literals,
    the others are not, and the long ones are there"""
    G = 1024
    blocks, kinds, long_ones = diet2.alternating(G)
    assert len(blocks) == 2 * G + 7 and long_ones
    for w in (0, 1, 3, 512, G - 1):
        seq = [kinds[k * G + (w + k) % G] for k in range(2)]
        assert seq[0] != seq[1]
    assert {len(blocks[b]) for b in long_ones} == {2046, 2047, 2048}
    assert {kinds[b] for b in long_ones} == {True, False}
    for b in list(range(0, len(blocks), 37)) + long_ones:
        pos, ln, ds = craft.token_arrays(oracle, blocks[b], 32, 10)
        assert bool((ln > 0).any()) != kinds[b], b
        assert not kinds[b] or (min(blocks[b]) >= 128 and max(blocks[b]) >= 144 and min(blocks[b]) < 144)
