"""The premises of tests/test_gpu_tile_diet.py, held against the oracle's tokens on the CPU: every crafted input of
tests/tile_diet_craft.py shows the token it was built for at the position it was built for -- the match whose bytes lie in the next
lane's word, the tail that lane 63 must not match into, the lanes that sum 288 bits, the widest pair of codes, the back-to-back starts,
the runs up to and beyond the cap.  No case is left out: an input that does not show its token is a bug of the crafting."""
import numpy as np
import pytest

import compress_craft as craft
import tile_diet_craft as diet

FAMILIES = [diet.lane_seams, diet.lane63, diet.bit_sums, diet.wide_codes, diet.start_flags, diet.sentinel_runs]


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: f.__name__)
def test_every_case_shows_its_tokens(oracle, family):
    cases = family()
    assert cases
    wrong = []
    for c in cases:
        assert c.expect, c.label
        pos, ln, ds = craft.token_arrays(oracle, c.data, c.cw, c.mm)
        assert int(pos[-1] + max(int(ln[-1]), 1)) == len(c.data), c.label         # the tokens cover the block
        bad = diet.check(c, pos, ln, ds)
        if bad:
            wrong.append((c.label, bad[:3]))
    assert not wrong, "%d of %d cases miss their tokens; first: %r" % (len(wrong), len(cases), wrong[:3])


def test_the_cases_reach_the_edges_they_were_built_for(oracle):
    seams = diet.lane_seams()
    three = [c for c in seams if c.label.startswith("seam")]
    toks = {(e[1] % 32, e[1] // 32, e[3]) for c in three if len(c.data) == 2048 for e in c.expect if e[0] == "tok"}
    for lane in (1, 31, 62):
        assert {(i, lane, d) for i in (29, 30, 31) for d in range(1, 33)} <= toks       # every distance at every seam position
    assert {(i, 0, d) for i in (29, 30, 31) for d in range(1, i + 1)} <= toks           # lane 0: d <= p
    assert {len(c.data) for c in three} == set(diet.SEAM_SIZES)
    # lane 63 of a full tile: local 29 .. 31 lie behind n - 5, where nothing may match -- whatever the lane reads as its next word
    assert any(e[0] == "nomatch" and e[1] // 32 == 63 for c in three if len(c.data) == 2048 for e in c.expect)
    longer = {(e[1] % 32, e[2]) for c in seams if c.label.startswith("long") for e in c.expect if e[0] == "tok"}
    assert longer >= {(i, L) for i in range(20, 32) for L in range(4, 11)}
    # 288 bits in every lane: 2048 literals, all of nine bits
    nine = diet.bit_sums()[0]
    assert len(nine.data) == 2048 and min(nine.data) >= 144
    # the widest pair: a nine-bit literal right in front of an 18-bit match, at every distance 129 .. 256, at even and odd positions
    wide = diet.wide_codes()[0]
    m = [e for e in wide.expect if e[0] == "tok"]
    assert {e[3] for e in m} == set(range(129, 257)) and {e[2] for e in m} == {10} and {e[1] & 1 for e in m} == {0, 1}
    assert all(wide.data[e[1] - 1] >= 144 for e in m)
    assert {c.route for c in diet.wide_codes()} == {"wide", "session", "small", "stream"}
    # start flags: every length back to back; the fewest starts a lane can have (length 10 throughout) is reached
    flags = diet.start_flags()
    for L in range(3, 11):
        c = next(c for c in flags if c.label == "back to back L=%d" % L)
        p = sorted(e[1] for e in c.expect)
        assert sum(1 for a, b in zip(p, p[1:]) if b - a == L) >= 20, L                   # runs of matches with nothing between them
    ends = next(c for c in flags if c.label == "lane end")
    assert {e[2] for e in ends.expect} == set(range(3, 11)) and all((e[1] + e[2]) % 32 == 0 for e in ends.expect)
    assert {len(c.data) for c in flags if c.route == "small"} == {5, 33, 100}
    # the cap: runs of every length 3 .. 13 at local 0 and 20 .. 31, for both caps and both window forms
    for cw, mm in diet.SENTINEL_CONFIGS:
        got = {((e[1] - 1) % 32, e[2]) for c in diet.sentinel_runs() if (c.cw, c.mm) == (cw, mm) for e in c.expect if e[0] == "tok"}
        assert got == {(i, min(R - 1, mm)) for i in (0,) + tuple(range(20, 32)) for R in range(4, 14)}
    assert len(diet.all_cases()) <= 1200
