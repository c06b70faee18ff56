"""CPU: the guard-band checker of tests/guards.py flags what tests/test_gpu_containment.py relies on it to flag.  A "kernel" here is a
few planted stores into an arena on the CPU; every case runs on the pattern and on its complement like the GPU cases do."""
import pytest
import torch

import guards

PITCH, ROWS, BAND = 64, 3, 256
SPECS = [("in", 100, 16, BAND, True, 3), ("out", ROWS * PITCH, 4, BAND), ("out_len", 4 * ROWS, 4, BAND), ("work", 512, 256, BAND)]
EXTENTS = [10, 0, 64]


def run_twice(plant):
    """-> (arena, unwritten in both runs): plant(arena) does the stores of the call under test"""
    clean = None
    for salt in (0x5A, 0x5A ^ 0xFF):
        a = guards.Arena(guards.Arena.size_for(SPECS), "cpu", salt)
        for s in SPECS:
            a.carve(*s)
        a.fill("in", torch.arange(90, dtype=torch.uint8))           # (the last 10 bytes stay pattern: the input's slack)
        plant(a)
        u = a.untouched_flat()
        clean = u if clean is None else clean & u
    return a, clean


def allowed(a):
    return {"out": guards.row_mask(ROWS, PITCH, EXTENTS, "cpu"), "out_len": True, "work": True}


def honest(a):
    out = a.view("out").view(ROWS, PITCH)
    out[0, :10] = 7
    out[2, :] = 9
    a.view("out_len").fill_(1)
    a.view("work").fill_(0xEE)


def test_pattern_depends_on_the_position_and_complements():
    p = guards.pattern(0, 1 << 17, 0x11, "cpu")
    q = guards.pattern(0, 1 << 17, 0x11 ^ 0xFF, "cpu")
    assert bool((p ^ q == 0xFF).all())
    for shift in (1, 4, 16, 256, 4096, 65536):
        assert not torch.equal(p[shift:], p[:-shift]), shift
    assert len(set(p[:256].tolist())) == 256
    assert torch.equal(guards.pattern(1000, 70000, 0x11, "cpu"), p[1000:70000])


def test_carving_alignment_bands_and_exact_sizes():
    a = guards.Arena(guards.Arena.size_for(SPECS), "cpu", 1)
    views = {s[0]: a.carve(*s) for s in SPECS}
    assert views["in"].data_ptr() % 16 == 3 and views["out"].data_ptr() % 4 == 0 and views["work"].data_ptr() % 256 == 0
    assert [views[s[0]].numel() for s in SPECS] == [s[1] for s in SPECS]
    spans = sorted((r.off - r.band, r.off + r.nbytes + r.band) for r in a.regions.values())
    assert spans[0][0] >= 0 and spans[-1][1] <= a.nbytes
    assert all(x[1] <= y[0] for x, y in zip(spans, spans[1:]))          # no band is shared


def test_confined_writes_pass():
    a, clean = run_twice(honest)
    assert guards.violations(a, clean, allowed(a)) == []
    assert guards.row_tails(a.split(clean)["out"][1], ROWS, PITCH).tolist() == [10, 0, 64]


@pytest.mark.parametrize("region,rel,where", [
    ("out", -BAND, "front band"), ("out", -1, "front band"), ("out", ROWS * PITCH, "back band"),
    ("out", ROWS * PITCH + BAND - 1, "back band"), ("out_len", 4 * ROWS, "back band"), ("work", 512, "back band"),
    ("work", -1, "front band"), ("out", 10, "region"), ("out", PITCH, "region"), ("out", 2 * PITCH - 1, "region"),
    ("in", 0, "region"), ("in", 99, "region"), ("in", 100, "back band")])
def test_one_planted_byte_is_reported(region, rel, where):
    def plant(a):
        honest(a)
        a.buf[a.regions[region].off + rel] = 0xA5
    a, clean = run_twice(plant)
    assert guards.violations(a, clean, allowed(a)) == [(region, where, rel, rel, 1)]


def test_a_store_of_the_patterns_own_value_is_caught_by_the_complement_run():
    first = {}

    def plant(a):
        honest(a)
        r = a.regions["out"]
        first.setdefault("v", int(a.pat[r.off + 10]))                   # what run 1's pattern holds there
        a.buf[r.off + 10] = first["v"]
    a, clean = run_twice(plant)
    assert guards.violations(a, clean, allowed(a)) == [("out", "region", 10, 10, 1)]
    # one run alone would have missed it
    b = guards.Arena(guards.Arena.size_for(SPECS), "cpu", 0x5A)
    for s in SPECS:
        b.carve(*s)
    b.buf[b.regions["out"].off + 10] = first["v"]
    assert bool(b.untouched_flat().all())


def test_prefix_grants_and_missing_regions():
    def plant(a):
        a.view("work")[:300] = 1
    a, clean = run_twice(plant)
    assert guards.violations(a, clean, {"work": 300}) == []
    assert guards.violations(a, clean, {"work": 256}) == [("work", "region", 256, 299, 44)]
    assert guards.violations(a, clean, {}) == [("work", "region", 0, 299, 300)]
    with pytest.raises(AssertionError):
        guards.violations(a, clean, {"in": True})                       # nothing of a read-only region can be granted


def test_a_carve_that_does_not_fit_raises():
    a = guards.Arena(4096, "cpu", 0)
    a.carve("a", 1000, 4, 512)
    with pytest.raises(ValueError):
        a.carve("b", 2000, 4, 512)
    with pytest.raises(ValueError):
        guards.Arena(100, "cpu", 0).carve("c", 10, 4, 64)
