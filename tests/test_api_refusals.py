"""CPU: tests/golden/api_refusals.json and api_refusals_containers.json replayed against the built library -- the return code and the
text of hdlz_last_error() of every entry point that takes device pointers, for every single bad argument and every pair of bad
arguments on two different parameters (the pairs pin the order of the checks).  Each fixture was recorded once by
tools/record_refusals.py from the library of the commit it names and is not regenerated when hdlz_api.hip is rewritten: what the
C-ABI refuses, in which order and in which words, stays.  The second fixture also holds `sizes`: what every *_work_bytes query of the
container headers answered over a table of shapes, so a scratch layout that is re-expressed keeps its size to the byte."""
import importlib.util
import os

import pytest

from conftest import REPO, load_golden


def _recorder():
    spec = importlib.util.spec_from_file_location("record_refusals", os.path.join(REPO, "tools", "record_refusals.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _device_visible():
    import torch
    return torch.cuda.is_available()


FIXTURES = ("api_refusals.json", "api_refusals_containers.json")
CONTAINERS_COMMIT = "b2603f71f8ca638cad8a30b9180823976b10cf96"      # the last commit in front of the rewrite of the container readers


def test_the_fixture_names_its_source_and_covers_every_pointer_call():
    from hdl_deflate_amd import _lib
    rec = _recorder()
    core, containers = (load_golden(f) for f in FIXTURES)
    for f, g in zip(FIXTURES, (core, containers)):
        assert len(g["commit"]) == 40 and int(g["commit"], 16) >= 0 and g["version"] == 0x000600, f
        assert os.path.getsize(os.path.join(REPO, "tests", "golden", f)) < 256 << 10, f
    assert containers["commit"] == CONTAINERS_COMMIT
    core_tables = (_lib.SIGNATURES, _lib.JOIN_SIGNATURES, _lib.UNJOIN_SIGNATURES, _lib.GZIP_SIGNATURES, _lib.BGZF_SIGNATURES,
                   _lib.BGZF_RANGE_SIGNATURES, _lib.BGZF_STORED_SIGNATURES)
    container_tables = (_lib.GUNZIP_SIGNATURES, _lib.ZIP_SIGNATURES, _lib.ZIP_WRITE_SIGNATURES, _lib.ZIP64_SIGNATURES, _lib.GZIP_MEMBERS_SIGNATURES)
    assert sorted(map(id, core_tables + container_tables)) == sorted(id(getattr(_lib, n)) for n in dir(_lib) if n.endswith("SIGNATURES"))   # all twelve
    pointer_calls = lambda tables: {name for t in tables for name, (_, argtypes) in t.items() if _lib.vp in argtypes}
    assert set(core["entries"]) == pointer_calls(core_tables) == set(rec.ENTRIES) and len(core["entries"]) == 23
    assert set(containers["entries"]) == pointer_calls(container_tables) == set(rec.CONTAINER_ENTRIES) and len(containers["entries"]) == 9
    assert len(pointer_calls(core_tables + container_tables)) == 32
    argtypes = {name: sig[1] for t in core_tables + container_tables for name, sig in t.items()}
    for g in (core, containers):
        for name, e in g["entries"].items():
            assert len(e["params"]) == len(argtypes[name]), name
            assert [i for i, p in enumerate(e["params"]) if p[1] == "p"] == [i for i, t in enumerate(argtypes[name]) if t is _lib.vp], name
            assert len(e["results"]) == len(rec.cases_of(e)) > len(e["faults"]) > 0, name
            assert max(e["results"]) < len(g["answers"])
            single = {(f[0], repr(f[1])) for f in e["faults"]}
            assert all((i, repr(v)) in single for i, p in enumerate(e["params"]) if p[1] == "p" and p[0] != "stream"
                       for v in [None if p[2] else {"slot": 0}] + [{"slot": s} for s in rec.SHIFTS]), name      # (thinning never drops a single fault)
        assert g["cases"] == sum(len(e["results"]) for e in g["entries"].values())


@pytest.mark.skipif(_device_visible(), reason="a case the library wrongly let through would launch kernels on host memory")
def test_every_recorded_refusal_is_given_again():
    from hdl_deflate_amd import _lib
    for fixture in FIXTURES:
        g = load_golden(fixture)
        bad = _recorder().replay(g, _lib.LIB_PATH)
        assert not bad, "%s: %d of %d cases differ; the first: %r" % (fixture, len(bad), g["cases"], bad[:3])


def test_every_scratch_size_query_answers_as_recorded():
    """the `sizes` table, value for value: every *_work_bytes query of the container headers over the product of its parameters' shapes
    (counts at 0, 1, the 64-member seams and both sides of 2^31; out_cap at both sides of a 32 KiB tile and of 2^32 - 512; every flag)"""
    from hdl_deflate_amd import _lib
    rec = _recorder()
    table = load_golden(FIXTURES[1])["sizes"]
    assert set(table["queries"]) == set(rec.SIZE_QUERIES) and table["shapes"] == rec.SHAPES
    size_queries = {name for t in (_lib.UNJOIN_SIGNATURES, _lib.GZIP_SIGNATURES, _lib.BGZF_SIGNATURES, _lib.BGZF_RANGE_SIGNATURES, _lib.GUNZIP_SIGNATURES,
                                   _lib.GZIP_MEMBERS_SIGNATURES, _lib.ZIP_SIGNATURES, _lib.ZIP64_SIGNATURES, _lib.ZIP_WRITE_SIGNATURES)
                    for name in t if name.endswith("_work_bytes")}
    assert set(table["queries"]) == size_queries and len(size_queries) == 17
    got = rec.sizes_of(rec.Driver(_lib.LIB_PATH).L, table)
    for q, e in table["queries"].items():
        assert len(e["values"]) == len(got[q]) > 0, q
        bad = [k for k, (g, w) in enumerate(zip(got[q], e["values"])) if g != w]
        assert not bad, "%s: %d of %d values differ; the first at %d: %d, recorded %d" % (q, len(bad), len(got[q]), bad[0], got[q][bad[0]], e["values"][bad[0]])
    assert any(v > 1 << 32 for e in table["queries"].values() for v in e["values"])      # (the table reaches sizes past 32 bits)
