"""CPU: tests/golden/api_refusals.json replayed against the built library -- the return code and the text of hdlz_last_error() of every
entry point that takes device pointers, for every single bad argument and every pair of bad arguments on two different parameters
(the pairs pin the order of the checks).  The fixture was recorded once by tools/record_refusals.py from the library of the commit
it names and is not regenerated when hdlz_api.hip is rewritten: what the C-ABI refuses, in which order and in which words, stays."""
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


def test_the_fixture_names_its_source_and_covers_every_pointer_call():
    from hdl_deflate_amd import _lib
    g = load_golden("api_refusals.json")
    assert len(g["commit"]) == 40 and int(g["commit"], 16) >= 0 and g["version"] == 0x000600
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "api_refusals.json")) < 256 << 10
    tables = (_lib.SIGNATURES, _lib.JOIN_SIGNATURES, _lib.UNJOIN_SIGNATURES, _lib.GZIP_SIGNATURES, _lib.BGZF_SIGNATURES,
              _lib.BGZF_RANGE_SIGNATURES, _lib.BGZF_STORED_SIGNATURES)
    takes_pointers = {name for t in tables for name, (_, argtypes) in t.items() if _lib.vp in argtypes}
    assert set(g["entries"]) == takes_pointers == set(_recorder().ENTRIES) and len(takes_pointers) == 23
    rec = _recorder()
    argtypes = {name: sig[1] for t in tables for name, sig in t.items()}
    for name, e in g["entries"].items():
        assert len(e["params"]) == len(argtypes[name]), name
        assert [i for i, p in enumerate(e["params"]) if p[1] == "p"] == [i for i, t in enumerate(argtypes[name]) if t is _lib.vp], name
        assert len(e["results"]) == len(rec.cases_of(e)) > len(e["faults"]) > 0, name
        assert max(e["results"]) < len(g["answers"])
    assert g["cases"] == sum(len(e["results"]) for e in g["entries"].values())


@pytest.mark.skipif(_device_visible(), reason="a case the library wrongly let through would launch kernels on host memory")
def test_every_recorded_refusal_is_given_again():
    from hdl_deflate_amd import _lib
    g = load_golden("api_refusals.json")
    bad = _recorder().replay(g, _lib.LIB_PATH)
    assert not bad, "%d of %d cases differ; the first: %r" % (len(bad), g["cases"], bad[:3])
