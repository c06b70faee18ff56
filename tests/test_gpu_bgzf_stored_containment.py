"""GPU (-m gpu): hdlz_bgzf_join_stored_ws (include/hdlz_bgzf_stored.h) inside the guard bands of tests/guards.py, as
tests/test_gpu_bgzf_containment.py runs the older join: every buffer carved out of one patterned arena, on the pattern and on its
complement -- no byte outside the stated "writes" changes, the scratch stays inside work_bytes, and the results depend neither on the
initial contents of the outputs and the scratch nor on bytes outside the stated "reads": the rows of the blocks that are stored and
the input bytes of the blocks that take the fixed form are left as the pattern, which differs between the two runs."""
import zlib

import numpy as np
import pytest
import torch

import bgzf_ref
import bgzf_stored_ref as ref
import guards
from bgzf_ref import OK, E_OUT_CAPACITY
from bgzf_stored_ref import FIXED, STORED, NONE_BAD
from hdl_deflate_amd import _lib
from hdl_deflate_amd.constants import out_bound

pytestmark = pytest.mark.gpu

BAND = 1 << 16
SALTS = (0x3C, 0x3C ^ 0xFF)


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def u8(a, dtype):
    return np.array(a, dtype).view(np.uint8)


@pytest.mark.parametrize("B, short, pitched", [(257, 0, False), (257, 1, False), (3, 0, False), (3, 29, False), (40, 0, True)])
def test_join_stored_inside_guard_bands(engine, oracle, B, short, pitched):
    L = engine.lib
    r = np.random.default_rng(B)
    pool = bgzf_ref.data(4096, B)
    if pitched:                                                         # rows of 77 bytes at a pitch of 80, the input 5 bytes off a 16-byte boundary
        blocks = [pool[a:a + 77] if k % 2 else bytes(r.integers(144, 256, 77, dtype=np.uint8)) for k, a in enumerate(r.integers(0, 1900, B))]
        in_pitch, bound = 80, 77
        starts = [b * in_pitch for b in range(B)]
    else:                                                               # text from the pool's first half, bytes that do not compress, short blocks
        blocks = [pool[a:a + n] if k % 3 else bytes(r.integers(144, 256, n, dtype=np.uint8))
                  for k, (a, n) in enumerate(zip(r.integers(0, 1800, B), r.integers(0, 201, B)))]
        in_pitch, bound = 0, 200
        starts = [int(x) for x in np.concatenate([[0], np.cumsum([len(b) for b in blocks])])]
    rows, statuses = ref.oracle_rows(oracle, blocks)
    want, offs, kinds = ref.file(rows, blocks, statuses)
    assert {FIXED, STORED} == set(kinds)
    pitch = (out_bound(200) + 3) & ~3
    cap = len(want) - short
    n_in = starts[B - 1] + len(blocks[B - 1]) if pitched else starts[B]
    wb = L.hdlz_bgzf_join_stored_work_bytes(B)
    specs = [("in", n_in, 16, BAND, True, 5), ("rows", B * pitch, 4, BAND, True), ("len", 4 * B, 4, BAND, True), ("status", 4 * B, 4, BAND, True),
             ("in_off", 8 * (B + 1), 8, BAND, True), ("crc", 4 * B, 4, BAND, True), ("file", cap, 16, BAND, False, 5), ("off", 8 * (B + 1), 8, BAND),
             ("kind", B, 1, BAND), ("result", 24, 8, BAND), ("work", wb, 8, BAND)]
    # (the rows' slack, the rows of stored blocks, the input of fixed blocks and the input's pitch gaps keep the pattern: not the call's to read)
    fills = {"len": u8([len(z) for z in rows], np.uint32), "status": u8(statuses, np.uint32), "in_off": u8(starts + [n_in] * pitched, np.int64),
             "crc": u8([zlib.crc32(b) for b in blocks], np.uint32)}
    clean, runs = None, []
    for salt in SALTS:
        a = guards.Arena(guards.Arena.size_for(specs), "cuda", salt)
        for s in specs:
            a.carve(*s)
        for name, data in fills.items():
            a.fill(name, data)
        for b, (z, blk, k) in enumerate(zip(rows, blocks, kinds)):
            if k == FIXED:
                a.fill("rows", z, at=b * pitch)
            else:
                a.fill("in", blk, at=starts[b])
        rc = L.hdlz_bgzf_join_stored_ws(a.ptr("in"), None if pitched else a.ptr("in_off"), in_pitch, bound, a.ptr("rows"), pitch, a.ptr("len"),
                                        a.ptr("status"), B, a.ptr("crc"), a.ptr("file"), cap, a.ptr("off"), a.ptr("kind"), a.ptr("result"),
                                        a.ptr("work"), wb, stream_ptr())
        assert rc == 0, L.hdlz_last_error()
        torch.cuda.synchronize()
        u = a.untouched_flat()
        clean = u if clean is None else clean & u
        runs.append({n: a.view(n).cpu().numpy().copy() for n in ("file", "off", "kind", "result")})
    written = np.zeros(cap, bool)                                      # the members that fit; the EOF member if all fits
    for b in range(B):
        if offs[b + 1] <= cap:
            written[offs[b]:offs[b + 1]] = True
    if not short:
        written[:] = True
    for run in runs:
        rec = _lib.BgzfStoredResult.from_buffer_copy(run["result"].tobytes())
        assert (rec.file_len, rec.nstored, rec.status, rec.first_bad) == (len(want), sum(kinds), E_OUT_CAPACITY if short else OK, NONE_BAD)
        assert list(run["off"].view(np.int64)) == offs and list(run["kind"]) == kinds
        assert np.array_equal(run["file"][written], np.frombuffer(want, np.uint8)[:cap][written])
    bad = guards.violations(a, clean, {"file": torch.from_numpy(written), "off": True, "kind": True, "result": True, "work": True})
    assert bad == [], bad
    parts = a.split(clean)
    assert not bool(parts["off"][1].any()) and not bool(parts["result"][1].any()) and not bool(parts["kind"][1].any())
