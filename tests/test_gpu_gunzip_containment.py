"""GPU (-m gpu): hdlz_gunzip_ws inside guard bands (tests/guards.py), in the manner of tests/test_gpu_checked_containment.py: every
buffer of the call carved out of one patterned arena, each case run on the pattern and on its complement.

  bands and read-only regions (d_in and what stands behind the streams, d_in_off) untouched;
  the five result arrays written for [0, nstreams) only, d_work only inside what was passed, rows inside the row -- an OK row exactly
  d_out_len[b] bytes;
  all results identical in both runs -- the runs differ in every byte behind a stream's end, every byte behind out_len and the initial
  content of every output and of the scratch, so none of those reaches a verdict -- and equal to the rule (gunzip_ref).
Both decode routes (one stream: the batch call's path; several: the member view) and both CRC mappings (rows below 64 KiB: a workgroup
per row; tiles from there on)."""
import numpy as np
import pytest

import guards
import gunzip_ref as G
import test_gpu_containment as C

pytestmark = pytest.mark.gpu


def gunzip_call(engine, oracle, label, streams, pitch, fixed=None, crc=True, mis=0, bound=None):
    """one guarded hdlz_gunzip_ws: ragged (bound = the stated in_len) or fixed = (in_len, in_pitch)"""
    L, B, band = engine.lib, len(streams), C.row_band(pitch)
    off = np.concatenate([[0], np.cumsum([len(z) for z in streams])]).astype(np.int64)
    ilen = fixed[0] if fixed else (max(len(z) for z in streams) if bound is None else bound)
    work_bytes = L.hdlz_gunzip_work_bytes(B, ilen, pitch, 0 if fixed else 1)
    assert work_bytes > 0
    if fixed:
        specs = [("in", (B - 1) * fixed[1] + fixed[0], 16, band, True, mis)]
    else:
        specs = [("in", int(off[-1]), 16, band, True, mis), ("in_off", 8 * (B + 1), 8, band, True)]
    results = ("out_len", "status", "in_used", "crc")
    specs += [("out", B * pitch, 4, band)] + [(n, 4 * B, 4, band) for n in results] + [("work", work_bytes, 256, C.WORK_BAND)]

    def setup(a):
        if fixed:
            for b, z in enumerate(streams):
                a.fill("in", z, at=b * fixed[1])
        else:
            a.fill("in", b"".join(streams))
            a.fill("in_off", off.view(np.uint8))

    def call(a):
        rc = L.hdlz_gunzip_ws(a.ptr("in"), None if fixed else a.ptr("in_off"), fixed[1] if fixed else 0, ilen, B, a.ptr("out"), pitch,
                              a.ptr("out_len"), a.ptr("status"), a.ptr("in_used"), a.ptr("crc") if crc else None, a.ptr("work"), work_bytes,
                              C.stream_ptr())
        assert rc == 0, (label, L.hdlz_last_error())

    a, clean, runs = C.two_runs(specs, setup, call, ("out",) + results)
    for n in results[:3] + (("crc",) if crc else ()):
        assert np.array_equal(runs[0][n], runs[1][n]), (label, n, "depends on bytes the call was not given")
    assert not fixed or all(len(z) == fixed[0] for z in streams)      # (fixed pitch here: rows without slack, so the rule sees what the call sees)
    exps = [G.expect(oracle, z, pitch) for z in streams]
    for k, r in enumerate(runs):
        st, ol, used, cw = (r[n].view(np.uint32) for n in ("status", "out_len", "in_used", "crc"))
        out = r["out"].reshape(B, pitch)
        for b in range(B):
            G.check((label, k, b), exps[b], st[b], ol[b], used[b], cw[b] if crc else exps[b]["crc"], out[b])
    st, ol = runs[1]["status"].view(np.uint32), runs[1]["out_len"].view(np.uint32)
    ext = [int(ol[b]) if st[b] == 0 else pitch for b in range(B)]       # an OK row: exactly out_len bytes; a failed one: anything inside the row
    allowed = {"out": guards.row_mask(B, pitch, ext, "cuda"), "out_len": True, "status": True, "in_used": True, "work": True}
    if crc:
        allowed["crc"] = True
    bad = guards.violations(a, clean, allowed)
    assert bad == [], (label, bad)
    parts = a.split(clean)
    for n in results[:3] + (("crc",) if crc else ()):
        assert not bool(parts[n][1].any()), (label, n, "not written")
    if not crc:
        assert bool(parts["crc"][1].all()), (label, "d_crc = NULL: nothing of that region may be written")
    return runs


def _mixed():
    pay, tr, hdr = dict(G.payload_cases()), dict(G.trailer_cases()), dict(G.header_cases())
    return [hdr["all four"], pay["level 6"], tr["cut at end + 4"], pay["stored"], hdr["wrong magic"], pay["several blocks"], tr["CRC bit 0"],
            hdr["name of 300, comment of 64"], hdr["cut at 5"], pay["empty"], tr["a second member behind"], hdr["FHCRC wrong by bit 0"],
            pay["full flush"], hdr["unterminated name"]]


def test_the_member_view_and_a_workgroup_per_row(engine, oracle):
    streams = _mixed()
    for mis in (0, 5):
        runs = gunzip_call(engine, oracle, ("rows", mis), streams, 65532, crc=mis == 0, mis=mis)
    st = list(runs[0]["status"].view(np.uint32))
    assert st == [0, 0, 5, 0, 11, 0, 12, 0, 5, 0, 0, 11, 0, 5], st


def test_the_member_view_and_the_tiles(engine, oracle):
    streams = _mixed() + G.lengths_case([32768, 32769, 65537, 131072, 131073])
    runs = gunzip_call(engine, oracle, "tiles", streams, 131072, mis=3)
    assert list(runs[0]["status"].view(np.uint32))[-5:] == [0, 0, 0, 0, 2]
    d = G.text(70000, 31)
    z = [G.gz(d, name=b"aaaa"), G.gz(d, name=b"bbbb", crc_xor=2)]           # (two rows of one length, without slack)
    runs = gunzip_call(engine, oracle, "tiles, pitched", z, 65536 + 8192, fixed=(len(z[0]), len(z[0])))
    assert list(runs[0]["status"].view(np.uint32)) == [0, 12]


def test_one_stream_takes_the_batch_calls_path_in_guarded_scratch(engine, oracle):
    """nstreams = 1: small streams (one wave), and a 3 MiB member (the whole-GPU chains, their scratch behind the call's own words) --
    intact, damaged in the trailer, and with its header refused (an empty range for the decoder)"""
    for z, pitch in ((dict(G.header_cases())["all four"], 65532), (dict(G.payload_cases())["level 9"], 131072),
                     (dict(G.trailer_cases())["ISIZE + 1"], 8192), (dict(G.header_cases())["cut at 12"], 64)):
        gunzip_call(engine, oracle, ("one small stream", len(z)), [z], pitch, fixed=(len(z), len(z)), mis=7)
        gunzip_call(engine, oracle, ("one small stream, ragged", len(z)), [z], pitch, crc=False)
    data = C.plain_bytes(3 << 20, 7)
    cap = (3 << 20) + 64
    good = G.gz(data, name=b"three.bin", hcrc=True)
    for k, z in enumerate((good, G.gz(data, name=b"three.bin", crc_xor=1 << 7), G.gz(data, flg=0x40), good[:-5])):
        runs = gunzip_call(engine, oracle, ("one large stream", k), [z], cap, fixed=(len(z), len(z)), mis=(0, 1, 2, 3)[k])
        assert int(runs[0]["status"].view(np.uint32)[0]) == (G.OK, G.E_BAD_CHECKSUM, G.E_BAD_HEADER, G.E_NO_EOF)[k]
