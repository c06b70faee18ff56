#!/usr/bin/env python3
"""Records what every entry point of libhdlz.so that takes device pointers answers to a bad argument: the return code and
hdlz_last_error() of every single fault and of every pair of faults on two different parameters (the pairs pin the ORDER of the
checks).  CPU only: the parameter checks stand in front of check_device(), so a call that passes them all ends with HDLZ_E_HIP and
touches nothing -- with a device it would launch kernels on host memory, hence the exit below.

    python tools/record_refusals.py --lib <libhdlz.so of the commit to pin> --commit <its hash> [--set core|containers] [--out <fixture>]

Two sets, a fixture each, recorded from different commits: `core` (ENTRIES -> tests/golden/api_refusals.json) and `containers`
(CONTAINER_ENTRIES: the readers and writers that came later -> tests/golden/api_refusals_containers.json, which also holds `sizes`:
what every *_work_bytes query of the container headers answers over a table of shapes, sizes_of() below).

A fixture depends on no address: a pointer is an offset into a 256-aligned host buffer, a scratch size is "query(args) + delta".
tests/test_api_refusals.py replays it (replay() below) against the built library."""
import argparse
import ctypes
import importlib.util
import itertools
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
SLOT = 1024                               # every pointer parameter gets a slot of its own in the host buffer
SHIFTS = (1, 2, 4, 8, 128)                # the displacements of a pointer ...
PAIR_SHIFTS = SHIFTS                      # ... and those that also go into the pairs (all of them: the fixture is ~100 KiB; thin HERE first)
# (Neither set needed thinning: the containers fixture, two ZIP writers of 17 pointers each included, is ~90 KiB against the test's cap of
# 256 KiB.  The rule if one ever does: every single fault stays, and for every pair of parameters the pair (null, or the undisplaced
# slot of an optional pointer) x (one displacement) stays -- drop displacements from PAIR_SHIFTS, never a fault from faults_of().)
U32, U64 = (1 << 32) - 1, (1 << 64) - 1


# ---- the good argument tuple of every entry point.  A parameter is (name, kind, good):
#   "p"   pointer: good True = its slot, None = null (an optional pointer: its faults are the slot and the displaced slot)
#   "n"   count (uint64)     "f"  flags      "w"  work_bytes: good = (query, args) of the size query
#   "cw"  cwindow            "mm"   maxmatch           "v"  a plain value, faulted only by `special`
# and `special` lists the entry point's own limits as (parameter, value).
def P(name, good=True):
    return (name, "p", good)


def V(name, good):
    return (name, "v", good)


_COMPRESS = [P("d_in"), P("d_in_off", None), V("in_pitch", 2048), V("in_len", 2048), ("nblocks", "n", 3), ("cwindow", "cw", 32), ("maxmatch", "mm", 10),
             P("d_out"), V("out_pitch", 2320), P("d_out_len"), P("d_status")]
_INFLATE = [P("d_in"), P("d_in_off", None), V("in_pitch", 2048), V("in_len", 2048), ("nstreams", "n", 3), ("flags", "f", 0), V("obsize", 0),
            P("d_out"), V("out_pitch", 4096), P("d_out_len"), P("d_status")]
_IN_LEN = [("in_len", 1 << 28), ("in_len", (1 << 28) - 1), ("in_len", 1 << 31), ("in_len", U32)]
_PITCH = [("out_pitch", 2319), ("out_pitch", 2), ("in_pitch", 2047), ("nblocks", 0)]
_OUT_PITCH = [("out_pitch", 4095), ("out_pitch", 2), ("in_pitch", 2047), ("nstreams", 0), ("nstreams", 1)]
_JOIN_HEAD = [P("d_rows"), V("row_pitch", 2320), P("d_len"), P("d_end_bits"), P("d_status"), P("d_in_off", None), V("in_len", 2048), ("nblocks", "n", 3)]
_UNJOIN = [P("d_stream"), V("stream_len", 4096), P("d_off"), P("d_out_off", None), V("out_len", 2048), ("nmembers", "n", 3), ("flags", "f", 0),
           P("d_out"), V("out_cap", 6144), P("d_member_status", None), P("d_result"), P("d_work")]
STREAM = [P("stream", None)]              # (never faulted: nothing checks it in front of the device)

ENTRIES = {
    "hdlz_compress_batch": (_COMPRESS + STREAM, _IN_LEN + _PITCH),
    "hdlz_compress_batch_bits": (_COMPRESS + [P("d_end_bits")] + STREAM, _IN_LEN + _PITCH),
    "hdlz_compress_streams": ([P("d_in"), V("in_pitch", 65536), V("in_len", 65536), ("nblocks", "n", 2), ("cwindow", "cw", 32), ("maxmatch", "mm", 10),
                               P("d_out"), V("out_pitch", 73744), P("d_out_len"), P("d_status"), P("d_work"),
                               ("work_bytes", "w", ("hdlz_streams_work_bytes", [65536, 2]))] + STREAM,
                              _IN_LEN + [("out_pitch", 73743), ("out_pitch", 4), ("nblocks", 0), ("nblocks", 1 << 32)]),
    "hdlz_compress_stream": ([P("d_in"), V("in_len", 65536), ("cwindow", "cw", 32), ("maxmatch", "mm", 10), P("d_out"), V("out_cap", 73744),
                              P("d_out_len"), P("d_status"), P("d_work"), ("work_bytes", "w", ("hdlz_stream_work_bytes", [65536]))] + STREAM,
                             _IN_LEN + [("out_cap", 4)]),
    "hdlz_compress_chunk": ([P("d_in"), V("in_len", 4096), V("q_end", 4096), V("final", 1), ("cwindow", "cw", 32), ("maxmatch", "mm", 10), P("d_out"),
                             V("out_cap", 8192), P("d_state")] + STREAM, _IN_LEN),
    "hdlz_inflate_chunk": ([P("d_in"), V("in_len", 4096), V("final", 1), ("flags", "f", 0), V("obsize", 0), P("d_out"), V("out_cap", 8192),
                            V("out_limit", 8192), P("d_state")] + STREAM, _IN_LEN),
    "hdlz_inflate_batch": (_INFLATE + STREAM, _IN_LEN + _OUT_PITCH),
    "hdlz_inflate_batch_ws": (_INFLATE + [P("d_work"), ("work_bytes", "w", ("hdlz_inflate_work_bytes", [3, 2048, 4096, 0, 0]))] + STREAM,
                              _IN_LEN + _OUT_PITCH),
    "hdlz_inflate_checked": (_INFLATE + [P("d_in_used"), P("d_adler"), P("d_work"),
                                         ("work_bytes", "w", ("hdlz_inflate_checked_work_bytes", [3, 2048, 4096, 0, 0]))] + STREAM,
                             _IN_LEN + _OUT_PITCH),
    "hdlz_compact_batch": ([P("d_rows"), V("row_pitch", 2320), P("d_len"), P("d_off"), ("nblocks", "n", 3), P("d_archive")] + STREAM, [("nblocks", 0)]),
    "hdlz_archive_batch_ws": ([P("d_rows"), V("row_pitch", 2320), P("d_len"), ("nblocks", "n", 3), P("d_archive"), V("archive_cap", 6960), P("d_off"),
                               P("d_work"), ("work_bytes", "w", ("hdlz_archive_work_bytes", [3]))] + STREAM, [("nblocks", 0)]),
    "hdlz_archive_batch": ([P("d_rows"), V("row_pitch", 2320), P("d_len"), ("nblocks", "n", 3), P("d_archive"), V("archive_cap", 6960), P("d_off")] + STREAM, [("nblocks", 0)]),
    "hdlz_join_batch_ws": (_JOIN_HEAD + [P("d_stream"), V("stream_cap", 8192), P("d_off"), P("d_result"), P("d_work"),
                                         ("work_bytes", "w", ("hdlz_join_work_bytes", [3]))] + STREAM, [("nblocks", 0)]),
    "hdlz_join_gzip_ws": (_JOIN_HEAD + [P("d_crc"), P("d_stream"), V("stream_cap", 8192), P("d_off"), P("d_result"), P("d_work"),
                                        ("work_bytes", "w", ("hdlz_join_gzip_work_bytes", [3]))] + STREAM, [("nblocks", 0)]),
    "hdlz_unjoin_ws": (_UNJOIN + [("work_bytes", "w", ("hdlz_unjoin_work_bytes", [3, 6144, 0]))] + STREAM, [("out_cap", 0), ("nmembers", 0)]),
    "hdlz_unjoin_gzip_ws": (_UNJOIN + [("work_bytes", "w", ("hdlz_unjoin_gzip_work_bytes", [3, 6144, 0]))] + STREAM, [("out_cap", 0), ("nmembers", 0)]),
    "hdlz_crc32_ws": ([P("d_data"), ("n", "n", 100000), P("d_crc"), P("d_work"), ("work_bytes", "w", ("hdlz_crc32_work_bytes", [100000]))] + STREAM, [("n", 0)]),
    "hdlz_crc32_batch_ws": ([P("d_data"), P("d_off", None), V("pitch", 2048), V("len", 2048), ("nblocks", "n", 3), P("d_crc")] + STREAM, [("len", 0), ("nblocks", 0)]),
    "hdlz_bgzf_join_ws": ([P("d_rows"), V("row_pitch", 2320), P("d_len"), P("d_status"), P("d_in_off", None), V("in_len", 2048), ("nblocks", "n", 3),
                           P("d_crc"), P("d_file"), V("file_cap", 8192), P("d_off"), P("d_result"), P("d_work"),
                           ("work_bytes", "w", ("hdlz_bgzf_join_work_bytes", [3]))] + STREAM, [("nblocks", 0)]),
    "hdlz_bgzf_join_stored_ws": ([P("d_in"), P("d_in_off", None), V("in_pitch", 2048), V("in_len", 2048), P("d_rows"), V("row_pitch", 2320), P("d_len"),
                                  P("d_status"), ("nblocks", "n", 3), P("d_crc"), P("d_file"), V("file_cap", 8192), P("d_off"), P("d_kind", None),
                                  P("d_result"), P("d_work"), ("work_bytes", "w", ("hdlz_bgzf_join_stored_work_bytes", [3]))] + STREAM, [("nblocks", 0)]),
    "hdlz_bgzf_index_ws": ([P("d_file"), V("file_len", 100000), V("member_cap", 16), P("d_off"), P("d_out_off"), P("d_result"), P("d_work"),
                            ("work_bytes", "w", ("hdlz_bgzf_index_work_bytes", [100000]))] + STREAM,
                           [("member_cap", 1 << 40), ("member_cap", (1 << 40) - 1), ("file_len", 0)]),
    "hdlz_bgzf_inflate_ws": ([P("d_file"), V("file_len", 4096), P("d_off"), P("d_out_off"), ("nmembers", "n", 3), ("flags", "f", 0), P("d_out"),
                              V("out_cap", 6144), P("d_member_status", None), P("d_result"), P("d_work"),
                              ("work_bytes", "w", ("hdlz_bgzf_inflate_work_bytes", [3, 0]))] + STREAM, [("out_cap", 0), ("nmembers", 0)]),
    "hdlz_bgzf_read_ranges_ws": ([P("d_file"), V("file_len", 4096), P("d_off"), P("d_out_off"), ("nmembers", "n", 3), P("d_ranges"), ("nranges", "n", 2),
                                  ("flags", "f", 0), P("d_out"), V("out_cap", 6144), P("d_range_off"), P("d_range_status", None), ("task_cap", "n", 4),
                                  P("d_result"), P("d_work"), ("work_bytes", "w", ("hdlz_bgzf_ranges_work_bytes", [2, 4, 0]))] + STREAM,
                                 [("out_cap", 0), ("nranges", 0), ("task_cap", 0)]),
}

# ---- the containers set: include/hdlz_gunzip.h, hdlz_gzip_members.h, hdlz_zip.h, hdlz_zip64.h, hdlz_zip_write.h
_MEMBER_INDEX = [P("d_file"), V("file_len", 100000), V("member_cap", 16), P("d_off"), P("d_out_off"), P("d_result"), P("d_work")]
_ZIP_INDEX = [P("d_file"), V("file_len", 100000), V("entry_cap", 16), V("out_align", 64), P("d_entries"), P("d_result"), P("d_work")]
_ZIP_INDEX_LIMITS = [("out_align", 0), ("out_align", 3), ("out_align", 512), ("out_align", 256), ("file_len", 1 << 32), ("file_len", U32), ("file_len", 0),
                     ("entry_cap", 0), ("entry_cap", 65536), ("entry_cap", 1 << 31), ("entry_cap", (1 << 31) - 1), ("entry_cap", 1 << 32)]
_ZIP_INFLATE = [P("d_file"), V("file_len", 100000), P("d_entries"), V("first", 0), ("count", "n", 3), V("in_len", 4096), P("d_out"), V("out_cap", 65536),
                P("d_entry_status", None), P("d_result"), P("d_work")]
_ZIP_INFLATE_LIMITS = [("file_len", 1 << 32), ("file_len", U32), ("first", 1 << 31), ("first", (1 << 31) - 1), ("first", (1 << 31) - 3), ("first", (1 << 31) - 4),
                       ("count", 0), ("count", 1), ("out_cap", 0), ("out_cap", 2), ("out_cap", 1 << 32), ("in_len", 1 << 28), ("in_len", U32)]
_ZIP_WRITE_HEAD = [P("d_in"), P("d_ent_off"), P("d_names"), P("d_name_off"), ("nentries", "n", 2), P("d_in_off"), P("d_rows"), V("row_pitch", 2320), P("d_len"),
                   P("d_end_bits"), P("d_status"), ("nblocks", "n", 3), P("d_blk_first"), P("d_crc"), ("flags", "f", 0), V("dos_datetime", 0x58210000),
                   V("out_align", 64)]
_ZIP_WRITE_TAIL = [V("total_in", 6144), P("d_file"), V("file_cap", 16384), P("d_entries", None), P("d_result"), P("d_work")]
_ZIP_WRITE_LIMITS = [("out_align", 0), ("out_align", 3), ("out_align", 512), ("out_align", 256), ("nentries", 0), ("nentries", 65535), ("nentries", 65536),
                     ("nblocks", 0), ("file_cap", 0), ("flags", 0x800), ("flags", 0x801)]
CONTAINER_ENTRIES = {
    "hdlz_gunzip_ws": ([P("d_in"), P("d_in_off", None), V("in_pitch", 2048), V("in_len", 2048), ("nstreams", "n", 3), P("d_out"), V("out_pitch", 4096),
                        P("d_out_len"), P("d_status"), P("d_in_used"), P("d_crc"), P("d_work"),
                        ("work_bytes", "w", ("hdlz_gunzip_work_bytes", [3, 2048, 4096, 0]))] + STREAM,
                       _IN_LEN + [("out_pitch", 1 << 32), ("out_pitch", U32 - 3), ("out_pitch", 4095), ("out_pitch", 2), ("out_pitch", 0), ("in_pitch", 2047),
                                  ("nstreams", 0), ("nstreams", 1), ("nstreams", 2)]),
    "hdlz_gzip_members_index_ws": (_MEMBER_INDEX + [("work_bytes", "w", ("hdlz_gzip_members_index_work_bytes", [100000]))] + STREAM,
                                   [("member_cap", 1 << 40), ("member_cap", (1 << 40) - 1), ("file_len", 0)]),
    "hdlz_gzip_members_inflate_ws": ([P("d_file"), V("file_len", 4096), P("d_off"), P("d_out_off"), ("nmembers", "n", 3), P("d_out"), V("out_cap", 6144),
                                      P("d_member_status", None), P("d_result"), P("d_work"),
                                      ("work_bytes", "w", ("hdlz_gzip_members_inflate_work_bytes", [3]))] + STREAM, [("out_cap", 0), ("nmembers", 0)]),
    "hdlz_zip_index_ws": (_ZIP_INDEX + [("work_bytes", "w", ("hdlz_zip_index_work_bytes", [100000, 16]))] + STREAM, _ZIP_INDEX_LIMITS),
    "hdlz_zip_inflate_ws": (_ZIP_INFLATE + [("work_bytes", "w", ("hdlz_zip_inflate_work_bytes", [3, 4096, 65536]))] + STREAM, _ZIP_INFLATE_LIMITS),
    "hdlz_zip64_index_ws": (_ZIP_INDEX + [("work_bytes", "w", ("hdlz_zip64_index_work_bytes", [100000, 16]))] + STREAM, _ZIP_INDEX_LIMITS),
    "hdlz_zip64_inflate_ws": (_ZIP_INFLATE + [("work_bytes", "w", ("hdlz_zip64_inflate_work_bytes", [3, 4096, 65536]))] + STREAM, _ZIP_INFLATE_LIMITS),
    "hdlz_zip_write_ws": (_ZIP_WRITE_HEAD + _ZIP_WRITE_TAIL + [("work_bytes", "w", ("hdlz_zip_write_work_bytes", [2, 3]))] + STREAM, _ZIP_WRITE_LIMITS),
    "hdlz_zip64_write_ws": (_ZIP_WRITE_HEAD + [V("zip64_from", U32)] + _ZIP_WRITE_TAIL + [("work_bytes", "w", ("hdlz_zip64_write_work_bytes", [2, 3]))] + STREAM,
                            _ZIP_WRITE_LIMITS + [("zip64_from", 1 << 32), ("zip64_from", 0)]),
}
# set -> (the entry points, the fixture)
SETS = {"core": (ENTRIES, "api_refusals.json"), "containers": (CONTAINER_ENTRIES, "api_refusals_containers.json")}

# ---- the sizes table of the containers set: every *_work_bytes query of the container headers over the product of its parameters' shapes
_COUNTS = [0, 1, 2, 3, 63, 64, 65, 1000, (1 << 31) - 1, 1 << 31]
SHAPES = {
    "count": _COUNTS,
    "file_len": _COUNTS + [U32, 1 << 32],                                      # (the classic ZIP index ends at 2^32)
    "in_len": [0, 4096, 1 << 20],
    "out": [0, 4, 32768, 32772, (1 << 32) - 512, 1 << 32],                      # out_pitch, out_cap or total_out
    "ragged": [0, 1],
    "hints": [0, 2, 4, 64, 1 << 30],                                           # the three mapping hints; bit 30 is undefined
    "zero": [0, 1],                                                            # (no flag is defined: 1 is undefined)
    "virtual": [0, 1, 2],                                                      # HDLZ_BGZF_RANGE_VIRTUAL; 2 is undefined
}
SIZE_QUERIES = {
    "hdlz_unjoin_work_bytes": ("count", "out", "hints"),
    "hdlz_crc32_work_bytes": ("file_len",),
    "hdlz_join_gzip_work_bytes": ("count",),
    "hdlz_unjoin_gzip_work_bytes": ("count", "out", "hints"),
    "hdlz_bgzf_join_work_bytes": ("count",),
    "hdlz_bgzf_index_work_bytes": ("file_len",),
    "hdlz_bgzf_inflate_work_bytes": ("count", "zero"),
    "hdlz_bgzf_ranges_work_bytes": ("count", "count", "virtual"),
    "hdlz_gunzip_work_bytes": ("count", "in_len", "out", "ragged"),
    "hdlz_gzip_members_index_work_bytes": ("file_len",),
    "hdlz_gzip_members_inflate_work_bytes": ("count",),
    "hdlz_zip_index_work_bytes": ("file_len", "count"),
    "hdlz_zip_inflate_work_bytes": ("count", "in_len", "out"),
    "hdlz_zip64_index_work_bytes": ("file_len", "count"),
    "hdlz_zip64_inflate_work_bytes": ("count", "in_len", "out"),
    "hdlz_zip64_write_work_bytes": ("count", "count"),
    "hdlz_zip_write_work_bytes": ("count", "count"),
}


def sizes_of(L, table):
    """table: {"shapes": .., "queries": {query: {"roles": [..]}}} -> {query: [its answers over itertools.product of its roles' shapes]}"""
    return {q: [getattr(L, q)(*args) for args in itertools.product(*[table["shapes"][r] for r in e["roles"]])] for q, e in table["queries"].items()}


def faults_of(params, special):
    """-> [(parameter index, value, in the pairs too)]: a value is an int, None (null), {"slot": shift} or {"need": delta}"""
    out = []
    for i, (name, kind, good) in enumerate(params):
        if name == "stream":
            continue
        if kind == "p":
            out.append((i, None if good else {"slot": 0}, True))
            out += [(i, {"slot": s}, s in PAIR_SHIFTS) for s in SHIFTS]
        elif kind == "n":
            out += [(i, v, True) for v in (1 << 31, (1 << 31) - 1, U64)]
        elif kind == "f":
            out += [(i, 1 << b, True) for b in range(9)] + [(i, 2 | 4, True), (i, 4 | 64, True)]
        elif kind == "w":
            out += [(i, {"need": -1}, True), (i, 0, True)]
        elif kind == "cw":
            out += [(i, 0, True), (i, 257, True)]
        elif kind == "mm":
            out.append((i, 7, True))
    names = [p[0] for p in params]
    out += [(names.index(n), v, True) for n, v in special]
    return out


def cases_of(entry):
    """the fixture's order of cases: every fault alone, then every pair (i < j) of pair faults on two different parameters"""
    f = entry["faults"]
    single = [(k,) for k in range(len(f))]
    pairs = [(a, b) for a, b in itertools.combinations(range(len(f)), 2) if f[a][2] and f[b][2] and f[a][0] != f[b][0]]
    return single + pairs


class Driver(object):
    """calls one library with the fixture's argument descriptions"""

    def __init__(self, lib_path):
        spec = importlib.util.spec_from_file_location("_hdlz_lib_tables", os.path.join(REPO, "hdl_deflate_amd", "_lib.py"))
        tables = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(tables)                    # the signature tables, without importing the package (and its default library)
        import torch  # noqa: F401                         # (first, as _lib.load() does: the library binds to the HIP runtime torch ships)
        self.L = ctypes.CDLL(lib_path)
        for t in (tables.SIGNATURES, tables.JOIN_SIGNATURES, tables.UNJOIN_SIGNATURES, tables.GZIP_SIGNATURES, tables.BGZF_SIGNATURES,
                  tables.BGZF_RANGE_SIGNATURES, tables.BGZF_STORED_SIGNATURES, tables.GUNZIP_SIGNATURES, tables.ZIP_SIGNATURES,
                  tables.ZIP_WRITE_SIGNATURES, tables.ZIP64_SIGNATURES, tables.GZIP_MEMBERS_SIGNATURES):
            for name, (restype, argtypes) in t.items():
                fn = getattr(self.L, name)
                fn.restype, fn.argtypes = restype, argtypes
        self.keep = (ctypes.c_uint8 * (64 * SLOT + 256))()
        base = ctypes.addressof(self.keep)
        self.base = base + (-base % 256)

    def value(self, i, param, v):
        if isinstance(v, dict) and "slot" in v:
            return self.base + i * SLOT + v["slot"]
        if isinstance(v, dict):
            query, qargs = param[2]
            return getattr(self.L, query)(*qargs) + v["need"]
        return v

    def call(self, name, params, faults):
        args = [({"slot": 0} if good else None) if kind == "p" else {"need": 0} if kind == "w" else good for _, kind, good in params]
        for i, v, _ in faults:
            args[i] = v
        args = [self.value(i, params[i], v) for i, v in enumerate(args)]
        self.L.hdlz_release_scratch()                      # (no device: leaves its own text in hdlz_last_error, so nothing stale is read)
        rc = getattr(self.L, name)(*args)
        return rc, self.L.hdlz_last_error().decode()


def run(driver, name, entry):
    """-> [(rc, message)] in the order of cases_of()"""
    params, faults = entry["params"], entry["faults"]
    return [driver.call(name, params, [faults[k] for k in case]) for case in cases_of(entry)]


def replay(fixture, lib_path):
    """-> [(entry point, case, got, want)] for every case of the fixture that the library answers differently.  The text is the
    library's own where it refuses; behind HDLZ_OK (0: nothing was written) and HDLZ_E_HIP (9: the HIP runtime's words for "no device",
    which belong to the machine) the code alone is compared"""
    d = Driver(lib_path)
    own = lambda ans: ans if ans[0] not in (0, 9) else (ans[0], None)
    table = [own(tuple(a)) for a in fixture["answers"]]
    bad = []
    for name, entry in fixture["entries"].items():
        got = run(d, name, entry)
        assert len(got) == len(entry["results"]), name
        for case, g, w in zip(cases_of(entry), got, entry["results"]):
            if own(g) != table[w]:
                bad.append((name, [entry["faults"][k] for k in case], g, table[w]))
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lib", required=True, help="the libhdlz.so to record from")
    ap.add_argument("--commit", required=True, help="the commit that library was built from, unmodified")
    ap.add_argument("--set", default="core", choices=sorted(SETS), help="which entry points, and so which fixture")
    ap.add_argument("--out", help="default: the set's fixture under tests/golden")
    a = ap.parse_args()
    entry_points, fixture_name = SETS[a.set]
    a.out = a.out or os.path.join(GOLDEN, fixture_name)
    import torch
    if torch.cuda.is_available():
        sys.exit("record_refusals.py runs without a HIP device only: a call that passed every check would launch kernels on host memory")
    d = Driver(a.lib)
    answers, index, entries, total = [], {}, {}, 0
    for name, (params, special) in entry_points.items():
        entry = {"params": [list(p) for p in params], "faults": [list(f) for f in faults_of(params, special)]}
        entry = json.loads(json.dumps(entry))              # (what the replay will see: lists, not tuples)
        results = []
        for ans in run(d, name, entry):
            if ans not in index:
                index[ans] = len(answers)
                answers.append(list(ans))
            results.append(index[ans])
        entry["results"] = results
        entries[name] = entry
        total += len(results)
    fixture = {"about": "tools/record_refusals.py: (return code, hdlz_last_error()) of every single fault and every pair of faults; "
                        "`results` index `answers`, in the order of cases_of()",
               "commit": a.commit, "version": d.L.hdlz_version(), "slot": SLOT, "cases": total, "answers": answers, "entries": entries}
    if a.set == "containers":
        table = {"shapes": SHAPES, "queries": {q: {"roles": list(roles)} for q, roles in SIZE_QUERIES.items()}}
        for q, values in sizes_of(d.L, table).items():
            table["queries"][q]["values"] = values
        fixture["sizes"] = table
    with open(a.out, "w") as f:
        f.write(json.dumps(fixture, separators=(",", ":")).replace('},"hdlz_', '},\n"hdlz_') + "\n")
    print("%d cases, %d distinct answers, %d bytes -> %s" % (total, len(answers), os.path.getsize(a.out), a.out))


if __name__ == "__main__":
    main()
