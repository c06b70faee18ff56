"""What hdlz_bgzf_join_stored_ws must answer (include/hdlz_bgzf_stored.h; a helper module like bgzf_ref.py, not a conftest): THE MEMBER
RULE of the header restated in Python on bgzf_ref's header / frame / EOF -- never from device output --, and the crafted blocks whose
row lengths sit on both sides of the rule's tie.  tests/test_bgzf_stored_cabi.py holds all of it against gzip.decompress."""
import zlib

import numpy as np

import bgzf_ref
from bgzf_ref import OK, E_OUT_CAPACITY, E_BAD_PARAM

E_SHORT_INPUT = 1
FIXED, STORED = 0, 1
STORED_MAX = 65505                                                     # 65536 - 23 - 8
NONE_BAD = 0xFFFFFFFF


def choose(row, block, status, row_pitch=None):
    """steps 1 to 5 for one block -> (status, kind, member): a failed block has kind FIXED and an empty member"""
    n, L = len(block), len(row)
    if status not in (OK, E_SHORT_INPUT):
        return status, FIXED, b""                                      # 1.
    if status == OK and (L < 8 or (row_pitch is not None and L > row_pitch)):
        return E_BAD_PARAM, FIXED, b""                                 # 2.
    if n > STORED_MAX:
        return E_OUT_CAPACITY, FIXED, b""                              # 3.
    usable = status == OK and L + 20 <= 65536                          # 4.
    if usable and L + 20 <= n + 31:                                    # 5.: a tie goes to the fixed form
        return OK, FIXED, bgzf_ref.frame(row[2:-4], zlib.crc32(block), n)
    stored = b"\x01" + n.to_bytes(2, "little") + (n ^ 0xFFFF).to_bytes(2, "little") + block
    return OK, STORED, bgzf_ref.frame(stored, zlib.crc32(block), n)


def file(rows, blocks, statuses=None, row_pitch=None):
    """-> (file, offsets[B + 1], kinds[B]): a failed block counts as a member of length 0 (6.); the EOF member behind the last.  What
    the record says of the same batch: record()."""
    statuses = [OK] * len(blocks) if statuses is None else statuses
    out, offs, kinds = b"", [], []
    for row, blk, st in zip(rows, blocks, statuses):
        _, kind, m = choose(row, blk, st, row_pitch)
        offs.append(len(out))
        kinds.append(kind)
        out += m
    offs.append(len(out))
    return out + bgzf_ref.EOF, offs, kinds


def record(rows, blocks, statuses=None, row_pitch=None, cap=None):
    """-> (file_len, nstored, status, first_bad) of hdlz_bgzf_stored_result (7.)"""
    statuses = [OK] * len(blocks) if statuses is None else statuses
    got = [choose(r, b, s, row_pitch) for r, b, s in zip(rows, blocks, statuses)]
    failed = [k for k, g in enumerate(got) if g[0] != OK]
    if failed:
        return 0, 0, max(g[0] for g in got), failed[0]
    f, _, kinds = file(rows, blocks, statuses, row_pitch)
    return len(f), sum(kinds), E_OUT_CAPACITY if cap is not None and len(f) > cap else OK, NONE_BAD


def distinct(n, high, seed):
    """n distinct byte values in random order, `high` of them >= 144 (nine bits as a fixed-Huffman literal, the others eight): no three
    bytes repeat, so every token is a literal and the row is 6 + ceil((3 + 8 n + high + 7) / 8) bytes"""
    r = np.random.default_rng(seed)
    v = np.concatenate([r.permutation(144)[:n - high], 144 + r.permutation(112)[:high]]).astype(np.uint8)
    return bytes(r.permutation(v))


def literal_row_len(n, high):
    return 6 + (3 + 8 * n + high + 7 + 7) // 8


# (label, block, the row's length, the form the rule picks): 100 bytes make a stored member of 131; the row's member is L + 20
CRAFTED = [("c=%d" % c, distinct(100, c, c), L, kind) for c, L, kind in
           ((22, 110, FIXED), (23, 111, FIXED), (30, 111, FIXED), (31, 112, STORED), (38, 112, STORED))] + \
    [("40 high", distinct(40, 40, 40), 53, STORED),
     ("5 random", bytes(np.random.default_rng(5).integers(0, 256, 5, dtype=np.uint8)), 13, FIXED)]


def oracle_rows(oracle, blocks):
    """-> (rows, statuses): what hdlz_compress_batch leaves for these blocks (below 5 bytes: no row, HDLZ_E_SHORT_INPUT)"""
    rows, statuses = [], []
    for b in blocks:
        rc, z = oracle.compress(bytes(b), 32, 10)
        assert rc == (E_SHORT_INPUT if len(b) < 5 else OK)
        rows.append(z)
        statuses.append(rc)
    return rows, statuses
