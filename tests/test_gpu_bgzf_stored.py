"""GPU (-m gpu): the BGZF writer with the stored fallback (include/hdlz_bgzf_stored.h) -- hdlz_bgzf_join_stored_ws byte for byte against
bgzf_stored_ref's statement of the member rule on the CPU oracle's rows (file, d_off, d_kind, the whole record), read by Python's gzip
and by the library's own index, reader and range reader, and the Engine's stored= keyword.  bgzf_stored_ref itself is held against
gzip.decompress in tests/test_bgzf_stored_cabi.py."""
import gzip

import numpy as np
import pytest
import torch

import bgzf_ref
import bgzf_stored_ref as ref
from bgzf_ref import OK, E_OUT_CAPACITY, EOF
from bgzf_stored_ref import FIXED, STORED, E_SHORT_INPUT, NONE_BAD
from hdl_deflate_amd import _lib
from hdl_deflate_amd.bgzf import virtual_offset
from hdl_deflate_amd.constants import pitch_for
from hdl_deflate_amd.errors import HdlzStatusError

pytestmark = pytest.mark.gpu

E_BAD_DISTANCE = 4


def dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype)).cuda()


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def rnd(n, seed, lo=0):
    return bytes(np.random.default_rng(seed).integers(lo, 256, n, dtype=np.uint8))


def text(n, seed):
    return bgzf_ref.data(2 * n, seed)[:n]


class Write(object):
    """CRC + compress + the stored join of a batch: every output pre-filled with junk.  Ragged (in_pitch None: the blocks back to back
    behind d_in_off) or pitched (d_in_off NULL, the first block `shift` bytes behind a 16-byte boundary).  forge: {block: status} put
    into d_status behind the compressor; spoil: the kinds the reference picks -- in front of the join the input bytes of every block
    that takes the fixed form and the row of every block that is stored are overwritten; older: hdlz_bgzf_join_ws from the same rows"""

    def __init__(self, engine, blocks, bound, cap=None, forge=None, spoil=None, older=False, in_pitch=None, shift=0, file_shift=0):
        L = self.L = engine.lib
        B = self.B = len(blocks)
        self.pitch = pitch_for(max(bound, 5))
        if in_pitch is None:
            flat = b"".join(blocks)
            starts = np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).astype(np.int64)
            self.in_off = dev(starts)
            off_ptr, pitch_arg = self.in_off.data_ptr(), 0
        else:
            assert all(len(b) == bound for b in blocks)
            flat = b"".join(b + b"\xEE" * (in_pitch - bound) for b in blocks)[:(B - 1) * in_pitch + bound]      # (ends where the last block ends)
            starts = np.arange(B + 1, dtype=np.int64) * in_pitch
            off_ptr, pitch_arg = None, in_pitch
        self.d_in = dev(np.frombuffer(bytes(shift) + flat + bytes(16), np.uint8))
        assert self.d_in.data_ptr() % 16 == 0
        in_ptr = self.d_in.data_ptr() + shift
        self.rows = torch.full((max(B, 1), self.pitch), 0xA5, dtype=torch.uint8, device="cuda")
        self.out_len, self.status, self.crc = (torch.full((max(B, 1),), -1, dtype=torch.int32, device="cuda") for _ in range(3))
        self.cap = L.hdlz_bgzf_stored_bound(B, bound) if cap is None else cap
        self.file = torch.full((file_shift + self.cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        self.file_ptr = self.file.data_ptr() + file_shift
        self.off = torch.full((B + 1,), -1, dtype=torch.int64, device="cuda")
        self.kind = torch.full((B + 8,), 0x77, dtype=torch.uint8, device="cuda")
        self.result = torch.full((3,), -1, dtype=torch.int64, device="cuda")
        wb = L.hdlz_bgzf_join_stored_work_bytes(B)
        self.work = torch.full((max(wb, 8) // 8,), -1, dtype=torch.int64, device="cuda")
        rc = L.hdlz_crc32_batch_ws(in_ptr, off_ptr, pitch_arg, bound if in_pitch else 0, B, self.crc.data_ptr(), stream_ptr())
        assert rc == 0, L.hdlz_last_error()
        if B:
            rc = L.hdlz_compress_batch(in_ptr, off_ptr, pitch_arg, bound, B, 32, 10, self.rows.data_ptr(), self.pitch, self.out_len.data_ptr(),
                                       self.status.data_ptr(), stream_ptr())
            assert rc == 0, L.hdlz_last_error()
        for b, st in (forge or {}).items():
            self.status[b] = st
        if spoil is not None:
            torch.cuda.synchronize()
            for b, k in enumerate(spoil):
                if k == FIXED:
                    self.d_in[shift + int(starts[b]):shift + int(starts[b]) + len(blocks[b])] ^= 0xFF
                else:
                    self.rows[b] ^= 0xFF
        if older:
            self.old_file = torch.full((L.hdlz_bgzf_bound(B, bound) + 64,), 0x5A, dtype=torch.uint8, device="cuda")
            old_off, old_res = torch.full((B + 1,), -1, dtype=torch.int64, device="cuda"), torch.full((2,), -1, dtype=torch.int64, device="cuda")
            rc = L.hdlz_bgzf_join_ws(self.rows.data_ptr(), self.pitch, self.out_len.data_ptr(), self.status.data_ptr(), off_ptr, bound, B,
                                     self.crc.data_ptr(), self.old_file.data_ptr(), self.old_file.numel() - 64, old_off.data_ptr(), old_res.data_ptr(),
                                     self.work.data_ptr() if wb else None, wb, stream_ptr())
            assert rc == 0, L.hdlz_last_error()
            torch.cuda.synchronize()
            self.old_rec = _lib.BgzfJoinResult.from_buffer_copy(old_res.cpu().numpy().tobytes())
            self.old_bytes = self.old_file.cpu().numpy().tobytes()
            self.old_offsets = [int(x) for x in old_off.cpu().numpy()]
            self.work.fill_(-1)
        rc = L.hdlz_bgzf_join_stored_ws(in_ptr, off_ptr, pitch_arg, bound, self.rows.data_ptr(), self.pitch, self.out_len.data_ptr(),
                                        self.status.data_ptr(), B, self.crc.data_ptr(), self.file_ptr, self.cap, self.off.data_ptr(),
                                        self.kind.data_ptr(), self.result.data_ptr(), self.work.data_ptr() if wb else None, wb, stream_ptr())
        assert rc == 0, L.hdlz_last_error()
        torch.cuda.synchronize()
        r = _lib.BgzfStoredResult.from_buffer_copy(self.result.cpu().numpy().tobytes())
        self.rec = (r.file_len, r.nstored, r.status, r.first_bad)
        self.bytes = self.file.cpu().numpy().tobytes()[file_shift:]
        self.offsets = [int(x) for x in self.off.cpu().numpy()]
        k = self.kind.cpu().numpy()
        self.kinds, self.kind_slack = [int(x) for x in k[:B]], k[B:].tobytes()
        self.lens = [int(x) for x in self.out_len.cpu().numpy()[:B]]


def check(w, blocks, want, offs, kinds):
    """the whole answer of a sound batch against the reference"""
    assert w.rec == (len(want), sum(kinds), OK, NONE_BAD), w.rec
    assert w.offsets == offs
    assert w.kinds == kinds and w.kind_slack == b"\x77" * 8
    assert w.bytes[:len(want)] == want, next(k for k in range(len(want)) if w.bytes[k] != want[k])
    assert w.bytes[w.cap:] == b"\xa5" * 64                                # never a byte at or behind file_cap


_mixed = {}


def mixed(oracle):
    """the mixed ragged batch and its reference, made once: the seven crafted blocks, lengths 0, 1 and 4, text, random bytes, more"""
    if not _mixed:
        blocks = [c[1] for c in ref.CRAFTED] + [b"", b"z", b"abcd", text(2048, 1), rnd(2048, 2)] + \
            [bgzf_ref.data(n, n) for n in (5, 31, 700, 2047, 64, 1999)] + [rnd(33, 3), text(33, 4), b""]
        rows, statuses = ref.oracle_rows(oracle, blocks)
        _mixed.update(blocks=blocks, rows=rows, statuses=statuses, file=ref.file(rows, blocks, statuses))
    return _mixed


def test_a_mixed_ragged_batch(engine, oracle):
    m = mixed(oracle)
    blocks, (want, offs, kinds) = m["blocks"], m["file"]
    assert [len(r) for r in m["rows"][:7]] == [c[2] for c in ref.CRAFTED] and kinds[:7] == [c[3] for c in ref.CRAFTED]
    assert kinds[7:12] == [STORED, STORED, STORED, FIXED, STORED]
    w = Write(engine, blocks, 2048)
    assert w.lens == [len(r) for r in m["rows"]]
    check(w, blocks, want, offs, kinds)
    assert gzip.decompress(w.bytes[:len(want)]) == b"".join(blocks)
    walk = bgzf_ref.walk(w.bytes[:len(want)])
    assert walk.off[:-1] == offs and walk.record() == (len(blocks) + 1, sum(map(len, blocks)), len(want), OK, 1)
    for b, blk in enumerate(blocks):                                     # a member never exceeds its block by more than 31 bytes
        assert offs[b + 1] - offs[b] <= len(blk) + 31
    # d_kind is optional; no blocks: the EOF member alone
    e = Write(engine, [], 64)
    assert e.rec == (28, 0, OK, NONE_BAD) and e.bytes[:28] == EOF and e.offsets == [0] and e.cap == 28 and e.kind_slack == b"\x77" * 8


@pytest.mark.parametrize("B", [513, 770])
def test_tile_seams(engine, oracle, B):
    """compressible blocks and blocks of high bytes alternate with period 3 -- the tile has 256 rows --, lengths 0 and 4 among them: stored
    and fixed members mix inside the tiles and across their seams"""
    r = np.random.default_rng(B)
    blocks = []
    for k in range(B):
        n = 5 + int(r.integers(0, 60))
        blocks.append(bytes([97 + k % 7]) * n if k % 3 == 0 else rnd(n, B + k, lo=144))
    for k, short in ((100, b""), (255, b"abcd"), (256, b""), (257, rnd(64, 9, lo=144)), (511, b"wxyz"), (512, b"")):
        blocks[k] = short
    rows, statuses = ref.oracle_rows(oracle, blocks)
    want, offs, kinds = ref.file(rows, blocks, statuses)
    for t in range(0, B - 1, 256):
        assert {FIXED, STORED} == set(kinds[t:t + 256])
    w = Write(engine, blocks, 64)
    check(w, blocks, want, offs, kinds)
    assert gzip.decompress(w.bytes[:len(want)]) == b"".join(blocks)


def test_all_fixed_files_are_the_older_writers(engine, oracle):
    for lengths, bound in (([40, 64, 700, 2048, 5, 31], 2048), ([8 + k % 57 for k in range(300)], 64), ([57344], 57344)):
        blocks = [bytes([97 + k % 5, 98]) * (n // 2) + b"c" * (n % 2) for k, n in enumerate(lengths)]
        rows, statuses = ref.oracle_rows(oracle, blocks)
        want, offs, kinds = ref.file(rows, blocks, statuses)
        assert kinds == [FIXED] * len(blocks)                            # the reference picks the fixed form everywhere
        w = Write(engine, blocks, bound, older=True)
        check(w, blocks, want, offs, kinds)
        assert (w.old_rec.file_len, w.old_rec.status, w.old_rec.first_bad) == (len(want), OK, NONE_BAD)
        assert w.old_bytes[:len(want)] == w.bytes[:len(want)] and w.old_offsets == w.offsets


def test_the_limits_of_a_member(engine, oracle):
    for n in (65280, 65505):                                             # random bytes: stored, whatever the row came to
        blk = rnd(n, n)
        w = Write(engine, [blk], n)
        assert w.rec == (n + 31 + 28, 1, OK, NONE_BAD) and w.kinds == [STORED] and int(w.status[0]) == OK
        assert gzip.decompress(w.bytes[:n + 59]) == blk and w.bytes[n + 59:] == b"\xa5" * 64
    high = rnd(58230, 5, lo=144)                                         # the fixed form fits (65536) and is the longer one (58261)
    w = Write(engine, [high], 58230)
    assert 58261 < w.lens[0] + 20 <= 65536 and w.rec == (58261 + 28, 1, OK, NONE_BAD) and gzip.decompress(w.bytes[:58289]) == high
    txt = text(65505, 6)                                                 # the longest block there is, compressible: the fixed form
    (row,), _ = ref.oracle_rows(oracle, [txt])
    w = Write(engine, [txt], 65505, older=True)
    assert w.rec == (len(row) + 20 + 28, 0, OK, NONE_BAD) and w.kinds == [FIXED] and w.bytes[:w.rec[0]] == w.old_bytes[:w.rec[0]]
    assert gzip.decompress(w.bytes[:w.rec[0]]) == txt
    over, small = rnd(65506, 7), text(100, 8)
    w = Write(engine, [small, over, small], 65506)
    assert w.rec == (0, 0, E_OUT_CAPACITY, 1) and w.kinds == [FIXED] * 3 and w.bytes[w.cap:] == b"\xa5" * 64
    w = Write(engine, [small, b"abcd", over, b""], 65506)                # SHORT_INPUT is no failure here
    assert w.rec == (0, 0, E_OUT_CAPACITY, 2) and w.kinds == [FIXED, STORED, FIXED, STORED]
    # a status that is the compressor's own failure fails the block with it; the worst status comes first, the lowest block is named
    w = Write(engine, [small, small, over], 65506, forge={1: E_BAD_DISTANCE})
    assert w.rec == (0, 0, E_BAD_DISTANCE, 1)
    w = Write(engine, [small, over, small], 65506, forge={2: E_BAD_DISTANCE})
    assert w.rec == (0, 0, E_BAD_DISTANCE, 1)
    rows, _ = ref.oracle_rows(oracle, [small, small])                    # a forged SHORT_INPUT: stored, whatever the row says
    want, offs, kinds = ref.file(rows, [small, small], [E_SHORT_INPUT, OK])
    assert kinds == [STORED, FIXED]
    check(Write(engine, [small, small], 100, forge={0: E_SHORT_INPUT}), [small, small], want, offs, kinds)


@pytest.mark.parametrize("n", [5, 33, 2047])
def test_pitched_input_at_odd_addresses(engine, oracle, n):
    """d_in_off = NULL, the input at an odd address and an odd pitch, the file at an odd address: sources and destinations of every
    residue modulo 16"""
    blocks = [rnd(n, 100 * n + k, lo=144 if k % 3 == 2 else 0) for k in range(35)]      # (33 bytes are stored only when nearly all are high)
    rows, statuses = ref.oracle_rows(oracle, blocks)
    want, offs, kinds = ref.file(rows, blocks, statuses)
    assert set(kinds) == ({FIXED} if n == 5 else {FIXED, STORED} if n == 33 else {STORED})
    seen = set()
    for shift, file_shift in ((1, 0), (7, 3)):
        w = Write(engine, blocks, n, in_pitch=n + 3, shift=shift, file_shift=file_shift)
        check(w, blocks, want, offs, kinds)
        seen |= {(w.file_ptr + o + (23 if k == STORED else 18)) % 16 for o, k in zip(offs, kinds)}
    assert len(seen) == 16, sorted(seen)                                 # (members of 2078 bytes: the odd residues and, shifted, the even ones)


def test_a_short_capacity(engine, oracle):
    blocks = [ref.CRAFTED[0][1], ref.CRAFTED[4][1], b"abcd", text(64, 1), rnd(40, 2, lo=144)]
    rows, statuses = ref.oracle_rows(oracle, blocks)
    want, offs, kinds = ref.file(rows, blocks, statuses)
    assert kinds == [FIXED, STORED, STORED, FIXED, STORED]
    for cap in (len(want) - 1, len(want) - 28, offs[3] + 5, 17, 0):
        w = Write(engine, blocks, 100, cap=cap)
        assert w.rec == (len(want), 3, E_OUT_CAPACITY, NONE_BAD) == ref.record(rows, blocks, statuses, cap=cap), cap
        assert w.offsets == offs and w.kinds == kinds
        fits = max(o for o in [0] + offs if o <= cap)
        assert w.bytes[:fits] == want[:fits], cap                        # the members in front are complete
        assert w.bytes[cap:] == b"\xa5" * 64, cap                        # never a byte at or behind file_cap


def test_the_join_reads_only_what_it_says(engine, oracle):
    """the input bytes of the blocks that take the fixed form and the rows of the blocks that are stored are overwritten between the
    compressor and the join: the file is the same"""
    m = mixed(oracle)
    blocks, (want, offs, kinds) = m["blocks"], m["file"]
    w = Write(engine, blocks, 2048, spoil=kinds)
    check(w, blocks, want, offs, kinds)


def test_the_readers_take_the_files(engine, oracle):
    m = mixed(oracle)
    big = [text(3000, 1), rnd(65280, 2), text(500, 3), rnd(65280, 4), rnd(65280, 5), text(65280, 6)]
    for blocks, bound in ((m["blocks"], 2048), (big, 65280)):
        w = Write(engine, blocks, bound)
        n, data = w.rec[0], b"".join(blocks)
        assert w.rec[2] == OK and (blocks is not big or w.kinds == [FIXED, STORED, FIXED, STORED, STORED, FIXED])
        f = w.bytes[:n]
        walk = bgzf_ref.walk(f)
        z = w.file[:n]
        off, out_off, rec = engine.bgzf_index(z)
        assert (rec.nmembers, rec.total_out, rec.file_used, rec.status, rec.eof_marker) == walk.record() == (len(blocks) + 1, len(data), n, OK, 1)
        assert list(off.cpu().numpy()) == walk.off and list(out_off.cpu().numpy()) == walk.out_off
        assert engine.inflate_bgzf(z).cpu().numpy().tobytes() == data
        b0, b1 = 1, len(blocks) - 1
        part = engine.inflate_bgzf(z, index=(off, out_off), members=(b0, b1))
        assert part.cpu().numpy().tobytes() == data[walk.out_off[b0]:walk.out_off[b1]]
        # ranges that start and end inside stored members and cross into fixed ones
        s = [b for b, k in enumerate(w.kinds) if k == STORED and len(blocks[b]) >= 33]
        o = walk.out_off
        ranges = [(o[s[0]] + 3, o[s[0]] + 30), (o[s[0]] + 7, o[s[0] + 1] + 9), (o[s[-1] - 1] + 1, o[s[-1]] + 20), (o[s[1]], o[s[1] + 1]), (0, len(data))]
        out, roff = engine.read_bgzf(z, ranges, index=(off, out_off))
        got, ro = out.cpu().numpy().tobytes(), [int(x) for x in roff.cpu().numpy()]
        assert [got[a:b] for a, b in zip(ro, ro[1:])] == [data[a:b] for a, b in ranges]
        virt = [(virtual_offset(walk.off[s[0]], 3), virtual_offset(walk.off[s[0]], 30)),
                (virtual_offset(walk.off[s[0]], 7), virtual_offset(walk.off[s[0] + 1], 9)),
                (virtual_offset(walk.off[s[-1] - 1], 1), virtual_offset(walk.off[s[-1]], 20))]
        out, roff = engine.read_bgzf(z, virt, index=(off, out_off), virtual=True)
        got, ro = out.cpu().numpy().tobytes(), [int(x) for x in roff.cpu().numpy()]
        assert [got[a:b] for a, b in zip(ro, ro[1:])] == [data[a:b] for a, b in ranges[:3]]


def test_engine_stored_keyword(engine):
    pieces = [text(30000, 1), rnd(40000, 2), text(50000, 3), rnd(65280, 4), text(20000, 5)]      # about 200 KB, text and random bytes
    data = b"".join(pieces)
    z = engine.compress_bgzf_bytes(data, stored=True, block=65280)
    B = -(-len(data) // 65280)
    assert gzip.decompress(z) == data and engine.inflate_bgzf_bytes(z) == (OK, data) and z.endswith(EOF)
    assert len(z) < len(data) + 31 * B + 28 + 1
    assert bgzf_ref.walk(z).record() == (B + 1, len(data), len(z), OK, 1)
    with pytest.raises(HdlzStatusError) as e:                            # without it: as before
        engine.compress_bgzf_bytes(data, block=65280)
    assert e.value.status == E_OUT_CAPACITY
    for short in (b"abc", b"a", b"abcd"):
        z = engine.compress_bgzf_bytes(short, stored=True)
        assert gzip.decompress(z) == short and len(z) == len(short) + 31 + 28 and bgzf_ref.walk(z).record() == (2, len(short), len(z), OK, 1)
        assert engine.inflate_bgzf_bytes(z) == (OK, short)
    assert engine.compress_bgzf_bytes(b"", stored=True) == EOF
    txt = text(150000, 7)
    for block in (57344, 2048, 65280):
        assert engine.compress_bgzf_bytes(txt, stored=True, block=block) == engine.compress_bgzf_bytes(txt, block=block)
    d = dev(np.frombuffer(txt, np.uint8))
    for block in (31, 65506, 65536):
        with pytest.raises(ValueError):
            engine.compress_bgzf(d, block=block, stored=True)
