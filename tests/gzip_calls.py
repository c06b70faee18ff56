"""Buffers and data of the gzip GPU tests (a helper module like guards.py, not a conftest): one compress + join call's buffers, the
ragged batches of small blocks and the blocks of mixed kinds that tests/test_gpu_gzip.py runs through the gzip calls."""
import random

import numpy as np
import torch

from hdl_deflate_amd import _lib
from hdl_deflate_amd.constants import out_bound
from hdl_deflate_amd.data import family_bytes


def round4(x):
    return (x + 3) & ~3


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


_pools = {}


def pool(f):
    """4 KiB of data family f (hdl_deflate_amd.data: 1 .. 4), 0 = random bytes"""
    if f not in _pools:
        _pools[f] = family_bytes(f, 4096, seed=11 + f) if f else bytes(random.Random(5).randrange(256) for _ in range(4096))
    return _pools[f]


def ragged_blocks(B, lo, hi, seed):
    r = random.Random(seed)
    out = []
    for k in range(B):
        n = r.randint(lo, hi)
        a = r.randrange(0, 4096 - n)
        out.append(pool(k % 5)[a:a + n])
    return out


class ZlibCall(object):
    """the buffers of one compress + join; ragged (in_off, `bound` = the stated in_len) or fixed = (n, in_pitch)"""

    def __init__(self, engine, blocks, cw=32, mm=10, bound=0, fixed=None, cap=None, pitch=None):
        self.L, self.B, self.cw, self.mm = engine.lib, len(blocks), cw, mm
        B = self.B
        nmax = max([len(b) for b in blocks] + [bound, 5])
        self.pitch = pitch or round4(out_bound(nmax))
        if fixed:
            n, in_pitch = fixed
            flat = np.zeros(B * in_pitch + 64, np.uint8)
            for b, blk in enumerate(blocks):
                flat[b * in_pitch:b * in_pitch + n] = np.frombuffer(blk, np.uint8)
            self.in_off, self.in_pitch, self.in_len = None, in_pitch, n
        else:
            flat = np.frombuffer(b"".join(blocks) + bytes(64), np.uint8)
            off = np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).astype(np.int64)
            self.in_off, self.in_pitch, self.in_len = dev(off), 0, bound
        self.d_in = dev(flat)
        self.rows = torch.zeros((max(B, 1), self.pitch), dtype=torch.uint8, device="cuda")
        self.out_len, self.status = (torch.full((max(B, 1),), -1, dtype=torch.int32, device="cuda") for _ in range(2))
        self.end_bits = torch.full((max(B, 1),), -1, dtype=torch.int64, device="cuda")
        self.cap = self.L.hdlz_join_bound(B, nmax) if cap is None else cap
        self.stream = torch.zeros(max(self.cap, 1), dtype=torch.uint8, device="cuda")
        self.off = torch.full((B + 1,), -1, dtype=torch.int64, device="cuda")
        self.result = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        self.wb = self.L.hdlz_join_work_bytes(B)
        self.work = torch.zeros(max(self.wb, 8) // 8, dtype=torch.int64, device="cuda")

    def _in(self):
        return (self.d_in.data_ptr(), self.in_off.data_ptr() if self.in_off is not None else None, self.in_pitch, self.in_len, self.B,
                self.cw, self.mm)

    def compress(self):
        rc = self.L.hdlz_compress_batch_bits(*self._in(), self.rows.data_ptr(), self.pitch, self.out_len.data_ptr(), self.status.data_ptr(),
                                             self.end_bits.data_ptr(), stream_ptr())
        assert rc == 0, self.L.hdlz_last_error()

    def compress_plain(self):
        """hdlz_compress_batch on the same input -> (rows, out_len, status) as numpy"""
        rows = torch.zeros_like(self.rows)
        ol, st = torch.zeros_like(self.out_len), torch.zeros_like(self.status)
        rc = self.L.hdlz_compress_batch(*self._in(), rows.data_ptr(), self.pitch, ol.data_ptr(), st.data_ptr(), stream_ptr())
        assert rc == 0, self.L.hdlz_last_error()
        torch.cuda.synchronize()
        return rows.cpu().numpy(), ol.cpu().numpy(), st.cpu().numpy()

    def join(self):
        rc = self.L.hdlz_join_batch_ws(self.rows.data_ptr(), self.pitch, self.out_len.data_ptr(), self.end_bits.data_ptr(),
                                       self.status.data_ptr(), self.in_off.data_ptr() if self.in_off is not None else None, self.in_len,
                                       self.B, self.stream.data_ptr(), self.cap, self.off.data_ptr(), self.result.data_ptr(),
                                       self.work.data_ptr() if self.wb else None, self.wb, stream_ptr())
        assert rc == 0, self.L.hdlz_last_error()

    def record(self):
        torch.cuda.synchronize()
        r = _lib.JoinResult.from_buffer_copy(self.result.cpu().numpy().tobytes())
        return r.stream_len, r.status, r.adler


_kinds = {}


def kind_pool(kind):
    """64 KiB of one kind of data: 1 .. 4 the bench families, 0 random bytes, 5 text of ten letters, 6 zeros"""
    if kind not in _kinds:
        r = random.Random(17 + kind)
        _kinds[kind] = (bytes(r.randrange(256) for _ in range(1 << 16)) if kind == 0 else bytes(1 << 16) if kind == 6 else
                       bytes(r.choice(b"abcdefgh \n") for _ in range(1 << 16)) if kind == 5 else family_bytes(kind, 1 << 16, seed=11 + kind))
    return _kinds[kind]


def blocks_of(lengths, seed, distinct=48):
    """one block per length: text, random bytes, zeros, the bench families in turn, every sixth a repeat of the block in front (same
    length) -- drawn from at most `distinct` places of the pools, so that the CPU reference compresses each block once"""
    r = random.Random(seed)
    out = []
    for k, n in enumerate(lengths):
        if k % 6 == 5 and len(out[-1]) == n:
            out.append(out[-1])
            continue
        a = 64 * r.randrange(distinct)
        out.append(kind_pool(k % 7)[a:a + n])
    return out


def offsets_of(blocks):
    return [0] + [int(x) for x in np.cumsum([len(b) for b in blocks])]


def flipped(z, at, xor):
    z = bytearray(z)
    z[at] ^= xor
    return bytes(z)
