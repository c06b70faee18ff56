"""The job from HOST buffers (Engine.compress_host / Engine.inflate_host): the PCIe hops overlapped with the kernels.  One staging
ring -- three streams, two buffer pairs, the events between them -- and the two payloads that run through it."""
import contextlib

import torch

from .constants import pitch_for


class Ring(object):
    """H2D of chunk k + 1 on s_in | kernels of chunk k on s_k | D2H of an earlier chunk on s_out, over two buffer pairs: chunk k uses
    pair j = k & 1 and goes through stage(j), compute(j) and drain(j), each a scope that makes its stream current, waits for what the
    step depends on and records the step's event on the way out.  These waits are the whole synchronisation of a job: a missing one
    is a rare wrong row, an added one a slower job."""

    def __init__(self, dev, k_priority=0):
        self.s_in, self.s_k, self.s_out = torch.cuda.Stream(dev), torch.cuda.Stream(dev, priority=k_priority), torch.cuda.Stream(dev)

    @contextlib.contextmanager
    def job(self, release=None):
        """the side streams start behind the caller's stream; on the way out (also on an exception: a failed C-ABI call in the loop)
        the caller's stream is behind them again, so nothing stays queued on the side streams behind the caller's back"""
        cur = torch.cuda.current_stream()
        for st in (self.s_in, self.s_k, self.s_out):
            st.wait_stream(cur)
        self.ev_in = [None, None]       # H2D of the chunk that uses buffer pair j
        self.ev_k = [None, None]        # compute of the chunk that last used buffer pair j
        self.ev_out = [None, None]      # D2H of the chunk that last used buffer pair j
        try:
            yield self
        finally:
            for st in (self.s_out, self.s_k, self.s_in):
                cur.wait_stream(st)
            self.s_out.synchronize()
            if release is not None:
                release()

    @contextlib.contextmanager
    def _step(self, stream, waits, done, j):
        with torch.cuda.stream(stream):
            for ev in waits:
                if ev is not None:
                    stream.wait_event(ev)
            yield
            done[j] = torch.cuda.Event()
            done[j].record(stream)

    def stage(self, j):                 # on s_in, behind the compute that read the staged input of pair j two chunks ago
        return self._step(self.s_in, (self.ev_k[j],), self.ev_in, j)

    def compute(self, j):               # on s_k, behind this chunk's H2D and the D2H that read pair j's results two chunks ago
        return self._step(self.s_k, (self.ev_in[j], self.ev_out[j]), self.ev_k, j)

    def drain(self, j):                 # on s_out, behind the chunk's compute
        return self._step(self.s_out, (self.ev_k[j],), self.ev_out, j)


def _pinned(t, shape, dtype):
    return torch.empty(shape, dtype=dtype, pin_memory=True) if t is None else t


def compress_host(eng, h_in, cwindow, maxmatch, chunk_blocks, h_archive, h_len, keep_buffers):
    """Engine.compress_host: the contract is in its docstring"""
    assert h_in.dtype == torch.uint8 and h_in.dim() == 2 and h_in.is_contiguous() and h_in.is_pinned()
    B, n = h_in.shape
    pitch = pitch_for(n)
    if chunk_blocks is None:
        # 48 MiB of input per chunk: its archive stays below 64 MiB -- D2H copies of 64 MiB and more were seen to cost 20 ms per job
        # (73 MiB: 60 ms instead of 40) or to block the host (inflate_host); 16 .. 48 MiB chunks measure the same 39.6 .. 40.0 ms
        chunk_blocks = max(1, min(B, (48 << 20) // max(n, 1)))
    C = chunk_blocks
    h_archive = _pinned(h_archive, B * eng.lib.hdlz_out_bound(n), torch.uint8)
    h_len = _pinned(h_len, B, torch.int32)
    assert h_archive.is_pinned() and h_len.is_pinned() and h_len.numel() == B and h_len.dtype == torch.int32
    assert h_archive.dtype == torch.uint8 and h_archive.dim() == 1 and h_archive.numel() >= B * eng.lib.hdlz_out_bound(n), \
        "h_archive must hold B * hdlz_out_bound(n) bytes (the size of the archive is only known at the end)"
    dev = eng.device
    # streams and staging buffers are kept between calls (a fresh stream has a fresh allocator pool: device mallocs in the job)
    ctx = eng._host_ctx
    if ctx is None or ctx["key"] != (C, n):
        ctx = {"key": (C, n), "ring": Ring(dev),
               "d_in": [torch.empty((C, n), dtype=torch.uint8, device=dev) for _ in range(2)],
               "d_arch": [torch.empty(C * pitch, dtype=torch.uint8, device=dev) for _ in range(2)],
               "d_len": [torch.empty(C, dtype=torch.int32, device=dev) for _ in range(2)],
               "d_rows": torch.empty((C, pitch), dtype=torch.uint8, device=dev),
               "d_tot": [torch.zeros(2, dtype=torch.int64, device=dev) for _ in range(2)]}     # archive bytes, failed blocks
        eng._host_ctx = ctx
    ring, d_in, d_arch, d_len, d_rows, d_tot = ctx["ring"], ctx["d_in"], ctx["d_arch"], ctx["d_len"], ctx["d_rows"], ctx["d_tot"]
    base, bad = 0, 0
    pending = None             # (j, first block, blocks) of the chunk whose D2H is still to be issued

    def drain(p):
        nonlocal base, bad
        j, b0, nb = p
        ring.ev_k[j].synchronize()
        total, nbad = d_tot[j].tolist()               # (the two words were written before ev_k[j])
        with ring.drain(j):
            h_archive[base:base + total].copy_(d_arch[j][:total], non_blocking=True)
            h_len[b0:b0 + nb].copy_(d_len[j][:nb], non_blocking=True)
        base += total
        bad += nbad

    with ring.job(None if keep_buffers else eng.release_host_buffers):
        for k, b0 in enumerate(range(0, B, C)):
            nb = min(C, B - b0)
            j = k & 1
            with ring.stage(j):
                d_in[j][:nb].copy_(h_in[b0:b0 + nb], non_blocking=True)
            with ring.compute(j):
                _, ol, st = eng.compress_batch(d_in[j][:nb], cwindow=cwindow, maxmatch=maxmatch, out=d_rows[:nb], out_pitch=pitch)
                _, off = eng.archive(d_rows[:nb], ol, archive=d_arch[j])      # scan + gather in one launch (hdlz_archive_batch)
                d_len[j][:nb].copy_(ol)
                d_tot[j][0] = off[nb]
                d_tot[j][1] = (st != 0).sum()
            if pending is not None:
                drain(pending)                            # chunk k - 1: its size is known now, its D2H runs beside chunk k's kernels
            pending = (j, b0, nb)
        if pending is not None:
            drain(pending)
    return h_archive, h_len, base, bad


def inflate_host(eng, h_z, h_off, out_pitch, flags, obsize, chunk_streams, h_out, h_len, h_status, keep_buffers, d2h):
    """Engine.inflate_host: the contract and the measurements behind the constants are in its docstring"""
    assert h_z.dtype == torch.uint8 and h_z.dim() == 1 and h_z.is_pinned() and out_pitch % 4 == 0
    h_off = torch.as_tensor(h_off, dtype=torch.int64)
    assert not h_off.is_cuda and h_off.dim() == 1 and h_off.numel() >= 1
    B = h_off.numel() - 1
    h_out = _pinned(h_out, (B, out_pitch), torch.uint8)
    h_len, h_status = _pinned(h_len, B, torch.int32), _pinned(h_status, B, torch.int32)
    assert h_out.is_pinned() and h_len.is_pinned() and h_status.is_pinned() and tuple(h_out.shape) == (B, out_pitch)
    assert h_out.dtype == torch.uint8 and h_out.is_contiguous() and h_len.numel() == B and h_status.numel() == B
    assert h_len.dtype == torch.int32 and h_status.dtype == torch.int32
    if B == 0:
        return h_out, h_len, h_status
    if chunk_streams is None:
        # 256 MiB of rows per chunk: a lane-per-stream batch needs ~10^5 streams to fill the GPU (131 072 streams of 2 KiB take
        # 0.73 ms, 16 384 take 0.6 ms as well), so small chunks only multiply the kernel time (profiles/r04_inflate_host.txt)
        chunk_streams = max(1, min(B, (256 << 20) // max(out_pitch, 1)))
    C = chunk_streams
    piece = max(1, (32 << 20) // max(out_pitch, 1))
    starts = [0] + list(range(max(1, C // 4), B, C))               # chunk k = streams [starts[k], starts[k + 1])
    ends = starts[1:] + [B]
    zlo = [int(h_off[b0]) & ~255 for b0 in starts]                  # (the H2D copies start at aligned host addresses)
    zhi = [min((int(h_off[b1]) + 255) & ~255, h_z.numel()) for b1 in ends]
    zmax = max(b - a for a, b in zip(zlo, zhi))                      # compressed bytes of the largest chunk
    dev = eng.device
    ctx = eng._ihost_ctx
    if ctx is None or ctx["key"] != (C, out_pitch) or ctx["zcap"] < zmax or ctx["h_off"].numel() < B + 1:
        # (the inflate stream has the higher priority: its workgroups are placed before the pending ones of the row copy beside it)
        ctx = {"key": (C, out_pitch), "zcap": zmax, "ring": Ring(dev, k_priority=-1),
               "d_z": [torch.zeros(zmax + 1024, dtype=torch.uint8, device=dev) for _ in range(2)],
               "d_len": [torch.empty((2, C), dtype=torch.int32, device=dev) for _ in range(2)],
               "d_off": [torch.empty(C + 1, dtype=torch.int64, device=dev) for _ in range(2)],
               "h_off": torch.empty(B + 1, dtype=torch.int64, pin_memory=True),
               "row_off": torch.arange(C, dtype=torch.int64, device=dev) * out_pitch,
               "d_out": [torch.empty((C, out_pitch), dtype=torch.uint8, device=dev) for _ in range(2)]}
        eng._ihost_ctx = ctx
    ctx["h_off"][:B + 1].copy_(h_off)                               # pinned copy of the offsets: the per-chunk H2D reads it asynchronously
    ring = ctx["ring"]
    with ring.job(None if keep_buffers else eng.release_host_buffers):
        for k, b0 in enumerate(starts):
            nb = ends[k] - b0
            j = k & 1
            za, zb = zlo[k], zhi[k]
            d_z, d_off, d_len, d_out = ctx["d_z"][j], ctx["d_off"][j], ctx["d_len"][j], ctx["d_out"][j]
            with ring.stage(j):
                d_z[:zb - za].copy_(h_z[za:zb], non_blocking=True)
                d_off[:nb + 1].copy_(ctx["h_off"][b0:b0 + nb + 1], non_blocking=True)
                d_off[:nb + 1].sub_(za)                             # offsets relative to the staged piece
            with ring.compute(j):
                _, ol, st = eng.inflate_batch(d_z, in_off=d_off[:nb + 1], out_pitch=out_pitch, flags=flags, obsize=obsize, out=d_out[:nb])
                d_len[0, :nb].copy_(ol)
                d_len[1, :nb].copy_(st)
            with ring.drain(j):
                if d2h == "kernel":
                    # rows -> pinned host rows by a kernel (row b of the chunk to h_out[b0 + b]; out_len bytes each)
                    rc = eng.lib.hdlz_compact_batch(d_out.data_ptr(), out_pitch, d_len[0].data_ptr(), ctx["row_off"].data_ptr(), nb,
                                                    h_out[b0:].data_ptr(), ring.s_out.cuda_stream)
                    eng._check(rc, "hdlz_compact_batch (rows -> pinned host memory)")
                else:
                    for r0 in range(0, nb, piece):                  # copy-engine transfers of at most 32 MiB (see the docstring)
                        r1 = min(nb, r0 + piece)
                        h_out[b0 + r0:b0 + r1].copy_(d_out[r0:r1], non_blocking=True)
                h_len[b0:b0 + nb].copy_(d_len[0, :nb], non_blocking=True)
                h_status[b0:b0 + nb].copy_(d_len[1, :nb], non_blocking=True)
    return h_out, h_len, h_status
