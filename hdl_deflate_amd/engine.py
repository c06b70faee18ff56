"""Batch engine: thin Python over the C-ABI (include/hdlz.h).  torch is used for device memory and
streams only.  All tensors live on the GPU; nothing here computes on the CPU."""
import ctypes
import functools

import torch

from . import _lib, host
from .constants import OK, E_SHORT_INPUT, E_OUT_CAPACITY, E_NO_EOF, E_BAD_HEADER, E_BAD_CHECKSUM, INFLATE_ONE_FIXED_BLOCK, inflate_cap, pitch_for
from .session import CompressSession, InflateSession
from .errors import Error, HdlzStatusError


def _container_is_gzip(container):
    """the joined stream's two frames: "zlib" (include/hdlz_join.h) and "gzip" (include/hdlz_gzip.h)"""
    if container not in ("zlib", "gzip"):
        raise ValueError("container must be \"zlib\" or \"gzip\", not %r" % (container,))
    return container == "gzip"


def _raise_unless_ok(rec, what, base=0):
    """a result record whose status is not OK -> HdlzStatusError, with .first_bad (counted from `base`) where the record has the word"""
    if rec.status != OK:
        raise HdlzStatusError(rec.status, what, first_bad=base + rec.first_bad if hasattr(rec, "first_bad") else None)


def _gzip_tail_status(st, behind_member, rest, head):
    """the status of a gzip walk whose one-stream call failed with `st`, `rest` bytes in front of the file's end: behind a member, fewer
    than 10 bytes that do not begin like the magic (head(): the first three of them) are no member -- too short for the device to
    look at the magic -- so E_BAD_HEADER, as gzip.decompress answers"""
    return E_BAD_HEADER if behind_member and rest < 10 and not b"\x1f\x8b\x08".startswith(head()) else st


def _is_index(t, count=None):
    """an index array as the library reads it: int64, contiguous, on the device (and of `count` words)"""
    assert t.is_cuda and t.dtype == torch.int64 and t.is_contiguous() and (count is None or t.numel() == count), \
        "an index must be a contiguous int64 device tensor" + ("" if count is None else " of %d words" % count)


def _block_offsets(plan, n, dev):
    """the blocks of chain.plan_blocks over n bytes -> their offsets int64[B + 1] on the device"""
    return torch.tensor([o for o, _ in plan] + [n], dtype=torch.int64).to(dev)


def _on_device(fn):
    """run an Engine method with the engine's GPU current: the C-ABI launches on the CURRENT HIP device and on torch's
    current stream of that device, so an engine built for cuda:1 must not enqueue on cuda:0 because the caller forgot
    torch.cuda.set_device"""
    @functools.wraps(fn)
    def wrapper(self, *a, **kw):
        with torch.cuda.device(self.device):
            return fn(self, *a, **kw)
    return wrapper


class Engine(object):
    """One engine per process/GPU.  Methods enqueue on torch's current stream and return device tensors."""

    def __init__(self, device=None):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("hdl_deflate_amd.Engine needs a HIP device (gfx950); there is no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.lib.hdlz_device_count() < 1:
            raise RuntimeError("no gfx950 device visible to libhdlz")
        self._host_ctx = self._ihost_ctx = None       # what compress_host / inflate_host keep between calls

    # -- helpers
    def _check(self, rc, what):
        if rc != OK:
            raise Error("%s failed: %s (%s)" % (what, self.lib.hdlz_status_string(rc).decode(),
                                                self.lib.hdlz_last_error().decode()))

    @staticmethod
    def _stream():
        return torch.cuda.current_stream().cuda_stream

    def _is_bytes(self, t, name, flat=False, room=0):
        """a buffer as the library reads or writes it: uint8, contiguous, on this engine's device (`flat`: one-dimensional; `room`: of at
        least that many bytes)"""
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and (t.dim() == 1 or not flat) and t.numel() >= room, \
            "%s must be a contiguous%s uint8 device tensor%s" % (name, " flat" if flat else "", " of at least %d bytes" % room if room else "")
        assert t.device == self.device, "%s on %s, engine on %s" % (name, t.device, self.device)

    def _scratch(self, need, work, dtype=None, full=False):
        """the scratch of one library call -> (tensor, its pointer or None when it is empty, its bytes).  Default: `need` bytes from
        torch's allocator, stream-ordered like every other tensor of the call (its blocks start at multiples of 512, which covers the
        8 and the 256 bytes the calls ask for).  A caller's tensor: of `dtype` where the method states one; `full`: refused here when
        it holds fewer than `need` bytes -- else the library decides, or takes a path that needs less."""
        if work is None:
            work = torch.empty(need, dtype=torch.uint8, device=self.device)
        assert work.is_cuda and work.is_contiguous() and work.device == self.device and (dtype is None or work.dtype == dtype)
        nbytes = work.numel() * work.element_size()
        assert nbytes >= need or not full, "the scratch holds %d bytes, the call needs %d" % (nbytes, need)
        return work, (work.data_ptr() if nbytes else None), nbytes

    def _enqueue(self, fn, Struct, scratch, *args):
        """a library call that ends (..., d_result, d_work, work_bytes, stream), enqueued: the record's tensor sized by the struct, the
        call with `scratch` (what _scratch returned) and its check -> the record's device tensor; no host sync"""
        result = torch.empty(ctypes.sizeof(Struct) // 8, dtype=torch.int64, device=self.device)
        self._check(getattr(self.lib, fn)(*args, result.data_ptr(), scratch[1], scratch[2], self._stream()), fn)
        return result

    def _record(self, fn, Struct, scratch, *args):
        """_enqueue, and the record read back -- the one host sync -> the result record"""
        return Struct.from_buffer_copy(self._enqueue(fn, Struct, scratch, *args).cpu().numpy().tobytes())

    def _member_index(self, call, Struct, work_bytes, d_file, member_cap):
        """bgzf_index and gzip_index: the index call with room for member_cap members (default: a guess, file_len // 4096 + 16), made once
        more with the true count when the file holds more -> (member_offsets int64[M + 1], out_offsets int64[M + 1], record)"""
        self._is_bytes(d_file, "d_file", flat=True)
        n, dev = d_file.numel(), d_file.device
        cap = n // 4096 + 16 if member_cap is None else int(member_cap)
        scratch = self._scratch(work_bytes(n), None)
        while True:
            off = torch.empty(cap + 1, dtype=torch.int64, device=dev)
            out_off = torch.empty(cap + 1, dtype=torch.int64, device=dev)
            rec = self._record(call, Struct, scratch, d_file.data_ptr() if n else None, n, cap, off.data_ptr(), out_off.data_ptr())
            if rec.status != E_OUT_CAPACITY or rec.nmembers <= cap:
                return off[:rec.nmembers + 1], out_off[:rec.nmembers + 1], rec
            cap = rec.nmembers

    def _member_range(self, off, out_off, members, out):
        """members=(b0, b1) of a file's index (None: all of them) and where they decode to -> (off, out_off, B, total, out): the two
        index slices of B + 1 words, the range's bytes -- one host sync -- and `out` (default: allocated here) with room for them"""
        _is_index(off)
        _is_index(out_off, off.numel())
        M = off.numel() - 1
        b0, b1 = (0, M) if members is None else (int(members[0]), int(members[1]))
        if not 0 <= b0 <= b1 <= M:
            raise ValueError("members=(%d, %d) is not a range of the file's %d members" % (b0, b1, M))
        off, out_off, B = off[b0:b1 + 1], out_off[b0:b1 + 1], b1 - b0
        total = int((out_off[B] - out_off[0]).item()) if B else 0
        if out is None:
            out = torch.empty(total, dtype=torch.uint8, device=off.device)
        self._is_bytes(out, "out", room=total)
        return off, out_off, B, total, out

    def _aligned_input(self, d_in, n):
        """the compress kernels load whole 16-byte pieces: an input that does not start at a multiple of 16 or has fewer than 16 bytes
        of its storage behind its n bytes is copied to a padded buffer first"""
        slack = d_in.untyped_storage().nbytes() - d_in.storage_offset() - n
        return self._stage(d_in) if d_in.data_ptr() % 16 or slack < 16 else d_in

    def _file_index(self, d_file, index, what):
        """the (member_offsets, out_offsets) of a BGZF file: the caller's, or taken here (bgzf_index) -- a file whose index stops with
        a status raises it, with .first_bad = the number of sound members"""
        if index is None:
            off, out_off, rec = self.bgzf_index(d_file)
            if rec.status != OK:
                raise HdlzStatusError(rec.status, "%s: the file's member index" % what, first_bad=rec.nmembers)
        else:
            off, out_off = index[0], index[1]
        _is_index(off)
        _is_index(out_off, off.numel())
        assert off.numel() >= 1
        return off, out_off

    def _prep(self, d_in, in_off, in_len, nblocks):
        self._is_bytes(d_in, "d_in")
        if in_off is not None:
            _is_index(in_off)
            nb = in_off.numel() - 1
            return in_off.data_ptr(), 0, (0 if in_len is None else in_len), nb
        assert d_in.dim() == 2 or nblocks is not None
        if d_in.dim() == 2:
            nb, pitch = d_in.shape
            return None, pitch, (pitch if in_len is None else in_len), nb
        return None, in_len, in_len, nblocks

    @staticmethod
    def _results(out, shape, nb, dev, checked=False):
        """the result tensors of a call: (out uint8[shape] unless given, out_len int32[nb], status int32[nb]) and, for the checked call,
        (in_used int32[nb], adler int32[nb]) behind them"""
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=dev)
        return (out,) + tuple(torch.empty(nb, dtype=torch.int32, device=dev) for _ in range(4 if checked else 2))

    def _stage(self, data):
        """host bytes (or a flat device tensor) -> a zero-padded device buffer of (n + 15) // 16 * 16 + 16 bytes"""
        n = len(data)
        on_device = torch.is_tensor(data)
        buf = torch.zeros((n + 15) // 16 * 16 + 16, dtype=torch.uint8, device=data.device if on_device else "cpu")
        if n:
            buf[:n] = data if on_device else torch.frombuffer(bytearray(data), dtype=torch.uint8)
        return buf.to(self.device)

    def _compress_one(self, d, n, cwindow, maxmatch):
        """ONE block of n bytes staged by _stage: the stream passes from STREAM_MIN on, a one-row batch below that
        -> (out uint8[>= out_len], out_len int32[1], status int32[1])"""
        if n >= self.STREAM_MIN:
            return self.compress_stream(d, n, cwindow=cwindow, maxmatch=maxmatch)
        out, ol, st = self.compress_batch(d.view(1, -1), in_len=n, cwindow=cwindow, maxmatch=maxmatch)
        return out[0], ol, st

    # -- STARTC for a batch
    @_on_device
    def compress_batch(self, d_in, in_off=None, in_len=None, nblocks=None, cwindow=32, maxmatch=10,
                       out=None, out_pitch=None, max_len=None):
        """d_in: uint8 [B, pitch] (fixed-size blocks) or flat uint8 with in_off int64[B+1] (ascending).
        Returns (out uint8[B, out_pitch], out_len int32[B], status int32[B]); per-block failures are statuses, never
        exceptions.  Ragged batches: pass `max_len` (an upper bound on the block lengths) or `out_pitch` -- without
        either the bound is computed from in_off with ONE host sync per call."""
        off_ptr, pitch, ilen, nb = self._prep(d_in, in_off, in_len, nblocks)
        if out_pitch is None:
            if max_len is None:
                max_len = ilen if in_off is None else int((in_off[1:] - in_off[:-1]).max().item()) if nb else 0
            out_pitch = pitch_for(max_len)
        if in_off is not None:
            # ragged: the bound the library gets is `max_len` (it packs small blocks per wave from it and gives a LONGER block
            # HDLZ_E_BAD_PARAM); `in_len` is not a bound here, as before round 5
            ilen = max_len if max_len is not None else 0
        out, out_len, status = self._results(out, (nb, out_pitch), nb, d_in.device)
        if in_off is None and ilen >= self.LARGE_BLOCK and pitch % 16 == 0 and nb <= self.MANY_WAVES and \
                out_pitch >= (self.lib.hdlz_out_bound(ilen) + 3) // 4 * 4 and self.lib.hdlz_streams_work_bytes(ilen, nb) != 0:
            # (a too small out_pitch stays on the batch path, which reports E_OUT_CAPACITY per block instead of failing the call)
            # few large blocks: one wave per block (hdlz_compress_batch) would leave the GPU idle (a 1 MiB block is 5.5 ms
            # on a wave); all tiles of all blocks go through the stream passes together instead (same bytes)
            work, wptr, wbytes = self._scratch(self.lib.hdlz_streams_work_bytes(ilen, nb), None)
            rc = self.lib.hdlz_compress_streams(d_in.data_ptr(), pitch, ilen, nb, cwindow, maxmatch, out.data_ptr(), out_pitch,
                                                out_len.data_ptr(), status.data_ptr(), wptr, wbytes, self._stream())
            self._check(rc, "hdlz_compress_streams")
            return out, out_len, status
        rc = self.lib.hdlz_compress_batch(d_in.data_ptr(), off_ptr, pitch, ilen, nb, cwindow, maxmatch,
                                          out.data_ptr(), out_pitch, out_len.data_ptr(), status.data_ptr(),
                                          self._stream())
        self._check(rc, "hdlz_compress_batch")
        return out, out_len, status

    # -- CRC-32 of a flat device buffer (include/hdlz_gzip.h)
    @_on_device
    def crc32(self, d_buf, out=None, work=None):
        """d_buf: flat uint8 device tensor, any alignment -> uint32 device tensor[1] holding zlib.crc32 of its bytes (hdlz_crc32_ws).
        No host sync: the word is ready in stream order.  `out`: the tensor to write (default: allocated here); `work`: the call's
        scratch, a device tensor of at least hdlz_crc32_work_bytes(n) bytes (default: allocated here)."""
        self._is_bytes(d_buf, "d_buf", flat=True)
        n, dev = d_buf.numel(), d_buf.device
        if out is None:
            out = torch.empty(1, dtype=torch.uint32, device=dev)
        assert out.is_cuda and out.dtype == torch.uint32 and out.numel() >= 1 and out.device == self.device
        work, wptr, wbytes = self._scratch(self.lib.hdlz_crc32_work_bytes(n), work, full=True)
        rc = self.lib.hdlz_crc32_ws(d_buf.data_ptr() if n else None, n, out.data_ptr(), wptr, wbytes, self._stream())
        self._check(rc, "hdlz_crc32_ws")
        return out

    # -- STARTC for a flat buffer, block by block, as ONE standard zlib stream (include/hdlz_join.h) or gzip member (include/hdlz_gzip.h)
    @_on_device
    def compress_joined(self, d_in, block=1 << 16, cwindow=32, maxmatch=10, out=None, container="zlib"):
        """d_in: flat uint8 device tensor of at least 5 bytes.  It is cut into blocks of `block` bytes (chain.plan_blocks: a tail under
        5 bytes shortens the block before it), the blocks are compressed independently (hdlz_compress_batch_bits, a ragged batch with
        the bound `block`) and joined into one stream that any inflater reads back as d_in (hdlz_join_batch_ws).
        -> (stream uint8[stream_len], member_offsets int64[B + 1]): member b starts at member_offsets[b], the final empty block at
        member_offsets[B].  `out`: the stream's buffer (default: hdlz_join_bound(B, block) bytes).  One host sync (the result record);
        raises HdlzStatusError on a status that is not OK.  An input that does not start at a multiple of 16 or has fewer than 16
        bytes of its storage behind it (the compress kernels load whole 16-byte pieces) is copied to a padded buffer first.
        container="gzip": the same members in the gzip frame (hdlz_join_gzip_ws; member_offsets[0] = 10): the CRC-32 of d_in is computed
        on the same stream in front of the compression (hdlz_crc32_ws), `out` defaults to hdlz_join_gzip_bound(B, block) bytes."""
        from .chain import plan_blocks
        gz = _container_is_gzip(container)
        bound, join, Result = (self.lib.hdlz_join_gzip_bound, "hdlz_join_gzip_ws", _lib.JoinGzipResult) if gz else \
            (self.lib.hdlz_join_bound, "hdlz_join_batch_ws", _lib.JoinResult)
        self._is_bytes(d_in, "d_in", flat=True)
        if not 32 <= block < (1 << 31):
            raise ValueError("block must be in [32, 2^31)")           # (plan_blocks may shorten a block by 16 bytes; a block is below 2 GiB)
        n = d_in.numel()
        plan = plan_blocks(n, block)
        B, dev = len(plan), d_in.device
        d_in = self._aligned_input(d_in, n)
        in_off = _block_offsets(plan, n, dev)
        pitch = pitch_for(block)
        rows, out_len, status = self._results(None, (B, pitch), B, dev)
        end_bits = torch.empty(B, dtype=torch.int64, device=dev)
        if out is None:
            out = torch.empty(bound(B, block), dtype=torch.uint8, device=dev)
        self._is_bytes(out, "out")
        offsets = torch.empty(B + 1, dtype=torch.int64, device=dev)
        scratch = self._scratch(self.lib.hdlz_join_work_bytes(B), None)                    # (the gzip join asks for the same)
        crc = self.crc32(d_in[:n]) if gz else None
        rc = self.lib.hdlz_compress_batch_bits(d_in.data_ptr(), in_off.data_ptr(), 0, block, B, cwindow, maxmatch, rows.data_ptr(), pitch,
                                               out_len.data_ptr(), status.data_ptr(), end_bits.data_ptr(), self._stream())
        self._check(rc, "hdlz_compress_batch_bits")
        rec = self._record(join, Result, scratch, rows.data_ptr(), pitch, out_len.data_ptr(), end_bits.data_ptr(), status.data_ptr(), in_off.data_ptr(),
                           block, B, *([crc.data_ptr()] if gz else []), out.data_ptr(), out.numel(), offsets.data_ptr())
        _raise_unless_ok(rec, "compress_joined")
        return out[:rec.stream_len], offsets

    # -- STARTD for a joined stream, member by member in parallel (include/hdlz_unjoin.h)
    @_on_device
    def inflate_joined(self, d_stream, member_offsets, block=None, out_offsets=None, total=None, out=None, work=None, flags=0,
                       container="zlib"):
        """d_stream: flat uint8 device tensor, the stream compress_joined returned; member_offsets: its int64[B + 1] index.  Where the
        members go is stated like the compress call's input: `block` (with `total`, the length of the data: the output offsets are
        rebuilt from chain.plan_blocks, the plan compress_joined used) or `out_offsets` int64[B + 1] on the device (`total` defaults
        to out.numel(), else to out_offsets[B], which costs a second host sync).  Every member is decoded by the batch kernels straight
        into the flat output and the stream is verified (markers, final block, Adler-32): hdlz_unjoin_ws.
        -> out uint8[total].  One host sync (the result record); raises HdlzStatusError -- with .first_bad, the record's word -- on a
        status that is not OK.  flags: one of the three INFLATE_*_PER_STREAM mapping hints, or 0.  `work`: the call's scratch, a uint8
        device tensor of at least unjoin_work_bytes(B, total, flags) bytes (default: allocated here).
        container="gzip": the stream of compress_joined(container="gzip"), verified as gzip (header, final block, CRC-32, ISIZE):
        hdlz_unjoin_gzip_ws; its scratch is hdlz_unjoin_gzip_work_bytes(B, total, flags) bytes."""
        from .chain import plan_blocks
        gz = _container_is_gzip(container)
        work_bytes, unjoin, Result = (self.lib.hdlz_unjoin_gzip_work_bytes, "hdlz_unjoin_gzip_ws", _lib.UnjoinGzipResult) if gz else \
            (self.lib.hdlz_unjoin_work_bytes, "hdlz_unjoin_ws", _lib.UnjoinResult)
        self._is_bytes(d_stream, "d_stream", flat=True)
        _is_index(member_offsets)
        B, dev = member_offsets.numel() - 1, d_stream.device
        out_len = 0
        if block is not None:
            if block % 4:
                raise ValueError("block = %d is not a multiple of 4: the members' output slots would not start at dword boundaries; "
                                 "read such a stream with inflate_bytes(z, verify=True)" % block)
            if total is None:
                raise ValueError("block= needs total=, the length of the data")
            plan = plan_blocks(total, block) if B else []
            if len(plan) != B:
                raise ValueError("%d bytes in blocks of %d are %d members, the index has %d" % (total, block, len(plan), B))
            if B and all(ln == block for _, ln in plan):
                out_len = block                                      # uniform: no offset array at all
            else:
                out_offsets = _block_offsets(plan, total, dev)
        elif out_offsets is None:
            raise ValueError("one of block= and out_offsets= says where the members go")
        if out_offsets is not None:
            _is_index(out_offsets, B + 1)
        if total is None:
            total = out.numel() if out is not None else int(out_offsets[B].item())
        if out is None:
            out = torch.empty(total, dtype=torch.uint8, device=dev)
        self._is_bytes(out, "out", room=total)
        rec = self._record(unjoin, Result, self._scratch(work_bytes(B, total, flags), work, torch.uint8), d_stream.data_ptr(), d_stream.numel(),
                           member_offsets.data_ptr(), out_offsets.data_ptr() if out_offsets is not None else None, out_len, B, flags,
                           out.data_ptr() if total else None, total, None)
        _raise_unless_ok(rec, "inflate_joined")
        return out[:rec.out_len]

    # -- BGZF, the self-indexing blocked gzip (include/hdlz_bgzf.h): CRC-32 per block, the writer, the member index, the reader
    @_on_device
    def crc32_batch(self, d_buf, offsets=None, pitch=None, length=None, out=None):
        """the CRC-32 (zlib.crc32) of every block of a batch -> uint32 device tensor[B] (hdlz_crc32_batch_ws; no scratch, no host sync).
        d_buf: uint8 device tensor, any alignment.  offsets: int64[B + 1] on the device, ascending: block b is the flat
        d_buf[offsets[b] - offsets[0] : offsets[b + 1] - offsets[0]]; else d_buf is [B, pitch] (or flat with pitch= and length=) and
        block b the first `length` (default: pitch) bytes of row b."""
        self._is_bytes(d_buf, "d_buf")
        if offsets is not None:
            _is_index(offsets)
            assert offsets.numel() >= 1
            B, off_ptr, pitch, length = offsets.numel() - 1, offsets.data_ptr(), 0, 0
        else:
            if d_buf.dim() == 2:
                B, pitch = d_buf.shape
            else:
                assert pitch, "a flat buffer needs offsets= or pitch="
                B = d_buf.numel() // pitch
            length = pitch if length is None else length
            assert 0 <= length <= pitch
            off_ptr = None
        if out is None:
            out = torch.empty(B, dtype=torch.uint32, device=d_buf.device)
        assert out.is_cuda and out.dtype == torch.uint32 and out.numel() >= B and out.device == self.device
        rc = self.lib.hdlz_crc32_batch_ws(d_buf.data_ptr() if d_buf.numel() else None, off_ptr, pitch, length, B,
                                          out.data_ptr() if B else None, self._stream())
        self._check(rc, "hdlz_crc32_batch_ws")
        return out

    @_on_device
    def compress_bgzf(self, d_in, block=57344, cwindow=32, maxmatch=10, out=None, stored=False):
        """d_in: flat uint8 device tensor -> file uint8[file_len], a BGZF file (the blocked gzip of htslib and bgzip) that gzip -d,
        Python's gzip and every htslib tool read back as d_in, and that carries its own member index (bgzf_index).  The input is cut
        into blocks of `block` bytes (chain.plan_blocks), the CRC-32 of every block is taken (crc32_batch), the blocks are compressed
        independently (hdlz_compress_batch) and framed as one gzip member each, with the EOF member behind them (hdlz_bgzf_join_ws).
        block must be in [32, 65536]; a member holds at most 64 KiB, which blocks of up to 58230 bytes always fit -- a larger block of
        bytes that do not compress fails with E_OUT_CAPACITY.  An empty input gives the 28-byte file (the EOF member alone); inputs of
        1 to 4 bytes raise as compress_joined does.  One host sync (the result record); raises HdlzStatusError -- with .first_bad --
        on a status that is not OK.  `out`: the file's buffer (default: hdlz_bgzf_bound(B, block) bytes).
        stored=True (include/hdlz_bgzf_stored.h): a block whose fixed-Huffman member would be longer than the block stored verbatim is
        written as a stored member (hdlz_bgzf_join_stored_ws), so no member exceeds its block by more than 31 bytes and no block fails
        for its content.  block must then be in [32, 65505] -- 65280 is the block size of bgzip and htslib --, inputs of 1 to 4 bytes
        give a valid file of two members, and the default `out` is hdlz_bgzf_stored_bound(B, block) bytes.  The blocks and the rows
        are the same either way, so an input whose blocks all compress gives the same file with and without it."""
        from .chain import plan_blocks
        self._is_bytes(d_in, "d_in", flat=True)
        if stored and not 32 <= block <= 65505:
            raise ValueError("block must be in [32, 65505]: a stored BGZF member holds at most 65505 bytes")
        if not 32 <= block <= 65536:
            raise ValueError("block must be in [32, 65536]: a BGZF member holds at most 64 KiB")
        bound, join, Result = (self.lib.hdlz_bgzf_stored_bound, "hdlz_bgzf_join_stored_ws", _lib.BgzfStoredResult) if stored else \
            (self.lib.hdlz_bgzf_bound, "hdlz_bgzf_join_ws", _lib.BgzfJoinResult)
        n, dev = d_in.numel(), d_in.device
        plan = [(0, n)] if stored and 0 < n < 5 else plan_blocks(n, block) if n else []      # (below 5 bytes the compressor never starts)
        B = len(plan)
        if n:
            d_in = self._aligned_input(d_in, n)
        in_off = _block_offsets(plan, n, dev)
        pitch = pitch_for(block)
        rows, out_len, status = self._results(None, (B, pitch), B, dev)
        if out is None:
            out = torch.empty(bound(B, block), dtype=torch.uint8, device=dev)
        self._is_bytes(out, "out")
        offsets = torch.empty(B + 1, dtype=torch.int64, device=dev)
        scratch = self._scratch(self.lib.hdlz_bgzf_join_work_bytes(B), None)               # (no blocks: none; the stored join asks for the same)
        crc = self.crc32_batch(d_in[:n], offsets=in_off)
        if B:
            rc = self.lib.hdlz_compress_batch(d_in.data_ptr(), in_off.data_ptr(), 0, block, B, cwindow, maxmatch, rows.data_ptr(), pitch,
                                              out_len.data_ptr(), status.data_ptr(), self._stream())
            self._check(rc, "hdlz_compress_batch")
        ptr = lambda t: t.data_ptr() if B else None                                        # (no blocks: the per-block arrays are null)
        row_args = (ptr(rows), pitch, ptr(out_len), ptr(status))
        file_args = (ptr(crc), out.data_ptr(), out.numel(), offsets.data_ptr())
        if stored:                                                                         # the input itself in front, d_kind (not asked for) behind
            args = (ptr(d_in), in_off.data_ptr(), 0, block) + row_args + (B,) + file_args + (None,)
        else:
            args = row_args + (in_off.data_ptr(), block, B) + file_args
        rec = self._record(join, Result, scratch, *args)
        _raise_unless_ok(rec, "compress_bgzf")
        return out[:rec.file_len]

    @_on_device
    def bgzf_index(self, d_file, member_cap=None):
        """d_file: flat uint8 device tensor, a BGZF file -> (member_offsets int64[M + 1], out_offsets int64[M + 1], record): member b is
        d_file[member_offsets[b] : member_offsets[b + 1]] and holds bytes [out_offsets[b], out_offsets[b + 1]) of the data; the record
        (a _lib.BgzfIndexResult: nmembers, total_out, file_used, status, eof_marker) is that of hdlz_bgzf_index_ws -- a status that is
        not OK is returned, not raised: the M members in front of the failure stay valid and indexed.  The members are found on the
        device; one host sync for the record.  member_cap: room for that many members (default: a guess, file_len // 4096 + 16); when
        the file holds more, the call is made once more with the true count."""
        return self._member_index("hdlz_bgzf_index_ws", _lib.BgzfIndexResult, self.lib.hdlz_bgzf_index_work_bytes, d_file, member_cap)

    @_on_device
    def inflate_bgzf(self, d_file, index=None, members=None, out=None, work=None):
        """d_file: flat uint8 device tensor, a BGZF file of this or any other writer (stored, fixed and dynamic blocks) -> out uint8[n],
        every member decoded in parallel and judged by its own trailer (CRC-32, ISIZE): hdlz_bgzf_inflate_ws.  index: the
        (member_offsets, out_offsets) of bgzf_index (default: taken here; a file whose index stops with a status raises it, with
        .first_bad = the number of sound members).  members=(b0, b1): only members b0 .. b1 - 1 are read and decoded -- the same bytes
        as that slice of the whole output.  One host sync for the record (and one for the range's length); raises HdlzStatusError --
        with .first_bad, counted from b0 -- on a status that is not OK.  `work`: the call's scratch, a uint8 device tensor of at
        least hdlz_bgzf_inflate_work_bytes(b1 - b0, 0) bytes at a multiple of 256 (default: allocated here)."""
        self._is_bytes(d_file, "d_file", flat=True)
        off, out_off, B, total, out = self._member_range(*self._file_index(d_file, index, "inflate_bgzf"), members, out)
        rec = self._record("hdlz_bgzf_inflate_ws", _lib.BgzfInflateResult, self._scratch(self.lib.hdlz_bgzf_inflate_work_bytes(B, 0), work, torch.uint8),
                           d_file.data_ptr() if d_file.numel() else None, d_file.numel(), off.data_ptr(), out_off.data_ptr(), B, 0,
                           out.data_ptr() if total else None, total, None)
        _raise_unless_ok(rec, "inflate_bgzf")
        return out[:rec.out_len]

    def compress_bgzf_bytes(self, data, block=57344, cwindow=32, maxmatch=10, stored=False):
        """host bytes -> the bytes of a BGZF file (compress_bgzf)"""
        d = self._stage(data)[:len(data)]
        return bytes(self.compress_bgzf(d, block=block, cwindow=cwindow, maxmatch=maxmatch, stored=stored).cpu().numpy().tobytes())

    def inflate_bgzf_bytes(self, z):
        """the bytes of a BGZF file -> (status, bytes): nothing but the file is needed -- no offsets, no block size, no capacity"""
        d = self._stage(z)[:len(z)]
        try:
            out = self.inflate_bgzf(d)
        except HdlzStatusError as e:
            return e.status, b""
        return OK, bytes(out.cpu().numpy().tobytes())

    # -- random access into a BGZF file (include/hdlz_bgzf_range.h): a batch of ranges by byte or virtual offset
    def _read_ranges(self, d_file, off, out_off, ranges, flags, out, out_cap, task_cap, work):
        """one hdlz_bgzf_read_ranges_ws call and its host sync -> (record, range_off int64[R + 1])"""
        R = ranges.shape[0]
        range_off = torch.empty(R + 1, dtype=torch.int64, device=d_file.device)
        scratch = self._scratch(self.lib.hdlz_bgzf_ranges_work_bytes(R, task_cap, flags), work, torch.uint8, full=True)
        rec = self._record("hdlz_bgzf_read_ranges_ws", _lib.BgzfRangesResult, scratch, d_file.data_ptr() if d_file.numel() else None, d_file.numel(),
                           off.data_ptr(), out_off.data_ptr(), off.numel() - 1, ranges.data_ptr() if R else None, R, flags,
                           out.data_ptr() if out_cap else None, out_cap, range_off.data_ptr(), None, task_cap)
        return rec, range_off

    @_on_device
    def read_bgzf(self, d_file, ranges, index=None, virtual=False, out=None, work=None, max_work_bytes=256 << 20):
        """d_file: flat uint8 device tensor, a BGZF file; ranges: R pairs (begin, end) -- an int64 device tensor [R, 2] or a Python
        sequence of pairs -> (out uint8[total], range_offsets int64[R + 1]), both on the device: range r's bytes are
        out[range_offsets[r] : range_offsets[r + 1]].  The pairs are byte offsets into the data (clipped to it: reading past the end
        is short), or with virtual=True virtual offsets, coffset << 16 | uoffset, as a .bai, .tbi or .csi index gives them
        (hdl_deflate_amd.bgzf.virtual_offset; they fit int64 for files below 2^47 bytes).  Ranges may overlap, repeat and come in any
        order.  Resolved, decoded, judged and trimmed on the device (hdlz_bgzf_read_ranges_ws): only the members the ranges touch are
        decoded, each judged whole by its own trailer.  index: the (member_offsets, out_offsets) of bgzf_index (default: taken here;
        a file whose index stops with a status raises it, as inflate_bgzf does).
        The ranges are processed in groups so that no group's scratch exceeds max_work_bytes: 131072 bytes of slots per range and
        48 bytes per touched member.  A group whose touched members do not fit is halved; a group of ONE range takes what it takes.
        One host sync per call made.  Without `out`: two per group, the sizing call and the read.  With `out`, which must have room
        for all the data: one per group when the guess of its touched members holds -- two per range and one per 256 bytes of room,
        as far as max_work_bytes lets them fit --, else the call that missed was the sizing call and a second one follows.
        `work`: the groups' scratch, a uint8 device tensor at a multiple of 256 whose size stands in for max_work_bytes.
        Raises HdlzStatusError with .first_bad = the index of the lowest failed range over all groups."""
        self._is_bytes(d_file, "d_file", flat=True)
        dev = d_file.device
        off, out_off = self._file_index(d_file, index, "read_bgzf")
        ranges = self._range_pairs(ranges, dev)
        flags = _lib.BGZF_RANGE_VIRTUAL if virtual else 0
        return self._ranged_read("read_bgzf", lambda n, ntasks: self.lib.hdlz_bgzf_ranges_work_bytes(n, ntasks, flags),
                                 lambda rg, dst, ntasks, scratch: self._read_ranges(d_file, off, out_off, rg, flags, dst, dst.numel(), ntasks, scratch),
                                 131072, 48, ranges, dev, out, work, max_work_bytes)

    def _ranged_read(self, what, query, call, slot_bytes, task_bytes, ranges, dev, out, work, max_work_bytes):
        """the groups of read_bgzf and read_seek.  query(n, ntasks): the scratch of a call of n ranges and ntasks tasks, of which
        slot_bytes are a range's slots and task_bytes a task's words; call(ranges, dst, ntasks, scratch) -> (record, range_off)"""
        R = ranges.shape[0]
        if work is not None:
            self._is_bytes(work, "work")
            max_work_bytes = work.numel()
        if out is not None:
            self._is_bytes(out, "out")
        group = max(1, (max_work_bytes - 8192) // (slot_bytes + 256))               # ranges of two tasks each
        while group > 1 and query(group, 2 * group) > max_work_bytes:
            group -= 1
        todo = [(g, min(R, g + group)) for g in range(0, R, group)][::-1]          # a stack: the lowest group on top
        pieces, offsets, pos = [], [], 0

        def scratch(n, ntasks):
            need = query(n, ntasks)
            return work if work is not None and work.numel() >= need else torch.empty(need, dtype=torch.uint8, device=dev)
        while todo:
            g0, g1 = todo.pop()
            rg, n = ranges[g0:g1], g1 - g0
            if out is None:
                dst, ntasks = torch.empty(0, dtype=torch.uint8, device=dev), 0     # the sizing call
            else:
                dst = out[pos:]
                fit = max(0, max_work_bytes - query(n, 0) - 9 * 256) // task_bytes  # task words that fit behind the group's slots
                ntasks = min(fit, 2 * n + dst.numel() // 256)                      # the guess
            rec, range_off = call(rg, dst, ntasks, scratch(n, ntasks))
            if rec.status == E_OUT_CAPACITY:                                       # the sizing call, or a guess that did not hold
                if rec.total_out == (1 << 64) - 1:
                    raise ValueError("%s: the lengths of the ranges exceed 64 bits: the index is not ascending" % what)
                if out is not None and rec.total_out > dst.numel():
                    raise ValueError("%s: `out` has room for %d bytes behind the earlier groups, this one holds %d" % (what, dst.numel(), rec.total_out))
                if n > 1 and query(n, rec.ntasks) > max_work_bytes:
                    mid = g0 + n // 2
                    todo += [(mid, g1), (g0, mid)]
                    continue
                if out is None:
                    dst = torch.empty(rec.total_out, dtype=torch.uint8, device=dev)
                rec, range_off = call(rg, dst, rec.ntasks, scratch(n, rec.ntasks))
            _raise_unless_ok(rec, what, base=g0)
            pieces.append(dst[:rec.total_out])
            offsets.append(range_off[:-1] + pos)
            pos += rec.total_out
        offsets.append(torch.tensor([pos], dtype=torch.int64, device=dev))
        if out is None:
            out = pieces[0] if len(pieces) == 1 else torch.cat(pieces) if pieces else torch.empty(0, dtype=torch.uint8, device=dev)
        return out[:pos], torch.cat(offsets)

    @staticmethod
    def _range_pairs(ranges, dev):
        """R pairs (begin, end), a Python sequence or an int64 device tensor [R, 2] -> the tensor (the words are unsigned)"""
        if not torch.is_tensor(ranges):
            pairs = [[int(v) - (1 << 64) if int(v) >= 1 << 63 else int(v) for v in pair] for pair in ranges]
            ranges = torch.tensor(pairs, dtype=torch.int64).reshape(-1, 2).to(dev)
        assert ranges.is_cuda and ranges.dtype == torch.int64 and ranges.dim() == 2 and ranges.shape[1] == 2 and ranges.is_contiguous()
        return ranges

    def read_bgzf_bytes(self, z, begin, end):
        """the bytes of a BGZF file -> (status, bytes [begin, end) of its data), clipped to the data"""
        d = self._stage(z)[:len(z)]
        try:
            out, _ = self.read_bgzf(d, [(begin, end)])
        except HdlzStatusError as e:
            return e.status, b""
        return OK, bytes(out.cpu().numpy().tobytes())

    # -- random access into any gzip or zlib stream (include/hdlz_seek.h): the seek index of the first read, ranges through it
    @_on_device
    def seek_index(self, d_file, container="gzip", span=1 << 18, point_cap=None, out=None, work=None):
        """d_file: flat uint8 device tensor, ONE zlib stream or a gzip file (its first member) of any writer -> (out uint8[total], a
        SeekIndex (hdl_deflate_amd/seek.py), record): the stream decoded whole and judged as inflate_checked / inflate_gzip judge one
        stream, and the seek points it passed on the way (hdlz_seek_index_ws) -- a block boundary at or behind every multiple of `span`
        bytes of output, each with the 32 KiB in front of it and the CRC-32 of its segment.  The record is a _lib.SeekResult; a
        stream that fails raises HdlzStatusError.  point_cap: room for that many points, 32 KiB of window each (default: a guess --
        the spans of `out`, or of eight times the file where that is less); when the stream holds more, the call is made once more
        with the true count, which decodes it once more.  out: room for the data (default:
        inflate_cap(file_len) bytes, allocated here; for gzip the ISIZE word when it does not exceed that).  One host sync per call
        made.  `work`: the call's scratch, a uint8 device tensor at a multiple of 256 (default: allocated here)."""
        self._is_bytes(d_file, "d_file", flat=True)
        gzip = _container_is_gzip(container)
        n, dev = d_file.numel(), d_file.device
        if out is None:
            cap = inflate_cap(n)
            if gzip and n >= 4:
                isize = int.from_bytes(bytes(d_file[n - 4:].cpu().numpy().tobytes()), "little")
                cap = isize if isize <= cap else cap
            out = torch.empty((cap + 3) & ~3, dtype=torch.uint8, device=dev)
        self._is_bytes(out, "out", flat=True)
        flags = _lib.SEEK_GZIP if gzip else _lib.SEEK_ZLIB
        cap = min(out.numel() // int(span) + 2, 8 * n // int(span) + 16) if point_cap is None else int(point_cap)
        while True:
            bit = torch.empty(cap + 1, dtype=torch.int64, device=dev)
            pos = torch.empty(cap + 1, dtype=torch.int64, device=dev)
            crc = torch.empty(cap, dtype=torch.int32, device=dev)
            win = torch.empty((cap, _lib.SEEK_WINDOW), dtype=torch.uint8, device=dev)
            scratch = self._scratch(self.lib.hdlz_seek_index_work_bytes(n, flags, out.numel(), cap), work, torch.uint8, full=True)
            rec = self._record("hdlz_seek_index_ws", _lib.SeekResult, scratch, d_file.data_ptr() if n else None, n, flags, int(span),
                               out.data_ptr() if out.numel() else None, out.numel(), *[t.data_ptr() if cap else None for t in (bit, pos, crc, win)], cap)
            if rec.status != E_OUT_CAPACITY or rec.npoints <= cap:
                break
            cap = rec.npoints
        _raise_unless_ok(rec, "seek_index")
        from .seek import SeekIndex
        k = rec.npoints
        return out[:rec.total_out], SeekIndex(bit[:k + 1], pos[:k + 1], crc[:k], win[:k], span, n, rec.total_out, rec.end_bit, rec.max_seg, container), rec

    def _read_seek_ranges(self, d_file, index, ranges, out, out_cap, task_cap, scratch):
        """one hdlz_seek_read_ranges_ws call and its host sync -> (record, range_off int64[R + 1])"""
        R = ranges.shape[0]
        range_off = torch.empty(R + 1, dtype=torch.int64, device=d_file.device)
        rec = self._record("hdlz_seek_read_ranges_ws", _lib.SeekRangesResult, self._scratch(0, scratch, torch.uint8),
                           d_file.data_ptr() if d_file.numel() else None, d_file.numel(), index.bit.data_ptr(), index.pos.data_ptr(),
                           index.crc.data_ptr(), index.win.data_ptr(), index.npoints, ranges.data_ptr() if R else None, R, 0, index.max_seg,
                           out.data_ptr() if out_cap else None, out_cap, range_off.data_ptr(), None, task_cap)
        return rec, range_off

    @_on_device
    def read_seek(self, d_file, ranges, index, out=None, work=None, max_work_bytes=256 << 20):
        """d_file: flat uint8 device tensor, the file `index` (a SeekIndex on this device) was taken from; ranges: R pairs (begin, end)
        of byte offsets into the data, as read_bgzf takes them -> (out uint8[total], range_offsets int64[R + 1]), both on the device.
        Only the segments the ranges touch are decoded (hdlz_seek_read_ranges_ws), each whole, from its seek point with its window
        as history, and judged by its length, end bit and CRC-32.  The ranges are processed in groups as in read_bgzf: two slots of
        max_seg bytes per range and 60 bytes per touched segment; out, work and max_work_bytes as there.  Raises HdlzStatusError with
        .first_bad = the index of the lowest failed range over all groups."""
        self._is_bytes(d_file, "d_file", flat=True)
        dev = d_file.device
        assert index.file_len == d_file.numel(), "the index was taken from a file of %d bytes, this one has %d" % (index.file_len, d_file.numel())
        for t in (index.bit, index.pos, index.crc, index.win):
            assert t.is_cuda and t.device == dev and t.is_contiguous(), "the index must be contiguous tensors on the file's device (SeekIndex.to)"
        assert index.win.data_ptr() % 16 == 0
        ranges = self._range_pairs(ranges, dev)
        return self._ranged_read("read_seek", lambda n, ntasks: self.lib.hdlz_seek_ranges_work_bytes(n, ntasks, index.max_seg, 0),
                                 lambda rg, dst, ntasks, scratch: self._read_seek_ranges(d_file, index, rg, dst, dst.numel(), ntasks, scratch),
                                 2 * ((index.max_seg + 255) & ~255), 60, ranges, dev, out, work, max_work_bytes)

    def read_seek_bytes(self, z, begin, end, index=None):
        """the bytes of a .gz file (or, with a zlib index, of a zlib stream) -> (status, bytes [begin, end) of its data), clipped to the
        data.  index: a SeekIndex of the file (default: taken here, as gzip -- which reads the whole file once)"""
        d = self._stage(z)[:len(z)]
        try:
            if index is None:
                _, index, _ = self.seek_index(d, container="gzip")
            out, _ = self.read_seek(d, [(begin, end)], index.to(d.device))
        except HdlzStatusError as e:
            return e.status, b""
        return OK, bytes(out.cpu().numpy().tobytes())

    # -- ZIP archives (include/hdlz_zip.h): the directory indexed and the entries read on the device
    @_on_device
    def zip_index(self, d_file, entry_cap=None, out_align=1, zip64="auto"):
        """d_file: flat uint8 device tensor, a ZIP file (.zip, .npz, .jar, .whl, .docx) -> a ZipIndex (hdl_deflate_amd/zip.py): the device
        records of hdlz_zip_index_ws, its result record, a host copy of the records and the entries' names.  A status that is not OK --
        the record's or an entry's -- is returned, not raised: the entries in front of a stop stay valid and indexed.  entry_cap: room
        for that many records (default: the sizing call first, then the call with the true count); out_align: every entry's slot in the
        flat output starts at a multiple of it (a power of two up to 256).  One host sync per call for the record, one for the records
        and one for the names.
        zip64: "auto" -- a file of 2^32 bytes or more goes to hdlz_zip64_index_ws (include/hdlz_zip64.h); a smaller one to the classic
        call first and to the new one only when that failed in its step 1 (status != OK and nentries == 0: a locator, say), so a file
        without a locator returns what it always did.  True / False force one call.  The index says which it was (.zip64): the records
        of the new call are 64 bytes each (ENTRY64_DTYPE on the host, the same names)."""
        from .zip import ZipIndex, ENTRY_DTYPE, ENTRY64_DTYPE, decode_name
        import numpy as np
        self._is_bytes(d_file, "d_file", flat=True)
        if zip64 not in ("auto", True, False):
            raise ValueError("zip64 must be \"auto\", True or False, not %r" % (zip64,))
        n, dev = d_file.numel(), d_file.device

        def run(wide):
            call, work_bytes, words = ("hdlz_zip64_index_ws", self.lib.hdlz_zip64_index_work_bytes, 8) if wide else \
                ("hdlz_zip_index_ws", self.lib.hdlz_zip_index_work_bytes, 6)
            cap = 0 if entry_cap is None else int(entry_cap)
            while True:
                entries = torch.empty((cap, words), dtype=torch.int64, device=dev)
                rec = self._record(call, _lib.ZipIndexResult, self._scratch(work_bytes(n, cap), None, full=True), d_file.data_ptr() if n else None,
                                   n, cap, out_align, entries.data_ptr() if cap else None)
                if entry_cap is not None or rec.status != E_OUT_CAPACITY or rec.nentries <= cap:
                    return entries, rec, cap
                cap = rec.nentries

        wide = zip64 is True or (zip64 == "auto" and n >= 1 << 32)
        entries, rec, cap = run(wide)
        if zip64 == "auto" and not wide and rec.status != OK and rec.nentries == 0:
            again = run(True)
            if again[1].status == OK or again[1].nentries:      # (else: no ZIP of either form -- the classic answer stands)
                wide, (entries, rec, cap) = True, again
        k = min(cap, rec.nentries)
        entries = entries[:k]
        host = np.frombuffer(entries.cpu().numpy().tobytes(), dtype=ENTRY64_DTYPE if wide else ENTRY_DTYPE)
        # the names: bytes [cd_off + 46, cd_off + 46 + name_len) of every record, gathered on the device, one copy to the host
        lens = host["name_len"].astype(np.int64)
        ends = np.cumsum(lens)
        raw = b""
        if k and int(ends[-1]):
            starts = torch.from_numpy((host["cd_off"].astype(np.int64) + 46) - (ends - lens)).to(dev)
            at = torch.repeat_interleave(starts, torch.from_numpy(lens).to(dev)) + torch.arange(int(ends[-1]), dtype=torch.int64, device=dev)
            raw = d_file[at].cpu().numpy().tobytes()
        names = [decode_name(raw[int(e - l):int(e)], int(f)) for e, l, f in zip(ends, lens, host["flags"])]
        return ZipIndex(entries, rec, host, names, out_align, wide)

    @_on_device
    def inflate_zip(self, d_file, index=None, first=0, count=None, out=None, work=None):
        """d_file: flat uint8 device tensor, a ZIP file; index: its ZipIndex (default: taken here, with slots at multiples of 16)
        -> (out uint8[n], out_off int64[count], status int32[count]), all on the device: entry first + k of the index stands at
        out[out_off[k] : out_off[k] + usize] and has status[k] -- HDLZ_OK, or why it was not read; nothing is raised for an entry.  Any
        range [first, first + count) reads without the rest.  The range is routed here: maximal runs of entries below ZIP_LARGE_MIN
        compressed bytes go in one hdlz_zip_inflate_ws call each, a wave per entry; every larger entry goes in a call of its own, decoded
        by the whole GPU (when its slot starts at a multiple of 4: index with out_align >= 4) -- in ascending order, all into the same
        flat `out`.  An index of hdlz_zip64_index_ws (index.zip64) is read by hdlz_zip64_inflate_ws, routed the same way.  out: at least
        the range's bytes rounded up to 4 (default: allocated here); work: the scratch of the largest call, uint8 at a multiple of 256
        (default: allocated here).  No host sync behind the index."""
        self._is_bytes(d_file, "d_file", flat=True)
        dev = d_file.device
        if index is None:
            index = self.zip_index(d_file, out_align=16)
        host, E = index.host, len(index.host)
        count = E - first if count is None else int(count)
        if not 0 <= first <= first + count <= E:
            raise ValueError("entries [%d, %d) are not a range of the index's %d entries" % (first, first + count, E))
        ok = host["status"] == OK
        rel = (host["out_off"] - (host["out_off"][first] if count else 0)).astype("int64")
        size = host["usize"].astype("int64") * ok
        total = int(rel[first + count - 1] + size[first + count - 1]) if count else 0
        room = (total + 3) & ~3
        if out is None:
            out = torch.empty(room, dtype=torch.uint8, device=dev)
        self._is_bytes(out, "out", flat=True, room=room)
        status = torch.empty(count, dtype=torch.int32, device=dev)
        out_off = index.entries[first:first + count, 2] - (index.entries[first, 2] if count else 0)
        # the calls: (first entry, count, in_len, out_cap)
        calls, e, end = [], first, first + count
        while e < end:
            if ok[e] and host["csize"][e] >= _lib.ZIP_LARGE_MIN:
                # (in_len sizes the decoder's scratch: a stored entry of a ZIP64 index, which may hold 4 GiB and more, is only copied)
                il = 0 if index.zip64 and host["method"][e] == 0 else min(int(host["csize"][e]) + 6, 0xFFFFFFFF)
                calls.append((e, 1, il, min((int(size[e]) + 3) & ~3, out.numel() - int(rel[e]))))
                e += 1
                continue
            b = e
            while e < end and not (ok[e] and host["csize"][e] >= _lib.ZIP_LARGE_MIN):
                e += 1
            cap = int(rel[e - 1] + size[e - 1] - rel[b])
            calls.append((b, e - b, 0, cap if e - b > 1 else min((cap + 3) & ~3, out.numel() - int(rel[b]))))      # (one entry: a row of whole words)
        work_bytes, inflate = (self.lib.hdlz_zip64_inflate_work_bytes, "hdlz_zip64_inflate_ws") if index.zip64 else \
            (self.lib.hdlz_zip_inflate_work_bytes, "hdlz_zip_inflate_ws")
        scratch = self._scratch(max([work_bytes(c, il, cap) for _, c, il, cap in calls] + [0]), work, torch.uint8)
        for b, c, il, cap in calls:                           # (the records are not read: every entry's verdict is in `status`)
            self._enqueue(inflate, _lib.ZipInflateResult, scratch, d_file.data_ptr(), d_file.numel(), index.entries.data_ptr(), b, c, il,
                          out.data_ptr() + int(rel[b]) if out.numel() else None, cap, status.data_ptr() + 4 * (b - first))
        return out[:total], out_off, status

    def read_zip_bytes(self, z):
        """the bytes of a ZIP file -> (status, {name: bytes}): every entry that read OK, as zipfile's read() gives it (of two entries of
        one name the later one).  status: that of the lowest failed entry; when every indexed entry is sound, that of the index (a
        directory that stops early, a file that is no ZIP)."""
        d = self._stage(z)[:len(z)]
        index = self.zip_index(d, out_align=16)
        out, out_off, status = self.inflate_zip(d, index)
        data, off, st = out.cpu().numpy(), out_off.cpu().numpy(), status.cpu().numpy()
        files, worst = {}, OK
        for k, name in enumerate(index.names):
            if st[k] == OK:
                files[name] = data[off[k]:off[k] + int(index.host["usize"][k])].tobytes()
            elif worst == OK:
                worst = int(st[k])
        return (worst if worst != OK else index.record.status), files

    # -- PNG images (include/hdlz_png.h): the chunks walked, the pixels inflated, unfiltered and expanded on the device
    PNG_ALONE_US = 1483.0            # a hdlz_png_decode_ws call of ONE 512 x 512 RGB image, end to end: 379.7 ms for 256 (profiles/png.txt)
    PNG_WAVE_US_PER_BYTE = 0.109     # the wave-per-image decode: 85.7 ms for 786944 bytes of scanlines (profiles/png.txt)

    @_on_device
    def png_index(self, d_files, offsets=None, lengths=None, out_align=64, expand=True, interlaced=False):
        """d_files: flat uint8 device tensor holding PNG files; offsets, lengths: int64 device tensors, file i is
        d_files[offsets[i] : offsets[i] + lengths[i]] (default: one file, all of d_files) -- the out_off and usize of Engine.inflate_zip's
        index fit as they stand -> a PngIndex (hdl_deflate_amd/png.py): the device records of hdlz_png_index_ws, its result record and a
        host copy.  An image's status stands in its record and is not raised.  expand: plain samples (HDLZ_PNG_EXPAND: (H, W, C), uint8 or
        little-endian uint16) or the scanlines as PNG packs them (HDLZ_PNG_RAW); out_align: every image's slot in the flat output starts
        at a multiple of it (a power of two up to 256).  interlaced: HDLZ_PNG_ADAM7 -- Adam7 interlaced images are indexed (the slot
        will hold the deinterlaced image) instead of refused.  One host sync for the records."""
        from .png import PngIndex, IMAGE_DTYPE
        import numpy as np
        self._is_bytes(d_files, "d_files", flat=True)
        dev = d_files.device
        if offsets is None:
            offsets = torch.zeros(1, dtype=torch.int64, device=dev)
            lengths = torch.full((1,), d_files.numel(), dtype=torch.int64, device=dev)
        offsets, lengths = offsets.to(torch.int64).contiguous(), lengths.to(torch.int64).contiguous()
        _is_index(offsets)
        _is_index(lengths, offsets.numel())
        n, flags = offsets.numel(), (_lib.PNG_EXPAND if expand else _lib.PNG_RAW) | (_lib.PNG_ADAM7 if interlaced else 0)
        images = torch.empty((n, ctypes.sizeof(_lib.PngImage) // 8), dtype=torch.int64, device=dev)
        rec = self._record("hdlz_png_index_ws", _lib.PngIndexResult, self._scratch(self.lib.hdlz_png_index_work_bytes(n, n), None, full=True),
                           d_files.data_ptr() if n else None, d_files.numel(), offsets.data_ptr() if n else None, lengths.data_ptr() if n else None,
                           n, flags, out_align, n, images.data_ptr() if n else None)
        host = np.frombuffer(images.cpu().numpy().tobytes(), dtype=IMAGE_DTYPE)
        return PngIndex(images, rec, host, out_align, bool(expand), bool(interlaced))

    @_on_device
    def decode_png(self, d_files, index, first=0, count=None, out=None, work=None):
        """d_files: the buffer the PngIndex `index` was taken of -> (out uint8[n], status int32[count]), both on the device: image
        first + k stands at out[rel : rel + out_len], rel = out_off[first + k] - out_off[first], and has status[k] -- HDLZ_OK, or why it
        was not read; nothing is raised for an image.  Any range [first, first + count) decodes without the rest.  The range is routed
        here as Engine.inflate_zip routes entries: maximal runs of images below PNG_LARGE_MIN compressed bytes go in one
        hdlz_png_decode_ws call each, a wave per image; every larger image goes in a call of its own, decoded by the whole GPU -- unless
        the range holds so many large images that their calls would cost more than the longest of them costs a wave: then the whole
        range is one call.  out: at
        least the range's bytes (default: allocated here); work: the scratch of the largest call, uint8 at a multiple of 256 (default:
        allocated here).  No host sync."""
        self._is_bytes(d_files, "d_files", flat=True)
        dev = d_files.device
        host, E = index.host, len(index.host)
        count = E - first if count is None else int(count)
        if not 0 <= first <= first + count <= E:
            raise ValueError("images [%d, %d) are not a range of the index's %d images" % (first, first + count, E))
        ok = host["status"] == OK
        end = first + count
        rel = (host["out_off"] - (host["out_off"][first] if count else 0)).astype("int64")
        size = host["out_len"].astype("int64") * ok
        total = int(rel[end - 1] + size[end - 1]) if count else 0
        if out is None:
            out = torch.empty(total, dtype=torch.uint8, device=dev)
        self._is_bytes(out, "out", flat=True, room=total)
        status = torch.empty(count, dtype=torch.int32, device=dev)
        r16 = lambda x: (int(x) + 15) & ~15
        # which images go alone: a call of its own costs PNG_ALONE_US whatever the image, a wave takes PNG_WAVE_US_PER_BYTE per decoded
        # byte and a batch pays only its longest image -- many large images are faster together
        large = ok & (host["zlen"] >= _lib.PNG_LARGE_MIN)
        large[:first] = large[end:] = False
        if large.any() and int(large.sum()) * self.PNG_ALONE_US > int(host["raw_len"][large].max()) * self.PNG_WAVE_US_PER_BYTE:
            large[:] = False
        calls, e = [], first
        while e < end:
            b = e
            if large[e]:
                e += 1
            else:
                while e < end and not large[e]:
                    e += 1
            last = e - 1
            calls.append((b, e - b, int(host["nidat"][b:e].sum()),
                          int(host["z_off"][last] - host["z_off"][b]) + r16(host["zlen"][last] + 8) * int(ok[last]),
                          int(host["raw_off"][last] - host["raw_off"][b]) + r16(host["raw_len"][last]) * int(ok[last]),
                          int(rel[last] + size[last] - rel[b])))
        scratch = self._scratch(max([self.lib.hdlz_png_decode_work_bytes(c, ic, zb, rb) for _, c, ic, zb, rb, _ in calls] + [0]), work, torch.uint8)
        flags = (_lib.PNG_EXPAND if index.expand else _lib.PNG_RAW) | (_lib.PNG_ADAM7 if index.interlaced else 0)
        for b, c, ic, zb, rb, cap in calls:                     # (the records are not read: every image's verdict is in `status`)
            self._enqueue("hdlz_png_decode_ws", _lib.PngDecodeResult, scratch, d_files.data_ptr(), d_files.numel(), index.images.data_ptr(), b, c,
                          flags, ic, zb, rb, out.data_ptr() + int(rel[b]) if out.numel() else None, cap, status.data_ptr() + 4 * (b - first))
        return out[:total], status

    # -- TIFF images (include/hdlz_tiff.h): the directory walked, the strips and tiles inflated, the predictor undone on the device
    @_on_device
    def tiff_index(self, d_files, offsets=None, lengths=None, pages=None, out_align=64):
        """d_files: flat uint8 device tensor holding TIFF files; offsets, lengths: int64 device tensors, file i is
        d_files[offsets[i] : offsets[i] + lengths[i]] (default: one file, all of d_files) -- the out_off and usize of Engine.inflate_zip's
        index fit as they stand; pages: per image the directory (IFD) read of its file, a sequence of ints or a tensor (default: the
        first of every file; a pyramid or a stack is read by naming its file once per page) -> a TiffIndex (hdl_deflate_amd/tiff.py):
        the device records of hdlz_tiff_index_ws, its result record and a host copy.  An image's status stands in its record and is not
        raised.  out_align: every image's slot in the flat output starts at a multiple of it (a power of two up to 256).  One host sync
        for the records."""
        from .tiff import TiffIndex, IMAGE_DTYPE
        import numpy as np
        self._is_bytes(d_files, "d_files", flat=True)
        dev = d_files.device
        if offsets is None:
            offsets = torch.zeros(1, dtype=torch.int64, device=dev)
            lengths = torch.full((1,), d_files.numel(), dtype=torch.int64, device=dev)
        offsets, lengths = offsets.to(torch.int64).contiguous(), lengths.to(torch.int64).contiguous()
        _is_index(offsets)
        _is_index(lengths, offsets.numel())
        n = offsets.numel()
        if pages is not None:
            pages = np.asarray(pages.cpu().numpy() if isinstance(pages, torch.Tensor) else pages, dtype=np.int64).reshape(-1)
            if pages.size != n or (n and (pages.min() < 0 or pages.max() > 0xFFFFFFFF)):
                raise ValueError("pages must hold one page number in [0, 2^32) per image (%d)" % n)
            pages = torch.from_numpy(pages.astype(np.uint32).view(np.int32).copy()).to(dev)
        images = torch.empty((n, ctypes.sizeof(_lib.TiffImage) // 8), dtype=torch.int64, device=dev)
        rec = self._record("hdlz_tiff_index_ws", _lib.TiffIndexResult, self._scratch(self.lib.hdlz_tiff_index_work_bytes(n, n), None, full=True),
                           d_files.data_ptr() if n else None, d_files.numel(), offsets.data_ptr() if n else None, lengths.data_ptr() if n else None,
                           pages.data_ptr() if pages is not None and n else None, n, out_align, n, images.data_ptr() if n else None)
        host = np.frombuffer(images.cpu().numpy().tobytes(), dtype=IMAGE_DTYPE)
        return TiffIndex(images, rec, host, out_align)

    @_on_device
    def decode_tiff(self, d_files, index, first=0, count=None, out=None, work=None):
        """d_files: the buffer the TiffIndex `index` was taken of -> (out uint8[n], status int32[count]), both on the device: image
        first + k stands at out[rel : rel + out_len], rel = out_off[first + k] - out_off[first], and has status[k] -- HDLZ_OK, or why it
        was not read; nothing is raised for an image.  Any range [first, first + count) decodes without the rest.  The range is routed
        here as Engine.decode_png routes: maximal runs of images go in one hdlz_tiff_decode_ws call each, a wave per strip or tile of
        all of them; an image of ONE deflate chunk in a file of at least TIFF_LARGE_MIN bytes goes in a call of its own, decoded by the
        whole GPU.  out: at least the range's bytes (default: allocated here); work: the scratch of the largest call, uint8 at a
        multiple of 256 (default: allocated here).  No host sync."""
        self._is_bytes(d_files, "d_files", flat=True)
        dev = d_files.device
        host, E = index.host, len(index.host)
        count = E - first if count is None else int(count)
        if not 0 <= first <= first + count <= E:
            raise ValueError("images [%d, %d) are not a range of the index's %d images" % (first, first + count, E))
        ok = host["status"] == OK
        end = first + count
        rel = (host["out_off"] - (host["out_off"][first] if count else 0)).astype("int64")
        size = host["out_len"].astype("int64") * ok
        total = int(rel[end - 1] + size[end - 1]) if count else 0
        if out is None:
            out = torch.empty(total, dtype=torch.uint8, device=dev)
        self._is_bytes(out, "out", flat=True, room=total)
        status = torch.empty(count, dtype=torch.int32, device=dev)
        # what an image takes of the decoded chunks: every chunk's bytes rounded up to 16 (step 7 of the header's rule)
        r16 = lambda x: (x + 15) & ~15
        nch = host["nchunks"].astype("int64")
        full = host["tile_w"].astype("int64") * host["tile_h"] * host["samples"] * (host["bits"] // 8)
        raw16 = ((nch - 1) * r16(full) + r16(host["raw_len"].astype("int64") - (nch - 1) * full)) * ok
        # which images go alone: a single-strip deflate image whose file -- all but the strip is a directory -- says the stream is a large
        # one (the strip's byte count stands in the file, on the device, and is not fetched for this)
        large = ok & (host["nchunks"] == 1) & (host["compression"] != 1) & (host["file_len"] >= _lib.TIFF_LARGE_MIN)
        large[:first] = large[end:] = False
        # ... unless they are so many that their calls would cost more than the longest of them costs a wave (decode_png's weighing, with
        # its two numbers: not measured again for TIFF)
        if large.any() and int(large.sum()) * self.PNG_ALONE_US > int(host["raw_len"][large].max()) * self.PNG_WAVE_US_PER_BYTE:
            large[:] = False
        calls, e = [], first
        while e < end:
            b = e
            if large[e]:
                e += 1
            else:
                while e < end and not large[e]:
                    e += 1
            last = e - 1
            calls.append((b, e - b, int(host["nchunks"][b:e][ok[b:e]].sum()), int(host["raw_off"][last] - host["raw_off"][b]) + int(raw16[last]),
                          int(rel[last] + size[last] - rel[b])))
        scratch = self._scratch(max([self.lib.hdlz_tiff_decode_work_bytes(c, cc, rb) for _, c, cc, rb, _ in calls] + [0]), work, torch.uint8)
        for b, c, cc, rb, cap in calls:                         # (the records are not read: every image's verdict is in `status`)
            self._enqueue("hdlz_tiff_decode_ws", _lib.TiffDecodeResult, scratch, d_files.data_ptr(), d_files.numel(), index.images.data_ptr(), b, c,
                          cc, rb, out.data_ptr() + int(rel[b]) if out.numel() else None, cap, status.data_ptr() + 4 * (b - first))
        return out[:total], status

    # -- PNG files written on the device (include/hdlz_png_write.h)
    PNG_FILTERS ={"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": 5}

    @_on_device
    def encode_png(self, d_pix, specs, filter="adaptive", block=1 << 16, idat=1 << 16, cwindow=32, maxmatch=10, out=None, out_align=64,
                   expand=True, check=True):
        """d_pix: flat uint8 device tensor holding the samples of n images in the layout decode_png delivers with expand set: C-order
        (H, W, C), uint8 or little-endian uint16.  specs: a numpy array of png.SPEC_DTYPE (pix_off, width, height, depth, colour), or
        a list of shapes (H, W, C, depth) of images packed in d_pix one behind the other, C = 1, 2, 3, 4 for grey, grey + alpha, RGB,
        RGBA -> (files uint8[total], PngIndex): every image's PNG file, packed -- image i is files[file_off : file_off + file_len] of
        its record --, and the index png_index would take of them under (out_align, expand): the files are not indexed again.
        filter: "adaptive" (per row the filter with the smallest sum of absolute residuals, libpng's rule), a name of PNG_FILTERS
        or 0 .. 4: that filter for every row.  hdlz_png_filter_ws filters all images into one packed buffer, every image of at least
        5 stream bytes is cut into blocks of `block` bytes (chain.plan_blocks, from the dimensions alone), ONE ragged
        hdlz_compress_batch_bits deflates all blocks, and hdlz_png_write_ws frames the files with IDAT chunks of `idat` bytes.  out:
        the files' buffer (default: hdlz_png_write_bound bytes).  One host sync (the record, with the images' records, offsets and
        lengths behind it).  check: raise HdlzStatusError -- with .first_bad, the lowest failed image -- on a status that is not OK;
        without it the statuses stand in the index's records and index.write_record, and the sound images are written.  The index also
        carries .row_filters (uint8 on the device: the filter of every row) and .row_base (where an image's rows start in it)."""
        from .png import PngIndex, IMAGE_DTYPE
        import numpy as np
        p = self._png_plan(d_pix, specs, filter, block, idat, cwindow, maxmatch, out, out_align, expand)
        self._png_launch(p)
        n, nres, nrec = p.n, p.nres, p.nrec
        back = p.res.cpu().numpy()                              # the one host sync
        rec = _lib.PngWriteResult.from_buffer_copy(back[:nres].tobytes())
        if check and rec.status != OK:
            raise HdlzStatusError(rec.status, "encode_png", first_bad=None if rec.first_bad == 2 ** 64 - 1 else rec.first_bad)
        host = np.frombuffer(back[nres:nres + nrec * n].tobytes(), dtype=IMAGE_DTYPE)
        ok = host["status"] == OK
        r16 = lambda x: (int(x) + 15) & ~15
        last = int(np.nonzero(ok)[0][-1]) if ok.any() else None
        record = _lib.PngIndexResult(n, 0 if last is None else int(host["z_off"][last]) + r16(host["zlen"][last] + 8),
                                     0 if last is None else int(host["raw_off"][last]) + r16(host["raw_len"][last]),
                                     int(host["out_off"][-1]) + int(host["out_len"][-1]) if n else 0, OK, 0)
        index = PngIndex(p.images.view(n, nrec), record, host, out_align, bool(expand))
        index.write_record, index.row_filters, index.row_base = rec, p.row_filter[:p.total_rows], p.row_base
        total = rec.total_len if rec.total_len <= p.out.numel() else 0
        return p.out[:total], index

    def _png_plan(self, d_pix, specs, filter, block, idat, cwindow, maxmatch, out, out_align, expand):
        """everything of encode_png in front of its launches: the specs, the block plan from the dimensions alone, one staged copy of
        the index arrays, every buffer of the three calls -> a namespace of them"""
        from types import SimpleNamespace
        from .png import SPEC_DTYPE, COLOUR_OF_CHANNELS
        from .chain import plan_blocks
        import numpy as np
        self._is_bytes(d_pix, "d_pix", flat=True)
        dev, pix_len = d_pix.device, d_pix.numel()
        mode = self.PNG_FILTERS.get(filter, filter) if isinstance(filter, str) else filter
        if isinstance(mode, bool) or not isinstance(mode, int) or not 0 <= mode <= 5:
            raise ValueError("filter must be one of %s or 0 .. 4, not %r" % (sorted(self.PNG_FILTERS), filter))
        if not 32 <= block < (1 << 31) or not 1 <= idat < (1 << 31):
            raise ValueError("block must be in [32, 2^31) and idat in [1, 2^31)")
        if isinstance(specs, np.ndarray) and specs.dtype == SPEC_DTYPE:
            sp = np.ascontiguousarray(specs)
        else:
            sp = np.zeros(len(specs), SPEC_DTYPE)
            at = 0
            for k, (h, w, c, depth) in enumerate(specs):
                if c not in COLOUR_OF_CHANNELS or depth not in (8, 16):
                    raise ValueError("image %d: %d channels of %d bits (1 .. 4 channels of 8 or 16 bits are written)" % (k, c, depth))
                sp[k] = (at, w, h, depth, COLOUR_OF_CHANNELS[c], 0)
                at += h * w * c * (depth // 8)
        n = len(sp)
        # the block plan, from the dimensions alone: what hdlz_png_filter_ws will answer for every image is known here
        raw_off, blk_first, in_off, row_base, runs = [0], [0], [0], [0], []
        for r in sp:
            w, h, depth, colour = int(r["width"]), int(r["height"]), int(r["depth"]), int(r["colour"])
            sound = 0 < w < (1 << 31) and 0 < h < (1 << 31) and colour in (0, 2, 4, 6) and depth in (8, 16) and not r["reserved"].any()
            raw_len = 0
            if sound:
                rb = w * {0: 1, 2: 3, 4: 2, 6: 4}[colour] * (depth // 8)
                sound = h * (rb + 1) <= (1 << 32) - 512 and int(r["pix_off"]) <= pix_len and h * rb <= pix_len - int(r["pix_off"])
                raw_len = h * (rb + 1) if sound else 0
            if raw_len >= 5:
                if runs and runs[-1][1] + runs[-1][2] == raw_off[-1]:
                    runs[-1][2] += raw_len
                else:
                    runs.append([in_off[-1], raw_off[-1], raw_len])      # a run of blocked streams: where it goes, where it lies, its bytes
                for _, ln in plan_blocks(raw_len, block):
                    in_off.append(in_off[-1] + ln)
            row_base.append(row_base[-1] + (h if sound else 0))
            raw_off.append(raw_off[-1] + raw_len)
            blk_first.append(len(in_off) - 1)
        B, total_raw = len(in_off) - 1, raw_off[-1]
        words = np.array(blk_first + in_off, dtype=np.int64)
        staged = torch.from_numpy(np.concatenate([words.view(np.uint8), sp.view(np.uint8).reshape(-1)])).to(dev)
        idx = staged[:8 * words.size].view(torch.int64)
        pitch = pitch_for(block)
        rows, out_len, status = self._results(None, (B, pitch), B, dev)
        if out is None:
            out = torch.empty(self.lib.hdlz_png_write_bound(n, total_raw, B, block, idat), dtype=torch.uint8, device=dev)
        self._is_bytes(out, "out", flat=True)
        nres, nrec = ctypes.sizeof(_lib.PngWriteResult) // 8, ctypes.sizeof(_lib.PngImage) // 8
        res = torch.empty(nres + (nrec + 2) * n, dtype=torch.int64, device=dev)
        # (16 bytes behind the streams: the compress kernels load whole 16-byte pieces.)  The blocks are cut from the packed streams as they
        # lie; only when a stream under 5 bytes -- which gets no blocks -- lies between two that have some are the blocked streams copied
        # to a buffer of their own, so that the blocks stand back to back (hdlz_png_write_ws uses only differences of d_in_off)
        raw = torch.empty(total_raw + 32, dtype=torch.uint8, device=dev)
        gaps = bool(runs) and (len(runs) > 1 or runs[0][1] != 0)
        cin = torch.empty(in_off[-1] + 32, dtype=torch.uint8, device=dev) if gaps else raw
        return SimpleNamespace(
            n=n, B=B, mode=mode, block=block, idat=idat, cwindow=cwindow, maxmatch=maxmatch, total_rows=row_base[-1], row_base=row_base, total_raw=total_raw,
            d_pix=d_pix, staged=staged, blk_first=idx[:n + 1], in_off=idx[n + 1:], specs=staged[8 * words.size:],
            raw=raw, cin=cin, runs=runs if gaps else [],
            fstatus=torch.empty(max(n, 1), dtype=torch.int32, device=dev), raw_off=torch.empty(n + 1, dtype=torch.int64, device=dev),
            row_filter=torch.empty(max(row_base[-1], 1), dtype=torch.uint8, device=dev),
            fwork=self._scratch(self.lib.hdlz_png_filter_work_bytes(n), None, full=True), rows=rows, pitch=pitch, len=out_len, status=status,
            end_bits=torch.empty(B, dtype=torch.int64, device=dev), out=out, nres=nres, nrec=nrec, res=res, images=res[nres:nres + nrec * n],
            file_off=res[nres + nrec * n:nres + (nrec + 1) * n], file_len=res[nres + (nrec + 1) * n:],
            wwork=self._scratch(self.lib.hdlz_png_write_work_bytes(n, B), None, full=True),
            flags=_lib.PNG_EXPAND if expand else _lib.PNG_RAW, out_align=out_align)

    def _png_launch(self, p):
        """the three calls of encode_png over a _png_plan, on the current stream: nothing is allocated, nothing crosses to the host
        -- a linear chain that a graph captures"""
        n, B = p.n, p.B
        ptr = lambda t, some: t.data_ptr() if some else None
        self._check(self.lib.hdlz_png_filter_ws(ptr(p.d_pix, p.d_pix.numel()), p.d_pix.numel(), ptr(p.specs, n), n, p.mode, p.total_rows, p.raw.data_ptr(),
                                                p.total_raw, p.row_filter.data_ptr(), ptr(p.fstatus, n), ptr(p.raw_off, n), p.fwork[1], p.fwork[2],
                                                self._stream()), "hdlz_png_filter_ws")
        for dst, src, ln in p.runs:
            p.cin[dst:dst + ln].copy_(p.raw[src:src + ln])
        if B:
            self._check(self.lib.hdlz_compress_batch_bits(p.cin.data_ptr(), p.in_off.data_ptr(), 0, p.block, B, p.cwindow, p.maxmatch, p.rows.data_ptr(),
                                                          p.pitch, p.len.data_ptr(), p.status.data_ptr(), p.end_bits.data_ptr(), self._stream()),
                        "hdlz_compress_batch_bits")
        some = lambda t: t.data_ptr() if B else None
        self._check(self.lib.hdlz_png_write_ws(ptr(p.specs, n), n, p.raw.data_ptr(), ptr(p.raw_off, n), ptr(p.fstatus, n), some(p.in_off), some(p.rows),
                                               p.pitch, some(p.len), some(p.end_bits), some(p.status), B, ptr(p.blk_first, n), p.idat, p.flags, p.out_align,
                                               ptr(p.out, p.out.numel()), p.out.numel(), ptr(p.file_off, n), ptr(p.file_len, n), None, ptr(p.images, n),
                                               p.res.data_ptr(), p.wwork[1], p.wwork[2], self._stream()), "hdlz_png_write_ws")

    # -- ZIP archives written on the device (include/hdlz_zip_write.h)
    ZIP_CRC_TILED_MIN = 1 << 17  # an entry of at least this many bytes gets a hdlz_crc32_ws call of its own

    @_on_device
    def compress_zip(self, d_in, entry_lengths, names, block=1 << 16, cwindow=32, maxmatch=10, store=None, out=None,
                     date_time=(1980, 1, 1, 0, 0, 0), out_align=1, zip64="auto"):
        """d_in: flat uint8 device tensor, the entries' bytes one behind the other; entry_lengths: their lengths, a host sequence;
        names: their names (str, written as UTF-8 -- flag bit 11 is set when one of them is not ASCII -- or bytes)
        -> (file uint8[file_len], ZipIndex): a ZIP archive that zipfile, unzip and numpy.load read, and its index as zip_index would
        return it (out_align: what its slots' starts are multiples of) -- the file is not indexed again.  Every entry of at least 5
        bytes is cut into blocks of `block` bytes (chain.plan_blocks), ALL blocks of all entries are compressed in one ragged
        hdlz_compress_batch_bits, and hdlz_zip_write_ws writes every entry deflated or stored, whichever is shorter; an entry under 5
        bytes, or one with store[e] true, gets no blocks and is stored.  The CRC-32 of the entries is taken on the same stream
        (crc32_batch; an entry of at least ZIP_CRC_TILED_MIN bytes by crc32, the whole GPU).  date_time: (year, month, day, hour,
        minute, second) of every entry.  `out`: the file's buffer (default: hdlz_zip_write_bound bytes).  One host sync (the record,
        with the entries' records behind it); raises HdlzStatusError -- with .first_bad, the lowest failed entry -- on a status that
        is not OK.
        zip64: "auto" -- hdlz_zip_write_ws, and so the bytes it always wrote, when there are at most 65535 entries and
        hdlz_zip_write_bound(...) < 2^32 - 1; otherwise hdlz_zip64_write_ws (include/hdlz_zip64.h) with zip64_from = FFFFFFFF: ZIP64
        fields only where the format needs them.  "always": zip64_from = 0; an integer up to FFFFFFFF is passed through as
        zip64_from.  The index of the new call has .zip64 set and 64-byte records."""
        from .zip import ZipIndex, ENTRY_DTYPE, ENTRY64_DTYPE, decode_name
        import numpy as np
        if zip64 not in ("auto", "always") and not (isinstance(zip64, int) and not isinstance(zip64, bool) and 0 <= zip64 <= 0xFFFFFFFF):
            raise ValueError("zip64 must be \"auto\", \"always\" or a zip64_from in [0, 0xFFFFFFFF], not %r" % (zip64,))
        z = self._zip_batch(d_in, entry_lengths, names, block, cwindow, maxmatch, store)
        classic = self.lib.hdlz_zip_write_bound(z.E, z.B, block, z.total, z.names.numel())
        z.zip64_from = None if zip64 == "auto" and z.E <= 65535 and classic < 0xFFFFFFFF else 0xFFFFFFFF if zip64 == "auto" else 0 if zip64 == "always" else zip64
        wide = z.zip64_from is not None
        if out is None:
            bound = self.lib.hdlz_zip64_write_bound(z.E, z.B, block, z.total, z.names.numel()) if wide else classic
            out = torch.empty(bound, dtype=torch.uint8, device=d_in.device)
        rec, res, back = self._zip_write(z, out, date_time, out_align)
        _raise_unless_ok(rec, "compress_zip")
        host = np.frombuffer(back.tobytes(), dtype=ENTRY64_DTYPE if wide else ENTRY_DTYPE)
        total_out = int(host["out_off"][-1]) + int(host["usize"][-1]) if z.E else 0
        record = _lib.ZipIndexResult(z.E, total_out, rec.cd_off, rec.cd_size, OK, 0)
        index = ZipIndex(res.view(z.E, 8 if wide else 6), record, host, [n if isinstance(n, str) else decode_name(n, z.flags) for n in names], out_align, wide)
        index.write_record = rec
        return out[:rec.file_len], index

    def _zip_batch(self, d_in, entry_lengths, names, block, cwindow, maxmatch, store):
        """what hdlz_zip_write_ws is given, on the device: the index arrays and the names (one staged copy), the CRC-32 of every entry,
        the rows of ONE hdlz_compress_batch_bits over all blocks of all entries -> a namespace of them (E entries, B blocks)"""
        from types import SimpleNamespace
        from .chain import plan_blocks
        from .zip import FLAG_UTF8
        import numpy as np
        self._is_bytes(d_in, "d_in", flat=True)
        lens = [int(x) for x in entry_lengths]
        E, total, dev = len(lens), d_in.numel(), d_in.device
        names = list(names)
        if len(names) != E or (store is not None and len(store) != E):
            raise ValueError("%d entries, %d names%s" % (E, len(names), "" if store is None else ", %d store flags" % len(store)))
        if min(lens, default=0) < 0 or sum(lens) != total:
            raise ValueError("the entries' lengths add up to %d bytes, d_in holds %d" % (sum(lens), total))
        if not 32 <= block < (1 << 31):
            raise ValueError("block must be in [32, 2^31)")
        raw = [n.encode("utf-8") if isinstance(n, str) else bytes(n) for n in names]
        flags = FLAG_UTF8 if any(not r.isascii() for r in raw) else 0
        # the block plan: per entry chain.plan_blocks, none for an entry under 5 bytes or one that is to be stored
        ent_off, name_off, blk_first, in_off, blocked = [0], [0], [0], [0], []
        for e, u in enumerate(lens):
            ent_off.append(ent_off[-1] + u)
            name_off.append(name_off[-1] + len(raw[e]))
            if u >= 5 and not (store is not None and store[e]):
                blocked.append(e)
                for _, ln in plan_blocks(u, block):
                    in_off.append(in_off[-1] + ln)
            blk_first.append(len(in_off) - 1)
        B = len(in_off) - 1
        # every index array and the names in ONE staged copy: four arrays of 64-bit words, the names' bytes behind them
        words = np.array(ent_off + name_off + blk_first + in_off, dtype=np.int64)
        staged = torch.from_numpy(np.concatenate([words.view(np.uint8), np.frombuffer(b"".join(raw), np.uint8)])).to(dev)
        idx = staged[:8 * words.size].view(torch.int64)
        d_ent_off, d_name_off, d_blk_first, d_in_off = idx[:E + 1], idx[E + 1:2 * E + 2], idx[2 * E + 2:3 * E + 3], idx[3 * E + 3:]
        # the CRC-32: runs of small entries in one crc32_batch each, a large entry by the tiled kernels into its own word
        crc = torch.zeros(max(E, 1), dtype=torch.int32, device=dev).view(torch.uint32)      # (a run without bytes is not summed: its words stay 0)
        e = 0
        while e < E:
            if lens[e] >= self.ZIP_CRC_TILED_MIN:
                self.crc32(d_in[ent_off[e]:ent_off[e + 1]], out=crc[e:e + 1])
                e += 1
                continue
            b = e
            while e < E and lens[e] < self.ZIP_CRC_TILED_MIN:
                e += 1
            if ent_off[e] > ent_off[b]:
                self.crc32_batch(d_in[ent_off[b]:ent_off[e]], offsets=d_ent_off[b:e + 1], out=crc[b:e])
        # ONE ragged compress over all blocks of all entries; the blocked entries in a buffer of their own when others lie between them
        pitch = pitch_for(block)
        rows, out_len, status = self._results(None, (B, pitch), B, dev)
        end_bits = torch.empty(B, dtype=torch.int64, device=dev)
        if B:
            cin = d_in if in_off[-1] == total else torch.cat([d_in[ent_off[k]:ent_off[k + 1]] for k in blocked])
            cin = self._aligned_input(cin, in_off[-1])
            rc = self.lib.hdlz_compress_batch_bits(cin.data_ptr(), d_in_off.data_ptr(), 0, block, B, cwindow, maxmatch, rows.data_ptr(), pitch,
                                                   out_len.data_ptr(), status.data_ptr(), end_bits.data_ptr(), self._stream())
            self._check(rc, "hdlz_compress_batch_bits")
        return SimpleNamespace(E=E, B=B, total=total, flags=flags, d_in=d_in, ent_off=d_ent_off, names=staged[8 * words.size:], name_off=d_name_off,
                               in_off=d_in_off, rows=rows, pitch=pitch, len=out_len, end_bits=end_bits, status=status, blk_first=d_blk_first, crc=crc,
                               staged=staged)

    def _zip_write(self, z, out, date_time, out_align):
        """hdlz_zip_write_ws -- or, with z.zip64_from set, hdlz_zip64_write_ws -- over a _zip_batch into `out` -> (the record, the
        entries' records int64[6 E] (int64[8 E]) on the device, the same on the host): the record and the entries' records stand in
        one tensor and come back in one copy, the call's one host sync"""
        from .zip import dos_datetime
        self._is_bytes(out, "out", flat=True)
        wide = getattr(z, "zip64_from", None) is not None
        nres = ctypes.sizeof(_lib.ZipWriteResult) // 8
        res = torch.empty(nres + (8 if wide else 6) * z.E, dtype=torch.int64, device=self.device)
        scratch = self._scratch((self.lib.hdlz_zip64_write_work_bytes if wide else self.lib.hdlz_zip_write_work_bytes)(z.E, z.B), None)
        ptr = lambda t: t.data_ptr() if z.B else None                    # (no blocks: the per-block arrays are null)
        some = lambda t: t.data_ptr() if t.numel() else z.staged.data_ptr()   # (no byte of an empty buffer is read: any address will do)
        front = (some(z.d_in), z.ent_off.data_ptr(), some(z.names), z.name_off.data_ptr(), z.E, ptr(z.in_off), ptr(z.rows),
                 z.pitch, ptr(z.len), ptr(z.end_bits), ptr(z.status), z.B, z.blk_first.data_ptr(), z.crc.data_ptr(), z.flags,
                 dos_datetime(date_time), out_align)
        back_ = (z.total, out.data_ptr() if out.numel() else None, out.numel(),
                 res[nres:].data_ptr() if z.E else None, res.data_ptr(), scratch[1], scratch[2], self._stream())
        if wide:
            self._check(self.lib.hdlz_zip64_write_ws(*front, z.zip64_from, *back_), "hdlz_zip64_write_ws")
        else:
            self._check(self.lib.hdlz_zip_write_ws(*front, *back_), "hdlz_zip_write_ws")
        back = res.cpu().numpy()
        return _lib.ZipWriteResult.from_buffer_copy(back[:nres].tobytes()), res[nres:], back[nres:]

    def write_zip_bytes(self, files, **kw):
        """{name: bytes} -> the bytes of a ZIP archive holding them in that order, the counterpart of read_zip_bytes; the keywords of
        compress_zip (block, cwindow, maxmatch, store, date_time, zip64) pass through"""
        names = list(files)
        data = [bytes(files[n]) for n in names]
        d = self._stage(b"".join(data))[:sum(len(x) for x in data)]
        out, _ = self.compress_zip(d, [len(x) for x in data], names, **kw)
        return bytes(out.cpu().numpy().tobytes())

    # -- STARTC for ONE large stream, spread over the whole GPU (same bytes as compress_batch with one block)
    STREAM_MIN = 1 << 14          # measured crossover with the single-wave batch path: ~8 KiB
    LARGE_BLOCK, MANY_WAVES = 1 << 16, 1200   # compress_batch: up to this many blocks of at least this size -> stream passes
                                              # (a wave does ~180 MB/s, the stream passes ~250 GB/s: crossover ~1400 blocks)

    @_on_device
    def compress_stream(self, d_in, n, cwindow=32, maxmatch=10, out=None, work=None):
        """d_in: flat uint8 device tensor, readable up to n rounded up to 16.
        Returns (out uint8[cap], out_len int32[1], status int32[1])."""
        self._is_bytes(d_in, "d_in", room=(n + 15) // 16 * 16)
        cap = pitch_for(n)
        out, out_len, status = self._results(out, cap, 1, d_in.device)
        work, wptr, wbytes = self._scratch(self.lib.hdlz_stream_work_bytes(n), work)
        rc = self.lib.hdlz_compress_stream(d_in.data_ptr(), n, cwindow, maxmatch, out.data_ptr(), out.numel(),
                                           out_len.data_ptr(), status.data_ptr(), wptr, wbytes, self._stream())
        self._check(rc, "hdlz_compress_stream")
        return out, out_len, status

    # -- STARTD for a batch
    @_on_device
    def inflate_batch(self, d_in, in_off=None, in_len=None, nblocks=None, out_pitch=None, flags=0, obsize=0,
                      out=None, work=None):
        """STARTD for a batch: d_in uint8 [B, pitch] (a stream per row, `in_len` bytes of it: default the pitch) or flat uint8 with in_off
        int64[B + 1] -- then `in_len`, if given, is an UPPER BOUND on the stream lengths: with it a batch of large streams can take
        the whole-GPU path (a stream longer than the bound is still decoded, by the serial pass).
        `work`: the call's scratch, a uint8 device tensor (hdlz_inflate_batch_ws: the library allocates nothing); default: a tensor of
        hdlz_inflate_work_bytes(...) bytes from torch's allocator, stream-ordered like every other tensor of the call; a smaller one
        (or an empty one) gives the same results through mappings that need less.
        -> (out uint8[B, out_pitch], out_len int32[B], status int32[B]); per-stream failures are statuses."""
        return self._inflate(False, d_in, in_off, in_len, nblocks, out_pitch, flags, obsize, out, work)

    # -- STARTD for a batch, verified: zlib header, Adler-32 trailer, bytes consumed
    @_on_device
    def inflate_checked(self, d_in, in_off=None, in_len=None, nblocks=None, out_pitch=None, flags=0, obsize=0,
                        out=None, work=None):
        """inflate_batch through hdlz_inflate_checked: the same decode, then every stream is judged -- E_BAD_HEADER, E_BAD_CHECKSUM, or
        E_NO_EOF for a cut trailer, with out_len 0 -- and reports the bytes it consumed (zlib's len - len(unused_data)) and the Adler-32
        of its output.  `work`: as inflate_batch, sized by hdlz_inflate_checked_work_bytes (the judging pass takes its share off the front).
        -> (out uint8[B, out_pitch], out_len int32[B], status int32[B], in_used int32[B], adler int32[B]: the 32 bits of the checksum)."""
        return self._inflate(True, d_in, in_off, in_len, nblocks, out_pitch, flags, obsize, out, work)

    def _inflate(self, checked, d_in, in_off, in_len, nblocks, out_pitch, flags, obsize, out, work):
        """inflate_batch (hdlz_inflate_batch_ws) / inflate_checked (hdlz_inflate_checked: two more result words per stream)"""
        call, sizer = ("hdlz_inflate_checked", "hdlz_inflate_checked_work_bytes") if checked else ("hdlz_inflate_batch_ws", "hdlz_inflate_work_bytes")
        off_ptr, pitch, ilen, nb = self._prep(d_in, in_off, in_len, nblocks)
        assert out_pitch is not None and out_pitch % 4 == 0
        res = self._results(out, (nb, out_pitch), nb, d_in.device, checked)
        need = getattr(self.lib, sizer)(nb, ilen, out_pitch, flags, 0 if in_off is None else 1) if work is None else 0      # (a caller's: as it is)
        work, wptr, wbytes = self._scratch(need, work, torch.uint8)
        rc = getattr(self.lib, call)(d_in.data_ptr(), off_ptr, pitch, ilen, nb, flags, obsize, res[0].data_ptr(), out_pitch,
                                     *[t.data_ptr() for t in res[1:]], wptr, wbytes, self._stream())
        self._check(rc, call)
        return res

    # -- gzip members of any writer, one per stream (include/hdlz_gunzip.h)
    @_on_device
    def inflate_gzip(self, d_in, in_off=None, in_len=None, nblocks=None, out_pitch=None, out=None, work=None):
        """d_in: as inflate_batch -- uint8 [B, pitch] or flat uint8 with in_off int64[B + 1] (then `in_len` is the bound on the lengths).
        Every stream is ONE gzip member of any writer (FEXTRA, FNAME, FCOMMENT, FHCRC) followed by anything: the header is walked, the
        payload decoded, CRC-32 and ISIZE verified on the device (hdlz_gunzip_ws; one stream per call: the whole-GPU decode).
        -> (out uint8[B, out_pitch], out_len int32[B], status int32[B], in_used int32[B], crc int32[B]: the 32 bits of the checksum);
        in_used is where the member ended -- the next member of a file starts there.  Per-stream failures are statuses.  `work`: the
        call's scratch, a uint8 device tensor of at least hdlz_gunzip_work_bytes(...) bytes at a multiple of 256 (default: allocated here)."""
        off_ptr, pitch, ilen, nb = self._prep(d_in, in_off, in_len, nblocks)
        assert out_pitch is not None and out_pitch % 4 == 0
        res = self._results(out, (nb, out_pitch), nb, d_in.device, True)
        need = self.lib.hdlz_gunzip_work_bytes(nb, ilen, out_pitch, 0 if in_off is None else 1)
        work, wptr, wbytes = self._scratch(need, work, torch.uint8, full=True)
        rc = self.lib.hdlz_gunzip_ws(d_in.data_ptr(), off_ptr, pitch, ilen, nb, res[0].data_ptr(), out_pitch,
                                     *[t.data_ptr() for t in res[1:]], wptr, wbytes, self._stream())
        self._check(rc, "hdlz_gunzip_ws")
        return res

    @_on_device
    def inflate_gzip_bytes(self, z, out_cap=None):
        """the bytes of a .gz file -> (status, bytes), with gzip.decompress's acceptance: one or more members back to back, zero bytes
        behind a member ignored, anything else behind a member E_BAD_HEADER, empty input (OK, b"").  z is staged once; every
        member is one device call (inflate_gzip with one stream) and one host sync, the next one starts at in_used.  Capacity of a
        call: out_cap when given; else the ISIZE word at the end of the remaining bytes when it does not exceed inflate_cap(remaining),
        and once more with inflate_cap(remaining) after E_OUT_CAPACITY."""
        n, pos, pieces = len(z), 0, []
        d = self._stage(z)[:n]
        tail_isize = int.from_bytes(bytes(z[n - 4:n]), "little") if n >= 4 else 0
        while pos < n:
            if pieces:                               # zero bytes behind a member are padding
                pos = n - len(bytes(z[pos:]).lstrip(b"\0"))
                if pos == n:
                    break
            st, out, used = self._gzip_one(d, pos, tail_isize, out_cap)
            if st != OK:
                return _gzip_tail_status(st, bool(pieces), n - pos, lambda: bytes(z[pos:pos + 3])), b""
            pieces.append(bytes(out.cpu().numpy().tobytes()))
            pos += used
        return OK, b"".join(pieces)

    # -- gzip files of many members: found, decoded and verified in one pass (include/hdlz_gzip_members.h)
    # read_gzip: spans from here on take the one-stream route.  ONE member costs its wave about 0.18 us a compressed byte and the
    # one-stream route 0.6 to 0.8 ms up to 512 KiB (profiles/gzip_members.txt, section 4): alone, a member is faster there from
    # between 4 and 7.5 KiB on.  But the waves of a file run side by side and the one-stream calls one behind the other, three
    # host syncs each, so M members of S bytes are faster by waves while S is below M times that span.  The default is the
    # smallest power of two above BGZF's largest member (64 KiB), so that blocked files never leave the wave route: there a
    # wave (23 ms) costs some 33 one-stream calls.
    GZIP_BIG_MEMBER = 1 << 17

    @_on_device
    def gzip_index(self, d_file, member_cap=None):
        """d_file: flat uint8 device tensor, a gzip file of any number of members -> (member_offsets int64[M + 1], out_offsets
        int64[M + 1], record): the GUESS of hdlz_gzip_members_index_ws -- every position that looks like a member header (and position
        0) starts a member, and the word in front of the next one is taken for its ISIZE.  The read verifies it (inflate_gzip_members).
        The record is a _lib.GzipMembersIndexResult (nmembers, total_out, status).  One host sync for the record.  member_cap: room for
        that many members (default: a guess, file_len // 4096 + 16); when the file holds more, the call is made once more with the
        true count."""
        return self._member_index("hdlz_gzip_members_index_ws", _lib.GzipMembersIndexResult, self.lib.hdlz_gzip_members_index_work_bytes, d_file, member_cap)

    def _gzip_members_call(self, d_file, off, out_off, B, out, out_cap, status, work=None):
        """one hdlz_gzip_members_inflate_ws, enqueued: no host read -> the record's device tensor"""
        return self._enqueue("hdlz_gzip_members_inflate_ws", _lib.GzipMembersInflateResult,
                             self._scratch(self.lib.hdlz_gzip_members_inflate_work_bytes(B), work, torch.uint8),
                             d_file.data_ptr() if d_file.numel() else None, d_file.numel(), off.data_ptr(), out_off.data_ptr(), B,
                             out.data_ptr() if out_cap else None, out_cap, status.data_ptr() if B else None)

    @_on_device
    def inflate_gzip_members(self, d_file, index=None, members=None, out=None, work=None):
        """the raw verified read of hdlz_gzip_members_inflate_ws: d_file as in gzip_index, index: its (member_offsets, out_offsets)
        (default: taken here), members=(b0, b1): only those -> (out uint8[total], member_status int32[B], record): member b's bytes
        are out[out_offsets[b] - out_offsets[b0] : out_offsets[b + 1] - out_offsets[b0]] where member_status[b] is OK; every other
        member is one the guess got wrong or the file has damaged -- no repair here, and nothing is raised on a member's status
        (read_gzip repairs).  The record is a _lib.GzipMembersInflateResult (out_len, first_bad, status).  `work`: the call's scratch,
        a uint8 device tensor of at least hdlz_gzip_members_inflate_work_bytes(b1 - b0) bytes at a multiple of 256."""
        self._is_bytes(d_file, "d_file", flat=True)
        off, out_off, B, total, out = self._member_range(*(self.gzip_index(d_file)[:2] if index is None else (index[0], index[1])), members, out)
        status = torch.empty(B, dtype=torch.int32, device=d_file.device)
        result = self._gzip_members_call(d_file, off, out_off, B, out, total, status, work)
        return out[:total], status, _lib.GzipMembersInflateResult.from_buffer_copy(result.cpu().numpy().tobytes())

    def _gzip_one(self, d_file, pos, tail_isize, out_cap=None):
        """gzip's acceptance of ONE member at `pos`, for both walkers (inflate_gzip_bytes, read_gzip): the one-stream call (a large member:
        the whole GPU).  Capacity: out_cap when given; else the ISIZE word at the file's end (tail_isize) when it does not exceed
        inflate_cap(remaining), and once more with inflate_cap(remaining) after E_OUT_CAPACITY
        -> (status, the member's bytes on the device, bytes consumed)"""
        rest = d_file.numel() - pos
        bound = inflate_cap(rest)
        isize = tail_isize if rest >= 4 else bound
        for cap in ([out_cap] if out_cap is not None else [isize, bound] if isize < bound else [bound]):
            out, ol, st, used, _ = self.inflate_gzip(d_file[pos:pos + rest], in_len=rest, nblocks=1, out_pitch=max(16, (cap + 15) // 16 * 16))
            st = int(st.item())
            if st != E_OUT_CAPACITY:
                break
        return (st, None, 0) if st != OK else (st, out[0, :int(ol.item())], int(used.item()))

    @_on_device
    def read_gzip(self, d_file, big_member=None):
        """d_file: flat uint8 device tensor, a .gz file of any number of members of any writer -> (out uint8[n] on the device, report),
        with inflate_gzip_bytes's acceptance (gzip.decompress's: members back to back, zero bytes behind a member ignored, anything
        else E_BAD_HEADER) but the members found and decoded in parallel: one gzip_index call, the verified read of every run of
        spans below `big_member` compressed bytes (default GZIP_BIG_MEMBER) enqueued without a sync in between, one D2H of the
        statuses (and one of the index's two arrays, which the walk below bisects).  Verified members are taken from where they lie.  Where the walk meets a member that did not verify -- a look-alike
        header split it, padding stands behind it, it is damaged -- or a span of big_member bytes and more, ONE iteration of
        inflate_gzip_bytes's loop runs there (the one-stream inflate_gzip call, then the skip of zero bytes) and the walk resumes at
        the candidate that stands where it ended; where none stands there the same call is made anyway and its answer is the file's.
        report: .status (OK: out is the data; else out is empty), .members (delivered), .candidates (of the index), .repairs and .big
        (one-stream calls of either kind), .member_status (numpy int32[candidates]; -1: not sent to the verified read)."""
        import bisect
        import types
        import numpy as np
        self._is_bytes(d_file, "d_file", flat=True)
        n, dev = d_file.numel(), d_file.device
        big_member = self.GZIP_BIG_MEMBER if big_member is None else int(big_member)
        off, out_off, rec = self.gzip_index(d_file)
        M = int(rec.nmembers)
        h_off, h_out = off.cpu().tolist(), out_off.cpu().tolist()
        is_big = [h_off[b + 1] - h_off[b] >= big_member for b in range(M)]
        status = torch.full((M,), -1, dtype=torch.int32, device=dev)
        runs, b = {}, 0                                   # first member of a run -> (its last + 1, its output)
        while b < M:
            if is_big[b]:
                b += 1
                continue
            e = b
            while e < M and not is_big[e]:
                e += 1
            total = h_out[e] - h_out[b]
            out = torch.empty(total, dtype=torch.uint8, device=dev)
            self._gzip_members_call(d_file, off[b:e + 1], out_off[b:e + 1], e - b, out, total, status[b:e])
            for k in range(b, e):
                runs[k] = (b, out)
            b = e
        h_status = status.cpu().numpy()                   # the one D2H of the statuses
        report = types.SimpleNamespace(status=OK, members=0, candidates=M, repairs=0, big=0, member_status=h_status)
        tail_isize = int.from_bytes(bytes(d_file[n - 4:].cpu().numpy().tobytes()), "little") if n >= 4 else 0
        pieces, pos = [], 0
        while pos < n:
            if report.members:                            # zero bytes behind a member are padding
                while pos < n:
                    nz = torch.nonzero(d_file[pos:pos + (1 << 20)])
                    if nz.numel():
                        pos += int(nz[0].item())
                        break
                    pos = min(n, pos + (1 << 20))
                if pos == n:
                    break
            b = bisect.bisect_left(h_off, pos, 0, M)
            b = b if b < M and h_off[b] == pos else None
            if b is not None and h_status[b] == OK:
                e = b
                while e < M and h_status[e] == OK:
                    e += 1
                b0, out = runs[b]
                pieces.append(out[h_out[b] - h_out[b0]:h_out[e] - h_out[b0]])
                report.members += e - b
                pos = h_off[e]
                continue
            st, out, used = self._gzip_one(d_file, pos, tail_isize)
            if b is not None and is_big[b]:
                report.big += 1
            else:
                report.repairs += 1
            if st != OK:
                report.status = _gzip_tail_status(st, report.members > 0, n - pos, lambda: bytes(d_file[pos:pos + 3].cpu().numpy().tobytes()))
                return torch.empty(0, dtype=torch.uint8, device=dev), report
            pieces.append(out)
            report.members += 1
            pos += used
        if len(pieces) == 1:
            return pieces[0], report
        return (torch.cat(pieces) if pieces else torch.empty(0, dtype=torch.uint8, device=dev)), report

    def read_gzip_bytes(self, z, big_member=None):
        """the bytes of a .gz file -> (status, bytes): what inflate_gzip_bytes answers wherever that is not E_OUT_CAPACITY, through
        read_gzip -- a launch chain for the whole file, not one per member"""
        d = self._stage(z)[:len(z)]
        out, report = self.read_gzip(d, big_member=big_member)
        return report.status, bytes(out.cpu().numpy().tobytes()) if report.status == OK else b""

    # -- archive compaction
    @_on_device
    def compact(self, rows, lens, offsets=None, archive=None):
        """rows uint8[B, pitch], lens int32[B] -> (archive uint8[total], offsets int64[B]).
        `offsets` (exclusive scan, e.g. global offsets after the multi-GPU length all-gather) and `archive`
        may be supplied; otherwise they are computed / allocated here (one host sync for the size)."""
        assert rows.is_cuda and rows.dtype == torch.uint8 and rows.dim() == 2 and rows.is_contiguous()
        assert rows.device == self.device and lens.is_cuda and lens.dtype == torch.int32 and lens.numel() == rows.shape[0]
        B, pitch = rows.shape
        lens = lens.contiguous()
        if offsets is None:
            l64 = lens.to(torch.int64)
            offsets = torch.cumsum(l64, 0) - l64
        assert offsets.is_cuda and offsets.dtype == torch.int64 and offsets.numel() == B, "offsets must be int64 [B] on the GPU"
        offsets = offsets.contiguous()
        if archive is None:
            total = int((offsets[-1] + lens[-1]).item()) if B else 0
            archive = torch.empty(total, dtype=torch.uint8, device=rows.device)
        rc = self.lib.hdlz_compact_batch(rows.data_ptr(), pitch, lens.data_ptr(), offsets.data_ptr(), B,
                                         archive.data_ptr(), self._stream())
        self._check(rc, "hdlz_compact_batch")
        return archive, offsets

    @_on_device
    def archive(self, rows, lens, archive=None, offsets=None, work=None):
        """rows uint8[B, pitch], lens int32[B] -> (archive uint8[cap], offsets int64[B + 1]) in ONE launch (hdlz_archive_batch): the
        exclusive scan of the lengths is made on the device, offsets[B] is the archive's length (no host sync: read it when needed),
        offsets is directly the `in_off` of a ragged inflate / compress call.  `archive` defaults to a buffer of B * pitch bytes."""
        assert rows.is_cuda and rows.dtype == torch.uint8 and rows.dim() == 2 and rows.is_contiguous() and rows.device == self.device
        assert lens.is_cuda and lens.dtype == torch.int32 and lens.numel() == rows.shape[0]
        B, pitch = rows.shape
        lens = lens.contiguous()
        if archive is None:
            archive = torch.empty(B * pitch, dtype=torch.uint8, device=rows.device)
        if offsets is None:
            offsets = torch.empty(B + 1, dtype=torch.int64, device=rows.device)
        self._is_bytes(archive, "archive")
        _is_index(offsets, B + 1)
        # the call's scratch (8 bytes per 256 rows), caller-owned like every other buffer of the call
        work, wptr, wbytes = self._scratch(self.lib.hdlz_archive_work_bytes(B), work)
        rc = self.lib.hdlz_archive_batch_ws(rows.data_ptr(), pitch, lens.data_ptr(), B, archive.data_ptr(), archive.numel(),
                                            offsets.data_ptr(), wptr, wbytes, self._stream())
        self._check(rc, "hdlz_archive_batch_ws")
        return archive, offsets

    # -- the job from HOST buffers: the PCIe hops overlapped with the kernels
    @_on_device
    def compress_host(self, h_in, cwindow=32, maxmatch=10, chunk_blocks=None, h_archive=None, h_len=None, keep_buffers=True):
        """h_in: PINNED host uint8 [B, n].  Compresses every block on the GPU and returns (h_archive, h_len, total, status_bad):
        the blocks' zlib streams back to back in pinned host memory (`h_archive[:total]`; block b at the exclusive scan of
        `h_len`), their lengths, and the number of blocks whose status is not OK (0 unless n < 5 / the capacity is wrong).
        The batch goes through the GPU in chunks of `chunk_blocks` blocks on three streams -- H2D of chunk k + 1, compress +
        hdlz_archive_batch (scan + gather) of chunk k, D2H of chunk k - 1's ARCHIVE (not its pitched rows) -- so the job costs about
        the slower PCIe direction instead of H2D + kernel + D2H.  One host sync per chunk (its archive size).
        The three side streams and the staging buffers are kept on the Engine between calls (`keep_buffers=False` or
        release_host_buffers() drops them); compress_host / inflate_host of ONE Engine must not run from two threads at once."""
        return host.compress_host(self, h_in, cwindow, maxmatch, chunk_blocks, h_archive, h_len, keep_buffers)

    def release_host_buffers(self):
        """drop the streams and the device / pinned staging buffers compress_host and inflate_host keep between calls (about
        2 C n + 3 C pitch bytes of HBM for chunks of C blocks: ~250 MB at the default 48 MiB chunk) and give the library's cached
        scratch back to the device"""
        self._host_ctx = self._ihost_ctx = None
        with torch.cuda.device(self.device):
            self._check(self.lib.hdlz_release_scratch(), "hdlz_release_scratch")

    @_on_device
    def inflate_host(self, h_z, h_off, out_pitch, flags=0, obsize=0, chunk_streams=None, h_out=None, h_len=None, h_status=None,
                     keep_buffers=True, d2h="copy"):
        """STARTD for a batch held in HOST memory: h_z PINNED flat uint8 (the zlib streams back to back), h_off int64 [B + 1] on the
        host (ascending; stream b = h_z[h_off[b]:h_off[b + 1]]).  Returns pinned (h_out uint8 [B, out_pitch], h_len int32 [B],
        h_status int32 [B]).  Chunks of `chunk_streams` streams (the first one a quarter of that: the pipeline fills sooner) on three
        streams, nothing but enqueues on the host -- no synchronisation before the end: H2D of chunk k + 1 | hdlz_inflate_batch of
        chunk k | D2H of chunk k - 1's rows in copies of at most 32 MiB (larger hipMemcpyAsync D2H copies were seen to block the host
        on ROCm 7.2).  Measured on BASELINE configs[3] (profiles/r04_inflate_host.txt): 42.5 ms against 37.7 ms for the rows alone at
        the link's 57 GB/s (round 3: 51.9 ms -- it waited on the host for a chunk's kernel before issuing its D2H, and its 48 MiB
        chunks ran the inflate kernel 43 times at the ~0.6 ms a lane-per-stream launch costs whatever its size).  What is left above the
        floor: a kernel that runs BESIDE a D2H -- the runtime's blit or a kernel of ours storing into the mapped rows, d2h="kernel" --
        completes only when the D2H's writes have drained (0.63 -> 3.1 ms in the kernel trace; its end-of-kernel write-back queues
        behind the PCIe-bound stores), so inflate and D2H alternate per chunk pair instead of overlapping freely.
        Buffers and streams are kept on the Engine between calls (see compress_host); one call at a time per Engine."""
        return host.inflate_host(self, h_z, h_off, out_pitch, flags, obsize, chunk_streams, h_out, h_len, h_status, keep_buffers, d2h)

    # -- streaming sessions (hdlz_compress_chunk / hdlz_inflate_chunk): the port adapter's streaming mode
    def compress_session(self, cwindow=32, maxmatch=10):
        return CompressSession(self, cwindow, maxmatch)

    def inflate_session(self, flags=0, obsize=0):
        return InflateSession(self, flags, obsize)

    # -- single-stream conveniences used by the port adapter (one START = one block)
    @_on_device
    def compress_bytes(self, data, cwindow=32, maxmatch=10, block=None, container="zlib"):
        """-> (status, bytes).  block=None: ONE block, what STARTC writes; a number: the input in blocks of that many bytes, joined into
        one standard zlib stream (compress_joined) or, with container="gzip", into one gzip member"""
        if _container_is_gzip(container) and block is None:
            raise ValueError("container=\"gzip\" is the joined stream's: give block=")
        if block is not None:
            if len(data) < 5:
                return E_SHORT_INPUT, b""
            try:
                z, _ = self.compress_joined(self._stage(data)[:len(data)], block=block, cwindow=cwindow, maxmatch=maxmatch, container=container)
            except HdlzStatusError as e:
                return e.status, b""
            return OK, bytes(z.cpu().numpy().tobytes())
        out, ol, st = self._compress_one(self._stage(data), len(data), cwindow, maxmatch)
        return int(st.item()), bytes(out[:int(ol.item())].cpu().numpy().tobytes())

    @_on_device
    def inflate_bytes(self, z, out_cap=None, flags=0, obsize=0, verify=False, members=None, container="zlib"):
        """-> (status, bytes); verify=True: through the checked call (header, Adler-32, trailer present).  Default capacity: deflate expands at most 1032:1 (a 258-byte match costs 2 bits), so
        1032 n + 258 bytes hold any stream, capped at the reference's 2^LMAX counter range (deflate.py:73-76).
        members=(offsets, block): z is a joined stream (compress_joined / compress_bytes(block=...)) with its member index -- a
        sequence or tensor of B + 1 offsets -- and the block size it was cut with: every member is decoded in parallel and the stream
        verified (inflate_joined).  The length of the data is not part of a stream: it is taken from out_cap when given, else the last
        two members are decoded once more as one short stream to measure them.  container="gzip" (with members=): z is the gzip form;
        without out_cap the length is the trailer's ISIZE, the length mod 2^32 -- exact for data below 4 GiB.  The word is read before
        the stream is verified: an ISIZE that the index cannot belong to, or that makes the decode fail where the measured length
        would not, answers E_BAD_CHECKSUM."""
        from .chain import plan_blocks
        gz = _container_is_gzip(container)
        if gz and members is None:
            raise ValueError("container=\"gzip\" is the joined stream's: give members=")
        if members is not None:
            offsets, block = members
            offs = [int(o) for o in (offsets.tolist() if torch.is_tensor(offsets) else offsets)]
            B = len(offs) - 1
            total = out_cap

            def measured():
                """-> (status, length of the data): the last two members decoded once more as one short stream"""
                k = max(B - 2, 0)                                # members 0 .. k - 1 hold `block` bytes each (chain.plan_blocks)
                st, tail = self.inflate_bytes(z[offs[k] - 2:], out_cap=2 * block + 16)
                return st, k * block + len(tail)
            from_isize = total is None and gz
            if from_isize:
                end = offs[B]
                if len(z) < end + 10:
                    return E_NO_EOF, b""
                # ISIZE is read before anything is verified: a length the index cannot belong to is a damaged trailer
                total = int.from_bytes(bytes(z[end + 6:end + 10]), "little")
                try:
                    fits = len(plan_blocks(total, block)) == B if B else total == 0
                except Error:
                    fits = False
                if not fits:
                    return E_BAD_CHECKSUM, b""
            elif total is None and B:
                st, total = measured()
                if st != OK:
                    return st, b""
            try:
                out = self.inflate_joined(self._stage(z)[:len(z)], torch.tensor(offs, dtype=torch.int64).to(self.device), block=block,
                                          total=total or 0, flags=flags, container=container)
            except HdlzStatusError as e:
                if from_isize and B:                             # the members' slots came from ISIZE: was it the word that was wrong?
                    st, true_total = measured()
                    if st == OK and true_total != total:
                        return E_BAD_CHECKSUM, b""
                return e.status, b""
            return OK, bytes(out.cpu().numpy().tobytes())
        n = len(z)
        d = self._stage(z).view(1, -1)
        cap = out_cap if out_cap is not None else inflate_cap(n)
        cap = (cap + 15) // 16 * 16
        if n >= 5 and (z[2] & 7) == 3:           # the bytes are here: BFINAL = 1, BTYPE = 01 -- a single fixed block takes that chain only
            flags |= INFLATE_ONE_FIXED_BLOCK
        out, ol, st = self._inflate(verify, d, None, n, None, cap, flags, obsize, None, None)[:3]
        st = int(st.item())
        return st, bytes(out[0, :int(ol.item())].cpu().numpy().tobytes())
