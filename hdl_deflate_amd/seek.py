"""The seek index of a gzip or zlib stream (include/hdlz_seek.h): what Engine.seek_index returns and Engine.read_seek reads through,
and its file format.  Host-only: the tensors may live on any device, dumps() copies them to the host.

THE FILE, little-endian, no padding:
    0    8 bytes   magic  b"HDLZSEEK"
    8    u32       version (1)
    12   u32       container: 1 = zlib, 2 = gzip (HDLZ_SEEK_ZLIB / HDLZ_SEEK_GZIP)
    16   u64       span
    24   u64       file_len, the length of the compressed file the index belongs to
    32   u64       n, the number of points (at least 1)
    40   u64       max_seg, the largest pos[k + 1] - pos[k]
    48             bit[n + 1]  u64  (bit[n] is end_bit)
    ...            pos[n + 1]  u64  (pos[n] is the length of the data)
    ...            crc[n]      u32
    ...            win[n][32768] bytes
so a file of n points holds 48 + 16 (n + 1) + 4 n + 32768 n bytes.  loads() refuses whatever is not one: a wrong magic or version, a
length that does not match the count, positions that do not ascend, a bit behind the file's end, a max_seg that is not the largest
segment."""
import struct

import numpy as np

MAGIC = b"HDLZSEEK"
VERSION = 1
WINDOW = 32768
HEADER = struct.Struct("<8sIIQQQQ")
CONTAINERS = {"zlib": 1, "gzip": 2}


def file_bytes(n):
    """the length of the file of an index of n points"""
    return HEADER.size + 16 * (n + 1) + 4 * n + WINDOW * n


class SeekIndex(object):
    """bit int64[n + 1], pos int64[n + 1], crc int32[n], win uint8[n, 32768] (the words are unsigned; torch has no such types), and
    span, file_len, container ("zlib" or "gzip").  total, end_bit and max_seg are host integers."""

    def __init__(self, bit, pos, crc, win, span, file_len, total, end_bit, max_seg, container):
        if container not in CONTAINERS:
            raise ValueError("container must be \"zlib\" or \"gzip\", not %r" % (container,))
        import torch
        n = crc.numel()
        assert n >= 1 and bit.numel() == n + 1 and pos.numel() == n + 1 and tuple(win.shape) == (n, WINDOW)
        assert bit.dtype == torch.int64 and pos.dtype == torch.int64 and crc.dtype == torch.int32 and win.dtype == torch.uint8
        self.bit, self.pos, self.crc, self.win = bit, pos, crc, win
        self.span, self.file_len, self.total, self.end_bit, self.max_seg = int(span), int(file_len), int(total), int(end_bit), int(max_seg)
        self.container = container

    @property
    def npoints(self):
        return self.crc.numel()

    def to(self, device):
        return SeekIndex(self.bit.to(device), self.pos.to(device), self.crc.to(device), self.win.to(device), self.span, self.file_len,
                         self.total, self.end_bit, self.max_seg, self.container)

    def dumps(self):
        """-> the bytes of the file stated above"""
        parts = [HEADER.pack(MAGIC, VERSION, CONTAINERS[self.container], self.span, self.file_len, self.npoints, self.max_seg)]
        for t, dt in ((self.bit, "<i8"), (self.pos, "<i8"), (self.crc, "<i4"), (self.win, "u1")):
            parts.append(t.detach().cpu().contiguous().numpy().astype(dt, copy=False).tobytes())
        return b"".join(parts)


def loads(b, device=None):
    """the bytes of an index file (SeekIndex.dumps) -> a SeekIndex on `device` (default: the host).  ValueError for anything else."""
    import torch
    b = bytes(b)
    if len(b) < HEADER.size:
        raise ValueError("truncated seek index: no header")
    magic, version, container, span, file_len, n, max_seg = HEADER.unpack_from(b, 0)
    if magic != MAGIC:
        raise ValueError("not a seek index: bad magic")
    if version != VERSION:
        raise ValueError("seek index: version %d, this module reads %d" % (version, VERSION))
    names = {v: k for k, v in CONTAINERS.items()}
    if container not in names:
        raise ValueError("seek index: unknown container %d" % container)
    if span < 1 or n < 1 or n >= 1 << 31:
        raise ValueError("seek index: span %d, %d points" % (span, n))
    if len(b) != file_bytes(n):
        raise ValueError("%sseek index: %d points announced, %d bytes where %d belong" % ("truncated " if len(b) < file_bytes(n) else "", n, len(b), file_bytes(n)))
    at = HEADER.size
    bit = np.frombuffer(b, "<u8", n + 1, at); at += 8 * (n + 1)
    pos = np.frombuffer(b, "<u8", n + 1, at); at += 8 * (n + 1)
    crc = np.frombuffer(b, "<u4", n, at); at += 4 * n
    win = np.frombuffer(b, "u1", WINDOW * n, at).reshape(n, WINDOW)
    if pos[0] != 0 or (n > 1 and not (np.all(pos[1:n] > pos[:n - 1]) and pos[n] >= pos[n - 1])) or pos[n] < pos[n - 1]:
        raise ValueError("seek index: the output offsets do not ascend from 0")
    if not np.all(bit[1:] > bit[:-1]) or int(bit[n]) > 8 * file_len:
        raise ValueError("seek index: the bit positions do not ascend inside the file")
    if int(np.max(pos[1:] - pos[:-1])) != max_seg:
        raise ValueError("seek index: max_seg is not the largest segment")
    t = [torch.from_numpy(a.astype(dt)) for a, dt in ((bit.view("<i8"), np.int64), (pos.view("<i8"), np.int64), (crc.view("<i4"), np.int32), (win, np.uint8))]
    idx = SeekIndex(t[0], t[1], t[2], t[3], span, file_len, int(pos[n]), int(bit[n]), max_seg, names[container])
    return idx if device is None else idx.to(device)
