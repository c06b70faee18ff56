"""Host-side pieces of BGZF random access (include/hdlz_bgzf_range.h): virtual offsets, and the .gzi index file.  Plain Python, no torch,
no device: what makes the device's member index usable by other tools, and theirs by Engine.read_bgzf."""
import struct

COFFSET_MAX = (1 << 48) - 1
UOFFSET_MAX = (1 << 16) - 1


def virtual_offset(coffset, uoffset):
    """coffset << 16 | uoffset: the file offset of a member's first byte and a byte position inside that member's data -- what a .bai,
    .tbi or .csi index stores.  coffset must be in [0, 2^48), uoffset in [0, 65536).  (The value fits a signed 64-bit word for
    files below 2^47 bytes.)"""
    coffset, uoffset = int(coffset), int(uoffset)
    if not 0 <= coffset <= COFFSET_MAX:
        raise ValueError("coffset %d is not in [0, 2^48)" % coffset)
    if not 0 <= uoffset <= UOFFSET_MAX:
        raise ValueError("uoffset %d is not in [0, 65536)" % uoffset)
    return coffset << 16 | uoffset


def split_virtual(v):
    """a virtual offset in [0, 2^64) -> (coffset, uoffset)"""
    v = int(v)
    if not 0 <= v < 1 << 64:
        raise ValueError("virtual offset %d is not in [0, 2^64)" % v)
    return v >> 16, v & UOFFSET_MAX


def gzi_dumps(member_offsets, out_offsets):
    """the member index of a BGZF file (Engine.bgzf_index, on the host: M + 1 ascending values each) -> the bytes of its .gzi file:
    a little-endian uint64 count n, then n pairs of little-endian uint64 (compressed offset, uncompressed offset) -- one pair for
    every member EXCEPT MEMBER 0 that holds at least one byte, ascending; so the closing EOF member has no entry.
    This is the index that htslib's bgzip -i writes on the fly, as the maintainers of this project read its format; no htslib
    was at hand to check a file against, and tests/test_bgzf_range_cabi.py pins the layout stated here."""
    off, out = [int(x) for x in member_offsets], [int(x) for x in out_offsets]
    if len(off) != len(out) or not off:
        raise ValueError("member_offsets and out_offsets hold M + 1 values each")
    pairs = [(off[b], out[b]) for b in range(1, len(off) - 1) if out[b + 1] > out[b]]
    return struct.pack("<Q", len(pairs)) + b"".join(struct.pack("<QQ", c, u) for c, u in pairs)


def gzi_loads(b):
    """the bytes of a .gzi file (gzi_dumps) -> (coffsets, uoffsets), two lists of n values.  ValueError for truncated input, a count
    that does not match the length, and entries that do not ascend.  (With the pair (0, 0) in front and the file's last member and
    the data's length behind, the lists are an index that Engine.read_bgzf takes: members without data change no position.)"""
    b = bytes(b)
    if len(b) < 8:
        raise ValueError("truncated .gzi: no count")
    (n,) = struct.unpack_from("<Q", b, 0)
    if len(b) < 8 + 16 * n:
        raise ValueError("truncated .gzi: %d entries announced, %d bytes behind the count" % (n, len(b) - 8))
    if len(b) != 8 + 16 * n:
        raise ValueError(".gzi: %d entries announced, %d bytes behind the count" % (n, len(b) - 8))
    words = struct.unpack_from("<%dQ" % (2 * n), b, 8)
    coffsets, uoffsets = list(words[0::2]), list(words[1::2])
    for k in range(n):                      # every listed member holds data, so both columns ascend strictly; entry 0 lies behind member 0
        if (coffsets[k] <= coffsets[k - 1] or uoffsets[k] <= uoffsets[k - 1]) if k else coffsets[0] == 0:
            raise ValueError(".gzi: entry %d does not ascend" % k)
    return coffsets, uoffsets
