"""hdl_deflate_amd -- MI355X-native deflate engine behind the HDL-deflate command surface.

Only the hot path of tomtor/HDL-deflate is here: STARTC (fixed-Huffman LZ77 compress) and STARTD
(inflate) as hand-written HIP kernels for gfx950 (csrc/, built into lib/libhdlz.so, C-ABI in
include/hdlz.h), plus the host-side mirror of the reference's port interface (port.py).
There is NO CPU fallback: every compute entry point raises if the HIP library or a GPU is missing.
"""
from .errors import Error, HdlzStatusError, HdlzRangeError                         # noqa: F401
from .constants import (IDLE, WRITE, READ, STARTC, STARTD, OK, E_SHORT_INPUT, E_OUT_CAPACITY,   # noqa: F401
                        E_BAD_BTYPE, E_BAD_DISTANCE, E_NO_EOF, E_DYNAMIC_UNSUPPORTED, E_BAD_SYMBOL,
                        E_BAD_PARAM, E_HIP, E_BAD_TREE, E_BAD_HEADER, E_BAD_CHECKSUM, INFLATE_ASSUME_FIXED, INFLATE_LANE_PER_STREAM, INFLATE_WAVE_PER_STREAM, INFLATE_GROUP_PER_STREAM, INFLATE_ONEBLOCK, INFLATE_ONE_FIXED_BLOCK,
                        STATUS_NAMES, out_bound)
from .port import Sig, DeflatePort, deflate                         # noqa: F401
from . import bgzf                                                  # noqa: F401  (host-only: virtual offsets, .gzi files)
from .bgzf import virtual_offset, split_virtual, gzi_dumps, gzi_loads   # noqa: F401
from .zip import ZipIndex                                           # noqa: F401  (what Engine.zip_index returns)
from .seek import SeekIndex                                         # noqa: F401  (what Engine.seek_index returns; seek.loads reads its file)
from . import seek                                                  # noqa: F401
from .png import load_png, save_png, PngIndex                       # noqa: F401  (PNG files into device tensors, and back)
from .tiff import load_tiff, TiffIndex                              # noqa: F401  (TIFF files into device tensors)
from .npz import load_npz, save_npz                                 # noqa: F401  (.npz files into device tensors, and back)


def join_bound(nblocks, in_len):
    """bytes that hold the joined stream of nblocks blocks of at most in_len bytes (same as hdlz_join_bound)"""
    return 8 + nblocks * (out_bound(in_len) - 1)


def unjoin_work_bytes(nmembers, total_out, flags=0):
    """the scratch hdlz_unjoin_ws asks for (hdlz_unjoin_work_bytes: host arithmetic of the library)"""
    from . import _lib
    return _lib.load().hdlz_unjoin_work_bytes(nmembers, total_out, flags)


def gunzip_work_bytes(nstreams, in_len, out_pitch, ragged=False):
    """the scratch hdlz_gunzip_ws asks for (hdlz_gunzip_work_bytes: host arithmetic of the library) -- Engine.inflate_gzip's `work`"""
    from . import _lib
    return _lib.load().hdlz_gunzip_work_bytes(nstreams, in_len, out_pitch, 1 if ragged else 0)


def gzip_members_index_work_bytes(file_len):
    """the scratch hdlz_gzip_members_index_ws asks for (hdlz_gzip_members_index_work_bytes: host arithmetic of the library)"""
    from . import _lib
    return _lib.load().hdlz_gzip_members_index_work_bytes(file_len)


def gzip_members_inflate_work_bytes(nmembers):
    """the scratch hdlz_gzip_members_inflate_ws asks for (hdlz_gzip_members_inflate_work_bytes) -- Engine.inflate_gzip_members's `work`"""
    from . import _lib
    return _lib.load().hdlz_gzip_members_inflate_work_bytes(nmembers)


def Engine(*a, **kw):
    """The HIP batch engine (imports torch lazily)."""
    from .engine import Engine as _E
    return _E(*a, **kw)
