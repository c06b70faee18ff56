"""ctypes loader for lib/libhdlz.so (the C-ABI of include/hdlz.h).  Fails loudly: there is no
Python or CPU implementation to fall back to."""
import ctypes
import os
from ctypes import c_char_p as cs, c_int as ci, c_size_t as sz, c_uint32 as u32, c_uint64 as u64, c_void_p as vp

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HDLZ_LIB") or os.path.join(_HERE, "lib", "libhdlz.so")   # HDLZ_LIB: A/B builds
_BATCH_IN = [vp, vp, u64, u32, u64]                   # d_in, d_in_off, in_pitch, in_len, nblocks
_INFLATE = _BATCH_IN + [u32, u32, vp, u64, vp, vp]    # ... flags, obsize, d_out, out_pitch, d_out_len, d_status
# name -> (restype, argtypes): every entry point of include/hdlz.h (tests/test_cabi_load.py holds the counts to the header)
SIGNATURES = {
    "hdlz_version": (ci, []),
    "hdlz_status_string": (cs, [ci]),
    "hdlz_last_error": (cs, []),
    "hdlz_device_count": (ci, []),
    "hdlz_out_bound": (sz, [sz]),
    "hdlz_release_scratch": (ci, []),
    "hdlz_compress_batch": (ci, _BATCH_IN + [ci, ci, vp, u64, vp, vp, vp]),
    "hdlz_inflate_work_bytes": (sz, [u64, u32, u64, u32, ci]),
    "hdlz_inflate_batch_ws": (ci, _INFLATE + [vp, sz, vp]),
    "hdlz_inflate_batch": (ci, _INFLATE + [vp]),
    "hdlz_inflate_checked_work_bytes": (sz, [u64, u32, u64, u32, ci]),
    "hdlz_inflate_checked": (ci, _INFLATE + [vp, vp, vp, sz, vp]),
    "hdlz_compact_batch": (ci, [vp, u64, vp, vp, u64, vp, vp]),
    "hdlz_archive_work_bytes": (sz, [u64]),
    "hdlz_archive_batch_ws": (ci, [vp, u64, vp, u64, vp, u64, vp, vp, sz, vp]),
    "hdlz_archive_batch": (ci, [vp, u64, vp, u64, vp, u64, vp, vp]),
    "hdlz_stream_work_bytes": (sz, [sz]),
    "hdlz_streams_work_bytes": (sz, [sz, u64]),
    "hdlz_compress_streams": (ci, [vp, u64, u32, u64, ci, ci, vp, u64, vp, vp, vp, sz, vp]),
    "hdlz_compress_stream": (ci, [vp, u32, ci, ci, vp, u64, vp, vp, vp, sz, vp]),
    "hdlz_compress_chunk": (ci, [vp, u32, u32, ci, ci, ci, vp, u64, vp, vp]),
    "hdlz_inflate_chunk": (ci, [vp, u32, ci, u32, u32, vp, u64, u32, vp, vp]),
}
EXPORTS = tuple(SIGNATURES)
# ... and every entry point of include/hdlz_join.h, the additive extension header (tests/test_joined_cabi.py holds these to that header)
JOIN_SIGNATURES = {
    "hdlz_join_bound": (sz, [u64, u32]),
    "hdlz_join_work_bytes": (sz, [u64]),
    "hdlz_compress_batch_bits": (ci, _BATCH_IN + [ci, ci, vp, u64, vp, vp, vp, vp]),
    # d_rows, row_pitch, d_len, d_end_bits, d_status, d_in_off, in_len, nblocks, d_stream, stream_cap, d_off, d_result, d_work, work_bytes, stream
    "hdlz_join_batch_ws": (ci, [vp, u64, vp, vp, vp, vp, u32, u64, vp, u64, vp, vp, vp, sz, vp]),
}
JOIN_EXPORTS = tuple(JOIN_SIGNATURES)
# ... and of include/hdlz_unjoin.h, the extension of that one (tests/test_unjoin_cabi.py)
UNJOIN_SIGNATURES = {
    "hdlz_unjoin_work_bytes": (sz, [u64, u64, u32]),
    # d_stream, stream_len, d_off, d_out_off, out_len, nmembers, flags, d_out, out_cap, d_member_status, d_result, d_work, work_bytes, stream
    "hdlz_unjoin_ws": (ci, [vp, u64, vp, vp, u32, u64, u32, vp, u64, vp, vp, vp, sz, vp]),
}
UNJOIN_EXPORTS = tuple(UNJOIN_SIGNATURES)
# ... and of include/hdlz_gzip.h: CRC-32 on the device, the joined stream as one gzip member (tests/test_gzip_cabi.py)
GZIP_SIGNATURES = {
    "hdlz_crc32_work_bytes": (sz, [u64]),
    "hdlz_crc32_ws": (ci, [vp, u64, vp, vp, sz, vp]),    # d_data, n, d_crc, d_work, work_bytes, stream
    "hdlz_join_gzip_bound": (sz, [u64, u32]),
    "hdlz_join_gzip_work_bytes": (sz, [u64]),
    # the first eight parameters of hdlz_join_batch_ws, d_crc, d_stream, stream_cap, d_off, d_result, d_work, work_bytes, stream
    "hdlz_join_gzip_ws": (ci, [vp, u64, vp, vp, vp, vp, u32, u64, vp, vp, u64, vp, vp, vp, sz, vp]),
    "hdlz_unjoin_gzip_work_bytes": (sz, [u64, u64, u32]),
    "hdlz_unjoin_gzip_ws": (ci, [vp, u64, vp, vp, u32, u64, u32, vp, u64, vp, vp, vp, sz, vp]),      # as hdlz_unjoin_ws
}
GZIP_EXPORTS = tuple(GZIP_SIGNATURES)
# ... and of include/hdlz_bgzf.h: BGZF, the self-indexing blocked gzip, written and read on the device (tests/test_bgzf_cabi.py)
BGZF_SIGNATURES = {
    "hdlz_crc32_batch_ws": (ci, [vp, vp, u64, u32, u64, vp, vp]),      # d_data, d_off, pitch, len, nblocks, d_crc, stream
    "hdlz_bgzf_bound": (sz, [u64, u32]),
    "hdlz_bgzf_join_work_bytes": (sz, [u64]),
    # d_rows, row_pitch, d_len, d_status, d_in_off, in_len, nblocks, d_crc, d_file, file_cap, d_off, d_result, d_work, work_bytes, stream
    "hdlz_bgzf_join_ws": (ci, [vp, u64, vp, vp, vp, u32, u64, vp, vp, u64, vp, vp, vp, sz, vp]),
    "hdlz_bgzf_index_work_bytes": (sz, [u64]),
    # d_file, file_len, member_cap, d_off, d_out_off, d_result, d_work, work_bytes, stream
    "hdlz_bgzf_index_ws": (ci, [vp, u64, u64, vp, vp, vp, vp, sz, vp]),
    "hdlz_bgzf_inflate_work_bytes": (sz, [u64, u32]),
    # d_file, file_len, d_off, d_out_off, nmembers, flags, d_out, out_cap, d_member_status, d_result, d_work, work_bytes, stream
    "hdlz_bgzf_inflate_ws": (ci, [vp, u64, vp, vp, u64, u32, vp, u64, vp, vp, vp, sz, vp]),
}
BGZF_EXPORTS = tuple(BGZF_SIGNATURES)
# ... and of include/hdlz_bgzf_range.h: batched range reads of a BGZF file by byte or virtual offset (tests/test_bgzf_range_cabi.py)
BGZF_RANGE_SIGNATURES = {
    "hdlz_bgzf_ranges_work_bytes": (sz, [u64, u64, u32]),
    # d_file, file_len, d_off, d_out_off, nmembers, d_ranges, nranges, flags, d_out, out_cap, d_range_off, d_range_status, task_cap,
    # d_result, d_work, work_bytes, stream
    "hdlz_bgzf_read_ranges_ws": (ci, [vp, u64, vp, vp, u64, vp, u64, u32, vp, u64, vp, vp, u64, vp, vp, sz, vp]),
}
BGZF_RANGE_EXPORTS = tuple(BGZF_RANGE_SIGNATURES)
BGZF_RANGE_VIRTUAL = 1
# ... and of include/hdlz_bgzf_stored.h: the BGZF writer that falls back to a stored member (tests/test_bgzf_stored_cabi.py)
BGZF_STORED_SIGNATURES = {
    "hdlz_bgzf_stored_bound": (sz, [u64, u32]),
    "hdlz_bgzf_join_stored_work_bytes": (sz, [u64]),
    # d_in, d_in_off, in_pitch, in_len, d_rows, row_pitch, d_len, d_status, nblocks, d_crc, d_file, file_cap, d_off, d_kind, d_result,
    # d_work, work_bytes, stream
    "hdlz_bgzf_join_stored_ws": (ci, [vp, vp, u64, u32, vp, u64, vp, vp, u64, vp, vp, u64, vp, vp, vp, vp, sz, vp]),
}
BGZF_STORED_EXPORTS = tuple(BGZF_STORED_SIGNATURES)
# ... and of include/hdlz_gunzip.h: gzip members of any writer, one per stream (tests/test_gunzip_cabi.py)
GUNZIP_SIGNATURES = {
    "hdlz_gunzip_work_bytes": (sz, [u64, u32, u64, ci]),
    # d_in, d_in_off, in_pitch, in_len, nstreams, d_out, out_pitch, d_out_len, d_status, d_in_used, d_crc, d_work, work_bytes, stream
    "hdlz_gunzip_ws": (ci, _BATCH_IN + [vp, u64, vp, vp, vp, vp, vp, sz, vp]),
}
GUNZIP_EXPORTS = tuple(GUNZIP_SIGNATURES)
# ... and of include/hdlz_zip.h: ZIP archives, the directory indexed and the entries read on the device (tests/test_zip_cabi.py)
ZIP_SIGNATURES = {
    "hdlz_zip_index_work_bytes": (sz, [u64, u64]),
    # d_file, file_len, entry_cap, out_align, d_entries, d_result, d_work, work_bytes, stream
    "hdlz_zip_index_ws": (ci, [vp, u64, u64, u32, vp, vp, vp, sz, vp]),
    "hdlz_zip_inflate_work_bytes": (sz, [u64, u32, u64]),
    # d_file, file_len, d_entries, first, count, in_len, d_out, out_cap, d_entry_status, d_result, d_work, work_bytes, stream
    "hdlz_zip_inflate_ws": (ci, [vp, u64, vp, u64, u64, u32, vp, u64, vp, vp, vp, sz, vp]),
}
ZIP_EXPORTS = tuple(ZIP_SIGNATURES)
ZIP_LARGE_MIN = 16384          # HDLZ_ZIP_LARGE_MIN
# ... and of include/hdlz_zip_write.h: a ZIP archive written from the rows of one compress batch (tests/test_zip_write_cabi.py)
ZIP_WRITE_SIGNATURES = {
    "hdlz_zip_write_bound": (sz, [u64, u64, u32, u64, u64]),      # nentries, nblocks, block_len, total_in, names_len
    "hdlz_zip_write_work_bytes": (sz, [u64, u64]),                # nentries, nblocks
    # d_in, d_ent_off, d_names, d_name_off, nentries, d_in_off, d_rows, row_pitch, d_len, d_end_bits, d_status, nblocks, d_blk_first, d_crc,
    # flags, dos_datetime, out_align, total_in, d_file, file_cap, d_entries, d_result, d_work, work_bytes, stream
    "hdlz_zip_write_ws": (ci, [vp, vp, vp, vp, u64, vp, vp, u64, vp, vp, vp, u64, vp, vp, u32, u32, u32, u64, vp, u64, vp, vp, vp, sz, vp]),
}
ZIP_WRITE_EXPORTS = tuple(ZIP_WRITE_SIGNATURES)
ZIP_FLAG_UTF8 = 0x800          # HDLZ_ZIP_FLAG_UTF8
# ... and of include/hdlz_zip64.h: ZIP64 archives indexed, read and written (tests/test_zip64_cabi.py)
ZIP64_SIGNATURES = {
    "hdlz_zip64_index_work_bytes": (sz, [u64, u64]),
    "hdlz_zip64_index_ws": (ci, [vp, u64, u64, u32, vp, vp, vp, sz, vp]),                              # as hdlz_zip_index_ws
    "hdlz_zip64_inflate_work_bytes": (sz, [u64, u32, u64]),
    "hdlz_zip64_inflate_ws": (ci, [vp, u64, vp, u64, u64, u32, vp, u64, vp, vp, vp, sz, vp]),          # as hdlz_zip_inflate_ws
    "hdlz_zip64_write_bound": (sz, [u64, u64, u32, u64, u64]),
    "hdlz_zip64_write_work_bytes": (sz, [u64, u64]),
    # as hdlz_zip_write_ws, zip64_from behind out_align
    "hdlz_zip64_write_ws": (ci, [vp, vp, vp, vp, u64, vp, vp, u64, vp, vp, vp, u64, vp, vp, u32, u32, u32, u64, u64, vp, u64, vp, vp, vp, sz, vp]),
}
ZIP64_EXPORTS = tuple(ZIP64_SIGNATURES)
# ... and of include/hdlz_gzip_members.h: a gzip file of many members, indexed by a guess and read verified (tests/test_gzip_members_cabi.py)
GZIP_MEMBERS_SIGNATURES = {
    "hdlz_gzip_members_index_work_bytes": (sz, [u64]),
    # d_file, file_len, member_cap, d_off, d_out_off, d_result, d_work, work_bytes, stream
    "hdlz_gzip_members_index_ws": (ci, [vp, u64, u64, vp, vp, vp, vp, sz, vp]),
    "hdlz_gzip_members_inflate_work_bytes": (sz, [u64]),
    # d_file, file_len, d_off, d_out_off, nmembers, d_out, out_cap, d_member_status, d_result, d_work, work_bytes, stream
    "hdlz_gzip_members_inflate_ws": (ci, [vp, u64, vp, vp, u64, vp, u64, vp, vp, vp, sz, vp]),
}
GZIP_MEMBERS_EXPORTS = tuple(GZIP_MEMBERS_SIGNATURES)
# ... and of include/hdlz_seek.h: the seek index of a gzip or zlib stream and batched ranges through it (tests/test_seek_cabi.py, which
# also holds its refusals: the recorded fixtures of tests/test_api_refusals.py cover the twelve *_SIGNATURES tables above and predate
# this header, hence the other name)
SEEK_CALLS = {
    "hdlz_seek_index_work_bytes": (sz, [u64, u32, u64, u64]),        # file_len, flags, out_cap, point_cap
    # d_file, file_len, flags, span, d_out, out_cap, d_bit, d_pos, d_crc, d_win, point_cap, d_result, d_work, work_bytes, stream
    "hdlz_seek_index_ws": (ci, [vp, u64, u32, u32, vp, u64, vp, vp, vp, vp, u64, vp, vp, sz, vp]),
    "hdlz_seek_ranges_work_bytes": (sz, [u64, u64, u64, u32]),       # nranges, task_cap, seg_cap, flags
    # d_file, file_len, d_bit, d_pos, d_crc, d_win, npoints, d_ranges, nranges, flags, seg_cap, d_out, out_cap, d_range_off, d_range_status,
    # task_cap, d_result, d_work, work_bytes, stream
    "hdlz_seek_read_ranges_ws": (ci, [vp, u64, vp, vp, vp, vp, u64, vp, u64, u32, u64, vp, u64, vp, vp, u64, vp, vp, sz, vp]),
}
SEEK_EXPORTS = tuple(SEEK_CALLS)
SEEK_ZLIB, SEEK_GZIP, SEEK_WINDOW = 1, 2, 32768      # HDLZ_SEEK_ZLIB, HDLZ_SEEK_GZIP, HDLZ_SEEK_WINDOW
# ... and of include/hdlz_png.h: PNG images indexed, inflated and unfiltered on the device (tests/test_png_cabi.py, which also holds its
# refusals, as tests/test_seek_cabi.py does for SEEK_CALLS)
PNG_CALLS = {
    "hdlz_png_index_work_bytes": (sz, [u64, u64]),                   # n, image_cap
    # d_files, files_len, d_file_off, d_file_len, n, flags, out_align, image_cap, d_images, d_result, d_work, work_bytes, stream
    "hdlz_png_index_ws": (ci, [vp, u64, vp, vp, u64, u32, u32, u64, vp, vp, vp, sz, vp]),
    "hdlz_png_decode_work_bytes": (sz, [u64, u64, u64, u64]),        # count, idat_cap, z_bytes, raw_bytes
    # d_files, files_len, d_images, first, count, flags, idat_cap, z_bytes, raw_bytes, d_out, out_cap, d_image_status, d_result, d_work,
    # work_bytes, stream
    "hdlz_png_decode_ws": (ci, [vp, u64, vp, u64, u64, u32, u64, u64, u64, vp, u64, vp, vp, vp, sz, vp]),
}
PNG_EXPORTS = tuple(PNG_CALLS)
PNG_RAW, PNG_EXPAND, PNG_LARGE_MIN = 0, 1, 16384     # HDLZ_PNG_RAW, HDLZ_PNG_EXPAND, HDLZ_PNG_LARGE_MIN
PNG_ADAM7 = 4                                        # HDLZ_PNG_ADAM7, OR-ed into either: interlaced images are read
# ... and of include/hdlz_png_write.h: PNG files written on the device (tests/test_png_write_cabi.py, which also holds its refusals)
PNG_WRITE_CALLS = {
    "hdlz_png_filter_work_bytes": (sz, [u64]),                       # n
    # d_pix, pix_len, d_specs, n, mode, total_rows, d_raw, raw_cap, d_row_filter, d_status, d_raw_off, d_work, work_bytes, stream
    "hdlz_png_filter_ws": (ci, [vp, u64, vp, u64, u32, u64, vp, u64, vp, vp, vp, vp, sz, vp]),
    "hdlz_png_write_bound": (sz, [u64, u64, u64, u32, u32]),         # n, total_raw, nblocks, block_len, idat_len
    "hdlz_png_write_work_bytes": (sz, [u64, u64]),                   # n, nblocks
    # d_specs, n, d_raw, d_raw_off, d_filter_status, d_in_off, d_rows, row_pitch, d_len, d_end_bits, d_status, nblocks, d_blk_first, idat_len,
    # flags, out_align, d_file, file_cap, d_file_off, d_file_len, d_image_status, d_images, d_result, d_work, work_bytes, stream
    "hdlz_png_write_ws": (ci, [vp, u64, vp, vp, vp, vp, vp, u64, vp, vp, vp, u64, vp, u32, u32, u32, vp, u64, vp, vp, vp, vp, vp, vp, sz, vp]),
}
PNG_WRITE_EXPORTS = tuple(PNG_WRITE_CALLS)
# HDLZ_PNG_FILTER_ADAPTIVE, HDLZ_PNGW_BAND, HDLZ_PNGW_STEP, HDLZ_PNGW_ROW_REG_MAX
PNG_FILTER_ADAPTIVE, PNGW_BAND, PNGW_STEP, PNGW_ROW_REG_MAX = 5, 8, 1024, 4096
# ... and of include/hdlz_tiff.h: TIFF images indexed, their strips and tiles inflated and unpredicted on the device (tests/test_tiff_cabi.py,
# which also holds its refusals)
TIFF_CALLS = {
    "hdlz_tiff_index_work_bytes": (sz, [u64, u64]),                  # n, image_cap
    # d_files, files_len, d_file_off, d_file_len, d_page, n, out_align, image_cap, d_images, d_result, d_work, work_bytes, stream
    "hdlz_tiff_index_ws": (ci, [vp, u64, vp, vp, vp, u64, u32, u64, vp, vp, vp, sz, vp]),
    "hdlz_tiff_decode_work_bytes": (sz, [u64, u64, u64]),            # count, chunk_cap, raw_bytes
    # d_files, files_len, d_images, first, count, chunk_cap, raw_bytes, d_out, out_cap, d_image_status, d_result, d_work, work_bytes, stream
    "hdlz_tiff_decode_ws": (ci, [vp, u64, vp, u64, u64, u64, u64, vp, u64, vp, vp, vp, sz, vp]),
}
TIFF_EXPORTS = tuple(TIFF_CALLS)
TIFF_LARGE_MIN = 16384                               # HDLZ_TIFF_LARGE_MIN (HDLZ_PNG_LARGE_MIN's number, not measured again for TIFF)
_lib = None


class CState(ctypes.Structure):
    """hdlz_cstate: the session of hdlz_compress_chunk (64 bytes)"""
    _fields_ = [(f, u32) for f in ("pos", "skip", "out_words", "base_bits", "carry_word", "adler_a", "adler_c", "started",
                                   "done", "out_len", "status")] + [("reserved", u32 * 5)]


class JoinResult(ctypes.Structure):
    """hdlz_join_result: the result record of hdlz_join_batch_ws (16 bytes)"""
    _fields_ = [("stream_len", u64), ("status", u32), ("adler", u32)]


class UnjoinResult(ctypes.Structure):
    """hdlz_unjoin_result: the result record of hdlz_unjoin_ws (24 bytes)"""
    _fields_ = [("out_len", u64), ("first_bad", u64), ("status", u32), ("adler", u32)]


class JoinGzipResult(ctypes.Structure):
    """hdlz_join_gzip_result: the result record of hdlz_join_gzip_ws (16 bytes)"""
    _fields_ = [("stream_len", u64), ("status", u32), ("crc", u32)]


class UnjoinGzipResult(ctypes.Structure):
    """hdlz_unjoin_gzip_result: the result record of hdlz_unjoin_gzip_ws (24 bytes)"""
    _fields_ = [("out_len", u64), ("first_bad", u64), ("status", u32), ("crc", u32)]


class BgzfJoinResult(ctypes.Structure):
    """hdlz_bgzf_join_result: the result record of hdlz_bgzf_join_ws (16 bytes)"""
    _fields_ = [("file_len", u64), ("status", u32), ("first_bad", u32)]


class BgzfStoredResult(ctypes.Structure):
    """hdlz_bgzf_stored_result: the result record of hdlz_bgzf_join_stored_ws (24 bytes)"""
    _fields_ = [("file_len", u64), ("nstored", u64), ("status", u32), ("first_bad", u32)]


class BgzfIndexResult(ctypes.Structure):
    """hdlz_bgzf_index_result: the result record of hdlz_bgzf_index_ws (32 bytes)"""
    _fields_ = [("nmembers", u64), ("total_out", u64), ("file_used", u64), ("status", u32), ("eof_marker", u32)]


class BgzfInflateResult(ctypes.Structure):
    """hdlz_bgzf_inflate_result: the result record of hdlz_bgzf_inflate_ws (24 bytes)"""
    _fields_ = [("out_len", u64), ("first_bad", u64), ("status", u32), ("reserved", u32)]


class BgzfRangesResult(ctypes.Structure):
    """hdlz_bgzf_ranges_result: the result record of hdlz_bgzf_read_ranges_ws (32 bytes)"""
    _fields_ = [("total_out", u64), ("ntasks", u64), ("first_bad", u64), ("status", u32), ("reserved", u32)]


class SeekResult(ctypes.Structure):
    """hdlz_seek_result: the result record of hdlz_seek_index_ws (40 bytes)"""
    _fields_ = [("npoints", u64), ("total_out", u64), ("end_bit", u64), ("max_seg", u64), ("status", u32), ("route", u32)]


SeekRangesResult = BgzfRangesResult      # hdlz_seek_ranges_result: a typedef of hdlz_bgzf_ranges_result


class GzipMembersIndexResult(ctypes.Structure):
    """hdlz_gzip_members_index_result: the result record of hdlz_gzip_members_index_ws (24 bytes)"""
    _fields_ = [("nmembers", u64), ("total_out", u64), ("status", u32), ("reserved", u32)]


class GzipMembersInflateResult(ctypes.Structure):
    """hdlz_gzip_members_inflate_result: the result record of hdlz_gzip_members_inflate_ws (24 bytes)"""
    _fields_ = [("out_len", u64), ("first_bad", u64), ("status", u32), ("reserved", u32)]


class ZipEntry(ctypes.Structure):
    """hdlz_zip_entry: one record of hdlz_zip_index_ws (48 bytes)"""
    _fields_ = [("cd_off", u64), ("payload_off", u64), ("out_off", u64), ("csize", u32), ("usize", u32), ("crc", u32),
                ("method", ctypes.c_uint16), ("flags", ctypes.c_uint16), ("name_len", ctypes.c_uint16), ("reserved", ctypes.c_uint16),
                ("status", u32)]


class Zip64Entry(ctypes.Structure):
    """hdlz_zip64_entry: one record of hdlz_zip64_index_ws (64 bytes)"""
    _fields_ = [("cd_off", u64), ("payload_off", u64), ("out_off", u64), ("csize", u64), ("usize", u64), ("crc", u32), ("status", u32),
                ("method", ctypes.c_uint16), ("flags", ctypes.c_uint16), ("name_len", ctypes.c_uint16), ("reserved", ctypes.c_uint16),
                ("reserved2", u64)]


class ZipIndexResult(ctypes.Structure):
    """hdlz_zip_index_result: the result record of hdlz_zip_index_ws (40 bytes)"""
    _fields_ = [("nentries", u64), ("total_out", u64), ("cd_off", u64), ("cd_size", u64), ("status", u32), ("reserved", u32)]


class ZipInflateResult(ctypes.Structure):
    """hdlz_zip_inflate_result: the result record of hdlz_zip_inflate_ws (24 bytes)"""
    _fields_ = [("out_len", u64), ("first_bad", u64), ("status", u32), ("reserved", u32)]


class ZipWriteResult(ctypes.Structure):
    """hdlz_zip_write_result: the result record of hdlz_zip_write_ws (40 bytes)"""
    _fields_ = [("file_len", u64), ("cd_off", u64), ("cd_size", u64), ("nstored", u64), ("status", u32), ("first_bad", u32)]


class PngImage(ctypes.Structure):
    """hdlz_png_image: one record of hdlz_png_index_ws (136 bytes)"""
    _fields_ = [(f, u64) for f in ("file_off", "file_len", "idat_off", "zlen", "plte_off", "trns_off", "used", "row_bytes", "raw_len",
                                   "out_len", "z_off", "raw_off", "out_off")] + \
               [(f, u32) for f in ("width", "height", "nidat", "plte_n", "trns_n", "status")] + \
               [(f, ctypes.c_uint8) for f in ("depth", "colour", "interlace", "channels_out", "sample_bytes")] + [("reserved", ctypes.c_uint8 * 3)]


class PngIndexResult(ctypes.Structure):
    """hdlz_png_index_result: the result record of hdlz_png_index_ws (40 bytes)"""
    _fields_ = [("nimages", u64), ("total_z", u64), ("total_raw", u64), ("total_out", u64), ("status", u32), ("reserved", u32)]


class PngDecodeResult(ctypes.Structure):
    """hdlz_png_decode_result: the result record of hdlz_png_decode_ws (24 bytes)"""
    _fields_ = [("out_len", u64), ("first_bad", u64), ("status", u32), ("reserved", u32)]


class PngSpec(ctypes.Structure):
    """hdlz_png_spec: one image of hdlz_png_filter_ws and hdlz_png_write_ws (24 bytes)"""
    _fields_ = [("pix_off", u64), ("width", u32), ("height", u32), ("depth", ctypes.c_uint8), ("colour", ctypes.c_uint8), ("reserved", ctypes.c_uint8 * 6)]


class PngWriteResult(ctypes.Structure):
    """hdlz_png_write_result: the result record of hdlz_png_write_ws (24 bytes)"""
    _fields_ = [("total_len", u64), ("first_bad", u64), ("status", u32), ("reserved", u32)]


class TiffImage(ctypes.Structure):
    """hdlz_tiff_image: one record of hdlz_tiff_index_ws (136 bytes)"""
    _fields_ = [(f, u64) for f in ("file_off", "file_len", "ifd_off", "next_ifd", "off_arr", "cnt_arr", "raw_len", "out_len", "chunk_off",
                                   "raw_off", "out_off")] + \
               [(f, u32) for f in ("width", "height", "tile_w", "tile_h", "nchunks", "compression", "photometric", "status")] + \
               [(f, ctypes.c_uint8) for f in ("off_type", "cnt_type", "bits", "samples", "format", "predictor", "big_endian", "tiled")] + \
               [("reserved", ctypes.c_uint8 * 8)]


class TiffIndexResult(ctypes.Structure):
    """hdlz_tiff_index_result: the result record of hdlz_tiff_index_ws (40 bytes)"""
    _fields_ = [("nimages", u64), ("total_chunks", u64), ("total_raw", u64), ("total_out", u64), ("status", u32), ("reserved", u32)]


class TiffDecodeResult(ctypes.Structure):
    """hdlz_tiff_decode_result: the result record of hdlz_tiff_decode_ws (24 bytes)"""
    _fields_ = [("out_len", u64), ("first_bad", u64), ("status", u32), ("reserved", u32)]


class IState(ctypes.Structure):
    """hdlz_istate: the session of hdlz_inflate_chunk (384 bytes)"""
    _fields_ = [(f, u32) for f in ("bitpos", "out_pos", "phase", "final_", "hm", "srem", "nlen", "ndist", "started",
                                   "done", "status", "need")] + [("reserved", u32 * 4), ("lengths", ctypes.c_uint8 * 320)]


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libhdlz.so is not built (%s): run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "or hdl_deflate_amd/csrc/build.sh -- there is no CPU fallback" % LIB_PATH)
    # torch ships its own libamdhip64.so (SONAME libamdhip64.so.7).  Import it FIRST so that libhdlz's
    # NEEDED libamdhip64.so.7 resolves to the runtime torch already loaded; the other order would put
    # two HIP runtimes in one process and torch's streams/pointers would be foreign to ours.
    import torch  # noqa: F401
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in list(SIGNATURES.items()) + list(JOIN_SIGNATURES.items()) + list(UNJOIN_SIGNATURES.items()) + \
            list(GZIP_SIGNATURES.items()) + list(BGZF_SIGNATURES.items()) + list(BGZF_RANGE_SIGNATURES.items()) + list(BGZF_STORED_SIGNATURES.items()) + \
            list(GUNZIP_SIGNATURES.items()) + list(ZIP_SIGNATURES.items()) + list(ZIP_WRITE_SIGNATURES.items()) + list(ZIP64_SIGNATURES.items()) + \
            list(GZIP_MEMBERS_SIGNATURES.items()) + list(SEEK_CALLS.items()) + list(PNG_CALLS.items()) + list(PNG_WRITE_CALLS.items()) + \
            list(TIFF_CALLS.items()):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L
