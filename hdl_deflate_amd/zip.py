"""Host side of include/hdlz_zip.h and hdlz_zip_write.h: the index of a ZIP file as Engine.zip_index and Engine.compress_zip return
it, the numpy view of its records, the decoding of entry names and the date words of a header.  Nothing here computes on file data:
the directory is indexed, the entries are read and the file is written on the device."""
import numpy as np

# hdlz_zip_entry, 48 bytes (little-endian, as the device writes it)
ENTRY_DTYPE = np.dtype([("cd_off", "<u8"), ("payload_off", "<u8"), ("out_off", "<u8"), ("csize", "<u4"), ("usize", "<u4"), ("crc", "<u4"),
                        ("method", "<u2"), ("flags", "<u2"), ("name_len", "<u2"), ("reserved", "<u2"), ("status", "<u4")])
assert ENTRY_DTYPE.itemsize == 48
# hdlz_zip64_entry, 64 bytes (include/hdlz_zip64.h): the same names, so code that reads index.host[...] works on both
ENTRY64_DTYPE = np.dtype([("cd_off", "<u8"), ("payload_off", "<u8"), ("out_off", "<u8"), ("csize", "<u8"), ("usize", "<u8"), ("crc", "<u4"),
                          ("status", "<u4"), ("method", "<u2"), ("flags", "<u2"), ("name_len", "<u2"), ("reserved", "<u2"), ("reserved2", "<u8")])
assert ENTRY64_DTYPE.itemsize == 64
FLAG_UTF8 = 0x800


def decode_name(raw, flags):
    """an entry's name as zipfile reads it: UTF-8 when flag bit 11 is set, cp437 otherwise"""
    return raw.decode("utf-8") if flags & FLAG_UTF8 else raw.decode("cp437")


def dos_datetime(date_time):
    """(year, month, day, hour, minute, second) -> date << 16 | time, the MS-DOS words of a ZIP header (what hdlz_zip_write_ws takes)"""
    y, mo, d, h, mi, s = (int(x) for x in date_time)
    if not (1980 <= y <= 2107 and 1 <= mo <= 12 and 1 <= d <= 31 and 0 <= h < 24 and 0 <= mi < 60 and 0 <= s < 60):
        raise ValueError("date_time %r is outside what a ZIP header holds (1980 .. 2107)" % (date_time,))
    return ((y - 1980) << 9 | mo << 5 | d) << 16 | (h << 11 | mi << 5 | s >> 1)


class ZipIndex(object):
    """The index of a ZIP file (Engine.zip_index).
    entries    int64[k, 6] on the device: the k records of hdlz_zip_index_ws (48 bytes each), what Engine.inflate_zip passes on;
               int64[k, 8] when zip64 is set: the records of hdlz_zip64_index_ws (64 bytes each, host: ENTRY64_DTYPE, the same names)
    zip64      which of the two calls wrote the records
    record     the call's result record (_lib.ZipIndexResult: nentries, total_out, cd_off, cd_size, status)
    host       the records on the host, a numpy array of ENTRY_DTYPE (cd_off, payload_off, out_off, csize, usize, crc, method, flags,
               name_len, status)
    names      the entries' names, in the directory's order
    out_align  what the slots' starts are multiples of
    write_record   an index that Engine.compress_zip hands back with the file it wrote: the writer's record (_lib.ZipWriteResult:
               file_len, cd_off, cd_size, nstored, status, first_bad); None for an index that was read"""
    write_record = None

    def __init__(self, entries, record, host, names, out_align, zip64=False):
        self.entries, self.record, self.host, self.names, self.out_align, self.zip64 = entries, record, host, names, out_align, bool(zip64)

    def __len__(self):
        return len(self.host)
