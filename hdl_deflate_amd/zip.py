"""Host side of include/hdlz_zip.h: the index of a ZIP file as Engine.zip_index returns it, the numpy view of its records and the
decoding of entry names.  Nothing here computes on file data: the directory is indexed and the entries are read on the device."""
import numpy as np

# hdlz_zip_entry, 48 bytes (little-endian, as the device writes it)
ENTRY_DTYPE = np.dtype([("cd_off", "<u8"), ("payload_off", "<u8"), ("out_off", "<u8"), ("csize", "<u4"), ("usize", "<u4"), ("crc", "<u4"),
                        ("method", "<u2"), ("flags", "<u2"), ("name_len", "<u2"), ("reserved", "<u2"), ("status", "<u4")])
assert ENTRY_DTYPE.itemsize == 48
FLAG_UTF8 = 0x800


def decode_name(raw, flags):
    """an entry's name as zipfile reads it: UTF-8 when flag bit 11 is set, cp437 otherwise"""
    return raw.decode("utf-8") if flags & FLAG_UTF8 else raw.decode("cp437")


class ZipIndex(object):
    """The index of a ZIP file (Engine.zip_index).
    entries    int64[k, 6] on the device: the k records of hdlz_zip_index_ws (48 bytes each), what Engine.inflate_zip passes on
    record     the call's result record (_lib.ZipIndexResult: nentries, total_out, cd_off, cd_size, status)
    host       the records on the host, a numpy array of ENTRY_DTYPE (cd_off, payload_off, out_off, csize, usize, crc, method, flags,
               name_len, status)
    names      the entries' names, in the directory's order
    out_align  what the slots' starts are multiples of"""

    def __init__(self, entries, record, host, names, out_align):
        self.entries, self.record, self.host, self.names, self.out_align = entries, record, host, names, out_align

    def __len__(self):
        return len(self.host)
