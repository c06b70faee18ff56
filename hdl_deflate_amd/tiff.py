"""TIFF files read into device tensors (include/hdlz_tiff.h): the tag directory is walked, every deflate strip or tile inflated, the
predictor undone and the samples swapped to little-endian on the device; only the records of the index pass through the host, no
pixel byte does."""
import numpy as np

from .constants import OK
from .errors import HdlzStatusError

# hdlz_tiff_image, 136 bytes (little-endian, as the device writes it)
IMAGE_DTYPE = np.dtype([(f, "<u8") for f in ("file_off", "file_len", "ifd_off", "next_ifd", "off_arr", "cnt_arr", "raw_len", "out_len",
                                             "chunk_off", "raw_off", "out_off")] +
                       [(f, "<u4") for f in ("width", "height", "tile_w", "tile_h", "nchunks", "compression", "photometric", "status")] +
                       [(f, "u1") for f in ("off_type", "cnt_type", "bits", "samples", "format", "predictor", "big_endian", "tiled")] +
                       [("reserved", "u1", (8,))])
assert IMAGE_DTYPE.itemsize == 136


def sample_dtype(fmt, bits):
    """the torch dtype of a sample of SampleFormat `fmt` (1 uint, 2 int, 3 float) and `bits` bits"""
    import torch
    return {(1, 8): torch.uint8, (1, 16): torch.uint16, (1, 32): torch.uint32, (1, 64): torch.uint64,
            (2, 8): torch.int8, (2, 16): torch.int16, (2, 32): torch.int32, (2, 64): torch.int64,
            (3, 32): torch.float32, (3, 64): torch.float64}[(int(fmt), int(bits))]


class TiffIndex(object):
    """The index of a batch of TIFF images (Engine.tiff_index).
    images     int64[n, 17] on the device: the n records of hdlz_tiff_index_ws (136 bytes each), what Engine.decode_tiff passes on
    record     the call's result record (_lib.TiffIndexResult: nimages, total_chunks, total_raw, total_out, status)
    host       the records on the host, a numpy array of IMAGE_DTYPE
    out_align  what the slots' starts are multiples of
    shapes, dtypes   per image what its slot holds: (H, W) or (H, W, C) of torch.uint8/16/32/64, int8/16/32/64 or float32/64 by
               SampleFormat and BitsPerSample; None for an image whose status is not OK"""

    def __init__(self, images, record, host, out_align):
        self.images, self.record, self.host, self.out_align = images, record, host, out_align
        self.shapes, self.dtypes = [], []
        for r in host:
            if r["status"] != OK:
                self.shapes.append(None)
                self.dtypes.append(None)
                continue
            h, w, c = int(r["height"]), int(r["width"]), int(r["samples"])
            self.shapes.append((h, w) if c == 1 else (h, w, c))
            self.dtypes.append(sample_dtype(r["format"], r["bits"]))

    def __len__(self):
        return len(self.host)


def load_tiff(engine, files, page=0):
    """files: the bytes of one TIFF file, a list of such, or (flat uint8 device tensor, offsets int64, lengths int64) -- file i is
    tensor[offsets[i] : offsets[i] + lengths[i]], which is what Engine.inflate_zip leaves of a ZIP of TIFFs -> a list of device tensors
    (one tensor for one `bytes`), views into one flat output with slots at multiples of 64: (H, W) or (H, W, C) in the file's sample
    type, little-endian.  page: the directory read of every file (an int), or one per file.  An image that fails raises
    HdlzStatusError with .first_bad = its index."""
    import torch
    one = isinstance(files, (bytes, bytearray, memoryview))
    if one:
        files = [bytes(files)]
    if isinstance(files, tuple):
        d, offsets, lengths = files
        offsets = torch.as_tensor(offsets, dtype=torch.int64).to(d.device)
        lengths = torch.as_tensor(lengths, dtype=torch.int64).to(d.device)
    else:
        blob = b"".join(files)
        d = engine._stage(blob)[:len(blob)]
        lens = np.array([len(f) for f in files], np.int64)
        offsets = torch.from_numpy(np.cumsum(lens) - lens).to(d.device)
        lengths = torch.from_numpy(lens).to(d.device)
    pages = None if isinstance(page, int) and page == 0 else np.broadcast_to(np.asarray(page, np.int64), (offsets.numel(),))
    index = engine.tiff_index(d, offsets, lengths, pages=pages, out_align=64)
    bad = np.nonzero(index.host["status"] != OK)[0]
    if len(bad):
        raise HdlzStatusError(int(index.host["status"][bad[0]]), "load_tiff: image %d" % bad[0], first_bad=int(bad[0]))
    out, status = engine.decode_tiff(d, index)
    bad = torch.nonzero(status != OK).reshape(-1)
    if bad.numel():
        k = int(bad[0])
        raise HdlzStatusError(int(status[k]), "load_tiff: image %d" % k, first_bad=k)
    res = []
    for k, r in enumerate(index.host):
        o, n = int(r["out_off"]), int(r["out_len"])
        res.append(out[o:o + n].view(index.dtypes[k]).reshape(index.shapes[k]))
    return res[0] if one else res
