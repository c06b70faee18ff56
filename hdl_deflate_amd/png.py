"""PNG files read into device tensors (include/hdlz_png.h): the chunks are walked, the IDAT stream inflated, the scanlines unfiltered
and expanded on the device; only the records of the index pass through the host, no pixel byte does."""
import numpy as np

from .constants import OK
from .errors import HdlzStatusError

# hdlz_png_image, 136 bytes (little-endian, as the device writes it)
IMAGE_DTYPE = np.dtype([(f, "<u8") for f in ("file_off", "file_len", "idat_off", "zlen", "plte_off", "trns_off", "used", "row_bytes",
                                             "raw_len", "out_len", "z_off", "raw_off", "out_off")] +
                       [(f, "<u4") for f in ("width", "height", "nidat", "plte_n", "trns_n", "status")] +
                       [(f, "u1") for f in ("depth", "colour", "interlace", "channels_out", "sample_bytes")] + [("reserved", "u1", (3,))])
assert IMAGE_DTYPE.itemsize == 136


class PngIndex(object):
    """The index of a batch of PNG files (Engine.png_index).
    images     int64[n, 17] on the device: the n records of hdlz_png_index_ws (136 bytes each), what Engine.decode_png passes on
    record     the call's result record (_lib.PngIndexResult: nimages, total_z, total_raw, total_out, status)
    host       the records on the host, a numpy array of IMAGE_DTYPE
    out_align  what the slots' starts are multiples of
    expand     True: HDLZ_PNG_EXPAND, plain samples; False: HDLZ_PNG_RAW, the scanlines as PNG packs them
    shapes, dtypes   per image what its slot holds: (H, W) or (H, W, C) of torch.uint8 or torch.uint16 when expand is set, else
               (H, row_bytes) of torch.uint8; None for an image whose status is not OK"""

    def __init__(self, images, record, host, out_align, expand):
        import torch
        self.images, self.record, self.host, self.out_align, self.expand = images, record, host, out_align, bool(expand)
        self.shapes, self.dtypes = [], []
        for r in host:
            if r["status"] != OK:
                self.shapes.append(None)
                self.dtypes.append(None)
                continue
            h, w, c = int(r["height"]), int(r["width"]), int(r["channels_out"])
            if not self.expand:
                self.shapes.append((h, int(r["row_bytes"])))
                self.dtypes.append(torch.uint8)
            else:
                self.shapes.append((h, w) if c == 1 else (h, w, c))
                self.dtypes.append(torch.uint16 if r["sample_bytes"] == 2 else torch.uint8)

    def __len__(self):
        return len(self.host)


def load_png(engine, files):
    """files: the bytes of one PNG file, a list of such, or (flat uint8 device tensor, offsets int64, lengths int64) -- file i is
    tensor[offsets[i] : offsets[i] + lengths[i]], which is what Engine.inflate_zip leaves of a ZIP of PNGs -> a list of device tensors
    (one tensor for one `bytes`), views into one flat output with slots at multiples of 64: (H, W) or (H, W, C), torch.uint8, or
    torch.uint16 for depth 16; palette images as RGB or RGBA.  An image that fails raises HdlzStatusError with .first_bad = its index."""
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
    index = engine.png_index(d, offsets, lengths, out_align=64, expand=True)
    bad = np.nonzero(index.host["status"] != OK)[0]
    if len(bad):
        raise HdlzStatusError(int(index.host["status"][bad[0]]), "load_png: image %d" % bad[0], first_bad=int(bad[0]))
    out, status = engine.decode_png(d, index)
    bad = torch.nonzero(status != OK).reshape(-1)
    if bad.numel():
        k = int(bad[0])
        raise HdlzStatusError(int(status[k]), "load_png: image %d" % k, first_bad=k)
    res = []
    for k, r in enumerate(index.host):
        o, n = int(r["out_off"]), int(r["out_len"])
        res.append(out[o:o + n].view(index.dtypes[k]).reshape(index.shapes[k]))
    return res[0] if one else res
