"""PNG files read into device tensors (include/hdlz_png.h): the chunks are walked, the IDAT stream inflated, the scanlines unfiltered
and expanded on the device; only the records of the index pass through the host, no pixel byte does.  And written from device tensors
(include/hdlz_png_write.h): filtered, deflated and framed on the device; the finished files are what crosses to the host."""
import numpy as np

from .constants import OK
from .errors import HdlzStatusError

# hdlz_png_image, 136 bytes (little-endian, as the device writes it)
IMAGE_DTYPE = np.dtype([(f, "<u8") for f in ("file_off", "file_len", "idat_off", "zlen", "plte_off", "trns_off", "used", "row_bytes",
                                             "raw_len", "out_len", "z_off", "raw_off", "out_off")] +
                       [(f, "<u4") for f in ("width", "height", "nidat", "plte_n", "trns_n", "status")] +
                       [(f, "u1") for f in ("depth", "colour", "interlace", "channels_out", "sample_bytes")] + [("reserved", "u1", (3,))])
assert IMAGE_DTYPE.itemsize == 136
# hdlz_png_spec, 24 bytes
SPEC_DTYPE = np.dtype([("pix_off", "<u8"), ("width", "<u4"), ("height", "<u4"), ("depth", "u1"), ("colour", "u1"), ("reserved", "u1", (6,))])
assert SPEC_DTYPE.itemsize == 24
COLOUR_OF_CHANNELS = {1: 0, 2: 4, 3: 2, 4: 6}


class PngIndex(object):
    """The index of a batch of PNG files (Engine.png_index).
    images     int64[n, 17] on the device: the n records of hdlz_png_index_ws (136 bytes each), what Engine.decode_png passes on
    record     the call's result record (_lib.PngIndexResult: nimages, total_z, total_raw, total_out, status)
    host       the records on the host, a numpy array of IMAGE_DTYPE
    out_align  what the slots' starts are multiples of
    expand     True: HDLZ_PNG_EXPAND, plain samples; False: HDLZ_PNG_RAW, the scanlines as PNG packs them
    interlaced True: taken with HDLZ_PNG_ADAM7 (Adam7 interlaced images are read), which Engine.decode_png passes on
    shapes, dtypes   per image what its slot holds: (H, W) or (H, W, C) of torch.uint8 or torch.uint16 when expand is set, else
               (H, row_bytes) of torch.uint8; None for an image whose status is not OK"""

    def __init__(self, images, record, host, out_align, expand, interlaced=False):
        import torch
        self.images, self.record, self.host, self.out_align, self.expand = images, record, host, out_align, bool(expand)
        self.interlaced = bool(interlaced)
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


def load_png(engine, files, interlaced=True):
    """files: the bytes of one PNG file, a list of such, or (flat uint8 device tensor, offsets int64, lengths int64) -- file i is
    tensor[offsets[i] : offsets[i] + lengths[i]], which is what Engine.inflate_zip leaves of a ZIP of PNGs -> a list of device tensors
    (one tensor for one `bytes`), views into one flat output with slots at multiples of 64: (H, W) or (H, W, C), torch.uint8, or
    torch.uint16 for depth 16; palette images as RGB or RGBA.  interlaced: Adam7 interlaced files are read like the others (False:
    they are refused, E_BAD_BTYPE).  An image that fails raises HdlzStatusError with .first_bad = its index."""
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
    index = engine.png_index(d, offsets, lengths, out_align=64, expand=True, interlaced=interlaced)
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


def save_png(engine, tensors, **kw):
    """tensors: one device tensor or a list of them, (H, W) or (H, W, C) of torch.uint8 or torch.uint16, C in 1 .. 4 -- grey, grey +
    alpha, RGB, RGBA; (H, W, 1) is grey -> the bytes of a PNG file (a list of them for a list): what load_png reads back to the same
    tensors.  The keywords of Engine.encode_png (filter, block, idat, cwindow, maxmatch) pass through.  No pixel byte crosses to the host
    before it is compressed: the tensors are gathered on the device, and the finished files come back in one copy.  An image that
    fails raises HdlzStatusError with .first_bad = its index."""
    import torch
    one = torch.is_tensor(tensors)
    ts = [tensors] if one else list(tensors)
    shapes, flat = [], []
    for k, t in enumerate(ts):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype in (torch.uint8, torch.uint16) and t.dim() in (2, 3)):
            raise ValueError("save_png: tensor %d must be a device tensor (H, W) or (H, W, C) of uint8 or uint16" % k)
        h, w, c = t.shape[0], t.shape[1], (t.shape[2] if t.dim() == 3 else 1)
        if c not in COLOUR_OF_CHANNELS:
            raise ValueError("save_png: tensor %d has %d channels (1 .. 4 are written)" % (k, c))
        shapes.append((h, w, c, 16 if t.dtype == torch.uint16 else 8))
        flat.append(t.contiguous().view(torch.uint8).reshape(-1))
    d_pix = flat[0] if len(flat) == 1 else torch.cat(flat) if flat else torch.empty(0, dtype=torch.uint8, device=engine.device)
    files, index = engine.encode_png(d_pix, shapes, **kw)
    host = files.cpu().numpy().tobytes()
    res = [host[int(r["file_off"]):int(r["file_off"]) + int(r["file_len"])] for r in index.host]
    return res[0] if one else res
