""".npz files (numpy.savez, numpy.savez_compressed) read into device tensors and written from them: the ZIP directory is indexed and
every entry decoded and judged on the device (include/hdlz_zip.h), the file is written there (include/hdlz_zip_write.h); only the few
header bytes of each .npy entry pass through the host, no array byte does."""
import ast

import numpy as np

from .constants import OK
from .errors import Error, HdlzStatusError

MAGIC = b"\x93NUMPY"
_HEAD = 12          # magic, two version bytes, the header length (2 bytes in version 1, 4 in versions 2 and 3)


def _torch_dtype(descr):
    """a .npy descr -> (torch dtype, numpy dtype); raises for object, structured and big-endian types"""
    import torch
    if not isinstance(descr, str):
        raise Error("load_npz: structured dtype %r" % (descr,))
    dt = np.dtype(descr)
    if dt.hasobject or dt.kind == "O":
        raise Error("load_npz: object arrays hold pickles, not bytes")
    if dt.byteorder == ">":
        raise Error("load_npz: big-endian dtype %r" % descr)
    table = {"b1": torch.bool, "u1": torch.uint8, "i1": torch.int8, "i2": torch.int16, "i4": torch.int32, "i8": torch.int64,
             "f2": torch.float16, "f4": torch.float32, "f8": torch.float64, "c8": torch.complex64, "c16": torch.complex128}
    key = dt.kind + str(dt.itemsize)
    if key not in table:
        raise Error("load_npz: dtype %r has no torch counterpart" % descr)
    return table[key], dt


def parse_header(head, text):
    """the 12 first bytes of a .npy file and its header text -> (descr, fortran_order, shape)"""
    d = ast.literal_eval(text.decode("latin1" if head[6] < 3 else "utf-8"))
    if not isinstance(d, dict) or set(d) != {"descr", "fortran_order", "shape"}:
        raise Error("load_npz: a .npy header must hold descr, fortran_order and shape")
    return d["descr"], bool(d["fortran_order"]), tuple(int(x) for x in d["shape"])


def header_span(head):
    """the 12 first bytes of a .npy file -> (where its header text starts, its length)"""
    if len(head) < 10 or head[:6] != MAGIC:
        raise Error("load_npz: not a .npy entry (magic)")
    if head[6] == 1:
        return 10, head[8] | head[9] << 8
    if head[6] in (2, 3) and len(head) >= 12:
        return 12, int.from_bytes(head[8:12], "little")
    raise Error("load_npz: .npy version %d.%d" % (head[6], head[7]))


def load_npz(engine, data):
    """data: the bytes of an .npz file, or a flat uint8 device tensor holding them -> {name: device tensor}, as numpy.load names the
    arrays (".npy" stripped).  The entries are decoded into one flat device buffer with slots at multiples of 64 (Engine.zip_index with
    out_align=64, Engine.inflate_zip) and the tensors are views into it; an entry that fails raises HdlzStatusError with .first_bad =
    its index.  Fortran order, object and big-endian dtypes raise."""
    import torch
    d = data if torch.is_tensor(data) else engine._stage(data)[:len(data)]
    index = engine.zip_index(d, out_align=64)
    if index.record.status != OK:
        raise HdlzStatusError(index.record.status, "load_npz: the file's directory", first_bad=int(index.record.nentries))
    out, out_off, status = engine.inflate_zip(d, index)
    bad = torch.nonzero(status != OK).reshape(-1)
    if bad.numel():
        k = int(bad[0])
        raise HdlzStatusError(int(status[k]), "load_npz: entry %r" % index.names[k], first_bad=k)
    picks = [k for k, n in enumerate(index.names) if n.endswith(".npy")]
    if not picks:
        return {}
    off, usize = index.host["out_off"].astype(np.int64), index.host["usize"].astype(np.int64)
    dev = out.device

    def gather(starts, lens):
        """bytes [starts[i], starts[i] + lens[i]) of `out`, one copy to the host -> the pieces"""
        lens = np.asarray(lens, np.int64)
        ends = np.cumsum(lens)
        if not int(ends[-1]):
            return [b""] * len(lens)
        base = torch.from_numpy(np.asarray(starts, np.int64) - (ends - lens)).to(dev)
        at = torch.repeat_interleave(base, torch.from_numpy(lens).to(dev)) + torch.arange(int(ends[-1]), dtype=torch.int64, device=dev)
        raw = out[at].cpu().numpy().tobytes()
        return [raw[int(e - l):int(e)] for e, l in zip(ends, lens)]

    heads = gather([off[k] for k in picks], [min(_HEAD, usize[k]) for k in picks])
    spans = [header_span(h) for h in heads]
    for k, (at, n) in zip(picks, spans):
        if at + n > usize[k]:
            raise Error("load_npz: entry %r is shorter than its header" % index.names[k])
    texts = gather([off[k] + at for k, (at, _) in zip(picks, spans)], [n for _, n in spans])
    arrays = {}
    for k, h, (at, n), text in zip(picks, heads, spans, texts):
        descr, fortran, shape = parse_header(h, text)
        dtype, dt = _torch_dtype(descr)
        if fortran and len(shape) > 1:
            raise Error("load_npz: entry %r is in Fortran order" % index.names[k])
        nbytes = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
        lo = int(off[k]) + at + n
        if lo + nbytes > off[k] + usize[k]:
            raise Error("load_npz: entry %r holds fewer bytes than its shape" % index.names[k])
        piece = out[lo:lo + nbytes]
        if (piece.data_ptr() if nbytes else 0) % dt.itemsize:
            piece = piece.clone()                     # (a writer that does not align the data: a device copy, still no host byte)
        arrays[index.names[k][:-4]] = piece.view(dtype).reshape(shape)
    return arrays


def _npy_descr(dtype):
    """a torch dtype -> its .npy descr: the reverse of _torch_dtype's table; raises for a dtype that is not in it (bfloat16 is one)"""
    import torch
    table = {torch.bool: "|b1", torch.uint8: "|u1", torch.int8: "|i1", torch.int16: "<i2", torch.int32: "<i4", torch.int64: "<i8",
             torch.float16: "<f2", torch.float32: "<f4", torch.float64: "<f8", torch.complex64: "<c8", torch.complex128: "<c16"}
    if dtype not in table:
        raise Error("save_npz: dtype %r has no .npy counterpart" % (dtype,))
    return table[dtype]


def save_npz(engine, arrays, compressed=True, **kw):
    """{name: device tensor} -> a flat uint8 device tensor, the .npz file numpy.load and load_npz read (numpy.savez_compressed; with
    compressed=False every entry is stored, as numpy.savez does).  Per tensor a .npy version 1.0 header is made on the host by numpy's
    own writer -- a few bytes; all headers are staged in one copy --, the entry is that header and the tensor's bytes in C order, its
    name `name + ".npy"`; the file is written by Engine.compress_zip, whose keywords (block, cwindow, maxmatch, date_time, zip64) pass
    through: past 65535 arrays or 4 GiB the file is ZIP64, as numpy's own is.  No array byte crosses to the host."""
    import io
    import torch
    names, tensors, heads = [], [], []
    for name, t in arrays.items():
        if not (torch.is_tensor(t) and t.is_cuda and t.device == engine.device):
            raise Error("save_npz: %r is not a tensor on %s" % (name, engine.device))
        h = io.BytesIO()
        np.lib.format.write_array_header_1_0(h, {"descr": _npy_descr(t.dtype), "fortran_order": False, "shape": tuple(t.shape)})
        names.append(name + ".npy")
        heads.append(h.getvalue())
        flat = t.reshape(-1).contiguous()
        tensors.append((torch.view_as_real(flat).reshape(-1) if flat.is_complex() else flat).view(torch.uint8))
    staged = engine._stage(b"".join(heads))
    pieces, lens, at = [], [], 0
    for h, t in zip(heads, tensors):
        pieces += [staged[at:at + len(h)], t]
        lens.append(len(h) + t.numel())
        at += len(h)
    d_in = torch.cat(pieces) if pieces else torch.empty(0, dtype=torch.uint8, device=engine.device)
    out, _ = engine.compress_zip(d_in, lens, names, store=None if compressed else [True] * len(names), **kw)
    return out
