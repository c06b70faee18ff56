"""CPU: the rule and the pixels of include/hdlz_tiff.h as tests/tiff_ref.py states them -- the reference every device result is held
against -- held against other readers and writers: files of the reference's writer read by Pillow / libtiff (where it is installed),
files written by libtiff itself (tests/golden/tiff, with their pixels beside them), and the rule's refusals on crafted files.

Pillow agrees with the format's text only for some sample types: uint8 with 1, 3 or 4 samples and uint16 grey in both byte orders,
strips and tiles, predictor 1 and 2; little-endian int16 / int32 / float32 grey; little-endian float32 with predictor 3.  It returns
wrong or narrowed data for 16-bit RGB(A), int8, uint32 and the big-endian 32-bit types.  Those, 64-bit samples, 2 and 8 samples and
big-endian predictor 3 rest on the serial rule and on the text of TIFF 6.0 and Adobe's Technical Note 3 alone: they are held to the
writer's own pixels (the writer and the reader are two texts), not to Pillow."""
import io
import os

import numpy as np
import pytest

import tiff_ref as T
from conftest import GOLD

GOLDEN = ("rgb_adobe", "rgb_adobe_pred2", "rgb_deflate", "grey16_adobe", "grey16_deflate_pred2", "rgb_adobe_pred2_strips")

# (format, bits, samples, big-endian, predictor): what Pillow reads as the text has it
PILLOW = [(1, 8, s, be, p) for s in (1, 3, 4) for be in (False, True) for p in (1, 2)] + \
         [(1, 16, 1, be, p) for be in (False, True) for p in (1, 2)] + \
         [(2, 16, 1, False, 1), (2, 32, 1, False, 1), (3, 32, 1, False, 1), (3, 32, 1, False, 3)]
LAYOUTS = [dict(rps=5), dict(tile=(16, 16))]


def _file(fmt, bits, samples, be, pred, layout, comp=8, w=37, h=45, seed=0, **kw):
    pix = T.random_pixels(h, w, samples, fmt, bits, seed + 1000 * bits + 10 * samples + fmt)
    return pix, T.make_tiff([dict(pix=pix, predictor=pred, compression=comp, **layout, **kw)], big=be)


@pytest.mark.parametrize("fmt,bits,samples,be,pred", PILLOW)
def test_tiff_ref_reads_images_as_pillow_does(fmt, bits, samples, be, pred):
    Image = pytest.importorskip("PIL.Image")
    import struct
    # (Pillow takes four samples as RGBA only with an ExtraSamples tag, 338, which the rule skips unread)
    kw = dict(photometric=2, extra=[(338, T.SHORT, 1, struct.pack(">H" if be else "<H", 2))]) if samples == 4 else {}
    for layout in LAYOUTS:
        pix, f = _file(fmt, bits, samples, be, pred, layout, **kw)
        ix, sts, outs = T.read([f])
        rec = ix["images"][0]
        assert sts == [T.OK], (layout, sts)
        got = T.array_of(rec, outs[0])
        assert got.tobytes() == pix.tobytes() and got.shape == pix.shape
        im = Image.open(io.BytesIO(f))
        im.load()
        want = np.asarray(im)
        assert want.shape == got.shape and want.astype(got.dtype).tobytes() == got.tobytes(), (layout, im.mode)


@pytest.mark.parametrize("be", [False, True])
@pytest.mark.parametrize("fmt,bits", [(1, 8), (2, 8), (1, 16), (2, 16), (1, 32), (2, 32), (3, 32), (1, 64), (2, 64), (3, 64)])
def test_the_writer_and_the_reader_agree_on_every_type(fmt, bits, be):
    """the types Pillow narrows or misreads among them: the writer's pixels come back through the reader's rule, byte for byte, for every
    predictor, compression, layout and sample count -- two texts of the same format (predict / unpredict), neither derived from the other"""
    k = 0
    for samples in (1, 2, 3, 4, 8):
        for pred in (1, 2, 3) if fmt == 3 else (1, 2):
            for comp in (1, 8, 32946):
                k += 1
                layout = (dict(rps=7), dict(tile=(16, 32)), dict(), dict(tile=(32, 16), arrays=T.SHORT))[k % 4]
                pix, f = _file(fmt, bits, samples, be, pred, layout, comp=comp, w=21, h=19, seed=k, pad=k % 3, unsorted=k if k % 2 else None)
                ix, sts, outs = T.read([f])
                rec = ix["images"][0]
                assert sts == [T.OK], (samples, pred, comp, layout, sts)
                assert (rec["format"], rec["bits"], rec["samples"], rec["predictor"], rec["compression"], rec["big_endian"]) == (fmt, bits, samples, pred, comp, int(be))
                assert outs[0] == pix.tobytes(), (samples, pred, comp, layout)


@pytest.mark.parametrize("name", GOLDEN)
def test_the_golden_libtiff_files_read_to_their_pixels(name):
    f = open(os.path.join(GOLD, "tiff", name + ".tif"), "rb").read()
    want = np.load(os.path.join(GOLD, "tiff", name + ".npy"))
    ix, sts, outs = T.read([f])
    got = T.array_of(ix["images"][0], outs[0])
    assert sts == [T.OK] and got.shape == want.shape and got.dtype == want.dtype and (got == want).all()
    assert ix["images"][0]["predictor"] == (2 if "pred2" in name else 1)


def test_the_golden_files_are_what_pillow_writes_today():
    """where Pillow is installed: it reads the committed files to the committed pixels (the files are libtiff's, not this project's)"""
    Image = pytest.importorskip("PIL.Image")
    for name in GOLDEN:
        im = Image.open(os.path.join(GOLD, "tiff", name + ".tif"))
        assert (np.asarray(im) == np.load(os.path.join(GOLD, "tiff", name + ".npy"))).all(), name


def test_several_pages_and_the_capacity_call():
    a, b, c = (T.random_pixels(9 + k, 7 + k, 1 + k, 1, 8 << k, k) for k in range(3))
    f = T.make_tiff([dict(pix=a), dict(pix=b, tile=(16, 16), predictor=2), dict(pix=c, compression=1)])
    ix, sts, outs = T.read([f, f, f, f], pages=[0, 1, 2, 3])
    assert sts == [T.OK, T.OK, T.OK, T.E_NO_EOF] and [outs[k] for k in range(3)] == [a.tobytes(), b.tobytes(), c.tobytes()]
    im = ix["images"]
    assert im[0]["next_ifd"] == im[1]["ifd_off"] and im[1]["next_ifd"] == im[2]["ifd_off"] and im[2]["next_ifd"] == 0
    assert im[3]["out_off"] == im[2]["out_off"] + 64 * -(-im[2]["out_len"] // 64) and im[3]["out_len"] == 0
    assert ix["total_chunks"] == 3 and ix["total_out"] == im[3]["out_off"]        # the end of the last slot: an empty one
    for cap in (0, 2):
        part = T.index([f, f, f, f], pages=[0, 1, 2, 3], image_cap=cap)
        assert part["status"] == T.E_OUT_CAPACITY and len(part["images"]) == cap and part["total_out"] == ix["total_out"]
    assert T.index([f], pages=[65536])["images"][0]["status"] == T.E_BAD_PARAM


def crafted():
    """[(label, file, the status THE RULE gives it)]: one file per refusal line, and the accepted oddities"""
    import struct
    pix = T.random_pixels(20, 24, 3, 1, 8, 5)
    good = T.make_tiff([dict(pix=pix, rps=6)])
    S, L = T.SHORT, T.LONG
    sh = lambda *v: struct.pack("<%dH" % len(v), *v)
    lo = lambda *v: struct.pack("<%dI" % len(v), *v)
    mk = lambda **kw: T.make_tiff([dict(dict(pix=pix, rps=6), **kw)])
    tiles = dict(tile=(16, 16))
    cases = [("sound", good, T.OK), ("bad magic", b"IJ" + good[2:], T.E_BAD_HEADER), ("mixed magic", b"II\0*" + good[4:], T.E_BAD_HEADER),
             ("BigTIFF", b"II+\0" + good[4:], T.E_BAD_BTYPE), ("BigTIFF, big-endian", b"MM\0+" + good[4:], T.E_BAD_BTYPE),
             ("three bytes", good[:3], T.E_BAD_HEADER), ("no room for the first offset", good[:6], T.E_BAD_HEADER),
             ("the directory leaves the file", good[:-3], T.E_NO_EOF), ("an odd directory offset", good[:4] + lo(9) + good[8:], T.E_BAD_HEADER),
             ("a directory offset inside the header", good[:4] + lo(4) + good[8:], T.E_BAD_HEADER),
             ("a directory offset behind the file", good[:4] + lo(len(good) + 10) + good[8:], T.E_NO_EOF),
             ("no directory at all", good[:4] + lo(0) + good[8:], T.E_NO_EOF),
             ("an array that leaves the file", mk(override={273: (L, 4, lo(1 << 20))}), T.E_NO_EOF),
             ("both layouts", mk(extra=[(322, S, 1, sh(16))]), T.E_BAD_HEADER),
             ("strip tags beside tiles", mk(extra=[(273, L, 1, lo(8))], **tiles), T.E_BAD_HEADER),
             ("neither layout", mk(override={273: None, 279: None}), T.E_BAD_HEADER),
             ("no byte counts", mk(override={279: None}), T.E_BAD_HEADER),
             ("tiles without their height", mk(override={323: None}, **tiles), T.E_BAD_HEADER),
             ("wrong array count", mk(override={279: (L, 3, lo(1, 2, 3))}), T.E_BAD_HEADER),
             ("LZW", mk(override={259: (S, 1, sh(5))}), T.E_BAD_BTYPE), ("JPEG", mk(override={259: (S, 1, sh(7))}), T.E_BAD_BTYPE),
             ("PackBits", mk(override={259: (S, 1, sh(32773))}), T.E_BAD_BTYPE), ("an unknown compression", mk(override={259: (S, 1, sh(999))}), T.E_BAD_HEADER),
             ("planar 2", mk(override={284: (S, 1, sh(2))}), T.E_BAD_BTYPE), ("planar 3", mk(override={284: (S, 1, sh(3))}), T.E_BAD_HEADER),
             ("bits 4", mk(override={258: (S, 3, sh(4, 4, 4))}), T.E_BAD_BTYPE), ("bits 0", mk(override={258: (S, 3, sh(0, 0, 0))}), T.E_BAD_HEADER),
             ("unequal bits", mk(override={258: (S, 3, sh(8, 8, 16))}), T.E_BAD_BTYPE), ("two bit widths for three samples", mk(override={258: (S, 2, sh(8, 8))}), T.E_BAD_HEADER),
             ("no BitsPerSample: 1 bit", mk(override={258: None}), T.E_BAD_BTYPE),
             ("predictor 3 on integers", mk(override={317: (S, 1, sh(3))}), T.E_BAD_BTYPE), ("predictor 4", mk(override={317: (S, 1, sh(4))}), T.E_BAD_HEADER),
             ("YCbCr", mk(photometric=6), T.E_BAD_BTYPE), ("a palette, as indices", T.make_tiff([dict(pix=pix[:, :, 0], photometric=3)]), T.OK),
             ("no photometric", mk(override={262: None}), T.OK), ("nine samples", mk(override={277: (S, 1, sh(9))}), T.E_BAD_BTYPE),
             ("complex samples", mk(override={339: (S, 3, sh(5, 5, 5))}), T.E_BAD_BTYPE), ("half floats", T.make_tiff([dict(pix=pix[:, :, 0].astype(np.uint16), override={339: (S, 1, sh(3))})]), T.E_BAD_BTYPE),
             ("width 0", mk(override={256: (L, 1, lo(0))}), T.E_BAD_HEADER), ("no width", mk(override={256: None}), T.E_BAD_HEADER),
             ("rows per strip 0", mk(override={278: (L, 1, lo(0))}), T.E_BAD_HEADER),
             ("a RATIONAL where a LONG belongs", mk(override={257: (5, 1, lo(20))}), T.E_BAD_HEADER),
             ("two widths", mk(override={256: (L, 2, lo(24, 24))}), T.E_BAD_HEADER),
             ("an image past the limits", mk(override={256: (L, 1, lo((1 << 31) - 1)), 257: (L, 1, lo((1 << 31) - 1))}), T.E_OUT_CAPACITY),
             ("SHORT arrays", mk(arrays=S), T.OK), ("SHORT offsets against LONG counts", mk(arrays=S, rps=20, override={279: (L, 1, lo(0))}), T.OK),
             ("a duplicate tag: the first wins", mk(extra=[(259, S, 1, sh(5)), (256, L, 1, lo(999))]), T.OK),
             ("a duplicate tag in front: the first wins", mk(extra=[(259, S, 1, sh(5))], extra_first=True), T.E_BAD_BTYPE),
             ("unsorted tags", mk(unsorted=3), T.OK), ("unsorted tags, tiles, big-endian", T.make_tiff([dict(pix=pix, unsorted=4, **tiles)], big=True), T.OK),
             ("unknown tags of every type", mk(extra=[(270, 2, 9, b"a string"), (33550, 12, 3, b"\0" * 24), (34735, S, 4, sh(1, 1, 0, 0)), (700, 7, 2, b"ab")]), T.OK),
             ("no RowsPerStrip: one strip", T.make_tiff([dict(pix=pix, rps_tag=False)]), T.OK),
             ("RowsPerStrip past the height", mk(rps=20, override={278: (L, 1, lo(0xFFFFFFFF))}), T.OK)]
    return cases


def test_the_rule_on_crafted_files():
    for label, f, want in crafted():
        rec = T.index([f])["images"][0]
        assert rec["status"] == want, (label, rec["status"], want)
        if want != T.OK:
            assert all(rec[k] == 0 for k in T.FIELDS if k not in ("file_off", "file_len", "status", "chunk_off", "raw_off", "out_off")), label


def test_pillow_reads_the_accepted_oddities():
    """unsorted tags are outside the format's letter (libtiff warns and reads on); the others are within it"""
    Image = pytest.importorskip("PIL.Image")
    for label, f, want in crafted():
        if want == T.OK and label in ("sound", "SHORT arrays", "unknown tags of every type", "no RowsPerStrip: one strip", "RowsPerStrip past the height"):
            _, sts, outs = T.read([f])
            im = Image.open(io.BytesIO(f))
            assert sts == [T.OK] and np.asarray(im).tobytes() == outs[0], label


def test_the_verdicts_of_damaged_chunks():
    pix = T.random_pixels(12, 10, 1, 1, 8, 9)
    flip = lambda at, bit=1: (lambda k, d: d if k != 1 else d[:at % len(d)] + bytes([d[at % len(d)] ^ bit]) + d[at % len(d) + 1:])
    mk = lambda **kw: T.make_tiff([dict(dict(pix=pix, rps=4, level=0), **kw)])       # (level 0: stored blocks -- a payload bit reaches only the Adler-32)
    for label, f, want in (("sound", mk(), T.OK), ("padded", mk(pad=5), T.OK), ("a payload bit", mk(damage=flip(12)), T.E_BAD_CHECKSUM),
                           ("an Adler byte", mk(damage=flip(-1)), T.E_BAD_CHECKSUM), ("a bad zlib header", mk(damage=flip(1, 0x20)), T.E_BAD_HEADER),
                           ("a chunk that decodes long", mk(damage=lambda k, d: d if k != 1 else __import__("zlib").compress(bytes(41), 0)), T.E_OUT_CAPACITY),
                           ("a chunk that decodes short", mk(damage=lambda k, d: d if k != 1 else __import__("zlib").compress(bytes(39), 0)), T.E_BAD_CHECKSUM),
                           ("a truncated stored chunk", mk(compression=1, override={279: (T.LONG, 3, __import__("struct").pack("<3I", 40, 39, 40))}), T.E_NO_EOF),
                           ("five bytes", mk(damage=lambda k, d: d if k != 1 else d[:5]), T.E_NO_EOF)):
        _, sts, outs = T.read([f])
        assert sts == [want], (label, sts, want)
        assert (outs[0] == pix.tobytes()) if want == T.OK else outs[0] is None
