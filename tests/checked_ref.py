"""What hdlz_inflate_checked must answer, from stock zlib and the CPU oracle (a helper module like guards.py, not a conftest).

The reference for the verdict is stock zlib -- zlib.decompressobj(): .eof, .unused_data, the error text; zlib.adler32 -- and, for the
decoder's own statuses, the oracle (which is bit-exact with the device's unchecked decode).  Never the library's own unchecked call."""
import random
import zlib

import numpy as np

OK, E_NO_EOF, E_BAD_HEADER, E_BAD_CHECKSUM = 0, 5, 11, 12


def zjudge(z):
    """-> ("ok", (bytes, consumed)) | ("chk" | "hdr" | "dec", zlib's message); anything but a clean end counts as an error"""
    d = zlib.decompressobj()
    try:
        out = d.decompress(z)
    except zlib.error as e:
        msg = str(e)
        if "incorrect data check" in msg:
            return "chk", msg
        if "incorrect header check" in msg or "invalid window size" in msg or "unknown compression method" in msg:
            return "hdr", msg
        return "dec", msg
    if not d.eof:
        return "dec", "incomplete"
    return "ok", (out, len(z) - len(d.unused_data))


def expect(oracle, z, cap, payload=None):
    """the rules of the damage sweep for one stream -> dict(status = a code, or None for "any status but OK"; out_len; and, where the
    rules state them, in_used / adler / data)"""
    rc, ref = oracle.inflate(z, out_cap=cap)
    if rc != OK:
        return dict(status=rc, out_len=0, in_used=0, adler=0)
    kind, info = zjudge(z)
    if kind == "ok":
        assert info[0] == ref
        return dict(status=OK, out_len=len(ref), in_used=info[1], adler=zlib.adler32(ref), data=ref)
    if kind == "chk":
        return dict(status=E_BAD_CHECKSUM, out_len=0, adler=zlib.adler32(ref))
    if kind == "hdr":
        return dict(status=E_BAD_HEADER, out_len=0, adler=zlib.adler32(ref))
    # the reference decodes more leniently than zlib.  The one stated exception: a flipped NLEN changes nothing
    if "invalid stored block lengths" in info and payload is not None and ref == payload:
        return dict(status=OK, out_len=len(ref), adler=zlib.adler32(ref), data=ref)
    return dict(status=None, out_len=0)


def check(label, exp, st, ol, used, ad, row):
    st, ol, used, ad = int(st), int(ol), int(used), int(ad) & 0xFFFFFFFF
    if exp["status"] is None:
        assert st != OK, (label, "must not be OK")
    else:
        assert st == exp["status"], (label, st, exp["status"])
    assert ol == exp["out_len"], (label, ol, exp["out_len"])
    if st != OK and st not in (E_BAD_HEADER, E_BAD_CHECKSUM):
        assert used == 0 and ad == 0, (label, st, used, ad)
    if "in_used" in exp:
        assert used == exp["in_used"], (label, used, exp["in_used"])
    if "adler" in exp and st in (OK, E_BAD_HEADER, E_BAD_CHECKSUM):
        assert ad == exp["adler"], (label, hex(ad), hex(exp["adler"]))
    if "data" in exp:
        assert bytes(row[:ol]) == exp["data"], (label, "bytes")


def run_ragged(engine, zs, pitch, flags=0, in_len=None, out=None):
    """the streams back to back as one ragged checked call -> (rows, out_len, status, in_used, adler) as numpy (adler as uint32)"""
    import torch
    flat = torch.from_numpy(np.frombuffer(b"".join(zs) + bytes(64), np.uint8).copy()).cuda()
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum([len(z) for z in zs])]).astype(np.int64)).cuda()
    o, ol, st, used, ad = engine.inflate_checked(flat, in_off=offs, in_len=in_len, out_pitch=pitch, flags=flags, out=out)
    torch.cuda.synchronize()
    return o.cpu().numpy(), ol.cpu().numpy(), st.cpu().numpy(), used.cpu().numpy(), ad.cpu().numpy().view(np.uint32)


def check_all(label, oracle, engine, zs, pitch, flags=0, in_len=None, payloads=None, exps=None):
    rows, ol, st, used, ad = run_ragged(engine, zs, pitch, flags, in_len)
    exps = exps or [expect(oracle, z, pitch, payloads[k] if payloads else None) for k, z in enumerate(zs)]
    for k in range(len(zs)):
        check((label, k), exps[k], st[k], ol[k], used[k], ad[k], rows[k])
    return rows, ol, st, used, ad


SWEEP_COUNTS = [(("chk", True), 4563), (("dec", False), 788), (("dec", True), 2), (("hdr", True), 11), (("ok", True), 36)]


def sweep(O):
    """the damage sweep's recipe: 27 streams of a 2 KiB payload, 200 single-bit flips each.  The generator is lazy and shares `r` with
    the flips: the order of the calls is part of the recipe.  -> (intact [(stream, payload)], damaged [(stream, payload)])"""
    r = random.Random(20261016)

    def data(kind, n):
        if kind == 'text':
            return bytes(r.choice(b'abcdefgh \n') for _ in range(n))
        if kind == 'rand':
            return bytes(r.getrandbits(8) for _ in range(n))
        if kind == 'runs':
            return b''.join(bytes([r.getrandbits(8)]) * r.randint(1, 40) for _ in range(n // 20))

    def streams():
        for kind in ('text', 'rand', 'runs'):
            d = data(kind, 2048)
            yield O.compress(d, 32, 10)[1], d
            yield O.compress(d, 256, 10)[1], d
            for lvl, strat in ((6, 0), (1, 0), (9, 0), (6, zlib.Z_FIXED), (0, 0), (6, zlib.Z_HUFFMAN_ONLY), (6, zlib.Z_RLE)):
                c = zlib.compressobj(lvl, zlib.DEFLATED, 15, 8, strat)
                yield c.compress(d) + c.flush(), d
    intact, damaged = [], []
    for z, d in streams():
        intact.append((z, d))
        for t in range(200):
            b = r.randrange(len(z) * 8)
            m = bytearray(z)
            m[b >> 3] ^= 1 << (b & 7)      # one damaged stream
            damaged.append((bytes(m), d))
    return intact, damaged
