"""Guard-band arena (a helper module like port_harness.py, not a conftest): every buffer of a C-ABI call is carved out of ONE flat
uint8 tensor that is filled with a position-dependent pattern, with a guard band on each side, so that after the call every byte the
call had no business writing can be compared with the pattern -- on the device, the scratch of a large stream is hundreds of MiB.

A byte counts as NOT WRITTEN only if it still equals the pattern in two runs, one on the pattern P (salt s) and one on its complement
~P (salt s ^ 0xFF): no stored value equals P[i] and ~P[i] at once, so a kernel that happens to store the fill value is seen in the
other run.  The same pair of runs differs in every byte the call was not given (input slack, scratch, unused output), so results that
are identical in both do not depend on those bytes.

    a = Arena(Arena.size_for(specs), device, salt); views = {s[0]: a.carve(*s) for s in specs}
    a.fill("in", data) ... call the library on the views' data_ptr() ...
    clean = a.untouched_flat()                       # & the other run's
    bad = violations(a, clean, {"out": row_mask(...), "out_len": True, ...})     # [] when the call stayed inside

tests/test_guards_cpu.py plants writes on a CPU arena to show that the checker reports what it must."""
import torch

_CHUNK = 1 << 24


def pattern(lo, hi, salt, device):
    """the fill value of the arena's bytes [lo, hi): depends on the position's low, middle and high bits, so neither zeros, nor a
    constant, nor a copy of the arena shifted by a few bytes, by 256 or by 64 KiB reproduces it"""
    out = torch.empty(hi - lo, dtype=torch.uint8, device=device)
    for a in range(lo, hi, _CHUNK):
        b = min(hi, a + _CHUNK)
        i = torch.arange(a, b, dtype=torch.int64, device=device)
        v = (i * 197 + (i >> 8) * 59 + (i >> 16) * 31 + 91) ^ salt
        out[a - lo:b - lo] = (v & 0xFF).to(torch.uint8)
    return out


class Region(object):
    def __init__(self, name, off, nbytes, band, readonly):
        self.name, self.off, self.nbytes, self.band, self.readonly = name, off, nbytes, band, readonly


class Arena(object):
    def __init__(self, nbytes, device, salt):
        self.nbytes, self.device, self.salt = int(nbytes), torch.device(device), salt & 0xFF
        self.pat = pattern(0, self.nbytes, self.salt, self.device)
        # the arena starts at a 4 KiB boundary, so that two arenas carved alike have the same layout (the pair of runs compares them)
        self._raw = torch.empty(self.nbytes + 4096, dtype=torch.uint8, device=self.device)
        skip = -self._raw.data_ptr() % 4096
        self.buf = self._raw[skip:skip + self.nbytes]
        self.buf.copy_(self.pat)
        self.base = self.buf.data_ptr()
        self.cursor = 0
        self.regions = {}
        self.order = []

    @staticmethod
    def size_for(specs):
        """bytes that hold carve(*s) for every s of specs whatever the base address: (name, nbytes, align, band, ...)"""
        return sum(int(s[1]) + 2 * int(s[3]) + 2 * int(s[2]) for s in specs) + 512

    def carve(self, name, nbytes, align, band, readonly=False, phase=0):
        """-> a uint8 view of exactly nbytes whose address is `phase` modulo `align`, with `band` guard bytes on each side that no other
        region or band shares"""
        assert name not in self.regions and align >= 1 and 0 <= phase < align and nbytes >= 0 and band >= 0
        addr = self.base + self.cursor + band
        addr += (phase - addr) % align
        off = addr - self.base
        if off + nbytes + band > self.nbytes:
            raise ValueError("arena of %d bytes cannot hold %r (%d bytes + 2 bands of %d at offset %d)" %
                             (self.nbytes, name, nbytes, band, off))
        self.cursor = off + nbytes + band
        self.regions[name] = Region(name, off, int(nbytes), int(band), readonly)
        self.order.append(name)
        return self.buf[off:off + nbytes]

    def fill(self, name, data, at=0):
        """put a case's data into an (input) region, from its byte `at` on: it becomes what untouched() expects there"""
        r = self.regions[name]
        if len(data) == 0:
            return
        t = torch.as_tensor(data, dtype=torch.uint8).reshape(-1).to(self.device) if not isinstance(data, (bytes, bytearray)) \
            else torch.frombuffer(bytearray(data), dtype=torch.uint8).to(self.device)
        assert 0 <= at and at + t.numel() <= r.nbytes
        self.buf[r.off + at:r.off + at + t.numel()] = t
        self.pat[r.off + at:r.off + at + t.numel()] = t

    def view(self, name):
        r = self.regions[name]
        return self.buf[r.off:r.off + r.nbytes]

    def ptr(self, name):
        """the region's address, also for an empty one (its place between the bands)"""
        return self.base + self.regions[name].off

    def expected(self, name):
        r = self.regions[name]
        return self.pat[r.off:r.off + r.nbytes]

    def untouched_flat(self):
        """bool[nbytes]: the byte still equals the pattern"""
        return self.buf == self.pat

    def split(self, flat):
        """per region: (band in front, the region, band behind) as views of a flat per-byte tensor"""
        return {n: (flat[r.off - r.band:r.off], flat[r.off:r.off + r.nbytes], flat[r.off + r.nbytes:r.off + r.nbytes + r.band])
                for n, r in self.regions.items()}

    def untouched(self):
        return self.split(self.untouched_flat())


def row_mask(nrows, pitch, extents, device):
    """bool[nrows * pitch]: byte k of row b is allowed iff k < extents[b]"""
    ext = torch.as_tensor(extents, dtype=torch.int64, device=device).reshape(nrows, 1)
    return (torch.arange(pitch, dtype=torch.int64, device=device).reshape(1, pitch) < ext).reshape(-1)


def row_tails(unwritten_body, nrows, pitch):
    """int64[nrows]: index of the row's last written byte + 1 (0: the row was not written at all)"""
    w = ~unwritten_body[:nrows * pitch].reshape(nrows, pitch)
    idx = torch.arange(1, pitch + 1, dtype=torch.int64, device=w.device).reshape(1, pitch)
    return (w * idx).max(dim=1).values if pitch else torch.zeros(nrows, dtype=torch.int64, device=w.device)


def violations(arena, unwritten_flat, allowed):
    """-> list of (region, where, first offset, last offset, count) for every written byte outside what `allowed` grants.
    allowed: {region name: True (the whole region) | a byte count (that prefix) | bool tensor over the region (True = may be written)};
    regions that are missing from it, read-only regions and everything between the regions (the bands) may not be written at all.
    Offsets are relative to the region's first byte (negative in the band in front); `where` is "front band", "region" or "back band"."""
    may = torch.zeros(arena.nbytes, dtype=torch.bool, device=arena.device)
    for name, grant in allowed.items():
        r = arena.regions[name]
        assert not r.readonly, "%s is read-only: nothing in it may be allowed" % name
        if grant is True:
            may[r.off:r.off + r.nbytes] = True
        elif isinstance(grant, int):
            assert 0 <= grant <= r.nbytes
            may[r.off:r.off + grant] = True
        else:
            assert grant.dtype == torch.bool and grant.numel() == r.nbytes, name
            may[r.off:r.off + r.nbytes] = grant.to(arena.device)
    bad = ~unwritten_flat & ~may
    if not bool(bad.any()):
        return []
    found = []
    covered = torch.zeros_like(bad)
    for name in arena.order:
        r = arena.regions[name]
        for where, lo, hi in (("front band", r.off - r.band, r.off), ("region", r.off, r.off + r.nbytes),
                              ("back band", r.off + r.nbytes, r.off + r.nbytes + r.band)):
            covered[lo:hi] = True
            idx = torch.nonzero(bad[lo:hi]).reshape(-1)
            if idx.numel():
                found.append((name, where, int(idx[0]) + lo - r.off, int(idx[-1]) + lo - r.off, int(idx.numel())))
    idx = torch.nonzero(bad & ~covered).reshape(-1)          # alignment gaps between two regions' bands
    if idx.numel():
        found.append(("(arena)", "gap", int(idx[0]), int(idx[-1]), int(idx.numel())))
    return found
